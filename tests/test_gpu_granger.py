"""window_granger on the device (K24) against ``window_granger_measures``, the NumPy long-double
restatement of the definition by explicit normal equations and Gaussian elimination
(tests/test_granger_host.py).

Cap.  RTOL = 1e-9, the suite's cap, absolute on every entry of every measure: the measures are
logarithms of ratios, so an absolute error of a measure is a relative error of the ratio.

Shapes (C, W, step, p, windows), the smallest at which the kernels can go wrong: the least of
everything with p = W // 8; overlap and exactly one 64-sample staging step; C = 17 across the tiles
of pairs with an odd W and the largest order; W past 1024 with an odd order; the longest window;
gaps and C = 66 across the 32-row block of the Gram workgroup (and the 64 mark); C = 130, order 1,
five Gram blocks a side for the triangular index.  Data are seeded normal rows with ``x[1:] += 0.7
roll(x[:-1], 3)``, so the direction is real, at offsets of 0 and 100 sigma.

Everything else here is bit for bit."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer
from openseize_amd.features import _stream

from test_connectivity_host import RTOL
from test_granger_host import NAMES, SHAPES, restated, stream, window_granger_measures

pytestmark = pytest.mark.gpu

LEAST, TILE, LONG, BLOCKS, MANY = SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[5], SHAPES[6]


@pytest.fixture(scope="module")
def wg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_granger
    return window_granger


@lru_cache(maxsize=None)
def device_all(shape, offset=0.0):
    """(nwin, every measure) from one array call, computed once."""
    from openseize_amd.features import window_granger
    nch, W, step, p, nwin = shape
    return window_granger(stream(shape, offset), W, step, measures=NAMES, order=p)


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def diag(a):
    return np.diagonal(a, axis1=-2, axis2=-1)


def assert_symmetric_with_fixed_points(M):
    for name in ("instant", "total"):
        assert same_bits(M[name], np.swapaxes(M[name], 1, 2)), name
    assert same_bits(M["total"], (M["granger"] + np.swapaxes(M["granger"], 1, 2)) + M["instant"])
    for name in NAMES:
        d = diag(M[name])
        assert np.all((bits(d) == 0) | np.isnan(d)), name     # +0.0, or NaN where the channel is lost
        assert np.all(np.isnan(M[name]) | (M[name] >= 0)) and not np.any(np.signbit(M[name])), name


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_restatement(wg, shape, offset):
    nch, W, step, p, nwin = shape
    want = restated(shape, offset)
    n, M = device_all(shape, offset)
    assert n == nwin and list(M) == list(NAMES)
    for name in NAMES:
        g = M[name]
        assert g.shape == (nwin, nch, nch) and g.dtype == np.float64 and np.all(np.isfinite(g)), (name, g.shape)
        ratio = float(np.max(np.abs(g - want[name]))) / RTOL
        print(f"C={nch} W={W} step={step} p={p} +{offset} {name}: {ratio:.2e} of the cap")
        assert np.all(np.abs(g - want[name]) <= RTOL), (shape, offset, name, ratio)
    assert np.all(diag(M["granger"]) == 0.0)
    assert_symmetric_with_fixed_points(M)


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] >= 257 and s[3] >= 3])
def test_the_driver_is_told_from_the_driven(wg, shape, offset):
    nch = shape[0]
    i = np.arange(nch - 1)
    want = restated(shape, offset)["granger"]
    assert np.all(want[:, i, i + 1] > want[:, i + 1, i]), shape       # first on the restatement alone
    got = device_all(shape, offset)[1]["granger"]
    assert np.all(got[:, i, i + 1] > got[:, i + 1, i]), shape


@pytest.mark.parametrize("shape", [TILE, LONG, BLOCKS])
def test_chunking_host_or_device_axis_and_launches_change_no_bit(wg, shape, monkeypatch):
    import torch
    nch, W, step, p, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    for chunk in (97, W + 1):                                 # an odd size and one that splits every window
        n2, G = wg(producer(np.array(x), chunk, -1), W, step, measures=NAMES, order=p)
        assert n2 == n
        for name in NAMES:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (name, chunk)
    t = torch.from_numpy(np.array(x)).cuda()
    n2, G = wg(t, W, step, measures=NAMES, order=p)
    assert n2 == n
    for name in NAMES:
        assert isinstance(G[name], torch.Tensor) and G[name].is_cuda and G[name].dtype == torch.float64
        assert same_bits(G[name], F[name]), name
    n2, G = wg(np.ascontiguousarray(x.T), W, step, measures=NAMES, order=p, axis=0)
    assert n2 == n
    for name in NAMES:
        assert G[name].shape == F[name].shape and same_bits(G[name], F[name]), name
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)           # every window is its own launch
    for data in (x, t):
        n2, G = wg(data, W, step, measures=NAMES, order=p)
        assert n2 == n and all(same_bits(G[name], F[name]) for name in NAMES)


def test_a_single_name_is_its_entry_of_the_whole(wg):
    nch, W, step, p, nwin = TILE
    x = stream(TILE, 100.0)
    n, F = device_all(TILE, 100.0)
    for name in NAMES:
        n2, one = wg(x, W, step, measures=name, order=p)
        assert n2 == n and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    back = tuple(reversed(NAMES))
    n2, G = wg(x, W, step, measures=back, order=p)
    assert list(G) == list(back) and all(same_bits(G[name], F[name]) for name in NAMES)
    n2, G = wg(x, W)                                         # the defaults: step = winsize, ("granger",), order 8
    n8, F8 = wg(x, W, W, measures="granger", order=8)
    assert n2 == n8 == x.shape[1] // W and list(G) == ["granger"] and same_bits(G["granger"], F8)


@pytest.mark.parametrize("shape,rows", [(BLOCKS, [3, 31, 32, 65]), (MANY, [7, 8, 15, 16, 63, 64, 129]), (TILE, [0, 16])])
def test_an_entry_depends_on_its_own_two_channels_only(wg, shape, rows):
    nch, W, step, p, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    n2, G = wg(x[rows], W, step, measures=NAMES, order=p)
    assert n2 == n
    for name in NAMES:
        assert same_bits(G[name], F[name][..., rows, :][..., rows]), name


def test_a_window_does_not_depend_on_step(wg):
    nch, W, step, p, nwin = TILE
    x = stream(TILE, 100.0)
    n, F = device_all(TILE, 100.0)
    n2, H = wg(x, W, 2 * step, measures=NAMES, order=p)
    assert n2 == (nwin + 1) // 2
    for name in NAMES:
        assert same_bits(H[name], F[name][::2]), name
    n1, one = wg(x[:, step:step + W], W, measures=NAMES, order=p)
    assert n1 == 1 and all(same_bits(one[name][0], F[name][1]) for name in NAMES)


def held(nwin, W, step, at):
    k = np.arange(nwin)
    return (k * step <= at) & (at < k * step + W)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_sample_stays_in_its_row_and_column(wg, bad):
    nch, W, step, p, nwin = TILE
    n, F = device_all(TILE, 100.0)
    y = np.array(stream(TILE, 100.0))
    y[2, 130] = bad
    n2, G = wg(y, W, step, measures=NAMES, order=p)
    hit = held(nwin, W, step, 130)
    assert n2 == n and 0 < hit.sum() < nwin
    lost = np.zeros((nwin, nch, nch), dtype=bool)
    lost[hit, 2, :] = lost[hit, :, 2] = True
    for name in NAMES:
        assert np.array_equal(np.isnan(G[name]), lost), name
        assert np.array_equal(bits(G[name])[~lost], bits(F[name])[~lost]), name


def test_a_constant_channel(wg):
    nch, W, step, p, nwin = TILE
    n, F = device_all(TILE, 100.0)
    y = np.array(stream(TILE, 100.0))
    y[2] = 7.5
    n2, G = wg(y, W, step, measures=NAMES, order=p)
    row = np.zeros((nch, nch), dtype=bool)
    row[2, :] = row[:, 2] = True
    for name in NAMES:
        assert np.array_equal(np.isnan(G[name]), np.broadcast_to(row, G[name].shape)), name
        assert np.array_equal(bits(G[name])[..., ~row], bits(F[name])[..., ~row]), name


@pytest.mark.parametrize("shape", [LEAST, TILE])
def test_scale_and_offset_of_a_channel_move_nothing_past_the_cap(wg, shape):
    nch, W, step, p, nwin = shape
    n, F = device_all(shape, 0.0)
    y = np.array(stream(shape, 0.0))
    y[1] = 1e3 * y[1] + 1e6
    n2, G = wg(y, W, step, measures=NAMES, order=p)
    assert n2 == n
    for name in NAMES:
        moved = float(np.max(np.abs(G[name] - F[name])))
        print(f"C={nch} W={W} p={p} {name}: moved by {moved / RTOL:.2e} of the cap")
        assert moved <= RTOL, (shape, name, moved)
    want = window_granger_measures(y, W, step, p)
    assert all(np.max(np.abs(G[name] - want[name])) <= RTOL for name in NAMES)


def test_results_that_do_not_fit_the_device_are_refused(wg, monkeypatch):
    """CUDA-fed results stay on the device: when they cannot fit, MemoryError names the sizes before
    a kernel runs.  Host-fed results come down push by push and are not refused."""
    import torch
    from openseize_amd import _device as dev
    nch, W, step, p, nwin = TILE
    x = stream(TILE, 100.0)
    t = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 1 << 40))
    launched = []
    plain = dev.window_granger
    monkeypatch.setattr(dev, "window_granger", lambda *a, **k: (launched.append(1), plain(*a, **k))[1])
    with pytest.raises(MemoryError, match=r"step \(now 100; winsize 257\).*17 channels"):
        wg(t, W, step, order=p)
    assert not launched
    n, M = wg(x, W, step, measures="total", order=p)
    assert n == nwin and launched and same_bits(M, device_all(TILE, 100.0)[1]["total"])
