"""window_mutual_info on the device (K25) against ``window_mi_measures``, the NumPy restatement of
the definition (tests/test_mi_host.py).

``counts`` must be exactly equal: the edges are K17's quantiles (numpy.quantile's bits) or the
uniform formula's IEEE operations, the bins are comparisons and the counts are integer sums on the
int8 matrix pipe.  An exact ``counts`` also pins the row map of the matrix operands and the map of
the accumulators, the only two that can go wrong.  ``mi``, ``nmi`` and ``joint`` stay within RTOL =
1e-9 (the suite's cap), absolute on every entry; the derived bound is about 2e-12 -- at most B^2 +
2 B <= 288 terms of size <= W ln W, divided by W -- and the ratio to the cap is printed.

Shapes (C, W, step, B, binning, windows), the smallest at which the kernels can go wrong: the least
of everything; exactly one 64-sample matrix step with overlap and a tile that is one channel;
padded samples, gaps and B = 3 padded to 4, so that 20 rows cross a tile; one sample past a step
and 272 rows; an odd W past 1024; the longest window, where the copied row takes a cell to n = W;
66 channels of 8 bins, several 64-row blocks a side, for the triangular index; 130 channels of few
bins.  Data are ``mixed`` rows -- each mixes in the one before, one is quantised, one is an exact
copy, one the square of another plus noise -- at offsets of 0 and 100 sigma.

Everything else here is bit for bit."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer
from openseize_amd.features import _stream

from test_connectivity_host import RTOL
from test_mi_host import NAMES, SHAPES, restated, stream, window_mi_measures

pytestmark = pytest.mark.gpu

ONE, CROSS, TILE, BLOCKS, MANY = SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[6], SHAPES[7]
TILED = [CROSS, TILE, BLOCKS]                                 # the three shapes with tiles and blocks


@pytest.fixture(scope="module")
def wm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_mutual_info
    return window_mutual_info


@lru_cache(maxsize=None)
def device_all(shape, offset=0.0):
    """(nwin, every measure) from one array call, computed once."""
    from openseize_amd.features import window_mutual_info
    nch, W, step, B, binning, nwin = shape
    return window_mutual_info(stream(shape, offset), W, step, measures=NAMES, bins=B, binning=binning)


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_symmetric_with_fixed_points(M, W):
    for name in NAMES[1:]:
        assert same_bits(M[name], np.swapaxes(M[name], 1, 2)), name
    assert same_bits(M["counts"], M["counts"].transpose(0, 2, 1, 4, 3))

    def diag(a):
        return np.diagonal(a, axis1=-2, axis2=-1)
    H = diag(M["mi"])
    assert same_bits(diag(M["joint"]), H)
    one = diag(M["nmi"])
    dead = np.isnan(H) | (H == 0.0)
    assert np.all(one[~dead] == 1.0) and np.all(np.isnan(one[dead]))
    marg = diag(M["counts"])                                 # (nwin, B, B, C): n_a on a = b, 0 elsewhere
    B = marg.shape[1]
    off = ~np.eye(B, dtype=bool)
    ok = ~np.isnan(H)
    assert np.all(marg[:, off][np.broadcast_to(ok[:, None], marg[:, off].shape)] == 0.0)
    kept = np.einsum("kaac->kca", marg)                      # (nwin, C, B)
    assert np.all(kept[ok].sum(axis=-1) == W)


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_restatement(wm, shape, offset):
    nch, W, step, B, binning, nwin = shape
    want = restated(shape, offset)
    n, M = device_all(shape, offset)
    assert n == nwin and list(M) == list(NAMES)
    assert M["counts"].shape == (nwin, B, B, nch, nch) and M["counts"].dtype == np.float64
    wrong = int(np.sum(M["counts"] != want["counts"]))
    print(f"C={nch} W={W} step={step} B={B} {binning} +{offset}: {wrong} of {want['counts'].size} counts differ")
    assert np.all(np.isfinite(want["counts"])) and want["counts"].max() <= W
    assert np.array_equal(M["counts"], want["counts"]), (shape, offset, wrong)
    assert np.all(M["counts"].sum(axis=(1, 2)) == W)
    for name in NAMES[1:]:
        g = M[name]
        assert g.shape == want[name].shape == (nwin, nch, nch) and g.dtype == np.float64, (name, g.shape)
        assert np.array_equal(np.isnan(g), np.isnan(want[name])), name
        err = np.abs(g - want[name])[~np.isnan(g)]
        ratio = float(err.max() / RTOL)
        print(f"    {name}: {ratio:.2e} of the cap")
        assert np.all(err <= RTOL), (shape, offset, name, ratio)
    assert np.all(M["mi"][~np.isnan(M["mi"])] >= 0.0) and not np.any(np.signbit(M["mi"]))
    assert_symmetric_with_fixed_points(M, W)


def test_the_copied_row_reaches_a_full_cell_and_the_square_is_seen(wm):
    nch, W, step, B, binning, nwin = SHAPES[5]
    n, M = device_all(SHAPES[5], 0.0)
    c = M["counts"][:, :, :, 0, 3]                           # row 3 is row 0: the joint histogram is diagonal
    assert np.all(c[:, ~np.eye(B, dtype=bool)] == 0.0) and np.all(np.einsum("kaa->k", c) == W)
    H = np.diagonal(M["mi"], axis1=1, axis2=2)
    assert np.max(np.abs(M["mi"][:, 0, 3] - H[:, 0])) <= RTOL and np.all(np.abs(M["nmi"][:, 0, 3] - 1.0) <= RTOL)
    nch, W, step, B, binning, nwin = SHAPES[4]               # row 4 is row 1 squared plus noise
    x = stream(SHAPES[4], 0.0)
    n, M = device_all(SHAPES[4], 0.0)
    for k in range(nwin):
        w = x[:, k * step:k * step + W]
        corr = np.corrcoef(w[1], w[4])[0, 1]
        print(f"window {k}: corr {corr:+.3f}, MI(x, x^2 + e) = {M['mi'][k, 1, 4]:.3f}, MI of rows 1 and 8 = {M['mi'][k, 1, 8]:.3f}")
        assert M["mi"][k, 1, 4] > 0.3


@pytest.mark.parametrize("shape", TILED)
def test_chunking_host_or_device_axis_and_launches_change_no_bit(wm, shape, monkeypatch):
    import torch
    nch, W, step, B, binning, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    kw = dict(measures=NAMES, bins=B, binning=binning)
    for chunk in (97, W + 1):
        n2, G = wm(producer(np.array(x), chunk, -1), W, step, **kw)
        assert n2 == n
        for name in NAMES:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (chunk, name)
    t = torch.from_numpy(np.array(x)).cuda()
    n2, G = wm(t, W, step, **kw)
    assert n2 == n
    for name in NAMES:
        assert isinstance(G[name], torch.Tensor) and G[name].is_cuda and G[name].dtype == torch.float64
        assert same_bits(G[name], F[name]), name
    n2, G = wm(np.ascontiguousarray(x.T), W, step, axis=0, **kw)
    assert n2 == n
    for name in NAMES:
        assert G[name].shape == F[name].shape and same_bits(G[name], F[name]), name
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)           # every window is its own launch
    for data in (x, t):
        n2, G = wm(data, W, step, **kw)
        assert n2 == n and all(same_bits(G[name], F[name]) for name in NAMES)


@pytest.mark.parametrize("shape", TILED)
def test_a_single_name_is_its_entry_of_the_whole(wm, shape):
    nch, W, step, B, binning, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    for name in NAMES:
        n2, one = wm(x, W, step, measures=name, bins=B, binning=binning)
        assert n2 == n and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    back = tuple(reversed(NAMES))
    n2, G = wm(x, W, step, measures=back, bins=B, binning=binning)
    assert list(G) == list(back) and all(same_bits(G[name], F[name]) for name in NAMES)
    n2, G = wm(x, W, bins=B, binning=binning)                # the defaults: step = winsize, mi alone, a dict
    assert n2 == x.shape[1] // W and list(G) == ["mi"] and same_bits(G["mi"][0], F["mi"][0])


@pytest.mark.parametrize("shape,rows", [(BLOCKS, [7, 8]), (BLOCKS, [3, 65]), (TILE, [0, 16]), (CROSS, [1, 4]),
                                        (MANY, [31, 129])])
def test_an_entry_depends_on_its_own_two_channels_only(wm, shape, rows):
    nch, W, step, B, binning, nwin = shape
    n, F = device_all(shape, 100.0)
    n2, G = wm(stream(shape, 100.0)[rows], W, step, measures=NAMES, bins=B, binning=binning)
    assert n2 == n
    for name in NAMES:
        assert same_bits(G[name], F[name][..., rows, :][..., rows]), name


@pytest.mark.parametrize("shape", TILED)
def test_a_window_does_not_depend_on_step(wm, shape):
    nch, W, step, B, binning, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    n2, H = wm(x, W, 2 * step, measures=NAMES, bins=B, binning=binning)
    assert n2 == (nwin + 1) // 2
    for name in NAMES:
        assert same_bits(H[name], F[name][::2]), name
    n1, one = wm(x[:, step:step + W], W, measures=NAMES, bins=B, binning=binning)
    assert n1 == 1 and all(same_bits(one[name][0], F[name][1]) for name in NAMES)


def held(nwin, W, step, at):
    k = np.arange(nwin)
    return (k * step <= at) & (at < k * step + W)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("shape", TILED)
def test_a_non_finite_sample_stays_in_its_row_and_column(wm, shape, bad):
    nch, W, step, B, binning, nwin = shape
    n, F = device_all(shape, 100.0)
    y = np.array(stream(shape, 100.0))
    at = step + 5                                            # in window 1, and in window 0 where they overlap
    y[2, at] = bad
    n2, G = wm(y, W, step, measures=NAMES, bins=B, binning=binning)
    hit = held(nwin, W, step, at)
    assert n2 == n and 0 < hit.sum() < nwin
    lost = np.zeros((nwin, nch, nch), dtype=bool)
    lost[hit, 2, :] = lost[hit, :, 2] = True
    for name in NAMES:
        gone = np.broadcast_to(lost[:, None, None], G[name].shape) if name == "counts" else lost
        was = np.isnan(F[name])                              # (nmi of a pair with H = 0: none in these data)
        assert np.array_equal(np.isnan(G[name]), gone | was), name
        assert np.array_equal(bits(G[name])[~gone], bits(F[name])[~gone]), name


@pytest.mark.parametrize("shape", TILED)
def test_a_constant_channel(wm, shape):
    nch, W, step, B, binning, nwin = shape
    n, F = device_all(shape, 100.0)
    y = np.array(stream(shape, 100.0))
    y[1] = 7.5
    n2, G = wm(y, W, step, measures=NAMES, bins=B, binning=binning)
    row = np.zeros((nch, nch), dtype=bool)
    row[1, :] = row[:, 1] = True
    assert n2 == n and np.all(np.isnan(G["nmi"][:, row]))
    assert np.all(G["mi"][:, row] == 0.0) and not np.any(np.signbit(G["mi"][:, row]))
    H = np.diagonal(G["mi"], axis1=1, axis2=2)               # (nwin, C)
    assert np.all(H[:, 1] == 0.0)
    assert same_bits(G["joint"][:, 1, :], H) and same_bits(G["joint"][:, :, 1], H)
    assert np.all(G["counts"][:, B - 1, :, 1, :].sum(axis=1) == W)      # a constant window is all bin B - 1
    for name in NAMES:
        assert np.array_equal(bits(G[name])[..., ~row], bits(F[name])[..., ~row]), name
    want = window_mi_measures(y, W, step, B, binning)
    assert np.array_equal(G["counts"], want["counts"])


@pytest.mark.parametrize("shape", TILED)
def test_quantile_counts_do_not_move_under_a_monotone_map(wm, shape):
    nch, W, step, B, binning, nwin = shape
    x = np.array(stream(shape, 0.0))
    y = x.copy()
    y[0], y[1] = np.exp(x[0]), np.exp(0.5 * x[1])            # rows 0 and 1 are continuous
    want = window_mi_measures(x, W, step, B, "quantile")["counts"]
    assert np.array_equal(window_mi_measures(y, W, step, B, "quantile")["counts"], want)
    n, c = wm(x, W, step, measures="counts", bins=B, binning="quantile")
    n2, d = wm(y, W, step, measures="counts", bins=B, binning="quantile")
    assert n == n2 == nwin and np.array_equal(c, want) and same_bits(c, d)


def test_results_that_do_not_fit_the_device_are_refused(wm, monkeypatch):
    """CUDA-fed results stay on the device: when they cannot fit, MemoryError names the sizes before
    a kernel runs.  Host-fed results come down push by push and are not refused."""
    import torch
    from openseize_amd import _device as dev
    nch, W, step, B, binning, nwin = TILE
    x = stream(TILE, 100.0)
    t = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 1 << 40))
    launched = []
    plain = dev.window_mi
    monkeypatch.setattr(dev, "window_mi", lambda *a, **k: (launched.append(1), plain(*a, **k))[1])
    with pytest.raises(MemoryError, match=r"256 more for counts.*step \(now 65; winsize 65\).*bins \(now 16\).*17 channels"):
        wm(t, W, step, measures=("mi", "counts"), bins=B, binning=binning)
    assert not launched
    n, M = wm(x, W, step, measures="mi", bins=B, binning=binning)
    assert n == nwin and launched and same_bits(M, device_all(TILE, 100.0)[1]["mi"])
