"""window_xcorr on the device (K23) against ``window_xcorr_measures``, the NumPy long-double
restatement of the definition (tests/test_xcorr_host.py).

Caps.  RTOL = 1e-9 (the suite's cap): absolute for ``normalize=True``, times sqrt(r_ii(0) r_jj(0))
for ``normalize=False``, on every entry of ``xcorr``, ``peak`` and ``signed``.  ``lag`` and the
sign of ``signed`` are compared exactly; for that the test first asserts, on the restatement
alone, that in every off-diagonal entry the largest |v| over the lags exceeds the runner-up by
more than two caps, so that no rounding within the caps can move the peak to another lag.

Shapes (C, W, step, L, windows), the smallest at which the kernel can go wrong: the least of
everything with L = W // 2; overlap and one partial tile; exactly one 64-sample staging step; C =
17 across the 16-row tile with an odd W past a step and the largest lag; W past 1024 with a lag
count that fills no group of 16; the longest window; gaps and C = 66 across the 32-row block of a
workgroup (and the 64-row mark), so off-diagonal blocks; C = 130, five blocks a side, for the
triangular index.  Data are seeded normal rows with ``x[1:] += 0.7 roll(x[:-1], 3)``, so the peaks
are real, at offsets of 0 and 100 sigma.

Everything else here is bit for bit."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer
from openseize_amd.features import _stream

from test_connectivity_host import RTOL
from test_xcorr_host import NAMES, caps, delayed, peak_margin, tie_rows, window_xcorr_measures

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 8, 4, 7), (3, 16, 5, 4, 7), (5, 64, 64, 8, 5), (17, 257, 100, 64, 4), (5, 1030, 515, 33, 4),
          (3, 4096, 4096, 64, 3), (66, 100, 150, 16, 4), (130, 64, 64, 5, 3)]
TILE, LONG, BLOCKS, MANY = SHAPES[3], SHAPES[4], SHAPES[6], SHAPES[7]


@pytest.fixture(scope="module")
def wx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_xcorr
    return window_xcorr


@lru_cache(maxsize=None)
def stream(shape, offset=0.0):
    """Seeded rows (C, n) of ``shape``: its windows and 3 samples of a window that is dropped.  Read-only."""
    nch, W, step, L, nwin = shape
    x = np.random.default_rng(29).standard_normal((nch, (nwin - 1) * step + W + 3))
    x[1:] += 0.7 * np.roll(x[:-1], 3, axis=1)
    x += offset
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def device_all(shape, offset=0.0, normalize=True):
    """(nwin, every measure) from one array call, computed once."""
    from openseize_amd.features import window_xcorr
    nch, W, step, L, nwin = shape
    return window_xcorr(stream(shape, offset), W, step, measures=NAMES, maxlag=L, normalize=normalize)


@lru_cache(maxsize=None)
def restated(shape, offset, normalize):
    nch, W, step, L, nwin = shape
    return caps(stream(shape, offset), W, step, L, normalize)


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_symmetric_with_fixed_points(M, L, normalize):
    X = M["xcorr"]
    for l in range(0, L + 1):
        assert same_bits(X[:, L + l], np.swapaxes(X[:, L - l], 1, 2)), l
    for name in ("peak", "signed"):
        assert same_bits(M[name], np.swapaxes(M[name], 1, 2)), name
    assert np.array_equal(M["lag"], -np.swapaxes(M["lag"], 1, 2), equal_nan=True)

    def diag(a):
        return np.diagonal(a, axis1=-2, axis2=-1)
    fixed = diag(X[:, L])
    ok = ~np.isnan(fixed)
    if normalize:
        assert np.all(fixed[ok] == 1.0)
    assert same_bits(diag(M["peak"]), fixed) and same_bits(diag(M["signed"]), fixed)
    assert np.all(diag(M["lag"])[ok] == 0.0) and np.all(np.isnan(diag(M["lag"])[~ok]))


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_restatement(wx, shape, offset):
    nch, W, step, L, nwin = shape
    for normalize in (True, False):
        want, cap = restated(shape, offset, normalize)
        margin = peak_margin(want, cap, L)
        print(f"C={nch} W={W} step={step} L={L} +{offset} normalize={normalize}: the peak leads by {margin:.2e} caps")
        assert margin > 2.0, (shape, offset, normalize, margin)
        n, M = device_all(shape, offset, normalize)
        assert n == nwin and list(M) == list(NAMES)
        assert M["xcorr"].shape == (nwin, 2 * L + 1, nch, nch) and np.all(np.isfinite(cap)) and np.all(cap > 0)
        for name in ("xcorr", "peak", "signed"):
            g, bound = M[name], cap[:, None] if name == "xcorr" else cap
            assert g.shape == want[name].shape and g.dtype == np.float64, (name, g.shape)
            ratio = float(np.max(np.abs(g - want[name]) / bound))
            print(f"    {name}: {ratio:.2e} of the cap")
            assert np.all(np.abs(g - want[name]) <= bound), (shape, offset, normalize, name, ratio)
        assert np.array_equal(M["lag"], want["lag"]), (shape, offset, normalize)
        assert np.array_equal(np.sign(M["signed"]), np.sign(want["signed"]))
        assert_symmetric_with_fixed_points(M, L, normalize)


@pytest.mark.parametrize("shape", [SHAPES[1], TILE, BLOCKS])
def test_lag_zero_is_window_connectivity_corr(wx, shape):
    from openseize_amd.features import window_connectivity
    nch, W, step, L, nwin = shape
    n, M = device_all(shape, 100.0, True)
    n2, corr = window_connectivity(stream(shape, 100.0), W, step, measures="corr")
    assert n2 == n and np.max(np.abs(M["xcorr"][:, L] - corr)) <= 2 * RTOL


@pytest.mark.parametrize("shape", [TILE, LONG, BLOCKS])
def test_chunking_host_or_device_axis_and_launches_change_no_bit(wx, shape, monkeypatch):
    import torch
    nch, W, step, L, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0, True)
    n2, G = wx(producer(np.array(x), 97, -1), W, step, measures=NAMES, maxlag=L)
    assert n2 == n
    for name in NAMES:
        assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), name
    t = torch.from_numpy(np.array(x)).cuda()
    n2, G = wx(t, W, step, measures=NAMES, maxlag=L)
    assert n2 == n
    for name in NAMES:
        assert isinstance(G[name], torch.Tensor) and G[name].is_cuda and G[name].dtype == torch.float64
        assert same_bits(G[name], F[name]), name
    n2, G = wx(np.ascontiguousarray(x.T), W, step, measures=NAMES, maxlag=L, axis=0)
    assert n2 == n
    for name in NAMES:
        assert G[name].shape == F[name].shape and same_bits(G[name], F[name]), name
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)           # every window is its own launch
    for data in (x, t):
        n2, G = wx(data, W, step, measures=NAMES, maxlag=L)
        assert n2 == n and all(same_bits(G[name], F[name]) for name in NAMES)


@pytest.mark.parametrize("normalize", [True, False])
def test_a_single_name_is_its_entry_of_the_whole(wx, normalize):
    nch, W, step, L, nwin = TILE
    x = stream(TILE, 100.0)
    n, F = device_all(TILE, 100.0, normalize)
    for name in NAMES:
        n2, one = wx(x, W, step, measures=name, maxlag=L, normalize=normalize)
        assert n2 == n and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    back = tuple(reversed(NAMES))
    n2, G = wx(x, W, step, measures=back, maxlag=L, normalize=normalize)
    assert list(G) == list(back) and all(same_bits(G[name], F[name]) for name in NAMES)
    if normalize:
        n2, G = wx(x, W, maxlag=L)                           # the defaults: step = winsize, peak and lag
        assert n2 == x.shape[1] // W and list(G) == ["peak", "lag"]
        assert same_bits(G["peak"][0], F["peak"][0]) and same_bits(G["lag"][0], F["lag"][0])


@pytest.mark.parametrize("shape,rows", [(BLOCKS, [3, 31, 32, 65]), (MANY, [15, 16, 63, 64, 129]), (TILE, [0, 16])])
def test_an_entry_depends_on_its_own_two_channels_only(wx, shape, rows):
    nch, W, step, L, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0, True)
    n2, G = wx(x[rows], W, step, measures=NAMES, maxlag=L)
    assert n2 == n
    for name in NAMES:
        assert same_bits(G[name], F[name][..., rows, :][..., rows]), name


def test_a_window_depends_on_neither_step_nor_maxlag(wx):
    nch, W, step, L, nwin = TILE
    x = stream(TILE, 100.0)
    n, F = device_all(TILE, 100.0, True)
    n2, H = wx(x, W, 2 * step, measures=NAMES, maxlag=L)
    assert n2 == (nwin + 1) // 2
    for name in NAMES:
        assert same_bits(H[name], F[name][::2]), name
    n1, one = wx(x[:, step:step + W], W, measures=NAMES, maxlag=L)
    assert n1 == 1 and all(same_bits(one[name][0], F[name][1]) for name in NAMES)
    for few in (0, 4, 17):
        for normalize in (True, False):
            n2, X = wx(x, W, step, measures="xcorr", maxlag=few, normalize=normalize)
            whole = device_all(TILE, 100.0, normalize)[1]["xcorr"]
            assert X.shape == (nwin, 2 * few + 1, nch, nch) and same_bits(X, whole[:, L - few:L + few + 1]), few


@pytest.mark.parametrize("normalize", [True, False])
def test_an_exact_tie_takes_the_positive_lag(wx, normalize):
    x = tie_rows()
    n, M = wx(x, 16, measures=NAMES, maxlag=4, normalize=normalize)
    want, _ = window_xcorr_measures(x, 16, 16, 4, normalize)
    v = M["xcorr"][0, :, 0, 1]
    assert n == 1 and same_bits(v[2], v[6]) and v[6] == np.abs(v).max()
    assert M["lag"][0, 0, 1] == 2.0 and M["lag"][0, 1, 0] == -2.0
    assert M["peak"][0, 0, 1] == M["signed"][0, 0, 1] == v[6]
    if normalize:
        assert np.max(np.abs(M["xcorr"] - want["xcorr"])) <= RTOL
    else:                                                    # every sum and the division by 16 are exact
        assert all(np.array_equal(M[name], want[name]) for name in NAMES)
    assert_symmetric_with_fixed_points(M, 4, normalize)


@pytest.mark.parametrize("d", [0, 1, 5, 16])
def test_a_delayed_channel_peaks_at_its_delay(wx, d):
    n, M = wx(delayed(d), 256, measures=("peak", "lag", "signed"), maxlag=16)
    assert n == 1 and M["lag"][0, 0, 1] == d and M["lag"][0, 1, 0] == -d
    assert M["peak"][0, 0, 1] > 0.9 and M["signed"][0, 0, 1] == M["peak"][0, 0, 1]


def held(nwin, W, step, at):
    k = np.arange(nwin)
    return (k * step <= at) & (at < k * step + W)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_sample_stays_in_its_row_and_column(wx, bad, normalize):
    nch, W, step, L, nwin = TILE
    n, F = device_all(TILE, 100.0, normalize)
    y = np.array(stream(TILE, 100.0))
    y[2, 130] = bad
    n2, G = wx(y, W, step, measures=NAMES, maxlag=L, normalize=normalize)
    hit = held(nwin, W, step, 130)
    assert n2 == n and 0 < hit.sum() < nwin
    lost = np.zeros((nwin, nch, nch), dtype=bool)
    lost[hit, 2, :] = lost[hit, :, 2] = True
    for name in NAMES:
        gone = np.broadcast_to(lost[:, None], G[name].shape) if name == "xcorr" else lost
        assert np.array_equal(np.isnan(G[name]), gone), name
        assert np.array_equal(bits(G[name])[~gone], bits(F[name])[~gone]), name


@pytest.mark.parametrize("normalize", [True, False])
def test_a_constant_channel(wx, normalize):
    nch, W, step, L, nwin = TILE
    n, F = device_all(TILE, 100.0, normalize)
    y = np.array(stream(TILE, 100.0))
    y[2] = 7.5
    n2, G = wx(y, W, step, measures=NAMES, maxlag=L, normalize=normalize)
    row = np.zeros((nch, nch), dtype=bool)
    row[2, :] = row[:, 2] = True
    for name in NAMES:
        if normalize:
            assert np.array_equal(np.isnan(G[name]), np.broadcast_to(row, G[name].shape)), name
        else:
            assert np.all(G[name][..., row] == 0.0), name
        assert np.array_equal(bits(G[name])[..., ~row], bits(F[name])[..., ~row]), name


def test_results_that_do_not_fit_the_device_are_refused(wx, monkeypatch):
    """CUDA-fed results stay on the device: when they cannot fit, MemoryError names the sizes before
    a kernel runs.  Host-fed results come down push by push and are not refused."""
    import torch
    from openseize_amd import _device as dev
    nch, W, step, L, nwin = TILE
    x = stream(TILE, 100.0)
    t = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 1 << 40))
    launched = []
    plain = dev.window_xcorr
    monkeypatch.setattr(dev, "window_xcorr", lambda *a, **k: (launched.append(1), plain(*a, **k))[1])
    with pytest.raises(MemoryError, match=r"step \(now 100; winsize 257\).*maxlag \(now 64\).*17 channels"):
        wx(t, W, step, maxlag=L)
    assert not launched
    n, M = wx(x, W, step, measures="peak", maxlag=L)
    assert n == nwin and launched and same_bits(M, device_all(TILE, 100.0, True)[1]["peak"])
