"""window_transfer_entropy on the device (K26) against ``window_te_measures``, the NumPy restatement
of the definition (tests/test_te_host.py).

``counts`` must be exactly equal: the bins are K25's bytes and the counts are integer sums on the
int8 matrix pipe.  The product is rectangular, with two different operands, so an exact ``counts``
pins the row map of either operand, which operand is which, and the map of the accumulators.
``te``, ``nte`` and ``net`` stay within RTOL = 1e-9 (the suite's cap), absolute on every entry; the
derived bound is about 1e-12 -- at most B^3 + 2 B^2 + B <= 648 terms of size <= T ln T, divided by T
-- and the ratio to the cap is printed.

Shapes (C, W, step, B, lag, binning, windows), the smallest at which each kernel can go wrong: the
least of everything (T = 15); T = 64, exactly one matrix step, with overlap, and a target channel
that is one block; padded T, gaps and B = 3 padded to 4, so that 20 source rows cross a tile; T =
65, one past a step, with 272 target and 68 source rows, partial last blocks on both sides, and two
finish tiles; an odd W past 1024 (the 1024-thread code instance) with 9 x 2 blocks; the longest
window and lag; lag = W / 2; 130 channels of few bins.  Data are ``mixed`` rows at offsets of 0 and
100 sigma, with 7 channels or more one row a constant and the last row driven by row 0 at the
shape's lag.

Everything else here is bit for bit."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer
from openseize_amd.features import _stream

from test_connectivity_host import RTOL
from test_te_host import CONSTANT, NAMES, SHAPES, assert_driven_pair_is_seen, restated, stream, window_te_measures

pytestmark = pytest.mark.gpu

ONE, CROSS, TILE, MANY = SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[7]
TILED = [ONE, CROSS, TILE]


@pytest.fixture(scope="module")
def wt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_transfer_entropy
    return window_transfer_entropy


def keywords(shape):
    nch, W, step, B, lag, binning, nwin = shape
    return dict(measures=NAMES, bins=B, lag=lag, binning=binning)


@lru_cache(maxsize=None)
def device_all(shape, offset=0.0):
    """(nwin, every measure) from one array call, computed once."""
    from openseize_amd.features import window_transfer_entropy
    nch, W, step, B, lag, binning, nwin = shape
    return window_transfer_entropy(stream(shape, offset), W, step, **keywords(shape))


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_antisymmetric_with_fixed_points(M):
    """net[j, i] is -net[i, j] with +0.0 for a zero on both sides; the diagonal of te, nte and net is
    +0.0 (NaN for a row that is lost), bit for bit."""
    net = M["net"]
    back = -np.swapaxes(net, 1, 2)
    back = np.where(back == 0.0, 0.0, back)                  # (-0.0 -> +0.0)
    assert np.array_equal(np.isnan(net), np.isnan(back))
    ok = ~np.isnan(net)
    assert np.array_equal(bits(net)[ok], bits(back)[ok])
    for name in NAMES[1:]:
        d = np.diagonal(M[name], axis1=1, axis2=2)
        lost = np.isnan(np.diagonal(M["te"], axis1=1, axis2=2))
        assert np.all(bits(d)[~lost] == 0) and np.all(np.isnan(d[lost])), name


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_restatement(wt, shape, offset):
    nch, W, step, B, lag, binning, nwin = shape
    T = W - lag
    want = restated(shape, offset)
    n, M = device_all(shape, offset)
    assert n == nwin and list(M) == list(NAMES)
    assert M["counts"].shape == (nwin, B, B, B, nch, nch) and M["counts"].dtype == np.float64
    wrong = int(np.sum(M["counts"] != want["counts"]))
    print(f"C={nch} W={W} step={step} B={B} lag={lag} {binning} +{offset}: {wrong} of {want['counts'].size} counts differ")
    assert np.all(np.isfinite(want["counts"])) and want["counts"].max() <= T
    assert np.array_equal(M["counts"], want["counts"]), (shape, offset, wrong)
    assert np.all(M["counts"].sum(axis=(1, 2, 3)) == T)
    ab = M["counts"].sum(axis=3)
    assert np.all(ab == ab[:, :, :, :1, :])                  # the same for every source of a target
    for name in NAMES[1:]:
        g = M[name]
        assert g.shape == want[name].shape == (nwin, nch, nch) and g.dtype == np.float64, (name, g.shape)
        assert np.array_equal(np.isnan(g), np.isnan(want[name])), name
        err = np.abs(g - want[name])[~np.isnan(g)]
        ratio = float(err.max() / RTOL)
        print(f"    {name}: {ratio:.2e} of the cap")
        assert np.all(err <= RTOL), (shape, offset, name, ratio)
    assert np.all(M["te"][~np.isnan(M["te"])] >= 0.0) and not np.any(np.signbit(M["te"]))
    assert_antisymmetric_with_fixed_points(M)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 7])
def test_the_constant_row_reaches_a_full_cell_and_gives_zero(wt, shape):
    nch, W, step, B, lag, binning, nwin = shape
    n, M = device_all(shape, 100.0)
    c = CONSTANT
    assert np.all(M["counts"][:, B - 1, B - 1, B - 1, c, c] == W - lag)        # all bin B - 1: one cell holds T
    assert np.all(M["counts"][:, B - 1, B - 1, :, :, c].sum(axis=1) == W - lag)
    for line in (M["te"][:, c, :], M["te"][:, :, c]):        # as a source and as a target
        assert np.all(bits(line) == 0)
    others = np.arange(nch) != c
    assert np.all(np.isnan(M["nte"][:, others, c])) and not np.any(np.isnan(M["nte"][:, c, :]))
    assert np.all(bits(M["nte"][:, c, :]) == 0)
    # the last row is driven by row 0 at this lag
    print(f"C={nch} lag={lag}: te 0 -> last {M['te'][:, 0, nch - 1]}, last -> 0 {M['te'][:, nch - 1, 0]}")
    if W >= 1000:                                            # (enough samples to tell)
        assert np.all(M["net"][:, 0, nch - 1] > 0)


@pytest.mark.parametrize("shape", TILED)
def test_chunking_host_or_device_axis_and_launches_change_no_bit(wt, shape, monkeypatch):
    import torch
    nch, W, step, B, lag, binning, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    kw = keywords(shape)
    for chunk in (97, W + 1):
        n2, G = wt(producer(np.array(x), chunk, -1), W, step, **kw)
        assert n2 == n
        for name in NAMES:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (chunk, name)
    t = torch.from_numpy(np.array(x)).cuda()
    n2, G = wt(t, W, step, **kw)
    assert n2 == n
    for name in NAMES:
        assert isinstance(G[name], torch.Tensor) and G[name].is_cuda and G[name].dtype == torch.float64
        assert same_bits(G[name], F[name]), name
    n2, G = wt(np.ascontiguousarray(x.T), W, step, axis=0, **kw)
    assert n2 == n
    for name in NAMES:
        assert G[name].shape == F[name].shape and same_bits(G[name], F[name]), name
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)           # every window is its own launch
    for data in (x, t):
        n2, G = wt(data, W, step, **kw)
        assert n2 == n and all(same_bits(G[name], F[name]) for name in NAMES)


@pytest.mark.parametrize("shape", TILED)
def test_a_single_name_is_its_entry_of_the_whole(wt, shape):
    nch, W, step, B, lag, binning, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    for name in NAMES:
        n2, one = wt(x, W, step, measures=name, bins=B, lag=lag, binning=binning)
        assert n2 == n and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    back = tuple(reversed(NAMES))
    n2, G = wt(x, W, step, measures=back, bins=B, lag=lag, binning=binning)
    assert list(G) == list(back) and all(same_bits(G[name], F[name]) for name in NAMES)
    n2, G = wt(x, W, bins=B, lag=lag, binning=binning)       # the defaults: step = winsize, te alone, a dict
    assert n2 == x.shape[1] // W and list(G) == ["te"] and same_bits(G["te"][0], F["te"][0])


@pytest.mark.parametrize("shape,rows", [(TILE, [0, 16]), (TILE, [16, 3]), (CROSS, [1, 4]), (ONE, [2, 0]),
                                        (MANY, [31, 129])])
def test_an_entry_depends_on_its_own_two_channels_only(wt, shape, rows):
    nch, W, step, B, lag, binning, nwin = shape
    n, F = device_all(shape, 100.0)
    n2, G = wt(stream(shape, 100.0)[rows], W, step, **keywords(shape))
    assert n2 == n
    for name in NAMES:
        assert same_bits(G[name], F[name][..., rows, :][..., rows]), name


@pytest.mark.parametrize("shape", TILED)
def test_a_window_does_not_depend_on_step_or_on_its_call(wt, shape):
    nch, W, step, B, lag, binning, nwin = shape
    x = stream(shape, 100.0)
    n, F = device_all(shape, 100.0)
    n2, H = wt(x, W, 2 * step, **keywords(shape))
    assert n2 == (nwin + 1) // 2
    for name in NAMES:
        assert same_bits(H[name], F[name][::2]), name
    for k in range(nwin):                                    # the windows of one call against separate calls
        n1, one = wt(x[:, k * step:k * step + W], W, **keywords(shape))
        assert n1 == 1 and all(same_bits(one[name][0], F[name][k]) for name in NAMES), k


def test_windows_on_both_sides_of_a_batch_edge(wt):
    """34 channels of 5 bins (padded to 8): a window's count matrix is 34^2 8^3 / 2 doubles, so one
    batch of kGramCap = 2^25 doubles holds 113 windows; 115 windows cross one edge."""
    lib = _lib.load()
    nch, W, B, lag, cap = 34, 16, 5, 1, 1 << 25
    one = nch * nch * 8 ** 3 // 2
    batch = cap // one
    nwin = batch + 2
    n = nwin - 1 + W
    front = nch * (16 + 18 + 2 * 8)
    assert 1 < batch < nwin < 2 * batch
    assert lib.osz_window_te_work(nch, n, W, 1, B, lag, 0b11) == ((W + 2) & ~1) + batch * (front + one)
    assert lib.osz_window_te_work(nch, batch - 1 + W, W, 1, B, lag, 0b11) == ((W + 2) & ~1) + batch * (front + one)
    assert lib.osz_window_te_work(nch, batch - 2 + W, W, 1, B, lag, 0b11) == ((W + 2) & ~1) + (batch - 1) * (front + one)
    x = np.random.default_rng(43).standard_normal((nch, n))
    x[1:] += 0.7 * x[:-1]
    kw = dict(measures=("te", "counts"), bins=B, lag=lag, binning="quantile")
    n2, F = wt(x, W, 1, **kw)
    assert n2 == nwin
    for k in (0, batch - 1, batch, nwin - 1):                # both sides of the edge, from one-batch calls
        n1, one_call = wt(x[:, k:k + W], W, 1, **kw)
        assert n1 == 1
        for name in ("te", "counts"):
            assert same_bits(one_call[name][0], F[name][k]), (k, name)
    want = window_te_measures(x[:, batch - 1:batch + W], W, 1, B, lag, "quantile")
    assert np.array_equal(F["counts"][batch - 1:batch + 1], want["counts"])
    assert np.max(np.abs(F["te"][batch - 1:batch + 1] - want["te"])) <= RTOL


def held(nwin, W, step, at):
    k = np.arange(nwin)
    return (k * step <= at) & (at < k * step + W)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("shape", TILED)
def test_a_non_finite_sample_stays_in_its_row_and_column(wt, shape, bad):
    nch, W, step, B, lag, binning, nwin = shape
    n, F = device_all(shape, 100.0)
    y = np.array(stream(shape, 100.0))
    at = step + 5                                            # in window 1, and in window 0 where they overlap
    y[2, at] = bad
    n2, G = wt(y, W, step, **keywords(shape))
    hit = held(nwin, W, step, at)
    assert n2 == n and 0 < hit.sum() < nwin
    lost = np.zeros((nwin, nch, nch), dtype=bool)
    lost[hit, 2, :] = lost[hit, :, 2] = True
    for name in NAMES:
        gone = np.broadcast_to(lost[:, None, None, None], G[name].shape) if name == "counts" else lost
        was = np.isnan(F[name])
        assert np.array_equal(np.isnan(G[name]), gone | was), name
        assert np.array_equal(bits(G[name])[~gone], bits(F[name])[~gone]), name


def test_the_driven_pair_on_the_device(wt):
    assert_driven_pair_is_seen(lambda rows, lag: wt(rows, 1024, 1024, measures="te", bins=4, lag=lag)[1])


def test_work_or_results_that_do_not_fit_the_device_are_refused(wt, monkeypatch):
    """MemoryError names bins and the channel count before anything is launched: for the work space of
    a launch, whatever feeds it, and for CUDA-fed results, which stay on the device."""
    import torch
    from openseize_amd import _device as dev
    nch, W, step, B, lag, binning, nwin = TILE
    x = stream(TILE, 100.0)
    t = torch.from_numpy(np.array(x)).cuda()
    launched = []
    plain = dev.window_te
    monkeypatch.setattr(dev, "window_te", lambda *a, **k: (launched.append(1), plain(*a, **k))[1])
    with monkeypatch.context() as low:
        low.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 1 << 40))
        with pytest.raises(MemoryError, match=r"64 more for counts.*step \(now 66; winsize 66\).*bins \(now 4\).*17 channels"):
            wt(t, W, step, measures=("te", "counts"), bins=B, lag=lag, binning=binning)
        with pytest.raises(MemoryError, match=r"work space.*bins \(now 4\).*17 channels"):
            wt(x, W, step, measures="te", bins=B, lag=lag, binning=binning)
        assert not launched
    n, M = wt(x, W, step, measures="te", bins=B, lag=lag, binning=binning)
    assert n == nwin and launched and same_bits(M, device_all(TILE, 100.0)[1]["te"])
