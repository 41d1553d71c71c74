"""window_quantiles on the device (K17) against ``window_quantile_stats``, the NumPy restatement of
the definitions (tests/test_quantiles_host.py), which sorts by the same integer keys.

Every comparison here is bit for bit: a measure is a selection from the sorted window followed by
at most four single IEEE operations, none contracted, so there is no tolerance to choose; and a
window's result depends on W, q and its own samples only."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_gpu_features import Reused, bits, same_bits
from test_quantiles_host import BOUNDS, NAMES, Q, window_quantile_stats

pytestmark = pytest.mark.gpu

SHAPES = [(4, 1), (5, 3), (63, 63), (64, 64), (65, 65), (250, 125), (67, 200), (1000, 333), (4096, 4096)]
SHAPES += [(W, 300) for B in BOUNDS for W in (B - 1, B, B + 1)                 # the two sides of every instance
           if W <= _lib.WQ_LONGEST and (W, 300) not in SHAPES]
WIDE = _lib.WQ_WAVE + 88                                     # a window of the 256-thread side
CUTS = [(250, 125), (67, 200), (WIDE, 250)]
Q16 = Q + (0.5, 0.999, 0.25, 1e-9, 0.5, 0.6180339887498949, 0.0, 1.0)


@pytest.fixture(scope="module")
def wq():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_quantiles
    return window_quantiles


@lru_cache(maxsize=None)
def walk():
    """A random walk plus noise plus an offset, 3 x 12 288, from a fixed seed.  Read-only."""
    rng = np.random.default_rng(47)
    x = np.cumsum(rng.standard_normal((3, 12288)), axis=-1) * 0.3 + rng.standard_normal((3, 12288)) + 100.0
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def signal(W, step, quantised=False):
    """Three windows of each channel of walk(), rounded to integers when ``quantised`` so that
    ties occur."""
    x = walk()[:, :min(W + 2 * step, 12288)]
    x = np.round(x) if quantised else np.array(x)
    x.setflags(write=False)
    return x


def assert_bits(F, ref, what):
    """The same NaN pattern, and the same bits everywhere else (which NaN an invalid operation gives
    is the processor's choice: its sign differs between the host and the device)."""
    for name in NAMES:
        got = F[name]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref[name].shape, (what, name)
        lost = np.isnan(ref[name])
        assert np.array_equal(np.isnan(got), lost), (what, name, got, ref[name])
        wrong = (bits(got) != bits(ref[name])) & ~lost
        assert not wrong.any(), (what, name, int(wrong.sum()), got[wrong][:4], ref[name][wrong][:4])


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("W,step", SHAPES)
def test_parity_with_the_restatement(wq, W, step, quantised):
    x = signal(W, step, quantised)
    if quantised:
        assert len(np.unique(x[0, :W])) < W or W < 6         # ties
    ref = window_quantile_stats(x, W, step, Q)
    nwin, F = wq(x, W, step, measures=NAMES, q=Q)
    assert nwin == ref["median"].shape[1] in (2, 3) and list(F) == list(NAMES)
    assert F["quantile"].shape == (len(Q), 3, nwin)
    assert_bits(F, ref, (W, step, quantised))
    assert not np.isnan(F["mad"]).any() and (quantised or np.all(F["mad"] > 0))


@pytest.mark.parametrize("W,step", [(5, 3), (250, 125), (WIDE, 250), (4096, 4096)])
def test_sixteen_quantiles_with_duplicates(wq, W, step):
    x = signal(W, step)
    assert len(Q16) == _lib.WQ_QMOST and len(set(Q16)) < len(Q16)
    ref = window_quantile_stats(x, W, step, Q16)
    nwin, F = wq(x, W, step, measures=NAMES, q=Q16)
    assert_bits(F, ref, (W, step))
    assert same_bits(F["quantile"][4], F["quantile"][8]) and same_bits(F["quantile"][2], F["quantile"][10])


def edge_data(W):
    """(4, 3 W): signed zeros; +-inf in a minority and in a majority of a window's samples; both
    signs over 600 orders of magnitude, subnormals included."""
    rng = np.random.default_rng(53)
    n = 3 * W
    zeros = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    other = rng.random(n) < 0.2
    zeros[other] = rng.choice([-1.5, 2.0], int(other.sum()))
    few = rng.standard_normal(n)
    few[rng.random(n) < 0.1] = np.inf
    few[rng.random(n) < 0.1] = -np.inf
    many = rng.standard_normal(n)
    many[rng.random(n) < 0.7] = np.inf
    many[2 * W:][rng.random(W) < 0.8] = -np.inf                                         # (the last window: -inf)
    wide = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-323.5, 300, n)
    wide[::7] = rng.choice([-1.0, 1.0], len(wide[::7])) * 5e-324 * rng.integers(1, 9, len(wide[::7]))
    return np.stack([zeros, few, many, wide])


@pytest.mark.parametrize("W", [4, 64, 250, WIDE, 4096])
def test_signed_zeros_infinities_and_the_whole_range(wq, W):
    x = edge_data(W)
    ref = window_quantile_stats(x, W, W, Q)
    nwin, F = wq(x, W, measures=NAMES, q=Q)
    assert nwin == 3
    assert_bits(F, ref, W)
    if W >= 64:
        zero = bits(x[0].reshape(3, W))
        assert np.all((zero == 0).any(axis=1) & (zero == 1 << 63).any(axis=1))          # both zeros in every window
        assert np.all(F["median"][0] == 0)
        assert np.isnan(F["mad"][2]).all() and np.isinf(F["median"][2]).all()           # the majority
        assert not np.isnan(F["mad"][1]).any() and np.isfinite(F["median"][1]).all()    # the minority
        assert not np.isnan(F["median"]).any()


@lru_cache(maxsize=None)
def long_signal():
    x = walk()[:, :2000]
    return x


@lru_cache(maxsize=None)
def device_all(W, step):
    """(nwin, all three measures) of long_signal() from one array call, computed once."""
    from openseize_amd.features import window_quantiles
    return window_quantiles(long_signal(), W, step, measures=NAMES, q=Q)


@pytest.mark.parametrize("W,step", CUTS)
def test_chunking_host_or_device_axis_and_recycled_buffers_change_no_bit(wq, W, step):
    import torch
    x = long_signal()
    nwin, F = device_all(W, step)
    assert nwin == (2000 - W) // step + 1
    assert_bits(F, window_quantile_stats(x, W, step, Q), (W, step))
    for cs in (7, W - 1, 777):
        n2, G = wq(producer(np.array(x), cs, -1), W, step, measures=NAMES, q=Q)
        assert n2 == nwin
        for name in NAMES:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (cs, name)
    xd = torch.from_numpy(np.array(x)).cuda()
    n2, G = wq(xd, W, step, measures=NAMES, q=Q, chunksize=301)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].is_cuda and same_bits(G[name], F[name]), name
    n2, G = wq(np.ascontiguousarray(x.T), W, step, measures=NAMES, q=Q, axis=0, chunksize=500)
    assert n2 == nwin
    assert G["median"].shape == (nwin, 3) and G["quantile"].shape == (len(Q), nwin, 3)
    for name in NAMES:
        assert same_bits(np.swapaxes(G[name], -1, -2), F[name]), name
    for pro in (Reused(xd, 333, -1), Reused(xd, 64, -1)):
        n2, G = wq(pro, W, step, measures=NAMES, q=Q)
        assert n2 == nwin
        for name in NAMES:
            assert G[name].is_cuda and same_bits(G[name], F[name]), name


def test_a_single_name_and_a_scalar_q_are_entries_of_the_whole(wq):
    x = long_signal()
    nwin, F = device_all(250, 125)
    for name in NAMES:
        n2, one = wq(x, 250, 125, measures=name, q=Q)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    for j, p in enumerate(Q):
        n2, one = wq(x, 250, 125, measures="quantile", q=p)
        assert one.shape == (3, nwin) and same_bits(one, F["quantile"][j]), p
    n2, G = wq(x, 250, 125, measures=("quantile",), q=(0.9, 0.05))         # another order, other company
    assert list(G) == ["quantile"] and G["quantile"].shape == (2, 3, nwin)
    assert same_bits(G["quantile"][0], F["quantile"][6]) and same_bits(G["quantile"][1], F["quantile"][1])
    n2, G = wq(x, 250, 125, measures=("quantile", "median"), q=[0.75])
    assert list(G) == ["quantile", "median"] and G["quantile"].shape == (1, 3, nwin)
    assert same_bits(G["quantile"][0], F["quantile"][5]) and same_bits(G["median"], F["median"])
    n2, G = wq(x, 250, 125, measures=("mad",))                             # (the median is not returned)
    assert list(G) == ["mad"] and same_bits(G["mad"], F["mad"])
    n2, G = wq(x, 250)                                                     # the defaults: step = winsize
    assert n2 == 8 and list(G) == ["median", "mad"]
    assert same_bits(G["median"], F["median"][:, ::2]) and same_bits(G["mad"], F["mad"][:, ::2])
    n2, one = wq(x, 250, 125, measures="quantile")                         # q = (0.25, 0.75)
    assert same_bits(one, F["quantile"][[2, 5]])


@pytest.mark.parametrize("W,step", CUTS)
def test_a_window_depends_on_its_own_samples_only(wq, W, step):
    x = long_signal()
    nwin, F = device_all(W, step)
    for k in sorted({1, nwin // 2, nwin - 1}):
        n1, G = wq(x[:, k * step:k * step + W], W, measures=NAMES, q=Q)    # alone, another step
        assert n1 == 1
        for name in NAMES:
            assert same_bits(G[name][..., 0], F[name][..., k]), (name, k)
    # the samples around window 2 changed: the stream's first two and last windows go
    y = np.array(x)
    y[:, :2 * step] = -3.0
    y[:, 2 * step + W:] *= 1.5
    n2, G = wq(y, W, step, measures=NAMES, q=Q)
    for name in NAMES:
        assert same_bits(G[name][..., 2], F[name][..., 2]), name
    # one row alone and 257 copies of it
    n1, one = wq(x[1], W, step, measures=NAMES, q=Q)
    n257, many = wq(np.tile(x[1], (257, 1)), W, step, measures=NAMES, q=Q)
    assert n1 == n257 == nwin
    for name in NAMES:
        lead = (len(Q),) if name == "quantile" else ()
        assert one[name].shape == lead + (nwin,) and same_bits(one[name], F[name][..., 1, :]), name
        assert many[name].shape == lead + (257, nwin)
        want = np.broadcast_to(bits(F[name][..., 1, :])[..., None, :], lead + (257, nwin))
        assert np.array_equal(bits(many[name]), want), name


@pytest.mark.parametrize("W,step", [(250, 125), (WIDE, 250)])
def test_nan_stays_in_its_windows(wq, W, step):
    x = long_signal()
    nwin, clean = device_all(W, step)
    y = np.array(x)
    y[1, 701] = np.nan                                       # (overlapping windows hold it)
    y[2, 1300] = -np.nan
    y[0, 0] = np.nan                                         # a window's first sample
    n2, F = wq(producer(y, 409, -1), W, step, measures=NAMES, q=Q)
    k = np.arange(nwin)
    hit = np.zeros((3, nwin), dtype=bool)
    hit[0] = k == 0
    hit[1] = (k * step <= 701) & (701 < k * step + W)
    hit[2] = (k * step <= 1300) & (1300 < k * step + W)
    assert hit[1].sum() >= 2 and hit[2].sum() >= 2 and n2 == nwin
    for name in NAMES:
        assert np.array_equal(np.isnan(F[name]), np.broadcast_to(hit, F[name].shape)), name
        assert np.array_equal(bits(F[name])[..., ~hit], bits(clean[name])[..., ~hit]), name


def test_more_windows_than_a_grid_dimension(wq):
    rng = np.random.default_rng(59)
    x = np.round(np.cumsum(rng.standard_normal((1, 70000)), axis=-1) * 0.3 + rng.standard_normal((1, 70000)), 1)
    picks = np.unique(np.concatenate([np.arange(0, 69993, 1747), [65534, 65535, 65536, 69992]]))
    ref = window_quantile_stats(x, 8, 1, Q)                  # (every window: a sort of eight samples each)
    nwin, F = wq(x, 8, 1, measures=NAMES, q=Q)
    assert nwin == 69993 > 65535 and F["median"].shape == (1, nwin) and F["quantile"].shape == (len(Q), 1, nwin)
    for name in NAMES:
        assert np.array_equal(bits(F[name])[..., picks], bits(ref[name])[..., picks]), name


def test_kinds_shapes_and_counts(wq):
    import ctypes
    import torch
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.osz_window_count.restype, lib.osz_window_count.argtypes = _lib.SIGNATURES["osz_window_count"]
    x = long_signal()
    for W, step in ((250, 125), (67, 200), (2000, 1), (1999, 1)):
        nwin, F = wq(x, W, step, measures="mad")
        assert nwin == lib.osz_window_count(2000, W, step) and isinstance(F, np.ndarray) and F.shape == (3, nwin)
        nwin, F = wq(torch.from_numpy(np.array(x[0])).cuda(), W, step, measures=("quantile", "median"), q=(0.1, 0.9))
        assert nwin == lib.osz_window_count(2000, W, step) and list(F) == ["quantile", "median"]
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 for v in F.values())
        assert tuple(F["quantile"].shape) == (2, nwin) and tuple(F["median"].shape) == (nwin,)
    with pytest.raises(ValueError, match="fewer than one window"):
        wq(torch.from_numpy(np.array(x)).cuda(), 2001)
    # a constant window
    nwin, F = wq(np.full((2, 300), 7.5), 100, measures=NAMES, q=Q)
    assert nwin == 3 and np.all(F["median"] == 7.5) and np.all(F["mad"] == 0) and np.all(F["quantile"] == 7.5)

    # a source that says it is longer than it is: found when the stream ends
    def short():
        yield torch.zeros((3, 90), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="before one window"):
        wq(producer(short, chunksize=50, axis=-1, shape=(3, 5000)), 100)
