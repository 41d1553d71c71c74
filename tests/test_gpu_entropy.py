"""window_entropy on the device (K16) against ``window_entropies``, the NumPy restatement of the
definitions (tests/test_entropy_host.py): the brute-force pair matrix and stable ranks.

Bounds.  ``sample_a`` and ``sample_b`` are exact: the device's rho differs from the restatement's
in the last bits only (the project's cap on a variance is 1e-9 relative, 5e-10 on rho), and every
parity test first asserts on the restatement that no element difference |x_a - x_b| of the window
lies within 1e-8 rho of rho, so no comparison can fall the other way.  ``sample`` is one division
and one logarithm of exact integers: 1e-12 relative where finite, the same kind (+inf, NaN) where
not.  ``permutation`` is a sum of at most 720 terms of magnitude <= 0.53, each good to a few ulp:
1e-12 absolute.

Everything else here is bit for bit: a window's result depends on W, the parameters and its own
samples only."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_entropy_host import (NAMES, pair_distances, pair_matches, permutation_entropy, sample_counts,
                               sample_entropy, window_entropies)
from test_gpu_features import Reused, bits, same_bits

pytestmark = pytest.mark.gpu

WIDE = _lib.WE_WIDE
SHAPES = [(4, 1), (5, 3), (63, 63), (64, 64), (65, 65), (250, 125), (67, 200), (1000, 333), (4096, 4096),
          (WIDE - 1, 300), (WIDE, 300), (WIDE + 1, 300)]          # (and the two sides of the 256-thread kernel)
CUTS = [(250, 125), (67, 200), (WIDE + 88, 250)]
R = {"std": 0.2, "absolute": 0.5}
MARGIN = 1e-8


@pytest.fixture(scope="module")
def we():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_entropy
    return window_entropy


@lru_cache(maxsize=None)
def walk():
    """A random walk plus noise plus an offset, 3 x 12 288, from a fixed seed.  Read-only."""
    rng = np.random.default_rng(41)
    x = np.cumsum(rng.standard_normal((3, 12288)), axis=-1) * 0.3 + rng.standard_normal((3, 12288)) + 100.0
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def signal(W, step, quantised=False):
    """Three windows of each channel of walk() (two of 4096 samples), rounded to integers when
    ``quantised`` so that ties occur."""
    x = walk()[:, :W + 2 * step if W < 4096 else 2 * W]
    x = np.round(x) if quantised else np.array(x)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def sample_reference(W, step, quantised=False):
    """(m, tolerance) -> name -> (3, nwin) of signal(W, step) for m = 1 .. 3 and both tolerances,
    "margin" beside the measures; the pair distances of a window are taken once."""
    x = signal(W, step, quantised)
    nwin = (x.shape[1] - W) // step + 1
    ref = {(m, tol): {name: np.full((3, nwin), np.nan) for name in ("sample", "sample_a", "sample_b", "margin")}
           for m in (1, 2, 3) for tol in R if W >= m + 2}
    for c in range(3):
        for k in range(nwin):
            w = x[c, k * step:k * step + W]
            dist = pair_distances(w)
            for tol in R:
                match, margin = pair_matches(dist, R[tol] * np.std(w) if tol == "std" else R[tol])
                for m in (1, 2, 3):
                    if W >= m + 2:
                        A, B = sample_counts(match, m)
                        out = ref[m, tol]
                        out["sample"][c, k], out["sample_a"][c, k], out["sample_b"][c, k] = sample_entropy(A, B), A, B
                        out["margin"][c, k] = margin
    return ref


def assert_sample(got, ref, what):
    assert float(ref["margin"].min()) > MARGIN, (what, ref["margin"].min())
    for name in ("sample_a", "sample_b"):
        assert got[name].dtype == np.float64 and np.array_equal(got[name], ref[name]), (what, name, got[name])
    g, r = got["sample"], ref["sample"]
    fin = np.isfinite(r)
    assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g == np.inf, r == np.inf), (what, g, r)
    assert np.array_equal(np.isfinite(g), fin), (what, g, r)
    over = np.abs(g[fin] - r[fin]) - 1e-12 * np.abs(r[fin])  # (A = B gives 0, and 0 it has to be)
    print(f"{what} sample: over 1e-12 relative by {float(over.max()) if fin.any() else 0.0:.2e}")
    assert np.all(over <= 0), (what, g, r)


def permutation_reference(x, W, step, order, delay, normalize):
    nwin = (x.shape[1] - W) // step + 1
    return np.array([[permutation_entropy(x[c, k * step:k * step + W], order, delay, normalize)
                      for k in range(nwin)] for c in range(x.shape[0])])


@pytest.mark.parametrize("tol", list(R))
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("W,step", SHAPES)
def test_sample_parity_with_the_restatement(we, W, step, m, tol):
    x = signal(W, step)
    if W < m + 2:                                            # no pair of templates
        with pytest.raises(ValueError, match="m \\+ 2"):
            we(x, W, step, measures=NAMES, m=m, r=R[tol], tolerance=tol, order=2)
        return
    ref = sample_reference(W, step)[m, tol]
    assert float(ref["margin"].min()) > MARGIN               # (before the device is asked)
    nwin, F = we(x, W, step, measures=NAMES, m=m, r=R[tol], tolerance=tol, order=2)
    assert nwin == ref["sample"].shape[1] in (2, 3) and list(F) == list(NAMES)
    assert_sample(F, ref, (W, step, m, tol))
    err = float(np.max(np.abs(F["permutation"] - permutation_reference(x, W, step, 2, 1, True))))
    assert err < 1e-12, err


@pytest.mark.parametrize("tol", list(R))
@pytest.mark.parametrize("W,step", SHAPES)
def test_sample_parity_on_quantised_data(we, W, step, tol):
    x = signal(W, step, True)
    assert len(np.unique(x[0, :W])) < W or W < 6             # ties
    ref = sample_reference(W, step, True)[2, tol]
    assert float(ref["margin"].min()) > MARGIN
    nwin, F = we(x, W, step, measures=("sample_b", "sample", "sample_a"), m=2, r=R[tol], tolerance=tol)
    assert list(F) == ["sample_b", "sample", "sample_a"]
    assert_sample(F, ref, (W, step, tol, "quantised"))
    if W >= 63:
        assert ref["sample_a"].min() > 0


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("W,step", SHAPES)
def test_permutation_parity_with_the_restatement(we, W, step, quantised):
    x = signal(W, step, quantised)
    for order in (2, 3, 4, 5, 6):
        for delay in (1, 3):
            if W <= (order - 1) * delay:                     # no vector
                with pytest.raises(ValueError, match="order - 1"):
                    we(x, W, step, measures="permutation", order=order, delay=delay)
                continue
            for normalize in (True, False):
                nwin, H = we(x, W, step, measures="permutation", order=order, delay=delay, normalize=normalize)
                ref = permutation_reference(x, W, step, order, delay, normalize)
                assert H.shape == ref.shape and H.dtype == np.float64
                err = float(np.max(np.abs(H - ref)))
                assert err < 1e-12, (W, order, delay, normalize, err)
    if W >= 250 and not quantised:
        assert 0.5 < ref.min() and ref.max() < np.log2(720)  # (the last: order 6, bits)


@lru_cache(maxsize=None)
def long_signal():
    x = walk()[:, :2000]
    return x


KW = dict(m=2, r=0.2, order=4, delay=2)


@lru_cache(maxsize=None)
def device_all(W, step):
    """(nwin, all four measures) of long_signal() from one array call, computed once."""
    from openseize_amd.features import window_entropy
    return window_entropy(long_signal(), W, step, measures=NAMES, **KW)


@pytest.mark.parametrize("W,step", CUTS)
def test_chunking_host_or_device_axis_and_recycled_buffers_change_no_bit(we, W, step):
    import torch
    x = long_signal()
    nwin, F = device_all(W, step)
    assert nwin == (2000 - W) // step + 1
    for cs in (7, W - 1, 777):
        n2, G = we(producer(np.array(x), cs, -1), W, step, measures=NAMES, **KW)
        assert n2 == nwin
        for name in NAMES:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (cs, name)
    xd = torch.from_numpy(np.array(x)).cuda()
    n2, G = we(xd, W, step, measures=NAMES, chunksize=301, **KW)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].is_cuda and same_bits(G[name], F[name]), name
    n2, G = we(np.ascontiguousarray(x.T), W, step, measures=NAMES, axis=0, chunksize=500, **KW)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].shape == (nwin, 3) and same_bits(G[name].T, F[name]), name
    for pro in (Reused(xd, 333, -1), Reused(xd, 64, -1)):
        n2, G = we(pro, W, step, measures=NAMES, **KW)
        assert n2 == nwin
        for name in NAMES:
            assert G[name].is_cuda and same_bits(G[name], F[name]), name


def test_a_single_name_is_its_entry_of_the_whole(we):
    x = long_signal()
    nwin, F = device_all(250, 125)
    for name in NAMES:
        n2, one = we(x, 250, 125, measures=name, **KW)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    n2, G = we(x, 250, 125, measures=("permutation", "sample_b"), **KW)
    assert list(G) == ["permutation", "sample_b"]
    assert same_bits(G["permutation"], F["permutation"]) and same_bits(G["sample_b"], F["sample_b"])
    n2, G = we(x, 250)                                       # the defaults: step = winsize, both entropies
    assert n2 == 8 and list(G) == ["sample", "permutation"]
    assert same_bits(G["sample"], F["sample"][:, ::2])       # (m = 2, r = 0.2 are the defaults)


@pytest.mark.parametrize("W,step", CUTS)
def test_a_window_depends_on_its_own_samples_only(we, W, step):
    x = long_signal()
    nwin, F = device_all(W, step)
    for k in sorted({1, nwin // 2, nwin - 1}):
        n1, G = we(x[:, k * step:k * step + W], W, measures=NAMES, **KW)       # alone, another step
        assert n1 == 1
        for name in NAMES:
            assert same_bits(G[name][:, 0], F[name][:, k]), (name, k)
    # the samples around window 2 changed: the stream's first two and last windows go
    y = np.array(x)
    y[:, :2 * step] = -3.0
    y[:, 2 * step + W:] *= 1.5
    n2, G = we(y, W, step, measures=NAMES, **KW)
    for name in NAMES:
        assert same_bits(G[name][:, 2], F[name][:, 2]), name
    # one row alone and 257 copies of it
    n1, one = we(x[1], W, step, measures=NAMES, **KW)
    n257, many = we(np.tile(x[1], (257, 1)), W, step, measures=NAMES, **KW)
    assert n1 == n257 == nwin
    for name in NAMES:
        assert one[name].shape == (nwin,) and same_bits(one[name], F[name][1]), name
        assert many[name].shape == (257, nwin)
        assert np.array_equal(bits(many[name]), np.broadcast_to(bits(F[name][1]), (257, nwin))), name


@pytest.mark.parametrize("W,step", [(250, 125), (WIDE + 88, 250)])
def test_non_finite_samples_stay_in_their_windows(we, W, step):
    x = long_signal()
    nwin, clean = device_all(W, step)
    y = np.array(x)
    y[1, 701] = np.nan                                       # (overlapping windows hold it)
    y[2, 1300] = -np.inf
    y[0, 0] = np.inf                                         # a window's first sample: its pivot
    n2, F = we(producer(y, 409, -1), W, step, measures=NAMES, **KW)
    k = np.arange(nwin)
    hit = np.zeros((3, nwin), dtype=bool)
    hit[0] = k == 0
    hit[1] = (k * step <= 701) & (701 < k * step + W)
    hit[2] = (k * step <= 1300) & (1300 < k * step + W)
    assert hit[1].sum() >= 2 and hit[2].sum() >= 2 and n2 == nwin
    for name in NAMES:
        assert np.array_equal(np.isnan(F[name]), hit), name
        assert np.array_equal(bits(F[name])[~hit], bits(clean[name])[~hit]), name


def test_more_windows_than_a_grid_dimension(we):
    rng = np.random.default_rng(43)
    x = (np.cumsum(rng.standard_normal((1, 70000)), axis=-1) * 0.3 + rng.standard_normal((1, 70000)) + 100.0)
    picks = np.unique(np.concatenate([np.arange(0, 69993, 1747), [65534, 65535, 65536, 69992]]))
    ref = {name: np.array([window_entropies(x[:, k:k + 8], 8, 1, m=2, r=0.5, order=3, margins=True)[name][0, 0]
                           for k in picks]) for name in NAMES + ("margin",)}
    assert float(ref["margin"].min()) > MARGIN
    nwin, F = we(x, 8, 1, measures=NAMES, m=2, r=0.5, order=3)
    assert nwin == 69993 > 65535 and F["sample"].shape == (1, nwin)
    got = {name: F[name][0, picks] for name in NAMES}
    assert_sample(got, ref, "70000")
    assert float(np.max(np.abs(got["permutation"] - ref["permutation"]))) < 1e-12
    assert ref["sample_b"].max() > 0


def test_kinds_shapes_and_counts(we):
    import ctypes
    import torch
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.osz_window_count.restype, lib.osz_window_count.argtypes = _lib.SIGNATURES["osz_window_count"]
    x = long_signal()
    for W, step in ((250, 125), (67, 200), (2000, 1), (1999, 1)):
        nwin, F = we(x, W, step, measures="permutation")
        assert nwin == lib.osz_window_count(2000, W, step) and isinstance(F, np.ndarray) and F.shape == (3, nwin)
        nwin, F = we(torch.from_numpy(np.array(x[0])).cuda(), W, step, measures=("sample_b", "permutation"))
        assert nwin == lib.osz_window_count(2000, W, step) and list(F) == ["sample_b", "permutation"]
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (nwin,) for v in F.values())
    with pytest.raises(ValueError, match="fewer than one window"):
        we(torch.from_numpy(np.array(x)).cuda(), 2001)
    # a constant window: every pair matches, one pattern
    nwin, F = we(np.full((2, 300), 7.5), 100, measures=NAMES)
    assert nwin == 3 and np.all(F["sample"] == 0) and np.all(F["permutation"] == 0)
    assert np.all(F["sample_a"] == 98 * 97 / 2) and np.all(F["sample_b"] == 98 * 97 / 2)

    # a source that says it is longer than it is: found when the stream ends
    def short():
        yield torch.zeros((3, 90), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="before one window"):
        we(producer(short, chunksize=50, axis=-1, shape=(3, 5000)), 100)
