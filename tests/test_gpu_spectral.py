"""GPU tests of window_spectral (K18) against tests/test_spectral_host.py's restatement.

The reduction alone (``dev.spectral_features`` on rows made here: positive, six decades, seeded)
against ``spectral_stats_of`` in long double, with u = 2^-53 and n the bins of the range, relative
to the reference value: ``total`` and ``band`` (n + 2) u -- all terms are positive, so any
summation order is within (n - 1) u; ``relative`` and ``centroid`` (2 n + 4) u; ``spread``,
``entropy`` and ``flatness`` the larger of 8 n u and 16 times the error of the float64 NumPy
evaluation of the same definition against the long-double one, measured on the test's own rows
(a different summation order, a device log a few ulp from libm's: measured against the reference,
never against the device); ``peak`` exact; ``edge`` by the two-sided rule ``edge_is_acceptable``
with eps = 2 n u.  Then that a row's bits are its own, and the public function against
``window_spectral_stats`` to RTOL = 1e-9 (the suite's spectra tolerance) of each feature's largest
value, ``peak`` by P_ref[k_got] >= max P_ref (1 - 1e-9) and ``edge`` by the two-sided rule with
eps = 1e-9; different cuts of one stream agree to SAME = 1e-12."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_gpu_features import Reused
from test_spectral_host import (CONTINUOUS, NAMES, edge_is_acceptable, spectral_stats_of, walk,
                                window_spectral_stats)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RTOL = 1e-9
SAME = 1e-12
DF = 0.37
EDGES = (0.5, 0.9, 0.95, 1.0)
# the range 1 .. nfreq - 2 of nfft holds nfft // 2 - 1 bins: both sides of every instance boundary,
# and three tiles with a partial last one
BOUNDARY = tuple(2 * (n + 1) for n in (_lib.WS_WAVE, _lib.WS_WAVE + 1, _lib.WS_LDS, _lib.WS_LDS + 1,
                                       2 * _lib.WS_LDS + 1000))
NFFTS = (8, 9, 64, 250, 1000, 4096) + BOUNDARY


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd import _device
    return _device


def plan(nfft):
    """(nfreq, k0, k1, five bands of bins, two of them overlapping the others)."""
    nfreq = nfft // 2 + 1
    k0, k1 = 1, nfreq - 2
    n = k1 - k0 + 1
    a, b, c, d = k0, k0 + max(1, n // 4), k0 + max(2, n // 2), k1 + 1
    return nfreq, k0, k1, ((a, b), (b, c), (c, d), (a, d), (b, d))


@lru_cache(maxsize=None)
def rows(nfft, tied=False):
    """3 x 3 rows of nfreq positive bins spanning six decades (quantised to whole decades when
    ``tied``).  Read-only."""
    e = np.random.default_rng(nfft).uniform(-3, 3, (3, 3, nfft // 2 + 1))
    P = 10.0 ** (np.round(e) if tied else e)
    P.setflags(write=False)
    return P


def planes(out, names, nb, ne):
    """name -> (nch, nseg), or (nb | ne, nch, nseg), from the (planes, nch, room) result."""
    res, p = {}, 0
    for name in NAMES:
        if name not in names:
            continue
        w = nb if name in ("band", "relative") else ne if name == "edge" else 1
        res[name] = out[p] if w == 1 and name not in ("band", "relative", "edge") else out[p:p + w]
        p += w
    assert p == out.shape[0]
    return res


def reduce(dev, P, k0, k1, bands, edges=EDGES, names=NAMES, normalize=True, win0=0, room=None):
    """name -> ndarray (nch, nseg) / (nb | ne, nch, nseg) of dev.spectral_features on P (nseg, nch, nfreq)."""
    import torch
    nseg, nch, _ = P.shape
    mask = dev.spectral_mask(names)
    npl = dev.spectral_planes(mask, len(bands), len(edges))
    out = torch.full((npl, nch, room or win0 + nseg), -7.0, dtype=torch.float64, device="cuda")
    got = dev.spectral_features(torch.from_numpy(np.array(P)).cuda(), k0, k1, DF, bands, edges,
                                normalize, mask, out, win0)
    assert got == nseg
    out = out.cpu().numpy()
    assert np.all(out[:, :, :win0] == -7.0) and np.all(out[:, :, win0 + nseg:] == -7.0)
    return planes(out[:, :, win0:win0 + nseg], names, len(bands), len(edges))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rowwise(v):
    """The restatement's (..., nseg, nch) as the device's (..., nch, nseg)."""
    return np.swapaxes(v, -1, -2)


def assert_reduction(got, P, k0, k1, bands, edges=EDGES):
    n = k1 - k0 + 1
    ref = spectral_stats_of(P, k0, k1, DF, bands, edges)
    f64 = spectral_stats_of(P, k0, k1, DF, bands, edges, dtype=np.float64)
    f = np.arange(k1 + 1) * np.float64(DF)
    for name in CONTINUOUS:
        r, g = rowwise(ref[name]), got[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name in ("total", "band"):
            tol = (n + 2) * U
        elif name in ("relative", "centroid"):
            tol = (2 * n + 4) * U
        else:
            tol = max(8 * n * U, 16 * float(np.max(np.abs(f64[name] - ref[name]) / np.abs(ref[name]))))
        err = np.abs(g - r) / np.abs(r)
        print(name, n, "err", float(err.max()), "tol", tol)
        assert np.all(err <= tol), (name, n, float(err.max()), tol)
    assert np.array_equal(bits(got["peak"]), bits(rowwise(f[ref["peak_bin"]]))), "peak"
    for j, p in enumerate(edges):
        k = np.searchsorted(f, got["edge"][j])
        assert np.array_equal(bits(f[np.minimum(k, k1)]), bits(got["edge"][j])), ("edge is not a bin", p)
        ok = edge_is_acceptable(P, k0, k1, rowwise(k), p, 2 * n * U)
        assert np.all(ok), ("edge", p, n, rowwise(k)[~ok], ref["edge_bin"][j][~ok])


@pytest.mark.parametrize("nfft", NFFTS)
def test_the_reduction_against_the_restatement(dev, nfft):
    nfreq, k0, k1, bands = plan(nfft)
    for tied in (False, True):
        P = rows(nfft, tied)
        got = reduce(dev, P, k0, k1, bands)
        assert_reduction(got, P, k0, k1, bands)
    if nfft in (9, 250):                                         # the whole axis, the entropy as it is
        P = rows(nfft)
        got = reduce(dev, P, 0, nfreq - 1, ((0, nfreq),), normalize=False)
        ref = spectral_stats_of(P, 0, nfreq - 1, DF, normalize=False)
        assert np.all(np.abs(got["entropy"] - rowwise(ref["entropy"])) <= 8 * nfreq * U * ref["entropy"].max())
        one = reduce(dev, P, 3, 3, ((3, 4),), names=("total", "entropy", "flatness", "spread", "edge", "peak"))
        assert np.all(one["entropy"] == 0) and np.all(one["flatness"] == 1)
        assert np.all(one["spread"] <= 4 * U * 3 * DF)           # (f P / P is f to an ulp)
        assert np.all(one["edge"] == 3 * DF) and np.all(one["peak"] == 3 * DF)
        assert np.array_equal(bits(one["total"]), bits(rowwise(DF * P[..., 3])))


@pytest.mark.parametrize("nfft", (8, 250, 1000) + BOUNDARY)
def test_a_row_depends_on_itself_only(dev, nfft):
    nfreq, k0, k1, bands = plan(nfft)
    P = rows(nfft)
    base = reduce(dev, P, k0, k1, bands)
    # the same rows elsewhere in a launch of another size, with another win0, beside a NaN row and
    # a row of zeros
    big = 10.0 ** np.random.default_rng(1).uniform(-3, 3, (7, 4, nfreq))
    where = [(5, 2), (0, 0), (6, 3), (2, 1), (3, 3), (1, 0), (4, 2), (0, 3), (6, 0)]
    for (s, c), row in zip(where, P.reshape(9, nfreq)):
        big[s, c] = row
    big[1, 1, k0 + (k1 - k0) // 2] = np.nan
    big[2, 2, k0:k1 + 1] = 0.0
    big[2, 2, 0] = 5.0                                           # (outside the range)
    big[3, 0, 0] = big[3, 0, nfreq - 1] = np.nan                 # (outside the range: an ordinary row)
    got = reduce(dev, big, k0, k1, bands, win0=11, room=40)
    for name in NAMES:
        g = np.stack([got[name][..., c, s] for s, c in where], axis=-1)
        # (row i of P: segment i // 3, channel i % 3)
        mine = np.stack([base[name][..., i % 3, i // 3] for i in range(9)], axis=-1)
        assert np.array_equal(bits(g), bits(mine)), name
        assert np.all(np.isnan(got[name][..., 1, 1])), name
        if name in ("total", "band"):
            assert np.all(got[name][..., 2, 2] == 0), name
        else:
            assert np.all(np.isnan(got[name][..., 2, 2])), name
        assert np.all(np.isfinite(got[name][..., 0, 3])), name
    # each feature alone
    for name in NAMES:
        alone = reduce(dev, P, k0, k1, bands, names=(name,))
        assert np.array_equal(bits(alone[name]), bits(base[name])), name
    # fewer bands and edges, in another order: the planes that remain
    few = reduce(dev, P, k0, k1, (bands[4], bands[1]), edges=(0.95, 0.5), names=("relative", "edge", "flatness"))
    assert np.array_equal(bits(few["relative"]), bits(base["relative"][[4, 1]]))
    assert np.array_equal(bits(few["edge"]), bits(base["edge"][[2, 0]]))
    assert np.array_equal(bits(few["flatness"]), bits(base["flatness"]))


def test_more_rows_than_a_grid_dimension(dev):
    nfreq, k0, k1, bands = plan(8)
    P = 10.0 ** np.random.default_rng(3).uniform(-3, 3, (70000, 1, nfreq))
    got = reduce(dev, P, k0, k1, bands)
    assert got["total"].shape == (1, 70000)
    assert_reduction(got, P, k0, k1, bands)
    first = reduce(dev, P[:9], k0, k1, bands)
    last = reduce(dev, P[-9:], k0, k1, bands)
    for name in NAMES:
        assert np.array_equal(bits(got[name][..., :9]), bits(first[name])), name
        assert np.array_equal(bits(got[name][..., -9:]), bits(last[name])), name


def test_the_binding_refuses_what_the_kernel_cannot_take(dev):
    import torch
    P = torch.ones((2, 3, 33), dtype=torch.float64, device="cuda")
    out = torch.empty((1, 3, 2), dtype=torch.float64, device="cuda")
    mask = dev.spectral_mask(("total",))
    for k0, k1 in ((-1, 5), (5, 4), (0, 33)):
        with pytest.raises(ValueError, match="bin range"):
            dev.spectral_features(P, k0, k1, DF, (), (), True, mask, out)
    with pytest.raises(ValueError, match="out"):
        dev.spectral_features(P, 1, 31, DF, (), (), True, mask, out[:, :, :1])
    with pytest.raises(ValueError, match="mask"):
        dev.spectral_features(P, 1, 31, DF, (), (), True, 0, out)
    bmask, emask = dev.spectral_mask(("band",)), dev.spectral_mask(("edge",))
    for bands in (((0, 4),), ((4, 4),), ((30, 33),)):            # below the range, empty, above it
        with pytest.raises(ValueError, match="band 0"):
            dev.spectral_features(P, 1, 31, DF, bands, (), True, bmask, out)
    for edges in ((0.0,), (1.5,)):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            dev.spectral_features(P, 1, 31, DF, (), edges, True, emask, out)
    many = torch.empty((17, 3, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="17 bands"):
        dev.spectral_features(P, 1, 31, DF, ((1, 2),) * 17, (), True, bmask, many)


# ---- the public function ----

FS = 250.0
BANDS = ((0.5, 4), (4, 8), (8, 13), (13, 30), (4, 30))
EDGE = (0.5, 0.95)
SHAPES = ((64, 64), (250, 125), (1000, 333), (4096, 4096))


@pytest.fixture(scope="module")
def ws(dev):
    from openseize_amd.features import window_spectral
    return window_spectral


@lru_cache(maxsize=None)
def stream():
    x = walk()
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def reference(W, step, detrend="constant", scaling="density"):
    return window_spectral_stats(stream(), FS, W, step, BANDS, EDGE, detrend=detrend, scaling=scaling)


@lru_cache(maxsize=None)
def device_all(W, step, detrend="constant", scaling="density"):
    from openseize_amd.features import window_spectral
    return window_spectral(stream(), FS, W, step, features=NAMES, bands=BANDS, edge=EDGE, detrend=detrend,
                           scaling=scaling)


def host(v):
    import torch
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def assert_function(F, ref, skip=None, tol=RTOL, against=None):
    """F against the restatement's ``ref``; the windows ``skip`` (C, nwin) left out.  With
    ``against`` (another result of the device) the continuous features are compared with it."""
    keep = slice(None) if skip is None else ~skip
    for name in CONTINUOUS:
        g, r = host(F[name]), host((ref if against is None else against)[name])
        assert g.shape == r.shape and g.dtype == np.float64, (name, g.shape, r.shape)
        scale = np.nanmax(np.abs(ref[name]))
        err = np.abs(g - r)[..., keep]
        print(name, "err", float(err.max() / scale), "tol", tol)
        assert np.all(err <= tol * scale), (name, float(err.max() / scale))


def assert_bins(F, ref, W, skip=None):
    P, k0, k1 = ref["P"], ref["k0"], ref["k1"]
    keep = np.ones(P.shape[:2], dtype=bool) if skip is None else ~skip
    df = FS / W
    kp = np.rint(np.nan_to_num(host(F["peak"])) / df).astype(np.int64)
    assert np.array_equal(bits((kp * df)[keep]), bits(host(F["peak"])[keep])), "peak is not a bin"
    R = P[..., k0:k1 + 1]
    kpc = np.clip(kp, k0, k1)
    at = np.take_along_axis(P, kpc[..., None], axis=-1)[..., 0]
    assert np.all(((kp >= k0) & (kp <= k1) & (at >= R.max(axis=-1) * (1 - 1e-9)))[keep]), "peak"
    for j, p in enumerate(EDGE):
        ke = np.rint(np.nan_to_num(host(F["edge"])[j]) / df).astype(np.int64)
        assert np.array_equal(bits((ke * df)[keep]), bits(host(F["edge"])[j][keep])), "edge is not a bin"
        assert np.all(edge_is_acceptable(P, k0, k1, np.where(keep, ke, ref["edge_bin"][j]), p, 1e-9)[keep]), ("edge", p)


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("detrend", ["constant", "linear"])
@pytest.mark.parametrize("W,step", SHAPES)
def test_the_function_against_the_restatement(ws, W, step, detrend, scaling):
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.osz_window_count.restype, lib.osz_window_count.argtypes = _lib.SIGNATURES["osz_window_count"]
    nwin, F = device_all(W, step, detrend, scaling)
    assert nwin == lib.osz_window_count(12288, W, step) == (12288 - W) // step + 1
    assert list(F) == list(NAMES) and all(isinstance(v, np.ndarray) for v in F.values())
    ref = reference(W, step, detrend, scaling)
    assert_function(F, ref)
    assert_bins(F, ref, W)


@pytest.mark.parametrize("W,step", SHAPES)
def test_cuts_of_one_stream_agree(ws, W, step):
    import torch
    x = stream()
    nwin, F = device_all(W, step)
    ref = reference(W, step)
    xd = torch.from_numpy(np.array(x)).cuda()
    kw = dict(features=NAMES, bands=BANDS, edge=EDGE)
    cuts = {"1000": lambda: ws(x, FS, W, step, chunksize=1000, **kw),
            "4097": lambda: ws(x, FS, W, step, chunksize=4097, **kw),
            "cuda": lambda: ws(xd, FS, W, step, **kw),
            "axis0": lambda: ws(np.ascontiguousarray(x.T), FS, W, step, axis=0, **kw),
            "reused": lambda: ws(Reused(xd, 4099, -1), FS, W, step, **kw),
            "producer": lambda: ws(producer(np.array(x), 777, -1), FS, W, step, **kw)}
    for how, call in cuts.items():
        n2, G = call()
        assert n2 == nwin, how
        if how in ("cuda", "reused"):
            assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in G.values()), how
        else:
            assert all(isinstance(v, np.ndarray) for v in G.values()), how
        if how == "axis0":
            G = {name: np.swapaxes(v, -1, -2) for name, v in G.items()}
        print(how)
        assert_function(G, ref, tol=SAME, against=F)
        assert_bins(G, ref, W)


def test_a_nan_sample_takes_its_windows(ws):
    W, step = 250, 125
    nwin, clean = device_all(W, step)
    ref = reference(W, step)
    y = np.array(stream())
    y[1, 7013] = np.nan
    y[2, 11000:] = np.nan
    k = np.arange(nwin)
    hit = np.zeros((3, nwin), dtype=bool)
    hit[1] = (k * step <= 7013) & (7013 < k * step + W)
    hit[2] = k * step + W > 11000
    assert hit[1].sum() == 2 and hit[2].sum() > 2
    n2, F = ws(producer(y, 4099, -1), FS, W, step, features=NAMES, bands=BANDS, edge=EDGE)
    assert n2 == nwin
    for name in NAMES:
        assert np.array_equal(np.isnan(F[name]), np.broadcast_to(hit, F[name].shape)), name
    assert_function(F, ref, skip=hit, tol=SAME, against=clean)
    assert_bins(F, ref, W, skip=hit)
    with pytest.raises(ValueError, match="infs or NaNs"):
        ws(y, FS, W, step, detrend="linear")


def test_kinds_shapes_and_order(ws):
    import torch
    x = stream()
    W, step = 250, 125
    nwin, F = device_all(W, step)
    assert F["total"].shape == (3, nwin) and F["band"].shape == (5, 3, nwin) == F["relative"].shape
    assert F["edge"].shape == (2, 3, nwin) and F["flatness"].shape == (3, nwin)
    # one name: an array; it is its entry of the whole, bit for bit
    for name in NAMES:
        n2, one = ws(x, FS, W, step, features=name, bands=BANDS, edge=EDGE)
        assert n2 == nwin and isinstance(one, np.ndarray) and np.array_equal(bits(one), bits(F[name])), name
    # the order asked; a single pair and a single fraction have no leading axis
    n2, G = ws(x, FS, W, step, features=("edge", "relative", "total"), bands=(8, 13), edge=0.95)
    assert list(G) == ["edge", "relative", "total"]
    assert G["edge"].shape == (3, nwin) == G["relative"].shape
    assert np.array_equal(bits(G["edge"]), bits(F["edge"][1])) and np.array_equal(bits(G["relative"]),
                                                                                 bits(F["relative"][2]))
    n2, G = ws(x, FS, W, step, features=["band"], bands=[(8, 13)])
    assert list(G) == ["band"] and G["band"].shape == (1, 3, nwin)
    # the defaults; one-dimensional data; CUDA in, CUDA out
    n2, G = ws(x[0], FS, W)
    assert n2 == 12288 // W and list(G) == ["total", "edge", "entropy"]
    assert all(isinstance(v, np.ndarray) and v.shape == (n2,) for v in G.values())
    n2, G = ws(torch.from_numpy(np.array(x[0])).cuda(), FS, W, step, features=("peak", "edge"), edge=EDGE)
    assert n2 == nwin and G["peak"].is_cuda and tuple(G["peak"].shape) == (nwin,)
    assert tuple(G["edge"].shape) == (2, nwin)
    # a range: the features of fmin .. fmax
    n2, G = ws(x, FS, W, step, features=("total", "entropy"), fmin=4, fmax=40)
    M = window_spectral_stats(x, FS, W, step, fmin=4, fmax=40)
    assert (M["k0"], M["k1"]) == (4, 40)
    for name in G:
        assert np.all(np.abs(G[name] - M[name]) <= RTOL * np.abs(M[name]).max()), name
    n2, raw = ws(x, FS, W, step, features="entropy", normalize=False)
    assert np.all(np.abs(raw - F["entropy"] * np.log(125)) <= 1e-12 * np.log(125))
    with pytest.raises(ValueError, match="larger than winsize"):
        ws(x, FS, W, W + 1)
    with pytest.raises(ValueError, match="fewer than one window"):
        ws(torch.from_numpy(np.array(x)).cuda(), FS, 12289)

    # a source that says it is longer than it is: found when the stream ends
    def short():
        yield torch.zeros((3, 90), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="before one window"):
        ws(producer(short, chunksize=50, axis=-1, shape=(3, 5000)), FS, 100)
