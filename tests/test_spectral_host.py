"""CPU-only tests of window_spectral (K18): ``window_spectral_stats``, the NumPy restatement that
tests/test_gpu_spectral.py compares the device against -- segments by slicing, scipy.signal.detrend,
the window, numpy.fft.rfft, the scale and the one-sided doubling, then the nine definitions in
numpy.longdouble (``spectral_stats_of`` is that second half alone, on given rows) -- pinned here
against scipy.signal.spectrogram, scipy.stats.entropy, numpy.searchsorted on a cumsum,
scipy.stats.gmean and numpy.average, on closed forms and on the rules for NaN and for rows of
zeros; the argument errors (raised with no GPU and before the stream is touched), the bin rule of
the bands, the C ABI of the entry point against the header, and the register report of
csrc/windowspec.hip (no scratch in any kernel)."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal as sps
import scipy.stats

from openseize_amd import _lib, features
from openseize_amd.features import spectral
from openseize_amd.features.spectral import window_spectral

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("total", "band", "relative", "peak", "centroid", "spread", "edge", "entropy", "flatness")
CONTINUOUS = ("total", "band", "relative", "centroid", "spread", "entropy", "flatness")


def periodograms(x, fs, W, step, window="hann", detrend="constant", scaling="density"):
    """(C, nwin, W // 2 + 1): the one-sided periodogram of every window of W samples, step apart."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    win = np.lib.stride_tricks.sliding_window_view(x, W, axis=-1)[:, ::step]
    coeffs = sps.get_window(window, W)
    norm = 1 / (fs * np.sum(coeffs ** 2)) if scaling == "density" else 1 / np.sum(coeffs) ** 2
    X = np.fft.rfft(sps.detrend(win, type=detrend, axis=-1) * coeffs, axis=-1)
    P = (X.real ** 2 + X.imag ** 2) * norm
    P[..., 1:(W // 2 if W % 2 == 0 else W // 2 + 1)] *= 2          # all but DC and, for even W, Nyquist
    return P


def spectral_stats_of(P, k0, k1, df, bands=(), edges=(), normalize=True, dtype=np.longdouble):
    """The nine definitions on the bins k0 .. k1 (inclusive) of the rows P (..., nfreq), evaluated
    in ``dtype`` and returned as float64: name -> (...), with a leading axis of len(bands) for band
    and relative ([b0, b1) pairs of bins) and of len(edges) for edge.  f_k = k df is one float64
    multiply.  A row with a NaN in the range is NaN everywhere; a row that sums to 0 has total and
    band 0 and NaN elsewhere.  "peak_bin" and "edge_bin" are the bins themselves (-1: none)."""
    P = np.asarray(P, dtype=np.float64)
    R = P[..., k0:k1 + 1]
    n = R.shape[-1]
    wild = np.isnan(R).any(axis=-1)
    R = np.where(wild[..., None], 0.0, R).astype(dtype)
    f64 = np.arange(k0, k1 + 1) * np.float64(df)
    f = f64.astype(dtype)
    df = dtype(df)
    S = R.sum(axis=-1)
    void = wild | (S == 0)
    Ssafe = np.where(void, 1, S)
    out = {}
    with np.errstate(all="ignore"):
        out["total"] = df * S
        band = [df * R[..., b0 - k0:b1 - k0].sum(axis=-1) for b0, b1 in bands]
        out["band"] = np.stack(band) if band else np.zeros((0,) + S.shape, dtype)
        out["relative"] = out["band"] / (df * Ssafe)
        kpk = np.argmax(R, axis=-1)                              # the first of the largest
        out["peak"] = f64[kpk].astype(dtype)
        c = (f * R).sum(axis=-1) / Ssafe
        out["centroid"] = c
        out["spread"] = np.sqrt((((f - c[..., None]) ** 2) * R).sum(axis=-1) / Ssafe)
        cum = np.cumsum(R, axis=-1)
        # (the total of the same running sum: p = 1 names the bin that reaches it)
        kedge = [np.argmax(cum >= dtype(p) * cum[..., -1:], axis=-1) for p in edges]
        out["edge"] = np.stack([f64[k].astype(dtype) for k in kedge]) if edges else np.zeros((0,) + S.shape, dtype)
        pk = R / Ssafe[..., None]
        lp = np.log(np.where(pk > 0, pk, 1))
        H = -(pk * lp).sum(axis=-1)
        if normalize:
            H = H / np.log(dtype(n)) if n > 1 else H * 0
        out["entropy"] = H
        out["flatness"] = np.where((pk == 0).any(axis=-1), 0, n * np.exp(lp.sum(axis=-1) / n))
    res = {}
    for name in NAMES:
        v = np.array(out[name], dtype=np.float64)
        v[..., wild if name in ("total", "band") else void] = np.nan
        res[name] = v
    res["peak_bin"] = np.where(void, -1, k0 + kpk)
    res["edge_bin"] = np.stack([np.where(void, -1, k0 + k) for k in kedge]) if edges else np.zeros((0,) + S.shape, int)
    return res


def bins_of(fs, W, fmin=None, fmax=None, bands=()):
    """(k0, k1, [b0, b1) pairs) by the masks of the definitions: fmin <= f <= fmax (bin 1 .. W // 2 by
    default), lo <= f < hi."""
    freqs = np.fft.rfftfreq(W, 1 / fs)
    inside = (freqs >= (freqs[1] if fmin is None else fmin)) & (freqs <= (freqs[-1] if fmax is None else fmax))
    ks = np.flatnonzero(inside)
    pairs = []
    for lo, hi in bands:
        kb = np.flatnonzero((freqs >= lo) & (freqs < hi))
        pairs.append((int(kb[0]), int(kb[-1]) + 1))
    return int(ks[0]), int(ks[-1]), pairs


def window_spectral_stats(x, fs, W, step, bands=(), edges=(), fmin=None, fmax=None, window="hann",
                          detrend="constant", scaling="density", normalize=True):
    """The definitions for x (C, N): name -> (C, nwin), (len(bands), C, nwin) for band and relative,
    (len(edges), C, nwin) for edge; "P" the periodograms (C, nwin, nfreq), "k0", "k1" the range."""
    P = periodograms(x, fs, W, step, window, detrend, scaling)
    k0, k1, pairs = bins_of(fs, W, fmin, fmax, bands)
    M = spectral_stats_of(P, k0, k1, fs / W, pairs, tuple(edges), normalize)
    M.update(P=P, k0=k0, k1=k1)
    return M


def edge_is_acceptable(P, k0, k1, k, p, eps):
    """The two-sided rule for the edge bins k (...) of the rows P (..., nfreq): with the long-double
    cumulative sums of the range, cum[k] >= p S (1 - eps) and cum[k - 1] < p S (1 + eps)."""
    R = np.asarray(P, dtype=np.float64)[..., k0:k1 + 1].astype(np.longdouble)
    cum = np.cumsum(R, axis=-1)
    i = np.asarray(k, dtype=np.int64) - k0
    inside = (i >= 0) & (i < R.shape[-1])
    ic = np.clip(i, 0, R.shape[-1] - 1)
    at = np.take_along_axis(cum, ic[..., None], axis=-1)[..., 0]
    below = np.take_along_axis(cum, np.maximum(ic - 1, 0)[..., None], axis=-1)[..., 0]
    thr = np.longdouble(p) * cum[..., -1]
    return inside & (at >= thr * (1 - eps)) & ((ic == 0) | (below < thr * (1 + eps)))


def walk(seed=18, shape=(3, 12288)):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal(shape), axis=-1) * 0.3 + rng.standard_normal(shape)


def test_names_are_public():
    assert features.window_spectral is window_spectral
    assert features.WINDOW_SPECTRAL == spectral.WINDOW_SPECTRAL == NAMES == tuple(_lib.WINDOW_SPECTRAL)
    assert list(_lib.WINDOW_SPECTRAL.values()) == list(range(9))
    assert (_lib.WS_BANDS_MOST, _lib.WS_EDGES_MOST) == (16, 16) and _lib.WS_WAVE < _lib.WS_LDS
    doc = window_spectral.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name
    assert "rectangle" in doc and "Simpson" in doc and "bit-reproducible per row" in doc and "1e-12" in doc


@pytest.mark.parametrize("detrend", ["constant", "linear"])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("W,step", [(64, 64), (250, 125), (1000, 333), (9, 4)])
def test_periodograms_are_scipy_spectrogram(W, step, detrend, scaling):
    x, fs = walk()[:, :4000], 250.0
    P = periodograms(x, fs, W, step, "hann", detrend, scaling)
    f, _, S = sps.spectrogram(x, fs, window="hann", nperseg=W, noverlap=W - step, detrend=detrend, scaling=scaling,
                              mode="psd", axis=-1)
    assert np.array_equal(f, np.fft.rfftfreq(W, 1 / fs))
    S = np.moveaxis(S, -1, 1)                                    # (C, nseg, nfreq)
    assert P.shape == S.shape == (3, (4000 - W) // step + 1, W // 2 + 1)
    assert np.max(np.abs(P - S)) <= 1e-12 * np.max(S)


def test_features_against_independent_routes():
    rng = np.random.default_rng(5)
    P = 10.0 ** rng.uniform(-3, 3, (4, 5, 129))
    k0, k1, df = 3, 100, 0.37
    edges = (0.1, 0.5, 0.9, 0.95, 1.0)
    bands = ((3, 10), (10, 40), (30, 101))
    M = spectral_stats_of(P, k0, k1, df, bands, edges)
    R, n = P[..., k0:k1 + 1], k1 - k0 + 1
    f = np.arange(k0, k1 + 1) * df
    rel = 1e-13
    assert np.allclose(M["entropy"], scipy.stats.entropy(R, axis=-1) / np.log(n), rtol=rel, atol=0)
    raw = spectral_stats_of(P, k0, k1, df, normalize=False)["entropy"]
    assert np.allclose(raw, scipy.stats.entropy(R, axis=-1), rtol=rel, atol=0)
    assert np.allclose(M["flatness"], scipy.stats.gmean(R, axis=-1) / R.mean(axis=-1), rtol=rel, atol=0)
    assert np.allclose(M["centroid"], np.average(np.broadcast_to(f, R.shape), weights=R, axis=-1), rtol=rel, atol=0)
    assert np.allclose(M["total"], df * R.sum(axis=-1), rtol=rel, atol=0)
    cen = M["centroid"][..., None]
    assert np.allclose(M["spread"], np.sqrt(np.average((f - cen) ** 2, weights=R, axis=-1)), rtol=rel, atol=0)
    assert np.array_equal(M["peak"], f[np.argmax(R, axis=-1)])
    cum = np.cumsum(R.astype(np.longdouble), axis=-1)
    for j, p in enumerate(edges):
        for idx in np.ndindex(R.shape[:-1]):
            k = int(np.searchsorted(cum[idx], np.longdouble(p) * cum[idx][-1], side="left"))
            assert M["edge_bin"][j][idx] == k0 + k and M["edge"][j][idx] == f[k], (p, idx)
            assert edge_is_acceptable(P[idx], k0, k1, k0 + k, p, 0.0)
            assert k == 0 or not edge_is_acceptable(P[idx], k0, k1, k0 + k - 1, p, 0.0)
    assert np.all(M["edge_bin"][-1] == k1)                       # p = 1: positive bins, the last one
    for j, (b0, b1) in enumerate(bands):
        assert np.allclose(M["band"][j], df * P[..., b0:b1].sum(axis=-1), rtol=rel, atol=0)
        assert np.allclose(M["relative"][j], P[..., b0:b1].sum(axis=-1) / R.sum(axis=-1), rtol=rel, atol=0)
    assert np.allclose(M["relative"][0] + M["relative"][1] + M["relative"][2]
                       - df * P[..., 30:40].sum(axis=-1) / M["total"], 1.0, rtol=1e-12)


def test_closed_forms():
    df = 0.5
    for n in (1, 2, 7, 64, 101):
        k0, k1 = 2, n + 1
        flat = np.full((1, n + 4), 3.25)
        M = spectral_stats_of(flat, k0, k1, df, ((k0, k1 + 1),), (0.5, 1.0))
        assert M["entropy"][0] == (1.0 if n > 1 else 0.0) and abs(M["flatness"][0] - 1) < 1e-15
        assert M["edge_bin"][0][0] == k0 + (n + 1) // 2 - 1      # the middle bin: the first to reach half
        assert M["edge_bin"][1][0] == k1 and M["relative"][0][0] == 1 and M["peak_bin"][0] == k0
        assert M["total"][0] == df * 3.25 * n and abs(M["centroid"][0] - df * (k0 + k1) / 2) < 1e-13
        one = np.zeros((1, n + 4))
        one[0, k0 + n // 2] = 7.0
        M = spectral_stats_of(one, k0, k1, df, (), (0.01, 0.5, 1.0))
        fk = (k0 + n // 2) * df
        assert M["entropy"][0] == 0 and M["spread"][0] == 0 and M["peak"][0] == fk and M["centroid"][0] == fk
        assert np.all(M["edge"][:, 0] == fk) and M["flatness"][0] == (0.0 if n > 1 else 1.0)
        assert spectral_stats_of(one, k0, k1, df, normalize=False)["entropy"][0] == 0
    # ties go to the lowest bin
    tie = np.array([[1.0, 5.0, 2.0, 5.0, 5.0, 0.5]])
    assert spectral_stats_of(tie, 0, 5, 1.0)["peak_bin"][0] == 1
    assert spectral_stats_of(tie, 2, 5, 1.0)["peak_bin"][0] == 3


def test_a_sine_at_a_bin_frequency():
    fs, W = 256.0, 256
    t = np.arange(4 * W) / fs
    x = np.sin(2 * np.pi * 10.0 * t) + 1e-3 * np.random.default_rng(2).standard_normal(t.shape)
    bands = ((1, 4), (4, 8), (8, 13), (13, 30))
    M = window_spectral_stats(x, fs, W, W // 2, bands, (0.5, 0.95))
    assert M["peak"].shape == (1, 7) and np.all(M["peak"] == 10.0)
    assert np.all(M["relative"][2] > 0.99) and np.all(M["relative"][[0, 1, 3]] < 0.01)
    assert np.all(np.abs(M["centroid"] - 10.0) < 0.1) and np.all(M["edge"][0] == 10.0)
    assert np.all(M["entropy"] < 0.3) and np.all(M["flatness"] < 1e-3)


def test_nan_and_zero_rows():
    rng = np.random.default_rng(7)
    P = 10.0 ** rng.uniform(-3, 3, (5, 40))
    bands, edges = ((2, 9), (9, 30)), (0.5, 1.0)
    clean = spectral_stats_of(P, 2, 30, 1.0, bands, edges)
    Q = P.copy()
    Q[1, 17] = np.nan                                            # in the range
    Q[2, 1] = np.nan                                             # outside it: nothing happens
    Q[3, 35] = np.nan
    Q[4, 2:31] = 0.0
    M = spectral_stats_of(Q, 2, 30, 1.0, bands, edges)
    for name in NAMES:
        assert np.all(np.isnan(M[name][..., 1])), name
        assert np.array_equal(M[name][..., [0, 2, 3]], clean[name][..., [0, 2, 3]]), name
        if name in ("total", "band"):
            assert np.all(M[name][..., 4] == 0), name
        else:
            assert np.all(np.isnan(M[name][..., 4])), name
    assert M["peak_bin"][1] == -1 and np.all(M["edge_bin"][:, 4] == -1)
    # a zero bin: flatness 0, the entropy skips it
    Z = P.copy()
    Z[0, 10] = 0.0
    M = spectral_stats_of(Z, 2, 30, 1.0)
    assert M["flatness"][0] == 0 and np.isfinite(M["entropy"][0]) and M["flatness"][1] > 0
    # through the whole function: the windows that hold the NaN
    x = walk()[:, :3000].copy()
    x[1, 1234] = np.nan
    M = window_spectral_stats(x, 100.0, 250, 125, ((1, 10),), (0.9,))
    k = np.arange(23)
    hit = np.zeros((3, 23), dtype=bool)
    hit[1] = (k * 125 <= 1234) & (1234 < k * 125 + 250)
    assert hit.sum() == 2
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), np.broadcast_to(hit, M[name].shape)), name


def test_bands_hold_lo_inclusive_hi_exclusive():
    fs, W = 256, 256
    freqs = np.fft.rfftfreq(W, 1 / fs)
    k0, k1 = spectral._bin_range(freqs, None, None)
    assert (k0, k1) == (1, 128) == bins_of(fs, W)[:2]
    bins, single = spectral._band_bins((4, 8), freqs, k0, k1)
    assert bins == [(4, 8)] and single                           # bins 4 .. 7
    bins, single = spectral._band_bins([(1, 4), (4, 8), (8, 13), (13, 30), (30, 128.5)], freqs, k0, k1)
    assert bins == [(1, 4), (4, 8), (8, 13), (13, 30), (30, 129)] and not single
    assert bins == bins_of(fs, W, bands=[(1, 4), (4, 8), (8, 13), (13, 30), (30, 128.5)])[2]
    assert spectral._band_bins(((3.5, 8.5),), freqs, k0, k1) == ([(4, 9)], False)
    assert spectral._bin_range(freqs, 4, 8) == (4, 8) == bins_of(fs, W, 4, 8)[:2]          # both ends inclusive
    assert spectral._bin_range(freqs, 3.5, 8.5) == (4, 8) and spectral._bin_range(freqs, 0, None) == (0, 128)
    fs, W = 250.0, 250                                           # an odd number of bins, fractional ends
    freqs = np.fft.rfftfreq(W, 1 / fs)
    assert spectral._bin_range(freqs, None, None) == (1, 125)
    assert spectral._bin_range(freqs, 0.5, 40.0) == (1, 40) == bins_of(fs, W, 0.5, 40.0)[:2]


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_spectral(x + 1j * x, 100.0, 100)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_spectral(x.reshape(2, 2, 500), 100.0, 100)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_spectral(x, 100.0, 501)
    most = _lib.WS_BANDS_MOST
    cases = (({"winsize": 7}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "step": 101}, "larger than winsize.*no gaps"),
             ({"winsize": 100, "features": "mean"}, "total.*flatness"),
             ({"winsize": 100, "features": ("total", "Edge")}, "Edge.*total"),
             ({"winsize": 100, "features": ()}, "total"), ({"winsize": 100, "features": 3}, "total"),
             ({"winsize": 100, "features": "band"}, "need bands"),
             ({"winsize": 100, "features": "relative", "bands": ()}, "bands must be"),
             ({"winsize": 100, "features": "band", "bands": [(1, 2)] * (most + 1)}, f"1 to {most}"),
             ({"winsize": 100, "features": "band", "bands": (4, np.nan)}, "bands must be"),
             ({"winsize": 100, "features": "band", "bands": ((4, 8), (8, "12"))}, "bands must be"),
             ({"winsize": 100, "features": "band", "bands": ((4, 8, 9),)}, "bands must be"),
             ({"winsize": 100, "features": "band", "bands": (8, 4)}, "holds no bin"),
             ({"winsize": 100, "features": "band", "bands": (4.1, 4.9)}, "holds no bin"),
             ({"winsize": 100, "features": "band", "bands": (0, 8)}, "does not lie inside"),
             ({"winsize": 100, "features": "band", "bands": (40, 60), "fmax": 45}, "does not lie inside"),
             ({"winsize": 100, "features": "band", "bands": (4, 8), "fmin": 5}, "does not lie inside"),
             ({"winsize": 100, "features": "edge", "edge": ()}, f"1 to {_lib.WS_EDGES_MOST}"),
             ({"winsize": 100, "features": "edge", "edge": [0.5] * (_lib.WS_EDGES_MOST + 1)}, "1 to 16"),
             ({"winsize": 100, "features": "edge", "edge": 0.0}, r"\(0, 1\]"),
             ({"winsize": 100, "features": "edge", "edge": (0.5, 1.0000001)}, r"\(0, 1\]"),
             ({"winsize": 100, "features": "edge", "edge": np.nan}, r"\(0, 1\]"),
             ({"winsize": 100, "features": "edge", "edge": "0.5"}, r"\(0, 1\]"),
             ({"winsize": 100, "features": "edge", "edge": None}, r"\(0, 1\]"),
             ({"winsize": 100, "fmin": 60}, "no bin lies"), ({"winsize": 100, "fmax": -1}, "no bin lies"),
             ({"winsize": 100, "fmin": 30, "fmax": 20}, "no bin lies"),
             ({"winsize": 100, "fmin": 4.1, "fmax": 4.9}, "no bin lies"),
             ({"winsize": 100, "fmin": np.nan}, "fmin"), ({"winsize": 100, "fmax": "40"}, "fmax"),
             ({"winsize": 100, "scaling": "power"}, "scaling"), ({"winsize": 100, "detrend": "quadratic"}, "detrend"),
             ({"winsize": 100, "detrend": None}, "detrend"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_spectral(src.pro, 100.0, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_spectral(x, 100.0, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_spectral(src.pro, 100.0, 100, features=NAMES, bands=(4, 8))
        assert not src.started
    # bands and edge are read only when asked
    src = Untouched((4, 50))
    with pytest.raises(ValueError, match="fewer than one window"):
        window_spectral(src.pro, 100.0, 100, features="total", bands="no", edge="no")

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device (this test runs without one)
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    with pytest.raises(ValueError, match="real data.*complex128 chunks"):
        window_spectral(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100.0, 100)
    with pytest.raises(TypeError):
        window_spectral(x, 100.0, 100, resolution=0.5)                    # no such argument


C_TYPES = {"void *": ctypes.c_void_p, "double *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "const int *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}


def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint osz_spectral_features\(([^)]*)\);", header)
    assert m, "osz_spectral_features is not declared"
    declared = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()       # drop the name
        declared.append(C_TYPES[ctype])
    restype, argtypes = _lib.SIGNATURES["osz_spectral_features"]
    assert restype is ctypes.c_int and len(declared) == 18
    assert argtypes == declared, (argtypes, declared)
    assert hasattr(lib, "osz_spectral_features"), "osz_spectral_features not exported"
    for name, value in _lib.WINDOW_SPECTRAL.items():
        assert re.search(rf"OSZ_WS_{name.upper()} = {value}\b", header), name
    assert re.search(r"typedef enum \{[^}]*OSZ_WS_COUNT = 9\s*\} osz_window_spectral_feature;", header)
    for name in ("BANDS_MOST", "EDGES_MOST", "WAVE", "LDS"):
        assert re.search(rf"#define OSZ_WS_{name} {getattr(_lib, 'WS_' + name)}\b", header), name
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowspec\.hip\b", makefile, re.M)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_spectral_kernels_use_no_scratch(tmp_path):
    """Both instances of the kernel of windowspec.hip -- one wave and 256 threads -- compiled for
    gfx950 with the library's flags: no scratch, no spilled register."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowspec.hip"), "-o", str(tmp_path / "windowspec.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=csrc)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\S+)", line)
        if not m:
            continue
        if m.group(1).strip() == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    assert len(kernels) == 2 and all("spectral_features_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
