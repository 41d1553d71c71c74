"""CPU-only tests of window_wavelet (K21): the names, ``wavelet_filters`` (the Daubechies filters
from the project's own spectral factorisation), ``wavelet_level`` and ``wavelet_bands``, the
argument errors (raised with no GPU and before the stream is touched), the C ABI of the entry point
against the header, the register report of csrc/windowwave.hip (no scratch, no spill in either
kernel), and ``window_wavelets``, the NumPy restatement of the definitions that
tests/test_gpu_wavelet.py compares the device against: index arrays ``(2 i + k) % n`` and plain
sums, callable in float64 and in long double (80-bit here).  The restatement is pinned on closed
forms (haar on a hand-worked window of 8, the energy identity for every named filter, a constant
window, the vanishing moments) and on the rule for non-finite samples.

The tolerance of the GPU test is fixed here, from the reference alone: E[name] is the largest
|float64 restatement - long-double restatement| over the GPU test's fixed inputs (``GPU_CASES``;
relative to the band's own long-double value for ``energy``, ``mean_abs`` and ``std``, absolute for
``relative`` and ``entropy``) and the GPU test's bound is 32 E[name] -- the margin that
tests/test_fractal_host.py justifies for lane-strided sums (up to W / 64 + 8 roundings where NumPy's
pairwise sums have log2 W) and for the device's log, sqrt and divisions of 1 to 2 ulp each where
the long-double route rounds once.  ``test_the_bound_of_the_gpu_test`` asserts 0 < 32 E <= 1e-11, so
the bound cannot hide a failure.  The cases are chosen so that the reference alone meets that cap:
a full-depth transform (a^J one coefficient) runs un-centred, because the a^J of a centred window is
then rounding noise alone, and the sinusoid on an offset of 1e4 has an amplitude of 100 and runs
un-centred with haar at one level only, because every detail coefficient of un-centred data is what
the filter leaves of 1e4 and a deeper level of 1e4 2^(j/2).  Measured on ``GPU_CASES``, the largest
of each over all cases:
    E[energy] = 4.05e-14   E[relative] = 2.45e-16   E[entropy] = 2.98e-16   E[mean_abs] = 3.24e-14
    E[std] = 1.27e-14
"""

import ctypes
import os
import re
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, features
from openseize_amd.features import wavelet, windowed
from openseize_amd.features.wavelet import wavelet_bands, wavelet_filters, wavelet_level, window_wavelet

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("energy", "relative", "entropy", "mean_abs", "std")
PER_BAND = ("energy", "relative", "mean_abs", "std")
RELATIVE_TO_ITSELF = ("energy", "mean_abs", "std")
NAMED = tuple(f"db{N}" for N in range(1, 11))
MARGIN = 32
WIDE = _lib.WW_WIDE


def transform(a, h, J):
    """The bands d^1, .., d^J, a^J of a^0 = ``a`` (one window) under the low-pass filter ``h``,
    periodised: a list of J + 1 arrays in the dtype of ``a``."""
    dtype = a.dtype
    h = np.asarray(h).astype(dtype)
    L = h.shape[0]
    g = h[::-1] * np.where(np.arange(L) % 2, -1, 1).astype(dtype)
    bands = []
    for _ in range(J):
        n = a.shape[0]
        assert n % 2 == 0
        at = (2 * np.arange(n // 2)[:, None] + np.arange(L)[None, :]) % n      # (n / 2, L)
        taps = a[at]
        bands.append(np.sum(taps * g, axis=1))
        a = np.sum(taps * h, axis=1)
    bands.append(a)
    return bands


def band_features(bands, normalize):
    """name -> the B values (entropy: one) of one window's bands."""
    dtype = bands[0].dtype
    B = len(bands)
    E = np.array([np.sum(c * c) for c in bands], dtype=dtype)
    total = np.sum(E)
    with np.errstate(all="ignore"):
        p = E / total
        H = -np.sum(np.where(p > 0, p * np.log(np.where(p > 0, p, 1)), 0))
        if normalize:
            H = H / np.log(dtype.type(B))
    return {"energy": E, "relative": p, "entropy": H if total > 0 else dtype.type(np.nan),
            "mean_abs": np.array([np.mean(np.abs(c)) for c in bands], dtype=dtype),
            "std": np.array([np.sqrt(np.mean((c - np.mean(c)) ** 2)) for c in bands], dtype=dtype)}


def window_wavelets(x, W, step, wavelet="db4", level=None, center=True, normalize=True, dtype=np.float64):
    """The definitions: name -> (B, C, nwin), "entropy" (C, nwin), for x (C, N), computed in
    ``dtype`` from the float64 filter of ``wavelet_filters``.  The mean comes from sums about the
    window's first sample.  A window that holds a NaN or +-inf is NaN in every feature."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    h = wavelet_filters(wavelet)[0]
    J = wavelet_level(W, h.shape[0]) if level is None else level
    assert W % (1 << J) == 0
    n = x.shape[-1]
    nwin = 0 if n < W else (n - W) // step + 1
    out = {name: np.full((J + 1, x.shape[0], nwin) if name in PER_BAND else (x.shape[0], nwin), np.nan, dtype=dtype)
           for name in NAMES}
    for c in range(x.shape[0]):
        for k in range(nwin):
            w = x[c, k * step:k * step + W]
            if not np.all(np.isfinite(w)):
                continue
            w = w.astype(dtype)
            if center:
                w = w - w[0]
                w = w - np.sum(w) / dtype(W)
            F = band_features(transform(w, h, J), normalize)
            for name in NAMES:
                out[name][..., c, k] = F[name]
    return out


def one(w, **kwargs):
    """The features of one window: arrays over the bands, the entropy a float."""
    w = np.asarray(w, dtype=np.float64)
    return {name: v[..., 0, 0] for name, v in window_wavelets(w, w.shape[0], 1, **kwargs).items()}


# ---- the fixed inputs of tests/test_gpu_wavelet.py ---------------------------------------------
@lru_cache(maxsize=None)
def gpu_signal(kind, C, N):
    """Seeded white noise ("white"), its cumulative sum ("walk") or 1e4 + 100 sin(2 pi f t + c) with
    f = 0.0837 + 0.05 c cycles a sample for channel c ("sine"), (C, N).  Read-only."""
    assert kind in ("white", "walk", "sine") and C in (1, 3) and N <= 13000
    x = np.random.default_rng(2121).standard_normal((C, N))
    if kind == "walk":
        x = np.cumsum(x, axis=-1)
    if kind == "sine":
        c = np.arange(C)[:, None]
        x = 1e4 + 100 * np.sin(2 * np.pi * (0.0837 + 0.05 * c) * np.arange(N)[None, :] + c)
    x.setflags(write=False)
    return x


DB3 = tuple(float(v) for v in wavelet_filters("db3")[0])
# kind, C, N, W, step, level (None: the default), wavelet, center, normalize
GPU_CASES = (
    ("white", 3, 40, 8, 8, 3, "db4", False, True),           # n_j < L from the start; a^3 one coefficient
    ("walk", 3, 84, 24, 12, 3, "db10", True, False),         # W no power of two, n = 24, 12, 6 under L = 20
    ("sine", 3, 384, 96, 48, 5, "db2", True, True),
    ("walk", 3, 384, 96, 48, 5, "db2", False, True),
    ("white", 3, WIDE + 900, WIDE, 300, None, "db4", True, True),          # the widest one-wave window
    ("walk", 3, 640 + 1500, 640, 500, 7, "db4", True, True),               # the narrowest 256-thread window
    ("white", 3, 4096, 1024, 1024, None, "db4", True, False),
    ("walk", 3, 3072, 1024, 512, None, "db4", False, True),
    ("white", 3, 12288, 4096, 4096, 12, "db10", False, True),              # n down to 2, L = 20
    ("sine", 3, 256, 64, 64, 1, "haar", True, True),
    ("sine", 3, 256, 64, 64, 1, "haar", False, False),
    ("walk", 3, 480, 96, 96, None, DB3, True, True),         # a sequence: db3's bits
)


@lru_cache(maxsize=None)
def gpu_reference(case, dtype=np.longdouble):
    """``window_wavelets`` of GPU_CASES[case] in ``dtype``, computed once.  Read-only."""
    kind, C, N, W, step, level, name, center, normalize = GPU_CASES[case]
    ref = window_wavelets(gpu_signal(kind, C, N), W, step, name, level, center, normalize, dtype)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def error_of(name, got, want):
    """|got - want|: relative to ``want`` for a feature held to its own size (a value that is
    exactly 0 -- the std of a band of one coefficient -- must be met exactly), else absolute."""
    err = np.abs(got.astype(np.longdouble) - want)
    if name in RELATIVE_TO_ITSELF:
        zero = want == 0
        err = np.where(zero, np.where(got == 0, 0, np.inf), err / np.where(zero, 1, np.abs(want)))
    return err


@lru_cache(maxsize=None)
def gpu_bounds():
    """name -> (E, 32 E) over GPU_CASES: the error of the float64 restatement against the
    long-double one."""
    E = dict.fromkeys(NAMES, 0.0)
    for case in range(len(GPU_CASES)):
        lo, hi = gpu_reference(case, np.float64), gpu_reference(case)
        for name in NAMES:
            assert np.all(np.isfinite(hi[name])), (case, name)
            E[name] = max(E[name], float(np.max(error_of(name, lo[name], hi[name]))))
    return {name: (e, MARGIN * e) for name, e in E.items()}


def test_names_are_public():
    assert features.window_wavelet is window_wavelet and features.wavelet_filters is wavelet_filters
    assert features.wavelet_level is wavelet_level and features.wavelet_bands is wavelet_bands
    assert features.WINDOW_WAVELET == wavelet.WINDOW_WAVELET == NAMES == tuple(_lib.WINDOW_WAVELET)
    assert features.WAVELETS == wavelet.WAVELETS == ("haar",) + NAMED
    assert list(_lib.WINDOW_WAVELET.values()) == list(range(5))
    assert wavelet.window_plan is windowed.window_plan and wavelet._advance is windowed._advance
    assert wavelet.window_count is windowed.window_count
    doc = window_wavelet.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name


def orthonormality(h):
    L = h.shape[0]
    return max([abs(np.sum(h) - np.sqrt(2.0))] +
               [abs(np.sum(h[:L - 2 * m] * h[2 * m:]) - (m == 0)) for m in range(L // 2)])


def test_the_named_filters():
    for N, name in enumerate(NAMED, 1):
        h, g = wavelet_filters(name)
        assert h.dtype == g.dtype == np.float64 and h.shape == g.shape == (2 * N,)
        assert np.array_equal(g, [(-1) ** k * h[2 * N - 1 - k] for k in range(2 * N)])
        assert abs(np.sum(h) - np.sqrt(2.0)) <= 4e-15          # (up to 20 roundings of values below 1, and the scaling's)
        worst = orthonormality(h)
        k = np.arange(2 * N, dtype=np.float64)
        moments = max(abs(np.sum(g * k ** p)) / np.sum(np.abs(g) * k ** p) for p in range(N))
        print(f"{name}: orthonormality {worst:.2e}, moments {moments:.2e}")
        assert worst <= 1e-13 and moments <= 1e-12, (name, worst, moments)
        h[0] = 5.0                                           # the caller's copy: the cache is not touched
        assert wavelet_filters(name)[0][0] != 5.0
    s2, s3 = np.sqrt(2.0), np.sqrt(3.0)
    db2 = np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * s2)
    assert np.all(np.abs(wavelet_filters("db2")[0] - db2) <= 4 * np.spacing(np.abs(db2)))
    for name in ("haar", "db1"):
        h, g = wavelet_filters(name)
        assert np.all(np.abs(h - s2 / 2) <= 4 * np.spacing(s2 / 2)) and np.array_equal(g, [h[1], -h[0]])


def test_a_filter_given_as_a_sequence():
    h3 = wavelet_filters("db3")[0]
    for given in (list(h3), tuple(h3), h3, h3.astype(np.longdouble)):
        h, g = wavelet_filters(given)
        assert np.array_equal(h, h3) and np.array_equal(g, wavelet_filters("db3")[1])
    # orthonormal without being a Daubechies filter: the time reverse, the maximum-phase factor
    assert np.array_equal(wavelet_filters(h3[::-1])[0], h3[::-1])
    bad = np.array(h3)
    bad[2] += 1e-9
    refused = (bad, h3 * (1 + 1e-9), [1.0, 1.0], [0.5, 0.5, 0.5, 0.5], h3[:5], [np.sqrt(2.0)], [], np.ones((2, 2)),
               np.r_[h3[:5], np.nan], [1j, 1.0], np.zeros(34), "db11", "sym4", "DB4", None, 4)
    for given in refused:
        with pytest.raises(ValueError, match="wavelet_filters"):
            wavelet_filters(given)
        with pytest.raises(ValueError, match="window_wavelet"):
            window_wavelet(Untouched((2, 500)).pro, 64, wavelet=given)
    close = np.array(h3)
    close[2] += 1e-12                                        # within the 1e-10 of the conditions
    assert np.array_equal(wavelet_filters(close)[0], close)


def test_wavelet_level_and_bands():
    # max(1, min(v, floor(log2(W / (L - 1))), 12)), by hand
    assert wavelet_level(1024, 8) == 7                       # 1024 / 7 = 146.3
    assert wavelet_level(512, 8) == 6 and wavelet_level(896, 8) == 7 and wavelet_level(4096, 8) == 9
    assert wavelet_level(96, 4) == 5                         # v = 5, 96 / 3 = 32
    assert wavelet_level(96, 6) == 4                         # 96 / 5 = 19.2
    assert wavelet_level(24, 20) == 1 and wavelet_level(8, 32) == 1         # the floor is 0 or less
    assert wavelet_level(4096, 2) == 12 and wavelet_level(64, 2) == 6 and wavelet_level(8192, 2) == 12
    assert wavelet_level(1000, 8) == 3 and wavelet_level(1002, 8) == 1      # v = 3, v = 1
    assert wavelet_level(4096, 20) == 7                      # 4096 / 19 = 215.6
    for bad in ((1001, 8), (64, 7), (64.0, 8), (64, 34), (0, 8), (64, 0), (True, 8)):
        with pytest.raises(ValueError, match="wavelet_level"):
            wavelet_level(*bad)
    assert wavelet_bands(256, 3) == ((64.0, 128.0), (32.0, 64.0), (16.0, 32.0), (0.0, 16.0))
    assert wavelet_bands(1.0, 1) == ((0.25, 0.5), (0.0, 0.25))
    assert len(wavelet_bands(500, 12)) == 13 and wavelet_bands(500, 12)[-1] == (0.0, 500 / 8192)
    for bad in ((256, 0), (256, 13), (256, 2.0), (0, 3), (-1.0, 3), ("256", 3), (np.inf, 3)):
        with pytest.raises(ValueError, match="wavelet_bands"):
            wavelet_bands(*bad)


def test_haar_on_a_hand_worked_window():
    w = [4.0, 6.0, 10.0, 12.0, 8.0, 6.0, 5.0, 5.0]
    r = np.sqrt(2.0)
    # a1 = (10, 22, 14, 10) / r, d1 = (-2, -2, 2, 0) / r; a2 = (16, 12), d2 = (-6, 2); a3 = 28 / r, d3 = 4 / r
    bands = transform(np.array(w), wavelet_filters("haar")[0], 3)
    for got, want in zip(bands, ([-2 / r, -2 / r, 2 / r, 0], [-6, 2], [4 / r], [28 / r])):
        assert np.allclose(got, want, rtol=0, atol=1e-14), (got, want)
    got = one(w, wavelet="haar", level=3, center=False, normalize=False)
    E = np.array([6.0, 40.0, 8.0, 392.0])
    assert np.allclose(got["energy"], E, rtol=1e-14) and np.sum(E) == np.sum(np.square(w))
    assert np.allclose(got["relative"], E / 446, rtol=1e-14)
    assert got["entropy"] == pytest.approx(-np.sum(E / 446 * np.log(E / 446)), abs=1e-15)
    assert np.allclose(got["mean_abs"], [6 / r / 4, 4.0, 4 / r, 28 / r], rtol=1e-14)
    assert np.allclose(got["std"], [np.sqrt(1.5 - 0.0625 * 2), 4.0, 0.0, 0.0], rtol=1e-14, atol=0)
    norm = one(w, wavelet="haar", level=3, center=False)["entropy"]
    assert norm == pytest.approx(got["entropy"] / np.log(4), abs=1e-15)
    # centred: the mean, 7, leaves every detail as it is and a^3 = 0 to rounding
    cen = one(w, wavelet="haar", level=3, normalize=False)
    assert np.allclose(cen["energy"][:3], E[:3], rtol=1e-14) and cen["energy"][3] < 1e-28


def test_the_energy_identity_for_every_named_filter():
    rng = np.random.default_rng(5)
    for name in ("haar",) + NAMED:
        L = wavelet_filters(name)[0].shape[0]
        for W, J in ((8, 3), (24, 3), (96, 5), (1024, None), (4096, 12)):
            x = rng.standard_normal(W) + 3.0
            if J is not None and W >> (J - 1) < L:
                assert W >> (J - 1) < L                      # (a level whose input is shorter than the filter)
            for center in (True, False):
                got = one(x, wavelet=name, level=J, center=center, dtype=np.longdouble)
                want = np.sum((x - np.mean(x)) ** 2) if center else np.sum(x * x)
                assert abs(np.sum(got["energy"]) / want - 1) <= 1e-12, (name, W, J, center)
                assert abs(np.sum(got["relative"]) - 1) <= 1e-15
    assert 8 >> 2 < 8 and 24 >> 2 < 20                       # db4 at (8, 3), db10 at (24, 3): such levels were met


def test_a_constant_window():
    for name in ("haar", "db4", "db10"):
        got = one(np.full(64, 2.5), wavelet=name, level=3)
        for f in ("energy", "mean_abs", "std"):
            assert got[f].shape == (4,) and np.all(got[f] == 0), (name, f)
        assert np.all(np.isnan(got["relative"])) and np.isnan(got["entropy"])
        # un-centred the whole energy is in a^J, whose coefficients are equal: std 0 to rounding
        raw = one(np.full(64, 2.5), wavelet=name, level=3, center=False)
        assert raw["relative"][3] == pytest.approx(1.0, abs=1e-13) and raw["entropy"] == pytest.approx(0.0, abs=1e-10)
        assert raw["energy"][3] == pytest.approx(64 * 6.25, rel=1e-13) and raw["std"][3] < 1e-13
        assert raw["mean_abs"][3] == pytest.approx(2.5 * 2 ** 1.5, rel=1e-13)


def test_vanishing_moments():
    # a polynomial of degree < N has no detail at level 1 where the filter does not wrap
    t = np.arange(64, dtype=np.longdouble) / 64
    for N in range(1, 11):
        h = wavelet_filters(f"db{N}")[0]
        poly = sum((p + 1) * t ** p for p in range(N))
        d1 = transform(poly, h, 1)[0]
        inside = d1[:(64 - 2 * N) // 2 + 1]                   # 2 i + 2 N - 1 <= 63
        assert inside.shape[0] >= 22 and np.max(np.abs(inside)) <= 1e-11, (N, float(np.max(np.abs(inside))))
        if N > 1:                                            # the wrap sees the jump from t = 63 / 64 back to 0
            assert np.max(np.abs(d1[inside.shape[0]:])) > 1e-3
        if N < 10:                                           # one degree more is seen
            assert np.min(np.abs(transform((64 * t) ** N, h, 1)[0][:inside.shape[0]])) > 1e-3


def test_non_finite_rule_of_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 600))
    clean = window_wavelets(x, 96, 48)
    y = x.copy()
    y[0, 170] = np.nan
    y[1, 570:] = np.inf
    M = window_wavelets(y, 96, 48)
    k = np.arange(11)
    hit = np.stack([(k * 48 <= 170) & (170 < k * 48 + 96), k * 48 + 96 > 570])
    assert hit[0].sum() == 2 and hit[1].sum() == 1
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), np.broadcast_to(hit, M[name].shape)), name
        assert np.array_equal(M[name][..., ~hit], clean[name][..., ~hit]), name


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_wavelet(x + 1j * x, 96)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_wavelet(x.reshape(2, 2, 500), 96)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_wavelet(x, 504)
    longest = _lib.WW_LONGEST
    cases = (({"winsize": 7}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 96.0}, "winsize"),
             ({"winsize": "96"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": longest + 2}, f"winsize.*{longest}"),
             ({"winsize": 96, "step": 0}, "step"), ({"winsize": 96, "step": -5}, "step"),
             ({"winsize": 96, "step": 12.5}, "step"),
             ({"winsize": 96, "level": 0}, "level"), ({"winsize": 96, "level": 13}, "level"),
             ({"winsize": 96, "level": 2.0}, "level"), ({"winsize": 96, "level": True}, "level"),
             ({"winsize": 96, "level": 6}, "winsize = 96.*J = 6"), ({"winsize": 100, "level": 3}, "winsize = 100.*J = 3"),
             ({"winsize": 4096, "level": 12, "wavelet": "haar", "step": 0}, "step"),
             ({"winsize": 97}, "winsize = 97 is odd"), ({"winsize": 97, "level": 1}, "winsize = 97.*J = 1"),
             ({"winsize": 96, "wavelet": "db11"}, "db11"), ({"winsize": 96, "wavelet": "sym4"}, "unknown wavelet"),
             ({"winsize": 96, "wavelet": [1.0, 1.0]}, "not orthonormal"),
             ({"winsize": 96, "wavelet": [0.7, 0.7, 0.1]}, "even number"),
             ({"winsize": 96, "wavelet": 4}, "wavelet must be"),
             ({"winsize": 96, "features": "power"}, "energy.*std"),
             ({"winsize": 96, "features": ("energy", "STD")}, "STD.*energy"),
             ({"winsize": 96, "features": ()}, "energy"), ({"winsize": 96, "features": 3}, "energy"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_wavelet(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_wavelet(x, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_wavelet(src.pro, 96, features=NAMES)
        assert not src.started

    # these pass the checks and reach the stream's first chunk, which is complex
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    for kwargs in ({}, {"wavelet": DB3, "level": 1}, {"winsize": 4096, "level": 12, "wavelet": "db10"},
                   {"features": NAMES, "center": False, "normalize": False}):
        with pytest.raises(ValueError, match="real data.*complex128 chunks"):
            window_wavelet(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), **{"winsize": 96, **kwargs})
    with pytest.raises(TypeError):
        window_wavelet(x, 96, fs=100)                                     # no such argument


C_TYPES = {"void *": ctypes.c_void_p, "double *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint osz_window_wavelet\(([^)]*)\);", header)
    assert m, "osz_window_wavelet is not declared"
    declared = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()       # drop the name
        declared.append(C_TYPES[ctype])
    restype, argtypes = _lib.SIGNATURES["osz_window_wavelet"]
    assert restype is ctypes.c_int and len(declared) == 16
    assert argtypes == declared, (argtypes, declared)
    assert hasattr(lib, "osz_window_wavelet"), "osz_window_wavelet not exported"
    for name, value in _lib.WINDOW_WAVELET.items():
        assert re.search(rf"OSZ_WW_{name.upper()} = {value}\b", header), name
    assert re.search(r"typedef enum \{[^}]*OSZ_WW_COUNT = 5\s*\} osz_window_wavelet_feature;", header)
    for name in ("LONGEST", "WIDE", "TAPS", "LEVELS"):
        assert re.search(rf"#define OSZ_WW_{name} {getattr(_lib, 'WW_' + name)}\b", header), name
    assert (_lib.WW_LONGEST, _lib.WW_WIDE, _lib.WW_TAPS, _lib.WW_LEVELS) == (4096, 512, 32, 12)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowwave\.hip\b", makefile, re.M)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_wavelet_kernels_use_no_scratch(tmp_path):
    """Both instances of the kernel of windowwave.hip, compiled for gfx950 with the library's flags:
    no scratch, no spilled VGPR or SGPR, no dynamic stack.  The register counts are printed, not
    fixed."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowwave.hip"), "-o", str(tmp_path / "windowwave.o"),
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
    assert len(kernels) == 2 and all("window_wavelet_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert use["Dynamic Stack"] == "False"


def test_the_bound_of_the_gpu_test():
    bounds = gpu_bounds()
    for name in NAMES:
        E, bound = bounds[name]
        print(f"E[{name}] = {E:.2e}, bound {bound:.2e}")
        assert 0 < bound == MARGIN * E <= 1e-11, (name, E)
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs an 80-bit long double"
