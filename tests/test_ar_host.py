"""CPU-only tests of window_ar (K22): the names, the argument errors (raised with no GPU and before
the stream is touched), the C ABI of the entry point against the header, the register report of
csrc/windowar.hip (no scratch, no spill in any instance), and ``window_ars``, the NumPy restatement
of the definitions that tests/test_gpu_ar.py compares the device against: Burg's recursion on the
error arrays and Levinson's on the biased autocorrelation, callable in float64 and in long double
(80-bit here).  The restatement is held to a second, independent form of each method (Burg's errors
recomputed at every order by filtering the window with the current polynomial, ``np.convolve``;
Yule-Walker by ``scipy.linalg.solve_toeplitz``) and pinned on closed forms (order 1, the
alternating window, an AR(2) realisation, |k| <= 1, E_p = E_0 prod (1 - k_m^2)) and on its rules: a
constant window, non-finite samples, independence of ``order``.

The tolerance of the GPU test is fixed here, from the reference alone: E[name, method] is the
largest |float64 restatement - long-double restatement| over the GPU test's fixed inputs
(``GPU_CASES``), absolute for ``coefficients`` and ``reflection``, relative to the long-double value
for ``error`` and ``error_path``, and the GPU test's bound is 32 E -- 32 for the device's lane-strided
sums and DPP folds where NumPy sums pairwise, and for its fused multiply-adds and divisions where the
long-double route rounds once.  ``test_the_bound_of_the_gpu_test`` asserts 0 < 32 E <= 1e-10, so the
bound cannot hide a failure.  The random walk is the worst conditioned of the inputs: its k_1 is
within 1e-3 of -1, so E_1 = E_0 (1 - k_1^2) multiplies the rounding of k_1 a thousandfold, and its
r_0 .. r_p are nearly equal, which Levinson's recursion amplifies.  Measured on ``GPU_CASES``, the
largest of each over all cases:
    burg         E[coefficients] = 1.31e-15  E[reflection] = 5.09e-16  E[error] = 2.94e-13  E[error_path] = 2.94e-13
    yule_walker  E[coefficients] = 7.11e-13  E[reflection] = 2.94e-13  E[error] = 1.87e-13  E[error_path] = 2.04e-13
"""

import ctypes
import os
import re
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest
import scipy.linalg
import scipy.signal

from openseize_amd import _device as dev
from openseize_amd import _lib, features
from openseize_amd.features import ar, windowed
from openseize_amd.features.ar import window_ar

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("coefficients", "reflection", "error", "error_path")
METHODS = ("burg", "yule_walker")
RELATIVE = ("error", "error_path")
MARGIN = 32
WIDE = _lib.AR_WIDE


def centred(w, center):
    """The window the model is fitted to: minus its mean, the mean from sums about w_0."""
    if not center:
        return w
    d = w - w[0]
    return d - np.sum(d) / w.dtype.type(w.shape[0])


def autocorrelation(x, p):
    """The biased r_0 .. r_p."""
    W = x.shape[0]
    return np.array([np.sum(x[:W - j] * x[j:]) for j in range(p + 1)], dtype=x.dtype) / x.dtype.type(W)


def ar_model(w, p, method, center=True):
    """(a_1 .. a_p, k_1 .. k_p, E_0 .. E_p) of one all-finite window, in w's dtype."""
    dtype = w.dtype.type
    x = centred(w, center)
    W = x.shape[0]
    a = np.zeros(p + 1, dtype=w.dtype)
    a[0] = 1
    k, E = np.full(p, np.nan, dtype=w.dtype), np.full(p + 1, np.nan, dtype=w.dtype)
    if method == "burg":
        f, b = x.copy(), x.copy()
        E[0] = np.sum(x * x) / dtype(W)
    else:
        r = autocorrelation(x, p)
        E[0] = r[0]
    with np.errstate(all="ignore"):
        for m in range(1, p + 1):
            if method == "burg":
                ff, bb = f[m:], b[m - 1:W - 1]
                km = -2 * np.sum(ff * bb) / np.sum(ff * ff + bb * bb)
                nf, nb = ff + km * bb, bb + km * ff
                f[m:], b[m:] = nf, nb
            else:
                km = -(r[m] + np.sum(a[1:m] * r[m - 1:0:-1])) / E[m - 1]
            if E[m - 1] == 0 or np.isnan(E[m - 1]):          # a spent or lost E ends the model here
                km = dtype(np.nan)
            a[1:m] = a[1:m] + km * a[m - 1:0:-1]
            a[m] = km
            k[m - 1], E[m] = km, E[m - 1] * (1 - km * km)
    if E[0] == 0:
        E[:] = 0
    return a[1:], k, E


def window_ars(x, W, step, order=8, method="burg", center=True, dtype=np.float64):
    """The definitions: "coefficients" and "reflection" (p, C, nwin), "error" (C, nwin) and
    "error_path" (p + 1, C, nwin) for x (C, N), computed in ``dtype``.  A window that holds a NaN or
    +-inf is NaN in every plane."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    C, n = x.shape
    nwin = 0 if n < W else (n - W) // step + 1
    p = order
    out = {"coefficients": np.full((p, C, nwin), np.nan, dtype=dtype), "reflection": np.full((p, C, nwin), np.nan, dtype=dtype),
           "error": np.full((C, nwin), np.nan, dtype=dtype), "error_path": np.full((p + 1, C, nwin), np.nan, dtype=dtype)}
    for c in range(C):
        for i in range(nwin):
            w = x[c, i * step:i * step + W]
            if not np.all(np.isfinite(w)):
                continue
            a, k, E = ar_model(w.astype(dtype), p, method, center)
            out["coefficients"][:, c, i], out["reflection"][:, c, i] = a, k
            out["error"][c, i], out["error_path"][:, c, i] = E[p], E
    return out


def one(w, **kwargs):
    """The measures of one window: (p,), (p,), a float and (p + 1,)."""
    w = np.asarray(w, dtype=np.float64)
    got = window_ars(w, w.shape[0], 1, **kwargs)
    return {name: (v[0, 0] if name == "error" else v[:, 0, 0]) for name, v in got.items()}


# ---- the independent forms ---------------------------------------------------------------------
def burg_by_filtering(w, p, center=True):
    """Burg with f and b recomputed from the window at every order: f_t = sum_j a_j x_{t-j} and
    b_t = sum_j a_j x_{t-m+1+j} of the order m - 1 polynomial a_0 .. a_{m-1}."""
    x = centred(w, center)
    W = x.shape[0]
    a = np.array([1.0], dtype=w.dtype)
    ks = []
    for m in range(1, p + 1):
        f, b = np.convolve(x, a)[:W], np.convolve(x, a[::-1])[:W]    # valid from t = m - 1 on
        ff, bb = f[m:], b[m - 1:W - 1]
        km = -2 * np.sum(ff * bb) / np.sum(ff * ff + bb * bb)
        ext = np.concatenate((a, [0]))
        a = ext + km * ext[::-1]
        ks.append(km)
    return a[1:], np.array(ks)


def yule_walker_by_toeplitz(w, p, center=True):
    """(a of order p, k_m as the last coefficient of the order-m solution, E_p = r_0 + sum a_j r_j)."""
    r = autocorrelation(centred(w, center), p)
    sol = [scipy.linalg.solve_toeplitz(r[:m], -r[1:m + 1]) for m in range(1, p + 1)]
    return sol[-1], np.array([s[-1] for s in sol]), r[0] + np.sum(sol[-1] * r[1:])


# ---- the fixed inputs of tests/test_gpu_ar.py --------------------------------------------------
KINDS = ("noise", "walk", "ar2", "eeg")


@lru_cache(maxsize=None)
def gpu_signal(kind, C, N):
    """Seeded, (C, N): white noise ("noise"), its cumulative sum ("walk"), the AR(2) process with
    the poles 0.98 e^{+-0.3i} driven by it ("ar2"), or two sinusoids, a slow walk, noise and an
    offset of 100 ("eeg").  Read-only."""
    assert kind in KINDS and C in (1, 3, 5) and N <= 9000
    rng = np.random.default_rng(2222)
    e = rng.standard_normal((C, N))
    if kind == "noise":
        x = e
    elif kind == "walk":
        x = np.cumsum(e, axis=-1)
    elif kind == "ar2":
        x = scipy.signal.lfilter([1.0], [1.0, -2 * 0.98 * np.cos(0.3), 0.98 ** 2], e, axis=-1)
    else:
        t = np.arange(N)
        slow = 0.05 * np.cumsum(rng.standard_normal((C, N)), axis=-1)
        x = np.sin(0.2 * t) + 0.5 * np.sin(0.7 * t + 1) + slow + 0.3 * e + 100.0
    x.setflags(write=False)
    return x


# kind, C, N, W, step, order: two to four windows and a ragged tail
GPU_CASES = (
    ("noise", 3, 16 * 4 + 5, 16, 16, 4),                     # one wave, most lanes idle, W = 4 p exactly
    ("eeg", 3, 16 * 4 + 5, 16, 16, 4),
    ("walk", 3, 250 + 2 * 125 + 37, 250, 125, 16),           # one wave, a ragged run per lane, overlap
    ("ar2", 3, 250 + 2 * 125 + 37, 250, 125, 16),
    ("eeg", 3, WIDE - 1 + 2 * 300 + 50, WIDE - 1, 300, 32),  # the widest one-wave window
    ("noise", 3, WIDE - 1 + 2 * 300 + 50, WIDE - 1, 300, 32),
    ("ar2", 3, 2 * WIDE + 100, WIDE, WIDE, 1),               # the first 256-thread window, order 1
    ("walk", 3, 2 * WIDE + 100, WIDE, WIDE, 1),
    ("noise", 3, 600 + 2 * 450 + 77, 600, 450, 32),          # 256 threads, ragged
    ("walk", 3, 600 + 2 * 450 + 77, 600, 450, 32),
    ("walk", 3, 4096 + 2048 + 300, 4096, 2048, 32),          # the longest window
    ("eeg", 3, 4096 + 2048 + 300, 4096, 2048, 32),
    ("ar2", 3, 1024 + 2 * 1500 + 200, 1024, 1500, 12),       # a gap between windows
    ("eeg", 3, 1024 + 2 * 1500 + 200, 1024, 1500, 12),
)


@lru_cache(maxsize=None)
def gpu_reference(case, method, dtype=np.longdouble):
    """``window_ars`` of GPU_CASES[case] in ``dtype``, computed once.  Read-only."""
    kind, C, N, W, step, order = GPU_CASES[case]
    ref = window_ars(gpu_signal(kind, C, N), W, step, order, method, True, dtype)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@lru_cache(maxsize=None)
def gpu_bounds():
    """(name, method) -> (E, 32 E) over GPU_CASES: the error of the float64 restatement against the
    long-double one, relative to the long-double value for the errors, absolute for the rest."""
    E = {(name, method): 0.0 for name in NAMES for method in METHODS}
    for case in range(len(GPU_CASES)):
        for method in METHODS:
            lo, hi = gpu_reference(case, method, np.float64), gpu_reference(case, method)
            for name in NAMES:
                assert np.all(np.isfinite(hi[name])), (case, method, name)
                err = np.abs(lo[name] - hi[name]) / (np.abs(hi[name]) if name in RELATIVE else 1)
                E[name, method] = max(E[name, method], float(np.max(err)))
    return {key: (e, MARGIN * e) for key, e in E.items()}


# ---- the tests ---------------------------------------------------------------------------------
def test_names_are_public():
    assert features.window_ar is window_ar
    assert features.WINDOW_ARS == ar.WINDOW_ARS == NAMES == tuple(_lib.WINDOW_AR)
    assert features.AR_METHODS == METHODS == tuple(_lib.AR_METHOD)
    assert list(_lib.WINDOW_AR.values()) == list(range(4)) and list(_lib.AR_METHOD.values()) == [0, 1]
    assert ar.window_plan is windowed.window_plan and ar._advance is windowed._advance
    assert ar.window_count is windowed.window_count
    doc = window_ar.__doc__
    for name in NAMES + METHODS:
        assert f'"{name}"' in doc, name


SHAPES = ((64, 8), (250, 16), (600, 32), (1024, 12), (4096, 32))


@lru_cache(maxsize=None)
def host_windows():
    """One window of every kind at every shape of SHAPES: ((kind, W, p), window)."""
    return tuple(((kind, W, p), gpu_signal(kind, 1, 4500)[0, 100:100 + W]) for W, p in SHAPES for kind in KINDS)


@pytest.mark.parametrize("method", METHODS)
def test_the_independent_form_agrees(method):
    worst = 0.0
    for key, w in host_windows():
        p = key[2]
        a, k, E = ar_model(w.astype(np.float64), p, method)
        if method == "burg":
            a2, k2 = burg_by_filtering(w.astype(np.float64), p)
        else:
            a2, k2, Ep = yule_walker_by_toeplitz(w.astype(np.float64), p)
            assert abs(Ep - E[p]) <= 1e-12 * abs(E[p]), key
        err = max(np.max(np.abs(a - a2)), np.max(np.abs(k - k2)))
        worst = max(worst, err)
        assert err <= 1e-12, (key, err)
    print(f"{method}: the two forms differ by at most {worst:.2e}")


def test_identities_of_the_restatement():
    for method in METHODS:
        for key, w in host_windows():
            for center in (True, False):
                a, k, E = ar_model(w.astype(np.longdouble), key[2], method, center)
                assert np.all(np.abs(k) <= 1), (method, key)
                assert a[-1] == k[-1] and np.all(np.diff(E) <= 0) and E[-1] > 0
                assert abs(E[-1] / (E[0] * np.prod(1 - k * k)) - 1) < 1e-15, (method, key)


def test_closed_forms():
    rng = np.random.default_rng(5)
    w = rng.standard_normal(100)
    x = (w - w[0]) - np.mean(w - w[0])
    k1 = -2 * np.sum(x[1:] * x[:-1]) / np.sum(x[1:] ** 2 + x[:-1] ** 2)
    got = one(w, order=1)
    assert got["reflection"][0] == pytest.approx(k1, rel=1e-14) and got["coefficients"][0] == got["reflection"][0]
    assert got["error"] == pytest.approx(np.mean(x * x) * (1 - k1 * k1), rel=1e-14)
    assert got["error_path"][0] == pytest.approx(np.mean(x * x), rel=1e-14) and got["error_path"][1] == got["error"]
    # the alternating window: burg predicts it exactly at order 1
    alt = (-1.0) ** np.arange(64)
    got = one(alt, order=4, center=False)
    assert got["reflection"][0] == 1.0 and np.all(np.isnan(got["reflection"][1:]))
    assert got["error_path"][0] == 1.0 and got["error_path"][1] == 0.0 and np.all(np.isnan(got["error_path"][2:]))
    assert np.all(np.isnan(got["coefficients"])) and np.isnan(got["error"])
    assert one(alt, order=1, center=False)["coefficients"][0] == 1.0
    got = one(alt, order=4, center=False, method="yule_walker")   # the biased estimate: k_1 = (W - 1) / W
    assert got["reflection"][0] == pytest.approx(63 / 64, rel=1e-15) and np.all(np.isfinite(got["error_path"]))


@pytest.mark.parametrize("method", METHODS)
def test_an_ar2_realisation_is_recovered(method):
    e = np.random.default_rng(11).standard_normal(6000)
    x = scipy.signal.lfilter([1.0], [1.0, -2 * 0.9 * np.cos(0.3), 0.81], e)[-4096:]
    got = one(x, order=2, method=method)
    assert np.max(np.abs(got["coefficients"] - [-2 * 0.9 * np.cos(0.3), 0.81])) < 0.05
    assert got["error"] == pytest.approx(1.0, abs=0.1)
    x1 = scipy.signal.lfilter([1.0], [1.0, -0.9], e)[-4096:]      # x_t = 0.9 x_{t-1} + e_t: a_1 = -0.9
    assert one(x1, order=1, method=method)["coefficients"][0] == pytest.approx(-0.9, abs=0.03)


@pytest.mark.parametrize("method", METHODS)
def test_a_constant_window(method):
    for w, center in ((np.full(64, 2.5), True), (np.zeros(64), False), (np.zeros(64), True)):
        got = one(w, order=4, method=method, center=center)
        assert np.all(got["error_path"] == 0) and got["error_path"].shape == (5,) and got["error"] == 0
        assert np.all(np.isnan(got["coefficients"])) and np.all(np.isnan(got["reflection"]))
    got = one(np.full(64, 2.5), order=4, method=method, center=False)   # not centred: x_t = x_{t-1}
    assert got["error_path"][0] == 6.25
    if method == "burg":                                     # predicted exactly at order 1
        assert got["reflection"][0] == -1.0 and got["error_path"][1] == 0.0
        assert np.all(np.isnan(got["reflection"][1:])) and np.all(np.isnan(got["error_path"][2:]))
    else:
        assert got["reflection"][0] == pytest.approx(-63 / 64, rel=1e-15) and np.all(np.isfinite(got["error_path"]))


@pytest.mark.parametrize("method", METHODS)
def test_non_finite_rule_of_the_restatement(method):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 600))
    clean = window_ars(x, 100, 50, 6, method)
    y = x.copy()
    y[0, 170] = np.nan
    y[1, 590:] = np.inf
    M = window_ars(y, 100, 50, 6, method)
    k = np.arange(11)
    hit = np.stack([(k * 50 <= 170) & (170 < k * 50 + 100), k * 50 + 100 > 590])
    assert hit[0].sum() == 2 and hit[1].sum() == 1
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), np.broadcast_to(hit, M[name].shape)), name
        assert np.array_equal(M[name][..., ~hit], clean[name][..., ~hit]), name


@pytest.mark.parametrize("method", METHODS)
def test_the_order_changes_no_bit_of_the_restatement(method):
    x = gpu_signal("walk", 3, 1200)
    lo, hi = window_ars(x, 300, 150, 6, method), window_ars(x, 300, 150, 12, method)
    assert np.array_equal(lo["reflection"], hi["reflection"][:6])
    assert np.array_equal(lo["error_path"], hi["error_path"][:7])
    assert np.array_equal(lo["error"], hi["error_path"][6])
    assert not np.array_equal(lo["coefficients"], hi["coefficients"][:6])


def test_argument_errors_come_before_the_stream(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_ar(x + 1j * x, 100)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_ar(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_ar(x, 501)
    longest = _lib.AR_LONGEST
    cases = (({"winsize": 15, "order": 2}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": longest + 1}, f"winsize.*{longest}"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "order": 0}, "order"), ({"winsize": 4096, "order": 33}, "order"),
             ({"winsize": 100, "order": 8.0}, "order"), ({"winsize": 100, "order": True}, "order"),
             ({"winsize": 31, "order": 8}, "4 order"), ({"winsize": 100, "order": 26}, "4 order = 104"),
             ({"winsize": 100, "method": "covariance"}, "method.*burg"), ({"winsize": 100, "method": "Burg"}, "method"),
             ({"winsize": 100, "method": 0}, "method"), ({"winsize": 100, "method": None}, "method"),
             ({"winsize": 100, "measures": "psd"}, "coefficients.*error_path"),
             ({"winsize": 100, "measures": ("error", "Reflection")}, "Reflection.*coefficients"),
             ({"winsize": 100, "measures": ()}, "coefficients"), ({"winsize": 100, "measures": 3}, "coefficients"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_ar(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_ar(x, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_ar(src.pro, 100, measures=NAMES)
        assert not src.started

    # a producer shows what it holds with its first chunk
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    for kwargs in ({}, {"method": "yule_walker", "order": 25, "measures": NAMES}):
        with pytest.raises(ValueError, match="real data.*complex128 chunks"):
            window_ar(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), **{"winsize": 100, **kwargs})
    with pytest.raises(TypeError):
        window_ar(x, 100, fs=100)                                         # no such argument


C_TYPES = {"void *": ctypes.c_void_p, "double *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint osz_window_ar\(([^)]*)\);", header)
    assert m, "osz_window_ar is not declared"
    declared = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()       # drop the name
        declared.append(C_TYPES[ctype])
    restype, argtypes = _lib.SIGNATURES["osz_window_ar"]
    assert restype is ctypes.c_int and len(declared) == 15
    assert argtypes == declared, (argtypes, declared)
    assert hasattr(lib, "osz_window_ar"), "osz_window_ar not exported"
    for name, value in _lib.WINDOW_AR.items():
        assert re.search(rf"OSZ_AR_{name.upper()} = {value}\b", header), name
    assert re.search(r"typedef enum \{[^}]*OSZ_AR_COUNT = 4\s*\} osz_window_ar_measure;", header)
    for name, value in _lib.AR_METHOD.items():
        assert re.search(rf"OSZ_AR_{name.upper()} = {value}\b", header), name
    assert re.search(r"typedef enum \{[^}]*OSZ_AR_YULE_WALKER = 1[^}]*\} osz_window_ar_method;", header)
    for name in ("LONGEST", "WIDE", "ORDER"):
        assert re.search(rf"#define OSZ_AR_{name} {getattr(_lib, 'AR_' + name)}\b", header), name
    assert (_lib.AR_LONGEST, _lib.AR_WIDE, _lib.AR_ORDER) == (4096, 512, 32)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowar\.hip\b", makefile, re.M)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_ar_kernels_use_no_scratch(tmp_path):
    """Every instance of the kernel of windowar.hip -- one per (threads, samples a thread) --
    compiled for gfx950 with the library's flags: no scratch, no spilled VGPR or SGPR, no dynamic
    stack.  The register counts are printed, not fixed."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowar.hip"), "-o", str(tmp_path / "windowar.o"),
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
    assert len(kernels) == 8 and all("window_ar_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert use["Dynamic Stack"] == "False"


def test_the_bound_of_the_gpu_test():
    bounds = gpu_bounds()
    for method in METHODS:
        for name in NAMES:
            E, bound = bounds[name, method]
            print(f"E[{name}, {method}] = {E:.2e}, bound {bound:.2e}")
            assert 0 < bound == MARGIN * E <= 1e-10, (name, method, E)
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs an 80-bit long double"
