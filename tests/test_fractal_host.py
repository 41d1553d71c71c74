"""CPU-only tests of window_fractal (K20): the names, ``dfa_scales``, the argument errors (raised
with no GPU and before the stream is touched), the C ABI of the entry point against the header, the
register report of csrc/windowfrac.hip (no scratch, no spill in any kernel), and
``window_fractals``, the NumPy restatement of the definitions that tests/test_gpu_fractal.py
compares the device against: loops over k and m for Higuchi, a ``cumsum`` and a per-box fit for
DFA, callable in float64 and in long double (80-bit here).  The restatement is pinned on closed
forms (a straight line, an alternating window, the parabola residual of DFA, white noise and a
random walk, a constant) and on the rule for non-finite samples.

The tolerance of the GPU test is fixed here, from the reference alone: for every continuous measure
E[name] is the largest |float64 restatement - long-double restatement| over the GPU test's fixed
inputs (``GPU_CASES``; relative to F for ``dfa_fluctuations``, absolute for the rest) and the GPU
test's bound is 32 E[name] -- 32 for the device's lane-strided sums (up to W / 64 + 8 roundings
where NumPy's pairwise sums have log2 W) and for its log, sqrt and divisions of 1 to 2 ulp each
where the long-double route rounds once.  ``test_the_bound_of_the_gpu_test`` asserts 32 E <= 1e-11,
so the bound cannot hide a failure.  Measured on ``GPU_CASES``, the largest of each over all cases
(the walk's profile reaches 1e5, whose ulp sets the float64 route's error in F; the offset of 1e4
sets that of katz, whose d is 1e-4 of the samples):
    E[higuchi] = 2.31e-15   E[katz] = 3.33e-14   E[dfa] = 5.67e-15   E[dfa_fluctuations] = 4.75e-14
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
from openseize_amd.features import fractal, windowed
from openseize_amd.features.fractal import dfa_scales, window_fractal

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("higuchi", "katz", "petrosian", "dfa", "dfa_fluctuations")
CONTINUOUS = ("higuchi", "katz", "dfa", "dfa_fluctuations")
MARGIN = 32
WIDE = _lib.WR_WIDE


def centred_slope(u, v):
    """sum (u - mean u) v / sum (u - mean u)^2."""
    du = u - np.mean(u)
    with np.errstate(all="ignore"):
        return np.sum(du * v) / np.sum(du * du)


def higuchi_lengths(w, kmax):
    """L(k), k = 1 .. kmax, of one window."""
    dtype = w.dtype.type
    W = w.shape[0]
    L = np.zeros(kmax, dtype=w.dtype)
    for k in range(1, kmax + 1):
        Lm = np.zeros(k, dtype=w.dtype)
        for m in range(k):
            n = (W - 1 - m) // k
            curve = w[m:m + n * k + 1:k]                    # x_m, x_{m+k}, .., x_{m+nk}
            Lm[m] = np.sum(np.abs(np.diff(curve))) * dtype(W - 1) / dtype(n * k) / dtype(k)
        L[k - 1] = np.mean(Lm)
    return L


def higuchi(w, kmax):
    L = higuchi_lengths(w, kmax)
    if np.any(L == 0):
        return w.dtype.type(np.nan)
    k = np.arange(1, kmax + 1).astype(w.dtype)
    return centred_slope(np.log(1 / k), np.log(L))


def katz(w):
    n = w.dtype.type(w.shape[0] - 1)
    with np.errstate(all="ignore"):
        L, d = np.sum(np.abs(np.diff(w))), np.max(np.abs(w - w[0]))
        return np.log(n) / (np.log(n) + np.log(d / L))


def petrosian_count(w):
    d = np.diff(w)
    return int(np.sum(((d[:-1] > 0) & (d[1:] < 0)) | ((d[:-1] < 0) & (d[1:] > 0))))


def petrosian(w):
    dtype = w.dtype.type
    W, N = dtype(w.shape[0]), dtype(petrosian_count(w))
    return np.log10(W) / (np.log10(W) + np.log10(W / (W + dtype(4) / dtype(10) * N)))


def fluctuations(w, scales):
    """F(n) of one window for every n of scales."""
    W = w.shape[0]
    y = np.cumsum(w - np.mean(w))
    F = np.zeros(len(scales), dtype=w.dtype)
    for s, n in enumerate(scales):
        boxes = y[:(W // n) * n].reshape(W // n, n)
        i = np.arange(n).astype(w.dtype)
        ic = i - np.mean(i)
        rss = w.dtype.type(0)
        for box in boxes:                                    # the least-squares line of each box
            slope, level = np.sum(ic * box) / np.sum(ic * ic), np.mean(box)
            rss += np.sum((box - level - slope * ic) ** 2)
        F[s] = np.sqrt(rss / w.dtype.type((W // n) * n))
    return F


def dfa(F, scales):
    if np.any(F == 0):
        return F.dtype.type(np.nan)
    return centred_slope(np.log(np.asarray(scales).astype(F.dtype)), np.log(F))


def window_fractals(x, W, step, kmax=8, scales=None, dtype=np.float64):
    """The definitions: name -> (C, nwin), "dfa_fluctuations" (S, C, nwin), for x (C, N), computed in
    ``dtype``.  A window that holds a NaN or +-inf is NaN in every measure.  ``scales=None`` means
    ``dfa_scales(W)``; for W < 32 it leaves the DFA measures out, as W < 2 kmax does "higuchi"."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1]
    nwin = 0 if n < W else (n - W) // step + 1
    if scales is None and W >= 32:
        scales = dfa_scales(W)
    out = {name: np.full((x.shape[0], nwin), np.nan, dtype=dtype) for name in ("katz", "petrosian")}
    if W >= 2 * kmax:
        out["higuchi"] = np.full((x.shape[0], nwin), np.nan, dtype=dtype)
    if scales is not None:
        out["dfa"] = np.full((x.shape[0], nwin), np.nan, dtype=dtype)
        out["dfa_fluctuations"] = np.full((len(scales), x.shape[0], nwin), np.nan, dtype=dtype)
    for c in range(x.shape[0]):
        for k in range(nwin):
            w = x[c, k * step:k * step + W]
            if not np.all(np.isfinite(w)):
                continue
            w = w.astype(dtype)
            out["katz"][c, k], out["petrosian"][c, k] = katz(w), petrosian(w)
            if "higuchi" in out:
                out["higuchi"][c, k] = higuchi(w, kmax)
            if scales is not None:
                F = fluctuations(w, scales)
                out["dfa_fluctuations"][:, c, k], out["dfa"][c, k] = F, dfa(F, scales)
    return {name: out[name] for name in NAMES if name in out}


def one(w, **kwargs):
    """The measures of one window: floats, the fluctuations an array."""
    w = np.asarray(w, dtype=np.float64)
    got = window_fractals(w, w.shape[0], 1, **kwargs)
    return {name: (v[:, 0, 0] if name == "dfa_fluctuations" else v[0, 0]) for name, v in got.items()}


# ---- the fixed inputs of tests/test_gpu_fractal.py ---------------------------------------------
@lru_cache(maxsize=None)
def gpu_signal(kind, C, N):
    """Seeded white noise ("white"), its cumulative sum ("walk") or noise + 1e4 ("offset"), (C, N).
    Read-only."""
    assert kind in ("white", "walk", "offset") and C in (1, 3, 5) and N <= 9000
    x = np.random.default_rng(2020).standard_normal((C, N))
    x = np.cumsum(x, axis=-1) if kind == "walk" else x + 1e4 if kind == "offset" else x
    x.setflags(write=False)
    return x


SCALES_32 = (4, 5, 6, 7, 9, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 63, 64, 65, 80, 96, 100, 127, 128, 150, 200,
             250, 300, 333, 400, 450, 500)
# kind, C, N, W, step, kmax, scales (None: the default)
GPU_CASES = (
    ("white", 3, 64, 8, 8, 4, None),                         # (no DFA: W < 32, and scales=(4,) is refused)
    ("walk", 3, 80, 32, 16, 16, None),                       # every n_mk is 1 or 2
    ("offset", 3, 189, 63, 63, 8, None),
    ("white", 5, 192, 64, 64, 8, None),
    ("walk", 1, 145, 65, 40, 8, None),
    ("offset", 3, 500, 250, 125, 8, None),
    ("white", 3, WIDE - 1 + 600, WIDE - 1, 300, 8, None),
    ("walk", 3, WIDE + 600, WIDE, 300, 8, None),
    ("offset", 3, WIDE + 1 + 600, WIDE + 1, 300, 8, None),
    ("walk", 3, 3600, 1000, 1300, 8, None),                  # gaps
    ("white", 1, 8192, 4096, 2000, 2, None),
    ("walk", 3, 8192, 4096, 2000, 8, None),
    ("offset", 1, 8192, 4096, 2000, 64, None),
    ("walk", 3, 2000, 1000, 1000, 8, (4, 500)),              # n = 4 and n = W // 2
    ("offset", 3, 2000, 1000, 1000, 8, SCALES_32),           # tails (7, 9, 333 ..); 1, 2, 4 .. 64 lanes a box
    ("white", 1, 4096, 4096, 4096, 8, (4, 127, 128, 2048)),
    ("white", 3, 500, 250, 250, 8, (4, 63, 64, 65, 125)),    # one wave: 1, 16 and 32 lanes a box
)
assert len(SCALES_32) == 32 and all(b > a for a, b in zip(SCALES_32, SCALES_32[1:]))


@lru_cache(maxsize=None)
def gpu_reference(case, dtype=np.longdouble):
    """``window_fractals`` of GPU_CASES[case] in ``dtype``, computed once.  Read-only."""
    kind, C, N, W, step, kmax, scales = GPU_CASES[case]
    ref = window_fractals(gpu_signal(kind, C, N), W, step, kmax, scales, dtype)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@lru_cache(maxsize=None)
def gpu_bounds():
    """name -> (E, 32 E) over GPU_CASES: the error of the float64 restatement against the
    long-double one, relative to F for the fluctuations, absolute for the rest."""
    E = dict.fromkeys(CONTINUOUS, 0.0)
    for case in range(len(GPU_CASES)):
        lo, hi = gpu_reference(case, np.float64), gpu_reference(case)
        for name in CONTINUOUS:
            if name in hi:
                assert np.all(np.isfinite(hi[name])), (case, name)
                err = np.abs(lo[name] - hi[name]) / (np.abs(hi[name]) if name == "dfa_fluctuations" else 1)
                E[name] = max(E[name], float(np.max(err)))
    return {name: (e, MARGIN * e) for name, e in E.items()}


def test_names_are_public():
    assert features.window_fractal is window_fractal and features.dfa_scales is dfa_scales
    assert features.WINDOW_FRACTALS == fractal.WINDOW_FRACTALS == NAMES == tuple(_lib.WINDOW_FRACTAL)
    assert list(_lib.WINDOW_FRACTAL.values()) == list(range(5))
    assert fractal.window_plan is windowed.window_plan and fractal._advance is windowed._advance
    assert fractal.window_count is windowed.window_count
    doc = window_fractal.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name


def test_closed_forms_of_the_dimensions():
    for W in (16, 100, 1000):
        line = one(3.0 + 0.25 * np.arange(W), kmax=8, scales=(4, 5, 8))
        assert line["higuchi"] == pytest.approx(1.0, abs=1e-13) and line["katz"] == pytest.approx(1.0, abs=1e-14)
        assert line["petrosian"] == 1.0
        alt = (-1.0) ** np.arange(W)
        assert petrosian_count(alt) == W - 2
        assert one(alt, scales=(4, 8))["petrosian"] == np.log10(W) / (np.log10(W) + np.log10(W / (W + 0.4 * (W - 2))))
    assert petrosian_count(np.array([0.0, 1.0, 1.0, 0.0, 0.0, -1.0, -1.0, -2.0])) == 0   # a zero difference is no sign
    assert petrosian_count(np.array([0.0, 1.0, 0.5, 0.5, 2.0, 1.0, 3.0, 4.0])) == 3
    # higuchi from the double loop of the definition, n_mk of 1 and 2 only
    rng = np.random.default_rng(9)
    w = rng.standard_normal(32)
    u, v = [], []
    for k in range(1, 17):
        Lk = 0.0
        for m in range(k):
            n = (31 - m) // k
            assert n in (1, 2) or k < 11
            Lk += sum(abs(w[m + i * k] - w[m + (i - 1) * k]) for i in range(1, n + 1)) * 31 / (n * k) / k
        u.append(np.log(1 / k))
        v.append(np.log(Lk / k))
    assert one(w, kmax=16)["higuchi"] == pytest.approx(np.polyfit(u, v, 1)[0], abs=1e-13)


def test_closed_form_of_dfa_on_a_ramp():
    # x_t = a t + b: the profile is a parabola of curvature a / 2, whose residual about its
    # least-squares line over n points has the mean square (a / 2)^2 (n^2 - 1)(n^2 - 4) / 180
    a, W = 0.75, 960
    scales = (4, 5, 6, 8, 10, 12, 15, 16, 20, 24, 30, 32, 40, 48, 60, 64, 80, 96, 120, 160, 240, 480)
    assert all(W % n == 0 for n in scales)
    got = one(a * np.arange(W) - 7.0, scales=scales, dtype=np.longdouble)
    want = np.array([(a / 2) ** 2 * (n * n - 1) * (n * n - 4) / 180 for n in scales])
    assert np.max(np.abs(got["dfa_fluctuations"] ** 2 / want - 1)) < 1e-12
    assert 2.0 < got["dfa"] < 2.05                           # (n^2 - 1)(n^2 - 4) < n^4: from above
    big = one(a * np.arange(4096.0), scales=(256, 512, 1024, 2048))
    assert big["dfa"] == pytest.approx(2.0, abs=1e-4)


def test_noise_and_its_walk_have_the_textbook_exponents():
    x = np.random.default_rng(77).standard_normal(4096)
    white, walk = one(x), one(np.cumsum(x))
    assert abs(white["higuchi"] - 2) < 0.05 and abs(white["dfa"] - 0.5) < 0.1
    assert abs(walk["higuchi"] - 1.5) < 0.1 and abs(walk["dfa"] - 1.5) < 0.1
    assert white["dfa_fluctuations"].shape == (16,) and np.all(np.diff(white["dfa_fluctuations"]) > 0)
    assert 1 < white["katz"] and 1 < white["petrosian"] < 1.1


def test_a_constant_window():
    got = one(np.full(64, 2.5))
    assert np.isnan(got["katz"]) and np.isnan(got["higuchi"]) and np.isnan(got["dfa"])
    assert np.all(got["dfa_fluctuations"] == 0) and got["petrosian"] == 1.0
    # one L(k) = 0 among positive ones is NaN too: x_t = x_{t+2}
    assert np.isnan(one(np.tile([1.0, 3.0], 16), kmax=2)["higuchi"])


def test_dfa_scales():
    for W in (32, 64, 250, 1000, 4096):
        ns = dfa_scales(W)
        assert isinstance(ns, tuple) and all(isinstance(n, int) for n in ns)
        assert ns[0] == 4 and ns[-1] == W // 4 and len(ns) >= 2 and all(b > a for a, b in zip(ns, ns[1:]))
    assert dfa_scales(4096) == (4, 6, 8, 12, 18, 25, 37, 53, 77, 111, 161, 233, 338, 489, 708, 1024)
    assert dfa_scales(4096, 2) == (4, 1024) and len(dfa_scales(4096, 32)) == 32
    for bad in ({"winsize": 31}, {"winsize": 64.0}, {"winsize": 64, "count": 1}, {"winsize": 64, "count": 33}):
        with pytest.raises(ValueError, match="dfa_scales"):
            dfa_scales(**bad)


def test_non_finite_rule_of_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 600))
    clean = window_fractals(x, 100, 50)
    y = x.copy()
    y[0, 170] = np.nan
    y[1, 590:] = np.inf
    M = window_fractals(y, 100, 50)
    k = np.arange(11)
    hit = np.stack([(k * 50 <= 170) & (170 < k * 50 + 100), k * 50 + 100 > 590])
    assert hit[0].sum() == 2 and hit[1].sum() == 1
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), np.broadcast_to(hit, M[name].shape)), name
        assert np.array_equal(M[name][..., ~hit], clean[name][..., ~hit]), name


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_fractal(x + 1j * x, 100)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_fractal(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_fractal(x, 501)
    longest = _lib.WR_LONGEST
    cases = (({"winsize": 7}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": longest + 1}, f"winsize.*{longest}"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "kmax": 1}, "kmax"), ({"winsize": 100, "kmax": 65}, "kmax"),
             ({"winsize": 100, "kmax": 8.0}, "kmax"), ({"winsize": 100, "kmax": 8, "measures": "katz", "step": 0}, "step"),
             ({"winsize": 15, "kmax": 8, "measures": "higuchi"}, "2 kmax"),
             ({"winsize": 100, "kmax": 51, "measures": ("katz", "higuchi")}, "2 kmax"),
             ({"winsize": 100, "scales": (4,)}, "from 2 to 32"), ({"winsize": 8, "scales": (4,), "kmax": 4}, "from 2 to 32"),
             ({"winsize": 100, "scales": ()}, "from 2 to 32"),
             ({"winsize": 4096, "scales": tuple(range(4, 37))}, "from 2 to 32"),
             ({"winsize": 100, "scales": (3, 10)}, "scale"), ({"winsize": 100, "scales": (4, 51)}, "scale.*50"),
             ({"winsize": 100, "scales": (4, 10.0)}, "scale"), ({"winsize": 100, "scales": (4, True)}, "scale"),
             ({"winsize": 100, "scales": (10, 4)}, "strictly increasing"),
             ({"winsize": 100, "scales": (4, 10, 10)}, "strictly increasing"),
             ({"winsize": 100, "scales": 10, "measures": "dfa_fluctuations"}, "sequence"),
             ({"winsize": 100, "scales": "4,10"}, "sequence"),
             ({"winsize": 31, "measures": "dfa"}, "winsize >= 32"),
             ({"winsize": 16, "kmax": 8, "measures": ("higuchi", "dfa_fluctuations")}, "winsize >= 32"),
             ({"winsize": 100, "measures": "hurst"}, "higuchi.*dfa"),
             ({"winsize": 100, "measures": ("higuchi", "DFA")}, "DFA.*higuchi"),
             ({"winsize": 100, "measures": ()}, "higuchi"), ({"winsize": 100, "measures": 3}, "higuchi"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_fractal(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_fractal(x, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_fractal(src.pro, 100, measures=NAMES)
        assert not src.started

    # scales and kmax are read only with the measure that takes them: these pass the checks and
    # reach the device, which this test runs without (or the stream's first chunk, which is complex)
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    for kwargs in ({}, {"measures": "katz", "scales": (3,), "winsize": 8}, {"measures": "dfa", "kmax": 60}):
        with pytest.raises(ValueError, match="real data.*complex128 chunks"):
            window_fractal(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), **{"winsize": 100, **kwargs})
    with pytest.raises(TypeError):
        window_fractal(x, 100, fs=100)                                    # no such argument


C_TYPES = {"void *": ctypes.c_void_p, "double *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "const int *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}


def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint osz_window_fractal\(([^)]*)\);", header)
    assert m, "osz_window_fractal is not declared"
    declared = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()       # drop the name
        declared.append(C_TYPES[ctype])
    restype, argtypes = _lib.SIGNATURES["osz_window_fractal"]
    assert restype is ctypes.c_int and len(declared) == 15
    assert argtypes == declared, (argtypes, declared)
    assert hasattr(lib, "osz_window_fractal"), "osz_window_fractal not exported"
    for name, value in _lib.WINDOW_FRACTAL.items():
        assert re.search(rf"OSZ_WR_{name.upper()} = {value}\b", header), name
    assert re.search(r"typedef enum \{[^}]*OSZ_WR_COUNT = 5\s*\} osz_window_fractal_measure;", header)
    for name in ("LONGEST", "WIDE", "KMAX", "SCALES"):
        assert re.search(rf"#define OSZ_WR_{name} {getattr(_lib, 'WR_' + name)}\b", header), name
    assert (_lib.WR_LONGEST, _lib.WR_KMAX, _lib.WR_SCALES) == (4096, 64, 32)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowfrac\.hip\b", makefile, re.M)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_fractal_kernels_use_no_scratch(tmp_path):
    """Both instances of the kernel of windowfrac.hip, compiled for gfx950 with the library's flags:
    no scratch, no spilled VGPR or SGPR.  The register counts are printed, not fixed."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowfrac.hip"), "-o", str(tmp_path / "windowfrac.o"),
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
    assert len(kernels) == 2 and all("window_fractal_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert use["Dynamic Stack"] == "False"


def test_the_bound_of_the_gpu_test():
    bounds = gpu_bounds()
    for name in CONTINUOUS:
        E, bound = bounds[name]
        print(f"E[{name}] = {E:.2e}, bound {bound:.2e}")
        assert 0 < bound == MARGIN * E <= 1e-11, (name, E)
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs an 80-bit long double"
