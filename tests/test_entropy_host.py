"""CPU-only tests of window_entropy (K16): the names, the argument errors (raised with no GPU and
before the stream is touched), the C ABI of the entry point against the header, the register
report of csrc/windowent.hip (no scratch in any kernel), and ``window_entropies``, the NumPy
restatement of the definitions that tests/test_gpu_entropy.py compares the device against: the
brute-force pair matrix for sample entropy, stable ranks for permutation entropy.  The
restatement is pinned here on closed forms (a ramp, a constant, a monotone and an alternating
window, the tie rule, the two IEEE cases of -ln(A / B)) and on the rule for non-finite samples."""

import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from openseize_amd import _lib, features
from openseize_amd.features import entropy, windowed
from openseize_amd.features.entropy import window_entropy

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sample", "sample_a", "sample_b", "permutation")


def pair_distances(w):
    """|x_a - x_b| of one window, every pair."""
    return np.abs(w[:, None] - w[None, :])


def pair_matches(dist, rho):
    """(match, margin): |x_a - x_b| <= rho of every pair, and the least | |x_a - x_b| - rho | over
    all pairs relative to rho (inf for rho = 0; the pairs a = b hold it to 1 at the most)."""
    margin = np.inf
    if rho > 0:
        gap = np.subtract(dist, rho)
        margin = float(np.abs(gap, out=gap).min() / rho)
    return dist <= rho, margin


def sample_counts(match, m):
    """(A, B) of one window from its matching pairs: B the pairs i < j of the templates
    0 .. W - m - 1 that match over m samples, A over m + 1 (every template matches itself, and the
    matrix is symmetric)."""
    N = match.shape[0] - m
    both = match[:N, :N].copy()
    for k in range(1, m):
        both &= match[k:N + k, k:N + k]
    B = (int(both.sum()) - N) // 2
    both &= match[m:N + m, m:N + m]
    return (int(both.sum()) - N) // 2, B


def sample_entropy(A, B):
    """-ln(A / B) as IEEE arithmetic gives it: +inf for A = 0 < B, NaN for B = 0."""
    with np.errstate(all="ignore"):
        return -np.log(np.float64(A) / np.float64(B))


def permutation_entropy(w, order, delay, normalize):
    """-sum p log2 p of the rank patterns of one window; the rank of element k of a vector is the
    number of elements below it plus the equal ones before it (a stable sort)."""
    nvec = w.shape[0] - (order - 1) * delay
    vec = w[np.arange(nvec)[:, None] + delay * np.arange(order)[None, :]]
    ranks = np.argsort(np.argsort(vec, axis=1, kind="stable"), axis=1, kind="stable")
    _, counts = np.unique(ranks @ (order ** np.arange(order)), return_counts=True)
    p = counts / nvec
    h = -np.sum(p * np.log2(p))
    return h / np.log2(math.factorial(order)) if normalize else h


def window_entropies(x, W, step, m=2, r=0.2, tolerance="std", order=3, delay=1, normalize=True, margins=False):
    """The definitions: name -> (C, nwin) for x (C, N).  A window that holds a NaN or +-inf is NaN
    in every measure.  With ``margins`` also "margin": how close, relative to rho, the closest
    element difference of the window comes to rho."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1]
    nwin = 0 if n < W else (n - W) // step + 1
    out = {name: np.full((x.shape[0], nwin), np.nan) for name in NAMES + (("margin",) if margins else ())}
    for c in range(x.shape[0]):
        for k in range(nwin):
            w = x[c, k * step:k * step + W]
            if not np.all(np.isfinite(w)):
                continue
            rho = r * np.std(w) if tolerance == "std" else float(r)
            match, margin = pair_matches(pair_distances(w), rho)
            A, B = sample_counts(match, m)
            out["sample"][c, k] = sample_entropy(A, B)
            out["sample_a"][c, k], out["sample_b"][c, k] = A, B
            out["permutation"][c, k] = permutation_entropy(w, order, delay, normalize)
            if margins:
                out["margin"][c, k] = margin
    return out


def one(w, **kwargs):
    """The measures of one window as floats."""
    w = np.asarray(w, dtype=np.float64)
    return {name: float(v[0, 0]) for name, v in window_entropies(w, w.shape[0], 1, **kwargs).items()}


def test_names_are_public():
    assert features.window_entropy is window_entropy
    assert features.WINDOW_ENTROPIES == entropy.WINDOW_ENTROPIES == NAMES == tuple(_lib.WINDOW_ENTROPY)
    assert list(_lib.WINDOW_ENTROPY.values()) == list(range(4))
    assert entropy.window_plan is windowed.window_plan and entropy._advance is windowed._advance
    assert entropy.window_count is windowed.window_count
    doc = window_entropy.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name


def test_closed_forms_of_sample_entropy():
    ramp = np.arange(50.0)
    for r, want in ((1, 47), (2.5, 93)):
        got = one(ramp, m=2, r=r, tolerance="absolute")
        assert got["sample_a"] == got["sample_b"] == want and got["sample"] == 0
    const = one(np.full(40, 3.25), m=2, r=0.2)
    assert const["sample"] == 0 and const["sample_a"] == const["sample_b"] == 38 * 37 / 2
    assert const["permutation"] == 0
    # one pair of templates of length 1 matches, none of length 2: A = 0 < B
    got = one([0.0, 0.05, 5.0, 10.0, 20.0], m=1, r=0.1, tolerance="absolute")
    assert got["sample_a"] == 0 and got["sample_b"] == 1 and got["sample"] == np.inf
    got = one(np.arange(5.0), m=1, r=0.1, tolerance="absolute")
    assert got["sample_a"] == 0 and got["sample_b"] == 0 and np.isnan(got["sample"])
    # the last sample is compared as the m + 1-th of a template only: the templates end at W - m - 1
    got = one([0.0, 0.0, 0.0, 0.0, 9.0], m=1, r=0.5, tolerance="absolute")
    assert got["sample_b"] == 6 and got["sample_a"] == 3                  # templates 0 .. 3; pairs below 3
    # <= and the std with divisor W
    w = np.array([0.0, 2.0, 0.0, 2.0, 0.0, 2.0])
    assert np.std(w) == 1.0
    assert one(w, m=1, r=2.0)["sample_b"] == 10 and one(w, m=1, r=1.999)["sample_b"] == 4
    # against the double loop of the definition
    rng = np.random.default_rng(5)
    w = np.cumsum(rng.standard_normal(60))
    for m in (1, 2, 3):
        rho = 0.3 * np.std(w)
        N = 60 - m
        A = B = 0
        for i in range(N):
            for j in range(i + 1, N):
                if max(abs(w[i + k] - w[j + k]) for k in range(m)) <= rho:
                    B += 1
                    A += abs(w[i + m] - w[j + m]) <= rho
        got = one(w, m=m, r=0.3)
        assert (got["sample_a"], got["sample_b"]) == (A, B) and B > A > 0
        assert got["sample"] == -np.log(A / B)


def test_closed_forms_of_permutation_entropy():
    for order in (2, 3, 6):
        for delay in (1, 3):
            assert one(np.arange(40.0) ** 3, order=order, delay=delay)["permutation"] == 0
            assert one(-np.arange(40.0), order=order, delay=delay)["permutation"] == 0
    alt = (-1.0) ** np.arange(41)                            # 40 vectors, 20 rising and 20 falling
    assert one(alt, order=2)["permutation"] == 1.0
    assert one(alt, order=2, normalize=False)["permutation"] == 1.0
    assert one(alt, order=2, delay=2)["permutation"] == 0    # x_t = x_{t+2}: every vector a tie, one pattern
    # a tie goes to the earlier sample: (1, 1) ranks as rising
    assert one([1.0, 1.0, 2.0, 3.0], order=2)["permutation"] == 0
    assert one([3.0, 2.0, 2.0, 1.0], order=2)["permutation"] == pytest.approx(
        -(1 / 3 * np.log2(1 / 3) + 2 / 3 * np.log2(2 / 3)), abs=1e-15)
    # every pattern of order 3 once: log2 6 bits, 1 when normalised
    w = [0.0, 1.0, 2.0, 0.0, 3.0, 2.0, 0.0, 1.0]             # 012 120 203 032 320 201
    assert one(w, order=3, normalize=False)["permutation"] == pytest.approx(np.log2(6), abs=1e-15)
    assert one(w, order=3)["permutation"] == pytest.approx(1.0, abs=1e-15)


def test_non_finite_rule_of_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 600))
    clean = window_entropies(x, 100, 50)
    y = x.copy()
    y[0, 170] = np.nan
    y[1, 590:] = np.inf
    M = window_entropies(y, 100, 50)
    k = np.arange(11)
    hit = np.stack([(k * 50 <= 170) & (170 < k * 50 + 100), k * 50 + 100 > 590])
    assert hit[0].sum() == 2 and hit[1].sum() == 1
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), hit), name
        assert np.array_equal(M[name][~hit], clean[name][~hit]), name


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_entropy(x + 1j * x, 100)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_entropy(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_entropy(x, 501)
    longest = _lib.WE_LONGEST
    cases = (({"winsize": 3}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": longest + 1}, f"winsize.*{longest}"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "m": 0}, "m must"), ({"winsize": 100, "m": 9}, "m must"),
             ({"winsize": 100, "m": 2.0}, "m must"),
             ({"winsize": 100, "r": -0.1}, "r must"), ({"winsize": 100, "r": np.nan}, "r must"),
             ({"winsize": 100, "r": np.inf}, "r must"), ({"winsize": 100, "r": "0.2"}, "r must"),
             ({"winsize": 100, "tolerance": "sd"}, "tolerance.*std.*absolute"),
             ({"winsize": 100, "tolerance": None}, "tolerance"),
             ({"winsize": 100, "order": 1}, "order"), ({"winsize": 100, "order": 7}, "order"),
             ({"winsize": 100, "order": 3.0}, "order"),
             ({"winsize": 100, "delay": 0}, "delay"), ({"winsize": 100, "delay": 1.5}, "delay"),
             ({"winsize": 9, "m": 8, "measures": "sample_b"}, "m \\+ 2"),
             ({"winsize": 100, "order": 3, "delay": 50, "measures": "permutation"}, "order - 1"),
             ({"winsize": 100, "measures": "approximate"}, "sample.*permutation"),
             ({"winsize": 100, "measures": ("sample", "Permutation")}, "Permutation.*sample"),
             ({"winsize": 100, "measures": ()}, "sample"), ({"winsize": 100, "measures": 3}, "sample"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_entropy(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_entropy(x, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_entropy(src.pro, 100, measures=NAMES)
        assert not src.started

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device (this test runs without one)
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    with pytest.raises(ValueError, match="real data.*complex128 chunks"):
        window_entropy(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_entropy(x, 100, fs=100)                                    # no such argument


C_TYPES = {"void *": ctypes.c_void_p, "double *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}


def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint osz_window_entropy\(([^)]*)\);", header)
    assert m, "osz_window_entropy is not declared"
    declared = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()       # drop the name
        declared.append(C_TYPES[ctype])
    restype, argtypes = _lib.SIGNATURES["osz_window_entropy"]
    assert restype is ctypes.c_int and len(declared) == 18
    assert argtypes == declared, (argtypes, declared)
    assert hasattr(lib, "osz_window_entropy"), "osz_window_entropy not exported"
    for name, value in _lib.WINDOW_ENTROPY.items():
        assert re.search(rf"OSZ_WE_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WE_COUNT = 4\b", header)
    assert re.search(r"typedef enum \{[^}]*OSZ_WE_COUNT = 4\s*\} osz_window_entropy_measure;", header)
    assert re.search(rf"#define OSZ_WE_LONGEST {_lib.WE_LONGEST}\b", header)
    assert re.search(rf"#define OSZ_WE_WIDE {_lib.WE_WIDE}\b", header)
    for name, value in _lib.WE_TOLERANCE.items():
        assert re.search(rf"OSZ_WE_TOL_{name.upper()} = {value}\b", header), name
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowent\.hip\b", makefile, re.M)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_entropy_kernels_use_no_scratch(tmp_path):
    """Both instances of the kernel of windowent.hip, compiled for gfx950 with the library's flags:
    no scratch, no spilled VGPR, and registers for eight waves a SIMD."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowent.hip"), "-o", str(tmp_path / "windowent.o"),
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
    assert len(kernels) == 2 and all("window_entropy_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 64
