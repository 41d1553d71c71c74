"""CPU-only tests of analytic_connectivity (K13): the names, the argument errors (raised with no
GPU and before the stream is touched), the C ABI of the entry points against the header, the
register report of csrc/pairtime.hip (no scratch in any kernel), and ``analytic_measures``, the
NumPy restatement of the five definitions that tests/test_gpu_analytic.py compares the device
against.  The restatement is pinned here: its aec against np.corrcoef of the envelopes, the
invariances under scaling, rotating and swapping channels, a zero-lag mixture (aec and plv high,
the orthogonalised and lag measures near 0: the reason those exist), and a pure delay of a
narrow-band signal (plv and wpli near 1)."""

import ctypes
import os
import re
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest
import scipy.signal as sps

from openseize_amd import _lib
from openseize_amd.experimental import coupling
from openseize_amd.experimental.coupling import connectivity
from openseize_amd.experimental.coupling.connectivity import analytic_connectivity

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("aec", "oaec", "plv", "ciplv", "wpli")
RTOL = 1e-9          # the suite's cap on a bound (tests/test_gpu_parity.py)
FS = 250.0


PAD = 1000           # samples cut from both ends: the transients of the band-pass and of the Hilbert transform


def band_noise(nch, n, seed, band=(8.0, 30.0)):
    """nch independent band-passed (zero-phase Butterworth) white noises at FS, n + 2 PAD samples."""
    sos = sps.butter(4, band, "bandpass", fs=FS, output="sos")
    return sps.sosfiltfilt(sos, np.random.default_rng(seed).standard_normal((nch, n + 2 * PAD)), axis=-1)


@lru_cache(maxsize=None)
def mixture(nch, n=8192, seed=0):
    """The analytic signals of x_0, x_0 + 0.5 x_1, x_2, ..., x_k independent 8-30 Hz noises at
    250 Hz, n samples from the middle of n + 2 PAD: channel 1 is a zero-lag mixture with channel 0.
    Read-only (shared between tests)."""
    x = band_noise(nch, n, seed)
    x[1] = x[0] + 0.5 * x[1]
    z = np.ascontiguousarray(sps.hilbert(x, axis=-1)[:, PAD:PAD + n])
    z.setflags(write=False)
    return z


def analytic_measures(z):
    """The definitions: (M, parts) for z (C, N) complex.  M maps each of METHODS to its (C, C)
    array with the fixed points of ``analytic_connectivity`` on the diagonal; the two
    correlations are np.corrcoef pair by pair.  ``parts`` holds what the GPU tests build their
    bounds from: ``N``; per channel ``A`` = sum a and ``Q`` = sum a^2; per ordered pair ``Saa`` =
    sum a_i a_j, ``Sm`` = sum m, ``Sb`` / ``Sbb`` = sum b / sum b^2 of b = m / a_i (the part of z_j
    orthogonal to z_i), ``raec`` and ``rorth`` = r(a_i, a_j) and r(a_i, b), and ``R`` / ``I`` = the
    real and imaginary part of s = sum conj(u_i) u_j / N."""
    nch, n = z.shape
    a = np.abs(z)
    u = z / a
    M = {name: np.zeros((nch, nch)) for name in METHODS}
    keys = ("Saa", "Sm", "Sb", "Sbb", "raec", "rorth", "R", "I")
    parts = {k: np.zeros((nch, nch)) for k in keys}
    parts.update(N=n, A=a.sum(axis=1), Q=(a * a).sum(axis=1))
    for i in range(nch):
        for j in range(nch):
            d = (np.conj(z[i]) * z[j]).imag
            m = np.abs(d)
            b = m / a[i]
            s = np.sum(np.conj(u[i]) * u[j]) / n
            parts["Saa"][i, j] = np.sum(a[i] * a[j])
            parts["Sm"][i, j] = np.sum(m)
            parts["Sb"][i, j] = np.sum(b)
            parts["Sbb"][i, j] = np.sum(b * b)
            parts["R"][i, j], parts["I"][i, j] = s.real, s.imag
            if i == j:
                continue
            parts["raec"][i, j] = np.corrcoef(a[i], a[j])[0, 1]
            parts["rorth"][i, j] = np.corrcoef(a[i], b)[0, 1]
            M["plv"][i, j] = np.abs(s)
            M["ciplv"][i, j] = np.abs(s.imag) / np.sqrt(1 - s.real ** 2)
            M["wpli"][i, j] = np.abs(np.sum(d)) / np.sum(m)
    M["aec"] = parts["raec"].copy()
    M["oaec"] = (parts["rorth"] + parts["rorth"].T) / 2
    eye = np.eye(nch, dtype=bool)
    for name in METHODS:
        M[name][eye] = 1.0 if name in ("aec", "plv") else 0.0
    return M, parts


def pearson_bound(tau, n, sp, sq, spp, sqq, spq_abs, r):
    """First-order bound on the error of a Pearson r computed from the five sums when every sum
    is off by at most tau times the sum of its terms' magnitudes."""
    dcov = tau * (spq_abs + 2 * np.abs(sp * sq) / n)
    dvp, dvq = tau * (spp + 2 * sp ** 2 / n), tau * (sqq + 2 * sq ** 2 / n)
    vp, vq = spp - sp ** 2 / n, sqq - sq ** 2 / n
    return dcov / np.sqrt(vp * vq) + np.abs(r) * (dvp / vp + dvq / vq) / 2


def bounds(parts):
    """name -> (C, C) bound on |device - yardstick| for the same complex128 input, from
    tau = (N + 16) 2^-53 (module docstring of tests/test_gpu_analytic.py)."""
    n = parts["N"]
    tau = (n + 16) * 2.0 ** -53
    A, Q = parts["A"], parts["Q"]
    with np.errstate(divide="ignore", invalid="ignore"):
        aec = pearson_bound(tau, n, A[:, None], A[None, :], Q[:, None], Q[None, :], parts["Saa"], parts["raec"])
        # r(a_i, b_{j|i}): p = a_i (row), q = b, sum |p q| = sum m
        orth = pearson_bound(tau, n, A[:, None], parts["Sb"], Q[:, None], parts["Sbb"], parts["Sm"], parts["rorth"])
        R, I = parts["R"], parts["I"]
        ciplv = tau * (1 / np.sqrt(1 - R ** 2) + np.abs(I) * np.abs(R) / (1 - R ** 2) ** 1.5)
    two = np.full_like(aec, 2 * tau)
    return {"aec": aec, "oaec": (orth + orth.T) / 2, "plv": two, "ciplv": ciplv, "wpli": two}


def test_names_are_public():
    assert callable(coupling.analytic_connectivity) and coupling.analytic_connectivity is analytic_connectivity
    assert coupling.ANALYTIC_METHODS == connectivity.ANALYTIC_METHODS == METHODS
    doc = analytic_connectivity.__doc__
    for name in METHODS:
        assert f'"{name}"' in doc
    assert "Hipp" in doc and "4096" in doc and connectivity._BLOCK == 4096
    assert tuple(_lib.ANALYTIC_MODE) == METHODS and list(_lib.ANALYTIC_MODE.values()) == [0, 1, 2, 3, 4]
    assert set(_lib.ANALYTIC_GROUP) == set(METHODS)


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    z = rng.standard_normal((4, 500)) + 1j * rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="build the analytic signal with `Analytic`"):
        analytic_connectivity(z.real)                                     # real data
    with pytest.raises(ValueError, match="two-dimensional"):
        analytic_connectivity(z[0])                                       # one channel
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        analytic_connectivity(z.reshape(2, 2, 500))
    for method, match in (("coherence", "aec.*oaec.*plv.*ciplv.*wpli"), (("wpli", "PLV"), "PLV.*aec"),
                          ((), "aec"), (3, "aec")):
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            analytic_connectivity(src.pro, method=method)
        assert not src.started, method
        with pytest.raises(ValueError, match=match):
            analytic_connectivity(z, method=method)
    for shape in ((5000,), (2, 2, 5000)):
        src = Untouched(shape)
        with pytest.raises(ValueError, match="two-dimensional"):
            analytic_connectivity(src.pro, method=METHODS)
        assert not src.started
    # a producer shows what it holds only with its first chunk: real chunks raise then, and
    # nothing has been asked of the device (this test runs without one)
    with pytest.raises(ValueError, match="build the analytic signal with `Analytic`"):
        analytic_connectivity(Untouched((4, 5000)).pro)
    with pytest.raises(TypeError):
        analytic_connectivity(z, fs=100)                                  # no such argument


C_TYPES = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "const double *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_analytic_work", "int64_t", 3), ("osz_analytic_accumulate", "int", 10),
                             ("osz_analytic_finish", "int", 8)):
        m = re.search(r"\b" + ret + " " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared"
        declared = []
        for arg in m.group(1).split(","):
            ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()   # drop the name
            declared.append(C_TYPES[ctype])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C_TYPES[ret] and len(declared) == nargs
        assert argtypes == declared, (name, argtypes, declared)
        assert hasattr(lib, name), f"{name} not exported"
    for k, (name, value) in enumerate(_lib.ANALYTIC_MODE.items()):
        assert value == k and re.search(rf"OSZ_ANALYTIC_{name.upper()} = {k}\b", header)
    for name in ("AMP", "ORTH", "LOCK", "LAG"):
        assert re.search(rf"OSZ_ANALYTIC_{name} = {getattr(_lib, 'ANALYTIC_' + name)}\b", header)
    assert re.search(rf"#define OSZ_ANALYTIC_BLOCK {connectivity._BLOCK}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bpairtime\.hip\b", makefile, re.M)
    # the work-space query needs no device
    lib.osz_analytic_work.restype, lib.osz_analytic_work.argtypes = _lib.SIGNATURES["osz_analytic_work"]
    assert lib.osz_analytic_work(3, 4097, 15) == 6 * 3 * 4097 + 2 * (10 * 9 + 3 * 3)
    assert lib.osz_analytic_work(3, 4096, _lib.ANALYTIC_LAG) == 6 * 3 * 4096 + (2 * 9 + 3 * 3)
    assert lib.osz_analytic_work(3, 10, 0) == -1 and lib.osz_analytic_work(3, 10, 16) == -1


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_pair_kernels_use_no_scratch(tmp_path):
    """Every kernel of pairtime.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled VGPR (the register tile of the widest sum group is sized for that)."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "pairtime.hip"), "-o", str(tmp_path / "pairtime.o"),
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
    pair = [k for k in kernels if "pair_accumulate_kernel" in k]
    assert len(pair) == 4 and len(kernels) == 7, sorted(kernels)       # one instance per sum group
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 512


def test_aec_is_corrcoef_of_the_envelopes():
    z = mixture(6)
    M, parts = analytic_measures(z)
    assert np.max(np.abs(M["aec"] - np.corrcoef(np.abs(z)))) < 1e-12
    for name in METHODS:
        assert np.all(np.isfinite(M[name])), name
    # Pearson r from the five sums, the form the device takes: the same number
    n, A, Q = parts["N"], parts["A"], parts["Q"]
    r = (n * parts["Saa"] - A[:, None] * A[None]) / np.sqrt((n * Q - A * A)[:, None] * (n * Q - A * A)[None])
    off = ~np.eye(6, dtype=bool)
    assert np.max(np.abs(r - M["aec"])[off]) < 1e-12
    b = bounds(parts)
    for name in METHODS:
        assert np.all(b[name][off] <= RTOL) and np.all(b[name][off] > 0), name


def test_invariances():
    """A positive real factor on a channel changes nothing; a rotation e^{i phi} of a channel
    leaves aec and plv alone; swapping two channels permutes the matrices."""
    z = np.array(mixture(4, 2048, seed=3))
    M, _ = analytic_measures(z)
    y = z.copy()
    y[1] *= 3.7
    y[3] *= 1e-3
    Ms, _ = analytic_measures(y)
    y = z.copy()
    y[2] = y[2] * np.exp(0.9j)
    Mr, _ = analytic_measures(y)
    perm = [2, 1, 0, 3]
    Mp, _ = analytic_measures(z[perm])
    for name in METHODS:
        assert np.max(np.abs(Ms[name] - M[name])) < 1e-10, name
        assert np.max(np.abs(M[name] - M[name].T)) < 1e-12, name
        assert np.max(np.abs(Mp[name] - M[name][np.ix_(perm, perm)])) < 1e-12, name
    for name in ("aec", "plv"):
        assert np.max(np.abs(Mr[name] - M[name])) < 1e-10, name
    assert np.max(np.abs(Mr["wpli"] - M["wpli"])[2]) > 1e-3                  # (the lag measures do move)


def test_zero_lag_mixture_is_what_the_orthogonalised_measures_remove():
    """aec 0.79 and plv 0.80 between x_0 and x_0 + 0.5 x_1; oaec -0.03, ciplv 0.01, wpli 0.01."""
    M, _ = analytic_measures(mixture(2))
    got = {name: M[name][0, 1] for name in METHODS}
    print({k: round(float(v), 3) for k, v in got.items()})
    assert got["aec"] > 0.7 and got["plv"] > 0.7
    for name in ("oaec", "ciplv", "wpli"):
        assert abs(got[name]) < 0.1, (name, got[name])


def test_pure_delay_of_a_narrow_band_signal_is_locked():
    """Channel 1 is channel 0 six samples later, 9-11 Hz at 250 Hz: a quarter cycle, the same
    phase difference at every sample up to the band's width: 2 pi 6 / 250 (f - 10) spans +-0.15 rad
    over the passband, for which plv = sin(0.15) / 0.15 = 0.996, and the filter's skirts span more."""
    n, delay = 8192, 6
    x = band_noise(1, n + delay, seed=5, band=(9.0, 11.0))[0]
    z = sps.hilbert(np.stack([x[delay:delay + n + 2 * PAD], x[:n + 2 * PAD]]), axis=-1)[:, PAD:-PAD]
    M, _ = analytic_measures(z)
    print({name: float(M[name][0, 1]) for name in METHODS})
    assert M["plv"][0, 1] > 0.98 and M["wpli"][0, 1] > 0.98 and M["ciplv"][0, 1] > 0.9
