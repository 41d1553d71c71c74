"""CPU-only tests of bispectrum / bicoherence (K14): the names, the argument errors (raised with
no GPU and before the stream is touched), the C ABI of the entry points against the header, the
register report of csrc/bispec.hip (no scratch in any kernel), and ``bispectral_sums``, the NumPy
restatement of the definition that tests/test_gpu_bispec.py compares the device against.  The
restatement is pinned here: against a triple Python loop over (segment, k1, k2), its sum |X|^2
against scipy.signal.csd's auto-spectrum, the ranges and the ordering of the two bicoherences,
and quadratic phase coupling: three tones at k1, k2 and k1 + k2 whose third phase is the sum of
the other two in every record (bicoherence near 1) or drawn by itself (near 0)."""

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
from openseize_amd.spectra import estimators
from openseize_amd.spectra.estimators import bicoherence, bispectrum

from test_csd_host import Untouched, rate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("kim", "hagihira")
RTOL = 1e-9          # the suite's cap on a bound (tests/test_gpu_parity.py)


def segment_spectra(x, fs, nfft, window, overlap, detrend, scaling):
    """X (segments, C, nfft // 2 + 1): the spectra ``csd`` sums -- every segment detrended,
    windowed, ``rfft``, times the square root of the scaling's norm.  x: (C, samples)."""
    stride = nfft - int(nfft * overlap)
    nseg = (x.shape[1] - nfft) // stride + 1
    win = sps.get_window(window, nfft)
    norm = 1 / (fs * np.sum(win ** 2)) if scaling == "density" else 1 / np.sum(win) ** 2
    X = np.empty((nseg, x.shape[0], nfft // 2 + 1), dtype=complex)
    for s in range(nseg):
        seg = x[:, s * stride:s * stride + nfft]
        if np.all(np.isfinite(seg)) or detrend == "linear":
            seg = sps.detrend(seg, type=detrend, axis=-1)
        else:
            seg = seg - seg.mean(axis=-1, keepdims=True)      # (NaN goes through a mean)
        X[s] = np.fft.rfft(seg * win, axis=-1) * np.sqrt(norm)
    return X


def gather_sums(X, k_lo, nb):
    """The four sums of the band k_lo .. k_lo + nb - 1 from segment spectra X (S, C, nfreq), by a
    vectorised gather: ``T`` = sum X1 X2 conj(X3) (C, nb, nb) complex, ``P12`` = sum |X1 X2|^2,
    ``A`` = sum |T| = sum |X1| |X2| |X3|, all NaN where k1 + k2 > nfreq - 1; ``power`` = sum |X|^2
    (C, nfreq); ``inside`` (nb, nb) the domain; ``cnt``."""
    nseg, nch, nfreq = X.shape
    k = k_lo + np.arange(nb)
    k3 = k[:, None] + k[None, :]
    inside = k3 <= nfreq - 1
    k3c = np.minimum(k3, nfreq - 1)
    T = np.zeros((nch, nb, nb), dtype=complex)
    P12, A = np.zeros((nch, nb, nb)), np.zeros((nch, nb, nb))
    for c in range(nch):
        for s in range(nseg):
            row = X[s, c]
            p = row[k][:, None] * row[k][None, :]
            t = p * np.conj(row[k3c])
            T[c] += t
            P12[c] += np.abs(p) ** 2
            A[c] += np.abs(row[k])[:, None] * np.abs(row[k])[None, :] * np.abs(row[k3c])
    for arr in (T, P12, A):
        arr[:, ~inside] = np.nan
    return {"T": T, "P12": P12, "A": A, "power": np.sum(np.abs(X) ** 2, axis=0), "inside": inside,
            "cnt": nseg, "k_lo": k_lo, "nb": nb}


def bispectral_sums(x, fs, nfft, window, overlap, detrend, scaling, k_lo, nb):
    """The definition: ``gather_sums`` of ``segment_spectra``, plus ``freqs`` of the band."""
    sums = gather_sums(segment_spectra(x, fs, nfft, window, overlap, detrend, scaling), k_lo, nb)
    sums["freqs"] = np.fft.rfftfreq(nfft, 1 / fs)[k_lo:k_lo + nb]
    return sums


def measures(sums):
    """(B, kim, hagihira, P3) of the sums: the mean bispectrum, the two bicoherences and
    sum |X3|^2 gathered at k1 + k2 (NaN outside the domain)."""
    k = sums["k_lo"] + np.arange(sums["nb"])
    k3 = np.minimum(k[:, None] + k[None, :], sums["power"].shape[1] - 1)
    P3 = np.where(sums["inside"], sums["power"][:, k3], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        kim = np.abs(sums["T"]) ** 2 / (sums["P12"] * P3)
        hag = np.abs(sums["T"]) / sums["A"]
    return sums["T"] / sums["cnt"], kim, hag, P3


def records(nrec, nfft, coupled, seed, k1, k2, noise):
    """nrec records of nfft samples, concatenated: each cos(k1) + cos(k2) + cos(k1 + k2) (bins of
    the record) with phases drawn uniformly per record -- the third the sum of the other two if
    ``coupled``, drawn by itself otherwise -- plus Gaussian noise of standard deviation ``noise``.
    At overlap 0 the segments are the records."""
    rng = np.random.default_rng(seed)
    n = np.arange(nfft)
    out = np.empty((nrec, nfft))
    for r in range(nrec):
        p1, p2, p3 = rng.uniform(0, 2 * np.pi, 3)
        if coupled:
            p3 = p1 + p2
        out[r] = (np.cos(2 * np.pi * k1 * n / nfft + p1) + np.cos(2 * np.pi * k2 * n / nfft + p2)
                  + np.cos(2 * np.pi * (k1 + k2) * n / nfft + p3) + noise * rng.standard_normal(nfft))
    return out.reshape(-1)


def tones(nfft):
    return max(3, nfft // 14), max(5, nfft // 9)


@lru_cache(maxsize=None)
def three_channels(nfft, nrec, noise, seed=0):
    """(3, nrec nfft): a coupled channel, an uncoupled one and noise alone.  Read-only (shared)."""
    k1, k2 = tones(nfft)
    x = np.stack([records(nrec, nfft, True, seed, k1, k2, noise), records(nrec, nfft, False, seed + 1, k1, k2, noise),
                  noise * np.random.default_rng(seed + 2).standard_normal(nrec * nfft)])
    x.setflags(write=False)
    return x


def test_names_are_public():
    assert callable(estimators.bispectrum) and callable(estimators.bicoherence)
    assert estimators.BICOHERENCE_METHODS == METHODS
    assert tuple(_lib.BISPEC_MODE) == ("spectrum",) + METHODS and list(_lib.BISPEC_MODE.values()) == [0, 1, 2]
    for name in METHODS:
        assert f'"{name}"' in bicoherence.__doc__
    assert "Kim" in bicoherence.__doc__ and "Hagihira" in bicoherence.__doc__
    assert "fmax" in bispectrum.__doc__ and "MemoryError" in bispectrum.__doc__


def test_restatement_is_the_triple_loop():
    nfft, nch, nseg, k_lo, nb = 16, 2, 5, 1, 8
    fs, _ = rate(nfft)
    x = np.random.default_rng(2).standard_normal((nch, nfft * nseg)) + 0.5
    X = segment_spectra(x, fs, nfft, "hann", 0.0, "constant", "density")
    assert X.shape == (nseg, nch, 9)
    got = gather_sums(X, k_lo, nb)
    T = np.full((nch, nb, nb), np.nan, dtype=complex)
    P12, A = np.full((nch, nb, nb), np.nan), np.full((nch, nb, nb), np.nan)
    for c in range(nch):
        for a in range(nb):
            for b in range(nb):
                k1, k2 = k_lo + a, k_lo + b
                if k1 + k2 > nfft // 2:
                    continue
                T[c, a, b], P12[c, a, b], A[c, a, b] = 0, 0, 0
                for s in range(nseg):
                    t = X[s, c, k1] * X[s, c, k2] * np.conj(X[s, c, k1 + k2])
                    T[c, a, b] += t
                    P12[c, a, b] += abs(X[s, c, k1] * X[s, c, k2]) ** 2
                    A[c, a, b] += abs(t)
    inside = got["inside"]
    assert np.array_equal(np.isnan(T[0].real), ~inside) and inside.sum() == 28 and got["cnt"] == nseg
    for name, want in (("T", T), ("P12", P12), ("A", A)):
        assert np.array_equal(np.isnan(got[name]), np.isnan(want)), name
        scale = np.nanmax(np.abs(want))
        assert np.nanmax(np.abs(got[name] - want)) < 1e-13 * scale, name


@pytest.mark.parametrize("nfft, window, overlap, detrend, scaling",
                         [(128, "hann", 0.5, "constant", "density"), (250, "hamming", 0.25, "linear", "spectrum")])
def test_restatement_power_is_scipy_autospectrum(nfft, window, overlap, detrend, scaling):
    fs, _ = rate(nfft)
    x = np.random.default_rng(3).standard_normal((2, 12 * nfft)) + 2.0
    sums = bispectral_sums(x, fs, nfft, window, overlap, detrend, scaling, 1, nfft // 2)
    for c in range(2):
        f, pxx = sps.csd(x[c], x[c], fs=fs, window=window, nperseg=nfft, noverlap=int(nfft * overlap), nfft=nfft,
                         detrend=detrend, scaling=scaling, return_onesided=False)
        half = pxx[:nfft // 2 + 1].real                       # (two-sided: no doubling, as in X)
        got = sums["power"][c] / sums["cnt"]
        assert np.max(np.abs(got - half)) < RTOL * np.max(half)
    assert np.array_equal(sums["freqs"], np.fft.rfftfreq(nfft, 1 / fs)[1:nfft // 2 + 1])


def test_ranges_symmetry_and_ordering():
    """0 <= kim, hagihira <= 1 (Cauchy-Schwarz, the triangle inequality), both symmetric, and
    kim <= hagihira^2: (sum |T|)^2 <= sum |X1 X2|^2 sum |X3|^2."""
    nfft = 128
    fs, _ = rate(nfft)
    x = three_channels(nfft, 24, 0.5)
    sums = bispectral_sums(x, fs, nfft, "hann", 0.5, "constant", "density", 1, 64)
    B, kim, hag, _ = measures(sums)
    inside = sums["inside"]
    assert inside.sum() == 63 * 64 // 2 and not inside[-1, -1] and inside[0, 62] and not inside[0, 63]
    for M in (kim, hag):
        assert np.array_equal(np.isnan(M), np.broadcast_to(~inside, M.shape))
        assert np.all(M[:, inside] >= 0) and np.all(M[:, inside] <= 1 + 1e-12)
        assert np.allclose(M, M.transpose(0, 2, 1), rtol=1e-12, atol=0, equal_nan=True)      # (NumPy's products: not the bits)
    assert np.allclose(B[:, inside], B.transpose(0, 2, 1)[:, inside], rtol=1e-13, atol=0)
    assert np.all(kim[:, inside] <= hag[:, inside] ** 2 * (1 + 1e-12))


@pytest.mark.parametrize("nfft, nrec", [(128, 24), (64, 32), (256, 16)])
def test_quadratic_phase_coupling(nfft, nrec):
    """kim at (k1, k2) = (9, 14), noise 0.5: 0.975 coupled / 0.002 uncoupled at nfft 128 with 24
    records, 0.939 / 0.062 at 64 with 32, 0.978 / 0.005 at 256 with 16."""
    k1, k2 = 9, 14
    fs, _ = rate(nfft)
    x = np.stack([records(nrec, nfft, True, 0, k1, k2, 0.5), records(nrec, nfft, False, 1, k1, k2, 0.5)])
    sums = bispectral_sums(x, fs, nfft, "hann", 0.0, "constant", "density", 1, nfft // 4)
    assert sums["cnt"] == nrec
    _, kim, hag, _ = measures(sums)
    print(nfft, float(kim[0, k2 - 1, k1 - 1]), float(kim[1, k2 - 1, k1 - 1]), float(hag[0, k2 - 1, k1 - 1]))
    assert kim[0, k2 - 1, k1 - 1] > 0.9 and kim[0, k1 - 1, k2 - 1] > 0.9
    assert kim[1, k2 - 1, k1 - 1] < 0.3
    assert hag[0, k2 - 1, k1 - 1] > 0.9


@pytest.mark.parametrize("func", [bispectrum, bicoherence])
def test_argument_errors_come_before_the_stream(func):
    cases = [({"detrend": "quadratic"}, "Trend type"),
             ({"resolution": 0.01}, "nfft"),                              # nfft 10000 > 5000 samples
             ({"fmin": 30.0, "fmax": 20.0}, "fmin.*fmax"),
             ({"fmin": 20.1, "fmax": 20.2}, "no bin"),                    # between two bins
             ({"fmin": 60.0}, "no bin"),                                  # above Nyquist
             ({"fmax": 0.0}, "no bin")]                                   # DC alone, which fmin=None leaves out
    if func is bicoherence:
        cases += [({"method": "coherence"}, "kim.*hagihira"), ({"method": ("kim", "Kim")}, "Kim.*kim"),
                  ({"method": ()}, "kim"), ({"method": 3}, "kim")]
    else:
        cases += [({"scaling": "power"}, "Unknown scaling")]
    for kwargs, match in cases:
        for shape in ((4, 5000), (5000,)):
            src = Untouched(shape)
            with pytest.raises(ValueError, match=match):
                func(src.pro, fs=100, **kwargs)
            assert not src.started, kwargs
    src = Untouched((2, 2, 5000))
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        func(src.pro, fs=100)
    assert not src.started
    with pytest.raises(ValueError, match="two-dimensional"):
        func(np.zeros((2, 3, 5000)), fs=100)
    if func is bicoherence:
        with pytest.raises(TypeError):
            func(Untouched((4, 5000)).pro, fs=100, scaling="density")     # it cancels: no such argument


def test_band_selection():
    plan = estimators._BispecPlan(100.0, 0.5, None, None, 16)
    assert (plan.k_lo, plan.nb) == (1, 100) and np.array_equal(plan.freqs, np.arange(1, 101) * 0.5)
    plan = estimators._BispecPlan(100.0, 0.5, 0, 10.0, 16)
    assert (plan.k_lo, plan.nb) == (0, 21) and plan.freqs[0] == 0.0 and plan.freqs[-1] == 10.0
    plan = estimators._BispecPlan(100.0, 0.5, 3.2, 10.3, 16)
    assert (plan.k_lo, plan.nb) == (7, 14)                                # 3.5 .. 10.0 Hz
    plan = estimators._BispecPlan(100.0, 0.5, 4.0, 4.0, 8)
    assert (plan.k_lo, plan.nb) == (8, 1)
    assert plan.push_bytes == 24


def test_host_result_that_does_not_fit_is_refused(monkeypatch):
    monkeypatch.setattr(estimators, "assignable", lambda *a, **k: False)
    for func in (bispectrum, bicoherence):
        with pytest.raises(MemoryError, match="fmax.*fewer channels"):
            func(np.zeros((4, 5000)), fs=100)                             # (no device is asked for before it)


C_TYPES = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "const double *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_bispec_work", "int64_t", 3), ("osz_bispec_accumulate", "int", 11),
                             ("osz_bispec_finish", "int", 10)):
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
    for k, (name, value) in enumerate(_lib.BISPEC_MODE.items()):
        assert value == k and re.search(rf"OSZ_BISPEC_{name.upper()} = {k}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bbispec\.hip\b", makefile, re.M)
    # the work-space query needs no device: the plane |X| of a push
    lib.osz_bispec_work.restype, lib.osz_bispec_work.argtypes = _lib.SIGNATURES["osz_bispec_work"]
    assert lib.osz_bispec_work(7, 3, 131) == 7 * 3 * 131 and lib.osz_bispec_work(0, 1, 1) == 0
    assert lib.osz_bispec_work(-1, 3, 131) == -1 and lib.osz_bispec_work(7, 0, 131) == -1
    assert lib.osz_bispec_work(7, 3, 0) == -1 and lib.osz_bispec_work(1, 1 << 14, 1 << 13) == -1


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_bispec_kernels_use_no_scratch(tmp_path):
    """Every kernel of bispec.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled VGPR (the rows of a wave's register tile are chosen for that)."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "bispec.hip"), "-o", str(tmp_path / "bispec.o"),
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
    assert len(kernels) == 3, sorted(kernels)                  # prepare, accumulate, finish
    for want in ("bispec_prepare_kernel", "bispec_accumulate_kernel", "bispec_finish_kernel"):
        assert any(want in k for k in kernels), want
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 512
