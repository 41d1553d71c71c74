"""CPU-only tests of window_connectivity (K19): the names, the argument errors (raised with no GPU
and before the stream is touched), the window bookkeeping across chunkings, the C ABI of the
entry points against the header, the register report of csrc/windowpair.hip (no scratch, no
spill in any kernel), and ``window_pair_measures``, the NumPy long-double restatement that
tests/test_gpu_connectivity.py compares the device against.  The restatement is pinned here
window by window against numpy.cov / numpy.corrcoef and, on a one-window stream, against
``analytic_measures`` of tests/test_analytic_host.py.  ``shifted_scheme`` restates the device's
arithmetic in float64 -- sums about each window's first sample, Pearson's r from the five sums,
the phasor Gram entries -- for the margin the GPU test's docstring quotes."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from openseize_amd import _device as dev
from openseize_amd import _lib, features, producer
from openseize_amd.features import connectivity, windowed
from openseize_amd.features.connectivity import window_connectivity

from test_analytic_host import analytic_measures, mixture
from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cov", "corr", "aec", "plv", "ciplv")
REAL, COMPLEX = NAMES[:2], NAMES[2:]
RTOL = 1e-9          # the suite's cap on a bound (tests/test_gpu_parity.py)


def window_starts(n, W, step):
    return np.arange(0 if n < W else (n - W) // step + 1) * step


def window_pair_measures(x, W, step, ddof=1):
    """The definitions, window by window: (M, parts) for x (C, N).  Real x: M["cov"] and
    M["corr"] (nwin, C, C) from long-double sums about each window's own mean (corr clipped to
    [-1, 1], diagonal 1.0), parts = {}.  Complex x: M["aec"], M["plv"], M["ciplv"] from
    ``analytic_measures`` of each window's samples alone, and parts["R"], parts["I"] (nwin, C, C),
    the real and imaginary part of s_ij in long double, for the condition factor of ciplv."""
    x = np.asarray(x)
    starts = window_starts(x.shape[1], W, step)
    nch = x.shape[0]
    if not np.iscomplexobj(x):
        M = {name: np.empty((starts.size, nch, nch)) for name in REAL}
        for k, s in enumerate(starts):
            w = x[:, s:s + W].astype(np.longdouble)
            d = w - w.mean(axis=1, keepdims=True)
            c = (d @ d.T) / np.longdouble(W - ddof)
            sd = np.sqrt(np.diag(c))
            with np.errstate(all="ignore"):
                r = np.clip(c / (sd[:, None] * sd[None, :]), -1, 1)
            r[np.eye(nch, dtype=bool) & ~np.isnan(r)] = 1.0
            M["cov"][k], M["corr"][k] = c, r
        return M, {}
    M = {name: np.empty((starts.size, nch, nch)) for name in COMPLEX}
    parts = {key: np.empty((starts.size, nch, nch)) for key in ("R", "I")}
    for k, s in enumerate(starts):
        w = x[:, s:s + W]
        Mk, _ = analytic_measures(w)
        for name in COMPLEX:
            M[name][k] = Mk[name]
        wl = w.astype(np.clongdouble)
        u = wl / np.abs(wl)
        sij = (np.conj(u) @ u.T) / np.longdouble(W)          # [i, j] = mean conj(u_i) u_j
        parts["R"][k], parts["I"][k] = sij.real, sij.imag
    return M, parts


def shifted_scheme(x, W, step, ddof=1):
    """The device's scheme in float64 (the order of the sums apart): name -> (nwin, C, C)."""
    x = np.asarray(x)
    starts = window_starts(x.shape[1], W, step)
    nch = x.shape[0]
    out = {name: np.empty((starts.size, nch, nch)) for name in (COMPLEX if np.iscomplexobj(x) else REAL)}

    def pearson(r):
        d = r - r[:, :1]
        S, G = d.sum(axis=1), d @ d.T
        cov = W * G - S[:, None] * S[None, :]
        v = np.diag(cov)
        with np.errstate(all="ignore"):
            return cov, cov / (np.sqrt(v)[:, None] * np.sqrt(v)[None, :])

    for k, s in enumerate(starts):
        w = x[:, s:s + W]
        if np.iscomplexobj(x):
            a = np.abs(w)
            ux, uy = w.real / a, w.imag / a
            out["aec"][k] = pearson(a)[1]
            re, im = (ux @ ux.T + uy @ uy.T) / W, (ux @ uy.T - (ux @ uy.T).T) / W
            out["plv"][k] = np.hypot(re, im)
            with np.errstate(all="ignore"):                  # (the diagonal: 0 / 0 before its fixed point)
                out["ciplv"][k] = np.abs(im) / np.sqrt(1 - re * re)
            np.fill_diagonal(out["aec"][k], 1.0)
            np.fill_diagonal(out["plv"][k], 1.0)
            np.fill_diagonal(out["ciplv"][k], 0.0)
        else:
            cov, r = pearson(w)
            out["cov"][k] = cov / (W * (W - ddof))
            out["corr"][k] = np.clip(r, -1, 1)
            np.fill_diagonal(out["corr"][k], 1.0)
    return out


def caps(x, W, step, ddof=1):
    """(M, name -> (nwin, C, C) caps on |device - M|): RTOL absolute for corr, aec and plv, times
    sqrt(c_ii c_jj) for cov, times 1 / sqrt(1 - R^2) + |I| |R| / (1 - R^2)^1.5 for ciplv (the
    formula of ``bounds`` in tests/test_analytic_host.py; 1 on the diagonal, a fixed point)."""
    M, parts = window_pair_measures(x, W, step, ddof)
    one = np.ones_like(next(iter(M.values())))
    if "cov" in M:
        d = np.sqrt(np.diagonal(M["cov"], axis1=1, axis2=2))
        return M, {"cov": RTOL * d[:, :, None] * d[:, None, :], "corr": RTOL * one}
    R, I = parts["R"], parts["I"]
    eye = np.eye(R.shape[1], dtype=bool)
    with np.errstate(all="ignore"):
        factor = 1 / np.sqrt(1 - R ** 2) + np.abs(I) * np.abs(R) / (1 - R ** 2) ** 1.5
    factor[:, eye] = 1.0
    return M, {"aec": RTOL * one, "plv": RTOL * one, "ciplv": RTOL * factor}


def test_names_are_public():
    assert features.window_connectivity is window_connectivity
    assert features.WINDOW_CONNECTIVITY == connectivity.WINDOW_CONNECTIVITY == NAMES == tuple(_lib.WINDOW_CONNECTIVITY)
    assert list(_lib.WINDOW_CONNECTIVITY.values()) == list(range(5)) and _lib.WC_REAL == REAL
    assert connectivity._advance is windowed._advance and connectivity.window_count is windowed.window_count
    assert connectivity.window_plan is windowed.window_plan
    assert _lib.WC_BLOCK % 64 == 0
    doc = window_connectivity.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name
    for word in ("symmetric bit for bit", "MemoryError", "zero-amplitude", "constant"):
        assert word in doc, word


def test_restatement_against_numpy_window_by_window():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 3000)) + 100.0
    x[1] = x[0] + 0.5 * (x[1] - 100.0)
    for W, step in ((250, 125), (4, 1), (67, 200)):
        for ddof in (0, 1):
            M, _ = window_pair_measures(x, W, step, ddof)
            S = shifted_scheme(x, W, step, ddof)
            starts = window_starts(3000, W, step)
            assert M["cov"].shape == M["corr"].shape == (starts.size, 5, 5)
            for k in (0, starts.size // 2, starts.size - 1):
                w = x[:, starts[k]:starts[k] + W]
                c, r = np.cov(w, ddof=ddof), np.corrcoef(w)
                scale = np.sqrt(np.diag(c))[:, None] * np.sqrt(np.diag(c))[None, :]
                assert np.max(np.abs(M["cov"][k] - c) / scale) < 1e-11, (W, k)     # (an offset of 100 sigma in float64)
                assert np.max(np.abs(M["corr"][k] - r)) < 1e-11, (W, k)
                assert np.max(np.abs(S["cov"][k] - M["cov"][k]) / scale) < 1e-12
                assert np.max(np.abs(S["corr"][k] - M["corr"][k])) < 1e-12
            assert np.all(np.diagonal(M["corr"], axis1=1, axis2=2) == 1.0)


def test_restatement_against_analytic_measures_on_one_window():
    z = mixture(5, 2048, seed=4)
    M, parts = window_pair_measures(z, 2048, 2048)
    want, wparts = analytic_measures(z)
    for name in COMPLEX:
        assert M[name].shape == (1, 5, 5)
        assert np.array_equal(M[name][0], want[name]), name
    assert np.max(np.abs(parts["R"][0] - wparts["R"])) < 1e-13 and np.max(np.abs(parts["I"][0] - wparts["I"])) < 1e-13
    # windows of a longer stream are the measures of their own samples alone
    M2, _ = window_pair_measures(z, 500, 300)
    for k in (0, 3, 5):
        wk, _ = analytic_measures(z[:, k * 300:k * 300 + 500])
        for name in COMPLEX:
            assert np.array_equal(M2[name][k], wk[name])
    S = shifted_scheme(z, 500, 300)
    _, cap = caps(z, 500, 300)
    for name in COMPLEX:
        assert np.all(np.isfinite(cap[name])) and np.all(np.abs(S[name] - M2[name]) <= 1e-3 * cap[name]), name


def test_rules_of_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 1000))
    x[2] = 7.5                                                # a constant channel
    M, _ = window_pair_measures(x, 100, 50)
    assert np.all(M["cov"][:, 2, :] == 0) and np.all(M["cov"][:, :, 2] == 0)
    assert np.all(np.isnan(M["corr"][:, 2, :])) and np.all(np.isnan(M["corr"][:, :, 2]))
    keep = np.ix_(range(M["corr"].shape[0]), [0, 1, 3], [0, 1, 3])
    assert np.all(np.isfinite(M["corr"][keep]))
    for name in REAL:
        assert np.array_equal(M[name], np.swapaxes(M[name], 1, 2), equal_nan=True), name


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    z = x + 1j * rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="take real data, got complex128 data"):
        window_connectivity(z, 100)                                         # corr of complex data
    with pytest.raises(ValueError, match="take complex .analytic. data, got float64 data"):
        window_connectivity(x, 100, measures=("plv", "ciplv"))
    with pytest.raises(ValueError, match="cannot come from one stream"):
        window_connectivity(x, 100, measures=("corr", "plv"))
    with pytest.raises(ValueError, match="two-dimensional.*stack at least two channels"):
        window_connectivity(x[0], 100)
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        window_connectivity(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_connectivity(x[:1], 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_connectivity(x[:1].T, 100, axis=0)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_connectivity(x, 501)
    cases = (({"winsize": 3}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "ddof": 2}, "ddof must be 0 or 1"), ({"winsize": 100, "ddof": -1}, "ddof"),
             ({"winsize": 100, "ddof": True}, "ddof"), ({"winsize": 100, "ddof": 1.5}, "ddof"),
             ({"winsize": 100, "measures": "coherence"}, "cov.*corr.*aec.*plv.*ciplv"),
             ({"winsize": 100, "measures": ("corr", "COV")}, "COV.*cov"),
             ({"winsize": 100, "measures": ()}, "cov"), ({"winsize": 100, "measures": 3}, "cov"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_connectivity(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_connectivity(x, **kwargs)
    for shape, match in (((5000,), "two-dimensional"), ((2, 2, 5000), "two-dimensional"), ((1, 5000), "two channels"),
                         ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_connectivity(src.pro, 100, measures=REAL)
        assert not src.started

    # a producer shows what it holds only with its first chunk: the wrong kind raises then, and
    # nothing has been asked of the device
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    with pytest.raises(ValueError, match="take real data, got complex128 chunks"):
        window_connectivity(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(ValueError, match="take complex .analytic. data, got float64 chunks"):
        window_connectivity(Untouched((4, 5000)).pro, 100, measures="aec")
    with pytest.raises(TypeError):
        window_connectivity(x, 100, fs=100)                                 # no such argument


@pytest.mark.parametrize("W,step", [(4, 1), (5, 3), (64, 64), (67, 200), (250, 125), (1000, 333), (1025, 2500)])
def test_windows_do_not_depend_on_the_chunk_lengths(W, step):
    """window_plan drives the pushes: whatever the chunk lengths, the windows completed are the
    windows of the stream, in order, each starting at k step."""
    n = 6000
    want = list(window_starts(n, W, step))

    def starts_of(chunk):
        lengths = [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
        got, done = [], 0
        for (start, nwin, keep, skip), m in zip(windowed.window_plan(lengths, W, step), lengths):
            if nwin:
                assert start == done * step
            got += [start + k * step for k in range(nwin)]
            done += nwin
        return got

    assert starts_of(n) == want and len(want) == windowed.window_count(n, W, step)
    for chunk in (7, 249, 250, 251, 4099):
        assert starts_of(chunk) == want, chunk


C_TYPES = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "const double *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_pairs_work", "int64_t", 6), ("osz_window_pairs", "int", 14)):
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
    for name, value in _lib.WINDOW_CONNECTIVITY.items():
        assert re.search(rf"OSZ_WC_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WC_COUNT = 5\b", header)
    assert re.search(rf"#define OSZ_WC_BLOCK {_lib.WC_BLOCK}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowpair\.hip\b", makefile, re.M)
    # the work-space query needs no device
    work = lib.osz_window_pairs_work
    work.restype, work.argtypes = _lib.SIGNATURES["osz_window_pairs_work"]
    B = _lib.WC_BLOCK
    assert work(3, 1000, 100, 50, 0b11, 0) == 2 * 3 * 19 + 19 * 9                  # sums, one batch of 19 windows
    assert work(3, 1000, 100, 50, 0b00100, 1) == 3 * 3 * 1000 + 2 * 3 * 19 + 19 * 9
    assert work(3, 1000, 100, 50, 0b11100, 1) == 3 * 3 * 1000 + 2 * 3 * 19 + 19 * 36  # the 2 C phasor rows
    assert work(3, 3 * B, B + 1, B, 0b10, 0) == 2 * 3 * 2 + 2 * 2 * 9               # two sub-blocks a window
    assert work(3, 50, 100, 50, 0b1, 0) == 0                                       # no window: nothing
    for bad in ((1, 1000, 100, 50, 1, 0), (3, -1, 100, 50, 1, 0), (3, 1000, 3, 50, 1, 0), (3, 1000, 100, 0, 1, 0),
                (3, 1000, 100, 50, 0, 0), (3, 1000, 100, 50, 32, 1), (3, 1000, 100, 50, 0b101, 0),
                (3, 1000, 100, 50, 0b101, 1), (3, 1000, 100, 50, 0b1, 1), (3, 1000, 100, 50, 0b100, 0)):
        assert work(*bad) == -1, bad


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_pair_kernels_use_no_scratch_and_no_spill(tmp_path):
    """Every kernel of windowpair.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled register of either kind, and the Gram kernel leaves room for two waves a SIMD (two
    workgroups a CU, which its 67.6 KB of LDS allow as well)."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowpair.hip"), "-o", str(tmp_path / "windowpair.o"),
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
    for stem, count in (("window_stage_kernel", 1), ("window_sums_kernel", 1), ("window_gram_kernel", 2),
                        ("window_finish_kernel", 2)):
        assert sum(stem in k for k in kernels) == count, (stem, sorted(kernels))
    assert len(kernels) == 6, sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 256
        if "window_gram_kernel" in name:
            assert int(use["LDS Size"]) <= 80 * 1024
