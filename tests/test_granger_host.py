"""CPU-only tests of window_granger (K24): the names, the argument errors (raised with no GPU and
before the stream is touched), the C ABI of the entry points against the header, the register
report of csrc/windowgranger.hip (no scratch, no spill, the LDS budget of the pair kernel), and
``window_granger_measures``, the NumPy long-double restatement of the definition that
tests/test_gpu_granger.py compares the device against.

The restatement does not share the kernel's algorithm: the lagged covariances are direct sums of
the centred rows, the 2p x 2p block-Toeplitz and p x p Toeplitz normal equations are assembled
explicitly, and both are solved by Gaussian elimination with partial pivoting written here
(numpy.linalg does not take long double); the kernel runs Levinson recursions.  The restatement is
pinned on what must hold of any correct one: every value >= 0, Geweke's identity for the total,
invariance under x_i -> a x_i + b, and the direction and size of the coupling of rows built with a
known delay.  The same elimination in float64 agrees with long double to 1e-13 on every shape the
GPU tests use (measured: <= 1e-15): the data are well conditioned, and the GPU tests' cap of 1e-9
hides nothing."""

import ctypes
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _device as dev
from openseize_amd import _lib, features, producer
from openseize_amd.features import granger
from openseize_amd.features.granger import window_granger

from test_connectivity_host import C_TYPES, ROOT, _hipcc, window_starts
from test_csd_host import Untouched

NAMES = ("granger", "instant", "total")

# (C, W, step, p, windows) of tests/test_gpu_granger.py, which says what each is for
SHAPES = [(2, 16, 16, 2, 7), (3, 64, 20, 8, 5), (17, 257, 100, 16, 4), (5, 1030, 515, 5, 3), (3, 4096, 4096, 16, 2),
          (66, 100, 150, 3, 3), (130, 128, 128, 1, 2)]


def coupled(nch, n, seed=29):
    """Seeded normal rows (C, n), each row but the first plus 0.7 of the row before it delayed by 3."""
    x = np.random.default_rng(seed).standard_normal((nch, n))
    x[1:] += 0.7 * np.roll(x[:-1], 3, axis=1)
    return x


@lru_cache(maxsize=None)
def stream(shape, offset=0.0):
    """The rows of ``shape``: its windows and 3 samples of a window that is dropped.  Read-only."""
    nch, W, step, p, nwin = shape
    x = coupled(nch, (nwin - 1) * step + W + 3) + offset
    x.setflags(write=False)
    return x


def eliminate(A, B):
    """X with A X = B for stacks A (n, m, m) and B (n, m, q) in their own dtype: Gaussian elimination
    with partial pivoting, then back substitution."""
    A, B = A.copy(), B.copy()
    n, m, _ = A.shape
    rows = np.arange(n)
    for c in range(m):
        piv = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        for M in (A, B):
            top, low = M[rows, c].copy(), M[rows, piv].copy()
            M[rows, c], M[rows, piv] = low, top
        f = A[:, c + 1:, c] / A[:, c, c][:, None]
        A[:, c + 1:, :] -= f[:, :, None] * A[:, c, :][:, None, :]
        B[:, c + 1:, :] -= f[:, :, None] * B[:, c, :][:, None, :]
    X = np.empty_like(B)
    for c in range(m - 1, -1, -1):
        acc = B[:, c, :] - np.einsum("nk,nkq->nq", A[:, c, c + 1:], X[:, c + 1:, :])
        X[:, c, :] = acc / A[:, c, c][:, None]
    return X


def window_granger_parts(x, W, step, order, dtype=np.longdouble):
    """Per window, in ``dtype``: E (nwin, C), the errors of the scalar Yule-Walker models, and for the
    pairs i < j (in the order of ``np.triu_indices(C, 1)``) S (nwin, npairs, 2, 2), the error
    covariance of the bivariate model, index 0 channel i and 1 channel j."""
    x = np.asarray(x)
    starts = window_starts(x.shape[1], W, step)
    nch, p = x.shape[0], order
    ii, jj = np.triu_indices(nch, 1)
    E = np.empty((starts.size, nch), dtype=dtype)
    S = np.empty((starts.size, ii.size, 2, 2), dtype=dtype)
    for k, s in enumerate(starts):
        with np.errstate(all="ignore"):
            w = x[:, s:s + W].astype(dtype)
            d = w - w.mean(axis=1, keepdims=True)
            # r[l][a, b] = r_ab(l), l = 0 .. p; r_ab(-l) = r_ba(l)
            r = np.stack([(d[:, :W - l] @ d[:, l:].T) / dtype(W) for l in range(p + 1)])
            # the scalar models: sum_k a_k r(l - k) = r(l), l = 1 .. p
            auto = np.stack([np.diagonal(r[l]) for l in range(p + 1)], axis=1)           # (C, p + 1)
            lags = np.abs(np.arange(1, p + 1)[:, None] - np.arange(1, p + 1)[None, :])
            a = eliminate(auto[:, lags], auto[:, 1:, None])[:, :, 0]
            E[k] = auto[:, 0] - np.sum(a * auto[:, 1:], axis=1)

            # C(l)_ab = r_{pair[b] pair[a]}(l) for l >= 0, C(-l) = C(l)^T: (npairs, 2, 2) per lag
            def C(l):
                m = r[abs(l)]
                c = np.array([[m[ii, ii], m[jj, ii]], [m[ii, jj], m[jj, jj]]]).transpose(2, 0, 1)
                return c if l >= 0 else c.transpose(0, 2, 1)
            # [A_1 .. A_p] R = [C(1) .. C(p)] with the block R[k, l] = C(l - k): solve R^T A^T = rhs^T
            R = np.empty((ii.size, 2 * p, 2 * p), dtype=dtype)
            rhs = np.empty((ii.size, 2, 2 * p), dtype=dtype)
            for l in range(1, p + 1):
                rhs[:, :, 2 * l - 2:2 * l] = C(l)
                for q in range(1, p + 1):
                    R[:, 2 * q - 2:2 * q, 2 * l - 2:2 * l] = C(l - q)
            A = eliminate(R.transpose(0, 2, 1), rhs.transpose(0, 2, 1)).transpose(0, 2, 1)   # (npairs, 2, 2 p)
            sig = C(0)
            for q in range(1, p + 1):
                sig = sig - A[:, :, 2 * q - 2:2 * q] @ C(q).transpose(0, 2, 1)
            S[k] = sig
    return E, S


def window_granger_measures(x, W, step, order, dtype=np.longdouble):
    """The definition, window by window, for x (C, N): name -> float64 (nwin, C, C).  A pair is NaN
    in every measure when one of E_i, E_j, S_ii, S_jj, det S is not finite and > 0; a finite value
    below 0 is 0.0; the diagonal is 0.0, NaN where E_i is not finite and > 0; total is the float64
    sum (granger[i, j] + granger[j, i]) + instant of the float64 values."""
    E, S = window_granger_parts(x, W, step, order, dtype)
    nwin, nch = E.shape
    ii, jj = np.triu_indices(nch, 1)
    M = {name: np.full((nwin, nch, nch), np.nan) for name in NAMES}
    with np.errstate(all="ignore"):
        det = S[:, :, 0, 0] * S[:, :, 1, 1] - S[:, :, 0, 1] * S[:, :, 1, 0]
        Ei, Ej, Sii, Sjj = E[:, ii], E[:, jj], S[:, :, 0, 0], S[:, :, 1, 1]
        good = np.ones(det.shape, dtype=bool)
        for v in (Ei, Ej, Sii, Sjj, det):
            good &= np.isfinite(v) & (v > 0)

        def written(v):
            v = np.where(good, v, np.nan).astype(np.float64)
            return np.where(v <= 0, 0.0, v)
        fij, fji, ins = written(np.log(Ej / Sjj)), written(np.log(Ei / Sii)), written(np.log(Sii * Sjj / det))
    tot = (fij + fji) + ins
    M["granger"][:, ii, jj], M["granger"][:, jj, ii] = fij, fji
    M["instant"][:, ii, jj] = M["instant"][:, jj, ii] = ins
    M["total"][:, ii, jj] = M["total"][:, jj, ii] = tot
    alive = np.where(np.isfinite(E) & (E > 0), 0.0, np.nan)
    for name in NAMES:
        M[name][:, np.arange(nch), np.arange(nch)] = alive
    return M


@lru_cache(maxsize=None)
def restated(shape, offset=0.0):
    nch, W, step, p, nwin = shape
    return window_granger_measures(stream(shape, offset), W, step, p)


def test_names_are_public():
    assert features.window_granger is window_granger
    assert features.WINDOW_GRANGER == granger.WINDOW_GRANGER == NAMES == tuple(_lib.WINDOW_GRANGER)
    assert list(_lib.WINDOW_GRANGER.values()) == list(range(3))
    assert _lib.WG_MAXORDER == 16 and _lib.WG_LONGEST == 4096
    doc = window_granger.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name
    for word in ("source", "target", "MemoryError", "constant", "ill-conditioned", "unspecified", "+0.0"):
        assert word in doc, word


def test_every_value_is_nonnegative_and_the_total_is_gewekes():
    x = coupled(4, 1500, seed=5) + 100.0
    for W, step, p in ((200, 100, 6), (16, 16, 2), (67, 200, 8)):
        E, S = window_granger_parts(x, W, step, p)
        M = window_granger_measures(x, W, step, p)
        ii, jj = np.triu_indices(4, 1)
        det = S[:, :, 0, 0] * S[:, :, 1, 1] - S[:, :, 0, 1] * S[:, :, 1, 0]
        assert np.all(E > 0) and np.all(det > 0)
        # before the floor at 0 is applied: rounding aside, nothing is negative
        raw = np.stack((np.log(E[:, jj] / S[:, :, 1, 1]), np.log(E[:, ii] / S[:, :, 0, 0]),
                        np.log(S[:, :, 0, 0] * S[:, :, 1, 1] / det)))
        assert raw.min() > -1e-15, raw.min()
        for name in NAMES:
            assert np.all(M[name] >= 0), name
        whole = np.log(E[:, ii] * E[:, jj] / det).astype(np.float64)
        assert np.max(np.abs(M["total"][:, ii, jj] - whole)) <= 1e-15 * max(1.0, whole.max())
        assert np.array_equal(M["total"], np.swapaxes(M["total"], 1, 2))
        assert np.array_equal(M["instant"], np.swapaxes(M["instant"], 1, 2))
        assert np.array_equal(M["total"], (M["granger"] + np.swapaxes(M["granger"], 1, 2)) + M["instant"])
        assert np.all(np.diagonal(M["granger"], axis1=1, axis2=2) == 0.0)


def test_the_measures_do_not_move_with_scale_and_offset():
    x = coupled(3, 600, seed=7)
    M = window_granger_measures(x, 200, 100, 5)
    y = x.copy()
    y[1] = -2.5e3 * y[1] + 1e6
    y[2] = 1e-4 * y[2] - 3.0
    N = window_granger_measures(y, 200, 100, 5)
    for name in NAMES:
        assert np.max(np.abs(M[name] - N[name])) < 1e-12, name


@pytest.mark.parametrize("p", [3, 8, 16])
def test_the_delayed_coupling_has_its_size_and_direction(p):
    """Two rows: x[1] = noise + 0.7 x[0] delayed by 3, x[0] white.  Given its own past x[1] has the
    error 1.49 and given x[0]'s too the error 1, so F_{0->1} is near ln 1.49 = 0.399 and F_{1->0}
    near 0.  (Measured at p = 16: 0.395 and 0.004.  With more rows the later sources are mixtures
    themselves -- the sum is taken from the rows as they were -- and drive less: 0.23 at p = 3.)"""
    M = window_granger_measures(coupled(2, 4096), 4096, 4096, p)
    for i in range(1):
        fwd, back = M["granger"][0, i, i + 1], M["granger"][0, i + 1, i]
        print(f"p={p} i={i}: F(i -> i+1) = {fwd:.4f}, F(i+1 -> i) = {back:.4f}")
        assert abs(fwd - np.log(1.49)) < 0.05, (p, i, fwd)
        assert back < 0.05, (p, i, back)


def test_rules_of_the_restatement():
    x = coupled(4, 1000, seed=3)
    x[2] = 7.5                                                # a constant channel
    x[0, 130] = np.nan
    M = window_granger_measures(x, 100, 50, 4)
    k = np.arange(M["granger"].shape[0])
    hit = (k * 50 <= 130) & (130 < k * 50 + 100)
    for name in NAMES:
        lost = np.zeros(M[name].shape, dtype=bool)
        lost[:, 2, :] = lost[:, :, 2] = True
        lost[hit, 0, :] = lost[hit, :, 0] = True
        assert np.array_equal(np.isnan(M[name]), lost), name
    clean = window_granger_measures(np.delete(np.nan_to_num(x), 2, axis=0)[:, 200:], 100, 50, 4)
    assert np.array_equal(clean["granger"][:, 1, 2], M["granger"][4:, 1, 3])


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_float64_elimination_agrees_with_long_double(shape, offset):
    nch, W, step, p, nwin = shape
    want = restated(shape, offset)
    got = window_granger_measures(stream(shape, offset), W, step, p, dtype=np.float64)
    for name in NAMES:
        worst = float(np.max(np.abs(got[name] - want[name])))
        print(f"C={nch} W={W} step={step} p={p} +{offset} {name}: float64 - long double = {worst:.2e}")
        assert want[name].shape == (nwin, nch, nch) and np.all(np.isfinite(want[name]))
        assert worst <= 1e-13, (shape, offset, name, worst)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="takes real data, got complex128 data"):
        window_granger(x + 1j * x, 100)
    with pytest.raises(ValueError, match="two-dimensional.*stack at least two channels"):
        window_granger(x[0], 100)
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        window_granger(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_granger(x[:1], 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_granger(x[:1].T, 100, axis=0)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_granger(x, 501)
    cases = (({"winsize": 15}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"), ({"winsize": 4097}, "winsize"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 200, "order": 0}, "order"), ({"winsize": 200, "order": 17}, "order"),
             ({"winsize": 200, "order": 4.0}, "order"), ({"winsize": 200, "order": True}, "order"),
             ({"winsize": 100, "order": 13}, "order must be at most winsize // 8 = 12"),
             ({"winsize": 16, "order": 3}, "winsize // 8"), ({"winsize": 63}, "winsize // 8 = 7, got 8"),
             ({"winsize": 100, "measures": "gc"}, "granger.*instant.*total"),
             ({"winsize": 100, "measures": ("granger", "TOTAL")}, "TOTAL.*total"),
             ({"winsize": 100, "measures": ()}, "granger"), ({"winsize": 100, "measures": 3}, "granger"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_granger(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_granger(x, **kwargs)
    for shape, match in (((5000,), "two-dimensional"), ((2, 2, 5000), "two-dimensional"), ((1, 5000), "two channels"),
                         ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_granger(src.pro, 100)
        assert not src.started

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    with pytest.raises(ValueError, match="takes real data, got complex128 chunks"):
        window_granger(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_granger(x, 100, maxlag=4)                                    # no such argument


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_granger_work", "int64_t", 6), ("osz_window_granger", "int", 13)):
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
    for name, value in _lib.WINDOW_GRANGER.items():
        assert re.search(rf"OSZ_WG_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WG_COUNT = 3\b", header)
    assert re.search(rf"#define OSZ_WG_MAXORDER {_lib.WG_MAXORDER}\b", header)
    assert re.search(rf"#define OSZ_WG_LONGEST {_lib.WG_LONGEST}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowgranger\.hip\b", makefile, re.M)
    # the work-space query needs no device: a sum and an error per (channel, window), then
    # (2 p + 1) C C doubles per window of a batch of at most 2^25 doubles
    work = lib.osz_window_granger_work
    work.restype, work.argtypes = _lib.SIGNATURES["osz_window_granger_work"]
    assert work(3, 1000, 100, 50, 4, 0b111) == 2 * 3 * 19 + 19 * 9 * 9
    assert work(3, 1000, 100, 50, 1, 0b010) == 2 * 3 * 19 + 19 * 3 * 9               # the mask does not enter
    assert work(3, 1000, 100, 50, 12, 0b1) == 2 * 3 * 19 + 19 * 25 * 9
    assert work(256, 1 << 20, 1024, 1024, 16, 0b101) == 2 * 256 * 1024 + 15 * 33 * 256 * 256   # 15 windows fill the cap
    assert work(2, 16, 16, 16, 2, 0b1) == 2 * 2 + 5 * 4
    assert work(3, 50, 100, 50, 4, 0b1) == 0                                         # no window: nothing
    for bad in ((1, 1000, 100, 50, 4, 1), (16385, 1000, 100, 50, 4, 1), (3, -1, 100, 50, 4, 1), (3, 1000, 15, 50, 1, 1),
                (3, 10000, 4097, 50, 4, 1), (3, 1000, 100, 0, 4, 1), (3, 1000, 100, 50, 0, 1), (3, 1000, 200, 50, 17, 1),
                (3, 1000, 100, 50, 100 // 8 + 1, 1), (3, 1000, 100, 50, -1, 1), (3, 1000, 100, 50, 4, 0),
                (3, 1000, 100, 50, 4, 8)):
        assert work(*bad) == -1, bad


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_granger_kernels_fit_their_budgets(tmp_path):
    """Every kernel of windowgranger.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled register of either kind, at most 256 registers of both files together, and the LDS of
    every instance of the pair kernel leaves room for two workgroups a CU."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowgranger.hip"), "-o", str(tmp_path / "windowgranger.o"),
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
    assert sum("granger_auto_kernel" in k for k in kernels) == 1, sorted(kernels)
    assert sum("granger_pair_kernel" in k for k in kernels) == 3, sorted(kernels)     # the orders to 4, 8 and 16
    assert len(kernels) == 4, sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 256
        if "granger_pair_kernel" in name:
            assert int(use["LDS Size"]) <= 80 * 1024
