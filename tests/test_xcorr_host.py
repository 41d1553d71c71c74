"""CPU-only tests of window_xcorr (K23): the names, the argument errors (raised with no GPU and
before the stream is touched), the C ABI of the entry points against the header, the register
report of csrc/windowxcorr.hip (no scratch, no spill, the LDS budget of the Gram kernel), and
``window_xcorr_measures``, the NumPy long-double restatement of the definition that
tests/test_gpu_xcorr.py compares the device against.  The restatement is pinned here against
numpy.correlate, numpy.corrcoef and numpy.cov, and on two closed forms: a delayed copy of a
channel, and two integer rows whose lags -2 and +2 tie exactly."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from openseize_amd import _device as dev
from openseize_amd import _lib, features, producer
from openseize_amd.features import xcorr
from openseize_amd.features.xcorr import window_xcorr, xcorr_lags

from test_connectivity_host import C_TYPES, ROOT, RTOL, _hipcc, window_starts
from test_csd_host import Untouched

NAMES = ("xcorr", "peak", "lag", "signed")


def scan_order(L):
    """The lags in the order the tie rule ranks equal maxima: 0, +1, -1, +2, -2, ..."""
    return np.array([0] + [s * a for a in range(1, L + 1) for s in (1, -1)])


def window_xcorr_measures(x, W, step, maxlag, normalize=True):
    """The definition, window by window, for x (C, N): name -> float64 array, "xcorr" (nwin, 2 L + 1,
    C, C) and "peak", "lag", "signed" (nwin, C, C), and R (nwin, C), r_ii(0) in long double.  The
    sums are long-double slices and ``@`` about each window's own mean.  An entry [i, j], i < j, is
    computed; [j, i] of lag -l is written from it, and the lags l and -l of the diagonal from l >= 0;
    lag 0 of the diagonal is the fixed point.  peak, lag and signed rank the float64 values of |v|:
    the first maximum in the order 0, +1, -1, +2, -2, ..."""
    x = np.asarray(x)
    starts = window_starts(x.shape[1], W, step)
    nch, L = x.shape[0], maxlag
    nl = 2 * L + 1
    M = {"xcorr": np.empty((starts.size, nl, nch, nch))}
    for name in NAMES[1:]:
        M[name] = np.empty((starts.size, nch, nch))
    R = np.empty((starts.size, nch), dtype=np.longdouble)
    iu = np.triu_indices(nch, 1)
    eye = np.eye(nch, dtype=bool)
    order = scan_order(L)
    for k, s in enumerate(starts):
        with np.errstate(all="ignore"):
            w = x[:, s:s + W].astype(np.longdouble)
            d = w - w.mean(axis=1, keepdims=True)
            r = np.empty((nl, nch, nch), dtype=np.longdouble)
            for l in range(-L, L + 1):
                a, b = (d[:, :W - l], d[:, l:]) if l >= 0 else (d[:, -l:], d[:, :W + l])
                r[L + l] = (a @ b.T) / np.longdouble(W)
            R[k] = np.diag(r[L])
            if normalize:
                sd = np.sqrt(R[k])
                v = np.clip(r / (sd[:, None] * sd[None, :]), -1, 1)
                v[L][eye & ~np.isnan(v[L])] = 1.0
            else:
                v = r
        v = v.astype(np.float64)
        for l in range(1, L + 1):                            # the diagonal: one value for l and -l
            v[L - l][eye] = v[L + l][eye]
        for l in range(-L, L + 1):                           # below the diagonal: the mirror of above
            v[L - l][iu[1], iu[0]] = v[L + l][iu]
        M["xcorr"][k] = v
        ranked = np.abs(v[L + order])                        # (nl, C, C) in scan order
        first = np.argmax(ranked, axis=0)[None]
        lost = np.isnan(ranked).any(axis=0)
        peak = np.take_along_axis(ranked, first, 0)[0]
        sgn = np.take_along_axis(v[L + order], first, 0)[0]
        lag = order[first[0]].astype(np.float64)
        peak[lost] = lag[lost] = sgn[lost] = np.nan
        for m in (peak, sgn):
            m[iu[1], iu[0]] = m[iu]
            m[eye] = v[L][eye]
        lag[iu[1], iu[0]] = -lag[iu]
        lag[eye] = np.where(np.isnan(v[L][eye]), np.nan, 0.0)
        M["peak"][k], M["lag"][k], M["signed"][k] = peak, lag, sgn
    return M, R


def caps(x, W, step, maxlag, normalize=True):
    """(M, cap): cap (nwin, C, C) bounds |device - M| for xcorr (every lag), peak and signed: RTOL
    absolute with ``normalize``, else RTOL sqrt(r_ii(0) r_jj(0))."""
    M, R = window_xcorr_measures(x, W, step, maxlag, normalize)
    if normalize:
        return M, RTOL * np.ones_like(M["peak"])
    sd = np.sqrt(R)
    return M, (RTOL * sd[:, :, None] * sd[:, None, :]).astype(np.float64)


def peak_margin(M, cap, L):
    """The smallest gap, over the off-diagonal entries, between the largest |v| and the runner-up,
    in units of the cap (inf where there is one lag or the cap is 0)."""
    a = np.sort(np.abs(M["xcorr"]), axis=1)
    if a.shape[1] < 2:
        return np.inf
    off = ~np.eye(a.shape[2], dtype=bool)
    with np.errstate(all="ignore"):
        gap = ((a[:, -1] - a[:, -2]) / cap)[:, off]
    gap = gap[np.isfinite(gap)]
    return np.inf if gap.size == 0 else float(gap.min())


def tie_rows():
    """Two zero-mean integer rows of 16 samples whose cross-correlation at the lags -2 and +2 is
    the same exact number, the largest of |v| over the lags -4 .. 4."""
    a, b = np.zeros(16), np.zeros(16)
    a[7], a[8], a[9] = 1, 2, 1
    b[6] = b[10] = 1
    return np.stack((16 * a - 4, 16 * b - 2))


def delayed(d, W=256, seed=11):
    """(2, W): row 1 is row 0 delayed by d samples plus 1 % noise, both cut from a longer record."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(W + 64)
    return np.stack((base[32:32 + W], base[32 - d:32 - d + W] + 0.01 * rng.standard_normal(W)))


def test_names_are_public():
    assert features.window_xcorr is window_xcorr and features.xcorr_lags is xcorr_lags
    assert features.WINDOW_XCORR == xcorr.WINDOW_XCORR == NAMES == tuple(_lib.WINDOW_XCORR)
    assert list(_lib.WINDOW_XCORR.values()) == list(range(4))
    assert _lib.WX_MAXLAG == 64 and _lib.WX_LONGEST == 4096
    assert np.array_equal(xcorr_lags(3), np.arange(-3, 4)) and np.array_equal(xcorr_lags(0), [0])
    with pytest.raises(ValueError, match="maxlag"):
        xcorr_lags(65)
    doc = window_xcorr.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name
    for word in ("tie rule", "MemoryError", "constant", "biased"):
        assert word in doc, word


def test_restatement_against_numpy():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 700)) + 100.0
    x[1:] += 0.7 * np.roll(x[:-1] - 100.0, 3, axis=1)
    for W, step, L in ((200, 100, 16), (8, 8, 4), (67, 200, 33)):
        M, R = window_xcorr_measures(x, W, step, L, True)
        U, _ = window_xcorr_measures(x, W, step, L, False)
        starts = window_starts(700, W, step)
        assert M["xcorr"].shape == U["xcorr"].shape == (starts.size, 2 * L + 1, 4, 4)
        for k in (0, starts.size - 1):
            w = x[:, starts[k]:starts[k] + W]
            d = w - w.mean(axis=1, keepdims=True)
            c = np.cov(w, ddof=0)
            scale = np.sqrt(np.diag(c))[:, None] * np.sqrt(np.diag(c))[None, :]
            for i in range(4):
                for j in range(4):
                    full = np.correlate(d[j], d[i], "full")[W - 1 - L:W + L] / W     # lags -L .. L
                    assert np.max(np.abs(U["xcorr"][k, :, i, j] - full)) / scale[i, j] < 1e-12, (W, k, i, j)
                    if i != j:
                        assert np.max(np.abs(M["xcorr"][k, :, i, j] - full / scale[i, j])) < 1e-12
            assert np.max(np.abs(M["xcorr"][k, L] - np.corrcoef(w))) < 1e-12
            assert np.max(np.abs(U["xcorr"][k, L] - c) / scale) < 1e-12
            assert np.max(np.abs(R[k] - np.diag(c)) / np.diag(c)) < 1e-12
        # |rho| <= 1 before clipping, up to rounding: the unclipped ratio of the other scaling
        sd = np.sqrt(R.astype(np.float64))
        assert np.max(np.abs(U["xcorr"]) / (sd[:, None, :, None] * sd[:, None, None, :])) <= 1 + 1e-12


def test_rules_of_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 1000))
    x[1:] += 0.7 * np.roll(x[:-1], 3, axis=1)
    x[2] = 7.5                                                # a constant channel
    L = 6
    for normalize in (True, False):
        M, _ = window_xcorr_measures(x, 100, 50, L, normalize)
        X = M["xcorr"]
        for l in range(-L, L + 1):
            assert np.array_equal(X[:, L + l], np.swapaxes(X[:, L - l], 1, 2), equal_nan=True)
        for name in ("peak", "signed"):
            assert np.array_equal(M[name], np.swapaxes(M[name], 1, 2), equal_nan=True), name
        assert np.array_equal(M["lag"], -np.swapaxes(M["lag"], 1, 2), equal_nan=True)
        keep = np.ix_(range(X.shape[0]), [0, 1, 3], [0, 1, 3])
        for name in NAMES[1:]:
            assert np.all(np.isfinite(M[name][keep])), name
            row, col = M[name][:, 2, :], M[name][:, :, 2]
            assert np.all(np.isnan(row) & np.isnan(col)) if normalize else np.all((row == 0) & (col == 0)), name
        assert np.all(np.isnan(X[:, :, 2, :])) if normalize else np.all(X[:, :, 2, :] == 0)
        diag = np.diagonal(M["peak"][keep], axis1=1, axis2=2)
        assert np.all(diag == 1.0) if normalize else np.all(diag == np.diagonal(X[:, L][keep], axis1=1, axis2=2))
        assert np.all(np.diagonal(M["lag"][keep], axis1=1, axis2=2) == 0.0)
        # peak, lag and signed are the xcorr planes' own values
        sub = X[:, :, [0, 1, 3]][:, :, :, [0, 1, 3]]
        sel = np.take_along_axis(sub, (M["lag"][keep] + L).astype(int)[:, None], axis=1)[:, 0]
        off = ~np.eye(3, dtype=bool)
        assert np.array_equal(sel[:, off], M["signed"][keep][:, off])
        assert np.array_equal(np.abs(sel)[:, off], M["peak"][keep][:, off])
        assert np.array_equal(M["peak"][keep][:, off], np.abs(sub).max(axis=1)[:, off])


@pytest.mark.parametrize("d", [0, 1, 5, 16])
def test_a_delayed_channel_peaks_at_its_delay(d):
    M, _ = window_xcorr_measures(delayed(d), 256, 256, 16)
    assert M["lag"][0, 0, 1] == d and M["lag"][0, 1, 0] == -d
    assert M["peak"][0, 0, 1] > 0.9 and M["signed"][0, 0, 1] > 0.9


def test_an_exact_tie_takes_the_positive_lag():
    x = tie_rows()
    assert np.all(x.sum(axis=1) == 0)
    for normalize in (True, False):
        M, _ = window_xcorr_measures(x, 16, 16, 4, normalize)
        v = M["xcorr"][0, :, 0, 1]
        assert v[4 - 2] == v[4 + 2] == np.abs(v).max() and np.sum(np.abs(v) == np.abs(v).max()) == 2
        assert M["lag"][0, 0, 1] == 2.0 and M["lag"][0, 1, 0] == -2.0
        assert M["peak"][0, 0, 1] == M["signed"][0, 0, 1] == v[6]
    M, _ = window_xcorr_measures(x, 16, 16, 4, True)
    assert abs(M["peak"][0, 0, 1] - 0.48596) < 1e-5


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="takes real data, got complex128 data"):
        window_xcorr(x + 1j * x, 100)
    with pytest.raises(ValueError, match="two-dimensional.*stack at least two channels"):
        window_xcorr(x[0], 100)
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        window_xcorr(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_xcorr(x[:1], 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_xcorr(x[:1].T, 100, axis=0)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_xcorr(x, 501)
    cases = (({"winsize": 7}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"), ({"winsize": 4097}, "winsize"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "maxlag": -1}, "maxlag"), ({"winsize": 100, "maxlag": 65}, "maxlag"),
             ({"winsize": 100, "maxlag": 4.0}, "maxlag"), ({"winsize": 100, "maxlag": True}, "maxlag"),
             ({"winsize": 100, "maxlag": 51}, "maxlag must be at most winsize // 2 = 50"),
             ({"winsize": 8, "maxlag": 5}, "winsize // 2"),
             ({"winsize": 100, "normalize": 1}, "normalize must be True or False"),
             ({"winsize": 100, "normalize": None}, "normalize"), ({"winsize": 100, "normalize": "yes"}, "normalize"),
             ({"winsize": 100, "measures": "corr"}, "xcorr.*peak.*lag.*signed"),
             ({"winsize": 100, "measures": ("peak", "LAG")}, "LAG.*lag"),
             ({"winsize": 100, "measures": ()}, "xcorr"), ({"winsize": 100, "measures": 3}, "xcorr"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_xcorr(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_xcorr(x, **kwargs)
    for shape, match in (((5000,), "two-dimensional"), ((2, 2, 5000), "two-dimensional"), ((1, 5000), "two channels"),
                         ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_xcorr(src.pro, 100)
        assert not src.started

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    with pytest.raises(ValueError, match="takes real data, got complex128 chunks"):
        window_xcorr(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_xcorr(x, 100, ddof=1)                                        # no such argument


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_xcorr_work", "int64_t", 6), ("osz_window_xcorr", "int", 15)):
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
    for name, value in _lib.WINDOW_XCORR.items():
        assert re.search(rf"OSZ_WX_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WX_COUNT = 4\b", header)
    assert re.search(rf"#define OSZ_WX_MAXLAG {_lib.WX_MAXLAG}\b", header)
    assert re.search(rf"#define OSZ_WX_LONGEST {_lib.WX_LONGEST}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowxcorr\.hip\b", makefile, re.M)
    # the work-space query needs no device: a sum per (channel, window), then (2 L + 1) C C doubles
    # per window of a batch of at most 2^25 doubles
    work = lib.osz_window_xcorr_work
    work.restype, work.argtypes = _lib.SIGNATURES["osz_window_xcorr_work"]
    assert work(3, 1000, 100, 50, 4, 0b1111) == 3 * 19 + 19 * 9 * 9
    assert work(3, 1000, 100, 50, 0, 0b0110) == 3 * 19 + 19 * 1 * 9                  # the mask does not enter
    assert work(3, 1000, 100, 50, 50, 0b1) == 3 * 19 + 19 * 101 * 9
    assert work(256, 1 << 20, 1024, 1024, 64, 0b1110) == 256 * 1024 + 3 * 129 * 256 * 256   # 3 windows fill the cap
    assert work(2, 8, 8, 8, 4, 0b1) == 2 + 9 * 4
    assert work(3, 50, 100, 50, 4, 0b1) == 0                                         # no window: nothing
    for bad in ((1, 1000, 100, 50, 4, 1), (16385, 1000, 100, 50, 4, 1), (3, -1, 100, 50, 4, 1), (3, 1000, 7, 50, 2, 1),
                (3, 10000, 4097, 50, 4, 1), (3, 1000, 100, 0, 4, 1), (3, 1000, 100, 50, -1, 1),
                (3, 1000, 100, 50, 51, 1), (3, 1000, 200, 50, 65, 1), (3, 1000, 100, 50, 4, 0),
                (3, 1000, 100, 50, 4, 16)):
        assert work(*bad) == -1, bad


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_xcorr_kernels_fit_their_budgets(tmp_path):
    """Every kernel of windowxcorr.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled register of either kind, at most 256 registers of both files together, and the Gram
    kernel's LDS leaves room for two workgroups a CU."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowxcorr.hip"), "-o", str(tmp_path / "windowxcorr.o"),
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
    for stem in ("xcorr_sums_kernel", "xcorr_gram_kernel", "xcorr_finish_kernel"):
        assert sum(stem in k for k in kernels) == 1, (stem, sorted(kernels))
    assert len(kernels) == 3, sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 256
        if "xcorr_gram_kernel" in name:
            assert int(use["LDS Size"]) <= 80 * 1024
    # the window dimension of the grid: a batch is at most 65535 windows
    source = open(os.path.join(csrc, "pair_window.h")).read()
    assert re.search(r"batch > 65535 \? 65535", source)
