"""CPU-only tests of window_mutual_info (K25): the names, the argument errors (raised with no GPU
and before the stream is touched), the C ABI and the entry checks of osz_window_mi and
osz_window_mi_work through ctypes without a device, the register report of csrc/windowmi.hip (no
scratch, no spill), and ``window_mi_measures``, the NumPy restatement of the definition that
tests/test_gpu_mi.py compares the device against.

The restatement does not share the kernel's arithmetic: the edges come from ``numpy.quantile`` or
the uniform formula, the bins from ``numpy.searchsorted``, the counts from ``numpy.add.at``, and the
entropies are the direct -sum p ln p in long double, where the kernel sums a table of n ln n: the
two formulas check each other (``test_the_table_form_agrees_with_the_direct_sum``: 3e-15 over W
16 .. 4096 and B 2 .. 16).  The restatement is pinned on what must hold of any correct one: MI(x, x)
= H, MI <= min(H_i, H_j), the known bias of independent rows, more for a coupled pair than for an
independent one, and -- the feature's reason to exist -- a dependence that no correlation sees."""

import ctypes
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _device as dev
from openseize_amd import _lib, features, producer
from openseize_amd.features import _stream, mutual_info
from openseize_amd.features.mutual_info import window_mutual_info

from test_connectivity_host import C_TYPES, ROOT, _hipcc, window_starts
from test_csd_host import Untouched

NAMES = ("counts", "mi", "nmi", "joint")
BINNINGS = ("quantile", "uniform")

# (C, W, step, B, binning, windows) of tests/test_gpu_mi.py, which says what each is for
SHAPES = [(2, 16, 16, 2, "quantile", 3), (3, 64, 32, 16, "quantile", 4), (5, 63, 70, 3, "uniform", 3),
          (17, 65, 65, 16, "quantile", 2), (9, 1031, 515, 8, "uniform", 3), (4, 4096, 4096, 5, "quantile", 2),
          (66, 128, 128, 8, "quantile", 2), (130, 32, 32, 2, "quantile", 2)]


def mixed(nch, n, seed=31):
    """Seeded normal rows (C, n), each row but the first plus 0.7 of the row before it; then row
    min(2, C - 1) is quantised (``round(3 x)``: many ties), row 3 (C >= 4) is an exact copy of row 0
    (a cell reaches n = W) and row 4 (C >= 5) is the square of row 1 plus a little noise."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nch, n))
    for c in range(1, nch):
        x[c] += 0.7 * x[c - 1]
    x[min(2, nch - 1)] = np.round(3.0 * x[min(2, nch - 1)])
    if nch >= 4:
        x[3] = x[0]
    if nch >= 5:
        x[4] = x[1] ** 2 + 0.1 * rng.standard_normal(n)
    return x


@lru_cache(maxsize=None)
def stream(shape, offset=0.0):
    """The rows of ``shape``: its windows and 3 samples of a window that is dropped.  Read-only."""
    nch, W, step, B, binning, nwin = shape
    x = mixed(nch, (nwin - 1) * step + W + 3) + offset
    x.setflags(write=False)
    return x


def bin_codes(w, B, binning):
    """The bins (C, W) of the window w (C, W) of finite samples, and whether each row is fit to bin."""
    with np.errstate(all="ignore"):
        if binning == "quantile":
            edges = np.quantile(w, np.arange(1, B) / B, axis=1, method="linear").T          # (C, B - 1)
            fit = np.ones(w.shape[0], dtype=bool)
        else:
            lo, hi = w.min(axis=1), w.max(axis=1)
            edges = lo[:, None] + np.arange(1, B)[None, :] * ((hi - lo) / B)[:, None]
            fit = np.isfinite(hi - lo)
    return np.stack([np.searchsorted(e, r, side="right") for e, r in zip(edges, w)]), fit


def plogp(N, W):
    """-sum p ln p over the last axes' cells of the counts N, p = N / W, in long double."""
    p = N.astype(np.longdouble) / np.longdouble(W)
    with np.errstate(all="ignore"):
        return -np.where(N > 0, p * np.log(np.where(N > 0, p, 1)), 0)


def window_mi_measures(x, W, step, B, binning):
    """The definition, window by window, for x (C, N): name -> float64, ``counts`` (nwin, B, B, C, C)
    and the others (nwin, C, C).  A row with a non-finite sample (under "uniform" also one whose hi -
    lo is not finite) is NaN in its row and column; mi below 0 is 0.0; nmi is NaN where H_i H_j = 0;
    the diagonal is H_i, 1.0 (NaN for H_i = 0), H_i and n_a on a = b."""
    x = np.asarray(x)
    starts = window_starts(x.shape[1], W, step)
    nch = x.shape[0]
    M = {"counts": np.full((starts.size, B, B, nch, nch), np.nan)}
    M.update({name: np.full((starts.size, nch, nch), np.nan) for name in NAMES[1:]})
    ii, jj = np.meshgrid(np.arange(nch), np.arange(nch), indexing="ij")
    for k, s in enumerate(starts):
        w = x[:, s:s + W]
        good = np.all(np.isfinite(w), axis=1)
        code, fit = bin_codes(np.where(good[:, None], w, 0.0), B, binning)
        good &= fit
        assert code.min() >= 0 and code.max() <= B - 1
        N = np.zeros((B, B, nch, nch), dtype=np.int64)
        np.add.at(N, (code[:, None, :], code[None, :, :], ii[:, :, None], jj[:, :, None]), 1)
        assert np.all(N.sum(axis=(0, 1)) == W)
        marg = np.stack([np.bincount(c, minlength=B) for c in code])                         # (C, B)
        H = plogp(marg, W).sum(axis=1)                                                       # (C,)
        Hij = plogp(N, W).sum(axis=(0, 1))
        with np.errstate(all="ignore"):
            mi = H[:, None] + H[None, :] - Hij
            mi = np.where(mi < 0, 0, mi)
            prod = H[:, None] * H[None, :]
            nmi = np.where(prod == 0, np.nan, np.clip(mi / np.sqrt(np.where(prod == 0, 1, prod)), 0, 1))
        up, d = np.triu_indices(nch, 1), np.arange(nch)
        for v in (mi, nmi, Hij):                              # computed for i < j and mirrored
            v[up[1], up[0]] = v[up]
        mi[d, d] = Hij[d, d] = H
        nmi[d, d] = np.where(H == 0, np.nan, 1.0)
        alive = good[:, None] & good[None, :]
        M["counts"][k] = np.where(alive[None, None], N, np.nan)
        for name, v in (("mi", mi), ("nmi", nmi), ("joint", Hij)):
            M[name][k] = np.where(alive, v.astype(np.float64), np.nan)
    return M


@lru_cache(maxsize=None)
def restated(shape, offset=0.0):
    nch, W, step, B, binning, nwin = shape
    return window_mi_measures(stream(shape, offset), W, step, B, binning)


def table_form(N, marg_i, marg_j, W):
    """MI of one pair from its counts by the kernel's formula, in float64: phi(n) = n ln n from a
    table, ln W as phi(W) / W, the cells in the order a, then b."""
    phi = np.zeros(W + 1)
    phi[1:] = np.arange(1, W + 1) * np.log(np.arange(1, W + 1))

    def S(cells):
        s = 0.0
        for n in cells:
            s += phi[n]
        return s
    hi, hj, hij = (phi[W] - S(marg_i)) / W, (phi[W] - S(marg_j)) / W, (phi[W] - S(N.ravel())) / W
    return (hi + hj) - hij, hi, hj, hij


def test_names_are_public():
    assert features.window_mutual_info is window_mutual_info
    assert features.WINDOW_MI == mutual_info.WINDOW_MI == NAMES == tuple(_lib.WINDOW_MI)
    assert features.MI_BINNINGS == mutual_info.MI_BINNINGS == BINNINGS == tuple(_lib.MI_BINNING)
    assert list(_lib.WINDOW_MI.values()) == list(range(4)) and list(_lib.MI_BINNING.values()) == [0, 1]
    assert _lib.WM_MAXBINS == 16 and _lib.WM_LONGEST == 4096
    doc = window_mutual_info.__doc__
    for name in NAMES + BINNINGS:
        assert f'"{name}"' in doc, name
    for word in ("MemoryError", "constant", "symmetric", "fixed points", "+0.0", "searchsorted", "nothing is atomic",
                 "offset"):
        assert word in doc, word


def test_mi_of_a_row_with_itself_is_its_entropy_and_no_pair_exceeds_it():
    x = mixed(6, 1500, seed=5) + 100.0
    for W, step, B, binning in ((200, 100, 8, "quantile"), (16, 16, 2, "uniform"), (67, 200, 16, "uniform"),
                                (500, 500, 5, "quantile")):
        M = window_mi_measures(x, W, step, B, binning)
        H = np.diagonal(M["mi"], axis1=1, axis2=2)
        assert np.array_equal(H, np.diagonal(M["joint"], axis1=1, axis2=2))
        # row 3 is a copy of row 0: the same bins, MI(x, x) = H(x)
        assert np.max(np.abs(M["mi"][:, 0, 3] - H[:, 0])) <= 1e-15 * np.log(B)
        assert np.max(np.abs(M["nmi"][:, 0, 3] - 1.0)) <= 1e-15
        least = np.minimum(H[:, :, None], H[:, None, :])
        assert np.all(M["mi"] <= least + 1e-15) and np.all(M["mi"] >= 0)
        assert np.all(M["joint"] <= H[:, :, None] + H[:, None, :] + 1e-15)
        assert np.all(H <= np.log(B) + 1e-15)
        assert np.all(M["counts"].sum(axis=(1, 2)) == W)
        for name in NAMES[1:]:
            assert np.array_equal(M[name], np.swapaxes(M[name], 1, 2)), name
        assert np.array_equal(M["counts"], M["counts"].transpose(0, 2, 1, 4, 3))
        if binning == "quantile":                                # continuous rows: W / B +- 1 a bin
            marg = np.diagonal(np.diagonal(M["counts"], axis1=3, axis2=4), axis1=1, axis2=2)   # (nwin, C, B)
            assert np.all(np.abs(marg[:, [0, 1, 4, 5]] - W / B) <= 1.0)


def test_independent_rows_have_the_known_bias_and_coupled_rows_exceed_it():
    """The plug-in estimate of independent rows is biased by (B - 1)^2 / (2 W): 2 W MI is close to
    chi-square with (B - 1)^2 degrees of freedom, so the mean over 40 windows of B = 4 is within
    7 % of it at one sigma; 25 % is allowed."""
    rng = np.random.default_rng(11)
    W, B, nwin = 1024, 4, 40
    x = rng.standard_normal((3, W * nwin))
    x[2] = 0.6 * x[0] + 0.8 * rng.standard_normal(W * nwin)
    for binning in BINNINGS[:1]:
        M = window_mi_measures(x, W, W, B, binning)
        bias = (B - 1) ** 2 / (2 * W)
        free, tied = M["mi"][:, 0, 1].mean(), M["mi"][:, 0, 2].mean()
        print(f"{binning}: independent {free:.5f} (bias {bias:.5f}), coupled {tied:.5f}")
        assert abs(free - bias) <= 0.25 * bias
        # a Gaussian pair of correlation 0.6 carries -ln(1 - 0.36) / 2 = 0.223 nats; four bins keep most
        assert 0.1 < tied < 0.223 + 2 * bias and tied > 10 * free


def test_a_dependence_without_correlation_is_seen():
    """y = x^2 + noise: the correlation of a symmetric x with its square is 0, the dependence total."""
    rng = np.random.default_rng(12)
    W = 4096
    x = rng.standard_normal((3, W))
    x[1] = x[0] ** 2 + 0.1 * rng.standard_normal(W)
    corr = np.corrcoef(x)
    for binning in BINNINGS:
        M = window_mi_measures(x, W, W, 8, binning)
        seen, free = M["mi"][0, 0, 1], M["mi"][0, 0, 2]
        print(f"{binning}: corr {corr[0, 1]:+.3f}, MI(x, x^2 + e) = {seen:.3f}, MI(x, independent) = {free:.4f}")
        assert abs(corr[0, 1]) < 0.1 and seen > 0.3 and seen > 20 * free


def test_the_bins_take_the_maximum_the_constant_and_a_monotone_map():
    rng = np.random.default_rng(13)
    w = rng.standard_normal((4, 200))
    w[1] = 7.5
    w[2] = np.round(3 * w[2])
    for B in (2, 3, 8, 16):
        for binning in BINNINGS:
            code, fit = bin_codes(w, B, binning)
            assert fit.all() and code.min() >= 0 and code.max() == B - 1
            assert np.all(code[np.arange(4), w.argmax(axis=1)] == B - 1)
            assert np.all(code[1] == B - 1)
        code, _ = bin_codes(w[[0, 3]], B, "quantile")
        assert np.array_equal(bin_codes(np.exp(w[[0, 3]]), B, "quantile")[0], code)


def test_rules_of_the_restatement():
    x = mixed(5, 1000, seed=3)
    x[2] = 7.5                                                # a constant channel
    x[0, 130] = np.nan
    x[1, 420] = -np.inf
    for binning in BINNINGS:
        M = window_mi_measures(x, 100, 50, 4, binning)
        k = np.arange(M["mi"].shape[0])
        lost = np.zeros(M["mi"].shape, dtype=bool)
        for row, at in ((0, 130), (1, 420)):
            hit = (k * 50 <= at) & (at < k * 50 + 100)
            lost[hit, row, :] = lost[hit, :, row] = True
        for name in ("mi", "joint"):
            assert np.array_equal(np.isnan(M[name]), lost), name
        assert np.array_equal(np.isnan(M["counts"]), np.broadcast_to(lost[:, None, None], M["counts"].shape))
        const = np.zeros(lost.shape, dtype=bool)
        const[:, 2, :] = const[:, :, 2] = True
        assert np.array_equal(np.isnan(M["nmi"]), lost | const)
        assert np.all(M["mi"][const & ~lost] == 0.0)
        H = np.diagonal(M["mi"], axis1=1, axis2=2)
        ok = ~lost[:, 2, 4]
        assert np.array_equal(M["joint"][ok, 2, 4], H[ok, 4])
        assert np.all(M["counts"][ok, 3, :, 2, 4].sum(axis=1) == 100)      # the constant row is all bin B - 1


@pytest.mark.parametrize("shape", SHAPES)
def test_the_table_form_agrees_with_the_direct_sum(shape):
    nch, W, step, B, binning, nwin = shape
    M = restated(shape)
    worst = 0.0
    for k in range(nwin):
        for i, j in ((0, 1), (nch - 2, nch - 1), (0, min(3, nch - 1))):
            N = M["counts"][k, :, :, i, j].astype(np.int64)
            mi, hi, hj, hij = table_form(N, N.sum(axis=1), N.sum(axis=0), W)
            mi = max(mi, 0.0) if i != j else hi
            worst = max(worst, abs(mi - M["mi"][k, i, j]), abs(hij - M["joint"][k, i, j]))
    print(f"C={nch} W={W} B={B} {binning}: table - direct = {worst:.2e}")
    # at most B^2 + 2 B <= 288 terms of size <= W ln W, each within an ulp, divided by W
    assert worst <= 288 * np.log(W) * 2.0 ** -52


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="takes real data, got complex128 data"):
        window_mutual_info(x + 1j * x, 100)
    with pytest.raises(ValueError, match="two-dimensional.*stack at least two channels"):
        window_mutual_info(x[0], 100)
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        window_mutual_info(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_mutual_info(x[:1], 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_mutual_info(x[:1].T, 100, axis=0)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_mutual_info(x, 501)
    cases = (({"winsize": 15}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"), ({"winsize": 4097}, "winsize"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "bins": 1}, "bins must be an integer from 2 to 16, got 1"),
             ({"winsize": 100, "bins": 17}, "bins"), ({"winsize": 100, "bins": 8.0}, "bins"),
             ({"winsize": 100, "bins": True}, "bins"), ({"winsize": 100, "bins": "8"}, "bins"),
             ({"winsize": 100, "binning": "equal"}, "binning must be one of.*quantile.*uniform.*got 'equal'"),
             ({"winsize": 100, "binning": 0}, "binning"), ({"winsize": 100, "binning": None}, "binning"),
             ({"winsize": 100, "binning": ("quantile",)}, "binning"),
             ({"winsize": 100, "measures": "MI"}, "counts.*mi.*nmi.*joint"),
             ({"winsize": 100, "measures": ("mi", "entropy")}, "entropy.*joint"),
             ({"winsize": 100, "measures": ()}, "mi"), ({"winsize": 100, "measures": 3}, "mi"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_mutual_info(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_mutual_info(x, **kwargs)
    for shape, match in (((5000,), "two-dimensional"), ((2, 2, 5000), "two-dimensional"), ((1, 5000), "two channels"),
                         ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_mutual_info(src.pro, 100)
        assert not src.started

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    with pytest.raises(ValueError, match="takes real data, got complex128 chunks"):
        window_mutual_info(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_mutual_info(x, 100, maxlag=4)                                # no such argument


def test_the_memory_error_names_its_extra_array():
    """_pair_planes words the array of its ``lags`` by ``more_for``: "xcorr" unless told otherwise."""
    import inspect
    sig = inspect.signature(_stream._pair_planes)
    assert sig.parameters["more_for"].default == "xcorr"
    src = inspect.getsource(mutual_info.window_mutual_info)
    assert 'more_for="counts"' in src


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_mi_work", "int64_t", 6), ("osz_window_mi", "int", 15)):
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
    for name, value in _lib.WINDOW_MI.items():
        assert re.search(rf"OSZ_WM_{name.upper()} = {value}\b", header), name
    for name, value in _lib.MI_BINNING.items():
        assert re.search(rf"OSZ_WM_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WM_COUNT = 4\b", header)
    assert re.search(rf"#define OSZ_WM_MAXBINS {_lib.WM_MAXBINS}\b", header)
    assert re.search(rf"#define OSZ_WM_LONGEST {_lib.WM_LONGEST}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowmi\.hip\b", makefile, re.M)


# ---- the entry checks, through ctypes without a device (as tests/test_pair_window_args_host.py: the
# pointers are fake addresses nothing dereferences and every case has n < winsize, so a check that
# wrongly passed returns OSZ_OK, which fails the assertion, and cannot reach a launch)
X, CNT, OUT, WORK = 0x1000, 0x4000, 0x2000, 0x3000         # 16-byte aligned, never read
NCH, N, W0, PITCH = 3, 10, 64, 16


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def arguments(**change):
    a = dict(x=X, pitch=PITCH, nch=NCH, n=N, winsize=W0, step=5, bins=8, binning=0, mask=15, counts=CNT, out=OUT,
             plane_pitch=0, work=WORK, work_len=None)
    a.update(change)
    assert a["n"] < a["winsize"], "every case is one without a window"
    return a


def work_of(lib, **change):
    a = arguments(**change)
    return lib.osz_window_mi_work(a["nch"], a["n"], a["winsize"], a["step"], a["bins"], a["mask"])


def call(lib, **change):
    short = change.pop("short", 0)
    a = arguments(**change)
    if a["work_len"] is None:
        a["work_len"] = max(work_of(lib, **change), 0) + short
    status = lib.osz_window_mi(a["x"], a["pitch"], a["nch"], a["n"], a["winsize"], a["step"], a["bins"], a["binning"],
                               a["mask"], a["counts"], a["out"], a["plane_pitch"], a["work"], a["work_len"], None)
    return status, lib.osz_last_error().decode()


def expected_work(nch, W, bins, batch):
    """[phi: W + 1 rounded up to even] and per window of a batch 16 edges and 18 doubles per channel,
    Wpad bytes of codes per channel and (nch Bp)^2 int32."""
    bp = 1 << (bins - 1).bit_length()
    wpad = -(-W // 64) * 64
    return ((W + 2) & ~1) + batch * (nch * (16 + 18 + wpad // 8) + (nch * bp) ** 2 // 2)


def test_the_work_space_query_needs_no_device(lib):
    work = lib.osz_window_mi_work
    assert work(3, 1000, 100, 50, 4, 0b1111) == expected_work(3, 100, 4, 19)
    assert work(3, 1000, 100, 50, 4, 0b0010) == expected_work(3, 100, 4, 19)          # the mask does not enter
    assert work(3, 1000, 100, 50, 5, 0b1) == expected_work(3, 100, 8, 19)             # B = 5 is padded to 8
    assert work(256, 1 << 20, 1024, 1024, 8, 0b10) == expected_work(256, 1024, 8, 16)  # 16 windows fill the cap
    assert work(2, 16, 16, 16, 2, 0b1) == expected_work(2, 16, 2, 1)
    assert work(3, 50, 100, 50, 4, 0b1) == expected_work(3, 100, 4, 1)                # no window: one batch slot
    for bad in ((1, 1000, 100, 50, 4, 1), (16385, 1000, 100, 50, 4, 1), (3, -1, 100, 50, 4, 1), (3, 1000, 15, 50, 4, 1),
                (3, 10000, 4097, 50, 4, 1), (3, 1000, 100, 0, 4, 1), (3, 1000, 100, 50, 1, 1), (3, 1000, 100, 50, 17, 1),
                (3, 1000, 100, 50, -1, 1), (3, 1000, 100, 50, 4, 0), (3, 1000, 100, 50, 4, 16)):
        assert work(*bad) == -1, bad


def test_valid_arguments_without_a_window_are_accepted(lib):
    status, msg = call(lib)
    assert status == _lib.OSZ_OK, msg
    for edge in (dict(nch=16384, winsize=16, n=15, pitch=16, bins=2), dict(bins=16, binning=1, winsize=4096),
                 dict(mask=1, out=None), dict(mask=14, counts=None)):    # the ends of the ranges; arrays a mask leaves alone
        status, msg = call(lib, **edge)
        assert status == _lib.OSZ_OK and work_of(lib, **edge) >= 0, (edge, msg)


BAD = {
    "null x": (dict(x=None), "null", False),
    "null out": (dict(out=None), "null", False),
    "null counts": (dict(counts=None), "null", False),
    "null out, nmi alone": (dict(out=None, mask=4), "null", False),
    "null work": (dict(work=None), "null", False),
    "nch 1": (dict(nch=1), "nch 1,", True),
    "nch 16385": (dict(nch=16385), "nch 16385,", True),
    "negative n": (dict(n=-1), "n -1,", True),
    "winsize below": (dict(winsize=15, n=2), "winsize 15,", True),
    "winsize above": (dict(winsize=4097), "winsize 4097,", True),
    "step 0": (dict(step=0), "step 0,", True),
    "mask 0": (dict(mask=0), "mask 0", True),
    "mask past the last bit": (dict(mask=16), "mask 16", True),
    "bins 1": (dict(bins=1), "bins 1", True),
    "bins 17": (dict(bins=17), "bins 17", True),
    "bins -3": (dict(bins=-3), "bins -3", True),
    "binning 2": (dict(binning=2), "binning must be 0 or 1, got 2", False),
    "binning -1": (dict(binning=-1), "binning must be 0 or 1, got -1", False),
    "pitch < n": (dict(pitch=N - 1), f"pitch {N - 1} is less than n {N}", False),
    "x not aligned": (dict(x=X + 4), "aligned", False),
    "out not aligned": (dict(out=OUT + 4), "aligned", False),
    "counts not aligned": (dict(counts=CNT + 4), "aligned", False),
    "work not 16-byte aligned": (dict(work=WORK + 8), "16-byte aligned", False),
    "work_len one short": (dict(short=-1), f"work holds {expected_work(NCH, W0, 8, 1) - 1} doubles", False),
}


@pytest.mark.parametrize("label", list(BAD))
def test_a_bad_argument_is_refused(lib, label):
    change, says, planned = BAD[label]
    change = dict(change)
    status, msg = call(lib, **change)
    assert status == _lib.OSZ_ERR_INVALID, (status, msg)
    assert msg.startswith("osz_window_mi: ") and re.search(re.escape(says) + r"(?!\d)", msg), msg
    change.pop("short", None)
    assert (work_of(lib, **change) == -1) == planned


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_mi_kernels_fit_their_budgets(tmp_path):
    """Every kernel of windowmi.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled register of either kind, and few enough registers for two workgroups a SIMD."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowmi.hip"), "-o", str(tmp_path / "windowmi.o"),
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
    for part, count in (("mi_phi_kernel", 1), ("mi_code_kernel", 4), ("mi_gram_kernel", 1), ("mi_finish_kernel", 4)):
        assert sum(part in k for k in kernels) == count, sorted(kernels)
    assert len(kernels) == 10, sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 128
        assert int(use["LDS Size"]) <= 16 * 1024             # (static: the finish adds its table, at most 32.8 KB)
