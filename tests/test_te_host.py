"""CPU-only tests of window_transfer_entropy (K26): the names, the argument errors (raised with no
GPU and before the stream is touched), the C ABI and the entry checks of osz_window_te and
osz_window_te_work through ctypes without a device, the register report of csrc/windowte.hip, and
``window_te_measures``, the NumPy restatement of the definition that tests/test_gpu_te.py compares
the device against.

The restatement shares no arithmetic with the kernel: the bins are ``test_mi_host.bin_codes``
(``numpy.quantile`` or the uniform formula, ``numpy.searchsorted``), the counts come from
``numpy.add.at`` and the entropies are the direct -sum p ln p in long double, TE = H(Y'Y) - H(Y') -
H(Y'YX) + H(Y'X) with Y' = Y_{t-1}, where the kernel sums a table of n ln n.  It is pinned on what
must hold of any correct one: the chi-square bias of independent rows, a driven pair seen in its
direction and at its lag only, a squared drive that no correlation sees, the conditioning, and the
agreement of the table form with the direct one."""

import ctypes
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _device as dev
from openseize_amd import _lib, features, producer
from openseize_amd.features import transfer_entropy
from openseize_amd.features.transfer_entropy import window_transfer_entropy

from test_connectivity_host import C_TYPES, ROOT, _hipcc, window_starts
from test_csd_host import Untouched
from test_mi_host import BINNINGS, bin_codes, mixed, plogp

NAMES = ("counts", "te", "nte", "net")

# (C, W, step, B, lag, binning, windows) of tests/test_gpu_te.py, which says what each is for
SHAPES = [(2, 16, 16, 2, 1, "quantile", 3), (3, 65, 32, 8, 1, "quantile", 4), (5, 63, 70, 3, 2, "uniform", 3),
          (17, 66, 66, 4, 1, "quantile", 2), (9, 1031, 515, 8, 3, "uniform", 3), (4, 4096, 4096, 5, 64, "quantile", 2),
          (3, 128, 128, 2, 64, "quantile", 2), (130, 32, 32, 2, 1, "quantile", 2)]
CONSTANT = 5             # the row of a shape of 7 channels or more that is a constant


def driven(x, lag, rng):
    """y_t = 0.8 x_{t-lag} + 0.3 y_{t-1} + 0.5 e_t, from y = 0 before the stream."""
    e = rng.standard_normal(x.size)
    y = np.zeros(x.size)
    for t in range(x.size):
        y[t] = (0.8 * x[t - lag] if t >= lag else 0.0) + (0.3 * y[t - 1] if t else 0.0) + 0.5 * e[t]
    return y


@lru_cache(maxsize=None)
def stream(shape, offset=0.0):
    """The rows of ``shape``: ``test_mi_host.mixed`` rows (one quantised, one an exact copy of row 0,
    one the square of row 1 plus noise), with 7 channels or more row ``CONSTANT`` a constant and the
    last row driven by row 0 at the shape's lag; its windows and 3 samples of a window that is
    dropped.  Read-only."""
    nch, W, step, B, lag, binning, nwin = shape
    x = mixed(nch, (nwin - 1) * step + W + 3)
    if nch >= 7:
        x[CONSTANT] = 7.5
        x[nch - 1] = driven(x[0], lag, np.random.default_rng(41))
    x = x + offset
    x.setflags(write=False)
    return x


def window_te_measures(x, W, step, B, lag, binning):
    """The definition, window by window, for x (C, N): name -> float64, ``counts`` (nwin, B, B, B, C,
    C) and the others (nwin, C, C), [i, j] from the source i to the target j.  A row with a non-finite
    sample (under "uniform" also one whose hi - lo is not finite) is NaN in its row and column; te
    below 0 is 0.0, and exactly 0.0 where the integers say so (a source of one bin, a target of one
    symbol); nte is NaN where every bin before is followed by one bin alone (Hc = 0); the diagonal of
    te, nte and net is 0.0."""
    x = np.asarray(x)
    starts = window_starts(x.shape[1], W, step)
    nch, T = x.shape[0], W - lag
    M = {"counts": np.full((starts.size, B, B, B, nch, nch), np.nan)}
    M.update({name: np.full((starts.size, nch, nch), np.nan) for name in NAMES[1:]})
    ii, jj = np.meshgrid(np.arange(nch), np.arange(nch), indexing="ij")
    d = np.arange(nch)
    for k, s in enumerate(starts):
        w = x[:, s:s + W]
        good = np.all(np.isfinite(w), axis=1)
        code, fit = bin_codes(np.where(good[:, None], w, 0.0), B, binning)
        good &= fit
        assert code.min() >= 0 and code.max() <= B - 1
        now, before, src = code[:, lag:], code[:, lag - 1:W - 1], code[:, :T]
        N = np.zeros((B, B, B, nch, nch), dtype=np.int64)
        np.add.at(N, (now[None, :, :], before[None, :, :], src[:, None, :], ii[:, :, None], jj[:, :, None]), 1)
        assert np.all(N.sum(axis=(0, 1, 2)) == T)
        Nab, Nbc, Nb = N.sum(axis=2), N.sum(axis=0), N.sum(axis=(0, 2))
        Hab, Hb = plogp(Nab, T).sum(axis=(0, 1)), plogp(Nb, T).sum(axis=0)
        Habc, Hbc = plogp(N, T).sum(axis=(0, 1, 2)), plogp(Nbc, T).sum(axis=(0, 1))
        te = Hab - Hb - Habc + Hbc
        hc = Hab - Hb
        settled = np.all(np.count_nonzero(Nab, axis=0) <= 1, axis=0)          # (C, C): Hc = 0 in integers
        one_bin = np.all(src == src[:, :1], axis=1)                            # a source of one bin
        one_symbol = np.all(now == now[:, :1], axis=1) & np.all(before == before[:, :1], axis=1)
        te = np.where((te < 0) | one_bin[:, None] | one_symbol[None, :], 0, te)
        with np.errstate(all="ignore"):
            nte = np.where(settled, np.nan, np.clip(te / np.where(settled, 1, hc), 0, 1))
        te, nte = te.astype(np.float64), nte.astype(np.float64)
        te[d, d] = nte[d, d] = 0.0
        net = te - te.T
        alive = good[:, None] & good[None, :]
        M["counts"][k] = np.where(alive[None, None, None], N, np.nan)
        for name, v in (("te", te), ("nte", nte), ("net", net)):
            M[name][k] = np.where(alive, v, np.nan)
    return M


@lru_cache(maxsize=None)
def restated(shape, offset=0.0):
    nch, W, step, B, lag, binning, nwin = shape
    return window_te_measures(stream(shape, offset), W, step, B, lag, binning)


def conditional_entropy(N, T):
    """Hc of the target from the counts N (B, B, B) of one pair, direct, in long double."""
    return float(plogp(N.sum(axis=2), T).sum() - plogp(N.sum(axis=(0, 2)), T).sum())


def table_form(N, W, T):
    """(te, hc) of one pair from its counts N[a, b, c] by the kernel's formula, in float64: phi(n) =
    n ln n from a table; b outermost, then a, then c."""
    phi = np.zeros(W + 1)
    phi[1:] = np.arange(1, W + 1) * np.log(np.arange(1, W + 1))
    B = N.shape[0]
    S3 = Sab = Sbc = Sb = 0.0
    for b in range(B):
        nbc, nb = [0] * B, 0
        for a in range(B):
            nab = 0
            for c in range(B):
                n = int(N[a, b, c])
                S3 += phi[n]
                nab += n
                nbc[c] += n
            Sab += phi[nab]
            nb += nab
        for c in range(B):
            Sbc += phi[nbc[c]]
        Sb += phi[nb]
    te = ((S3 - Sab) - (Sbc - Sb)) / float(T)
    return (te if te > 0.0 else 0.0), (Sb - Sab) / float(T)


def test_names_are_public():
    assert features.window_transfer_entropy is window_transfer_entropy
    assert features.WINDOW_TE == transfer_entropy.WINDOW_TE == NAMES == tuple(_lib.WINDOW_TE)
    assert list(_lib.WINDOW_TE.values()) == list(range(4))
    assert _lib.WT_MAXBINS == 8 and _lib.WT_MAXLAG == 64 and _lib.WT_LONGEST == 4096
    doc = window_transfer_entropy.__doc__
    for name in NAMES + BINNINGS:
        assert f'"{name}"' in doc, name
    for word in ("fixed point", "+0.0", "MemoryError", "nothing is atomic", "searchsorted"):
        assert word in doc, word


def test_independent_rows_have_the_chi_square_bias():
    """2 T TE of independent rows is close to chi-square with B (B - 1)^2 degrees of freedom (B
    values of the bin before, each a (B - 1) x (B - 1) table), so the mean over 40 windows of B = 4
    is within about 4 % of B (B - 1)^2 / (2 T) at one sigma; 25 % is allowed."""
    rng = np.random.default_rng(21)
    W, B, nwin = 1024, 4, 40
    x = rng.standard_normal((2, W * nwin))
    for lag in (1, 3):
        M = window_te_measures(x, W, W, B, lag, "quantile")
        bias = B * (B - 1) ** 2 / (2 * (W - lag))
        free = M["te"][:, 0, 1].mean()
        print(f"lag {lag}: independent {free:.5f}, bias {bias:.5f}, ratio {free / bias:.3f}")
        assert abs(free - bias) <= 0.25 * bias


def driven_rows(lag, n, seed=22):
    """x white, y driven by x at ``lag``, z white and independent."""
    rng = np.random.default_rng(seed)
    x, z = rng.standard_normal(n), rng.standard_normal(n)
    return np.stack([x, driven(x, lag, rng), z])


def assert_driven_pair_is_seen(te_of, say=print):
    """te_of(rows, lag) -> te (nwin, 3, 3) of W = 1024, B = 4, quantile bins: the thresholds of the
    driven pair, for the restatement and for the device."""
    for u in (1, 3, 16):
        rows = driven_rows(u, 4 * 1024)
        at, past = te_of(rows, u).mean(axis=0), te_of(rows, u + 2).mean(axis=0)
        say(f"u = {u}: x->y {at[0, 1]:.4f}, y->x {at[1, 0]:.4f}, z->y {at[2, 1]:.4f}, x->y at u + 2 {past[0, 1]:.4f}")
        assert at[0, 1] > 0.25
        for other in (at[1, 0], at[2, 1], past[0, 1]):
            assert at[0, 1] > 5 * other


def test_a_driven_pair_is_seen_in_its_direction_and_at_its_lag():
    assert_driven_pair_is_seen(lambda rows, lag: window_te_measures(rows, 1024, 1024, 4, lag, "quantile")["te"])


def test_a_squared_drive_without_correlation_is_seen():
    """y_t = x_{t-2}^2 + 0.1 e_t: no correlation at the lag, a drive all the same.  The restatement
    reaches 0.558 nats under quantile bins and 0.063 under uniform ones (x^2 is skewed: most samples share
    the lowest of four equal parts of the range) at W = 4096 and B = 4; the floors are half of that."""
    rng = np.random.default_rng(23)
    W = 4096
    x = rng.standard_normal(W)
    y = np.concatenate([np.zeros(2), x[:-2] ** 2]) + 0.1 * rng.standard_normal(W)
    corr = np.corrcoef(x[:-2], y[2:])[0, 1]
    for binning, floor in (("quantile", 0.279), ("uniform", 0.0315)):
        te = window_te_measures(np.stack([x, y]), W, W, 4, 2, binning)["te"][0]
        print(f"{binning}: corr {corr:+.3f}, x->y {te[0, 1]:.4f}, y->x {te[1, 0]:.4f}")
        assert abs(corr) < 0.1 and te[0, 1] > 5 * te[1, 0] and te[0, 1] > floor


def test_the_conditioning():
    x = np.array(mixed(6, 1500, seed=5)) + 100.0
    for W, step, B, lag, binning in ((200, 100, 8, 1, "quantile"), (16, 16, 2, 1, "uniform"), (67, 200, 7, 5, "uniform"),
                                     (500, 500, 5, 64, "quantile")):
        M = window_te_measures(x, W, step, B, lag, binning)
        T, cnt = W - lag, M["counts"]
        assert np.all(cnt.sum(axis=(1, 2, 3)) == T)
        ab = cnt.sum(axis=3)                                  # (nwin, B, B, source, target)
        assert np.all(ab == ab[:, :, :, :1, :])               # the same for every source
        for k, s in enumerate(window_starts(x.shape[1], W, step)):
            code, _ = bin_codes(x[:, s:s + W], B, binning)
            for j in range(x.shape[0]):
                own = np.zeros((B, B))
                np.add.at(own, (code[j, lag:], code[j, lag - 1:W - 1]), 1)
                assert np.array_equal(ab[k, :, :, 0, j], own)
            for i, j in ((0, 1), (4, 2), (5, 0)):
                hc = conditional_entropy(cnt[k, :, :, :, i, j].astype(np.int64), T)
                assert M["te"][k, i, j] <= hc + 1e-15
        assert np.all(M["te"] >= 0) and np.all((M["nte"] >= 0) & (M["nte"] <= 1) | np.isnan(M["nte"]))
        assert np.array_equal(M["net"], -np.swapaxes(M["net"], 1, 2))
        if lag == 1:                                          # row 3 is row 0: x_{t-1} is y_{t-1}, which is given
            assert np.all(M["te"][:, 3, 0] <= 1e-15) and np.all(M["te"][:, 0, 3] <= 1e-15)


def test_rules_of_the_restatement():
    x = np.array(mixed(5, 1000, seed=3))
    x[2] = 7.5                                                # a constant channel
    x[0, 130] = np.nan
    x[1, 420] = -np.inf
    for binning in BINNINGS:
        M = window_te_measures(x, 100, 50, 4, 2, binning)
        k = np.arange(M["te"].shape[0])
        lost = np.zeros(M["te"].shape, dtype=bool)
        for row, at in ((0, 130), (1, 420)):
            hit = (k * 50 <= at) & (at < k * 50 + 100)
            lost[hit, row, :] = lost[hit, :, row] = True
        for name in ("te", "net"):
            assert np.array_equal(np.isnan(M[name]), lost), name
        assert np.array_equal(np.isnan(M["counts"]), np.broadcast_to(lost[:, None, None, None], M["counts"].shape))
        const = np.zeros(lost.shape, dtype=bool)
        const[:, 2, :] = const[:, :, 2] = True
        target = np.zeros(lost.shape, dtype=bool)
        target[:, :, 2] = True
        target[:, 2, 2] = False                               # (the diagonal is 0.0)
        assert np.array_equal(np.isnan(M["nte"]), lost | target)
        assert np.all(M["te"][const & ~lost] == 0.0)
        diag = np.broadcast_to(np.eye(5, dtype=bool), lost.shape)
        for name in NAMES[1:]:
            assert np.all(M[name][diag & ~lost] == 0.0), name


@pytest.mark.parametrize("shape", SHAPES)
def test_the_table_form_agrees_with_the_direct_sum(shape):
    nch, W, step, B, lag, binning, nwin = shape
    M = restated(shape)
    worst = 0.0
    for k in range(nwin):
        for i, j in ((0, 1), (1, 0), (nch - 2, nch - 1), (nch - 1, 0), (0, min(3, nch - 1))):
            te, hc = table_form(M["counts"][k, :, :, :, i, j].astype(np.int64), W, W - lag)
            worst = max(worst, abs(te - M["te"][k, i, j]))
            worst = max(worst, abs(hc - conditional_entropy(M["counts"][k, :, :, :, i, j].astype(np.int64), W - lag)))
    print(f"C={nch} W={W} B={B} lag={lag} {binning}: table - direct = {worst:.2e}")
    # at most B^3 + 2 B^2 + B <= 648 terms of size <= T ln T, each within an ulp, divided by T
    assert worst <= 648 * np.log(W) * 2.0 ** -52


def test_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(dev, "require_gpu", no_device)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="takes real data, got complex128 data"):
        window_transfer_entropy(x + 1j * x, 100)
    with pytest.raises(ValueError, match="two-dimensional.*stack at least two channels"):
        window_transfer_entropy(x[0], 100)
    with pytest.raises(ValueError, match="two-dimensional.*reshape"):
        window_transfer_entropy(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_transfer_entropy(x[:1], 100)
    with pytest.raises(ValueError, match="at least two channels"):
        window_transfer_entropy(x[:1].T, 100, axis=0)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_transfer_entropy(x, 501)
    cases = (({"winsize": 15}, "winsize"), ({"winsize": 100.0}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": 4097}, "winsize"), ({"winsize": 100, "step": 0}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "bins": 1}, "bins must be an integer from 2 to 8, got 1"),
             ({"winsize": 100, "bins": 9}, "bins must be an integer from 2 to 8, got 9"),
             ({"winsize": 100, "bins": 8.0}, "bins"), ({"winsize": 100, "bins": True}, "bins"),
             ({"winsize": 100, "lag": 0}, "lag must be an integer from 1 to 50, got 0"),
             ({"winsize": 200, "lag": 65}, "lag must be an integer from 1 to 64, got 65"),
             ({"winsize": 100, "lag": 51}, "lag must be an integer from 1 to 50, got 51"),
             ({"winsize": 100, "lag": 1.5}, "lag"), ({"winsize": 100, "lag": True}, "lag"),
             ({"winsize": 100, "binning": "equal"}, "binning must be one of.*quantile.*uniform.*got 'equal'"),
             ({"winsize": 100, "binning": 0}, "binning"),
             ({"winsize": 100, "measures": "TE"}, "counts.*te.*nte.*net"),
             ({"winsize": 100, "measures": ("te", "mi")}, "mi.*net"),
             ({"winsize": 100, "measures": ()}, "te"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_transfer_entropy(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_transfer_entropy(x, **kwargs)
    for shape, match in (((5000,), "two-dimensional"), ((2, 2, 5000), "two-dimensional"), ((1, 5000), "two channels"),
                         ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_transfer_entropy(src.pro, 100)
        assert not src.started

    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    with pytest.raises(ValueError, match="takes real data, got complex128 chunks"):
        window_transfer_entropy(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_transfer_entropy(x, 100, maxlag=4)                           # no such argument


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_te_work", "int64_t", 7), ("osz_window_te", "int", 16)):
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
    for name, value in _lib.WINDOW_TE.items():
        assert re.search(rf"OSZ_WT_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WT_COUNT = 4\b", header)
    assert re.search(rf"#define OSZ_WT_MAXBINS {_lib.WT_MAXBINS}\b", header)
    assert re.search(rf"#define OSZ_WT_MAXLAG {_lib.WT_MAXLAG}\b", header)
    assert re.search(rf"#define OSZ_WT_LONGEST {_lib.WT_LONGEST}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowte\.hip\b", makefile, re.M)
    assert callable(dev.window_te) and callable(dev.window_te_work)


# ---- the entry checks, through ctypes without a device (as tests/test_mi_host.py: the pointers are
# fake addresses nothing dereferences and every case has n < winsize, so a check that wrongly passed
# returns OSZ_OK, which fails the assertion, and cannot reach a launch)
X, CNT, OUT, WORK = 0x1000, 0x4000, 0x2000, 0x3000         # 16-byte aligned, never read
NCH, N, W0, PITCH = 3, 10, 64, 16


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def arguments(**change):
    a = dict(x=X, pitch=PITCH, nch=NCH, n=N, winsize=W0, step=5, bins=8, lag=1, binning=0, mask=15, counts=CNT, out=OUT,
             plane_pitch=0, work=WORK, work_len=None)
    a.update(change)
    assert a["n"] < a["winsize"], "every case is one without a window"
    return a


def work_of(lib, **change):
    a = arguments(**change)
    return lib.osz_window_te_work(a["nch"], a["n"], a["winsize"], a["step"], a["bins"], a["lag"], a["mask"])


def call(lib, **change):
    short = change.pop("short", 0)
    a = arguments(**change)
    if a["work_len"] is None:
        a["work_len"] = max(work_of(lib, **change), 0) + short
    status = lib.osz_window_te(a["x"], a["pitch"], a["nch"], a["n"], a["winsize"], a["step"], a["bins"], a["lag"],
                               a["binning"], a["mask"], a["counts"], a["out"], a["plane_pitch"], a["work"], a["work_len"],
                               None)
    return status, lib.osz_last_error().decode()


def expected_work(nch, W, bins, batch):
    """[phi: W + 1 rounded up to even] and per window of a batch 16 edges and 18 doubles per channel,
    Wpad bytes of codes and Wpad bytes of symbols per channel and (nch Bp^2) (nch Bp) int32."""
    bp = 1 << (bins - 1).bit_length()
    wpad = -(-W // 64) * 64
    return ((W + 2) & ~1) + batch * (nch * (16 + 18 + 2 * (wpad // 8)) + nch * nch * bp ** 3 // 2)


def test_the_work_space_query_needs_no_device(lib):
    work = lib.osz_window_te_work
    assert work(3, 1000, 100, 50, 4, 1, 0b1111) == expected_work(3, 100, 4, 19)
    assert work(3, 1000, 100, 50, 4, 50, 0b0010) == expected_work(3, 100, 4, 19)      # neither the mask nor the lag enters
    assert work(3, 1000, 100, 50, 5, 1, 0b1) == expected_work(3, 100, 8, 19)          # B = 5 is padded to 8
    assert work(256, 1 << 20, 1024, 1024, 8, 1, 0b10) == expected_work(256, 1024, 8, 2)   # two windows fill kGramCap
    assert 2 * 256 * 256 * 8 ** 3 // 2 == 1 << 25
    assert work(2, 16, 16, 16, 2, 8, 0b1) == expected_work(2, 16, 2, 1)
    assert work(3, 50, 100, 50, 4, 1, 0b1) == expected_work(3, 100, 4, 1)             # no window: one batch slot
    for bad in ((1, 1000, 100, 50, 4, 1, 1), (16385, 1000, 100, 50, 4, 1, 1), (3, -1, 100, 50, 4, 1, 1),
                (3, 1000, 15, 50, 4, 1, 1), (3, 10000, 4097, 50, 4, 1, 1), (3, 1000, 100, 0, 4, 1, 1),
                (3, 1000, 100, 50, 1, 1, 1), (3, 1000, 100, 50, 9, 1, 1), (3, 1000, 100, 50, -1, 1, 1),
                (3, 1000, 100, 50, 4, 0, 1), (3, 1000, 100, 50, 4, 51, 1), (3, 1000, 200, 50, 4, 65, 1),
                (3, 1000, 100, 50, 4, -2, 1), (3, 1000, 100, 50, 4, 1, 0), (3, 1000, 100, 50, 4, 1, 16)):
        assert work(*bad) == -1, bad


def test_valid_arguments_without_a_window_are_accepted(lib):
    status, msg = call(lib)
    assert status == _lib.OSZ_OK, msg
    for edge in (dict(nch=16384, winsize=16, n=15, pitch=16, bins=2, lag=8), dict(bins=8, binning=1, winsize=4096, lag=64),
                 dict(winsize=128, n=100, pitch=100, lag=64), dict(mask=1, out=None), dict(mask=14, counts=None)):
        status, msg = call(lib, **edge)                       # the ends of the ranges; arrays a mask leaves alone
        assert status == _lib.OSZ_OK and work_of(lib, **edge) >= 0, (edge, msg)


BAD = {
    "null x": (dict(x=None), "null", False),
    "null out": (dict(out=None), "null", False),
    "null counts": (dict(counts=None), "null", False),
    "null out, nte alone": (dict(out=None, mask=4), "null", False),
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
    "bins 9": (dict(bins=9), "bins 9", True),
    "bins -3": (dict(bins=-3), "bins -3", True),
    "lag 0": (dict(lag=0), "lag 0,", True),
    "lag 65": (dict(lag=65, winsize=200), "lag 65,", True),
    "lag past half the window": (dict(lag=33), "lag 33,", True),
    "lag -1": (dict(lag=-1), "lag -1,", True),
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
    assert msg.startswith("osz_window_te: ") and re.search(re.escape(says) + r"(?!\d)", msg), msg
    change.pop("short", None)
    assert (work_of(lib, **change) == -1) == planned


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_te_kernels_fit_their_budgets(tmp_path):
    """Every kernel of windowte.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled register of either kind, VGPRs + AGPRs <= 128 and static LDS <= 16 KB; and K25's kernels
    are not instantiated a second time."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowte.hip"), "-o", str(tmp_path / "windowte.o"),
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
    for part, count in (("te_symbol_kernel", 1), ("te_gram_kernel", 1), ("te_finish_kernel", 3), ("te_counts_kernel", 1),
                        ("mi_", 0)):
        assert sum(part in k for k in kernels) == count, sorted(kernels)
    assert len(kernels) == 6, sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 128
        assert int(use["LDS Size"]) <= 16 * 1024             # (static: the finish adds its table, at most 32.8 KB)
