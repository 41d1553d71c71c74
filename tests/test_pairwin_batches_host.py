"""tests/pairwin_batches.py checked without a GPU: (1) the restated planner asks for the work space
the built library asks for, and every case of the corpus crosses the batch edges it is here for -- a
case that drifts to one batch after a constant changes fails here, not silently on the GPU; (2) the
restatements of the four host modules are reachable at the picks of every case: finite, the caps
finite, the peaks of K23 clear of ties, and for K24 and K25 the float64 form within RTOL / 32 of the
long-double one, so the cap hides nothing on these inputs; (3) ``check`` raises for five defects of a
batch walk planted into a float64 "device result" of a toy stream, and passes without them."""

import ctypes
import os
import re
from functools import lru_cache

import numpy as np
import pytest

import pairwin_batches as pb
from openseize_amd import _lib
from test_connectivity_host import RTOL, shifted_scheme


# ------------------------------------------------------------------ (1) the planner
def work_query(case, nwin=None):
    lib = ctypes.CDLL(_lib.LIB_PATH)                         # the queries need no device
    fn = getattr(lib, f"osz_window_{case.kernel}_work")
    fn.restype, fn.argtypes = _lib.SIGNATURES[f"osz_window_{case.kernel}_work"]
    n = pb.samples(case, nwin)
    if case.kernel == "pairs":
        mask = sum(1 << _lib.WINDOW_CONNECTIVITY[name] for name in case.names)
        return fn(case.nch, n, case.W, pb.STEP, mask, int(case.cplx))
    table = {"xcorr": _lib.WINDOW_XCORR, "granger": _lib.WINDOW_GRANGER, "mi": _lib.WINDOW_MI}[case.kernel]
    return fn(case.nch, n, case.W, pb.STEP, case.param, sum(1 << table[name] for name in case.names))


def test_the_constants_are_the_librarys():
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    head = open(os.path.join(csrc, "pair_window.h")).read()
    assert re.search(r"kGramCap = \(int64_t\)1 << 25;", head) and pb.GRAM_CAP == 1 << 25
    assert re.search(r"batch > 65535 \? 65535", head) and pb.GRID_Y == 65535
    mi = open(os.path.join(csrc, "windowmi.hip")).read()
    assert re.search(r"\bkMiEdges = OSZ_WM_MAXBINS;", mi) and pb.MI_EDGES == _lib.WM_MAXBINS
    assert re.search(r"\bkMiMeta = OSZ_WM_MAXBINS \+ 2;", mi) and pb.MI_META == _lib.WM_MAXBINS + 2
    assert re.search(r"\bkMiStep = 64;", mi) and pb.MI_STEP == 64
    assert pb.WC_BLOCK == _lib.WC_BLOCK


@pytest.mark.parametrize("case", pb.CASES, ids=lambda c: c.key)
def test_the_restated_planner_is_the_librarys_and_the_case_crosses_its_edges(case):
    P = pb.plan_of(case)
    nbatch, binds, batch = case.want
    print(f"{case.key}: nwin {P.nwin}, one {P.one}, batch {P.batch} ({P.binds}), batches {P.batches}, work {P.work}")
    assert P.work == work_query(case), (case.key, P.work, work_query(case))
    assert P.nwin == case.nwin and P.batch == batch and P.binds == binds, (case.key, P)
    assert len(P.batches) == nbatch >= 2, (case.key, P.batches)
    assert [w0 for w0, _ in P.batches] == [k * batch for k in range(nbatch)]
    assert all(count == batch for _, count in P.batches[:-1]) and 0 < P.batches[-1][1] < batch
    assert sum(count for _, count in P.batches) == P.nwin
    at = pb.picks(P.batches)
    for w0, count in P.batches:
        assert (w0 == 0 or {w0 - 1, w0} <= set(at)) and any(w0 < w < w0 + count - 1 or count <= 2 for w in at)
    assert at[0] == 0 and at[-1] == P.nwin - 1 and len(at) <= 3 * nbatch
    # which limit binds, from the formulas and not from the planner's word alone
    raw = pb.GRAM_CAP // P.one
    if binds == "gram":
        assert batch == raw < pb.GRID_Y
    elif binds == "grid":
        assert batch == pb.GRID_Y < raw
    else:
        assert batch < min(raw, pb.GRID_Y)
    # one batch's windows alone are one batch, and so is every part of the GPU test; the planner holds
    # for them and for a stream that ends on the edge too
    for w0, count in P.batches:
        part = pb.plan_of(case, count)
        assert part.batches == [(0, count)] and part.work == work_query(case, count), (case.key, count)
    for nwin in (batch, batch + 1):
        edge = pb.plan_of(case, nwin)
        assert len(edge.batches) == (1 if nwin == batch else 2) and edge.work == work_query(case, nwin), (case.key, nwin)


def test_the_figures_of_the_corpus():
    """The batch sizes as derived by hand from the planner's rule: 2^25 // one, 1 .. 65535, K25's cap."""
    def batch(key):
        return pb.plan_of(pb.BY_KEY[key]).batch
    assert batch("three-xcorr") == (1 << 25) // (129 * 34 * 34) == 225
    assert batch("three-granger") == (1 << 25) // (33 * 34 * 34) == 879
    assert batch("three-mi") == (1 << 25) // (128 * 34 * 34) == 226 < (1 << 25) // ((16 + 18 + 16) * 34)
    assert batch("three-pairs-complex") == (1 << 25) // (9 * 4 * 18 * 18) == 2876
    assert batch("two-pairs-real-ddof0") == batch("two-pairs-real-ddof1") == (1 << 25) // (9 * 18 * 18) == 11507
    assert batch("gram-xcorr-two-channels") == (1 << 25) // (129 * 4) == 65027
    assert batch("staging-mi") == (1 << 25) // ((16 + 18 + 4096 // 8) * 2) == 30727
    assert pb.BY_KEY["two-pairs-real-ddof0"].nwin == pb.BY_KEY["two-pairs-real-ddof1"].nwin == 11509
    assert pb.BY_KEY["staging-mi"].nwin == 30730 and pb.BY_KEY["gram-xcorr-two-channels"].nwin == 65030
    assert pb.samples(pb.BY_KEY["three-xcorr"]) == 578 and pb.samples(pb.BY_KEY["three-granger"]) == 1886
    assert pb.samples(pb.BY_KEY["three-mi"]) == 517 and pb.samples(pb.BY_KEY["three-pairs-complex"]) == 13945
    assert {c.kernel for c in pb.THREE} == {c.kernel for c in pb.DIRECT} == {"pairs", "xcorr", "granger", "mi"}
    assert len(pb.THREE) == 4 and len(pb.DIRECT) == 7 and all(c.nwin == 65538 for c in pb.DIRECT if c.want[1] == "grid")


# ------------------------------------------------------------------ (2) the references are reachable
def table_mi(counts, W):
    """mi and joint (C, C) from counts (B, B, C, C) by the kernel's formula in float64: phi(n) = n ln n
    from a table, ln W as phi(W) / W (``table_form`` of tests/test_mi_host.py, every pair at once)."""
    phi = np.zeros(W + 1)
    phi[1:] = np.arange(1, W + 1) * np.log(np.arange(1, W + 1))
    N = counts.astype(np.int64)
    nch = N.shape[-1]
    d = np.arange(nch)
    marg = N[:, :, d, d].sum(axis=1)                         # (B, C): the diagonal pair holds n_a on a = b
    H = (phi[W] - phi[marg].sum(axis=0)) / W
    hij = (phi[W] - phi[N].sum(axis=(0, 1))) / W
    mi = np.maximum((H[:, None] + H[None, :]) - hij, 0.0)
    mi[d, d] = hij[d, d] = H
    return mi, hij


@pytest.mark.parametrize("case", pb.CASES, ids=lambda c: c.key)
def test_the_restatements_are_reachable_at_the_picks(case):
    x = pb.stream(case)
    at = pb.picks(pb.plan_of(case).batches)
    assert x.shape == (case.nch, pb.samples(case)) and np.iscomplexobj(x) == case.cplx
    want, cap = pb.references(case, x, at)
    for name, shape in pb.shapes(case, len(at)).items():
        assert want[name].shape == shape and want[name].dtype == np.float64, (name, want[name].shape)
        alive = np.isfinite(want[name])
        if case.kernel == "mi" and name == "nmi":             # NaN where a row is constant in its window
            assert np.array_equal(~alive, np.isnan(want[name]))
        else:
            assert alive.all(), (case.key, name)
        if cap[name] is not None:
            assert cap[name].shape == shape and np.all(np.isfinite(cap[name])) and np.all(cap[name] > 0), (case.key, name)
    if case.kernel == "xcorr":
        margin = pb.lag_margin(case, x, at)
        print(f"{case.key}: the peak leads by {margin:.2e} caps")
        assert margin > 2.0, (case.key, margin)
    if case.kernel == "granger":
        plain, _ = pb.references(case, x, at, np.float64)
        for name in case.names:
            gap = float(np.max(np.abs(plain[name] - want[name])))
            print(f"{case.key} {name}: float64 - long double = {gap:.2e}")
            assert gap <= RTOL / 32, (case.key, name, gap)
    if case.kernel == "mi":
        full = want if "counts" in want else pb.references(case._replace(names=("counts",) + case.names), x, at)[0]
        for k in range(len(at)):
            mi, joint = table_mi(full["counts"][k], case.W)
            for name, v in (("mi", mi), ("joint", joint)):
                gap = float(np.max(np.abs(v - want[name][k])))
                assert gap <= RTOL / 32, (case.key, name, at[k], gap)


# ------------------------------------------------------------------ (3) mutants
TOY = pb.Case("toy", "pairs", 3, 16, 1, None, pb.REAL, False, 11, (3, "gram", 5))
TOY_BATCHES = [(0, 5), (5, 5), (10, 1)]
SENTINEL = -7.0


@lru_cache(maxsize=None)
def toy():
    """(x, whole, parts, at, refs) of the toy stream: the float64 scheme of the device as its result."""
    x = pb.stream(TOY) + 100.0
    whole = shifted_scheme(x, TOY.W, pb.STEP, TOY.param)
    parts = [(w0, shifted_scheme(x[:, pb.batch_columns(TOY, w0, count)], TOY.W, pb.STEP, TOY.param))
             for w0, count in TOY_BATCHES]
    at = pb.picks(TOY_BATCHES)
    return x, whole, parts, at, pb.references(TOY, x, at)


def sums_from(x, W, shift):
    """``shifted_scheme`` for real rows with the per-channel sums of window k taken from window k -
    shift[k]: the defect of a ``chan`` indexed batch-relative where it is absolute."""
    nwin = x.shape[1] - W + 1
    out = {name: np.empty((nwin, x.shape[0], x.shape[0])) for name in pb.REAL}
    for k in range(nwin):
        w, v = x[:, k:k + W], x[:, k - shift[k]:k - shift[k] + W]
        d = w - w[:, :1]
        S, G = (v - v[:, :1]).sum(axis=1), d @ d.T
        cov = W * G - S[:, None] * S[None, :]
        sd = np.sqrt(np.diag(cov))
        out["cov"][k] = cov / (W * (W - 1))
        out["corr"][k] = np.clip(cov / (sd[:, None] * sd[None, :]), -1, 1)
        np.fill_diagonal(out["corr"][k], 1.0)
    return out


def mutants():
    x, whole, parts, at, refs = toy()

    def late(M):                                             # the second batch one window late
        M[6:11] = M[5:10].copy()
        M[5] = SENTINEL

    def relative(M):                                         # the second batch over the first
        M[0:5] = M[5:10].copy()
        M[5:10] = SENTINEL

    def last_bit(M):                                         # one element of the last batch, one ulp
        M[10, 1, 2] = np.nextafter(M[10, 1, 2], np.inf)

    def unwritten(M):                                        # the last, shorter batch never launched
        M[10] = SENTINEL

    found = {}
    for name, edit in (("late", late), ("relative", relative), ("last-bit", last_bit), ("unwritten", unwritten)):
        found[name] = {k: v.copy() for k, v in whole.items()}
        for k in found[name] if name != "last-bit" else ("cov",):
            edit(found[name][k])
    shift = np.zeros(11, dtype=int)
    shift[5:10] = 5
    found["sums"] = sums_from(x, TOY.W, shift)
    return found


def split(M):
    return [(w0, {k: v[w0:w0 + count] for k, v in M.items()}) for w0, count in TOY_BATCHES]


def test_check_passes_on_the_toy_stream():
    x, whole, parts, at, refs = toy()
    assert at == [0, 2, 4, 5, 7, 9, 10]
    ratios = pb.check(TOY, whole, parts, at, refs, say=print)
    assert set(ratios) == set(pb.REAL) and max(ratios.values()) < 1e-3
    clean = sums_from(x, TOY.W, np.zeros(11, dtype=int))     # the mutants' scheme without the defect
    pb.check(TOY, clean, split(clean), at, refs)


@pytest.mark.parametrize("name", ["late", "relative", "sums", "last-bit", "unwritten"])
def test_check_raises_for_a_defect_of_the_batch_walk(name):
    x, whole, parts, at, refs = toy()
    M = mutants()[name]
    with pytest.raises(AssertionError, match="differ from the call over their own samples"):
        pb.check(TOY, M, parts, at, refs)                    # (a): against the batches run alone
    if name == "last-bit":                                   # one ulp is (a)'s alone to see
        pb.check(TOY, M, split(M), at, refs)
        return
    with pytest.raises(AssertionError, match="of the cap at window"):
        pb.check(TOY, M, split(M), at, refs)                 # (b): with (a) blinded, the picks still see it


def test_check_wants_every_window_and_every_finite_result():
    x, whole, parts, at, refs = toy()
    with pytest.raises(AssertionError, match="the parts hold"):
        pb.check(TOY, whole, parts[:2], at, refs)
    with pytest.raises(AssertionError, match="not in order"):
        pb.check(TOY, whole, [parts[0], parts[2]], at, refs)
    M = {k: v.copy() for k, v in whole.items()}
    M["corr"][5, 0, 1] = np.nan                              # a read outside the stream's columns
    with pytest.raises(AssertionError, match="not finite at windows"):
        pb.check(TOY, M, split(M), at, refs)
    assert pb.same_bits(np.array([np.nan, 0.0]), np.array([-np.nan, 0.0]))
    assert not pb.same_bits(np.array([0.0]), np.array([-0.0])) and not pb.same_bits(np.zeros(2), np.zeros(3))
