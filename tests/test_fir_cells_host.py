"""Every compiled instance of the stand-alone FIR is accounted for, without a GPU: (1) the
fir_nega_kernel and fir_oa_kernel instances in the built library are exactly the corpus cells of
tests/fir_cells.py plus its UNREACHED list; (2) each entry's plan for every push of its schedule, as
g++ builds it from the library's own planner (fir_plan.h), is its declared cells and the Python
restatement of the planner, and the invariant the seam kernel rests on holds over a grid; (3) the
schedules reach the cases they are there for; (4) the rounded-FFT reference is the exact one;
(5) the GPU test's bound would catch a dropped or a misplaced tap."""

import numpy as np
import pytest

import fir_cells as fc

TOL = 1e-12          # the bound of tests/test_gpu_fir_cells.py


@pytest.fixture(scope="module")
def exe():
    return fc.build_host_exe()


def _pushes(e):
    if e.kind == "narrow":
        return fc.narrow_schedule(e)
    if e.kind == "wide":
        return fc.wide_schedule(e)
    n, out = fc.part_length(e), []
    for cs in fc.part_chunkings(e):
        out += [n] if cs is None else sorted({cs, n % cs} - {0})
    return out


def test_inventory_is_corpus_plus_unreached():
    from openseize_amd import _lib
    compiled, triples = fc.compiled_cells(_lib.LIB_PATH)
    nega = {c for c in compiled if c[0] == "nega"}
    pair = {c for c in compiled if c[0] == "pair"}
    assert nega == {("nega", nb) for nb in range(24, 32)}, sorted(nega)
    assert len(pair) == len(triples) == 24, sorted(triples)      # 8 block heights x 3 variants
    # the variants as compiled: 0 with the spectrum resident, 1 and 2 with it requested per pair
    assert triples == {(nr, -1 if pf == 0 else 16, pf) for nr in range(8, 16) for pf in (0, 1, 2)}, sorted(triples)
    corpus = {c for e in fc.CORPUS for c in e.cells}
    unreached = set(fc.UNREACHED)
    assert not corpus & unreached
    assert all(isinstance(r, str) and r for r in fc.UNREACHED.values())
    assert corpus | unreached == compiled, (sorted(compiled - corpus - unreached), sorted((corpus | unreached) - compiled))
    assert len(unreached) == 23 and corpus & pair == {fc.PAIR}
    assert fc.PAIR[2] == fc.pf_table()[fc.PAIR[1]]               # the variant OSZ_FIR_PF_TABLE names


def test_corpus_is_what_it_says():
    ids = [fc.entry_id(e) for e in fc.CORPUS]
    assert len(set(ids)) == len(ids)
    narrow = {e.ntaps: e.cells for e in fc.NARROW}
    for nb in range(24, 32):
        lo, hi = max(2, 8193 - 256 * (nb + 1) + 1), 8193 - 256 * nb
        assert narrow[lo] == narrow[hi] == (("nega", nb),), (nb, lo, hi)
        assert nb == 24 or fc.piece_plan(hi + 1)[:2] == ("nega", nb - 1)
    assert narrow[1] == (fc.PAIR,) and all(e.nch == 3 for e in fc.NARROW)
    assert [(e.ntaps, e.nch) for e in fc.WIDE] == [(1794, 64), (1026, 64), (2, 64), (1, 64), (4097, 64)]
    assert [(e.ntaps, e.nch) for e in fc.PARTITIONED] == [(t, 2) for t in (2050, 4096, 4097, 6145, 32768)]
    assert [e.cells[0] for e in fc.one_per_cell()] == [("nega", nb) for nb in range(31, 23, -1)] + [fc.PAIR]
    for e in fc.CORPUS:
        h, x = fc.taps_of(e), fc.data_of(e, 1000)
        assert len(h) == e.ntaps and np.all(h != 0) and np.all(h == np.rint(h)) and np.abs(h).max() <= 8
        assert x.shape == (e.nch, 1000) and np.all(x == np.rint(x)) and np.abs(x).max() == 8
        assert len(fc.pieces_of(e.ntaps)) == len(e.cells)
    assert len(fc.pieces_of(32768)) == 16 and fc.part_chunkings(fc.PARTITIONED[-1])[0] < fc.PART


@pytest.mark.parametrize("e", fc.CORPUS, ids=fc.entry_id)
def test_host_plan_is_the_declared_cells_and_the_restatement(exe, e):
    pushes = _pushes(e)
    plans = fc.host_plans(exe, [(e.ntaps, e.nch, fc.CUS, n) for n in pushes])
    for n, plan in zip(pushes, plans):
        assert tuple(fc.cell_of_record(p) for p in plan) == e.cells, (fc.entry_id(e), n, plan)
        want = fc.expected_records(e, n, 0, fc.CUS)
        assert plan == [{k: r[k] for k in fc._KEYS} for r in want], (fc.entry_id(e), n)
        assert sum(p["taps"] for p in plan) == e.ntaps


def test_host_plan_over_other_machines(exe):
    """The restatement against the header where the round search matters: other CU counts and widths."""
    cases = [(t, c, cus, n) for t in (1, 2, 1025, 2049, 4097) for c in (1, 3, 16, 64, 200, 256)
             for cus in (1, 80, 256, 304) for n in (1, 3839, 3840, 50_000, 400_001, 3_000_000)]
    for (t, c, cus, n), plan in zip(cases, fc.host_plans(exe, cases)):
        e = fc.Entry(t, c, "narrow", tuple(fc.cell_of_record(p) for p in plan))
        assert plan == [{k: r[k] for k in fc._KEYS} for r in fc.expected_records(e, n, 0, cus)], (t, c, cus, n)


def test_seam_invariant_over_the_grid(exe):
    rc, checked, lines = fc.host_grid(exe)
    assert rc == 0, lines
    assert checked == 18 * 200 * 6 * 4 * 3


@pytest.mark.parametrize("e", fc.NARROW, ids=fc.entry_id)
def test_narrow_schedule_reaches_the_seams(e):
    S, w = fc.last_step(e), e.ntaps - 1
    lens = fc.narrow_schedule(e)
    plans = [fc.expected_records(e, n, 0, fc.CUS)[0] for n in lens]
    assert lens[0] == 5 * S and plans[0]["nruns"] == 2                        # whole blocks only, in two runs
    assert any(n % S == 0 for n in lens) and any(n % S == S - 1 for n in lens)
    if w > 0:
        assert any(n % S == w and n > S for n in lens)                        # a last block of exactly the tail
    if w > 1:
        assert any(n > S and 0 < n % S < w for n in lens)                    # a last block shorter than the tail
        # pushes shorter than the tail, back to back, in one run: part of the old state outlives them
        k = lens.index(w - 1)
        assert lens[k + 1] == w - 1 and lens[k - 1] == 1
        assert all(plans[j]["nruns"] == 1 and lens[j] < w for j in (k - 1, k, k + 1))
    else:
        assert len(lens) == 7 and plans[1]["nruns"] == 1 and lens[1] == 1    # (no push can be shorter than a tail of w <= 1)
    assert sum(lens) <= 160_000


@pytest.mark.parametrize("e", fc.WIDE, ids=fc.entry_id)
def test_wide_first_push_has_runs_of_three_whole(e):
    n = fc.wide_schedule(e)[0]
    recs = fc.expected_records(e, n, 0, fc.CUS)
    assert n == fc.WIDE_BLOCKS * recs[-1]["step"]
    for r in recs:
        assert max(fc.whole_per_run(r)) >= 3, (fc.entry_id(e), r, fc.whole_per_run(r))
    if e.ntaps == 4097:
        # the issue's figure: the single tap's piece runs 8 runs of 3 pairs at 64 channels, 256 CUs
        assert recs[-1]["nruns"] == 8 and fc.whole_per_run(recs[-1]) == [3] * 8 and recs[-1]["accum"] == 1
    n2 = fc.wide_schedule(e)[1]
    assert 0 < n2 % recs[-1]["step"] < recs[-1]["step"] - 1                  # the second push is ragged


def test_narrow_pair_runs_hold_one_pair_only():
    """Why the wide entries exist: with few channels the planner cuts a run per pair of blocks."""
    e = next(e for e in fc.NARROW if e.ntaps == 1)
    for c, n in ((3, 200_003), (3, 150_001), (2, 30_011)):
        r = fc.expected_records(fc.Entry(1, c, "narrow", e.cells), n, 0, fc.CUS)[0]
        assert max(fc.whole_per_run(r)) == 1, (c, n, r)


FFT = [e for e in fc.CORPUS if fc.uses_fft(e)]


@pytest.mark.parametrize("e", FFT, ids=fc.entry_id)
def test_rounded_fft_reference_is_the_exact_one(e):
    x, ref, scale = fc.clean(e)
    raw = fc.fft_unrounded(x, fc.taps_of(e))
    dist = float(np.max(np.abs(raw - np.rint(raw))))
    print(f"{fc.entry_id(e)}: FFT within {dist:.2e} of an integer, scale {scale:.0f}")
    assert dist < 1e-6
    assert np.array_equal(ref, np.rint(raw)) and ref.shape == (e.nch, x.shape[1] + e.ntaps - 1)
    assert np.array_equal(ref[0], fc.exact(x[:1], fc.taps_of(e))[0].astype(np.float64))
    assert scale < 2.0 ** 40 and 64.0 * e.ntaps < 2.0 ** 53               # |x|, |h| <= 8: every sum is exact


@pytest.mark.parametrize("e", fc.CORPUS, ids=fc.entry_id)
def test_bound_catches_a_dropped_or_misplaced_tap(e):
    """One channel of the entry's stream: the reference without its last tap, and the reference one
    sample late, are further than 1e-4 of the scale from the true one."""
    x, ref, scale = fc.clean(e)
    h = fc.taps_of(e)
    n = min(x.shape[1], 60_000)
    true = fc.exact(x[:1, :n], h)[0].astype(np.float64)
    assert np.array_equal(true[:n], ref[0, :n])
    dropped = true.copy()
    dropped[e.ntaps - 1:] -= h[-1] * x[0, :n]                                # (integers: exact)
    shifted = np.concatenate([[0.0], true[:-1]])
    for name, wrong in (("dropped", dropped), ("shifted", shifted)):
        miss = float(np.max(np.abs(wrong - true))) / scale
        assert miss > 1e-4 > TOL, (fc.entry_id(e), name, miss)
