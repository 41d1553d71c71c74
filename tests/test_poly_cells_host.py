"""Every compiled polyphase-resampler instance is accounted for, without a GPU: (1) the
poly_block_kernel instances and poly_kernel in the built library are exactly the corpus cells of
tests/poly_cells.py plus its UNREACHED list; (2) the corpus covers what it claims to (tails, stream
shapes, splits); (3) each entry's plan, as g++ builds it from the library's own planner
(poly_plan.h), is its declared cell and its declared tails; (4) each block-kernel entry's plan and
table G drive the NumPy restatement of poly_block_kernel against the definition in longdouble --
so a cell that fails only on the GPU (tests/test_gpu_poly_cells.py) is a kernel bug, not a table
bug.  The bound is the GPU test's: 1e-12 of max |reference|."""

import numpy as np
import pytest

import poly_cells as pc

TOL = 1e-12
BLOCK = [e for e in pc.CORPUS if e.cell != pc.FALLBACK]


@pytest.fixture(scope="module")
def exe():
    return pc.build_host_exe()


@pytest.fixture(scope="module")
def plans(exe):
    ps = pc.host_plans(exe, [(e.L, e.M, pc.taps_of(e), pc.centre_of(e)) for e in pc.CORPUS])
    return {pc.entry_id(e): p for e, p in zip(pc.CORPUS, ps)}


def test_inventory_is_corpus_plus_unreached():
    from openseize_amd import _lib
    compiled = pc.compiled_cells(_lib.LIB_PATH)
    assert len(compiled) == 11, sorted(compiled)          # ten block instances (3 + 3 + 2 + 2) and the fallback
    corpus = {e.cell for e in pc.CORPUS}
    unreached = set(pc.UNREACHED)
    assert not corpus & unreached
    assert all(isinstance(r, str) and r for r in pc.UNREACHED.values())
    assert corpus | unreached == compiled, (sorted(compiled - corpus - unreached), sorted((corpus | unreached) - compiled))
    assert unreached == {(1, 1, 128, 4)}


def test_corpus_ids_are_unique_and_taps_carry_weight():
    ids = [pc.entry_id(e) for e in pc.CORPUS]
    assert len(set(ids)) == len(ids)
    for e in pc.CORPUS:
        h = pc.taps_of(e)
        assert len(h) == e.ntaps
        if e.pad is None:
            assert np.all(h != 0.0), pc.entry_id(e)
        else:
            nz = np.flatnonzero(h)
            assert nz[0] > 0 and nz[-1] < len(h) - 1 and np.all(h[nz[0]:nz[-1] + 1] != 0.0)     # zeros in front and behind only
            assert e.centre != (e.ntaps - 1) // 2


def test_corpus_covers_what_the_kernels_can_do():
    by = {}
    for e in pc.CORPUS:
        by.setdefault(e.cell, []).append(e)
    cnts = {pc.entry_id(e): pc.stream_counts(e.L, e.M, e.ntaps, pc.centre_of(e)) for e in pc.CORPUS}
    for cell in pc.DAILY:
        es = by[cell]
        assert frozenset().union(*(e.tails for e in es)) == frozenset(range(8)), (cell, [sorted(e.tails) for e in es])
        cs = [cnts[pc.entry_id(e)] for e in es]
        assert any(0 < c.max() < 8 for c in cs), (cell, "no stream without a whole block")
        assert any(c.max() >= 32 for c in cs), (cell, "no stream of four whole blocks")
        assert any(len(set(c[r])) > 1 for c in cs for r in range(len(c))), (cell, "no class with two counts")
    for cell in (pc.R256, pc.R128, pc.R64):
        es = by[cell]
        few = [e for e in es if e.ntaps < e.L]
        assert few and all((cnts[pc.entry_id(e)].sum(1) == 0).any() for e in few), cell      # msub == 0 for some classes
        assert any(e.ntaps == 1 for e in es) and any(e.ntaps == 2 for e in es), cell
    # uneven phase-group splits: ph0, ph1 = eg M / EG
    for cell, Ms in ((pc.D128_2, (2,)), (pc.D64_2, (3,)), (pc.D64_4, (4, 5))):
        for M in Ms:
            assert any(e.M == M for e in by[cell]), (cell, M)
    assert any(e.M % 2 for e in by[pc.D128_2]) and any(e.M % 4 for e in by[pc.D64_4])
    for cell in (pc.D128, pc.D64):
        assert any((e.L, e.M) == (1, 1) for e in by[cell]), cell
    fb = by[pc.FALLBACK]
    assert any(e.L == 1 for e in fb) and any(e.L > 1 for e in fb)
    padded = [e for e in pc.CORPUS if e.pad is not None]
    assert {e.cell == pc.FALLBACK for e in padded} == {True, False}
    assert any((e.L, e.M, e.ntaps) == (1, 54, 1207) for e in by[pc.D64_4]) and any((e.L, e.M) == (1, 55) for e in fb)


@pytest.mark.parametrize("e", pc.CORPUS, ids=pc.entry_id)
def test_host_plan_is_the_declared_cell_and_tails(plans, e):
    p = plans[pc.entry_id(e)]
    assert pc.cell_of_plan(p) == e.cell, (e.cell, p)
    assert p["half"] == pc.centre_of(e) and p["H"] == (e.ntaps - 1 + e.L - 1) // e.L + 1
    cnt = pc.stream_counts(e.L, e.M, e.ntaps, p["half"])
    assert pc.tails_of(cnt) == e.tails, (sorted(pc.tails_of(cnt)), sorted(e.tails))
    coprime = np.gcd(e.L, e.M) == 1       # (else residue classes share their phase phi: taps met twice, others never)
    assert cnt.sum() == e.ntaps or not coprime                  # every tap in exactly one stream
    if e.cell == pc.FALLBACK:
        assert p["lds_bytes"] == 0 and p["G"] is None
        return
    assert p["lds_bytes"] <= (150 if p["NT"] == 64 else 53) * 1024
    assert cnt.max() <= p["apad"] and p["apad"] % 8 == 0
    # the table holds the taps of a stream in its first cnt places and padding behind them
    G = p["G"]
    filled = np.arange(p["apad"])[None, None, :] < cnt[:, :, None]
    assert np.all(G[~filled] == 0.0)
    if e.pad is None:
        assert np.all(G[filled] != 0.0)
    hL = e.L * pc.taps_of(e)
    assert np.array_equal(np.sort(G[filled]), np.sort(hL)) if coprime else np.isin(G[filled], hL).all()
    if (e.L, e.M, e.ntaps) == (1, 54, 1207):
        # the largest window the block kernel takes: 152496 B as planned, the pitch search may add
        assert 152496 <= p["lds_bytes"] <= 150 * 1024


def _check(p, h, n, seed):
    x = np.random.default_rng(seed).standard_normal(n)
    got, fast = pc.block_model(p, x)
    ref = pc.definition(x, h, p["L"], p["M"], p["half"])[0]
    assert got.shape == ref.shape
    scale = np.max(np.abs(ref))
    err = float(np.max(np.abs(got - ref))) / float(scale) if scale > 0 else float(np.max(np.abs(got)))
    return err, fast


@pytest.mark.parametrize("e", BLOCK, ids=pc.entry_id)
def test_dataflow_model_of_the_entry_against_the_definition(plans, e):
    """One push of a stream that gives the first tile a window reaching before the stream, one tile
    its whole window inside it (the descriptor walk) and a ragged last tile."""
    p = plans[pc.entry_id(e)]
    n = pc.first_push(p) + int(0.3 * p["NT"] * pc.R * e.M) + 5
    err, fast = _check(p, pc.taps_of(e), n, e.ntaps)
    assert fast >= e.L, (pc.entry_id(e), fast)
    assert err < TOL, (pc.entry_id(e), err)


def test_dataflow_model_exhaustive_small(exe):
    """Every (L, M, ntaps, centre) with L, M <= 6 and ntaps <= 20."""
    rng = np.random.default_rng(7)
    keys = [(L, M, m, c) for L in range(1, 7) for M in range(1, 7) for m in range(1, 21) for c in range(m)]
    taps = {m: rng.standard_normal(m) / np.sqrt(m) for m in range(1, 21)}
    ps = pc.host_plans(exe, [(L, M, taps[m], c) for L, M, m, c in keys])
    worst = (0.0, None)
    for (L, M, m, c), p in zip(keys, ps):
        assert p["kernel"] == 1 and p["half"] == c
        err, _ = _check(p, taps[m], 29 + M, m)
        worst = max(worst, (err, (L, M, m, c)), key=lambda t: t[0])
    assert worst[0] < TOL, worst


def test_schedule_of_the_gpu_test_reaches_the_descriptor_path(plans):
    """The first push of the GPU test's ragged stream stages one tile through the buffer descriptor,
    the stream stays small, and the later pushes are the short ones they are meant to be."""
    for e in pc.CORPUS:
        p = plans[pc.entry_id(e)]
        n, lens = pc.schedule(p, None if e.pad is None else e.pad[1])
        assert sum(lens) == n and min(lens) >= 0 and lens[6] > 0, (pc.entry_id(e), n, lens)
        assert lens[1:6] == [1, 0, p["H"] - 1, p["H"] - 1, e.M - 1] and lens[7] == 5
        assert n <= 52000, (pc.entry_id(e), n)
        if p["kernel"]:
            nout = -(-(lens[0] * e.L - p["half"]) // e.M)
            assert pc.descriptor_classes(p, 0, lens[0], 0) >= e.L, pc.entry_id(e)
            assert nout > p["NT"] * pc.R * e.L
