"""Every compiled chain-kernel instance is accounted for, without a GPU: (1) the instances of the
five families in the built library are exactly the corpus cells of tests/chain_cells.py plus its
UNREACHED list; (2) each corpus entry's plan, as g++ builds it from the library's own planner
(spec_tables.h), is its declared cell; (3) each corpus entry's tables drive the NumPy restatement
of its kernel's dataflow against scipy, at the tolerances of tests/test_spec_host.py -- so a cell
that fails only on the GPU (tests/test_gpu_chain_cells.py) is a kernel bug, not a table bug."""

import numpy as np
import pytest
import scipy.signal as sps

import chain_cells as cc

MODELLED = [c for c in cc.CORPUS if c.cell[0] != "scan"]     # (the time scan has no tables)


@pytest.fixture(scope="module")
def exe():
    return cc.build_host_exe()


def test_inventory_is_corpus_plus_unreached():
    from openseize_amd import _lib
    compiled = cc.compiled_cells(_lib.LIB_PATH)
    assert len(compiled) == 253, len(compiled)       # 126 + 63 + 24 + 24 + 16
    corpus = [c.cell for c in cc.CORPUS]
    assert len(set(corpus)) == len(corpus), "a cell twice in the corpus"
    unreached = set(cc.UNREACHED)
    assert not set(corpus) & unreached
    assert all(isinstance(r, str) and r for r in cc.UNREACHED.values())
    assert set(corpus) | unreached == compiled, (sorted(compiled - set(corpus) - unreached),
                                                 sorted((set(corpus) | unreached) - compiled))


@pytest.mark.parametrize("c", cc.CORPUS, ids=cc.cell_id)
def test_host_plan_is_the_declared_cell(exe, c):
    p = cc.host_plan(exe, cc.fir_taps(c.taps, c.cutoff), cc.design_sos(*c.design))
    got = dict(cc.cells_of_plan(p))
    assert c.cell in got, (c.cell, got)
    # the recorded fit ratio (what the GPU test's tolerance comes from) is still the planner's
    assert got[c.cell] == pytest.approx(c.ratio, rel=1e-3)


def _stream(sos, taps, lens, seed):
    x = np.random.default_rng(seed).standard_normal(sum(lens))
    u = np.convolve(x, taps)
    zi0 = sps.sosfilt_zi(sos) * u[0]
    return x, u, zi0


def _zpn(exe, taps, sos):
    T = cc.tables_zp(exe, taps, sos, mode="zpn")
    assert T["eligible"]
    m = cc.ModelZpn(T)
    S, L = m.S, m.L
    lens = [S * 5 + 1024, S * 4, S * 3 + S - 17, S + 5, S * 3 + S, S * 3 + 300, 2 * S]
    x, u, zi0 = _stream(sos, taps, lens, len(taps))
    f, _ = sps.sosfilt(sos, u, zi=zi0)
    ref = sps.sosfilt(sos, np.concatenate([f, np.zeros(32768)])[::-1])[::-1][:len(f)]
    zir = sps.sosfilt(sos, np.zeros(7680), zi=zi0)[0]
    carry, held = sps.sosfilt(sos, zir[::-1])[::-1], np.zeros(L)
    out, o = [], 0
    for k, n in enumerate(lens):
        y, carry, held = m.chunk(x[o:o + n], carry, held, nruns=[1, 2, 3, 1, 2, 2, 1][k])
        out.append(y)
        o += n
    got = np.concatenate(out)
    assert np.isfinite(got).all()
    tol = max(3e-12, 1e-16 / T["ratio"])
    return np.max(np.abs(got[L:] - ref[:len(got) - L])) / np.max(np.abs(ref)), tol


def _zp(exe, taps, sos):
    T = cc.tables_zp(exe, taps, sos)
    assert T["eligible"]
    m = cc.ModelZp(T)
    S, L = m.S, m.L
    lens = [2 * S * 5 + 1024, 2 * S * 4, 2 * S * 3 + S + 17, 2 * S + 5, 2 * S * 3 + 2 * S - 1, 2 * S * 3 + 300]
    x, u, zi0 = _stream(sos, taps, lens, len(taps))
    f, _ = sps.sosfilt(sos, u, zi=zi0)
    ref = sps.sosfilt(sos, np.concatenate([f, np.zeros(8192)])[::-1])[::-1][:len(f)]
    zir = sps.sosfilt(sos, np.zeros(7680), zi=zi0)[0]
    carry, held = sps.sosfilt(sos, zir[::-1])[::-1], np.zeros(L)
    out, o = [], 0
    for k, n in enumerate(lens):
        y, carry, held = m.chunk(x[o:o + n], carry, held, nruns=[1, 2, 3, 1, 2, 2][k])
        out.append(y)
        o += n
    got = np.concatenate(out)
    assert np.isfinite(got).all()
    return np.max(np.abs(got[L:] - ref[:len(got) - L])) / np.max(np.abs(ref)), 1e-12


def _fwd(exe, taps, sos):
    T = cc.tables_zp(exe, taps, sos, mode="specn")
    assert T["eligible"]
    m = cc.ModelSpecN(T)
    S = m.S
    lens = [S * 5 + 1024, S * 4, S * 3 + S - 17, S + 5, S * 3 + S, 2 * S]
    x, u, zi0 = _stream(sos, taps, lens, len(taps))
    ref, _ = sps.sosfilt(sos, u, zi=zi0)
    carry = np.zeros(7680)
    cl = 4096 + 256 * T["Rf"]
    carry[:cl] = sps.sosfilt(sos, np.zeros(cl), zi=zi0)[0]
    err, o, scale = 0.0, 0, np.max(np.abs(ref))
    for k, n in enumerate(lens):
        f, carry = m.chunk(x[o:o + n], carry, nruns=[1, 2, 3, 1, 2, 1][k])
        err = max(err, np.max(np.abs(f - ref[o:o + n])) / scale)
        o += n
    err = max(err, np.max(np.abs(carry[:len(taps) - 1] - ref[o:o + len(taps) - 1])) / scale)
    return err, max(1e-12, 1e-16 / T["ratio"])


def _spec(exe, taps, sos):
    T = cc.tables(exe, taps, sos)
    assert T["eligible"]
    m = cc.Model(T, len(taps))
    S = m.S
    lens = [2 * S * 5 + 1024, 2 * S * 4, 2 * S * 3 + S + 17, 2 * S + 5, 2 * S * 3 + 2 * S - 1]
    x, u, zi0 = _stream(sos, taps, lens, len(taps))
    ref, _ = sps.sosfilt(sos, u, zi=zi0)
    carry = np.zeros(7680)
    carry[:m.CL] = sps.sosfilt(sos, np.zeros(m.CL), zi=zi0)[0]
    err, o, scale = 0.0, 0, np.max(np.abs(ref))
    for k, n in enumerate(lens):
        f, carry = m.chunk(x[o:o + n], carry, nruns=[1, 2, 3, 4, 2][k])
        err = max(err, np.max(np.abs(f - ref[o:o + n])) / scale)
        o += n
    return err, 1e-12


def test_regression_held_rows_of_a_run_start_are_complete(exe):
    """A run of chain_zpn_kernel starts one block early with no previous block, so that block's rows
    0 .. D + Rf - 1 miss the previous tail and right burst; its last R rows are held for the run
    before.  Blocks of 20 rows with 12 held rows (and of 21 with 10 held rows and three rows of right
    burst) overlapped those rows and left errors of 2e-8 and 5e-11 at every run boundary (the NumPy
    model of these tables; the kernel has the same dataflow).  build_zpn now keeps
    R + Rf <= 2 NB - 32, and these designs take other routes."""
    for taps_n, design in ((640, ("cheby2", 1, (40.0,), 0.3, "lowpass")),          # was (20, 2, 2, 12)
                           (1025, ("cheby1", 5, (3.0,), 0.05, "highpass")),        # was (20, 4, 2, 12): 2e-8
                           (1793, ("cheby2", 1, (80.0,), 0.008, "highpass"))):     # was (21, 2, 2, 12)
        p = cc.host_plan(exe, cc.fir_taps(taps_n), cc.design_sos(*design))
        assert p["kernel"] != 2 or p["R"] + p["Rf"] <= 2 * p["rows"] - 32, (design, p)
    for c in cc.CORPUS:
        if c.cell[0] == "zpn":
            p = cc.host_plan(exe, cc.fir_taps(c.taps, c.cutoff), cc.design_sos(*c.design))
            assert p["R"] + p["Rf"] <= 2 * p["rows"] - 32, (c.cell, p)


@pytest.mark.parametrize("c", MODELLED, ids=cc.cell_id)
def test_dataflow_model_of_the_cell_against_scipy(exe, c):
    """The cell's tables through the NumPy model of its kernel (ModelZpn, ModelSpecN, ModelZp, the
    pair Model) against scipy, every kind of chunk, at the tolerance of tests/test_spec_host.py."""
    taps, sos = cc.fir_taps(c.taps, c.cutoff), cc.design_sos(*c.design)
    err, tol = {"zpn": _zpn, "zp": _zp, "fwd": _fwd, "spec": _spec}[c.cell[0]](exe, taps, sos)
    assert err < tol, (c.cell, err, tol)
