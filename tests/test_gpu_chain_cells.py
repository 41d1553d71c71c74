"""Every reachable chain-kernel instance (tests/chain_cells.py: CORPUS) on the GPU through the C ABI,
against SciPy / the oracle over the whole stream.  Each case asserts the library's own plan
(osz_chain_zp_plan / osz_chain_forward_plan) is the declared cell with a compiled instance, then
runs chunk geometries that reach the kernel's edges: the shortest chunk, closing blocks of 1, S - 1
and S samples, an exact multiple of S, and the split output layout; with three channels every run
is one block (run boundaries, pre-roll), with 128 channels a run holds several blocks (held rows,
carries inside a run).  Tolerance per cell: max(1e-11, 30e-16 / fit ratio), at most 1e-9
(DESIGN 4a)."""

from functools import partial

import numpy as np
import pytest

import chain_cells as cc

pytestmark = pytest.mark.gpu

ZERO_PHASE = [c for c in cc.CORPUS if c.cell[0] in ("zpn", "zp")]
FORWARD = [c for c in cc.CORPUS if c.cell[0] in ("fwd", "spec", "scan")]


def _many_channel_cells():
    """One cell per (family, NM, NS, RM) class at each end of its row range."""
    by = {}
    for c in cc.CORPUS:
        if c.cell[0] == "scan":
            key = ("scan", c.cell[2])
        else:
            key = (c.cell[0],) + tuple(c.cell[2:])
        by.setdefault(key, []).append(c)
    out = []
    for cs in by.values():
        cs = sorted(cs, key=lambda c: c.cell[1])
        out += [cs[0]] + ([cs[-1]] if len(cs) > 1 else [])
    return [c.cell for c in out]


MANY = set(_many_channel_cells())


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


def _filters(c):
    return cc.fir_taps(c.taps, c.cutoff), np.atleast_2d(cc.design_sos(*c.design))


def _zp_plan_matches(dev, c, fir, iir):
    p = dev.chain_zp_plan(fir, iir)
    fam, rows, nm = c.cell[:3]
    assert p["has_instance"] == 1, (c.cell, p)
    if fam == "zpn":
        assert (p["kernel"], p["rows"], p["NM"], p["NS"], p["RM"]) == (2, rows, nm, c.cell[3], c.cell[4]), (c.cell, p)
    else:
        assert (p["kernel"], p["rows"], p["NM"]) == (1, rows, nm), (c.cell, p)
    return p


def _zero_phase(dev, c, C, lens_of, split=False, seed=0):
    h, sos = _filters(c)
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        p = _zp_plan_matches(dev, c, fir, iir)
        m = dev.chain_zp_min_chunk(fir, iir)
        warm = iir.warm_len
    finally:
        fir.close()
        iir.close()
    S = 256 * p["rows"]
    lens = lens_of(S, m)
    assert min(lens) >= m
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=seed)
    outs = [cc.run_stream(dev, x, h, sos, lens, split=s) for s in ((False, True) if split else (False,))]
    pick = sorted({0, C // 2, C - 1})
    xh = x[pick].cpu().numpy()
    ref = cc.whole_stream_reference(xh, h, sos)
    worst = 0.0
    for got, lag in outs:
        g = got[pick].cpu().numpy()
        hi = total - lag - max(6000, warm)
        assert hi >= sum(lens[:3]), (c.cell, hi, lens)          # the compared region spans three chunks
        assert np.isfinite(g[:, lag:lag + hi]).all(), c.cell
        for k in range(len(pick)):
            err = np.max(np.abs(g[k, lag:lag + hi] - ref[k, :hi])) / np.max(np.abs(ref[k]))
            worst = max(worst, err)
    return worst


@pytest.mark.parametrize("c", ZERO_PHASE, ids=cc.cell_id)
def test_zero_phase_cell_few_channels(dev, c):
    """Three channels: every block is a run of its own.  Chunks: the shortest the step takes,
    closing blocks of 1, S - 1 and S samples, an exact multiple of S; plain and split layout."""
    tol = cc.tolerance(c)

    def lens(S, m):
        return [m, m + S + 1, m + 2 * S - 1, m + 3 * S, m + S // 2, 3 * m, m + S + 1]

    err = _zero_phase(dev, c, 3, lens, split=True, seed=c.taps)
    print(f"{cc.cell_id(c)} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err < tol, (c.cell, err, tol)


@pytest.mark.parametrize("c", [c for c in ZERO_PHASE if c.cell in MANY], ids=cc.cell_id)
def test_zero_phase_cell_many_channels(dev, c):
    """128 channels, chunks of 12 blocks and more: several blocks per run (four runs)."""
    tol = cc.tolerance(c)

    def lens(S, m):
        return [12 * S + 1, 14 * S - 1, 13 * S, 12 * S + S // 2]

    err = _zero_phase(dev, c, 128, lens, seed=7 + c.taps)
    print(f"{cc.cell_id(c)} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err < tol, (c.cell, err, tol)


def _forward(dev, c, C, lens_of, seed=0, max_pairs=40):
    from oracle import oracle as orc
    h, sos = _filters(c)
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        p = dev.chain_forward_plan(fir, iir)
        fam, rows = c.cell[:2]
        assert p["has_instance"] == 1, (c.cell, p)
        if fam == "fwd":
            assert (p["route"], p["rows"], p["NM"], p["NS"]) == (2, rows, c.cell[2], c.cell[3]), (c.cell, p)
        elif fam == "spec":
            assert (p["route"], p["rows"], p["NM"]) == (1, rows, c.cell[2]), (c.cell, p)
        else:
            assert (p["route"], p["rows"], p["lane_table"]) == (0, rows, c.cell[2]), (c.cell, p)
        S = 256 * rows
        if fam == "scan":
            # chain.hip: whole pairs of 2 S after a pre-roll of ceil((warm_len + taps - 1) / pair)
            # pairs per run; every chunk holds several of them beyond the plain kernels' head
            pair = 2 * S
            pre = -(-(iir.warm_len + len(h) - 1) // pair)
            np_ = max(6, min(8 * pre + 2, max_pairs))          # (8 pre: two runs or more, each with its pre-roll)
            lens = [np_ * pair + 2, (np_ + 1) * pair, (np_ + 2) * pair + 4, np_ * pair][:4 if C <= 3 else 3]
        else:
            lens = lens_of(S)
        total = sum(lens)
        x = dev.synth_normal(C, total, seed=seed)
        got, n0 = [], 0
        for n in lens:
            got.append(dev.chain_forward(fir, iir, x[:, n0:n0 + n].contiguous())[[0, C // 2, C - 1]].cpu().numpy())
            n0 += n
    finally:
        fir.close()
        iir.close()
    got = np.concatenate(got, -1)
    xh = x[[0, C // 2, C - 1]].cpu().numpy()
    u = orc.convolve_direct(xh, h, "full")[:, :total]
    want, _ = orc.sosfilt(u, sos, total)
    return max(np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k])) for k in range(3))


@pytest.mark.parametrize("c", FORWARD, ids=cc.cell_id)
def test_forward_cell_few_channels(dev, c):
    tol = cc.tolerance(c)
    m = {"fwd": 2, "spec": 4}

    def lens(S):
        k = m[c.cell[0]]
        return [k * S, 3 * S + 1, 4 * S - 1, 5 * S, 6 * S + 2]

    err = _forward(dev, c, 3, lens, seed=c.taps)
    print(f"{cc.cell_id(c)} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err < tol, (c.cell, err, tol)


@pytest.mark.parametrize("c", [c for c in FORWARD if c.cell in MANY], ids=cc.cell_id)
def test_forward_cell_many_channels(dev, c):
    tol = cc.tolerance(c)

    def lens(S):
        return [12 * S + 1, 14 * S - 1, 13 * S]

    err = _forward(dev, c, 128, lens, seed=11 + c.taps, max_pairs=16)
    print(f"{cc.cell_id(c)} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err < tol, (c.cell, err, tol)


def _public_cells():
    """NM = 2, and NM = 4, 6, 8 with more than two slow modes: one zero-phase cell each."""
    out = []
    for nm in (2, 4, 6, 8):
        cs = [c for c in cc.CORPUS if c.cell[0] == "zpn" and c.cell[2] == nm and (nm == 2 or c.cell[3] > 2)]
        out.append(max(cs, key=lambda c: c.ratio))
    return out


@pytest.mark.parametrize("c", _public_cells(), ids=cc.cell_id)
def test_public_sosfiltfilt_on_the_cell(dev, c):
    """The public generators (oaconvolve -> sosfiltfilt) take the one-kernel route for the cell and
    match the oracle's chunk-local scheme at 1e-9 (as test_gpu_zp's realistic cascades)."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    h, sos = _filters(c)
    C, cs = 3, 65536
    total = 6 * cs + 4321
    x = dev.synth_normal(C, total, seed=900 + c.taps)
    steps, plain = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain(*a, **k))[1]
    try:
        src = producer(x, cs, -1)
        fir = producer(partial(nm.oaconvolve, src, h, -1, "same"), cs, -1, shape=src.shape)
        got = torch.cat([y for y in nm.sosfiltfilt(fir, sos, -1)], -1).cpu().numpy()
    finally:
        dev.chain_zp_step = plain
    assert len(steps) == 5, (c.cell, len(steps))
    want = orc.sosfiltfilt(np.concatenate(orc.oaconvolve(x.cpu().numpy(), h, "same"), -1), sos, cs)
    assert np.max(np.abs(got - want)) < 1e-9 * np.max(np.abs(want)), c.cell
