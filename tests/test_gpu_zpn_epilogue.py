"""The chain kernel's epilogue on the paths a block can take through it (chain_zpn_body.h: the fit's
rows, the forward and backward bursts, the held rows, the row stores and the hand-over of `held`
and `cr` end at the first row the launch does not have, instead of one specialised copy per row
count).  On the benchmark's filter pair (firwin(1024, 0.2) -> butter(6, [0.05, 0.3], 'bandpass'):
chain_zpn_kernel<27, 6, 2, 5, true>, R = 3 held rows, Rf = 2) against the whole stream's reference
at the cell's tolerance (tests/chain_cells.py), shapes chosen for the paths, not the workload:

  channels     3: every block is a run of its own -- its first block and the pre-roll hand-over
               in every run; 130: several blocks per run
  chunks       the shortest the step accepts, closing blocks of 1, 256 and S - 1 samples
  split        the boundary n0 between the caller's two output buffers inside the rows a block
               holds back, exactly on a row boundary of them, and one sample either side (the
               `o - S + L >= n0` and `o + L >= n0` branches)
  non-finite   one sample in a chunk's opening block, in a middle block, in its closing block:
               the reach is the reference's (the oracle, as tests/test_gpu_nonfinite.py pins it)

and one instance each of the families with more burst rows (RM = 8, RM = 12) and of the forward
chain, from the corpus of tests/chain_cells.py at the same small shapes."""

from functools import partial

import numpy as np
import pytest
import scipy.signal as sps

import chain_cells as cc

pytestmark = pytest.mark.gpu

S = 256 * 27


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


@pytest.fixture(scope="module")
def pair():
    """The benchmark's filters and the tolerance of the cell the host planner gives them."""
    h = sps.firwin(1024, 0.2)
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    cells = dict((cell[0], (cell, ratio)) for cell, ratio in
                 cc.cells_of_plan(cc.host_plan(cc.build_host_exe(), h, sos)))
    assert cells["zpn"][0] == ("zpn", 27, 6, 2, 5), cells
    cell, ratio = cells["zpn"]
    return h, sos, cc.tolerance(cc.Cell(cell, 1024, 0.2, None, ratio))


def _run_split(dev, x, h, sos, lens, cut):
    """cc.run_stream's split layout with the boundary where the test wants it: every step's first
    `cut` outputs go to the tail of the previous buffer, the rest to the head of the current one.
    Column q of the result is stream sample q - lag."""
    import torch
    C = x.shape[0]
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        lag = dev.chain_zp_lag(fir, iir)
        assert lag >= 0
        iir.set_state_scaled((x[:, :1] * float(h[0])).contiguous(), 0)
        dev.chain_zp_open(fir, iir, 0)
        bufs = [torch.full((C, cut), float("nan"), dtype=torch.float64, device="cuda")]
        bufs += [torch.full((C, n), float("nan"), dtype=torch.float64, device="cuda") for n in lens]
        o = 0
        for k, n in enumerate(lens):
            prev, cur = bufs[k], bufs[k + 1]
            dev.chain_zp_step(fir, iir, x[:, o:o + n], out=cur[:, :n - cut], tail=prev[:, prev.shape[1] - cut:])
            o += n
        return torch.cat(bufs, 1)[:, :sum(lens)], lag
    finally:
        fir.close()
        iir.close()


def _worst(got, ref, hi):
    return max(np.max(np.abs(got[k, :hi] - ref[k, :hi])) / np.max(np.abs(ref[k])) for k in range(len(ref)))


# the rows block 1 holds back are outputs S .. S + 256 R - 1 of a chunk (R = 3): a boundary inside
# the second of them, on the boundary between the first and the second, and one sample either side
CUTS = {"plain": None, "inside": S + 300, "row": S + 256, "row-1": S + 255, "row+1": S + 257}


@pytest.fixture(scope="module", params=[(3, None), (130, 12)], ids=["3ch", "130ch"])
def stream(request, dev, pair):
    """One stream and its reference per channel count, shared by the output layouts."""
    h, sos, tol = pair
    C, blocks = request.param
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        p = dev.chain_zp_plan(fir, iir)
        m = dev.chain_zp_min_chunk(fir, iir)
        warm = iir.warm_len
    finally:
        fir.close()
        iir.close()
    assert (p["kernel"], p["rows"], p["NM"], p["NS"], p["R"], p["Rf"], p["RM"], p["has_instance"]) == \
        (2, 27, 6, 2, 3, 2, 5, 1), p
    whole = S * (blocks if blocks else -(-m // S))
    closing = [1, 256, S - 1]
    lens = ([m] if not blocks else []) + [whole + lc for lc in closing] + [whole + 1]
    assert min(lens) >= m and [n - (n - 1) // S * S for n in lens[-4:-1]] == closing
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=60 + C)
    pick = sorted({0, C // 2, C - 1})
    ref = cc.whole_stream_reference(x[pick].cpu().numpy(), h, sos)
    ref.setflags(write=False)
    return C, lens, x, pick, ref, warm


@pytest.mark.parametrize("where", list(CUTS), ids=list(CUTS))
def test_headline_instance_paths(dev, pair, stream, where):
    h, sos, tol = pair
    C, lens, x, pick, ref, warm = stream
    total = sum(lens)
    cut = CUTS[where]
    if cut is None:
        got, lag = cc.run_stream(dev, x, h, sos, lens)
    else:
        assert S < cut < S + 256 * 3 and cut < min(lens)
        got, lag = _run_split(dev, x, h, sos, lens, cut)
    g = got[pick].cpu().numpy()
    hi = total - lag - max(6000, warm)
    assert hi >= sum(lens[:-1]), (hi, lens)              # every closing block lies in the compared region
    assert np.isfinite(g[:, lag:lag + hi]).all()
    err = _worst(g[:, lag:], ref, hi)
    print(f"zpn-27-6-2-5 C {C} {where} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err < tol, (C, where, err, tol)


def test_headline_instance_nonfinite_reach(dev, pair):
    """One non-finite sample per channel in the chunk's opening block, in a middle block and in
    its closing block, on the public generators (the one-kernel route); three channels and a clean
    one, so every block is a run.  Lost chunks and finite values as the oracle has them."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    h, sos, _ = pair
    cs, nchunks = 131072, 8
    total = cs * (nchunks - 1) + 4321
    where = [3 * cs + 5,                    # the opening block of a chunk
             3 * cs + 9 * S + 100,          # a middle block: a later run of the same chunk
             4 * cs - 7]                    # the closing block
    C = len(where) + 1
    x = np.random.default_rng(61).standard_normal((C, total))
    x[0, where[0]] = np.nan
    x[1, where[1]] = np.inf
    x[2, where[2]] = np.nan
    steps, plain = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.append(a[2].shape[1]), plain(*a, **k))[1]
    try:
        src = producer(torch.from_numpy(x).cuda(), cs, -1)
        fir = producer(partial(nm.oaconvolve, src, h, -1, "same"), cs, -1, shape=src.shape)
        got = torch.cat(list(nm.sosfiltfilt(fir, sos, -1)), -1).cpu().numpy()
    finally:
        dev.chain_zp_step = plain
    assert sum(steps) == (nchunks - 2) * cs, steps                      # the one-kernel route
    want = orc.sosfiltfilt(np.concatenate(orc.oaconvolve(x, h, "same"), -1), sos, cs)
    ok = np.isfinite(want)
    lost = lambda a: [[bool(~np.isfinite(a[c, k * cs:(k + 1) * cs]).all()) for k in range(nchunks)] for c in range(C)]
    assert lost(got) == lost(want)
    assert np.array_equal(ok, np.isfinite(got))
    assert ok[C - 1].all() and not ok[:3].all(1).any()
    assert np.max(np.abs(got[ok] - want[ok])) < 1e-9 * np.max(np.abs(want[ok]))


def _cell(name):
    return next(c for c in cc.CORPUS if c.cell == name)


@pytest.mark.parametrize("name", [("zpn", 24, 6, 2, 8), ("zpn", 23, 6, 2, 12)], ids=["RM8", "RM12"])
@pytest.mark.parametrize("C,blocks", [(3, None), (130, 12)], ids=["3ch", "130ch"])
def test_long_left_tail_instances(dev, name, C, blocks):
    """Six modes, two of them slow, as the headline -- with eight and with twelve burst rows."""
    c = _cell(name)
    h, sos = cc.fir_taps(c.taps, c.cutoff), np.atleast_2d(cc.design_sos(*c.design))
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        p = dev.chain_zp_plan(fir, iir)
        m = dev.chain_zp_min_chunk(fir, iir)
        warm = iir.warm_len
    finally:
        fir.close()
        iir.close()
    assert (p["kernel"], p["rows"], p["NM"], p["NS"], p["RM"], p["has_instance"]) == (2,) + name[1:] + (1,), p
    Sb = 256 * p["rows"]
    whole = Sb * (blocks if blocks else -(-m // Sb))
    lens = [whole + lc for lc in (1, 256, Sb - 1)] + [whole + 1]
    assert min(lens) >= m
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=70 + C + p["RM"])
    pick = sorted({0, C // 2, C - 1})
    ref = cc.whole_stream_reference(x[pick].cpu().numpy(), h, sos)
    tol = cc.tolerance(c)
    # (split: the boundary inside the rows block 1 holds back)
    for cut in (None, Sb + 256 * (p["R"] - 1) + 44):
        assert cut is None or cut < min(lens)
        got, lag = cc.run_stream(dev, x, h, sos, lens) if cut is None else _run_split(dev, x, h, sos, lens, cut)
        g = got[pick].cpu().numpy()
        hi = total - lag - max(6000, warm)
        assert hi >= sum(lens[:2]), (hi, lens)
        assert np.isfinite(g[:, lag:lag + hi]).all()
        err = _worst(g[:, lag:], ref, hi)
        print(f"{cc.cell_id(c)} C {C} cut {cut} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err < tol, (name, C, cut, err, tol)


@pytest.mark.parametrize("C,blocks", [(3, 2), (130, 12)], ids=["3ch", "130ch"])
def test_forward_chain_instance(dev, C, blocks):
    """chain_zpn_kernel<27, 6, 2, 5, false> on its corpus pair: no left tail, nothing held."""
    from oracle import oracle as orc
    c = _cell(("fwd", 27, 6, 2))
    h, sos = cc.fir_taps(c.taps, c.cutoff), np.atleast_2d(cc.design_sos(*c.design))
    lens = [blocks * S + lc for lc in (1, 256, S - 1)] + [blocks * S + 1]
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=80 + C)
    pick = sorted({0, C // 2, C - 1})
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        p = dev.chain_forward_plan(fir, iir)
        assert (p["route"], p["rows"], p["NM"], p["NS"], p["has_instance"]) == (2, 27, 6, 2, 1), p
        got, n0 = [], 0
        for n in lens:
            got.append(dev.chain_forward(fir, iir, x[:, n0:n0 + n].contiguous())[pick].cpu().numpy())
            n0 += n
    finally:
        fir.close()
        iir.close()
    got = np.concatenate(got, -1)
    u = orc.convolve_direct(x[pick].cpu().numpy(), h, "full")[:, :total]
    want, _ = orc.sosfilt(u, sos, total)
    tol = cc.tolerance(c)
    err = _worst(got, want, total)
    print(f"{cc.cell_id(c)} C {C} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert np.isfinite(got).all() and err < tol, (C, err, tol)
