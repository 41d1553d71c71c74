"""The chain kernel's resident instances on the benchmark's own filter pair (firwin(1024, 0.2) ->
butter(6, [0.05, 0.3], 'bandpass')): chain_zpn_kernel<27, 6, 2, 5, true> and its forward twin
<27, 6, 2, 5, false> keep a thread's mode powers in registers for the whole launch
(chain_zpn_body.h: zpn_resident) instead of forming them in every block.  The powers are indexed
by the thread, so what can go wrong shows where a closing block ends: inside a row (1, 255, 257,
S - 1 samples), at a row's boundary (256) -- with three channels (every block a run of its own)
and with 130 (several blocks per run, a channel count that is no multiple of anything).  Against
the whole stream's reference at the cell's tolerance (tests/chain_cells.py: max(1e-11, 30e-16 /
fit ratio)), as tests/test_gpu_chain_cells.py checks the corpus."""

import numpy as np
import pytest
import scipy.signal as sps

import chain_cells as cc

pytestmark = pytest.mark.gpu

CLOSING = ("1", "255", "256", "257", "S-1")


def _closing(S):
    return [1, 255, 256, 257, S - 1]


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
    """The filters, and the (cell, fit ratio) the host planner gives them for both chains."""
    h = sps.firwin(1024, 0.2)
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    cells = dict((cell[0], (cell, ratio)) for cell, ratio in
                 cc.cells_of_plan(cc.host_plan(cc.build_host_exe(), h, sos)))
    assert cells["zpn"][0] == ("zpn", 27, 6, 2, 5) and cells["fwd"][0] == ("fwd", 27, 6, 2), cells
    return h, sos, cells


def _tolerance(cells, fam):
    cell, ratio = cells[fam]
    return cc.tolerance(cc.Cell(cell, 1024, 0.2, None, ratio))


def _worst(got, ref, hi):
    return max(np.max(np.abs(got[k, :hi] - ref[k, :hi])) / np.max(np.abs(ref[k])) for k in range(len(ref)))


@pytest.mark.parametrize("C,blocks", [(3, None), (130, 12)], ids=["3ch", "130ch"])
def test_zero_phase_resident_instance(dev, pair, C, blocks):
    """Chunks whose closing block holds 1, 255, 256, 257 and S - 1 samples, behind the shortest
    whole number of blocks the step takes (three channels) or twelve blocks (130 channels: four
    runs of several blocks); one more chunk so that every closing block lies inside the compared
    region.  Plain and split output layout."""
    h, sos, cells = pair
    fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
    try:
        p = dev.chain_zp_plan(fir, iir)
        m = dev.chain_zp_min_chunk(fir, iir)
        warm = iir.warm_len
    finally:
        fir.close()
        iir.close()
    assert (p["kernel"], p["rows"], p["NM"], p["NS"], p["RM"], p["has_instance"]) == (2, 27, 6, 2, 5, 1), p
    S = 256 * p["rows"]
    whole = S * (blocks if blocks else -(-m // S))
    lens = [whole + lc for lc in _closing(S)] + [whole + 1]
    assert min(lens) >= m and [n - (n - 1) // S * S for n in lens[:5]] == _closing(S)
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=20 + C)
    pick = sorted({0, C // 2, C - 1})
    ref = cc.whole_stream_reference(x[pick].cpu().numpy(), h, sos)
    tol = _tolerance(cells, "zpn")
    for split in (False, True):
        got, lag = cc.run_stream(dev, x, h, sos, lens, split=split)
        g = got[pick].cpu().numpy()
        hi = total - lag - max(6000, warm)
        assert hi >= sum(lens[:5]), (hi, lens)
        assert np.isfinite(g[:, lag:lag + hi]).all()
        err = _worst(g[:, lag:], ref, hi)
        print(f"zpn-27-6-2-5 C {C} split {split} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err < tol, (C, split, err, tol)


@pytest.mark.parametrize("C,blocks", [(3, 2), (130, 12)], ids=["3ch", "130ch"])
def test_forward_resident_instance(dev, pair, C, blocks):
    """The forward chain (FIR -> sosfilt) on the same pair and the same closing blocks, against
    the oracle's cascade over the direct convolution."""
    from oracle import oracle as orc
    h, sos, cells = pair
    S = 256 * 27
    lens = [blocks * S + lc for lc in _closing(S)] + [blocks * S + 1]
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=40 + C)
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
    tol = _tolerance(cells, "fwd")
    err = _worst(got, want, total)
    print(f"fwd-27-6-2 C {C} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert np.isfinite(got).all() and err < tol, (C, err, tol)
