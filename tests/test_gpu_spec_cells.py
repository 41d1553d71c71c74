"""Every compiled instance of the windowed-DFT engine (tests/spec_cells.py: CASES) on the GPU
through dev.SpecStream, against the long-double DFT of the same segments.

Every case: the input of spec_cells.signal, every push a column slice of a wider tensor (row
pitch > n); after every push SpecStream.last_launches() is what the restated planners say that
push must launch (family, size, mode, detrend, HALF or half-carry, segments, R, runs, head or
body, the radix plan); the output has the shape and the segment count of the push; every
(segment, channel) row is compared in spec_cells.row_metric with the reference, at
spec_cells.bound = 16 e64(case).  PSD_MEAN is read through mean() and mean_device(), which must
agree to a rounding of the division.  A ragged or extra case is pushed a second time in one
piece, which must report one body launch and agree with the pieces within one bound.  A runs
case must report R >= 2 and more than one run; the mixed-radix and split ones the half-carry
their case names.  Every row is compared with the long-double reference, except in the runs
cases of spec_cells.SUBSET_TAGS (the long transforms, above spec_cells.LD_POINTS): there the
channels of spec_cells.subset (the first, the last and every 16th) are, and the others are
compared with the float64 pipeline at the bound plus e64.  A case whose reference is identically zero
(nwin = 1, constant detrend) must give zeros.

Every comparison prints its error, e64 and error / bound.
"""

import numpy as np
import pytest

import spec_cells as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


def _handle(dev, case, monkeypatch):
    for k in ("OSZ_SPEC_FUSED", "OSZ_SPEC_V8", "OSZ_SPEC_MIX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    st = dev.SpecStream(case.nwin, case.nfft, case.stride, C.window(case), C.SCALE,
                        "linear" if case.linear else "constant", case.mode, case.nch)
    for k, _ in case.env:          # the switches are read when the handle is created
        monkeypatch.delenv(k)
    return st


def _push_all(st, wide, pushes, plan, case):
    """Push wide[:, :sum(pushes)] in the given pieces, checking every push's report and output
    shape -> the concatenated segments (None in PSD_MEAN)."""
    import torch
    outs, a = [], 0
    for n, (nseg, want) in zip(pushes, plan):
        piece = wide[:, a:a + n]
        assert piece.stride(0) > n and piece.stride(1) == 1
        out = st.push(piece)
        got = st.last_launches()
        assert [{k: r[k] for k in C.FIELDS} for r in got] == want, (case.name, a, n, got, want)
        if case.mode == C.MEAN:
            assert out is None
        else:
            assert tuple(out.shape) == (nseg, case.nch, case.nfft // 2 + 1)
            assert out.dtype == (torch.complex128 if case.mode == C.DFT else torch.float64)
            outs.append(out)
        a += n
    return torch.cat(outs, 0).cpu().numpy() if outs else None


def _estimate(st, out, case, nseg):
    """The handle's estimate of every channel; PSD_MEAN through mean() and mean_device()."""
    if case.mode != C.MEAN:
        assert out.shape[0] == nseg
        return out
    cnt, mean = st.mean()
    cnt2, mean_d = st.mean_device()
    assert cnt == cnt2 == nseg, (cnt, cnt2, nseg)
    mean_d = mean_d.cpu().numpy()
    assert mean.shape == mean_d.shape == (case.nch, case.nfft // 2 + 1)
    assert np.allclose(mean, mean_d, rtol=4.5e-16, atol=0.0), np.abs(mean - mean_d).max()   # one division each
    return mean


@pytest.mark.parametrize("case", C.CASES, ids=[f"{C.group(c)}:{c.name}" for c in C.CASES])
def test_cell(dev, case, monkeypatch):
    import torch
    x = C.signal(case)
    ref = C.reference(case, x)
    plan = C.plan_pushes(case)
    n = x.shape[1]
    wide = torch.full((case.nch, n + 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :n] = torch.from_numpy(x).cuda()
    st = _handle(dev, case, monkeypatch)
    assert sum(s for s, _ in plan) == ref.nseg > 0
    got = _estimate(st, _push_all(st, wide, case.pushes, plan, case), case, ref.nseg)
    # the launches: the instance the case is there for, and what a runs case is about
    recs = [r for _, rs in plan for r in rs]
    assert recs and all(C.instance_of(r) == case.want for r in recs), (case.want, recs)
    if case.kind == "runs":
        assert all(r["R"] >= 2 and r["nruns"] >= 2 for r in recs), recs
        if case.want[0] in ("mix", "split"):
            assert all(r["half"] == case.halfcarry for r in recs)
    if case.zero:
        assert not np.any(ref.exact) and not np.any(got), case.name
        return
    assert np.isfinite(got).all()
    worst, err = C.check_estimate(got, case, ref)
    print(f"{case.name}: error {err:.3g} e64 {ref.e64:.3g} error/e64 {err / ref.e64:.3g} worst/bound {worst:.3g}")
    assert worst <= 1.0, (case.name, err, ref.e64, worst)
    if case.kind != "runs" and len(case.pushes) > 1:
        # cut anywhere or pushed whole: the same segments
        one = C.Case(*case)._replace(pushes=(n,))
        st1 = _handle(dev, one, monkeypatch)
        whole = _estimate(st1, _push_all(st1, wide, one.pushes, C.plan_pushes(one), one), one, ref.nseg)
        worst1, err1 = C.check_estimate(whole, case, ref)
        assert worst1 <= 1.0, (case.name, err1, ref.e64)
        diff = float(C.row_metric(got, whole, case.mode).max())
        print(f"{case.name}: pieces against one push {diff:.3g}")
        assert diff <= C.bound(case, ref.e64), (case.name, diff)
