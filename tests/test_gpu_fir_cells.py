"""Every reachable instance of the stand-alone FIR (tests/fir_cells.py: CORPUS) on the GPU through
dev.FirStream, against the exact integer convolution of the whole stream (int64 np.convolve; the
rounded float64 FFT convolution for the wide and the 32768-tap entries, shown equal to it in
tests/test_fir_cells_host.py).

Every input is a slice, never .contiguous(), of a wider NaN-filled device tensor (odd element offset,
row pitch larger than n); every output goes through out= into a slice of a NaN-filled tensor of its
own, whose margins must still be NaN everywhere after the call.  After every push
FirStream.last_launches() must be the entry's declared cells with the step, nblocks, R and nruns the
restated planner (fir_cells.push_plan) gives for the device's CU count.

Bound: 1e-12 of max |reference|, the bound of test_oaconvolve_few_channels_joined_chunks and of the
resampler sweep.  Float64 FFT convolution is within 1e-15 of the exact reference; a wrong or misplaced
tap costs at least 1e-4 (test_fir_cells_host.py)."""

import numpy as np
import pytest

import fir_cells as fc

pytestmark = pytest.mark.gpu

TOL = 1e-12
OFF_IN, OFF_OUT, EXTRA = 3, 5, 67
ONE_PER_CELL = fc.one_per_cell()


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


@pytest.fixture(scope="module")
def cus(dev):
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _on_device(xh):
    """The rows of xh inside a wider NaN-filled tensor: slices of it have a row pitch and an odd offset."""
    import torch
    wide = torch.full((xh.shape[0], xh.shape[1] + EXTRA), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, OFF_IN:OFF_IN + xh.shape[1]] = torch.tensor(xh, device="cuda")
    return wide[:, OFF_IN:OFF_IN + xh.shape[1]]


class _Out:
    """An output of n columns inside a NaN-filled tensor of its own."""

    def __init__(self, nch, n):
        import torch
        self.n = n
        self.wide = torch.full((nch, n + EXTRA), float("nan"), dtype=torch.float64, device="cuda")
        self.view = self.wide[:, OFF_OUT:OFF_OUT + n]
        assert self.view.stride(0) > n and (n == 0 or not self.view.is_contiguous())

    def check(self, what):
        import torch
        assert bool(torch.isnan(self.wide[:, :OFF_OUT]).all()), (what, "written in front of the output")
        assert bool(torch.isnan(self.wide[:, OFF_OUT + self.n:]).all()), (what, "written behind the output")
        assert bool(torch.isfinite(self.view).all()), (what, "output not written everywhere")
        return self.view


def _push(st, e, piece, skip, cus, what):
    """One push of a slice with `skip`, into an output with margins; the launch records asserted."""
    n = piece.shape[1]
    assert n == 0 or (piece.stride(0) > n and not piece.is_contiguous())
    out = _Out(e.nch, n - skip)
    st.push(piece, skip=skip, out=out.view)
    got = st.last_launches()
    assert tuple(fc.cell_of_record(r) for r in got) == e.cells, (what, [fc.cell_name(fc.cell_of_record(r)) for r in got])
    assert got == fc.expected_records(e, n, skip, cus), (what, got)
    return out.check(what), got


def _flush(st, e, skip, drop, what):
    out = _Out(e.nch, e.ntaps - 1 - skip - drop)
    st.flush("cuda", skip=skip, drop=drop, out=out.view)
    return out.check(what)


def _stream(dev, e, xd, lens, cus, skip0=0, fskip=0, fdrop=0, st=None):
    """The pushes of `lens` (the first with skip0) and the flush; (outputs joined, records of each push)."""
    import torch
    own = st is None
    st = dev.FirStream(fc.taps_of(e), e.nch) if own else st
    try:
        outs, recs, o = [], [], 0
        for k, n in enumerate(lens):
            y, r = _push(st, e, xd[:, o:o + n], skip0 if k == 0 else 0, cus, (fc.entry_id(e), "push", k, n))
            assert y.shape == (e.nch, n - (skip0 if k == 0 else 0))
            outs.append(y)
            recs.append(r)
            o += n
        tail = _flush(st, e, fskip, fdrop, (fc.entry_id(e), "flush"))
        assert tail.shape == (e.nch, e.ntaps - 1 - fskip - fdrop)
        outs.append(tail)
    finally:
        if own:
            st.close()
    return torch.cat(outs, 1).cpu().numpy(), recs


def _expect(ref, n, w, skip0=0, fskip=0, fdrop=0):
    return np.concatenate([ref[:, skip0:n], ref[:, n + fskip:n + w - fdrop]], 1)


def _report(e, what, got, want, scale):
    assert got.shape == want.shape, (fc.entry_id(e), what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) / scale if got.size else 0.0
    print(f"{'+'.join(fc.cell_name(c) for c in dict.fromkeys(e.cells))} {fc.entry_id(e)} {what} err {err:.3e} "
          f"ratio {err / TOL:.4f}")
    return err


@pytest.mark.parametrize("e", fc.NARROW + fc.WIDE, ids=fc.entry_id)
def test_entry_schedule_against_the_exact_convolution(dev, cus, e):
    """Narrow entries: the ragged schedule of fir_cells.narrow_schedule and the flush.  Wide entries:
    48 blocks in one push, where the record must show a run of three whole blocks (pairs), and a
    ragged push."""
    x, ref, scale = fc.clean(e)
    lens = fc.narrow_schedule(e) if e.kind == "narrow" else fc.wide_schedule(e)
    n = sum(lens)
    assert x.shape == (e.nch, n) and ref.shape == (e.nch, n + e.ntaps - 1)
    got, recs = _stream(dev, e, _on_device(x), lens, cus)
    if e.kind == "wide":
        for r in recs[0]:
            runs = fc.whole_per_run(r)
            assert max(runs) >= 3, (fc.entry_id(e), r, runs)
    err = _report(e, "schedule", got, ref, scale)
    assert err < TOL, (fc.entry_id(e), err)


@pytest.mark.parametrize("e", ONE_PER_CELL, ids=fc.entry_id)
def test_left_cut_sweep(dev, cus, e):
    """A first push of 4 S + 3 samples cut on the left by 1, w / 2, w, a whole block, a block and a
    sample, two blocks and five samples (a first block loaded directly in front of requested ones)
    and all of it (an empty output), then a push of 2 S + 7 without a cut."""
    S, w = fc.last_step(e), e.ntaps - 1
    n1, n2 = 4 * S + 3, 2 * S + 7
    x, ref, scale = fc.clean(e, n1 + n2)
    xd = _on_device(x)
    st = dev.FirStream(fc.taps_of(e), e.nch)
    worst = 0.0
    try:
        for skip in sorted({1, w // 2, w, S, S + 1, 2 * S + 5, n1}):
            st.reset()
            got, recs = _stream(dev, e, xd, [n1, n2], cus, skip0=skip, fskip=w, st=st)
            assert recs[0][0]["skip"] == skip and recs[1][0]["skip"] == 0
            err = _report(e, f"skip {skip}", got, ref[:, skip:n1 + n2], scale)
            worst = max(worst, err)
    finally:
        st.close()
    assert worst < TOL, (fc.entry_id(e), worst)


@pytest.mark.parametrize("e", fc.PARTITIONED, ids=fc.entry_id)
def test_partitioned_entry_in_chunks(dev, cus, e):
    """'full' in chunks of 777, of 3000 and in one push (32768 taps: 777 and one push); the run in the
    smallest chunks cuts its first push on the left and its flush on both sides."""
    x, ref, scale = fc.clean(e)
    n, w = x.shape[1], e.ntaps - 1
    xd = _on_device(x)
    worst = 0.0
    for k, cs in enumerate(fc.part_chunkings(e)):
        lens = [n] if cs is None else [cs] * (n // cs) + ([n % cs] if n % cs else [])
        cut = dict(skip0=321, fskip=5, fdrop=7) if k == 0 else {}
        got, recs = _stream(dev, e, xd, lens, cus, **cut)
        assert all(len(r) == len(e.cells) and all(q["accum"] == 1 and q["skip"] == 0 for q in r) for r in recs)
        err = _report(e, f"chunks {cs}", got, _expect(ref, n, w, **cut), scale)
        worst = max(worst, err)
    assert worst < TOL, (fc.entry_id(e), worst)


STATE = ONE_PER_CELL + [e for e in fc.PARTITIONED if e.ntaps in (4097, 32768)]


@pytest.mark.parametrize("e", STATE, ids=fc.entry_id)
def test_state_resumes_and_reset_restarts_bit_for_bit(dev, cus, e):
    import torch
    S = fc.last_step(e)
    if e.kind == "part":
        x, ref, scale = fc.clean(e)
        cut = 7001
    else:
        x, ref, scale = fc.clean(e, 6 * S + 10)
        cut = 2 * S + 5
    n = x.shape[1]
    xd = _on_device(x)
    st, other = dev.FirStream(fc.taps_of(e), e.nch), dev.FirStream(fc.taps_of(e), e.nch)
    try:
        size = int(st.lib.osz_fir_state_size(st.h))
        assert size == e.nch * sum(t - 1 for _, t in fc.pieces_of(e.ntaps)) + \
            (e.nch * (len(e.cells) - 1) * fc.PART if len(e.cells) > 1 else 0)
        first, _ = _push(st, e, xd[:, :cut], 0, cus, (fc.entry_id(e), "prefix"))
        state = st.get_state()
        assert state.shape == (size,) and np.isfinite(state).all()
        rest, _ = _push(st, e, xd[:, cut:], 0, cus, (fc.entry_id(e), "rest"))
        tail = _flush(st, e, 0, 0, (fc.entry_id(e), "flush"))
        other.set_state(state)
        again, _ = _push(other, e, xd[:, cut:], 0, cus, (fc.entry_id(e), "resumed"))
        assert torch.equal(again, rest), fc.entry_id(e)
        assert torch.equal(_flush(other, e, 0, 0, (fc.entry_id(e), "resumed flush")), tail)
        st.reset()
        assert not st.get_state().any()
        assert torch.equal(_push(st, e, xd[:, :cut], 0, cus, (fc.entry_id(e), "prefix again"))[0], first)
        assert torch.equal(_push(st, e, xd[:, cut:], 0, cus, (fc.entry_id(e), "rest again"))[0], rest)
        got = torch.cat([first, rest, tail], 1).cpu().numpy()
    finally:
        st.close()
        other.close()
    err = _report(e, "resumed", got, ref, scale)
    assert err < TOL, (fc.entry_id(e), err)
