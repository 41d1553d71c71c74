"""Every reachable polyphase-resampler instance (tests/poly_cells.py: CORPUS) on the GPU through
dev.PolyStream, against the definition in longdouble
    y[j] = sum_k L h[k] xup[j M + centre - k]
over the whole stream.  Each case first asserts the library's own plan (osz_poly_plan) is the
declared cell, then pushes a stream of two channels as slices of a wider tensor (a row pitch:
ldx > n) of these lengths: one that puts a whole tile's window inside the chunk (the
buffer-descriptor staging path; never less than one tile of input and 17 samples), 1, 0, H - 1
twice (history carried over pushes shorter than itself), M - 1 (may produce nothing), the rest but
for 5 samples, those 5, and an empty push with final (no input pointer at all).

Bound: 1e-12 of max |reference|, the bound of test_polyphase_large_decimation_stays_on_the_tiled_
kernel.  The same sum in float64 in another order is within 1.1e-15 of longdouble; a missing or
misplaced tap of these random filters costs about 1 / ntaps >= 1e-4."""

import functools

import numpy as np
import pytest

import poly_cells as pc

pytestmark = pytest.mark.gpu

TOL = 1e-12
C = 2
ONE_PER_CELL = pc.one_per_cell()


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


def _open(dev, e):
    """(stream, plan) of the entry, the plan asserted to be the declared cell."""
    ps = dev.PolyStream(pc.taps_of(e), e.L, e.M, C, centre=e.centre)
    try:
        p = dev.poly_plan(ps)
        assert pc.cell_of_plan(p) == e.cell, (pc.entry_id(e), pc.cell_name(e.cell), p)
        assert p["half"] == pc.centre_of(e)
        p.update(L=e.L, M=e.M, m=e.ntaps)
    except Exception:
        ps.close()
        raise
    return ps, p


def _on_device(xh):
    """The rows of xh inside a wider tensor: slices of it have a row pitch and an odd offset."""
    import torch
    wide = torch.full((xh.shape[0], xh.shape[1] + 67), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 3:3 + xh.shape[1]] = torch.tensor(xh, device="cuda")
    return wide[:, 3:3 + xh.shape[1]]


def _ragged(dev, ps, xd, lens):
    """The pushes of the schedule (slices, never .contiguous()) and the flush; [outputs]."""
    import torch
    outs, o = [], 0
    for n in lens:
        piece = xd[:, o:o + n]
        assert n == 0 or (piece.stride(0) > n and not piece.is_contiguous())
        outs.append(ps.push(piece, final=False))
        o += n
    assert o == xd.shape[1]
    outs.append(ps.push(torch.empty((C, 0), dtype=torch.float64, device="cuda"), final=True))
    return outs


@functools.lru_cache(maxsize=None)
def _clean(key):
    """(x, longdouble reference, its scale) of an entry's stream: computed once, never written."""
    e, n = key
    x = np.random.default_rng([77, e.L, e.M, e.ntaps]).standard_normal((C, n))
    ref = pc.definition(x, pc.taps_of(e), e.L, e.M, pc.centre_of(e))
    for a in (x, ref):
        a.setflags(write=False)
    return x, ref, float(np.max(np.abs(ref)))


def _run_entry(dev, e, spoil=None):
    import torch
    ps, p = _open(dev, e)
    try:
        n, lens = pc.schedule(p, None if e.pad is None else e.pad[1])
        x, ref, scale = _clean((e, n))
        if spoil is not None:
            x = x.copy()
            spoil(x, p)
            ref = pc.definition(x, pc.taps_of(e), e.L, e.M, pc.centre_of(e))
        if p["kernel"]:
            assert pc.descriptor_classes(p, 0, lens[0], 0) >= e.L        # a whole tile on the descriptor path
        outs = _ragged(dev, ps, _on_device(x), lens)
        got = torch.cat(outs, 1).cpu().numpy()
    finally:
        ps.close()
    assert sum(o.shape[1] for o in outs) == -(-n * e.L // e.M) == ref.shape[1], (pc.entry_id(e), [o.shape[1] for o in outs])
    return got, ref, scale, p


@pytest.mark.parametrize("e", pc.CORPUS, ids=pc.entry_id)
def test_entry_ragged_stream_against_the_definition(dev, e):
    got, ref, scale, p = _run_entry(dev, e)
    assert np.isfinite(got).all(), pc.entry_id(e)
    err = float(np.max(np.abs(got - ref))) / scale
    print(f"{pc.cell_name(e.cell)} {pc.entry_id(e)} err {err:.3e} ratio {err / TOL:.4f}")
    assert err < TOL, (pc.entry_id(e), pc.cell_name(e.cell), err)


@pytest.mark.parametrize("e", pc.CORPUS, ids=pc.entry_id)
def test_entry_non_finite_reach(dev, e):
    """One NaN one tile in, one Inf at the last sample, in different channels: lost are exactly the
    outputs a tap touches them with (the caller's zero-valued taps included, the table's padding
    never), the others hold the tolerance."""
    def spoil(x, p):
        tile = p["NT"] * pc.R * e.M if p["kernel"] else 256 * e.M // e.L
        x[0, tile] = np.nan
        x[1, -1] = np.inf

    got, ref, scale, p = _run_entry(dev, e, spoil)
    want = np.isfinite(ref)
    assert not want.all() and want.any()
    bad = np.flatnonzero((np.isfinite(got) != want).ravel())
    assert bad.size == 0, (pc.entry_id(e), pc.cell_name(e.cell), bad[:8], bad.size)
    err = float(np.max(np.abs(got[want] - ref[want]))) / scale
    assert err < TOL, (pc.entry_id(e), pc.cell_name(e.cell), err)


@pytest.mark.parametrize("e", ONE_PER_CELL, ids=pc.entry_id)
def test_cuts_agree_bit_for_bit(dev, e):
    import torch
    ps, p = _open(dev, e)
    try:
        n, lens = pc.schedule(p)
        xd = _on_device(_clean((e, n))[0])
        cut = torch.cat(_ragged(dev, ps, xd, lens), 1)
        ps.reset()
        whole = ps.push(xd, final=True)
    finally:
        ps.close()
    assert whole.shape == cut.shape and torch.equal(whole, cut), pc.entry_id(e)


@pytest.mark.parametrize("e", ONE_PER_CELL, ids=pc.entry_id)
def test_state_resumes_and_reset_restarts_bit_for_bit(dev, e):
    import torch
    ps, p = _open(dev, e)
    other, _ = _open(dev, e)
    try:
        n, lens = pc.schedule(p)
        xd = _on_device(_clean((e, n))[0])
        cut = lens[0] + 1
        first = ps.push(xd[:, :cut], final=False)
        state = ps.get_state()
        assert state[0] == cut and state[1] == first.shape[1] and len(state) == 2 + C * p["H"]
        rest = ps.push(xd[:, cut:], final=True)
        other.set_state(state)
        again = other.push(xd[:, cut:], final=True)
        assert torch.equal(again, rest), pc.entry_id(e)
        ps.reset()
        assert list(ps.get_state()[:2]) == [0.0, 0.0] and not ps.get_state()[2:].any()
        assert torch.equal(ps.push(xd[:, :cut], final=False), first), pc.entry_id(e)
        assert torch.equal(ps.push(xd[:, cut:], final=True), rest), pc.entry_id(e)
    finally:
        ps.close()
        other.close()
    assert first.shape[1] + rest.shape[1] == -(-n * e.L // e.M)


def test_fallback_grid_stride_second_trip(dev):
    """poly_kernel launches at most 4096 x 256 threads: 1 060 000 outputs make a thread take a
    second trip through its grid-stride loop (the smallest stream that does).  One push with final,
    against float64 scipy.signal.resample_poly of the same array; the bound is held over all outputs
    and, on its own, over those past index 1 048 576."""
    import scipy.signal as sps
    e = next(e for e in pc.CORPUS if (e.L, e.M, e.ntaps) == (4, 57, 229))
    h = pc.taps_of(e)
    n = 57 * 265_000
    x = dev.synth_normal(1, n, seed=457)
    ps = dev.PolyStream(h, 4, 57, 1)
    try:
        assert pc.cell_of_plan(dev.poly_plan(ps)) == pc.FALLBACK
        got = ps.push(x, final=True).cpu().numpy()
    finally:
        ps.close()
    ref = sps.resample_poly(x.cpu().numpy(), 4, 57, axis=-1, window=h)
    assert got.shape == ref.shape == (1, 1_060_000) and got.shape[1] > 4096 * 256
    scale = np.max(np.abs(ref))
    err = np.abs(got - ref)[0] / scale
    print(f"grid stride: first trip {err[:4096 * 256].max():.3e} second trip {err[4096 * 256:].max():.3e}")
    assert err.max() < TOL
    assert err[4096 * 256:].max() < TOL


def _planned(dev, monkeypatch):
    """dev.PolyStream recording the plan of every stream the public API opens."""
    seen = []

    class Recording(dev.PolyStream):
        def __init__(self, taps, L, M, nch, centre=None):
            super().__init__(taps, L, M, nch, centre=centre)
            seen.append((dev.poly_plan(self), len(taps)))

    monkeypatch.setattr(dev, "PolyStream", Recording)
    return seen


def test_public_downsample_by_64_takes_the_fallback(dev, monkeypatch):
    """downsample(x, 64, fs) with the default design (1431 taps): the route a user takes to
    poly_kernel, against the oracle's whole-stream resampler."""
    from oracle import oracle as orc
    from openseize_amd.resampling.resampling import downsample
    fs = 20000.0
    x = np.random.default_rng(64).standard_normal((3, 200_000))
    seen = _planned(dev, monkeypatch)
    got = np.asarray(downsample(x, 64, fs, chunksize=30_011, axis=-1))
    assert [pc.cell_of_plan(p) for p, _ in seen] == [pc.FALLBACK], seen
    h = orc.resample_filter(1, 64, fs)
    assert len(h) == 1431
    ref = orc.polyphase_resample(x, 1, 64, h)
    assert got.shape == ref.shape == (3, 3125)
    assert np.max(np.abs(got - ref)) < TOL * np.max(np.abs(ref))


def test_public_resample_with_a_tight_transition(dev, monkeypatch):
    """resample(x, 1, 5, fs, fpass=, fstop=) with a transition band tight enough for more than 4200
    taps: four phase groups at M = 5 (the uneven split) from the public API."""
    from oracle import oracle as orc
    from openseize_amd.filtering.fir import Kaiser
    from openseize_amd.resampling.resampling import resample
    fs, edge = 5000.0, 500.0
    band = dict(fpass=edge * (1 - 0.0025), fstop=edge * (1 + 0.0025))
    h = Kaiser(band["fpass"], band["fstop"], fs, gpass=0.1, gstop=40).coeffs
    assert len(h) >= 4200
    x = np.random.default_rng(15).standard_normal((3, 200_000))
    seen = _planned(dev, monkeypatch)
    got = np.asarray(resample(x, 1, 5, fs, chunksize=30_011, axis=-1, **band))
    assert [pc.cell_of_plan(p) for p, _ in seen] == [pc.D64_4] and seen[0][1] >= len(h), seen
    ref = orc.polyphase_resample(x, 1, 5, h)
    assert got.shape == ref.shape == (3, 40_000)
    assert np.max(np.abs(got - ref)) < TOL * np.max(np.abs(ref))
