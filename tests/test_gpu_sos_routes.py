"""Every launch route of the stand-alone SOS cascade (tests/sos_routes.py: CASES) on the GPU
through dev.SosStream, against the serial 80-bit recurrence of tests/host/sos_ref_ld.c.

Every case: inputs N(0, 1) + 0.5 from fixed seeds, each a slice of a wider NaN-filled tensor
(row pitch > n; the outputs' surroundings must still be NaN afterwards); the handle's warm_len
is the restated sos_warmup_len of the filter; SosStream.last_launches() is the case's declared
list of launches; every channel is compared with the reference.  A forward pass follows a short
one, so it starts from a carried state, and the state it leaves is compared too (against the
largest input or output of its section over the pass: a state is a combination of the last two
of each).  An unaligned case is also run aligned, and the two must agree bit for bit.  The
forced-short cases shorten warm_len to one tile on a filter that still holds 8 % of its
response there (alone for the trimmed bodies, in front of eight fast sections for the lean ones)
and compare with segmented_ref on the nseg, segment length and pre the handle
reported: a segment start or a pre-roll off by a sample or a tile then costs about 1e-2.

The non-finite cases put a NaN into the first tile of channel 0 and an Inf at the last sample of
channel 1 of every pass's input (a backward pass's fb is then NaN in channel 1: fa and fb are
forward outputs of one stream) and ask for the reference's finite pattern exactly.  That is less
than "an isolated Inf at the last sample of fa": with a finite fb behind it the reference is NaN
throughout, while a backward pass in segments keeps it inside the segment it falls in -- the
segments have no seal, sos_tile.h rules such an fa out, and only the probe of fb's last sample is
tested here, not an Inf crossing a backward seam.

Error: max |got - ref| / max |ref| per channel.  Bound: sos_routes.bound -- max(1e-12, 16 e64),
never above 1e-8.  Every comparison prints its error, bound and ratio with the route it took.

Measured on an MI355X, worst error / bound: sos_kernel 0.25 and backwards 0.24 (lp_ill, 79
tiles), guarded 0.008; sos_split2 0.16, backwards 0.14, unaligned with a guarded tail 0.15, with a
pre-roll 0.005; sos_split_lean 0.10, backwards 0.09 (cheby16); sos_dual 0.006, sos_dual2 0.006,
sos_dual_lean 0.018 (bp32); the forced-short cases against segmented_ref 0.006 (trimmed bodies)
and 0.016 (lean bodies).  stress3 is the
exception on every route (sos_routes.SCAN_BOUND).
"""

import functools

import numpy as np
import pytest

import sos_routes as R

pytestmark = pytest.mark.gpu

SPLITS = ("sos_split2", "sos_split_lean", "sos_dual2", "sos_dual_lean")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


@functools.lru_cache(maxsize=6)
def _signal(nch, n, seed, nonfinite):
    x = R.signal(nch, n, seed)
    if nonfinite == "pass":
        x[0, 100] = np.nan
        x[1, -1] = np.inf
    elif nonfinite == "behind":
        x[1, :] = np.nan
    x.setflags(write=False)
    return x


def _inputs(case, warm_len):
    """The case's host inputs: prefix (the short forward pass in front), x, fa, fb."""
    inp = {}
    if case.op in ("forward", "step"):
        inp["prefix"] = _signal(case.nch, 777, 104, "")
        inp["x"] = _signal(case.nch, case.n if case.op == "forward" else case.nx, 101, "pass" if case.nonfinite else "")
    if case.op in ("backward", "step"):
        inp["fa"] = _signal(case.nch, case.n, 102, "pass" if case.nonfinite else "")
        # fa and fb are forward outputs of one stream: behind a non-finite sample of fa, fb is NaN
        # throughout (sos_tile.h, "NaN reach": what the backward routes rely on)
        inp["fb"] = None if case.fb == "none" else _signal(case.nch, R.fb_len(case.fb, warm_len), 103,
                                                           "behind" if case.nonfinite else "")
    return inp


def _wide(nch, n, one_in, odd):
    """A NaN-filled (nch, pitch > n) tensor and the (nch, n) slice of it that starts 16-byte
    aligned on every row -- or one sample in, or on an odd pitch."""
    import torch
    pitch = n + 10 + (n & 1) + (1 if odd else 0)
    off = 3 if one_in else 2
    buf = torch.full((nch, pitch), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[:, off:off + n]
    assert view.stride(0) > n and view.data_ptr() % 16 == (8 if one_in else 0) and view.stride(0) % 2 == int(odd)
    return buf, view, off


def _place(arr, one_in, odd):
    import torch
    buf, view, off = _wide(arr.shape[0], arr.shape[1], one_in, odd)
    view.copy_(torch.tensor(arr))
    return buf, view, off


def _surroundings_nan(buf, off, n):
    import torch
    return bool(torch.isnan(buf[:, :off]).all()) and bool(torch.isnan(buf[:, off + n:]).all())


def _run(dev, case, align):
    """The case on the GPU -> (outputs by name, carried state or None, launches)."""
    from openseize_amd import _lib
    f, sos = R.FILTERS[case.key], R.design(case.key)
    odd = align == "odd"
    s = dev.SosStream(sos, case.nch)
    try:
        assert s.warm_len == (R.NEVER if f.w is None else f.w * R.TILE), (s.warm_len, f.w)
        if case.warm is not None:
            _lib.check(s.lib.osz_sos_set_warmup_len(s.h, case.warm))
            assert s.warm_len == case.warm
        inp = _inputs(case, s.warm_len)
        outs, state, held = {}, None, []

        def out_for(src, name):
            if case.alias:
                return src
            buf, view, off = _wide(src[1].shape[0], src[1].shape[1], align == "y1", odd)
            held.append((name, buf, off, view.shape[1]))
            return buf, view, off

        if "prefix" in inp:
            s.forward(_place(inp["prefix"], False, False)[1])
        if case.op == "forward":
            x = _place(inp["x"], align == "x1", odd)
            held.append(("x", x[0], x[2], case.n))
            y = out_for(x, "y")
            s.forward(x[1], out=y[1])
            outs["y"] = y[1]
        else:
            fa = _place(inp["fa"], align == "x1", odd)
            held.append(("fa", fa[0], fa[2], case.n))
            fb = None if inp["fb"] is None else _place(inp["fb"], align == "fb1", odd)[1]
            y = out_for(fa, "y")
            if case.op == "backward":
                s.backward(fa[1], fb, out=y[1])
            else:
                x = _place(inp["x"], align == "x1", odd)
                held.append(("x", x[0], x[2], case.nx))
                fo = out_for(x, "f")
                s.step(x[1], fa[1], fb, f_out=fo[1], y_out=y[1])
                outs["f"] = fo[1]
            outs["y"] = y[1]
        launches = s.last_launches()
        if case.op != "backward":
            state = s.get_state()
        outs = {k: v.cpu().numpy() for k, v in outs.items()}
        for name, buf, off, n in held:
            assert _surroundings_nan(buf, off, n), f"{case.name}: wrote outside {name}"
        return outs, state, launches
    finally:
        s.close()


@functools.lru_cache(maxsize=2)
def _reference_of(key_case):
    """(outputs by name, (zf, scale) or None) of the case in 80 bits; key_case.expect holds the
    segments the handle reported for a `segmented` case, as (rev, nseg, seglen, pre)."""
    case = key_case
    sos = R.design(case.key)
    warm_len = case.warm if case.warm is not None else (R.FILTERS[case.key].w or 0) * R.TILE or R.NEVER
    inp = _inputs(case, warm_len)
    segs = dict((rev, rest) for rev, *rest in case.expect)
    outs, state = {}, None
    if "x" in inp:
        z0 = R.forward_ref(inp["prefix"], sos)[1]
        y, zf, peak = R.run_ref(inp["x"], sos, z0)
        if case.ref == "segmented":
            y, zf = R.segmented_ref(inp["x"], sos, z0, *segs[0])
        outs["y" if case.op == "forward" else "f"] = y
        state = (zf, np.maximum(peak, np.abs(z0).max(-1)))
    if "fa" in inp:
        # a truncated warm-up that has converged is compared with the one that reads all of fb;
        # a forced length is part of the scheme
        start = R.backward_start(inp["fa"], inp["fb"], sos, case.warm if case.warm is not None else R.NEVER)
        if case.ref == "segmented":
            outs["y"] = R.segmented_ref(inp["fa"], sos, start, *segs[1], rev=True)[0]
        else:
            outs["y"] = R.run_ref(inp["fa"], sos, start, rev=True)[0]
    return outs, state


def _reference(case, launches):
    segs = []
    if case.ref == "segmented":
        for r in launches:
            if r["kernel"] in SPLITS:
                if r["rev"] in (0, -1):
                    segs.append((0, r["nseg"], r["seglen"], r["pre"]))
                if r["rev"] in (1, -1):
                    segs.append((1, r["nseg"], r["seglen_b"] if r["rev"] == -1 else r["seglen"], r["pre"]))
    return _reference_of(case._replace(name="", align="", alias=False, expect=tuple(segs)))


def _compare(case, got, state, ref, ref_state):
    bound, where, worst = R.bound(case.key), R.route(case), 0.0
    with np.errstate(invalid="ignore"):
        for name in sorted(ref):
            assert got[name].shape == ref[name].shape
            assert np.array_equal(np.isfinite(got[name]), np.isfinite(ref[name])), \
                f"{case.name} {name}: finite pattern differs from the reference's"
            err = float(R.rel_err(got[name], ref[name]).max())
            print(f"ROUTE {where} | {case.name} {name}: err {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
            worst = max(worst, err)
        if ref_state is not None:
            zf, scale = ref_state
            assert np.array_equal(np.isfinite(state), np.isfinite(zf)), f"{case.name}: state's finite pattern"
            ok = np.isfinite(zf)
            dz = np.where(ok, np.abs(state.astype(R.LD) - zf), 0).max(-1) / np.where(scale > 0, scale, 1)
            err = float(dz.max())
            print(f"ROUTE {where} | {case.name} state: err {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
            worst = max(worst, err)
    assert worst <= bound, f"{case.name}: {worst:.3g} > {bound:.3g} on {where}"


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_route(dev, case):
    got, state, launches = _run(dev, case, case.align)
    assert launches == list(case.expect), (case.name, launches)
    ref, ref_state = _reference(case, launches)
    _compare(case, got, state, ref, ref_state)
    if case.align:
        twin, twin_state, twin_launches = _run(dev, case, "")
        assert all(r["al16"] != 0 for r in twin_launches) and any(r["al16"] == 1 for r in twin_launches)
        for name in got:
            assert np.array_equal(got[name], twin[name]), f"{case.name} {name}: differs from the aligned run"
        assert state is None or np.array_equal(state, twin_state)
