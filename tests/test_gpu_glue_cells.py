"""Every producer-arithmetic kernel (csrc/glue.hip: osz_moments_*, osz_col_moments, the sixteen osz_ew
instances, osz_complex_join, osz_magphase, osz_simpson; csrc/misc.hip: osz_take, osz_synth_normal) on the
GPU against the references of tests/glue_cells.py, at the corpus lengths that tests/test_glue_cells_host.py
shows to sit on every edge of the launch arithmetic.

Every input is a slice, never .contiguous(), of a wider NaN-filled device tensor (odd element offset, row
pitch larger than n).  Where the Python wrapper allocates a contiguous output of its own (ew, complex_join,
magphase, take; also the vectors of col_moments, moments finish and simpson) the test calls the C entry point
the way _device.py does, with the output a slice of a NaN-filled tensor whose margins must still be NaN
everywhere afterwards; the slice itself starts as a finite sentinel, so an element the kernel skips shows.
One call per kernel goes through the wrapper as well.

ew (all sixteen (op, kind)), complex_join, take and synth_normal: bit for bit (any NaN equals any NaN, signed
zeros must match).  Bounds of the rest, none of them taken from what the device gives:
  moments      |mean - ref| <= 1e-12 mean|x|;  |std - ref| <= 1e-12 kappa ref, kappa = E[x^2] / var, which is
               what sqrt(E[x^2] - E[x]^2), the reference's formula, itself imposes (the float64 NumPy formula
               keeps it with a ratio of at most 5e-4, test_glue_cells_host.py)
  col_moments  mean as above; |std - ref| <= 1e-12 ref + 4 u max|x| (the rounding of v - m)
  magphase     |mag - ref| <= 1e-14 ref, phase to 1e-13 (by value away from the cut, on the circle everywhere);
               the special values equal float64 NumPy's bit for bit
  simpson      1e-12 dx sum|p|
A flat row (var = 0) has no kappa: there the std must not exceed 1e-6 |c| = |c| sqrt(1e-12); NaN passes,
because the reference's formula gives NaN there too whenever rounding leaves E[x^2] below E[x]^2, and parity
with it, not a clamp, is the contract.

Measured on an MI355X (worst err / bound over all cases of a kind; every bit-for-bit case agrees):
  moments      mean 0.0004 (the N(1000, 1) rows; 0.0002 .. 0.0003 on the others), std 0.0005 (N(1000, 1);
               0.0003 on N(1, 3), 0.0004 on N(1e5, 1), 0.0002 on the rows with NaN)
  col_moments  mean 0.0007, std 0.0005
  magphase     mag 0.021 (2.1e-16 relative), phase 0.010 (1.0e-15) by value and on the circle
  simpson      0.0002
  none is near 0.25 of its bound.
  The thirteen special values of magphase equal NumPy's bit for bit: (1, -1e-20) gives float64(2 pi),
  (1, -0) gives -0, (-1, -0) gives pi, (inf, nan) gives |z| = inf and a NaN phase, (inf, -inf) gives 7 pi / 4.
  Constant rows, twenty cases each (std; the mean is within 1.5e-15 |c| of c everywhere):
    0.0      0 in every case
    0.1      9.1e-10 (a single push of 1, 256 or 257), 5.0e-9 (524288, alone and in the stream), NaN in the
             other fifteen cases
    7.7      5.9e-8 .. 3.6e-7 in eight cases, NaN in twelve
    123.456  1.1e-6 .. 3.2e-6 in nine cases, NaN in eleven
  so a flat channel gives NaN more often than a value, and the values are |c| times 1e-8 .. 5e-8; float64 NumPy's own
  formula at 600001 samples gives 5.6e-9, 8.4e-8, 3.3e-6 and 0 on the same four rows.
"""

import ctypes

import numpy as np
import pytest

import glue_cells as gc

pytestmark = pytest.mark.gpu

OFF_IN, OFF_OUT, EXTRA, EXTRA_AB = 3, 5, 67, 41
SENTINEL = 0.123456789e-7
INVALID = -1                              # OSZ_ERR_INVALID


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


def _nan_of(dtype):
    import torch
    return complex(np.nan, np.nan) if dtype == torch.complex128 else float("nan")


def _on_device(xh, off=OFF_IN, extra=EXTRA):
    """The rows of xh inside a wider NaN-filled tensor: slices of it have a row pitch and an odd offset."""
    import torch
    t = torch.tensor(xh, device="cuda")
    rows, n = xh.shape
    wide = torch.full((rows, n + extra), _nan_of(t.dtype), dtype=t.dtype, device="cuda")
    wide[:, off:off + n] = t
    view = wide[:, off:off + n]
    assert view.stride(0) == n + extra and view.stride(1) == 1 and (n == 0 or not view.is_contiguous() or rows == 1)
    return view


def _vec_on_device(vh, off=OFF_IN):
    """A vector at an odd offset inside a longer NaN-filled one."""
    import torch
    wide = torch.full((len(vh) + 2 * off + 1,), float("nan"), dtype=torch.float64, device="cuda")
    wide[off:off + len(vh)] = torch.tensor(vh, device="cuda")
    return wide[off:off + len(vh)]


class _Out:
    """An output of n columns inside a NaN-filled tensor of its own; the output itself starts as SENTINEL."""

    def __init__(self, rows, n, dtype=None, extra=EXTRA):
        import torch
        dtype = dtype or torch.float64
        self.n = n
        self.wide = torch.full((rows, n + extra), _nan_of(dtype), dtype=dtype, device="cuda")
        self.view = self.wide[:, OFF_OUT:OFF_OUT + n]
        self.view.fill_(SENTINEL)
        self.ld = self.view.stride(0)
        assert self.ld == n + extra

    def check(self, what):
        import torch
        parts = torch.view_as_real(self.wide) if self.wide.is_complex() else self.wide.unsqueeze(-1)
        assert bool(torch.isnan(parts[:, :OFF_OUT]).all()), (what, "written in front of the output")
        assert bool(torch.isnan(parts[:, OFF_OUT + self.n:]).all()), (what, "written behind the output")
        return self.view.cpu().numpy()


def _ok(status):
    from openseize_amd import _lib
    _lib.check(status)


# ------------------------------------------------------------------ ew
def _ew_operands(kind, a, b):
    if kind == gc.BCAST_FULL:
        return _on_device(a, OFF_OUT, EXTRA_AB), _on_device(b, OFF_IN, EXTRA_AB)
    a1, b1 = gc.operands(kind, a, b)
    return _vec_on_device(a1), _vec_on_device(b1, OFF_OUT)


def _ew_case(dev, op, kind, rows, n, seed=1):
    """One direct osz_ew call on pitched operands into an output with margins, against float64 NumPy."""
    x, a, b = gc.ew_data(rows, n, seed)
    a1, b1 = gc.operands(kind, a, b)
    xd = _on_device(x)
    ad, bd = _ew_operands(kind, a, b)
    ldab = ad.stride(0) if kind == gc.BCAST_FULL else 0
    if kind == gc.BCAST_FULL:
        assert ldab == bd.stride(0) == n + EXTRA_AB != xd.stride(0)
    out = _Out(rows, n)
    _ok(dev.require_gpu().osz_ew(op, dev.ptr(xd), xd.stride(0), rows, n, dev.ptr(ad),
                                      dev.ptr(bd) if op == gc.EW_STANDARDIZE else None, kind, ldab,
                                      dev.ptr(out.view), out.ld, dev.stream_ptr()))
    what = (gc.OP_NAME[op], gc.KIND_NAME[kind], rows, n)
    got = out.check(what)
    want = gc.ew_ref(op, x, a1, b1, kind)
    if not gc.same_bits(got, want):
        bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
        r, c = bad[0]
        raise AssertionError((what, f"{len(bad)} elements differ, first at {r, c}: x {x[r, c]!r} got {got[r, c]!r} "
                                    f"want {want[r, c]!r}"))


@pytest.mark.parametrize("kind", range(4), ids=gc.KIND_NAME)
@pytest.mark.parametrize("op", range(4), ids=gc.OP_NAME)
def test_ew_instance_bit_for_bit(dev, op, kind):
    from openseize_amd import _lib
    assert (_lib.EW_ADD, _lib.EW_MUL, _lib.EW_DIV, _lib.EW_STANDARDIZE) == (0, 1, 2, 3) == tuple(range(4))
    assert (_lib.BCAST_SCALAR, _lib.BCAST_ROW, _lib.BCAST_COL, _lib.BCAST_FULL) == (0, 1, 2, 3)
    for n in gc.N_ROW:
        _ew_case(dev, op, kind, 3, n)


@pytest.mark.parametrize("op,kind,n", [(gc.EW_ADD, gc.BCAST_SCALAR, gc.N_CAP), (gc.EW_MUL, gc.BCAST_ROW, gc.N_CAP),
                                       (gc.EW_DIV, gc.BCAST_COL, gc.N_CAP), (gc.EW_STANDARDIZE, gc.BCAST_FULL, gc.N_CAP),
                                       (gc.EW_DIV, gc.BCAST_FULL, gc.N_FULL)],
                         ids=lambda v: str(v))
def test_ew_past_the_block_cap(dev, op, kind, n):
    _ew_case(dev, op, kind, 2, n, seed=2)


def test_ew_wrapper_and_its_contiguous_path(dev):
    """dev.ew: every kind once; FULL with b pitched differently from a (the wrapper makes both contiguous)."""
    import torch
    rows, n = 3, 257
    x, a, b = gc.ew_data(rows, n, 3)
    xd = _on_device(x)
    for kind in range(4):
        a1, b1 = gc.operands(kind, a, b)
        ad, bd = _ew_operands(kind, a, b)
        for op in range(4):
            y = dev.ew(op, xd, ad, bd if op == gc.EW_STANDARDIZE else None, kind)
            assert gc.same_bits(y.cpu().numpy(), gc.ew_ref(op, x, a1, b1, kind)), (op, kind)
    ad, bd = _on_device(a, OFF_OUT, EXTRA_AB), _on_device(b, OFF_IN, EXTRA_AB + 2)
    assert ad.stride(0) != bd.stride(0)
    y = dev.ew(gc.EW_STANDARDIZE, xd, ad, bd, gc.BCAST_FULL)
    assert gc.same_bits(y.cpu().numpy(), gc.ew_ref(gc.EW_STANDARDIZE, x, a, b, gc.BCAST_FULL))
    assert torch.isnan(ad).sum() == np.isnan(a).sum()                   # the operands are left as they were


def test_ew_refuses_instead_of_crashing(dev):
    lib = dev.require_gpu()
    rows, n = 3, 65
    x, a, b = gc.ew_data(rows, n, 4)
    xd, ad, bd = _on_device(x), _on_device(a, OFF_OUT, EXTRA_AB), _on_device(b, OFF_IN, EXTRA_AB)
    out = _Out(rows, n)

    def call(op, kind, b_ptr, ldx, ldab, ldy=out.ld):
        return lib.osz_ew(op, dev.ptr(xd), ldx, rows, n, dev.ptr(ad), b_ptr, kind, ldab, dev.ptr(out.view), ldy,
                          dev.stream_ptr())
    ldx, ldab = xd.stride(0), ad.stride(0)
    assert call(4, gc.BCAST_FULL, dev.ptr(bd), ldx, ldab) == INVALID            # unknown op
    assert call(-1, gc.BCAST_FULL, dev.ptr(bd), ldx, ldab) == INVALID
    assert call(gc.EW_ADD, 4, dev.ptr(bd), ldx, ldab) == INVALID                # unknown kind
    assert call(gc.EW_ADD, -1, dev.ptr(bd), ldx, ldab) == INVALID
    assert call(gc.EW_STANDARDIZE, gc.BCAST_FULL, None, ldx, ldab) == INVALID   # standardize without b
    assert call(gc.EW_ADD, gc.BCAST_FULL, None, n - 1, ldab) == INVALID         # ldx < n
    assert call(gc.EW_ADD, gc.BCAST_FULL, None, ldx, n - 1) == INVALID          # FULL with ldab < n
    assert call(gc.EW_ADD, gc.BCAST_FULL, None, ldx, ldab, ldy=n - 1) == INVALID
    assert b"osz_ew" in lib.osz_last_error()
    import torch
    torch.cuda.synchronize()
    assert bool((out.check("refused") == SENTINEL).all())                       # nothing was launched
    assert call(gc.EW_ADD, gc.BCAST_FULL, None, ldx, ldab) == 0
    assert gc.same_bits(out.check("after the refusals"), gc.ew_ref(gc.EW_ADD, x, a, None, gc.BCAST_FULL))


# ------------------------------------------------------------------ complex_join
@pytest.mark.parametrize("n", gc.N_ROW + (gc.N_CAP, gc.N_FULL))
def test_complex_join_bit_for_bit(dev, n):
    import torch
    rows = 3 if n <= max(gc.N_ROW) else 2
    x, a, _ = gc.ew_data(rows, n, 5)
    re, im = _on_device(x), _on_device(a, OFF_OUT, EXTRA_AB)
    assert re.stride(0) != im.stride(0)
    out = _Out(rows, n, torch.complex128)
    _ok(dev.require_gpu().osz_complex_join(dev.ptr(re), re.stride(0), dev.ptr(im), im.stride(0), rows, n,
                                                dev.ptr(out.view), out.ld, dev.stream_ptr()))
    want = np.empty((rows, n), dtype=np.complex128)
    want.real, want.imag = x, a
    assert gc.same_bits(out.check(("complex_join", n)), want), n
    if n == 257:
        assert gc.same_bits(dev.complex_join(re, im).cpu().numpy(), want)


# ------------------------------------------------------------------ take
def _take_case(dev, form, nidx, rows, n_src):
    import torch
    rng = np.random.default_rng([6, nidx])
    x = rng.standard_normal((rows, n_src))
    x[0, 0], x[-1, -1], x[0, n_src // 2] = -0.0, np.nan, np.inf
    idx = gc.take_indices(form, nidx, n_src)
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < n_src)               # every index inside the row
    xd = _on_device(x)
    # the index list at an odd offset of a longer one (an empty list still has an address)
    idw = torch.zeros(len(idx) + 4, dtype=torch.int64, device="cuda")
    idw[3:3 + len(idx)] = torch.tensor(idx, device="cuda")
    idd = idw[3:3 + len(idx)]
    out = _Out(rows, max(len(idx), 1))
    _ok(dev.require_gpu().osz_take(dev.ptr(xd), xd.stride(0), rows, ctypes.c_void_p(idw.data_ptr() + 24),
                                        len(idx), dev.ptr(out.view), out.ld, dev.stream_ptr()))
    got = out.check(("take", form, nidx))
    if len(idx) == 0:
        assert bool((got == SENTINEL).all())
    else:
        assert gc.same_bits(got, x[:, idx]), (form, nidx)
    return xd, idd, x, idx


@pytest.mark.parametrize("nidx", gc.NIDX)
def test_take_bit_for_bit(dev, nidx):
    big = nidx > 1000
    for form in gc.TAKE_FORMS[:4]:
        xd, idd, x, idx = _take_case(dev, form, nidx, 2 if big else 3, nidx + (1031 if big else 41))
        if nidx == 257:
            assert gc.same_bits(dev.take(xd, idd).cpu().numpy(), x[:, idx]), form


def test_take_whole_grid_and_empty(dev):
    _take_case(dev, "mask", gc.NIDX_FULL, 1, gc.NIDX_FULL + 77)
    xd, idd, x, idx = _take_case(dev, "empty", 0, 3, 300)
    y = dev.take(xd, idd)
    assert tuple(y.shape) == (3, 0)


# ------------------------------------------------------------------ streaming moments
def _finish(dev, st):
    """osz_moments_finish into vectors with margins."""
    mean, sd = _Out(1, st.nch), _Out(1, st.nch)
    _ok(st.lib.osz_moments_finish(st.h, dev.ptr(mean.view), dev.ptr(sd.view), dev.stream_ptr()))
    return mean.check("moments mean")[0], sd.check("moments std")[0]


def _run_moments(dev, st, xd, lens, ignore):
    o = 0
    for n in lens:
        piece = xd[:, o:o + n]
        assert piece.stride(0) > piece.shape[1]
        st.push(piece, ignore_nan=ignore)
        o += n
    return _finish(dev, st)


WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.mark.parametrize("n", gc.N_MOM)
def test_moments_against_the_long_double_stream(dev, n):
    """A single push of n and the ragged stream (n, 1, 257, 0, 8193), ignore_nan both ways; rows N(1, 3),
    N(1000, 1), N(1e5, 1), one with 1 % NaN and one that is all NaN inside one push (257 rows of these kinds
    in turn for n <= 257)."""
    rows = gc.moments_nrows(n)
    kind = np.arange(rows) % len(gc.ROW_KINDS)
    failed = []
    for stream in (False, True):
        x = gc.moments_data(n, stream)
        lens = gc.moments_lens(n, stream)
        xd = _on_device(x)
        chunks = gc.chunks_of(x, lens)
        for ignore in (True, False):
            st = dev.MomentsStream(rows)
            try:
                mean, sd = _run_moments(dev, st, xd, lens, ignore)
            finally:
                st.close()
            ref = gc.moments_ref(chunks, ignore)
            # the NaN rule: a NaN poisons its own row only; an all-NaN push gives NaN either way
            want_nan = (kind == 4) | ((kind == 3) & (not ignore) & np.isnan(x).any(1))
            assert np.array_equal(np.isnan(ref[0].astype(np.float64)), want_nan)
            assert np.array_equal(np.isnan(mean), want_nan) and np.isnan(sd[want_nan]).all(), (n, stream, ignore)
            rm, rs = gc.moments_ratios(mean, sd, chunks, ignore, ref=ref)
            for k, name in enumerate(gc.ROW_KINDS):
                m, s = float(rm[kind == k].max()), float(rs[kind == k].max())
                print(f"moments n {n} stream {int(stream)} ignore_nan {int(ignore)} rows {rows} {name}: "
                      f"mean ratio {m:.4f} std ratio {s:.4f}")
                _note(("mean", name), m)
                _note(("std", name), s)
                if not (m < 1 and s < 1):
                    failed.append((stream, ignore, name, m, s))
    print("worst so far", {f"{a} {b}": round(v, 4) for (a, b), v in WORST.items()})
    assert not failed, (n, failed)


def test_moments_reset_restarts_bit_for_bit_and_handles_are_apart(dev):
    n = 8193
    x, lens = gc.moments_data(n, True), gc.moments_lens(n, True)
    xd = _on_device(x)
    other_x = gc.moments_data(16385, False)
    other_xd = _on_device(other_x)
    st, other = dev.MomentsStream(x.shape[0]), dev.MomentsStream(x.shape[0])
    try:
        first = _run_moments(dev, st, xd, lens, True)
        _ok(st.lib.osz_moments_reset(st.h, dev.stream_ptr()))
        again = _run_moments(dev, st, xd, lens, True)
        assert gc.same_bits(again[0], first[0]) and gc.same_bits(again[1], first[1])
        # two handles fed in turn: each gives what it gives alone
        alone = _run_moments(dev, other, other_xd, (16385,), True)
        _ok(st.lib.osz_moments_reset(st.h, dev.stream_ptr()))
        _ok(other.lib.osz_moments_reset(other.h, dev.stream_ptr()))
        o = 0
        for k, m in enumerate(lens):
            st.push(xd[:, o:o + m], ignore_nan=True)
            o += m
            if k == 1:
                other.push(other_xd, ignore_nan=True)
        mixed, mixed_other = _finish(dev, st), _finish(dev, other)
        assert gc.same_bits(mixed[0], first[0]) and gc.same_bits(mixed[1], first[1])
        assert gc.same_bits(mixed_other[0], alone[0]) and gc.same_bits(mixed_other[1], alone[1])
        # finish reads, it does not consume
        twice = _finish(dev, st)
        assert gc.same_bits(twice[0], first[0]) and gc.same_bits(twice[1], first[1])
        # the wrapper's own finish
        mean, sd = st.finish()
        assert gc.same_bits(mean.cpu().numpy(), first[0]) and gc.same_bits(sd.cpu().numpy(), first[1])
    finally:
        st.close()
        other.close()


def test_moments_refuses_a_pitch_below_the_length(dev):
    x = gc.moments_data(257, False)[:5]
    xd = _on_device(x)
    st = dev.MomentsStream(5)
    try:
        assert st.lib.osz_moments_push(st.h, dev.ptr(xd), 256, 257, 1, dev.stream_ptr()) == INVALID
        assert st.lib.osz_moments_push(st.h, dev.ptr(xd), xd.stride(0), -1, 1, dev.stream_ptr()) == INVALID
    finally:
        st.close()


def test_moments_of_constant_rows(dev):
    """Flat channels: var = 0, where the cancelling formula has no relative accuracy.  The std must not
    exceed 1e-6 |c|; what the device returns is printed (NaN where rounding leaves E[x^2] < E[x]^2)."""
    c = np.array(gc.CONSTANTS)
    failed = []
    for n in gc.N_MOM:
        for stream in (False, True):
            lens = gc.moments_lens(n, stream)
            x = np.repeat(c[:, None], sum(lens), axis=1)
            st = dev.MomentsStream(len(c))
            try:
                mean, sd = _run_moments(dev, st, _on_device(x), lens, True)
            finally:
                st.close()
            print(f"constant rows {gc.CONSTANTS} n {n} stream {int(stream)}: std " + " ".join(f"{v:.3e}" for v in sd)
                  + " mean - c " + " ".join(f"{v:.1e}" for v in mean - c))
            assert np.all(np.abs(mean - c) <= gc.TOL * np.abs(c)), (n, stream, mean)
            if np.any(sd > 1e-6 * np.abs(c)):
                failed.append((n, stream, sd))
    assert not failed, failed


# ------------------------------------------------------------------ col_moments
@pytest.mark.parametrize("nred", gc.NRED)
def test_col_moments_against_two_pass_long_double(dev, nred):
    lib = dev.require_gpu()
    failed = []
    for ncols in gc.NCOLS:
        x = gc.col_data(nred, ncols)
        xd = _on_device(x)
        for ignore in (True, False):
            mean, sd = _Out(1, ncols), _Out(1, ncols)
            _ok(lib.osz_col_moments(dev.ptr(xd), xd.stride(0), nred, ncols, int(ignore), dev.ptr(mean.view),
                                         dev.ptr(sd.view), dev.stream_ptr()))
            m, s = mean.check(("col mean", nred, ncols))[0], sd.check(("col std", nred, ncols))[0]
            ref = gc.col_moments_ref(x, ignore)
            # an all-NaN column gives NaN; a NaN poisons its own column only, and only when it is not ignored
            want_nan = np.isnan(x).all(0) if ignore else np.isnan(x).any(0)
            assert np.array_equal(np.isnan(m), want_nan) and np.array_equal(np.isnan(s), want_nan), (nred, ncols, ignore)
            if nred == 1:
                assert not s[~want_nan].any() and not np.signbit(s[~want_nan]).any()      # exactly 0
                assert gc.same_bits(m, x[0])
            rm, rs = gc.col_ratios(m, s, x, ignore, ref=ref)
            print(f"col_moments {nred} x {ncols} ignore_nan {int(ignore)}: mean ratio {rm.max():.4f} std ratio {rs.max():.4f}")
            _note(("col", "mean"), rm.max())
            _note(("col", "std"), rs.max())
            if not (rm.max() < 1 and rs.max() < 1):
                failed.append((ncols, ignore, float(rm.max()), float(rs.max())))
            if ncols == 257 and ignore:
                wm, ws = dev.col_moments(xd, ignore_nan=True)
                assert gc.same_bits(wm.cpu().numpy(), m) and gc.same_bits(ws.cpu().numpy(), s)
                only = _Out(1, ncols)                                                    # the mean alone
                _ok(lib.osz_col_moments(dev.ptr(xd), xd.stride(0), nred, ncols, 1, dev.ptr(only.view), None,
                                             dev.stream_ptr()))
                assert gc.same_bits(only.check("col mean alone")[0], m)
    print("worst so far", {f"{a} {b}": round(v, 4) for (a, b), v in WORST.items() if a == "col"})
    assert not failed, (nred, failed)
    assert lib.osz_col_moments(dev.ptr(xd), xd.shape[1] - 1, nred, xd.shape[1], 1, dev.ptr(mean.view), None,
                               dev.stream_ptr()) == INVALID


# ------------------------------------------------------------------ magphase
def _magphase(dev, zd, want_mag=True, want_phase=True):
    rows, n = zd.shape
    mag, ph = _Out(rows, n), _Out(rows, n)
    _ok(dev.require_gpu().osz_magphase(dev.ptr(zd), zd.stride(0), rows, n, dev.ptr(mag.view) if want_mag else None,
                                            dev.ptr(ph.view) if want_phase else None, mag.ld, dev.stream_ptr()))
    return mag.check("mag"), ph.check("phase")


@pytest.mark.parametrize("n", gc.N_ROW + (gc.N_CAP,))
def test_magphase_against_long_double(dev, n):
    rows = 3 if n <= max(gc.N_ROW) else 2
    z = gc.magphase_data(rows, n)
    if n >= 2:
        z[0, 0], z[0, 1] = complex(1.0, 1e-12), complex(1.0, -1e-12)      # next to the cut, on either side of it
    zd = _on_device(z)
    mag, ph = _magphase(dev, zd)
    rmag, rph = gc.magphase_ref(z)
    emag = float(np.max(np.abs(mag.astype(gc.LD) - rmag) / rmag))
    two_pi = 2 * np.arctan2(gc.LD(0), gc.LD(-1))
    away = np.minimum(rph, two_pi - rph) > 1e-6
    eph = float(np.max(np.abs(ph.astype(gc.LD) - rph)[away], initial=0.0))
    ecirc = float(np.max(np.abs(np.exp(1j * ph) - np.exp(1j * rph.astype(np.float64)))))
    print(f"magphase n {n}: mag err {emag:.3e} ratio {emag / gc.TOL_MAG:.4f} phase err {eph:.3e} ratio "
          f"{eph / gc.TOL_PHASE:.4f} circle {ecirc:.3e} ratio {ecirc / gc.TOL_PHASE:.4f}")
    _note(("magphase", "mag"), emag / gc.TOL_MAG)
    _note(("magphase", "phase"), max(eph, ecirc) / gc.TOL_PHASE)
    assert (~away).sum() <= 4 and ph.min() >= 0 and ph.max() <= 2 * np.pi
    assert emag <= gc.TOL_MAG and eph <= gc.TOL_PHASE and ecirc <= gc.TOL_PHASE, (n, emag, eph, ecirc)
    # one output alone: the other is left untouched, the wanted one has the same bits
    only_mag, untouched = _magphase(dev, zd, want_phase=False)
    assert gc.same_bits(only_mag, mag) and bool((untouched == SENTINEL).all())
    untouched, only_ph = _magphase(dev, zd, want_mag=False)
    assert gc.same_bits(only_ph, ph) and bool((untouched == SENTINEL).all())
    print("worst so far", {f"{a} {b}": round(v, 4) for (a, b), v in WORST.items() if a == "magphase"})


def test_magphase_special_values_are_numpys(dev):
    z = gc.SPECIAL_Z.reshape(1, -1).copy()
    mag, ph = _magphase(dev, _on_device(z))
    wmag, wph = gc.magphase_numpy(z)
    for k in range(z.shape[1]):
        print(f"magphase {z[0, k]!r}: mag {mag[0, k]!r} (NumPy {wmag[0, k]!r}) phase {ph[0, k]!r} (NumPy {wph[0, k]!r})")
    k = list(gc.SPECIAL_Z).index(complex(1.0, -1e-20))
    assert wph[0, k] == 2 * np.pi                             # a phase that rounds to 2 pi IS 2 pi
    bad = [(z[0, k], mag[0, k], wmag[0, k], ph[0, k], wph[0, k]) for k in range(z.shape[1])
           if not (gc.same_bits(mag[:, k], wmag[:, k]) and gc.same_bits(ph[:, k], wph[:, k]))]
    assert not bad, bad


def test_magphase_wrapper(dev):
    import torch
    z = gc.magphase_data(3, 257)
    zd = _on_device(z)
    mag, ph = _magphase(dev, zd)
    wm, wp = dev.magphase(zd)
    assert gc.same_bits(wm.cpu().numpy(), mag) and gc.same_bits(wp.cpu().numpy(), ph)
    wm, wp = dev.magphase(zd, want_phase=False)
    assert wp is None and gc.same_bits(wm.cpu().numpy(), mag)
    wm, wp = dev.magphase(zd, want_mag=False)
    assert wm is None and gc.same_bits(wp.cpu().numpy(), ph)
    buf = torch.full((3, 257), SENTINEL, dtype=torch.float64, device="cuda")
    wm, wp = dev.magphase(zd, mag_out=buf)
    assert wm is buf and gc.same_bits(buf.cpu().numpy(), mag) and gc.same_bits(wp.cpu().numpy(), ph)
    with pytest.raises(ValueError):
        dev.magphase(zd, mag_out=buf[:, :256])
    lib = dev.require_gpu()
    assert lib.osz_magphase(dev.ptr(zd), 256, 3, 257, dev.ptr(buf), None, 257, dev.stream_ptr()) == INVALID
    assert lib.osz_magphase(dev.ptr(zd), zd.stride(0), 3, 257, dev.ptr(buf), None, 256, dev.stream_ptr()) == INVALID
    assert lib.osz_magphase(dev.ptr(zd), zd.stride(0), 3, 257, None, None, 257, dev.stream_ptr()) == INVALID


# ------------------------------------------------------------------ simpson
@pytest.mark.parametrize("dx", gc.SIMPSON_DX)
def test_simpson_against_long_double(dev, dx):
    lib = dev.require_gpu()
    p = gc.simpson_data()
    failed, worst = [], 0.0
    for rows in gc.SIMPSON_ROWS:
        pd = _on_device(p[:rows])
        for a in gc.SIMPSON_A:
            for m in gc.M_SIMPSON:
                out = _Out(1, rows)
                _ok(lib.osz_simpson(dev.ptr(pd), pd.stride(0), rows, a, m, dx, dev.ptr(out.view), dev.stream_ptr()))
                got = out.check(("simpson", rows, a, m))[0]
                seg = p[:rows, a:a + m]
                err = np.abs(got.astype(gc.LD) - gc.simpson_ref(seg, dx))
                ratio = float(np.max(err / gc.simpson_bound(seg, dx)))
                print(f"simpson rows {rows} a {a} m {m} dx {dx}: ratio {ratio:.4f}")
                worst = max(worst, ratio)
                if m == 1:
                    assert not got.any()
                if not ratio < 1:
                    failed.append((rows, a, m, ratio))
    _note(("simpson", "sum"), worst)
    print("worst so far", {f"{a} {b}": round(v, 4) for (a, b), v in WORST.items() if a == "simpson"})
    assert not failed, failed
    # the wrapper, and a range that runs past the row
    m = 2050
    got = dev.simpson(pd, 3, m, dx).cpu().numpy()
    assert np.all(np.abs(got.astype(gc.LD) - gc.simpson_ref(p[:, 3:3 + m], dx)) <= gc.simpson_bound(p[:, 3:3 + m], dx))
    out = _Out(1, pd.shape[0])
    assert lib.osz_simpson(dev.ptr(pd), 3 + m - 1, pd.shape[0], 3, m, dx, dev.ptr(out.view), dev.stream_ptr()) == INVALID
    assert lib.osz_simpson(dev.ptr(pd), pd.stride(0), pd.shape[0], 3, 0, dx, dev.ptr(out.view), dev.stream_ptr()) == INVALID
    import torch
    torch.cuda.synchronize()
    assert bool((out.check("simpson refused") == SENTINEL).all())


# ------------------------------------------------------------------ synth_normal
def test_synth_normal_blocks_are_slices_of_the_whole(dev):
    """The value depends on (seed, channel, sample) alone: blocks generated with (ch0, n0) offsets are the
    matching slices of one whole call, past the 1024-block cap too, and into a pitched out=."""
    import torch
    n = gc.N_SYNTH
    whole = dev.synth_normal(3, n, seed=5)
    assert tuple(whole.shape) == (3, n) and bool(torch.isfinite(whole).all())
    for ch0, nch, n0, m in ((0, 3, 0, 257), (1, 2, 1, 256), (2, 1, 255, 2049), (1, 2, n - 262145, 262145),
                            (0, 1, 262144, n - 262144), (1, 1, n - 1, 1)):
        part = dev.synth_normal(nch, m, seed=5, ch0=ch0, n0=n0)
        assert torch.equal(part, whole[ch0:ch0 + nch, n0:n0 + m]), (ch0, nch, n0, m)
    out = _Out(2, n)
    got = dev.synth_normal(2, n, seed=5, ch0=1, out=out.view)
    assert got is out.view
    assert gc.same_bits(out.check("synth_normal"), whole[1:3].cpu().numpy())
    assert not torch.equal(dev.synth_normal(3, 257, seed=6), whole[:, :257])
    assert not torch.equal(whole[0, :1000], whole[1, :1000]) and not torch.equal(whole[0, :999], whole[0, 1:1000])
