"""The launch routes of the stand-alone SOS cascade (csrc/sos.hip) and what tests them.

One call of SosStream.forward / backward / step reaches one of fifteen kernel instances
(REACHABLE), chosen by nsec, nch, the chunk length in tiles, warm_len, pointer alignment and
aliasing.  This module holds

* the definition they are compared with: tests/host/sos_ref_ld.c, a serial DF2T cascade in
  80-bit long double, compiled here with ``gcc -O2`` into a shared object of its own, and on
  it ``forward_ref``, ``backward_ref`` (the chunk-local scheme of include/osz_hip.h) and
  ``segmented_ref`` (the truncated scheme of sos_segment, fed with the nseg, segment length
  and pre the handle reported);
* ``warmup_len``: sos_warmup_len restated in longdouble NumPy, where each filter's w comes from;
* FILTERS: SciPy designs, each with the w it must get and its e64, the error of the float64
  serial recurrence (scipy.signal.sosfilt) against the 80-bit one over 600 000 samples of
  N(0, 1) + 0.5, relative to max |ref| (``measure_e64``);
* CASES: (filter, nch, lengths, alignment, aliasing, fb kind) with the launches each must
  produce, as SosStream.last_launches() reports them;
* UNREACHED: compiled instances (and one branch) no call reaches, with the reason and the
  source line that makes it so;
* ``bound``: the tolerance of a filter, and SCAN_BOUND, the filters that miss it on every route
  alike, with the figures measured.

Shared by tests/test_sos_routes_host.py (no GPU) and tests/test_gpu_sos_routes.py.
"""

import ctypes
import os
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4 * 64 * 32            # kSosNW * 64 * kSosT
NEVER = 1 << 62               # warm_len of a cascade that has not converged within the cap
CAP = 1 << 24
LD = np.longdouble
FIELDS = ("kernel", "rev", "guard", "al16", "nseg", "seglen", "seglen_b", "pre", "prex", "warmup",
          "n", "n_b")

# ------------------------------------------------------------------ the 80-bit reference
_REF = {}


def ref_lib(plain=False):
    """tests/host/sos_ref_ld.c as a shared object of its own (one build per process); plain:
    without its shortcut past a NaN state."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 80-bit format here"
    tag = "plain" if plain else "lib"
    if tag not in _REF:
        src = os.path.join(ROOT, "tests", "host", "sos_ref_ld.c")
        with tempfile.TemporaryDirectory() as tmp:      # a loaded library outlives its file
            path = os.path.join(tmp, "libsos_ref_ld.so")
            subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-shared", "-fPIC"]
                                  + (["-DSOS_REF_PLAIN"] if plain else []) + [src, "-o", path, "-lm"])
            lib = ctypes.CDLL(path)
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        lib.sos_ref_ld.restype = ctypes.c_int
        lib.sos_ref_ld.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, i64, vp, i64, i64, i64, vp, vp, vp]
        assert ctypes.sizeof(ctypes.c_longdouble) == np.dtype(LD).itemsize == 16
        _REF[tag] = lib
    return _REF[tag]


def _pool():
    if "pool" not in _REF:
        from concurrent.futures import ThreadPoolExecutor
        _REF["pool"] = ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1)))
    return _REF["pool"]


def run_ref(x, sos, zi=None, rev=False, want_y=True, plain=False):
    """The cascade over x (nch, n) from state zi (nsec, nch, 2; None: zero), samples in rising
    (rev: falling) order -> (y float64 or None, zf longdouble, peak longdouble (nsec, nch)).
    Channels are independent: each is one call of the serial C recurrence, a few at a time."""
    lib = ref_lib(plain)
    x = np.ascontiguousarray(x, np.float64)
    sos = np.ascontiguousarray(sos, np.float64)
    nch, n = x.shape
    nsec = sos.shape[0]
    zi = np.zeros((nsec, nch, 2), LD) if zi is None else np.asarray(zi, LD)
    assert zi.shape == (nsec, nch, 2)
    y = np.empty_like(x) if want_y else None
    zf, peak = np.empty((nsec, nch, 2), LD), np.empty((nsec, nch), LD)

    def one(c):
        zc, zo, pk = np.ascontiguousarray(zi[:, c:c + 1]), np.empty((nsec, 1, 2), LD), np.empty((nsec, 1), LD)
        rc = lib.sos_ref_ld(sos.ctypes.data, nsec, 1, x[c].ctypes.data, n, y[c].ctypes.data if want_y else None,
                            n, n, -1 if rev else 1, zc.ctypes.data, zo.ctypes.data, pk.ctypes.data)
        assert rc == 0
        zf[:, c], peak[:, c] = zo[:, 0], pk[:, 0]

    list(_pool().map(one, range(nch)) if nch > 1 else map(one, range(nch)))
    return y, zf, peak


def forward_ref(x, sos, zi=None):
    y, zf, _ = run_ref(x, sos, zi)
    return y, zf


def zi_unit(sos):
    """The steady-state unit-step state of each section (scipy.signal.sosfilt_zi), as
    osz_sos_create derives it, in long double: (nsec, 2)."""
    sos = np.asarray(sos, np.float64).astype(LD)
    out, scale = np.zeros((sos.shape[0], 2), LD), LD(1)
    for s, (b0, b1, b2, a0, a1, a2) in enumerate(sos):
        b0, b1, b2, a1, a2 = b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0
        g = (b0 + b1 + b2) / (1 + a1 + a2)
        out[s] = scale * (g - b0), scale * (b2 - a2 * g)
        scale = scale * g
    return out


def warm_state(fb, sos, warm_len):
    """State after the chunk-local warm-up over fb[:, :min(nb, warm_len)], run backwards from
    zi_unit * its last sample."""
    m = min(fb.shape[1], warm_len)
    head = np.ascontiguousarray(fb[:, :m])
    z0 = zi_unit(sos)[:, None, :] * head[:, m - 1].astype(LD)[None, :, None]
    return run_ref(head, sos, z0, rev=True, want_y=False)[1]


def backward_start(fa, fb, sos, warm_len):
    if fb is not None:
        return warm_state(fb, sos, warm_len)
    with np.errstate(invalid="ignore"):      # an Inf there times a zero of zi_unit is the NaN it should be
        return zi_unit(sos)[:, None, :] * fa[:, -1].astype(LD)[None, :, None]


def backward_ref(fa, fb, sos, warm_len):
    """osz_sosfiltfilt_chunk as include/osz_hip.h defines it: back-filter fa from the state the
    warm-up over fb leaves, or without fb from zi_unit * fa[:, -1]."""
    return run_ref(fa, sos, backward_start(fa, fb, sos, warm_len), rev=True)[0]


def segmented_ref(x, sos, zi, nseg, seglen, pre, rev=False):
    """One pass cut as sos_segment cuts it: segment s covers seglen samples in processing order
    (the last one the rest); s > 0 starts from a ZERO state `pre` samples early and those outputs
    are dropped; segment 0 starts from zi, the last segment gives the carried state -> (y, zf)."""
    xp = np.ascontiguousarray(x[:, ::-1]) if rev else np.ascontiguousarray(x)
    n = xp.shape[1]
    y, zf = np.empty_like(xp), None
    assert nseg >= 1 and (nseg - 1) * seglen < n and (nseg == 1 or pre <= seglen)
    for s in range(nseg):
        begin = s * seglen
        length = n - begin if s == nseg - 1 else seglen
        p = pre if s > 0 else 0
        ys, zf, _ = run_ref(xp[:, begin - p:begin + length], sos, zi if s == 0 else None)
        y[:, begin:begin + length] = ys[:, p:]
    return (np.ascontiguousarray(y[:, ::-1]) if rev else y), zf


# ------------------------------------------------------------------ sos_warmup_len, restated
def warmup_len(sos, quantum=TILE, cap=CAP):
    """sos_warmup_len of sos.hip in longdouble NumPy: the smallest multiple of `quantum` with
    ||M^k||_inf < 1e-18, M the state-transition matrix of the whole cascade; NEVER when that
    takes `cap` samples or more (osz_sos_create)."""
    sos = np.asarray(sos, np.float64)
    c = sos / sos[:, 3:4]                         # build_section divides in float64
    ns = len(c)
    d = 2 * ns
    M = np.zeros((d, d), LD)
    for col in range(d):
        z, zn, u = np.zeros(d, LD), np.zeros(d, LD), LD(0)
        z[col] = 1
        for s in range(ns):
            b0, b1, b2, _, a1, a2 = (LD(v) for v in c[s])
            y = b0 * u + z[2 * s]
            zn[2 * s] = b1 * u - a1 * y + z[2 * s + 1]
            zn[2 * s + 1] = b2 * u - a2 * y
            u = y
        M[:, col] = zn
    Mq, base, e = np.eye(d, dtype=LD), M, quantum
    while e > 0:
        if e & 1:
            Mq = Mq @ base
        base = base @ base
        e >>= 1
    P, length = Mq, quantum
    while length < cap:
        nm = np.abs(P).sum(axis=1).max()
        if nm != nm:
            break
        if nm < LD("1e-18"):
            return length
        P = P @ Mq
        length += quantum
    return NEVER


# ------------------------------------------------------------------ filters
Filt = namedtuple("Filt", "design nsec w e64 role")


def _sp():
    import scipy.signal as sps
    return sps


# e64: measure_e64 on this project's CPU reference build (SciPy's float64 sosfilt against the
# 80-bit recurrence); w: warmup_len / TILE (None: NEVER).  tests/test_sos_routes_host.py
# re-measures both.
FILTERS = {
    "hp1": Filt(lambda s: s.butter(1, 0.3, "highpass", output="sos"), 1, 1, 1.08e-16, "one section"),
    "lp4": Filt(lambda s: s.butter(4, 0.2, output="sos"), 2, 1, 7.55e-16, "fast, w = 1"),
    "bp6": Filt(lambda s: s.butter(6, [0.05, 0.3], "bandpass", output="sos"), 6, 1, 9.72e-15, "the project's usual"),
    "bp8": Filt(lambda s: s.butter(8, [0.1, 0.4], "bandpass", output="sos"), 8, 1, 3.71e-15, "= kSos2MaxSec"),
    "bp9": Filt(lambda s: s.butter(9, [0.1, 0.4], "bandpass", output="sos"), 9, 1, 9.09e-15, "first lean route"),
    "bp32": Filt(lambda s: s.butter(32, [0.2, 0.6], "bandpass", output="sos"), 32, 1, 1.39e-14, "= kSosMaxSec"),
    "ellip8": Filt(lambda s: s.ellip(8, 0.5, 60, [0.1, 0.4], "bandpass", output="sos"), 8, 2, 5.61e-15, "slow, trimmed body"),
    "cheby16": Filt(lambda s: s.cheby1(16, 1, [0.2, 0.5], "bandpass", output="sos"), 16, 3, 5.6e-13, "slow, lean"),
    "narrow2": Filt(lambda s: s.butter(2, [0.1 - 1.5e-4, 0.1 + 1.5e-4], "bandpass", output="sos"), 2, 18, 2.33e-14,
                    "8 % of the response one tile back"),
    "narrow10": Filt(lambda s: np.vstack([s.butter(2, [0.1 - 1.5e-4, 0.1 + 1.5e-4], "bandpass", output="sos"),
                                          s.butter(8, [0.05, 0.3], "bandpass", output="sos")]), 10, 19, 2.71e-14,
                     "the same in front of 8 fast sections: the lean routes' seams"),
    "stress3": Filt(lambda s: s.butter(3, [0.5, 4], "bandpass", fs=5000, output="sos"), 3, 24, 3.73e-12,
                    "the stress filter"),
    "lp_ill": Filt(lambda s: s.butter(2, 3e-4, output="sos"), 1, 10, 1.74e-11, "ill-conditioned"),
    "notch": Filt(lambda s: s.tf2sos(*s.iirnotch(0.1, 3e5)), 1, None, 1.66e-13,
                  "decays over about 8e7 samples, above the cap: never segmented"),
}


def design(key):
    return np.ascontiguousarray(FILTERS[key].design(_sp()), np.float64)


def signal(nch, n, seed):
    """N(0, 1) + 0.5 from a fixed seed."""
    return np.random.default_rng(seed).standard_normal((nch, n)) + 0.5


def rel_err(got, ref):
    """max |got - ref| / max |ref| per channel (non-finite reference samples left out)."""
    ok = np.isfinite(ref)
    scale = np.where(ok, np.abs(ref), 0).max(axis=-1)
    diff = np.where(ok, np.abs(got.astype(LD) - ref.astype(LD)), 0).max(axis=-1)
    return (diff / np.where(scale > 0, scale, 1)).astype(np.float64)


def measure_e64(key, n=600000):
    sos = design(key)
    x = signal(1, n, 64)
    ref = forward_ref(x, sos)[0]
    return float(rel_err(_sp().sosfilt(sos, x, axis=-1), ref)[0])


# Filters that miss max(1e-12, 16 e64) on EVERY route alike, the unsegmented one-workgroup
# sos_kernel included: that is the conditioning of the parallel scan on the filter, not a route's
# seam, and the filter keeps the bound the project held before (1e-12 at w = 1, 1e-8 otherwise).
#   stress3 (16 e64 = 5.97e-11), error / (16 e64) measured on an MI355X, 3 channels:
#     sos_kernel 1 tile 1.62, 191 tiles 2.15; sos_split2 + seal 192 tiles 2.03, 193 tiles 2.03;
#     sos_split2 + seal + guarded tail 1.46 and 1.53; backwards sos_kernel 1.86 and 1.63,
#     sos_split2 1.36 and 2.07, sos_split2 unaligned + guarded tail 2.13 and 2.07
#   so 22 to 34 e64 where the other twelve filters stay below 4 e64.  Its poles lie at radius
#   0.9965 to 0.9997, within 0.0045 rad of z = 1.  Supposed, not measured: every lane filters its
#   32 samples from a zero state and the true start state's response is added afterwards
#   (sos.hip, steps 1 and 3); this close to z = 1 both terms carry the slow transient of the
#   input's mean (0.5) and cancel, where the serial recurrence never leaves the steady state.
SCAN_BOUND = {"stress3": 1e-8}


def bound(key):
    """The tolerance of a filter on every route: max(1e-12, 16 e64), never above 1e-8.  1e-12 is the tightest
    bound the project held for these routes before, 1e-8 the loosest; 16 = four scan levels
    (within a lane, across a wave, across waves, the tile carry) each injecting roundings that
    travel through the same dynamics as the serial recurrence's own, times 4 of headroom.
    SCAN_BOUND: the filters that miss it on every route alike."""
    if key in SCAN_BOUND:
        assert FILTERS[key].w != 1
        return SCAN_BOUND[key]
    b = max(1e-12, 16 * FILTERS[key].e64)
    assert b <= 1e-8
    return b


# ------------------------------------------------------------------ launches
# an instance is (kernel, REV, GUARD, AL16) as a launch record names it (-1: not a parameter of
# that kernel; REV -1: the dual launches run one pass of each direction)
REACHABLE = frozenset(
    [("sos_kernel", rev, guard, -1) for rev in (0, 1) for guard in (0, 1)]
    + [("sos_split_lean", rev, 0, -1) for rev in (0, 1)]
    + [("sos_split2", rev, 0, al) for rev in (0, 1) for al in (0, 1)]
    + [("sos_dual", -1, 0, -1), ("sos_dual_lean", -1, 0, -1), ("sos_dual2", -1, 0, 0), ("sos_dual2", -1, 0, 1),
       ("seal", 0, 0, -1)])

# what is compiled (or written) and never runs: (what, why, the line of csrc/sos.hip that makes it so)
UNREACHED = (
    ("sos_kernel, sos_split_lean_kernel and sos_split_kernel at T, NW = (32, 8), (16, 8), (16, 4)",
     "osz_sos_create fixes the geometry of every handle at kSosT = 32, kSosNW = 4, so sos_launch only ever "
     "takes its first branch",
     "const int T = kSosT, NW = kSosNW;"),
    ("sos_split_kernel<T, NW, REV> (kernel name sos_split), every instance",
     "sos_launch_main picks it only when sos_lean() is false, and sos_lean() is a constant true",
     "static constexpr bool sos_lean() { return true; }"),
    ("sos_split2_kernel<32, 4, REV, AL16, PF = true> and sos_dual2_kernel<32, 4, AL16, PF = true>",
     "both launch sites pick a PF instance only when sos_pf() is true, and sos_pf() is a constant false",
     "static constexpr bool sos_pf() { return false; }"),
    ("the `if (bw.prex)` fallback of osz_sosfiltfilt_step (the warm-up as a launch of its own in front "
     "of sos_dual_kernel)",
     "bw.prex is set only under dual2, which holds nx and na at 8 tiles or more, so tmin / 4 >= 2 and the "
     "dual launch in segments always returns first",
     "if (bw.prex) {   // not the trimmed dual launch after all: the warm-up as its own launch"),
)
UNREACHED_KERNELS = frozenset(["sos_split"])


def _rec(kernel, rev, n, guard=0, al16=-1, nseg=1, seglen=None, seglen_b=0, pre=0, prex=0, warmup=0, n_b=0):
    return dict(kernel=kernel, rev=rev, guard=guard, al16=al16, nseg=nseg, seglen=n if seglen is None else seglen,
                seglen_b=seglen_b, pre=pre, prex=prex, warmup=warmup, n=n, n_b=n_b)


def K(n, rev=0, guard=0, warmup=0):
    """sos_kernel over n samples."""
    return _rec("sos_kernel", rev, n, guard=guard, warmup=warmup)


def SPLIT(key, tiles, seg_tiles, nseg, rev=0, al16=1, prex=0, pre=None):
    """One pass in time segments: sos_split2 up to kSos2MaxSec = 8 sections, sos_split_lean above."""
    f = FILTERS[key]
    lean = f.nsec > 8
    return _rec("sos_split_lean" if lean else "sos_split2", rev, tiles * TILE, al16=-1 if lean else al16, nseg=nseg,
                seglen=seg_tiles * TILE, pre=f.w * TILE if pre is None else pre, prex=prex)


def SEAL(tiles, seg_tiles, nseg):
    return _rec("seal", 0, tiles * TILE, nseg=nseg, seglen=seg_tiles * TILE)


def DUAL(tx, ta):
    """sos_dual_kernel: one workgroup per channel and pass."""
    return _rec("sos_dual", -1, tx * TILE, seglen=tx * TILE, seglen_b=ta * TILE, n_b=ta * TILE)


def DUALSEG(key, tx, ta, nseg, al16=1, prex=0, pre=TILE):
    """Both passes in nseg time segments each: sos_dual2 up to 8 sections, sos_dual_lean above."""
    lean = FILTERS[key].nsec > 8
    return _rec("sos_dual_lean" if lean else "sos_dual2", -1, tx * TILE, al16=-1 if lean else al16, nseg=nseg,
                seglen=-(-tx // nseg) * TILE, seglen_b=-(-ta // nseg) * TILE, pre=pre, prex=prex, n_b=ta * TILE)


# op: forward | backward | step.  n: samples of the forward chunk (forward) or of fa (backward,
# step); nx: samples of step's forward chunk.  fb: none | 1 | w-1 | w | long (nb = 1, warm_len - 1,
# warm_len, warm_len + 4321).  align: "" or which view starts one sample into its buffer (x1: the
# input -- x, fa; y1: the output; fb1) or odd (every row pitch odd).  alias: out= is the input.
# warm: None or the length osz_sos_set_warmup_len forces.  ref: plain (the unsegmented
# definition) | segmented (segmented_ref on what the handle reported).  nonfinite: a NaN in the
# first tile of channel 0 and an Inf at the last sample of channel 1 of every input pass.
Case = namedtuple("Case", "name key op nch n nx fb align alias warm ref nonfinite expect")


def _case(name, key, op, n, expect, nch=3, nx=0, fb="none", align="", alias=False, warm=None, ref="plain",
          nonfinite=False):
    return Case(name, key, op, nch, n, nx, fb, align, alias, warm, ref, nonfinite, tuple(expect))


def fb_len(kind, warm_len):
    return {"none": 0, "1": 1, "w-1": warm_len - 1, "w": warm_len, "long": warm_len + 4321}[kind]


def _single_pass():
    out = []
    for op, rev in (("forward", 0), ("backward", 1)):
        fwd = not rev

        def add(name, key, n, expect, **kw):
            out.append(_case(f"{op}-{key}-{name}", key, op, n, expect, **kw))

        def tail(main, rem):     # whole tiles first in processing order, then the guarded rest
            return main + [K(rem, rev, guard=1)]

        # the guarded kernel alone
        # (a band-pass has no DC gain: started backwards from zi_unit * fa[:, -1], its steady state,
        # its first outputs are zero but for roundings, and an error relative to max |ref| says
        # nothing before the pass has run a few dozen samples -- so n = 1, 2 go backwards through a
        # low-pass only)
        for n in (1, 2, 63, 8191):
            add(f"n{n}", "lp4", n, [K(n, rev, guard=1)])
            if fwd or n >= 63:
                add(f"n{n}", "bp6", n, [K(n, rev, guard=1)])
        for key, f in FILTERS.items():
            if f.w is None:
                continue
            w = f.w
            # whole tiles, one workgroup per channel: max_seg = ntiles / (4 w) < 2
            add("1tile", key, TILE, [K(TILE, rev)])
            add("8w-1", key, (8 * w - 1) * TILE, [K((8 * w - 1) * TILE, rev)])
            # two segments of 4 w tiles
            two = [SPLIT(key, 8 * w, 4 * w, 2, rev)] + ([SEAL(8 * w, 4 * w, 2)] if fwd else [])
            add("8w", key, 8 * w * TILE, two)
            # uneven: 4 w + 1 and 4 w tiles
            add("8w+1", key, (8 * w + 1) * TILE,
                [SPLIT(key, 8 * w + 1, 4 * w + 1, 2, rev)] + ([SEAL(8 * w + 1, 4 * w + 1, 2)] if fwd else []))
            if w == 1:           # 13 / 4 = 3 segments: 5, 5 and 3 tiles
                add("13", key, 13 * TILE, [SPLIT(key, 13, 5, 3, rev)] + ([SEAL(13, 5, 3)] if fwd else []))
            # main plus tail through the carry; backwards the main launch starts `rem` samples into
            # the row, an odd count: its rows are no longer 16-byte aligned
            odd = [SPLIT(key, 8 * w, 4 * w, 2, rev, al16=1 if fwd else 0)] + ([SEAL(8 * w, 4 * w, 2)] if fwd else [])
            add("8w+1s", key, 8 * w * TILE + 1, tail(odd, 1))
            add("8w+8191s", key, 8 * w * TILE + 8191, tail(odd, 8191))
        # never segmented: in place, as many channels as resident workgroups, a cascade that has
        # not converged
        for key in ("lp4", "bp9"):       # w = 1: every length of the segmented group, in place
            add("8w-alias", key, 8 * TILE, [K(8 * TILE, rev)], alias=True)
            add("8w+1-alias", key, 9 * TILE, [K(9 * TILE, rev)], alias=True)
            add("13-alias", key, 13 * TILE, [K(13 * TILE, rev)], alias=True)
            add("8w+1s-alias", key, 8 * TILE + 1, tail([K(8 * TILE, rev)], 1), alias=True)
            add("8w+8191s-alias", key, 8 * TILE + 8191, tail([K(8 * TILE, rev)], 8191), alias=True)
        add("768ch", "lp4", 8 * TILE, [K(8 * TILE, rev)], nch=768)
        add("16", "notch", 16 * TILE, [K(16 * TILE, rev)])
        # two segments because 500 channels leave room for two: ceil(768 / 500)
        add("500ch", "lp4", 8 * TILE, [SPLIT("lp4", 8, 4, 2, rev)] + ([SEAL(8, 4, 2)] if fwd else []), nch=500)
        # rows that are not 16-byte aligned
        for align in ("x1", "y1", "odd"):
            add(f"8w-{align}", "lp4", 8 * TILE,
                [SPLIT("lp4", 8, 4, 2, rev, al16=0)] + ([SEAL(8, 4, 2)] if fwd else []), align=align)
        # non-finite samples on the lean route
        add("8w-nonfinite", "bp9", 8 * TILE, [SPLIT("bp9", 8, 4, 2, rev)] + ([SEAL(8, 4, 2)] if fwd else []),
            nonfinite=True)
        # a pre-roll forced too short on the filter that keeps 8 % of its response a tile back
        add("short-8", "narrow2", 8 * TILE,
            [SPLIT("narrow2", 8, 4, 2, rev, pre=TILE)] + ([SEAL(8, 4, 2)] if fwd else []), warm=TILE, ref="segmented")
        add("short-13", "narrow2", 13 * TILE,
            [SPLIT("narrow2", 13, 5, 3, rev, pre=TILE)] + ([SEAL(13, 5, 3)] if fwd else []), warm=TILE,
            ref="segmented")
        # the same on the lean body: that filter in front of eight fast sections
        add("short-8", "narrow10", 8 * TILE,
            [SPLIT("narrow10", 8, 4, 2, rev, pre=TILE)] + ([SEAL(8, 4, 2)] if fwd else []), warm=TILE, ref="segmented")
        add("short-13", "narrow10", 13 * TILE,
            [SPLIT("narrow10", 13, 5, 3, rev, pre=TILE)] + ([SEAL(13, 5, 3)] if fwd else []), warm=TILE,
            ref="segmented")
        # a warm_len that is no whole number of tiles: no segments
        add("ragged-warm", "narrow2", 8 * TILE, [K(8 * TILE, rev)], warm=8000)
    return out


def _warmups():
    """The chunk-local warm-up of the backward pass."""
    out = []

    def add(name, key, n, fb, expect, **kw):
        out.append(_case(f"backward-{key}-{name}-fb{fb}", key, "backward", n, expect, fb=fb, **kw))

    def wk(n, guard=0):
        return K(n, 1, guard=guard, warmup=1)

    for key in ("lp4", "bp8"):       # trimmed body, w = 1: the warm-up rides the launch when it is a whole tile
        main = SPLIT(key, 8, 4, 2, 1)
        ride = SPLIT(key, 8, 4, 2, 1, prex=1)
        add("8", key, 8 * TILE, "1", [wk(1, 1), main])
        add("8", key, 8 * TILE, "w-1", [wk(TILE - 1, 1), main])
        add("8", key, 8 * TILE, "w", [ride])
        add("8", key, 8 * TILE, "long", [ride])
        add("8+100s", key, 8 * TILE + 100, "w", [ride, K(100, 1, guard=1)])
        add("7", key, 7 * TILE, "w", [wk(TILE), K(7 * TILE, 1)])
    for align in ("x1", "y1", "fb1", "odd"):
        add(f"8-{align}", "lp4", 8 * TILE, "w", [SPLIT("lp4", 8, 4, 2, 1, al16=0, prex=1)], align=align)
    # lean bodies take no pre-roll
    lean = SPLIT("bp9", 8, 4, 2, 1)
    add("8", "bp9", 8 * TILE, "w-1", [wk(TILE - 1, 1), lean])
    add("8", "bp9", 8 * TILE, "w", [wk(TILE), lean])
    add("8", "bp9", 8 * TILE, "long", [wk(TILE), lean])
    # w = 2: a warm-up launch of two tiles, or of one tile and a guarded rest
    slow = SPLIT("ellip8", 16, 8, 2, 1)
    add("16", "ellip8", 16 * TILE, "1", [wk(1, 1), slow])
    add("16", "ellip8", 16 * TILE, "w-1", [wk(TILE), wk(TILE - 1, 1), slow])
    add("16", "ellip8", 16 * TILE, "w", [wk(2 * TILE), slow])
    add("16", "ellip8", 16 * TILE, "long", [wk(2 * TILE), slow])
    # forced short pre-roll and ragged warm_len (see _single_pass)
    add("short-8", "narrow2", 8 * TILE, "w", [SPLIT("narrow2", 8, 4, 2, 1, prex=1, pre=TILE)], warm=TILE,
        ref="segmented")
    add("short-8", "narrow2", 8 * TILE, "long", [SPLIT("narrow2", 8, 4, 2, 1, prex=1, pre=TILE)], warm=TILE,
        ref="segmented")
    add("short-8-fb1", "narrow2", 8 * TILE, "w", [SPLIT("narrow2", 8, 4, 2, 1, al16=0, prex=1, pre=TILE)],
        warm=TILE, ref="segmented", align="fb1")
    add("short-8", "narrow10", 8 * TILE, "w", [wk(TILE), SPLIT("narrow10", 8, 4, 2, 1, pre=TILE)], warm=TILE,
        ref="segmented")       # lean: the one-tile warm-up stays a launch of its own
    add("ragged-warm", "narrow2", 8 * TILE, "long", [wk(8000, 1), K(8 * TILE, 1)], warm=8000)
    return out


def _steps():
    """osz_sosfiltfilt_step: the dual launches, and the two separate passes it falls back to."""
    out = []

    def add(name, key, tx, ta, fb, expect, nch=96, extra=0, **kw):
        out.append(_case(f"step-{key}-{name}-fb{fb}", key, "step", ta * TILE, expect, nch=nch, nx=tx * TILE + extra,
                         fb=fb, **kw))

    def wk(n, guard=0):
        return K(n, 1, guard=guard, warmup=1)

    seal = SEAL(8, 4, 2)
    add("8x8", "lp4", 8, 8, "none", [DUALSEG("lp4", 8, 8, 2), seal])
    add("8x8", "lp4", 8, 8, "1", [wk(1, 1), DUALSEG("lp4", 8, 8, 2), seal])
    add("8x8", "lp4", 8, 8, "w-1", [wk(TILE - 1, 1), DUALSEG("lp4", 8, 8, 2), seal])
    add("8x8", "lp4", 8, 8, "w", [DUALSEG("lp4", 8, 8, 2, prex=1), seal])
    add("8x8", "lp4", 8, 8, "long", [DUALSEG("lp4", 8, 8, 2, prex=1), seal])
    add("8x8", "bp8", 8, 8, "w", [DUALSEG("bp8", 8, 8, 2, prex=1), seal])
    add("8x16", "lp4", 8, 16, "w", [DUALSEG("lp4", 8, 16, 2, prex=1), seal])
    add("7x7", "lp4", 7, 7, "w", [wk(TILE), DUAL(7, 7)])
    add("7x7", "lp4", 7, 7, "none", [DUAL(7, 7)])
    for key in ("bp9", "bp32"):
        add("8x8", key, 8, 8, "w", [wk(TILE), DUALSEG(key, 8, 8, 2), seal])
    add("8x8", "bp9", 8, 8, "none", [DUALSEG("bp9", 8, 8, 2), seal])
    add("16x16", "ellip8", 16, 16, "w", [wk(2 * TILE), DUAL(16, 16)])     # w = 2: no segments in a dual launch
    add("16x16-400ch", "lp4", 16, 16, "w", [DUALSEG("lp4", 16, 16, 4, prex=1), SEAL(16, 4, 4)], nch=400)
    # not fusable: fewer than 96 channels, or a ragged forward chunk
    add("8x8-95ch", "lp4", 8, 8, "w", [SPLIT("lp4", 8, 4, 2), seal, SPLIT("lp4", 8, 4, 2, 1, prex=1)], nch=95)
    add("8+1sx8", "lp4", 8, 8, "w",
        [SPLIT("lp4", 8, 4, 2), seal, K(1, 0, guard=1), SPLIT("lp4", 8, 4, 2, 1, prex=1)], extra=1)
    for align in ("x1", "y1", "fb1", "odd"):
        add(f"8x8-{align}", "lp4", 8, 8, "w", [DUALSEG("lp4", 8, 8, 2, al16=0, prex=1), seal], align=align)
    add("8x8-nonfinite", "bp9", 8, 8, "w", [wk(TILE), DUALSEG("bp9", 8, 8, 2), seal], nonfinite=True)
    add("short-8x8", "narrow2", 8, 8, "w", [DUALSEG("narrow2", 8, 8, 2, prex=1), seal], warm=TILE, ref="segmented")
    add("short-8x16", "narrow2", 8, 16, "none", [DUALSEG("narrow2", 8, 16, 2), seal], warm=TILE, ref="segmented")
    add("short-8x8", "narrow10", 8, 8, "w", [wk(TILE), DUALSEG("narrow10", 8, 8, 2), seal], warm=TILE, ref="segmented")
    add("short-8x16", "narrow10", 8, 16, "none", [DUALSEG("narrow10", 8, 16, 2), seal], warm=TILE, ref="segmented")
    add("ragged-warm-8x8", "narrow2", 8, 8, "long", [wk(8000, 1), DUAL(8, 8)], warm=8000)
    return out


CASES = tuple(_single_pass() + _warmups() + _steps())
assert len({c.name for c in CASES}) == len(CASES)


def instance(rec):
    return (rec["kernel"], rec["rev"], rec["guard"], rec["al16"])


def route(case):
    """The case's launches as one word, for the reports."""
    return "+".join(r["kernel"] + ("", "<rev>")[r["rev"] == 1] + ("", "<guard>")[r["guard"]]
                    + ("", "<unaligned>")[r["al16"] == 0] + ("", "<warmup>")[r["warmup"]]
                    + ("", "<preroll>")[r["prex"]] for r in case.expect)
