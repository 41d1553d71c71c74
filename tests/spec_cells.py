"""The kernel instances of the windowed-DFT engine (csrc/spec.hip) and what tests them.

One osz_spec_push reaches one of 150 separately compiled kernel instances, chosen by nfft, nwin,
stride, mode and detrend (``compiled_instances`` reads their number off the launch tables of
spec.hip), or the staged rocFFT route.  This module holds

* the definition they are compared with (``segment_rows`` and ``spectrum``): per segment and
  channel, in numpy.longdouble, the mean or the least-squares line taken off the nwin samples,
  times the window, zero-padded to nfft, scipy.fft.rfft of the long-double array (80-bit here:
  ``assert_80_bit``), times scale; |X|^2 doubled except at DC and (even nfft) Nyquist;
* the same pipeline in plain float64 NumPy (np.fft.rfft), whose error against the long-double
  one on the case's own input is the yardstick e64(case);
* ``row_metric``: per (segment, channel) row, max_k |X - Xref| / rms_k |Xref| for the DFT mode
  and max_k |P - Pref| / mean_k Pref for the PSD modes, the maximum over rows of which is a
  case's error;
* the planners restated: ``mix_plan``, ``mix_threads``, ``split_plan``, the Bluestein length and
  the order of choice of osz_spec_create (``route``), and ``plan_pushes``: the launch records a
  sequence of pushes must produce, as SpecStream.last_launches() reports them;
* CASES: for every compiled instance a *ragged* case (about seven segments in pushes cut at 1,
  nwin // 3, nwin - 1, nwin + 7, nwin + 2 stride (the end of a segment), 3 nwin + 11,
  3 nwin + 12, ...: a push with no segment, head
  segments out of carries of 1 and nwin - 1 samples, a head and a body launch in one push, odd
  and even segment counts) and one or two *runs* cases (enough segments x channels that the
  launch site plans R >= 2 segments or pairs per run, an odd segment count, runs of unequal
  length; for the mixed-radix and split kernels one with the half-carry of the trend sums and
  one without), plus per family zero padding, nwin = 1 and 2, every first- and later-pass radix,
  prime / even / odd R0 of the split kernel and the staged route;
* UNREACHED: compiled instances no handle reaches (none today: spec8_kernel<4096, ..., HALF> needs
  OSZ_SPEC_V8=2 beside the cube, and its cases set it);
* ``bound``: 16 e64(case), and FAMILY_BOUND for a family that misses it on all instances alike.

Inputs.  N(0, 1) + 0.5 + a ramp rising by 2 per window, every push a column slice of a wider
tensor.  Noise alone cannot meet the conditions the corpus asks of its inputs in EVERY row (the
DC, Nyquist and first bins each hold at least 1 % of the row's mean power, so that a wrong
factor 2 at an undoubled bin shows): a real bin of white noise falls below 1 % of the mean in
one row of nine, and a runs case has thousands of rows.  So a deterministic pedestal is added,
the same in every channel: an alternation a_N (-1)^n and two stride-periodic sign patterns
a_0 p_0[n mod stride] + a_1 p_1[n mod stride], chosen against the detrended window so that every
segment sees them add up coherently at the Nyquist bin, at DC and at bin 1; each amplitude is
5.5 standard deviations of what the noise puts into that bin, 2 at the most (``pedestal``),
times 1, 1.125, ... 1.5 by channel (``pedestal_gain``).
The window is 0.2 + U(0, 1) times a half-cosine rise: asymmetric, strictly positive.  scale = 0.7.

Every row of every case is checked against the long-double reference, except in the runs cases of
SUBSET_TAGS (more than LD_POINTS = 24 million points: the long transforms): those check the
channels of ``subset`` -- the first, the last and every 16th, with all their segments -- against
the long-double reference and the others against the float64 pipeline at the bound plus e64.

Shared by tests/test_spec_cells_host.py (no GPU) and tests/test_gpu_spec_cells.py.
"""

import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_HIP = os.path.join(ROOT, "openseize_amd", "csrc", "spec.hip")
LD = np.longdouble
SCALE = 0.7
MEAN, PSD, DFT = 0, 1, 2                     # osz_spec_mode
MODES = (MEAN, PSD, DFT)
FAMILIES = ("cube", "fft8", "mix", "split", "blue", "staged")
FIELDS = ("family", "size", "mode", "linear", "half", "nseg", "R", "nruns", "head", "npass", "R0", "S0", "radix")

# constants of specmix.h, specsplit.h and spec.hip (test_spec_cells_host reads them off the source)
K_MAX_PASS, K_MAX_M, K_MAX_SPLIT_LOCAL, K_MAX_SPLIT_R0 = 14, 10208, 10176, 32
RUN_DIV = {"cube": 512, "fft8": 2048, "blue": 2048, "mix": 2048, "split": 2048}
RUN_CAP = {"cube": 32, "fft8": 64, "blue": 64, "mix": 64, "split": 64}
STAGED_ELEMS = 1 << 27


def assert_80_bit():
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 80-bit format here"


# ------------------------------------------------------------------ the planners, restated
def mix_plan(nfft):
    """specmix_plan: the radix plan of the nfft / 2 point transform, or None."""
    if nfft < 4 or nfft & 1:
        return None
    m, radix = nfft // 2, []
    if m > K_MAX_M:
        return None
    for r in (10, 4, 2, 3, 5, 7):
        while m % r == 0 and len(radix) < K_MAX_PASS:
            radix.append(r)
            m //= r
    return tuple(radix) if m == 1 and radix else None


def mix_threads(M):
    return 64 if M <= 640 else 128 if M <= 1280 else 256 if M <= 2560 else 512 if M <= 5120 else 1024


def split_plan(nfft):
    """specsplit_plan: (R0, radix) with radix[0] = R0 and the plan of S0 behind it, or None."""
    if nfft < 4 or nfft & 1:
        return None
    M = nfft // 2
    if M <= K_MAX_M:
        return None
    for R in range(2, K_MAX_SPLIT_R0 + 1):
        if M % R:
            continue
        S0 = M // R
        if 2 * S0 > K_MAX_SPLIT_LOCAL or 2 * S0 <= 1280:
            continue
        rad = mix_plan(2 * S0)
        if rad is None or len(rad) + 1 > K_MAX_PASS:
            continue
        return R, (R,) + rad
    return None


def blue_m(nfft):
    m = 512
    while m < 2 * nfft - 1:
        m <<= 1
    return m


Route = namedtuple("Route", "family size half radix R0 S0")


def route(nwin, nfft, stride, env=None):
    """The order of choice of osz_spec_create -> Route.  env: OSZ_SPEC_FUSED / _V8 / _MIX."""
    env = env or {}
    fused = nwin == 4096 and nfft == 4096 and int(env.get("OSZ_SPEC_FUSED", 1)) != 0
    v8 = int(env.get("OSZ_SPEC_V8", 1))
    pow2 = 512 <= nfft <= 8192 and nfft & (nfft - 1) == 0
    fused8 = pow2 and v8 != 0 and (not fused or v8 == 2)
    if fused8:
        return Route("fft8", nfft, int(nwin == nfft and 2 * stride == nfft), (), 0, 0)
    if fused:
        return Route("cube", 4096, int(stride == 2048), (), 0, 0)
    mix_on = int(env.get("OSZ_SPEC_MIX", 1)) != 0
    if mix_on:
        rad = mix_plan(nfft)
        if rad:
            return Route("mix", mix_threads(nfft // 2), int(2 * stride == nwin and nwin == nfft and rad[0] % 2 == 0),
                         rad, 0, 0)
        sp = split_plan(nfft)
        if sp:
            R0, rad = sp
            S0 = nfft // 2 // R0
            return Route("split", mix_threads(2 * S0),
                         int(2 * stride == nwin and nwin == nfft and (nfft // 2) % 2 == 0), rad, R0, S0)
        if 2 <= nfft <= 4096:
            return Route("blue", blue_m(nfft), -1, (), 0, 0)
    return Route("staged", nfft, -1, (), 0, 0)


def _record(rt, mode, linear, nseg, R, nruns, head):
    return dict(family=rt.family, size=rt.size, mode=mode, linear=linear, half=rt.half, nseg=nseg, R=R, nruns=nruns,
                head=head, npass=len(rt.radix), R0=rt.R0, S0=rt.S0, radix=tuple(rt.radix))


def _run(rt, nseg, nch):
    """(R, nruns) of one launch over nseg segments, as its launch site plans them."""
    fam = rt.family
    items = nseg if fam in ("mix", "split") else (nseg + 1) // 2
    work = items * nch * ((rt.R0 + 1) // 2 if fam == "split" else 1)
    R = max(1, min(RUN_CAP[fam], work // RUN_DIV[fam]))
    return R, -(-items // R)


def plan_pushes(case):
    """Per push of case.pushes: (segments it emits, the launch records it must produce)."""
    rt = route(case.nwin, case.nfft, case.stride, dict(case.env))
    out, ncarry = [], 0
    for n in case.pushes:
        total = ncarry + n
        nseg = (total - case.nwin) // case.stride + 1 if total >= case.nwin else 0
        recs = []
        if nseg > 0 and rt.family == "cube":
            recs.append(_record(rt, case.mode, case.linear, nseg, *_run(rt, nseg, case.nch), -1))
        elif nseg > 0 and rt.family == "staged":
            per = max(1, STAGED_ELEMS // (case.nch * case.nfft))
            per = min(per, nseg, 65535)
            for s0 in range(0, nseg, per):
                recs.append(_record(rt, case.mode, case.linear, min(per, nseg - s0), per, 1, -1))
        elif nseg > 0:
            nhead = min(nseg, -(-ncarry // case.stride)) if ncarry > 0 else 0
            if nhead:
                recs.append(_record(rt, case.mode, case.linear, nhead, *_run(rt, nhead, case.nch), 1))
            if nseg > nhead:
                recs.append(_record(rt, case.mode, case.linear, nseg - nhead, *_run(rt, nseg - nhead, case.nch), 0))
        out.append((nseg, recs))
        ncarry = total - nseg * case.stride
    return out


def instance_of(rec):
    """(family, size, mode, linear, half) as the launch tables index it (half -1: no such index;
    the half-carry of mix and split is an argument, not an instance)."""
    half = rec["half"] if rec["family"] in ("cube", "fft8") else -1
    return (rec["family"], rec["size"], rec["mode"], rec["linear"], half)


def compiled_instances(text=None):
    """The full product of the launch tables of spec.hip, from their dimensions and the sizes
    their switch statements name, read as text."""
    text = text if text is not None else open(SPEC_HIP).read()

    def dims(pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return tuple(int(d) for d in re.findall(r"\[(\d+)\]", m.group(1)))

    def sizes(pattern):
        got = sorted({int(s) for s in re.findall(pattern, text)})
        assert got, pattern
        return got

    out = set()

    def add(family, size_list, dm, kernel):
        assert len(dm) in (2, 3), (family, dm)
        for size in size_list:
            for mode in range(dm[0]):
                for lin in range(dm[1]):
                    for half in (range(dm[2]) if len(dm) == 3 else (-1,)):
                        out.add((family, size, mode, lin, half))
        # every cell of the table names the kernel once, and nothing else instantiates it
        assert text.count(kernel) == int(np.prod(dm)), (kernel, text.count(kernel), dm)

    add("cube", [4096], dims(r"static const kern_t ck((?:\[\d+\])+) = \{\s*\{\{spec_cube_kernel"), "spec_cube_kernel<")
    add("fft8", sizes(r"rc = spec8_launch<(\d+)>"),
        dims(r"static const kern_t ks((?:\[\d+\])+) = \{\s*\{\{spec8_kernel"), "spec8_kernel<N, ")
    add("mix", sizes(r"rc = specmix_launch_nt<(\d+)>"),
        dims(r"static const kern_t ks((?:\[\d+\])+) = \{\s*\{mix::specmix_kernel"), "mix::specmix_kernel<")
    add("split", sizes(r"rc = specsplit_launch_nt<(\d+)>"),
        dims(r"static const kern_t ks((?:\[\d+\])+) = \{\s*\{mix::specsplit_kernel"), "mix::specsplit_kernel<")
    add("blue", sizes(r"rc = blue_launch<(\d+)>"),
        dims(r"static const kern_t ks((?:\[\d+\])+) = \{\{spec_blue_kernel"), "spec_blue_kernel<N, ")
    return frozenset(out)


# ------------------------------------------------------------------ cases
# kind: ragged | runs | extra.  pushes: samples per push.  env: the OSZ_SPEC_* switches set while
# the handle is created.  want: the instance the case is there for, (family, size, mode, linear,
# half), half -1 where the table has no such index; halfcarry: what mix and split must report.
# zero: the reference is identically zero (nwin = 1, constant detrend) and so must the output be.
Case = namedtuple("Case", "name kind nwin nfft stride mode linear nch pushes env want halfcarry seed zero")

# seeds of the cases whose default seed (0) misses the input conditions (test_spec_cells_host)
SEEDS = {
    **{f"blue-1024-n257-m{m}-lin-ragged": 2 for m in MODES},
    "fft8-pad333of512-m0-lin-extra": 8, "fft8-pad333of512-m2-lin-extra": 8,
    "mix-pad333of648-m0-lin-extra": 1, "mix-pad333of648-m2-lin-extra": 1,
    "blue-pad201of347-m0-lin-extra": 13, "blue-pad201of347-m2-lin-extra": 13,
    **{f"mix-radix-n4-m{m}-const-extra": 31 for m in MODES},
    **{f"mix-radix-n6-m{m}-const-extra": 3 for m in MODES},
}


def _cuts(nwin, stride, nseg):
    """Push lengths of a ragged case with nseg segments in all."""
    end = nwin + (nseg - 1) * stride + min(stride - 1, 5)
    cuts = sorted({c for c in (1, nwin // 3, nwin - 1, nwin + 7, nwin + 2 * stride, 3 * nwin + 11, 3 * nwin + 12)
                   if 0 < c < end})
    cuts.append(end)
    return tuple(b - a for a, b in zip([0] + cuts[:-1], cuts))


def _odd_stride(nwin):
    return max(1, (3 * nwin // 5) | 1) if nwin > 2 else 1


def _mk(name, kind, nwin, nfft, stride, mode, linear, nch, pushes, env=(), zero=False):
    rt = route(nwin, nfft, stride, dict(env))
    want = (rt.family, rt.size, mode, linear, rt.half if rt.family in ("cube", "fft8") else -1)
    return Case(name, kind, nwin, nfft, stride, mode, linear, nch, tuple(pushes), tuple(env), want,
                rt.half if rt.family in ("mix", "split") else -1, SEEDS.get(name, 0), zero)


def _runs_shape(family, NW=1, halfcarry=1):
    """(nseg, nch) of a runs case: the fewest rows with R = 2 (pairs: 9 segments, 5 pairs, three
    runs of 1, 2 and 2 pairs, the last pair half empty; mix and split without the half-carry: 5
    segments, runs of 1, 2 and 2) or R = 3 (mix and split with the half-carry: 7 segments, runs of
    2, 2 and 3, so that one segment takes its sums from a segment that took them itself)."""
    if family in ("mix", "split"):
        return (7, -(-3 * RUN_DIV[family] // (7 * NW))) if halfcarry else (5, -(-2 * RUN_DIV[family] // (5 * NW)))
    return 9, -(-2 * RUN_DIV[family] // 5)


def _smallest(pred, lo, hi, step=1):
    for n in range(lo, hi, step):
        if pred(n):
            return n
    raise AssertionError("no length")


def _instance_cases():
    out = []

    def both(tag, nwin, nfft, stride, env=(), runs_stride=None):
        fam = route(nwin, nfft, stride, dict(env))
        for mode in MODES:
            for lin in (0, 1):
                nm = f"{tag}-m{mode}-{'lin' if lin else 'const'}"
                out.append(_mk(nm + "-ragged", "ragged", nwin, nfft, stride, mode, lin, 3, _cuts(nwin, stride, 7), env))
                rs = stride if runs_stride is None else runs_stride
                NW = (fam.R0 + 1) // 2 if fam.family == "split" else 1
                nseg, nch = _runs_shape(fam.family, NW, route(nwin, nfft, rs, dict(env)).half)
                out.append(_mk(nm + "-runs", "runs", nwin, nfft, rs, mode, lin, nch,
                               (nwin + (nseg - 1) * rs + 3,), env))

    # cube: nwin = nfft = 4096; HALF is stride == 2048
    both("cube-half", 4096, 4096, 2048)
    both("cube-any", 4096, 4096, _odd_stride(4096), runs_stride=257)
    # fft8: HALF is nwin == N and 2 stride == N; N = 4096 with nwin == N is the cube's unless OSZ_SPEC_V8=2
    for N in (512, 1024, 2048, 4096, 8192):
        env = (("OSZ_SPEC_V8", "2"),) if N == 4096 else ()
        both(f"fft8-{N}-half", N, N, N // 2, env)
        both(f"fft8-{N}-any", N, N, _odd_stride(N), env, runs_stride=129)
    # mix: the smallest nfft of each workgroup size (NT = 64: from M = 320, half its reach), with an odd stride; the
    # runs case at 50 % overlap, where M even means the half-carry, and a second runs case at the
    # smallest nfft with the other parity of M
    lows = {64: 320, 128: 641, 256: 1281, 512: 2561, 1024: 5121}
    for NT, lo in lows.items():
        def ok(M, parity=None):
            r = route(2 * M, 2 * M, M, {})
            return r.family == "mix" and r.size == NT and (parity is None or M % 2 == parity)
        M = _smallest(ok, lo, K_MAX_M + 1)
        both(f"mix-{NT}-n{2 * M}", 2 * M, 2 * M, _odd_stride(2 * M), runs_stride=M)
        M2 = _smallest(lambda m: ok(m, 1 - M % 2), lo, K_MAX_M + 1)
        for mode in MODES:
            for lin in (0, 1):
                nseg, nch = _runs_shape("mix", 1, 1 - M2 % 2)
                out.append(_mk(f"mix-{NT}-n{2 * M2}-m{mode}-{'lin' if lin else 'const'}-runs", "runs", 2 * M2, 2 * M2,
                               M2, mode, lin, nch, (2 * M2 + (nseg - 1) * M2 + 3,)))
    # split: the same per workgroup size of the 2 S0 local points
    for NT in (256, 512, 1024):
        def oks(M, parity=None):
            r = route(2 * M, 2 * M, M, {})
            return r.family == "split" and r.size == NT and (parity is None or M % 2 == parity)
        M = _smallest(oks, K_MAX_M + 1, 40 * K_MAX_M)
        both(f"split-{NT}-n{2 * M}", 2 * M, 2 * M, _odd_stride(2 * M), runs_stride=M)
        M2 = _smallest(lambda m: oks(m, 1 - M % 2), K_MAX_M + 1, 40 * K_MAX_M)
        r2 = route(2 * M2, 2 * M2, M2, {})
        for mode in MODES:
            for lin in (0, 1):
                nseg, nch = _runs_shape("split", (r2.R0 + 1) // 2, r2.half)
                out.append(_mk(f"split-{NT}-n{2 * M2}-m{mode}-{'lin' if lin else 'const'}-runs", "runs", 2 * M2, 2 * M2,
                               M2, mode, lin, nch, (2 * M2 + (nseg - 1) * M2 + 3,)))
    # blue: the smallest nfft of each convolution length (512: from 193, three quarters of its reach;
    # shorter ones would need a pedestal above 2 to meet the input conditions in thousands of rows)
    for m, lo in ((512, 193), (1024, 257), (2048, 513), (4096, 1025), (8192, 2049)):
        n = _smallest(lambda q: route(q, q, 1, {}) == Route("blue", m, -1, (), 0, 0), lo, 4097)
        both(f"blue-{m}-n{n}", n, n, _odd_stride(n), runs_stride=65)
    return out


def _extra_cases():
    out = []

    def add(tag, nwin, nfft, stride, combos=None, env=(), zero=False, nseg=7):
        for mode, lin in (combos or [(m, l) for m in MODES for l in (0, 1)]):
            out.append(_mk(f"{tag}-m{mode}-{'lin' if lin else 'const'}-extra", "extra", nwin, nfft, stride, mode, lin, 3,
                           _cuts(nwin, stride, nseg), env, zero))

    some = [(MEAN, 1), (PSD, 0), (DFT, 1)]
    const = [(MEAN, 0), (PSD, 0), (DFT, 0)]
    # zero padding (nwin < nfft, nwin odd), nwin = 2 and nwin = 1 (constant detrend: all zeros)
    pads = {"cube": None, "fft8": (333, 512), "mix": (333, 648), "split": (4099, 20580), "blue": (201, 347),
            "staged": (333, 4099)}
    for fam, p in pads.items():
        if p is None:
            continue        # the cube has nwin == nfft == 4096 only
        nwin, nfft = p
        assert route(nwin, nfft, 1).family == fam, (fam, p)
        add(f"{fam}-pad{nwin}of{nfft}", nwin, nfft, _odd_stride(nwin), some)
        add(f"{fam}-nwin2of{nfft}", 2, nfft, 1, const, nseg=5)
        add(f"{fam}-nwin1of{nfft}", 1, nfft, 1, const, zero=True, nseg=5)
    # mixed radix: each first-pass radix (10, 4, 5, 2, 3, 7) at the smallest nfft that has it, and
    # each later-pass radix behind a first one
    for nfft in (20, 8, 10, 4, 6, 14,                # first pass alone: 10, 4, 5, 2, 3, 7
                 200, 80, 40, 60, 100, 140,          # behind a 10: 10, 4, 2, 3, 5, 7
                 24, 36, 50, 98, 42, 1260):          # 4 2 3; 2 3 3; 5 5; 7 7; 3 7; 10 3 3 7
        assert route(nfft, nfft, 1).family == "mix"
        # (below 64 points with the constant trend only: a fitted line leaves a window this short
        # too little for the input conditions)
        add(f"mix-radix-n{nfft}", nfft, nfft, _odd_stride(nfft), some if nfft >= 64 else const)
    # split: a prime R0 (the self-paired workgroup of an odd R0) and an even R0
    # (24010: R0 = 5; 21952: R0 = 4; 30618: R0 = 7; the instance cases have R0 = 3, 4 and 11)
    for nfft in (24010, 21952, 30618):
        assert route(nfft, nfft, 1).family == "split", nfft
        add(f"split-r0-n{nfft}", nfft, nfft, _odd_stride(nfft), some, nseg=3)
    # staged: a prime nfft above the chirp transform's reach; and what test_spectra_fused_4096
    # compares the cube with
    add("staged-n4099", 4099, 4099, _odd_stride(4099), nseg=4)
    add("staged-n4096-env", 4096, 4096, 2048, some, nseg=4,
        env=(("OSZ_SPEC_FUSED", "0"), ("OSZ_SPEC_V8", "0"), ("OSZ_SPEC_MIX", "0")))
    # R >= 2 on a HEAD launch (the head buffer, its own pitch): a small stride, a first push that only
    # fills the carry with nwin - 1 samples, then four or eight head segments and three in the chunk
    for tag, nwin, stride, nch in (("fft8-512", 512, 64, 1024), ("mix-64-n640", 640, 160, 1024), ("blue-512-n193", 193, 24, 1024)):
        nhead = -(-(nwin - 1) // stride)
        for mode, lin in ((DFT, 1), (MEAN, 0)):
            out.append(_mk(f"{tag}-headruns-m{mode}-{'lin' if lin else 'const'}-extra", "extra", nwin, nwin, stride, mode,
                           lin, nch, (nwin - 1, (nhead + 2) * stride + 4)))
    add("blue-n2", 2, 2, 1, const, nseg=5)
    add("blue-n3", 3, 3, 2, some, nseg=5)
    return out


CASES = tuple(_instance_cases() + _extra_cases())
assert len({c.name for c in CASES}) == len(CASES)

# compiled instances no handle reaches: (instance, why, the line of spec.hip that makes it so)
UNREACHED = ()


def group(case):
    """What test_gpu_spec_cells parametrises by: family and size."""
    return f"{case.want[0]}-{case.want[1]}"


GROUPS = tuple(sorted({group(c) for c in CASES}, key=lambda g: (FAMILIES.index(g.split("-")[0]), int(g.split("-")[1]))))


# ------------------------------------------------------------------ inputs
def window(case):
    rng = np.random.default_rng(7000 + case.nwin)
    rise = 0.5 * (1.0 - np.cos(np.pi * (np.arange(case.nwin) + 0.5) / case.nwin))
    return (0.2 + rng.random(case.nwin)) * (0.05 + 0.95 * rise)


def _perp(g, linear):
    """g minus its mean (and its least-squares line): detrending is a symmetric projection, so
    sum (d - trend(d)) g = sum d perp(g)."""
    g = g - g.mean()
    if linear and len(g) > 1:
        t = np.arange(len(g)) - 0.5 * (len(g) - 1)
        g = g - t * (t @ g) / (t @ t)
    return g


def pedestal(case):
    """The deterministic part of a case's input over n samples -> function n -> array."""
    w, nwin, S = window(case), case.nwin, case.stride
    m = np.arange(nwin)
    parts = []
    for basis in (np.ones(nwin), np.cos(2 * np.pi * m / case.nfft)):
        g = _perp(w * basis, case.linear)
        V = np.zeros(S)
        np.add.at(V, m % S, g)
        gain, noise = np.abs(V).sum(), np.sqrt(g @ g)
        amp = min(5.5 * noise / gain, 2.0) if gain > 0 else 0.0
        parts.append(amp * np.where(V >= 0, 1.0, -1.0))
    gN = _perp(w * (-1.0) ** m, case.linear)
    gainN, noiseN = abs(gN @ (-1.0) ** m), np.sqrt(gN @ gN)
    pat = parts[0] + parts[1]
    # (what the two patterns themselves put into the Nyquist bin, with either sign -- an odd stride
    # flips the alternation from segment to segment --, comes on top)
    cross = abs(pat[m % S] @ gN)
    aN = min((5.5 * noiseN + cross) / gainN, 2.0) if gainN > 0 else 0.0

    def make(n):
        idx = np.arange(n)
        return pat[idx % S] + aN * (1.0 - 2.0 * (idx & 1))
    return make


def signal(case):
    """(nch, n) float64: N(0, 1) + 0.5 + a ramp rising by 2 per window + the pedestal times the
    channel's gain."""
    n = sum(case.pushes)
    rng = np.random.default_rng(9000 + 131 * case.seed + len(case.name))
    x = rng.standard_normal((case.nch, n))
    x += 0.5 + 2.0 * np.arange(n) / case.nwin
    x += pedestal_gain(case.nch)[:, None] * pedestal(case)(n)
    return x


def pedestal_gain(nch):
    """The pedestal's amplitude in channel c, 1 to 1.5 times: channels differ in more than their noise."""
    return 1.0 + 0.125 * (np.arange(nch) % 5)


def total_segments(case):
    n = sum(case.pushes)
    return (n - case.nwin) // case.stride + 1 if n >= case.nwin else 0


# A runs case is checked against the long-double reference in EVERY row where that reference costs
# a few seconds at the most: up to LD_POINTS = rows x nfft (24 million: about 3.5 s).  Above, the
# channels of ``subset`` against long double and the others against the float64 pipeline at the
# bound plus e64.  SUBSET_TAGS: the instance tags (name up to the mode) of the cases that do so.
LD_POINTS = 24_000_000
SUBSET_TAGS = ("fft8-4096-any", "fft8-4096-half", "fft8-8192-any", "fft8-8192-half", "mix-512-n5184",
               "mix-1024-n10290", "mix-1024-n10368", "split-512-n20480", "split-512-n24010", "split-1024-n20580",
               "split-1024-n21870")


def uses_subset(case):
    return case.kind == "runs" and total_segments(case) * case.nch * case.nfft > LD_POINTS


def tag(case):
    return re.sub(r"-m\d-(lin|const)-\w+$", "", case.name)


def subset(nch):
    """The channels a runs case checks against the long-double reference: the first, the last
    and every 16th."""
    return sorted(set(range(0, nch, 16)) | {nch - 1})


# ------------------------------------------------------------------ the reference
def segment_rows(x, case, dtype):
    """(nseg, nch, nwin) of dtype: the segments of x (nch, n)."""
    v = np.lib.stride_tricks.sliding_window_view(x, case.nwin, axis=-1)[:, ::case.stride]
    return np.ascontiguousarray(np.moveaxis(v, 0, 1)[:total_segments(case)], dtype=dtype)


def _detrended(seg, w, linear, dtype):
    nwin = seg.shape[-1]        # (seg is this function's to overwrite: segment_rows copies)
    seg -= seg.mean(axis=-1, keepdims=True)
    if linear and nwin > 1:
        t = np.arange(nwin, dtype=dtype) - dtype(nwin - 1) / dtype(2)
        slope = (seg @ t)[..., None] / (t @ t)
        for c in range(seg.shape[1]):          # channel by channel: no second array of the whole size
            seg[:, c] -= slope[:, c] * t
    seg *= w.astype(dtype)
    return seg


def spectrum(x, case, dtype=LD, linear=None):
    """(nseg, nch, nfreq) complex: the scaled DFT of every detrended, windowed, padded segment, in
    long double through scipy.fft.rfft or in float64 through np.fft.rfft."""
    linear = case.linear if linear is None else linear
    rows = _detrended(segment_rows(x, case, dtype), window(case), linear, dtype)
    if dtype is LD:
        import scipy.fft
        assert_80_bit()
        pad = np.zeros(rows.shape[:-1] + (case.nfft,), LD)
        pad[..., :case.nwin] = rows
        X = scipy.fft.rfft(pad, axis=-1)
        assert X.dtype == np.complex256, X.dtype
        return X * LD(SCALE)
    X = np.fft.rfft(rows, n=case.nfft, axis=-1)
    assert X.dtype == np.complex128
    return X * SCALE


def power(X, nfft):
    P = X.real * X.real + X.imag * X.imag
    P[..., 1:] *= 2
    if nfft % 2 == 0:
        P[..., -1] /= 2
    return P


def estimate(X, case):
    """What the handle's mode makes of the segment spectra: DFT (nseg, nch, nfreq) complex, PSD
    the same real, MEAN (nch, nfreq)."""
    if case.mode == DFT:
        return X
    P = power(X, case.nfft)
    return P if case.mode == PSD else P.mean(axis=0)


def row_metric(got, ref, mode):
    """Per row (every axis but the last): max_k |got - ref| over rms_k |ref| (DFT) or mean_k ref
    (PSD modes), in the reference's precision.  A row whose reference is zero: 0 when got is too, inf otherwise."""
    d = np.abs(got.astype(ref.dtype) - ref).max(axis=-1)
    if mode == DFT:
        den = np.sqrt((ref.real * ref.real + ref.imag * ref.imag).mean(axis=-1))
    else:
        den = ref.mean(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, d / den, np.where(d > 0, np.inf, 0.0)).astype(np.float64)


Ref = namedtuple("Ref", "exact chans approx e64 nseg")


def reference(case, x=None, X64=None):
    """The case's reference: ``exact`` the long-double estimate of the channels ``chans`` (all of
    them but in a case of SUBSET_TAGS: ``subset``), ``approx`` the float64 pipeline's estimate of every
    channel (X64: its segment spectra, when the caller has them), e64 the worst row of approx
    against exact."""
    x = signal(case) if x is None else x
    chans = subset(case.nch) if uses_subset(case) else list(range(case.nch))
    exact = estimate(spectrum(x[chans], case, LD), case)
    approx = estimate(spectrum(x, case, np.float64) if X64 is None else X64, case)
    pick = approx[chans] if case.mode == MEAN else approx[:, chans]
    e64 = float(row_metric(pick, exact, case.mode).max())
    return Ref(exact, chans, approx, e64, total_segments(case))


# Measured: e64 of every case (over a family's cases: cube 1.4e-14 ... 1.4e-12, fft8 4.9e-16 ... 2.7e-12,
# mix 2.5e-16 ... 2.9e-12, split 7.4e-16 ... 8.8e-12, blue 4.1e-16 ... 4.9e-13, staged 2.0e-15 ... 4.6e-13),
# and below on an MI355X the worst error / (16 e64) of a family's cases.
# e64 is what float64 costs the whole pipeline, not the transform alone (that
# is 1 to 2e-15 of a row's rms): the mean of nwin samples around 0.5 + the ramp carries a rounding
# of about 1e-16 times that mean into every sample, the window adds those up coherently at DC and
# Nyquist (~ nwin / 3 of them), and in the PSD modes the error of a bin is twice its amplitude
# times that -- the ramp alone puts 0.05 nwin times the mean power into DC under the constant
# trend.  Hence the largest e64 at the longest transforms in PSD mode with the constant trend.
# test_gpu_spec_cells prints every ratio.
# name -> e64 measured (0: a case whose reference is zero); test_spec_cells_host asks a re-measured e64
# to lie within a factor 2 of it
E64 = {
    "cube-half-m0-const-ragged": 8.11e-14, "cube-half-m0-const-runs": 3.3e-13, "cube-half-m0-lin-ragged": 2.1e-14,
    "cube-half-m0-lin-runs": 7.18e-14, "cube-half-m1-const-ragged": 3.88e-13, "cube-half-m1-const-runs": 1.43e-12,
    "cube-half-m1-lin-ragged": 1.18e-13, "cube-half-m1-lin-runs": 3.02e-13, "cube-half-m2-const-ragged": 2.07e-14,
    "cube-half-m2-const-runs": 7.76e-14, "cube-half-m2-lin-ragged": 3.66e-14, "cube-half-m2-lin-runs": 1.01e-13,
    "cube-any-m0-const-ragged": 6.73e-14, "cube-any-m0-const-runs": 6.35e-14, "cube-any-m0-lin-ragged": 3.32e-14,
    "cube-any-m0-lin-runs": 1.83e-14, "cube-any-m1-const-ragged": 5.31e-13, "cube-any-m1-const-runs": 1.81e-13,
    "cube-any-m1-lin-ragged": 8.07e-14, "cube-any-m1-lin-runs": 7.78e-14, "cube-any-m2-const-ragged": 2.9e-14,
    "cube-any-m2-const-runs": 1.42e-14, "cube-any-m2-lin-ragged": 2.83e-14, "cube-any-m2-lin-runs": 2e-14,
    "fft8-512-half-m0-const-ragged": 1.52e-14, "fft8-512-half-m0-const-runs": 3.55e-14,
    "fft8-512-half-m0-lin-ragged": 5.91e-15, "fft8-512-half-m0-lin-runs": 1.59e-14,
    "fft8-512-half-m1-const-ragged": 4.57e-14, "fft8-512-half-m1-const-runs": 1.45e-13,
    "fft8-512-half-m1-lin-ragged": 2.29e-14, "fft8-512-half-m1-lin-runs": 5.1e-14,
    "fft8-512-half-m2-const-ragged": 6.64e-15, "fft8-512-half-m2-const-runs": 2.02e-14,
    "fft8-512-half-m2-lin-ragged": 9.1e-15, "fft8-512-half-m2-lin-runs": 2.94e-14,
    "fft8-512-any-m0-const-ragged": 1.16e-14, "fft8-512-any-m0-const-runs": 1.21e-14,
    "fft8-512-any-m0-lin-ragged": 3.68e-15, "fft8-512-any-m0-lin-runs": 4.29e-15,
    "fft8-512-any-m1-const-ragged": 4.26e-14, "fft8-512-any-m1-const-runs": 4.83e-14,
    "fft8-512-any-m1-lin-ragged": 1.74e-14, "fft8-512-any-m1-lin-runs": 1.93e-14,
    "fft8-512-any-m2-const-ragged": 6.48e-15, "fft8-512-any-m2-const-runs": 8.98e-15,
    "fft8-512-any-m2-lin-ragged": 1.07e-14, "fft8-512-any-m2-lin-runs": 1.22e-14,
    "fft8-1024-half-m0-const-ragged": 4.66e-14, "fft8-1024-half-m0-const-runs": 8.13e-14,
    "fft8-1024-half-m0-lin-ragged": 1.33e-14, "fft8-1024-half-m0-lin-runs": 3e-14,
    "fft8-1024-half-m1-const-ragged": 1.15e-13, "fft8-1024-half-m1-const-runs": 3.11e-13,
    "fft8-1024-half-m1-lin-ragged": 3.76e-14, "fft8-1024-half-m1-lin-runs": 1.12e-13,
    "fft8-1024-half-m2-const-ragged": 1.17e-14, "fft8-1024-half-m2-const-runs": 3.13e-14,
    "fft8-1024-half-m2-lin-ragged": 1.18e-14, "fft8-1024-half-m2-lin-runs": 5.03e-14,
    "fft8-1024-any-m0-const-ragged": 3.48e-14, "fft8-1024-any-m0-const-runs": 1.75e-14,
    "fft8-1024-any-m0-lin-ragged": 9.42e-15, "fft8-1024-any-m0-lin-runs": 8.32e-15,
    "fft8-1024-any-m1-const-ragged": 2.29e-13, "fft8-1024-any-m1-const-runs": 4.12e-14,
    "fft8-1024-any-m1-lin-ragged": 4.91e-14, "fft8-1024-any-m1-lin-runs": 2.18e-14,
    "fft8-1024-any-m2-const-ragged": 2.37e-14, "fft8-1024-any-m2-const-runs": 6.92e-15,
    "fft8-1024-any-m2-lin-ragged": 2.82e-14, "fft8-1024-any-m2-lin-runs": 9.48e-15,
    "fft8-2048-half-m0-const-ragged": 1.23e-13, "fft8-2048-half-m0-const-runs": 1.83e-13,
    "fft8-2048-half-m0-lin-ragged": 3.07e-14, "fft8-2048-half-m0-lin-runs": 5.57e-14,
    "fft8-2048-half-m1-const-ragged": 2.57e-13, "fft8-2048-half-m1-const-runs": 7.73e-13,
    "fft8-2048-half-m1-lin-ragged": 1.03e-13, "fft8-2048-half-m1-lin-runs": 2.11e-13,
    "fft8-2048-half-m2-const-ragged": 1.87e-14, "fft8-2048-half-m2-const-runs": 5.78e-14,
    "fft8-2048-half-m2-lin-ragged": 3.27e-14, "fft8-2048-half-m2-lin-runs": 7.61e-14,
    "fft8-2048-any-m0-const-ragged": 1.11e-13, "fft8-2048-any-m0-const-runs": 2.25e-14,
    "fft8-2048-any-m0-lin-ragged": 1.81e-14, "fft8-2048-any-m0-lin-runs": 1.59e-14,
    "fft8-2048-any-m1-const-ragged": 4.74e-13, "fft8-2048-any-m1-const-runs": 7.06e-14,
    "fft8-2048-any-m1-lin-ragged": 8.54e-14, "fft8-2048-any-m1-lin-runs": 4.31e-14,
    "fft8-2048-any-m2-const-ragged": 3.66e-14, "fft8-2048-any-m2-const-runs": 9.61e-15,
    "fft8-2048-any-m2-lin-ragged": 2.02e-14, "fft8-2048-any-m2-lin-runs": 1.24e-14,
    "fft8-4096-half-m0-const-ragged": 1.17e-13, "fft8-4096-half-m0-const-runs": 3.02e-13,
    "fft8-4096-half-m0-lin-ragged": 6.34e-14, "fft8-4096-half-m0-lin-runs": 7.52e-14,
    "fft8-4096-half-m1-const-ragged": 5.63e-13, "fft8-4096-half-m1-const-runs": 1.14e-12,
    "fft8-4096-half-m1-lin-ragged": 1.62e-13, "fft8-4096-half-m1-lin-runs": 3.07e-13,
    "fft8-4096-half-m2-const-ragged": 2.86e-14, "fft8-4096-half-m2-const-runs": 6.3e-14,
    "fft8-4096-half-m2-lin-ragged": 3.6e-14, "fft8-4096-half-m2-lin-runs": 8.64e-14,
    "fft8-4096-any-m0-const-ragged": 7.4e-14, "fft8-4096-any-m0-const-runs": 5.35e-14,
    "fft8-4096-any-m0-lin-ragged": 1.96e-14, "fft8-4096-any-m0-lin-runs": 3.37e-14,
    "fft8-4096-any-m1-const-ragged": 7.43e-13, "fft8-4096-any-m1-const-runs": 8.46e-14,
    "fft8-4096-any-m1-lin-ragged": 1.48e-13, "fft8-4096-any-m1-lin-runs": 5.19e-14,
    "fft8-4096-any-m2-const-ragged": 3.98e-14, "fft8-4096-any-m2-const-runs": 8.33e-15,
    "fft8-4096-any-m2-lin-ragged": 6.12e-14, "fft8-4096-any-m2-lin-runs": 1.13e-14,
    "fft8-8192-half-m0-const-ragged": 5.7e-13, "fft8-8192-half-m0-const-runs": 6.48e-13,
    "fft8-8192-half-m0-lin-ragged": 4.13e-14, "fft8-8192-half-m0-lin-runs": 6.99e-14,
    "fft8-8192-half-m1-const-ragged": 1.25e-12, "fft8-8192-half-m1-const-runs": 2.66e-12,
    "fft8-8192-half-m1-lin-ragged": 1.64e-13, "fft8-8192-half-m1-lin-runs": 3.53e-13,
    "fft8-8192-half-m2-const-ragged": 4.85e-14, "fft8-8192-half-m2-const-runs": 1e-13,
    "fft8-8192-half-m2-lin-ragged": 4.57e-14, "fft8-8192-half-m2-lin-runs": 1.16e-13,
    "fft8-8192-any-m0-const-ragged": 3.49e-13, "fft8-8192-any-m0-const-runs": 6.03e-14,
    "fft8-8192-any-m0-lin-ragged": 3.19e-14, "fft8-8192-any-m0-lin-runs": 7.37e-14,
    "fft8-8192-any-m1-const-ragged": 2.38e-12, "fft8-8192-any-m1-const-runs": 1.44e-13,
    "fft8-8192-any-m1-lin-ragged": 2.36e-13, "fft8-8192-any-m1-lin-runs": 1.05e-13,
    "fft8-8192-any-m2-const-ragged": 9.27e-14, "fft8-8192-any-m2-const-runs": 1.12e-14,
    "fft8-8192-any-m2-lin-ragged": 1.18e-13, "fft8-8192-any-m2-lin-runs": 1.49e-14,
    "mix-64-n640-m0-const-ragged": 2.52e-14, "mix-64-n640-m0-const-runs": 4.88e-14,
    "mix-64-n640-m0-lin-ragged": 1.1e-14, "mix-64-n640-m0-lin-runs": 1.93e-14,
    "mix-64-n640-m1-const-ragged": 1.5e-13, "mix-64-n640-m1-const-runs": 2.04e-13,
    "mix-64-n640-m1-lin-ragged": 4.6e-14, "mix-64-n640-m1-lin-runs": 5.51e-14,
    "mix-64-n640-m2-const-ragged": 2.04e-14, "mix-64-n640-m2-const-runs": 2.79e-14,
    "mix-64-n640-m2-lin-ragged": 3.34e-14, "mix-64-n640-m2-lin-runs": 3.04e-14,
    "mix-64-n686-m0-const-runs": 4.13e-14, "mix-64-n686-m0-lin-runs": 2.73e-14,
    "mix-64-n686-m1-const-runs": 1.28e-13, "mix-64-n686-m1-lin-runs": 6.07e-14,
    "mix-64-n686-m2-const-runs": 1.57e-14, "mix-64-n686-m2-lin-runs": 2.06e-14,
    "mix-128-n1296-m0-const-ragged": 5.74e-14, "mix-128-n1296-m0-const-runs": 1.12e-13,
    "mix-128-n1296-m0-lin-ragged": 1.16e-14, "mix-128-n1296-m0-lin-runs": 3.98e-14,
    "mix-128-n1296-m1-const-ragged": 2.59e-13, "mix-128-n1296-m1-const-runs": 3.8e-13,
    "mix-128-n1296-m1-lin-ragged": 7.41e-14, "mix-128-n1296-m1-lin-runs": 1.66e-13,
    "mix-128-n1296-m2-const-ragged": 2.47e-14, "mix-128-n1296-m2-const-runs": 3.31e-14,
    "mix-128-n1296-m2-lin-ragged": 3.29e-14, "mix-128-n1296-m2-lin-runs": 4.51e-14,
    "mix-128-n1350-m0-const-runs": 9.37e-14, "mix-128-n1350-m0-lin-runs": 3.47e-14,
    "mix-128-n1350-m1-const-runs": 2.49e-13, "mix-128-n1350-m1-lin-runs": 7.92e-14,
    "mix-128-n1350-m2-const-runs": 2.09e-14, "mix-128-n1350-m2-lin-runs": 2.8e-14,
    "mix-256-n2592-m0-const-ragged": 8.97e-14, "mix-256-n2592-m0-const-runs": 2.3e-13,
    "mix-256-n2592-m0-lin-ragged": 2.82e-14, "mix-256-n2592-m0-lin-runs": 6.21e-14,
    "mix-256-n2592-m1-const-ragged": 3.92e-13, "mix-256-n2592-m1-const-runs": 9.18e-13,
    "mix-256-n2592-m1-lin-ragged": 1.47e-13, "mix-256-n2592-m1-lin-runs": 2.42e-13,
    "mix-256-n2592-m2-const-ragged": 2.73e-14, "mix-256-n2592-m2-const-runs": 6.03e-14,
    "mix-256-n2592-m2-lin-ragged": 6.22e-14, "mix-256-n2592-m2-lin-runs": 7.46e-14,
    "mix-256-n2646-m0-const-runs": 1.92e-13, "mix-256-n2646-m0-lin-runs": 6.07e-14,
    "mix-256-n2646-m1-const-runs": 5.18e-13, "mix-256-n2646-m1-lin-runs": 1.42e-13,
    "mix-256-n2646-m2-const-runs": 3.24e-14, "mix-256-n2646-m2-lin-runs": 5.11e-14,
    "mix-512-n5184-m0-const-ragged": 2.76e-13, "mix-512-n5184-m0-const-runs": 6.95e-13,
    "mix-512-n5184-m0-lin-ragged": 1.81e-14, "mix-512-n5184-m0-lin-runs": 6.55e-14,
    "mix-512-n5184-m1-const-ragged": 7.12e-13, "mix-512-n5184-m1-const-runs": 1.56e-12,
    "mix-512-n5184-m1-lin-ragged": 1.4e-13, "mix-512-n5184-m1-lin-runs": 2.42e-13,
    "mix-512-n5184-m2-const-ragged": 3.51e-14, "mix-512-n5184-m2-const-runs": 7.81e-14,
    "mix-512-n5184-m2-lin-ragged": 6.28e-14, "mix-512-n5184-m2-lin-runs": 8.09e-14,
    "mix-512-n5250-m0-const-runs": 3.88e-13, "mix-512-n5250-m0-lin-runs": 1.01e-13,
    "mix-512-n5250-m1-const-runs": 1.11e-12, "mix-512-n5250-m1-lin-runs": 2.65e-13,
    "mix-512-n5250-m2-const-runs": 5.13e-14, "mix-512-n5250-m2-lin-runs": 6.83e-14,
    "mix-1024-n10290-m0-const-ragged": 2.74e-13, "mix-1024-n10290-m0-const-runs": 6.01e-13,
    "mix-1024-n10290-m0-lin-ragged": 2.98e-14, "mix-1024-n10290-m0-lin-runs": 8.68e-14,
    "mix-1024-n10290-m1-const-ragged": 1.24e-12, "mix-1024-n10290-m1-const-runs": 2.33e-12,
    "mix-1024-n10290-m1-lin-ragged": 1.8e-13, "mix-1024-n10290-m1-lin-runs": 4.23e-13,
    "mix-1024-n10290-m2-const-ragged": 4.46e-14, "mix-1024-n10290-m2-const-runs": 8.56e-14,
    "mix-1024-n10290-m2-lin-ragged": 6.79e-14, "mix-1024-n10290-m2-lin-runs": 1.2e-13,
    "mix-1024-n10368-m0-const-runs": 8.52e-13, "mix-1024-n10368-m0-lin-runs": 1.43e-13,
    "mix-1024-n10368-m1-const-runs": 2.92e-12, "mix-1024-n10368-m1-lin-runs": 3.95e-13,
    "mix-1024-n10368-m2-const-runs": 1.03e-13, "mix-1024-n10368-m2-lin-runs": 1.29e-13,
    "split-256-n20790-m0-const-ragged": 1.12e-12, "split-256-n20790-m0-const-runs": 1.61e-12,
    "split-256-n20790-m0-lin-ragged": 8.51e-14, "split-256-n20790-m0-lin-runs": 1.44e-13,
    "split-256-n20790-m1-const-ragged": 4.06e-12, "split-256-n20790-m1-const-runs": 4.64e-12,
    "split-256-n20790-m1-lin-ragged": 2.56e-13, "split-256-n20790-m1-lin-runs": 4.39e-13,
    "split-256-n20790-m2-const-ragged": 1.07e-13, "split-256-n20790-m2-const-runs": 1.16e-13,
    "split-256-n20790-m2-lin-ragged": 1.44e-13, "split-256-n20790-m2-lin-runs": 1.34e-13,
    "split-256-n20800-m0-const-runs": 1.67e-12, "split-256-n20800-m0-lin-runs": 1.64e-13,
    "split-256-n20800-m1-const-runs": 6.74e-12, "split-256-n20800-m1-lin-runs": 7.5e-13,
    "split-256-n20800-m2-const-runs": 1.72e-13, "split-256-n20800-m2-lin-runs": 2.33e-13,
    "split-512-n20480-m0-const-ragged": 9.17e-13, "split-512-n20480-m0-const-runs": 1.82e-12,
    "split-512-n20480-m0-lin-ragged": 8.33e-14, "split-512-n20480-m0-lin-runs": 1.06e-13,
    "split-512-n20480-m1-const-ragged": 8.81e-12, "split-512-n20480-m1-const-runs": 5.69e-12,
    "split-512-n20480-m1-lin-ragged": 3.82e-13, "split-512-n20480-m1-lin-runs": 4.93e-13,
    "split-512-n20480-m2-const-ragged": 2.31e-13, "split-512-n20480-m2-const-runs": 1.44e-13,
    "split-512-n20480-m2-lin-ragged": 1.76e-13, "split-512-n20480-m2-lin-runs": 2.14e-13,
    "split-512-n24010-m0-const-runs": 1.06e-12, "split-512-n24010-m0-lin-runs": 1.29e-13,
    "split-512-n24010-m1-const-runs": 4.19e-12, "split-512-n24010-m1-lin-runs": 5.1e-13,
    "split-512-n24010-m2-const-runs": 9.84e-14, "split-512-n24010-m2-lin-runs": 1.93e-13,
    "split-1024-n20580-m0-const-ragged": 1.08e-12, "split-1024-n20580-m0-const-runs": 1.38e-12,
    "split-1024-n20580-m0-lin-ragged": 5.54e-14, "split-1024-n20580-m0-lin-runs": 1.12e-13,
    "split-1024-n20580-m1-const-ragged": 6.57e-12, "split-1024-n20580-m1-const-runs": 4.51e-12,
    "split-1024-n20580-m1-lin-ragged": 2.63e-13, "split-1024-n20580-m1-lin-runs": 4.96e-13,
    "split-1024-n20580-m2-const-ragged": 1.73e-13, "split-1024-n20580-m2-const-runs": 1.12e-13,
    "split-1024-n20580-m2-lin-ragged": 1.58e-13, "split-1024-n20580-m2-lin-runs": 1.58e-13,
    "split-1024-n21870-m0-const-runs": 1.17e-12, "split-1024-n21870-m0-lin-runs": 1.61e-13,
    "split-1024-n21870-m1-const-runs": 3.66e-12, "split-1024-n21870-m1-lin-runs": 3.87e-13,
    "split-1024-n21870-m2-const-runs": 8.92e-14, "split-1024-n21870-m2-lin-runs": 1.07e-13,
    "blue-512-n193-m0-const-ragged": 5.24e-15, "blue-512-n193-m0-const-runs": 9.58e-15,
    "blue-512-n193-m0-lin-ragged": 3.25e-15, "blue-512-n193-m0-lin-runs": 4.47e-15,
    "blue-512-n193-m1-const-ragged": 2.17e-14, "blue-512-n193-m1-const-runs": 3.18e-14,
    "blue-512-n193-m1-lin-ragged": 1.09e-14, "blue-512-n193-m1-lin-runs": 1.38e-14,
    "blue-512-n193-m2-const-ragged": 5.74e-15, "blue-512-n193-m2-const-runs": 9.06e-15,
    "blue-512-n193-m2-lin-ragged": 6.51e-15, "blue-512-n193-m2-lin-runs": 7.97e-15,
    "blue-1024-n257-m0-const-ragged": 5.39e-15, "blue-1024-n257-m0-const-runs": 6.19e-15,
    "blue-1024-n257-m0-lin-ragged": 3.47e-15, "blue-1024-n257-m0-lin-runs": 4.59e-15,
    "blue-1024-n257-m1-const-ragged": 2.44e-14, "blue-1024-n257-m1-const-runs": 2.09e-14,
    "blue-1024-n257-m1-lin-ragged": 1.6e-14, "blue-1024-n257-m1-lin-runs": 1.22e-14,
    "blue-1024-n257-m2-const-ragged": 6.99e-15, "blue-1024-n257-m2-const-runs": 5.71e-15,
    "blue-1024-n257-m2-lin-ragged": 1.08e-14, "blue-1024-n257-m2-lin-runs": 7e-15,
    "blue-2048-n513-m0-const-ragged": 3e-14, "blue-2048-n513-m0-const-runs": 8.07e-15,
    "blue-2048-n513-m0-lin-ragged": 1.26e-14, "blue-2048-n513-m0-lin-runs": 7.53e-15,
    "blue-2048-n513-m1-const-ragged": 1.27e-13, "blue-2048-n513-m1-const-runs": 1.64e-14,
    "blue-2048-n513-m1-lin-ragged": 6.42e-14, "blue-2048-n513-m1-lin-runs": 1.38e-14,
    "blue-2048-n513-m2-const-ragged": 1.8e-14, "blue-2048-n513-m2-const-runs": 4.47e-15,
    "blue-2048-n513-m2-lin-ragged": 2.96e-14, "blue-2048-n513-m2-lin-runs": 6.01e-15,
    "blue-4096-n1025-m0-const-ragged": 4.78e-14, "blue-4096-n1025-m0-const-runs": 2.11e-14,
    "blue-4096-n1025-m0-lin-ragged": 6.04e-15, "blue-4096-n1025-m0-lin-runs": 3.56e-14,
    "blue-4096-n1025-m1-const-ragged": 1.2e-13, "blue-4096-n1025-m1-const-runs": 3.17e-14,
    "blue-4096-n1025-m1-lin-ragged": 4.69e-14, "blue-4096-n1025-m1-lin-runs": 5.47e-14,
    "blue-4096-n1025-m2-const-ragged": 1.39e-14, "blue-4096-n1025-m2-const-runs": 6.41e-15,
    "blue-4096-n1025-m2-lin-ragged": 2.94e-14, "blue-4096-n1025-m2-lin-runs": 8.98e-15,
    "blue-8192-n2049-m0-const-ragged": 1.34e-13, "blue-8192-n2049-m0-const-runs": 3.9e-14,
    "blue-8192-n2049-m0-lin-ragged": 1.96e-14, "blue-8192-n2049-m0-lin-runs": 3.5e-14,
    "blue-8192-n2049-m1-const-ragged": 4.85e-13, "blue-8192-n2049-m1-const-runs": 6.39e-14,
    "blue-8192-n2049-m1-lin-ragged": 7.35e-14, "blue-8192-n2049-m1-lin-runs": 4.9e-14,
    "blue-8192-n2049-m2-const-ragged": 3.65e-14, "blue-8192-n2049-m2-const-runs": 9.44e-15,
    "blue-8192-n2049-m2-lin-ragged": 3.15e-14, "blue-8192-n2049-m2-lin-runs": 9.75e-15,
    "fft8-pad333of512-m0-lin-extra": 3.35e-15, "fft8-pad333of512-m1-const-extra": 5.3e-14,
    "fft8-pad333of512-m2-lin-extra": 2.01e-14, "fft8-nwin2of512-m0-const-extra": 4.92e-16,
    "fft8-nwin2of512-m1-const-extra": 9.53e-16, "fft8-nwin2of512-m2-const-extra": 5.53e-16,
    "fft8-nwin1of512-m0-const-extra": 0, "fft8-nwin1of512-m1-const-extra": 0, "fft8-nwin1of512-m2-const-extra": 0,
    "mix-pad333of648-m0-lin-extra": 5.3e-15, "mix-pad333of648-m1-const-extra": 2.02e-13,
    "mix-pad333of648-m2-lin-extra": 1.32e-14, "mix-nwin2of648-m0-const-extra": 7.01e-16,
    "mix-nwin2of648-m1-const-extra": 1.04e-15, "mix-nwin2of648-m2-const-extra": 4.68e-16,
    "mix-nwin1of648-m0-const-extra": 0, "mix-nwin1of648-m1-const-extra": 0, "mix-nwin1of648-m2-const-extra": 0,
    "split-pad4099of20580-m0-lin-extra": 7e-14, "split-pad4099of20580-m1-const-extra": 1.88e-12,
    "split-pad4099of20580-m2-lin-extra": 6.62e-14, "split-nwin2of20580-m0-const-extra": 8.55e-16,
    "split-nwin2of20580-m1-const-extra": 1.63e-15, "split-nwin2of20580-m2-const-extra": 7.43e-16,
    "split-nwin1of20580-m0-const-extra": 0, "split-nwin1of20580-m1-const-extra": 0,
    "split-nwin1of20580-m2-const-extra": 0, "blue-pad201of347-m0-lin-extra": 4.83e-15,
    "blue-pad201of347-m1-const-extra": 3.57e-14, "blue-pad201of347-m2-lin-extra": 6.5e-15,
    "blue-nwin2of347-m0-const-extra": 2.7e-15, "blue-nwin2of347-m1-const-extra": 3.41e-15,
    "blue-nwin2of347-m2-const-extra": 1.53e-15, "blue-nwin1of347-m0-const-extra": 0,
    "blue-nwin1of347-m1-const-extra": 0, "blue-nwin1of347-m2-const-extra": 0,
    "staged-pad333of4099-m0-lin-extra": 1.97e-14, "staged-pad333of4099-m1-const-extra": 8.56e-14,
    "staged-pad333of4099-m2-lin-extra": 9.8e-15, "staged-nwin2of4099-m0-const-extra": 2.42e-15,
    "staged-nwin2of4099-m1-const-extra": 3.5e-15, "staged-nwin2of4099-m2-const-extra": 1.96e-15,
    "staged-nwin1of4099-m0-const-extra": 0, "staged-nwin1of4099-m1-const-extra": 0,
    "staged-nwin1of4099-m2-const-extra": 0, "mix-radix-n20-m0-const-extra": 4.87e-16,
    "mix-radix-n20-m1-const-extra": 1.46e-15, "mix-radix-n20-m2-const-extra": 1.19e-15,
    "mix-radix-n8-m0-const-extra": 2.48e-16, "mix-radix-n8-m1-const-extra": 6.4e-16,
    "mix-radix-n8-m2-const-extra": 4.73e-16, "mix-radix-n10-m0-const-extra": 2.84e-16,
    "mix-radix-n10-m1-const-extra": 1.06e-15, "mix-radix-n10-m2-const-extra": 6.52e-16,
    "mix-radix-n4-m0-const-extra": 3.17e-16, "mix-radix-n4-m1-const-extra": 6.45e-16,
    "mix-radix-n4-m2-const-extra": 3.61e-16, "mix-radix-n6-m0-const-extra": 3.18e-16,
    "mix-radix-n6-m1-const-extra": 1.16e-15, "mix-radix-n6-m2-const-extra": 7.21e-16,
    "mix-radix-n14-m0-const-extra": 4.27e-16, "mix-radix-n14-m1-const-extra": 1.18e-15,
    "mix-radix-n14-m2-const-extra": 1.24e-15, "mix-radix-n200-m0-lin-extra": 3.79e-15,
    "mix-radix-n200-m1-const-extra": 1.21e-14, "mix-radix-n200-m2-lin-extra": 1.04e-14,
    "mix-radix-n80-m0-lin-extra": 2.05e-15, "mix-radix-n80-m1-const-extra": 1.01e-14,
    "mix-radix-n80-m2-lin-extra": 6.52e-15, "mix-radix-n40-m0-const-extra": 1.03e-15,
    "mix-radix-n40-m1-const-extra": 3.46e-15, "mix-radix-n40-m2-const-extra": 1.97e-15,
    "mix-radix-n60-m0-const-extra": 1.45e-15, "mix-radix-n60-m1-const-extra": 3.87e-15,
    "mix-radix-n60-m2-const-extra": 1.67e-15, "mix-radix-n100-m0-lin-extra": 1.62e-15,
    "mix-radix-n100-m1-const-extra": 1.37e-14, "mix-radix-n100-m2-lin-extra": 9.05e-15,
    "mix-radix-n140-m0-lin-extra": 1.24e-15, "mix-radix-n140-m1-const-extra": 2.1e-14,
    "mix-radix-n140-m2-lin-extra": 5.17e-15, "mix-radix-n24-m0-const-extra": 7.97e-16,
    "mix-radix-n24-m1-const-extra": 2.5e-15, "mix-radix-n24-m2-const-extra": 1.01e-15,
    "mix-radix-n36-m0-const-extra": 9.25e-16, "mix-radix-n36-m1-const-extra": 2.74e-15,
    "mix-radix-n36-m2-const-extra": 1.59e-15, "mix-radix-n50-m0-const-extra": 7.03e-16,
    "mix-radix-n50-m1-const-extra": 3.94e-15, "mix-radix-n50-m2-const-extra": 1.83e-15,
    "mix-radix-n98-m0-lin-extra": 1.78e-15, "mix-radix-n98-m1-const-extra": 9.78e-15,
    "mix-radix-n98-m2-lin-extra": 5.82e-15, "mix-radix-n42-m0-const-extra": 1.44e-15,
    "mix-radix-n42-m1-const-extra": 3.06e-15, "mix-radix-n42-m2-const-extra": 1.21e-15,
    "mix-radix-n1260-m0-lin-extra": 1.69e-14, "mix-radix-n1260-m1-const-extra": 1.91e-13,
    "mix-radix-n1260-m2-lin-extra": 3.12e-14, "split-r0-n24010-m0-lin-extra": 2.74e-14,
    "split-r0-n24010-m1-const-extra": 1.21e-12, "split-r0-n24010-m2-lin-extra": 5.18e-14,
    "split-r0-n21952-m0-lin-extra": 3.37e-14, "split-r0-n21952-m1-const-extra": 1.25e-12,
    "split-r0-n21952-m2-lin-extra": 6.02e-14, "split-r0-n30618-m0-lin-extra": 3.45e-14,
    "split-r0-n30618-m1-const-extra": 2.55e-12, "split-r0-n30618-m2-lin-extra": 7.64e-14,
    "staged-n4099-m0-const-extra": 1.49e-13, "staged-n4099-m0-lin-extra": 3.97e-14,
    "staged-n4099-m1-const-extra": 4.61e-13, "staged-n4099-m1-lin-extra": 9.63e-14,
    "staged-n4099-m2-const-extra": 2.59e-14, "staged-n4099-m2-lin-extra": 3.17e-14,
    "staged-n4096-env-m0-lin-extra": 3.61e-14, "staged-n4096-env-m1-const-extra": 2.76e-13,
    "staged-n4096-env-m2-lin-extra": 4.08e-14, "fft8-512-headruns-m2-lin-extra": 5.19e-15,
    "fft8-512-headruns-m0-const-extra": 7.02e-15, "mix-64-n640-headruns-m2-lin-extra": 1.46e-14,
    "mix-64-n640-headruns-m0-const-extra": 2.14e-14, "blue-512-n193-headruns-m2-lin-extra": 4.68e-15,
    "blue-512-n193-headruns-m0-const-extra": 5.57e-15, "blue-n2-m0-const-extra": 8.8e-16,
    "blue-n2-m1-const-extra": 8.95e-16, "blue-n2-m2-const-extra": 4.74e-16, "blue-n3-m0-lin-extra": 4.09e-16,
    "blue-n3-m1-const-extra": 9.05e-16, "blue-n3-m2-lin-extra": 2.29e-15,
}
# worst error / (16 e64) over a family's cases (ragged, runs, extra), MI355X: at most 2.9 e64.  Every row
# against long double; WORST_RATIO_SUBSET: the runs cases of SUBSET_TAGS, whose rows outside ``subset`` are
# measured against the float64 pipeline at 17 e64
WORST_RATIO = {"cube": 0.15, "fft8": 0.16, "mix": 0.18, "split": 0.18, "blue": 0.15, "staged": 0.13}
WORST_RATIO_SUBSET = {"fft8": 0.16, "mix": 0.18, "split": 0.24}

# (none does today) a family that misses 16 e64 on ALL its instances alike keeps the smallest power-of-two multiple of
# e64 that holds with a factor 2 to spare, never above 1e-12: family -> that multiple
FAMILY_BOUND = {}


def bound(case, e64):
    """16 e64(case): the kernels sum in another order, take their twiddles from tables and use
    other radices than pocketfft.  FAMILY_BOUND: another multiple, capped at 1e-12."""
    mult = FAMILY_BOUND.get(case.want[0], 16)
    return min(mult * e64, 1e-12) if mult != 16 else 16 * e64


def check_estimate(got, case, ref):
    """got: the handle's estimate of every channel (DFT / PSD: (nseg, nch, nfreq); MEAN: (nch,
    nfreq)) -> (worst error / bound over ALL rows, worst error on the long-double rows).  Rows of
    ``ref.chans`` against the long-double reference at the bound; in a runs case the others
    against the float64 pipeline at the bound plus e64."""
    b = bound(case, ref.e64)
    pick = got[ref.chans] if case.mode == MEAN else got[:, ref.chans]
    err = float(row_metric(pick, ref.exact, case.mode).max()) if pick.size else 0.0
    worst = err / b if b > 0 else (0.0 if err == 0 else np.inf)
    if len(ref.chans) < case.nch:
        rest = sorted(set(range(case.nch)) - set(ref.chans))
        g, a = (got[rest], ref.approx[rest]) if case.mode == MEAN else (got[:, rest], ref.approx[:, rest])
        worst = max(worst, float(row_metric(g, a, case.mode).max()) / (b + ref.e64))
    return worst, err


def input_conditions(case, x=None, X64=None):
    """(the smallest share of a row's mean power that its DC, first and Nyquist bins hold, over
    every row; for linear detrend the smallest change the fitted line makes to a row's spectrum,
    relative to its rms), from the float64 pipeline."""
    x = signal(case) if x is None else x
    X = spectrum(x, case, np.float64) if X64 is None else X64
    P = power(X, case.nfft)
    bins = [0, 1] + ([P.shape[-1] - 1] if case.nfft % 2 == 0 else [])
    bins = [b for b in bins if b < P.shape[-1]]
    share = float((P[..., bins] / P.mean(axis=-1, keepdims=True)).min())
    change = np.inf
    if case.linear and case.nwin > 1:
        # spectrum with the line left in minus spectrum without = slope times the spectrum of the
        # windowed ramp, one vector for all rows
        seg = segment_rows(x, case, np.float64)
        seg -= seg.mean(axis=-1, keepdims=True)
        t = np.arange(case.nwin) - 0.5 * (case.nwin - 1)
        slope = np.abs(seg @ t) / (t @ t)
        L = np.fft.rfft(t * window(case), n=case.nfft) * SCALE
        rms = np.sqrt((X.real * X.real + X.imag * X.imag).mean(-1))
        change = float((slope * np.sqrt((np.abs(L) ** 2).mean()) / rms).min())
    return share, change
