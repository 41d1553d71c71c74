"""The compiled instances ("cells") of the polyphase resampler (csrc/poly.hip) and what tests them.

A cell is (kernel, ONE, NT, EG): (1, ONE, NT, EG) is poly_block_kernel<ONE, NT, EG>, (0, 0, 0, 0) the
cache-path fallback poly_kernel.  A corpus entry is (L, M, ntaps, centre or None) with its declared
cell and its declared set of tails: cnt % 8 over the phase streams of the entry, cnt being the
count of taps the block kernel multiplies in one stream (whole blocks of 8 plus one of seven
straight-line tail cases).  UNREACHED names every compiled instance no (L, M, ntaps) reaches, with
the planner's reason.  Shared by tests/test_poly_cells_host.py (inventory, plans and the NumPy
restatement of the block kernel, no GPU) and tests/test_gpu_poly_cells.py (every entry through
dev.PolyStream)."""

import os
import re
import struct
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALLBACK = (0, 0, 0, 0)
R, BLK, BATCH = 4, 8, 24        # kPolyR, kPolyBlk, kPolyBatch of poly.hip

# pad: None, or (taps of the window, stream length) of an entry built as the public API builds it
# (numerical._resample_padded): ntaps and centre are then those of the padded window
Entry = namedtuple("Entry", "L M ntaps centre cell tails pad", defaults=(None,))


def _e(cell, L, M, ntaps, tails, centre=None, pad=None):
    return Entry(L, M, ntaps, centre, cell, frozenset(tails), pad)


D256, D128_2, D64_2, D64_4 = (1, 1, 256, 1), (1, 1, 128, 2), (1, 1, 64, 2), (1, 1, 64, 4)
D128, D64 = (1, 1, 128, 1), (1, 1, 64, 1)
R256, R128, R64 = (1, 0, 256, 1), (1, 0, 128, 1), (1, 0, 64, 1)

# the seven instances the public API's default designs use
DAILY = (D256, D128_2, D64_2, D64_4, R256, R128, R64)

CORPUS = [
    # <true,256,1>
    _e(D256, 1, 2, 3, (1, 2)),
    _e(D256, 1, 2, 9, (4, 5)),
    _e(D256, 1, 2, 21, (2, 3)),
    _e(D256, 1, 2, 37, (2, 3)),
    _e(D256, 1, 2, 160, (0,)),
    _e(D256, 1, 5, 7, (1, 2)),
    _e(D256, 1, 5, 23, (4, 5)),
    _e(D256, 1, 5, 48, (1, 2)),
    _e(D256, 1, 5, 113, (6, 7)),
    _e(D256, 1, 5, 171, (2, 3)),
    # <true,128,2>: EG = 2, the uneven split at M = 5 and 7 and the even one at M = 2
    _e(D128_2, 1, 5, 400, (0,)),
    _e(D128_2, 1, 7, 10, (1, 2)),
    _e(D128_2, 1, 7, 33, (4, 5)),
    _e(D128_2, 1, 7, 45, (6, 7)),
    _e(D128_2, 1, 7, 160, (6, 7)),
    _e(D128_2, 1, 7, 300, (2, 3)),
    _e(D128_2, 1, 10, 25, (2, 3)),
    _e(D128_2, 1, 10, 226, (6, 7)),
    _e(D128_2, 1, 2, 3400, (4,)),
    # <true,64,2>: the uneven split at M = 3 and 13
    _e(D64_2, 1, 10, 431, (3, 4)),
    _e(D64_2, 1, 13, 30, (2, 3)),
    _e(D64_2, 1, 13, 60, (4, 5)),
    _e(D64_2, 1, 13, 110, (0, 1)),
    _e(D64_2, 1, 13, 293, (6, 7)),
    _e(D64_2, 1, 13, 600, (6, 7)),
    _e(D64_2, 1, 20, 50, (2, 3)),
    _e(D64_2, 1, 3, 5000, (2, 3)),
    # <true,64,4>: EG = 4, the uneven splits at M = 5, 25 and 54; (1, 54, 1207) is the largest window the block kernel takes
    _e(D64_4, 1, 20, 470, (0, 7)),
    _e(D64_4, 1, 25, 60, (2, 3)),
    _e(D64_4, 1, 25, 110, (4, 5)),
    _e(D64_4, 1, 25, 210, (0, 1)),
    _e(D64_4, 1, 25, 561, (6, 7)),
    _e(D64_4, 1, 25, 1130, (5, 6)),
    _e(D64_4, 1, 40, 90, (2, 3)),
    _e(D64_4, 1, 40, 895, (6, 7)),
    _e(D64_4, 1, 54, 120, (2, 3)),
    _e(D64_4, 1, 54, 1207, (6, 7)),
    _e(D64_4, 1, 4, 5300, (5,)),
    _e(D64_4, 1, 5, 4200, (0,)),
    # the single-group small tiles: L = M = 1
    _e(D128, 1, 1, 4500, (4,)),
    _e(D64, 1, 1, 9000, (0,)),
    # <false,256,1>
    _e(R256, 3, 1, 1, (1,)),
    _e(R256, 3, 1, 2, (1,)),
    _e(R256, 3, 1, 5, (1, 2)),
    _e(R256, 3, 1, 14, (4, 5)),
    _e(R256, 3, 1, 19, (6, 7)),
    _e(R256, 3, 1, 69, (7,)),
    _e(R256, 3, 1, 200, (2, 3)),
    _e(R256, 3, 2, 2, (1,)),
    _e(R256, 3, 2, 20, (3, 4)),
    _e(R256, 3, 2, 69, (3, 4)),
    _e(R256, 3, 2, 91, (0, 7)),
    _e(R256, 3, 2, 301, (2, 3)),
    # <false,128,1>
    _e(R128, 2, 7, 40, (2, 3)),
    _e(R128, 2, 7, 159, (3, 4)),
    _e(R128, 2, 7, 500, (3, 4)),
    _e(R128, 5, 3, 64, (4, 5)),
    _e(R128, 5, 3, 113, (0, 7)),
    _e(R128, 5, 3, 333, (6, 7)),
    _e(R128, 7, 3, 1, (1,)),
    _e(R128, 7, 3, 2, (1,)),
    _e(R128, 7, 3, 3, (1,)),
    _e(R128, 7, 3, 5, (1,)),
    # <false,64,1>
    _e(R64, 3, 11, 100, (3, 4)),
    _e(R64, 3, 11, 247, (0, 7)),
    _e(R64, 3, 11, 800, (0, 1)),
    _e(R64, 3, 11, 1070, (0, 1)),
    _e(R64, 4, 25, 300, (3,)),
    _e(R64, 4, 25, 561, (5, 6)),
    _e(R64, 4, 25, 1900, (3,)),
    _e(R64, 4, 54, 1, (1,)),
    _e(R64, 4, 54, 2, (1,)),
    _e(R64, 4, 54, 3, (1,)),
    _e(R64, 4, 54, 229, (1, 2)),
    # the fallback; (1, 55, 1230) is the first neighbour of (1, 54, 1207)
    _e(FALLBACK, 1, 64, 130, (2, 3)),
    _e(FALLBACK, 1, 64, 1431, (6, 7)),
    _e(FALLBACK, 3, 64, 2, (1,)),
    _e(FALLBACK, 3, 64, 400, (2, 3)),
    _e(FALLBACK, 4, 57, 229, (1, 2)),
    _e(FALLBACK, 1, 55, 1230, (6, 7)),
    # built as the public API builds them (numerical._resample_padded): 100 taps, seven zeros in front and one
    # behind for a stream of 12000 samples; 400 taps, 57 and 2 zeros for 20000 samples
    _e(R128, 3, 7, 108, (5, 6), centre=56, pad=(100, 12000)),
    _e(FALLBACK, 3, 64, 459, (2, 3), centre=256, pad=(400, 20000)),
]

# compiled instances no handle reaches, with the planner's reason
UNREACHED = {
    (1, 1, 128, 4): ("polyplan::plan takes the 128-thread tile only when its window fits 53 KB, and "
                     "polyplan::phase_groups takes four groups only when the window exceeds 53 KB"),
}


def entry_id(e):
    c = "" if e.centre is None else f"-c{e.centre}"
    return f"L{e.L}-M{e.M}-n{e.ntaps}{c}"


def cell_name(cell):
    return "poly_kernel" if cell == FALLBACK else "<%s,%d,%d>" % ("true" if cell[1] else "false", cell[2], cell[3])


def centre_of(e):
    return (e.ntaps - 1) // 2 if e.centre is None else e.centre


def taps_of(e):
    """Every tap carries weight (no window hides a dropped edge tap below the tolerance); the padded
    entries: such a window of pad[0] taps with SciPy's zeros around it."""
    rng = np.random.default_rng([20240, e.L, e.M, e.ntaps if e.pad is None else e.pad[0]])
    if e.pad is None:
        return rng.standard_normal(e.ntaps) / np.sqrt(e.ntaps)
    from openseize_amd.core import numerical as nm
    taps, centre = nm._resample_padded(rng.standard_normal(e.pad[0]) / np.sqrt(e.pad[0]), e.L, e.M, e.pad[1])
    assert (len(taps), centre) == (e.ntaps, e.centre), (entry_id(e), len(taps), centre)
    return taps


def one_per_cell():
    """The first entry of every cell that has more than a handful of taps."""
    seen, out = set(), []
    for e in CORPUS:
        if e.cell not in seen and e.ntaps >= 20:
            seen.add(e.cell)
            out.append(e)
    return out


# ------------------------------------------------------------------------------ the definition
def definition(x, h, L, M, centre=None):
    """y[j] = sum_k L h[k] xup[j M + centre - k], xup = x zero-stuffed by L, zeros outside,
    j < ceil(n L / M); in np.longdouble, by direct convolution (a NaN lands exactly where a tap
    touches it).  x: (channels, n)."""
    x = np.atleast_2d(x)
    n, m = x.shape[1], len(h)
    centre = (m - 1) // 2 if centre is None else centre
    nout = -(-n * L // M)
    hl = np.asarray(h, np.longdouble) * L
    idx = np.arange(nout) * M + centre
    out = np.zeros((x.shape[0], nout), np.longdouble)
    for c in range(x.shape[0]):
        xup = np.zeros(n * L, np.longdouble)
        xup[::L] = x[c]
        full = np.convolve(xup, hl)
        ok = idx < len(full)
        out[c, ok] = full[idx[ok]]
    return out


# --------------------------------------------------------------------- the host harness (g++)
_EXE = {}


def build_host_exe():
    """tests/host/poly_host_check.cpp built by g++ from the library's own poly_plan.h (once per
    process)."""
    if "path" not in _EXE:
        src = os.path.join(ROOT, "tests", "host", "poly_host_check.cpp")
        inc = os.path.join(ROOT, "openseize_amd", "csrc")
        path = os.path.join(tempfile.mkdtemp(), "poly_host_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", inc, src, "-o", path])
        _EXE["path"] = path
    return _EXE["path"]


_KEYS = ("kernel", "ONE", "NT", "EG", "apad", "se", "lds_bytes", "H", "half", "stepw", "dqs")


def host_plans(exe, cases):
    """[(L, M, taps, centre)] -> the plan of each as the library makes it, with its table G[L][M][apad]
    (None for the fallback) and the (L, M, ntaps) it was made for."""
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(cases)))
            for L, M, taps, centre in cases:
                taps = np.ascontiguousarray(taps, np.float64)
                f.write(struct.pack("<iiii", len(taps), centre, L, M))
                f.write(taps.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    pos, out = 0, []
    for L, M, taps, centre in cases:
        p = dict(zip(_KEYS, struct.unpack_from("<11i", raw, pos)))
        n, = struct.unpack_from("<q", raw, pos + 48)
        G = np.frombuffer(raw, np.float64, n, pos + 56).copy()
        pos += 56 + 8 * n
        p.update(L=L, M=M, m=len(taps), G=G.reshape(L, M, p["apad"]) if p["kernel"] else None)
        out.append(p)
    assert pos == len(raw)
    return out


def cell_of_plan(p):
    return (p["kernel"], p["ONE"], p["NT"], p["EG"])


_NM_BLOCK = re.compile(r"poly_block_kernel<(true|false), (\d+), (\d+)>")
_NM_FALLBACK = re.compile(r"\bosz::poly_kernel\(")


def compiled_cells(lib_path):
    """The cells compiled into the library, from `nm -C`."""
    out = subprocess.check_output(["nm", "-C", lib_path], text=True)
    cells = {(1, int(m.group(1) == "true"), int(m.group(2)), int(m.group(3))) for m in _NM_BLOCK.finditer(out)}
    if _NM_FALLBACK.search(out):
        cells.add(FALLBACK)
    return cells


# ------------------------------------------------------- the block kernel's index arithmetic
def class_params(L, M, m, half, jf):
    """(r, phi, msub, i0) of the residue class whose first output in a tile is jf."""
    r = jf % L
    phi = (r * M + half) % L
    msub = (m - phi + L - 1) // L if phi < m else 0
    itop = (jf * M + half - phi) // L
    return r, phi, msub, itop - (msub - 1)


def stream_counts(L, M, m, half):
    """cnt[r][ph]: the taps poly_block_kernel multiplies in phase stream ph of residue class r."""
    out = np.zeros((L, M), int)
    for r in range(L):
        msub = class_params(L, M, m, half, r)[2]
        cq, crem = ((msub - 1) // M, (msub - 1) % M) if msub > 0 else (0, -1)
        out[r] = [cq + 1 if ph <= crem else cq for ph in range(M)]
    return out


def tails_of(cnt):
    return frozenset(int(c) % BLK for c in np.ravel(cnt) if c > 0)


def pad(i):
    return i + (i >> 2)


def descriptor_classes(p, nin, n, nout, final=False):
    """How many (tile, class) windows of a push of n samples (nin consumed, nout produced before it)
    poly_block_kernel stages through the buffer descriptor: the whole window inside the chunk."""
    L, M, m, half = p["L"], p["M"], p["m"], p["half"]
    navail = nin + n
    j1 = max(nout, -(-navail * L // M) if final else -(-(navail * L - half) // M))
    NJ, nth = p["NT"] * R, p["NT"] * p["EG"]
    wtot = (NJ + p["apad"]) * M
    hits = 0
    for J0 in range(nout, j1, NJ * L):
        for cls in range(L):
            i0 = class_params(L, M, m, half, J0 + cls)[3]
            hits += i0 >= nin and i0 + wtot <= navail and M <= nth
    return hits


def first_push(p):
    """The shortest first push (and 17 samples) in which one tile, every class of it, has its whole
    window inside the chunk -- the buffer-descriptor staging path; never less than one tile of input
    plus 17 samples."""
    L, M, m, half = p["L"], p["M"], p["m"], p["half"]
    NJ = p["NT"] * R
    wtot = (NJ + p["apad"]) * M
    k = 0
    while True:
        i0 = [class_params(L, M, m, half, k * NJ * L + cls)[3] for cls in range(L)]
        if min(i0) >= 0:
            return max(NJ * M, max(i0) + wtot) + 17
        k += 1


def schedule(p, n=None):
    """(n, push lengths) of the ragged stream of tests/test_gpu_poly_cells.py; a last, empty push
    with final=True follows.  n: the stream length, where the entry's taps were made for one."""
    M, H = p["M"], p["H"]
    if p["kernel"]:
        tile = p["NT"] * R * M
        p1 = first_push(p)
    else:
        tile = 256 * M // p["L"]
        p1 = tile + 17
    head = [p1, 1, 0, H - 1, H - 1, M - 1]
    if n is None:
        n = max(sum(head) + int(1.3 * tile) + 5, 0 if p["kernel"] else 20000)
    return n, head + [n - sum(head) - 5, 5]


# ----------------------------------------------------- the block kernel restated in NumPy
def block_model(p, x):
    """poly_block_kernel on one channel, one push of the whole stream with final=True, driven by the
    library's plan and table: the window staged deinterleaved by phase into a flat LDS image of
    se doubles per stream at poly_pad positions (through the buffer-descriptor walk where the kernel
    takes it, element-wise elsewhere), cnt taps per stream from cq and crem in whole blocks of 8 and
    a tail, the table's padding never multiplied, the phase groups' partial sums added in order.
    Unstaged LDS is NaN: a read of it that reaches an output shows.  Returns (y, descriptor windows)."""
    L, M, m, half, G = p["L"], p["M"], p["m"], p["half"], p["G"]
    NT, EG, apad, se = p["NT"], p["EG"], p["apad"], p["se"]
    NJ, NTH = NT * R, NT * EG
    n = len(x)
    j1 = -(-n * L // M)
    nstream = NJ + apad
    wtot = nstream * M
    lds = p["lds_bytes"] // 8
    assert lds == M * se + (0 if L == 1 else NJ * L)
    assert pad(nstream - 1) < se, "a phase stream runs into the next one"
    y = np.full(j1, np.nan)
    t4 = 4 * np.arange(NT)
    fast = 0
    for J0 in range(0, j1, NJ * L):
        outbuf = np.full((L, NJ), np.nan)
        for cls in range(L):
            r, phi, msub, i0 = class_params(L, M, m, half, J0 + cls)
            win = np.full(lds, np.nan)
            if i0 >= 0 and i0 + wtot <= n and M <= NTH:
                fast += 1
                stepw, dqs = p["stepw"], p["dqs"]
                tw = np.arange(NTH)
                e0, iu = tw % M, tw // M
                for w0 in range(0, wtot, BATCH * stepw):
                    whole = w0 + BATCH * stepw + NTH - stepw <= wtot
                    for u in range(BATCH):
                        w = w0 + u * stepw + tw
                        if w0 + u * stepw < wtot:
                            v = np.where(w < wtot, x[np.minimum(i0 + w, n - 1)], 0.0)   # (behind the descriptor: 0)
                        else:
                            v = np.zeros(NTH)
                        assert not whole or (w < wtot).all()
                        keep = np.ones(NTH, bool) if whole else iu < nstream
                        a = e0[keep] * se + pad(iu[keep])
                        assert a.size == 0 or a.max() < M * se
                        win[a] = v[keep]
                        iu = iu + dqs
            else:
                w = np.arange(wtot)
                g = i0 + w
                ok = (g >= 0) & (g < n)
                a = (w % M) * se + pad(w // M)
                assert a.max() < M * se
                win[a] = np.where(ok, x[np.clip(g, 0, n - 1)], 0.0)
            cq, crem = ((msub - 1) // M, (msub - 1) - (msub - 1) // M * M) if msub > 0 else (0, -1)
            part = np.zeros((EG, NT, R))
            for eg in range(EG):
                for ph in range(eg * M // EG, (eg + 1) * M // EG):
                    cnt = cq + 1 if ph <= crem else cq
                    nfull = cnt & ~(BLK - 1)
                    assert cnt <= apad and (cnt == nfull or nfull + BLK <= apad)
                    if cnt:
                        at = ph * se + pad(np.arange(cnt)[:, None, None] + t4[None, :, None] + np.arange(R))
                        part[eg] += np.einsum("a,ats->ts", G[r, ph, :cnt], win[at])
            outbuf[cls] = part.sum(0).reshape(NJ) if EG > 1 else part[0].reshape(NJ)
        tile = outbuf.T.reshape(-1)                    # outbuf[cls + L * output]
        k = min(j1 - J0, NJ * L)
        y[J0:J0 + k] = tile[:k]
    return y, fast
