"""The compiled instances ("cells") of the stand-alone overlap-add FIR (csrc/fir.hip) and what tests them.

A cell is ("nega", NB): fir_nega_kernel<NB>, or ("pair", NR, PF): fir_oa_kernel<NR, 16, PF> (PF = 0 is
the instance with the spectrum resident, fir_oa_kernel<NR, -1, 0>).  A corpus entry is (ntaps, nch,
kind) with the declared cell of each of its pieces; kind names what is pushed:
  narrow   C = 3, the ragged schedule of narrow_schedule(): the seams between pushes and runs;
  wide     C = 64, one push of 48 blocks and a ragged one: runs of several whole blocks / pairs;
  part     C = 2, filters cut into pieces of 2048 taps, in chunks.
UNREACHED names every compiled instance no handle reaches, with the planner's reason.  Taps are
nonzero integers in [-8, 8], data integers in [-8, 8]: the convolution is an integer, computed exactly
in int64 (np.convolve) or, where that is slow, as the rounded float64 FFT convolution
(test_fir_cells_host.py shows the two agree and how far the FFT is from an integer).  Shared by
tests/test_fir_cells_host.py (inventory, plans, schedules, the reference; no GPU) and
tests/test_gpu_fir_cells.py (every entry through dev.FirStream)."""

import functools
import os
import re
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TAPS, PART, MAX_PARTS = 2049, 2048, 16      # kFirMaxTaps, kFirPart, kFirMaxParts of fir_plan.h
PAIR = ("pair", 15, 1)                          # the one pair instance a handle reaches
CUS = 256                                       # compute units the host tests plan for (MI355X)
WIDE_BLOCKS = 48

Entry = namedtuple("Entry", "ntaps nch kind cells")


def _e(ntaps, nch, kind, *cells):
    return Entry(ntaps, nch, kind, tuple(cells))


def _n(nb):
    return ("nega", nb)


CORPUS = [
    # narrow: both ends of every NB range, and the single tap
    _e(2, 3, "narrow", _n(31)), _e(257, 3, "narrow", _n(31)),
    _e(258, 3, "narrow", _n(30)), _e(513, 3, "narrow", _n(30)),
    _e(514, 3, "narrow", _n(29)), _e(769, 3, "narrow", _n(29)),
    _e(770, 3, "narrow", _n(28)), _e(1025, 3, "narrow", _n(28)),
    _e(1026, 3, "narrow", _n(27)), _e(1281, 3, "narrow", _n(27)),
    _e(1282, 3, "narrow", _n(26)), _e(1537, 3, "narrow", _n(26)),
    _e(1538, 3, "narrow", _n(25)), _e(1793, 3, "narrow", _n(25)),
    _e(1794, 3, "narrow", _n(24)), _e(2049, 3, "narrow", _n(24)),
    _e(1, 3, "narrow", PAIR),
    # wide: the lower end of three ranges, the pair cell writing and the pair cell accumulating
    _e(1794, 64, "wide", _n(24)),
    _e(1026, 64, "wide", _n(27)),
    _e(2, 64, "wide", _n(31)),
    _e(1, 64, "wide", PAIR),
    _e(4097, 64, "wide", _n(24), _n(24), PAIR),
    # partitioned
    _e(2050, 2, "part", _n(24), _n(31)),
    _e(4096, 2, "part", _n(24), _n(24)),
    _e(4097, 2, "part", _n(24), _n(24), PAIR),
    _e(6145, 2, "part", _n(24), _n(24), _n(24), PAIR),
    _e(32768, 2, "part", *([_n(24)] * 16)),
]

_WHY_NR = ("fir_plan.h: fir_piece_plan gives fir_nega_kernel every piece of 2 ... 2049 taps, so fir_oa_kernel is "
           "left the pieces of one tap, whose block is fir_pair_step(1) / 256 = 15 rows")
_WHY_PF = "fir_pf_table.h: OSZ_FIR_PF_TABLE names variant 1 for 15 rows"
UNREACHED = {("pair", nr, pf): _WHY_NR for nr in range(8, 15) for pf in (0, 1, 2)}
UNREACHED.update({("pair", 15, pf): _WHY_PF for pf in (0, 2)})


def entry_id(e):
    return f"{e.kind}-t{e.ntaps}-c{e.nch}"


def cell_name(cell):
    return "fir_nega_kernel<%d>" % cell[1] if cell[0] == "nega" else "fir_oa_kernel<%d, 16, %d>" % cell[1:]


NARROW = [e for e in CORPUS if e.kind == "narrow"]
WIDE = [e for e in CORPUS if e.kind == "wide"]
PARTITIONED = [e for e in CORPUS if e.kind == "part"]


def one_per_cell():
    """The first narrow entry of every cell: NB 31 ... 24 and the pair cell."""
    seen, out = set(), []
    for e in NARROW:
        if e.cells[0] not in seen:
            seen.add(e.cells[0])
            out.append(e)
    return out


# -------------------------------------------------------------- the planner restated in Python
def pieces_of(ntaps):
    """[(offset, taps)] of the pieces of a filter."""
    if ntaps <= MAX_TAPS:
        return [(0, ntaps)]
    nparts = -(-ntaps // PART)
    assert nparts <= MAX_PARTS
    return [(q * PART, min(PART, ntaps - q * PART)) for q in range(nparts)]


def piece_plan(taps):
    """(kernel, rows, step) of a piece."""
    if 2 <= taps <= MAX_TAPS:
        nb = min(31, (8193 - taps) // 256)
        return "nega", nb, 256 * nb
    nr = min(15, (4097 - taps) // 256)
    return "pair", nr, 256 * nr


def push_plan(n, step, nch, cus):
    """(nblocks, R, nruns) of a push of n samples."""
    nblocks = -(-n // step)
    R = max(2, min(32, nblocks * nch // 384)) & ~1
    nruns = -(-nblocks // R)
    slots = 2 * cus
    best, best_waste = nruns, 2.0
    for cand in range(nruns, nruns + 8):
        w = cand * nch
        waste = 1.0 - w / (-(-w // slots) * slots)
        if waste < best_waste - 1e-9:
            best, best_waste = cand, waste
    return nblocks, R, max(1, min(best, nblocks // 2))


def run_start(r, nblocks, nruns):
    """fir_run_start of fir_pair.h: the first block of run r."""
    return min(2 * (r * ((nblocks + 1) // 2) // nruns), nblocks)


def whole_per_run(rec):
    """From a launch record: per run, the most consecutive whole blocks (nega) or whole pairs (pair) --
    blocks (pairs) that lie inside the push and behind the left cut."""
    step, n, skip, nblocks, nruns = (rec[k] for k in ("step", "n", "skip", "nblocks", "nruns"))
    unit = 1 if rec["kernel"] == "nega" else 2
    out = []
    for r in range(nruns):
        b0, b1 = run_start(r, nblocks, nruns), run_start(r + 1, nblocks, nruns)
        best = cur = 0
        for b in range(b0, b1, unit):
            ok = b + unit <= b1 and (b + unit) * step <= n and b * step >= skip
            cur = cur + 1 if ok else 0
            best = max(best, cur)
        out.append(best)
    return out


def expected_records(e, n, skip, cus):
    """What FirStream.last_launches() must report after a push of n samples with `skip`."""
    ps = pieces_of(e.ntaps)
    recs = []
    for q, ((off, taps), cell) in enumerate(zip(ps, e.cells)):
        kernel, rows, step = piece_plan(taps)
        nblocks, R, nruns = push_plan(n, step, e.nch, cus)
        recs.append(dict(kernel=kernel, rows=rows, pf=cell[2] if kernel == "pair" else 0, piece=q, taps=taps,
                         step=step, nblocks=nblocks, R=R, nruns=nruns, accum=int(len(ps) > 1), n=n,
                         skip=skip if len(ps) == 1 else 0))
    return recs


def cell_of_record(r):
    return ("nega", r["rows"]) if r["kernel"] == "nega" else ("pair", r["rows"], r["pf"])


# -------------------------------------------------------------------------- what is pushed
def last_step(e):
    """The block length of the entry's last piece: the cell a wide entry is about."""
    return piece_plan(pieces_of(e.ntaps)[-1][1])[2]


def narrow_schedule(e):
    """The pushes of a narrow entry, S = step, w = ntaps - 1: whole blocks only (two runs, the tail left
    in registers); one sample; w - 1 twice (pushes shorter than the tail back to back: the seam
    kernel's leftover of the old state); a last block of one sample; a last block of w samples;
    a last block one short of whole; one ragged block; two whole blocks."""
    S, w = last_step(e), e.ntaps - 1
    return [5 * S, 1] + ([w - 1, w - 1] if w > 1 else []) + [4 * S + 1, 4 * S + w, 2 * S + S - 1, S - 1, 2 * S]


def wide_schedule(e):
    S = last_step(e)
    return [WIDE_BLOCKS * S, 7 * S + 777]


PART_N = {32768: 40000}
PART_CHUNKS = {32768: (777, None)}


def part_length(e):
    return PART_N.get(e.ntaps, 30011)


def part_chunkings(e):
    """Chunk lengths of a partitioned entry; None: one push."""
    return PART_CHUNKS.get(e.ntaps, (777, 3000, None))


def stream_length(e):
    return {"narrow": lambda: sum(narrow_schedule(e)), "wide": lambda: sum(wide_schedule(e)),
            "part": lambda: part_length(e)}[e.kind]()


def taps_of(e):
    """Nonzero integers in [-8, 8]: every tap carries weight."""
    rng = np.random.default_rng([2024, e.ntaps])
    return (rng.integers(1, 9, e.ntaps) * rng.choice([-1, 1], e.ntaps)).astype(np.float64)


def data_of(e, n=None):
    """Integers in [-8, 8], (nch, n), seeded per entry."""
    n = stream_length(e) if n is None else n
    return np.random.default_rng([77, e.ntaps, e.nch]).integers(-8, 9, (e.nch, n)).astype(np.float64)


# ------------------------------------------------------------------------------ the reference
def uses_fft(e):
    return e.kind == "wide" or e.ntaps == 32768


def exact(x, h):
    """The full convolution of every row of x with h, exactly: int64 np.convolve."""
    xi, hi = np.asarray(x).astype(np.int64), np.asarray(h).astype(np.int64)
    assert np.array_equal(xi, x) and np.array_equal(hi, h)
    return np.stack([np.convolve(r, hi) for r in np.atleast_2d(xi)])


def fft_unrounded(x, h):
    import scipy.signal as sps
    return sps.oaconvolve(np.atleast_2d(x), np.asarray(h, np.float64)[None], axes=-1)


def reference(x, h, fft):
    """(nch, n + ntaps - 1) float64: the exact integer convolution."""
    return np.rint(fft_unrounded(x, h)) if fft else exact(x, h).astype(np.float64)


@functools.lru_cache(maxsize=None)
def clean(e, n=None):
    """(x, reference, its scale) of an entry's stream: computed once, never written."""
    x = data_of(e, n)
    ref = reference(x, taps_of(e), uses_fft(e))
    for a in (x, ref):
        a.setflags(write=False)
    return x, ref, float(np.max(np.abs(ref)))


# --------------------------------------------------------------------- the host harness (g++)
_EXE = {}


def build_host_exe():
    """tests/host/fir_plan_check.cpp built by g++ from the library's own fir_plan.h (once per process)."""
    if "path" not in _EXE:
        src = os.path.join(ROOT, "tests", "host", "fir_plan_check.cpp")
        inc = os.path.join(ROOT, "openseize_amd", "csrc")
        path = os.path.join(tempfile.mkdtemp(), "fir_plan_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", inc, src, "-o", path])
        _EXE["path"] = path
    return _EXE["path"]


_KEYS = ("kernel", "rows", "pf", "piece", "taps", "step", "nblocks", "R", "nruns")


def host_plans(exe, cases):
    """[(ntaps, nch, cus, n)] -> per case the list of per-piece plans as the library's header makes them
    (dicts with _KEYS, kernel by name)."""
    text = "".join("%d %d %d %d\n" % c for c in cases)
    out = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, check=True).stdout
    plans = [[] for _ in cases]
    for line in out.splitlines():
        v = [int(t) for t in line.split()]
        p = dict(zip(_KEYS, v[1:]))
        p["kernel"] = ("nega", "pair")[p["kernel"]]
        plans[v[0]].append(p)
    assert all(plans)
    return plans


def host_grid(exe):
    """The seam invariant over the grid (see fir_plan_check.cpp); (cases checked, failures as text)."""
    res = subprocess.run([exe, "grid"], capture_output=True, text=True)
    lines = res.stdout.splitlines()
    return res.returncode, int(lines[-1].split()[1]) if lines and lines[-1].startswith("checked") else 0, lines[:20]


_NM_NEGA = re.compile(r"fir_nega_kernel<(\d+)>")
_NM_PAIR = re.compile(r"fir_oa_kernel<(\d+), (-?\d+), (\d+)>")


def compiled_cells(lib_path):
    """The cells compiled into the library, from `nm -C`; and the (NR, HPRE, PF) triples as compiled."""
    out = subprocess.check_output(["nm", "-C", lib_path], text=True)
    cells = {("nega", int(m.group(1))) for m in _NM_NEGA.finditer(out)}
    triples = {tuple(int(g) for g in m.groups()) for m in _NM_PAIR.finditer(out)}
    cells |= {("pair", nr, pf) for nr, _, pf in triples}
    return cells, triples


def pf_table():
    """OSZ_FIR_PF_TABLE of fir_pf_table.h: the variant of block heights 8 ... 15."""
    text = open(os.path.join(ROOT, "openseize_amd", "csrc", "fir_pf_table.h")).read()
    m = re.search(r"#define OSZ_FIR_PF_TABLE \{([^}]*)\}", text)
    vals = [int(v) for v in m.group(1).split(",")]
    assert len(vals) == 8
    return dict(zip(range(8, 16), vals))
