"""Sweep of FIR lengths x scipy designs through the chain planners (tests/host/spec_host_check.cpp,
built by g++ from the library's own spec_tables.h): which compiled chain-kernel instance ("cell")
each (FIR, cascade) pair lands on, and one representative design per cell, printed as the
CORPUS block of tests/chain_cells.py.  Not collected by pytest (run it by hand:
``python tests/chain_cell_sweep.py [--jobs N]``); it needs g++ only.

A representative is the design with the best-conditioned fit of its cell whose plan does not
change when the FIR is one tap longer or shorter or the cut-off moves by 0.005 (not at a plan
boundary)."""

import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chain_cells as cc  # noqa: E402

TAPS = [2, 33, 64, 129, 257, 300, 400, 513, 640, 769, 900, 1025, 1100, 1200, 1281, 1400, 1537, 1650,
        1793, 1850, 1950, 2048]
FAST_WN = [0.05, 0.1, 0.2, 0.3, 0.45]
SLOW_WN = [0.004, 0.008, 0.015, 0.025, 0.035]
BANDS = [(0.05, 0.3), (0.1, 0.2), (0.2, 0.4), (0.3, 0.6), (0.02, 0.1), (0.01, 0.05), (0.005, 0.03),
         (0.04, 0.08), (0.15, 0.17)]
KINDS = [("butter", ()), ("cheby1", (1.0,)), ("cheby1", (0.1,)), ("cheby1", (3.0,)), ("cheby2", (40.0,)),
         ("cheby2", (60.0,)), ("cheby2", (80.0,)), ("ellip", (0.5, 50.0)), ("ellip", (0.1, 70.0)),
         ("ellip", (1.0, 80.0))]


def designs():
    for kind, rip in KINDS:
        for order in range(1, 21):          # (more than 16: nine sections and up, the time scan's own)
            for btype in ("lowpass", "highpass"):
                for wn in FAST_WN + SLOW_WN:
                    yield (kind, order, rip, wn, btype)
        for order in range(1, 11):
            for btype in ("bandpass", "bandstop"):
                for wn in BANDS:
                    yield (kind, order, rip, wn, btype)


def plan_of(args):
    exe, taps_n, cutoff, design = args
    try:
        sos = cc.design_sos(*design)
    except Exception:
        return None
    if not np.all(np.isfinite(sos)) or len(sos) > 32:
        return None
    return (taps_n, cutoff, design, cc.host_plan(exe, cc.fir_taps(taps_n, cutoff), sos))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    exe = cc.build_host_exe()
    work = [(exe, t, 0.2, d) for t in TAPS for d in designs()]
    best = {}                                            # cell -> (ratio, taps, cutoff, design)
    with Pool(a.jobs) as pool:
        for res in pool.imap_unordered(plan_of, work, chunksize=32):
            if res is None:
                continue
            taps_n, cutoff, design, p = res
            for cell, ratio in cc.cells_of_plan(p, taps_n):
                if cell not in best or ratio > best[cell][0]:
                    # (not at a plan boundary: the neighbours land on the same cell)
                    near = [cc.host_plan(exe, cc.fir_taps(t, c), cc.design_sos(*design))
                            for t, c in ((taps_n + 1, cutoff), (max(2, taps_n - 1), cutoff),
                                         (taps_n, cutoff + 0.005))] if taps_n > 2 else []
                    if all(cell in [c for c, _ in cc.cells_of_plan(q, taps_n)] for q in near):
                        best[cell] = (ratio, taps_n, cutoff, design)
    print(f"# {len(best)} cells from {len(work)} (FIR, design) pairs")
    print("CORPUS = [")
    for cell in sorted(best):
        ratio, taps_n, cutoff, design = best[cell]
        print(f"    Cell({cell!r}, {taps_n}, {cutoff}, {design!r}, {ratio:.3e}),")
    print("]")


if __name__ == "__main__":
    main()
