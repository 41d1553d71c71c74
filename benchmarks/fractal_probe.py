"""window_fractal at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise,
2^21 samples per channel resident on the device, windows (W, step) = (1024, 1024), (1024, 512) and
(256, 128); kmax = 8 and the default scales, dfa_scales(W).

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  higuchi        window_fractal(measures="higuchi") (one launch of csrc/windowfrac.hip);
  dfa            window_fractal(measures="dfa");
  all            the five measures, one read of the stream;
  torch_higuchi  the same number without it: x.unfold(-1, W, step) and, for every k and m, the
                 strided slice w[:, m::k], its diff, abs and sum, then the centred slope;
  torch_dfa      the same number without it: cumsum of the unfolded windows less their means and,
                 per scale, a reshape into boxes with the closed-form line of each box, the mean
                 squared residual, then the centred slope.
The torch contenders are timed on the first --torch-windows windows of the data (all channels of as
many leading samples as hold that many windows) and scaled to all windows -- unfold with step < W
copies the stream, and every (k, m) and every scale is a pass over it through full-size
temporaries.  Their lines say how many windows were measured.

One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For the library's contenders also the kernel's time by the library's HIP-event kernel
timer, taken in a run of its own, and the share of the floor of the kernel's own compiled inner
loops (counted in the gfx950 assembly of windowfrac.hip):
  higuchi  a step -- one |x_{t+k} - x_t| a lane -- is 15 vector instructions, 3 of them float64 (the
           subtraction and the two accumulations; a wave's float64 instruction issues every 4
           cycles of a SIMD, a 32-bit one every 2: 36 cycles), and one ds_read_b64.  A wave takes
           ceil((W - k) / NT) steps for k = 1 .. kmax.
           share_of_valu_issue = wave steps / s x 36 cycles over 256 CUs x 4 SIMDs x 2.4 GHz;
  dfa      every scale reads its boxes twice and a box's first value once, the scan writes the
           profile once: 8-byte LDS accesses at 32 a cycle and CU (ds_read_b64, 256 B / clk).
           share_of_lds = accesses / s over 256 CUs x 32 x 2.4 GHz.
           The two loops over a box are 12 and 14 vector instructions a sample and lane, 6 and 8
           of them float64 (80 cycles for both), and one ds_read_b64 each: the vector unit, not the
           LDS, is the floor.  A window has sum over the scales of (W // n) n / 64 such wave steps
           if every lane is busy.  share_of_valu_issue as for higuchi, with 80 cycles.
For `higuchi` and `dfa` the largest difference from the torch contender on the windows that one
measured.

    python benchmarks/fractal_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/fractal_probe.jsonl]
"""

import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
KERNEL = b"window_fractal"
KMAX = 8
SIMD_RATE = 256 * 4 * 2.4e9                     # cycles of all SIMDs a second
LDS_RATE = 256 * 32 * 2.4e9                     # 8-byte LDS accesses a second
STEP_CYCLES = 36                                # a step of higuchi
BOX_CYCLES = 80                                 # a sample of dfa, both loops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-windows", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import dfa_scales, window_fractal
    lib = _lib.load()
    n = 1 << a.log2n

    def slope(u, v):
        du = u - u.mean()
        return (du * v).sum(-1) / (du * du).sum()

    def torch_higuchi(x, W, step):
        w = x.unfold(-1, W, step).reshape(-1, W)                   # (windows, W)
        lnL = []
        for k in range(1, KMAX + 1):
            L = 0
            for m in range(k):
                nmk = (W - 1 - m) // k
                L = L + w[:, m:m + nmk * k + 1:k].diff(dim=-1).abs().sum(-1) * (W - 1) / (nmk * k) / k
            lnL.append(torch.log(L / k))
        u = torch.log(1.0 / torch.arange(1, KMAX + 1, device=x.device, dtype=torch.float64))
        return {"higuchi": slope(u, torch.stack(lnL, -1))}

    def torch_dfa(x, W, step):
        w = x.unfold(-1, W, step).reshape(-1, W)
        y = (w - w.mean(-1, keepdim=True)).cumsum(-1)
        scales = dfa_scales(W)
        lnF = []
        for s in scales:
            nb = W // s
            box = y[:, :nb * s].reshape(-1, nb, s)
            ic = torch.arange(s, device=x.device, dtype=torch.float64) - 0.5 * (s - 1)
            line = (box * ic).sum(-1, keepdim=True) / (ic * ic).sum() * ic + box.mean(-1, keepdim=True)
            lnF.append(0.5 * torch.log(((box - line) ** 2).sum((1, 2)) / (nb * s)))
        u = torch.log(torch.tensor(scales, device=x.device, dtype=torch.float64))
        return {"dfa": slope(u, torch.stack(lnF, -1))}

    def ours(measures):
        def route(x, W, step):
            got = window_fractal(x, W, step, measures=measures, kmax=KMAX)[1]
            return got if isinstance(got, dict) else {measures: got}
        return route

    fns = {"higuchi": ours("higuchi"), "dfa": ours("dfa"), "all": ours(tuple(_lib.WINDOW_FRACTAL)),
           "torch_higuchi": torch_higuchi, "torch_dfa": torch_dfa}
    against = {"higuchi": "torch_higuchi", "dfa": "torch_dfa"}

    def timed(fn, x, W, step):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(x, W, step)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    def kernel_ms():
        launches, total = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.osz_profile_query(KERNEL, ctypes.byref(launches), ctypes.byref(total)))
        return launches.value, total.value

    def part(k, x, W, step):
        """What contender k is timed on, and the windows that holds."""
        nwin = (n - W) // step + 1
        if not k.startswith("torch"):
            return x, nwin * x.shape[0]
        per = max(1, min(nwin, a.torch_windows // x.shape[0]))
        return x[:, :(per - 1) * step + W], per * x.shape[0]

    def floors(W):
        """(wave steps of higuchi, LDS accesses of dfa, wave steps of dfa) of one window."""
        nt = 256 if W >= _lib.WR_WIDE else 64
        steps = (nt // 64) * sum(math.ceil((W - k) / nt) for k in range(1, KMAX + 1))
        lds = W + sum((W // s) * (2 * s + 1) for s in dfa_scales(W))
        return steps, lds, sum((W // s) * s for s in dfa_scales(W)) / 64.0

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        diffs = {}
        for W, step in SHAPES:                                      # warm-up of every shape
            results = {k: timed(fns[k], part(k, x, W, step)[0], W, step)[1] for k in fns}
            for k, t in against.items():
                per = part(t, x, W, step)[1] // nch
                diffs[k, (W, step)] = {f: float((results[k][f].reshape(nch, -1)[:, :per].reshape(-1) - v).abs().max())
                                       for f, v in results[t].items()}
            del results
            torch.cuda.empty_cache()
        times = {(k, s): [] for k in fns for s in SHAPES}
        for _ in range(a.runs):
            for W, step in SHAPES:
                for k in fns:
                    ms, out = timed(fns[k], part(k, x, W, step)[0], W, step)
                    del out
                    times[k, (W, step)].append(ms)
        kernels = {}
        for W, step in SHAPES:                                      # the kernel's time, in runs of their own
            for k in fns:
                if k.startswith("torch"):
                    continue
                _lib.check(lib.osz_profile_reset())
                _lib.check(lib.osz_profile_enable(1))
                ms, out = timed(fns[k], x, W, step)
                del out
                _lib.check(lib.osz_profile_enable(0))
                kernels[k, (W, step)] = (ms,) + kernel_ms()
        chunks = n / float(1 << 20)
        for W, step in SHAPES:
            windows = ((n - W) // step + 1) * nch
            steps, lds, boxsteps = floors(W)
            for k in fns:
                measured = part(k, x, W, step)[1]
                t = np.array(times[k, (W, step)]) * (windows / measured)
                line = {"probe": "fractal", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "windows": windows, "windows_measured": measured,
                        "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if (k, (W, step)) in kernels:
                    ms, launches, total = kernels[k, (W, step)]
                    line["timed_call_ms"] = round(ms, 3)
                    line["kernel_launches"] = launches
                    line["kernel_ms_per_chunk"] = round(total / chunks, 4)
                    if k == "higuchi" and total:
                        line["share_of_valu_issue"] = round(windows * steps * STEP_CYCLES / (total * 1e-3) / SIMD_RATE, 4)
                    if k == "dfa" and total:
                        line["share_of_lds"] = round(windows * lds / (total * 1e-3) / LDS_RATE, 4)
                        line["share_of_valu_issue"] = round(windows * boxsteps * BOX_CYCLES / (total * 1e-3) / SIMD_RATE, 4)
                if (k, (W, step)) in diffs:
                    line["max_diff_from_torch"] = {f: float(f"{v:.2e}") for f, v in diffs[k, (W, step)].items()}
                lines.append(line)
                print(json.dumps(line), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
