"""window_entropy at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise,
2^21 samples per channel resident on the device, windows (W, step) = (1024, 1024) and (256, 128).

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  sample        window_entropy(measures="sample"), m = 2, r = 0.2 (one launch of csrc/windowent.hip);
  permutation3  window_entropy(measures="permutation"), order 3;
  permutation5  the same at order 5;
  both          ("sample", "permutation") at order 3, one read of the stream;
  torch_sample  sample entropy without it: x.unfold(-1, W, step), the Chebyshev distance of every
                pair of templates from a broadcast (windows, W, W) difference, batched so that the
                difference stays under 2 GiB, and a count;
  torch_perm3   permutation entropy without it: unfold twice, a stable argsort of the argsort for
  torch_perm5   the ranks, one bincount over (window, pattern); batched under 2 GiB of ranks.
The torch contenders are timed on the first --torch-windows windows of the data (all channels of
as many leading samples as hold that many windows) and scaled to all windows: at 256 channels the
whole of `torch_sample` is 5 10^11 pair tests through several full-size temporaries.  Their lines
say how many windows were measured.

One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For the library's contenders also the kernel's time by the library's HIP-event kernel
timer, taken in a run of its own.  For `sample` the pair tests per second -- a pair test is one
|x_t - x_{t+L}| <= rho, sum over the lags L = 1 .. W - m - 1 of W - L of them a window -- and two
shares of what the vector unit can issue.  The compiled inner loop spends six vector instructions
on a pair test per lane: v_add_f64 and v_cmp_le_f64 (float64: a wave's instruction every 4 cycles
of a SIMD, half the float32 rate, as the 78.6 TFLOP/s float64 vector peak says), v_cmp_le_i32,
v_add_u32 and v_cndmask_b32 for the run length and, per two pair tests, a v_cndmask_b32 and a
v_addc_co_u32 for the count B (every 2 cycles each); the count A is three scalar instructions.
  share_of_f64_issue   pair tests / s over 256 CUs x 4 SIMDs x 2.4 GHz x 64 lanes / 8 cycles;
  share_of_valu_issue  the same over 16 cycles, all six instructions.
For `sample` and `permutation3` the largest difference from the torch contender on the windows
that one measured (the counts A and B themselves for `sample`).

    python benchmarks/entropy_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/entropy_probe.jsonl]
"""

import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (256, 128))
KERNEL = b"window_entropy"
M, R_STD = 2, 0.2
LANE_RATE = 256 * 4 * 2.4e9 * 64                # lane-instructions a second at one wave instruction a cycle and SIMD
BATCH_BYTES = 2 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-windows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import window_entropy
    lib = _lib.load()
    n = 1 << a.log2n

    def torch_sample(x, W, step):
        w = x.unfold(-1, W, step).reshape(-1, W)                   # (windows, W)
        N = W - M
        A, B = [], []
        for k in range(0, w.shape[0], max(1, BATCH_BYTES // (8 * W * W))):
            v = w[k:k + max(1, BATCH_BYTES // (8 * W * W))]
            rho = R_STD * v.std(-1, unbiased=False)
            match = (v[:, :, None] - v[:, None, :]).abs_() <= rho[:, None, None]
            both = match[:, :N, :N] & match[:, 1:N + 1, 1:N + 1]
            B.append((both.sum((1, 2)) - N) // 2)                  # (the matrix is symmetric, its diagonal set)
            both &= match[:, 2:N + 2, 2:N + 2]
            A.append((both.sum((1, 2)) - N) // 2)
        A, B = torch.cat(A).double(), torch.cat(B).double()
        return {"sample": -torch.log(A / B), "sample_a": A, "sample_b": B}

    def torch_perm(order):
        def route(x, W, step):
            w = x.unfold(-1, W, step).reshape(-1, W)
            nvec, bins = W - order + 1, order ** order
            weights = order ** torch.arange(order, device=x.device)
            out = []
            per = max(1, BATCH_BYTES // (8 * nvec * order))
            for k in range(0, w.shape[0], per):
                vec = w[k:k + per].unfold(-1, order, 1)            # (windows, nvec, order)
                ranks = vec.argsort(dim=-1, stable=True).argsort(dim=-1, stable=True)
                code = (ranks * weights).sum(-1) + bins * torch.arange(vec.shape[0], device=x.device)[:, None]
                p = torch.bincount(code.reshape(-1), minlength=bins * vec.shape[0]).reshape(-1, bins).double() / nvec
                out.append(-torch.xlogy(p, p).sum(-1) / math.log(2.0) / math.log2(math.factorial(order)))
            return {"permutation": torch.cat(out)}
        return route

    def ours(measures, order=3):
        def route(x, W, step):
            got = window_entropy(x, W, step, measures=measures, m=M, r=R_STD, order=order)[1]
            return got if isinstance(got, dict) else {measures: got}
        return route

    fns = {"sample": ours(("sample", "sample_a", "sample_b")), "permutation3": ours("permutation", 3),
           "permutation5": ours("permutation", 5), "both": ours(("sample", "permutation"), 3),
           "torch_sample": torch_sample, "torch_perm3": torch_perm(3), "torch_perm5": torch_perm(5)}
    against = {"sample": "torch_sample", "permutation3": "torch_perm3"}

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
            for k in fns:
                measured = part(k, x, W, step)[1]
                t = np.array(times[k, (W, step)]) * (windows / measured)
                line = {"probe": "entropy", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "windows": windows, "windows_measured": measured,
                        "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if (k, (W, step)) in kernels:
                    ms, launches, total = kernels[k, (W, step)]
                    line["timed_call_ms"] = round(ms, 3)
                    line["kernel_launches"] = launches
                    line["kernel_ms_per_chunk"] = round(total / chunks, 4)
                    if k == "sample" and total:
                        tests = windows * sum(W - lag for lag in range(1, W - M))
                        line["pair_tests_per_s"] = float(f"{tests / (total * 1e-3):.4e}")
                        line["share_of_f64_issue"] = round(tests / (total * 1e-3) / (LANE_RATE / 8), 4)
                        line["share_of_valu_issue"] = round(tests / (total * 1e-3) / (LANE_RATE / 16), 4)
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
