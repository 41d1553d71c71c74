"""window_granger at the sizes a user runs: 16, 64 and 256 channels, 2^21 float64 samples per channel
resident on the device (seeded normal noise, each channel mixed with its neighbour delayed by three
samples), windows (W, step) = (1024, 1024), (1024, 512) and (256, 128), order 8 and 16.

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, alternating runs of each in one process:
  ours         window_granger(x, W, step, "granger", order) on the resident tensor;
  torch_solve  the same numbers by PyTorch from ``window_xcorr(..., "xcorr", maxlag=p,
               normalize=False)``: the 2p x 2p block-Toeplitz matrix of every pair and the p x p
               Toeplitz matrix of every channel assembled with one indexing expression each, batched
               torch.linalg.solve, the error covariances and the logarithms.
Every contender runs over the first windows whose results and temporaries stay under a byte budget
(4 GiB of results for ours, 2 GiB for the block-Toeplitz matrices) and its time is scaled to all
windows; the share is in the line.  One JSON line per contender, size, window shape and order: ms
per 2^20-sample chunk (median and spread of the runs).  For ours, from a run of its own with the
library's kernel timers on, the Gram kernel (xcorr_gram_kernel) and the pair kernel
(granger_pair_kernel, csrc/windowgranger.hip) alone: their ms per chunk, the pair kernel's share of
the call, and its rate against the float64 vector issue rate, counting the float64 multiplies and
fused multiply-adds of the compiled recursion -- 24 per (m, k) of the inner sweep, (p - 1)(p - 2) / 2
of them, and 52 per order -- per pair i < j and window against 39.3e12 lanes a second.  ours also
carries the largest difference of ``granger`` from the PyTorch route over the windows both hold.

    python benchmarks/granger_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/granger_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
ORDERS = (8, 16)
PEAK_FMA = 39.3e12
OURS_BYTES = 4 << 30
TORCH_BYTES = 2 << 30


def pair_ops(p):
    """The float64 vector multiplies and fused multiply-adds of one pair's block recursion."""
    return 24 * (p - 1) * (p - 2) // 2 + 52 * p - 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import window_granger, window_xcorr
    lib = _lib.load()
    n = 1 << a.log2n
    chunks = n / float(1 << 20)

    def ours(x, W, step, p, per):
        return window_granger(x[:, :(per - 1) * step + W], W, step, measures="granger", order=p)[1]

    def torch_solve(x, W, step, p, per):
        nch = x.shape[0]
        r = window_xcorr(x[:, :(per - 1) * step + W], W, step, measures="xcorr", maxlag=p, normalize=False)[1]
        pair = torch.triu_indices(nch, nch, 1, device=x.device)              # (2, npairs): i and j
        u = torch.arange(2 * p, device=x.device)
        # R[2 q + a, 2 l + b] = C(l - q)_ab = r_{pair[b] pair[a]}(l - q); the lag axis of r starts at -p
        lag = (p + u[None, :] // 2 - u[:, None] // 2)[None]                   # (1, 2p, 2p)
        first, second = pair[u % 2].T[:, None, :], pair[u % 2].T[:, :, None]  # (npairs, 1, 2p), (npairs, 2p, 1)
        R = r[:, lag, first, second]                                          # (per, npairs, 2p, 2p)
        ab = torch.arange(2, device=x.device)
        rhs = r[:, (p + 1 + u // 2)[None, None, :], pair[u % 2].T[:, None, :], pair[ab].T[:, :, None]]   # (per, npairs, 2, 2p)
        A = torch.linalg.solve(R.transpose(-1, -2), rhs.transpose(-1, -2)).transpose(-1, -2)
        c0 = r[:, p][:, pair[ab].T[:, None, :], pair[ab].T[:, :, None]]       # C(0)_ab = r_ba(0)
        S = c0 - A @ rhs.transpose(-1, -2)                                    # sum_q A_q C(q)^T
        q = torch.arange(p, device=x.device)
        auto = torch.diagonal(r[:, p:], dim1=-2, dim2=-1).transpose(1, 2)     # (per, C, p + 1): r_cc(0 .. p)
        T = auto[:, :, (q[:, None] - q[None, :]).abs()]
        coef = torch.linalg.solve(T, auto[:, :, 1:, None])[..., 0]
        E = auto[:, :, 0] - (coef * auto[:, :, 1:]).sum(-1)
        F = torch.zeros((per, nch, nch), dtype=torch.float64, device=x.device)
        F[:, pair[0], pair[1]] = torch.log(E[:, pair[1]] / S[:, :, 1, 1])
        F[:, pair[1], pair[0]] = torch.log(E[:, pair[0]] / S[:, :, 0, 0])
        return F

    def timed(fn, *args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(*args)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    def kernel_ms(name):
        launches, total = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.osz_profile_query(name, ctypes.byref(launches), ctypes.byref(total)))
        return launches.value, total.value

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        x[1:] += 0.7 * torch.roll(x[:-1].clone(), 3, dims=1)
        npairs = nch * (nch - 1) // 2
        for W, step in SHAPES:
            nwin = (n - W) // step + 1
            for p in ORDERS:
                per = {"ours": min(nwin, max(1, OURS_BYTES // (8 * nch * nch))),
                       "torch_solve": min(nwin, max(1, TORCH_BYTES // (8 * npairs * 4 * p * p)))}
                fns = {"ours": (ours, (x, W, step, p, per["ours"])),
                       "torch_solve": (torch_solve, (x, W, step, p, per["torch_solve"]))}
                # warm-up, and the agreement of the routes on the windows they share
                mine = timed(ours, *fns["ours"][1])[1]
                theirs = timed(torch_solve, *fns["torch_solve"][1])[1]
                k = min(mine.shape[0], theirs.shape[0])
                agree = float((mine[:k] - theirs[:k]).abs().max())
                del mine, theirs
                torch.cuda.empty_cache()
                times = {k: [] for k in fns}
                for _ in range(a.runs):
                    for k, (fn, args) in fns.items():
                        ms, out = timed(fn, *args)
                        del out
                        times[k].append(ms)
                _lib.check(lib.osz_profile_reset())                           # the kernels alone, in a run of its own
                _lib.check(lib.osz_profile_enable(1))
                whole, out = timed(ours, *fns["ours"][1])
                del out
                _lib.check(lib.osz_profile_enable(0))
                gram, pairk = kernel_ms(b"window_granger_gram"), kernel_ms(b"window_granger_pair")
                torch.cuda.empty_cache()
                for k, t in times.items():
                    share = per[k] / nwin
                    t = np.array(t) / share
                    line = {"probe": "granger", "contender": k, "channels": nch, "samples": n, "winsize": W, "step": step,
                            "order": p, "windows": nwin, "windows_timed_share": round(share, 6),
                            "runs_ms": [round(float(v), 3) for v in t],
                            "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                            "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                    if k == "ours":
                        ops = pair_ops(p) * npairs * per[k]
                        line.update(gram_launches=gram[0], gram_ms_per_chunk=round(gram[1] / share / chunks, 4),
                                    pair_ms_per_chunk=round(pairk[1] / share / chunks, 4),
                                    pair_share_of_the_call=round(pairk[1] / whole, 4),
                                    pair_over_gram=round(pairk[1] / gram[1], 4),
                                    pair_ops_per_pair=pair_ops(p),
                                    pair_share_of_fp64_vector_rate=round(ops / (pairk[1] * 1e-3) / PEAK_FMA, 4),
                                    largest_difference_from_torch_solve=agree)
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
