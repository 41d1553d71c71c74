"""window_transfer_entropy at the sizes a user runs: 16, 64 and 256 channels, 2^21 float64 samples
per channel resident on the device (seeded normal noise, each channel mixed with its neighbour),
windows (W, step) = (1024, 1024), (1024, 512) and (256, 128), 4 and 8 quantile bins, lag 1.

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, five alternating runs of each in one process:
  ours_te       window_transfer_entropy(x, W, step, "te", bins, lag) on the resident tensor;
  ours_mi       window_mutual_info(x, W, step, "mi", bins) over the same windows: K26's Gram kernel
                does 2 Bp times K25's multiply-adds (the full rectangle of Bp^2 against Bp rows a
                channel, where K25 does the upper triangle of Bp against Bp);
  torch_onehot  the same ``te`` by PyTorch: ``x.unfold`` windows, ``torch.quantile`` edges (the same
                type-7 quantiles), ``torch.searchsorted(right=True)``, one-hot float32 rows (exact up
                to 2^24) of the (bin now, bin before) symbols and of the bins, one batched
                ``torch.matmul`` of the (C B^2, T) rows with the (C B, T) rows transposed, then
                ``torch.xlogy`` and sums.
Every contender runs over the first windows whose results and temporaries stay under a budget (4 GiB
of results and 4e13 int8 multiply-adds of the Gram kernel for ours; 1 GiB of one-hot rows and counts
and 2^24 samples, torch.quantile's limit, for PyTorch) and its time is scaled to all windows; the
share is in the line.  One JSON line per contender, size, window shape and B: ms per 2^20-sample
chunk (median and spread of the runs).  For ours_te, from a run of its own with the library's kernel
timers on: the edges (K17's kernel) and the four steps -- code, symbol, Gram and finish kernels --
alone, their ms per chunk and shares of the call; the Gram kernel's int8 multiply-adds -- the 64 x 64
blocks of (C Bp^2) x (C Bp) rows times T rounded up to 64 -- against the int8 matrix peak, 2.5e15
multiply-adds a second; and the largest difference of ``te`` from the PyTorch route over the windows
both hold.  No counter pass is taken here.

    python benchmarks/te_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/te_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
BINS = (4, 8)
LAG = 1
PEAK_I8_MAC = 2.5e15
OURS_BYTES = 4 << 30
OURS_MACS = int(4e13)
TORCH_BYTES = 1 << 30
KERNELS = ("edges", "code", "symbol", "gram", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--bins", type=int, nargs="+", default=list(BINS))
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import window_mutual_info, window_transfer_entropy
    lib = _lib.load()
    n = 1 << a.log2n
    chunks = n / float(1 << 20)

    def ours_te(x, W, step, B, per):
        return window_transfer_entropy(x[:, :(per - 1) * step + W], W, step, measures="te", bins=B, lag=LAG)[1]

    def ours_mi(x, W, step, B, per):
        return window_mutual_info(x[:, :(per - 1) * step + W], W, step, measures="mi", bins=B)[1]

    def torch_onehot(x, W, step, B, per):
        nch, T = x.shape[0], W - LAG
        w = x[:, :(per - 1) * step + W].unfold(1, W, step).transpose(0, 1).contiguous()      # (per, C, W)
        q = torch.arange(1, B, dtype=torch.float64, device=x.device) / B
        edges = torch.quantile(w, q, dim=2).permute(1, 2, 0).contiguous()                     # (per, C, B - 1)
        code = torch.searchsorted(edges, w, right=True)                                        # (per, C, W)
        symbol = code[:, :, LAG:] * B + code[:, :, LAG - 1:W - 1]                              # (per, C, T)
        target = torch.nn.functional.one_hot(symbol, B * B).to(torch.float32)                  # (per, C, T, B^2)
        source = torch.nn.functional.one_hot(code[:, :, :T], B).to(torch.float32)              # (per, C, T, B)
        target = target.permute(0, 1, 3, 2).reshape(per, nch * B * B, T)
        source = source.permute(0, 1, 3, 2).reshape(per, nch * B, T)
        N = torch.matmul(target, source.transpose(1, 2)).to(torch.float64)                     # (per, C B^2, C B)
        N = N.reshape(per, nch, B, B, nch, B)                                                  # [k, j, a, b, i, c]
        nab, nbc, nb = N.sum(dim=5), N.sum(dim=2), N.sum(dim=(2, 5))
        s3, sab = torch.xlogy(N, N).sum(dim=(2, 3, 5)), torch.xlogy(nab, nab).sum(dim=(2, 3))
        sbc, sb = torch.xlogy(nbc, nbc).sum(dim=(2, 4)), torch.xlogy(nb, nb).sum(dim=2)
        te = (((s3 - sab) - (sbc - sb)) / T).clamp_min(0.0).transpose(1, 2).contiguous()       # (per, i, j)
        idx = torch.arange(nch, device=x.device)
        te[:, idx, idx] = 0.0
        return te

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
        x[1:] += 0.7 * x[:-1].clone()
        for W, step in SHAPES:
            nwin = (n - W) // step + 1
            tpad = -(-(W - LAG) // 64) * 64
            for B in a.bins:
                bp = 1 << (B - 1).bit_length()
                macs = -(-nch * bp * bp // 64) * -(-nch * bp // 64) * 64 * 64 * tpad    # of the Gram kernel, per window
                few = min(nwin, max(1, OURS_MACS // macs), max(1, OURS_BYTES // (8 * nch * nch)))
                heavy = 16 * nch * B * B * W + 24 * nch * nch * B ** 3                   # PyTorch's bytes per window
                per = {"ours_te": few, "ours_mi": few,
                       "torch_onehot": min(nwin, max(1, TORCH_BYTES // heavy), max(1, (1 << 24) // (nch * W)))}
                fns = {"ours_te": (ours_te, (x, W, step, B, per["ours_te"])),
                       "ours_mi": (ours_mi, (x, W, step, B, per["ours_mi"])),
                       "torch_onehot": (torch_onehot, (x, W, step, B, per["torch_onehot"]))}
                # warm-up, and the agreement of the routes on the windows they share
                mine = timed(ours_te, *fns["ours_te"][1])[1]
                theirs = timed(torch_onehot, *fns["torch_onehot"][1])[1]
                timed(ours_mi, *fns["ours_mi"][1])
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
                _lib.check(lib.osz_profile_reset())                 # the kernels alone, in a run of their own
                _lib.check(lib.osz_profile_enable(1))
                whole, out = timed(ours_te, *fns["ours_te"][1])
                del out
                _lib.check(lib.osz_profile_enable(0))
                parts = {name: kernel_ms(f"window_te_{name}".encode()) for name in KERNELS}
                torch.cuda.empty_cache()
                for k, t in times.items():
                    share = per[k] / nwin
                    t = np.array(t) / share
                    line = {"probe": "te", "contender": k, "channels": nch, "samples": n, "winsize": W, "step": step,
                            "bins": B, "lag": LAG, "windows": nwin, "windows_timed_share": round(share, 6),
                            "runs_ms": [round(float(v), 3) for v in t],
                            "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                            "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                    if k == "ours_te":
                        for name, (launches, ms) in parts.items():
                            line[f"{name}_ms_per_chunk"] = round(ms / share / chunks, 4)
                            line[f"{name}_share_of_the_call"] = round(ms / whole, 4)
                        line["gram_launches"] = parts["gram"][0]
                        line["gram_share_of_int8_peak"] = round(macs * per[k] / (parts["gram"][1] * 1e-3) / PEAK_I8_MAC, 5)
                        line["largest_difference_from_torch_onehot"] = agree
                    lines.append(line)
                    print(json.dumps(line), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
