"""window_mutual_info at the sizes a user runs: 16, 64 and 256 channels, 2^21 float64 samples per
channel resident on the device (seeded normal noise, each channel mixed with its neighbour), windows
(W, step) = (1024, 1024), (1024, 512) and (256, 128), 4, 8 and 16 quantile bins.

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, five alternating runs of each in one process:
  ours_mi       window_mutual_info(x, W, step, "mi", bins) on the resident tensor;
  ours_all      the same call with all four measures (``counts`` is B^2 planes a window);
  torch_onehot  the same ``mi`` by PyTorch: ``x.unfold`` windows, ``torch.quantile`` edges (the same
                type-7 quantiles), ``torch.bucketize(right=True)``, one-hot float32 rows (exact up to
                2^24) and one batched ``torch.matmul`` of the (C B, W) rows with their transpose, then
                ``torch.xlogy`` and sums.
Every contender runs over the first windows whose results and temporaries stay under a byte budget
(4 GiB of results and 2e14 int8 multiply-adds of the Gram kernel for ours; 1 GiB of joint counts and
2^24 samples, torch.quantile's limit, for PyTorch) and its time is scaled to all windows; the share
is in the line.  One JSON line per contender, size, window shape and B: ms per
2^20-sample chunk (median and spread of the runs).  For ours, from a run of its own with the
library's kernel timers on: the edges (K17's kernel), code, Gram and finish kernels alone, their ms
per chunk and shares of the call; the Gram kernel's int8 multiply-adds -- (C Bp)(C Bp + 64) / 2 rows
pairs of its 64-row blocks times W rounded up to 64 -- against the int8 matrix peak, 2.5e15
multiply-adds a second (twice the bf16 rate); the finish's table reads, pairs x B^2 of 8 bytes,
against the LDS rate of ``ds_read_b64``, 256 B a clock and CU at 2.4 GHz.  ours_mi also carries the
largest difference of ``mi`` from the PyTorch route over the windows both hold.  No counter pass is
taken here.

    python benchmarks/mi_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/mi_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
BINS = (4, 8, 16)
PEAK_I8_MAC = 2.5e15
LDS_BYTES = 256 * 256 * 2.4e9
OURS_BYTES = 4 << 30
OURS_MACS = int(2e14)
TORCH_BYTES = 1 << 30
KERNELS = ("edges", "code", "gram", "finish")


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
    from openseize_amd.features import WINDOW_MI, window_mutual_info
    lib = _lib.load()
    n = 1 << a.log2n
    chunks = n / float(1 << 20)

    def ours(x, W, step, B, per, names):
        return window_mutual_info(x[:, :(per - 1) * step + W], W, step, measures=names, bins=B)[1]

    def torch_onehot(x, W, step, B, per):
        nch = x.shape[0]
        w = x[:, :(per - 1) * step + W].unfold(1, W, step).transpose(0, 1).contiguous()      # (per, C, W)
        q = torch.arange(1, B, dtype=torch.float64, device=x.device) / B
        edges = torch.quantile(w, q, dim=2).permute(1, 2, 0).contiguous()                     # (per, C, B - 1)
        code = torch.searchsorted(edges, w, right=True)                                        # (per, C, W)
        hot = torch.nn.functional.one_hot(code, B).to(torch.float32)                           # (per, C, W, B)
        rows = hot.permute(0, 1, 3, 2).reshape(per, nch * B, W)
        N = torch.matmul(rows, rows.transpose(1, 2)).to(torch.float64)                         # (per, C B, C B)
        N = N.reshape(per, nch, B, nch, B)
        p = N / W
        hij = -torch.xlogy(p, p).sum(dim=(2, 4))                                               # (per, C, C)
        h = torch.diagonal(hij, dim1=1, dim2=2)
        mi = (h[:, :, None] + h[:, None, :] - hij).clamp_min(0.0)
        idx = torch.arange(nch, device=x.device)
        mi[:, idx, idx] = h
        return mi

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
        npairs = nch * (nch - 1) // 2
        for W, step in SHAPES:
            nwin = (n - W) // step + 1
            wpad = -(-W // 64) * 64
            for B in a.bins:
                bp = 1 << (B - 1).bit_length()
                blocks = -(-nch * bp // 64)
                macs = blocks * (blocks + 1) // 2 * 64 * 64 * wpad          # of the Gram kernel, per window
                few = max(1, OURS_MACS // macs)
                per = {"ours_mi": min(nwin, few, max(1, OURS_BYTES // (8 * nch * nch))),
                       "ours_all": min(nwin, few, max(1, OURS_BYTES // (8 * nch * nch * (3 + B * B)))),
                       "torch_onehot": min(nwin, max(1, TORCH_BYTES // (8 * (nch * B) ** 2 + 4 * nch * B * W)),
                                           max(1, (1 << 24) // (nch * W)))}      # (torch.quantile takes 2^24 elements)
                fns = {"ours_mi": (ours, (x, W, step, B, per["ours_mi"], "mi")),
                       "ours_all": (ours, (x, W, step, B, per["ours_all"], tuple(WINDOW_MI))),
                       "torch_onehot": (torch_onehot, (x, W, step, B, per["torch_onehot"]))}
                # warm-up, and the agreement of the routes on the windows they share
                mine = timed(ours, *fns["ours_mi"][1])[1]
                theirs = timed(torch_onehot, *fns["torch_onehot"][1])[1]
                timed(ours, *fns["ours_all"][1])
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
                alone = {}
                for k in ("ours_mi", "ours_all"):                   # the kernels alone, in a run of their own
                    _lib.check(lib.osz_profile_reset())
                    _lib.check(lib.osz_profile_enable(1))
                    whole, out = timed(ours, *fns[k][1])
                    del out
                    _lib.check(lib.osz_profile_enable(0))
                    alone[k] = (whole, {name: kernel_ms(f"window_mi_{name}".encode()) for name in KERNELS})
                    torch.cuda.empty_cache()
                for k, t in times.items():
                    share = per[k] / nwin
                    t = np.array(t) / share
                    line = {"probe": "mi", "contender": k, "channels": nch, "samples": n, "winsize": W, "step": step,
                            "bins": B, "windows": nwin, "windows_timed_share": round(share, 6),
                            "runs_ms": [round(float(v), 3) for v in t],
                            "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                            "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                    if k in alone:
                        whole, parts = alone[k]
                        for name, (launches, ms) in parts.items():
                            line[f"{name}_ms_per_chunk"] = round(ms / share / chunks, 4)
                            line[f"{name}_share_of_the_call"] = round(ms / whole, 4)
                        line["gram_launches"] = parts["gram"][0]
                        line["gram_share_of_int8_peak"] = round(macs * per[k] / (parts["gram"][1] * 1e-3) / PEAK_I8_MAC, 5)
                        reads = 8.0 * npairs * B * B * per[k]
                        line["finish_share_of_lds_read_rate"] = round(reads / (parts["finish"][1] * 1e-3) / LDS_BYTES, 5)
                    if k == "ours_mi":
                        line["largest_difference_from_torch_onehot"] = agree
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
