"""window_ar at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise, 2^21
samples per channel resident on the device, windows (W, step) = (1024, 1024), (1024, 512) and
(256, 128); orders 8 and 32, both methods, measures ("coefficients", "error").

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  burg8, burg32        window_ar(method="burg", order=8 / 32) (one launch of csrc/windowar.hip);
  yw8, yw32            window_ar(method="yule_walker", order=8 / 32);
  features2            window_features(features=("mean", "var")): what one read of the stream costs;
  torch_burg8, torch_burg32  the same numbers without the kernel: x.unfold(-1, W, step), the mean
                       taken off, and per order the products f b, f f and b b, their sums over the
                       window, k, and the two updated error arrays as new tensors; the Levinson
                       step on (windows, m) tensors.
The torch contenders are timed on the first --torch-windows windows of the data (all channels of as
many leading samples as hold that many windows) and scaled to all windows -- unfold with step < W
copies the stream, and every order is several passes over it through full-size temporaries.  Their
lines say how many windows were measured.

One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For the library's contenders also the kernel's time by the library's HIP-event kernel
timer, taken in a run of its own.  For burg also the shares of two floors, both counted in the
gfx950 assembly of windowar.hip, where an order of a wave that holds R slots a lane is 5 R + 30
float64 instructions with 256 threads (5 R + 24 in a one-wave workgroup) -- 5 R fused multiply-adds
(num, the two of den, the two updates), 12 additions of the two wave sums, the division's 11, and with
256 threads the 6 additions over the waves -- and 37 32-bit ones (28 DPP moves among them), 2 R
more in the one wave that zeroes the slot an order retires; a wave's float64 instruction issues
every 4 cycles of a SIMD, a 32-bit one every 2:
  share_of_fma_floor   the 5 R fused multiply-adds alone, 20 R cycles an order and wave, over the
                       kernel's time on 256 CUs x 4 SIMDs x 2.4 GHz: what the recursion itself needs;
  share_of_valu_issue  every vector instruction of the order loop, 4 (5 R + 30) + 2 x 37 cycles (4 (5 R
                       + 24) + 2 (37 + 2 R) in a one-wave workgroup), over the same: what the
                       compiled loop needs if nothing ever waits.
For burg8 and burg32 the largest difference from the torch contender on the windows that one
measured.

    python benchmarks/ar_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/ar_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
KERNEL = b"window_ar"
MEASURES = ("coefficients", "error")
SIMD_RATE = 256 * 4 * 2.4e9                     # cycles of all SIMDs a second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-windows", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import window_ar, window_features
    lib = _lib.load()
    n = 1 << a.log2n

    def torch_burg(p):
        def route(x, W, step):
            w = x.unfold(-1, W, step).reshape(-1, W)                # (windows, W)
            w = w - w.mean(-1, keepdim=True)
            E = (w * w).sum(-1) / W
            f, b = w[:, 1:], w[:, :-1]                              # f_t and b_{t-1}, t = m .. W - 1
            coef = w.new_zeros((w.shape[0], 0))
            for m in range(1, p + 1):
                k = (-2.0 * (f * b).sum(-1) / ((f * f).sum(-1) + (b * b).sum(-1)))[:, None]
                f, b = (f + k * b)[:, 1:], (b + k * f)[:, :-1]
                coef = torch.cat((coef + k * coef.flip(-1), k), dim=-1)
                E = E * (1.0 - k[:, 0] * k[:, 0])
            return {"coefficients": coef.T, "error": E}
        return route

    def ours(method, p):
        def route(x, W, step):
            return window_ar(x, W, step, measures=MEASURES, order=p, method=method)[1]
        return route

    def features2(x, W, step):
        return window_features(x, W, step, features=("mean", "var"))[1]

    fns = {"burg8": ours("burg", 8), "burg32": ours("burg", 32), "yw8": ours("yule_walker", 8),
           "yw32": ours("yule_walker", 32), "features2": features2, "torch_burg8": torch_burg(8),
           "torch_burg32": torch_burg(32)}
    against = {"burg8": "torch_burg8", "burg32": "torch_burg32"}
    orders = {"burg8": 8, "burg32": 32}

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

    def floors(W, p):
        """(cycles of the fused multiply-adds, cycles of every vector instruction) of one window's
        order loop, all its waves."""
        nt = 256 if W >= _lib.AR_WIDE else 64
        R = 1
        while nt * R < W:
            R *= 2
        waves = nt // 64
        every = 4 * (5 * R + 30) + 2 * 37 if waves > 1 else 4 * (5 * R + 24) + 2 * (37 + 2 * R)
        return p * waves * 20 * R, p * waves * every

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        diffs = {}
        for W, step in SHAPES:                                      # warm-up of every shape
            results = {k: timed(fns[k], part(k, x, W, step)[0], W, step)[1] for k in fns}
            for k, t in against.items():
                per = part(t, x, W, step)[1] // nch
                diffs[k, (W, step)] = {
                    f: float((results[k][f].reshape(-1, nch, results[k][f].shape[-1])[:, :, :per].reshape(-1, nch * per)
                              - v.reshape(-1, nch * per)).abs().max()) for f, v in results[t].items()}
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
                if k.startswith("torch") or k == "features2":
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
                line = {"probe": "ar", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "windows": windows, "windows_measured": measured,
                        "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if (k, (W, step)) in kernels:
                    ms, launches, total = kernels[k, (W, step)]
                    line["timed_call_ms"] = round(ms, 3)
                    line["kernel_launches"] = launches
                    line["kernel_ms_per_chunk"] = round(total / chunks, 4)
                    if k in orders and total:
                        fma, every = floors(W, orders[k])
                        line["share_of_fma_floor"] = round(windows * fma / (total * 1e-3) / SIMD_RATE, 4)
                        line["share_of_valu_issue"] = round(windows * every / (total * 1e-3) / SIMD_RATE, 4)
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
