"""window_features at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise,
2^21 samples per channel resident on the device, windows (W, step) = (1024, 1024), (1024, 512)
and (256, 128).

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  all          window_features with all thirteen features (one launch of csrc/windowfeat.hip);
  line_length  window_features with that one feature (the same kernel instance, one plane stored);
  torch        the same thirteen without it: x.unfold(-1, W, step) and torch reductions over the
               views, full-size temporaries for the differences and the Teager terms.
One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For the library's contenders also the kernel's time by the library's HIP-event kernel
timer, taken in a run of its own, and its share of the 8 TB/s HBM roofline at 8 B per sample (the
stream read once; with step < W the re-reads are meant to hit the caches).  For `all` the largest
difference of each feature from the torch contender, relative to the largest magnitude of the
feature.

    python benchmarks/features_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/features_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM = 8.0e12
SHAPES = ((1024, 1024), (1024, 512), (256, 128))
KERNEL = b"window_features"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=("all", "line_length", "torch"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import WINDOW_FEATURES, window_features
    lib = _lib.load()
    n = 1 << a.log2n

    def torch_route(x, W, step):
        w = x.unfold(-1, W, step)                                  # (C, nwin, W) view
        mean = w.mean(-1)
        d = w - mean[..., None]
        d2 = d * d
        m2, m3, m4 = d2.mean(-1), (d2 * d).mean(-1), (d2 * d2).mean(-1)
        del d, d2
        mn, mx = w.amin(-1), w.amax(-1)
        dx = x[:, 1:] - x[:, :-1]
        dw = dx.unfold(-1, W - 1, step)
        v1 = dw.var(-1, unbiased=False)
        ddx = dx[:, 1:] - dx[:, :-1]
        v2 = ddx.unfold(-1, W - 2, step).var(-1, unbiased=False)
        neg = x < 0
        mob = torch.sqrt(v1 / m2)
        return {"mean": mean, "var": m2, "rms": (w * w).mean(-1).sqrt(), "skew": m3 / m2 ** 1.5,
                "kurtosis": m4 / (m2 * m2), "min": mn, "max": mx, "ptp": mx - mn,
                "line_length": dw.abs().sum(-1),
                "zero_crossings": (neg[:, 1:] != neg[:, :-1]).unfold(-1, W - 1, step).sum(-1).double(),
                "mobility": mob, "complexity": torch.sqrt(v2 / v1) / mob,
                "teager": (x[:, 1:-1] ** 2 - x[:, :-2] * x[:, 2:]).unfold(-1, W - 2, step).mean(-1)}

    fns = {"all": lambda x, W, step: window_features(x, W, step, features=WINDOW_FEATURES)[1],
           "line_length": lambda x, W, step: window_features(x, W, step, features="line_length")[1],
           "torch": torch_route}

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

    names = [k for k in fns if a.only is None or k == a.only]
    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        diffs = {}
        for W, step in SHAPES:                                      # warm-up of every shape
            results = {k: timed(fns[k], x, W, step)[1] for k in names}
            if "all" in results and "torch" in results:
                diffs[W, step] = {f: float((results["all"][f] - results["torch"][f]).abs().max()
                                           / results["torch"][f].abs().max()) for f in WINDOW_FEATURES}
            del results
            torch.cuda.empty_cache()
        times = {(k, s): [] for k in names for s in SHAPES}
        for _ in range(a.runs):
            for W, step in SHAPES:
                for k in names:
                    ms, out = timed(fns[k], x, W, step)
                    del out
                    times[k, (W, step)].append(ms)
        kernels = {}
        for W, step in SHAPES:                                      # the kernel's time, in runs of their own
            for k in names:
                if k == "torch":
                    continue
                _lib.check(lib.osz_profile_reset())
                _lib.check(lib.osz_profile_enable(1))
                ms, out = timed(fns[k], x, W, step)
                del out
                _lib.check(lib.osz_profile_enable(0))
                kernels[k, (W, step)] = (ms,) + kernel_ms()
        chunks = n / float(1 << 20)
        for W, step in SHAPES:
            for k in names:
                t = np.array(times[k, (W, step)])
                line = {"probe": "features", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "windows": (n - W) // step + 1,
                        "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if (k, (W, step)) in kernels:
                    ms, launches, total = kernels[k, (W, step)]
                    line["timed_call_ms"] = round(ms, 3)
                    line["kernel_launches"] = launches
                    line["kernel_ms_per_chunk"] = round(total / chunks, 4)
                    if total:
                        line["kernel_share_of_hbm_roofline"] = round(8.0 * nch * n / (total * 1e-3) / PEAK_HBM, 4)
                if k == "all" and (W, step) in diffs:
                    line["max_rel_diff_from_torch"] = {f: float(f"{v:.2e}") for f, v in diffs[W, step].items()}
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
