"""window_quantiles at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise,
2^21 samples per channel resident on the device, windows (W, step) = (1024, 1024), (1024, 512),
(256, 128) and (4096, 4096).

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  median        window_quantiles(measures="median") (one launch of csrc/windowquant.hip, one sort);
  median_mad    ("median", "mad"): the second sort;
  all           ("median", "mad", "quantile") with q = (0.25, 0.75, 0.9), one read of the stream;
  quantile      "quantile" alone, the same q;
  features      window_features(("min", "max")) on the same shape: the floor of one read of the stream;
  torch_median      the same numbers without it: x.unfold(-1, W, step), torch.sort of every window,
  torch_median_mad  indexing and the rule of the definition (a second sort of |x - median| for the
  torch_all         mad), batched so that the windows of one sort stay under 2 GiB;
  torch_quantile    torch.quantile(windows, q, dim=-1) in batches of at most 2^24 elements, the
                    largest input it accepts.
The torch contenders are timed on the first --torch-windows windows per channel count (all channels
of as many leading samples as hold that many windows) and scaled to all windows; their lines say how
many windows were measured.

One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For the library's contenders also the kernel's time by the library's HIP-event kernel
timer, taken in a run of its own, and from it
  compare_exchanges_per_s  windows x sorts x Wpad / 2 x log2 Wpad (log2 Wpad + 1) / 2 over the
                           kernel's time: what the bitonic network needs, pads included;
  share_of_valu_issue      the vector instructions of those compare-exchanges over what the chip
                           issues, 256 CUs x 4 SIMDs x 2.4 GHz x 64 lanes / 2 cycles.  Counted from
                           the compiled kernel: a compare-exchange inside a thread is v_cmp_u64 and
                           four v_cndmask_b32, five for two keys; one across lanes or waves is, for
                           each of its two keys, two cross-lane moves (or one ds_read_b64), a
                           v_mov_b32, v_cmp_u64 and two v_cndmask_b32, six.  The 64-bit compare is
                           counted as one issue slot like the others.
For `median`, `median_mad`, `all` and `quantile` the largest difference from the torch contender on
the windows that one measured, and whether every bit agrees.

    python benchmarks/quantiles_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/quantiles_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128), (4096, 4096))
KERNEL = b"window_quantiles"
QS = (0.25, 0.75, 0.9)
LANE_RATE = 256 * 4 * 2.4e9 * 64                # lane-instructions a second at one wave instruction a cycle and SIMD
BATCH_BYTES = 2 << 30
QUANTILE_MOST = 1 << 24                         # torch.quantile takes no larger input


def network(W, narrowest, wave):
    """(compare-exchanges, vector lane-instructions) of one sort of a window of W samples."""
    wpad = narrowest
    while wpad < W:
        wpad <<= 1
    K = wpad // (64 if W <= wave else 256)
    lg = wpad.bit_length() - 1
    inside = sum(min(s, K.bit_length() - 1) for s in range(1, lg + 1))       # stages of distance < K
    stages = lg * (lg + 1) // 2
    return wpad // 2 * stages, wpad // 2 * (5 * inside + 12 * (stages - inside))


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
    from openseize_amd.features import window_features, window_quantiles
    lib = _lib.load()
    n = 1 << a.log2n

    def median_of(s):
        W = s.shape[-1]
        return (s[:, (W - 1) // 2] + s[:, W // 2]) / 2.0

    def torch_route(measures):
        def route(x, W, step):
            w = x.unfold(-1, W, step).reshape(-1, W)                   # (windows, W)
            out = {f: [] for f in measures}
            per = max(1, BATCH_BYTES // (8 * W))
            for k in range(0, w.shape[0], per):
                v = w[k:k + per]
                s = v.sort(dim=-1).values
                med = median_of(s)
                if "median" in out:
                    out["median"].append(med)
                if "mad" in out:
                    out["mad"].append(median_of((v - med[:, None]).abs_().sort(dim=-1).values))
                if "quantile" in out:
                    planes = []
                    for p in QS:
                        h = p * (W - 1)
                        lo = int(h)
                        g, hi = h - lo, min(lo + 1, W - 1)
                        lo_v, hi_v = s[:, lo], s[:, hi]
                        d = hi_v - lo_v
                        lerp = lo_v + d * g if g < 0.5 else hi_v - d * (1.0 - g)
                        planes.append(torch.where(lo_v == hi_v, lo_v, lerp))
                    out["quantile"].append(torch.stack(planes))
            return {f: torch.cat(v, dim=-1) for f, v in out.items()}
        return route

    def torch_quantile(x, W, step):
        w = x.unfold(-1, W, step).reshape(-1, W)
        q = torch.tensor(QS, dtype=torch.float64, device=x.device)
        per = max(1, QUANTILE_MOST // W)
        return {"quantile": torch.cat([torch.quantile(w[k:k + per], q, dim=-1) for k in range(0, w.shape[0], per)],
                                      dim=-1)}

    def ours(measures):
        def route(x, W, step):
            got = window_quantiles(x, W, step, measures=measures, q=QS)[1]
            got = got if isinstance(got, dict) else {measures: got}
            return {f: v.reshape(v.shape[:-2] + (-1,)) for f, v in got.items()}        # (.., channel x window)
        return route

    def floor(x, W, step):
        return window_features(x, W, step, features=("min", "max"))[1]

    fns = {"median": ours("median"), "median_mad": ours(("median", "mad")),
           "all": ours(("median", "mad", "quantile")), "quantile": ours("quantile"), "features": floor,
           "torch_median": torch_route(("median",)), "torch_median_mad": torch_route(("median", "mad")),
           "torch_all": torch_route(("median", "mad", "quantile")), "torch_quantile": torch_quantile}
    against = {"median": "torch_median", "median_mad": "torch_median_mad", "all": "torch_all",
               "quantile": "torch_quantile"}
    sorts = {"median": 1, "median_mad": 2, "all": 2, "quantile": 1}

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
            nwin = (n - W) // step + 1
            for k, t in against.items():
                per = part(t, x, W, step)[1] // nch
                worst, same = 0.0, True
                for f, v in results[t].items():
                    got = results[k][f].reshape(-1, nch, nwin)[:, :, :per].reshape(v.shape)
                    worst = max(worst, float((got - v).abs().max()))
                    same = same and bool((got.view(torch.int64) == v.contiguous().view(torch.int64)).all())
                diffs[k, (W, step)] = (worst, same)
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
            for k in sorts:
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
                line = {"probe": "quantiles", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "windows": windows, "windows_measured": measured,
                        "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if (k, (W, step)) in kernels:
                    ms, launches, total = kernels[k, (W, step)]
                    line["timed_call_ms"] = round(ms, 3)
                    line["kernel_launches"] = launches
                    line["kernel_ms_per_chunk"] = round(total / chunks, 4)
                    if total:
                        ces, instrs = network(W, _lib.WQ_NARROWEST, _lib.WQ_WAVE)
                        line["compare_exchanges_per_s"] = float(f"{windows * sorts[k] * ces / (total * 1e-3):.4e}")
                        line["share_of_valu_issue"] = round(windows * sorts[k] * instrs / (total * 1e-3) / (LANE_RATE / 2),
                                                            4)
                if (k, (W, step)) in diffs:
                    line["max_diff_from_torch"] = float(f"{diffs[k, (W, step)][0]:.2e}")
                    line["same_bits_as_torch"] = diffs[k, (W, step)][1]
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
