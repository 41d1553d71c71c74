"""window_wavelet at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise,
2^21 samples per channel resident on the device, windows (W, step) = (1024, 1024), (1024, 512) and
(256, 128); db4 and the default level, wavelet_level(W, 8).

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  rel_ent     window_wavelet(features=("relative", "entropy")) (one launch of csrc/windowwave.hip);
  all         the five features, one read of the stream;
  torch       relative and entropy without it: x.unfold(-1, W, step) less the windows' means and, per
              level, a circular pad by L - 2 and one strided conv1d with the two filters, the bands'
              sums of squares, then the ratios and the entropy;
  torch_matmul  the same with the pad's unfold(-1, L, 2) times the (L, 2) filter matrix in place of
              conv1d, whose float64 route is a slow one here;
  features2   window_features(features=("mean", "var")): what one read of the stream costs.
The torch contenders are timed on the first --torch-windows windows of the data (all channels of as
many leading samples as hold that many windows) and scaled to all windows -- unfold with step < W
copies the stream and every level writes its coefficients.  Their lines say how many windows were
measured.

One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For the library's contenders also the kernel's time by the library's HIP-event kernel
timer, taken in a run of its own, and the shares of two floors of the kernel's compiled inner loop
(counted in the gfx950 assembly of windowwave.hip).  A step -- one pair of taps of one output a lane
-- is 8 vector instructions: v_add_u32, v_subrev_u32, v_min_u32 and v_lshl_add_u32 for the wrapped
address and four v_fmac_f64 (a wave's float64 instruction issues every 4 cycles of a SIMD, a 32-bit
one every 2: 24 cycles), and one ds_read_b128 (4 cycles of the CU's LDS, 256 B / clk; lane i reads
the 16 bytes at 16 i, no bank conflict away from the wrap); a pair of taps costs a wave two more
ds_read_b128, of the four filter values at one address for all lanes.  All reads of a pair of taps
are issued before the one wait in front of the multiply-adds.  Per level min(NT / 64, ceil(n_j /
128)) waves have outputs, ceil(n_j / 2 / NT) a lane, and take L / 2 pairs of taps:
  share_of_valu_issue = wave steps / s x 24 cycles over 256 CUs x 4 SIMDs x 2.4 GHz;
  share_of_lds        = wave reads / s x 4 cycles over 256 CUs x 2.4 GHz.
No counter pass is taken.  For `rel_ent` the largest difference from a torch contender on the
windows that one measured.

    python benchmarks/wavelet_probe.py [--channels 16 64 256] [--log2n 21] [--contenders ..]
                                       [--out profiles/wavelet_probe.jsonl]
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
KERNEL = b"window_wavelet"
WAVELET = "db4"
SIMD_RATE = 256 * 4 * 2.4e9                     # cycles of all SIMDs a second
LDS_RATE = 256 * 2.4e9                          # cycles of all LDS arrays a second
STEP_VALU_CYCLES = 24
READ_LDS_CYCLES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-windows", type=int, default=32768)
    ap.add_argument("--contenders", nargs="+", default=["rel_ent", "all", "torch", "torch_matmul", "features2"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import wavelet_filters, wavelet_level, window_features, window_wavelet
    lib = _lib.load()
    n = 1 << a.log2n
    lo, hi = wavelet_filters(WAVELET)
    L = lo.shape[0]
    filt = torch.from_numpy(np.stack([lo, hi])).cuda()               # (2, L)

    def levels_of(w, J, how):
        """The sums of squares of d^1 .. d^J, a^J of the windows w (m, W): (m, J + 1)."""
        a0, E = w[:, None, :], []
        for _ in range(J):
            pad = torch.nn.functional.pad(a0, (0, L - 2), mode="circular")
            if how == "conv1d":
                both = torch.nn.functional.conv1d(pad, filt[:, None, :], stride=2)         # (m, 2, n / 2)
            else:
                both = (pad[:, 0].unfold(-1, L, 2) @ filt.T).transpose(1, 2)
            E.append((both[:, 1] ** 2).sum(-1))
            a0 = both[:, :1]
        E.append((a0[:, 0] ** 2).sum(-1))
        return torch.stack(E, -1)

    def torch_route(how):
        def run(x, W, step):
            J = wavelet_level(W, L)
            w = x.unfold(-1, W, step).reshape(-1, W)
            E = levels_of(w - w.mean(-1, keepdim=True), J, how)
            p = E / E.sum(-1, keepdim=True)
            H = -(p * torch.log(p)).sum(-1) / math.log(J + 1)
            return {"relative": p.T.reshape(J + 1, x.shape[0], -1), "entropy": H.reshape(x.shape[0], -1)}
        return run

    def ours(names):
        def run(x, W, step):
            return window_wavelet(x, W, step, features=names, wavelet=WAVELET)[1]
        return run

    def features2(x, W, step):
        return window_features(x, W, step, features=("mean", "var"))[1]

    fns = {"rel_ent": ours(("relative", "entropy")), "all": ours(tuple(_lib.WINDOW_WAVELET)),
           "torch": torch_route("conv1d"), "torch_matmul": torch_route("matmul"), "features2": features2}
    fns = {k: fn for k, fn in fns.items() if k in a.contenders}

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

    def wave_steps(W):
        """The wave steps and the wave-wide LDS reads of the inner loop that one window takes."""
        nt = 256 if W > _lib.WW_WIDE else 64
        J = wavelet_level(W, L)
        waves = [min(nt // 64, math.ceil((W >> (j + 1)) / 64)) for j in range(J)]
        each = [math.ceil((W >> (j + 1)) / nt) for j in range(J)]
        return (sum(w * q for w, q in zip(waves, each)) * (L // 2),
                sum(w * (q + 2) for w, q in zip(waves, each)) * (L // 2))

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        diffs = {}
        for W, step in SHAPES:                                      # warm-up of every shape
            results = {k: timed(fns[k], part(k, x, W, step)[0], W, step)[1] for k in fns}
            per = part("torch", x, W, step)[1] // nch
            for t in ("torch", "torch_matmul"):
                if t in results and "rel_ent" in results:
                    diffs[W, step] = {f: float((results["rel_ent"][f][..., :per] - v).abs().max())
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
            for k in ("rel_ent", "all"):
                if k not in fns:
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
            steps, reads = wave_steps(W)
            for k in fns:
                measured = part(k, x, W, step)[1]
                t = np.array(times[k, (W, step)]) * (windows / measured)
                line = {"probe": "wavelet", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "level": wavelet_level(W, L), "windows": windows, "windows_measured": measured,
                        "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if (k, (W, step)) in kernels:
                    ms, launches, total = kernels[k, (W, step)]
                    line["timed_call_ms"] = round(ms, 3)
                    line["kernel_launches"] = launches
                    line["kernel_ms_per_chunk"] = round(total / chunks, 4)
                    if total:
                        per_s = windows / (total * 1e-3)
                        line["share_of_valu_issue"] = round(per_s * steps * STEP_VALU_CYCLES / SIMD_RATE, 4)
                        line["share_of_lds"] = round(per_s * reads * READ_LDS_CYCLES / LDS_RATE, 4)
                if k == "rel_ent" and (W, step) in diffs:
                    line["max_diff_from_torch"] = {f: float(f"{v:.2e}") for f, v in diffs[W, step].items()}
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
