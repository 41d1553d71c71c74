"""window_connectivity at the sizes a user runs: 16, 64 and 256 channels, 2^21 samples per channel
resident on the device (seeded normal float64 noise; for the complex measures two such planes as
real and imaginary part), windows (W, step) = (1024, 1024), (1024, 512) and (256, 128).

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, five alternating runs of each in one process:
  corr          window_connectivity(x, W, step, "corr") on the resident real tensor;
  plv_ciplv     window_connectivity(z, W, step, ("plv", "ciplv")) on the resident complex tensor;
  aec_plv_ciplv the three complex measures from one pass;
  torch_real    the same Gram matrices by PyTorch: x.unfold(-1, W, step), centred about the window
                means, one batched torch.matmul (rocBLAS) over as many windows as keep the centred
                copy under 2 GiB, the time scaled to all windows;
  torch_phasor  the same for the 2 C phasor rows [u_x; u_y] (staged before the clock starts, not
                centred).
One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs).  For ours, from a run of its own with the library's kernel timers on, the Gram kernel
(window_gram_kernel, csrc/windowpair.hip) alone: its ms per chunk and its share of the float64
peak in FMAs, counting C (C + 1) / 2 W per window for C rows and 2 C (2 C + 1) / 2 W for the phasor
rows against 39.3e12 FMA lanes a second.  `corr` also carries the largest difference between its
matrices and those made from the torch Gram matrices of the timed windows.

    python benchmarks/connectivity_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/connectivity_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
PEAK_FMA = 39.3e12
TORCH_BYTES = 2 << 30
OURS = {"corr": ("corr",), "plv_ciplv": ("plv", "ciplv"), "aec_plv_ciplv": ("aec", "plv", "ciplv")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.features import window_connectivity
    lib = _lib.load()
    n = 1 << a.log2n
    chunks = n / float(1 << 20)

    def ours(data, W, step, names):
        return window_connectivity(data, W, step, measures=names)[1]

    def torch_gram(rows, W, step, centre):
        """(the Gram matrices of the first windows that fit, the share of all windows they are)"""
        u = rows.unfold(-1, W, step)                                          # (R, nwin, W), a view
        per = max(1, min(u.shape[1], TORCH_BYTES // (8 * rows.shape[0] * W)))
        w = u[:, :per].permute(1, 0, 2)
        w = w - w.mean(-1, keepdim=True) if centre else w.contiguous()
        return torch.matmul(w, w.transpose(1, 2)), per / u.shape[1]

    def timed(fn, *args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(*args)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    def gram_ms():
        launches, total = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.osz_profile_query(b"window_gram", ctypes.byref(launches), ctypes.byref(total)))
        return launches.value, total.value

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        z = torch.complex(x, dev.synth_normal(nch, n, seed=1000 + nch))
        amp = z.abs()
        phasor = torch.cat(((z.real / amp), (z.imag / amp)))                  # (2 C, n)
        del amp
        for W, step in SHAPES:
            nwin = (n - W) // step + 1
            fns = {k: (ours, (x if k == "corr" else z, W, step, names)) for k, names in OURS.items()}
            fns["torch_real"] = (torch_gram, (x, W, step, True))
            fns["torch_phasor"] = (torch_gram, (phasor, W, step, False))
            # warm-up, and the agreement of the two routes on the windows torch holds
            r = timed(fns["corr"][0], *fns["corr"][1])[1]
            G, share = timed(fns["torch_real"][0], *fns["torch_real"][1])[1]
            d = torch.diagonal(G, dim1=1, dim2=2).sqrt()
            agree = float((G / (d[:, :, None] * d[:, None, :]) - r["corr"][:G.shape[0]]).abs().max())
            del r, G, d
            for k in ("plv_ciplv", "aec_plv_ciplv", "torch_phasor"):
                out = timed(fns[k][0], *fns[k][1])[1]
                del out
            torch.cuda.empty_cache()
            times = {k: [] for k in fns}
            shares = {}
            for _ in range(a.runs):
                for k, (fn, args) in fns.items():
                    ms, out = timed(fn, *args)
                    if k.startswith("torch"):
                        shares[k] = out[1]
                    del out
                    times[k].append(ms)
            kernel = {}
            for k in OURS:                                                    # the Gram kernel alone, in a run of its own
                _lib.check(lib.osz_profile_reset())
                _lib.check(lib.osz_profile_enable(1))
                ms, out = timed(fns[k][0], *fns[k][1])
                del out
                _lib.check(lib.osz_profile_enable(0))
                kernel[k] = gram_ms()
            torch.cuda.empty_cache()
            fma = {"corr": nch * (nch + 1) / 2 * W * nwin, "plv_ciplv": 2 * nch * (2 * nch + 1) / 2 * W * nwin}
            fma["aec_plv_ciplv"] = fma["corr"] + fma["plv_ciplv"]
            for k, t in times.items():
                t = np.array(t) / shares.get(k, 1.0)
                line = {"probe": "connectivity", "contender": k, "channels": nch, "samples": n, "winsize": W,
                        "step": step, "windows": nwin, "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if k in shares:
                    line["windows_timed_share"] = round(shares[k], 5)
                if k in kernel:
                    launches, total = kernel[k]
                    line.update(gram_launches=launches, gram_ms_per_chunk=round(total / chunks, 4), gram_fma=fma[k],
                                gram_share_of_fp64_peak=round(fma[k] / (total * 1e-3) / PEAK_FMA, 4))
                if k == "corr":
                    line["largest_difference_from_torch"] = agree
                lines.append(line)
                print(json.dumps(line), flush=True)
        del x, z, phasor
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
