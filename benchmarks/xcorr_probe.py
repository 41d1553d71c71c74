"""window_xcorr at the sizes a user runs: 16, 64 and 256 channels, 2^21 float64 samples per channel
resident on the device (seeded normal noise, each channel mixed with its neighbour delayed by three
samples), windows (W, step) = (1024, 1024), (1024, 512) and (256, 128), maxlag 16 and 64.

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, alternating runs of each in one process:
  ours_peak_lag  window_xcorr(x, W, step, ("peak", "lag"), maxlag) on the resident tensor;
  ours_all       the four measures, ("xcorr", "peak", "lag", "signed"), from one pass;
  torch_matmul   the same numbers by PyTorch: x.unfold(-1, W, step), centred about the window means,
                 one batched torch.matmul (rocBLAS) per lag on the two shifted slices, normalised by
                 the lag-0 diagonal, then max, argmax and gather over the lags;
  torch_fft      the same by zero-padded torch.fft.rfft (2 W points), the products conj(F_i) F_j of
                 all pairs, irfft, the lags -L .. L cut out, and the same finish.
Every contender runs over the first windows whose results and temporaries stay under a byte budget
(4 GiB of results for ours, 2 GiB for each PyTorch temporary) and its time is scaled to all
windows; the share is in the line.  One JSON line per contender, size, window shape and maxlag: ms
per 2^20-sample chunk (median and spread of the runs).  For ours, from a run of its own with the
library's kernel timers on, the Gram kernel (xcorr_gram_kernel, csrc/windowxcorr.hip) alone: its ms
per chunk and its share of the float64 matrix peak in FMAs, counting C (C + 1) / 2 (2 L + 1) W per
window against 39.3e12 FMA lanes a second.  ours_all also carries the largest difference of its
``xcorr`` from each PyTorch route over the windows both hold, and the two routes' own difference.

    python benchmarks/xcorr_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/xcorr_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
MAXLAGS = (16, 64)
PEAK_FMA = 39.3e12
OURS_BYTES = 4 << 30
TORCH_BYTES = 2 << 30
OURS = {"ours_peak_lag": ("peak", "lag"), "ours_all": ("xcorr", "peak", "lag", "signed")}


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
    from openseize_amd.features import window_xcorr
    lib = _lib.load()
    n = 1 << a.log2n
    chunks = n / float(1 << 20)

    def ours(x, W, step, L, names, per):
        return window_xcorr(x[:, :(per - 1) * step + W], W, step, measures=names, maxlag=L)[1]

    def centred(x, W, step, per):
        w = x.unfold(-1, W, step)[:, :per].permute(1, 0, 2)                   # (per, C, W)
        return w - w.mean(-1, keepdim=True)

    def finish(r, L):
        """(per, 2 L + 1, C, C) lagged sums -> (xcorr, peak, lag)"""
        d = torch.diagonal(r[:, L], dim1=1, dim2=2).sqrt()
        rho = (r / (d[:, None, :, None] * d[:, None, None, :])).clamp(-1, 1)
        peak, at = rho.abs().max(dim=1)
        return rho, peak, (at - L).to(torch.float64)

    def torch_matmul(x, W, step, L, per):
        d = centred(x, W, step, per)
        r = torch.empty((per, 2 * L + 1) + (x.shape[0],) * 2, dtype=torch.float64, device=x.device)
        for l in range(-L, L + 1):
            lo, hi = max(0, -l), W - max(0, l)
            r[:, L + l] = torch.matmul(d[:, :, lo:hi], d[:, :, lo + l:hi + l].transpose(1, 2))
        return finish(r, L)

    def torch_fft(x, W, step, L, per):
        F = torch.fft.rfft(centred(x, W, step, per), n=2 * W)                 # (per, C, W + 1)
        cc = torch.fft.irfft(F.conj()[:, :, None, :] * F[:, None, :, :], n=2 * W)   # [.., i, j, l] = sum d_i[t] d_j[t + l]
        r = torch.cat((cc[..., 2 * W - L:], cc[..., :L + 1]), dim=-1).permute(0, 3, 1, 2)
        return finish(r, L)

    def timed(fn, *args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(*args)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    def gram_ms():
        launches, total = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.osz_profile_query(b"window_xcorr_gram", ctypes.byref(launches), ctypes.byref(total)))
        return launches.value, total.value

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        x[1:] += 0.7 * torch.roll(x[:-1].clone(), 3, dims=1)
        cc8 = 8 * nch * nch
        for W, step in SHAPES:
            nwin = (n - W) // step + 1
            for L in MAXLAGS:
                nl = 2 * L + 1
                per = {"ours_peak_lag": min(nwin, max(1, OURS_BYTES // (2 * cc8))),
                       "ours_all": min(nwin, max(1, OURS_BYTES // ((nl + 3) * cc8))),
                       "torch_matmul": min(nwin, max(1, TORCH_BYTES // max(nl * cc8, 8 * nch * W))),
                       "torch_fft": min(nwin, max(1, TORCH_BYTES // (16 * nch * nch * (W + 1))))}
                fns = {k: (ours, (x, W, step, L, names, per[k])) for k, names in OURS.items()}
                fns["torch_matmul"] = (torch_matmul, (x, W, step, L, per["torch_matmul"]))
                fns["torch_fft"] = (torch_fft, (x, W, step, L, per["torch_fft"]))
                # warm-up, and the agreement of the routes on the windows they share
                out = timed(fns["ours_peak_lag"][0], *fns["ours_peak_lag"][1])[1]
                del out
                mine = timed(fns["ours_all"][0], *fns["ours_all"][1])[1]
                rho_m = timed(fns["torch_matmul"][0], *fns["torch_matmul"][1])[1][0]
                rho_f = timed(fns["torch_fft"][0], *fns["torch_fft"][1])[1][0]
                km, kf = min(per["ours_all"], rho_m.shape[0]), min(per["ours_all"], rho_f.shape[0])
                agree = {"largest_difference_from_torch_matmul": float((mine["xcorr"][:km] - rho_m[:km]).abs().max()),
                         "largest_difference_from_torch_fft": float((mine["xcorr"][:kf] - rho_f[:kf]).abs().max()),
                         "largest_difference_between_torch_routes":
                             float((rho_m[:min(km, kf)] - rho_f[:min(km, kf)]).abs().max())}
                del mine, rho_m, rho_f
                torch.cuda.empty_cache()
                times = {k: [] for k in fns}
                for _ in range(a.runs):
                    for k, (fn, args) in fns.items():
                        ms, out = timed(fn, *args)
                        del out
                        times[k].append(ms)
                kernel = {}
                for k in OURS:                                                # the Gram kernel alone, in a run of its own
                    _lib.check(lib.osz_profile_reset())
                    _lib.check(lib.osz_profile_enable(1))
                    ms, out = timed(fns[k][0], *fns[k][1])
                    del out
                    _lib.check(lib.osz_profile_enable(0))
                    kernel[k] = gram_ms()
                torch.cuda.empty_cache()
                for k, t in times.items():
                    share = per[k] / nwin
                    t = np.array(t) / share
                    line = {"probe": "xcorr", "contender": k, "channels": nch, "samples": n, "winsize": W, "step": step,
                            "maxlag": L, "windows": nwin, "windows_timed_share": round(share, 6),
                            "runs_ms": [round(float(v), 3) for v in t],
                            "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                            "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                    if k in kernel:
                        launches, total = kernel[k]
                        fma = nch * (nch + 1) / 2 * nl * W * per[k]
                        line.update(gram_launches=launches, gram_ms_per_chunk=round(total / share / chunks, 4),
                                    gram_fma_per_window=nch * (nch + 1) / 2 * nl * W,
                                    gram_share_of_fp64_peak=round(fma / (total * 1e-3) / PEAK_FMA, 4))
                    if k == "ours_all":
                        line.update(agree)
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
