"""window_coherence at the sizes a user runs: 16, 64 and 256 channels, 2^21 float64 samples per
channel resident on the device (seeded normal noise, each channel mixed with its neighbour), fs =
256, the five EEG bands (1-4, 4-8, 8-13, 13-30, 30-45 Hz), and (nperseg, overlap, nsub, step) =
(256, 0.5, 7, W), (256, 0.5, 7, W / 2) and (128, 0.5, 15, W / 4) with W = 1024 in all three.

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, five alternating runs of each in one process, for ``coh`` alone, ``wpli`` alone and
all six measures:
  ours        window_coherence on the resident tensor;
  loop        what a caller does today: ``coherence`` / ``phase_connectivity`` once per window from
              Python, the band means taken with ``mean`` over the bins of each band;
  torch       PyTorch on the same segments: ``unfold`` into segments, mean removed, Hann window,
              ``torch.fft.rfft``, the bins of the bands kept, ``unfold`` over the segment axis into
              windows, ``einsum`` outer products -- for coh the sums of conj(X_i) X_j and of |X|^2,
              for wpli the (window, segment, i, j, bin) products themselves, whose imaginary parts
              are summed plain and in magnitude -- and the band means.  (All six: not written out.)
Every contender runs over the first windows whose results and temporaries stay under a budget (2 GiB
of results for ours, 64 windows for the loop, 1 GiB of products for PyTorch) and its time is scaled to
all windows; the share is in the line.  One JSON line per contender, size, shape and measure set: ms
per 2^20-sample chunk (median and spread of the runs).  For ours, from a run of its own with the
library's kernel timers on: the reduction (K27's instances) alone and the rest of the call (the
transforms of spec.hip, the carry and the allocations), and the largest difference from the PyTorch
route over the windows both hold.  No counter pass is taken here.

    python benchmarks/coherence_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/coherence_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 256.0
BANDS = ((1.0, 4.0), (4.0, 8.0), (8.0, 13.0), (13.0, 30.0), (30.0, 45.0))
SHAPES = ((256, 7, 1), (256, 7, 2), (128, 15, 4))          # (nperseg, nsub, W / step), overlap 0.5
SIX = ("coh", "imcoh", "plv", "pli", "wpli", "dwpli")
SETS = {"coh": "coh", "wpli": "wpli", "six": SIX}
OURS_BYTES = 2 << 30
LOOP_WINDOWS = 64
TORCH_BYTES = 1 << 30
KERNELS = ("cross", "lock", "lag")


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
    from openseize_amd.features import window_coherence
    from openseize_amd.spectra.estimators import coherence, phase_connectivity
    lib = _lib.load()
    n = 1 << a.log2n
    chunks = n / float(1 << 20)

    def bins_of(L):
        freqs = np.fft.rfftfreq(L, 1 / FS)
        return [(int(np.searchsorted(freqs, lo)), int(np.searchsorted(freqs, hi))) for lo, hi in BANDS]

    def ours(x, L, W, step, measures, per):
        return window_coherence(x[:, :(per - 1) * step + W], FS, W, step, measures=measures, bands=BANDS, nperseg=L)[1]

    def loop(x, L, W, step, measures, per):
        bins, out = bins_of(L), []
        for k in range(per):
            piece = x[:, k * step:k * step + W]
            found = {}
            if measures == "coh" or measures is SIX:
                found["coh"] = coherence(piece, FS, resolution=FS / L)[2]
            if measures != "coh":
                names = "wpli" if measures == "wpli" else SIX[1:]
                got = phase_connectivity(piece, FS, method=names, resolution=FS / L)[2]
                found.update({"wpli": got} if measures == "wpli" else got)
            out.append({name: torch.stack([m[..., b0:b1].mean(-1) for b0, b1 in bins]) for name, m in found.items()})
        return out

    def torch_route(x, L, W, step, measures, per):
        h, nsub, m = L // 2, (W - L) // (L // 2) + 1, step // (L // 2)
        bins = bins_of(L)
        seg = x[:, :(per - 1) * step + W].unfold(1, L, h)                               # (C, nseg, L)
        seg = (seg - seg.mean(-1, keepdim=True)) * torch.hann_window(L, periodic=True, dtype=x.dtype, device=x.device)
        X = torch.fft.rfft(seg, dim=-1)[..., bins[0][0]:bins[-1][1]]                     # (C, nseg, kept bins)
        Xw = X.unfold(1, nsub, m).permute(1, 3, 0, 2)                                    # (nwin, nsub, C, bins)
        if measures == "coh":
            S = torch.einsum("wsif,wsjf->wijf", Xw.conj(), Xw)
            p = (Xw.real ** 2 + Xw.imag ** 2).sum(1)                                      # (nwin, C, bins)
            v = (S.real ** 2 + S.imag ** 2) / (p[:, :, None] * p[:, None])
        else:
            d = torch.einsum("wsif,wsjf->wsijf", Xw.conj(), Xw).imag
            v = d.sum(1).abs() / d.abs().sum(1)
        k0 = bins[0][0]
        return torch.stack([v[..., b0 - k0:b1 - k0].mean(-1) for b0, b1 in bins], dim=1)  # (nwin, bands, C, C)

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
        return total.value

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        x[1:] += 0.7 * x[:-1].clone()
        for L, nsub, div in SHAPES:
            h = L // 2
            W = L + (nsub - 1) * h
            step = W // div
            nwin = (n - W) // step + 1
            kept = bins_of(L)[-1][1] - bins_of(L)[0][0]
            for label, measures in SETS.items():
                count = 6 if label == "six" else 1
                per = {"ours": min(nwin, max(1, OURS_BYTES // (8 * count * len(BANDS) * nch * nch))),
                       "loop": min(nwin, LOOP_WINDOWS)}
                fns = {"ours": ours, "loop": loop}
                if label != "six":
                    heavy = 16 * nch * nch * kept * (nsub * 3 if label == "wpli" else 3)   # PyTorch's bytes per window
                    per["torch"] = min(nwin, max(1, TORCH_BYTES // heavy))
                    fns["torch"] = torch_route
                args = {k: (x, L, W, step, measures, per[k]) for k in fns}
                mine = timed(ours, *args["ours"])[1]                                       # warm-up, and the agreement
                timed(loop, *args["loop"])
                agree = None
                if "torch" in fns:
                    theirs = timed(torch_route, *args["torch"])[1]
                    k = min(mine.shape[0], theirs.shape[0])
                    off = ~torch.eye(nch, dtype=torch.bool, device=x.device)
                    agree = float((mine[:k] - theirs[:k])[..., off].abs().max())
                    del theirs
                del mine
                torch.cuda.empty_cache()
                times = {k: [] for k in fns}
                for _ in range(a.runs):
                    for k, fn in fns.items():
                        ms, out = timed(fn, *args[k])
                        del out
                        times[k].append(ms)
                _lib.check(lib.osz_profile_reset())                     # the kernels alone, in a run of their own
                _lib.check(lib.osz_profile_enable(1))
                whole, out = timed(ours, *args["ours"])
                del out
                _lib.check(lib.osz_profile_enable(0))
                reduction = sum(kernel_ms(f"window_coherence_{name}".encode()) for name in KERNELS)
                torch.cuda.empty_cache()
                for k, t in times.items():
                    share = per[k] / nwin
                    t = np.array(t) / share
                    line = {"probe": "coherence", "contender": k, "measures": label, "channels": nch, "samples": n,
                            "nperseg": L, "nsub": nsub, "winsize": W, "step": step, "windows": nwin,
                            "windows_timed_share": round(share, 6), "runs_ms": [round(float(v), 3) for v in t],
                            "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                            "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                    if k == "ours":
                        line["reduction_ms_per_chunk"] = round(reduction / share / chunks, 4)
                        line["rest_ms_per_chunk"] = round((whole - reduction) / share / chunks, 4)
                        line["reduction_share_of_the_call"] = round(reduction / whole, 4)
                        line["largest_difference_from_torch"] = agree
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
