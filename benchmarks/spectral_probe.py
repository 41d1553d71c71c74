"""window_spectral at the sizes a user runs: 16, 64 and 256 channels of seeded normal float64 noise,
2^21 samples per channel resident on the device, windows (W, step) = (1024, 1024), (1024, 512) and
(256, 128); five bands, two edge fractions, all nine features.

Contenders, timed with device events around work that ends in a synchronise, after a warm-up of
every shape, five alternating runs of each in one process:
  call        window_spectral(...) on the resident tensor: segmenter, transforms, reduction, the
              concatenation of the pushes' results (for each value of --push-bytes: the bound on one
              push's periodograms, features/spectral.py _SPECTRAL_PUSH_BYTES);
  transform   the SpecStream pushes of the same stream alone, in the same pieces;
  reduction   one launch of osz_spectral_features (csrc/windowspec.hip) on ALL the periodograms of
              the stream, resident: its rate over the bytes of the range, 8 B per bin, against the
              8.0 TB/s of the data sheet and the 6.29 TB/s a copy reaches;
  reduction_sums  the same launch without entropy and flatness: what the two logarithms per bin cost;
  torch       the same nine features from the same periodograms by PyTorch ops: sum, cumsum +
              searchsorted, argmax, log, in batches of segments whose temporaries stay under 1 GiB.
One JSON line per contender, size and window shape: ms per 2^20-sample chunk (median and spread of
the runs); for `reduction` also the largest relative difference of a continuous feature from the
torch contender and the share of rows whose peak and edge bins agree.

    python benchmarks/spectral_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/spectral_probe.jsonl]
"""

import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1024), (1024, 512), (256, 128))
FS = 256.0
BANDS = ((0.5, 4.0), (4.0, 8.0), (8.0, 13.0), (13.0, 30.0), (30.0, 100.0))
EDGES = (0.9, 0.95)
NAMES = ("total", "band", "relative", "peak", "centroid", "spread", "edge", "entropy", "flatness")
CONTINUOUS = ("total", "band", "relative", "centroid", "spread", "entropy", "flatness")
BATCH_BYTES = 1 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--push-bytes", type=int, nargs="+", default=None,
                    help="bounds on one push's periodograms to time `call` with (default: the library's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.core import numerical as nm
    from openseize_amd.features import spectral
    from openseize_amd.features.spectral import window_spectral
    _lib.load()
    n = 1 << a.log2n
    bounds = a.push_bytes or [spectral._SPECTRAL_PUSH_BYTES]

    def plan(W):
        freqs = np.fft.rfftfreq(W, 1 / FS)
        k0, k1 = spectral._bin_range(freqs, None, None)
        bins, _ = spectral._band_bins(BANDS, freqs, k0, k1)
        return k0, k1, bins, FS / W

    def pushes(x, W, step, bound, keep):
        """The periodograms of x, pushed in the pieces window_spectral pushes; kept when ``keep``."""
        coeffs, scale = nm._window_and_scale("hann", W, FS, "density")
        nch, nfreq = x.shape[0], W // 2 + 1
        spec = dev.SpecStream(W, W, step, coeffs, scale, "constant", _lib.SPEC_PSD_SEGMENTS, nch)
        cap = max(1, bound // (8 * nch * nfreq)) * step
        parts = []
        try:
            for at in range(0, x.shape[1], cap):
                P = spec.push(x[:, at:at + cap])
                if keep:
                    parts.append(P)
        finally:
            spec.close()
        return torch.cat(parts) if keep else None

    def reduction(P, W, names=NAMES):
        k0, k1, bins, df = plan(W)
        mask = dev.spectral_mask(names)
        out = torch.empty((dev.spectral_planes(mask, len(bins), len(EDGES)), P.shape[1], P.shape[0]),
                          dtype=torch.float64, device=P.device)
        dev.spectral_features(P, k0, k1, df, bins, EDGES, True, mask, out)
        return out

    def torch_route(P, W):
        k0, k1, bins, df = plan(W)
        nk = k1 - k0 + 1
        f = torch.arange(k0, k1 + 1, dtype=torch.float64, device=P.device) * df
        per = max(1, BATCH_BYTES // (8 * P.shape[1] * P.shape[2]))
        outs = []
        for s in range(0, P.shape[0], per):
            Q = P[s:s + per]
            R = Q[..., k0:k1 + 1]
            S = R.sum(-1)
            total = df * S
            band = torch.stack([df * Q[..., b0:b1].sum(-1) for b0, b1 in bins])
            peak = f[R.argmax(-1)]
            cen = (R * f).sum(-1) / S
            spread = ((R * (f - cen[..., None]) ** 2).sum(-1) / S).sqrt()
            cum = R.cumsum(-1)
            edge = torch.stack([f[torch.searchsorted(cum, (p * cum[..., -1:]).contiguous()).clamp_(max=nk - 1)[..., 0]]
                                for p in EDGES])
            pk = R / S[..., None]
            lp = pk.log()
            ent = -(torch.xlogy(pk, pk)).sum(-1) / math.log(nk)
            flat = nk * torch.exp(lp.mean(-1))
            rows = [total[None], band, band / total, peak[None], cen[None], spread[None], edge, ent[None], flat[None]]
            outs.append(torch.cat(rows).transpose(-1, -2))           # (planes, nch, segments)
        return torch.cat(outs, dim=-1)

    def timed(fn, *args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(*args)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    lines = []
    chunks = n / float(1 << 20)
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        for W, step in SHAPES:
            k0, k1, bins, df = plan(W)
            P = pushes(x, W, step, bounds[0], True)

            def call(bound):
                spectral._SPECTRAL_PUSH_BYTES = bound
                return window_spectral(x, FS, W, step, features=NAMES, bands=BANDS, edge=EDGES)[1]

            fns = {("call", b): (call, (b,)) for b in bounds}
            fns["transform", bounds[0]] = (pushes, (x, W, step, bounds[0], False))
            fns["reduction", None] = (reduction, (P, W))
            fns["reduction_sums", None] = (reduction, (P, W, NAMES[:7]))
            fns["torch", None] = (torch_route, (P, W))
            results = {k: timed(fn, *args)[1] for k, (fn, args) in fns.items()}          # warm-up
            ours, theirs = results["reduction", None], results["torch", None]
            whole = results["call", bounds[0]]
            agree = {}
            p = 0
            for name in NAMES:
                w = len(bins) if name in ("band", "relative") else len(EDGES) if name == "edge" else 1
                g, t = ours[p:p + w], theirs[p:p + w]
                if name in CONTINUOUS:
                    agree[name] = float(((g - t).abs() / t.abs()).max())
                else:
                    agree[name + "_same_bin"] = float((g == t).double().mean())
                same = torch.equal(whole[name].reshape(g.shape).view(torch.int64), g.view(torch.int64))
                agree.setdefault("call_is_reduction_bit_for_bit", True)
                agree["call_is_reduction_bit_for_bit"] = agree["call_is_reduction_bit_for_bit"] and bool(same)
                p += w
            del results, ours, theirs, whole
            torch.cuda.empty_cache()
            times = {k: [] for k in fns}
            for _ in range(a.runs):
                for k, (fn, args) in fns.items():
                    ms, out = timed(fn, *args)
                    del out
                    times[k].append(ms)
            spectral._SPECTRAL_PUSH_BYTES = bounds[0]
            nseg = P.shape[0]
            hbm = 8.0 * nseg * nch * (k1 - k0 + 1)
            for (k, bound), t in times.items():
                t = np.array(t)
                line = {"probe": "spectral", "contender": k, "channels": nch, "samples": n, "winsize": W, "step": step,
                        "windows": nseg * nch, "bins": k1 - k0 + 1, "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if bound is not None:
                    line["push_bytes"] = bound
                if k.startswith("reduction"):
                    rate = hbm / (float(np.median(t)) * 1e-3)
                    line.update(range_bytes=hbm, bytes_per_s=float(f"{rate:.4e}"),
                                share_of_8_tb_s=round(rate / 8.0e12, 4), share_of_6_29_tb_s=round(rate / 6.29e12, 4))
                if k == "reduction":
                    line["against_torch"] = agree
                lines.append(line)
                print(json.dumps(line), flush=True)
            del P
            torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
