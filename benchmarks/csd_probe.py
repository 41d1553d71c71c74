"""csd at the sizes a user runs: 16, 64 and 256 channels, nfft 4096 (fs 1024, resolution 0.25),
50 % overlap, 2^22 seeded samples per channel resident on the device.

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  csd    spectra.estimators.csd (K10);
  torch  the same numbers from public API without it: stft(x, fs, boundary=False,
         padded=False, asarray=False) and acc += conj(X)[:, None] * X[None] per segment in
         PyTorch (a (C, C, nfreq) complex temporary per segment: run where that is affordable,
         16 and 64 channels);
  psd    psd of the same data, the floor every Welch pass pays.
One JSON line per contender and size: ms per 2^20-sample chunk (median and spread of the five
runs), and for csd the flop count 8 nseg nfreq C (C + 1) / 2 from the shapes, that count over
the time as a share of the 78.6 TFLOP/s float64 vector peak, the share of the call spent in
osz_cross_accumulate (the library's HIP-event kernel timer, in a run of its own), and the
largest difference from the torch contender over max|S|.

    python benchmarks/csd_probe.py [--channels 16 64 256] [--log2n 22] [--out profiles/csd_probe.jsonl]
    python benchmarks/csd_probe.py --channels 256 --only csd --runs 1      # under rocprofv3 --kernel-trace --stats
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS, RESOLUTION, NFFT = 1024.0, 0.25, 4096
PEAK_F64 = 78.6e12
TORCH_MAX_CHANNELS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=["csd", "torch", "psd"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.spectra.estimators import csd, psd, stft
    lib = _lib.load()
    n = 1 << a.log2n
    nfreq = NFFT // 2 + 1

    def run_csd(x):
        return csd(x, FS, resolution=RESOLUTION)[2]

    def run_psd(x):
        return psd(x, FS, resolution=RESOLUTION)[2]

    def run_torch(x):
        _, _, segments = stft(x, FS, resolution=RESOLUTION, boundary=False, padded=False, asarray=False)
        acc = torch.zeros((x.shape[0], x.shape[0], nfreq), dtype=torch.complex128, device=x.device)
        count = 0
        for X in segments:                                  # (C, nfreq), scaled by sqrt(norm)
            acc += torch.conj(X)[:, None] * X[None]
            count += 1
        acc /= count
        acc[..., 1:-1] *= 2
        return acc

    def timed(fn, x):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(x)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        x[1:] += 0.5 * x[0]                                 # (something for the off-diagonal to find)
        names = [k for k in ("csd", "torch", "psd")
                 if (a.only is None or k == a.only) and (k != "torch" or nch <= TORCH_MAX_CHANNELS)]
        fns = {"csd": run_csd, "torch": run_torch, "psd": run_psd}
        results = {}
        for k in names:                                     # warm-up of every shape
            results[k] = timed(fns[k], x)[1]
        err = None
        if "csd" in results and "torch" in results:
            err = float((results["csd"] - results["torch"]).abs().max() / results["torch"].abs().max())
        results.clear()
        times = {k: [] for k in names}
        for _ in range(a.runs):
            for k in names:
                ms, out = timed(fns[k], x)
                del out
                times[k].append(ms)
        share = None
        if "csd" in names:                                  # the kernel's share, in a run of its own
            _lib.check(lib.osz_profile_reset())
            _lib.check(lib.osz_profile_enable(1))
            ms, out = timed(run_csd, x)
            del out
            _lib.check(lib.osz_profile_enable(0))
            launches, total = ctypes.c_int64(), ctypes.c_double()
            _lib.check(lib.osz_profile_query(b"cross_accumulate", ctypes.byref(launches), ctypes.byref(total)))
            share = (launches.value, total.value, total.value / ms)
        nseg = (n - NFFT) // (NFFT // 2) + 1
        chunks = n / float(1 << 20)
        for k in names:
            t = np.array(times[k])
            line = {"probe": "csd", "contender": k, "channels": nch, "samples": n, "nfft": NFFT, "overlap": 0.5,
                    "segments": nseg, "runs_ms": [round(float(v), 3) for v in t],
                    "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                    "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
            if k == "csd":
                flop = 8 * nseg * nfreq * nch * (nch + 1) // 2
                line["flop"] = flop
                line["share_of_f64_peak"] = round(flop / (float(np.median(t)) * 1e-3) / PEAK_F64, 4)
                if share:
                    line["accumulate_launches"] = share[0]
                    line["accumulate_ms"] = round(share[1], 3)
                    line["accumulate_share_of_call"] = round(share[2], 4)
                    line["accumulate_share_of_f64_peak"] = round(flop / (share[1] * 1e-3) / PEAK_F64, 4) if share[1] else None
                if err is not None:
                    line["max_diff_from_torch_over_max"] = err
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
