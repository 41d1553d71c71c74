"""phase_connectivity at the sizes a user runs: 16, 64 and 256 channels, nfft 4096 (fs 1024,
resolution 0.25), 50 % overlap, 2^22 seeded samples per channel resident on the device.

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  imcoh / plv / pli / wpli / dwpli   spectra.estimators.phase_connectivity with that one method;
  all    the five methods in one call (one pass over the stream);
  torch  the same five from public API without it: stft(x, fs, boundary=False, padded=False,
         asarray=False) and per segment z = conj(X)[:, None] * X[None] in PyTorch, its sums for
         every measure, and the table of the docstring at the end ((C, C, nfreq) temporaries per
         segment: run where that is affordable, 16 and 64 channels).
One JSON line per contender and size: ms per 2^20-sample chunk (median and spread of the five
runs).  For the lag measures the flop count of osz_lag_accumulate, 8 per (segment, pair, bin)
(one product, two fused multiply-adds, three additions; the comparisons and selects of the
sign are not counted), over the kernel's time by the library's HIP-event kernel timer -- taken
in a run of its own -- as a share of the 78.6 TFLOP/s float64 vector peak (a peak only FMAs
reach: four of the six counted instructions are not), and for `all` the largest difference of
each measure from the torch contender (off the diagonal, without the first and last bin).

    python benchmarks/phase_probe.py [--channels 16 64 256] [--log2n 22] [--out profiles/phase_probe.jsonl]
    python benchmarks/phase_probe.py --channels 256 --only wpli --runs 1     # under rocprofv3 --kernel-trace --stats
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
METHODS = ("imcoh", "plv", "pli", "wpli", "dwpli")
LAG_FLOP = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=METHODS + ("all", "torch"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.spectra.estimators import phase_connectivity, stft
    lib = _lib.load()
    n = 1 << a.log2n
    nfreq = NFFT // 2 + 1

    def run(method):
        return lambda x: phase_connectivity(x, FS, method=method, resolution=RESOLUTION)[2]

    def run_torch(x):
        _, _, segments = stft(x, FS, resolution=RESOLUTION, boundary=False, padded=False, asarray=False)
        shape = (x.shape[0], x.shape[0], nfreq)
        sz, sn = (torch.zeros(shape, dtype=torch.complex128, device=x.device) for _ in range(2))
        sd, sa, sq, sg = (torch.zeros(shape, dtype=torch.float64, device=x.device) for _ in range(4))
        power = torch.zeros(shape[1:], dtype=torch.float64, device=x.device)
        count = 0
        for X in segments:                                  # (C, nfreq), scaled by sqrt(norm)
            z = torch.conj(X)[:, None] * X[None]
            d = z.imag
            sz += z
            sn += z / z.abs()
            sd += d
            sa += d.abs()
            sq += d * d
            sg += torch.sign(d)
            power += X.real ** 2 + X.imag ** 2
            count += 1
        return {"imcoh": sz.imag / torch.sqrt(power[:, None] * power[None]), "plv": sn.abs() / count,
                "pli": sg.abs() / count, "wpli": sd.abs() / sa, "dwpli": (sd ** 2 - sq) / (sa ** 2 - sq)}

    def timed(fn, x):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(x)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    def kernel_ms(name):
        launches, total = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.osz_profile_query(name, ctypes.byref(launches), ctypes.byref(total)))
        return launches.value, total.value

    fns = {m: run(m) for m in METHODS}
    fns["all"] = run(METHODS)
    fns["torch"] = run_torch
    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        x[1:] += 0.5 * x[0]                                 # (something for the off-diagonal to find)
        names = [k for k in fns if (a.only is None or k == a.only) and (k != "torch" or nch <= TORCH_MAX_CHANNELS)]
        results = {}
        for k in names:                                     # warm-up of every shape
            results[k] = timed(fns[k], x)[1]
        diff = None
        if "all" in results and "torch" in results:
            off = ~torch.eye(nch, dtype=torch.bool, device=x.device)
            diff = {m: float((results["all"][m] - results["torch"][m])[off][..., 1:-1].abs().max()) for m in METHODS}
        results.clear()
        times = {k: [] for k in names}
        for _ in range(a.runs):
            for k in names:
                ms, out = timed(fns[k], x)
                del out
                times[k].append(ms)
        kernels = {}
        for k in names:                                     # the kernels' shares, in runs of their own
            if k == "torch":
                continue
            _lib.check(lib.osz_profile_reset())
            _lib.check(lib.osz_profile_enable(1))
            ms, out = timed(fns[k], x)
            del out
            _lib.check(lib.osz_profile_enable(0))
            kernels[k] = (ms, {q.decode(): kernel_ms(q) for q in (b"lag_accumulate", b"cross_accumulate",
                                                                   b"unit_phasors", b"phase_finish")})
        nseg = (n - NFFT) // (NFFT // 2) + 1
        chunks = n / float(1 << 20)
        for k in names:
            t = np.array(times[k])
            line = {"probe": "phase", "contender": k, "channels": nch, "samples": n, "nfft": NFFT, "overlap": 0.5,
                    "segments": nseg, "runs_ms": [round(float(v), 3) for v in t],
                    "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                    "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
            if k in kernels:
                ms, per = kernels[k]
                line["timed_call_ms"] = round(ms, 3)
                line["kernel_ms"] = {q: round(v[1], 3) for q, v in per.items() if v[0]}
                line["kernel_launches"] = {q: v[0] for q, v in per.items() if v[0]}
                lag = per["lag_accumulate"]
                if lag[0] and lag[1]:
                    flop = LAG_FLOP * nseg * nfreq * nch * (nch + 1) // 2
                    line["lag_flop"] = flop
                    line["lag_share_of_call"] = round(lag[1] / ms, 4)
                    line["lag_share_of_f64_peak"] = round(flop / (lag[1] * 1e-3) / PEAK_F64, 4)
            if k == "all" and diff is not None:
                line["max_diff_from_torch"] = diff
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
