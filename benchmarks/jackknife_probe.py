"""jackknife at the sizes a user runs: 16, 64 and 256 channels, nfft 4096 (fs 1024, resolution
0.25), 50 % overlap, 2^22 seeded samples per channel resident on the device.

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  coherence / imcoh / plv / pli / wpli / dwpli   spectra.estimators.jackknife with that one method;
  all          the six methods in one call (two passes over the stream);
  plain:NAME   the estimate alone -- coherence, or phase_connectivity with that method; plain:all
               is coherence plus phase_connectivity with all five.  Twice its time is the floor of
               a two-pass design;
  torch        the six standard errors from public API without the kernel: two passes over
               stft(x, fs, boundary=False, padded=False, asarray=False), the totals in the first,
               and in the second per segment the downdated measures, their deviations and squares
               in PyTorch ((C, C, nfreq) temporaries per segment: 16 and 64 channels, fewer runs).
               This is already the downdated form; the literal leave-one-out loop costs N + 1
               plain estimates.
One JSON line per contender and size: ms per 2^20-sample chunk (median and spread of the runs).
For the jackknife contenders the time of osz_jackknife_accumulate by the library's HIP-event
kernel timer -- taken in a run of its own -- its share of the call, and for the single methods
the counted flop per (segment, pair, bin) over that time as a share of the 78.6 TFLOP/s float64
vector peak (FLOP below: a fused multiply-add counts 2, a division or square root 1 although it
issues many instructions, compares and selects 0); for `all` the largest difference of each
standard error from the torch contender (off the diagonal, without the first and last bin).

    python benchmarks/jackknife_probe.py [--channels 16 64 256] [--log2n 22] [--out profiles/jackknife_probe.jsonl]
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
METHODS = ("coherence", "imcoh", "plv", "pli", "wpli", "dwpli")
# per (segment, pair, bin) in jackknife_accumulate_kernel's pair loop
FLOP = {"coherence": 17, "imcoh": 10, "plv": 17, "pli": 9, "wpli": 10, "dwpli": 16}
KERNELS = (b"jackknife_accumulate", b"jackknife_finish", b"lag_accumulate", b"cross_accumulate",
           b"unit_phasors", b"phase_finish", b"cross_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--only", default=None, help="one contender's name")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.spectra.estimators import coherence, jackknife, phase_connectivity, stft
    lib = _lib.load()
    n = 1 << a.log2n
    nfreq = NFFT // 2 + 1

    def run(method):
        return lambda x: jackknife(x, FS, method=method, resolution=RESOLUTION)[3]

    def plain(method):
        if method == "coherence":
            return lambda x: coherence(x, FS, resolution=RESOLUTION)[2]
        if method == "all":
            return lambda x: (coherence(x, FS, resolution=RESOLUTION)[2],
                              phase_connectivity(x, FS, method=METHODS[1:], resolution=RESOLUTION)[2])
        return lambda x: phase_connectivity(x, FS, method=method, resolution=RESOLUTION)[2]

    def measures(A, U, D, B, Q, G, Pi, Pj, count):
        return {"coherence": (A.real ** 2 + A.imag ** 2) / (Pi * Pj), "imcoh": A.imag / torch.sqrt(Pi * Pj),
                "plv": U.abs() / count, "pli": G.abs() / count, "wpli": D.abs() / B,
                "dwpli": (D ** 2 - Q) / (B ** 2 - Q)}

    def segments_of(x):
        return stft(x, FS, resolution=RESOLUTION, boundary=False, padded=False, asarray=False)[2]

    def terms(X):
        z = torch.conj(X)[:, None] * X[None]
        d = z.imag
        return z, z / z.abs(), d, d.abs(), d * d, torch.sign(d), X.real ** 2 + X.imag ** 2

    def run_torch(x):
        shape = (x.shape[0], x.shape[0], nfreq)
        total = None
        count = 0
        for X in segments_of(x):                            # (C, nfreq), scaled by sqrt(norm)
            t = terms(X)
            total = [v.clone() for v in t] if total is None else [s.add_(v) for s, v in zip(total, t)]
            count += 1
        A, U, D, B, Q, G, P = total
        theta = measures(A, U, D, B, Q, G, P[:, None], P[None], count)
        s1 = {m: torch.zeros(shape, dtype=torch.float64, device=x.device) for m in METHODS}
        s2 = {m: torch.zeros(shape, dtype=torch.float64, device=x.device) for m in METHODS}
        for X in segments_of(x):
            z, u, d, a, q, g, p = terms(X)
            left = measures(A - z, U - u, D - d, B - a, Q - q, G - g, (P - p)[:, None], (P - p)[None], count - 1)
            for m in METHODS:
                delta = left[m] - theta[m]
                s1[m] += delta
                s2[m] += delta * delta
        return {m: torch.sqrt(torch.clamp((count - 1) / count * (s2[m] - s1[m] ** 2 / count), min=0.0))
                for m in METHODS}

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
    for m in METHODS + ("all",):
        fns["plain:" + m] = plain(m)
    fns["torch"] = run_torch
    lines = []
    for nch in a.channels:
        x = dev.synth_normal(nch, n, seed=nch)
        x[1:] += 0.5 * x[0]                                 # (something for the off-diagonal to find)
        names = [k for k in fns if (a.only is None or k == a.only) and (k != "torch" or nch <= TORCH_MAX_CHANNELS)]
        results = {}
        for k in names:                                     # warm-up of every shape
            out = timed(fns[k], x)[1]
            if k in ("all", "torch"):
                results[k] = out
            del out
        diff = None
        if "all" in results and "torch" in results:
            off = ~torch.eye(nch, dtype=torch.bool, device=x.device)
            diff = {m: float((results["all"][m] - results["torch"][m])[off][..., 1:-1].abs().max()) for m in METHODS}
        results.clear()
        times = {k: [] for k in names}
        for r in range(a.runs):
            for k in names:
                if k == "torch" and r >= a.torch_runs:
                    continue
                ms, out = timed(fns[k], x)
                del out
                times[k].append(ms)
        kernels = {}
        for k in names:                                     # the kernels' shares, in runs of their own
            if k == "torch" or k.startswith("plain:"):
                continue
            _lib.check(lib.osz_profile_reset())
            _lib.check(lib.osz_profile_enable(1))
            ms, out = timed(fns[k], x)
            del out
            _lib.check(lib.osz_profile_enable(0))
            kernels[k] = (ms, {q.decode(): kernel_ms(q) for q in KERNELS})
        nseg = (n - NFFT) // (NFFT // 2) + 1
        chunks = n / float(1 << 20)
        for k in names:
            t = np.array(times[k])
            line = {"probe": "jackknife", "contender": k, "channels": nch, "samples": n, "nfft": NFFT, "overlap": 0.5,
                    "segments": nseg, "runs_ms": [round(float(v), 3) for v in t],
                    "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                    "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
            if k in kernels:
                ms, per = kernels[k]
                line["timed_call_ms"] = round(ms, 3)
                line["kernel_ms"] = {q: round(v[1], 3) for q, v in per.items() if v[0]}
                line["kernel_launches"] = {q: v[0] for q, v in per.items() if v[0]}
                jack = per["jackknife_accumulate"]
                if jack[0] and jack[1]:
                    line["jackknife_share_of_call"] = round(jack[1] / ms, 4)
                    line["jackknife_ms_per_chunk"] = round(jack[1] / chunks, 4)
                    if k in FLOP:
                        flop = FLOP[k] * nseg * nfreq * nch * (nch + 1) // 2
                        line["jackknife_flop"] = flop
                        line["jackknife_share_of_f64_peak"] = round(flop / (jack[1] * 1e-3) / PEAK_F64, 4)
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
