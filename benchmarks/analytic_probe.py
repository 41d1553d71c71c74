"""analytic_connectivity at the sizes a user runs: 16, 64 and 256 channels of complex128 analytic
signal (seeded normal real and imaginary parts, channels 1.. mixed with channel 0), 2^21 samples
per channel resident on the device.

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, five alternating runs of each in one process:
  aec / oaec / plv / ciplv / wpli   analytic_connectivity with that one method, i.e. one sum group
                                    of csrc/pairtime.hip alone (plv and ciplv share LOCK);
  all          the five methods in one call (one pass over the stream, four pair launches per push);
  torch_gemm   aec and plv without it: torch.corrcoef(|z|) and |conj(u) u^T| / N -- GEMMs;
  torch_pairs  oaec and wpli without it (ciplv would ride on plv's GEMM): d = x_i y_j - y_i x_j broadcast
               over all pairs, 2^16 samples at a time ((C, C, 2^16) float64 temporaries: run where that is
               affordable, 16 and 64 channels), its sums, and the table of the docstring.
One JSON line per contender and size: ms per 2^20-sample chunk (median and spread of the runs).
For the library's contenders also the kernels' times by the library's HIP-event kernel timer,
taken in a run of its own, and the pair kernels' float64 work counted from the code per (pair,
sample) -- AMP 1 instruction (1 FMA), LAG 4 (1 product, 1 FMA, 2 additions), ORTH 9 (3 products,
3 FMAs, 3 additions), LOCK 6 (2 products, 2 FMAs, 2 additions); |d| is an input modifier -- over
the C (C + 1) / 2 pairs of the result, as a share of the 78.6 TFLOP/s float64 vector peak in flop
(an FMA two) and in instructions (39.3 T lanes/s).  For `all` the largest difference of each
measure from the torch contenders, off the diagonal.

    python benchmarks/analytic_probe.py [--channels 16 64 256] [--log2n 21] [--out profiles/analytic_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F64 = 78.6e12
TORCH_PAIRS_MAX_CHANNELS = 64
METHODS = ("aec", "oaec", "plv", "ciplv", "wpli")
# (instructions, flop) per (pair, sample) of each sum group
WORK = {"aec": (1, 2), "oaec": (9, 12), "plv": (6, 8), "ciplv": (6, 8), "wpli": (4, 5), "all": (20, 27)}
KERNELS = (b"pair_prepare", b"pair_accumulate", b"pair_fold", b"analytic_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=METHODS + ("all", "torch_gemm", "torch_pairs"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.experimental.coupling import analytic_connectivity
    lib = _lib.load()
    n = 1 << a.log2n

    def run(method):
        return lambda z: analytic_connectivity(z, method=method)[1]

    def torch_gemm(z):
        amp = z.abs()
        u = z / amp
        return {"aec": torch.corrcoef(amp), "plv": (torch.conj(u) @ u.T).abs() / z.shape[1]}

    def pearson(cnt, sp, sq, spp, sqq, spq):
        return (cnt * spq - sp * sq) / torch.sqrt((cnt * spp - sp * sp) * (cnt * sqq - sq * sq))

    def torch_pairs(z):
        nch, cnt = z.shape
        x, y, amp = z.real.contiguous(), z.imag.contiguous(), z.abs()
        sd, sm, sb, sbb = (torch.zeros((nch, nch), dtype=torch.float64, device=z.device) for _ in range(4))
        for at in range(0, cnt, 1 << 16):
            cut = slice(at, at + (1 << 16))
            d = x[:, None, cut] * y[None, :, cut] - y[:, None, cut] * x[None, :, cut]
            m = d.abs()
            b = m / amp[:, None, cut]                              # b[i, j]: the part of z_j orthogonal to z_i
            sd += d.sum(-1)
            sm += m.sum(-1)
            sb += b.sum(-1)
            sbb += (b * b).sum(-1)
        sa, sq = amp.sum(-1), (amp * amp).sum(-1)
        r = pearson(cnt, sa[:, None], sb, sq[:, None], sbb, sm)
        return {"oaec": (r + r.T) / 2, "wpli": sd.abs() / sm}

    def timed(fn, z):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(z)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop), out

    def kernel_ms(name):
        launches, total = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.osz_profile_query(name, ctypes.byref(launches), ctypes.byref(total)))
        return launches.value, total.value

    fns = {m: run(m) for m in METHODS}
    fns["all"] = run(METHODS)
    fns["torch_gemm"] = torch_gemm
    fns["torch_pairs"] = torch_pairs
    lines = []
    for nch in a.channels:
        parts = dev.synth_normal(2 * nch, n, seed=nch)
        parts[1:nch] += 0.5 * parts[0]                         # (something for the off-diagonal to find)
        parts[nch + 1:] += 0.5 * parts[nch]
        z = torch.complex(parts[:nch], parts[nch:])
        del parts
        names = [k for k in fns if (a.only is None or k == a.only)
                 and (k != "torch_pairs" or nch <= TORCH_PAIRS_MAX_CHANNELS)]
        results = {}
        for k in names:                                         # warm-up of every shape
            results[k] = timed(fns[k], z)[1]
        diff = None
        if "all" in results:
            off = ~torch.eye(nch, dtype=torch.bool, device=z.device)
            diff = {m: float((results["all"][m] - results[k][m])[off].abs().max())
                    for k in ("torch_gemm", "torch_pairs") if k in results for m in results[k]}
        results.clear()
        times = {k: [] for k in names}
        for _ in range(a.runs):
            for k in names:
                ms, out = timed(fns[k], z)
                del out
                times[k].append(ms)
        kernels = {}
        for k in names:                                         # the kernels' shares, in runs of their own
            if k.startswith("torch"):
                continue
            _lib.check(lib.osz_profile_reset())
            _lib.check(lib.osz_profile_enable(1))
            ms, out = timed(fns[k], z)
            del out
            _lib.check(lib.osz_profile_enable(0))
            kernels[k] = (ms, {q.decode(): kernel_ms(q) for q in KERNELS})
        chunks = n / float(1 << 20)
        for k in names:
            t = np.array(times[k])
            line = {"probe": "analytic", "contender": k, "channels": nch, "samples": n,
                    "runs_ms": [round(float(v), 3) for v in t],
                    "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                    "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
            if k in kernels:
                ms, per = kernels[k]
                line["timed_call_ms"] = round(ms, 3)
                line["kernel_ms_per_chunk"] = {q: round(v[1] / chunks, 4) for q, v in per.items() if v[0]}
                line["kernel_launches"] = {q: v[0] for q, v in per.items() if v[0]}
                pair = per["pair_accumulate"]
                if pair[0] and pair[1]:
                    instr, flop = WORK[k]
                    work = n * nch * (nch + 1) // 2
                    line["pair_instructions_per_pair_sample"] = instr
                    line["pair_flop_per_pair_sample"] = flop
                    line["pair_share_of_call"] = round(pair[1] / ms, 4)
                    line["pair_share_of_f64_peak_flop"] = round(flop * work / (pair[1] * 1e-3) / PEAK_F64, 4)
                    line["pair_share_of_f64_peak_instructions"] = round(
                        instr * work / (pair[1] * 1e-3) / (PEAK_F64 / 2), 4)
            if k == "all" and diff:
                line["max_diff_from_torch"] = diff
            lines.append(line)
            print(json.dumps(line), flush=True)
        del z
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
