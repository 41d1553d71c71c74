"""bispectrum / bicoherence at the sizes a user runs: 16 and 64 channels, nfft 4096 (fs 1024,
resolution 0.25), 50 % overlap, 2^20 seeded samples per channel resident on the device (511
segments), bands of 128, 512 and the full 2048 bins (from bin 1; a band is skipped where its
sums do not fit into the free device memory).

Contenders, timed with device events around a call that ends in a synchronise, after a warm-up
of every shape, alternating runs in one process (five of the library's calls, two of PyTorch's):
  bispectrum   spectra.estimators.bispectrum (K14: the four sums, the mean);
  bicoherence  spectra.estimators.bicoherence(method=("kim", "hagihira")): the same pass, two ratios;
  torch        the same sums from public API without K14: stft(x, fs, boundary=False, padded=False,
               asarray=False) stacked to (nseg, C, nfreq), then X[..., k1, None] * X[..., None, k2] *
               conj(X[..., k1 + k2]) summed over the segments for the WHOLE nb x nb square (a
               broadcast knows no triangle), batched over segments and channels so that its
               temporaries stay under 2 GiB, and the two ratios from them.
One JSON line per contender and shape: ms per 2^20-sample chunk (median and spread), and for the
library's calls the float64 instructions the pair loop executes -- 12 per (entry, segment) over the
entries k2 <= k1 inside the domain -- the time of osz_bispec_accumulate's two kernels alone (the
library's HIP-event kernel timer, in a run of its own), the pair kernel's instruction rate as a share
of the float64 vector peak (39.3 T lanes/s: 78.6 TFLOP/s counts an FMA as two), and the largest
difference of the two bicoherences from the torch contender.

    python benchmarks/bispec_probe.py [--channels 16 64] [--bands 128 512 2048] [--out profiles/bispec_probe.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS, RESOLUTION, NFFT = 1024.0, 0.25, 4096
PEAK_F64_LANES = 39.3e12
INSTRUCTIONS = 12                       # per (entry, segment): DESIGN.md, K14
TORCH_BATCH = 1 << 24                   # complex entries per temporary (0.25 GiB; five live at most)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--bands", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--only", choices=["bispectrum", "bicoherence", "torch"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd import _lib
    from openseize_amd.spectra.estimators import bicoherence, bispectrum, stft
    lib = _lib.load()
    n = 1 << a.log2n
    nfreq = NFFT // 2 + 1
    freqs = np.fft.rfftfreq(NFFT, 1 / FS)

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
        x[:, 1:] += 0.5 * x[:, :-1] ** 2                    # (a quadratic term: something for the bispectrum to find)
        for nb in a.bands:
            if (32 + 16 + 16) * nch * nb * nb > torch.cuda.mem_get_info()[0]:
                print(json.dumps({"probe": "bispec", "channels": nch, "band_bins": nb, "skipped": "sums do not fit"}))
                continue
            fmax = freqs[nb]                                # bins 1 .. nb
            k = torch.arange(1, nb + 1, device="cuda")
            k3 = k[:, None] + k[None, :]
            inside = k3 <= nfreq - 1
            k3c = k3.clamp(max=nfreq - 1)

            def run_bispectrum(x):
                return bispectrum(x, FS, resolution=RESOLUTION, fmax=fmax)[2]

            def run_bicoherence(x):
                return bicoherence(x, FS, method=("kim", "hagihira"), resolution=RESOLUTION, fmax=fmax)[2]

            def run_torch(x):
                _, _, segments = stft(x, FS, resolution=RESOLUTION, boundary=False, padded=False, asarray=False)
                X = torch.stack(list(segments))             # (nseg, C, nfreq), scaled by sqrt(norm)
                power = (X.real ** 2 + X.imag ** 2).sum(0)
                T = torch.zeros((nch, nb, nb), dtype=torch.complex128, device=x.device)
                P12, A = torch.zeros_like(T.real), torch.zeros_like(T.real)
                cb = min(nch, max(1, TORCH_BATCH // (nb * nb)))
                sb = max(1, TORCH_BATCH // (cb * nb * nb))
                for c0 in range(0, nch, cb):
                    for s0 in range(0, X.shape[0], sb):
                        Xb = X[s0:s0 + sb, c0:c0 + cb]
                        X1 = Xb[..., 1:nb + 1]
                        P = X1[..., :, None] * X1[..., None, :]
                        t = P * torch.conj(Xb[..., k3c])
                        T[c0:c0 + cb] += t.sum(0)
                        A[c0:c0 + cb] += t.abs().sum(0)
                        del t
                        P12[c0:c0 + cb] += (P.real ** 2 + P.imag ** 2).sum(0)
                        del P
                nan = torch.full_like(A, float("nan"))
                kim = torch.where(inside, (T.real ** 2 + T.imag ** 2) / (P12 * power[:, k3c]), nan)
                hag = torch.where(inside, T.abs() / A, nan)
                return {"kim": kim, "hagihira": hag}

            fns = {"bispectrum": run_bispectrum, "bicoherence": run_bicoherence, "torch": run_torch}
            names = [name for name in fns if a.only is None or name == a.only]
            results = {}
            for name in names:                              # warm-up of every shape
                results[name] = timed(fns[name], x)[1]
            err = None
            if "bicoherence" in results and "torch" in results:
                err = max(float((results["bicoherence"][m] - results["torch"][m])[:, inside].abs().max())
                          for m in ("kim", "hagihira"))
            results.clear()
            torch.cuda.empty_cache()
            times = {name: [] for name in names}
            for run in range(a.runs):
                for name in names:
                    if name == "torch" and run >= a.torch_runs:
                        continue
                    ms, out = timed(fns[name], x)
                    del out
                    times[name].append(ms)
            kernel = None
            if "bicoherence" in names:                      # the kernels alone, in a run of their own
                _lib.check(lib.osz_profile_reset())
                _lib.check(lib.osz_profile_enable(1))
                ms, out = timed(run_bicoherence, x)
                del out
                _lib.check(lib.osz_profile_enable(0))
                kernel = {}
                for kname in ("bispec_prepare", "bispec_accumulate"):
                    launches, total = ctypes.c_int64(), ctypes.c_double()
                    _lib.check(lib.osz_profile_query(kname.encode(), ctypes.byref(launches), ctypes.byref(total)))
                    kernel[kname] = (launches.value, total.value)
                kernel["call_ms"] = ms
            nseg = (n - NFFT) // (NFFT // 2) + 1
            entries = int((inside & (k[None, :] <= k[:, None])).sum())
            instructions = INSTRUCTIONS * entries * nseg * nch
            chunks = n / float(1 << 20)
            for name in names:
                t = np.array(times[name])
                line = {"probe": "bispec", "contender": name, "channels": nch, "band_bins": nb, "samples": n,
                        "nfft": NFFT, "overlap": 0.5, "segments": nseg, "runs_ms": [round(float(v), 3) for v in t],
                        "ms_per_chunk": round(float(np.median(t)) / chunks, 4),
                        "spread_ms_per_chunk": round(float(t.max() - t.min()) / chunks, 4)}
                if name != "torch":
                    line["entries_per_channel"] = entries
                    line["f64_instructions"] = instructions
                if name == "bicoherence" and kernel:
                    acc_ms = kernel["bispec_accumulate"][1]
                    line["accumulate_launches"] = kernel["bispec_accumulate"][0]
                    line["accumulate_ms"] = round(acc_ms, 3)
                    line["prepare_ms"] = round(kernel["bispec_prepare"][1], 3)
                    line["accumulate_share_of_call"] = round(acc_ms / kernel["call_ms"], 4)
                    line["accumulate_share_of_f64_peak"] = (round(instructions / (acc_ms * 1e-3) / PEAK_F64_LANES, 4)
                                                            if acc_ms else None)
                    if err is not None:
                        line["max_diff_from_torch"] = err
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
