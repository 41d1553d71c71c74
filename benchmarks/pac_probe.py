"""ModulationIndex at the size of a real job: one channel of 1 h at 5 kHz resident on the
device (1.8e7 samples, chunksize 1e7), 10 phase bands x 20 amplitude bands, 18 bins, 200
surrogates.

Three things are timed, every one with a device synchronise at its end:
  estimate():  the whole call (30 band filters, 30 Hilbert transforms, bins, amplitudes, the
               accumulate kernel per chunk, the finish), once, after a warm-up on a short
               signal;
  kernel leg:  osz_pac_accumulate alone on resident bins / amplitudes of the two chunk
               lengths of that stream (random bins, amplitudes in [0.1, 1.1)), all
               P x A x (S + 1) sets: device events around the two calls, each of which is
               the accumulate kernel and the small count kernel before it (P rows of bytes
               against P A (S + 1) walks of the accumulate kernel);
  torch leg:   the same sums built from existing parts on the same device,
               torch.bincount(bins[p], weights=amp[a].roll(-sigma_s)) -- one roll per (a, s),
               shared by the phase rows, one bincount per (p, a, s), the bins widened to
               int64 once outside the timed region -- on a subset of --torch-rolls rolls and
               --torch-counts bincounts per chunk, each scaled by its count in the full job.
The two legs alternate, --runs times each; the medians and every run are reported.  Before the
timing the kernel's sums are compared with the torch construction's on the subset.

Floors of the kernel leg, from the shapes (N = P A (S + 1) L adds per chunk):
  adds:   N f64 adds at 3.93e13 adds/s (the MI355X f64 vector rate);
  LDS:    one ds_read_b64 and one ds_write_b64 per add: 8 N bytes read at 150 TB/s and 8 N
          bytes written at 50 TB/s (ds_write_b64 moves a third of what ds_read_b64 does);
  bytes:  every wave reads its own L bins bytes and 8 L amplitude bytes, 9 N bytes, against
          the Infinity Cache (8.6 TB/s measured) and HBM (6.3 TB/s measured).

    python benchmarks/pac_probe.py [--seconds 3600] [--out profiles/pac_probe.jsonl]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 5000
VALU_ADDS_PER_S = 3.93e13
LDS_READ_BYTES_PER_S = 150e12
LDS_WRITE_BYTES_PER_S = 50e12
MALL_BYTES_PER_S = 8.6e12
HBM_BYTES_PER_S = 6.3e12


def drifting_theta_gamma(n, fs, seed=0):
    """An 8 Hz rhythm with a random-walking phase that modulates an 80 Hz amplitude."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    phi = 2 * np.pi * 8 * t + 0.5 * 2 * np.pi / np.sqrt(fs) * np.cumsum(rng.standard_normal(n))
    return (2.0 * np.sin(phi) + 0.7 * (1.0 + 0.8 * np.cos(phi)) * np.sin(2 * np.pi * 80 * t)
            + 0.5 * rng.standard_normal(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600)
    ap.add_argument("--chunksize", type=int, default=int(1e7))
    ap.add_argument("--phase-bands", type=int, default=10)
    ap.add_argument("--amp-bands", type=int, default=20)
    ap.add_argument("--surrogates", type=int, default=200)
    ap.add_argument("--nbins", type=int, default=18)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-rolls", type=int, default=8)
    ap.add_argument("--torch-counts", type=int, default=16)
    ap.add_argument("--skip-estimate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _device as dev
    from openseize_amd.experimental.coupling.estimators import ModulationIndex
    from openseize_amd.filtering.special import Hilbert

    n = int(a.seconds * FS)
    P, A, S, nbins = a.phase_bands, a.amp_bands, a.surrogates, a.nbins
    nsets = S + 1
    lengths = [min(a.chunksize, n - k) for k in range(0, n, a.chunksize)]
    phase_centers = np.linspace(4, 22, P)
    amp_centers = np.linspace(40, 230, A)
    kw = dict(phase_bandwidth=2, amp_bandwidth=20, surrogates=S, verbose=False)

    t_estimate = mi_max = None
    if not a.skip_estimate:
        x = torch.from_numpy(drifting_theta_gamma(n, FS)).cuda()
        warm = ModulationIndex(Hilbert(width=4, fs=FS), chunksize=a.chunksize, nbins=nbins)
        warm.estimate(x[:min(n, 400000)], phase_centers, amp_centers, **{**kw, "surrogates": 4})
        torch.cuda.synchronize()
        est = ModulationIndex(Hilbert(width=4, fs=FS), chunksize=a.chunksize, nbins=nbins, seed=0)
        t0 = time.perf_counter()
        mi, _, _ = est.estimate(x, phase_centers, amp_centers, **kw)
        torch.cuda.synchronize()
        t_estimate = time.perf_counter() - t0
        mi_max = float(mi.max())
        print(f"estimate(): {t_estimate:.2f} s", file=sys.stderr, flush=True)
        del x, est, warm
        torch.cuda.empty_cache()

    # resident inputs of the two legs
    gen = torch.Generator(device="cuda").manual_seed(1)
    chunks = []
    for L in lengths:
        bins = torch.randint(0, nbins, (P, L), dtype=torch.uint8, device="cuda", generator=gen)
        amp = torch.rand((A, L), dtype=torch.float64, device="cuda", generator=gen) + 0.1
        chunks.append((bins, amp))
    rng = np.random.default_rng(0)
    max_shift = min(a.chunksize, n)
    shifts = [int(rng.integers(FS, max_shift - FS)) for _ in range(S)]
    dshifts = torch.tensor(shifts, dtype=torch.int64, device="cuda")
    sums = dev.zeros((P, A, nsets, nbins), torch.float64)
    counts = dev.zeros((P, nbins), torch.int64)

    def kernel_leg():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for bins, amp in chunks:
            dev.pac_accumulate(bins, amp, dshifts, nbins, sums, counts)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / 1e3

    # the subset of the torch leg: rolls over (a, s), bincounts over (p, a, s)
    sig = [0] + shifts
    roll_set = [(i % A, (i * 7) % nsets) for i in range(a.torch_rolls)]
    count_set = [(i % P, roll_set[i % len(roll_set)]) for i in range(a.torch_counts)]
    wide = [[bins[p].long() for p in range(P)] for bins, _ in chunks]

    def torch_leg(keep=None):
        """Seconds the full job would take: the timed rolls and bincounts scaled by count."""
        total = 0.0
        for k, (bins, amp) in enumerate(chunks):
            L = bins.shape[1]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            rolled = {(ai, s): amp[ai].roll(-(sig[s] % L)) for ai, s in roll_set}
            ev[1].record()
            outs = [torch.bincount(wide[k][p], weights=rolled[key], minlength=nbins)
                    for p, key in count_set]
            ev[2].record()
            torch.cuda.synchronize()
            total += (ev[0].elapsed_time(ev[1]) / len(roll_set) * A * nsets
                      + ev[1].elapsed_time(ev[2]) / len(count_set) * P * A * nsets) / 1e3
            if keep is not None:
                keep.append(outs)
        return total

    # warm-up of both legs, and the comparison of their sums on the subset
    kernel_leg()
    ref = []
    torch_leg(ref)
    got = sums.cpu().numpy()
    want = np.zeros((len(count_set), nbins))
    for outs in ref:
        want += np.stack([o.cpu().numpy() for o in outs])
    worst = max(float(np.max(np.abs(got[p, ai, s] - want[i]) / want[i].max()))
                for i, (p, (ai, s)) in enumerate(count_set))
    assert worst < 1e-11, worst

    t_kernel, t_torch = [], []
    for _ in range(a.runs):
        t_kernel.append(kernel_leg())
        t_torch.append(torch_leg())
        print(f"kernel {t_kernel[-1]:.3f} s, torch (scaled) {t_torch[-1]:.1f} s", file=sys.stderr,
              flush=True)
    k_med, t_med = statistics.median(t_kernel), statistics.median(t_torch)

    adds = P * A * nsets * sum(lengths)
    floors = {
        "adds_floor_s": adds / VALU_ADDS_PER_S,
        "lds_floor_s": 8 * adds / LDS_READ_BYTES_PER_S + 8 * adds / LDS_WRITE_BYTES_PER_S,
        "bytes_floor_mall_s": 9 * adds / MALL_BYTES_PER_S,
        "bytes_floor_hbm_s": 9 * adds / HBM_BYTES_PER_S,
    }
    line = {
        "probe": "pac",
        "samples": n, "fs": FS, "chunksize": a.chunksize, "phase_bands": P, "amp_bands": A,
        "surrogates": S, "nbins": nbins, "runs": a.runs,
        "estimate_s": None if t_estimate is None else round(t_estimate, 4),
        "mi_max": mi_max,
        "kernel_s_runs": [round(v, 5) for v in t_kernel],
        "kernel_s": round(k_med, 5),
        "torch_rolls_timed": len(roll_set), "torch_counts_timed": len(count_set),
        "torch_s_scaled_runs": [round(v, 3) for v in t_torch],
        "torch_s_scaled": round(t_med, 3),
        "torch_over_kernel": round(t_med / k_med, 2),
        "subset_max_error_of_row_scale": worst,
        "adds": adds,
        "adds_per_s": round(adds / k_med, 1),
        **{k: round(v, 5) for k, v in floors.items()},
        **{k[:-2] + "_fraction": round(v / k_med, 4) for k, v in floors.items()},
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
