"""PhaseLock at the size of a real job: one channel of 1 h at 5 kHz resident on the device
(1.8e7 samples, chunksize 1e7), index() on the 6-10 Hz phase, estimate() at 20 centres
from 20 to 200 Hz (bandwidth 4, window 2 s = 10 000 samples, 300 surrogates).

Prints one JSON line: wall times of index() and estimate() (host clock around work that
ends in a device synchronise, after a warm-up of both on a short signal); the per-launch
time of osz_lock_accumulate from the library's HIP-event kernel timer (a second estimate()
run with the timer on); the adds that launch does, counted on the host from the indices
and the surrogate shifts; and the fractions of two floors it reaches:
  VALU: one f64 add per (set, offset, valid index) at 3.93e13 adds/s (the MI355X f64
        vector rate, 78.6 TFLOP/s counting an FMA as two);
  LDS:  one 8-byte ds_read_b64 per add at 150 TB/s (every CU streaming).

    python benchmarks/phaselock_probe.py [--seconds 3600] [--out FILE]
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 5000
VALU_ADDS_PER_S = 3.93e13
LDS_BYTES_PER_S = 150e12


def theta_gamma(n, fs, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    theta = np.sin(2 * np.pi * 8 * t)
    gamma = (1.0 + 0.8 * np.cos(2 * np.pi * 8 * t)) * np.sin(2 * np.pi * 80 * t)
    return 2.0 * theta + 0.7 * gamma + 0.5 * rng.standard_normal(n)


def valid_counts(indices, lengths, shifts, max_shift, W):
    """Valid windows per set (set 0, then one per shift), as osz_lock_accumulate counts
    them: q' = (q + shift) % max_shift contributes iff ceil(W/2) <= q' <= L - W // 2."""
    h = -(-W // 2)
    sig = np.asarray(shifts, dtype=np.int64)
    out = np.zeros(sig.size + 1, dtype=np.int64)
    for q, L in zip(indices, lengths):
        q = np.sort(q)
        hi = L - W // 2
        out[0] += np.count_nonzero((q >= h) & (q <= hi))
        if hi < h or not sig.size:
            continue
        cnt = lambda a, b: np.maximum(np.searchsorted(q, b, "right") - np.searchsorted(q, a), 0)
        split = max_shift - sig                          # q >= split wraps
        unwrapped = cnt(np.maximum(h - sig, 0), np.minimum(hi - sig, split - 1))
        wrapped = cnt(np.maximum(h - sig + max_shift, split), hi - sig + max_shift)
        out[1:] += unwrapped + wrapped
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600)
    ap.add_argument("--chunksize", type=int, default=int(1e7))
    ap.add_argument("--centres", type=int, default=20)
    ap.add_argument("--surrogates", type=int, default=300)
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from openseize_amd import _lib
    from openseize_amd.experimental.coupling.estimators import PhaseLock
    from openseize_amd.filtering.special import Hilbert
    lib = _lib.load()

    n = int(a.seconds * FS)
    x = torch.from_numpy(theta_gamma(n, FS)).cuda()
    centres = np.linspace(20, 200, a.centres)
    kw = dict(bandwidth=4, window=a.window, surrogates=a.surrogates, ncores=1, verbose=False)

    # warm-up: every kernel and FIR plan of the timed path, on a short signal
    warm = PhaseLock(Hilbert(width=4, fs=FS), chunksize=a.chunksize)
    xw = x[:min(n, 200000)]
    warm.index(xw, [6, 10], [4, 12])
    warm.estimate(xw, centres[:2], **{**kw, "surrogates": 4})
    torch.cuda.synchronize()

    est = PhaseLock(Hilbert(width=4, fs=FS), chunksize=a.chunksize, seed=0)
    t0 = time.perf_counter()
    est.index(x, [6, 10], [4, 12])
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t0

    state = est.rng.bit_generator.state
    t0 = time.perf_counter()
    powers, pvalues = est.estimate(x, centres, **kw)
    torch.cuda.synchronize()
    t_estimate = time.perf_counter() - t0

    # the same call with the kernel timer on
    est.rng.bit_generator.state = state
    _lib.check(lib.osz_profile_reset())
    _lib.check(lib.osz_profile_enable(1))
    t0 = time.perf_counter()
    est.estimate(x, centres, **kw)
    torch.cuda.synchronize()
    t_estimate_timed = time.perf_counter() - t0
    _lib.check(lib.osz_profile_enable(0))
    launches, total_ms = ctypes.c_int64(), ctypes.c_double()
    _lib.check(lib.osz_profile_query(b"lock_accumulate", ctypes.byref(launches),
                                     ctypes.byref(total_ms)))

    # adds, from the indices and the shifts the estimate drew
    W = a.window * FS
    max_shift = min(a.chunksize, n)
    lengths = [min(a.chunksize, n - k) for k in range(0, n, a.chunksize)]
    idx = [i.cpu().numpy() for i in est.indices]
    rng = np.random.default_rng()
    rng.bit_generator.state = state
    adds = 0
    for _ in centres:
        shifts = [rng.integers(0, max_shift) for _ in range(a.surrogates)]
        adds += int(valid_counts(idx, lengths, shifts, max_shift, W).sum()) * W
    per_launch_ms = total_ms.value / max(launches.value, 1)
    kernel_s = total_ms.value / 1e3
    valu_s = adds / VALU_ADDS_PER_S
    lds_s = adds * 8 / LDS_BYTES_PER_S
    line = {
        "probe": "phaselock",
        "samples": n, "fs": FS, "chunksize": a.chunksize, "centres": a.centres,
        "surrogates": a.surrogates, "window_samples": W,
        "indices": int(sum(i.size for i in idx)),
        "index_s": round(t_index, 4),
        "estimate_s": round(t_estimate, 4),
        "estimate_s_with_kernel_timer": round(t_estimate_timed, 4),
        "lock_accumulate_launches": launches.value,
        "lock_accumulate_ms_per_launch": round(per_launch_ms, 4),
        "lock_accumulate_total_s": round(kernel_s, 4),
        "adds": adds,
        "adds_per_launch": adds // max(launches.value, 1),
        "valu_floor_s": round(valu_s, 5),
        "lds_floor_s": round(lds_s, 5),
        "valu_floor_fraction": round(valu_s / kernel_s, 4) if kernel_s else None,
        "lds_floor_fraction": round(lds_s / kernel_s, 4) if kernel_s else None,
        "power_checksum": float(np.sum(powers)),
        "target_estimate_s": 5.0,
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
