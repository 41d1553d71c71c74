"""Generate tests/golden/g21_phaselock.npz by RUNNING the reference PhaseLock.

Run with the reference openseize package importable (tests never import it):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<openseize checkout>/src \
        python3 tests/golden/make_golden_phaselock.py

The reference estimators module imports ``openseize.coupling.transforms``, a
package path that does not exist; it loads once ``openseize.coupling`` and
``openseize.coupling.transforms`` are aliased to the experimental package.
Only data is written.  Keys, per case prefix:

The input signals are not stored: ``signal(fs, seconds, seed)`` below regenerates
them (NumPy's default_rng stream is stable), and the tests restate it.

  a_*  signal(500, 30, 2101), chunksize 7000 (two full chunks and a short one),
       window 1 (W = 500)
       phases            reference Analytic(...).phases of the 6-10 Hz band, concatenated
       idx, idx_len      reference indices, concatenated, and the length of each chunk's list
       pow1, pv1         estimate(..., ncores=1)    (3 centres x W)
       pow3, pv3         estimate(..., ncores=3)
       rng1, rng3        rng.integers(0, 2**62) drawn once after each estimate
       amp60             reference Analytic amplitudes of the standardized 60 Hz band
  b_*  signal(333, 30, 2102), window 1 (odd W = 333)
  c_*  the a_ signal in one chunk (chunksize > n, so the shifts run modulo n)
  d_*  the a_ signal, surrogates=None: powers only
  e_*  shuffle(): 5 successive calls at seed 7 on the a_ indices, concatenated
"""

import os
import sys

import numpy as np

import openseize
import openseize.experimental.coupling as _cpl
import openseize.experimental.coupling.transforms as _tr

sys.modules["openseize.coupling"] = _cpl
sys.modules["openseize.coupling.transforms"] = _tr
openseize.coupling = _cpl

from openseize import producer                                      # noqa: E402
from openseize.core import protools                                 # noqa: E402
from openseize.experimental.coupling.estimators import PhaseLock    # noqa: E402
from openseize.filtering import fir                                 # noqa: E402
from openseize.filtering.special import Hilbert                     # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CENTERS = [40, 60, 80]


def signal(fs, seconds, seed):
    """8 Hz phase modulating the amplitude of a 60 Hz carrier, plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(fs * seconds)) / fs
    theta = np.sin(2 * np.pi * 8 * t + 0.3)
    gamma = (1.0 + 0.8 * np.cos(2 * np.pi * 8 * t + 0.3)) * np.sin(2 * np.pi * 60 * t)
    return 2.0 * theta + 0.7 * gamma + 0.5 * rng.standard_normal(t.size)


def run_case(x, fs, cs, window, surrogates, out, prefix, phases=False, amp=False):
    est = PhaseLock(Hilbert(width=4, fs=fs), chunksize=cs, seed=0)
    est.index(x, fpass=[6, 10], fstop=[4, 12])
    out[f"{prefix}idx"] = np.concatenate(est.indices).astype(np.int64)
    out[f"{prefix}idx_len"] = np.array([len(a) for a in est.indices], dtype=np.int64)
    if phases:
        filt = fir.Kaiser([6, 10], [4, 12], fs)
        y = filt(producer(x, cs, -1), chunksize=cs, axis=-1)
        an = _tr.Analytic(y, fs, cs, -1, width=4, gpass=est.hilbert.gpass,
                          gstop=est.hilbert.gstop)
        out[f"{prefix}phases"] = np.concatenate(list(an.phases))
    for cores in ((1, 3) if surrogates else (1,)):
        est.rng = np.random.default_rng(0)
        pw, pv = est.estimate(x, CENTERS, bandwidth=8, window=window, surrogates=surrogates,
                              ncores=cores, verbose=False)
        out[f"{prefix}pow{cores}"] = pw
        if surrogates:
            out[f"{prefix}pv{cores}"] = pv
        out[f"{prefix}rng{cores}"] = np.array([est.rng.integers(0, 2**62)], dtype=np.int64)
    if amp:
        filt = fir.Kaiser(60 + np.array([-4, 4]), 60 + np.array([-8, 8]), fs)
        z = protools.standardize(filt(producer(x, cs, -1), chunksize=cs, axis=-1), axis=-1)
        an = _tr.Analytic(z, fs, cs, -1, width=4, gpass=est.hilbert.gpass,
                          gstop=est.hilbert.gstop)
        out[f"{prefix}amp60"] = np.concatenate(list(an.amplitudes))
    return est


def main():
    out = {}
    x = signal(500, 30, 2101)
    est = run_case(x, 500, 7000, 1, 25, out, "a_", phases=True, amp=True)
    xb = signal(333, 30, 2102)
    run_case(xb, 333, 7000, 1, 25, out, "b_", amp=True)
    run_case(x, 500, 40000, 1, 25, out, "c_", amp=True)
    run_case(x, 500, 7000, 1, None, out, "d_")
    est.rng = np.random.default_rng(7)
    out["e_shuffle"] = np.concatenate([np.concatenate(est.shuffle(x.size)) for _ in range(5)])
    path = os.path.join(OUT, "g21_phaselock.npz")
    np.savez_compressed(path, **out)
    print(f"g21_phaselock.npz: {os.path.getsize(path) / 1e3:.0f} kB, {len(out)} arrays")


if __name__ == "__main__":
    main()
