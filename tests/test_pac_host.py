"""ModulationIndex without a GPU: a NumPy restatement of the three device entry points
(``pac_bins``, ``pac_sums``, ``pac_mi`` -- the definitions tests/test_gpu_pac.py holds the
kernels to), shown to be meaningful on a signal with known coupling built from SciPy's own
filters; the argument errors, raised before a source is touched; the order of the shift
draws; and the C ABI of the entry points."""

import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as sps

from openseize_amd import _lib, producer
from openseize_amd.experimental.coupling.estimators import ModulationIndex
from openseize_amd.filtering.special import Hilbert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS, SECONDS = 500, 30
PHASE_CENTERS, PHASE_BW = [4, 8, 12], [2, 4, 4]
AMP_CENTERS, AMP_BW = [40, 60, 80], 20
SEEDS = [2101, 2102, 5]


# ------------------------------------------------------------------ the restatement
def pac_bins(phases, nbins):
    """osz_phase_bins from phases in [0, 2 pi): uint8 codes, 255 where the phase is NaN."""
    phases = np.asarray(phases, dtype=float)
    with np.errstate(invalid="ignore"):
        b = np.minimum(nbins - 1, np.floor(phases * nbins / (2 * np.pi)))
    return np.where(np.isnan(phases), 255, b).astype(np.uint8)


def pac_sums(bins_chunks, amp_chunks, shifts, nbins):
    """osz_pac_accumulate over all chunks: (sums (P, A, S + 1, nbins), counts (P, nbins)).
    bins_chunks: (P, L) uint8 per chunk, amp_chunks: (A, L) per chunk.  Set 0 pairs sample i
    with amp[i], set s with amp[(i + shifts[s - 1] % L) % L]; codes >= nbins are skipped."""
    P, A = bins_chunks[0].shape[0], amp_chunks[0].shape[0]
    sums = np.zeros((P, A, len(shifts) + 1, nbins))
    counts = np.zeros((P, nbins), dtype=np.int64)
    for bins, amp in zip(bins_chunks, amp_chunks):
        L = bins.shape[1]
        if L == 0:
            continue
        keep = [np.flatnonzero(bins[p] < nbins) for p in range(P)]
        for p in range(P):
            counts[p] += np.bincount(bins[p][keep[p]], minlength=nbins)
        for s, shift in enumerate([0] + [int(v) for v in shifts]):
            rolled = np.roll(amp, -(shift % L), axis=1)
            for p in range(P):
                for a in range(A):
                    sums[p, a, s] += np.bincount(bins[p][keep[p]], weights=rolled[a][keep[p]],
                                                 minlength=nbins)
    return sums, counts


def pac_mi(sums, counts):
    """osz_pac_finish: (mi (P, A, S + 1), dist (P, A, nbins)); a phase row with an empty bin
    is NaN throughout."""
    nbins = sums.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = sums / counts[:, None, None, :]
        m[(counts == 0).any(axis=1)] = np.nan
        P = m / m.sum(axis=-1, keepdims=True)
        plogp = np.where(P == 0, 0.0, P * np.log(np.where(P == 0, 1.0, P)))
    return 1 + plogp.sum(axis=-1) / np.log(nbins), P[:, :, 0]


def pac_shifts(seed, min_shift, max_shift, surrogates):
    """(the shifts one estimate() call draws, the generator after them)."""
    rng = np.random.default_rng(seed)
    return [rng.integers(min_shift, max_shift - min_shift) for _ in range(surrogates)], rng


def surrogate_z(mi):
    """(mi_0 - mean_s) / std_s (ddof 1) over the last axis' sets 1..S."""
    return (mi[..., 0] - mi[..., 1:].mean(axis=-1)) / mi[..., 1:].std(axis=-1, ddof=1)


# ------------------------------------------------------------------ the test signal
def drifting_signal(seed, fs=FS, seconds=SECONDS):
    """An 8 Hz rhythm whose phase random-walks (0.5 cycles per sqrt(second)) and modulates
    the amplitude of a 60 Hz rhythm, plus white noise.  A strictly periodic signal would keep
    its index under any time shift; the drift is what the surrogates destroy."""
    rng = np.random.default_rng(seed)
    n = int(fs * seconds)
    t = np.arange(n) / fs
    phi = 2 * np.pi * 8 * t + 0.5 * 2 * np.pi / np.sqrt(fs) * np.cumsum(rng.standard_normal(n))
    return (2 * np.sin(phi) + 0.7 * (1 + 0.8 * np.cos(phi)) * np.sin(2 * np.pi * 60 * t)
            + 0.5 * rng.standard_normal(n))


def scipy_band(x, center, bw, fs=FS):
    """The analytic signal of x in the band centre -+ bw/2 (transition bw/2 either side): a
    60 dB Kaiser firwin and scipy.signal.hilbert."""
    ntaps, beta = sps.kaiserord(60, (bw / 2) / (fs / 2))
    ntaps += 1 - ntaps % 2
    h = sps.firwin(ntaps, [center - 0.75 * bw, center + 0.75 * bw], window=("kaiser", beta),
                   pass_zero=False, fs=fs)
    return sps.hilbert(sps.fftconvolve(x, h, mode="same"))


def scipy_comodulogram(seed, nbins=18, surrogates=50):
    x = drifting_signal(seed)
    zp = [scipy_band(x, c, bw) for c, bw in zip(PHASE_CENTERS, PHASE_BW)]
    za = [scipy_band(x, c, AMP_BW) for c in AMP_CENTERS]
    bins = pac_bins(np.mod(np.angle(np.stack(zp)), 2 * np.pi), nbins)
    shifts, _ = pac_shifts(0, FS, x.size, surrogates)
    return pac_mi(*pac_sums([bins], [np.abs(np.stack(za))], shifts, nbins))[0]


def check_coupling(mi):
    """The qualitative facts of the drifting signal on an (3, 3, S + 1) index array."""
    real = mi[..., 0]
    assert np.unravel_index(np.argmax(real), real.shape) == (1, 1), real
    others = real[:, [0, 2]]
    assert real[1, 1] > 10 * others.max(), (real[1, 1], others.max())
    z = surrogate_z(mi)[1, 1]
    assert z > 20, z


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_finds_the_coupling(seed):
    mi = scipy_comodulogram(seed)
    print(f"seed {seed}: mi[8, 60] = {mi[1, 1, 0]:.4g}, largest in the 40 / 80 Hz rows "
          f"{mi[:, [0, 2], 0].max():.3g}, z = {surrogate_z(mi)[1, 1]:.1f}")
    check_coupling(mi)


def test_pac_mi_hand_cases():
    counts = np.array([[5, 5, 5, 5]])
    uniform = np.full((1, 1, 1, 4), 10.0)
    mi, dist = pac_mi(uniform, counts)
    assert abs(mi[0, 0, 0]) < 1e-15 and np.allclose(dist, 0.25)
    onebin = np.zeros((1, 1, 1, 4))
    onebin[..., 2] = 7.0
    mi, dist = pac_mi(onebin, counts)
    assert mi[0, 0, 0] == 1.0 and list(dist[0, 0]) == [0, 0, 1, 0]
    mi, dist = pac_mi(uniform, np.array([[5, 0, 5, 5]]))
    assert np.isnan(mi).all() and np.isnan(dist).all()
    # the empty bin of one phase row leaves the other row alone
    mi, _ = pac_mi(np.full((2, 1, 1, 4), 10.0), np.array([[5, 0, 5, 5], [1, 2, 3, 4]]))
    assert np.isnan(mi[0]).all() and np.isfinite(mi[1]).all()


def test_pac_bins_hand_cases():
    two_pi = 2 * np.pi
    ph = np.array([0.0, two_pi / 18 * 0.999, two_pi / 18 * 1.001, np.nextafter(two_pi, 0), np.nan])
    assert list(pac_bins(ph, 18)) == [0, 0, 1, 17, 255]
    assert list(pac_bins(ph, 2)) == [0, 0, 0, 1, 255]


def test_pac_sums_hand_case():
    bins = np.array([[0, 1, 255, 1, 0]], dtype=np.uint8)
    amp = np.array([[1.0, 2.0, 4.0, 8.0, 16.0]])
    sums, counts = pac_sums([bins], [amp], [1, 6, 5], 2)
    assert counts.tolist() == [[2, 2]]
    assert sums[0, 0, 0].tolist() == [17.0, 10.0]          # no shift
    assert sums[0, 0, 1].tolist() == [3.0, 20.0]           # i -> amp[(i + 1) % 5]
    assert sums[0, 0, 2].tolist() == [3.0, 20.0]           # 6 mod 5
    assert sums[0, 0, 3].tolist() == [17.0, 10.0]          # 5 mod 5


# ------------------------------------------------------------------ the estimator's arguments
class Untouched:
    """A 1-D (or other) producer over a generating function that records whether it was
    ever started."""

    def __init__(self, shape, axis=-1):
        self.started = False

        def gen():
            self.started = True
            yield np.zeros(shape)

        self.pro = producer(gen, chunksize=1000, axis=axis, shape=shape)


def estimator(nbins=18, chunksize=7000, seed=0):
    return ModulationIndex(Hilbert(width=4, fs=FS), chunksize=chunksize, nbins=nbins, seed=seed)


def test_attributes():
    h = Hilbert(width=4, fs=FS)
    est = ModulationIndex(h, chunksize=1234, nbins=12, seed=3)
    assert est.hilbert is h and est.fs == FS and est.chunksize == 1234 and est.nbins == 12
    assert est.rng.integers(0, 2**62) == np.random.default_rng(3).integers(0, 2**62)
    assert ModulationIndex(h).nbins == 18 and ModulationIndex(h).chunksize == int(10e6)


@pytest.mark.parametrize("kwargs, nbins, match", [
    ({}, 1, "nbins"),
    ({}, 65, "nbins"),
    ({"phase_centers": [1.5]}, 18, "phase band at 1.5"),          # stop edge 1.5 - 2 < 0
    ({"phase_centers": [2], "phase_bandwidth": 2}, 18, "phase band at 2"),       # reaches 0 Hz
    ({"amp_centers": [230]}, 18, "amp band at 230"),              # stop edge 230 + 20 = Nyquist
    ({"phase_bandwidth": [2, 4]}, 18, "phase_bandwidth"),
    ({"amp_bandwidth": [20, 20, 20]}, 18, "amp_bandwidth"),
    ({"min_shift": 2500}, 18, "min_shift"),                       # 2 min_shift >= max_shift = 5000
    ({"min_shift": 3000}, 18, "min_shift"),
    ({"surrogates": -3}, 18, "surrogates"),
])
def test_argument_errors_come_before_the_stream(kwargs, nbins, match):
    src = Untouched((5000,))
    args = {"phase_centers": [4, 8, 12], "amp_centers": [40, 60], "verbose": False}
    args.update(kwargs)
    before = np.random.default_rng(0).integers(0, 2**62)
    est = estimator(nbins=nbins)
    with pytest.raises(ValueError, match=match):
        est.estimate(src.pro, **args)
    assert not src.started
    assert est.rng.integers(0, 2**62) == before                   # nothing was drawn either


def test_shape_errors_come_before_the_stream():
    est = estimator()
    with pytest.raises(ValueError, match="1-D"):
        est.estimate(np.zeros((2, 5000)), [8], [60], verbose=False)
    src = Untouched((2, 5000))
    with pytest.raises(ValueError, match="1-D"):
        est.estimate(src.pro, [8], [60], verbose=False)
    assert not src.started
    src, other = Untouched((5000,)), Untouched((4000,))
    with pytest.raises(ValueError, match="4000"):
        est.estimate(src.pro, [8], [60], amplitude_signal=other.pro, verbose=False)
    with pytest.raises(ValueError, match="1-D"):
        est.estimate(src.pro, [8], [60], amplitude_signal=np.zeros((2, 5000)), verbose=False)
    assert not src.started and not other.started
    # the default min_shift is int(fs): 500 samples against a 900-sample signal
    short = Untouched((900,))
    with pytest.raises(ValueError, match="min_shift"):
        est.estimate(short.pro, [8], [60], verbose=False)
    assert not short.started


def test_shift_draw_helper():
    shifts, rng = pac_shifts(4, 500, 7000, 10)
    assert all(500 <= s < 6500 for s in shifts) and len(set(shifts)) > 1
    fresh = np.random.default_rng(4)
    for _ in range(10):
        fresh.integers(500, 6500)
    assert rng.integers(0, 2**62) == fresh.integers(0, 2**62)
    assert pac_shifts(4, 500, 7000, 0)[0] == []


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    declared = set(re.findall(r"\b(osz_[a-z0-9_]+)\s*\(", header))
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("osz_phase_bins", "osz_pac_accumulate", "osz_pac_finish"):
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name), f"{name} not exported"
    from openseize_amd import _device as dev
    assert callable(dev.phase_bins) and callable(dev.pac_accumulate) and callable(dev.pac_finish)
