"""CPU-only tests of csd / coherence: the names, the argument errors (raised with no GPU and
before the stream is touched), the C ABI of the two kernels' entry points, and the NumPy
restatement of the definition that tests/test_gpu_csd.py compares the device against -- pinned
here against pairwise scipy.signal.csd / coherence, so the GPU tests get a whole (C, C, nfreq)
expected value without C^2 SciPy calls."""

import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as sps

from openseize_amd import _lib, producer
from openseize_amd.spectra.estimators import coherence, csd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nfft, window, overlap, detrend, scaling, channels, samples): every nfft route of the windowed
# DFT (1000 / 10000: specmix, 1024 / 4096: powers of two, 999: chirp, 20480: specsplit), both
# detrends, both scalings, overlaps 0 / 0.5 / 0.6, four windows; at least 9 segments each
CASES = [
    (1000, "hann", 0.5, "constant", "density", 5, 50000),
    (1024, "hamming", 0.6, "linear", "spectrum", 13, 50000),
    (999, "boxcar", 0.0, "constant", "density", 5, 50000),
    (4096, "blackman", 0.5, "linear", "density", 13, 120000),
    (10000, "hamming", 0.6, "linear", "spectrum", 5, 120000),
    (20480, "hann", 0.5, "constant", "spectrum", 5, 300000),
]
# the coherence is compared where both auto-spectra reach FLOOR of max|S| (a ratio's error is
# the spectrum's error over the auto-spectra)
FLOOR = 1e-3


def rate(nfft):
    """(fs, resolution) with int(fs / resolution) == nfft exactly (a power-of-two quotient)."""
    fs, resolution = nfft / 4.0, 0.25
    assert int(fs / resolution) == nfft
    return fs, resolution


def signal(nch, n, ramp, seed=0):
    """Per channel seeded white noise plus linspace(0, 1, C)[c] x one shared AR(1) noise (pole
    0.6), an offset of 3 and, with ``ramp``, 1e-4 n -- so that detrending matters and the
    coherence runs from 0 to nearly 1 over the channels."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nch, n))
    shared = sps.lfilter([1.0], [1.0, -0.6], rng.standard_normal(n))
    x += np.linspace(0, 1, nch)[:, None] * shared + 3.0
    if ramp:
        x += 1e-4 * np.arange(n)
    return x


def welch_cross(x, fs, nfft, window, overlap, detrend, scaling):
    """The definition: (segments, freqs, S) with S[i, j] the mean over the segments of
    conj(X_i) X_j, X the rfft of the detrended, windowed segment, scaled and one-sided."""
    stride = nfft - int(nfft * overlap)
    nseg = (x.shape[1] - nfft) // stride + 1
    win = sps.get_window(window, nfft)
    norm = 1 / (fs * np.sum(win ** 2)) if scaling == "density" else 1 / np.sum(win) ** 2
    S = np.zeros((x.shape[0], x.shape[0], nfft // 2 + 1), dtype=complex)
    for s in range(nseg):
        seg = x[:, s * stride:s * stride + nfft]
        if np.all(np.isfinite(seg)) or detrend == "linear":
            seg = sps.detrend(seg, type=detrend, axis=-1)
        else:
            seg = seg - seg.mean(axis=-1, keepdims=True)      # (NaN goes through a mean)
        X = np.fft.rfft(seg * win, axis=-1)
        S += np.conj(X)[:, None] * X[None]
    S *= norm / nseg
    S[..., 1:(-1 if nfft % 2 == 0 else None)] *= 2
    return nseg, np.fft.rfftfreq(nfft, 1 / fs), S


def coherence_of(S):
    """(|S_ij|^2 / (S_ii S_jj), the entries where both auto-spectra reach FLOOR of max|S|)."""
    p = np.real(np.einsum("iif->if", S))
    with np.errstate(divide="ignore", invalid="ignore"):
        coh = np.abs(S) ** 2 / (p[:, None] * p[None])
    ok = p >= FLOOR * np.max(np.abs(S))
    return coh, ok[:, None] & ok[None]


def test_names_are_public():
    from openseize_amd.spectra import estimators
    assert callable(estimators.csd) and callable(estimators.coherence)
    assert csd.__doc__ and "scipy.signal.csd" in csd.__doc__


class Untouched:
    """A producer over a generating function that records whether it was ever started."""

    def __init__(self, shape, axis=-1):
        self.started = False

        def gen():
            self.started = True
            yield np.zeros(shape)

        self.pro = producer(gen, chunksize=100, axis=axis, shape=shape)


@pytest.mark.parametrize("func", [csd, coherence])
def test_argument_errors_come_before_the_stream(func):
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="psd"):
        func(rng.standard_normal(5000), fs=100)                       # one channel: psd's job
    with pytest.raises(ValueError, match="two-dimensional"):
        func(rng.standard_normal((2, 3, 5000)), fs=100)
    for kwargs, match in (({"detrend": "quadratic"}, "Trend type"),
                          ({"resolution": 0.01}, "nfft")):              # nfft 10000 > 5000 samples
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            func(src.pro, fs=100, **kwargs)
        assert not src.started
    for shape in ((5000,), (2, 2, 5000)):
        src = Untouched(shape)
        with pytest.raises(ValueError):
            func(src.pro, fs=100)
        assert not src.started


def test_unknown_scaling_comes_before_the_stream():
    src = Untouched((4, 5000))
    with pytest.raises(ValueError, match="Unknown scaling"):
        csd(src.pro, fs=100, scaling="power")
    assert not src.started
    with pytest.raises(TypeError):
        coherence(src.pro, fs=100, scaling="density")                 # it cancels: no such argument


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    declared = set(re.findall(r"\b(osz_[a-z0-9_]+)\s*\(", header))
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("osz_cross_accumulate", "osz_cross_finish"):
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(lib, name), f"{name} not exported"
    assert (_lib.CROSS_SPECTRUM, _lib.CROSS_COHERENCE) == (0, 1)
    assert re.search(r"OSZ_CROSS_SPECTRUM = 0", header) and re.search(r"OSZ_CROSS_COHERENCE = 1", header)


@pytest.mark.parametrize("case", CASES[:4], ids=lambda c: f"nfft{c[0]}-{c[1]}")
def test_restatement_is_scipy(case):
    """The restatement against pairwise SciPy on 5 x 50000 samples: 1e-12 of the output scale
    (measured: 3e-16 ... 1e-15 for the spectra, 1.2e-14 for the coherence)."""
    assert csd is not None                      # (this file is about the new names)
    nfft, window, overlap, detrend, scaling, _, _ = case
    fs, nch, n = 1000.0, 5, 50000
    kw = dict(fs=fs, window=window, nperseg=nfft, noverlap=int(nfft * overlap), nfft=nfft, detrend=detrend)
    stride = nfft - int(nfft * overlap)
    for ramp in (True, False):
        x = signal(nch, n, ramp)
        nseg, freqs, S = welch_cross(x, fs, nfft, window, overlap, detrend, scaling)
        assert nseg == (n - nfft) // stride + 1
        scale = np.max(np.abs(S))
        coh, ok = coherence_of(S)
        for i in range(nch):
            f, pxx = sps.welch(x[i], scaling=scaling, **kw)
            assert np.array_equal(f, freqs)
            assert np.max(np.abs(S[i, i] - pxx)) < 1e-12 * scale
            for j in range(nch):
                _, pxy = sps.csd(x[i], x[j], scaling=scaling, **kw)
                assert np.max(np.abs(S[i, j] - pxy)) < 1e-12 * scale, (i, j)
                if not ramp:
                    _, cxy = sps.coherence(x[i], x[j], **kw)
                    assert np.max(np.abs(coh[i, j] - cxy)[ok[i, j]]) < 1e-12, (i, j)
        assert np.max(np.abs(S - np.conj(S.transpose(1, 0, 2)))) < 1e-16 * scale
        if not ramp:
            assert np.mean(~ok) <= 0.005
