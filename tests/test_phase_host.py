"""CPU-only tests of phase_connectivity (K11): the names, the argument errors (raised with no
GPU and before the stream is touched), the C ABI of the three entry points against the header,
and ``phase_measures``, the NumPy restatement of the five definitions that
tests/test_gpu_phase.py compares the device against.  The restatement is pinned here: its imcoh
against pairwise scipy.signal.csd, a delayed copy of a channel (plv = pli = wpli = 1), the
invariances under scaling and negating a channel, and dwpli against its pairwise form."""

import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal as sps

from openseize_amd import _lib
from openseize_amd.spectra import estimators
from openseize_amd.spectra.estimators import phase_connectivity

from test_csd_host import CASES, Untouched, rate, signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("imcoh", "plv", "pli", "wpli", "dwpli")
RTOL = 1e-9          # the suite's bound on a spectrum's error over max|X| (tests/test_gpu_parity.py)


def phase_measures(x, fs, nfft, window, overlap, detrend):
    """The definitions: (segments, freqs, M, parts).  M maps each of METHODS to its (C, C, nfreq)
    array, with the fixed points of ``phase_connectivity`` (diagonal, real bins, NaN rows).
    Segments are cut as in test_csd_host.welch_cross; with z_s = conj(X_i) X_j and d_s = Im z_s,
    ``parts`` holds what the GPU tests build their tolerances from: ``N``, ``M`` = max|X|,
    ``xmin`` = min|X| over the bins that are not real, ``xlast`` = min|X| at the last bin,
    ``sd`` / ``sa`` / ``sq`` = sum d, sum |d|, sum d^2, and ``unsafe`` = per entry the number of
    segments with |d_s| < 20 RTOL M^2."""
    stride = nfft - int(nfft * overlap)
    nseg = (x.shape[1] - nfft) // stride + 1
    win = sps.get_window(window, nfft)
    X = []
    for s in range(nseg):
        seg = x[:, s * stride:s * stride + nfft]
        if np.all(np.isfinite(seg)) or detrend == "linear":
            seg = sps.detrend(seg, type=detrend, axis=-1)
        else:
            seg = seg - seg.mean(axis=-1, keepdims=True)      # (NaN goes through a mean)
        X.append(np.fft.rfft(seg * win, axis=-1))
    X = np.array(X) * np.sqrt(1 / (fs * np.sum(win ** 2)))    # (nseg, C, nfreq), csd's "density"
    nch, nfreq = X.shape[1:]
    big = np.nanmax(np.abs(X))
    shape = (nch, nch, nfreq)
    sz, sn = np.zeros(shape, complex), np.zeros(shape, complex)
    sd, sa, sq, sg = (np.zeros(shape) for _ in range(4))
    unsafe = np.zeros(shape, int)
    with np.errstate(divide="ignore", invalid="ignore"):
        for Xs in X:
            z = np.conj(Xs)[:, None] * Xs[None]
            d = z.imag
            sz += z
            sn += z / np.abs(z)
            sd += d
            sa += np.abs(d)
            sq += d * d
            sg += np.sign(d)
            unsafe += np.abs(d) < 20 * RTOL * big ** 2
        p = np.sum(np.abs(X) ** 2, axis=0)                    # (C, nfreq) sum |X|^2
        pn = np.sum(np.abs(X / np.abs(X)) ** 2, axis=0)       # ... of the unit phasors
        M = {"imcoh": sz.imag / np.sqrt(p[:, None] * p[None]),
             "plv": np.abs(sn) / nseg,
             "pli": np.abs(sg) / nseg,
             "wpli": np.abs(sd) / sa,
             "dwpli": (sd ** 2 - sq) / (sa ** 2 - sq)}
    eye = np.eye(nch, dtype=bool)
    for name, m in M.items():
        own = pn if name == "plv" else p
        lost = np.isnan(own)[:, None] | np.isnan(own)[None]
        if name != "plv":
            m[..., real_bins(nfft)] = 0.0
        m[eye] = 1.0 if name == "plv" else 0.0
        m[lost] = np.nan
    inner = np.setdiff1d(np.arange(nfreq), real_bins(nfft))
    parts = dict(N=nseg, M=big, xmin=np.nanmin(np.abs(X[..., inner])), xlast=np.nanmin(np.abs(X[..., -1])),
                 sd=sd, sa=sa, sq=sq, unsafe=unsafe)
    return nseg, np.fft.rfftfreq(nfft, 1 / fs), M, parts


def real_bins(nfft):
    """The bins where a real signal's spectrum is real: 0, and the last one for even nfft."""
    return [0, nfft // 2] if nfft % 2 == 0 else [0]


def test_names_are_public():
    assert callable(estimators.phase_connectivity)
    assert estimators.PHASE_METHODS == METHODS
    doc = phase_connectivity.__doc__
    for name in METHODS:
        assert f'"{name}"' in doc
    assert "rounding noise" in doc and "64 B per (pair, bin)" in doc
    assert tuple(_lib.PHASE_MODE) == METHODS and list(_lib.PHASE_MODE.values()) == [0, 1, 2, 3, 4]


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="psd"):
        phase_connectivity(rng.standard_normal(5000), fs=100)             # one channel
    with pytest.raises(ValueError, match="two-dimensional"):
        phase_connectivity(rng.standard_normal((2, 3, 5000)), fs=100)
    for kwargs, match in (({"detrend": "quadratic"}, "Trend type"),
                          ({"resolution": 0.01}, "nfft"),                 # nfft 10000 > 5000 samples
                          ({"window": "no such window"}, "window"),
                          ({"method": "coherence"}, "imcoh.*plv.*pli.*wpli.*dwpli"),
                          ({"method": ("wpli", "PLV")}, "PLV.*imcoh"),
                          ({"method": ()}, "imcoh"),
                          ({"method": 3}, None)):
        src = Untouched((4, 5000))
        with pytest.raises((ValueError, TypeError), match=match):
            phase_connectivity(src.pro, fs=100, **kwargs)
        assert not src.started, kwargs
    for shape in ((5000,), (2, 2, 5000)):
        src = Untouched(shape)
        with pytest.raises(ValueError):
            phase_connectivity(src.pro, fs=100, method=METHODS)
        assert not src.started
    with pytest.raises(TypeError):
        phase_connectivity(Untouched((4, 5000)).pro, fs=100, scaling="density")   # no such argument


C_TYPES = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "const double *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("osz_lag_accumulate", 6), ("osz_unit_phasors", 3), ("osz_phase_finish", 10)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared"
        declared = []
        for arg in m.group(1).split(","):
            ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()   # drop the name
            declared.append(C_TYPES[ctype])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(declared) == nargs
        assert argtypes == declared, (name, argtypes, declared)
        assert hasattr(lib, name), f"{name} not exported"
    for k, (name, value) in enumerate(_lib.PHASE_MODE.items()):
        assert value == k and re.search(rf"OSZ_PHASE_{name.upper()} = {k}\b", header)


@pytest.mark.parametrize("case", CASES[:4], ids=lambda c: f"nfft{c[0]}-{c[1]}")
def test_imcoh_is_scipy(case):
    """Im(Pxy) / sqrt(Pxx Pyy) of pairwise scipy.signal.csd / welch, at 1e-12 (imcoh is <= 1)."""
    nfft, window, overlap, detrend, _, _, _ = case
    fs, nch, n = 1000.0, 5, 50000
    kw = dict(fs=fs, window=window, nperseg=nfft, noverlap=int(nfft * overlap), nfft=nfft, detrend=detrend)
    x = signal(nch, n, ramp=True)
    nseg, freqs, M, parts = phase_measures(x, fs, nfft, window, overlap, detrend)
    assert nseg == (n - nfft) // (nfft - int(nfft * overlap)) + 1 == parts["N"]
    inner = np.ones(nfft // 2 + 1, bool)
    inner[real_bins(nfft)] = False
    pxx = [sps.welch(x[i], **kw)[1] for i in range(nch)]
    for i in range(nch):
        for j in range(nch):
            f, pxy = sps.csd(x[i], x[j], **kw)
            assert np.array_equal(f, freqs)
            want = pxy.imag / np.sqrt(pxx[i] * pxx[j])
            if i == j:
                assert np.all(M["imcoh"][i, j] == 0.0)
            else:
                assert np.max(np.abs(M["imcoh"][i, j] - want)[inner]) < 1e-12, (i, j)
                assert np.all(M["imcoh"][i, j][~inner] == 0.0)
    assert np.max(np.abs(M["imcoh"].transpose(1, 0, 2) + M["imcoh"])) < 1e-15


def test_delayed_copy_is_fully_locked():
    """Channel 1 is channel 0 delayed by 3 samples, channel 0 a sum of sinusoids at bin centres
    (so every segment sees the same phase difference, none a multiple of pi): plv, pli and wpli
    of the pair are 1 at those bins (the mean is all the detrending may remove: a fitted line has
    power at every bin and differs from segment to segment).  Channel 2 is unrelated noise."""
    nfft, n, delay = 256, 256 * 8, 3
    bins = np.array([5, 17, 40, 77, 100])
    rng = np.random.default_rng(3)
    t = np.arange(n + delay)
    base = sum(a * np.cos(2 * np.pi * k * t / nfft + ph)
               for k, a, ph in zip(bins, rng.uniform(0.5, 2, 5), rng.uniform(0, 6, 5)))
    x = np.stack([base[delay:], base[:n], rng.standard_normal(n)])
    assert np.all(np.abs(np.sin(2 * np.pi * bins * delay / nfft)) > 0.1)
    for window, detrend in (("hann", "constant"), ("boxcar", "constant")):
        nseg, _, M, _ = phase_measures(x, 256.0, nfft, window, 0.5, detrend)
        assert nseg == 15
        for name in ("plv", "pli", "wpli"):
            assert np.max(np.abs(M[name][0, 1, bins] - 1.0)) < 1e-9, (name, window)
            assert np.max(M[name][0, 2, bins]) < 0.9                    # (the noise is not locked)
        assert np.max(np.abs(M["dwpli"][0, 1, bins] - 1.0)) < 1e-9


def test_invariances():
    """Scaling a channel by a positive number changes nothing; negating a channel changes only
    the sign of imcoh in its row and column."""
    nfft, nch, n = 200, 4, 3000
    x = signal(nch, n, ramp=False, seed=7)
    _, _, M, _ = phase_measures(x, 50.0, nfft, "hann", 0.5, "linear")
    y = x.copy()
    y[1] *= 3.7
    y[3] *= 1e-3
    _, _, Ms, _ = phase_measures(y, 50.0, nfft, "hann", 0.5, "linear")
    y = x.copy()
    y[2] = -y[2]
    _, _, Mn, _ = phase_measures(y, 50.0, nfft, "hann", 0.5, "linear")
    flip = np.ones((nch, nch, 1))
    flip[2, :] = flip[:, 2] = -1
    flip[2, 2] = 1
    for name in METHODS:
        assert np.all(np.isfinite(M[name][..., 1:]))
        assert np.max(np.abs(Ms[name] - M[name])[..., 1:]) < (0 if name == "pli" else 1e-9) + 1e-300, name
        want = M[name] * flip if name == "imcoh" else M[name]
        assert np.array_equal(Mn[name][..., 1:], want[..., 1:]), name
        if name != "imcoh":
            assert np.max(np.abs(M[name] - M[name].transpose(1, 0, 2))) < 1e-12


def test_dwpli_is_its_pairwise_form():
    """sum_{s != t} d_s d_t / sum_{s != t} |d_s d_t| from the segments themselves."""
    nfft, nch, n = 64, 3, 64 * 7
    x = signal(nch, n, ramp=False, seed=11)
    fs = 64.0
    nseg, _, M, _ = phase_measures(x, fs, nfft, "hann", 0.5, "constant")
    win = sps.get_window("hann", nfft)
    X = np.array([np.fft.rfft(sps.detrend(x[:, s * 32:s * 32 + nfft], type="constant") * win)
                  for s in range(nseg)])
    d = (np.conj(X)[:, :, None] * X[:, None]).imag                    # (nseg, C, C, nfreq)
    off = ~np.eye(nseg, dtype=bool)
    num = np.einsum("sijf,tijf,st->ijf", d, d, off)
    den = np.einsum("sijf,tijf,st->ijf", np.abs(d), np.abs(d), off)
    with np.errstate(invalid="ignore"):
        want = num / den                                              # (0 / 0 at the real bins)
    for i in range(nch):
        for j in range(nch):
            if i != j:
                assert np.max(np.abs(M["dwpli"][i, j, 1:-1] - want[i, j, 1:-1])) < 1e-9
