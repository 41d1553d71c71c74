"""CPU-only tests of window_coherence (K27): the names, the argument errors (raised with no GPU and
before the stream is touched), the C ABI and the entry checks of osz_window_coherence and
osz_window_coherence_work through ctypes without a device, the register report of
csrc/windowcoh.hip, and ``window_coherence_measures``, the NumPy restatement that
tests/test_gpu_coherence.py compares the device against.

The restatement is the two restatements the suite already pins, applied window by window:
``test_phase_host.phase_measures`` and ``test_csd_host.welch_cross`` on the samples of each window
alone, then ``numpy.mean`` over the bins of each band.  It is pinned here on what must hold of any
correct one: SciPy's coherence of a slice, a delayed copy that is fully locked, a one-bin band, the
invariances under scaling and negating a channel, and the independence of a window from the rest
of the stream."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.signal as sps

from openseize_amd import _device as dev
from openseize_amd import _lib, features, producer
from openseize_amd.features import coherence as module
from openseize_amd.features.coherence import window_coherence

from test_connectivity_host import ROOT, _hipcc
from test_csd_host import Untouched, signal, welch_cross
from test_phase_host import RTOL, phase_measures

NAMES = ("coh", "imcoh", "plv", "pli", "wpli", "dwpli")
C_TYPES = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "const int *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}

# (C, nperseg, h, nsub, m, nwin, bands in bins [b0, b1)) of tests/test_gpu_coherence.py, which says
# what each is for, and the overlap that gives each stride
SHAPES = [(5, 64, 32, 7, 2, 6, ((1, 5), (8, 13), (13, 31))),
          (17, 64, 32, 4, 1, 5, ((1, 2), (4, 12))),
          (70, 128, 64, 3, 3, 3, ((2, 63),)),
          (9, 256, 64, 5, 4, 3, ((1, 127), (60, 70))),
          (6, 63, 21, 9, 1, 4, ((1, 31),)),
          (2, 8, 4, 2, 2, 3, ((1, 3),))]
OVERLAP = {(64, 32): 0.5, (128, 64): 0.5, (256, 64): 0.75, (63, 21): 0.67, (8, 4): 0.5}


def geometry(shape):
    """(overlap, W, step, n) of a shape: the stream holds its windows and 3 samples of one that is dropped."""
    _, L, h, nsub, m, nwin, _ = shape
    overlap = OVERLAP[L, h]
    assert L - int(L * overlap) == h
    W, step = L + (nsub - 1) * h, m * h
    return overlap, W, step, (nwin - 1) * step + W + 3


def window_coherence_measures(x, fs, nperseg, overlap, window, detrend, nsub, step, bands):
    """The definition, window by window: (nwin, M, parts).  ``bands`` are pairs of bins [b0, b1).
    M maps each of NAMES to its (nwin, nbands, C, C) array: per window k ``phase_measures`` and
    ``welch_cross`` of x[:, k step : k step + W] alone, coh = |S_ij|^2 / (S_ii S_jj) with the
    diagonal 1.0 and the rows of a channel whose power is NaN lost, and ``numpy.mean`` over each
    band's bins.  ``parts[k]`` is window k's ``parts`` of ``phase_measures`` (N, M, xmin, sd, sa,
    sq, unsafe), what the tolerances are built from."""
    h = nperseg - int(nperseg * overlap)
    W = nperseg + (nsub - 1) * h
    nch = x.shape[0]
    nwin = 0 if x.shape[1] < W else (x.shape[1] - W) // step + 1
    M = {name: np.empty((nwin, len(bands), nch, nch)) for name in NAMES}
    parts = []
    for k in range(nwin):
        piece = x[:, k * step:k * step + W]
        nseg, _, per_bin, part = phase_measures(piece, fs, nperseg, window, overlap, detrend)
        assert nseg == nsub == part["N"]
        _, _, S = welch_cross(piece, fs, nperseg, window, overlap, detrend, "density")
        p = np.real(np.einsum("iif->if", S))
        with np.errstate(divide="ignore", invalid="ignore"):
            coh = np.abs(S) ** 2 / (p[:, None] * p[None])
        coh[np.eye(nch, dtype=bool)] = 1.0
        coh[np.isnan(p)[:, None] | np.isnan(p)[None]] = np.nan
        per_bin = dict(per_bin, coh=coh)
        for b, (b0, b1) in enumerate(bands):
            for name in NAMES:
                M[name][k, b] = np.mean(per_bin[name][..., b0:b1], axis=-1)
        parts.append(part)
    return nwin, M, parts


def bounds(parts, bands, nch):
    """The bounds of tests/test_gpu_phase.py's header with N = nsub, per bin and averaged over each
    band: (bound, unsafe, share).  ``bound[name]`` is (nwin, nbands, C, C) or, for plv / imcoh / coh,
    (nwin, 1, 1, 1); ``unsafe`` the band mean of a window's 2 unsafe / N, pli's allowance; ``share``
    the share of sign-unsafe (pair, bin) entries off the diagonal over the bands' bins."""
    nwin, nb = len(parts), len(bands)
    out = {name: np.empty((nwin, nb, nch, nch)) for name in ("wpli", "dwpli")}
    out["plv"] = np.empty((nwin, 1, 1, 1))
    unsafe = np.empty((nwin, nb, nch, nch))
    off = ~np.eye(nch, dtype=bool)
    bad = total = 0
    for k, part in enumerate(parts):
        N, M = part["N"], part["M"]
        out["plv"][k] = 4 * RTOL * M / part["xmin"]
        with np.errstate(divide="ignore", invalid="ignore"):
            wpli = 4 * RTOL * N * M ** 2 / part["sa"]
            dwpli = 16 * RTOL * N * M ** 2 * part["sa"] / (part["sa"] ** 2 - part["sq"])
        for b, (b0, b1) in enumerate(bands):
            out["wpli"][k, b] = np.mean(wpli[..., b0:b1], axis=-1)
            out["dwpli"][k, b] = np.mean(dwpli[..., b0:b1], axis=-1)
            unsafe[k, b] = np.mean(2 * part["unsafe"][..., b0:b1] / N, axis=-1)
            bad += np.count_nonzero(part["unsafe"][off][:, b0:b1])
            total += part["unsafe"][off][:, b0:b1].size
    out["imcoh"] = out["coh"] = out["plv"]
    return out, unsafe, bad / total


# ---- the pins of the restatement

def test_coh_of_a_window_is_scipy():
    """coh of one window against scipy.signal.coherence on that slice, bin by bin through one-bin
    bands, at 1e-12."""
    nch, L, nsub, step = 4, 64, 5, 96
    h = 32
    W = L + (nsub - 1) * h
    x = signal(nch, 3 * step + W, False, seed=3)
    bands = [(k, k + 1) for k in range(1, 31)]
    nwin, M, _ = window_coherence_measures(x, 64.0, L, 0.5, "hann", "constant", nsub, step, bands)
    assert nwin == 4
    for k in (0, 3):
        piece = x[:, k * step:k * step + W]
        for i in range(nch):
            for j in range(nch):
                _, cxy = sps.coherence(piece[i], piece[j], fs=64.0, window="hann", nperseg=L, noverlap=32, nfft=L,
                                       detrend="constant")
                assert np.max(np.abs(M["coh"][k, :, i, j] - cxy[1:31])) < 1e-12, (k, i, j)


def test_delayed_copy_is_fully_locked():
    """Channel 1 is channel 0 delayed by 3 samples, channel 0 a sum of sinusoids at the centres of
    the bins 5 .. 9 (a circular shift inside a periodic signal, a boxcar window, nothing for the
    detrend to remove): plv = pli = wpli = coh = 1 in the band of those bins.  Channel 2 is noise."""
    L, nsub, delay = 64, 4, 3
    W = L + (nsub - 1) * 32
    n = 2 * W
    rng = np.random.default_rng(3)
    t = np.arange(n + delay)
    bins = np.arange(5, 10)
    base = sum(a * np.cos(2 * np.pi * k * t / L + ph)
               for k, a, ph in zip(bins, rng.uniform(0.5, 2, 5), rng.uniform(0, 6, 5)))
    x = np.stack([base[delay:], base[:n], rng.standard_normal(n)])
    assert np.all(np.abs(np.sin(2 * np.pi * bins * delay / L)) > 0.1)
    nwin, M, _ = window_coherence_measures(x, 64.0, L, 0.5, "boxcar", "constant", nsub, W, [(5, 10), (5, 6)])
    assert nwin == 2
    for name in ("plv", "pli", "wpli", "coh", "dwpli"):
        assert np.max(np.abs(M[name][:, :, 0, 1] - 1.0)) < 1e-9, name
    assert np.max(M["plv"][:, 0, 0, 2]) < 0.95 and np.max(M["coh"][:, 0, 0, 2]) < 0.95     # (the noise is not locked)


def test_a_one_bin_band_is_the_bin_and_a_band_is_the_mean():
    nch, L, nsub = 3, 64, 4
    W = L + (nsub - 1) * 32
    x = signal(nch, W + 64, False, seed=5)
    _, M, _ = window_coherence_measures(x, 64.0, L, 0.5, "hann", "constant", nsub, 64, [(7, 8), (7, 10), (8, 9), (9, 10)])
    _, _, per_bin, _ = phase_measures(x[:, 64:64 + W], 64.0, L, "hann", 0.5, "constant")
    for name in NAMES[1:]:
        assert np.array_equal(M[name][1, 0], per_bin[name][..., 7]), name
        third = (M[name][:, 0] + M[name][:, 2] + M[name][:, 3]) / 3
        assert np.max(np.abs(M[name][:, 1] - third)) < 1e-15, name


def test_invariances():
    """Scaling a channel by a positive number moves every measure by rounding only; negating a
    channel changes only the sign of imcoh in its row and column."""
    nch, L, nsub = 4, 64, 5
    W = L + (nsub - 1) * 32
    x = signal(nch, 2 * W, False, seed=7)
    bands = [(1, 6), (6, 31)]
    args = (64.0, L, 0.5, "hann", "linear", nsub, W, bands)
    _, M, _ = window_coherence_measures(x, *args)
    y = x.copy()
    y[1] *= 3.7
    y[3] *= 1e-3
    _, Ms, _ = window_coherence_measures(y, *args)
    y = x.copy()
    y[2] = -y[2]
    _, Mn, _ = window_coherence_measures(y, *args)
    flip = np.ones((nch, nch))
    flip[2, :] = flip[:, 2] = -1
    flip[2, 2] = 1
    for name in NAMES:
        assert np.all(np.isfinite(M[name]))
        assert np.max(np.abs(Ms[name] - M[name])) < 1e-9, name
        want = M[name] * flip if name == "imcoh" else M[name]
        assert np.max(np.abs(Mn[name] - want)) < 1e-12, name


def test_a_window_does_not_know_the_stream():
    """Window k of a long stream is window 0 of the stream cut at k step, whatever the step."""
    nch, L, nsub = 3, 63, 4
    h = 21
    W = L + (nsub - 1) * h
    x = signal(nch, 6 * h + W + 5, False, seed=9)
    args = (63.0, L, 0.67, "hamming", "constant", nsub)
    nwin, M, _ = window_coherence_measures(x, *args, h, [(1, 31)])
    nwin2, M2, _ = window_coherence_measures(x, *args, 2 * h, [(1, 31)])
    assert (nwin, nwin2) == (7, 4)
    for k in range(nwin):
        _, cut, _ = window_coherence_measures(x[:, k * h:], *args, 5 * h, [(1, 31)])
        for name in NAMES:
            assert np.array_equal(M[name][k], cut[name][0]), (name, k)
            if k % 2 == 0:
                assert np.array_equal(M2[name][k // 2], cut[name][0]), (name, k)


def coupled(nsub=31, nwin=8, seed=6):
    """(x, fs, nperseg, W): three channels of white noise; in the first half of the stream channels
    0 and 1 carry one 8 - 13 Hz rhythm, channel 1 a quarter cycle behind channel 0.  ``nwin`` windows
    of ``nsub`` half-overlapping segments of 128 samples at fs = 128, the rhythm on in the first half."""
    fs, L, h = 128.0, 128, 64
    W = L + (nsub - 1) * h
    n = nwin * W
    rng = np.random.default_rng(seed)
    sos = sps.butter(4, [8.0, 13.0], btype="bandpass", fs=fs, output="sos")
    rhythm = sps.sosfiltfilt(sos, rng.standard_normal(n + 2048))[1024:1024 + n]
    analytic = sps.hilbert(rhythm / rhythm.std())
    on = (np.arange(n) < n // 2).astype(float)
    x = 0.5 * rng.standard_normal((3, n))
    x[0] += analytic.real * on
    x[1] += analytic.imag * on
    return x, fs, L, W


def test_a_coupling_that_switches_off_is_followed():
    """imcoh, wpli and coh of the coupled pair are near 1 in the band of the rhythm while it is on and
    small after; a band or a channel without it stays small: with a margin, so that
    tests/test_gpu_coherence.py can rely on 0.5."""
    x, fs, L, W = coupled()
    nwin, M, _ = window_coherence_measures(x, fs, L, 0.5, "hann", "constant", 31, W, [(8, 13), (20, 40)])
    assert nwin == 8
    for name in ("imcoh", "wpli", "coh"):
        print(name, np.round(M[name][:, :, 0, 1].T, 2).tolist(), np.round(M[name][:, 0, 0, 2], 2).tolist())
        assert np.all(np.abs(M[name][:4, 0, 0, 1]) > 0.8), name
        assert np.all(np.abs(M[name][4:, 0, 0, 1]) < 0.4), name
        assert np.all(np.abs(M[name][:, 1, 0, 1]) < 0.4) and np.all(np.abs(M[name][:, 0, 0, 2]) < 0.4), name
    assert np.all(M["imcoh"][:4, 0, 0, 1] < 0)                       # channel 1 lags: conj(X_0) X_1 turns clockwise


def test_the_gpu_shapes_are_safe_to_rely_on():
    """The inputs of tests/test_gpu_coherence.py, on the reference alone: the share of sign-unsafe
    (pair, bin) entries stays ten times below the cap of 1e-3 and every bound is finite and below 1e-3."""
    from test_gpu_coherence import reference
    for shape in SHAPES:
        nch, bands = shape[0], shape[6]
        _, _, _, _, parts = reference(shape)
        bound, _, share = bounds(parts, bands, nch)
        off = ~np.eye(nch, dtype=bool)
        print(shape[:6], f"unsafe share {share:.2e}", {name: float(np.max(b[..., off] if b.shape[-1] > 1 else b))
                                                       for name, b in bound.items()})
        assert share <= 1e-4
        for name, b in bound.items():
            worst = np.max(b[..., off] if b.shape[-1] > 1 else b)
            assert np.isfinite(worst) and worst <= 1e-3, (shape[:6], name, worst)


# ---- the public function

def test_names_are_public():
    assert features.window_coherence is window_coherence and features.WINDOW_COHERENCE == NAMES
    assert module.WINDOW_COHERENCE == NAMES and tuple(_lib.WINDOW_COHERENCE) == NAMES
    assert list(_lib.WINDOW_COHERENCE.values()) == list(range(6)) and _lib.WK_BANDS_MOST == 16
    doc = window_coherence.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc
    for said in ("symmetric bit for bit", "written, not computed", "faverage", "1e-12", "MemoryError"):
        assert said in doc, said


def test_argument_errors_come_before_the_stream():
    x = np.random.default_rng(1).standard_normal((4, 5000))
    ok = dict(fs=64.0, winsize=256, nperseg=64, bands=(4, 8))
    cases = (({"nperseg": None}, "nperseg.*required"), ({"nperseg": 7}, "nperseg must be an integer >= 8, got 7"),
             ({"nperseg": 64.0}, "nperseg"), ({"nperseg": True}, "nperseg"),
             ({"winsize": 256.0}, "winsize"), ({"winsize": True}, "winsize"), ({"step": 32.0}, "step"),
             ({"winsize": 250}, "winsize = 250 must be.*nearest are 224 and 256"),
             ({"winsize": 64}, "winsize = 64 must be.*nearest are 96 and 128"),
             ({"winsize": 40}, "nearest are 96 and 128"),
             ({"step": 48}, "step = 48 a positive multiple of 32 .the nearest are 32 and 64"),
             ({"step": 0}, "step"), ({"step": 10}, "nearest are 32 and 64"),
             ({"winsize": 112, "overlap": 0.25, "step": None}, "step = 112 a positive multiple of 48"),
             ({"overlap": 1.0}, "overlap must be a number in .0, 1., got 1.0"), ({"overlap": -0.1}, "overlap"),
             ({"overlap": "half"}, "overlap"),
             ({"bands": None}, "bands is required"), ({"bands": ()}, "bands must be"), ({"bands": (4,)}, "bands must be"),
             ({"bands": [(4, 8)] * 17}, "1 to 16 pairs"), ({"bands": [(4, float("nan"))]}, "bands must be"),
             ({"bands": (8, 4)}, "holds no bin"), ({"bands": (4.1, 4.9)}, "holds no bin"),
             ({"bands": (0, 8)}, "does not lie within the bins 1 .. 31"),
             ({"bands": [(4, 8), (20, 33)]}, "does not lie within the bins 1 .. 31"),     # (the Nyquist bin of 64)
             ({"fs": 0}, "fs must be a positive finite number"), ({"fs": "64"}, "fs"),
             ({"detrend": "quadratic"}, "detrend must be 'constant' or 'linear', got 'quadratic'"),
             ({"window": "no such window"}, "window"),
             ({"measures": "COH"}, "coh.*imcoh.*plv.*pli.*wpli.*dwpli"), ({"measures": ("coh", "ciplv")}, "ciplv.*dwpli"),
             ({"measures": ()}, "coh"))
    for change, match in cases:
        kwargs = dict(ok, **change)
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_coherence(src.pro, **kwargs)
        assert not src.started, change
        with pytest.raises(ValueError, match=match):
            window_coherence(x, **kwargs)
    for shape, match in (((5000,), "two-dimensional"), ((2, 2, 5000), "two-dimensional"), ((1, 5000), "two channels"),
                         ((4, 200), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_coherence(src.pro, **ok)
        assert not src.started
    with pytest.raises(ValueError, match="takes real data, got complex128 data"):
        window_coherence(x.astype(complex), **ok)

    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    with pytest.raises(ValueError, match="takes real data, got complex128 chunks"):
        window_coherence(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), **ok)
    with pytest.raises(TypeError):
        window_coherence(x, scaling="density", **ok)                         # no such argument
    # an odd nperseg has no Nyquist bin: its last bin is allowed, an even one's is not
    assert module._bands((1, 32), np.fft.rfftfreq(63, 1 / 63.0), 31) == ([(1, 32)], True)
    assert module._bands([(1, 32)], np.fft.rfftfreq(64, 1 / 64.0), 31) == ([(1, 32)], False)
    with pytest.raises(ValueError, match="does not lie within"):
        module._bands((1, 33), np.fft.rfftfreq(64, 1 / 64.0), 31)


# ---- the C ABI

def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_coherence_work", "int64_t", 7), ("osz_window_coherence", "int", 14)):
        m = re.search(r"\b" + ret + " " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared"
        declared = []
        for arg in m.group(1).split(","):
            ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()   # drop the name
            declared.append(C_TYPES[ctype])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C_TYPES[ret] and len(declared) == nargs
        assert argtypes == declared, (name, argtypes, declared)
        assert hasattr(lib, name), f"{name} not exported"
    for name, value in _lib.WINDOW_COHERENCE.items():
        assert re.search(rf"OSZ_WK_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WK_COUNT = 6\b", header)
    assert re.search(rf"#define OSZ_WK_BANDS_MOST {_lib.WK_BANDS_MOST}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowcoh\.hip\b", makefile, re.M)
    assert callable(dev.window_coherence)


# ---- the entry checks, through ctypes without a device (as tests/test_te_host.py: the pointers are
# fake addresses nothing dereferences and every case holds fewer segments than a window, so a check
# that wrongly passed returns OSZ_OK, which fails the assertion, and cannot reach a launch)
X, OUT, WORK = 0x1000, 0x2000, 0x3000                      # 16-byte aligned, never read
NSEG, NCH, NFREQ, NSUB = 3, 3, 33, 4


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def arguments(**change):
    a = dict(x=X, nseg=NSEG, nch=NCH, nfreq=NFREQ, nsub=NSUB, mstep=2, bands=[(1, 5), (8, 32)], nbands=None, mask=63,
             out=OUT, plane_pitch=0, work=WORK, work_len=0)
    a.update(change)
    if a["nbands"] is None:
        a["nbands"] = len(a["bands"]) if a["bands"] is not None else 1
    assert a["nseg"] < a["nsub"] or a["nsub"] < 2, "every case is one without a window"
    return a


def work_of(lib, **change):
    a = arguments(**change)
    return lib.osz_window_coherence_work(a["nseg"], a["nch"], a["nfreq"], a["nsub"], a["mstep"], a["nbands"], a["mask"])


def call(lib, **change):
    a = arguments(**change)
    barr = None
    if a["bands"] is not None:
        flat = [b for pair in a["bands"] for b in pair]
        barr = ctypes.cast((ctypes.c_int * max(len(flat), 1))(*flat), ctypes.c_void_p)
    status = lib.osz_window_coherence(a["x"], a["nseg"], a["nch"], a["nfreq"], a["nsub"], a["mstep"], barr, a["nbands"],
                                      a["mask"], a["out"], a["plane_pitch"], a["work"], a["work_len"], None)
    return status, lib.osz_last_error().decode()


def test_the_work_space_query_needs_no_device(lib):
    work = lib.osz_window_coherence_work
    assert work(100, 3, 33, 4, 2, 2, 63) == 0                  # the sums stay in registers: no work space
    assert work(0, 2, 2, 2, 1, 1, 1) == 0 and work(2 ** 31 - 1, 16384, 8191, 2, 1, 16, 32) == 0
    for bad in ((-1, 3, 33, 4, 2, 2, 63), (2 ** 31, 3, 33, 4, 2, 2, 63), (100, 1, 33, 4, 2, 2, 63),
                (100, 16385, 33, 4, 2, 2, 63), (100, 3, 1, 4, 2, 2, 63), (100, 16384, 8192, 4, 2, 2, 63),
                (100, 3, 33, 1, 2, 2, 63), (100, 3, 33, 4, 0, 2, 63), (100, 3, 33, 4, 2, 0, 63),
                (100, 3, 33, 4, 2, 17, 63), (100, 3, 33, 4, 2, 2, 0), (100, 3, 33, 4, 2, 2, 64)):
        assert work(*bad) == -1, bad


def test_valid_arguments_without_a_window_are_accepted(lib):
    status, msg = call(lib)
    assert status == _lib.OSZ_OK, msg
    for edge in (dict(nseg=0), dict(nch=16384, nfreq=8191, bands=[(1, 8191)]), dict(nsub=2, nseg=1), dict(mask=1),
                 dict(mask=32), dict(work=None), dict(bands=[(k, k + 1) for k in range(1, 17)]), dict(bands=[(32, 33)]),
                 dict(mstep=2 ** 31 - 1)):
        status, msg = call(lib, **edge)                       # the ends of the ranges
        assert status == _lib.OSZ_OK and work_of(lib, **edge) == 0, (edge, msg)


BAD = {
    "null X": (dict(x=None), "null", False),
    "null bands": (dict(bands=None), "null", False),
    "null out": (dict(out=None), "null", False),
    "negative nseg": (dict(nseg=-1), "nseg -1,", True),
    "nch 1": (dict(nch=1), "nch 1,", True),
    "nch 16385": (dict(nch=16385), "nch 16385,", True),
    "nfreq 1": (dict(nfreq=1, bands=[(1, 2)]), "nfreq 1,", True),
    "nsub 1": (dict(nsub=1), "nsub 1,", True),
    "mstep 0": (dict(mstep=0), "mstep 0,", True),
    "no band": (dict(bands=[], nbands=0), "nbands 0,", True),
    "17 bands": (dict(bands=[(1, 2)] * 17), "nbands 17,", True),
    "mask 0": (dict(mask=0), "mask 0", True),
    "mask past the last bit": (dict(mask=64), "mask 64", True),
    "band from DC": (dict(bands=[(0, 5)]), "band 0, bins [0, 5), is empty or outside 1 .. 32", False),
    "band past the last bin": (dict(bands=[(1, 5), (8, 34)]), "band 1, bins [8, 34), is empty or outside 1 .. 32", False),
    "empty band": (dict(bands=[(5, 5)]), "band 0, bins [5, 5), is empty", False),
    "reversed band": (dict(bands=[(9, 5)]), "band 0, bins [9, 5), is empty", False),
    "plane_pitch below": (dict(plane_pitch=-1), "plane_pitch -1 holds fewer than 0 windows", False),
    "X not aligned": (dict(x=X + 8), "aligned", False),
    "out not aligned": (dict(out=OUT + 4), "aligned", False),
    "work not aligned": (dict(work=WORK + 4), "aligned", False),
    "work_len below": (dict(work_len=-1), "work holds -1 doubles", False),
}


@pytest.mark.parametrize("label", list(BAD))
def test_a_bad_argument_is_refused(lib, label):
    change, says, planned = BAD[label]
    status, msg = call(lib, **change)
    assert status == _lib.OSZ_ERR_INVALID, (status, msg)
    assert msg.startswith("osz_window_coherence: ") and re.search(re.escape(says) + r"(?!\d)", msg), msg
    assert (work_of(lib, **change) == -1) == planned


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_coherence_kernels_fit_their_budgets(tmp_path):
    """Every kernel of windowcoh.hip, compiled for gfx950 with the library's flags: the three
    instances, no scratch, no spilled register of either kind, at most 256 VGPRs (two workgroups a
    CU) and the 32.5 KB stage and 2 KB turn of static LDS."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowcoh.hip"), "-o", str(tmp_path / "windowcoh.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=csrc)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\S+)", line)
        if not m:
            continue
        if m.group(1).strip() == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    assert len(kernels) == 3 and all("window_coherence_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 256
        assert int(use["LDS Size"]) <= 36 * 1024
