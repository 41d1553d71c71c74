"""CPU-only tests of jackknife (K12): the names, the argument errors (raised with no GPU and
before the stream is touched), the C ABI of the entry points against the header,
``jackknife_interval``, and the two NumPy yardsticks that tests/test_gpu_jackknife.py compares
the device against:

``literal_jackknife``    for every s the measures are recomputed from the spectra without segment
                         s (``np.delete(X, s, 0)``) by the published definitions -- those of
                         ``test_phase_host.phase_measures``, plus coherence;
``downdated_jackknife``  theta_(s) from the totals minus segment s's contribution, the table of
                         ``jackknife``'s docstring: what the kernel does.

Both take se^2 = (N - 1) / N (sum d_s^2 - (sum d_s)^2 / N), d_s = theta_(s) - theta -- the literal
form as sum (d_s - mean d)^2, which is that number without the rounding of the subtraction, the
downdated form from the two running sums with the device's floor -- and write the fixed points.  They are pinned here: against each other on every
input the GPU tests use (which pins the inputs' conditioning: the downdate cancels where a
segment dominates a sum), by the invariances under scaling and negating a channel, and by a pair
that is a pure delay of one signal (plv, pli, wpli do not vary: se = 0)."""

import ctypes
import os
import re
from functools import lru_cache

import numpy as np
import pytest
import scipy.signal as sps
from scipy.stats import t as student

from openseize_amd import _lib
from openseize_amd.spectra import estimators, metrics
from openseize_amd.spectra.estimators import jackknife

from test_csd_host import CASES, Untouched, rate, signal
from test_phase_host import C_TYPES, RTOL, real_bins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("coherence", "imcoh", "plv", "pli", "wpli", "dwpli")

# what the GPU tests run on.  The kernel alone: (channels, segments) of Gaussian spectra with
# NFREQ bins (one full block of 64 lanes and a partial one), channel counts across the lane's
# 4-channel register tile and the 8- and 16-channel workgroup blocks
NFREQ = 101
KERNEL_SHAPES = [(nch, nseg) for nch in (2, 5, 9, 17) for nseg in (2, 3, 7)]
# end to end, (nfft, window, overlap, detrend, channels, samples, seed): the first four routes of
# the windowed DFT, then 12 segments of 101 bins around the tile edges
STREAM_SHAPES = [(c[0], c[1], c[2], c[3], c[5], c[6], 0) for c in CASES[:4]]
STREAM_SHAPES += [(200, "hann", 0.5, "constant", nch, 1300, nch) for nch in (5, 9, 17)]
STREAM_IDS = [f"nfft{s[0]}-{s[1]}-{s[3]}-{s[4]}ch" for s in STREAM_SHAPES]


def gaussian_spectra(nch, nseg, nfreq=NFREQ):
    """(nseg, nch, nfreq) complex Gaussian values, seeded by the shape."""
    rng = np.random.default_rng(1000 * nch + nseg)
    return rng.standard_normal((nseg, nch, nfreq)) + 1j * rng.standard_normal((nseg, nch, nfreq))


def segment_spectra(x, fs, nfft, window, overlap, detrend):
    """(nseg, C, nfreq) Welch segment spectra of x (C, n), cut, detrended, windowed and scaled
    as in ``test_phase_host.phase_measures``."""
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
    return np.array(X) * np.sqrt(1 / (fs * np.sum(win ** 2)))


@lru_cache(maxsize=None)
def stream_input(shape):
    """(x, fs, resolution, X) of a STREAM_SHAPES row, read-only."""
    nfft, window, overlap, detrend, nch, n, seed = shape
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=False, seed=seed)
    X = segment_spectra(x, fs, nfft, window, overlap, detrend)
    x.setflags(write=False)
    X.setflags(write=False)
    return x, fs, resolution, X


def _terms(X):
    """What one segment adds to each sum, for the pairs i <= j: z = conj(X_i) X_j, u = z / |z|,
    d = Im z, |d|, d^2, sign d -- (nseg, pairs, nfreq) each -- and p = |X|^2 (nseg, C, nfreq).
    Every one is elementwise in the segment: the terms of ``np.delete(X, s, 0)`` are
    ``np.delete(terms, s, 0)``, value for value."""
    iu, ju = np.triu_indices(X.shape[1])
    z = np.conj(X[:, iu]) * X[:, ju]
    d = z.imag
    return dict(z=z, u=z / np.abs(z), d=d, a=np.abs(d), q=d * d, g=np.sign(d), p=np.abs(X) ** 2), iu, ju


def _measures(S, n, iu, ju):
    """The published definitions from the sums S over n segments (pairs i <= j)."""
    pp = S["p"][iu] * S["p"][ju]
    return {"coherence": np.abs(S["z"]) ** 2 / pp,
            "imcoh": S["z"].imag / np.sqrt(pp),
            "plv": np.abs(S["u"]) / n,
            "pli": np.abs(S["g"]) / n,
            "wpli": np.abs(S["d"]) / S["a"],
            "dwpli": (S["d"] ** 2 - S["q"]) / (S["a"] ** 2 - S["q"])}


BLOCK = 128           # bins worked on at a time: everything here is elementwise in the bin


def _standard_errors(X, nfft, prepare, one_pass):
    """se of every method.  ``prepare(terms, totals)`` returns the function s -> the sums without
    segment s.  ``one_pass``: the variance as the device takes it, sum d^2 - (sum d)^2 / N from
    running sums, 0 where it does not exceed the 4 N 2^-53 sum d^2 its own subtraction may
    carry; else the same number as sum (d_s - mean d)^2, which carries no such rounding.
    -> (se: name -> (C, C, nfreq), unsafe: per entry the segments with |d_s| < 20 RTOL max|X|^2)."""
    n, nch, nfreq = X.shape
    iu, ju = np.triu_indices(nch)
    half = {m: np.empty((len(iu), nfreq)) for m in METHODS}
    doubt = np.empty((len(iu), nfreq), int)
    tiny = 20 * RTOL * np.nanmax(np.abs(X)) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo in range(0, nfreq, BLOCK):
            at = slice(lo, lo + BLOCK)
            T = _terms(X[..., at])[0]
            total = {k: v.sum(0) for k, v in T.items()}
            theta = _measures(total, n, iu, ju)
            without = prepare(T, total)
            devs = {m: np.empty((n,) + theta[m].shape) for m in METHODS}
            for s in range(n):
                left = _measures(without(s), n - 1, iu, ju)
                for m in METHODS:
                    devs[m][s] = left[m] - theta[m]
            for m in METHODS:
                if one_pass:
                    s1, s2 = np.zeros(theta[m].shape), np.zeros(theta[m].shape)
                    for dev in devs[m]:
                        s1 += dev
                        s2 += dev * dev
                    var = s2 - s1 ** 2 / n
                    var = np.where(var <= 4 * n * 2.0 ** -53 * s2, 0.0, var)      # (false for a NaN: it stays)
                else:
                    var = np.sum((devs[m] - np.sum(devs[m], 0) / n) ** 2, 0)
                half[m][:, at] = np.sqrt((n - 1) / n * var)
            doubt[:, at] = np.sum(T["a"] < tiny, axis=0)
        own = {m: np.sum(np.abs(X) ** 2, axis=0) for m in METHODS}
        own["plv"] = np.sum(np.abs(X / np.abs(X)) ** 2, axis=0)       # (0 / 0 where X is 0, as the device)
    se = {}
    for m in METHODS:
        full = np.zeros((nch, nch, nfreq))
        full[iu, ju] = half[m]
        full[ju, iu] = half[m]
        if m != "plv":
            full[..., real_bins(nfft)] = 0.0
        full[np.eye(nch, dtype=bool)] = 0.0
        lost = np.isnan(own[m])
        full[lost[:, None] | lost[None]] = np.nan
        se[m] = full
    unsafe = np.zeros((nch, nch, nfreq), int)
    unsafe[iu, ju] = doubt
    unsafe[ju, iu] = doubt
    return se, unsafe


def literal_jackknife(X, nfft, delete=False):
    """The definition: for every s each sum is taken again over the N - 1 other segments, and
    the measures from those sums.  ``delete``: literally ``np.delete(terms, s, 0).sum(0)``, N^2
    additions per entry; otherwise the same N - 1 terms added as (those before s, in order) +
    (those after s, in order) from two running sums -- nothing is ever subtracted -- which is what
    13 channels x 120 segments can afford (the two are compared in this file).  The variance is
    taken about the mean of the d_s: the same number as sum d^2 - (sum d)^2 / N, without the
    rounding of that subtraction, which a square root turns into 1e-8 where the d_s are equal
    (two segments: coherence, plv, pli and wpli of the one segment left are 1; pli where the
    signs balance)."""
    def prepare(T, total):
        if delete:
            return lambda s: {k: np.delete(v, s, 0).sum(0) for k, v in T.items()}
        before = {k: np.cumsum(v, 0) for k, v in T.items()}
        after = {k: np.cumsum(v[::-1], 0)[::-1] for k, v in T.items()}
        last = X.shape[0] - 1
        return lambda s: {k: (before[k][s - 1] if s else 0.0) + (after[k][s + 1] if s < last else 0.0) for k in T}
    return _standard_errors(X, nfft, prepare, one_pass=False)


def downdated_jackknife(X, nfft):
    """The table: the totals minus what segment s added, and the variance from the two running
    sums, as on the device.  With two segments dwpli's theta_(s) is (d^2 - d^2) / (|d|^2 - d^2) of
    the one segment left, which a downdate only rounds to: there it is the NaN of the definition,
    as on the device."""
    def prepare(T, total):
        def without(s):
            S = {k: total[k] - v[s] for k, v in T.items()}
            if X.shape[0] == 2:
                S["q"] = S["d"] ** 2
                S["a"] = np.abs(S["d"])
            return S
        return without
    return _standard_errors(X, nfft, prepare, one_pass=True)


def nfft_of(nfreq):
    """An nfft with nfreq bins whose last bin is not real (odd), for spectra that are not a DFT."""
    return 2 * nfreq - 1


def test_names_are_public():
    assert callable(estimators.jackknife) and callable(metrics.jackknife_interval)
    assert estimators.JACKKNIFE_METHODS == METHODS == ("coherence",) + estimators.PHASE_METHODS
    assert tuple(_lib.JACK_MODE) == METHODS and list(_lib.JACK_MODE.values()) == [0, 1, 2, 3, 4, 5]
    doc = " ".join(jackknife.__doc__.split())
    for name in METHODS:
        assert f'"{name}"' in doc
    for phrase in ("(N - 1) / N (sum_s d_s^2 - (sum_s d_s)^2 / N)", "clamped at 0", "at least two segments",
                   "16 B per (pair, bin) per method", "not independent", "overlap=0", "N = 2", "RuntimeError"):
        assert phrase in doc, phrase


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="psd"):
        jackknife(rng.standard_normal(5000), fs=100)                      # one channel
    with pytest.raises(ValueError, match="two-dimensional"):
        jackknife(rng.standard_normal((2, 3, 5000)), fs=100)
    for kwargs, match in (({"detrend": "quadratic"}, "Trend type"),
                          ({"resolution": 0.01}, "nfft"),                 # nfft 10000 > 5000 samples
                          ({"window": "no such window"}, "window"),
                          ({"method": "csd"}, "coherence.*imcoh.*plv.*pli.*wpli.*dwpli"),
                          ({"method": ("wpli", "Coherence")}, "Coherence.*coherence"),
                          ({"method": ()}, "coherence"),
                          ({"method": 3}, None)):
        src = Untouched((4, 5000))
        with pytest.raises((ValueError, TypeError), match=match):
            jackknife(src.pro, fs=100, **kwargs)
        assert not src.started, kwargs
    for shape in ((5000,), (2, 2, 5000)):
        src = Untouched(shape)
        with pytest.raises(ValueError):
            jackknife(src.pro, fs=100, method=METHODS)
        assert not src.started
    # nfft 200 at a stride of 100: 299 samples hold one segment, 300 would hold two
    for shape, axis in (((4, 299), -1), ((200, 4), 0)):
        src = Untouched(shape, axis=axis)
        with pytest.raises(ValueError, match="at least two segments"):
            jackknife(src.pro, fs=100, axis=axis, method=METHODS)
        assert not src.started
    with pytest.raises(TypeError):
        jackknife(Untouched((4, 5000)).pro, fs=100, scaling="density")    # no such argument


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("osz_jackknife_accumulate", 11), ("osz_jackknife_finish", 11)):
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
    for k, (name, value) in enumerate(_lib.JACK_MODE.items()):
        assert value == k and re.search(rf"OSZ_JACK_{name.upper()} = {k}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bjackknife\.hip\b", makefile, re.M)


def agree(got, want, tol):
    """NaN where want is NaN and nowhere else; elsewhere within tol max(1, |want|).
    -> the largest error over that scale."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    both = np.isinf(want) & ok
    assert np.array_equal(got[both], want[both])
    ok &= ~np.isinf(want)
    if not ok.any():
        return 0.0
    worst = float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))))
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("nch,nseg", KERNEL_SHAPES)
def test_the_two_forms_agree_on_the_kernel_inputs(nch, nseg):
    X = gaussian_spectra(nch, nseg)
    lit, _ = literal_jackknife(X, nfft_of(NFREQ))
    down, _ = downdated_jackknife(X, nfft_of(NFREQ))
    for m in METHODS:
        print(f"{m} {nch} ch x {nseg} segments: {agree(down[m], lit[m], 1e-11):.1e}")
    if nseg == 2:
        off = ~np.eye(nch, dtype=bool)
        assert np.all(np.isnan(lit["dwpli"][off][:, 1:]))            # 0 / 0 everywhere, as documented
        assert np.all(np.isfinite(lit["wpli"][off][:, 1:]))


def test_the_literal_form_is_np_delete():
    """The two running sums of ``literal_jackknife`` against ``np.delete(...).sum(0)``."""
    for X, nfft in ((gaussian_spectra(5, 7), nfft_of(NFREQ)), (gaussian_spectra(9, 3), nfft_of(NFREQ)),
                    (gaussian_spectra(2, 2), nfft_of(NFREQ)), (stream_input(STREAM_SHAPES[4])[3], 200)):
        fast, unsafe = literal_jackknife(X, nfft)
        slow, unsafe_slow = literal_jackknife(X, nfft, delete=True)
        assert np.array_equal(unsafe, unsafe_slow)
        for m in METHODS:
            cut = slice(1, None) if m == "plv" else slice(None)
            agree(fast[m][..., cut], slow[m][..., cut], 1e-13)


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=STREAM_IDS)
def test_the_two_forms_agree_on_the_stream_inputs(shape):
    nfft = shape[0]
    X = stream_input(shape)[3]
    assert X.shape[0] >= 12
    lit, unsafe = literal_jackknife(X, nfft)
    down, _ = downdated_jackknife(X, nfft)
    for m in METHODS:
        cut = slice(1, None) if m == "plv" else slice(None)         # (bin 0: the phase of rounding noise)
        print(f"{m} {STREAM_IDS[STREAM_SHAPES.index(shape)]}: {agree(down[m][..., cut], lit[m][..., cut], 1e-11):.1e}")
        assert np.array_equal(lit[m], lit[m].transpose(1, 0, 2), equal_nan=True)
    inner = np.ones(unsafe.shape, bool)
    inner[np.eye(shape[4], dtype=bool)] = False
    inner[..., real_bins(nfft)] = False
    assert np.mean(unsafe[inner] > 0) <= 1e-3


def test_fixed_points_and_nan_rows():
    X = gaussian_spectra(5, 7, 33).copy()
    X[..., 0] = X[..., 0].real
    X[..., -1] = X[..., -1].real
    X[3, 2] = np.nan
    for form in (literal_jackknife, downdated_jackknife):
        se, _ = form(X, 64)
        for m in METHODS:
            assert np.all(np.isnan(se[m][2])) and np.all(np.isnan(se[m][:, 2])), m
            rest = np.delete(np.delete(se[m], 2, 0), 2, 1)
            assert np.all(np.isfinite(rest))
            assert np.all(rest[np.eye(4, dtype=bool)] == 0.0)
            if m != "plv":
                assert np.all(rest[..., [0, -1]] == 0.0)
                # (where all the d_s have one sign pli, wpli and dwpli are 1 whichever segment is left
                # out, and pli's deviations are equal too where the signs balance: a true 0)
                inner = rest[~np.eye(4, dtype=bool)][:, 1:-1]
                assert np.all(inner > 0.0) if m in ("coherence", "imcoh") else np.mean(inner > 0.0) > 0.9
            else:
                # real spectra: u = +-1, plv and its se are computed and the se is not zero everywhere
                assert np.any(rest[..., [0, -1]] > 0.0)


def test_scaling_or_negating_a_channel_changes_no_standard_error():
    nfft, nch, n = 200, 4, 3000
    x = signal(nch, n, ramp=False, seed=7)
    se, _ = literal_jackknife(segment_spectra(x, 50.0, nfft, "hann", 0.5, "linear"), nfft)
    y = x.copy()
    y[1] *= 3.7
    y[3] *= 1e-3
    scaled, _ = literal_jackknife(segment_spectra(y, 50.0, nfft, "hann", 0.5, "linear"), nfft)
    y = x.copy()
    y[2] = -y[2]
    negated, _ = literal_jackknife(segment_spectra(y, 50.0, nfft, "hann", 0.5, "linear"), nfft)
    off = ~np.eye(nch, dtype=bool)
    for m in METHODS:
        assert np.all(np.isfinite(se[m][..., 1:])) and np.mean(se[m][off][:, 1:-1] > 0.0) > 0.9
        assert np.max(np.abs(scaled[m] - se[m])[..., 1:]) < 1e-9, m
        # (imcoh changes sign in row and column 2, and every deviation with it)
        assert np.max(np.abs(negated[m] - se[m])[..., 1:]) < 1e-13, m


def test_a_pure_delay_has_no_spread():
    """The pair of test_phase_host.test_delayed_copy_is_fully_locked: channel 1 is channel 0 delayed
    by 3 samples, sinusoids at bin centres, so the phase difference is the same in every segment
    and never a multiple of pi: plv = pli = wpli = 1 whichever segment is left out, se = 0.
    Against unrelated noise (channel 2) the spread is there."""
    nfft, n, delay = 256, 256 * 8, 3
    bins = np.array([5, 17, 40, 77, 100])
    rng = np.random.default_rng(3)
    t = np.arange(n + delay)
    base = sum(a * np.cos(2 * np.pi * k * t / nfft + ph)
               for k, a, ph in zip(bins, rng.uniform(0.5, 2, 5), rng.uniform(0, 6, 5)))
    x = np.stack([base[delay:], base[:n], rng.standard_normal(n)])
    for window in ("hann", "boxcar"):
        X = segment_spectra(x, 256.0, nfft, window, 0.5, "constant")
        assert X.shape[0] == 15
        for form in (literal_jackknife, downdated_jackknife):
            se, _ = form(X, nfft)
            for m in ("plv", "pli", "wpli"):
                assert np.max(se[m][0, 1, bins]) < 1e-9, (m, window)
                assert np.min(se[m][0, 2, bins]) > 1e-3, (m, window)


def test_interval_is_students_t_by_hand():
    rng = np.random.default_rng(2)
    est, se = rng.random((3, 3, 17)), 0.1 * rng.random((3, 3, 17))
    for n, alpha in ((12, 0.05), (2, 0.05), (99, 0.01)):
        lower, upper = metrics.jackknife_interval(est, se, n, alpha)
        q = student.ppf(1 - alpha / 2, n - 1)
        assert isinstance(lower, np.ndarray) and lower.shape == est.shape
        assert np.array_equal(lower, est - q * se) and np.array_equal(upper, est + q * se)
    assert abs(student.ppf(0.975, 11) - 2.200985160082949) < 1e-12          # (the tabulated 2.201)
    lower, upper = metrics.jackknife_interval(est, se, 12)
    assert np.allclose(upper - lower, 2 * 2.200985160082949 * se, rtol=1e-12, atol=0)
    # nothing is clipped: a small estimate's interval reaches below 0
    lower, _ = metrics.jackknife_interval(np.array([0.01]), np.array([0.05]), 12)
    assert lower[0] < 0
    with pytest.raises(ValueError):
        metrics.jackknife_interval(est, se, 1)


def test_interval_of_tensors_is_tensors():
    import torch
    rng = np.random.default_rng(4)
    est, se = rng.random((2, 2, 9)), 0.1 * rng.random((2, 2, 9))
    lower, upper = metrics.jackknife_interval(torch.from_numpy(est), torch.from_numpy(se), 12)
    assert torch.is_tensor(lower) and torch.is_tensor(upper) and lower.dtype == torch.float64
    want = metrics.jackknife_interval(est, se, 12)
    assert np.array_equal(lower.numpy(), want[0]) and np.array_equal(upper.numpy(), want[1])
