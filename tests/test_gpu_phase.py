"""GPU tests of phase_connectivity (K11) against ``phase_measures``, the NumPy restatement of
the definitions that tests/test_phase_host.py pins.

Tolerances are first-order bounds computed from the yardstick's own spectra, with the suite's
RTOL = 1e-9 of M = max|X| as the error of a spectrum value (tests/test_gpu_parity.py), N segments:
  plv, imcoh   4 RTOL M / min|X|: a unit phasor X / |X| moves by at most RTOL M / |X|, a product
               of two by twice that, and so does their mean; imcoh is a ratio of sums of the
               same products.  min|X| is taken over the bins that are not real; plv is compared
               at the Nyquist bin too, there with min|X| of that bin (and not at bin 0, which
               holds what detrending left of the mean);
  wpli         4 RTOL N M^2 / min sum|d_s|: every d_s moves by at most 2 RTOL M^2, numerator and
               denominator by N times that;
  dwpli        16 RTOL N M^2 sum|d| / ((sum|d|)^2 - sum d^2), per entry: the same for the squares;
each asserted to be <= 1e-4 on the yardstick alone.  pli counts signs: an entry is sign-safe when
every |d_s| >= 20 RTOL M^2; safe entries agree to 1e-12, an entry with k unsafe segments may
differ by 2k / N, and at most 0.1 % of the entries may be unsafe.  Two routes to one estimate
agree to 1e-12; what must be the same bits is compared as bits."""

from functools import lru_cache

import numpy as np
import pytest

from test_csd_host import CASES, rate, signal
from test_phase_host import METHODS, RTOL, phase_measures, real_bins

pytestmark = pytest.mark.gpu

SAME = 1e-12
LOOSEST = 1e-4
# (nfft, window, overlap, detrend, channels, samples, seed): the first four routes of the windowed
# DFT, then the tile edges: 12 segments of 101 bins (one full and one partial block of 64) at
# channel counts around the lane's 4-channel register tile and the workgroup's 8-channel block
SHAPES = [(c[0], c[1], c[2], c[3], c[5], c[6], 0) for c in CASES[:4]]
SHAPES += [(200, "hann", 0.5, "constant", nch, 1300, nch) for nch in (2, 5, 7, 8, 9, 13, 70)]
IDS = [f"nfft{s[0]}-{s[1]}-{s[3]}-{s[4]}ch" for s in SHAPES]


@pytest.fixture(scope="module")
def est():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()      # fails loudly if the HIP library was not built
    from openseize_amd.spectra import estimators
    return estimators


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint64)


@lru_cache(maxsize=None)
def yardstick(shape):
    nfft, window, overlap, detrend, nch, n, seed = shape
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=False, seed=seed)
    x.setflags(write=False)
    return (x, fs, resolution) + phase_measures(x, fs, nfft, window, overlap, detrend)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_measures_are_the_yardstick(est, shape):
    nfft, window, overlap, detrend, nch, n, _ = shape
    x, fs, resolution, nseg, freqs, want, parts = yardstick(shape)
    cnt, f, got = est.phase_connectivity(x, fs, method=METHODS, resolution=resolution, window=window,
                                         overlap=overlap, detrend=detrend)
    assert cnt == nseg and np.array_equal(f, freqs) and tuple(got) == METHODS
    nfreq = nfft // 2 + 1
    inner = np.ones((nch, nch, nfreq), bool)               # what is computed, not written
    inner[np.eye(nch, dtype=bool)] = False
    inner[..., real_bins(nfft)] = False
    N, M = parts["N"], parts["M"]
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = {"plv": 4 * RTOL * M / parts["xmin"],
                 "wpli": 4 * RTOL * N * M ** 2 / np.min(parts["sa"][inner]),
                 "dwpli": 16 * RTOL * N * M ** 2 * parts["sa"] / (parts["sa"] ** 2 - parts["sq"])}
    bound["imcoh"] = bound["plv"]
    diag = np.eye(nch, dtype=bool)
    for name in METHODS:
        m = got[name]
        assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (nch, nch, nfreq)
        # the fixed points
        if name == "plv":
            # (at bin 0 a detrended channel may be exactly 0 in a segment: 0 / 0, NaN by the rule)
            assert np.all(m[diag][:, 1:] == 1.0) and np.all((m[diag][:, 0] == 1.0) | np.isnan(m[diag][:, 0]))
        else:
            assert np.all(m[diag] == 0.0), name
        if name != "plv":
            assert np.all(m[..., real_bins(nfft)] == 0.0), name
        if name == "imcoh":
            assert np.array_equal(m.transpose(1, 0, 2), -m)
        else:
            assert np.array_equal(bits(m.transpose(1, 0, 2)), bits(m))
        where = inner
        err = np.abs(m - want[name])
        if name == "plv" and nfft % 2 == 0:
            # the Nyquist bin is computed too for plv (bin 0 is the phase of rounding noise)
            last = 4 * RTOL * M / parts["xlast"]
            print(f"plv nfft {nfft} x {nch}, last bin: max err {np.max(err[~diag, -1]):.2e}, bound {last:.2e}")
            assert np.all(err[~diag, -1] <= last)
        if name == "pli":
            safe = parts["unsafe"] == 0
            share = float(np.mean(~safe[where]))
            worst = float(np.max(err[where & safe], initial=0.0))
            print(f"pli nfft {nfft} x {nch}: {share:.5f} of the entries unsafe, safe ones differ by {worst:.1e}")
            assert share <= 1e-3
            assert worst <= SAME
            assert np.all(err[where] <= 2 * parts["unsafe"][where] / N + SAME)
            continue
        limit = np.broadcast_to(bound[name], err.shape)[where]
        print(f"{name} nfft {nfft} x {nch}: max err {np.max(err[where]):.2e}, bound {np.max(limit):.2e}")
        assert np.max(limit) <= LOOSEST, name
        assert np.all(err[where] <= limit), name


@pytest.mark.parametrize("nch", [2, 5, 17])
def test_lag_kernel_alone(est, nch):
    """osz_lag_accumulate on random spectra against NumPy (1e-12 of each plane's max), one
    segment and seven, the lower triangle untouched, and 7 segments = 3 + 4 bit for bit."""
    import torch
    from openseize_amd import _device as dev
    nfreq = 101
    rng = np.random.default_rng(nch)
    upper = np.triu(np.ones((nch, nch), bool))
    for nseg in (1, 7):
        X = rng.standard_normal((nseg, nch, nfreq)) + 1j * rng.standard_normal((nseg, nch, nfreq))
        d = (np.conj(X)[:, :, None] * X[:, None]).imag
        want = np.stack([d.sum(0), np.abs(d).sum(0), (d * d).sum(0), np.sign(d).sum(0)])
        want[:, ~upper] = -7.0                                       # (what the tensor held before)
        lag = torch.zeros((4, nch, nch, nfreq), dtype=torch.float64, device="cuda")
        lag[:, cuda(~upper)] = -7.0
        start = lag.clone()
        dev.lag_accumulate(cuda(X), lag)
        for p in range(4):
            assert np.max(np.abs(host(lag[p]) - want[p])) <= SAME * np.max(np.abs(want[p])), (nseg, p)
        if nseg == 7:
            parts = start.clone()
            dev.lag_accumulate(cuda(X[:3]), parts)
            dev.lag_accumulate(cuda(X[3:]), parts)
            assert np.array_equal(bits(parts), bits(lag))
    # the normalisation: X / |X|, 0 -> NaN
    Z = X[0].copy()
    Z[0, 0] = 0.0
    U = host(dev.unit_phasors(cuda(Z)))
    assert np.isnan(U[0, 0].real) and np.isnan(U[0, 0].imag)
    U[0, 0] = Z[0, 0] = 1.0
    assert np.max(np.abs(U - Z / np.abs(Z))) < 1e-15


def test_cuts_of_one_stream_agree(est):
    from openseize_amd import producer
    nfft, nch, n = 1000, 5, 50000
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True)
    kw = dict(method=METHODS, resolution=resolution, overlap=0.6, detrend="linear")
    cnt, _, onhost = est.phase_connectivity(x, fs, **kw)
    cnt_r, _, resident = est.phase_connectivity(cuda(x), fs, **kw)
    cnt_p, _, chunked = est.phase_connectivity(producer(x, 1000, -1), fs, **kw)
    mask = np.random.default_rng(5).random(n) > 0.3
    cnt_m, _, masked = est.phase_connectivity(producer(x, 1000, -1, mask=mask), fs, **kw)
    cnt_k, _, kept = est.phase_connectivity(x[:, mask], fs, **kw)
    assert cnt == cnt_r == cnt_p and cnt_m == cnt_k
    # pushes of a few strides each: the sums do not depend on where the stream is cut
    small = est._CROSS_PUSH_BYTES
    est._CROSS_PUSH_BYTES = 3 * 16 * nch * (nfft // 2 + 1)
    try:
        cnt_s, _, pieces = est.phase_connectivity(x, fs, **kw)
    finally:
        est._CROSS_PUSH_BYTES = small
    _, _, again = est.phase_connectivity(x, fs, **kw)
    _, _, turned = est.phase_connectivity(np.ascontiguousarray(x.T), fs, axis=0, **kw)
    assert cnt_s == cnt
    for name in METHODS:
        # (bin 0 of plv is the phase of rounding noise: the routes need not round alike there)
        cut = slice(1, None) if name == "plv" else slice(None)
        assert np.max(np.abs(host(resident[name]) - onhost[name])[..., cut]) < SAME, name
        assert np.max(np.abs(chunked[name] - onhost[name])[..., cut]) < SAME, name
        assert np.max(np.abs(masked[name] - kept[name])[..., cut]) < SAME, name
        assert np.array_equal(bits(pieces[name]), bits(onhost[name])), name
        assert np.array_equal(bits(again[name]), bits(onhost[name])), name
        assert np.array_equal(bits(turned[name]), bits(onhost[name])), name
        # one name alone: the same bits as in the tuple
        cnt_1, _, alone = est.phase_connectivity(x, fs, **dict(kw, method=name))
        assert cnt_1 == cnt and isinstance(alone, np.ndarray)
        assert np.array_equal(bits(alone), bits(onhost[name])), name


def test_result_lives_where_the_data_lives(est):
    import torch
    from openseize_amd import producer
    nfft, nch, n = 1024, 4, 30000
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=False)
    _, _, onhost = est.phase_connectivity(x, fs, method=METHODS, resolution=resolution)
    _, _, ondev = est.phase_connectivity(cuda(x), fs, method=METHODS, resolution=resolution)
    _, _, chained = est.phase_connectivity(producer(cuda(x), 5000, -1), fs, resolution=resolution)
    assert torch.is_tensor(chained) and chained.is_cuda and chained.dtype == torch.float64
    for name in METHODS:
        assert isinstance(onhost[name], np.ndarray)
        m = ondev[name]
        assert torch.is_tensor(m) and m.is_cuda and m.dtype == torch.float64 and m.shape == onhost[name].shape
        assert np.max(np.abs(host(m) - onhost[name])[..., 1:]) < SAME
        if name == "imcoh":
            assert torch.equal(m.transpose(0, 1), -m)
        else:
            assert np.array_equal(bits(m.transpose(0, 1).contiguous()), bits(m))
    assert np.array_equal(bits(chained), bits(ondev["wpli"]))           # (wpli is the default)


def test_nonfinite_samples_stay_in_their_row_and_column(est):
    nfft, nch, n = 1000, 5, 30000
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True)
    _, _, clean = est.phase_connectivity(x, fs, method=METHODS, resolution=resolution)
    x[2, 12345] = np.nan
    others = np.ix_([0, 1, 3, 4], [0, 1, 3, 4])
    for data in (x, cuda(x)):
        _, _, got = est.phase_connectivity(data, fs, method=METHODS, resolution=resolution)
        for name in METHODS:
            m = host(got[name])
            assert np.all(np.isnan(m[2])) and np.all(np.isnan(m[:, 2])), name
            assert np.array_equal(bits(m[others]), bits(clean[name][others])), name
        for method in ("pli", METHODS):
            with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
                est.phase_connectivity(data, fs, method=method, resolution=resolution, detrend="linear")


def test_csd_and_coherence_kept_their_bits(est):
    """csd / coherence share their loop with phase_connectivity now: on one input they return
    the bits recorded from the build before that (tests/golden/g23_csd_bits.npz)."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_csd_bits.npz"))
    nfft, nch, n = 200, 5, 1300
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True, seed=23)
    cnt, _, S = est.csd(x, fs, resolution=resolution, overlap=0.6, detrend="linear", scaling="spectrum")
    _, _, C = est.coherence(cuda(x), fs, resolution=resolution)
    assert cnt == int(gold["cnt"])
    assert np.array_equal(bits(S), gold["csd"]) and np.array_equal(bits(C), gold["coherence"])
