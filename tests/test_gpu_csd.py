"""GPU tests of csd / coherence (K10) against the NumPy restatement of the definition that
tests/test_csd_host.py pins to pairwise scipy.signal.csd / coherence.

Tolerances: the spectra at the suite's RTOL = 1e-9 of max|S| (tests/test_gpu_parity.py).  The
coherence is a ratio, so its error is the spectrum's error over the auto-spectra: it is compared
where both S_ii and S_jj reach FLOOR = 1e-3 of max|S|, at 4 RTOL / FLOOR = 4e-6 absolute (first
order error of |S_ij|^2 / (S_ii S_jj) for a coherence <= 1), and at most 0.5 % of the entries
may fall outside that condition.  Two routes to one estimate agree to 1e-12."""

from functools import partial

import numpy as np
import pytest

from test_csd_host import CASES, FLOOR, coherence_of, rate, signal, welch_cross

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SAME = 1e-12
IDS = [f"nfft{c[0]}-{c[1]}-{c[3]}-{c[4]}" for c in CASES]


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(np.max(np.abs(b))), 1e-300)
    return float(np.max(np.abs(a - b))) / scale


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


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_csd_is_scipy(est, case):
    nfft, window, overlap, detrend, scaling, nch, n = case
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True)
    nseg, freqs, want = welch_cross(x, fs, nfft, window, overlap, detrend, scaling)
    cnt, f, S = est.csd(x, fs, resolution=resolution, window=window, overlap=overlap, detrend=detrend,
                        scaling=scaling)
    err = rel_err(S, want)
    print(f"csd nfft {nfft}: {cnt} segments, rel err {err:.2e}")
    assert cnt == nseg and np.array_equal(f, freqs)
    assert isinstance(S, np.ndarray) and S.dtype == np.complex128 and S.shape == (nch, nch, nfft // 2 + 1)
    assert err < RTOL


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_coherence_is_scipy(est, case):
    nfft, window, overlap, detrend, _, nch, n = case
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=False)
    nseg, freqs, S = welch_cross(x, fs, nfft, window, overlap, detrend, "density")
    assert nseg >= 9
    want, ok = coherence_of(S)
    cnt, f, C = est.coherence(x, fs, resolution=resolution, window=window, overlap=overlap, detrend=detrend)
    assert cnt == nseg and np.array_equal(f, freqs)
    assert isinstance(C, np.ndarray) and C.dtype == np.float64 and C.shape == want.shape
    err = float(np.max(np.abs(C - want)[ok]))
    print(f"coherence nfft {nfft}: abs err {err:.2e} on {np.mean(ok):.4f} of the entries")
    assert np.mean(~ok) <= 0.005
    assert err < 4 * RTOL / FLOOR
    assert np.array_equal(C, C.transpose(1, 0, 2), equal_nan=True)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[2]], ids=["nfft1000", "nfft4096", "nfft999"])
def test_diagonal_is_psd_and_matrix_is_hermitian(est, case):
    nfft, window, overlap, detrend, scaling, nch, n = case
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True)
    kw = dict(resolution=resolution, window=window, overlap=overlap, detrend=detrend, scaling=scaling)
    cnt, _, S = est.csd(x, fs, **kw)
    pcnt, _, P = est.psd(x, fs, **kw)
    diag = np.einsum("iif->if", S)
    assert cnt == pcnt
    assert rel_err(diag.real, P) < SAME
    assert np.all(diag.imag == 0.0)
    assert np.array_equal(S.transpose(1, 0, 2), np.conj(S))


@pytest.mark.parametrize("nch", [2, 5, 13, 70, 256])
def test_channel_counts_and_axis(est, nch):
    """Tile edges: channel counts around the 4-channel register tile and the 16-channel block,
    101 bins (one full and one partial block of 64)."""
    nfft, n = 200, 1300
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True, seed=nch)
    nseg, _, want = welch_cross(x, fs, nfft, "hann", 0.5, "constant", "density")
    cnt, _, S = est.csd(x, fs, resolution=resolution)
    assert cnt == nseg and rel_err(S, want) < RTOL
    assert np.array_equal(S.transpose(1, 0, 2), np.conj(S))
    _, _, St = est.csd(np.ascontiguousarray(x.T), fs, axis=0, resolution=resolution)
    assert np.array_equal(bits(St), bits(S))
    want_c, ok = coherence_of(want)
    _, _, C = est.coherence(x, fs, resolution=resolution)
    assert float(np.max(np.abs(C - want_c)[ok])) < 4 * RTOL / FLOOR


def test_cuts_of_one_stream_agree(est):
    from openseize_amd import producer
    nfft, nch, n = 1000, 5, 50000
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True)
    kw = dict(resolution=resolution, overlap=0.6, detrend="linear")
    cnt, _, host = est.csd(x, fs, **kw)
    cnt_r, _, resident = est.csd(cuda(x), fs, **kw)
    cnt_p, _, chunked = est.csd(producer(x, 1000, -1), fs, **kw)
    assert cnt == cnt_r == cnt_p
    assert rel_err(resident.cpu().numpy(), host) < SAME
    assert rel_err(chunked, host) < SAME
    # pushes of a few strides each: the sums do not depend on where the stream is cut
    small = est._CROSS_PUSH_BYTES
    est._CROSS_PUSH_BYTES = 3 * 16 * nch * (nfft // 2 + 1)
    try:
        cnt_s, _, pieces = est.csd(x, fs, **kw)
    finally:
        est._CROSS_PUSH_BYTES = small
    assert cnt_s == cnt and np.array_equal(bits(pieces), bits(host))
    mask = np.random.default_rng(5).random(n) > 0.3
    cnt_m, _, masked = est.csd(producer(x, 1000, -1, mask=mask), fs, **kw)
    cnt_k, _, kept = est.csd(x[:, mask], fs, **kw)
    assert cnt_m == cnt_k and rel_err(masked, kept) < SAME
    _, _, cm = est.coherence(producer(x, 1000, -1, mask=mask), fs, **kw)
    _, _, ck = est.coherence(x[:, mask], fs, **kw)
    assert float(np.max(np.abs(cm - ck))) < SAME


def test_result_lives_where_the_data_lives(est):
    import scipy.signal as sps
    import torch
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    nfft, nch, n = 1024, 4, 30000
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=False)
    for func, dtype in ((est.csd, torch.complex128), (est.coherence, torch.float64)):
        _, _, onhost = func(x, fs, resolution=resolution)
        assert isinstance(onhost, np.ndarray)
        _, _, ondev = func(cuda(x), fs, resolution=resolution)
        assert torch.is_tensor(ondev) and ondev.is_cuda and ondev.dtype == dtype
        assert ondev.shape == onhost.shape and rel_err(ondev.cpu().numpy(), onhost) < SAME
        _, _, chained = func(producer(cuda(x), 5000, -1), fs, resolution=resolution)
        assert torch.is_tensor(chained) and chained.is_cuda
    # a chain of this library's producers over host data: CUDA tensors inside, an ndarray out
    h = sps.firwin(64, 0.4)
    fir = producer(partial(nm.oaconvolve, producer(x, 5000, -1), h, -1, "same"), 5000, -1, shape=x.shape)
    cnt, _, S = est.csd(fir, fs, resolution=resolution)
    assert isinstance(S, np.ndarray)
    y = np.concatenate(list(nm.oaconvolve(producer(x, 5000, -1), h, -1, "same")), -1)
    nseg, _, want = welch_cross(y, fs, nfft, "hann", 0.5, "constant", "density")
    assert cnt == nseg and rel_err(S, want) < RTOL


def test_nonfinite_samples_follow_scipy_pair_by_pair(est):
    nfft, nch, n = 1000, 5, 30000
    fs, resolution = rate(nfft)
    x = signal(nch, n, ramp=True)
    _, _, clean = welch_cross(x, fs, nfft, "hann", 0.5, "constant", "density")
    x[2, 12345] = np.nan
    others = [0, 1, 3, 4]
    for data in (x, cuda(x)):
        _, _, S = est.csd(data, fs, resolution=resolution)
        S = S if isinstance(S, np.ndarray) else S.cpu().numpy()
        assert np.all(np.isnan(S[2].real)) and np.all(np.isnan(S[:, 2].real))
        assert rel_err(S[np.ix_(others, others)], clean[np.ix_(others, others)]) < RTOL
        _, _, C = est.coherence(data, fs, resolution=resolution)
        C = C if isinstance(C, np.ndarray) else C.cpu().numpy()
        assert np.all(np.isnan(C[2])) and np.all(np.isnan(C[:, 2]))
        assert np.all(np.isfinite(C[np.ix_(others, others)][..., 1:]))
        for func in (est.csd, est.coherence):
            with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
                func(data, fs, resolution=resolution, detrend="linear")


def test_two_calls_give_the_same_bits(est):
    nfft, nch, n = 4096, 13, 60000
    fs, resolution = rate(nfft)
    x = cuda(signal(nch, n, ramp=True))
    first = est.csd(x, fs, resolution=resolution)
    second = est.csd(x, fs, resolution=resolution)
    assert first[0] == second[0]
    assert np.array_equal(bits(first[2].cpu().numpy()), bits(second[2].cpu().numpy()))
    c1, c2 = est.coherence(x, fs, resolution=resolution)[2], est.coherence(x, fs, resolution=resolution)[2]
    assert np.array_equal(bits(c1.cpu().numpy()), bits(c2.cpu().numpy()))
