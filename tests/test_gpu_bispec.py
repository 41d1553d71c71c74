"""GPU tests of bispectrum / bicoherence (K14) against ``bispectral_sums``, the NumPy restatement
of the definition that tests/test_bispec_host.py pins.

Tolerances.  The kernel alone, on the SAME complex128 input as NumPy: Re and Im of sum T and sum
|T| within 1e-13 sum |T| of that entry, sum |X1 X2|^2 and sum |X|^2 (all terms positive) within
1e-13 of themselves -- each is nseg + O(1) roundings of terms bounded by those -- and both ratios
within 1e-12 absolute everywhere, with no floor: (sum |T|)^2 <= sum |X1 X2|^2 sum |X3|^2.  The
estimators, whose spectra come from two different FFTs: the bispectrum at the suite's RTOL = 1e-9
of max|B| (tests/test_gpu_parity.py); the bicoherences, ratios of three factors each with relative
error at most RTOL / sqrt(FLOOR), entering squared in a ratio <= 1, at 6 RTOL / FLOOR absolute
where the channel's sum |X|^2 at all three bins reaches FLOOR = 1e-3 of its maximum over the band
(the form of the coherence test), and at most 0.5 % of the in-domain entries may fall outside that
condition.  Different routes to one estimate give the same bits."""

import numpy as np
import pytest

from test_bispec_host import bispectral_sums, gather_sums, measures, segment_spectra, three_channels, tones
from test_csd_host import rate

pytestmark = pytest.mark.gpu

RTOL = 1e-9
FLOOR = 1e-3
METHODS = ("kim", "hagihira")

# (nfft, window, overlap, records, noise, first and last bin of the band): three channels each,
# coupled / uncoupled / noise only, tones at bins max(3, nfft // 14) and max(5, nfft // 9)
CASES = [
    (128, "hann", 0.0, 24, 0.5, 1, 64),
    (128, "hann", 0.5, 24, 0.5, 1, 64),
    (250, "hamming", 0.5, 20, 1.0, 1, 125),
    (1000, "hann", 0.5, 12, 1.0, 20, 319),
    (999, "hann", 0.25, 12, 1.0, 1, 199),
    (4096, "hann", 0.5, 9, 4.0, 100, 611),
]
IDS = [f"nfft{c[0]}-{c[1]}-{c[2]}" for c in CASES]


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
    return torch.from_numpy(np.array(x, order="C")).cuda()           # (a copy: the shared inputs are read-only)


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(host(a))
    return a.view(np.uint64)


_WANT = {}


def expected(case):
    """(x, fs, resolution, band keywords, the restatement's sums): computed once per case, shared
    and left unchanged."""
    if case not in _WANT:
        nfft, window, overlap, nrec, noise, first, last = case
        fs, resolution = rate(nfft)
        x = three_channels(nfft, nrec, noise)
        freqs = np.fft.rfftfreq(nfft, 1 / fs)
        band = dict(fmin=None if first == 1 else freqs[first], fmax=None if last == nfft // 2 else freqs[last])
        want = bispectral_sums(x, fs, nfft, window, overlap, "constant", "density", first, last - first + 1)
        _WANT[case] = (x, fs, resolution, band, want)
    return _WANT[case]


def test_kernel_alone_is_numpy_on_the_same_spectra():
    import torch
    from openseize_amd import _device as dev
    nseg, nch, nfreq, k_lo, nb = 7, 3, 131, 3, 128           # two blocks of 64 lanes, four row tiles, a cut domain
    rng = np.random.default_rng(14)
    X = rng.standard_normal((nseg, nch, nfreq)) + 1j * rng.standard_normal((nseg, nch, nfreq))
    want = gather_sums(X, k_lo, nb)
    _, kim_w, hag_w, _ = measures(want)

    def run(cuts):
        sums = dev.zeros((4, nch, nb, nb), torch.float64)
        power = dev.zeros((nch, nfreq), torch.float64)
        at = 0
        for n in cuts:
            dev.bispec_accumulate(cuda(X[at:at + n]), k_lo, nb, sums, power)
            at += n
        return sums, power

    sums, power = run((3, 4))
    one, power_one = run((7,))
    assert np.array_equal(bits(sums), bits(one)) and np.array_equal(bits(power), bits(power_one))
    got = host(sums)
    low = np.tril(np.ones((nb, nb), dtype=bool)) & want["inside"]        # what the kernel computes: k2 <= k1
    assert low.sum() > 0 and np.all(got[:, :, ~low] == 0.0)              # the rest is not touched
    A = want["A"][:, low]
    errs = {"re": np.abs(got[0][:, low] - want["T"].real[:, low]) / A,
            "im": np.abs(got[1][:, low] - want["T"].imag[:, low]) / A,
            "p12": np.abs(got[2][:, low] - want["P12"][:, low]) / want["P12"][:, low],
            "abs": np.abs(got[3][:, low] - A) / A,
            "power": np.abs(host(power) - want["power"]) / want["power"]}
    print({k: float(v.max()) for k, v in errs.items()})
    for name, err in errs.items():
        assert err.max() < 1e-13, name
    inside = want["inside"]
    for mode, ratio in (("kim", kim_w), ("hagihira", hag_w)):
        M = host(dev.bispec_finish(mode, nseg, k_lo, sums, power))
        assert M.shape == (nch, nb, nb) and M.dtype == np.float64
        assert np.array_equal(np.isnan(M), np.broadcast_to(~inside, M.shape))
        err = float(np.max(np.abs(M - ratio)[:, inside]))
        print(mode, err)
        assert err < 1e-12
        assert np.array_equal(M, M.transpose(0, 2, 1), equal_nan=True)
    B = host(dev.bispec_finish("spectrum", nseg, k_lo, sums, power))
    assert B.dtype == np.complex128 and np.array_equal(np.isnan(B), np.broadcast_to(~inside, B.shape))
    assert np.max(np.abs(B - want["T"] / nseg)[:, inside] / (want["A"][:, inside] / nseg)) < 1e-13


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bispectrum_is_the_restatement(est, case):
    nfft, window, overlap = case[:3]
    x, fs, resolution, band, want = expected(case)
    B_want = measures(want)[0]
    inside = want["inside"]
    cnt, freqs, B = est.bispectrum(x, fs, resolution=resolution, window=window, overlap=overlap, **band)
    assert cnt == want["cnt"] and np.array_equal(freqs, want["freqs"])
    assert isinstance(B, np.ndarray) and B.dtype == np.complex128 and B.shape == (3, want["nb"], want["nb"])
    assert np.array_equal(np.isnan(B), np.broadcast_to(~inside, B.shape))
    assert np.array_equal(np.isnan(B.real), np.isnan(B.imag))
    err = float(np.max(np.abs(B - B_want)[:, inside]) / np.max(np.abs(B_want[:, inside])))
    print(f"bispectrum nfft {nfft}: {cnt} segments, {want['nb']} bins, rel err {err:.2e}")
    assert err < RTOL
    assert np.array_equal(bits(B), bits(B.transpose(0, 2, 1)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bicoherence_is_the_restatement(est, case):
    nfft, window, overlap = case[:3]
    x, fs, resolution, band, want = expected(case)
    _, kim, hag, P3 = measures(want)
    inside = want["inside"]
    k = want["k_lo"] + np.arange(want["nb"])
    p = want["power"][:, k]
    floor = FLOOR * p.max(axis=1)[:, None, None]
    ok = inside & (p[:, :, None] >= floor) & (p[:, None, :] >= floor) & (np.nan_to_num(P3) >= floor)
    left_out = 1 - ok.sum() / (3 * inside.sum())
    cnt, freqs, M = est.bicoherence(x, fs, method=METHODS, resolution=resolution, window=window, overlap=overlap,
                                    **band)
    assert cnt == want["cnt"] and np.array_equal(freqs, want["freqs"]) and tuple(M) == METHODS
    for name, ratio in (("kim", kim), ("hagihira", hag)):
        got = M[name]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ratio.shape
        assert np.array_equal(np.isnan(got), np.broadcast_to(~inside, got.shape))
        err = float(np.max(np.abs(got - ratio)[ok]))
        print(f"{name} nfft {nfft}: abs err {err:.2e}, {left_out:.4%} of the domain left out")
        assert left_out <= 0.005
        assert err < 6 * RTOL / FLOOR
        assert np.all(got[:, inside] >= 0) and np.all(got[:, inside] <= 1 + 1e-9)


def test_quadratic_phase_coupling_through_the_device(est):
    case = CASES[0]
    nfft, window, overlap = case[:3]
    x, fs, resolution, band, want = expected(case)
    k1, k2 = tones(nfft)
    assert (k1, k2) == (9, 14)
    a, b = k2 - want["k_lo"], k1 - want["k_lo"]
    kim = measures(want)[1]
    assert kim[0, a, b] > 0.9 and kim[1, a, b] < 0.3
    _, _, got = est.bicoherence(x, fs, method="kim", resolution=resolution, window=window, overlap=overlap, **band)
    print("kim at the tones: coupled", float(got[0, a, b]), "uncoupled", float(got[1, a, b]),
          "noise", float(got[2, a, b]))
    assert got[0, a, b] > 0.9 and got[0, b, a] > 0.9
    assert got[1, a, b] < 0.3


@pytest.mark.parametrize("nch", [1, 2, 5, 17])
def test_tile_edges(est, nch):
    """Bands around the 64-lane block and the 8-row / 32-row tiles, from two first bins; one
    channel is one-dimensional data."""
    nfft, n = 300, 1500
    fs, resolution = rate(nfft)
    freqs = np.fft.rfftfreq(nfft, 1 / fs)
    x = np.random.default_rng(nch).standard_normal((nch, n)) + 1.0
    X = segment_spectra(x, fs, nfft, "hann", 0.5, "constant", "density")
    data = x[0] if nch == 1 else x
    shape = (lambda nb: (nb, nb)) if nch == 1 else (lambda nb: (nch, nb, nb))
    for first in (1, 7):
        for nb in (1, 2, 63, 64, 65, 130):
            want = gather_sums(X, first, nb)
            B_want = measures(want)[0]
            inside = want["inside"]
            cnt, f, B = est.bispectrum(data, fs, resolution=resolution, fmin=freqs[first], fmax=freqs[first + nb - 1])
            assert cnt == X.shape[0] and np.array_equal(f, freqs[first:first + nb]) and B.shape == shape(nb)
            B3 = B.reshape(nch, nb, nb)
            assert np.array_equal(np.isnan(B3), np.broadcast_to(~inside, B3.shape)), (first, nb)
            err = float(np.max(np.abs(B3 - B_want)[:, inside]) / np.max(np.abs(B_want[:, inside])))
            assert err < RTOL, (first, nb, err)
            assert np.array_equal(bits(B3), bits(B3.transpose(0, 2, 1)))
    if nch > 1:
        _, _, Bt = est.bispectrum(np.ascontiguousarray(x.T), fs, axis=0, resolution=resolution, fmin=freqs[7],
                                  fmax=freqs[136])
        assert np.array_equal(bits(Bt), bits(B))
    # fmin = 0 includes DC and shifts the band by one bin
    _, f1, B1 = est.bispectrum(data, fs, resolution=resolution, fmax=freqs[70])
    _, f0, B0 = est.bispectrum(data, fs, resolution=resolution, fmin=0, fmax=freqs[70])
    assert f0[0] == 0.0 and np.array_equal(f0[1:], f1) and B0.shape[-1] == B1.shape[-1] + 1
    assert np.array_equal(bits(B0[..., 1:, 1:]), bits(B1))
    assert np.all(np.isfinite(B0[..., 0, :].real))


def test_same_bits_by_every_route(est, monkeypatch):
    from openseize_amd import _device as dev
    from openseize_amd import producer
    case = CASES[3]
    nfft, window, overlap = case[:3]
    x, fs, resolution, band, want = expected(case)
    kw = dict(resolution=resolution, window=window, overlap=overlap, **band)
    seen = []
    plain = dev.bispec_finish
    monkeypatch.setattr(dev, "bispec_finish", lambda mode, count, k_lo, sums, power:
                        (seen.append(sums), plain(mode, count, k_lo, sums, power))[1])
    cnt, _, B = est.bispectrum(x, fs, **kw)
    denominator = host(seen[0][3])                            # sum |T| as the device holds it (k2 <= k1)
    cnt_r, _, resident = est.bispectrum(cuda(x), fs, **kw)
    import torch
    assert torch.is_tensor(resident) and resident.is_cuda and resident.dtype == torch.complex128
    assert cnt_r == cnt and np.array_equal(bits(resident), bits(B))
    for chunksize in (700, 1000, 4321):                       # (nfft is 1000)
        cnt_p, _, chunked = est.bispectrum(producer(x, chunksize, -1), fs, **kw)
        assert cnt_p == cnt and isinstance(chunked, np.ndarray) and np.array_equal(bits(chunked), bits(B)), chunksize
    # pushes of two strides each: a chunk takes several pushes
    monkeypatch.setattr(est, "_CROSS_PUSH_BYTES", 2 * 24 * 3 * (nfft // 2 + 1))
    cnt_s, _, pieces = est.bispectrum(x, fs, **kw)
    assert cnt_s == cnt and np.array_equal(bits(pieces), bits(B))
    monkeypatch.undo()
    _, _, again = est.bispectrum(x, fs, **kw)
    assert np.array_equal(bits(again), bits(B))
    assert np.array_equal(bits(B), bits(B.transpose(0, 2, 1)))
    # a tuple of methods against the single names; on the device too
    _, _, both = est.bicoherence(x, fs, method=("hagihira", "kim"), **kw)
    assert tuple(both) == ("hagihira", "kim")
    for name in METHODS:
        _, _, single = est.bicoherence(x, fs, method=name, **kw)
        assert np.array_equal(bits(single), bits(both[name])), name
        assert np.array_equal(single, single.transpose(0, 2, 1), equal_nan=True)
        _, _, ondev = est.bicoherence(cuda(x), fs, method=name, **kw)
        assert torch.is_tensor(ondev) and ondev.dtype == torch.float64 and np.array_equal(bits(ondev), bits(single))
    # hagihira times its denominator is |bispectrum| times the count
    low = np.tril(np.ones(B.shape[-2:], dtype=bool)) & want["inside"]
    lhs = both["hagihira"][:, low] * denominator[:, low]
    rhs = np.abs(B[:, low]) * cnt
    assert np.max(np.abs(lhs - rhs) / rhs) < 1e-12


def test_nonfinite_samples_stay_in_their_channel(est):
    case = CASES[2]
    nfft, window, overlap = case[:3]
    x, fs, resolution, band, want = expected(case)
    inside = want["inside"]
    kw = dict(resolution=resolution, window=window, overlap=overlap, **band)
    _, _, clean = est.bispectrum(x, fs, **kw)
    _, _, clean_k = est.bicoherence(x, fs, method="kim", **kw)
    bad = np.array(x)
    bad[1, 1234] = np.nan
    for data in (bad, cuda(bad)):
        _, _, B = est.bispectrum(data, fs, **kw)
        B = host(B)
        assert np.all(np.isnan(B[1][inside]))
        assert np.array_equal(bits(B[[0, 2]]), bits(clean[[0, 2]]))
        _, _, K = est.bicoherence(data, fs, method="kim", **kw)
        K = host(K)
        assert np.all(np.isnan(K[1][inside])) and np.array_equal(bits(K[[0, 2]]), bits(clean_k[[0, 2]]))
        for func in (est.bispectrum, est.bicoherence):
            with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
                func(data, fs, detrend="linear", **kw)


def test_sums_that_do_not_fit_the_device_are_refused_before_the_stream(est, monkeypatch):
    import torch
    from test_csd_host import Untouched
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (1 << 20, 1 << 30))
    for func in (est.bispectrum, est.bicoherence):
        src = Untouched((4, 5000))
        with pytest.raises(MemoryError, match="32 B per channel.*fmax.*fewer channels"):
            func(src.pro, fs=100)                              # 4 x 100 x 100 pairs x 40 B and more > 1 MiB
        assert not src.started
        cnt, _, M = func(src.pro, fs=100, fmax=10.0)           # 20 bins: fits (the source is all zeros)
        assert cnt == 49 and M.shape == (4, 20, 20)           # (5000 - 200) // 100 + 1 segments
