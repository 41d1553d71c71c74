"""ModulationIndex on the device: the three entry points of csrc/pac.hip against the NumPy
restatement of test_pac_host.py (the accumulate kernel on edge geometries, with bins given as
bytes so that no phase rounding is involved), and estimate() end to end against the
restatement fed with the library's own analytic phases and amplitudes."""

import functools

import numpy as np
import pytest
from scipy import stats
from scipy.stats import false_discovery_control as fdr

from test_pac_host import (AMP_BW, AMP_CENTERS, FS, PHASE_BW, PHASE_CENTERS, check_coupling,
                           drifting_signal, estimator, pac_bins, pac_mi, pac_shifts, pac_sums)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ osz_pac_accumulate alone
def _run_accumulate(bins_chunks, amp_chunks, shifts, nbins):
    import torch
    from openseize_amd import _device as dev
    P, A = bins_chunks[0].shape[0], amp_chunks[0].shape[0]
    sums = dev.zeros((P, A, len(shifts) + 1, nbins), torch.float64)
    counts = dev.zeros((P, nbins), torch.int64)
    dshifts = torch.from_numpy(np.asarray(shifts, dtype=np.int64)).cuda()
    for bins, amp in zip(bins_chunks, amp_chunks):
        dev.pac_accumulate(torch.from_numpy(bins).cuda(), torch.from_numpy(amp).cuda(), dshifts,
                           nbins, sums, counts)
    return sums.cpu().numpy(), counts.cpu().numpy()


def _geometry(rng, lengths, P, A, S, nbins, shifts=None, codes=None, none=0.0):
    """Random bins (drawn from ``codes``, a share ``none`` of them the no-bin code 255) and
    amplitudes in [0.1, 1.1) per chunk; S shifts below the longest chunk unless given."""
    codes = np.arange(nbins) if codes is None else np.asarray(codes)
    bins, amps = [], []
    for L in lengths:
        b = codes[rng.integers(0, codes.size, (P, L))].astype(np.uint8)
        b[rng.random((P, L)) < none] = 255
        bins.append(b)
        amps.append(rng.random((A, L)) + 0.1)
    if shifts is None:
        shifts = rng.integers(0, max(lengths), S)
    return bins, amps, [int(s) for s in shifts], nbins


# the accumulate kernel steps through a run 256 samples at a time (4 per lane) and takes
# 128-thread workgroups above 32 bins; the count kernel takes tiles of 16384 samples on at
# most 1024 workgroups
GEOMETRIES = {
    "a_random": lambda r: _geometry(r, [20000, 20000, 7000], 3, 5, 20, 18),
    "b_L1": lambda r: _geometry(r, [1], 2, 2, 3, 18, shifts=[0, 1, 5]),
    "b_L63": lambda r: _geometry(r, [63], 2, 2, 3, 18),
    "b_L64": lambda r: _geometry(r, [64], 2, 2, 3, 18),
    "b_L65": lambda r: _geometry(r, [65, 64, 1], 2, 2, 3, 18),
    "c_step_plus_one": lambda r: _geometry(r, [257], 2, 2, 4, 18, shifts=[0, 1, 128, 256]),
    "c_count_tile_plus_one": lambda r: _geometry(r, [16385], 2, 1, 2, 18),
    "c_count_grid_plus_one": lambda r: _geometry(r, [1024 * 16384 + 1], 1, 1, 1, 64),
    "d_S0": lambda r: _geometry(r, [1500], 2, 2, 0, 18),
    "d_S1": lambda r: _geometry(r, [1500], 2, 2, 1, 18),
    "d_S2000": lambda r: _geometry(r, [1500], 1, 2, 2000, 18),
    "e_shift_edges": lambda r: _geometry(r, [1000], 2, 2, 5, 18, shifts=[0, 1, 999, 1000, 1003]),
    "e_short_last_chunk": lambda r: _geometry(r, [1000, 300], 2, 2, 5, 18,
                                              shifts=[0, 1, 999, 1000, 1003]),
    "f_nbins2": lambda r: _geometry(r, [5000, 777], 2, 2, 6, 2),
    "f_nbins32": lambda r: _geometry(r, [5000, 777], 2, 2, 6, 32),
    "f_nbins33": lambda r: _geometry(r, [5000, 777], 2, 2, 6, 33),
    "f_nbins64": lambda r: _geometry(r, [5000, 777], 2, 3, 6, 64),
    "g_empty_bin_and_no_bin": lambda r: _geometry(r, [6000, 900], 2, 2, 5, 18,
                                                  codes=[0, 1, 2, 3, 4, 6, 9, 17], none=0.1),
    "h_single": lambda r: _geometry(r, [3000, 100], 1, 1, 4, 18),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_pac_accumulate_matches_restatement(name):
    rng = np.random.default_rng(sorted(GEOMETRIES).index(name) + 311)
    bins, amps, shifts, nbins = GEOMETRIES[name](rng)
    got_s, got_c = _run_accumulate(bins, amps, shifts, nbins)
    want_s, want_c = pac_sums(bins, amps, shifts, nbins)
    np.testing.assert_array_equal(got_c, want_c)
    if name.startswith("g_"):
        assert (want_c[:, 5] == 0).all() and sum(b.size for b in bins) > want_c.sum()
    scale = want_s.max(axis=-1, keepdims=True)                  # of the row of nbins sums
    err = np.abs(got_s - want_s) / np.maximum(scale, 1e-300)
    print(f"{name}: largest error {err.max():.2e} of the row scale")
    assert np.all(err <= 1e-12)
    again_s, again_c = _run_accumulate(bins, amps, shifts, nbins)
    assert again_s.tobytes() == got_s.tobytes() and again_c.tobytes() == got_c.tobytes()


def test_pac_accumulate_nan_amplitude():
    """One NaN in an amplitude row reaches exactly the (a, s, b) sums it is added to."""
    rng = np.random.default_rng(5)
    bins, amps, shifts, nbins = _geometry(rng, [4000, 1000], 2, 3, 12, 18)
    amps[0][1, 1234] = np.nan
    got, _ = _run_accumulate(bins, amps, shifts, nbins)
    want, _ = pac_sums(bins, amps, shifts, nbins)
    bad = np.isnan(want)
    assert bad[:, 1].sum() == 2 * 13 and not bad[:, [0, 2]].any()
    np.testing.assert_array_equal(np.isnan(got), bad)
    np.testing.assert_allclose(got[~bad], want[~bad], rtol=1e-12, atol=0)


def test_pac_accumulate_empty_chunk_and_bad_arguments():
    import torch
    from openseize_amd import _device as dev
    sums = dev.zeros((1, 1, 2, 18), torch.float64)
    counts = dev.zeros((1, 18), torch.int64)
    shifts = torch.tensor([3], dtype=torch.int64, device="cuda")
    dev.pac_accumulate(torch.empty((1, 0), dtype=torch.uint8, device="cuda"),
                       torch.empty((1, 0), dtype=torch.float64, device="cuda"), shifts, 18, sums,
                       counts)
    assert not sums.cpu().numpy().any() and not counts.cpu().numpy().any()
    bins = torch.zeros((1, 10), dtype=torch.uint8, device="cuda")
    amp = torch.ones((1, 10), dtype=torch.float64, device="cuda")
    for nbins in (1, 65):
        with pytest.raises(ValueError, match="nbins"):
            dev.pac_accumulate(bins, amp, shifts, nbins, dev.zeros((1, 1, 2, nbins), torch.float64),
                               dev.zeros((1, nbins), torch.int64))
    with pytest.raises(ValueError):
        dev.pac_accumulate(bins, amp[:, :9], shifts, 18, sums, counts)


# ------------------------------------------------------------ osz_phase_bins
def _complex_samples(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.mark.parametrize("nbins", [2, 18, 64])
def test_phase_bins_are_the_bins_of_magphase(nbins):
    import torch
    from openseize_amd import _device as dev
    z = _complex_samples(3 * 10007, 1).reshape(3, 10007)
    z[0, :6] = [0, -1, complex(-1, -0.0), 1, complex(np.nan, 1), complex(1, -1e-300)]
    zd = torch.from_numpy(z).cuda()
    got = dev.phase_bins(zd, nbins).cpu().numpy()
    phases = dev.magphase(zd, want_mag=False)[1].cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == z.shape
    np.testing.assert_array_equal(got, pac_bins(phases, nbins))
    assert got[0, 4] == 255 and got[0, 0] == 0 and (got[got != 255] < nbins).all()
    assert set(np.unique(got[1])) == set(range(nbins))


def test_phase_bins_against_numpy_angle():
    """Against numpy.angle on 1e5 samples: a device phase may differ from NumPy's in the last
    bits, so a sample within 1e-9 rad of a bin edge may fall either way; 6e-4 such samples
    are expected among 1e5 for 18 edges."""
    import torch
    from openseize_amd import _device as dev
    nbins = 18
    z = _complex_samples(100000, 2)
    got = dev.phase_bins(torch.from_numpy(z).cuda().reshape(1, -1), nbins).cpu().numpy()[0]
    phases = np.mod(np.angle(z), 2 * np.pi)
    miss = np.flatnonzero(got != pac_bins(phases, nbins))
    print(f"{miss.size} of {z.size} samples in another bin than numpy.angle's")
    assert miss.size <= 5
    edge = np.abs(phases[miss] - np.round(phases[miss] * nbins / (2 * np.pi)) * 2 * np.pi / nbins)
    assert np.all(edge < 1e-9), edge


# ------------------------------------------------------------ osz_pac_finish
def test_pac_finish_matches_restatement():
    import torch
    from openseize_amd import _device as dev
    rng = np.random.default_rng(9)
    sums = rng.random((4, 3, 6, 18)) * 1e4
    sums[1, 2, 3, [0, 7]] = 0.0                  # P_b = 0: 0 ln 0 = 0
    sums[3, 1, :, :17] = 0.0                     # all mass in one bin: 1
    counts = rng.integers(1, 5000, (4, 18))
    counts[2, 11] = 0                            # an empty bin: the row is NaN
    mi, dist = (t.cpu().numpy() for t in dev.pac_finish(torch.from_numpy(sums).cuda(),
                                                        torch.from_numpy(counts).cuda()))
    want_mi, want_dist = pac_mi(sums, counts)
    assert mi.shape == (4, 3, 6) and dist.shape == (4, 3, 18)
    assert np.isnan(mi[2]).all() and np.isnan(dist[2]).all()
    keep = [0, 1, 3]
    assert np.isfinite(mi[keep]).all() and np.isfinite(dist[keep]).all()
    np.testing.assert_allclose(mi[keep], want_mi[keep], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dist[keep], want_dist[keep], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mi[3, 1], 1.0, rtol=0, atol=1e-12)
    assert (mi[keep] >= -1e-12).all() and (mi[keep] <= 1 + 1e-12).all()


# ------------------------------------------------------------ estimate() end to end
SEED, SURROGATES = 2101, 50
ESTIMATE = dict(phase_centers=PHASE_CENTERS, amp_centers=AMP_CENTERS, phase_bandwidth=PHASE_BW,
                amp_bandwidth=AMP_BW, surrogates=SURROGATES, verbose=False)


def _library_band(x, center, bw, cs):
    """(phase chunks, amplitude chunks) of one band from the library's own filters."""
    from openseize_amd import producer
    from openseize_amd.experimental.coupling.transforms import Analytic
    from openseize_amd.filtering import fir
    fpass = center + np.array([-bw / 2, bw / 2])
    fstop = fpass + np.array([-bw / 2, bw / 2])
    filt = fir.Kaiser(fpass, fstop, FS)
    an = Analytic(filt(producer(x, cs, -1), chunksize=cs, axis=-1), FS, cs, -1, width=4)
    return [np.asarray(a) for a in an.phases], [np.asarray(a) for a in an.amplitudes]


@functools.lru_cache(maxsize=None)
def _expected(cs):
    """The restatement on the library's phases and amplitudes, with estimate()'s shifts:
    (mi of all sets (P, A, S + 1), dist, adjusted p-values)."""
    x = drifting_signal(SEED)
    ph = [_library_band(x, c, bw, cs)[0] for c, bw in zip(PHASE_CENTERS, PHASE_BW)]
    am = [_library_band(x, c, AMP_BW, cs)[1] for c in AMP_CENTERS]
    nchunks = len(ph[0])
    bins = [pac_bins(np.stack([rows[k] for rows in ph]), 18) for k in range(nchunks)]
    amps = [np.stack([rows[k] for rows in am]) for k in range(nchunks)]
    shifts, _ = pac_shifts(0, FS, min(cs, x.size), SURROGATES)
    mi, dist = pac_mi(*pac_sums(bins, amps, shifts, 18))
    sur = mi[..., 1:]
    z = (mi[..., 0] - sur.mean(axis=-1)) / sur.std(axis=-1, ddof=1)
    p = fdr(stats.norm.sf(z).ravel()).reshape(z.shape)
    return mi, dist, p


@functools.lru_cache(maxsize=None)
def _estimated(cs, kind):
    """estimate() on the drifting signal as ndarray or CUDA tensor: ((mi, p, dist), the
    (P, A, S + 1) indices osz_pac_finish returned on the way, rng's next draw)."""
    import torch
    from openseize_amd import _device as dev
    x = drifting_signal(SEED)
    x = torch.from_numpy(x).cuda() if kind == "cuda" else x
    est = estimator(chunksize=cs)
    seen, plain = [], dev.pac_finish
    dev.pac_finish = lambda *a: (seen.append(plain(*a)), seen[-1])[1]
    try:
        out = est.estimate(x, **ESTIMATE)
    finally:
        dev.pac_finish = plain
    assert len(seen) == 1
    return out, seen[0][0].cpu().numpy(), est.rng.integers(0, 2**62)


@pytest.mark.parametrize("kind", ["ndarray", "cuda"])
@pytest.mark.parametrize("cs", [7000, 40000])
def test_estimate_matches_restatement(cs, kind):
    (mi, p, dist), mi_all, _ = _estimated(cs, kind)
    want_all, want_dist, want_p = _expected(cs)
    assert all(isinstance(v, np.ndarray) for v in (mi, p, dist))
    assert mi.shape == (3, 3) and p.shape == (3, 3) and dist.shape == (3, 3, 18)
    assert mi.dtype == np.float64 and p.dtype == np.float64
    np.testing.assert_array_equal(mi, mi_all[..., 0])
    np.testing.assert_allclose(mi_all, want_all, rtol=0, atol=1e-10)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-10, atol=0)
    np.testing.assert_allclose(p, want_p, rtol=0, atol=1e-7)
    np.testing.assert_allclose(dist.sum(axis=-1), 1.0, rtol=0, atol=1e-12)
    # the library's band filters, not SciPy's: the facts of test_pac_host.py hold for them too
    check_coupling(mi_all)
    assert p[1, 1] < 1e-6


@pytest.mark.parametrize("cs", [7000, 40000])
def test_estimate_host_and_device_input_agree(cs):
    (mi_h, p_h, dist_h), all_h, _ = _estimated(cs, "ndarray")
    (mi_d, p_d, dist_d), all_d, _ = _estimated(cs, "cuda")
    for name, d, h in (("mi", mi_d, mi_h), ("mi of all sets", all_d, all_h), ("dist", dist_d, dist_h)):
        print(f"cs {cs}: {name} of CUDA against host input: largest relative difference "
              f"{np.max(np.abs(d - h) / np.abs(h)):.2e}")
    np.testing.assert_allclose(mi_d, mi_h, rtol=1e-12, atol=0)
    np.testing.assert_allclose(all_d, all_h, rtol=1e-12, atol=0)
    np.testing.assert_allclose(dist_d, dist_h, rtol=1e-12, atol=0)
    np.testing.assert_allclose(p_d, p_h, rtol=0, atol=1e-9)


def test_estimate_rerun_gives_the_same_bytes_and_draws():
    cs = 7000
    x = drifting_signal(SEED)
    (mi, p, dist), _, after = _estimated(cs, "ndarray")
    est = estimator(chunksize=cs)
    for _ in range(2):
        est.rng = np.random.default_rng(0)
        again = est.estimate(x, **ESTIMATE)
        for got, first in zip(again, (mi, p, dist)):
            assert got.tobytes() == first.tobytes()
    # rng advanced by exactly SURROGATES draws of integers(min_shift, max_shift - min_shift)
    _, fresh = pac_shifts(0, FS, cs, SURROGATES)
    assert after == fresh.integers(0, 2**62)
    assert est.rng.integers(0, 2**62) == after


def test_estimate_without_surrogates():
    cs = 7000
    est = estimator(chunksize=cs, seed=3)
    mi, p, dist = est.estimate(drifting_signal(SEED), [8], [60], phase_bandwidth=4, surrogates=None,
                               verbose=False)
    assert p.dtype == object and p.shape == (1, 1) and p[0, 0] is None
    assert est.rng.integers(0, 2**62) == np.random.default_rng(3).integers(0, 2**62)
    (want, _, want_dist), _, _ = _estimated(cs, "ndarray")
    np.testing.assert_allclose(mi[0, 0], want[1, 1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(dist[0, 0], want_dist[1, 1], rtol=1e-12, atol=0)


def test_amplitude_signal():
    cs = 7000
    x = drifting_signal(SEED)
    args = dict(phase_centers=[8], amp_centers=[60], phase_bandwidth=4, surrogates=SURROGATES,
                verbose=False)
    alone = estimator(chunksize=cs).estimate(x, **args)
    same = estimator(chunksize=cs).estimate(x, amplitude_signal=x.copy(), **args)
    for a, b in zip(alone, same):
        assert a.tobytes() == b.tobytes()
    assert alone[1][0, 0] < 1e-6
    # amplitudes of an unrelated noise: one cell, so the adjusted p-value is the unadjusted one
    noise = np.random.default_rng(11).standard_normal(x.size)
    mi, p, _ = estimator(chunksize=cs).estimate(x, amplitude_signal=noise, **args)
    print(f"independent amplitudes: mi = {mi[0, 0]:.3g}, p = {p[0, 0]:.3g}")
    assert p[0, 0] > 0.01


def test_empty_bin_names_the_phase_centre():
    """A flat channel has one phase (that of 0 + 0j) at every sample and leaves 17 of the 18 bins
    empty.  A signal of fewer samples than bins cannot be used for this: it is shorter than the
    561 taps of the 8 Hz band filter, which refuses it in words of its own before any bin is
    counted."""
    est = estimator(chunksize=7000)
    x = np.zeros(9000)
    with pytest.raises(ValueError, match="at 8 Hz"):
        est.estimate(x, [8], [60], phase_bandwidth=4, surrogates=None, verbose=False)


# ------------------------------------------------------------ the wrappers' own checks
def test_pac_accumulate_refuses_shifts_that_are_not_int64_on_the_device():
    import torch
    from openseize_amd import _device as dev
    bins = torch.zeros((1, 100), dtype=torch.uint8, device="cuda")
    amp = torch.ones((1, 100), dtype=torch.float64, device="cuda")
    sums = dev.zeros((1, 1, 3, 18), torch.float64)
    counts = dev.zeros((1, 18), torch.int64)
    good = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device="cuda")
    for bad in (good[:2].int(), good[:2].cpu(), good[::2], good[:2].reshape(1, 2)):
        with pytest.raises(ValueError, match="shifts"):
            dev.pac_accumulate(bins, amp, bad, 18, sums, counts)
    assert not sums.any() and not counts.any()
    dev.pac_accumulate(bins, amp, good[:2], 18, sums, counts)
    assert counts[0, 0] == 100 and sums[0, 0, :, 0].tolist() == [100.0, 100.0, 100.0]


def test_magphase_mag_out():
    """The amplitudes land in the given rows and are the ones of a call without ``mag_out``;
    rows of another shape, type, layout or device are refused."""
    import torch
    from openseize_amd import _device as dev
    gen = torch.Generator(device="cuda").manual_seed(3)
    z = torch.randn((2, 300), dtype=torch.complex128, device="cuda", generator=gen)
    want, _ = dev.magphase(z, want_phase=False)
    block = torch.zeros((3, 300), dtype=torch.float64, device="cuda")
    got, ph = dev.magphase(z, want_phase=False, mag_out=block[1:3])
    assert ph is None and got.data_ptr() == block[1].data_ptr()
    assert torch.equal(block[1:3], want) and not block[0].any()
    for bad in (block[:1], block[:2].float(), torch.zeros((2, 600), dtype=torch.float64,
                                                          device="cuda")[:, ::2],
                torch.zeros((2, 300), dtype=torch.float64)):
        with pytest.raises(ValueError, match="mag_out"):
            dev.magphase(z, want_phase=False, mag_out=bad)
