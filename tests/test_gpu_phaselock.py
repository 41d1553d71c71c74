"""PhaseLock on the device: index() against the reference's indices, estimate() against
the reference's powers, p-values and rng state (tests/golden/g21_phaselock.npz), and the
osz_lock_accumulate kernel against the NumPy restatement of test_phaselock_host.py on
edge geometries."""

import numpy as np
import pytest

from test_phaselock_host import CASES, CENTERS, lock_sums, signal, split

pytestmark = pytest.mark.gpu

SECONDS = 30


def estimator(case, seed=0):
    from openseize_amd.experimental.coupling.estimators import PhaseLock
    from openseize_amd.filtering.special import Hilbert
    fs, cs, _ = CASES[case]
    return PhaseLock(Hilbert(width=4, fs=fs), chunksize=cs, seed=seed)


def case_signal(case):
    fs, _, seed = CASES[case]
    return signal(fs, SECONDS, seed)


@pytest.mark.parametrize("case", sorted(CASES))
def test_index_matches_reference(golden, case):
    g = golden("g21_phaselock.npz")
    est = estimator(case)
    est.index(case_signal(case), fpass=[6, 10], fstop=[4, 12])
    assert all(isinstance(a, np.ndarray) and a.dtype == np.int64 for a in est.indices)
    ref = split(g[f"{case}idx"], g[f"{case}idx_len"])
    fs, cs, _ = CASES[case]
    assert len(est.indices) == len(ref)
    glob = [np.concatenate([a + k * cs for k, a in enumerate(lists)])
            for lists in (est.indices, ref)]
    diff = np.setxor1d(*glob)
    if case != "b_":      # the fixture's phases (a_ signal) mark the samples on a bound
        ph = g["a_phases"][diff]
        assert np.all(np.abs(ph - 0.05) < 1e-9), ph
    else:
        assert diff.size == 0, diff
    # indices are ascending positions within their chunk
    for k, a in enumerate(est.indices):
        assert np.all(np.diff(a) > 0) and a.min(initial=0) >= 0
        assert a.max(initial=0) < min(cs, fs * SECONDS - k * cs)


def _fixture_estimate(g, case, ncores, surrogates=25):
    est = estimator(case)
    est.indices = split(g[f"{case}idx"], g[f"{case}idx_len"])
    pw, pv = est.estimate(case_signal(case), CENTERS, bandwidth=8, window=1,
                          surrogates=surrogates, ncores=ncores, verbose=False)
    return est, pw, pv


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("ncores", [1, 3])
def test_estimate_matches_reference(golden, case, ncores):
    g = golden("g21_phaselock.npz")
    est, pw, pv = _fixture_estimate(g, case, ncores)
    ref_pw, ref_pv = g[f"{case}pow{ncores}"], g[f"{case}pv{ncores}"]
    assert pw.shape == ref_pw.shape and pv.shape == ref_pv.shape
    np.testing.assert_allclose(pw, ref_pw, rtol=0, atol=1e-9 * np.abs(ref_pw).max())
    np.testing.assert_allclose(pv, ref_pv, rtol=0, atol=1e-7)
    assert est.rng.integers(0, 2**62) == g[f"{case}rng{ncores}"][0]


def test_estimate_without_surrogates(golden):
    g = golden("g21_phaselock.npz")
    est, pw, pv = _fixture_estimate(g, "a_", 1, surrogates=None)
    np.testing.assert_allclose(pw, g["d_pow1"], rtol=0, atol=1e-9 * np.abs(g["d_pow1"]).max())
    assert pv.dtype == object and pv.shape == (3,) and all(v is None for v in pv)
    assert est.rng.integers(0, 2**62) == g["d_rng1"][0]


def test_device_input_and_repeatability(golden):
    """A CUDA-tensor signal gives CUDA indices and the same numbers as the host signal;
    a second run gives the same bits."""
    import torch
    g = golden("g21_phaselock.npz")
    x = case_signal("a_")
    host = estimator("a_")
    host.index(x, fpass=[6, 10], fstop=[4, 12])
    devi = estimator("a_")
    devi.index(torch.from_numpy(x).cuda(), fpass=[6, 10], fstop=[4, 12])
    assert all(torch.is_tensor(a) and a.is_cuda for a in devi.indices)
    for a, b in zip(host.indices, devi.indices):
        np.testing.assert_array_equal(a, b.cpu().numpy())
    runs = []
    for est, sig in ((host, x), (devi, torch.from_numpy(x).cuda()), (host, x)):
        est.rng = np.random.default_rng(0)
        runs.append(est.estimate(sig, CENTERS, bandwidth=8, window=1, surrogates=25,
                                 ncores=1, verbose=False))
    np.testing.assert_allclose(runs[1][0], runs[0][0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(runs[1][1], runs[0][1], rtol=0, atol=1e-9)
    assert runs[2][0].tobytes() == runs[0][0].tobytes()
    assert runs[2][1].tobytes() == runs[0][1].tobytes()
    assert g["a_pow1"].shape == runs[0][0].shape


def test_no_valid_window_raises():
    est = estimator("a_")
    est.indices = [np.array([1, 2, 3], dtype=np.int64)]    # every window starts before 0
    with pytest.raises(ValueError, match="index set 0"):
        est.estimate(case_signal("a_"), [60], bandwidth=8, window=1, surrogates=2,
                     verbose=False)


# ------------------------------------------------------------ the kernel alone
def _run_kernel(amps, indices, shifts, max_shift, W):
    import torch
    from openseize_amd import _device as dev
    sums = dev.zeros((len(shifts) + 1, W), torch.float64)
    counts = dev.zeros((len(shifts) + 1,), torch.int64)
    dshifts = torch.tensor(np.asarray(shifts, dtype=np.int64), device="cuda")
    for amp, idx in zip(amps, indices):
        dev.lock_accumulate(torch.from_numpy(amp).cuda(),
                            torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda(),
                            dshifts, max_shift, W, sums, counts)
    return sums.cpu().numpy(), counts.cpu().numpy()


def _geometry(rng, lengths, density, W, S, max_shift=None):
    amps = [rng.standard_normal(n) for n in lengths]
    indices = [np.flatnonzero(rng.random(n) < density) for n in lengths]
    max_shift = max_shift or max(lengths)
    shifts = rng.integers(0, max_shift, S)
    return amps, indices, shifts, max_shift, W


GEOMETRIES = {
    "random": lambda r: _geometry(r, [20000, 20000, 7000], 0.02, 1000, 20),
    "tile_plus_one": lambda r: _geometry(r, [30000], 0.01, 2049, 5),
    "W_gt_L": lambda r: _geometry(r, [3000, 3000, 500], 0.05, 1001, 4),
    "odd_prime_W": lambda r: _geometry(r, [10000, 4001], 0.03, 997, 7),
    "empty_set": lambda r: _geometry(r, [5000, 5000], 0.0, 101, 3),
    "short_last_chunk": lambda r: _geometry(r, [8000, 8000, 900], 0.05, 301, 30),
    "S1": lambda r: _geometry(r, [6000], 0.05, 64, 1),
    "S2000": lambda r: _geometry(r, [4000, 1500], 0.02, 37, 2000),
    "dense_wide": lambda r: _geometry(r, [12000], 0.3, 3000, 2),
    "W_gt_every_L": lambda r: _geometry(r, [500, 300], 0.1, 1001, 3),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_lock_accumulate_matches_restatement(name):
    rng = np.random.default_rng(sorted(GEOMETRIES).index(name) + 77)
    amps, indices, shifts, max_shift, W = GEOMETRIES[name](rng)
    got_s, got_c = _run_kernel(amps, indices, shifts, max_shift, W)
    want_s, want_c = lock_sums(amps, indices, shifts, max_shift, W)
    np.testing.assert_array_equal(got_c, want_c)
    scale = max(np.abs(want_s).max(), 1e-300)
    np.testing.assert_allclose(got_s, want_s, rtol=1e-12, atol=1e-12 * scale)
    again = _run_kernel(amps, indices, shifts, max_shift, W)
    assert again[0].tobytes() == got_s.tobytes()


def test_lock_accumulate_exact_edges():
    """Positions at exactly ceil(W/2) and L - W//2 count, one step outside does not, for
    the real set and for a shift that wraps them there."""
    W, L = 7, 50
    amp = np.arange(1.0, L + 1)
    idx = np.array([3, 4, 47, 48])     # h = 4: valid are 4 and 47 (47 + 7 // 2 = 50)
    shifts = [L - 1, 1, 3]             # -> {2, 3, 46, 47}, {4, 5, 48, 49}, {6, 7, 0, 1}
    got_s, got_c = _run_kernel([amp], [idx], shifts, L, W)
    want_s, want_c = lock_sums([amp], [idx], shifts, L, W)
    assert list(want_c) == [2, 2, 2, 2]
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_allclose(got_s, want_s, rtol=1e-15)
