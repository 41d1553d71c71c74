"""PhaseLock on the device: index() against the reference's indices, estimate() against
the reference's powers, p-values and rng state (tests/golden/g21_phaselock.npz), and the
osz_lock_accumulate kernel against the NumPy restatement of test_phaselock_host.py on
edge geometries.

EDGES pins the kernel to its own constants (csrc/coupling.hip), against the restatement in
long double:
  kLockSpan = kLockSeg - kLockTile = 6144   positions 6143 apart share a batch and read LDS up
                                            to index 6143 + kn - 1; 6144 apart they do not
  kLockTile = 512 * 4 = 2048                W = 2048, 2049, 4096, 4097: one, two, three tiles
  kLockQ = 512                              511, 512, 513 and 1025 positions; a batch that ends
                                            where its round ends, and one that ends inside it
  W = 1, 2, 3, L and L + 1 (no valid position); shifts 0, 1, max_shift - 1 and those that put a
  position on ceil(W/2) and on L - W//2 and one step outside, unwrapped and wrapped; max_shift
  above the chunk's length; an L = 0 chunk and a chunk without positions.
Counts are exact.  The sums are non-negative squares added in index order, so the kernel is within
(positions per set + 1) 2^-53 <= 2.3e-13 relative for the <= 2000 positions of every EDGES case;
asserted is this suite's 1e-12 of the row's largest entry.  Largest error measured on an MI355X
over EDGES: 2.5e-15 of the row scale (batch_end_on_round_end, 1025 positions per set); the cases of
three positions or fewer are within 1.9e-16."""

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
def _run_kernel(amps, indices, shifts, max_shift, W, init=None):
    """The accumulators after every chunk; ``init``: (sums, counts) to start from instead of zeros."""
    import torch
    from openseize_amd import _device as dev
    if init is None:
        sums = dev.zeros((len(shifts) + 1, W), torch.float64)
        counts = dev.zeros((len(shifts) + 1,), torch.int64)
    else:
        sums, counts = (torch.from_numpy(np.array(a)).cuda() for a in init)
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


# ------------------------------------------------------------ the kernel on its own constants
LOCK_THREADS, LOCK_PER = 512, 4              # kLockThreads, kLockPer: window offsets per thread
LOCK_TILE = LOCK_THREADS * LOCK_PER          # kLockTile = 2048 window offsets per workgroup
LOCK_SEG = 8192                              # kLockSeg: the amp^2 segment in LDS
LOCK_SPAN = LOCK_SEG - LOCK_TILE             # kLockSpan = 6144: a batch's positions span less than this
LOCK_Q = LOCK_THREADS                        # kLockQ = 512 positions staged per round
MAX_POSITIONS = 2000                         # per set: the kernel's error is at most this many u = 2^-53


def _span_case(rng, apart, W):
    """Three positions ``apart`` apart, the first window starting 5 samples into the chunk, the last ending
    with it.  6143 apart the first two share a batch and the second reads LDS up to 6143 + kn - 1 (kn = 2048
    for a full tile: index 8190 of 8192); 6144 apart every position starts a batch of its own."""
    h = -(-W // 2)
    idx = h + 5 + apart * np.arange(3)
    L = int(idx[-1]) + W // 2
    assert apart in (LOCK_SPAN - 1, LOCK_SPAN) and apart - 1 + min(W, LOCK_TILE) < LOCK_SEG
    return [rng.standard_normal(L)], [idx], np.array([0, 1, 7, L - 1]), L, W


def _round_case(rng, nidx, spacing, W=5):
    """``nidx`` valid positions ``spacing`` apart from the first valid one (h = 3) to the last (its window
    ends with the chunk); the shift by L // 2 splits them over the unwrapped and the wrapped range."""
    idx = -(-W // 2) + spacing * np.arange(nidx)
    L = int(idx[-1]) + W // 2
    return [rng.standard_normal(L)], [idx], np.array([0, spacing, L - 1, L // 2, 1]), L, W


def _window_case(rng, L, W, density=None, idx=None, shifts=None):
    idx = np.flatnonzero(rng.random(L) < density) if idx is None else np.asarray(idx)
    shifts = [0, 1, L - 1, int(rng.integers(0, L))] if shifts is None else shifts
    return [rng.standard_normal(L)], [idx], np.asarray(shifts, dtype=np.int64), L, W


def _chunks(rng, lengths, counts, shifts, max_shift, W):
    """Chunks of the given lengths with ``counts[i]`` seeded positions each (0: an empty index set)."""
    amps = [rng.standard_normal(n) for n in lengths]
    indices = [np.sort(rng.choice(n, k, replace=False)) if k else np.empty(0, dtype=np.int64)
               for n, k in zip(lengths, counts)]
    return amps, indices, np.asarray(shifts, dtype=np.int64), max_shift, W


EDGES = {}
for _W in (LOCK_TILE, LOCK_TILE + 1, 2 * LOCK_TILE + 1):
    # a batch span of exactly kLockSpan - 1 and of kLockSpan, with one, two and three tiles of offsets
    EDGES[f"span_{LOCK_SPAN - 1}_W{_W}"] = lambda r, W=_W: _span_case(r, LOCK_SPAN - 1, W)
    EDGES[f"span_{LOCK_SPAN}_W{_W}"] = lambda r, W=_W: _span_case(r, LOCK_SPAN, W)
for _n in (1, LOCK_Q - 1, LOCK_Q, LOCK_Q + 1, 2 * LOCK_Q + 1):
    # a round of exactly kLockQ positions, one fewer, one more, and two rounds and one position
    EDGES[f"round_{_n}"] = lambda r, n=_n: _round_case(r, n, 2)
EDGES.update({
    # 12 * kLockQ = kLockSpan: position 512 is exactly kLockSpan past position 0, so the batch that the span
    # rule would end there ends with the round as well; 13 apart the batch ends inside the round, at 473
    "batch_end_on_round_end": lambda r: _round_case(r, 2 * LOCK_Q + 1, LOCK_SPAN // LOCK_Q),
    "batch_end_inside_round": lambda r: _round_case(r, LOCK_Q + 88, LOCK_SPAN // LOCK_Q + 1),
    "W1": lambda r: _window_case(r, 5000, 1, 0.1),
    "W2": lambda r: _window_case(r, 5000, 2, 0.1),
    "W3": lambda r: _window_case(r, 5000, 3, 0.1),
    f"W{LOCK_TILE}": lambda r: _window_case(r, 12000, LOCK_TILE, 0.02),
    f"W{2 * LOCK_TILE}": lambda r: _window_case(r, 12000, 2 * LOCK_TILE, 0.02),
    # W = L: one valid position, ceil(W / 2); W = L + 1: none
    "W_eq_L_even": lambda r: _window_case(r, 1000, 1000, idx=range(497, 504), shifts=[0, 1, 2, 999, 998, 500]),
    "W_eq_L_odd": lambda r: _window_case(r, 1001, 1001, idx=range(497, 505), shifts=[0, 1, 2, 1000, 999, 500]),
    "W_eq_L_plus_1": lambda r: _window_case(r, 1000, 1001, 0.3),
    # h = 1025, qmax = 7975, max_shift = L = 9000: shifts that put a position on h, on qmax and one step
    # outside each, unwrapped (position 100) and wrapped (position 8000); W even and above kLockTile
    "shift_edges_W2050": lambda r: _window_case(
        r, 9000, LOCK_TILE + 2, idx=[100, 8000],
        shifts=[0, 1, 8999, 925, 924, 7875, 7876, 2025, 2024, 8975, 8976]),
    # h = 4, qmax = 46: test_lock_accumulate_exact_edges with an even W
    "shift_edges_W8": lambda r: _window_case(r, 50, 8, idx=[3, 4, 46, 47], shifts=[49, 1, 3, 0, 42, 43, 7, 8]),
    # max_shift above the chunk's length, as on a short last chunk: shifted positions fall past the data
    "max_shift_gt_L": lambda r: _chunks(r, [700], [70], [0, 1, 4999, 650, 4400, 4950], 5000, 101),
    "short_last_chunk": lambda r: _chunks(r, [3000, 700], [300, 70], [0, 1, 2999, 650, 2400], 3000, 101),
    # an L = 0 chunk and a chunk without positions between two real ones
    "empty_chunks_between": lambda r: _chunks(r, [4000, 0, 3000, 4000], [200, 0, 0, 200], [0, 1, 3999, 1234],
                                              4000, 301),
})
# counts worked out by hand for the case built to sit on h and qmax (set 0 first)
EDGE_COUNTS = {"shift_edges_W2050": [0, 0, 0, 0, 1, 0, 2, 1, 2, 1, 1, 0]}


def test_edges_sit_on_the_constants():
    assert (LOCK_TILE, LOCK_SPAN, LOCK_Q) == (2048, 6144, 512)
    r = np.random.default_rng(0)
    idx = EDGES["batch_end_on_round_end"](r)[1][0]
    assert idx[LOCK_Q] - idx[0] == LOCK_SPAN and idx[LOCK_Q - 1] - idx[0] < LOCK_SPAN and idx.size == 2 * LOCK_Q + 1
    idx = EDGES["batch_end_inside_round"](r)[1][0]
    assert idx[472] - idx[0] < LOCK_SPAN <= idx[473] - idx[0] and idx.size > LOCK_Q
    for name in EDGES:
        amps, indices, shifts, max_shift, W = EDGES[name](np.random.default_rng(1))
        assert sum(len(i) for i in indices) <= MAX_POSITIONS and all(0 <= s < max_shift for s in shifts), name
        assert all(np.all(np.diff(i) > 0) for i in indices), name
        if name.startswith(("span_", "round_")):      # first window from the chunk's start region, last to its end
            assert indices[0][-1] + W // 2 == amps[0].size, name


@pytest.mark.parametrize("name", sorted(EDGES))
def test_lock_accumulate_edges(name):
    """Counts exact; sums within 1e-12 of their row's largest entry of the long-double restatement (a row
    without positions must be exactly zero).  The sums are of non-negative squares added in index order,
    so the kernel's relative error is at most (positions per set + 1) u <= 2.3e-13 for the <= 2000 positions
    of every case here.  The worst error of each case is printed; the largest measured is in the module docstring."""
    rng = np.random.default_rng([sorted(EDGES).index(name), LOCK_Q])
    amps, indices, shifts, max_shift, W = EDGES[name](rng)
    want_s, want_c = lock_sums(amps, indices, shifts, max_shift, W, dtype=np.longdouble)
    assert want_c.max() <= MAX_POSITIONS
    if name in EDGE_COUNTS:
        assert list(want_c) == EDGE_COUNTS[name]
    got_s, got_c = _run_kernel(amps, indices, shifts, max_shift, W)
    np.testing.assert_array_equal(got_c, want_c)
    scale = np.abs(want_s).max(axis=1)
    err = np.abs(got_s.astype(np.longdouble) - want_s)
    live = scale > 0
    worst = float((err[live].max(axis=1) / scale[live]).max()) if live.any() else 0.0
    print(f"{name}: worst error {worst:.2e} of the row scale, at most {int(want_c.max())} positions per set")
    assert np.all(err <= 1e-12 * scale[:, None]), worst
    again = _run_kernel(amps, indices, shifts, max_shift, W)
    assert again[0].tobytes() == got_s.tobytes() and again[1].tobytes() == got_c.tobytes()


def test_no_valid_position_leaves_the_accumulators_alone():
    """W = L + 1, a chunk of length 0 and a chunk without positions add nothing: accumulators that already
    hold values keep their bytes."""
    rng = np.random.default_rng(1001)
    for name in ("W_eq_L_plus_1",):
        amps, indices, shifts, max_shift, W = EDGES[name](rng)
        sums0 = rng.standard_normal((len(shifts) + 1, W)) ** 2
        counts0 = np.arange(len(shifts) + 1, dtype=np.int64) * 3 + 1
        got_s, got_c = _run_kernel(amps, indices, shifts, max_shift, W, init=(sums0, counts0))
        assert got_s.tobytes() == sums0.tobytes() and got_c.tobytes() == counts0.tobytes()
    amps, indices, shifts, max_shift, W = EDGES["empty_chunks_between"](rng)
    assert [a.size for a in amps] == [4000, 0, 3000, 4000] and [i.size for i in indices] == [200, 0, 0, 200]
    both = _run_kernel(amps, indices, shifts, max_shift, W)
    real = _run_kernel(amps[::3], indices[::3], shifts, max_shift, W)
    assert both[0].tobytes() == real[0].tobytes() and both[1].tobytes() == real[1].tobytes()
    assert real[1][0] > 0
    # and alone on accumulators in use
    sums0, counts0 = real
    got_s, got_c = _run_kernel(amps[1:3], indices[1:3], shifts, max_shift, W, init=(sums0, counts0))
    assert got_s.tobytes() == sums0.tobytes() and got_c.tobytes() == counts0.tobytes()
