"""osz_phase_index (csrc/coupling.hip: phase_count_kernel, phase_scan_kernel, phase_scatter_kernel) called
through ctypes with work and output buffers of the test's own, against np.flatnonzero.  Every comparison is
exact: the indices, their count and their ascending order.

Ground truth without trigonometry: z[i] = m[i] * u[k[i]] with u the eight compass directions (+-1, 0),
(0, +-1), (+-1, +-1) and m a positive power of two, and the band (k0 pi/4 - 0.1, k0 pi/4 + 0.1).  The phase
of such a sample is within an ulp of k pi/4, so the samples that pass are exactly those with k == k0 whatever
the last bit of atan2, and the expected result is np.flatnonzero(k == k0).

Sizes, from kPiThreads = 256 (threads of the count and scatter blocks), kPiMaxBlk = 1024 (most partition
blocks, and the threads of the one scan block: 16 waves of 64) and the smallest span 16 * kPiThreads = 4096:
  0, 1, 63, 64, 65, 255, 256, 257      one block; a wave, a trip of the scatter loop, and one past each
  4095, 4096, 4097                     one block of the smallest span, then two (the second holds 1 sample)
  64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 1
                                       64, 64, 65 and 66 blocks: the scan's first wave is full, then block 64
                                       is the first to add a wave total (wsum) to its offset
  1023 * 4096 + 1, 1024 * 4096         1024 blocks of the smallest span: every scan thread has a block, and
                                       the total, taken from thread 1023, ends in a real block
  1024 * 4096 + 1                      the span grows: 4352, 964 blocks
  10 000 000                           PhaseLock's default chunk: span 9984, 1002 blocks
span and nblk are recomputed here by the entry point's formula and asserted to be these.

Patterns (PATTERNS): none, all, only sample 0, only sample n - 1, one per block at offset b mod span (the
last sample of a block that is shorter than that), (b mod 7) * 37 passes in block b at seeded places -- so
every block offset differs from a multiple of anything --, blocks 63 and 64 full and the rest empty, the last
(partial) block full and the rest empty, seeded random at density 0.3.  The three largest sizes keep none,
all, one per block and random.

Buffers: work (2049 int64) and out (n + 64 int64) are filled with -1 before the call; out[count:] must be -1
afterwards, the tail past n included.  A second call with another poison must give the same count and
indices, a third call with the first poison the same bytes.

Also: the strictness of both comparisons at a phase that is exactly float64(pi); NaN, infinite, zero and
signed-zero samples against np.arctan2 mapped as phase_2pi (common.h) documents, cross-checked bit for bit
against osz_magphase's phase; and the dev.phase_index wrapper against the raw call.

On an MI355X the 10 000 000-sample size took 0.6 s for its four patterns, nearly all of it building and
uploading the 160 MB of samples; the other three large sizes took 0.25 s each, no small size over 0.1 s."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PI_THREADS, PI_MAXBLK = 256, 1024          # kPiThreads, kPiMaxBlk
MIN_SPAN = 16 * PI_THREADS
WORK_LEN = 2 * PI_MAXBLK + 1               # blkcnt, blkoff, total
TAIL = 64                                  # out is this much longer than n
K0 = 3                                     # the band sits on 3 pi / 4

UX = np.array([1.0, 1.0, 0.0, -1.0, -1.0, -1.0, 0.0, 1.0])
UY = np.array([0.0, 1.0, 1.0, 1.0, 0.0, -1.0, -1.0, -1.0])


def partition(n):
    """(span, nblk) of osz_phase_index."""
    span = max(-(-n // PI_MAXBLK), MIN_SPAN)
    span = -(-span // PI_THREADS) * PI_THREADS
    return span, -(-n // span)


SMALL = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097,
         64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 1)
LARGE = (1023 * 4096 + 1, 1024 * 4096, 1024 * 4096 + 1, 10_000_000)
PATTERNS = ("none", "all", "first", "last", "one_per_block", "ramp", "blocks_63_64", "last_block", "random")
LARGE_PATTERNS = ("none", "all", "one_per_block", "random")


def test_sizes_mean_what_they_say():
    assert partition(4095) == (4096, 1) and partition(4096) == (4096, 1) and partition(4097) == (4096, 2)
    assert [partition(n)[1] for n in (64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 1)] == [64, 64, 65, 66]
    assert partition(1023 * 4096 + 1) == (4096, 1024) and partition(1024 * 4096) == (4096, 1024)
    assert partition(1024 * 4096 + 1) == (4352, 964)
    assert partition(10_000_000) == (9984, 1002)
    assert all(partition(n)[0] == MIN_SPAN for n in SMALL + LARGE[:2] if n)
    assert all(partition(n)[1] <= PI_MAXBLK for n in SMALL + LARGE if n)
    assert 0 < 10_000_000 - 1001 * 9984 < 9984 and 0 < 1024 * 4096 + 1 - 963 * 4352 < 4352   # partial last blocks


def mask_of(pattern, n, rng):
    """The samples that pass, a bool vector, or None where the pattern does not apply to n."""
    span, nblk = partition(n) if n else (MIN_SPAN, 0)
    m = np.zeros(n, dtype=bool)
    if pattern == "none":
        return m
    if n == 0:
        return None
    starts = np.arange(nblk, dtype=np.int64) * span
    ends = np.minimum(starts + span, n)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[n - 1] = True
    elif pattern == "one_per_block":
        m[np.minimum(starts + np.arange(nblk) % span, ends - 1)] = True
    elif pattern == "ramp":
        for b in range(nblk):
            size = int(ends[b] - starts[b])
            m[starts[b] + rng.choice(size, min((b % 7) * 37, size), replace=False)] = True
    elif pattern == "blocks_63_64":
        if nblk < 64:
            return None
        m[starts[63]:ends[min(64, nblk - 1)]] = True
    elif pattern == "last_block":
        m[starts[-1]:] = True
    elif pattern == "random":
        m = rng.random(n) < 0.3
    else:
        raise KeyError(pattern)
    return m


class Samples:
    """z[i] = m[i] * u[k[i]]: the samples that do not pass are drawn once per size, the mask picks those
    that point along u[K0]."""

    def __init__(self, n, rng, k0=K0):
        self.n, self.k0 = n, k0
        self.other = (k0 + 1 + rng.integers(0, 7, n)) % 8
        assert not np.any(self.other == k0)
        self.m = 2.0 ** rng.integers(-20, 21, n)
        self.base = np.stack([self.m * UX[self.other], self.m * UY[self.other]], axis=1)

    def z(self, mask):
        """(z as an (n, 2) float64 array, the expected indices)."""
        z = self.base.copy()
        z[mask, 0], z[mask, 1] = self.m[mask] * UX[self.k0], self.m[mask] * UY[self.k0]
        k = np.where(mask, self.k0, self.other)
        return z, np.flatnonzero(k == self.k0)

    @property
    def band(self):
        return self.k0 * np.pi / 4 - 0.1, self.k0 * np.pi / 4 + 0.1


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


def raw_call(dev, zd, n, lo, hi, poison=-1):
    """One osz_phase_index call on the device samples zd ((n, 2) float64): (count, out of n + TAIL int64, work),
    the two buffers still on the device."""
    import torch
    from openseize_amd import _lib
    work = torch.full((WORK_LEN,), poison, dtype=torch.int64, device="cuda")
    out = torch.full((n + TAIL,), poison, dtype=torch.int64, device="cuda")
    count = ctypes.c_int64(-99)
    _lib.check(_lib.load().osz_phase_index(dev.ptr(zd) if n else None, n, float(lo), float(hi), dev.ptr(work),
                                           dev.ptr(out), ctypes.byref(count), dev.stream_ptr()))
    return count.value, out, work


def check_case(dev, z, lo, hi, want, what):
    """Three calls on z: the count, the indices and their order are ``want`` exactly, nothing is written past
    the count or outside the work entries in use, another poison changes nothing, a repeat gives the same bytes.
    (The comparisons of the buffers run on the device; only the count and the work vector come back.)"""
    import torch
    n = len(z)
    zd = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    wd = torch.from_numpy(np.ascontiguousarray(want, dtype=np.int64)).cuda()
    count, out, work = raw_call(dev, zd, n, lo, hi)
    assert count == want.size, (what, count, want.size)
    assert torch.equal(out[:count], wd), (what, "indices")
    assert bool((out[count:] == -1).all()), (what, "written past the count")
    work = work.cpu().numpy()
    if n:
        span, nblk = partition(n)
        assert work[2 * PI_MAXBLK] == count and np.all(work[nblk:PI_MAXBLK] == -1), (what, "work")
        assert np.all(work[PI_MAXBLK + nblk:2 * PI_MAXBLK] == -1), (what, "work")
    else:
        assert np.all(work == -1), (what, "work touched at n = 0")
    other = 0x5555555555
    count2, out2, _ = raw_call(dev, zd, n, lo, hi, poison=other)
    assert count2 == count and torch.equal(out2[:count], wd), (what, "depends on the poison")
    assert bool((out2[count:] == other).all()), (what, "written past the count")
    count3, out3, work3 = raw_call(dev, zd, n, lo, hi)
    assert count3 == count and torch.equal(out3, out) and work3.cpu().numpy().tobytes() == work.tobytes(), what


def _run_size(dev, n, patterns):
    rng = np.random.default_rng([n, 4096])
    s = Samples(n, rng)
    ran = []
    for pattern in patterns:
        mask = mask_of(pattern, n, rng)
        if mask is None:
            continue
        z, want = s.z(mask)
        assert np.array_equal(want, np.flatnonzero(mask))
        check_case(dev, z, *s.band, want, (n, pattern))
        ran.append(pattern)
    return ran


@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_every_pattern(dev, n):
    ran = _run_size(dev, n, PATTERNS)
    if n == 0:
        assert ran == ["none"]
    else:
        assert ran == [p for p in PATTERNS if p != "blocks_63_64" or partition(n)[1] >= 64]
    assert ("blocks_63_64" in ran) == (n >= 64 * 4096 - 1)


@pytest.mark.parametrize("n", LARGE)
def test_large_sizes(dev, n):
    assert _run_size(dev, n, LARGE_PATTERNS) == list(LARGE_PATTERNS)


@pytest.mark.parametrize("k0", range(8))
def test_every_compass_direction(dev, k0):
    """The band on each of the eight directions, k0 = 0 included: its band (-0.1, 0.1) takes phase 0 and
    nothing near 2 pi, because no compass sample lies there."""
    n = 2 * 4096 + 77
    rng = np.random.default_rng([k0, 8])
    s = Samples(n, rng, k0=k0)
    z, want = s.z(rng.random(n) < 0.3)
    check_case(dev, z, *s.band, want, ("compass", k0))


def test_both_comparisons_are_strict(dev):
    """z = (-1, +0) has the phase float64(pi) exactly: lo = pi excludes it, hi = pi excludes it, the next
    float64 on the far side of either includes it."""
    z = np.array([[1.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [-1.0, 0.0], [-2.0, 0.0], [1.0, 0.0]])
    at = np.array([1, 3, 4])
    assert np.all(np.arctan2(z[at, 1], z[at, 0]) == np.pi)
    none = np.empty(0, dtype=np.int64)
    check_case(dev, z, np.pi, 4.0, none, "lo = pi")
    check_case(dev, z, 3.0, np.pi, none, "hi = pi")
    check_case(dev, z, np.nextafter(np.pi, 0.0), 4.0, at, "lo just below pi")
    check_case(dev, z, 3.0, np.nextafter(np.pi, 4.0), at, "hi just above pi")
    check_case(dev, z, np.nextafter(np.pi, 0.0), np.nextafter(np.pi, 4.0), at, "one float64 inside")
    check_case(dev, z, np.pi, np.pi, none, "an empty band")


SPECIAL = np.array([[np.nan, 1.0], [1.0, np.nan], [np.inf, np.inf], [0.0, 0.0], [-0.0, -0.0], [0.0, -0.0],
                    [1.0, -1e-300], [1.0, 0.0], [-1.0, -0.0], [-np.inf, 1.0], [np.nan, np.nan]])


def phase_2pi(z):
    """numpy.angle mapped as phase_2pi of common.h: 2 pi added to a negative angle (-0.0 is not negative)."""
    p = np.arctan2(z[:, 1], z[:, 0])
    return np.where(p < 0, p + 2 * np.pi, p)


def test_special_samples(dev):
    import torch
    # the specials, ordinary samples across a block edge, the specials again
    rng = np.random.default_rng(12)
    k = len(SPECIAL)
    z = np.concatenate([SPECIAL, rng.standard_normal((4096 + 50, 2)), SPECIAL[::-1]])
    special = np.r_[0:k, len(z) - k:len(z)]
    p = phase_2pi(z)
    assert np.isnan(p[[0, 1, 10]]).all() and p[2] == np.pi / 4 and p[3] == 0 and not np.signbit(p[3])
    assert p[4] == np.pi and p[5] == 0 and np.signbit(p[5]) and p[6] == 2 * np.pi and p[7] == 0
    assert p[8] == np.pi and p[9] == np.pi
    # osz_magphase reports these phases bit for bit, as common.h promises of the two kernels' shared phase_2pi
    _, ph = dev.magphase(torch.from_numpy(z.copy()).view(torch.complex128).reshape(1, -1).cuda(), want_mag=False)
    ph = ph.cpu().numpy()[0]
    assert np.array_equal(np.isnan(ph[special]), np.isnan(p[special]))
    fin = special[~np.isnan(p[special])]
    assert np.array_equal(ph[fin].view(np.uint64), p[fin].view(np.uint64))
    bands = [(-0.05, 0.05),               # takes 0 and -0.0, nothing near 2 pi (the reference compares likewise)
             (-np.inf, np.inf),           # everything but NaN: a NaN phase never passes
             (6.2, 6.3), (2 * np.pi, 7.0), (6.2, 2 * np.pi),     # 2 pi itself is a phase: strict on both sides
             (0.7, 0.8), (3.1, 3.2), (0.0, 7.0), (-1.0, 0.0), (np.nan, 7.0), (0.0, np.nan)]
    ordinary = np.setdiff1d(np.arange(len(z)), special)
    for lo, hi in bands:
        # no ordinary sample is so near a bound that the last bit of atan2 decides; the specials are exact
        for bound in (lo, hi):
            assert not np.any(np.abs(p[ordinary] - bound) < 1e-9)
        with np.errstate(invalid="ignore"):
            want = np.flatnonzero((p > lo) & (p < hi))
        check_case(dev, z, lo, hi, want, ("special", lo, hi))
    assert np.flatnonzero((p[:k] > -0.05) & (p[:k] < 0.05)).tolist() == [3, 5, 7]
    assert np.flatnonzero((p[:k] > -np.inf) & (p[:k] < np.inf)).tolist() == [2, 3, 4, 5, 6, 7, 8, 9]
    assert np.flatnonzero((p[:k] > 6.2) & (p[:k] < 2 * np.pi)).tolist() == []


def test_wrapper_returns_the_raw_indices(dev):
    import torch
    n = 65 * 4096 + 1
    rng = np.random.default_rng(65)
    s = Samples(n, rng)
    z, want = s.z(rng.random(n) < 0.3)
    zd = torch.from_numpy(z).cuda()
    count, out, _ = raw_call(dev, zd, n, *s.band)
    got = dev.phase_index(zd.view(torch.complex128).reshape(-1), *s.band)
    assert got.is_cuda and got.dtype == torch.int64 and got.numel() == count == want.size
    assert torch.equal(got, out[:count]) and np.array_equal(got.cpu().numpy(), want)
    empty = dev.phase_index(zd.view(torch.complex128).reshape(-1)[:0], *s.band)
    assert empty.numel() == 0 and empty.dtype == torch.int64
