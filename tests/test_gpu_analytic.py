"""GPU tests of analytic_connectivity (K13) against ``analytic_measures``, the NumPy restatement
of the definitions that tests/test_analytic_host.py pins.

Both sides get the same complex128 array, so the only error is in evaluating the terms and in
the order of the sums.  tau = (N + 16) 2^-53 bounds the relative error of any sum of N terms
against the sum of its terms' magnitudes: the worst case of any summation order, N 2^-53, plus a
few roundings per term.  Propagated to first order (test_analytic_host.bounds):
  a Pearson r   dcov = tau (sum|pq| + 2 |sum p sum q| / N), dvar_p = tau (sum p^2 + 2 (sum p)^2 / N),
                bound = dcov / sqrt(var_p var_q) + |r| (dvar_p / var_p + dvar_q / var_q) / 2
                (aec: one r; oaec: the mean of the bounds of its two);
  plv, wpli     2 tau (a ratio of a sum to a sum of magnitudes / to N);
  ciplv         tau (1 / sqrt(1 - R^2) + |I| |R| / (1 - R^2)^(3/2)), s = R + i I.
Every bound is asserted to be <= 1e-9 (the suite's RTOL) on the yardstick alone, then the error to
be within its bound entry by entry.  What must be the same bits is compared as bits.

Shapes: the lane's register tile is 4 channels and the workgroup's 8, so 2, 3, 5, 7, 8, 9 channels
and 17 (three block rows); N = 37 (less than a wave), one block, one block + 1, three blocks + 37."""

from functools import lru_cache

import numpy as np
import pytest

from test_analytic_host import FS, METHODS, RTOL, analytic_measures, bounds, mixture

pytestmark = pytest.mark.gpu

BLOCK = 4096
NMAX = 3 * BLOCK + 37
SHAPES = [(nch, NMAX) for nch in (2, 3, 5, 7, 8, 9, 17)]
SHAPES += [(5, 37), (17, 37), (9, BLOCK), (3, BLOCK), (8, BLOCK + 1), (5, BLOCK + 1)]


@pytest.fixture(scope="module")
def conn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()      # fails loudly if the HIP library was not built
    from openseize_amd.experimental.coupling import connectivity
    assert connectivity._BLOCK == BLOCK
    return connectivity


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint64)


def signal(nch, n):
    """The zero-lag mixture of test_analytic_host, cut to n samples (read-only)."""
    return mixture(nch, NMAX)[:, :n]


@lru_cache(maxsize=None)
def yardstick(nch, n):
    return analytic_measures(signal(nch, n))


def within_bounds(got, want, parts, label):
    nch = want["aec"].shape[0]
    off = ~np.eye(nch, dtype=bool)
    limit = bounds(parts)
    for name in METHODS:
        m = host(got[name])
        assert m.dtype == np.float64 and m.shape == (nch, nch)
        err = np.abs(m - want[name])
        print(f"{label} {name}: max err {np.max(err[off]):.2e}, largest bound {np.max(limit[name][off]):.2e}")
        assert np.max(limit[name][off]) <= RTOL, name
        assert np.all(err[off] <= limit[name][off]), name
        assert np.all(m[~off] == (1.0 if name in ("aec", "plv") else 0.0)), name
        assert np.array_equal(bits(m.T), bits(m)), name


@pytest.mark.parametrize("nch,n", SHAPES, ids=[f"{c}ch-{n}" for c, n in SHAPES])
def test_measures_are_the_yardstick(conn, nch, n):
    want, parts = yardstick(nch, n)
    cnt, got = conn.analytic_connectivity(signal(nch, n), method=METHODS)
    assert cnt == n and tuple(got) == METHODS
    within_bounds(got, want, parts, f"{nch} ch x {n}")


@pytest.mark.parametrize("nch", [2, 5, 17])
def test_accumulate_kernel_alone(conn, nch):
    """osz_analytic_accumulate on random complex data against NumPy: every sum within tau of the
    sum of its terms' magnitudes, 37 samples and seven blocks, the strictly lower triangle
    untouched, and 7 blocks = 3 + 4 in two calls bit for bit."""
    import torch
    from openseize_amd import _device as dev
    rng = np.random.default_rng(nch)
    upper = np.triu(np.ones((nch, nch), bool))
    for n in (37, 7 * BLOCK):
        tau = (n + 16) * 2.0 ** -53
        z = rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))
        a = np.abs(z)
        u = z / a
        want, mag = np.zeros((10, nch, nch)), np.zeros((10, nch, nch))
        for i in range(nch):
            q = np.conj(z[i]) * z                                   # (nch, n): row j is the pair (i, j)
            d, m = q.imag, np.abs(q.imag)
            want[0, i] = mag[0, i] = (a[i] * a).sum(1)
            want[1, i] = mag[1, i] = want[9, i] = mag[9, i] = mag[8, i] = m.sum(1)
            want[2, i] = mag[2, i] = (m / a[i]).sum(1)
            want[3, i] = mag[3, i] = (m / a).sum(1)
            want[4, i] = mag[4, i] = ((m / a[i]) ** 2).sum(1)
            want[5, i] = mag[5, i] = ((m / a) ** 2).sum(1)
            s = np.conj(u[i]) * u
            want[6, i], want[7, i], want[8, i] = s.real.sum(1), s.imag.sum(1), d.sum(1)
            mag[6, i] = (np.abs(u[i].real * u.real) + np.abs(u[i].imag * u.imag)).sum(1)
            mag[7, i] = (np.abs(u[i].real * u.imag) + np.abs(u[i].imag * u.real)).sum(1)
        sums = torch.zeros((10, nch, nch), dtype=torch.float64, device="cuda")
        sums[:, cuda(~upper)] = -7.0                                # (what the tensor held before)
        chan = torch.zeros((3, nch), dtype=torch.float64, device="cuda")
        start = sums.clone()
        dev.analytic_accumulate(cuda(z), 15, sums, chan)
        got = host(sums)
        assert np.all(got[:, ~upper] == -7.0)
        err = np.abs(got - want)[:, upper]
        print(f"{nch} ch x {n}: worst error / (tau magnitude) {np.max(err / (tau * mag[:, upper])):.3f}")
        assert np.all(err <= tau * mag[:, upper])
        own = np.stack([a.sum(1), (a * a).sum(1), np.full(nch, float(n))])
        assert np.all(np.abs(host(chan) - own) <= tau * own)
        # one group alone keeps the bits it has among all four
        lag = torch.zeros((2, nch, nch), dtype=torch.float64, device="cuda")
        dev.analytic_accumulate(cuda(z), 8, lag, torch.zeros_like(chan))
        assert np.array_equal(bits(lag)[:, upper], bits(sums[8:])[:, upper])
        assert np.array_equal(bits(sums[9])[upper], bits(sums[1])[upper])        # sum m of ORTH and of LAG
        if n == 7 * BLOCK:
            parts, cparts = start.clone(), torch.zeros_like(chan)
            zd = cuda(z)
            dev.analytic_accumulate(zd[:, :3 * BLOCK], 15, parts, cparts)
            dev.analytic_accumulate(zd[:, 3 * BLOCK:], 15, parts, cparts)
            assert np.array_equal(bits(parts), bits(sums)) and np.array_equal(bits(cparts), bits(chan))


def test_cuts_of_one_stream_agree(conn):
    from openseize_amd import producer
    nch, n = 5, NMAX
    z = signal(nch, n)
    cnt, onhost = conn.analytic_connectivity(z, method=METHODS)
    cnt_r, resident = conn.analytic_connectivity(cuda(z), method=METHODS)
    cnt_p, chunked = conn.analytic_connectivity(producer(z, 1000, -1), method=METHODS)
    cnt_c, coarse = conn.analytic_connectivity(z, method=METHODS, chunksize=5000)
    _, again = conn.analytic_connectivity(z, method=METHODS)
    cnt_t, turned = conn.analytic_connectivity(np.ascontiguousarray(z.T), method=METHODS, axis=0)
    mask = np.random.default_rng(5).random(n) > 0.3
    cnt_m, masked = conn.analytic_connectivity(producer(z, 1000, -1, mask=mask), method=METHODS)
    cnt_k, kept = conn.analytic_connectivity(np.ascontiguousarray(z[:, mask]), method=METHODS)
    # pushes of one block each
    whole = conn._PUSH_BYTES
    conn._PUSH_BYTES = 1
    try:
        cnt_s, pieces = conn.analytic_connectivity(z, method=METHODS)
    finally:
        conn._PUSH_BYTES = whole
    assert cnt == cnt_r == cnt_p == cnt_c == cnt_t == cnt_s == n and cnt_m == cnt_k == int(mask.sum())
    for name in METHODS:
        for label, other in (("resident", resident), ("chunked", chunked), ("coarse", coarse), ("again", again),
                             ("turned", turned), ("pieces", pieces)):
            assert np.array_equal(bits(other[name]), bits(onhost[name])), (name, label)
        assert np.array_equal(bits(masked[name]), bits(kept[name])), name
        # one name alone: the same bits as in the tuple
        cnt_1, alone = conn.analytic_connectivity(z, method=name)
        assert cnt_1 == n and isinstance(alone, np.ndarray)
        assert np.array_equal(bits(alone), bits(onhost[name])), name


def test_result_lives_where_the_data_lives(conn):
    import torch
    from openseize_amd import producer
    z = signal(4, BLOCK + 1)
    order = ("wpli", "aec", "ciplv")
    _, onhost = conn.analytic_connectivity(z, method=order)
    _, ondev = conn.analytic_connectivity(cuda(z), method=order)
    _, chained = conn.analytic_connectivity(producer(cuda(z), 1500, -1))
    _, single = conn.analytic_connectivity(z, method=("plv",))
    assert tuple(onhost) == tuple(ondev) == order and tuple(single) == ("plv",)
    assert torch.is_tensor(chained) and chained.is_cuda and chained.dtype == torch.float64
    for name in order:
        assert isinstance(onhost[name], np.ndarray)
        m = ondev[name]
        assert torch.is_tensor(m) and m.is_cuda and m.dtype == torch.float64 and tuple(m.shape) == (4, 4)
        assert np.array_equal(bits(m), bits(onhost[name]))
    _, oaec = conn.analytic_connectivity(z, method="oaec")
    assert np.array_equal(bits(chained), bits(oaec))                         # (oaec is the default)
    with pytest.raises(ValueError, match="without a sample"):
        conn.analytic_connectivity(np.zeros((3, 0), complex))


@pytest.mark.parametrize("bad", [np.nan, np.inf, 0.0], ids=["nan", "inf", "zero"])
def test_bad_samples_stay_in_their_row_and_column(conn, bad):
    nch, n = 9, BLOCK + 37
    z = np.array(signal(nch, n))
    _, clean = conn.analytic_connectivity(z, method=METHODS)
    z[2, 1234] = bad
    rest = [c for c in range(nch) if c != 2]
    others = np.ix_(rest, rest)
    for data in (z, cuda(z)):
        _, got = conn.analytic_connectivity(data, method=METHODS)
        for name in METHODS:
            m = host(got[name])
            assert np.all(np.isnan(m[2])) and np.all(np.isnan(m[:, 2])), name
            assert np.all(np.isfinite(clean[name]))
            assert np.array_equal(bits(m[others]), bits(clean[name][others])), name


def test_band_pass_to_analytic_to_connectivity(conn):
    """Real data -> Butter (zero-phase) -> Analytic -> analytic_connectivity, against the
    yardstick on the same producer's chunks gathered with to_array: the plumbing (complex chunks,
    chunk sizes that are no multiple of the block), not the filters."""
    from openseize_amd import producer
    from openseize_amd.experimental.coupling.transforms import Analytic
    from openseize_amd.filtering.iir import Butter
    nch, n, cs = 4, 20000, 3000
    x = np.random.default_rng(9).standard_normal((nch, n))
    x[1] += 0.5 * x[0]
    filt = Butter(fpass=[8, 30], fstop=[4, 40], fs=FS, gpass=1, gstop=40)
    an = Analytic(filt(producer(x, cs, -1), chunksize=cs, axis=-1, dephase=True), FS, cs, -1, width=4)
    z = an.signal.to_array(dtype=complex)
    assert isinstance(z, np.ndarray) and z.shape == (nch, n) and np.iscomplexobj(z)
    want, parts = analytic_measures(z)
    cnt, got = conn.analytic_connectivity(an.signal, method=METHODS)
    assert cnt == n and all(isinstance(got[name], np.ndarray) for name in METHODS)
    within_bounds(got, want, parts, "chain")
    # the same signal as one array: the same bits
    _, direct = conn.analytic_connectivity(z, method=METHODS)
    for name in METHODS:
        assert np.array_equal(bits(direct[name]), bits(got[name])), name
