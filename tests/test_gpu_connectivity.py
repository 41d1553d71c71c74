"""window_connectivity on the device (K19) against ``window_pair_measures``, the NumPy long-double
restatement (tests/test_connectivity_host.py; for complex data ``analytic_measures`` of
tests/test_analytic_host.py window by window).

Caps.  RTOL = 1e-9 (the suite's cap, tests/test_gpu_parity.py): absolute for ``corr``, ``aec`` and
``plv``, times sqrt(c_ii c_jj) for ``cov``, times the condition factor 1 / sqrt(1 - R^2) +
|I| |R| / (1 - R^2)^1.5 for ``ciplv`` (``bounds`` of tests/test_analytic_host.py), R and I from
the long-double restatement.  No entry is left out, and every factor on these inputs is asserted
to be finite.  On exactly these inputs ``shifted_scheme`` -- the kernel's scheme in float64: sums
about each window's first sample, Pearson's r from the five sums, the phasor Gram entries -- stays
within 1.4e-5 of the caps (worst: ``cov``, C = 65 at 100 sigma, W = 250; ``aec`` 1.1e-5 at W = 1000,
``corr`` 8.4e-6, ``plv`` 6.7e-7, ``ciplv`` 3.3e-7): the caps leave more than four orders of margin, a
failure is a bug and not rounding.

Inputs.  Real: seeded normal noise (C, 6000), channel 1 replaced by channel 0 + 0.5 channel 1, at
offsets of 0 and 100 sigma, C in 3, 16, 17, 33 and 65: both sides of a 16-row tile, a second and
third tile row, and -- the workgroup's block being 64 rows -- 65 for a second block row.
Complex: ``mixture(C, 6000)``, and complex white noise of 100 samples for W < 64.  The restatement
costs 0.1 ms per pair and window in Python, so C = 3, 16 and 17 run every shape and C = 33 (66
phasor rows: the second block row of the phasor product) the shapes of at most 16 windows.

Everything else here is bit for bit."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_analytic_host import analytic_measures, bounds, mixture
from test_connectivity_host import COMPLEX, REAL, RTOL, caps, window_starts

pytestmark = pytest.mark.gpu

BLOCK = _lib.WC_BLOCK
N = max(6000, BLOCK + 2501 + 1)              # (the three shapes about BLOCK need two windows 2500 apart)
SHAPES = [(4, 1), (5, 3), (63, 63), (64, 64), (65, 65), (67, 200), (250, 125), (1000, 333),
          (BLOCK - 1, 2500), (BLOCK, 2500), (BLOCK + 1, 2500)]
FEW = [(W, step) for W, step in SHAPES if (6000 - W) // step + 1 <= 16]
CUTS = [(250, 125), (67, 200), (BLOCK + 1, 2500)]


@pytest.fixture(scope="module")
def wc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_connectivity
    return window_connectivity


@lru_cache(maxsize=None)
def real(nch, offset=0.0):
    """Seeded normal noise (nch, N), channel 1 mixed with channel 0, plus ``offset`` sigma.  Read-only."""
    x = np.random.default_rng(19).standard_normal((nch, N))
    x[1] = x[0] + 0.5 * x[1]
    x += offset
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def analytic(nch, W):
    """The complex input of a shape: the band-limited mixture, white noise for W < 64.  Read-only."""
    if W >= 64:
        return mixture(nch, N)
    rng = np.random.default_rng(23)
    z = rng.standard_normal((nch, 100)) + 1j * rng.standard_normal((nch, 100))
    z.setflags(write=False)
    return z


@lru_cache(maxsize=None)
def device_all(kind, nch, offset, W, step):
    """(nwin, every measure of the kind) from one array call, computed once."""
    from openseize_amd.features import window_connectivity
    x = real(nch, offset) if kind == "real" else analytic(nch, W)
    return window_connectivity(x, W, step, measures=REAL if kind == "real" else COMPLEX)


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_within_caps(got, x, W, step, label):
    want, cap = caps(x, W, step)
    for name in want:
        g = got[name]
        assert g.shape == want[name].shape and g.dtype == np.float64, (name, g.shape)
        assert np.all(np.isfinite(cap[name])) and np.all(cap[name] > 0), (label, name)
        ratio = float(np.max(np.abs(g - want[name]) / cap[name]))
        print(f"{label} W={W} step={step} {name}: {ratio:.2e} of the cap")
        assert np.all(np.abs(g - want[name]) <= cap[name]), (label, name, W, step, ratio)
        assert same_bits(g, np.swapaxes(g, 1, 2)), name


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("nch", [3, 16, 17, 33, 65])
@pytest.mark.parametrize("W,step", SHAPES)
def test_real_parity_with_the_restatement(wc, W, step, nch, offset):
    x = real(nch, offset)
    nwin, M = device_all("real", nch, offset, W, step)
    assert nwin == (N - W) // step + 1 and list(M) == list(REAL)
    assert_within_caps(M, x, W, step, f"real C={nch} +{offset}")
    assert np.all(np.diagonal(M["corr"], axis1=1, axis2=2) == 1.0)


@pytest.mark.parametrize("nch,W,step", [(c, W, s) for c in (3, 16, 17) for W, s in SHAPES]
                         + [(33, W, s) for W, s in FEW])
def test_complex_parity_with_the_restatement(wc, W, step, nch):
    z = analytic(nch, W)
    nwin, M = device_all("complex", nch, 0.0, W, step)
    assert nwin == (z.shape[1] - W) // step + 1 and list(M) == list(COMPLEX)
    assert_within_caps(M, z, W, step, f"complex C={nch}")
    for name in COMPLEX:
        assert np.all(np.diagonal(M[name], axis1=1, axis2=2) == (0.0 if name == "ciplv" else 1.0)), name


def sources(kind):
    return (real(17, 100.0), REAL) if kind == "real" else (analytic(3, 250), COMPLEX)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("W,step", CUTS)
def test_chunking_host_or_device_and_axis_change_no_bit(wc, W, step, kind):
    import torch
    x, names = sources(kind)
    nwin, F = device_all(kind, x.shape[0], 100.0 if kind == "real" else 0.0, W, step)
    for cs in (7, 249, 250, 251, 4099):
        n2, G = wc(producer(np.array(x), cs, -1), W, step, measures=names)
        assert n2 == nwin
        for name in names:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (cs, name)
    n2, G = wc(torch.from_numpy(np.array(x)).cuda(), W, step, measures=names, chunksize=3001)
    assert n2 == nwin
    for name in names:
        assert G[name].is_cuda and same_bits(G[name], F[name]), name
    n2, G = wc(np.ascontiguousarray(x.T), W, step, measures=names, axis=0, chunksize=5000)
    assert n2 == nwin
    for name in names:
        assert G[name].shape == (nwin, x.shape[0], x.shape[0]) and same_bits(G[name], F[name]), name


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_a_single_name_is_its_entry_of_the_whole(wc, kind):
    x, names = sources(kind)
    nwin, F = device_all(kind, x.shape[0], 100.0 if kind == "real" else 0.0, 250, 125)
    for name in names:
        n2, one = wc(x, 250, 125, measures=name)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
        assert same_bits(one, np.swapaxes(one, 1, 2)), name
    back = tuple(reversed(names))
    n2, G = wc(x, 250, 125, measures=back)
    assert list(G) == list(back) and all(same_bits(G[name], F[name]) for name in names)
    if kind == "real":
        n2, G = wc(x, 250)                                   # the defaults: step = winsize, ("corr",)
        assert n2 == N // 250 and list(G) == ["corr"] and same_bits(G["corr"], F["corr"][::2])
        n2, c0 = wc(x, 250, 125, measures="cov", ddof=0)     # ddof enters cov alone, as one division
        assert np.max(np.abs(c0 * 250 / 249 - F["cov"]) / np.abs(F["cov"])) < 1e-15


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("W", [250, BLOCK + 1])
def test_an_entry_depends_on_its_own_two_channels_and_window_only(wc, W, kind):
    """The first 5 channels of the C = 33 input given alone are the [:5, :5] corner of the whole
    (C = 65 for real data: a second block row), and a window's matrix does not depend on step."""
    big = real(65, 100.0) if kind == "real" else analytic(33, W)
    names = REAL if kind == "real" else COMPLEX
    step = W // 2
    nwin, F = wc(big, W, step, measures=names)
    n5, G = wc(big[:5], W, step, measures=names)
    assert n5 == nwin
    for name in names:
        assert same_bits(G[name], F[name][:, :5, :5]), name
    # rows 60 .. 64 (across the block's edge) alone, and the last 6 rows of 33 (their phasor rows
    # move from 27 .. 32 and 60 .. 65 to 0 .. 5 and 6 .. 11)
    lo = big.shape[0] - (5 if kind == "real" else 6)
    n5, G = wc(big[lo:], W, step, measures=names)
    for name in names:
        assert same_bits(G[name], F[name][:, lo:, lo:]), name
    # step changed with W fixed: windows that start at the same sample agree
    n2, H = wc(big[:17], W, 2 * step, measures=names)
    n3, K = wc(big[:17], W, step + 1, measures=names)
    assert n2 == (nwin + 1) // 2
    for name in names:
        assert same_bits(H[name], F[name][::2, :17, :17]), name
        assert same_bits(K[name][0], F[name][0, :17, :17]), name
    # one window alone
    k = nwin - 1
    n1, one = wc(big[:17, k * step:k * step + W], W, measures=names)
    assert n1 == 1
    for name in names:
        assert same_bits(one[name][0], F[name][k, :17, :17]), name


def held(nwin, W, step, at):
    k = np.arange(nwin)
    return (k * step <= at) & (at < k * step + W)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("W,step", [(250, 125), (BLOCK + 1, 2500)])
def test_a_non_finite_sample_stays_in_its_row_and_column(wc, W, step, bad):
    x = real(17, 100.0)
    nwin, F = device_all("real", 17, 100.0, W, step)
    y = np.array(x)
    y[2, 2600] = bad
    n2, G = wc(y, W, step, measures=REAL)
    hit = held(nwin, W, step, 2600)
    assert n2 == nwin and 0 < hit.sum() < nwin
    lost = np.zeros((nwin, 17, 17), dtype=bool)
    lost[hit, 2, :] = lost[hit, :, 2] = True
    for name in REAL:
        assert np.array_equal(np.isnan(G[name]), lost), name
        assert np.array_equal(bits(G[name])[~lost], bits(F[name])[~lost]), name


@pytest.mark.parametrize("W,step", [(250, 125), (BLOCK + 1, 2500)])
def test_a_zero_amplitude_sample_stays_in_its_row_and_column(wc, W, step):
    z = analytic(17, W)
    nwin, F = device_all("complex", 17, 0.0, W, step)
    y = np.array(z)
    y[2, 2600] = 0.0
    n2, G = wc(y, W, step, measures=COMPLEX)
    hit = held(nwin, W, step, 2600)
    lost = np.zeros((nwin, 17, 17), dtype=bool)
    lost[hit, 2, :] = lost[hit, :, 2] = True
    for name in COMPLEX:
        assert np.array_equal(np.isnan(G[name]), lost), name
        assert np.array_equal(bits(G[name])[~lost], bits(F[name])[~lost]), name
    y[2, 2600] = np.nan
    n2, G = wc(y, W, step, measures=COMPLEX)
    for name in COMPLEX:
        assert np.array_equal(np.isnan(G[name]), lost), name
        assert np.array_equal(bits(G[name])[~lost], bits(F[name])[~lost]), name


def test_a_constant_channel(wc):
    x = real(17, 100.0)
    nwin, F = device_all("real", 17, 100.0, 250, 125)
    y = np.array(x)
    y[2] = 7.5
    n2, G = wc(y, 250, 125, measures=REAL)
    row = np.zeros((17, 17), dtype=bool)
    row[2, :] = row[:, 2] = True
    assert np.all(G["cov"][:, row] == 0.0)
    assert np.array_equal(np.isnan(G["corr"]), np.broadcast_to(row, (nwin, 17, 17)))
    for name in REAL:
        assert np.array_equal(bits(G[name])[:, ~row], bits(F[name])[:, ~row]), name


def test_kinds_and_fixed_points(wc):
    import torch
    for x, names in ((real(3), REAL), (analytic(3, 250), COMPLEX)):
        nwin, M = wc(x, 250, 125, measures=names)
        t = torch.from_numpy(np.array(x)).cuda()
        n2, T = wc(t, 250, 125, measures=names)
        assert n2 == nwin == (N - 250) // 125 + 1
        for name in names:
            assert isinstance(M[name], np.ndarray) and M[name].dtype == np.float64 and M[name].shape == (nwin, 3, 3)
            assert isinstance(T[name], torch.Tensor) and T[name].device == t.device
            assert T[name].dtype == torch.float64 and tuple(T[name].shape) == (nwin, 3, 3)
            assert same_bits(T[name], M[name]), name
            if name != "cov":
                assert np.all(np.diagonal(M[name], axis1=1, axis2=2) == (0.0 if name == "ciplv" else 1.0)), name
        n2, one = wc(t, 250, 125, measures=names[0])
        assert isinstance(one, torch.Tensor) and one.is_cuda and tuple(one.shape) == (nwin, 3, 3)


def test_a_one_window_stream_is_analytic_connectivity(wc):
    """winsize = the stream's length: aec, plv and ciplv agree with analytic_connectivity within
    the sum of the two routes' caps against the restatement."""
    from openseize_amd.experimental.coupling.connectivity import analytic_connectivity
    z = mixture(5, N)
    want, parts = analytic_measures(z)
    theirs = bounds(parts)
    _, cap = caps(z, N, N)
    nwin, M = wc(z, N, measures=COMPLEX)
    cnt, A = analytic_connectivity(z, method=COMPLEX)
    assert nwin == 1 and cnt == N
    off = ~np.eye(5, dtype=bool)
    for name in COMPLEX:
        limit = cap[name][0] + theirs[name]
        err = np.abs(M[name][0] - A[name])
        print(f"{name}: max difference {np.max(err[off]):.2e}, least limit {np.min(limit[off]):.2e}")
        assert np.all(np.isfinite(limit[off])) and np.all(err[off] <= limit[off]), name
        assert np.array_equal(np.diagonal(M[name][0]), np.diagonal(A[name])), name
        assert np.all(np.abs(M[name][0] - want[name]) <= cap[name][0]), name


def test_results_that_do_not_fit_the_device_are_refused(wc, monkeypatch):
    """CUDA-fed results stay on the device: when they cannot fit, MemoryError names the sizes before
    a kernel runs.  Host-fed results come down push by push and are not refused."""
    import torch
    x = real(3)
    t = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 1 << 40))
    with pytest.raises(MemoryError, match=r"step \(now 125; winsize 250\).*3 channels"):
        wc(t, 250, 125)
    nwin, M = wc(x, 250, 125, measures="corr")
    assert nwin == (N - 250) // 125 + 1 and same_bits(M, device_all("real", 3, 0.0, 250, 125)[1]["corr"])
