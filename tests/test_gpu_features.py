"""window_features on the device (K15) against ``window_measures``, the NumPy restatement of the
thirteen definitions (tests/test_features_host.py), evaluated in long double.

Bounds.  ``min``, ``max``, ``ptp`` and ``zero_crossings`` are exact.  Every other feature is within
RTOL = 1e-9 (the suite's cap, tests/test_gpu_parity.py) times a scale: mean |x| for ``mean``,
max(1, |skew|) for ``skew`` (near 0 for noise), mean(x_t^2 + |x_{t-1} x_{t+1}|) for ``teager`` (a
difference of products), the value itself for the rest.  On exactly these inputs the float64
restatement stays within 2e-12 of the long-double one under these scales (worst: ``complexity``
at W = 4) and a pivot-shifted one-pass scheme, what the kernel does, within 3e-13: the cap leaves
three orders of margin, a failure is a bug and not rounding.

Everything else here is bit for bit: a window's result depends on W and its own samples only."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer
from openseize_amd.core.producer import Producer

from test_features_host import EXACT, NAMES, scales, window_measures

pytestmark = pytest.mark.gpu

RTOL = 1e-9
LONG = _lib.WF_LONG
SHAPES = [(250, 125), (4, 1), (67, 200), (1000, 333), (4096, 4096), (63, 63), (64, 64), (65, 65),
          (LONG - 1, 2500), (LONG, 2500), (LONG + 1, 2500)]
CUTS = [(250, 125), (67, 200), (LONG + 1, 2500)]


@pytest.fixture(scope="module")
def wf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_features
    return window_features


@lru_cache(maxsize=None)
def noise(offset=0.0):
    """Seeded normal noise, 3 x 20 000, plus ``offset`` standard deviations.  Read-only."""
    x = np.random.default_rng(20).standard_normal((3, 20000)) + offset
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def device_all(offset, W, step):
    """(nwin, all thirteen features) of noise(offset) from one array call, computed once."""
    from openseize_amd.features import window_features
    return window_features(noise(offset), W, step, features=NAMES)


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_close(got, x, W, step, where=None):
    ref, sc = scales(x, W, step)
    for name in NAMES:
        g, r = got[name], ref[name]
        assert g.shape == r.shape and g.dtype == np.float64, (name, g.shape, r.shape)
        if where is not None:
            g, r, s = g[where], r[where], sc[name][where]
        else:
            s = sc[name]
        if name in EXACT:
            assert np.array_equal(g, r.astype(np.float64)), name
        else:
            err = float(np.max(np.abs(g - r) / s))
            print(f"W={W} step={step} {name}: {err:.2e}")
            assert err < RTOL, (name, W, step, err)


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("W,step", SHAPES)
def test_parity_with_the_restatement(wf, W, step, offset):
    x = noise(offset)
    nwin, F = device_all(offset, W, step)
    assert nwin == (20000 - W) // step + 1 and list(F) == list(NAMES)
    assert_close(F, x, W, step)


@pytest.mark.parametrize("W,step", CUTS)
def test_chunking_host_or_device_and_axis_change_no_bit(wf, W, step):
    import torch
    x = noise(100.0)
    nwin, F = device_all(100.0, W, step)
    for cs in (7, 249, 250, 251, 4099):
        n2, G = wf(producer(np.array(x), cs, -1), W, step, features=NAMES)
        assert n2 == nwin
        for name in NAMES:
            assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), (cs, name)
    n2, G = wf(torch.from_numpy(np.array(x)).cuda(), W, step, features=NAMES, chunksize=3001)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].is_cuda and same_bits(G[name], F[name]), name
    n2, G = wf(np.ascontiguousarray(x.T), W, step, features=NAMES, axis=0, chunksize=5000)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].shape == (nwin, 3) and same_bits(G[name].T, F[name]), name


def test_a_single_name_is_its_entry_of_the_whole(wf):
    x = noise()
    nwin, F = device_all(0.0, 250, 125)
    for name in NAMES:
        n2, one = wf(x, 250, 125, features=name)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    n2, G = wf(x, 250, 125, features=("teager", "mean"))
    assert list(G) == ["teager", "mean"] and same_bits(G["teager"], F["teager"]) and same_bits(G["mean"], F["mean"])
    n2, G = wf(x, 250)                                       # the defaults: step = winsize, two features
    assert n2 == 80 and list(G) == ["line_length", "var"]
    assert same_bits(G["var"], F["var"][:, ::2])


@pytest.mark.parametrize("W,step", [(250, 125), (67, 200), (LONG + 1, 2500)])
def test_a_window_depends_on_its_own_samples_only(wf, W, step):
    x = noise(100.0)
    nwin, F = device_all(100.0, W, step)
    for k in sorted({1, nwin // 2, nwin - 1}):
        n1, G = wf(x[:, k * step:k * step + W], W, features=NAMES)
        assert n1 == 1
        for name in NAMES:
            assert same_bits(G[name][:, 0], F[name][:, k]), (name, k)
    # one row alone and 257 copies of it
    n1, one = wf(x[1], W, step, features=NAMES)
    n257, many = wf(np.tile(x[1], (257, 1)), W, step, features=NAMES)
    assert n1 == n257 == nwin
    for name in NAMES:
        assert one[name].shape == (nwin,) and same_bits(one[name], F[name][1]), name
        assert many[name].shape == (257, nwin)
        assert np.array_equal(bits(many[name]), np.broadcast_to(bits(F[name][1]), (257, nwin))), name


def test_more_windows_than_a_grid_dimension(wf):
    x = np.random.default_rng(21).standard_normal((1, 70000))
    nwin, F = wf(x, 4, 1, features=NAMES)
    assert nwin == 69997 > 65535
    assert_close(F, x, 4, 1)


def test_non_finite_samples_stay_in_their_windows(wf):
    W, step = 250, 125
    x = noise()
    nwin, clean = device_all(0.0, W, step)
    y = np.array(x)
    y[1, 7013] = np.nan
    y[2, 19000:] = np.nan
    n2, F = wf(producer(y, 4099, -1), W, step, features=NAMES)
    k = np.arange(nwin)
    hit = np.zeros((3, nwin), dtype=bool)
    hit[1] = (k * step <= 7013) & (7013 < k * step + W)
    hit[2] = k * step + W > 19000
    assert hit[1].sum() == 2 and hit[2].sum() > 2
    for name in NAMES:
        assert np.array_equal(np.isnan(F[name]), hit), name
        assert np.array_equal(bits(F[name])[~hit], bits(clean[name])[~hit]), name
    for W, step in ((250, 125), (4, 1), (LONG, 2500)):
        z = np.array(x)
        z[0, 100] = np.inf
        z[1, 5000] = -np.inf
        z[2, 0] = np.inf                                     # a window's first sample: its pivot
        z[2, 777] = np.inf
        z[2, 800] = -np.inf
        nwin, F = wf(z, W, step, features=NAMES)
        with np.errstate(all="ignore"):
            ref = window_measures(z, W, step)
        fin = np.all(np.isfinite(z[:, np.arange(nwin)[:, None] * step + np.arange(W)[None, :]]), axis=-1)
        assert not fin.all()
        for name in NAMES:
            assert np.array_equal(F[name][~fin], ref[name][~fin], equal_nan=True), (name, W)
        _, tidy = device_all(0.0, W, step) if (W, step) in SHAPES else wf(np.array(x), W, step, features=NAMES)
        for name in NAMES:
            assert np.array_equal(bits(F[name])[fin], bits(tidy[name])[fin]), (name, W)


def test_kinds_shapes_and_counts(wf):
    import ctypes
    import torch
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.osz_window_count.restype, lib.osz_window_count.argtypes = _lib.SIGNATURES["osz_window_count"]
    x = noise()
    for W, step in ((250, 125), (67, 200), (20000, 1), (19999, 1)):
        nwin, F = wf(x, W, step, features="rms")
        assert nwin == lib.osz_window_count(20000, W, step) and isinstance(F, np.ndarray) and F.shape == (3, nwin)
        nwin, F = wf(torch.from_numpy(np.array(x[0])).cuda(), W, step, features=("rms", "ptp"))
        assert nwin == lib.osz_window_count(20000, W, step)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (nwin,) for v in F.values())
    with pytest.raises(ValueError, match="fewer than one window"):
        wf(torch.from_numpy(np.array(x)).cuda(), 20001)

    # a source that says it is longer than it is: found when the stream ends
    def short():
        yield torch.zeros((3, 90), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="before one window"):
        wf(producer(short, chunksize=50, axis=-1, shape=(3, 5000)), 100)


class Reused(Producer):
    """Chunks of a CUDA tensor, each copied into ONE reused buffer and yielded as a view of it;
    the buffer is overwritten when the stream ends (tests/test_gpu_recycled.py)."""

    @property
    def shape(self):
        return tuple(self.data.shape)

    def __iter__(self):
        import torch
        x, cs = self.data, self.chunksize
        buf = torch.empty((x.shape[0], cs), dtype=torch.float64, device="cuda")
        try:
            for start in range(0, x.shape[1], cs):
                m = min(cs, x.shape[1] - start)
                dst = buf[:, :m]
                dst.copy_(x[:, start:start + m])
                yield dst
        finally:
            buf.fill_(1e200)


@pytest.mark.parametrize("W,step", CUTS)
def test_a_source_that_recycles_its_buffer(wf, W, step):
    import torch
    x = noise(100.0)
    nwin, F = device_all(100.0, W, step)
    xd = torch.from_numpy(np.array(x)).cuda()

    def gen():
        buf = torch.empty((3, 1000), dtype=torch.float64, device="cuda")
        for start in range(0, 20000, 1000):
            buf.copy_(xd[:, start:start + 1000])
            yield buf
    for pro in (Reused(xd, 333, -1), Reused(xd, 4099, -1), producer(gen, chunksize=777, axis=-1, shape=(3, 20000))):
        n2, G = wf(pro, W, step, features=NAMES)
        assert n2 == nwin
        for name in NAMES:
            assert G[name].is_cuda and same_bits(G[name], F[name]), name
