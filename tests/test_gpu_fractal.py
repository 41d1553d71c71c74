"""window_fractal on the device (K20) against ``window_fractals``, the NumPy restatement of the
definitions (tests/test_fractal_host.py), run in long double on the fixed inputs ``GPU_CASES``.

Bounds.  Every continuous measure is held to 32 E[name], E the error of the float64 restatement
against the long-double one over the same inputs (``gpu_bounds`` of the host module, which asserts
32 E <= 1e-11): absolute for ``higuchi``, ``katz`` and ``dfa``, relative to F for
``dfa_fluctuations``.  ``petrosian`` is held to 4 ulp: its count is an integer, the rest three
logarithms.  No window is left out of a comparison.

Everything else here is bit for bit: a window's result depends on W, ``kmax``, ``scales`` and its
own samples only."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_fractal_host import GPU_CASES, NAMES, SCALES_32, gpu_bounds, gpu_reference, gpu_signal
from test_gpu_features import bits, same_bits

pytestmark = pytest.mark.gpu

WIDE = _lib.WR_WIDE
CUTS = [(250, 125), (WIDE + 88, 300)]
KW = dict(kmax=6, scales=(4, 7, 16, 40, 64, 100))


@pytest.fixture(scope="module")
def wr():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_fractal
    return window_fractal


@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_parity_with_the_restatement(wr, case):
    kind, C, N, W, step, kmax, scales = GPU_CASES[case]
    x = gpu_signal(kind, C, N)
    ref, bounds = gpu_reference(case), gpu_bounds()
    names = tuple(name for name in NAMES if name in ref)
    if W < 32:                                               # the one scale that fits is refused
        assert names == NAMES[:3]
        with pytest.raises(ValueError, match="from 2 to 32"):
            wr(x, W, step, measures=NAMES, kmax=kmax, scales=(4,))
    else:
        assert names == NAMES
    nwin, F = wr(x, W, step, measures=names, kmax=kmax, scales=scales)
    assert nwin == (N - W) // step + 1 and list(F) == list(names)
    for name in names:
        got, want = F[name], ref[name]
        assert got.dtype == np.float64 and got.shape == want.shape, (name, got.shape, want.shape)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), name
        err = np.abs(got.astype(np.longdouble) - want)
        if name == "petrosian":
            err, bound = err / np.spacing(np.abs(want.astype(np.float64))), 4.0
        else:
            err, bound = (err / np.abs(want) if name == "dfa_fluctuations" else err), bounds[name][1]
        print(f"{GPU_CASES[case][:6]} {name}: error {float(err.max()):.2e}, bound {bound:.2e}")
        assert float(err.max()) <= bound, (name, float(err.max()), bound)


@lru_cache(maxsize=None)
def long_signal():
    return gpu_signal("walk", 5, 2000)


@lru_cache(maxsize=None)
def device_all(W, step):
    """(nwin, all five measures) of long_signal() from one array call, computed once."""
    from openseize_amd.features import window_fractal
    return window_fractal(long_signal(), W, step, measures=NAMES, **KW)


@pytest.mark.parametrize("W,step", CUTS)
def test_the_other_measures_the_step_and_the_channels_change_no_bit(wr, W, step):
    x = long_signal()
    nwin, F = device_all(W, step)
    assert nwin == (2000 - W) // step + 1 and list(F) == list(NAMES)
    assert F["dfa_fluctuations"].shape == (6, 5, nwin) and F["higuchi"].shape == (5, nwin)
    for name in NAMES:                                       # a tuple call against each single-name call
        n2, one = wr(x, W, step, measures=name, **KW)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    n2, G = wr(x, W, step, measures=("dfa_fluctuations", "katz"), **KW)
    assert list(G) == ["dfa_fluctuations", "katz"]
    assert same_bits(G["katz"], F["katz"]) and same_bits(G["dfa_fluctuations"], F["dfa_fluctuations"])
    n2, G = wr(x, W, 2 * step, measures=NAMES, **KW)         # another step, on the common windows
    assert n2 == (2000 - W) // (2 * step) + 1
    for name in NAMES:
        assert same_bits(G[name], F[name][..., ::2][..., :n2]), name
    n2, G = wr(x[:, :3 * W], W, measures=NAMES, **KW)        # step = W against the overlapping step
    for k in range(n2):
        if k * W % step == 0:
            for name in NAMES:
                assert same_bits(G[name][..., k], F[name][..., k * W // step]), (name, k)
    n1, one = wr(x[3], W, step, measures=NAMES, **KW)        # one channel alone, and among five
    assert n1 == nwin
    for name in NAMES:
        assert one[name].shape == F[name].shape[:-2] + (nwin,) and same_bits(one[name], F[name][..., 3, :]), name
    n2, G = wr(np.array(x), W, step, measures=NAMES, **KW)   # a rerun
    for name in NAMES:
        assert same_bits(G[name], F[name]), name


@pytest.mark.parametrize("W,step", CUTS)
def test_chunking_host_or_device_and_the_launch_split_change_no_bit(wr, W, step, monkeypatch):
    import torch
    from openseize_amd import _device as dev
    from openseize_amd.features import _stream
    x = long_signal()
    nwin, F = device_all(W, step)
    n2, G = wr(producer(np.array(x), 251, -1), W, step, measures=NAMES, **KW)
    assert n2 == nwin
    for name in NAMES:
        assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), name
    xd = torch.from_numpy(np.array(x)).cuda()
    n2, G = wr(xd, W, step, measures=NAMES, chunksize=301, **KW)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].is_cuda and same_bits(G[name], F[name]), name
    calls = []
    inner = dev.window_fractal
    monkeypatch.setattr(dev, "window_fractal", lambda *a, **k: calls.append(1) or inner(*a, **k))
    n2, G = wr(np.array(x), W, step, measures=NAMES, **KW)
    assert n2 == nwin and len(calls) == 1                    # the default bound: one push, one launch
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)
    for label, source in (("array", np.array(x)), ("producer", producer(np.array(x), 251, -1)), ("CUDA", xd)):
        del calls[:]
        n2, G = wr(source, W, step, measures=NAMES, **KW)
        assert n2 == nwin and len(calls) == nwin, (label, n2, len(calls))
        for name in NAMES:
            assert same_bits(G[name], F[name]), (label, name)


@pytest.mark.parametrize("W,step", CUTS)
def test_non_finite_samples_stay_in_their_windows(wr, W, step):
    x = long_signal()
    nwin, clean = device_all(W, step)
    y = np.array(x)
    y[1, 701] = np.nan                                       # (overlapping windows hold it)
    end = (nwin - 1) * step + W - 10                         # ten samples before the last window's end
    y[2, end:] = np.inf                                      # a run at the end
    y[0, 0] = -np.inf                                        # a window's first sample: its pivot
    n2, F = wr(producer(y, 409, -1), W, step, measures=NAMES, **KW)
    k = np.arange(nwin)
    hit = np.zeros((5, nwin), dtype=bool)
    hit[0] = k == 0
    hit[1] = (k * step <= 701) & (701 < k * step + W)
    hit[2] = k * step + W > end
    assert hit[1].sum() >= 2 and hit[2].sum() >= 1 and n2 == nwin
    for name in NAMES:
        assert np.array_equal(np.isnan(F[name]), np.broadcast_to(hit, F[name].shape)), name
        assert np.array_equal(bits(F[name])[..., ~hit], bits(clean[name])[..., ~hit]), name


def test_kinds_and_shapes(wr):
    import torch
    x = long_signal()
    nwin, F = wr(x[0], 250, 125, measures="higuchi")
    assert nwin == 15 and isinstance(F, np.ndarray) and F.shape == (15,)
    nwin, F = wr(x[0], 250, 125, measures="dfa_fluctuations", scales=SCALES_32[:20])
    assert F.shape == (20, 15)
    nwin, F = wr(np.ascontiguousarray(x.T), 250, 125, measures=NAMES, axis=0, chunksize=500, **KW)
    ref = device_all(250, 125)[1]
    for name in NAMES:
        assert F[name].shape == ref[name].shape[:-2] + (15, 5) and same_bits(np.swapaxes(F[name], -1, -2), ref[name]), name
    nwin, F = wr(torch.from_numpy(np.array(x)).cuda(), 250, 125, **KW)           # the defaults
    assert list(F) == ["higuchi", "dfa"] and all(v.is_cuda and tuple(v.shape) == (5, 15) for v in F.values())
    assert same_bits(F["higuchi"], ref["higuchi"]) and same_bits(F["dfa"], ref["dfa"])
    nwin, F = wr(torch.from_numpy(np.array(x[1])).cuda(), 250, measures=("dfa_fluctuations", "petrosian"), **KW)
    assert nwin == 8 and F["dfa_fluctuations"].is_cuda and tuple(F["dfa_fluctuations"].shape) == (6, 8)
    assert tuple(F["petrosian"].shape) == (8,)
    # a constant window
    nwin, F = wr(np.full((2, 300), 7.5), 100, measures=NAMES)
    assert nwin == 3 and np.all(np.isnan(F["katz"])) and np.all(np.isnan(F["higuchi"])) and np.all(np.isnan(F["dfa"]))
    assert np.all(F["dfa_fluctuations"] == 0) and np.all(F["petrosian"] == 1.0)


def test_the_launch_wrapper_checks_its_result(wr):
    import torch
    from openseize_amd import _device as dev
    x = torch.from_numpy(np.array(long_signal())).cuda()
    mask = dev.name_mask(_lib.WINDOW_FRACTAL, NAMES)
    out = torch.full((4 + 6, 5, 15 + 2), -1.0, dtype=torch.float64, device="cuda")
    assert dev.window_fractal(x, 250, 125, mask, 6, KW["scales"], out, win0=1) == 15
    ref = device_all(250, 125)[1]
    got = out.cpu().numpy()
    assert np.all(got[:, :, 0] == -1.0) and np.all(got[:, :, 16] == -1.0)         # nothing else is touched
    assert same_bits(got[0, :, 1:16], ref["higuchi"]) and same_bits(got[4:, :, 1:16], ref["dfa_fluctuations"])
    with pytest.raises(ValueError, match="contiguous"):
        dev.window_fractal(x, 250, 125, mask, 6, KW["scales"], out[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous float64 \\(10, 5"):
        dev.window_fractal(x, 250, 125, mask, 6, KW["scales"], out[:9].contiguous())
    with pytest.raises(ValueError, match="measure mask"):
        dev.window_fractal(x, 250, 125, 0, 6, KW["scales"], out)
    with pytest.raises(ValueError, match="measure mask"):
        dev.window_fractal(x, 250, 125, 32, 6, KW["scales"], out)
