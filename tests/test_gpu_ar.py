"""window_ar on the device (K22) against ``window_ars``, the NumPy restatement of the definitions
(tests/test_ar_host.py), run in long double on the fixed inputs ``GPU_CASES``, for both methods.

Bounds.  Every measure is held to 32 E[name, method], E the error of the float64 restatement against
the long-double one over the same inputs (``gpu_bounds`` of the host module, which asserts 32 E <=
1e-10): absolute for ``coefficients`` and ``reflection``, relative to the long-double value for
``error`` and ``error_path``.  No window is left out of a comparison.

Everything else here is bit for bit: a window's result depends on W, ``method``, ``center`` and its
own samples only -- not on ``order`` either."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_ar_host import GPU_CASES, METHODS, NAMES, RELATIVE, gpu_bounds, gpu_reference, gpu_signal
from test_gpu_features import bits, same_bits

pytestmark = pytest.mark.gpu

CUTS = [(250, 125), (600, 300)]
P = 6


@pytest.fixture(scope="module")
def wa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_ar
    return window_ar


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_parity_with_the_restatement(wa, case, method):
    kind, C, N, W, step, order = GPU_CASES[case]
    x = gpu_signal(kind, C, N)
    ref, bounds = gpu_reference(case, method), gpu_bounds()
    nwin, F = wa(x, W, step, measures=NAMES, order=order, method=method)
    assert nwin == (N - W) // step + 1 and list(F) == list(NAMES)
    for name in NAMES:
        got, want = F[name], ref[name]
        assert got.dtype == np.float64 and got.shape == want.shape, (name, got.shape, want.shape)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), name
        err = np.abs(got.astype(np.longdouble) - want)
        err, bound = (err / np.abs(want) if name in RELATIVE else err), bounds[name, method][1]
        print(f"{GPU_CASES[case]} {method} {name}: error {float(err.max()):.2e}, bound {bound:.2e}")
        assert float(err.max()) <= bound, (name, float(err.max()), bound)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_identities_of_the_device_output(wa, case, method):
    kind, C, N, W, step, order = GPU_CASES[case]
    nwin, F = wa(gpu_signal(kind, C, N), W, step, measures=NAMES, order=order, method=method)
    assert np.all(np.abs(F["reflection"]) <= 1)
    assert same_bits(F["error_path"][order], F["error"])
    assert np.all(np.diff(F["error_path"], axis=0) <= 0)
    assert same_bits(F["coefficients"][order - 1], F["reflection"][order - 1])


@lru_cache(maxsize=None)
def long_signal():
    return gpu_signal("walk", 5, 2000)


@lru_cache(maxsize=None)
def device_all(W, step, method="burg", order=P):
    """(nwin, all four measures) of long_signal() from one array call, computed once."""
    from openseize_amd.features import window_ar
    return window_ar(long_signal(), W, step, measures=NAMES, order=order, method=method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("W,step", CUTS)
def test_the_other_measures_the_order_the_step_and_the_channels_change_no_bit(wa, W, step, method):
    x = long_signal()
    kw = dict(order=P, method=method)
    nwin, F = device_all(W, step, method)
    assert nwin == (2000 - W) // step + 1 and list(F) == list(NAMES)
    assert F["coefficients"].shape == (P, 5, nwin) and F["reflection"].shape == (P, 5, nwin)
    assert F["error"].shape == (5, nwin) and F["error_path"].shape == (P + 1, 5, nwin)
    for name in NAMES:                                       # a tuple call against each single-name call
        n2, one = wa(x, W, step, measures=name, **kw)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[name]), name
    n2, G = wa(x, W, step, measures=("error_path", "coefficients"), **kw)
    assert list(G) == ["error_path", "coefficients"]
    assert same_bits(G["coefficients"], F["coefficients"]) and same_bits(G["error_path"], F["error_path"])
    n2, G = device_all(W, step, method, 2 * P)               # the first planes of twice the order
    assert n2 == nwin and G["reflection"].shape == (2 * P, 5, nwin)
    assert same_bits(G["reflection"][:P], F["reflection"]) and same_bits(G["error_path"][:P + 1], F["error_path"])
    assert same_bits(G["error_path"][P], F["error"]) and not same_bits(G["coefficients"][:P], F["coefficients"])
    n2, G = wa(x, W, 2 * step, measures=NAMES, **kw)         # another step, on the common windows
    assert n2 == (2000 - W) // (2 * step) + 1
    for name in NAMES:
        assert same_bits(G[name], F[name][..., ::2][..., :n2]), name
    n1, one = wa(x[3], W, step, measures=NAMES, **kw)        # one channel alone, and among five
    assert n1 == nwin
    for name in NAMES:
        assert one[name].shape == F[name].shape[:-2] + (nwin,) and same_bits(one[name], F[name][..., 3, :]), name
    n2, G = wa(np.array(x), W, step, measures=NAMES, **kw)   # a rerun
    for name in NAMES:
        assert same_bits(G[name], F[name]), name


@pytest.mark.parametrize("W,step", CUTS)
def test_chunking_host_or_device_and_the_launch_split_change_no_bit(wa, W, step, monkeypatch):
    import torch
    from openseize_amd import _device as dev
    from openseize_amd.features import _stream
    x = long_signal()
    kw = dict(order=P, measures=NAMES)
    nwin, F = device_all(W, step)
    n2, G = wa(producer(np.array(x), 251, -1), W, step, **kw)
    assert n2 == nwin
    for name in NAMES:
        assert isinstance(G[name], np.ndarray) and same_bits(G[name], F[name]), name
    xd = torch.from_numpy(np.array(x)).cuda()
    n2, G = wa(xd, W, step, chunksize=301, **kw)
    assert n2 == nwin
    for name in NAMES:
        assert G[name].is_cuda and same_bits(G[name], F[name]), name
    calls = []
    inner = dev.window_ar
    monkeypatch.setattr(dev, "window_ar", lambda *a, **k: calls.append(1) or inner(*a, **k))
    n2, G = wa(np.array(x), W, step, **kw)
    assert n2 == nwin and len(calls) == 1                    # the default bound: one push, one launch
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)
    for label, source in (("array", np.array(x)), ("producer", producer(np.array(x), 251, -1)), ("CUDA", xd)):
        del calls[:]
        n2, G = wa(source, W, step, **kw)
        assert n2 == nwin and len(calls) == nwin, (label, n2, len(calls))
        for name in NAMES:
            assert same_bits(G[name], F[name]), (label, name)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("W,step", CUTS)
def test_non_finite_samples_stay_in_their_windows(wa, W, step, method):
    x = long_signal()
    nwin, clean = device_all(W, step, method)
    y = np.array(x)
    y[1, 701] = np.nan                                       # (overlapping windows hold it)
    end = (nwin - 1) * step + W - 10                         # ten samples before the last window's end
    y[2, end:] = np.inf                                      # a run at the end
    y[0, 0] = -np.inf                                        # a window's first sample: its pivot
    n2, F = wa(producer(y, 409, -1), W, step, measures=NAMES, order=P, method=method)
    k = np.arange(nwin)
    hit = np.zeros((5, nwin), dtype=bool)
    hit[0] = k == 0
    hit[1] = (k * step <= 701) & (701 < k * step + W)
    hit[2] = k * step + W > end
    assert hit[1].sum() >= 2 and hit[2].sum() >= 1 and n2 == nwin
    for name in NAMES:
        assert np.array_equal(np.isnan(F[name]), np.broadcast_to(hit, F[name].shape)), name
        assert np.array_equal(bits(F[name])[..., ~hit], bits(clean[name])[..., ~hit]), name


def test_kinds_and_shapes(wa):
    import torch
    x = long_signal()
    ref = device_all(250, 125)[1]
    nwin, F = wa(x[0], 250, 125, measures="reflection", order=P)
    assert nwin == 15 and isinstance(F, np.ndarray) and F.shape == (P, 15) and same_bits(F, ref["reflection"][:, 0])
    nwin, F = wa(x[0], 250, 125, measures="error", order=P)
    assert F.shape == (15,) and same_bits(F, ref["error"][0])
    nwin, F = wa(np.ascontiguousarray(x.T), 250, 125, measures=NAMES, order=P, axis=0, chunksize=500)
    for name in NAMES:
        assert F[name].shape == ref[name].shape[:-2] + (15, 5) and same_bits(np.swapaxes(F[name], -1, -2), ref[name]), name
    nwin, F = wa(torch.from_numpy(np.array(x)).cuda(), 250, 125)                 # the defaults: burg, order 8, centred
    big = device_all(250, 125, "burg", 8)[1]
    assert list(F) == ["coefficients", "error"] and all(v.is_cuda for v in F.values())
    assert tuple(F["coefficients"].shape) == (8, 5, 15) and tuple(F["error"].shape) == (5, 15)
    assert same_bits(F["coefficients"], big["coefficients"]) and same_bits(F["error"], big["error"])
    nwin, F = wa(torch.from_numpy(np.array(x[1])).cuda(), 250, measures=("error_path", "reflection"), order=P)
    assert nwin == 8 and F["error_path"].is_cuda and tuple(F["error_path"].shape) == (P + 1, 8)
    assert tuple(F["reflection"].shape) == (P, 8)
    for method in METHODS:
        # a constant window: nothing to model when centred (or all zero)
        for w, center in ((np.full((2, 300), 7.5), True), (np.zeros((2, 1200)), False)):
            nwin, F = wa(w, w.shape[1] // 3, measures=NAMES, order=4, method=method, center=center)
            assert nwin == 3 and np.all(F["error"] == 0) and np.all(F["error_path"] == 0)
            assert np.all(np.isnan(F["coefficients"])) and np.all(np.isnan(F["reflection"]))
        # not centred it is x_t = x_{t-1}: burg predicts it exactly at order 1
        nwin, F = wa(np.full((2, 300), 7.5), 100, measures=NAMES, order=4, method=method, center=False)
        assert np.all(F["error_path"][0] == 56.25)
        if method == "burg":
            assert np.all(F["reflection"][0] == -1.0) and np.all(F["error_path"][1] == 0)
            assert np.all(np.isnan(F["reflection"][1:])) and np.all(np.isnan(F["error_path"][2:]))
            assert np.all(np.isnan(F["coefficients"])) and np.all(np.isnan(F["error"]))
        else:
            assert np.all(np.isfinite(F["error_path"])) and np.all(np.abs(F["reflection"][0] + 0.99) < 1e-15)
    # the alternating window
    for W in (64, 600):
        alt = np.tile((-1.0) ** np.arange(W), (2, 2))
        nwin, F = wa(alt, W, measures=NAMES, order=4, center=False)
        assert nwin == 2 and np.all(F["reflection"][0] == 1.0) and np.all(np.isnan(F["reflection"][1:]))
        assert np.all(F["error_path"][0] == 1.0) and np.all(F["error_path"][1] == 0) and np.all(np.isnan(F["error_path"][2:]))
        assert np.all(np.isnan(F["error"])) and np.all(np.isnan(F["coefficients"]))
        nwin, k1 = wa(alt, W, measures="coefficients", order=1, center=False)
        assert np.all(k1 == 1.0)
        nwin, F = wa(alt, W, measures=NAMES, order=4, center=False, method="yule_walker")
        assert np.all(np.abs(F["reflection"][0] - (W - 1) / W) < 1e-15) and np.all(np.isfinite(F["error_path"]))


def test_the_launch_wrapper_checks_its_result(wa):
    import torch
    from openseize_amd import _device as dev
    x = torch.from_numpy(np.array(long_signal())).cuda()
    mask = dev.name_mask(_lib.WINDOW_AR, NAMES)
    planes = 3 * P + 2
    out = torch.full((planes, 5, 15 + 2), -1.0, dtype=torch.float64, device="cuda")
    assert dev.window_ar(x, 250, 125, mask, P, "burg", True, out, win0=1) == 15
    ref = device_all(250, 125)[1]
    got = out.cpu().numpy()
    assert np.all(got[:, :, 0] == -1.0) and np.all(got[:, :, 16] == -1.0)         # nothing else is touched
    assert same_bits(got[:P, :, 1:16], ref["coefficients"]) and same_bits(got[P:2 * P, :, 1:16], ref["reflection"])
    assert same_bits(got[2 * P, :, 1:16], ref["error"]) and same_bits(got[2 * P + 1:, :, 1:16], ref["error_path"])
    out = torch.full((P + 1, 5, 15), -1.0, dtype=torch.float64, device="cuda")    # two of the four
    assert dev.window_ar(x, 250, 125, dev.name_mask(_lib.WINDOW_AR, ("reflection", "error")), P, "burg", True, out) == 15
    got = out.cpu().numpy()
    assert same_bits(got[:P], ref["reflection"]) and same_bits(got[P], ref["error"])
    out = torch.full((planes, 5, 17), -1.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        dev.window_ar(x, 250, 125, mask, P, "burg", True, out[:, :, ::2])
    with pytest.raises(ValueError, match=f"contiguous float64 \\({planes}, 5"):
        dev.window_ar(x, 250, 125, mask, P, "burg", True, out[:planes - 1].contiguous())
    with pytest.raises(ValueError, match="measure mask"):
        dev.window_ar(x, 250, 125, 0, P, "burg", True, out)
    with pytest.raises(ValueError, match="measure mask"):
        dev.window_ar(x, 250, 125, 16, P, "burg", True, out)
    assert np.all(out.cpu().numpy() == -1.0)
