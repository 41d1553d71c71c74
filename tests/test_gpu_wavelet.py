"""window_wavelet on the device (K21) against ``window_wavelets``, the NumPy restatement of the
definitions (tests/test_wavelet_host.py), run in long double on the fixed inputs ``GPU_CASES``.

Bounds.  Every feature is held to 32 E[name], E the error of the float64 restatement against the
long-double one over the same inputs (``gpu_bounds`` of the host module, which asserts 0 < 32 E <=
1e-11): relative to the band's own value for ``energy``, ``mean_abs`` and ``std`` (a value that is
exactly 0, the std of a band of one coefficient, must be met exactly), absolute for ``relative``
and ``entropy``.  The band energies of the device add up to the window's to 1e-12.  No window is
left out of a comparison.

Everything else here is bit for bit: a window's result depends on W, the filter, J, ``center``,
``normalize`` and its own samples only."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

from test_gpu_features import bits, same_bits
from test_wavelet_host import DB3, GPU_CASES, NAMES, PER_BAND, error_of, gpu_bounds, gpu_reference, gpu_signal

pytestmark = pytest.mark.gpu

WIDE = _lib.WW_WIDE
# W, step, level, wavelet: one wave with W no power of two; 256 threads with a level under the filter
CUTS = [(96, 48, 4, "db4"), (WIDE + 128, 320, 7, "db6")]


@pytest.fixture(scope="module")
def ww():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd.features import window_wavelet
    return window_wavelet


@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_parity_with_the_restatement(ww, case):
    kind, C, N, W, step, level, name, center, normalize = GPU_CASES[case]
    x = gpu_signal(kind, C, N)
    ref, bounds = gpu_reference(case), gpu_bounds()
    nwin, F = ww(x, W, step, features=NAMES, wavelet=name, level=level, center=center, normalize=normalize)
    assert nwin == (N - W) // step + 1 and list(F) == list(NAMES)
    for f in NAMES:
        got, want = F[f], ref[f]
        assert got.dtype == np.float64 and got.shape == want.shape, (f, got.shape, want.shape)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), f
        err, bound = float(np.max(error_of(f, got, want))), bounds[f][1]
        print(f"{GPU_CASES[case][:6]} {f}: error {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (f, err, bound)
    # the energy identity on the device's own numbers
    for c in range(C):
        for k in range(nwin):
            w = x[c, k * step:k * step + W].astype(np.longdouble)
            want = np.sum((w - np.mean(w)) ** 2) if center else np.sum(w * w)
            got = np.sum(F["energy"][:, c, k].astype(np.longdouble))
            assert abs(got / want - 1) <= 1e-12, (c, k, float(got), float(want))
            assert abs(np.sum(F["relative"][:, c, k]) - 1) <= 1e-14
    if not isinstance(name, str):                            # the sequence is db3's values: db3's bits
        n2, G = ww(x, W, step, features=NAMES, wavelet="db3", level=level, center=center, normalize=normalize)
        assert name == DB3 and n2 == nwin
        for f in NAMES:
            assert same_bits(G[f], F[f]), f
    if normalize:                                            # the other setting moves the entropy alone
        n2, G = ww(x, W, step, features=NAMES, wavelet=name, level=level, center=center, normalize=False)
        B = F["energy"].shape[0]
        assert np.max(np.abs(G["entropy"] / np.log(B) - F["entropy"])) <= 4e-16
        for f in PER_BAND:
            assert same_bits(G[f], F[f]), f


@lru_cache(maxsize=None)
def long_signal():
    return gpu_signal("walk", 3, 2600)


@lru_cache(maxsize=None)
def device_all(W, step, level, name):
    """(nwin, all five features) of long_signal() from one array call, computed once."""
    from openseize_amd.features import window_wavelet
    return window_wavelet(long_signal(), W, step, features=NAMES, wavelet=name, level=level)


@pytest.mark.parametrize("W,step,level,name", CUTS)
def test_the_other_features_the_step_and_the_channels_change_no_bit(ww, W, step, level, name):
    x = long_signal()
    KW = dict(wavelet=name, level=level)
    nwin, F = device_all(W, step, level, name)
    assert nwin == (2600 - W) // step + 1 and list(F) == list(NAMES)
    assert F["energy"].shape == (level + 1, 3, nwin) and F["entropy"].shape == (3, nwin)
    for f in NAMES:                                          # a tuple call against each single-name call
        n2, one = ww(x, W, step, features=f, **KW)
        assert n2 == nwin and isinstance(one, np.ndarray) and same_bits(one, F[f]), f
    n2, G = ww(x, W, step, features=("std", "relative"), **KW)
    assert list(G) == ["std", "relative"] and same_bits(G["std"], F["std"]) and same_bits(G["relative"], F["relative"])
    for other in (W, W // 2, 3 * W // 2, 1):                 # another step, on the common windows
        n2, G = ww(x[:, :4 * W], W, other, features=NAMES, **KW)
        assert n2 == (4 * W - W) // other + 1
        met = 0
        for k in range(n2):
            if k * other % step == 0 and k * other // step < nwin:
                met += 1
                for f in NAMES:
                    assert same_bits(G[f][..., k], F[f][..., k * other // step]), (f, other, k)
        assert met >= 2, other
    n1, one = ww(x[1], W, step, features=NAMES, **KW)        # one channel alone, and among three
    assert n1 == nwin
    for f in NAMES:
        assert one[f].shape == F[f].shape[:-2] + (nwin,) and same_bits(one[f], F[f][..., 1, :]), f
    n2, G = ww(np.array(x), W, step, features=NAMES, **KW)   # a rerun
    for f in NAMES:
        assert same_bits(G[f], F[f]), f


@pytest.mark.parametrize("W,step,level,name", CUTS)
def test_chunking_host_or_device_and_the_launch_split_change_no_bit(ww, W, step, level, name, monkeypatch):
    import torch
    from openseize_amd import _device as dev
    from openseize_amd.features import _stream
    x = long_signal()
    KW = dict(wavelet=name, level=level, features=NAMES)
    nwin, F = device_all(W, step, level, name)
    n2, G = ww(producer(np.array(x), 251, -1), W, step, **KW)
    assert n2 == nwin
    for f in NAMES:
        assert isinstance(G[f], np.ndarray) and same_bits(G[f], F[f]), f
    xd = torch.from_numpy(np.array(x)).cuda()
    n2, G = ww(xd, W, step, chunksize=301, **KW)
    assert n2 == nwin
    for f in NAMES:
        assert G[f].is_cuda and same_bits(G[f], F[f]), f
    calls = []
    inner = dev.window_wavelet
    monkeypatch.setattr(dev, "window_wavelet", lambda *a, **k: calls.append(1) or inner(*a, **k))
    n2, G = ww(np.array(x), W, step, **KW)
    assert n2 == nwin and len(calls) == 1                    # the default bound: one push, one launch
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)
    for label, source in (("array", np.array(x)), ("producer", producer(np.array(x), 251, -1)), ("CUDA", xd)):
        del calls[:]
        n2, G = ww(source, W, step, **KW)
        assert n2 == nwin and len(calls) == nwin, (label, n2, len(calls))
        for f in NAMES:
            assert same_bits(G[f], F[f]), (label, f)


@pytest.mark.parametrize("W,step,level,name", CUTS)
def test_non_finite_samples_stay_in_their_windows(ww, W, step, level, name):
    x = long_signal()
    nwin, clean = device_all(W, step, level, name)
    y = np.array(x)
    y[1, 701] = np.nan                                       # (overlapping windows hold it)
    end = (nwin - 1) * step + W - 10                         # ten samples before the last window's end
    y[2, end:] = np.inf                                      # a run at the end
    y[0, 0] = -np.inf                                        # a window's first sample: its pivot
    n2, F = ww(producer(y, 409, -1), W, step, features=NAMES, wavelet=name, level=level)
    k = np.arange(nwin)
    hit = np.zeros((3, nwin), dtype=bool)
    hit[0] = k == 0
    hit[1] = (k * step <= 701) & (701 < k * step + W)
    hit[2] = k * step + W > end
    assert hit[1].sum() >= 2 and hit[2].sum() >= 1 and n2 == nwin
    for f in NAMES:
        assert np.array_equal(np.isnan(F[f]), np.broadcast_to(hit, F[f].shape)), f
        assert np.array_equal(bits(F[f])[..., ~hit], bits(clean[f])[..., ~hit]), f


def test_kinds_shapes_and_a_constant_window(ww):
    import torch
    x = long_signal()
    nwin, F = ww(x[0], 96, 48, features="entropy")
    assert nwin == 53 and isinstance(F, np.ndarray) and F.shape == (53,)
    nwin, F = ww(x[0], 96, 48, features="std", level=2)
    assert F.shape == (3, 53)
    W, step, level, name = CUTS[0]
    ref = device_all(W, step, level, name)[1]
    nwin, F = ww(np.ascontiguousarray(x.T), W, step, features=NAMES, wavelet=name, level=level, axis=0, chunksize=500)
    for f in NAMES:
        assert F[f].shape == ref[f].shape[:-2] + (53, 3) and same_bits(np.swapaxes(F[f], -1, -2), ref[f]), f
    nwin, F = ww(torch.from_numpy(np.array(x)).cuda(), W, step, level=level)      # the defaults: db4
    assert list(F) == ["relative", "entropy"] and all(v.is_cuda for v in F.values())
    assert tuple(F["relative"].shape) == (5, 3, 53) and tuple(F["entropy"].shape) == (3, 53)
    assert same_bits(F["relative"], ref["relative"]) and same_bits(F["entropy"], ref["entropy"])
    nwin, F = ww(torch.from_numpy(np.array(x[1])).cuda(), W, features=("mean_abs", "entropy"), level=level)
    assert nwin == 27 and F["mean_abs"].is_cuda and tuple(F["mean_abs"].shape) == (5, 27)
    assert tuple(F["entropy"].shape) == (27,)
    nwin, F = ww(producer(np.array(x), 700, -1), 1024, features=NAMES)            # a producer; the default level
    assert nwin == 2 and F["energy"].shape == (8, 3, 2) and F["entropy"].shape == (3, 2)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in F.values())
    # a constant window: centred it has no energy at all
    for W in (96, 1024):
        nwin, F = ww(np.full((2, 3 * W), 7.5), W, features=NAMES)
        assert nwin == 3
        for f in ("energy", "mean_abs", "std"):
            assert np.all(F[f] == 0), (W, f)
        assert np.all(np.isnan(F["relative"])) and np.all(np.isnan(F["entropy"]))


def test_the_launch_wrapper_checks_its_result(ww):
    import torch
    from openseize_amd import _device as dev
    x = torch.from_numpy(np.array(long_signal())).cuda()
    W, step, level, name = CUTS[0]
    nwin, ref = device_all(W, step, level, name)
    h = _lib_filter(name)
    mask = dev.name_mask(_lib.WINDOW_WAVELET, NAMES)
    planes = 4 * (level + 1) + 1
    out = torch.full((planes, 3, nwin + 2), -1.0, dtype=torch.float64, device="cuda")
    assert dev.window_wavelet(x, W, step, mask, h, level, True, True, out) == nwin
    got = out.cpu().numpy()
    assert np.all(got[:, :, nwin:] == -1.0)                  # nothing else is touched
    B = level + 1
    assert same_bits(got[:B, :, :nwin], ref["energy"]) and same_bits(got[2 * B, :, :nwin], ref["entropy"])
    assert same_bits(got[3 * B + 1:, :, :nwin], ref["std"])
    with pytest.raises(ValueError, match="contiguous"):
        dev.window_wavelet(x, W, step, mask, h, level, True, True, out[:, :, ::2])
    with pytest.raises(ValueError, match=f"contiguous float64 \\({planes}, 3"):
        dev.window_wavelet(x, W, step, mask, h, level, True, True, out[:planes - 1].contiguous())
    with pytest.raises(ValueError, match="feature mask"):
        dev.window_wavelet(x, W, step, 0, h, level, True, True, out)
    with pytest.raises(ValueError, match="feature mask"):
        dev.window_wavelet(x, W, step, 32, h, level, True, True, out)
    for bad, match in (((h[:5], level), "taps"), ((h, 13), "levels"), ((h, 6), "levels")):   # the library's own checks
        big = torch.empty((4 * 14 + 1, 3, nwin), dtype=torch.float64, device="cuda")[:4 * (bad[1] + 1) + 1]
        with pytest.raises(ValueError, match=match):
            dev.window_wavelet(x, W, step, mask, bad[0], bad[1], True, True, big)


def _lib_filter(name):
    from openseize_amd.features import wavelet_filters
    return wavelet_filters(name)[0]
