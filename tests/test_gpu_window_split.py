"""The launch split of the window family's streaming loop (``features/_stream.py`` ``_launches``):
a push whose results would exceed ``_PUSH_BYTES`` goes to the device in several launches, each on a
column range of the push's rows -- a view that starts at any 8-byte offset (16 for complex rows)
with a pitch longer than its length.  At the default bound of 1 GiB no other test splits a push;
here the bound is one byte, so every launch holds exactly one window, and the results must be the
bits of the unsplit call, whatever the source.

One bound serves ``window_features``, ``window_entropy``, ``window_quantiles`` and
``window_connectivity``: it is patched in the shared module alone, and the number of launches is
asserted, so a function that kept a bound of its own would fail here."""

from functools import lru_cache

import numpy as np
import pytest

from openseize_amd import _lib, producer

pytestmark = pytest.mark.gpu

SHAPES = [(250, 125), (67, 200), (64, 64)]       # overlap; gaps and a misaligned first sample; abutting

# function, the launch it makes (of openseize_amd._device), whether it takes complex data, arguments
CASES = {
    "features": ("window_features", "window_features", False, dict(features=tuple(_lib.WINDOW_FEATURE))),
    "entropy": ("window_entropy", "window_entropy", False, dict(measures=tuple(_lib.WINDOW_ENTROPY))),
    "quantiles": ("window_quantiles", "window_quantiles", False,
                  dict(measures=tuple(_lib.WINDOW_QUANTILE), q=(0.1, 0.5, 0.5))),
    "real pairs": ("window_connectivity", "window_pairs", False, dict(measures=("cov", "corr"))),
    "complex pairs": ("window_connectivity", "window_pairs", True, dict(measures=("aec", "plv", "ciplv"))),
}


@lru_cache(maxsize=None)
def noise(is_complex):
    """Seeded normal noise, 3 x 2000, real or complex.  Read-only."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((3, 2000))
    if is_complex:
        x = x + 1j * rng.standard_normal((3, 2000))
    x.setflags(write=False)
    return x


def bits(a):
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("W,step", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_one_window_per_launch_changes_no_bit(case, W, step, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    from openseize_amd import _device as dev
    from openseize_amd import features
    from openseize_amd.features import _stream
    function, launch, is_complex, kwargs = CASES[case]
    run = getattr(features, function)
    x = noise(is_complex)
    names = kwargs.get("features") or kwargs["measures"]

    calls = []
    inner = getattr(dev, launch)
    monkeypatch.setattr(dev, launch, lambda *a, **k: calls.append(1) or inner(*a, **k))
    nwin, whole = run(np.array(x), W, step, **kwargs)
    assert nwin == (2000 - W) // step + 1 and list(whole) == list(names)
    assert len(calls) == 1                       # the default bound: one push, one launch

    monkeypatch.setattr(_stream, "_PUSH_BYTES", 1)
    sources = {"array": lambda: np.array(x), "producer": lambda: producer(np.array(x), 251, -1),
               "CUDA tensor": lambda: torch.from_numpy(np.array(x)).cuda()}
    for label, source in sources.items():
        del calls[:]
        n2, split = run(source(), W, step, **kwargs)
        assert n2 == nwin and len(calls) == nwin, (label, n2, len(calls))
        assert list(split) == list(names)
        for name in names:
            assert (torch.is_tensor(split[name]) and split[name].is_cuda) == (label == "CUDA tensor"), (label, name)
            a, b = bits(split[name]), bits(whole[name])
            assert a.shape == b.shape and np.array_equal(a, b), (label, name)
