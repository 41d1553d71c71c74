"""window_entropy: sample and permutation entropy of every window of a stream (no counterpart in
the reference) -- the pattern counts that ``window_features``, whose thirteen features are sums
and extremes, leaves out.  Sample entropy is O(W^2) compare-and-count per window; the device kernel
of ``csrc/windowent.hip`` (K16), ``osz_window_entropy``, holds the window in LDS and gives every
measure asked from one read of the stream.  The windows, the streaming loop and the layout of the
result are those of ``features/windowed.py``.
"""

import math

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core.producer import Producer, producer
from openseize_amd.features.windowed import (_PUSH_BYTES, _advance, _is_complex, window_count,  # noqa: F401
                                             window_plan)

WINDOW_ENTROPIES = tuple(_lib.WINDOW_ENTROPY)
_SAMPLE = ("sample", "sample_a", "sample_b")


def _names(measures):
    names = (measures,) if isinstance(measures, str) or not isinstance(measures, (tuple, list)) else tuple(measures)
    bad = [f for f in names if not isinstance(f, str) or f not in WINDOW_ENTROPIES]
    if bad or not names:
        raise ValueError(f"unknown window entropy measure(s) {bad}: choose from {WINDOW_ENTROPIES}")
    return names


def _size(value, least, most, what):
    if (isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least
            or (most is not None and value > most)):
        span = f">= {least}" if most is None else f"from {least} to {most}"
        raise ValueError(f"window_entropy: {what} must be an integer {span}, got {value!r}")
    return int(value)


_COMPLEX = "window_entropy takes real data, got {}"


def window_entropy(data, winsize, step=None, measures=("sample", "permutation"), m=2, r=0.2, tolerance="std",
                   order=3, delay=1, normalize=True, axis=-1, chunksize=None):
    """Sample and permutation entropy of every window of ``winsize`` samples, ``step`` apart, per
    channel.

    ``data``, ``winsize`` = W, ``step``, ``axis`` and ``chunksize`` are those of ``window_features``:
    real one- or two-dimensional data, samples along ``axis`` -- an ndarray, a CUDA tensor or a
    producer; window k covers the samples k step .. k step + W - 1 of the stream, whatever the
    chunks are, and a trailing window the stream does not fill is dropped.  W is an integer from 4
    to ``_lib.WE_LONGEST`` (4096: the device holds a window in LDS).

    ``measures`` is one name or a tuple of names of ``WINDOW_ENTROPIES``.  With x_0 .. x_{W-1} the
    samples of one window:

    ``"sample"``       -ln(A / B), sample entropy (Richman & Moorman 2000).  The templates are
                       i = 0 .. W - m - 1, the same for both lengths; B is the number of pairs i < j
                       with max_{k < m} |x_{i+k} - x_{j+k}| <= rho and A the same with k <= m,
                       ``<=`` in float64.  rho = r std(window) (divisor W) for ``tolerance="std"``,
                       rho = r for ``tolerance="absolute"``.  ``m`` is an integer from 1 to 8, ``r``
                       a finite float >= 0.  A = 0 < B gives +inf and B = 0 NaN, as IEEE
                       arithmetic does from the definition; a constant window gives 0.
    ``"sample_a"``, ``"sample_b"``  A and B as float64, exact: what a caller pools over epochs.
    ``"permutation"``  -sum p log2 p, permutation entropy (Bandt & Pompe 2002), over log2 d! when
                       ``normalize``.  The vectors are (x_t, x_{t+tau}, .., x_{t+(d-1) tau}) for
                       t = 0 .. W - 1 - (d - 1) tau, d = ``order`` an integer from 2 to 6 and tau =
                       ``delay`` an integer >= 1; the rank of element k is #{l : x_l < x_k} +
                       #{l < k : x_l = x_k} (a tie goes to the earlier sample); p is the histogram
                       of the d! rank patterns over the number of vectors.

    Returns ``(nwin, E)``: ``nwin`` the windows per channel, E float64 with the sample axis of the
    data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for one-dimensional --
    for one name, for a tuple a dict of name -> such an array in the order asked, all from ONE
    read of the stream and bit-identical to the single-name call.  Host data gives ndarrays, CUDA
    data CUDA tensors.

    A window that holds a NaN or +-inf is NaN in every measure, the counts included.  A window's
    bits depend on W, the parameters and its own samples only: not on ``step``, the number of
    channels, the chunking, host or CUDA data, or the other measures asked (the counts are
    integers, and the sums behind the std and the entropy run in an order that is a function of W
    and ``order`` alone, without floating-point atomics).  The std comes from sums about the
    window's first sample, so an offset of the data costs no accuracy.

    Complex data, more than two dimensions, sizes that are not integers, ``winsize`` out of range,
    ``winsize < m + 2`` with a sample measure asked, ``winsize <= (order - 1) delay`` with
    ``"permutation"`` asked, ``m``, ``r``, ``order`` or ``delay`` out of range, an unknown
    ``tolerance``, an unknown or empty ``measures`` raise ``ValueError`` before the stream or the
    device is touched (a producer's complex chunks when the first one arrives); so does a stream
    shorter than ``winsize``.
    """
    names = _names(measures)
    W = _size(winsize, 4, _lib.WE_LONGEST, f"winsize (the longest window is {_lib.WE_LONGEST} samples)")
    step = W if step is None else _size(step, 1, None, "step")
    m = _size(m, 1, 8, "m")
    order = _size(order, 2, 6, "order")
    delay = _size(delay, 1, None, "delay")
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not math.isfinite(r) or r < 0:
        raise ValueError(f"window_entropy: r must be a finite float >= 0, got {r!r}")
    if not isinstance(tolerance, str) or tolerance not in _lib.WE_TOLERANCE:
        raise ValueError(f"window_entropy: unknown tolerance {tolerance!r}: choose from {tuple(_lib.WE_TOLERANCE)}")
    if W < m + 2 and any(f in _SAMPLE for f in names):
        raise ValueError(f"window_entropy: sample entropy with m = {m} needs winsize >= m + 2 = {m + 2}, got {W}")
    if W <= (order - 1) * delay and "permutation" in names:
        raise ValueError(f"window_entropy: permutation entropy with order = {order}, delay = {delay} needs winsize > "
                         f"(order - 1) delay = {(order - 1) * delay}, got {W}")
    if isinstance(data, Producer):
        pro = producer(data, data.chunksize, axis)
    else:
        if dev.is_arraylike(data) and _is_complex(data):
            raise ValueError(_COMPLEX.format(f"{data.dtype} data"))
        pro = producer(data, int(10e6) if chunksize is None else chunksize, axis)
    if not 1 <= len(pro.shape) <= 2:
        raise ValueError(f"window_entropy needs one- or two-dimensional data, got shape {tuple(pro.shape)}: "
                         "reshape the channel axes into one")
    layout = dev.Layout(pro.shape, axis)
    if pro.shape[layout.axis] < W:
        raise ValueError(f"window_entropy: the stream holds {pro.shape[layout.axis]} samples, fewer than one "
                         f"window of {W}")
    nch = layout.nch
    planes = [f for f in WINDOW_ENTROPIES if f in names]     # the planes a push writes
    mask = dev.entropy_mask(planes)
    host = dev.origin_is_host(pro)
    torch = dev.torch
    most = max(1, _PUSH_BYTES // (8 * len(planes) * nch))    # windows per launch
    parts, carry, skip, total, started = [], None, 0, 0, False
    for arr in dev.pull_resident(pro, pro):
        if _is_complex(arr):
            raise ValueError(_COMPLEX.format(f"{arr.dtype} chunks"))
        if not started:
            dev.require_gpu()
            started = True
        x2d, was_host = layout.to2d(arr)
        host = host or was_host
        have = 0 if carry is None else carry.shape[1]
        drop, nwin, keep, skip = _advance(have, skip, x2d.shape[1], W, step)
        if drop:
            x2d = x2d[:, drop:]
        if carry is not None:
            x2d = torch.cat((carry, x2d), dim=1)
        for k0 in range(0, nwin, most):
            k1 = min(k0 + most, nwin)
            out = torch.empty((len(planes), nch, k1 - k0), dtype=torch.float64, device=x2d.device)
            dev.window_entropy(x2d[:, k0 * step:(k1 - 1) * step + W], W, step, mask, m, r, tolerance, order, delay,
                               normalize, out)
            parts.append(out.cpu().numpy() if host else out)
        total += nwin
        # (a copy: a source may fill the chunk's memory again before the next push reads it)
        carry = x2d[:, x2d.shape[1] - keep:].clone() if keep else None
    if total == 0:
        raise ValueError(f"window_entropy: the stream ended before one window of {W} samples was full")
    if host:
        stacked = np.concatenate(parts, axis=2)
        shaped = [np.moveaxis(p.reshape(layout.other + (total,)), -1, layout.axis) for p in stacked]
    else:
        stacked = torch.cat(parts, dim=2)
        shaped = [layout.from2d(p, False) for p in stacked]
    out = {name: shaped[planes.index(name)] for name in names}
    return total, out[names[0]] if isinstance(measures, str) or not isinstance(measures, (tuple, list)) else out
