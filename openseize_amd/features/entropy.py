"""window_entropy: sample and permutation entropy of every window of a stream (no counterpart in
the reference) -- the pattern counts that ``window_features``, whose thirteen features are sums
and extremes, leaves out.  Sample entropy is O(W^2) compare-and-count per window; the device kernel
of ``csrc/windowent.hip`` (K16), ``osz_window_entropy``, holds the window in LDS and gives every
measure asked from one read of the stream.  The windows, the streaming loop and the layout of the
result are those of ``window_features``: ``features/_stream.py``.
"""

import math

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)

WINDOW_ENTROPIES = tuple(_lib.WINDOW_ENTROPY)
_SAMPLE = ("sample", "sample_a", "sample_b")


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
    who = "window_entropy"
    names = _stream._names(measures, WINDOW_ENTROPIES, "window entropy measure(s)")
    W = _stream._size(winsize, 4, _lib.WE_LONGEST, who, f"winsize (the longest window is {_lib.WE_LONGEST} samples)")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    m = _stream._size(m, 1, 8, who, "m")
    order = _stream._size(order, 2, 6, who, "order")
    delay = _stream._size(delay, 1, None, who, "delay")
    if not _stream._is_real(r) or not math.isfinite(r) or r < 0:
        raise ValueError(f"window_entropy: r must be a finite float >= 0, got {r!r}")
    if not isinstance(tolerance, str) or tolerance not in _lib.WE_TOLERANCE:
        raise ValueError(f"window_entropy: unknown tolerance {tolerance!r}: choose from {tuple(_lib.WE_TOLERANCE)}")
    if W < m + 2 and any(f in _SAMPLE for f in names):
        raise ValueError(f"window_entropy: sample entropy with m = {m} needs winsize >= m + 2 = {m + 2}, got {W}")
    if W <= (order - 1) * delay and "permutation" in names:
        raise ValueError(f"window_entropy: permutation entropy with order = {order}, delay = {delay} needs winsize > "
                         f"(order - 1) delay = {(order - 1) * delay}, got {W}")
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    planes = [f for f in WINDOW_ENTROPIES if f in names]     # the planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_ENTROPY, planes)
    parts, host = _stream._planes(who, pro, W, step, kind, layout, len(planes),
                                  lambda x, out: dev.window_entropy(x, W, step, mask, m, r, tolerance, order, delay, normalize, out))
    return _stream._result(parts, host, layout, measures, names, {f: (i, None) for i, f in enumerate(planes)})
