"""window_quantiles: median, median absolute deviation and quantiles of every window of a stream
(no counterpart in the reference) -- the order statistics that ``window_features`` (sums and
extremes) and ``window_entropy`` (pattern counts) leave out: a robust baseline and scale, a
quantile envelope, the interquartile range.  The device kernel of ``csrc/windowquant.hip`` (K17),
``osz_window_quantiles``, sorts each window on chip from one read of the stream and gives every
measure asked.  The windows, the streaming loop and the layout of the result are those of
``window_features``: ``features/_stream.py``.
"""

import math

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)
from openseize_amd.features._stream import _is_real

WINDOW_QUANTILES = tuple(_lib.WINDOW_QUANTILE)


def _probabilities(q):
    """(values, scalar) of ``q``: a float, or a sequence of 1 to _lib.WQ_QMOST floats in [0, 1]."""
    scalar = _is_real(q)
    if not scalar and not isinstance(q, (tuple, list, np.ndarray)):
        raise ValueError(f"window_quantiles: q must be a float or a sequence of floats in [0, 1], got {q!r}")
    values = [q] if scalar else list(np.asarray(q).tolist() if isinstance(q, np.ndarray) else q)
    if not 1 <= len(values) <= _lib.WQ_QMOST:
        raise ValueError(f"window_quantiles: q must hold from 1 to {_lib.WQ_QMOST} values, got {len(values)}")
    for p in values:
        if not _is_real(p) or not math.isfinite(p) or not 0.0 <= p <= 1.0:
            raise ValueError(f"window_quantiles: every q must be a finite float in [0, 1], got {p!r}")
    return [float(p) for p in values], scalar


def window_quantiles(data, winsize, step=None, measures=("median", "mad"), q=(0.25, 0.75), axis=-1, chunksize=None):
    """Median, median absolute deviation and quantiles of every window of ``winsize`` samples,
    ``step`` apart, per channel.

    ``data``, ``winsize`` = W, ``step``, ``axis`` and ``chunksize`` are those of ``window_entropy``:
    real one- or two-dimensional data, samples along ``axis`` -- an ndarray, a CUDA tensor or a
    producer; window k covers the samples k step .. k step + W - 1 of the stream, whatever the
    chunks are, and a trailing window the stream does not fill is dropped.  W is an integer from 4
    to ``_lib.WQ_LONGEST`` (4096: the device sorts a window on chip).

    ``measures`` is one name or a tuple of names of ``WINDOW_QUANTILES``.  With s_0 <= .. <=
    s_{W-1} the samples of one window in ascending total order (-0.0 before +0.0: the order is a
    function of the bits):

    ``"median"``    (s_{(W-1)//2} + s_{W//2}) / 2, one addition and one division in float64.
    ``"quantile"``  for each p of ``q`` Hyndman & Fan's type 7 as ``numpy.quantile`` computes its
                    ``"linear"`` method: h = p (W - 1), lo = floor(h), g = h - lo, hi = min(lo + 1,
                    W - 1), a = s_lo, b = s_hi; a where a == b, else with d = b - a the value
                    a + d g for g < 0.5 and b - d (1 - g) otherwise; every operation one IEEE
                    operation.  ``q`` is a float or a sequence of 1 to ``_lib.WQ_QMOST`` (16)
                    floats in [0, 1], in any order; duplicates give duplicate planes.  It is read
                    only when ``"quantile"`` is asked.
    ``"mad"``       the median, by the rule above, of |x_t - median| over the window: unscaled, the
                    caller multiplies by 1.4826 for a normal standard deviation.

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64 with the sample axis of the
    data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for one-dimensional --
    for one name, for a tuple a dict of name -> such an array in the order asked, all from ONE
    read of the stream and bit-identical to the single-name call.  ``"quantile"`` with a sequence
    ``q`` has one more leading axis of len(q), with a scalar ``q`` none.  Host data gives ndarrays,
    CUDA data CUDA tensors.

    A window that holds a NaN is NaN in every measure.  +-inf are ordinary values of the sort, and
    the measures are what IEEE arithmetic gives from the definitions: ``mad`` is NaN where the
    median is infinite (inf - inf), and a quantile between an infinite and a finite sample is NaN
    where the rule multiplies inf by 0 or subtracts inf from inf (q = 0 of a window whose least
    sample alone is -inf: -inf + inf 0).  A window's bits depend on W, ``q`` and its own samples only:
    not on ``step``, the number of channels, the chunking, host or CUDA data, the other measures
    or the other values of ``q`` asked (the sort compares integer keys, and each measure is a
    selection followed by at most four IEEE operations).

    Complex data, more than two dimensions, sizes that are not integers, ``winsize`` out of range,
    ``step < 1``, an unknown or empty ``measures``, and -- when ``"quantile"`` is asked -- a ``q``
    that is empty, longer than 16, not finite or outside [0, 1] raise ``ValueError`` before the
    stream or the device is touched (a producer's complex chunks when the first one arrives); so
    does a stream shorter than ``winsize``.
    """
    who = "window_quantiles"
    names = _stream._names(measures, WINDOW_QUANTILES, "window quantile measure(s)")
    W = _stream._size(winsize, 4, _lib.WQ_LONGEST, who, f"winsize (the longest window is {_lib.WQ_LONGEST} samples)")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    qs, scalar = _probabilities(q) if "quantile" in names else ([], True)
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    present = [f for f in WINDOW_QUANTILES if f in names]    # the measures a launch writes, in the kernel's order
    mask = dev.name_mask(_lib.WINDOW_QUANTILE, present)
    width = {f: len(qs) if f == "quantile" else 1 for f in present}
    where = {f: (sum(width[g] for g in present[:i]), None if f != "quantile" or scalar else len(qs))
             for i, f in enumerate(present)}
    nplanes = sum(width.values())
    parts, host = _stream._planes(who, pro, W, step, kind, layout, nplanes,
                                  lambda x, out: dev.window_quantiles(x, W, step, mask, qs, out))
    return _stream._result(parts, host, layout, measures, names, where)
