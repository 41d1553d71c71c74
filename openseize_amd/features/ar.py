"""window_ar: the autoregressive model of every window of a stream (no counterpart in the
reference) -- its coefficients, its reflection coefficients and its innovation variance, by Burg's
recursion or from the biased autocorrelation (Yule-Walker): the parametric member of the family
beside ``window_features`` (moments), ``window_entropy`` (pattern counts), ``window_quantiles``
(order statistics), ``window_spectral`` (periodogram summaries), ``window_fractal`` (scaling
exponents) and ``window_wavelet`` (sub-bands).  Burg is ``order`` sequential passes over the
prediction errors of a window; the device kernel of ``csrc/windowar.hip`` (K22), ``osz_window_ar``,
keeps the errors in registers and gives every measure asked from one read of the stream.  The
windows, the streaming loop and the layout of the result are those of ``window_features``:
``features/_stream.py``.
"""

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)

WINDOW_ARS = tuple(_lib.WINDOW_AR)
AR_METHODS = tuple(_lib.AR_METHOD)


def window_ar(data, winsize, step=None, measures=("coefficients", "error"), order=8, method="burg", center=True,
              axis=-1, chunksize=None):
    """The autoregressive model of ``order`` = p of every window of ``winsize`` samples, ``step``
    apart, per channel.

    ``data``, ``winsize`` = W, ``step``, ``axis`` and ``chunksize`` are those of ``window_fractal``:
    real one- or two-dimensional data, samples along ``axis`` -- an ndarray, a CUDA tensor or a
    producer; window k covers the samples k step .. k step + W - 1 of the stream, whatever the
    chunks are, and a trailing window the stream does not fill is dropped.  W is an integer from 16
    to ``_lib.AR_LONGEST`` (4096: the device holds a window on chip), ``order`` an integer from 1 to
    ``_lib.AR_ORDER`` = 32, and ``winsize >= 4 * order`` is required.

    With x_0 .. x_{W-1} the samples of one window, minus their mean when ``center`` is true (the
    mean comes from sums about the window's first sample, so an offset of the data costs no
    accuracy), the model is x_t + sum_{k=1..p} a_k x_{t-k} = e_t -- the signs of ``arburg``: the
    process x_t = 0.9 x_{t-1} + e_t has a_1 = -0.9.  Everything is float64.

    ``method="burg"``         Burg (1968).  f_t = b_t = x_t and E_0 = (1 / W) sum x_t^2.  For m = 1 ..
                              p: num = sum_{t=m}^{W-1} f_t b_{t-1}, den = sum_{t=m}^{W-1} (f_t^2 +
                              b_{t-1}^2) -- the direct sum, not its downdating recursion -- and k_m =
                              -2 num / den; then for t = m .. W - 1, both from the old values, f_t <-
                              f_t + k_m b_{t-1} and b_t <- b_{t-1} + k_m f_t.
    ``method="yule_walker"``  r_j = (1 / W) sum_{t=0}^{W-1-j} x_t x_{t+j}, j = 0 .. p -- the biased
                              estimate, which keeps |k| < 1 -- E_0 = r_0 and k_m = -(r_m +
                              sum_{j=1}^{m-1} a^(m-1)_j r_{m-j}) / E_{m-1}.
    Both take the Levinson step a^(m)_j = a^(m-1)_j + k_m a^(m-1)_{m-j} for j < m, a^(m)_m = k_m and
    E_m = E_{m-1} (1 - k_m^2).

    ``measures`` is one name or a tuple of names of ``WINDOW_ARS``:

    ``"coefficients"``  a^(p)_1 .. a^(p)_p, with a leading axis: (p, C, nwin) for (C, N) data.
    ``"reflection"``    k_1 .. k_p: (p, C, nwin).
    ``"error"``         E_p, the innovation variance: (C, nwin).
    ``"error_path"``    E_0 .. E_p, what AIC or FPE order selection reads: (p + 1, C, nwin).

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64 with the sample axis of the
    data replaced by the window axis (one-dimensional data has no C axis) for one name, for a
    tuple a dict of name -> such an array in the order asked, all from ONE read of the stream and
    bit-identical to the single-name call.  Host data gives ndarrays, CUDA data CUDA tensors.

    A window that holds a NaN or +-inf is NaN in every plane, and no other window moves a bit.  A
    window with E_0 = 0 (constant when centred, all-zero otherwise) has ``"error"`` 0 and
    ``"error_path"`` 0; its ``"coefficients"`` and ``"reflection"`` are NaN.  An E_{m-1} that is 0
    (or a den that is 0) at a later order -- a window a model of order m - 1 predicts exactly --
    makes k_m and everything of the orders from m on NaN, the planes m .. p of ``"error_path"``
    included, and moves nothing before it.  A window's bits depend on W, ``method``, ``center`` and
    its own samples only: not on ``step``, the number of channels, the chunking, host or CUDA data,
    or the other measures asked.  Nor do they depend on ``order``: ``"reflection"[m - 1]`` = k_m and
    ``"error_path"[m]`` for m <= p' are the same bits with ``order=p'`` as with ``order=p > p'``
    (every sum runs in an order that is a function of (W, m) or (W, j) alone, without
    floating-point atomics).

    Complex data, more than two dimensions, sizes that are not integers, ``winsize`` or ``order``
    out of range, ``winsize < 4 * order``, an unknown ``method``, an unknown or empty ``measures``
    raise ``ValueError`` before the stream or the device is touched (a producer's complex chunks
    when the first one arrives); so does a stream shorter than ``winsize``.
    """
    who = "window_ar"
    names = _stream._names(measures, WINDOW_ARS, "window AR measure(s)")
    W = _stream._size(winsize, 16, _lib.AR_LONGEST, who, f"winsize (the longest window is {_lib.AR_LONGEST} samples)")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    p = _stream._size(order, 1, _lib.AR_ORDER, who, "order")
    if W < 4 * p:
        raise ValueError(f"window_ar: order = {p} needs winsize >= 4 order = {4 * p}, got {W}")
    if not isinstance(method, str) or method not in AR_METHODS:
        raise ValueError(f"window_ar: unknown method {method!r}: choose from {AR_METHODS}")
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    stacked = {"coefficients": p, "reflection": p, "error": None, "error_path": p + 1}
    where, count = {}, 0                                     # the planes a launch writes
    for f in WINDOW_ARS:
        if f in names:
            where[f] = (count, stacked[f])
            count += stacked[f] or 1
    mask = dev.name_mask(_lib.WINDOW_AR, where)
    parts, host = _stream._planes(who, pro, W, step, kind, layout, count,
                                  lambda x, out: dev.window_ar(x, W, step, mask, p, method, center, out))
    return _stream._result(parts, host, layout, measures, names, where)
