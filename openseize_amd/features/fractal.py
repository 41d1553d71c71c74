"""window_fractal: Higuchi, Katz and Petrosian fractal dimensions and the exponent of detrended
fluctuation analysis of every window of a stream (no counterpart in the reference) -- the scaling
family that ``window_features`` (sums and extremes), ``window_entropy`` (pattern counts),
``window_quantiles`` (order statistics) and ``window_spectral`` (periodogram summaries) leave out.
Higuchi is W kmax strided differences per window, DFA a prefix sum and many small least-squares
fits; the device kernel of ``csrc/windowfrac.hip`` (K20), ``osz_window_fractal``, holds the window
in LDS and gives every measure asked from one read of the stream.  The windows, the streaming loop
and the layout of the result are those of ``window_features``: ``features/_stream.py``.
"""

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)

WINDOW_FRACTALS = tuple(_lib.WINDOW_FRACTAL)
_DFA = ("dfa", "dfa_fluctuations")


def dfa_scales(winsize, count=16):
    """The default scales of ``"dfa"`` for windows of ``winsize`` samples: the distinct values of
    floor(geomspace(4, winsize // 4, count) + 0.5), a strictly increasing tuple of ints from 4 to
    ``winsize // 4``.  ``winsize`` is an integer >= 32 (below that fewer than two scales differ by
    a factor worth a fit), ``count`` an integer from 2 to ``_lib.WR_SCALES``."""
    W = _stream._size(winsize, 32, None, "dfa_scales", "winsize")
    count = _stream._size(count, 2, _lib.WR_SCALES, "dfa_scales", "count")
    return tuple(int(n) for n in np.unique(np.floor(np.geomspace(4, W // 4, count) + 0.5).astype(np.int64)))


def _scales(scales, W):
    """The scales of a DFA measure as a tuple of ints, checked."""
    who = "window_fractal"
    if scales is None:
        if W < 32:
            raise ValueError(f"{who}: scales=None needs winsize >= 32 (dfa_scales), got {W}: give scales")
        return dfa_scales(W)
    if isinstance(scales, (str, bytes)) or not hasattr(scales, "__len__") or not hasattr(scales, "__iter__"):
        raise ValueError(f"{who}: scales must be a sequence of integers or None, got {scales!r}")
    if not 2 <= len(scales) <= _lib.WR_SCALES:
        raise ValueError(f"{who}: scales must hold from 2 to {_lib.WR_SCALES} box sizes, got {len(scales)}")
    ns = tuple(_stream._size(n, 4, W // 2, who, f"a scale (winsize // 2 is {W // 2})") for n in scales)
    if any(b <= a for a, b in zip(ns, ns[1:])):
        raise ValueError(f"{who}: scales must be strictly increasing, got {ns}")
    return ns


def window_fractal(data, winsize, step=None, measures=("higuchi", "dfa"), kmax=8, scales=None, axis=-1,
                   chunksize=None):
    """Fractal dimensions and the DFA exponent of every window of ``winsize`` samples, ``step``
    apart, per channel.

    ``data``, ``winsize`` = W, ``step``, ``axis`` and ``chunksize`` are those of ``window_entropy``:
    real one- or two-dimensional data, samples along ``axis`` -- an ndarray, a CUDA tensor or a
    producer; window k covers the samples k step .. k step + W - 1 of the stream, whatever the
    chunks are, and a trailing window the stream does not fill is dropped.  W is an integer from 8
    to ``_lib.WR_LONGEST`` (4096: the device holds a window in LDS).

    ``measures`` is one name or a tuple of names of ``WINDOW_FRACTALS``.  With x_0 .. x_{W-1} the
    samples of one window, everything in float64:

    ``"higuchi"``    Higuchi (1988).  For k = 1 .. ``kmax`` and m = 0 .. k - 1, n_mk =
                     floor((W - 1 - m) / k) and L_m(k) = (sum_{i=1..n_mk} |x_{m+ik} - x_{m+(i-1)k}|)
                     (W - 1) / (n_mk k) / k; L(k) is the mean of L_m(k) over m.  The result is the
                     least-squares slope of v = ln L(k) on u = ln(1 / k), the abscissa centred:
                     sum (u - mean u) v / sum (u - mean u)^2.  ``kmax`` is an integer from 2 to
                     ``_lib.WR_KMAX`` = 64, and ``winsize >= 2 * kmax`` is required.  An L(k) = 0
                     gives NaN.
    ``"katz"``       Katz (1988).  L = sum |x_{i+1} - x_i|, d = max_i |x_i - x_0|, n = W - 1: ln n /
                     (ln n + ln(d / L)).  A constant window is NaN.
    ``"petrosian"``  Petrosian (1995).  N is the number of i with d_i = x_{i+1} - x_i and d_{i+1} of
                     strictly opposite sign (a zero difference is no sign): log10 W / (log10 W +
                     log10(W / (W + 0.4 N))).
    ``"dfa"``        Detrended fluctuation analysis (Peng et al. 1994).  y_t = sum_{j<=t} (x_j -
                     mean) is the profile.  For each n of ``scales`` = n_1 < .. < n_S take the
                     floor(W / n) boxes of n samples counted from the window's first sample (the
                     tail is dropped) and fit in each a straight line to y by least squares; F(n) =
                     sqrt(mean over all boxed samples of the squared residual).  The result is the
                     least-squares slope of ln F(n) on ln n, centred as above.  An F(n) = 0 gives
                     NaN.
    ``"dfa_fluctuations"``  the F(n) themselves, with a leading axis over the scales:
                     (S, C, nwin) for (C, N) data.

    ``scales`` is a strictly increasing sequence of 2 to ``_lib.WR_SCALES`` = 32 integers, each 4 <=
    n <= W // 2; ``None`` means ``dfa_scales(W)`` and needs W >= 32.  It is read only when a DFA
    measure is asked.

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64 with the sample axis of the
    data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for one-dimensional --
    for one name, for a tuple a dict of name -> such an array in the order asked, all from ONE
    read of the stream and bit-identical to the single-name call.  Host data gives ndarrays, CUDA
    data CUDA tensors.

    A window that holds a NaN or +-inf is NaN in every measure.  A window's bits depend on W,
    ``kmax``, ``scales`` and its own samples only: not on ``step``, the number of channels, the
    chunking, host or CUDA data, or the other measures asked (every sum runs in an order that is a
    function of (W, k) or (W, n) alone, without floating-point atomics).  The mean comes from sums
    about the window's first sample and the sums of a box run about the box's first profile value,
    so an offset of the data or a wandering profile costs no accuracy.

    Complex data, more than two dimensions, sizes that are not integers, ``winsize`` or ``kmax``
    out of range, ``winsize < 2 * kmax`` with ``"higuchi"`` asked, ``scales`` that are not
    integers, not increasing, too many or too large, ``scales=None`` with W < 32 and a DFA measure
    asked, an unknown or empty ``measures`` raise ``ValueError`` before the stream or the device is
    touched (a producer's complex chunks when the first one arrives); so does a stream shorter
    than ``winsize``.
    """
    who = "window_fractal"
    names = _stream._names(measures, WINDOW_FRACTALS, "window fractal measure(s)")
    W = _stream._size(winsize, 8, _lib.WR_LONGEST, who, f"winsize (the longest window is {_lib.WR_LONGEST} samples)")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    kmax = _stream._size(kmax, 2, _lib.WR_KMAX, who, "kmax")
    if W < 2 * kmax and "higuchi" in names:
        raise ValueError(f"window_fractal: higuchi with kmax = {kmax} needs winsize >= 2 kmax = {2 * kmax}, got {W}")
    ns = _scales(scales, W) if any(f in _DFA for f in names) else ()
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    where, count = {}, 0                                     # the planes a launch writes
    for f in WINDOW_FRACTALS:
        if f in names:
            where[f] = (count, len(ns)) if f == "dfa_fluctuations" else (count, None)
            count += len(ns) if f == "dfa_fluctuations" else 1
    mask = dev.name_mask(_lib.WINDOW_FRACTAL, where)
    parts, host = _stream._planes(who, pro, W, step, kind, layout, count,
                                  lambda x, out: dev.window_fractal(x, W, step, mask, kmax, ns, out))
    return _stream._result(parts, host, layout, measures, names, where)
