"""window_features: time-resolved per-channel features of a stream (no counterpart in the
reference): line length, variance / RMS and the higher moments, the extremes, zero crossings, the
Hjorth parameters and the Teager energy of every window of ``winsize`` samples, ``step`` apart --
what a long recording is reduced to before anyone looks for where it changes.  All thirteen come
from one read of the data by the device kernel of ``csrc/windowfeat.hip`` (K15):
``osz_window_features``.
"""

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)

WINDOW_FEATURES = tuple(_lib.WINDOW_FEATURE)


def window_features(data, winsize, step=None, features=("line_length", "var"), axis=-1, chunksize=None):
    """Features of every window of ``winsize`` samples, ``step`` apart, per channel.

    ``data`` is real, one- or two-dimensional, samples along ``axis``: an ndarray, a CUDA tensor or
    a producer.  ``chunksize`` applies to arrays only (default ``int(10e6)``).  ``winsize`` = W is
    an integer >= 4, ``step`` an integer >= 1 that defaults to ``winsize``; ``step < W`` overlaps
    the windows, ``step > W`` leaves gaps.  Window k covers the samples k step .. k step + W - 1
    counted from the first sample of the stream, whatever the chunks are; a trailing window the
    stream does not fill is dropped.

    ``features`` is one name or a tuple of names of ``WINDOW_FEATURES``.  With x_0 .. x_{W-1} the
    samples of one window, dx_t = x_{t+1} - x_t, ddx_t = dx_{t+1} - dx_t and m_k the k-th central
    moment about the window's own mean with divisor W:

    ``"mean"``, ``"var"``, ``"rms"``    the mean, m_2 (``np.var``), sqrt(mean x^2);
    ``"skew"``, ``"kurtosis"``          m_3 / m_2^1.5 and m_4 / m_2^2: biased, Pearson's (not excess), as
                                        ``scipy.stats.skew(bias=True)`` and ``kurtosis(fisher=False)``;
    ``"min"``, ``"max"``, ``"ptp"``     as NumPy's;
    ``"line_length"``                   sum |dx_t|;
    ``"zero_crossings"``                the number of t with (x_t < 0) != (x_{t+1} < 0);
    ``"mobility"``                      sqrt(var(dx) / var(x)), Hjorth's, per sample (times fs: per second);
    ``"complexity"``                    sqrt(var(ddx) / var(dx)) / mobility;
    ``"teager"``                        the mean over t = 1 .. W - 2 of x_t^2 - x_{t-1} x_{t+1}.

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64 with the sample axis of the
    data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for one-dimensional --
    for one name, for a tuple a dict of name -> such an array in the order asked, all from ONE
    read of the stream and bit-identical to the single-name call.  Host data gives ndarrays, CUDA
    data CUDA tensors.

    A window that holds a NaN is NaN in every feature; +-inf and a zero variance give what IEEE
    arithmetic gives from the definitions.  A window's bits depend on W and its own samples only:
    not on ``step``, the number of channels, the chunking, host or CUDA data, or the other
    features asked (the device sums a window in an order that is a function of W alone, without
    atomics).  The moments are sums about the window's first sample, so an offset of the data
    costs no accuracy.

    Complex data, more than two dimensions, ``winsize < 4``, ``step < 1``, sizes that are not
    integers, an unknown or empty ``features`` raise ``ValueError`` before the stream or the device
    is touched (a producer's complex chunks when the first one arrives); so does a stream shorter
    than ``winsize``.  Device memory does not grow with a host-fed stream: fewer than ``winsize``
    samples (or, between two chunks, the unfinished windows' samples) are carried, and each push's
    results come down as they are made; CUDA-fed streams keep theirs on the device.
    """
    who = "window_features"
    names = _stream._names(features, WINDOW_FEATURES, "window feature(s)")
    W = _stream._size(winsize, 4, None, who, "winsize")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    order = [f for f in WINDOW_FEATURES if f in names]       # the planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_FEATURE, order)
    parts, host = _stream._planes(who, pro, W, step, kind, layout, len(order),
                                  lambda x, out: dev.window_features(x, W, step, mask, out))
    return _stream._result(parts, host, layout, features, names, {f: (i, None) for i, f in enumerate(order)})
