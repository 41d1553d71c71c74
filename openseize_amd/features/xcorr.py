"""window_xcorr: the lagged cross-correlation of every channel pair per window of a stream (no
counterpart in the reference): which channel leads, by how many samples, and how strongly -- the
normalised cross-correlation over the lags -``maxlag`` .. ``maxlag``, its peak, the lag of the
peak and the signed value there, one (C, C) matrix (or one per lag) per window of ``winsize``
samples, ``step`` apart, from one pass over the stream.  The lagged sums are Gram products with
one operand shifted in time and run on the float64 matrix pipe: ``csrc/windowxcorr.hip`` (K23),
``osz_window_xcorr``.
"""

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream

WINDOW_XCORR = tuple(_lib.WINDOW_XCORR)


def xcorr_lags(maxlag):
    """The lags of the lag axis of ``"xcorr"``: ``np.arange(-maxlag, maxlag + 1)``."""
    L = _stream._size(maxlag, 0, _lib.WX_MAXLAG, "xcorr_lags", "maxlag")
    return np.arange(-L, L + 1)


def window_xcorr(data, winsize, step=None, measures=("peak", "lag"), maxlag=16, normalize=True, axis=-1,
                 chunksize=None):
    """Lagged cross-correlation of every channel pair in every window of ``winsize`` samples, ``step`` apart.

    ``data`` is two-dimensional real data with C >= 2 channels, samples along ``axis``: an ndarray, a
    CUDA tensor or a producer.  ``chunksize`` applies to arrays only (default ``int(10e6)``).
    ``winsize`` = W is an integer from 8 to 4096, ``step`` an integer >= 1 that defaults to
    ``winsize`` (``step < W`` overlaps the windows, ``step > W`` leaves gaps), ``maxlag`` = L an
    integer from 0 to min(64, W // 2).  Window k covers the samples k step .. k step + W - 1 counted
    from the first sample of the stream, whatever the chunks are; a trailing window the stream does
    not fill is dropped.

    Per window, d_i is row i minus its mean over the window, and for -L <= l <= L

        r_ij(l) = (1 / W) sum_t d_i[t] d_j[t + l],   t over max(0, -l) .. min(W, W - l) - 1

    (the biased estimate), rho_ij(l) = r_ij(l) / sqrt(r_ii(0) r_jj(0)) clipped to [-1, 1].  v is rho
    with ``normalize=True`` and r with ``normalize=False``.  A peak at a positive lag means that
    channel j trails channel i; r_ji(l) = r_ij(-l).

    ``measures`` is one name or a tuple of names of ``WINDOW_XCORR``:

    ``"xcorr"``   v itself, shape (nwin, 2 L + 1, C, C): index L + l of the lag axis is lag l
                  (``xcorr_lags(L)``);
    ``"peak"``    max over l of ``|v_ij(l)|``, shape (nwin, C, C);
    ``"lag"``     the l that attains the peak, as float64, shape (nwin, C, C);
    ``"signed"``  v_ij at that lag, with its sign, shape (nwin, C, C).

    The tie rule, for i < j: the candidates are compared on the float64 values of ``|v|`` that are
    returned; among equal maxima the smallest ``|l|`` wins, of +l and -l the positive one; the
    [j, i] entry is written from the [i, j] one.

    Returns ``(nwin, M)``: M is the array of one name, for a tuple a dict of name -> array in the
    order asked, all from ONE pass over the stream and bit-identical to the single-name call.  Host
    data gives ndarrays, CUDA data CUDA tensors.

    Guarantees.  ``xcorr[k, L + l, i, j]`` and ``xcorr[k, L - l, j, i]`` are the same bits, ``peak``
    and ``signed`` are symmetric bit for bit and ``lag[j, i]`` is ``-lag[i, j]``: each is written
    from one computed value.  The diagonal: with ``normalize=True`` the lag-0 plane is 1.0, ``peak``
    1.0, ``lag`` 0.0 and ``signed`` 1.0, fixed points; with ``normalize=False`` they are r_ii(0),
    r_ii(0), 0.0 and r_ii(0); the other lags of the diagonal are the autocorrelation, lag l and -l
    the same bits.  An entry's bits depend on W, ``normalize`` and the window's samples of its own
    two channels only: not on ``step``, the chunking, host or CUDA data, ``axis``, the other measures
    asked, which other channels are present or how the windows are split over launches, and a plane
    ``xcorr[:, L + l]`` not on ``maxlag`` either (every sum is the matrix instruction's chain over
    the window's samples in time order, whichever lags are computed with it; nothing is atomic).
    The mean is taken about the window's first sample of the row, so an offset of the data costs no
    accuracy.  A NaN or +-inf in channel k makes row and column k NaN in every measure, ``lag`` and
    the diagonal included, in the windows that hold it; no other entry of any window moves a bit.
    A constant channel gives NaN in its row and column with ``normalize=True``, as ``corr`` does,
    and 0 in ``xcorr``, ``peak``, ``signed`` and ``lag`` with ``normalize=False``.

    Complex data, one-dimensional data, more than two dimensions, fewer than two channels, sizes
    out of range or not integers, ``maxlag > winsize // 2``, a ``normalize`` that is not a bool and
    an unknown or empty ``measures`` raise ``ValueError`` before the stream or the device is touched
    (a producer shows what it holds with its first chunk: complex chunks are raised then); so does a
    stream shorter than ``winsize``.

    Memory.  A push writes at most 1 GiB of results: 8 C^2 bytes per window and matrix measure and
    8 (2 L + 1) C^2 for ``xcorr``.  Host-fed results come down push by push and device memory does
    not grow with the stream; CUDA-fed results stay on the device: when they do not fit the free
    device memory, ``MemoryError`` is raised before anything runs.
    """
    who = "window_xcorr"
    names = _stream._names(measures, WINDOW_XCORR, "window cross-correlation measure(s)")
    W = _stream._size(winsize, 8, _lib.WX_LONGEST, who, "winsize")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    L = _stream._size(maxlag, 0, _lib.WX_MAXLAG, who, "maxlag")
    if L > W // 2:
        raise ValueError(f"window_xcorr: maxlag must be at most winsize // 2 = {W // 2}, got {L}")
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError(f"window_xcorr: normalize must be True or False, got {normalize!r}")
    normalize = bool(normalize)
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind, pairs=True)
    order = [m for m in WINDOW_XCORR[1:] if m in names]       # the (C, C) planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_XCORR, names)
    planes, full = _stream._pair_planes(who, pro, W, step, kind, layout, layout.to2d, len(order),
                                        lambda x, out, xc: dev.window_xcorr(x, W, step, L, normalize, mask, xc, out),
                                        advice=f", lower maxlag (now {L})", lags=2 * L + 1 if "xcorr" in names else 0)
    found = {name: planes[p] for p, name in enumerate(order)}
    if full is not None:
        found["xcorr"] = full
    return found[names[0]].shape[0], _stream._asked(measures, names, found)
