"""window_mutual_info: the binned mutual information of every channel pair per window of a stream
(no counterpart in the reference): the nonlinear companion of ``window_connectivity``,
``window_xcorr`` and ``window_granger``, which see only what a covariance sees.  Every channel is
cut into ``bins`` bins per window, the joint histograms of all pairs are ONE Gram product of the
channels' one-hot bin-indicator rows -- 0 / 1 bytes in, exact integers out, on the int8 matrix pipe
-- and the entropies are sums of a table of n ln n: ``csrc/windowmi.hip`` (K25), ``osz_window_mi``.
"""

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream

WINDOW_MI = tuple(_lib.WINDOW_MI)
MI_BINNINGS = tuple(_lib.MI_BINNING)


def window_mutual_info(data, winsize, step=None, measures=("mi",), bins=8, binning="quantile", axis=-1,
                       chunksize=None):
    """Binned mutual information of every channel pair in every window of ``winsize`` samples, ``step`` apart.

    ``data`` is two-dimensional real data with C >= 2 channels, samples along ``axis``: an ndarray, a
    CUDA tensor or a producer.  ``chunksize`` applies to arrays only (default ``int(10e6)``).
    ``winsize`` = W is an integer from 16 to 4096, ``step`` an integer >= 1 that defaults to
    ``winsize`` (``step < W`` overlaps the windows, ``step > W`` leaves gaps), ``bins`` = B an integer
    from 2 to 16, ``binning`` a name of ``MI_BINNINGS``.  Window k covers the samples k step .. k step
    + W - 1 counted from the first sample of the stream, whatever the chunks are; a trailing window
    the stream does not fill is dropped.

    Per window and channel there are B - 1 edges e_1 <= .. <= e_{B-1}:

    ``"quantile"``  e_k = ``numpy.quantile(window, k / B, method="linear")`` (Hyndman & Fan type 7,
                    ``window_quantiles``' arithmetic to the bit): bins of W / B +- 1 samples of
                    continuous data;
    ``"uniform"``   e_k = lo + k ((hi - lo) / B), lo and hi the window's minimum and maximum, every
                    operation one IEEE operation.  A window whose hi - lo is not finite counts as
                    non-finite.

    The bin of a sample is the number of edges <= it (``numpy.searchsorted(edges, x, side="right")``),
    0 .. B - 1: the maximum lands in bin B - 1 and a constant window is all bin B - 1.  n_ab(i, j) is
    the number of samples of the window with channel i in bin a and channel j in bin b, n_a(i) the
    marginal count, and with phi(n) = n ln n, phi(0) = 0,

        H_i   = ln W - (sum_a phi(n_a)) / W
        H_ij  = ln W - (sum_ab phi(n_ab)) / W
        MI_ij = H_i + H_j - H_ij                (nats; the plug-in estimate, no bias correction)

    ``measures`` is one name or a tuple of names of ``WINDOW_MI``:

    ``"counts"``  n_ab(i, j) itself, shape (nwin, B, B, C, C), float64 holding exact integers:
                  ``counts[k, a, b, i, j]``; for pooling over epochs and for exact tests;
    ``"mi"``      MI_ij, shape (nwin, C, C); a finite value below 0 is written as +0.0;
    ``"nmi"``     MI_ij / sqrt(H_i H_j) clipped to [0, 1], NaN where H_i H_j = 0;
    ``"joint"``   H_ij.

    Returns ``(nwin, M)``: M is the array of one name, for a tuple a dict of name -> array in the
    order asked, all from ONE pass over the stream and bit-identical to the single-name call.  Host
    data gives ndarrays, CUDA data CUDA tensors.

    Guarantees.  ``mi``, ``nmi`` and ``joint`` are symmetric bit for bit -- they are computed once
    for i < j and mirrored -- and ``counts[k, a, b, i, j]`` and ``counts[k, b, a, j, i]`` are the
    same bits.  The diagonal holds fixed points: ``mi[i, i]`` = ``joint[i, i]`` = H_i, ``nmi[i, i]``
    = 1.0 (NaN for H_i = 0) and ``counts[k, a, b, i, i]`` = n_a for a = b, 0 elsewhere.  An entry's
    bits depend on W, ``bins``, ``binning`` and the window's samples of its own two channels, in the
    order the data has them, only: not on ``step``, the chunking, host or CUDA data, ``axis``, the other measures asked, which other
    channels are present or how the windows are split over launches (the counts are integers, the sum
    over the cells runs in an order that is a function of B alone, phi(n) is read from one table, so
    it is a function of n alone; ln W is taken as phi(W) / W, so a constant channel has H = 0.0
    exactly; nothing is atomic).  A NaN or +-inf in channel k makes row and column k NaN in every
    measure, ``counts`` included, in the windows that hold it; no other entry of any window moves a
    bit.  A constant channel gives ``mi`` 0.0, ``joint`` the other channel's H and ``nmi`` NaN.  An
    offset of the data costs nothing: the bins are comparisons.

    Complex data, one-dimensional data, more than two dimensions, fewer than two channels, sizes
    out of range or not integers, an unknown ``binning`` and an unknown or empty ``measures`` raise
    ``ValueError`` before the stream or the device is touched (a producer shows what it holds with
    its first chunk: complex chunks are raised then); so does a stream shorter than ``winsize``.

    Memory.  A push writes at most 1 GiB of results: 8 C^2 bytes per window and matrix measure and
    8 B^2 C^2 for ``counts``.  Host-fed results come down push by push and device memory does not
    grow with the stream; CUDA-fed results stay on the device: when they do not fit the free device
    memory, ``MemoryError`` is raised before anything runs.
    """
    who = "window_mutual_info"
    names = _stream._names(measures, WINDOW_MI, "window mutual-information measure(s)")
    W = _stream._size(winsize, 16, _lib.WM_LONGEST, who, "winsize")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    B = _stream._size(bins, 2, _lib.WM_MAXBINS, who, "bins")
    if not isinstance(binning, str) or binning not in MI_BINNINGS:
        raise ValueError(f"window_mutual_info: binning must be one of {MI_BINNINGS}, got {binning!r}")
    how = _lib.MI_BINNING[binning]
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind, pairs=True)
    order = [m for m in WINDOW_MI[1:] if m in names]          # the (C, C) planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_MI, names)
    planes, cells = _stream._pair_planes(who, pro, W, step, kind, layout, layout.to2d, len(order),
                                         lambda x, out, cnt: dev.window_mi(x, W, step, B, how, mask, cnt, out),
                                         advice=f", lower bins (now {B})", lags=B * B if "counts" in names else 0,
                                         more_for="counts")
    found = {name: planes[p] for p, name in enumerate(order)}
    if cells is not None:
        found["counts"] = cells.reshape((cells.shape[0], B, B) + tuple(cells.shape[2:]))
    return found[names[0]].shape[0], _stream._asked(measures, names, found)
