"""window_transfer_entropy: the binned transfer entropy of every ordered channel pair per window of
a stream (no counterpart in the reference): the nonlinear, directed member of the pair family, where
``window_granger`` is linear and directed and ``window_mutual_info`` nonlinear and undirected.  Every
channel is cut into ``bins`` bins per window as ``window_mutual_info`` cuts it, the three-way
histograms n(y_t, y_{t-1}, x_{t-u}) of all ordered pairs are ONE rectangular product of the targets'
one-hot (bin now, bin before) rows with the sources' one-hot bin rows -- 0 / 1 bytes in, exact
integers out, on the int8 matrix pipe -- and the entropies are sums of a table of n ln n:
``csrc/windowte.hip`` (K26), ``osz_window_te``.
"""

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features.mutual_info import MI_BINNINGS

WINDOW_TE = tuple(_lib.WINDOW_TE)


def window_transfer_entropy(data, winsize, step=None, measures=("te",), bins=4, lag=1, binning="quantile", axis=-1,
                            chunksize=None):
    """Binned transfer entropy of every ordered channel pair in every window of ``winsize`` samples, ``step`` apart.

    ``data``, ``winsize`` = W (16 to 4096), ``step``, ``binning``, ``axis`` and ``chunksize`` are
    those of ``window_mutual_info``, and so are the windows: window k covers the samples k step ..
    k step + W - 1 of the stream, whatever the chunks are, and a trailing window the stream does not
    fill is dropped.  ``bins`` = B is an integer from 2 to 8 (a (bin now, bin before) symbol is one
    byte), ``lag`` = u an integer from 1 to min(64, W // 2): how far back the source is read.

    The bins are ``window_mutual_info``'s, cut per window and channel from all W samples: the same
    edges (``"quantile"`` or ``"uniform"``), the same rule -- the bin of a sample is the number of
    edges <= it, ``numpy.searchsorted(edges, x, side="right")`` -- the same bytes.  With T = W - u,
    n_abc(i, j) counts the t = u .. W - 1 of the window with the target j in bin a at t and in bin b
    at t - 1 and the source i in bin c at t - u, and with phi(n) = n ln n, phi(0) = 0,

        S3 = sum_abc phi(n_abc)           Sab = sum_ab phi(sum_c n_abc)
        Sbc = sum_bc phi(sum_a n_abc)     Sb = sum_b phi(sum_ac n_abc)
        TE_{i -> j} = I(Y_t ; X_{t-u} | Y_{t-1}) = ((S3 - Sab) - (Sbc - Sb)) / T
        Hc_j = H(Y_t | Y_{t-1}) = (Sb - Sab) / T

    in nats: the plug-in estimate, no bias correction (independent channels give about B (B - 1)^2 /
    (2 T)).  The marginals are integer sums of the pair's own cells; every float64 sum runs with b
    outermost, then a, then c, and the four are combined in the order written above.

    ``measures`` is one name or a tuple of names of ``WINDOW_TE``:

    ``"counts"``  n_abc(i, j) itself, shape (nwin, B, B, B, C, C), float64 holding exact integers:
                  ``counts[k, a, b, c, i, j]``;
    ``"te"``      TE, shape (nwin, C, C): ``[k, i, j]`` is i -> j, the row the source and the column
                  the target, as in ``window_granger``; a finite value below 0 is written as +0.0;
    ``"nte"``     te / Hc_j clipped to [0, 1], NaN where Hc_j = 0;
    ``"net"``     te[k, i, j] - te[k, j, i], each side its own float64 subtraction: ``net[j, i]``
                  is ``-net[i, j]``, and a zero is +0.0 on both sides.

    Returns ``(nwin, M)``: M is the array of one name, for a tuple a dict of name -> array in the
    order asked, all from ONE pass over the stream and bit-identical to the single-name call.  Host
    data gives ndarrays, CUDA data CUDA tensors.

    Guarantees.  Pair locality: an entry's bits depend on W, ``bins``, ``lag``, ``binning`` and the
    window's samples of its own two channels only: not on ``step``, the chunking, host or CUDA data,
    ``axis``, the other measures asked, which other channels are present or how the windows are
    split over launches (the counts are integers, each sum runs in one thread in an order that is a
    function of B alone, phi(n) is read from one table, nothing is atomic).  Diagonal: ``te``,
    ``nte`` and ``net`` hold the fixed point +0.0 on the diagonal, a channel is not its own source;
    ``counts[..., i, i]`` is what the definition gives.  Non-finite samples: a NaN or +-inf makes its
    channel's row and column NaN in every measure, ``counts`` included, in the windows that hold it
    (under ``"uniform"`` a hi - lo that is not finite counts the same way); no other bit of any
    window moves.  Constant channel: as a target it gives ``te`` +0.0 exactly and ``nte`` NaN, as a
    source ``te`` +0.0 exactly (S3 meets Sab and Sbc meets Sb term for term).  Count sums:
    ``counts`` sum to T over (a, b, c), and their sum over c is the same array for every source of
    a target.

    Complex data, one-dimensional data, more than two dimensions, fewer than two channels, sizes
    out of range or not integers, an unknown ``binning`` and an unknown or empty ``measures`` raise
    ``ValueError`` before the stream or the device is touched (a producer shows what it holds with
    its first chunk: complex chunks are raised then); so does a stream shorter than ``winsize``.

    Memory.  A launch works in 4 Bp^3 C^2 bytes per window of a batch, Bp = B rounded up to a power
    of two: when the work space of a push exceeds the free device memory, ``MemoryError`` is raised
    before anything is launched, and it names ``bins`` and the channel count.  A push writes at most
    1 GiB of results, 8 C^2 bytes per window and matrix measure and 8 B^3 C^2 for ``counts``;
    CUDA-fed results stay on the device, and when they do not fit the free device memory,
    ``MemoryError`` is raised before anything runs.
    """
    who = "window_transfer_entropy"
    names = _stream._names(measures, WINDOW_TE, "window transfer-entropy measure(s)")
    W = _stream._size(winsize, 16, _lib.WT_LONGEST, who, "winsize")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    B = _stream._size(bins, 2, _lib.WT_MAXBINS, who, "bins")
    u = _stream._size(lag, 1, min(_lib.WT_MAXLAG, W // 2), who, "lag")
    if not isinstance(binning, str) or binning not in MI_BINNINGS:
        raise ValueError(f"{who}: binning must be one of {MI_BINNINGS}, got {binning!r}")
    how = _lib.MI_BINNING[binning]
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind, pairs=True)
    order = [m for m in WINDOW_TE[1:] if m in names]          # the (C, C) planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_TE, names)

    def launch(x, out, cnt):
        need = 8 * dev.window_te_work(x.shape[0], x.shape[1], W, step, B, u, mask)
        free = dev.torch.cuda.mem_get_info()[0]
        if need > free:
            raise MemoryError(f"{who}: the work space of one launch, {need / 1e9:.2f} GB, is more than the "
                              f"{free / 1e9:.2f} GB of device memory that are free: lower bins (now {B}) or select "
                              f"fewer of the {x.shape[0]} channels")
        dev.window_te(x, W, step, B, u, how, mask, cnt, out)

    planes, cells = _stream._pair_planes(who, pro, W, step, kind, layout, layout.to2d, len(order), launch,
                                         advice=f", lower bins (now {B})", lags=B ** 3 if "counts" in names else 0,
                                         more_for="counts")
    found = {name: planes[p] for p, name in enumerate(order)}
    if cells is not None:
        found["counts"] = cells.reshape((cells.shape[0], B, B, B) + tuple(cells.shape[2:]))
    return found[names[0]].shape[0], _stream._asked(measures, names, found)
