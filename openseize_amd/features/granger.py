"""window_granger: time-domain Granger causality of every ordered channel pair per window of a
stream, with Geweke's decomposition (no counterpart in the reference): which channel drives which,
window by window -- F_{i->j}, the instantaneous coupling and their total, one (C, C) matrix per
window of ``winsize`` samples, ``step`` apart, from one pass over the stream.  The lagged
covariances are ``window_xcorr``'s Gram products on the float64 matrix pipe; the bivariate
Yule-Walker equations of every pair are solved by the block Levinson recursion:
``csrc/windowgranger.hip`` (K24), ``osz_window_granger``.
"""

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream

WINDOW_GRANGER = tuple(_lib.WINDOW_GRANGER)


def window_granger(data, winsize, step=None, measures=("granger",), order=8, axis=-1, chunksize=None):
    """Granger causality of every ordered channel pair in every window of ``winsize`` samples, ``step`` apart.

    ``data`` is two-dimensional real data with C >= 2 channels, samples along ``axis``: an ndarray, a
    CUDA tensor or a producer.  ``chunksize`` applies to arrays only (default ``int(10e6)``).
    ``winsize`` = W is an integer from 16 to 4096, ``step`` an integer >= 1 that defaults to
    ``winsize`` (``step < W`` overlaps the windows, ``step > W`` leaves gaps), ``order`` = p an
    integer from 1 to min(16, W // 8).  Window k covers the samples k step .. k step + W - 1 counted
    from the first sample of the stream, whatever the chunks are; a trailing window the stream does
    not fill is dropped.

    Per window and ordered pair (i, j), d is the row minus its mean over the window, r_ab(l) =
    (1 / W) sum_t d_a[t] d_b[t + l] the biased estimate of ``window_xcorr`` and z_t = (d_i[t],
    d_j[t])^T.  C(l) = E[z_t z_{t-l}^T] has the entries C(l)_ab = r_ba(l), C(-l) = C(l)^T.  The full
    model z_t = sum_{k=1..p} A_k z_{t-k} + e_t solves the bivariate Yule-Walker equations C(l) =
    sum_k A_k C(l - k), l = 1 .. p, and S = C(0) - sum_k A_k C(k)^T is its 2 x 2 error covariance.
    The restricted models are the scalar Yule-Walker models of d_i and d_j alone, of the same order,
    with the errors E_i and E_j (``window_ar``'s ``"error"`` with ``method="yule_walker"``).

    ``measures`` is one name or a tuple of names of ``WINDOW_GRANGER``, each (nwin, C, C) float64:

    ``"granger"``  F_{i->j} = ln(E_j / S_jj) at [k, i, j]: the row is the source and the column the
                   target, as a positive ``lag`` of ``window_xcorr`` means that j trails i;
    ``"instant"``  ln(S_ii S_jj / det S), the coupling within one sample;
    ``"total"``    (granger[k, i, j] + granger[k, j, i]) + instant[k, i, j], the float64 sum in
                   exactly that order: Geweke's total interdependence.

    A finite value below 0, which only rounding can produce, is written as +0.0.

    Returns ``(nwin, M)``: M is the array of one name, for a tuple a dict of name -> array in the
    order asked, all from ONE pass over the stream and bit-identical to the single-name call.  Host
    data gives ndarrays, CUDA data CUDA tensors.

    Guarantees.  ``instant`` and ``total`` are symmetric bit for bit: both mirrors are written from
    one computed value.  The diagonal is the fixed point 0.0 in every measure, and NaN in the
    windows where the channel is lost.  An entry's bits depend on W, ``order`` and the window's
    samples of its own two channels only: not on ``step``, the chunking, host or CUDA data,
    ``axis``, the other measures asked, which other channels are present or how the windows are
    split over launches (the sums are ``window_xcorr``'s, the order of every operation after them is
    a function of ``order`` alone, nothing is atomic).  A NaN or +-inf in channel k makes row and
    column k NaN in every measure, the diagonal included, in the windows that hold it; no other
    entry of any window moves a bit.  A constant channel (r_kk(0) = 0) gives NaN in its row and
    column.  A pair is NaN in all three measures and both directions when one of E_i, E_j, S_ii,
    S_jj or det S is not finite and > 0.  Linearly dependent channels (a channel that is a copy, a
    multiple or a filtered version of another within the order) make the equations ill-conditioned:
    their values are unspecified and may be NaN or large.

    Complex data, one-dimensional data, more than two dimensions, fewer than two channels, sizes
    out of range or not integers, ``order > winsize // 8`` and an unknown or empty ``measures``
    raise ``ValueError`` before the stream or the device is touched (a producer shows what it holds
    with its first chunk: complex chunks are raised then); so does a stream shorter than
    ``winsize``.

    Memory.  A push writes at most 1 GiB of results, 8 C^2 bytes per window and measure.  Host-fed
    results come down push by push and device memory does not grow with the stream; CUDA-fed
    results stay on the device: when they do not fit the free device memory, ``MemoryError`` is
    raised before anything runs.
    """
    who = "window_granger"
    names = _stream._names(measures, WINDOW_GRANGER, "window Granger measure(s)")
    W = _stream._size(winsize, 16, _lib.WG_LONGEST, who, "winsize")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    p = _stream._size(order, 1, _lib.WG_MAXORDER, who, "order")
    if p > W // 8:
        raise ValueError(f"window_granger: order must be at most winsize // 8 = {W // 8}, got {p}")
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind, pairs=True)
    planes = [m for m in WINDOW_GRANGER if m in names]       # the (C, C) planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_GRANGER, names)
    whole, _ = _stream._pair_planes(who, pro, W, step, kind, layout, layout.to2d, len(planes),
                                    lambda x, out, _: dev.window_granger(x, W, step, p, mask, out))
    return whole.shape[1], _stream._asked(measures, names, {name: whole[planes.index(name)] for name in names})
