"""window_connectivity: time-resolved channel-pair matrices of a stream (no counterpart in the
reference): the covariance and correlation of real data, the amplitude-envelope correlation and
the phase-locking values of an analytic signal, one (C, C) matrix per window of ``winsize``
samples, ``step`` apart -- what ``numpy.corrcoef`` or ``analytic_connectivity`` give window by
window, from one pass over the stream.  The pair sums are Gram products with time as the inner
dimension and run on the float64 matrix pipe: ``csrc/windowpair.hip`` (K19), ``osz_window_pairs``.
"""

import functools

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)

WINDOW_CONNECTIVITY = tuple(_lib.WINDOW_CONNECTIVITY)
_REAL = _lib.WC_REAL


def _kind(names, is_complex, what):
    if is_complex != (names[0] not in _REAL):
        raise ValueError(f"window_connectivity: {names} take {'real' if names[0] in _REAL else 'complex (analytic)'} "
                         f"data, got {what}: {_REAL} are the measures of real data, "
                         f"{tuple(m for m in WINDOW_CONNECTIVITY if m not in _REAL)} those of an analytic signal")


def _rows(arr, layout, is_complex):
    """A chunk -> ((nch, n) float64 or complex128 CUDA rows, came_from_host)."""
    if not is_complex:
        return layout.to2d(arr)
    torch = dev.torch
    host = not dev.is_tensor(arr) or not arr.is_cuda
    t = arr if dev.is_tensor(arr) else torch.from_numpy(np.ascontiguousarray(arr))
    t = t.cuda().to(torch.complex128).movedim(layout.axis, -1)
    return t.reshape(layout.nch, t.shape[-1]).contiguous(), host


def window_connectivity(data, winsize, step=None, measures=("corr",), ddof=1, axis=-1, chunksize=None):
    """Channel-pair matrices of every window of ``winsize`` samples, ``step`` apart.

    ``data`` is two-dimensional with C >= 2 channels, samples along ``axis``: an ndarray, a CUDA
    tensor or a producer.  ``chunksize`` applies to arrays only (default ``int(10e6)``).
    ``winsize`` = W is an integer >= 4, ``step`` an integer >= 1 that defaults to ``winsize``;
    ``step < W`` overlaps the windows, ``step > W`` leaves gaps.  Window k covers the samples
    k step .. k step + W - 1 counted from the first sample of the stream, whatever the chunks are;
    a trailing window the stream does not fill is dropped.

    ``measures`` is one name or a tuple of names of ``WINDOW_CONNECTIVITY``.  Real data:

    ``"cov"``    ``numpy.cov`` of the window's rows with divisor W - ``ddof`` (``ddof`` 0 or 1);
    ``"corr"``   ``numpy.corrcoef``, clipped to [-1, 1] as NumPy clips; the diagonal is 1.0.

    Complex data are a band-passed analytic signal z = a u, a = |z|, as for
    ``analytic_connectivity``, whose definitions and diagonal fixed points these are, applied to
    the window's samples alone:

    ``"aec"``    Pearson's r of the envelopes a_i, a_j; diagonal 1.0;
    ``"plv"``    |s_ij|, s_ij = mean conj(u_i) u_j; diagonal 1.0;
    ``"ciplv"``  |Im s_ij| / sqrt(1 - (Re s_ij)^2); diagonal 0.0.

    Returns ``(nwin, M)``: M float64 of shape (nwin, C, C), whatever ``axis`` is, for one name,
    for a tuple a dict of name -> such an array in the order asked, all from ONE pass over the
    stream and bit-identical to the single-name call.  Host data gives ndarrays, CUDA data CUDA
    tensors.

    Guarantees.  A matrix is symmetric bit for bit: [i, j] and [j, i] are written from one value.
    An entry's bits depend on W, ``ddof`` and the window's samples of its own two channels only:
    not on ``step``, the chunking, host or CUDA data, the other measures asked or which other
    channels are present (a pair sum is the matrix instruction's chain over the two rows in time
    order, in sub-blocks of ``_lib.WC_BLOCK`` samples counted from the window's start and folded
    in order; nothing is atomic).  The sums are taken about the window's first sample of each
    channel, so an offset of the data costs no accuracy.  A non-finite sample in channel k makes
    row and column k NaN, the diagonal included, in the windows that hold it, and so does a
    zero-amplitude sample of complex data; no other entry of any window moves a bit.  A constant
    channel gives ``cov`` exactly 0 and ``corr`` NaN in its row and column.

    One-dimensional data, more than two dimensions, fewer than two channels, ``winsize < 4``,
    ``step < 1``, sizes that are not integers, ``ddof`` other than 0 or 1, an unknown or empty
    ``measures``, real and complex measures mixed, and a measure that does not suit the data raise
    ``ValueError`` before the stream or the device is touched (a producer shows what it holds with
    its first chunk: the wrong kind is raised then); so does a stream shorter than ``winsize``.

    Memory.  A push writes at most 1 GiB of results (8 C^2 bytes per window and measure).
    Host-fed results come down push by push and device memory does not grow with the stream;
    CUDA-fed results stay on the device: when the 8 P C^2 nwin bytes of P measures do not fit the
    free device memory, ``MemoryError`` is raised before anything runs.
    """
    who = "window_connectivity"
    names = _stream._names(measures, WINDOW_CONNECTIVITY, "window connectivity measure(s)")
    if len({m in _REAL for m in names}) > 1:
        raise ValueError(f"window_connectivity: {_REAL} take real data and the other measures of {WINDOW_CONNECTIVITY} "
                         f"complex (analytic) data: {names} cannot come from one stream")
    W = _stream._size(winsize, 4, None, who, "winsize")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    if isinstance(ddof, bool) or ddof not in (0, 1):
        raise ValueError(f"window_connectivity: ddof must be 0 or 1, got {ddof!r}")
    kind = functools.partial(_kind, names)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind, pairs=True)
    is_complex = names[0] not in _REAL
    order = [m for m in WINDOW_CONNECTIVITY if m in names]    # the planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_CONNECTIVITY, order)
    planes, _ = _stream._pair_planes(who, pro, W, step, kind, layout, lambda arr: _rows(arr, layout, is_complex),
                                     len(order), lambda x, out, _: dev.window_pairs(x, W, step, ddof, mask, out))
    return planes.shape[1], _stream._asked(measures, names, {name: planes[order.index(name)] for name in names})
