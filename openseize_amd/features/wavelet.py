"""window_wavelet: the sub-band energies and statistics of a discrete wavelet transform of every
window of a stream (no counterpart in the reference) -- relative wavelet energy and wavelet entropy
(Rosso et al. 2001) and the per-band mean absolute value and standard deviation of Subasi (2007):
the dyadic, time-localised bands that the rectangle sums of ``window_spectral`` are not.  The
transform is defined here: orthonormal filters, periodised within the window.  The device kernel
of ``csrc/windowwave.hip`` (K21), ``osz_window_wavelet``, holds the window in LDS, transforms it
level by level there and writes only the statistics.  The Daubechies filters are built on the host
by spectral factorisation (no wavelet library is needed).  The windows, the streaming loop and the
layout of the result are those of ``window_features``: ``features/_stream.py``.
"""

from functools import lru_cache
from math import comb

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream
from openseize_amd.features._stream import _advance, window_count, window_plan  # noqa: F401  (the family's)

WINDOW_WAVELET = tuple(_lib.WINDOW_WAVELET)
WAVELETS = ("haar",) + tuple(f"db{N}" for N in range(1, 11))
_PER_BAND = ("energy", "relative", "mean_abs", "std")
_TOL = 1e-10                                                 # of the orthonormality conditions


@lru_cache(maxsize=None)
def _daubechies(N):
    """The low-pass decomposition filter of the Daubechies wavelet with N vanishing moments, 2N
    float64 values (read-only): the minimum-phase spectral factor of P(y) = sum_{k<N} C(N-1+k, k)
    y^k, y = (2 - z - 1/z) / 4 -- of each pair of roots z, 1/z the one inside the unit circle --
    times (1 + z)^N, scaled to the sum sqrt 2."""
    zs = []
    if N > 1:
        for y in np.roots([comb(N - 1 + k, k) for k in range(N - 1, -1, -1)]):
            b = 1 - 2 * y                                    # z^2 - 2 b z + 1 = 0
            r = np.sqrt(b * b - 1 + 0j)
            z = b + r if abs(b + r) >= abs(b - r) else b - r   # the root outside: no cancellation
            zs.append(1 / z)                                 # (the two multiply to 1)
    h = np.real(np.poly(zs)) if zs else np.ones(1)
    for _ in range(N):
        h = np.convolve(h, [1.0, 1.0])
    h = h * (np.sqrt(2.0) / np.sum(h))
    h.setflags(write=False)
    return h


def _orthonormal(h, who):
    """``who``'s ValueError unless |sum h - sqrt 2| and |sum_k h_k h_{k+2m} - delta_m| are <= 1e-10."""
    L = h.shape[0]
    worst = abs(float(np.sum(h)) - np.sqrt(2.0))
    for m in range(L // 2):
        worst = max(worst, abs(float(np.sum(h[:L - 2 * m] * h[2 * m:])) - (m == 0)))
    if not worst <= _TOL:
        raise ValueError(f"{who}: the filter is not orthonormal: sum h = sqrt 2 and sum_k h_k h_(k+2m) = delta_m "
                         f"must hold to {_TOL}, the worst is off by {worst:.3g}")


def _lowpass(wavelet, who):
    """The low-pass decomposition filter of ``wavelet``, a name of WAVELETS or the filter itself."""
    if isinstance(wavelet, str):
        if wavelet not in WAVELETS:
            raise ValueError(f"{who}: unknown wavelet {wavelet!r}: choose from {WAVELETS} or give the low-pass "
                             "decomposition filter")
        return _daubechies(1 if wavelet == "haar" else int(wavelet[2:]))
    try:
        h = np.array(wavelet, dtype=np.float64)
    except (TypeError, ValueError):
        h = None
    if h is None or h.ndim != 1 or not 2 <= h.shape[0] <= _lib.WW_TAPS or h.shape[0] % 2 or not np.all(np.isfinite(h)):
        raise ValueError(f"{who}: wavelet must be a name of {WAVELETS} or a sequence of an even number, 2 to "
                         f"{_lib.WW_TAPS}, of finite real filter values, got {wavelet!r}")
    _orthonormal(h, who)
    h.setflags(write=False)
    return h


def wavelet_filters(wavelet):
    """``(lo, hi)``: the float64 decomposition filters h and g, g_k = (-1)^k h_{L-1-k}, of ``wavelet``
    -- a name of ``WAVELETS`` ("haar" is "db1"; "dbN" has 2N taps) or a low-pass filter h itself, a
    sequence of even length 2 .. ``_lib.WW_TAPS`` that passes the orthonormality checks of
    ``window_wavelet`` (else ``ValueError``)."""
    h = _lowpass(wavelet, "wavelet_filters")
    g = h[::-1] * np.where(np.arange(h.shape[0]) % 2, -1.0, 1.0)
    return np.array(h), g


def wavelet_level(winsize, taps):
    """The default level of windows of ``winsize`` samples and a filter of ``taps`` values: max(1,
    min(v, floor(log2(winsize / (taps - 1))), ``_lib.WW_LEVELS``)), v the exponent of 2 in
    ``winsize`` (``taps`` = 2 uses log2 winsize) -- the deepest level whose input is still at least
    as long as the filter, among those that halve evenly.  An odd ``winsize`` raises."""
    W = _stream._size(winsize, 2, None, "wavelet_level", "winsize")
    L = _stream._size(taps, 2, _lib.WW_TAPS, "wavelet_level", "taps")
    if W % 2 or L % 2:
        raise ValueError(f"wavelet_level: winsize and taps must be even, got {W} and {L}")
    v = (W & -W).bit_length() - 1
    span, deep = max(L - 1, 1), 0
    while (span << (deep + 1)) <= W:                         # floor(log2(W / span)), in integers
        deep += 1
    return max(1, min(v, deep, _lib.WW_LEVELS))


def wavelet_bands(fs, level):
    """The nominal edges ``(f_lo, f_hi)`` of the ``level`` + 1 bands in plane order: (fs / 2^(j+1),
    fs / 2^j) for d^j, j = 1 .. level, then (0, fs / 2^(level+1)) for a^level."""
    J = _stream._size(level, 1, _lib.WW_LEVELS, "wavelet_bands", "level")
    if not _stream._is_real(fs) or not fs > 0 or not np.isfinite(fs):
        raise ValueError(f"wavelet_bands: fs must be a positive number, got {fs!r}")
    fs = float(fs)
    return tuple((fs / 2 ** (j + 1), fs / 2 ** j) for j in range(1, J + 1)) + ((0.0, fs / 2 ** (J + 1)),)


def window_wavelet(data, winsize, step=None, features=("relative", "entropy"), wavelet="db4", level=None,
                   center=True, normalize=True, axis=-1, chunksize=None):
    """Wavelet sub-band energies and statistics of every window of ``winsize`` samples, ``step``
    apart, per channel.

    ``data``, ``winsize`` = W, ``step``, ``axis`` and ``chunksize`` are those of ``window_fractal``:
    real one- or two-dimensional data, samples along ``axis`` -- an ndarray, a CUDA tensor or a
    producer; window k covers the samples k step .. k step + W - 1 of the stream, whatever the
    chunks are, and a trailing window the stream does not fill is dropped.  W is an integer from 8
    to ``_lib.WW_LONGEST`` (4096: the device holds a window and its approximations in LDS).

    ``wavelet`` is a name of ``WAVELETS`` -- "haar" = "db1", "db2" .. "db10", L = 2N taps -- or the
    low-pass decomposition filter h itself: a sequence of even length L, 2 .. ``_lib.WW_TAPS`` = 32,
    with |sum h - sqrt 2| <= 1e-10 and |sum_k h_k h_{k+2m} - delta_m| <= 1e-10 for every m (the
    orthonormality that makes the band energies add up to the window's).  g_k = (-1)^k h_{L-1-k}.

    The transform is periodised within the window.  a^0 is the window, minus its mean when
    ``center`` (the mean from sums about the window's first sample); with n_j the length of a^j,
        a^{j+1}_i = sum_k h_k a^j_{(2i+k) mod n_j},   d^{j+1}_i = sum_k g_k a^j_{(2i+k) mod n_j}
    for i = 0 .. n_j / 2 - 1 and j = 0 .. J - 1.  ``level`` = J is an integer 1 ..
    ``_lib.WW_LEVELS`` = 12 with W a multiple of 2^J; ``None`` means ``wavelet_level(W, L)``.  n_j <
    L is allowed: the filter wraps more than once.  The B = J + 1 bands are d^1, d^2, .., d^J, a^J
    in this order; ``wavelet_bands(fs, J)`` gives their nominal edges.

    ``features`` is one name or a tuple of names of ``WINDOW_WAVELET``, everything in float64:

    ``"energy"``    E_b = sum c^2 over the band's coefficients.
    ``"relative"``  p_b = E_b / sum_b E_b.
    ``"entropy"``   -sum_b p_b ln p_b, a term with p_b = 0 being 0; divided by ln B when
                    ``normalize``.
    ``"mean_abs"``  the mean of |c| over the band's coefficients.
    ``"std"``       the population standard deviation of the band's coefficients (ddof 0), from
                    deviations about the band's mean: an offset of un-centred data costs a^J no
                    accuracy.

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64.  ``"entropy"`` has the
    sample axis of the data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for
    one-dimensional; the four per-band features carry a leading axis over the bands: (B, C, nwin).
    One name gives the bare array, a tuple a dict of name -> array in the order asked, all from ONE
    read of the stream and bit-identical to the single-name call.  Host data gives ndarrays, CUDA
    data CUDA tensors.

    A window that holds a NaN or +-inf is NaN in every feature.  A window with sum_b E_b = 0 (a
    constant window with ``center``) gives ``energy``, ``mean_abs`` and ``std`` 0 and ``relative``
    and ``entropy`` NaN.  A window's bits depend on W, the filter, J, ``center``, ``normalize`` and
    its own samples only: not on ``step``, the number of channels, the chunking, host or CUDA data,
    or the other features asked.

    Complex data, more than two dimensions, sizes that are not integers, ``winsize`` or ``level``
    out of range, a ``winsize`` that is no multiple of 2^J (or odd with ``level=None``), an unknown
    ``wavelet`` or a sequence that is not orthonormal, an unknown or empty ``features`` raise
    ``ValueError`` before the stream or the device is touched (a producer's complex chunks when the
    first one arrives); so does a stream shorter than ``winsize``.
    """
    who = "window_wavelet"
    names = _stream._names(features, WINDOW_WAVELET, "window wavelet feature(s)")
    W = _stream._size(winsize, 8, _lib.WW_LONGEST, who, f"winsize (the longest window is {_lib.WW_LONGEST} samples)")
    step = W if step is None else _stream._size(step, 1, None, who, "step")
    h = _lowpass(wavelet, who)
    if level is None:
        if W % 2:
            raise ValueError(f"{who}: winsize = {W} is odd: no level J has winsize a multiple of 2^J")
        J = wavelet_level(W, h.shape[0])
    else:
        J = _stream._size(level, 1, _lib.WW_LEVELS, who, "level")
    if W % (1 << J):
        raise ValueError(f"{who}: winsize = {W} is not a multiple of 2^J = {1 << J} for level J = {J}")
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    nch, B = layout.nch, J + 1
    where, count = {}, 0                                     # the planes a launch writes
    for f in WINDOW_WAVELET:
        if f in names:
            where[f] = (count, B) if f in _PER_BAND else (count, None)
            count += B if f in _PER_BAND else 1
    mask = dev.name_mask(_lib.WINDOW_WAVELET, where)
    parts, host = _stream._planes(who, pro, W, step, kind, layout, count,
                                  lambda x, out: dev.window_wavelet(x, W, step, mask, h, J, center, normalize, out))
    return _stream._result(parts, host, layout, features, names, where)
