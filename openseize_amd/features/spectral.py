"""window_spectral: the spectrum of every window of a stream reduced to a few numbers (no
counterpart in the reference) -- band power and relative band power, peak frequency, centroid and
spread, spectral edge frequencies, spectral entropy and flatness over time: what sleep staging,
seizure detection and depth-of-anaesthesia features are built from, and what ``window_features``
(sums and extremes), ``window_entropy`` (pattern counts) and ``window_quantiles`` (order statistics)
leave out.  The periodograms are those of ``stft``: the segmenter and transforms of ``csrc/spec.hip``;
the device kernel of ``csrc/windowspec.hip`` (K18), ``osz_spectral_features``, reduces each of them
in one launch per push, so the (C, nfreq, nseg) spectrogram is never held.  The windows and the
layout of the result are those of ``window_features``: ``features/_stream.py``.
"""

import math

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core import numerical as nm
from openseize_amd.features import _stream
from openseize_amd.features._stream import _is_complex, _is_real

WINDOW_SPECTRAL = tuple(_lib.WINDOW_SPECTRAL)

# bytes of periodograms one push may write (osz_spectral_features reads them once and they go).
# benchmarks/spectral_probe.py: bounds of 64, 128 and 256 MiB, which would keep a push's periodograms
# in the Infinity Cache, measured 2 .. 30 % slower than this one -- more launches, nothing gained.
_SPECTRAL_PUSH_BYTES = 1 << 30


def _frequency(value, what):
    if not _is_real(value) or not math.isfinite(value):
        raise ValueError(f"window_spectral: {what} must be a finite number, got {value!r}")
    return float(value)


def _bin_range(freqs, fmin, fmax):
    """(k0, k1), inclusive: the bins with fmin <= freqs[k] <= fmax; bin 1 .. the last by default
    (the detrend removes DC)."""
    k0 = 1 if fmin is None else int(np.searchsorted(freqs, _frequency(fmin, "fmin"), side="left"))
    k1 = len(freqs) - 1 if fmax is None else int(np.searchsorted(freqs, _frequency(fmax, "fmax"), side="right")) - 1
    if k0 > k1 or k0 >= len(freqs) or k1 < 0:
        raise ValueError(f"window_spectral: no bin lies in fmin = {fmin!r} .. fmax = {fmax!r} (the bins are "
                         f"{freqs[1] - freqs[0]:g} apart, from 0 to {freqs[-1]:g})")
    return k0, k1


def _band_bins(bands, freqs, k0, k1):
    """(pairs of bins [b0, b1), single) of ``bands``: one (lo, hi) pair or a sequence of 1 to
    _lib.WS_BANDS_MOST pairs; a band holds the bins with lo <= freqs[k] < hi."""
    what = (f"window_spectral: bands must be a (lo, hi) pair or a sequence of 1 to {_lib.WS_BANDS_MOST} pairs of "
            f"finite frequencies, got {bands!r}")
    if isinstance(bands, np.ndarray):
        bands = bands.tolist()
    if not isinstance(bands, (tuple, list)) or not bands:
        raise ValueError(what)
    single = len(bands) == 2 and all(_is_real(v) for v in bands)
    pairs = [bands] if single else list(bands)
    if not 1 <= len(pairs) <= _lib.WS_BANDS_MOST:
        raise ValueError(what)
    bins = []
    for pair in pairs:
        if isinstance(pair, np.ndarray):
            pair = pair.tolist()
        if (not isinstance(pair, (tuple, list)) or len(pair) != 2
                or not all(_is_real(v) and math.isfinite(v) for v in pair)):
            raise ValueError(what)
        lo, hi = float(pair[0]), float(pair[1])
        b0 = int(np.searchsorted(freqs, lo, side="left"))
        b1 = int(np.searchsorted(freqs, hi, side="left"))
        if b0 >= b1:
            raise ValueError(f"window_spectral: the band ({lo:g}, {hi:g}) holds no bin (lo <= f < hi, the bins are "
                             f"{freqs[1] - freqs[0]:g} apart)")
        if b0 < k0 or b1 > k1 + 1:
            raise ValueError(f"window_spectral: the band ({lo:g}, {hi:g}) does not lie inside the range "
                             f"{freqs[k0]:g} .. {freqs[k1]:g} of fmin and fmax")
        bins.append((b0, b1))
    return bins, single


def _fractions(edge):
    """(values, scalar) of ``edge``: a float, or a sequence of 1 to _lib.WS_EDGES_MOST floats in (0, 1]."""
    scalar = _is_real(edge)
    if not scalar and not isinstance(edge, (tuple, list, np.ndarray)):
        raise ValueError(f"window_spectral: edge must be a float or a sequence of floats in (0, 1], got {edge!r}")
    values = [edge] if scalar else list(np.asarray(edge).tolist() if isinstance(edge, np.ndarray) else edge)
    if not 1 <= len(values) <= _lib.WS_EDGES_MOST:
        raise ValueError(f"window_spectral: edge must hold from 1 to {_lib.WS_EDGES_MOST} values, got {len(values)}")
    for p in values:
        if not _is_real(p) or not math.isfinite(p) or not 0.0 < p <= 1.0:
            raise ValueError(f"window_spectral: every edge must be a finite float in (0, 1], got {p!r}")
    return [float(p) for p in values], scalar


def window_spectral(data, fs, winsize, step=None, features=("total", "edge", "entropy"), bands=None, edge=0.95,
                    fmin=None, fmax=None, window="hann", detrend="constant", scaling="density", normalize=True,
                    axis=-1, chunksize=None):
    """Spectral features of every window of ``winsize`` samples, ``step`` apart, per channel.

    ``data``, ``axis`` and ``chunksize`` are those of ``window_features``: real one- or
    two-dimensional data, samples along ``axis`` -- an ndarray, a CUDA tensor or a producer.
    ``winsize`` = W is an integer >= 8 and ``step`` an integer with 1 <= step <= W that defaults
    to W: window k covers the samples k step .. k step + W - 1 of the stream, whatever the chunks
    are, and a trailing window the stream does not fill is dropped.  The segmenter has no gaps:
    ``step > winsize`` is refused.  Each window is detrended (``detrend``: "constant" or "linear"),
    multiplied by ``window`` (``scipy.signal.get_window``) and transformed at nfft = W -- no zero
    padding -- into the one-sided periodogram P_k of ``stft`` at ``fs`` and ``scaling`` ("density"
    or "spectrum"), k = 0 .. W // 2, at the frequencies ``numpy.fft.rfftfreq(W, 1 / fs)``.

    The features are taken over the bins with ``fmin`` <= f <= ``fmax``; by default from bin 1 to
    bin W // 2 (the detrend removes bin 0).  With n the number of bins in the range, df = fs / W,
    f_k = k df and all sums over the range:

    ``"total"``     df sum P_k.  A rectangle sum, not the Simpson rule of ``metrics.power``.
    ``"band"``      df sum of P_k over the bins with lo <= f_k < hi for each band of ``bands``: one
                    (lo, hi) pair, or a sequence of 1 to ``_lib.WS_BANDS_MOST`` (16) pairs.
                    Adjacent bands partition the axis, overlaps are allowed; every band must hold
                    a bin and lie inside the range.  ``bands`` is read only when ``"band"`` or
                    ``"relative"`` is asked, and is required then.
    ``"relative"``  band / total.
    ``"peak"``      f_k of the largest P_k, ties going to the lowest k.
    ``"centroid"``  c = sum f_k P_k / sum P_k.
    ``"spread"``    sqrt(sum (f_k - c)^2 P_k / sum P_k), summed about c.
    ``"edge"``      for each p of ``edge`` the lowest f_k whose cumulative sum of P reaches p sum P:
                    a bin's frequency, nothing is interpolated; p = 1 gives a bin whose cumulative
                    sum reaches the total.  ``edge`` is a float or a sequence of 1 to
                    ``_lib.WS_EDGES_MOST`` (16) floats in (0, 1], read only when ``"edge"`` is asked.
    ``"entropy"``   -sum p_k ln p_k with p_k = P_k / sum P (a bin with p_k = 0 adds 0), divided by
                    ln n when ``normalize`` is set; 0 for n = 1.
    ``"flatness"``  n exp((1 / n) sum ln p_k): the geometric over the arithmetic mean of the
                    range, 0 where a p_k is 0.

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64 with the sample axis of the
    data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for one-dimensional --
    for one name, for a tuple a dict of name -> such an array in the order asked, all from ONE
    pass over the stream.  ``"band"`` and ``"relative"`` with a sequence of bands have one more
    leading axis of len(bands), with a single pair none; ``"edge"`` likewise.  Host data gives
    ndarrays, CUDA data CUDA tensors.

    A window that holds a NaN is NaN in every feature, ``"peak"`` and ``"edge"`` included (with
    ``detrend="linear"`` the least-squares fit refuses non-finite data as the reference's does:
    ``ValueError``).  A window whose range sums to exactly 0 has ``total`` and ``band`` 0 and every
    other feature NaN.

    The reduction is bit-reproducible per row: a window's features depend on its periodogram, the
    range, ``bands`` and ``edge`` only -- not on the other windows or channels of the launch, nor
    on the other features asked, so a single-name call equals its entry of a tuple call made on
    the same periodograms bit for bit.  The periodograms are ``spec.hip``'s and carry its guarantee:
    different cuts of one stream into chunks agree to 1e-12 of the largest bin, not to the bit,
    because two segments share a transform; continuous features follow to that accuracy, and
    ``peak`` and ``edge``, being bin-valued, may move to a neighbouring bin where two candidates
    are within it.

    Complex data, more than two dimensions, sizes that are not integers, ``step`` outside 1 ..
    ``winsize``, an unknown or empty ``features``, bad ``bands``, ``edge``, ``fmin`` or ``fmax``,
    an unknown ``scaling`` or ``detrend`` raise ``ValueError`` before the stream or the device is
    touched (a producer's complex chunks when the first one arrives); so does a stream shorter
    than ``winsize``.
    """
    who = "window_spectral"
    names = _stream._names(features, WINDOW_SPECTRAL, "window spectral feature(s)")
    W = _stream._size(winsize, 8, None, who, "winsize")
    if step is not None and not isinstance(step, bool) and isinstance(step, (int, np.integer)) and step > W:
        raise ValueError(f"window_spectral: step = {step} is larger than winsize = {W}: the segmenter has no gaps, "
                         "step must be from 1 to winsize")
    step = W if step is None else _stream._size(step, 1, W, who, "step")
    fs = _frequency(fs, "fs")
    if fs <= 0:
        raise ValueError(f"window_spectral: fs must be positive, got {fs!r}")
    if detrend not in _lib.DETREND:
        raise ValueError(f"window_spectral: detrend must be 'constant' or 'linear', got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"window_spectral: scaling must be 'density' or 'spectrum', got {scaling!r}")
    freqs = np.fft.rfftfreq(W, 1 / fs)
    k0, k1 = _bin_range(freqs, fmin, fmax)
    banded = "band" in names or "relative" in names
    if banded and bands is None:
        raise ValueError("window_spectral: 'band' and 'relative' need bands, a (lo, hi) pair or a sequence of pairs")
    bins, one_band = _band_bins(bands, freqs, k0, k1) if banded else ([], True)
    fracs, one_edge = _fractions(edge) if "edge" in names else ([], True)
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind)
    coeffs, scale = nm._window_and_scale(window, W, fs, scaling)
    nch, nfreq = layout.nch, W // 2 + 1
    df = float(fs) / W
    present = [f for f in WINDOW_SPECTRAL if f in names]     # the features a push writes, in the kernel's order
    mask = dev.spectral_mask(present)
    width = {f: len(bins) if f in ("band", "relative") else len(fracs) if f == "edge" else 1 for f in present}
    single = {"band": one_band, "relative": one_band, "edge": one_edge}
    where = {f: (sum(width[g] for g in present[:i]), None if single.get(f, True) else width[f])
             for i, f in enumerate(present)}
    nplanes = dev.spectral_planes(mask, len(bins), len(fracs))
    host = dev.origin_is_host(pro)
    torch = dev.torch
    cap = max(1, _SPECTRAL_PUSH_BYTES // (8 * nch * nfreq)) * step       # samples per push
    parts, spec = [], None
    try:
        for arr in dev.pull_resident(pro, pro):
            kind(_is_complex(arr), f"{arr.dtype} chunks")
            if spec is None:
                dev.require_gpu()
                spec = dev.SpecStream(W, W, step, coeffs, scale, detrend, _lib.SPEC_PSD_SEGMENTS, nch)
            x2d, was_host = layout.to2d(arr)
            host = host or was_host
            for at in range(0, x2d.shape[1], cap):
                P = spec.push(x2d[:, at:at + cap])           # (nseg, nch, nfreq); the handle keeps the tail
                nseg = P.shape[0]
                if nseg == 0:
                    continue
                if nm._linear_trend_refuses(P, detrend) is not None:
                    # (a least-squares trend refuses non-finite data: core/numerical.py:691)
                    raise ValueError(nm._REFUSED)
                out = torch.empty((nplanes, nch, nseg), dtype=torch.float64, device=P.device)
                dev.spectral_features(P, k0, k1, df, bins, fracs, normalize, mask, out)
                parts.append(out.cpu().numpy() if host else out)
    finally:
        if spec is not None:
            spec.close()
    if not parts:
        raise ValueError(f"window_spectral: the stream ended before one window of {W} samples was full")
    return _stream._result(parts, host, layout, features, names, where)
