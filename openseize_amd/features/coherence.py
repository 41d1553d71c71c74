"""window_coherence: sliding-window spectral connectivity (no counterpart in the reference) -- the
coherence, its imaginary part, the phase-locking value and the phase-lag indices of every channel
pair, per frequency band and per window of a stream: what ``coherence`` and ``phase_connectivity``
give for a whole stream, taken over each window's own Welch segments and averaged over the bins of
a band, from one pass.  The segments are cut and transformed once by ``csrc/spec.hip`` however many
windows share them; ``csrc/windowcoh.hip`` (K27), ``osz_window_coherence``, sums a window's segments
and folds the bins of a band on chip, so no (C, C, nfreq) array is ever held.
"""

import math

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core import numerical as nm
from openseize_amd.features import _stream
from openseize_amd.features._stream import _is_complex, _is_real

WINDOW_COHERENCE = tuple(_lib.WINDOW_COHERENCE)

# bytes of segment spectra one push may transform (they stay until the windows that read them are done)
_COHERENCE_PUSH_BYTES = 1 << 30

_WHO = "window_coherence"


def _grid(nperseg, overlap, winsize, step):
    """(h, nsub, m): the stride of the segments, the segments of a window and the segments between
    two windows, after the checks of ``nperseg``, ``overlap``, ``winsize`` and ``step``."""
    L = _stream._size(nperseg, 8, None, _WHO, "nperseg")
    if not _is_real(overlap) or not 0.0 <= overlap < 1.0:
        raise ValueError(f"{_WHO}: overlap must be a number in [0, 1), got {overlap!r}")
    h = L - int(L * overlap)
    W = _stream._size(winsize, 1, None, _WHO, "winsize")
    step = W if step is None else _stream._size(step, 1, None, _WHO, "step")
    nsub = (W - L) // h + 1 if W >= L else 0
    if nsub < 2 or L + (nsub - 1) * h != W or step % h:
        below = L + (max(nsub, 2) - 1) * h
        lower = max(h, step // h * h)
        raise ValueError(f"{_WHO}: a window is nsub >= 2 segments of nperseg = {L} samples, {h} apart, and step a "
                         f"multiple of that stride: winsize = {W} must be nperseg + (nsub - 1) {h} (the nearest are "
                         f"{below} and {below + h}) and step = {step} a positive multiple of {h} (the nearest are "
                         f"{lower} and {lower + h})")
    return h, nsub, step // h


def _bands(bands, freqs, last):
    """(pairs of bins [b0, b1), single) of ``bands``: one (lo, hi) pair or a sequence of 1 to
    _lib.WK_BANDS_MOST pairs; a band holds the bins with lo <= freqs[k] < hi (the rule of
    ``window_spectral``), all of them within 1 .. ``last``."""
    what = (f"{_WHO}: bands must be a (lo, hi) pair or a sequence of 1 to {_lib.WK_BANDS_MOST} pairs of finite "
            f"frequencies, got {bands!r}")
    if isinstance(bands, np.ndarray):
        bands = bands.tolist()
    if not isinstance(bands, (tuple, list)) or not bands:
        raise ValueError(what)
    single = len(bands) == 2 and all(_is_real(v) for v in bands)
    pairs = [bands] if single else list(bands)
    if not 1 <= len(pairs) <= _lib.WK_BANDS_MOST:
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
            raise ValueError(f"{_WHO}: the band ({lo:g}, {hi:g}) holds no bin (lo <= f < hi, the bins are "
                             f"{freqs[1] - freqs[0]:g} apart)")
        if b0 < 1 or b1 > last + 1:
            raise ValueError(f"{_WHO}: the band ({lo:g}, {hi:g}) does not lie within the bins {freqs[1]:g} .. "
                             f"{freqs[last]:g} where the spectrum of a real signal is complex (DC and the Nyquist bin "
                             "are real)")
        bins.append((b0, b1))
    return bins, single


def window_coherence(data, fs, winsize, step=None, measures=("coh",), bands=None, nperseg=None, overlap=0.5,
                     window="hann", detrend="constant", axis=-1, chunksize=None):
    """Spectral connectivity of every channel pair per frequency band and per window of ``winsize`` samples.

    ``data``, ``axis`` and ``chunksize`` are those of ``window_connectivity``: real two-dimensional
    data with C >= 2 channels, samples along ``axis`` -- an ndarray, a CUDA tensor or a producer.

    Segments are cut from the first sample of the stream exactly as ``csd`` cuts them: length
    ``nperseg`` (an integer >= 8, required), stride h = nperseg - int(nperseg overlap), ``overlap``
    in [0, 1), each detrended (``detrend``: "constant" or "linear"), multiplied by ``window``
    (``scipy.signal.get_window``) and transformed at nfft = nperseg.  The scaling is the density's
    and fixed: every measure is a ratio.  Every segment is transformed once, however many windows
    share it.  A window is a run of ``nsub`` >= 2 consecutive segments: ``winsize`` must equal
    nperseg + (nsub - 1) h, and ``step``, which defaults to ``winsize``, must be a positive multiple
    of h (else ``ValueError`` with the two nearest valid values).  With m = step / h, window k is the
    segments k m .. k m + nsub - 1: the samples k step .. k step + winsize - 1, whatever the chunks
    are; m < nsub overlaps the windows, m > nsub leaves gaps, and a trailing window the stream does
    not fill is dropped.

    ``bands`` is required: one (lo, hi) pair or a sequence of 1 to ``_lib.WK_BANDS_MOST`` (16) pairs
    of frequencies.  A band holds the bins f_k = k fs / nperseg with lo <= f_k < hi; bands may
    overlap, every band must hold a bin and lie within the bins 1 .. ceil(nperseg / 2) - 1, where the
    spectrum of a real signal is complex (DC and the Nyquist bin of an even ``nperseg`` are refused).

    ``measures`` is one name or a tuple of names of ``WINDOW_COHERENCE``.  Per bin of a window they
    are exactly the definitions of ``coherence`` and ``phase_connectivity`` applied to the window's
    N = nsub segments alone, with z_s = conj(X_i) X_j, d_s = Im z_s and all sums over the segments:

    ``"coh"``    |sum z|^2 / (sum |X_i|^2 sum |X_j|^2), the magnitude-squared coherence;
    ``"imcoh"``  Im sum z / sqrt(sum |X_i|^2 sum |X_j|^2);
    ``"plv"``    |sum z / |z|| / N;
    ``"pli"``    |sum sign d| / N;
    ``"wpli"``   |sum d| / sum |d|;
    ``"dwpli"``  ((sum d)^2 - sum d^2) / ((sum |d|)^2 - sum d^2).

    A band's value is the arithmetic mean of its bins' values (the ``faverage`` convention), not a
    measure of band-summed spectra.

    Returns ``(nwin, M)``: for one name M is float64 of shape (nwin, nbands, C, C), or (nwin, C, C)
    when ``bands`` is a single pair; for a tuple a dict of name -> such an array in the order asked,
    all from ONE pass over the stream.  Host data gives ndarrays, CUDA data CUDA tensors.

    Guarantees.  All measures but ``imcoh`` are symmetric bit for bit; ``imcoh[j, i]`` is the negated
    ``imcoh[i, j]``, a zero +0.0 on both sides.  The diagonal is written, not computed: 1.0 for
    ``coh`` and ``plv``, 0.0 for the rest.  A non-finite sample in channel c makes row and column c
    NaN, the diagonal included, in exactly the windows whose segments hold it, in every band and
    measure, and moves no other entry beyond what ``spec.hip`` promises (with ``detrend="linear"``
    non-finite data raise ``ValueError``, as ``csd`` does).  A zero denominator gives NaN, as IEEE
    does, and a channel without power in a bin of a band (a constant channel) is NaN in its row and
    column of ``coh``, ``imcoh`` and ``plv``, the diagonal included.  The segment spectra carry
    ``spec.hip``'s guarantee: different cuts of a stream agree to 1e-12 of the largest bin, not to
    the bit.  Given the spectra, the reduction is bit-reproducible: an entry's bits depend on nsub,
    the band's bins and the window's spectra of its own two channels only (the sums run in segment
    order, the band mean in bin order, nothing is atomic) -- not on ``step``, on which other
    channels, bands or measures were asked, nor on where a push or a launch was cut.

    Complex data, one-dimensional data, more than two dimensions, fewer than two channels, sizes
    that are not integers, a ``winsize`` or ``step`` that does not fit the segment grid, bad
    ``bands``, ``overlap`` outside [0, 1), an unknown ``detrend`` or ``window``, and unknown or empty
    ``measures`` raise ``ValueError`` before the stream or the device is touched (a producer's
    complex chunks when the first one arrives); so does a stream shorter than ``winsize``.

    Memory.  A push transforms at most about 1 GiB of segment spectra; between pushes the spectra of
    the segments that belong to unfinished windows stay on the device.  A launch writes at most
    1 GiB of results, 8 nbands C^2 bytes per window and measure; host-fed results come down launch
    by launch, CUDA-fed results stay on the device: when they do not fit the free device memory,
    ``MemoryError`` is raised before the first launch.
    """
    who = _WHO
    names = _stream._names(measures, WINDOW_COHERENCE, "window coherence measure(s)")
    if nperseg is None:
        raise ValueError(f"{who}: nperseg, the length of a segment, is required: an integer >= 8")
    h, nsub, m = _grid(nperseg, overlap, winsize, step)
    L, W = int(nperseg), int(winsize)
    if not _is_real(fs) or not math.isfinite(fs) or fs <= 0:
        raise ValueError(f"{who}: fs must be a positive finite number, got {fs!r}")
    if detrend not in _lib.DETREND:
        raise ValueError(f"{who}: detrend must be 'constant' or 'linear', got {detrend!r}")
    if bands is None:
        raise ValueError(f"{who}: bands is required, a (lo, hi) pair or a sequence of pairs")
    bins, one_band = _bands(bands, np.fft.rfftfreq(L, 1 / float(fs)), (L + 1) // 2 - 1)
    coeffs, scale = nm._window_and_scale(window, L, float(fs), "density")
    kind = _stream._real_only(who)
    pro, layout = _stream._open(who, data, axis, chunksize, W, kind, pairs=True)
    nch, nfreq, nb = layout.nch, L // 2 + 1, len(bins)
    order = [name for name in WINDOW_COHERENCE if name in names]      # the planes a launch writes
    mask = dev.name_mask(_lib.WINDOW_COHERENCE, order)
    window_bytes = 8 * len(order) * nb * nch * nch
    cap = max(1, _COHERENCE_PUSH_BYTES // (16 * nch * nfreq)) * h       # samples per push
    torch = dev.torch
    host = dev.origin_is_host(pro)
    parts, spec, carry, skip = [], None, None, 0
    try:
        for arr in dev.pull_resident(pro, pro):
            kind(_is_complex(arr), f"{arr.dtype} chunks")
            if spec is None:
                dev.require_gpu()
                spec = dev.SpecStream(L, L, h, coeffs, scale, detrend, _lib.SPEC_DFT_SEGMENTS, nch)
            x2d, was_host = layout.to2d(arr)
            host = host or was_host
            for at in range(0, x2d.shape[1], cap):
                X = spec.push(x2d[:, at:at + cap])             # (nseg, nch, nfreq); the handle keeps the tail
                if X.shape[0] == 0:
                    continue
                if nm._linear_trend_refuses(X, detrend) is not None:
                    # (a least-squares trend refuses non-finite data: core/numerical.py:691)
                    raise ValueError(nm._REFUSED)
                # the bookkeeping of _stream._launches on the segment axis: a window is nsub segments, m apart
                have = 0 if carry is None else carry.shape[0]
                drop, nwin, keep, skip = _stream._advance(have, skip, X.shape[0], nsub, m)
                if drop:
                    X = X[drop:]
                if carry is not None:
                    X = torch.cat((carry, X), dim=0)
                most = max(1, _stream._PUSH_BYTES // window_bytes)       # windows per launch
                for k0 in range(0, nwin, most):
                    k1 = min(k0 + most, nwin)
                    if not parts and not host:                 # (before the first launch)
                        expect = _stream.window_count((pro.shape[layout.axis] - L) // h + 1, nsub, m)
                        need, free = window_bytes * expect, torch.cuda.mem_get_info()[0]
                        if need > free:
                            raise MemoryError(f"{who}: the results of {expect} windows, {len(order)} x {nb} bands x "
                                              f"({nch}, {nch}) float64 each, need {need / 1e9:.2f} GB, more than the "
                                              f"{free / 1e9:.2f} GB of device memory that are free: raise step (now "
                                              f"{m * h}; winsize {W}), ask for fewer of the {nb} bands or select fewer "
                                              f"of the {nch} channels")
                    out = torch.empty((len(order), k1 - k0, nb, nch, nch), dtype=torch.float64, device=X.device)
                    dev.window_coherence(X[k0 * m:(k1 - 1) * m + nsub], nsub, m, bins, mask, out)
                    parts.append(out.cpu().numpy() if host else out)
                # (a copy: the spectra of a push are a new tensor, but a view would keep all of it)
                carry = X[X.shape[0] - keep:].clone() if keep else None
    finally:
        if spec is not None:
            spec.close()
    if not parts:
        raise ValueError(f"{who}: the stream ended before one window of {W} samples was full")
    planes = np.concatenate(parts, axis=1) if host else torch.cat(parts, dim=1)
    if one_band:
        planes = planes.reshape((len(order), planes.shape[1], nch, nch))
    found = {name: planes[p] for p, name in enumerate(order)}
    return planes.shape[1], _stream._asked(measures, names, found)
