"""psd / stft / csd / coherence: user API over the windowed-DFT path.

Same signatures and return values as reference spectra/estimators.py:59-156
(``psd`` -> (cnt, freqs, mean PSD)) and :160-284 (``stft`` -> (freqs, time,
X)).  ``psd`` keeps the segment average on the device: the ``osz_spec`` handle
accumulates the periodogram sum (K6) and the mean is taken once at the end --
mathematically the running mean of estimators.py:149-152.  ``csd`` and
``coherence`` have no counterpart in the reference: they are ``psd``'s Welch
average taken over every PAIR of channels (K10), with ``scipy.signal.csd`` /
``scipy.signal.coherence`` as the yardstick.
"""

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core import numerical as nm
from openseize_amd.core.producer import producer
from openseize_amd.core.resources import assignable


def _welch_plan(data, fs, axis, resolution, window, overlap, scaling):
    """What every Welch estimator here starts from: the producer (chunksize forced to
    ``int(fs)``, estimators.py:141, worked on as a coarse copy), nfft = int(fs / resolution)
    (:144), the segment stride, the window with its sqrt(norm) and the (channels, samples)
    layout.  Touches neither the stream nor the device."""
    pro = producer(data, chunksize=int(fs), axis=axis)
    pro = nm._coarse(pro, int(np.prod(pro.shape)) // max(pro.shape[axis], 1))
    nfft = int(fs / resolution)
    freqs = np.fft.rfftfreq(nfft, 1 / fs)
    stride = nfft - int(nfft * overlap)
    coeffs, scale = nm._window_and_scale(window, nfft, fs, scaling)
    axis_n = nm.normalize_axis(axis, len(pro.shape))
    return pro, nfft, freqs, stride, coeffs, scale, axis_n, dev.Layout(pro.shape, axis_n)


class _Feed:
    """The stream of ``pro`` as float64 (channels, samples) CUDA tensors, empty pieces left
    out; ``host`` says afterwards whether the estimate goes back as an ndarray."""

    def __init__(self, pro, axis_n, layout):
        self.pro, self.axis_n, self.layout, self.host = pro, axis_n, layout, True

    def __iter__(self):
        pro, layout, pipe = self.pro, self.layout, None
        for arr in dev.pull_resident(nm._batched(pro, self.axis_n, layout.nch), pro):
            if dev.is_tensor(arr):
                x2d, self.host = layout.to2d(arr)
            else:
                # host-fed: the next piece is staged (pinned ring, H2D stream)
                # while this one's segments are transformed
                pipe = pipe or dev.HostPipe(layout)
                x2d, self.host = pipe.feed(arr), True
            if x2d.shape[1]:
                yield x2d
        # a chain of this library's producers over host data hands CUDA tensors to
        # this loop (dev.pull_resident); the estimate still goes back as an ndarray
        self.host = self.host or dev.origin_is_host(pro)


def psd(data, fs, axis=-1, resolution=0.5, window="hann", overlap=0.5,
        detrend="constant", scaling="density"):
    """Welch power spectrum (density) estimate.  chunksize is forced to
    ``int(fs)`` (estimators.py:141) and nfft = int(fs / resolution) (:144)."""
    pro, nfft, freqs, stride, coeffs, scale, axis_n, layout = _welch_plan(
        data, fs, axis, resolution, window, overlap, scaling)
    spec = dev.SpecStream(nfft, nfft, stride, coeffs, scale, detrend,
                          _lib.SPEC_PSD_MEAN, layout.nch)
    feed = _Feed(pro, axis_n, layout)
    try:
        for x2d in feed:
            spec.push(x2d)
        host = feed.host
        # device input: the average is taken on the device and stays there
        cnt, mean = spec.mean() if host else spec.mean_device()
    finally:
        spec.close()
    if nm._linear_trend_refuses(mean[None], detrend) is not None:
        # (a least-squares trend refuses non-finite data in the reference: core/numerical.py:691)
        raise ValueError(nm._REFUSED)
    if cnt == 0:
        # the reference's loop variable is unbound here (estimators.py:156)
        raise UnboundLocalError(
            "no complete segment: data is shorter than nfft = int(fs/resolution)")
    result = mean.reshape(layout.other + (mean.shape[-1],))
    if host:
        return cnt, freqs, np.moveaxis(result, -1, axis_n)
    return cnt, freqs, result.movedim(-1, axis_n).contiguous()


# bytes of segment spectra one push may write (osz_cross_accumulate reads them once and they go)
_CROSS_PUSH_BYTES = 1 << 30


def _cross_sums(data, fs, axis, resolution, window, overlap, detrend, scaling):
    """-> (cnt, freqs, raw sums (C, C, nfreq) complex128 on the device [i <= j filled], nfft,
    host): the Welch loop ``csd`` and ``coherence`` share."""
    pro, nfft, freqs, stride, coeffs, scale, axis_n, layout = _welch_plan(
        data, fs, axis, resolution, window, overlap, scaling)
    if len(pro.shape) == 1:
        raise ValueError("cross-spectra need two-dimensional data (channels x samples); "
                         "for a single channel use psd")
    if len(pro.shape) != 2:
        raise ValueError(f"cross-spectra need two-dimensional data (channels x samples), got shape "
                         f"{tuple(pro.shape)}: reshape the channel axes into one")
    if detrend not in _lib.DETREND:
        raise ValueError("Trend type must be 'linear' or 'constant'.")
    if pro.shape[axis_n] < nfft:
        raise ValueError(f"no complete segment: {pro.shape[axis_n]} samples along axis {axis_n} are fewer "
                         f"than nfft = int(fs / resolution) = {nfft}")
    nch, nfreq = layout.nch, nfft // 2 + 1
    if dev.origin_is_host(pro):
        _host_result_fits(nch, nfreq)            # (before any work is done for it)
    dev.require_gpu()
    spec = dev.SpecStream(nfft, nfft, stride, coeffs, scale, detrend, _lib.SPEC_DFT_SEGMENTS, nch)
    feed = _Feed(pro, axis_n, layout)
    cap = max(1, _CROSS_PUSH_BYTES // (16 * nch * nfreq)) * stride
    cnt = 0
    try:
        acc = dev.zeros((nch, nch, nfreq), dev.torch.complex128)
        for x2d in feed:
            for at in range(0, x2d.shape[1], cap):
                X = spec.push(x2d[:, at:at + cap])         # (nseg, nch, nfreq), the handle keeps the tail
                if X.shape[0] == 0:
                    continue
                if nm._linear_trend_refuses(X, detrend) is not None:
                    # (a least-squares trend refuses non-finite data: core/numerical.py:691)
                    raise ValueError(nm._REFUSED)
                dev.cross_accumulate(X, acc)
                cnt += X.shape[0]
    finally:
        spec.close()
    if cnt == 0:
        raise ValueError(f"no complete segment: the stream ended before nfft = int(fs / resolution) = {nfft} "
                         "samples")
    return cnt, freqs, acc, nfft, feed.host


def _host_result_fits(nch, nfreq):
    shape = (nch, nch, nfreq)
    if not assignable(shape, dtype=complex, msg=False):
        raise MemoryError(f"the {shape} complex128 result needs {16 * nch * nch * nfreq / 1e9:.2f} GB of host "
                          "memory, more than is available: select fewer channels or lower the resolution")


def csd(data, fs, axis=-1, resolution=0.5, window="hann", overlap=0.5,
        detrend="constant", scaling="density"):
    """Welch cross-spectral (density) estimate over all channel pairs.

    ``data`` is anything ``producer`` takes, two-dimensional: samples along ``axis``, the C
    channels along the other axis.  Segments are cut as in ``psd`` (nfft = int(fs /
    resolution), stride = nfft - int(nfft * overlap), a trailing partial segment dropped).
    Returns ``(cnt, freqs, S)``: S is complex128 (C, C, nfreq) whatever ``axis`` was, S[i, j] the
    mean over the ``cnt`` segments of conj(X_i) X_j, one-sided -- ``scipy.signal.csd(x[i], x[j],
    fs, window, nperseg=nfft, noverlap=int(nfft * overlap), nfft=nfft, detrend=detrend,
    scaling=scaling)``.  S[j, i] is conj(S[i, j]) bit for bit and the diagonal, which is
    ``psd``, has imaginary part 0.0.  Host data gives an ndarray, CUDA data a CUDA tensor.

    With ``detrend="constant"`` a non-finite sample in channel k makes row and column k NaN and
    leaves every other pair as it is without it; ``detrend="linear"`` raises ``ValueError`` then.

    Device memory: the (C, C, nfreq) sums, and per push the segment spectra of at most
    ``max(1, 2**30 // (16 C nfreq))`` strides of samples per channel (one more segment than
    that many at most, about 1 GiB) -- it does not grow with the stream.  The sums of a
    (segment, pair, bin) are added in segment order, so the estimate does not depend on how
    the stream is cut into chunks, and two calls give the same bits.
    """
    cnt, freqs, acc, nfft, host = _cross_sums(data, fs, axis, resolution, window, overlap,
                                              detrend, scaling)
    if host:
        _host_result_fits(acc.shape[0], acc.shape[2])
    S = dev.cross_finish(acc, cnt, nfft, _lib.CROSS_SPECTRUM)
    return cnt, freqs, S.cpu().numpy() if host else S


def coherence(data, fs, axis=-1, resolution=0.5, window="hann", overlap=0.5,
              detrend="constant"):
    """Magnitude-squared coherence |S_ij|^2 / (S_ii S_jj) of the Welch cross-spectra of
    ``csd`` (same arguments; the scaling cancels, as in ``scipy.signal.coherence``).
    Returns ``(cnt, freqs, C)`` with C float64 (C, C, nfreq), symmetric; a bin where an
    auto-spectrum is 0 is NaN, as it is in SciPy."""
    cnt, freqs, acc, nfft, host = _cross_sums(data, fs, axis, resolution, window, overlap,
                                              detrend, "density")
    if host:
        _host_result_fits(acc.shape[0], acc.shape[2])
    C = dev.cross_finish(acc, cnt, nfft, _lib.CROSS_COHERENCE)
    return cnt, freqs, C.cpu().numpy() if host else C


def stft(data, fs, axis=-1, resolution=0.5, window="hann", overlap=0.5,
         detrend="constant", scaling="density", boundary=True, padded=True,
         asarray=True):
    """Short-time Fourier transform (estimators.py:160-284).  With
    ``asarray`` the per-segment estimates are stacked on a new last axis when
    they fit in memory (:279-282), else a producer is returned."""
    pro = producer(data, chunksize=int(fs), axis=axis)
    pro = nm._coarse(pro, int(np.prod(pro.shape)) // max(pro.shape[axis], 1))
    nfft = int(fs / resolution)
    freqs, time, result = nm.stft(pro, fs, nfft, window, overlap, axis,
                                  detrend, scaling, boundary, padded)
    if asarray:
        if assignable(result.shape):
            result = dev.stack(list(result), axis=-1)
    return freqs, time, result
