"""psd / stft / csd / coherence / phase_connectivity: user API over the windowed-DFT path.

Same signatures and return values as reference spectra/estimators.py:59-156
(``psd`` -> (cnt, freqs, mean PSD)) and :160-284 (``stft`` -> (freqs, time,
X)).  ``psd`` keeps the segment average on the device: the ``osz_spec`` handle
accumulates the periodogram sum (K6) and the mean is taken once at the end --
mathematically the running mean of estimators.py:149-152.  ``csd`` and
``coherence`` have no counterpart in the reference: they are ``psd``'s Welch
average taken over every PAIR of channels (K10), with ``scipy.signal.csd`` /
``scipy.signal.coherence`` as the yardstick.  ``phase_connectivity`` (K11) takes the
phase-based measures (imcoh, plv, pli, wpli, dwpli) from the same segments, and ``jackknife``
(K12) gives coherence and those five their delete-one standard errors in a second pass.
``bispectrum`` and ``bicoherence`` (K14) are the third-order Welch average of every channel by
itself, X(f1) X(f2) conj X(f1 + f2) over a band of bin pairs, from the same segments.
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


def _cross_stream(data, fs, axis, resolution, window, overlap, detrend, scaling, begin, arrays=1,
                  at_least=1, per_channel=None):
    """The Welch loop over all channel pairs that ``csd``, ``coherence`` and
    ``phase_connectivity`` share.  Checks the arguments (touching neither the stream nor the
    device), then calls ``begin(nch, nfreq)`` once -- it allocates the sums and returns the
    function every push's (nseg, nch, nfreq) complex128 spectra are handed to, which may
    overwrite them.  ``arrays``: how many complex128 (C, C, nfreq) arrays' worth of host memory
    the result takes; ``at_least``: the segments the data's shape must promise.
    ``per_channel``: None for the estimators over channel PAIRS, or what a per-channel estimator
    (``bispectrum``) changes -- one-dimensional data is one channel (noted in ``flat``), and the object's
    ``host_fits(nch)`` / ``device_fits(nch)`` (the latter right after the device is found) and
    ``push_bytes`` (device bytes a push takes per (segment, channel, bin)) replace the pairs'.
    -> (cnt, freqs, nfft, host)."""
    pro, nfft, freqs, stride, coeffs, scale, axis_n, layout = _welch_plan(
        data, fs, axis, resolution, window, overlap, scaling)
    if per_channel is not None:
        per_channel.flat = len(pro.shape) == 1
        if len(pro.shape) > 2:
            raise ValueError(f"the bispectrum needs one- or two-dimensional data (channels x samples), got shape "
                             f"{tuple(pro.shape)}: reshape the channel axes into one")
    elif len(pro.shape) == 1:
        raise ValueError("cross-spectra need two-dimensional data (channels x samples); "
                         "for a single channel use psd")
    elif len(pro.shape) != 2:
        raise ValueError(f"cross-spectra need two-dimensional data (channels x samples), got shape "
                         f"{tuple(pro.shape)}: reshape the channel axes into one")
    if detrend not in _lib.DETREND:
        raise ValueError("Trend type must be 'linear' or 'constant'.")
    if pro.shape[axis_n] < nfft:
        raise ValueError(f"no complete segment: {pro.shape[axis_n]} samples along axis {axis_n} are fewer "
                         f"than nfft = int(fs / resolution) = {nfft}")
    if (pro.shape[axis_n] - nfft) // stride + 1 < at_least:
        raise ValueError(f"the jackknife needs at least two segments: {pro.shape[axis_n]} samples along axis "
                         f"{axis_n} hold one of nfft = {nfft} at a stride of {stride}")
    nch, nfreq = layout.nch, nfft // 2 + 1
    host_fits = (lambda: _host_result_fits(nch, nfreq, arrays)) if per_channel is None else (
        lambda: per_channel.host_fits(nch))
    if dev.origin_is_host(pro):
        host_fits()                              # (before any work is done for it)
    dev.require_gpu()
    if per_channel is not None:
        per_channel.device_fits(nch)
    spec = dev.SpecStream(nfft, nfft, stride, coeffs, scale, detrend, _lib.SPEC_DFT_SEGMENTS, nch)
    feed = _Feed(pro, axis_n, layout)
    push_bytes = 16 if per_channel is None else per_channel.push_bytes
    cap = max(1, _CROSS_PUSH_BYTES // (push_bytes * nch * nfreq)) * stride
    cnt = 0
    try:
        each = begin(nch, nfreq)
        for x2d in feed:
            for at in range(0, x2d.shape[1], cap):
                X = spec.push(x2d[:, at:at + cap])         # (nseg, nch, nfreq), the handle keeps the tail
                if X.shape[0] == 0:
                    continue
                if nm._linear_trend_refuses(X, detrend) is not None:
                    # (a least-squares trend refuses non-finite data: core/numerical.py:691)
                    raise ValueError(nm._REFUSED)
                each(X)
                cnt += X.shape[0]
    finally:
        spec.close()
    if cnt == 0:
        raise ValueError(f"no complete segment: the stream ended before nfft = int(fs / resolution) = {nfft} "
                         "samples")
    if feed.host:
        host_fits()
    return cnt, freqs, nfft, feed.host


def _cross_sums(data, fs, axis, resolution, window, overlap, detrend, scaling):
    """-> (cnt, freqs, raw sums (C, C, nfreq) complex128 on the device [i <= j filled], nfft,
    host): what ``csd`` and ``coherence`` take from the loop."""
    sums = []

    def begin(nch, nfreq):
        acc = dev.zeros((nch, nch, nfreq), dev.torch.complex128)
        sums.append(acc)
        return lambda X: dev.cross_accumulate(X, acc)

    cnt, freqs, nfft, host = _cross_stream(data, fs, axis, resolution, window, overlap, detrend,
                                           scaling, begin)
    return cnt, freqs, sums[0], nfft, host


def _host_result_fits(nch, nfreq, arrays=1):
    shape = (nch, nch, nfreq)
    if not assignable((arrays,) + shape, dtype=complex, msg=False):
        raise MemoryError(f"the {shape} complex128 result needs {arrays * 16 * nch * nch * nfreq / 1e9:.2f} GB of "
                          "host memory, more than is available: select fewer channels or lower the resolution")


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
    C = dev.cross_finish(acc, cnt, nfft, _lib.CROSS_COHERENCE)
    return cnt, freqs, C.cpu().numpy() if host else C


PHASE_METHODS = tuple(_lib.PHASE_MODE)        # ("imcoh", "plv", "pli", "wpli", "dwpli")


def _phase_methods(method):
    names = (method,) if isinstance(method, str) or not isinstance(method, (tuple, list)) else tuple(method)
    bad = [m for m in names if not isinstance(m, str) or m not in PHASE_METHODS]
    if bad or not names:
        raise ValueError(f"unknown phase connectivity method(s) {bad}: choose from {PHASE_METHODS}")
    return names


def phase_connectivity(data, fs, method="wpli", axis=-1, resolution=0.5, window="hann",
                       overlap=0.5, detrend="constant"):
    """Phase-based connectivity over all channel pairs, from the Welch segments of ``csd``.

    ``data``, the segment cutting and the argument errors are those of ``csd`` (nfft = int(fs /
    resolution), stride = nfft - int(nfft * overlap), a trailing partial segment dropped;
    two-dimensional data, samples along ``axis``).  ``method`` is one name or a tuple of names;
    with X[s, c, f] the segment spectra, z_s = conj(X_i) X_j, d_s = Im z_s and N = cnt:

    ``"imcoh"``  Im(sum z_s) / sqrt(sum |X_i|^2 sum |X_j|^2), the imaginary part of coherency
                 (Nolte et al. 2004); antisymmetric, M[j, i] = -M[i, j];
    ``"plv"``    |sum z_s / |z_s|| / N, the phase-locking value in its spectral form (Lachaux et
                 al. 1999);
    ``"pli"``    |sum sign(d_s)| / N, the phase-lag index (Stam et al. 2007);
    ``"wpli"``   |sum d_s| / sum |d_s|, the weighted phase-lag index (Vinck et al. 2011);
    ``"dwpli"``  ((sum d_s)^2 - sum d_s^2) / ((sum |d_s|)^2 - sum d_s^2), its debiased square.

    Returns ``(cnt, freqs, M)``: for one name M is float64 (C, C, nfreq) whatever ``axis`` was,
    for a tuple a dict of name -> such an array, every measure from ONE pass over the stream and
    bit-identical to the single-name call.  Host data gives ndarrays, CUDA data CUDA tensors.
    All but imcoh are symmetric, bit for bit; imcoh's mirror is the negated value.

    Fixed points, written and not computed: the diagonal is 1.0 for plv and 0.0 for the others;
    at f = 0, and at the Nyquist bin when nfft is even, the spectra are real, and imcoh, pli,
    wpli and dwpli are 0.0 there (both mirrors +0.0).  ``plv`` at f = 0 is NOT fixed: under
    detrending X[s, c, 0] is what rounding left of a removed mean, and plv there is the phase
    of rounding noise (a channel whose X is exactly 0 in a segment gives NaN, 0 / 0).  NaN
    overrides the fixed points: where a channel's own sums are NaN, its row and column are.
    Elsewhere a zero denominator gives NaN, as IEEE does.

    With ``detrend="constant"`` a non-finite sample in channel k makes row and column k NaN and
    leaves every other pair as it is without it; ``detrend="linear"`` raises ``ValueError`` then.

    Device memory: per (pair, bin) 16 B of complex sums for imcoh, 16 B for plv (the sums of the
    unit phasors X / |X|, since z / |z| = conj(X_i / |X_i|) X_j / |X_j|) and 32 B for pli, wpli
    and dwpli together (sum d, sum |d|, sum d^2, sum sign d) -- only what the requested methods
    need, up to 64 B per (pair, bin) with everything requested -- plus 8 B per returned measure
    and per push the segment spectra ``csd`` documents (about 1 GiB at most).  Every sum is added
    in segment order: the estimate does not depend on how the stream is cut into chunks, and two
    calls give the same bits.
    """
    names = _phase_methods(method)
    need_acc, need_plv = "imcoh" in names, "plv" in names
    need_lag = any(m in names for m in ("pli", "wpli", "dwpli"))
    sums = {}

    def begin(nch, nfreq):
        if need_acc:
            sums["acc"] = dev.zeros((nch, nch, nfreq), dev.torch.complex128)
        if need_plv:
            sums["accn"] = dev.zeros((nch, nch, nfreq), dev.torch.complex128)
        if need_lag:
            sums["lag"] = dev.zeros((4, nch, nch, nfreq), dev.torch.float64)

        def each(X):
            if need_lag:
                dev.lag_accumulate(X, sums["lag"])
            if need_acc:
                dev.cross_accumulate(X, sums["acc"])
            if need_plv:
                # last: the normalisation overwrites the push's spectra
                dev.cross_accumulate(dev.unit_phasors(X), sums["accn"])
        return each

    # (float64 results: two of them take one complex128 array's worth of host memory)
    cnt, freqs, nfft, host = _cross_stream(data, fs, axis, resolution, window, overlap, detrend,
                                           "density", begin, arrays=(len(set(names)) + 1) // 2)
    out = {}
    for m in names:
        if m not in out:
            M = dev.phase_finish(m, cnt, nfft, **sums)
            out[m] = M.cpu().numpy() if host else M
    return cnt, freqs, out[names[0]] if isinstance(method, str) else out


JACKKNIFE_METHODS = ("coherence",) + PHASE_METHODS


def _jackknife_methods(method):
    names = (method,) if isinstance(method, str) or not isinstance(method, (tuple, list)) else tuple(method)
    bad = [m for m in names if not isinstance(m, str) or m not in JACKKNIFE_METHODS]
    if bad or not names:
        raise ValueError(f"unknown jackknife method(s) {bad}: choose from {JACKKNIFE_METHODS}")
    return names


def jackknife(data, fs, method="coherence", axis=-1, resolution=0.5, window="hann", overlap=0.5,
              detrend="constant"):
    """Coherence and phase connectivity over all channel pairs with their delete-one jackknife
    standard errors over the Welch segments (Thomson & Chave 1991; Bokil et al. 2007).

    ``data``, the segment cutting and the argument errors are those of ``csd``; ``method`` is one
    of ``JACKKNIFE_METHODS`` = ``("coherence",) + PHASE_METHODS`` or a tuple of them.  Returns
    ``(cnt, freqs, estimate, stderr)``: ``estimate`` is bit for bit what ``coherence`` /
    ``phase_connectivity`` return for the same arguments, ``stderr`` is float64 (C, C, nfreq); a
    tuple of names gives two dicts of name -> array.  Host data gives ndarrays, CUDA data CUDA
    tensors.  Fewer than two segments raise ``ValueError`` (at least two segments are needed),
    before the stream is started when the data's shape tells.

    Definition.  With N = cnt segments, theta the measure from all of them, theta_(s) the
    measure with segment s left out and d_s = theta_(s) - theta,

        stderr^2 = (N - 1) / N (sum_s d_s^2 - (sum_s d_s)^2 / N),   clamped at 0,

    the deviations taken from theta (the theta_(s) differ by O(1 / N): their own squares would
    cancel).  The subtraction itself carries up to (3 N + 1) roundings of sum d_s^2: a difference
    that does not exceed 4 N 2^-53 sum d_s^2 is written as 0 -- the theta_(s) are then equal to
    within rounding, as with two segments, where coherence, plv, pli and wpli of the one segment
    left are 1 whichever is left out.  Every measure is a function of sums over the segments, so theta_(s) is that
    function of the totals minus segment s's contribution: with z_s = conj(X_i) X_j, d = Im z_s,
    p_i = |X_i|^2, u_s = z_s / |z_s| and the totals A = sum z, P = sum p, U = sum u, D = sum d,
    B = sum |d|, Q = sum d^2, G = sum sign d,

    ``"coherence"``  |A - z_s|^2 / ((P_i - p_i)(P_j - p_j))
    ``"imcoh"``      Im(A - z_s) / sqrt((P_i - p_i)(P_j - p_j))
    ``"plv"``        |U - u_s| / (N - 1)
    ``"pli"``        |G - sign d| / (N - 1)
    ``"wpli"``       |D - d| / (B - |d|)
    ``"dwpli"``      ((D - d)^2 - (Q - d^2)) / ((B - |d|)^2 - (Q - d^2))

    A zero denominator gives NaN or inf, as IEEE does; with N = 2 dwpli's theta_(s) is 0 / 0
    everywhere (written as NaN, not left to the rounding of the downdate) and so is its stderr.
    Overlapping segments are not independent: with
    ``overlap`` > 0 the jackknife treats correlated segments as independent draws and
    understates the error; ``overlap=0`` gives the textbook jackknife.  No bias correction and no
    variance-stabilising transform is applied; ``metrics.jackknife_interval`` turns ``stderr``
    into a Student-t interval.

    Two passes over ``data``, which must give the same stream twice (``RuntimeError`` if the
    passes count different numbers of segments).  Pass 1 is ``coherence`` /
    ``phase_connectivity``: the totals and the estimates.  Pass 2 cuts the same segments again
    and per push adds d_s and d_s^2 of every (pair, bin) in segment order from the stored sums:
    ``stderr`` has the same bits however the stream is chunked and two calls give the same bits.
    It costs about what pass 1 costs with one kernel launch per method and push, plus the second
    read of the stream.

    Fixed points, written and not computed: the diagonal of ``stderr`` is 0.0; for every method
    but plv it is 0.0 at f = 0, and at the Nyquist bin when nfft is even (the phase measures are
    the constant 0 there; coherence at a real bin is a correlation of real numbers, with half the
    degrees of freedom of the other bins, and gets no error bar).  NaN overrides them, as in
    ``phase_connectivity``: with ``detrend="constant"`` a non-finite sample in channel k makes row
    and column k of ``estimate`` and ``stderr`` NaN and leaves every other pair's bits as they
    are; ``detrend="linear"`` raises ``ValueError`` then.  ``stderr`` is symmetric bit for bit
    for every method (imcoh's deviations change sign together).

    Device memory: the totals of ``phase_connectivity`` (16 B per (pair, bin) for coherence and
    imcoh together, 16 B for plv, 32 B for pli, wpli and dwpli together), plus 16 B per (pair,
    bin) per method for the two running sums, 8 B per returned array and per push the segment
    spectra ``csd`` documents.
    """
    names = _jackknife_methods(method)
    need_acc = any(m in names for m in ("coherence", "imcoh"))
    need_plv = "plv" in names
    need_lag = any(m in names for m in ("pli", "wpli", "dwpli"))
    order = sorted(set(names), key=lambda m: (m == "plv", JACKKNIFE_METHODS.index(m)))   # plv last
    sums, dev2 = {}, {}

    def totals(nch, nfreq):
        if need_acc:
            sums["acc"] = dev.zeros((nch, nch, nfreq), dev.torch.complex128)
        if need_plv:
            sums["accn"] = dev.zeros((nch, nch, nfreq), dev.torch.complex128)
        if need_lag:
            sums["lag"] = dev.zeros((4, nch, nch, nfreq), dev.torch.float64)

        def each(X):
            if need_lag:
                dev.lag_accumulate(X, sums["lag"])
            if need_acc:
                dev.cross_accumulate(X, sums["acc"])
            if need_plv:
                # last: the normalisation overwrites the push's spectra
                dev.cross_accumulate(dev.unit_phasors(X), sums["accn"])
        return each

    # (an estimate and its stderr, float64 both, take one complex128 array's worth of host memory)
    args = (data, fs, axis, resolution, window, overlap, detrend, "density")
    cnt, freqs, nfft, host = _cross_stream(*args, totals, arrays=len(order), at_least=2)
    if cnt < 2:
        raise ValueError(f"the jackknife needs at least two segments: the stream held {cnt}")
    estimate = {}
    for m in order:
        M = (dev.cross_finish(sums["acc"], cnt, nfft, _lib.CROSS_COHERENCE) if m == "coherence"
             else dev.phase_finish(m, cnt, nfft, **sums))
        estimate[m] = M.cpu().numpy() if host else M

    def deviations(nch, nfreq):
        for m in order:
            dev2[m] = dev.zeros((2, nch, nch, nfreq), dev.torch.float64)

        def each(X):
            for m in order:
                if m == "plv":
                    dev.unit_phasors(X)          # last: the normalisation overwrites the push's spectra
                dev.jackknife_accumulate(m, X, cnt, dev2[m], **sums)
        return each

    again, _, _, _ = _cross_stream(*args, deviations, arrays=len(order), at_least=2)
    if again != cnt:
        raise RuntimeError(f"the two passes of the jackknife counted {cnt} and {again} segments: the data "
                           "must give the same stream every time it is iterated")
    stderr = {}
    for m in order:
        E = dev.jackknife_finish(m, dev2.pop(m), cnt, nfft, **sums)
        stderr[m] = E.cpu().numpy() if host else E
    if isinstance(method, str):
        return cnt, freqs, estimate[method], stderr[method]
    return cnt, freqs, {m: estimate[m] for m in names}, {m: stderr[m] for m in names}


BICOHERENCE_METHODS = tuple(m for m in _lib.BISPEC_MODE if m != "spectrum")        # ("kim", "hagihira")


def _bicoherence_methods(method):
    names = (method,) if isinstance(method, str) or not isinstance(method, (tuple, list)) else tuple(method)
    bad = [m for m in names if not isinstance(m, str) or m not in BICOHERENCE_METHODS]
    if bad or not names:
        raise ValueError(f"unknown bicoherence method(s) {bad}: choose from {BICOHERENCE_METHODS}")
    return names


class _BispecPlan:
    """The band of ``bispectrum`` / ``bicoherence`` and what ``_cross_stream`` asks a per-channel
    estimator: the memory checks and the bytes of a push.  Touches neither stream nor device."""

    push_bytes = 24        # 16 B of spectra and the 8 B of the plane |X| per (segment, channel, bin)

    def __init__(self, fs, resolution, fmin, fmax, out_bytes):
        nfft = int(fs / resolution)
        freqs = np.fft.rfftfreq(nfft, 1 / fs)
        if fmin is not None and fmax is not None and fmin > fmax:
            raise ValueError(f"fmin = {fmin} is above fmax = {fmax}")
        inside = np.ones(freqs.size, dtype=bool)
        if fmin is None:
            inside[:1] = False       # DC: under detrending what rounding left of a removed mean
        else:
            inside &= freqs >= fmin
        if fmax is not None:
            inside &= freqs <= fmax
        bins = np.flatnonzero(inside)
        if bins.size == 0:
            raise ValueError(f"no bin of the {freqs.size} (spacing {fs / nfft:g} Hz) lies in the band "
                             f"fmin = {fmin}, fmax = {fmax}")
        self.k_lo, self.nb, self.out_bytes = int(bins[0]), int(bins.size), out_bytes
        self.freqs = freqs[self.k_lo:self.k_lo + self.nb]

    def _refuse(self, nch, what, need, have):
        raise MemoryError(f"the bispectral {what} of {nch} channel(s) x {self.nb} x {self.nb} band-bin pairs need "
                          f"{need / 1e9:.2f} GB, more than the {have} available: lower fmax (the pairs grow "
                          "with the square of the band) or select fewer channels")

    def host_fits(self, nch):
        if not assignable((self.out_bytes // 8, nch, self.nb, self.nb), dtype=float, msg=False):
            self._refuse(nch, "results", self.out_bytes * nch * self.nb ** 2, "host memory")

    def device_fits(self, nch):
        need = (32 + self.out_bytes) * nch * self.nb ** 2           # the four sums and the results
        free = dev.torch.cuda.mem_get_info()[0]
        if need > free:
            self._refuse(nch, "sums (32 B per channel and pair) and results", need,
                         f"{free / 1e9:.2f} GB of device memory")


def _bispec_sums(plan, data, fs, axis, resolution, window, overlap, detrend, scaling):
    """-> (cnt, sums (4, C, nb, nb) and power (C, nfreq) on the device, host): what ``bispectrum`` and ``bicoherence`` take from the Welch loop."""
    kept = []

    def begin(nch, nfreq):
        sums = dev.zeros((4, nch, plan.nb, plan.nb), dev.torch.float64)
        power = dev.zeros((nch, nfreq), dev.torch.float64)
        kept.extend((sums, power))
        return lambda X: dev.bispec_accumulate(X, plan.k_lo, plan.nb, sums, power)

    cnt, _, _, host = _cross_stream(data, fs, axis, resolution, window, overlap, detrend, scaling, begin,
                                    per_channel=plan)
    return cnt, kept[0], kept[1], host


def _bispec_result(M, host, flat):
    M = M[0] if flat else M
    return M.cpu().numpy() if host else M


def bispectrum(data, fs, axis=-1, resolution=0.5, window="hann", overlap=0.5,
               detrend="constant", scaling="density", fmin=None, fmax=None):
    """Welch-averaged bispectrum of every channel: quadratic phase coupling between the rhythms
    at f1, f2 and f1 + f2.

    ``data`` is anything ``producer`` takes, one-dimensional (one channel) or two-dimensional
    (samples along ``axis``, the C channels along the other axis).  Segments are cut as in ``psd``
    and ``csd`` (nfft = int(fs / resolution), stride = nfft - int(nfft * overlap), a trailing
    partial segment dropped) and X[s, c, k] is the segment spectrum ``csd`` sums: detrended,
    windowed, ``rfft``, times the square root of the scaling's norm.

    The band is the bins k with fmin <= freqs[k] <= fmax; ``fmin=None`` starts at bin 1 (DC is
    under detrending what rounding left of a removed mean; ``fmin=0`` includes it), ``fmax=None``
    ends at the last bin.  With the band's nb bins k_lo .. k_lo + nb - 1, returns ``(cnt, freqs,
    B)``: ``freqs`` those nb frequencies and B complex128 (C, nb, nb) whatever ``axis`` was, (nb,
    nb) for one-dimensional data,

        B[c, a, b] = (1 / cnt) sum_s X[s, c, k1] X[s, c, k2] conj(X[s, c, k1 + k2]),
        k1 = k_lo + a, k2 = k_lo + b

    with the third factor read from the whole spectrum (k1 + k2 need not lie in the band) and no
    one-sided doubling.  B is symmetric in (a, b) bit for bit (k2 <= k1 is computed, both mirrors
    are written); entries with k1 + k2 > nfft // 2 lie outside the principal domain of a real
    signal and are NaN, written and not computed.  Host data gives an ndarray, CUDA data a CUDA
    tensor.

    With ``detrend="constant"`` a non-finite sample in channel k makes channel k's entries NaN and
    leaves every other channel's bits alone; ``detrend="linear"`` raises ``ValueError`` then.

    Device memory: 32 B of sums per channel and band-bin pair (nb^2 of them: ``MemoryError``,
    before anything is computed, when they or the result do not fit -- lower ``fmax`` or select
    fewer channels), and per push the segment spectra and the plane |X| of at most ``max(1,
    2**30 // (24 C nfreq))`` strides of samples per channel (about 1 GiB) -- it does not grow with
    the stream.  Every sum is added in segment order, no atomics: the estimate does not depend on
    how the stream is cut into chunks, and two calls give the same bits.
    """
    plan = _BispecPlan(fs, resolution, fmin, fmax, 16)
    cnt, sums, power, host = _bispec_sums(plan, data, fs, axis, resolution, window, overlap, detrend, scaling)
    B = dev.bispec_finish("spectrum", cnt, plan.k_lo, sums, power)
    return cnt, plan.freqs, _bispec_result(B, host, plan.flat)


def bicoherence(data, fs, method="kim", axis=-1, resolution=0.5, window="hann",
                overlap=0.5, detrend="constant", fmin=None, fmax=None):
    """Bicoherence of every channel: the bispectrum of ``bispectrum`` (same data, segments, band
    and argument errors) normalised to [0, 1].  ``method`` is one name or a tuple of names; with
    X1, X2, X3 = X[s, c, k1], X[s, c, k2], X[s, c, k1 + k2] and T = X1 X2 conj(X3):

    ``"kim"``       |sum T|^2 / (sum |X1 X2|^2 sum |X3|^2), the squared bicoherence of Kim & Powers
                    (1979); at most 1 by Cauchy-Schwarz;
    ``"hagihira"``  |sum T| / sum |T|, the amplitude-normalised bicoherence (Hagihira et al. 2001);
                    at most 1 by the triangle inequality, and kim <= hagihira^2.

    The scaling cancels in both.  Returns ``(cnt, freqs, M)``: for one name M is float64 with the
    shape of ``bispectrum``'s B, for a tuple a dict of name -> such an array in the order asked,
    every measure from ONE pass over the stream and bit-identical to the single-name call.
    Symmetric bit for bit, NaN outside the principal domain; a zero denominator gives what IEEE
    gives.  Memory and reproducibility as for ``bispectrum``, plus 8 B per entry and measure.
    """
    names = _bicoherence_methods(method)
    plan = _BispecPlan(fs, resolution, fmin, fmax, 8 * len(set(names)))
    cnt, sums, power, host = _bispec_sums(plan, data, fs, axis, resolution, window, overlap, detrend, "density")
    out = {}
    for m in names:
        if m not in out:
            out[m] = _bispec_result(dev.bispec_finish(m, cnt, plan.k_lo, sums, power), host, plan.flat)
    return cnt, plan.freqs, out[names[0]] if isinstance(method, str) else out


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
