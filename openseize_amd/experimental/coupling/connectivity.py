"""analytic_connectivity: envelope and phase coupling of analytic signals over all channel
pairs, in the time domain (no counterpart in the reference).  The frequency-domain half of the
family is ``spectra.estimators.phase_connectivity``; this one takes band-passed analytic signals,
typically ``Analytic(Butter(...)(x, ..., dephase=True), fs, chunksize, axis, width=...).signal``,
and reduces over time.  The sums over all pairs are the device kernels of ``csrc/pairtime.hip``
(K13): ``osz_analytic_accumulate`` and ``osz_analytic_finish``.
"""

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core.producer import Producer, producer
from openseize_amd.experimental.coupling.transforms import _complex_rows

ANALYTIC_METHODS = tuple(_lib.ANALYTIC_MODE)      # ("aec", "oaec", "plv", "ciplv", "wpli")

# samples per time block: the stream is summed in blocks of this many samples counted from its
# first sample, whatever the chunks are (OSZ_ANALYTIC_BLOCK of the C ABI)
_BLOCK = _lib.ANALYTIC_BLOCK
# bytes of work space (staged planes, block partials) one push may take
_PUSH_BYTES = 1 << 30


def _methods(method):
    names = (method,) if isinstance(method, str) or not isinstance(method, (tuple, list)) else tuple(method)
    bad = [m for m in names if not isinstance(m, str) or m not in ANALYTIC_METHODS]
    if bad or not names:
        raise ValueError(f"unknown analytic connectivity method(s) {bad}: choose from {ANALYTIC_METHODS}")
    return names


_REAL = ("analytic_connectivity takes complex data, got {}: build the analytic signal with `Analytic` "
         "(experimental.coupling.transforms) from the band-passed data and pass its `signal`")


def _is_complex(arr):
    return arr.is_complex() if dev.is_tensor(arr) else np.iscomplexobj(arr)


def analytic_connectivity(signal, method="oaec", axis=-1, chunksize=None):
    """Amplitude-envelope and phase coupling over all channel pairs of an analytic signal.

    ``signal`` is complex and two-dimensional, samples along ``axis`` and the C channels along
    the other axis: an ndarray, a CUDA tensor, or a producer of complex chunks such as
    ``Analytic(band_passed, fs, chunksize, axis, width=...).signal``.  ``chunksize`` applies to
    arrays only (default ``int(10e6)``, as ``Transform``).  ``method`` is one name or a tuple of
    names; with a = |z|, u = z / a, and per pair d_t = Im(conj(z_i) z_j) = x_i y_j - y_i x_j,
    m_t = |d_t|, r(p, q) the Pearson correlation over the N samples:

    ``"aec"``    r(a_i, a_j), the amplitude-envelope correlation;
    ``"oaec"``   (r(a_i, m / a_i) + r(a_j, m / a_j)) / 2, the orthogonalised envelope correlation
                 (Hipp et al. 2012): m / a_i is the envelope of the part of z_j orthogonal to z_i
                 sample by sample, which zero-lag leakage cannot reach.  Signed, no absolute value;
    ``"plv"``    |sum conj(u_i) u_j| / N, the phase-locking value (Lachaux et al. 1999);
    ``"ciplv"``  |Im s| / sqrt(1 - (Re s)^2) with s = sum conj(u_i) u_j / N, the corrected
                 imaginary plv (Bruna et al. 2018);
    ``"wpli"``   |sum d_t| / sum m_t, the weighted phase-lag index (Vinck et al. 2011) over time.

    Returns ``(n, M)``: ``n`` the samples consumed, M float64 (C, C) for one name, for a tuple a
    dict of name -> such an array in the order asked, every measure from ONE pass over the stream
    and bit-identical to the single-name call.  Host data gives ndarrays, CUDA data CUDA tensors.

    All measures are symmetric bit for bit.  The diagonal is written, not computed: 1.0 for aec
    and plv, 0.0 for oaec, ciplv and wpli.  NaN overrides it: a non-finite sample or a sample of
    amplitude zero (u = 0 / 0) in channel k makes row and column k NaN and leaves every other
    pair exactly as it is without it.  Elsewhere a zero denominator gives what IEEE gives.

    Real data, one-dimensional data, more than two dimensions, an unknown or empty ``method``
    raise ``ValueError`` before the stream or the device is touched (a producer's chunks show
    their type only when the first one arrives: real chunks raise then); so does a stream that
    ends without a sample.

    The stream is summed in blocks of 4096 samples counted from its first sample, each block in a
    fixed order and the blocks in order, without atomics: the result does not depend on how the
    stream is cut into chunks, and two calls give the same bits.  Device memory does not grow
    with the stream: 8 B per pair and sum (aec 1 sum, oaec 5, plv / ciplv 2 together, wpli 2; only
    what ``method`` needs), fewer than 4096 samples carried between chunks, and per push at most
    about 1 GiB of staged samples and block partials.
    """
    names = _methods(method)
    if isinstance(signal, Producer):
        pro = producer(signal, signal.chunksize, axis)
    else:
        if dev.is_arraylike(signal) and not _is_complex(signal):
            raise ValueError(_REAL.format(f"{signal.dtype} data"))
        pro = producer(signal, int(10e6) if chunksize is None else chunksize, axis)
    if len(pro.shape) != 2:
        raise ValueError(f"analytic_connectivity needs two-dimensional data (channels x samples), got shape "
                         f"{tuple(pro.shape)}: "
                         + ("stack at least two channels" if len(pro.shape) < 2
                            else "reshape the channel axes into one"))
    groups = 0
    for name in names:
        groups |= _lib.ANALYTIC_GROUP[name]
    layout = dev.Layout(pro.shape, axis)
    nch = layout.nch
    planes = dev.analytic_planes(groups)
    host = dev.origin_is_host(pro)
    torch, sums, chan, carry = dev.torch, None, None, None
    count = 0
    for arr in dev.pull_resident(pro, pro):
        if not _is_complex(arr):
            raise ValueError(_REAL.format(f"{arr.dtype} chunks"))
        if sums is None:
            dev.require_gpu()
            sums = dev.zeros((planes, nch, nch), torch.float64)
            chan = dev.zeros((3, nch), torch.float64)
            # whole blocks one push takes: 48 B of staged planes per (channel, sample), 8 B per
            # (plane, pair) and block of partials
            cap = max(1, _PUSH_BYTES // (48 * nch * _BLOCK + 8 * planes * nch * nch)) * _BLOCK
        z2d, was_host = _complex_rows(arr, layout)
        host = host or was_host
        if z2d.shape[1] == 0:
            continue
        count += z2d.shape[1]
        if carry is not None:
            z2d = torch.cat((carry, z2d), dim=1)
        full = z2d.shape[1] // _BLOCK * _BLOCK
        for at in range(0, full, cap):
            dev.analytic_accumulate(z2d[:, at:min(at + cap, full)], groups, sums, chan)
        # (a copy: a source may fill the chunk's memory again before the next push reads it)
        carry = z2d[:, full:].clone() if full < z2d.shape[1] else None
    if count == 0:
        raise ValueError("analytic_connectivity: the stream ended without a sample")
    if carry is not None:
        dev.analytic_accumulate(carry, groups, sums, chan)
    out = {}
    for name in names:
        if name not in out:
            M = dev.analytic_finish(name, count, groups, sums, chan)
            out[name] = M.cpu().numpy() if host else M
    return count, out[names[0]] if isinstance(method, str) else out
