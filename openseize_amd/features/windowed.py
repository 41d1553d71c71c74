"""window_features: time-resolved per-channel features of a stream (no counterpart in the
reference): line length, variance / RMS and the higher moments, the extremes, zero crossings, the
Hjorth parameters and the Teager energy of every window of ``winsize`` samples, ``step`` apart --
what a long recording is reduced to before anyone looks for where it changes.  All thirteen come
from one read of the data by the device kernel of ``csrc/windowfeat.hip`` (K15):
``osz_window_features``.
"""

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core.producer import Producer, producer

WINDOW_FEATURES = tuple(_lib.WINDOW_FEATURE)

# bytes of results one push may write (the samples of a push are the source's chunk and the carry)
_PUSH_BYTES = 1 << 30


def _names(features):
    names = (features,) if isinstance(features, str) or not isinstance(features, (tuple, list)) else tuple(features)
    bad = [f for f in names if not isinstance(f, str) or f not in WINDOW_FEATURES]
    if bad or not names:
        raise ValueError(f"unknown window feature(s) {bad}: choose from {WINDOW_FEATURES}")
    return names


def _size(value, least, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f"window_features: {what} must be an integer >= {least}, got {value!r}")
    return int(value)


def window_count(n, winsize, step):
    """The windows of ``winsize`` samples, ``step`` apart, that ``n`` samples hold (a trailing
    window the samples do not fill is dropped)."""
    return 0 if n < winsize else (n - winsize) // step + 1


def _advance(have, skip, m, winsize, step):
    """One chunk of ``m`` samples arrives with ``have`` samples carried (they start at the next
    unfinished window) and ``skip`` samples still to discard in front of that window (a gap,
    ``step > winsize``, that the last chunk ended in).  Returns ``(drop, nwin, keep, skip)``:
    ``drop`` samples leave the chunk's front, the carry and the rest hold ``nwin`` whole windows,
    their last ``keep`` samples are carried on, and ``skip`` are still to discard."""
    drop = min(skip, m)
    avail = have + m - drop
    nwin = window_count(avail, winsize, step)
    used = nwin * step                          # where the next unfinished window starts
    if used <= avail:
        return drop, nwin, avail - used, skip - drop
    return drop, nwin, 0, skip - drop + used - avail


def window_plan(lengths, winsize, step):
    """The bookkeeping of the streaming loop as a function of the chunk lengths alone: per chunk
    ``(start, nwin, keep, skip)`` -- the stream index of the first sample the push holds (carry
    included), the windows it completes, the samples carried on and the samples of a gap still to
    discard."""
    plan, have, skip, seen = [], 0, 0, 0
    for m in lengths:
        drop, nwin, keep, skip = _advance(have, skip, m, winsize, step)
        plan.append((seen + drop - have, nwin, keep, skip))
        seen += m
        have = keep
    return plan


_COMPLEX = "window_features takes real data, got {}"


def _is_complex(arr):
    return arr.is_complex() if dev.is_tensor(arr) else np.iscomplexobj(arr)


def window_features(data, winsize, step=None, features=("line_length", "var"), axis=-1, chunksize=None):
    """Features of every window of ``winsize`` samples, ``step`` apart, per channel.

    ``data`` is real, one- or two-dimensional, samples along ``axis``: an ndarray, a CUDA tensor or
    a producer.  ``chunksize`` applies to arrays only (default ``int(10e6)``).  ``winsize`` = W is
    an integer >= 4, ``step`` an integer >= 1 that defaults to ``winsize``; ``step < W`` overlaps
    the windows, ``step > W`` leaves gaps.  Window k covers the samples k step .. k step + W - 1
    counted from the first sample of the stream, whatever the chunks are; a trailing window the
    stream does not fill is dropped.

    ``features`` is one name or a tuple of names of ``WINDOW_FEATURES``.  With x_0 .. x_{W-1} the
    samples of one window, dx_t = x_{t+1} - x_t, ddx_t = dx_{t+1} - dx_t and m_k the k-th central
    moment about the window's own mean with divisor W:

    ``"mean"``, ``"var"``, ``"rms"``    the mean, m_2 (``np.var``), sqrt(mean x^2);
    ``"skew"``, ``"kurtosis"``          m_3 / m_2^1.5 and m_4 / m_2^2: biased, Pearson's (not excess), as
                                        ``scipy.stats.skew(bias=True)`` and ``kurtosis(fisher=False)``;
    ``"min"``, ``"max"``, ``"ptp"``     as NumPy's;
    ``"line_length"``                   sum |dx_t|;
    ``"zero_crossings"``                the number of t with (x_t < 0) != (x_{t+1} < 0);
    ``"mobility"``                      sqrt(var(dx) / var(x)), Hjorth's, per sample (times fs: per second);
    ``"complexity"``                    sqrt(var(ddx) / var(dx)) / mobility;
    ``"teager"``                        the mean over t = 1 .. W - 2 of x_t^2 - x_{t-1} x_{t+1}.

    Returns ``(nwin, F)``: ``nwin`` the windows per channel, F float64 with the sample axis of the
    data replaced by the window axis -- (C, nwin) for (C, N) data, (nwin,) for one-dimensional --
    for one name, for a tuple a dict of name -> such an array in the order asked, all from ONE
    read of the stream and bit-identical to the single-name call.  Host data gives ndarrays, CUDA
    data CUDA tensors.

    A window that holds a NaN is NaN in every feature; +-inf and a zero variance give what IEEE
    arithmetic gives from the definitions.  A window's bits depend on W and its own samples only:
    not on ``step``, the number of channels, the chunking, host or CUDA data, or the other
    features asked (the device sums a window in an order that is a function of W alone, without
    atomics).  The moments are sums about the window's first sample, so an offset of the data
    costs no accuracy.

    Complex data, more than two dimensions, ``winsize < 4``, ``step < 1``, sizes that are not
    integers, an unknown or empty ``features`` raise ``ValueError`` before the stream or the device
    is touched (a producer's complex chunks when the first one arrives); so does a stream shorter
    than ``winsize``.  Device memory does not grow with a host-fed stream: fewer than ``winsize``
    samples (or, between two chunks, the unfinished windows' samples) are carried, and each push's
    results come down as they are made; CUDA-fed streams keep theirs on the device.
    """
    names = _names(features)
    W = _size(winsize, 4, "winsize")
    step = W if step is None else _size(step, 1, "step")
    if isinstance(data, Producer):
        pro = producer(data, data.chunksize, axis)
    else:
        if dev.is_arraylike(data) and _is_complex(data):
            raise ValueError(_COMPLEX.format(f"{data.dtype} data"))
        pro = producer(data, int(10e6) if chunksize is None else chunksize, axis)
    if not 1 <= len(pro.shape) <= 2:
        raise ValueError(f"window_features needs one- or two-dimensional data, got shape {tuple(pro.shape)}: "
                         "reshape the channel axes into one")
    layout = dev.Layout(pro.shape, axis)
    if pro.shape[layout.axis] < W:
        raise ValueError(f"window_features: the stream holds {pro.shape[layout.axis]} samples, fewer than one "
                         f"window of {W}")
    nch = layout.nch
    order = [f for f in WINDOW_FEATURES if f in names]       # the planes a push writes
    mask = dev.window_mask(order)
    host = dev.origin_is_host(pro)
    torch = dev.torch
    most = max(1, _PUSH_BYTES // (8 * len(order) * nch))     # windows per launch
    parts, carry, skip, total, started = [], None, 0, 0, False
    for arr in dev.pull_resident(pro, pro):
        if _is_complex(arr):
            raise ValueError(_COMPLEX.format(f"{arr.dtype} chunks"))
        if not started:
            dev.require_gpu()
            started = True
        x2d, was_host = layout.to2d(arr)
        host = host or was_host
        have = 0 if carry is None else carry.shape[1]
        drop, nwin, keep, skip = _advance(have, skip, x2d.shape[1], W, step)
        if drop:
            x2d = x2d[:, drop:]
        if carry is not None:
            x2d = torch.cat((carry, x2d), dim=1)
        for k0 in range(0, nwin, most):
            k1 = min(k0 + most, nwin)
            out = torch.empty((len(order), nch, k1 - k0), dtype=torch.float64, device=x2d.device)
            dev.window_features(x2d[:, k0 * step:(k1 - 1) * step + W], W, step, mask, out)
            parts.append(out.cpu().numpy() if host else out)
        total += nwin
        # (a copy: a source may fill the chunk's memory again before the next push reads it)
        carry = x2d[:, x2d.shape[1] - keep:].clone() if keep else None
    if total == 0:
        raise ValueError(f"window_features: the stream ended before one window of {W} samples was full")
    if host:
        planes = np.concatenate(parts, axis=2)
        shaped = [np.moveaxis(p.reshape(layout.other + (total,)), -1, layout.axis) for p in planes]
    else:
        planes = torch.cat(parts, dim=2)
        shaped = [layout.from2d(p, False) for p in planes]
    out = {name: shaped[order.index(name)] for name in names}
    return total, out[names[0]] if isinstance(features, str) or not isinstance(features, (tuple, list)) else out
