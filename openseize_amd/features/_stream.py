"""What the window_* functions share: the checks of their arguments, the opening of the stream,
the loop that carries the samples of the unfinished windows from chunk to chunk and splits a chunk's
windows into launches, and the shaping of the planes into the result.  The kernels, their
parameters and the names they take are each function's own, in its own module.
"""

import functools

import numpy as np

from openseize_amd import _device as dev
from openseize_amd.core.producer import Producer, producer

# bytes of results one launch may write (the samples of a push are the source's chunk and the
# carry).  _launches reads it when it is called: a test that patches it here reaches every function.
_PUSH_BYTES = 1 << 30


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


def _is_complex(arr):
    return arr.is_complex() if dev.is_tensor(arr) else np.iscomplexobj(arr)


def _is_real(p):
    return not isinstance(p, bool) and isinstance(p, (int, float, np.integer, np.floating))


def _is_one(asked):
    """Whether ``asked`` is one name, whose result is returned bare, and not a tuple or list of
    names, whose results are returned as a dict."""
    return isinstance(asked, str) or not isinstance(asked, (tuple, list))


def _names(asked, table, noun):
    names = (asked,) if _is_one(asked) else tuple(asked)
    bad = [f for f in names if not isinstance(f, str) or f not in table]
    if bad or not names:
        raise ValueError(f"unknown {noun} {bad}: choose from {table}")
    return names


def _size(value, least, most, who, what):
    if (isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least
            or (most is not None and value > most)):
        span = f">= {least}" if most is None else f"from {least} to {most}"
        raise ValueError(f"{who}: {what} must be an integer {span}, got {value!r}")
    return int(value)


def _real_only(who):
    """The kind check of a function of real data: ``kind(is_complex, what)`` refuses complex ``what``."""
    def kind(is_complex, what):
        if is_complex:
            raise ValueError(f"{who} takes real data, got {what}")
    return kind


def _open(who, data, axis, chunksize, W, kind, pairs=False):
    """``(pro, layout)`` of ``data``, an array (cut into chunks of ``chunksize``) or a producer, after
    the checks that need no chunk, in this order: ``kind(is_complex, what)`` of array data (a
    producer shows what it holds with its first chunk), one or two dimensions, and one window of
    ``W`` samples.  A function of channel ``pairs`` takes two dimensions and two channels or more."""
    if isinstance(data, Producer):
        pro = producer(data, data.chunksize, axis)
    else:
        if dev.is_arraylike(data):
            kind(_is_complex(data), f"{data.dtype} data")
        pro = producer(data, int(10e6) if chunksize is None else chunksize, axis)
    ndim = len(pro.shape)
    if not (2 if pairs else 1) <= ndim <= 2:
        needs = "two-dimensional data (channels x samples)" if pairs else "one- or two-dimensional data"
        hint = "stack at least two channels" if pairs and ndim < 2 else "reshape the channel axes into one"
        raise ValueError(f"{who} needs {needs}, got shape {tuple(pro.shape)}: {hint}")
    layout = dev.Layout(pro.shape, axis)
    if pairs and layout.nch < 2:
        raise ValueError(f"{who} needs at least two channels, got shape {tuple(pro.shape)}")
    if pro.shape[layout.axis] < W:
        raise ValueError(f"{who}: the stream holds {pro.shape[layout.axis]} samples, fewer than one window of {W}")
    return pro, layout


def _launches(who, pro, W, step, kind, rows, window_bytes):
    """The streaming loop of the functions that window raw samples.  Every chunk of ``pro`` goes
    through ``kind(is_complex, what)``, the kind check of ``_open``, and through ``rows(arr) ->
    (x2d, was_host)``, its (nch, n) CUDA rows; the device is asked for when the first chunk has
    passed its check.  Yields ``(x, n, host)`` per launch: rows that hold exactly ``n``
    whole windows of ``W`` samples, ``step`` apart, beginning with the first window of the stream
    not yet yielded; ``n`` results of ``window_bytes`` bytes are at most ``_PUSH_BYTES``; ``host``
    says whether the results go down to the host."""
    torch = dev.torch
    host = dev.origin_is_host(pro)
    most = max(1, _PUSH_BYTES // window_bytes)               # windows per launch
    carry, skip, total, started = None, 0, 0, False
    for arr in dev.pull_resident(pro, pro):
        kind(_is_complex(arr), f"{arr.dtype} chunks")
        if not started:
            dev.require_gpu()
            started = True
        x2d, was_host = rows(arr)
        host = host or was_host
        have = 0 if carry is None else carry.shape[1]
        drop, nwin, keep, skip = _advance(have, skip, x2d.shape[1], W, step)
        if drop:
            x2d = x2d[:, drop:]
        if carry is not None:
            x2d = torch.cat((carry, x2d), dim=1)
        for k0 in range(0, nwin, most):
            k1 = min(k0 + most, nwin)
            yield x2d[:, k0 * step:(k1 - 1) * step + W], k1 - k0, host
        total += nwin
        # (a copy: a source may fill the chunk's memory again before the next push reads it)
        carry = x2d[:, x2d.shape[1] - keep:].clone() if keep else None
    if total == 0:
        raise ValueError(f"{who}: the stream ended before one window of {W} samples was full")


def _planes(who, pro, W, step, kind, layout, count, launch):
    """The launches of a per-channel function that writes ``count`` planes per window: for every
    ``(x, n, host)`` of ``_launches``, ``launch(x, out)`` fills ``out``, a float64 (count, nch, n)
    CUDA tensor allocated here, which goes down to the host if ``host``.  Returns ``(parts, host)``,
    what ``_result`` takes."""
    nch = layout.nch
    parts, host = [], None
    for x, n, host in _launches(who, pro, W, step, kind, layout.to2d, 8 * count * nch):
        out = dev.torch.empty((count, nch, n), dtype=dev.torch.float64, device=x.device)
        launch(x, out)
        parts.append(out.cpu().numpy() if host else out)
    return parts, host


def _pair_planes(who, pro, W, step, kind, layout, rows, count, launch, advice="", lags=0, more_for="xcorr"):
    """The launches of a channel-pair function that writes ``count`` (nch, nch) planes per window and,
    with ``lags`` (window_xcorr's ``"xcorr"``; ``more_for`` is the noun a message gives them), ``lags``
    more in an array of their own: for every ``(x, n, host)`` of ``_launches``, ``launch(x, out,
    more)`` fills ``out``, a float64 (count, n, nch, nch) CUDA tensor allocated here (None for no plane), and ``more``, (n, lags, nch, nch) (None for
    no lag); both go down to the host if ``host``.  Returns ``(planes, more)`` of the whole stream,
    (count, nwin, nch, nch) and (nwin, lags, nch, nch).  CUDA-fed results stay on the device: when
    they exceed the free device memory, MemoryError before the first launch, with ``advice`` on
    ``who``'s own parameters."""
    torch, nch = dev.torch, layout.nch
    window_bytes = 8 * nch * nch * (count + lags)
    empty = functools.partial(torch.empty, dtype=torch.float64)
    parts, more = [], []
    for x, n, host in _launches(who, pro, W, step, kind, rows, window_bytes):
        if not parts and not more and not host:              # (before the first launch)
            expect = window_count(pro.shape[layout.axis], W, step)
            need, free = window_bytes * expect, torch.cuda.mem_get_info()[0]
            if need > free:
                raise MemoryError(f"{who}: the results of {expect} windows, {count} x ({nch}, {nch}) float64 each"
                                  f"{f' and {lags} more for {more_for}' if lags else ''}, need {need / 1e9:.2f} GB, more than "
                                  f"the {free / 1e9:.2f} GB of device memory that are free: raise step (now {step}; "
                                  f"winsize {W}){advice} or select fewer of the {nch} channels")
        out = empty((count, n, nch, nch), device=x.device) if count else None
        xc = empty((n, lags, nch, nch), device=x.device) if lags else None
        launch(x, out, xc)
        if count:
            parts.append(out.cpu().numpy() if host else out)
        if lags:
            more.append(xc.cpu().numpy() if host else xc)

    def whole(found, axis):
        return None if not found else np.concatenate(found, axis=axis) if host else torch.cat(found, dim=axis)
    return whole(parts, 1), whole(more, 0)


def _asked(asked, names, found):
    """``found[name]`` for one name ``asked``, else the dict of ``names`` in the order asked."""
    return found[names[0]] if _is_one(asked) else {name: found[name] for name in names}


def _result(parts, host, layout, asked, names, where):
    """``(nwin, F)`` of a per-channel function from ``parts``, the (planes, nch, n) results of its
    launches: ndarrays if ``host``, else CUDA tensors.  Every plane gets the layout of the data
    with the window axis in place of the sample axis.  ``where[name]`` is ``(first, count)``: the
    first plane of ``name`` and, for a name with a leading axis of its own, how many planes that
    axis stacks (None: one plane and no such axis).  F is the array of ``names[0]`` when ``asked``
    is one name, else the dict of ``names`` in their order."""
    if host:
        planes = np.concatenate(parts, axis=2)
        shaped = [np.moveaxis(p.reshape(layout.other + p.shape[1:]), -1, layout.axis) for p in planes]
        stack = np.stack
    else:
        planes = dev.torch.cat(parts, dim=2)
        shaped = [layout.from2d(p, False) for p in planes]
        stack = dev.torch.stack
    out = {}
    for name in names:
        first, count = where[name]
        out[name] = shaped[first] if count is None else stack(shaped[first:first + count])
    return planes.shape[2], out[names[0]] if _is_one(asked) else out
