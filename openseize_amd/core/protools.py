"""Producer-level glue: lazily evaluated array operations on producers.

Mirror of the reference's ``core/protools.py`` (cited per function), written
from scratch.  ``pad`` is on the hot path (STFT boundary handling, reference
core/numerical.py:1044,1051); the others are SURVEY section 8f rank 2 -- they
keep a chain of producers (filter -> standardize -> psd ...) lazy and, for
device-resident producers, resident in HBM.  The shape bookkeeping (pad,
squeeze, expand_dims, slicing) moves no sample; every function that computes
(add, multiply, multiply_along_axis, mean, std, standardize) runs the kernels
of ``csrc/glue.hip`` through the C ABI -- ``osz_ew``, ``osz_moments_*``,
``osz_col_moments`` -- for host chunks (uploaded, result brought back as an
ndarray) and device chunks alike: there is no NumPy arithmetic path.
"""

from functools import partial

import numpy as np

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core import arraytools, sources
from openseize_amd.core.producer import Producer, producer


def pad(pro, amt, axis, value=0):
    """Constant padding before and after ``axis`` (core/protools.py:182-232): along the
    production axis two extra arrays frame the stream, along any other axis every
    produced array grows."""
    before, after = (amt, amt) if isinstance(amt, int) else tuple(amt)
    grown = [n + before + after if i == arraytools.normalize_axis(axis, pro.ndim) else n
             for i, n in enumerate(pro.shape)]
    along_stream = arraytools.normalize_axis(axis, pro.ndim) == pro.axis
    gen = _production_axis_padder if along_stream else _other_axis_padder
    return producer(partial(gen, pro, (before, after), axis, value), pro.chunksize, pro.axis,
                    shape=grown)


@sources.relay
@dev.chain_aware
def _production_axis_padder(pro, amt, axis, value):
    """Only the first and last produced arrays change
    (core/protools.py:229-251)."""
    left_shape, right_shape = list(pro.shape), list(pro.shape)
    left_shape[axis], right_shape[axis] = amt[0], amt[1]
    it = iter(pro)
    first = next(it, None)
    ref = first if first is not None else None
    if ref is None:
        import numpy as np
        ref = np.zeros(0)
    yield dev.zeros_like_kind(ref, left_shape, value)
    if first is not None:
        yield first
        yield from it
    yield dev.zeros_like_kind(ref, right_shape, value)


@sources.fresh
@dev.chain_aware
def _other_axis_padder(pro, amt, axis, value):
    """Every produced array grows along a non-production axis
    (core/protools.py:254-264)."""
    for arr in pro:
        yield arraytools.pad_along_axis(arr, amt, axis, constant_values=value)


# ---------------------------------------------------------------------------
# the rest of the reference's protools
# ---------------------------------------------------------------------------
def squeeze(pro, axis=None):
    """Removes singleton axes (core/protools.py:36-70); the production axis keeps
    its meaning: its new index is the number of kept axes in front of it."""
    if axis is None:
        kept = [i for i, n in enumerate(pro.shape) if n > 1]
    else:
        gone = arraytools.normalize_axis(axis, pro.ndim)
        if pro.shape[gone] != 1:
            raise ValueError("cannot select an axis to squeeze out which has "
                             "size not equal to one")
        kept = [i for i in range(pro.ndim) if i != gone]
    if pro.axis not in kept:
        raise ValueError(f"{(pro.axis, pro.shape[pro.axis])} is not in list")
    return producer(partial(_map_gen, pro, partial(dev.squeeze, axis=axis)), pro.chunksize,
                    kept.index(pro.axis), shape=tuple(pro.shape[i] for i in kept))


@sources.relay
@dev.chain_aware
def _map_gen(pro, func):
    for arr in pro:
        yield func(arr)


# -- elementwise arithmetic: one HIP kernel (osz_ew) whatever the operand is --
def _as_device(value, device):
    """float64 CUDA tensor of a number / ndarray / tensor (plumbing only)."""
    import torch
    if dev.is_tensor(value):
        if value.is_complex():
            raise TypeError("protools arithmetic runs float64 kernels: complex input is not supported")
        return value.to(device=device, dtype=torch.float64)
    value = np.asarray(value)
    if np.iscomplexobj(value):
        raise TypeError("protools arithmetic runs float64 kernels: complex input is not supported")
    return torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(device)


def _operand(value, layout, chunk_shape, device):
    """Classifies an operand that broadcasts against a chunk and lays it out
    for the (rows, samples) kernel: one value, one per row (constant along the
    production axis), one per sample (constant across the other axes) or a
    full matrix.  Returns (tensor, kind)."""
    t = _as_device(value, device)
    ndim = len(chunk_shape)
    t = t.reshape((1,) * (ndim - t.ndim) + tuple(t.shape))
    if t.numel() == 1:
        return t.reshape(1), _lib.BCAST_SCALAR
    if t.shape[layout.axis] == 1:
        across = list(chunk_shape)
        across[layout.axis] = 1
        return t.broadcast_to(across).movedim(layout.axis, -1).reshape(-1).contiguous(), _lib.BCAST_ROW
    if all(size == 1 for i, size in enumerate(t.shape) if i != layout.axis):
        if t.shape[layout.axis] != chunk_shape[layout.axis]:
            raise ValueError("operands could not be broadcast together with shapes "
                             f"{tuple(chunk_shape)} {tuple(t.shape)}")
        return t.reshape(-1).contiguous(), _lib.BCAST_COL
    full, _ = layout.to2d(t.broadcast_to(tuple(chunk_shape)))
    return full, _lib.BCAST_FULL


def _apply(op, arr, axis, a, b=None):
    """One chunk through osz_ew; host chunks go up and come back."""
    layout = dev.Layout(arr.shape, axis)
    x2d, host = layout.to2d(arr)
    a2, kind = _operand(a, layout, arr.shape, x2d.device)
    b2 = None if b is None else _operand(b, layout, arr.shape, x2d.device)[0]
    return layout.from2d(dev.ew(op, x2d, a2, b2, kind), host)


@sources.fresh
@dev.chain_aware
def _arith_gen(pro, other, op, verb):
    """pro (op) other, chunk by chunk: ``other`` is a number, an array that
    broadcasts against every produced chunk, or a producer of the same shape
    (reference core/protools.py:72-180)."""
    if isinstance(other, Producer):
        if tuple(pro.shape) != tuple(other.shape):
            raise ValueError(f"producers can not be {verb} with shapes"
                             f"{pro.shape} {other.shape}")
        other.chunksize = pro.chunksize          # walk both streams in step
        for left, right in zip(pro, other):
            yield _apply(op, left, pro.axis, right)
    else:
        for arr in pro:
            yield _apply(op, arr, pro.axis, other)


def _same_shape_producer(pro, genfunc):
    return producer(genfunc, chunksize=pro.chunksize, axis=pro.axis, shape=pro.shape)


def add(pro, other):
    """Adds a number, array or producer to every produced array
    (core/protools.py:72-125) with the device kernel ``osz_ew``."""
    return _same_shape_producer(pro, partial(_arith_gen, pro, other, _lib.EW_ADD, "added together"))


def multiply(pro, other):
    """Multiplies every produced array by a number, array or producer
    (core/protools.py:127-180) with the device kernel ``osz_ew``."""
    return _same_shape_producer(pro, partial(_arith_gen, pro, other, _lib.EW_MUL, "multiplied"))


def expand_dims(pro, axis=0):
    """Inserts new axes (core/protools.py:266-320).  The old axes fill, in order, the
    positions the new ones leave free; the production axis is wherever its old axis
    lands."""
    wanted = (axis,) if isinstance(axis, int) else tuple(axis)
    ndim = pro.ndim + len(wanted)
    fresh = {arraytools.normalize_axis(ax, ndim) for ax in wanted}
    old = iter(enumerate(pro.shape))
    shape, new_axis = [], None
    for pos in range(ndim):
        if pos in fresh:
            shape.append(1)
            continue
        idx, size = next(old)
        shape.append(int(size))
        if idx == pro.axis:
            new_axis = pos
    func = partial(_map_gen, pro, partial(dev.expand_dims, axes=tuple(sorted(fresh))))
    return producer(func, pro.chunksize, new_axis, tuple(shape))


def multiply_along_axis(pro, arr, axis):
    """Produced arrays times a 1-D array laid along one axis, the production
    axis included (core/protools.py:334-426).  Along the production axis the
    multiplier is walked in step with the data (one value per sample, kernel
    operand kind COL); along any other axis it is constant over a chunk."""
    factors = np.array(arr)
    if factors.ndim > 1:
        raise ValueError("Dimensions of multiplier arr must be exactly 1.")
    if len(factors) != pro.shape[axis]:
        raise ValueError("operands could not be broadcast together with shapes "
                         f"{pro.shape} {factors.shape}")
    if np.iscomplexobj(factors):
        raise TypeError("multiply_along_axis: the device kernels are float64, got a complex multiplier")
    along = arraytools.normalize_axis(axis, pro.ndim)
    return _same_shape_producer(pro, partial(_scale_gen, pro, factors.astype(np.float64), along))


@sources.fresh
@dev.chain_aware
def _scale_gen(pro, factors, along):
    laid = [1] * pro.ndim
    if along == pro.axis:
        seen = 0
        for arr in pro:
            m = arr.shape[pro.axis]
            laid[along] = m
            yield _apply(_lib.EW_MUL, arr, pro.axis, factors[seen:seen + m].reshape(laid))
            seen += m
        return
    laid[along] = len(factors)
    for k, arr in enumerate(pro):
        # Reference quirk Q14 (pinned by g12_protools.npz): the producer is zipped with the
        # reshaped multiplier ARRAY (zip_longest(pro, x, fillvalue=x), core/protools.py:418-426),
        # and iterating an array walks its axis 0.  When the multiplied axis IS axis 0,
        # produced chunk k < len(arr) therefore meets the single value arr[k]; along any
        # other axis the one item of that walk is the whole multiplier (the docstring's
        # (2, 4, 1250), axis=1 example) and every chunk sees the plain broadcast.
        quirk = along == 0 and k < len(factors)
        yield _apply(_lib.EW_MUL, arr, pro.axis, factors[k] if quirk else factors.reshape(laid))


def slice_along_axis(pro, start=None, stop=None, step=None, axis=-1):
    """Slices a producer; along the production axis this is a mask
    (core/protools.py:428-482)."""
    start, stop, step = slice(start, stop, step).indices(pro.shape[axis])
    if arraytools.normalize_axis(axis, pro.ndim) == pro.axis:
        mask = np.zeros(pro.shape[axis], dtype=bool)
        mask[start:stop:step] = True
        return producer(pro, pro.chunksize, pro.axis, mask=mask)
    new_shape = list(pro.shape)
    new_shape[axis] = (stop - start) // step
    func = partial(_map_gen, pro, partial(arraytools.slice_along_axis, start=start,
                                          stop=stop, step=step, axis=axis))
    return producer(func, pro.chunksize, pro.axis, shape=new_shape)


# -- moments: streaming kernel along the production axis, per-chunk column
# -- kernel along any other axis
def _restore(vec, dims, at, keepdims, host):
    """(prod(dims),) device vector -> array shaped ``dims`` (with a singleton
    at ``at`` when keepdims) of the kind the chunks had."""
    out = vec.reshape(tuple(dims))
    if keepdims:
        out = out.unsqueeze(at)
    if not host:
        return out
    out = out.cpu().numpy()
    return out[()] if out.ndim == 0 else out


def _stream_moments(pro, ax, ignore_nan):
    """One pass over the producer with the streaming moments kernel
    (osz_moments_*): per-channel mean and std along the production axis."""
    layout = dev.Layout(pro.shape, ax)
    acc = dev.MomentsStream(layout.nch)
    host = True
    try:
        # (a chain of this library's producers over host data hands CUDA tensors to this
        # loop; the statistics still go back as ndarrays)
        for arr in dev.pull_resident(pro, pro):
            x2d, host = layout.to2d(arr)
            acc.push(x2d, ignore_nan)
        return layout, acc.finish(), host or dev.origin_is_host(pro)
    finally:
        acc.close()


def _chunk_moments(arr, ax, ignore_nan):
    """Mean and std of ONE chunk along a non-production axis (osz_col_moments):
    returns ((mean, std) with a singleton at ax, came_from_host)."""
    import torch
    host = not dev.is_tensor(arr) or not arr.is_cuda
    t = _as_device(arr, "cuda")
    moved = t.movedim(ax, 0)
    rest = tuple(moved.shape[1:])
    mu, sd = dev.col_moments(moved.reshape(moved.shape[0], -1).contiguous(), ignore_nan)
    return tuple(v.reshape(rest).unsqueeze(ax) for v in (mu, sd)), host


def _per_chunk_stat(pro, ax, ignore_nan, keepdims, which):
    pieces, host = [], True
    for arr in dev.pull_resident(pro, pro):
        stats, host = _chunk_moments(arr, ax, ignore_nan)
        pieces.append(stats[which])
    host = host or dev.origin_is_host(pro)
    result = dev.concatenate(pieces, pro.axis)
    if not keepdims:
        result = result.squeeze(ax)
    return result.cpu().numpy() if host else result


def mean(pro, axis=-1, ignore_nan=True, keepdims=False):
    """Mean along axis (core/protools.py:500-545).  Along the production axis
    every chunk's (nan)mean is weighted by the chunk length, exactly as the
    reference combines them; the chunks are folded by the streaming moments
    kernel in one pass.  Along another axis every chunk is reduced on its own
    and the results are concatenated."""
    ax = arraytools.normalize_axis(axis, pro.ndim)
    if ax != pro.axis:
        return _per_chunk_stat(pro, ax, ignore_nan, keepdims, 0)
    layout, (mu, _), host = _stream_moments(pro, ax, ignore_nan)
    return _restore(mu, layout.other, ax, keepdims, host)


def std(pro, axis=-1, ignore_nan=True, keepdims=False):
    """Standard deviation along axis (core/protools.py:547-592): along the
    production axis sqrt(E[x^2] - E[x]^2) with both expectations combined over
    the chunks like ``mean`` (one pass instead of the reference's two); along
    another axis the two-pass (nan)std of every chunk."""
    ax = arraytools.normalize_axis(axis, pro.ndim)
    if ax != pro.axis:
        return _per_chunk_stat(pro, ax, ignore_nan, keepdims, 1)
    layout, (_, sd), host = _stream_moments(pro, ax, ignore_nan)
    return _restore(sd, layout.other, ax, keepdims, host)


def standardize(pro, axis=-1, ignore_nan=True):
    """(x - mean) / std along axis as a producer (core/protools.py:594-671).
    Along the production axis the moments are taken first (one pass, on the
    device) and every chunk is then normalised by ``osz_ew``; along another
    axis each chunk is normalised by its own column moments."""
    ax = arraytools.normalize_axis(axis, pro.ndim)
    if ax != pro.axis:
        return _same_shape_producer(pro, partial(_standardize_chunks, pro, ax, ignore_nan))
    layout, (mu, sd), _ = _stream_moments(pro, ax, ignore_nan)
    # plain host arrays keep the returned producer picklable
    mu, sd = mu.cpu().numpy(), sd.cpu().numpy()
    return _same_shape_producer(pro, partial(_standardize_rows, pro, mu, sd))


@sources.fresh
@dev.chain_aware
def _standardize_rows(pro, mu, sd):
    import torch
    for arr in pro:
        layout = dev.Layout(arr.shape, pro.axis)
        x2d, host = layout.to2d(arr)
        a, b = (torch.from_numpy(v).to(x2d.device) for v in (mu, sd))
        yield layout.from2d(dev.ew(_lib.EW_STANDARDIZE, x2d, a, b, _lib.BCAST_ROW), host)


@sources.fresh
@dev.chain_aware
def _standardize_chunks(pro, ax, ignore_nan):
    for arr in pro:
        (mu, sd), host = _chunk_moments(arr, ax, ignore_nan)
        out = _apply(_lib.EW_STANDARDIZE, _as_device(arr, "cuda"), pro.axis, mu, sd)
        yield out.cpu().numpy() if host else out
