"""The batch walk of the channel-pair window kernels on the device (K19 osz_window_pairs, K23
osz_window_xcorr, K24 osz_window_granger, K25 osz_window_mi): every case of tests/pairwin_batches.py
-- three batches, two batches of K19's real plan, the 65535-window clamp of a grid's y, K25's own
cap -- through ``check`` of that module.

(a) One call over every window has the bits of one call per batch over that batch's own samples,
each of which is a single batch with w0 = 0.  (b) At both ends, on both sides of every batch edge
and inside every batch the call agrees with the kernel's host restatement under the caps of its own
parity test (``caps`` for K19 and K23, RTOL absolute for K24 and K25, ``counts`` and ``lag`` exactly).
(c) What the restatement says is finite is finite: the rows are a column range of a wider tensor
whose other columns are NaN, so a read outside [0, n) poisons a result.

Then the public functions with pushes of a batch and a half, from a host array and from a CUDA
tensor, and the entry points called directly with a plane pitch, a row pitch and a work space larger
than what they need, whose slack and guard must keep their bits.

Results stay on the device; the bit comparisons are made there on an int64 view with the NaNs made
one, and only the picked windows come to the host.  Every result array starts as -7.0."""

from functools import lru_cache

import numpy as np
import pytest

import pairwin_batches as pb
from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.features import _stream

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
LEFT, RIGHT = 5, 8                        # NaN columns on both sides of the stream
PITCH_MORE, PLANE_MORE, GUARD = 13, 7, 64   # of the direct calls
KEY = dict(ids=lambda c: c.key)
TABLE = {"pairs": _lib.WINDOW_CONNECTIVITY, "xcorr": _lib.WINDOW_XCORR, "granger": _lib.WINDOW_GRANGER,
         "mi": _lib.WINDOW_MI}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch


def blank(*shape):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")


def padded(x, left, right):
    """The rows x on the device as a column range of a NaN-filled tensor: (view, whole tensor)."""
    import torch
    t = torch.from_numpy(np.array(x))
    wide = torch.full((x.shape[0], left + x.shape[1] + right), float("nan"), dtype=t.dtype, device="cuda")
    wide[:, left:left + x.shape[1]] = t.cuda()
    return wide[:, left:left + x.shape[1]], wide


@lru_cache(maxsize=None)
def rows(key):
    return padded(pb.stream(pb.BY_KEY[key]), LEFT, RIGHT)[0]


def matrices(case):
    """The names of a case that are (C, C) planes of ``out``, in the order the kernel writes them."""
    return [m for m in TABLE[case.kernel] if m in case.names and m not in ("xcorr", "counts")]


def run(case, x):
    """name -> (nwin, ...) CUDA results of one call of the case's wrapper over the rows x."""
    nch, W, nwin = case.nch, case.W, pb.window_count(x.shape[1], case.W, pb.STEP)
    assert x.stride(0) > x.shape[1] and x.stride(1) == 1     # the pitch exceeds n in every call
    mask, order = dev.name_mask(TABLE[case.kernel], case.names), matrices(case)
    out = blank(len(order), nwin, nch, nch)
    found = {name: out[p] for p, name in enumerate(order)}
    if case.kernel == "pairs":
        done = dev.window_pairs(x, W, pb.STEP, case.param, mask, out)
    elif case.kernel == "granger":
        done = dev.window_granger(x, W, pb.STEP, case.param, mask, out)
    elif case.kernel == "xcorr":
        lags = 2 * case.param + 1
        xc = blank(nwin, lags, nch, nch) if "xcorr" in case.names else None
        done = dev.window_xcorr(x, W, pb.STEP, case.param, case.flag, mask, xc, out)
        if xc is not None:
            found["xcorr"] = xc
    else:
        B = case.param
        counts = blank(nwin, B * B, nch, nch) if "counts" in case.names else None
        done = dev.window_mi(x, W, pb.STEP, B, _lib.MI_BINNING[case.flag], mask, counts, out)
        if counts is not None:
            found["counts"] = counts.view(nwin, B, B, nch, nch)
    assert done == nwin
    assert {k: tuple(v.shape) for k, v in found.items()} == pb.shapes(case, nwin)
    return found


@lru_cache(maxsize=None)
def whole(key):
    """One call over every window of the case, computed once and left unchanged."""
    return run(pb.BY_KEY[key], rows(key))


def parts(case, batches):
    """One call per batch over the batch's own samples: (w0, results), in order."""
    x = rows(case.key)
    for w0, count in batches:
        cut = x[:, pb.batch_columns(case, w0, count)]
        assert pb.plan_of(case, count).batches == [(0, count)]
        yield w0, run(case, cut)


@pytest.mark.parametrize("case", pb.CASES, **KEY)
def test_every_batch_has_the_bits_of_its_own_call_and_the_picks_agree_with_the_restatement(torch, case):
    P = pb.plan_of(case)
    print(f"{case.key}: C={case.nch} W={case.W} {case.param} {case.flag}: {P.nwin} windows in batches {P.batches} "
          f"({P.binds} binds)")
    assert len(P.batches) == case.want[0] and P.batch == case.want[2]
    x = pb.stream(case)
    at = pb.picks(P.batches)
    if case.kernel == "xcorr":
        assert pb.lag_margin(case, x, at) > 2.0
    pb.check(case, whole(case.key), parts(case, P.batches), at, pb.references(case, x, at), say=print)


def public(case, data):
    from openseize_amd import features
    W, names = case.W, case.names
    if case.kernel == "pairs":
        return features.window_connectivity(data, W, pb.STEP, measures=names, ddof=case.param)
    if case.kernel == "xcorr":
        return features.window_xcorr(data, W, pb.STEP, measures=names, maxlag=case.param, normalize=case.flag)
    if case.kernel == "granger":
        return features.window_granger(data, W, pb.STEP, measures=names, order=case.param)
    return features.window_mutual_info(data, W, pb.STEP, measures=names, bins=case.param, binning=case.flag)


@pytest.mark.parametrize("case", pb.THREE, **KEY)
def test_the_public_function_with_pushes_of_a_batch_and_a_half(torch, case, monkeypatch):
    """A push of batch + batch // 2 windows spans a batch edge, and the stream spans several pushes."""
    P = pb.plan_of(case)
    push = P.batch + P.batch // 2
    assert not {"xcorr", "counts"} & set(case.names) and P.batch < push < P.nwin
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 8 * case.nch * case.nch * len(case.names) * push)
    wrapper = {"pairs": "window_pairs", "xcorr": "window_xcorr", "granger": "window_granger", "mi": "window_mi"}[case.kernel]
    plain, launched = getattr(dev, wrapper), []
    monkeypatch.setattr(dev, wrapper, lambda *a, **k: (launched.append(plain(*a, **k)), launched[-1])[1])
    want = whole(case.key)
    x = np.array(pb.stream(case))
    for data in (x, torch.from_numpy(x).cuda()):
        del launched[:]
        nwin, G = public(case, data)
        assert nwin == P.nwin and launched == [push] * (P.nwin // push) + [P.nwin % push], launched
        for name in case.names:
            g = G[name]
            assert isinstance(g, np.ndarray if data is x else torch.Tensor), name
            g = torch.from_numpy(g).cuda() if data is x else g
            assert g.is_cuda and pb.same_bits(g, want[name]), (case.key, name, "host" if data is x else "cuda")


def all_sentinel(t):
    import torch
    return pb.same_bits(t, torch.full_like(t, SENTINEL))


@pytest.mark.parametrize("case", pb.DIRECT, **KEY)
def test_the_entry_point_keeps_to_its_planes_and_its_work_space(torch, case):
    """The entry point called directly: a row pitch of n + 13 with NaN padding, a plane pitch of nwin
    C^2 + 7, a work space of exactly osz_*_work doubles at the head of one 64 doubles longer."""
    lib = dev.require_gpu()
    nch, W, cc = case.nch, case.W, case.nch * case.nch
    x, wide = padded(pb.stream(case), 0, PITCH_MORE)
    n, pitch = x.shape[1], wide.stride(0)
    nwin = pb.window_count(n, W, pb.STEP)
    mask, order = dev.name_mask(TABLE[case.kernel], case.names), matrices(case)
    tail = (mask, int(case.cplx)) if case.kernel == "pairs" else (case.param, mask)
    need = getattr(lib, f"osz_window_{case.kernel}_work")(nch, n, W, pb.STEP, *tail)
    assert need == pb.plan_of(case).work and pitch == n + PITCH_MORE and nwin == case.nwin
    plane_pitch = nwin * cc + PLANE_MORE
    out = blank(len(order) * plane_pitch + GUARD)
    work = blank(need + GUARD)
    assert work.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0
    lead = {"xcorr": 2 * case.param + 1, "mi": case.param * case.param}.get(case.kernel, 0)
    more = blank(nwin * lead * cc + GUARD) if lead else None
    p, st = dev.ptr, dev.stream_ptr()
    if case.kernel == "pairs":
        rc = lib.osz_window_pairs(p(wide), pitch, nch, n, int(case.cplx), W, pb.STEP, case.param, mask, p(out),
                                  plane_pitch, p(work), need, st)
    elif case.kernel == "granger":
        rc = lib.osz_window_granger(p(wide), pitch, nch, n, W, pb.STEP, case.param, mask, p(out), plane_pitch, p(work),
                                    need, st)
    elif case.kernel == "xcorr":
        rc = lib.osz_window_xcorr(p(wide), pitch, nch, n, W, pb.STEP, case.param, int(case.flag), mask, p(more), p(out),
                                  plane_pitch, p(work), need, st)
    else:
        rc = lib.osz_window_mi(p(wide), pitch, nch, n, W, pb.STEP, case.param, _lib.MI_BINNING[case.flag], mask, p(more),
                               p(out), plane_pitch, p(work), need, st)
    _lib.check(rc)
    torch.cuda.synchronize()
    want = whole(case.key)
    planes = out[:len(order) * plane_pitch].view(len(order), plane_pitch)
    for k, name in enumerate(order):
        assert pb.same_bits(planes[k, :nwin * cc].view(nwin, nch, nch), want[name]), (case.key, name)
    assert all_sentinel(planes[:, nwin * cc:]), (case.key, "the slack of a plane was written")
    assert all_sentinel(out[len(order) * plane_pitch:]), (case.key, "past the last plane")
    assert all_sentinel(work[need:]), (case.key, "past the work space")
    if lead:
        name = "xcorr" if case.kernel == "xcorr" else "counts"
        assert pb.same_bits(more[:nwin * lead * cc].view(want[name].shape), want[name]), (case.key, name)
        assert all_sentinel(more[nwin * lead * cc:]), (case.key, f"past {name}")
