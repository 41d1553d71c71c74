"""Sources that reuse their chunk buffers, on the device and on the host.

A chunk handed on by a source may be rewritten once the consumer pulls the next one (the ordinary
iterator contract, core/sources.py).  ``Recycler`` below is such a source: every chunk is copied
into the same buffer -- one CUDA tensor, a ring of column ranges of one tensor (whose neighbouring
slots look like one stream to the joining code), or one ndarray -- and yielded; after the last
chunk the buffer is overwritten with a finite sentinel, so that whatever reads a chunk after the
stream has ended fails the tolerance.  Every op is compared with the oracle on the plain data,
with every output chunk kept until the stream has ended (no op may hand out a view of memory it
writes again later), chunk lengths as over an ArrayProducer, non-finite masks exactly."""

from functools import partial

import numpy as np
import pytest
import scipy.signal as sps

from openseize_amd import producer
from openseize_amd.core.producer import MaskedProducer, Producer

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SENTINEL = 1e200
KINDS = ("one", "ring2", "ring3", "host")
SOS = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
ZP_CS = 65536                                  # the zero-phase kernel's routes: cs >= 65536, >= 6 chunks
ZP_TOTAL = 6 * ZP_CS + 1000


@pytest.fixture(scope="module")
def osz():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd.core import numerical as nm
    return nm


class Recycler(Producer):
    """Chunks of ``data`` along ``axis``, each written into a reused buffer and yielded."""

    def __init__(self, data, chunksize, axis, kind):
        super().__init__(data, chunksize, axis)
        self.kind = kind

    @property
    def shape(self):
        return tuple(self.data.shape)

    def __iter__(self):
        import torch
        x, cs, axis = self.data, self.chunksize, self.axis
        n = x.shape[axis]
        dims = list(x.shape)
        if self.kind == "host":
            dims[axis] = cs
            buf = np.empty(dims)
            slots = [buf]
        else:
            ring = {"one": 1, "ring2": 2, "ring3": 3}[self.kind]
            dims[axis] = ring * cs
            buf = torch.empty(dims, dtype=torch.float64, device="cuda")
            slots = [buf.narrow(axis, r * cs, cs) for r in range(ring)]
        try:
            for k, start in enumerate(range(0, n, cs)):
                m = min(cs, n - start)
                slot = slots[k % len(slots)]
                if self.kind == "host":
                    idx = [slice(None)] * x.ndim
                    idx[axis] = slice(0, m)
                    src = list(idx)
                    src[axis] = slice(start, start + m)
                    dst = slot[tuple(idx)]
                    np.copyto(dst, x[tuple(src)])
                else:
                    dst = slot.narrow(axis, 0, m)
                    dst.copy_(x.narrow(axis, start, m))     # (on the current stream)
                yield dst
        finally:
            if self.kind == "host":
                buf.fill(SENTINEL)
            else:
                buf.fill_(SENTINEL)


def recycled(xh, cs, kind, axis=-1):
    import torch
    data = xh if kind == "host" else torch.from_numpy(np.ascontiguousarray(xh)).cuda()
    return Recycler(data, cs, axis, kind)


def plain(xh, cs, kind, axis=-1):
    import torch
    data = xh if kind == "host" else torch.from_numpy(np.ascontiguousarray(xh)).cuda()
    return producer(data, cs, axis)


def host(a):
    import torch
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def assemble(chunks, axis=-1):
    """All output chunks, kept until the stream has ended, then joined on the host."""
    return np.concatenate([host(c) for c in chunks], axis=axis)


def assert_matches(y, want):
    y, want = np.asarray(y), np.asarray(want)
    assert y.shape == want.shape, (y.shape, want.shape)
    bad_y, bad_w = ~np.isfinite(y), ~np.isfinite(want)
    assert np.array_equal(bad_y, bad_w), (int(bad_y.sum()), int(bad_w.sum()))
    ok = ~bad_w
    scale = max(float(np.max(np.abs(want[ok]))) if ok.any() else 0.0, 1e-300)
    err = float(np.max(np.abs(y[ok] - want[ok]))) / scale if ok.any() else 0.0
    assert err < RTOL, err


def lengths(chunks, axis=-1):
    return [c.shape[axis] for c in chunks]


class Spy:
    """Counts calls of ``owner.name`` and the sample counts of their 2-D argument ``arg`` (None:
    the calls alone)."""

    def __init__(self, owner, name, arg):
        self.owner, self.name, self.arg = owner, name, arg
        self.widths = []

    def __enter__(self):
        plain_ = self.plain = getattr(self.owner, self.name)

        def spy(*a, **k):
            self.widths.append(0 if self.arg is None else a[self.arg].shape[1])
            return plain_(*a, **k)
        setattr(self.owner, self.name, spy)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self.plain)


def signal(C, total, seed):
    return np.random.default_rng(seed).standard_normal((C, total))


# ------------------------------------------------------------------------------------ the FIR
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", (4, 64))
def test_oaconvolve(osz, kind, C):
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    cs, total = 30000, 30000 * 7 + 1234
    xh = signal(C, total, 11)
    for taps_n in (76, 1024):
        h = sps.firwin(taps_n, 0.3)
        for mode in ("full", "same", "valid"):
            want_len = lengths(list(osz.oaconvolve(plain(xh, cs, kind), h, -1, mode)))
            with Spy(dev.FirStream, "push", 1) as spy:
                got = list(osz.oaconvolve(recycled(xh, cs, kind), h, -1, mode))
            assert lengths(got) == want_len
            assert max(spy.widths) <= cs                # a foreign source: one chunk per push
            assert_matches(assemble(got), np.concatenate(orc.oaconvolve(xh, h, mode), -1))


# --------------------------------------------------------------------------------- the IIRs
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", (4, 64))
def test_sosfilt_with_zi(osz, kind, C):
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    cs, total = 30000, 30000 * 7 + 555
    xh = signal(C, total, 12)
    zi = np.random.default_rng(3).standard_normal((SOS.shape[0], C, 2))
    want_len = lengths(list(osz.sosfilt(plain(xh, cs, kind), SOS, -1, zi=zi)))
    with Spy(dev.SosStream, "forward", 1) as spy:
        got = list(osz.sosfilt(recycled(xh, cs, kind), SOS, -1, zi=zi))
    assert lengths(got) == want_len and max(spy.widths) <= cs
    assert_matches(assemble(got), orc.sosfilt(xh, SOS, cs, zi=zi)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", (4, 64))
def test_sosfiltfilt_zero_phase_route(osz, kind, C):
    """sosfiltfilt alone on the one-kernel zero-phase route: the stream's end keeps chunk n-2
    while it pulls the last one."""
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    xh = signal(C, ZP_TOTAL, 13)
    with Spy(dev, "chain_zp_step", 2) as spy:
        got = list(osz.sosfiltfilt(recycled(xh, ZP_CS, kind), SOS, -1))
    assert spy.widths and max(spy.widths) <= ZP_CS          # the zero-phase kernel, one chunk a launch
    assert lengths(got) == lengths(list(osz.sosfiltfilt(plain(xh, ZP_CS, kind), SOS, -1)))
    assert_matches(assemble(got), orc.sosfiltfilt(xh, SOS, ZP_CS))


@pytest.mark.parametrize("kind", KINDS)
def test_sosfiltfilt_separate_kernels(osz, kind):
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    cs, total = 20000, 20000 * 5 + 77
    xh = signal(4, total, 14)
    with Spy(dev, "chain_zp_step", 2) as spy:
        got = list(osz.sosfiltfilt(recycled(xh, cs, kind), SOS, -1))
    assert not spy.widths
    assert_matches(assemble(got), orc.sosfiltfilt(xh, SOS, cs))


@pytest.mark.parametrize("kind", ("one", "ring2", "host"))
def test_lfilter_filtfilt(osz, kind):
    from oracle import oracle as orc
    cs, total = 30000, 30000 * 6 + 999
    xh = signal(4, total, 15)
    ba = sps.butter(4, 0.2)
    got = list(osz.lfilter(recycled(xh, cs, kind), ba, -1))
    assert_matches(assemble(got), orc.lfilter(xh, ba, cs)[0])
    got = list(osz.filtfilt(recycled(xh, cs, kind), ba, -1))
    assert_matches(assemble(got), orc.filtfilt(xh, ba, cs))


# --------------------------------------------------------------- FIR -> IIR through the class API
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dephase", (False, True))
@pytest.mark.parametrize("C", (4, 64))
def test_fir_then_iir_class_api_fused(osz, kind, dephase, C):
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    from openseize_amd.filtering.fir import Kaiser
    from openseize_amd.filtering.iir import Butter
    xh = signal(C, ZP_TOTAL, 16)
    kais = Kaiser(fpass=200, fstop=400, fs=5000, gpass=0.5, gstop=40)
    butter = Butter(fpass=[300, 900], fstop=[150, 1300], fs=5000, gpass=1, gstop=40)
    assert np.ndim(butter.coeffs) == 2
    spied = ("chain_zp_step", 2) if dephase else ("chain_forward", 2)
    with Spy(dev, *spied) as spy:
        fir = kais(recycled(xh, ZP_CS, kind), ZP_CS, axis=-1)
        got = list(butter(fir, ZP_CS, axis=-1, dephase=dephase))
    assert spy.widths and max(spy.widths) <= ZP_CS          # the fused route, one chunk a launch
    u = np.concatenate(orc.oaconvolve(xh, kais.coeffs, "same"), -1)
    want = orc.sosfiltfilt(u, butter.coeffs, ZP_CS) if dephase else orc.sosfilt(u, butter.coeffs, ZP_CS)[0]
    assert lengths(got) == orc.rechunk_lengths(ZP_TOTAL, ZP_CS)
    assert_matches(assemble(got), want)


# ------------------------------------------------------------------------ resampling, spectra
@pytest.mark.parametrize("kind", ("one", "ring2", "host"))
def test_resampling(osz, kind):
    from openseize_amd.resampling.resampling import downsample, resample, upsample
    xh = signal(4, 60000 + 321, 17)
    for op in (partial(downsample, M=5), partial(upsample, L=3), partial(resample, L=3, M=2)):
        want = list(op(plain(xh, 6000, kind), fs=5000, chunksize=6000, axis=-1))
        got = list(op(recycled(xh, 6000, kind), fs=5000, chunksize=6000, axis=-1))
        assert lengths(got) == lengths(want)
        assert_matches(assemble(got), assemble(want))
    # and against the oracle: the whole-stream resample_poly with the port's own window
    from oracle import oracle as orc
    from openseize_amd.core.numerical import _resample_plan
    from openseize_amd.filtering.fir import Kaiser
    src = recycled(xh, 6000, kind)
    _, h = _resample_plan(src, 1, 5, 5000, Kaiser, -1, {})
    y = assemble(list(downsample(src, 5, fs=5000, chunksize=6000, axis=-1)))
    assert_matches(y, orc.polyphase_resample(xh, 1, 5, h))


@pytest.mark.parametrize("kind", ("one", "ring2", "host"))
def test_psd_and_stft(osz, kind):
    from oracle import oracle as orc
    from openseize_amd.spectra.estimators import psd, stft
    fs = 1000
    xh = signal(4, 100 * fs + 333, 18)
    cnt, f, p = psd(recycled(xh, fs, kind), fs, axis=-1)
    rc, rf, rp = orc.psd(xh, fs)
    assert cnt == rc and np.array_equal(f, rf)
    assert_matches(host(p), rp)
    f, t, X = stft(recycled(xh, fs, kind), fs, axis=-1, asarray=True)
    rf, rt, rX = orc.stft(xh, fs)
    assert np.allclose(t, rt, rtol=0, atol=1e-12)
    assert_matches(host(X), rX)


@pytest.mark.parametrize("kind", ("one", "ring2", "host"))
def test_masked_over_recycler(osz, kind):
    from oracle import oracle as orc
    cs, total = 30000, 30000 * 6 + 4321
    xh = signal(4, total, 19)
    mask = np.random.default_rng(5).random(total) > 0.3
    mask[60000:95000] = False
    src = MaskedProducer(recycled(xh, cs, kind), mask, cs, -1)
    kept = orc.masked_stream(xh, mask, cs)
    assert_matches(assemble(list(src)), kept)
    h = sps.firwin(255, 0.2)
    src = MaskedProducer(recycled(xh, cs, kind), mask, cs, -1)
    assert_matches(assemble(list(osz.oaconvolve(src, h, -1, "same"))),
                   np.concatenate(orc.oaconvolve(kept, h, "same"), -1))


@pytest.mark.parametrize("piece", (ZP_CS // 3, ZP_CS, 5 * ZP_CS // 2))
def test_genproducer_over_one_cuda_tensor(osz, piece):
    """A generating function that refills one CUDA tensor: the GenProducer's chunks are its own,
    so the joined, read-ahead routes stay open behind it -- and right."""
    import torch
    from oracle import oracle as orc
    xh = signal(4, ZP_TOTAL, 20)
    x = torch.from_numpy(xh).cuda()

    def gen():
        buf = torch.empty((4, piece), dtype=torch.float64, device="cuda")
        for s in range(0, ZP_TOTAL, piece):
            m = min(piece, ZP_TOTAL - s)
            buf[:, :m].copy_(x[:, s:s + m])
            yield buf[:, :m]
        buf.fill_(SENTINEL)

    pro = producer(gen, ZP_CS, -1, shape=xh.shape)
    chunks = list(pro)
    assert lengths(chunks) == orc.rechunk_lengths(ZP_TOTAL, ZP_CS)
    assert np.array_equal(assemble(chunks), xh)
    assert_matches(assemble(list(osz.sosfilt(pro, SOS, -1))), orc.sosfilt(xh, SOS, ZP_CS)[0])
    assert_matches(assemble(list(osz.sosfiltfilt(pro, SOS, -1))), orc.sosfiltfilt(xh, SOS, ZP_CS))


# ---------------------------------------------------------------------------- non-finite samples
def nonfinite(case, C=4):
    xh = signal(C, ZP_TOTAL, 21)
    if case == "nan_chunk2":
        xh[1, 2 * ZP_CS + 12345] = np.nan
    elif case == "inf_second_to_last":
        # chunk n-2 of 7, behind the head of it the zero-phase steps see: the zero-phase end's
        # rare path (a channel that first goes bad in the last two chunks) re-reads chunk n-2
        xh[2, 5 * ZP_CS + 9 * ZP_CS // 10] = np.inf
    elif case == "channel_to_end":
        xh[3, 3 * ZP_CS + 777:] = np.nan
    return xh


CASES = ("nan_chunk2", "inf_second_to_last", "channel_to_end")


@pytest.mark.parametrize("kind", ("one", "ring2", "host"))
@pytest.mark.parametrize("case", CASES)
def test_nonfinite_oaconvolve(osz, kind, case):
    from oracle import oracle as orc
    xh = nonfinite(case)
    h = sps.firwin(256, 0.2)
    got = list(osz.oaconvolve(recycled(xh, ZP_CS, kind), h, -1, "same"))
    assert_matches(assemble(got), np.concatenate(orc.oaconvolve(xh, h, "same"), -1))


@pytest.mark.parametrize("kind", ("one", "ring2", "host"))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dephase", (False, True))
def test_nonfinite_fir_then_iir(osz, kind, case, dephase):
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    xh = nonfinite(case)
    h = sps.firwin(256, 0.2)
    src = recycled(xh, ZP_CS, kind)
    fir = producer(partial(osz.oaconvolve, src, h, -1, "same"), ZP_CS, -1, shape=src.shape)
    spied = ("chain_zp_step", 2) if dephase else ("chain_forward", 2)
    with Spy(dev, *spied) as spy, Spy(dev.FirStream, "restore", None) as restored:
        got = list((osz.sosfiltfilt if dephase else osz.sosfilt)(fir, SOS, -1))
    assert spy.widths                                       # the fused route
    if dephase and case == "inf_second_to_last":
        # the zero-phase end's rare path: the states at chunk n-2 restored, chunk n-2 read again
        assert restored.widths
    u = np.concatenate(orc.oaconvolve(xh, h, "same"), -1)
    want = orc.sosfiltfilt(u, SOS, ZP_CS) if dephase else orc.sosfilt(u, SOS, ZP_CS)[0]
    assert_matches(assemble(got), want)


# ------------------------------------------------------------------------------- nfft_factor
@pytest.mark.parametrize("factor", (8, 64))
def test_nfft_factor_reach(osz, factor):
    """The reference's segment length is 8 * 2^ceil(log2 taps) * nfft_factor: a NaN loses the
    whole segment it falls in, whatever nfft_factor says -- through oaconvolve and through the
    FIR fused into sosfilt / sosfiltfilt."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    xh = signal(4, ZP_TOTAL, 22)
    xh[1, 2 * ZP_CS + 40000] = np.nan
    h = sps.firwin(76, 0.2)
    x = torch.from_numpy(xh).cuda()
    u = np.concatenate(orc.oaconvolve(xh, h, "same", nfft_factor=factor), -1)
    got = list(osz.oaconvolve(producer(x, ZP_CS, -1), h, -1, "same", nfft_factor=factor))
    assert_matches(assemble(got), u)
    for dephase, spied in ((False, "chain_forward"), (True, "chain_zp_step")):
        fir = producer(partial(osz.oaconvolve, producer(x, ZP_CS, -1), h, -1, "same", nfft_factor=factor),
                       ZP_CS, -1, shape=xh.shape)
        with Spy(dev, spied, 2) as spy:
            got = list((osz.sosfiltfilt if dephase else osz.sosfilt)(fir, SOS, -1))
        assert spy.widths                                   # the fused route carries the factor
        want = orc.sosfiltfilt(u, SOS, ZP_CS) if dephase else orc.sosfilt(u, SOS, ZP_CS)[0]
        assert_matches(assemble(got), want)
