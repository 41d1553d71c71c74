"""GPU parity of the zero-phase chain kernel (C ABI osz_chain_zp_*, csrc/chain_zp.hip):
FIR -> forward cascade -> backward cascade of a chunked stream in one launch per chunk,
against SciPy's convolve + sosfilt forward + sosfilt backward over the whole stream (what the
reference's oaconvolve -> sosfiltfilt, core/numerical.py:158-298 + :338-411, computes away
from the stream's ends when chunks are much longer than the cascade's memory), and through
the public generators against the CPU oracle's chunk-local scheme and the two-kernel step."""

import os
from functools import partial

import numpy as np
import pytest
import scipy.signal as sps

from chain_cells import run_stream, whole_stream_reference  # noqa: F401 (benchmarks/dc_probe.py reads them here)

pytestmark = pytest.mark.gpu

RTOL = 1e-9
BP = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()
    from openseize_amd import _device
    return _device


CASES = [
    # taps, cascade, channels, chunk lengths (u: what the kernel transforms at once -- a block of
    # 27 rows = 6912 samples at 1024 taps, a pair of 2 x 2816 on the pair kernel -- = half the
    # shortest chunk a step takes)
    (1024, BP, 5, lambda u: [u * 6 + 1024, u * 4, u * 3 + u // 2 + 17, u * 2 + 5, u * 4 - 1, u * 3 + 300, 2 * u,
                             3 * u + 1]),
    (1024, BP, 256, lambda u: [u * 30 + 777] * 3),
    (1024, BP, 64, [1 << 18] * 3),
    (300, BP, 7, [150000, 150000, 90001]),
    (513, sps.butter(5, 0.3, output="sos"), 3, [100000] * 3),
    (777, sps.cheby1(3, 1, [0.16, 0.48], "bandpass", output="sos"), 4, [65536, 70000, 65537]),
    (64, sps.ellip(4, 0.5, 50, 0.25, "highpass", output="sos"), 2, [80000, 80001]),
    # a long FIR: blocks of 24 rows (the shortest the one-block kernel has)
    (1700, BP, 3, lambda u: [u * 7 + 33, u * 5, u * 6 - 1]),
    # eight modes (two of them slow): the fit of sixteen two-sided modes is the worst-conditioned the
    # tables admit for eight modes (spec::build_zpn: up to 1e-16 / ratio of the output scale, here 6e-11) -- 5e-10 asserted
    (1024, sps.butter(8, [0.05, 0.3], "bandpass", output="sos"), 3, lambda u: [u * 6 + 1000, u * 7, u * 5 + 5], 5e-10),
]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_zero_phase_stream_against_scipy(dev, case, split):
    taps_n, sos, C, lens = CASES[case][:4]
    tol = CASES[case][4] if len(CASES[case]) > 4 else 1e-11
    h = sps.firwin(taps_n, 0.2)
    if callable(lens):
        fir, iir = dev.FirStream(h, 1), dev.SosStream(sos, 1)
        try:
            lens = lens(dev.chain_zp_min_chunk(fir, iir) // 2)
        finally:
            fir.close()
            iir.close()
    total = sum(lens)
    x = dev.synth_normal(C, total, seed=3 + case)
    got, lag = run_stream(dev, x, h, sos, lens, split)
    pick = sorted({0, C // 2, C - 1})
    ref = whole_stream_reference(x[pick].cpu().numpy(), h, sos)
    g = got[pick].cpu().numpy()
    assert np.isfinite(g[:, lag:]).all()
    hi = total - lag - 6000                       # the stream's end is the caller's
    err = np.max(np.abs(g[:, lag:lag + hi] - ref[:, :hi])) / np.max(np.abs(ref))
    assert err < tol, (taps_n, C, err)


def test_what_the_kernel_refuses(dev):
    """Pairs of filters outside the scheme report -1 (and the public generators then take
    the two-kernel step): a FIR long enough to be partitioned, a cascade that hardly
    forgets, poles that repeat."""
    def lag(taps_n, sos):
        fir, iir = dev.FirStream(sps.firwin(taps_n, 0.2), 2), dev.SosStream(sos, 2)
        try:
            return dev.chain_zp_lag(fir, iir)
        finally:
            fir.close()
            iir.close()
    assert lag(1024, BP) == 768          # three rows of left tail at the default cut (1e-15)
    assert lag(1900, BP) == 768         # (blocks of 23 rows since round 5; rounds 3-4 refused above 1793 taps)
    assert lag(3000, BP) == -1          # a partitioned FIR
    assert lag(256, sps.butter(4, [0.0002, 0.0016], "bandpass", output="sos")) == -1
    assert lag(256, np.vstack([sps.butter(2, 0.2, output="sos")] * 2)) == -1


def test_full_size_chunks_linearity_and_checksum(dev):
    """BASELINE cfg-3's chunk shape (256 channels x 2^20 samples, three chunks): the kernel is
    linear (a x1 + b x2 in = a y1 + b y2 out, to rounding) and reproducible bit for bit."""
    import torch
    h = sps.firwin(1024, 0.2)
    C, cs = 256, 1 << 20
    x1 = [dev.synth_normal(C, cs, seed=11, n0=k * cs) for k in range(3)]
    x2 = [dev.synth_normal(C, cs, seed=12, n0=k * cs) for k in range(3)]

    def run(chunks):
        fir, iir = dev.FirStream(h, C), dev.SosStream(BP, C)
        try:
            iir.set_state(None)
            dev.chain_zp_open(fir, iir, 0)
            return [dev.chain_zp_step(fir, iir, c) for c in chunks]
        finally:
            fir.close()
            iir.close()

    y1, y2 = run(x1), run(x2)
    y12 = run([0.5 * a - 2.0 * b for a, b in zip(x1, x2)])
    again = run(x1)
    for k in range(3):
        want = 0.5 * y1[k] - 2.0 * y2[k]
        assert float((y12[k] - want).abs().max()) < 1e-12 * float(want.abs().max())
        assert torch.equal(again[k].view(torch.int64), y1[k].view(torch.int64))


def test_public_generators_take_the_kernel_and_match_the_reference_scheme(dev):
    """FIR producer -> sosfiltfilt generator on device-resident data: the zero-phase flow
    (numerical._zero_phase_stream) chunk for chunk against the two-kernel flow
    (OSZ_CHAIN_ZP=0) and against the oracle's oaconvolve('same') -> chunk-local sosfiltfilt
    on three channels: odd and even left cuts, ragged last chunk, a stream ending exactly on
    a chunk, a real pole."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm

    def chain(x, taps, sos, cs):
        src = producer(x, cs, -1)
        fir = producer(partial(nm.oaconvolve, src, taps, -1, "same"), cs, -1, shape=src.shape)
        return [c for c in nm.sosfiltfilt(fir, sos, -1)]

    for taps_n, sos, C, cs, total in ((1024, BP, 256, 6144 * 24, 6144 * 24 * 6 + 6144 * 9 + 321),
                                      (301, BP, 5, 100000, 100000 * 8),
                                      (64, sps.butter(5, 0.3, output="sos"), 4, 70001, 70001 * 7 + 5)):
        taps = sps.firwin(taps_n, 0.2)
        x = dev.synth_normal(C, total, seed=44)
        steps, plain_zp = [], dev.chain_zp_step
        dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain_zp(*a, **k))[1]
        try:
            got = chain(x, taps, sos, cs)
        finally:
            dev.chain_zp_step = plain_zp
        assert len(steps) == -(-total // cs) - 2, (taps_n, len(steps))
        os.environ["OSZ_CHAIN_ZP"] = "0"
        try:
            ref = chain(x, taps, sos, cs)
        finally:
            del os.environ["OSZ_CHAIN_ZP"]
        assert [g.shape for g in got] == [r.shape for r in ref], taps_n
        for k, (a, b) in enumerate(zip(got, ref)):
            err = float((a - b).abs().max()) / float(b.abs().max())
            assert err < 1e-11, (taps_n, C, k, err)
        pick = [0, C // 2, C - 1]
        xh = x[pick].cpu().numpy()
        want = orc.sosfiltfilt(np.concatenate(orc.oaconvolve(xh, taps, "same"), -1), sos, cs)
        gh = torch.cat(got, -1)[pick].cpu().numpy()
        assert np.max(np.abs(gh - want)) < RTOL * np.max(np.abs(want)), taps_n


@pytest.mark.gpu
@pytest.mark.parametrize("fed", ["resident", "host"])
def test_plain_sosfiltfilt_takes_the_zero_phase_kernel(dev, fed):
    """sosfiltfilt with NO FIR in front of it (core/numerical.py:338-411) on long streams of
    long chunks: the zero-phase kernel with the identity as its FIR, chunk for chunk against
    the separate kernels (OSZ_CHAIN_ZP=0) and against the oracle's chunk-local scheme --
    resident and host-fed, a ragged last chunk and a stream ending on a chunk boundary, a
    cascade with a real pole, the sample axis first; a cascade the tables refuse (a narrow
    band: ringing longer than the guard rows) and a short stream stay on the separate kernels."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm

    def run(x, sos, cs, axis):
        return [c for c in nm.sosfiltfilt(producer(x, cs, axis), sos, axis)]

    narrow = sps.butter(4, [0.01, 0.02], "bandpass", output="sos")
    # (the last-but-two: the worst-conditioned fit the tables admit, 1e-16 / ratio = 3e-10 of the
    # output scale: 1e-9 asserted chunk for chunk where the others hold 1e-11)
    for sos, C, cs, total, axis, zp in ((BP, 64, 131072, 131072 * 6 + 4321, -1, True),
                                        (sps.butter(5, 0.3, output="sos"), 5, 70000, 70000 * 7, 0, True),
                                        (sps.cheby1(6, 0.5, 0.2, output="sos"), 3, 100001, 100001 * 6 + 17, -1, True),
                                        # a left tail of six rows: blocks of 26, the eight-row instance
                                        (sps.butter(6, [0.05, 0.2], "bandpass", output="sos"), 4, 131072,
                                         131072 * 6 + 77, -1, True),
                                        # a left tail of nine rows (the alpha / beta band-pass of SURVEY 8d at the
                                        # default cut): blocks of 23, the twelve-row instance, held rows in both
                                        # halves of the window
                                        (sps.butter(6, [8 / 250, 30 / 250], "bandpass", output="sos"), 4, 131072,
                                         131072 * 6 + 77, -1, True),
                                        # eight sections alone: its fit wants 2 x 24 samples, which fit beside the
                                        # cube since the burst rows come by products instead of from a table
                                        (sps.butter(8, [0.05, 0.3], "bandpass", output="sos"), 3, 131072,
                                         131072 * 6 + 4099, -1, True),
                                        (narrow, 4, 131072, 131072 * 6 + 5, -1, False),
                                        (BP, 4, 131072, 131072 * 5, -1, False)):
        xd = dev.synth_normal(C, total, seed=71)
        if axis == 0:
            xd = xd.t().contiguous()
        x = xd.cpu().numpy() if fed == "host" else xd
        steps, plain_zp = [], dev.chain_zp_step
        dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain_zp(*a, **k))[1]
        try:
            got = run(x, sos, cs, axis)
        finally:
            dev.chain_zp_step = plain_zp
        nchunks = -(-total // cs)
        assert len(steps) == (nchunks - 2 if zp else 0), (C, cs, len(steps))
        os.environ["OSZ_CHAIN_ZP"] = "0"
        try:
            ref = run(x, sos, cs, axis)
        finally:
            del os.environ["OSZ_CHAIN_ZP"]
        assert [g.shape for g in got] == [r.shape for r in ref]
        assert all(isinstance(g, np.ndarray) == (fed == "host") for g in got)
        to_np = (lambda a: a) if fed == "host" else (lambda a: a.cpu().numpy())
        tol = 1e-9 if (C, cs) in ((4, 131072), (3, 131072)) and zp else 1e-11      # (the ill-conditioned fits: 1e-16 / ratio)
        for k, (a, b) in enumerate(zip(got, ref)):
            a, b = to_np(a), to_np(b)
            assert np.max(np.abs(a - b)) < tol * np.max(np.abs(b)), (C, cs, k)
        gh = np.concatenate([to_np(g) for g in got], axis)
        xh = xd.cpu().numpy()
        if axis == 0:
            gh, xh = gh.T, xh.T
        pick = [0, C // 2, C - 1]
        want = orc.sosfiltfilt(xh[pick], sos, cs)
        assert np.max(np.abs(gh[pick] - want)) < RTOL * np.max(np.abs(want)), (C, cs)


def _large_inputs(dev, kind, C, cs, nchunks, extra):
    """Streams whose magnitude is far above their in-band signal, the way raw recordings are:
    (x, the noise alone).  The system is linear, so the oracle on the noise alone gives the
    in-band output's scale."""
    import torch
    total = cs * nchunks + extra
    noise = dev.synth_normal(C, total, seed=91)
    x = noise.clone()
    sign = torch.tensor([[1.0], [-1.0], [0.3]], dtype=torch.float64, device="cuda")[:C]
    if kind == "offset 1e4 + drift":
        ramp = torch.linspace(0.0, 1.0, total, dtype=torch.float64, device="cuda")[None]
        x += 1e4 + 2e3 * ramp * sign
    elif kind == "step to 1e6 at chunk 3":            # an electrode pop / a DC step, far behind any first look
        x[:, 3 * cs + 1234:] += 1e6 * sign
    elif kind == "rail for 5000 samples":             # an amplifier in saturation, mid-stream
        a = 4 * cs + 40000
        x[:, a:a + 5000] = 1e6 * sign
    elif kind == "offset 1e7":
        x += 1e7 * sign
    else:
        raise ValueError(kind)
    return x, noise


LARGE = ["offset 1e4 + drift", "step to 1e6 at chunk 3", "rail for 5000 samples", "offset 1e7"]


def _magnitude_bound(x, inband):
    """What a float64 path may differ by from another float64 path on this input: the suite's
    1e-9 of the in-band output's scale, plus float64's own rounding on the INPUT's magnitude --
    a 4096-point transform there and back on samples of magnitude max|x| rounds at about 90 eps
    max|x| (measured: 2.0e-8 at 10^6, 1.9e-7 at 10^7; the cut itself is 0.3e-15 max|x|, a
    sixtieth of that), the reference's own FFT convolution and recurrences at eps max|x| and up.
    256 eps max|x| bounds it.  Nothing else grows with the input."""
    return RTOL * inband + 256 * np.finfo(np.float64).eps * float(np.max(np.abs(x)))


@pytest.mark.gpu
@pytest.mark.parametrize("after_fir", [True, False])
@pytest.mark.parametrize("kind", LARGE)
def test_input_magnitude_is_not_in_the_error(dev, kind, after_fir):
    """What the zero-phase kernel cuts off (its bursts, at a tolerance relative to the norm of
    the composite impulse response) scales with the INPUT's magnitude.  Rounds 3-4 cut at 1e-12
    and asked for 1e-15 after a look at the first 8192 samples of the first chunk; an offset
    that appeared later got the loose cut.  The cut is 1e-15 for every
    stream now, which is float64's own rounding on the input: offsets of 10^4 with a drift,
    a step to 10^6 at chunk 3 of 8, a rail of 10^6 for 5000 samples mid-stream and an offset
    of 10^7 from sample 0 all stay within 1e-9 of the in-band output's scale + 256 eps max|x|
    (float64's rounding in a transform of such samples) of the oracle's chunk-local scheme
    (core/numerical.py:338-411) -- measured 8e-9 of the in-band scale at 10^6 and 7e-8 at 10^7,
    the contract is 1e-6 -- on the one-kernel route (asserted), behind a FIR and alone, seam
    chunks included."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    C, cs = 3, 65536
    taps = sps.firwin(256, 0.4)
    x, noise = _large_inputs(dev, kind, C, cs, 8, 12345)
    steps, plain_zp = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain_zp(*a, **k))[1]
    try:
        src = producer(x, cs, -1)
        if after_fir:
            src = producer(partial(nm.oaconvolve, src, taps, -1, "same"), cs, -1, shape=src.shape)
        got = torch.cat([c for c in nm.sosfiltfilt(src, BP, -1)], -1).cpu().numpy()
    finally:
        dev.chain_zp_step = plain_zp
    assert len(steps) == 7, len(steps)            # nine chunks: all but the last two on the kernel

    def oracle(arr):
        u = np.concatenate(orc.oaconvolve(arr, taps, "same"), -1) if after_fir else arr
        return orc.sosfiltfilt(u, BP, cs)

    xh = x.cpu().numpy()
    want = oracle(xh)
    inband = float(np.max(np.abs(oracle(noise.cpu().numpy()))))
    err = float(np.max(np.abs(got - want)))
    assert err < _magnitude_bound(xh, inband), (kind, err, inband)
    assert err < 1e-6 * inband, (kind, err, inband)                     # north_star's contract
    # the suite's 1e-9 of the output scale -- except under the offset of 10^7, where the output IS
    # the in-band signal (no transient: the forward pass starts from sosfilt_zi * x[0]) and 1e-9 of
    # it lies below float64's rounding of the input (eps max|x| = 1e-9 per operation, in the
    # reference's recurrences as in any transform): there the two bounds above are what holds
    if kind != "offset 1e7":
        assert err < RTOL * float(np.max(np.abs(want))), (kind, err)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LARGE[:3])
def test_input_magnitude_forward_chain(dev, kind):
    """The same for the public sosfilt behind a FIR producer (osz_chain_forward's spectral
    kernels cut the cascade's right tail at the same tolerance): within the same
    bound of the oracle's oaconvolve -> sosfilt (core/numerical.py:158-298 into :301-335)."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    C, cs = 3, 65536
    taps = sps.firwin(256, 0.4)
    x, noise = _large_inputs(dev, kind, C, cs, 8, 12345)
    fused, plain = [], dev.chain_forward
    dev.chain_forward = lambda *a, **k: (fused.append(1), plain(*a, **k))[1]
    try:
        src = producer(x, cs, -1)
        fir = producer(partial(nm.oaconvolve, src, taps, -1, "same"), cs, -1, shape=src.shape)
        got = torch.cat([c for c in nm.sosfilt(fir, BP, -1)], -1).cpu().numpy()
    finally:
        dev.chain_forward = plain
    assert len(fused) == 8, len(fused)

    def oracle(arr):
        return orc.sosfilt(np.concatenate(orc.oaconvolve(arr, taps, "same"), -1), BP, cs)[0]

    xh = x.cpu().numpy()
    want = oracle(xh)
    inband = float(np.max(np.abs(oracle(noise.cpu().numpy()))))
    err = float(np.max(np.abs(got - want)))
    assert err < _magnitude_bound(xh, inband), (kind, err, inband)
    assert err < 1e-6 * inband and err < RTOL * float(np.max(np.abs(want))), (kind, err, inband)


@pytest.mark.gpu
def test_few_channels_take_several_chunks_per_launch(dev):
    """At 32 channels a launch over one 2^20-sample chunk runs at 0.7 of the 256-channel rate
    (what it pays once -- tables, every run's pre-roll block, the launch -- over ten blocks per
    workgroup).  Chunks of a resident source that lie one behind the other in memory go through
    the zero-phase kernel 2^28 / (C x chunksize) at a time (numerical._zp_group); the generator still yields
    chunk-sized arrays, the same as with one launch per chunk (OSZ_ZP_GROUP=1) to rounding and
    within 1e-9 of the oracle's chunk-local scheme (core/numerical.py:338-411).  Host-fed
    streams and sources whose chunks are separate buffers keep one launch per chunk."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    taps = sps.firwin(301, 0.3)
    C, cs, nchunks = 32, 65536, 23
    total = cs * (nchunks - 1) + 4321
    x = dev.synth_normal(C, total, seed=5)

    def run(data, after_fir, make=None):
        sizes, plain = [], dev.chain_zp_step
        dev.chain_zp_step = lambda *a, **k: (sizes.append(a[2].shape[1] // cs), plain(*a, **k))[1]
        try:
            src = make() if make else producer(data, cs, -1)
            if after_fir:
                src = producer(partial(nm.oaconvolve, src, taps, -1, "same"), cs, -1, shape=src.shape)
            return [c for c in nm.sosfiltfilt(src, BP, -1)], sizes
        finally:
            dev.chain_zp_step = plain

    for after_fir in (True, False):
        got, sizes = run(x, after_fir)
        # chunk 0 alone (the stream's start), then as many as make 2^28 channel-samples (64 at most):
        # chunks 1-20 -- all there are before the stream's last two -- in one step
        assert sizes == [1, 20], sizes
        os.environ["OSZ_ZP_GROUP"] = "8"
        try:
            _, sizes8 = run(x, after_fir)
        finally:
            del os.environ["OSZ_ZP_GROUP"]
        assert sizes8 == [1, 8, 8, 4], sizes8
        assert [g.shape[-1] for g in got] == [cs] * (nchunks - 1) + [4321]
        os.environ["OSZ_ZP_GROUP"] = "1"
        try:
            one, sizes1 = run(x, after_fir)
        finally:
            del os.environ["OSZ_ZP_GROUP"]
        assert sizes1 == [1] * (nchunks - 2)
        y, y1 = torch.cat(got, -1), torch.cat(one, -1)
        assert float((y - y1).abs().max()) < 1e-12 * float(y1.abs().max())
        pick = [0, 17, 31]
        xh = x[pick].cpu().numpy()
        u = np.concatenate(orc.oaconvolve(xh, taps, "same"), -1) if after_fir else xh
        want = orc.sosfiltfilt(u, BP, cs)
        assert np.max(np.abs(y[pick].cpu().numpy() - want)) < RTOL * np.max(np.abs(want))
    # a single channel as a 1-D array (its chunk views carry a row pitch of their own length: the
    # joined view must not inherit it -- found by tests/fuzz_gpu.py)
    x1 = x[3, :cs * 9 + 99].contiguous()
    sizes, plain = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (sizes.append(a[2].shape[1] // cs), plain(*a, **k))[1]
    try:
        y1 = torch.cat(list(nm.sosfiltfilt(producer(x1, cs, 0), BP, 0)), 0).cpu().numpy()
    finally:
        dev.chain_zp_step = plain
    assert sizes == [1, 7], sizes
    want1 = orc.sosfiltfilt(x1.cpu().numpy()[None], BP, cs)[0]
    assert np.max(np.abs(y1 - want1)) < RTOL * np.max(np.abs(want1))
    # host data: every chunk through the staging ring, one launch each
    _, sizes = run(x.cpu().numpy()[:, :cs * 7], True)
    assert sizes == [1] * 5, sizes
    # a generating source (every chunk a buffer of its own): nothing to join
    def gen():
        for k in range(7):
            yield dev.synth_normal(C, cs, seed=5, n0=k * cs)
    _, sizes = run(None, False, make=lambda: producer(gen, cs, -1, shape=(C, 7 * cs)))
    assert sizes == [1] * 5, sizes


@pytest.mark.gpu
def test_tolerance_knob_reaches_every_table(dev):
    """osz_chain_zp_tolerance: 0 is the default (1e-15); a relaxed cut shortens the zero-phase
    kernel's lag, and the pair kernels' tables (build_zp builds them where the one-block tables are
    not eligible; it ignored the knob until round 5: ADVICE r4) follow it too -- checked through the
    lag, which is 256 x the left tail's rows for either kernel."""
    taps = sps.firwin(256, 0.4)
    f0, i0 = dev.FirStream(taps, 1), dev.SosStream(BP, 1)
    try:
        tight = dev.chain_zp_lag(f0, i0)
        dev.chain_zp_tolerance(f0, i0, 1e-12)
        loose = dev.chain_zp_lag(f0, i0)
        dev.chain_zp_tolerance(f0, i0, 0.0)
        again = dev.chain_zp_lag(f0, i0)
    finally:
        f0.close()
        i0.close()
    assert tight > loose > 0 and again == tight, (tight, loose, again)


@pytest.mark.gpu
@pytest.mark.parametrize("fed", ["resident", "host"])
def test_reference_outputs_where_the_route_engages(dev, golden, fed):
    """g18_chain_long.npz: outputs of the REFERENCE ITSELF (oaconvolve 'same' -> sosfiltfilt as
    chained producers, core/numerical.py:158-298 into :338-411; tests/golden/make_golden.py) at a
    geometry the zero-phase route takes -- 1024 taps, the 6-section band-pass of cfg-3, six
    chunks of 65 536 + a ragged one; channel 1 on an offset of 10^4 with a drift.  The public
    generators run it with osz_chain_zp_step for chunks 0 .. 4 (asserted) and match the
    reference's numbers to 1e-9 of each channel's output scale, resident and host-fed."""
    import torch
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    g = golden("g18_chain_long.npz")
    x, want, h, sos, cs = g["x32"].astype(np.float64), g["y"], g["h"], g["sos"], int(g["chunksize"])
    src_data = x if fed == "host" else torch.from_numpy(x).cuda()
    steps, plain = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain(*a, **k))[1]
    try:
        src = producer(src_data, cs, -1)
        fir = producer(partial(nm.oaconvolve, src, h, -1, "same"), cs, -1, shape=src.shape)
        pieces = [c for c in nm.sosfiltfilt(fir, sos, -1)]
    finally:
        dev.chain_zp_step = plain
    nchunks = -(-x.shape[1] // cs)
    assert len(steps) == nchunks - 2 == 5, len(steps)
    assert [p.shape[-1] for p in pieces] == list(g["piece_lengths"])
    got = np.concatenate([p if isinstance(p, np.ndarray) else p.cpu().numpy() for p in pieces], -1)
    for c in range(x.shape[0]):
        scale = np.max(np.abs(want[c]))
        assert np.max(np.abs(got[c] - want[c])) < RTOL * scale, (c, np.max(np.abs(got[c] - want[c])) / scale)


def _coverage_filters():
    from openseize_amd.core import numerical as nm
    from openseize_amd.filtering import iir
    return [
        ("headline", sps.butter(6, [0.05, 0.3], "bandpass", output="sos"), True),
        ("Butter [8, 30] / [3, 60] Hz at 500 Hz", iir.Butter(fpass=[8, 30], fstop=[3, 60], fs=500, gpass=1, gstop=40).coeffs, True),
        ("Cheby1 [200, 600] / [150, 650] Hz at 2500 Hz", iir.Cheby1(fpass=[200, 600], fstop=[150, 650], fs=2500).coeffs, False),
        ("0.5-4 Hz at 5 kHz", sps.butter(4, [0.0002, 0.0016], "bandpass", output="sos"), False),
        ("eight sections", sps.butter(8, [0.05, 0.3], "bandpass", output="sos"), True),
        ("Notch(60, 8, 500)", nm._ba_to_sos(iir.Notch(60, 8, 500).coeffs)[0], True),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_routes_and_parity_of_realistic_cascades(dev, which):
    """The six cascades of profiles/r04_zp_coverage.jsonl behind a 1024-tap FIR through the public
    generators, against the oracle's oaconvolve('same') -> chunk-local sosfiltfilt
    (core/numerical.py:158-298, :338-411) at 1e-9: the headline, the class-API cfg-3 of SURVEY 8d,
    the reference's own Cheby1 test filter (tests/test_iir.py:132-158: nine sections), SURVEY 7's
    stress filter, an eight-section band-pass, the Notch.  Four of them take the one-kernel
    route (asserted); nine sections and a band 0.0002 of Nyquist wide stay on the separate kernels."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import producer
    from openseize_amd.core import numerical as nm
    name, sos, zp = _coverage_filters()[which]
    sos = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    C, cs = 3, 65536
    total = 6 * cs + 4321
    taps = sps.firwin(1024, 0.2)
    x = dev.synth_normal(C, total, seed=300 + which)
    steps, plain = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain(*a, **k))[1]
    try:
        src = producer(x, cs, -1)
        fir = producer(partial(nm.oaconvolve, src, taps, -1, "same"), cs, -1, shape=src.shape)
        got = torch.cat([c for c in nm.sosfiltfilt(fir, sos, -1)], -1).cpu().numpy()
    finally:
        dev.chain_zp_step = plain
    assert len(steps) == (5 if zp else 0), (name, len(steps))
    want = orc.sosfiltfilt(np.concatenate(orc.oaconvolve(x.cpu().numpy(), taps, "same"), -1), sos, cs)
    assert np.max(np.abs(got - want)) < RTOL * np.max(np.abs(want)), name


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_forward_chain_routes_and_parity(dev, which):
    """The same six cascades behind a 1024-tap FIR through osz_chain_forward (FIR -> sosfilt, one
    launch per chunk), held against the oracle: np.convolve's meaning of the overlap add
    (core/numerical.py:158-298) into the DF2T cascade (scipy's sosfilt, :338-386), three chunks
    with the carried states between them and a ragged last one.  Which kernel ran is asserted
    (osz_chain_forward_route): the one-block kernel without its left tail for four of them, the
    scan in time for nine sections and for the band 0.0002 of Nyquist wide."""
    from oracle import oracle as orc
    name, sos, spectral = _coverage_filters()[which]
    sos = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    C, lens = 3, (200000, 200000, 77777)
    taps = sps.firwin(1024, 0.2)
    x = dev.synth_normal(C, sum(lens), seed=500 + which)
    fir, iir = dev.FirStream(taps, C), dev.SosStream(sos, C)
    assert dev.chain_forward_route(fir, iir) == (2 if spectral else 0), name
    got, n0 = [], 0
    for n in lens:
        got.append(dev.chain_forward(fir, iir, x[:, n0:n0 + n].contiguous()).cpu().numpy())
        n0 += n
    fir.close(); iir.close()
    got = np.concatenate(got, -1)
    u = orc.convolve_direct(x.cpu().numpy(), taps, "full")[:, :sum(lens)]
    want, _ = orc.sosfilt(u, sos, sum(lens))
    assert np.max(np.abs(got - want)) < RTOL * np.max(np.abs(want)), name
