"""GPU parity: the HIP path (through the C ABI) against the golden vectors the
reference produced and against the CPU oracle on seeded inputs.

Tolerance: BASELINE.json's north_star asks for 1e-6 relative on float64 filter
outputs and bit-exact indexing/masking.  The float checks below use
RTOL = 1e-9 of the output scale (three orders tighter than required).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(np.max(np.abs(b))), 1e-300)
    return float(np.max(np.abs(a - b))) / scale


@pytest.fixture(scope="module")
def osz():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import openseize_amd  # noqa: F401
    from openseize_amd import _lib
    _lib.load()      # fails loudly if the HIP library was not built
    from openseize_amd.core import numerical as nm
    return nm


def producer(*a, **k):
    from openseize_amd import producer as p
    return p(*a, **k)


# --------------------------------------------------------------------- FIR
@pytest.mark.parametrize("taps", [76, 255, 256, 1024])
@pytest.mark.parametrize("mode", ["full", "same", "valid"])
def test_oaconvolve_golden(osz, golden, taps, mode):
    g = golden("g2_fir.npz")
    x, h = g["x"], g[f"h{taps}"]
    for cs in (1000, 4096):
        y = np.concatenate(list(osz.oaconvolve(producer(x, cs, -1), h, -1, mode)), -1)
        assert rel_err(y, g[f"y_t{taps}_{mode}"]) < RTOL


def test_oaconvolve_long_and_axis(osz, golden):
    g = golden("g2_fir.npz")
    x, h = g["x_long"], g["h76"]
    for mode in ("full", "same", "valid"):
        y = np.concatenate(list(osz.oaconvolve(producer(x, 16384, -1), h, -1, mode)), -1)
        assert rel_err(y[:, :400], g[f"ylong_{mode}_head"]) < RTOL
        assert rel_err(y[:, -400:], g[f"ylong_{mode}_tail"]) < RTOL
        assert rel_err(y[:, ::37], g[f"ylong_{mode}_dec"]) < RTOL
    y = np.concatenate(list(osz.oaconvolve(
        producer(g["x3"], 700, 1), g["kaiser_h"], 1, "same")), 1)
    assert rel_err(y, g["kaiser_axis1_same"]) < RTOL


def test_fir_class_api(osz, golden):
    from openseize_amd.filtering.fir import Kaiser
    g = golden("g2_fir.npz")
    kais = Kaiser(fpass=200, fstop=400, fs=5000, gpass=0.5, gstop=40)
    assert np.array_equal(kais.coeffs, g["kaiser_h"])
    xk = g["xk"]
    for mode in ("full", "same", "valid"):
        y = kais(xk, chunksize=2000, axis=-1, mode=mode)
        assert isinstance(y, np.ndarray)
        assert rel_err(y, g[f"kaiser_arr_{mode}"]) < RTOL
        res = kais(producer(xk, 2000, -1), chunksize=2000, axis=-1, mode=mode)
        assert [a.shape[-1] for a in res] == list(g[f"kaiser_pro_len_{mode}"])
        assert tuple(res.shape) == tuple(g[f"kaiser_pro_shape_{mode}"])


def test_remez_class_api(osz, golden):
    """A Remez design applied through FIR.__call__ (array in -> array out, producer in ->
    producer out) against the reference's output (tests/golden/g16_remez.npz)."""
    from openseize_amd.filtering.fir import Remez
    g = golden("g16_remez.npz")
    filt = Remez(bands=[0, 300, 400, 800, 900, 2500], desired=[0, 1, 0], fs=5000, gpass=.5, gstop=40)
    assert np.array_equal(filt.coeffs, g["coeffs0"])
    y = filt(g["x"], chunksize=4000, axis=-1, mode="same")
    assert isinstance(y, np.ndarray) and rel_err(y, g["y0_same"]) < RTOL
    res = filt(producer(g["x"], 4000, -1), chunksize=4000, axis=-1, mode="full")
    assert [a.shape[-1] for a in res] == list(g["y0_full_lens"])


def test_impulse_responses_golden(osz, golden):
    """impulse_response() runs a unit pulse through the filter's own streaming path:
    against the reference's (filtering/mixins.py:226-238, :279-286)."""
    from openseize_amd.filtering.fir import Kaiser
    from openseize_amd.filtering.iir import Butter, Notch
    g = golden("g17_responses.npz")
    filts = {"butter": Butter(fpass=[8, 30], fstop=[3, 60], fs=500, gpass=1, gstop=40),
             "notch": Notch(60, 8, 500),
             "kaiser": Kaiser(fpass=200, fstop=400, fs=5000, gpass=0.5, gstop=40)}
    for name, filt in filts.items():
        resp = filt.impulse_response()
        want = g[f"{name}_impulse"]
        assert resp.shape == want.shape, name
        assert np.max(np.abs(resp - want)) < 1e-12 * np.max(np.abs(want)), name


def test_oaconvolve_edges(osz):
    rng = np.random.default_rng(1)
    from oracle import oracle as orc
    # data shorter than the window -> ValueError (reference: broadcasting ValueError)
    with pytest.raises(ValueError):
        list(osz.oaconvolve(producer(rng.standard_normal((2, 50)), 10, -1),
                            np.ones(64), -1, "same"))
    # the reference's quirk lengths: plain np.convolve answer here
    h = np.hanning(9) / 4
    for n in (4087, 4088, 4089, 9, 10):
        x = rng.standard_normal((2, n))
        for mode in ("full", "same", "valid"):
            y = np.concatenate(list(osz.oaconvolve(producer(x, 1000, -1), h, -1, mode)), -1)
            assert rel_err(y, orc.convolve_direct(x, h, mode)) < RTOL
    # chunks of 1 sample, single tap, max supported taps, tiny chunks vs oracle
    x = rng.standard_normal((3, 300))
    for taps, cs in ((1, 7), (2049, 100000), (33, 1), (300, 299)):
        xx = rng.standard_normal((2, 5000)) if taps > 300 else x
        h = rng.standard_normal(taps)
        y = np.concatenate(list(osz.oaconvolve(producer(xx, cs, -1), h, -1, "full")), -1)
        assert rel_err(y, orc.convolve_direct(xx, h, "full")) < RTOL


def test_documented_divergences_are_exactly_these(osz, golden):
    """DESIGN section 2 lists the inputs on which the product deliberately does NOT
    follow the reference; this pins which inputs those are and what comes back.
    Q12: the reference's short-data fallback with an odd nfft raises inside the overlap
    add (flag recorded by make_golden.py from the reference itself, numerical.py:210-249);
    the product returns the linear convolution.  Q3: data shorter than the window is a
    ValueError on both sides.  Q13: FIR.__call__ along axis 0 raises IndexError in the
    reference (filtering/bases.py:411); here it filters along that axis."""
    from oracle import oracle as orc
    from openseize_amd.filtering.fir import Kaiser
    g = golden("g2_fir.npz")
    assert bool(g["quirk_odd_fallback_raises"])          # what the reference did
    x, h = g["x"][:, :5003], g["h1024"]
    with pytest.raises(ValueError):                      # the oracle follows the reference
        orc.oaconvolve(x, h, "same")
    for mode in ("full", "same", "valid"):
        y = np.concatenate(list(osz.oaconvolve(producer(x, 1000, -1), h, -1, mode)), -1)
        assert rel_err(y, orc.convolve_direct(x, h, mode)) < RTOL
    # the even neighbour is NOT a divergence: golden outputs of the reference
    y = np.concatenate(list(osz.oaconvolve(producer(g["x"], 1000, -1), h, -1, "same")), -1)
    assert rel_err(y, g["y_t1024_same"]) < RTOL
    with pytest.raises(ValueError):
        list(osz.oaconvolve(producer(x[:, :500], 100, -1), h, -1, "same"))
    kais = Kaiser(fpass=30, fstop=60, fs=500, gpass=1, gstop=40)
    xt = np.ascontiguousarray(g["x"].T)                  # samples along axis 0
    y0 = kais(xt, chunksize=1000, axis=0, mode="same")
    y1 = kais(g["x"], chunksize=1000, axis=-1, mode="same")
    assert y0.shape == xt.shape and rel_err(y0.T, y1) < RTOL


def test_oaconvolve_every_block_height(osz):
    """One filter length in each of eight ranges of 200 taps, 1850 ... 2049 down to 58 ... 257:
    fir_part_push sends every one of them to fir_nega_kernel, and they happen to land on its
    eight block heights, NB = 24 ... 31 (8 ... 15 were the rows of fir_oa_kernel, which these
    filters ran before fir_nega_kernel arrived; this test does not assert which instance
    runs -- tests/test_gpu_fir_cells.py does, and reaches the runs of several whole blocks
    that three channels never get here).  In one chunk and in several (tail carried across
    pushes, ragged last block), and a partitioned filter (accumulating stores)."""
    from scipy.signal import oaconvolve as sp_oa
    rng = np.random.default_rng(77)
    x = rng.standard_normal((3, 150001))
    for rows in range(8, 16):
        taps = 4096 - 256 * rows + 1 - int(rng.integers(0, 200))
        h = rng.standard_normal(taps) / np.sqrt(taps)
        for cs in (150001, 40000):
            y = np.concatenate(list(osz.oaconvolve(producer(x, cs, -1), h, -1, "full")), -1)
            assert rel_err(y, sp_oa(x, h[None], axes=-1)) < RTOL, (rows, taps, cs)
    h = rng.standard_normal(4500) / 70
    y = np.concatenate(list(osz.oaconvolve(producer(x, 150001, -1), h, -1, "same")), -1)
    assert rel_err(y, sp_oa(x, h[None], mode="same", axes=-1)) < RTOL


def test_oaconvolve_long_filters(osz):
    """More than 2049 taps: the filter is cut into 2048-tap pieces whose
    delayed outputs are accumulated (partitioned overlap-add)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(31)
    x = rng.standard_normal((2, 30011))
    for taps, cs in ((2050, 100000), (4097, 3000), (5000, 777), (9001, 12000)):
        h = rng.standard_normal(taps) / taps
        for mode in ("full", "same", "valid"):
            y = np.concatenate(list(osz.oaconvolve(producer(x, cs, -1), h, -1, mode)), -1)
            assert rel_err(y, orc.convolve_direct(x, h, mode)) < RTOL
    with pytest.raises(NotImplementedError):
        list(osz.oaconvolve(producer(rng.standard_normal((1, 40000)), 5000, -1),
                            np.ones(16 * 2048 + 1), -1, "full"))


# --------------------------------------------------------------------- SOS
FILTERS = ["butter_lp", "butter_bp6", "cheby1_bp", "butter_cls6"]


@pytest.mark.parametrize("name", FILTERS)
def test_sosfilt_golden(osz, golden, name):
    g = golden("g3_sosfilt.npz")
    x, sos = g["x"], g[f"sos_{name}"]
    for cs in (1000, 4096):
        y = np.concatenate(list(osz.sosfilt(producer(x, cs, -1), sos, -1)), -1)
        assert rel_err(y, g[f"y_{name}_cs{cs}"]) < RTOL
    y = np.concatenate(list(osz.sosfilt(producer(x, 1000, -1), sos, -1,
                                        zi=g[f"zi_{name}"])), -1)
    assert rel_err(y, g[f"yzi_{name}"]) < RTOL


def test_sosfilt_axis_and_state(osz, golden):
    g = golden("g3_sosfilt.npz")
    y = np.concatenate(list(osz.sosfilt(producer(g["x3"], 1000, 1),
                                        g["sos_butter_lp"], 1)), 1)
    assert rel_err(y, g["y3_butter_lp"]) < RTOL
    # ragged chunking (tiles, partial tiles, 1-sample chunks) against the oracle
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    import torch
    rng = np.random.default_rng(5)
    sos = g["sos_butter_bp6"]
    x = rng.standard_normal((5, 70001))
    ref, zf = orc.sosfilt(x, sos, 70001)
    st = dev.SosStream(sos, 5)
    xd = torch.from_numpy(x).cuda()
    cuts = [0, 1, 2, 33, 2048, 2049, 16384 + 2049, 16384 * 3 + 7, 70000, 70001]
    out = [st.forward(xd[:, a:b].contiguous()).cpu().numpy()
           for a, b in zip(cuts[:-1], cuts[1:])]
    assert rel_err(np.concatenate(out, -1), ref) < RTOL
    assert rel_err(st.get_state(), zf) < 1e-7
    st.close()


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("cs", [200, 1000, 4096, 6007])
def test_sosfiltfilt_golden(osz, golden, name, cs):
    g = golden("g4_sosfiltfilt.npz")
    y = np.concatenate(list(osz.sosfiltfilt(producer(g["x"], cs, -1),
                                            g[f"sos_{name}"], -1)), -1)
    assert rel_err(y, g[f"y_{name}_cs{cs}"]) < RTOL


def test_iir_class_api(osz, golden):
    from openseize_amd.filtering.iir import Butter
    g = golden("g4_sosfiltfilt.npz")
    butter = Butter(fpass=[8, 30], fstop=[3, 60], fs=500, gpass=1, gstop=40)
    y = butter(g["x"], chunksize=2000, axis=-1, dephase=True)
    assert isinstance(y, np.ndarray) and rel_err(y, g["cls_dephase"]) < RTOL
    y = butter(g["x"], chunksize=2000, axis=-1, dephase=False)
    assert rel_err(y, g["cls_causal"]) < RTOL


@pytest.mark.parametrize("name", ["butter_lp", "cheby1_bp", "ellip_lp", "butter_bp", "notch"])
def test_ba_filters_golden(osz, golden, name):
    """lfilter / filtfilt (ba format) run as a biquad cascade on the device.
    Tolerance 1e-7: the cascade and the reference's direct form are two
    realisations of the same transfer function (measured <= 3e-8 apart on
    these filters, the 18th-order direct form being the inaccurate one)."""
    from openseize_amd.filtering.bases import IIR
    g = golden("g10_ba.npz")
    x, coeffs = g["x"], (g[f"b_{name}"], g[f"a_{name}"])
    for cs in (1000, 4000):
        y = np.concatenate(list(osz.lfilter(producer(x, cs, -1), coeffs, -1)), -1)
        assert rel_err(y, g[f"lfilter_{name}_cs{cs}"]) < 1e-7
        y = np.concatenate(list(osz.filtfilt(producer(x, cs, -1), coeffs, -1)), -1)
        assert rel_err(y, g[f"filtfilt_{name}_cs{cs}"]) < 1e-7
    if name == "notch":
        y = np.concatenate(list(osz.lfilter(producer(x, 1000, -1), coeffs, -1,
                                            zi=g["notch_zi"])), -1)
        assert rel_err(y, g["notch_lfilter_zi"]) < RTOL
        from openseize_amd.filtering.iir import Notch
        notch = Notch(60, 8, 500)
        assert np.array_equal(notch.coeffs[0], coeffs[0])
        y = notch(np.ascontiguousarray(x.T), chunksize=1500, axis=0, dephase=True)
        assert rel_err(y, g["notch_axis0"]) < 1e-7
    else:
        # a user zi of any order is mapped onto the cascade states
        import scipy.signal as sps
        zi = np.random.default_rng(3).standard_normal((x.shape[0], len(coeffs[1]) - 1))
        want, _ = sps.lfilter(coeffs[0], coeffs[1], x, axis=-1, zi=zi)
        got = np.concatenate(list(osz.lfilter(producer(x, 1000, -1), coeffs, -1, zi=zi)), -1)
        assert rel_err(got, want) < 1e-6          # north_star's bar; the direct form is the noisy side


def test_sos_stress_narrowband(osz):
    """Poles close to the unit circle (0.5-4 Hz band at fs = 5 kHz): the
    block-parallel scan must stay within tolerance of the serial recurrence."""
    import scipy.signal as sps
    from oracle import oracle as orc
    sos = sps.butter(3, [0.5, 4], "bandpass", fs=5000, output="sos")
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, 120000)) + 5.0
    ref, _ = orc.sosfilt(x, sos, 120000)
    y = np.concatenate(list(osz.sosfilt(producer(x, 50000, -1), sos, -1)), -1)
    assert rel_err(y, ref) < 1e-8
    ref = orc.sosfiltfilt(x, sos, 50000)
    y = np.concatenate(list(osz.sosfiltfilt(producer(x, 50000, -1), sos, -1)), -1)
    assert rel_err(y, ref) < 1e-8


def test_sosfiltfilt_warmup_truncation(osz, golden):
    """The backward warm-up stops after warmup_len samples (the point where the
    cascade's transition matrix has decayed below 1e-18): results must equal the
    oracle, which back-filters the whole next chunk like the reference."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    g = golden("g4_sosfiltfilt.npz")
    rng = np.random.default_rng(11)
    x = rng.standard_normal((4, 90000))
    for name in ("butter_bp6", "cheby1_bp"):
        sos = g[f"sos_{name}"]
        st = dev.SosStream(sos, 4)
        wl = st.lib.osz_sos_warmup_len(st.h)
        st.close()
        assert 0 < wl < 30000          # truncation is active for 30000-sample chunks
        y = np.concatenate(list(osz.sosfiltfilt(producer(x, 30000, -1), sos, -1)), -1)
        assert rel_err(y, orc.sosfiltfilt(x, sos, 30000)) < 1e-12


def test_sos_time_split_few_channels(osz, golden):
    """With few channels a chunk is cut into time segments that start from a
    zero state warmup_len samples early (sos_split_kernel): forward, carried
    state and forward-backward results must still equal the serial oracle."""
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    import torch
    g = golden("g4_sosfiltfilt.npz")
    rng = np.random.default_rng(13)
    x = rng.standard_normal((3, 300001)) + 2.0
    for name in ("butter_bp6", "butter_lp"):
        sos = g[f"sos_{name}"]
        ref, zf = orc.sosfilt(x, sos, 300001)
        y = np.concatenate(list(osz.sosfilt(producer(x, 131072, -1), sos, -1)), -1)
        assert rel_err(y, ref) < 1e-12
        st = dev.SosStream(sos, 3)
        xd = torch.from_numpy(x).cuda()
        st.forward(xd[:, :262144].contiguous())
        assert rel_err(st.get_state(), orc.sosfilt(x[:, :262144], sos, 262144)[1]) < 1e-9
        st.close()
        y = np.concatenate(list(osz.sosfiltfilt(producer(x, 131072, -1), sos, -1)), -1)
        assert rel_err(y, orc.sosfiltfilt(x, sos, 131072)) < 1e-12


# --------------------------------------------------------------- resampling
@pytest.mark.parametrize("LM", [(1, 5), (3, 1), (3, 2), (2, 7), (3, 11)])
def test_resample_golden(osz, golden, LM):
    from openseize_amd.resampling.resampling import resample
    g = golden("g5_resample.npz")
    L, M = LM
    for cs in (3000, 7001):
        y = resample(g["x"], L, M, 5000, chunksize=cs, axis=-1)
        assert rel_err(y, g[f"y_L{L}_M{M}_cs{cs}"]) < RTOL
    pro = resample(producer(g["x"], 3000, -1), L, M, 5000, 3000, axis=-1)
    assert [a.shape[-1] for a in pro] == list(g[f"len_L{L}_M{M}"])
    assert tuple(pro.shape) == tuple(g[f"shape_L{L}_M{M}"])


def test_resample_wrappers(osz, golden):
    from openseize_amd.resampling.resampling import downsample, upsample, resample
    g = golden("g5_resample.npz")
    x = g["x"]
    assert rel_err(downsample(x, 5, 5000, chunksize=4000, axis=-1), g["down5"]) < RTOL
    assert rel_err(upsample(x[:, :6000], 3, 5000, chunksize=2000, axis=-1), g["up3"]) < RTOL
    xt = np.ascontiguousarray(x[:2, :5000].T)
    assert rel_err(downsample(xt, 5, 5000, chunksize=1000, axis=0), g["down5_axis0"]) < RTOL
    assert downsample(x, 1, 5000, 1000) is x and resample(x, 4, 4, 5000, 1000) is x
    with pytest.raises(ValueError):
        downsample(x[:, :5], 5, 5000, chunksize=1000)


def test_downsample_every_tile_shape(osz):
    """Decimators from M = 2 to M = 40: the window of M phase streams picks the
    256-, 128- or 64-thread tile and, on the two smaller ones, the kernel with
    two phase groups per workgroup -- all against whole-array
    scipy.signal.resample_poly with the same filter (what the reference calls
    per chunk, core/numerical.py:610)."""
    import scipy.signal as sps
    from oracle import oracle as orc
    from openseize_amd.filtering.fir import Kaiser
    from openseize_amd.resampling.resampling import downsample
    rng = np.random.default_rng(41)
    fs = 20480.0
    x = rng.standard_normal((3, 300007))
    for M in (2, 3, 7, 8, 10, 13, 16, 25, 40):
        cutoff = fs / (2 * M)
        h = Kaiser(cutoff - cutoff / 10, cutoff + cutoff / 10, fs, gpass=0.1, gstop=40).coeffs
        want = orc.polyphase_resample(x, 1, M, h)
        assert rel_err(want, sps.resample_poly(x, 1, M, axis=-1, window=h)) < RTOL
        for cs in (300007, 65536 + 11):
            y = downsample(x, M, fs, chunksize=cs, axis=-1)
            assert rel_err(y, want) < RTOL, (M, cs, len(h))


# ------------------------------------------------------------------ spectra
def test_periodogram_golden(osz, golden):
    g = golden("g6_periodogram.npz")
    x = g["x"]
    for window in ("hann", "hamming", "boxcar", "blackman"):
        for detrend in ("constant", "linear"):
            for scaling in ("density", "spectrum"):
                f, p = osz.periodogram(x, 500, None, window, -1, detrend, scaling)
                assert rel_err(p, g[f"p_{window}_{detrend}_{scaling}"]) < RTOL
    assert np.array_equal(f, g["freqs"])
    f, X = osz.modified_dft(x, 500, 1024, "hann", -1, "constant", "density")
    assert X.shape == g["dft_hann"].shape
    assert np.max(np.abs(X - g["dft_hann"])) < RTOL * np.max(np.abs(g["dft_hann"]))
    f, p = osz.periodogram(x[:, :1023], 500)
    assert rel_err(p, g["p_odd"]) < RTOL and np.array_equal(f, g["freqs_odd"])
    f, p = osz.periodogram(x, 500, 2048)
    assert rel_err(p, g["p_pad2048"]) < RTOL
    f, p = osz.periodogram(x, 500, 512, "hann", -1, "linear", "spectrum")
    assert rel_err(p, g["p_crop512"]) < RTOL
    with pytest.raises(ValueError):
        osz.modified_dft(x, 500, 1024, "hann", -1, "constant", "power")
    with pytest.raises(ValueError):
        osz.periodogram(np.zeros((3, 0)), 500)


def test_psd_golden(osz, golden):
    from openseize_amd.spectra.estimators import psd
    g = golden("g7_welch.npz")
    x = g["x"]
    for ov in (0.0, 0.5, 0.6):
        cnt, f, p = psd(x, 1024, axis=-1, resolution=1.0, overlap=ov)
        assert cnt == int(g[f"cnt_ov{ov}"])
        assert rel_err(p, g[f"psd_ov{ov}"]) < RTOL
        assert np.array_equal(f, g["freqs"])
    cnt, f, p = psd(x, 1024, axis=-1, resolution=0.5, window="hamming",
                    detrend="linear", scaling="spectrum")
    assert cnt == int(g["cnt_hamming"])
    assert rel_err(p, g["psd_hamming_linear_spectrum"]) < RTOL
    cnt, f, p = psd(np.ascontiguousarray(x[:2].T), 1000, axis=0, resolution=2.0)
    assert cnt == int(g["cnt_axis0"]) and rel_err(p, g["psd_axis0_nfft500"]) < RTOL


def test_welch_producer(osz, golden):
    g = golden("g7_welch.npz")
    pro = producer(g["x"], 5000, -1)
    f, wp = osz.welch(pro, 1024, 1024, "hann", 0.5, -1, "constant", "density")
    segs = list(wp)
    assert tuple(wp.shape) == tuple(g["welch_shape"])
    assert len(segs) == int(g["welch_nseg"])
    assert rel_err(segs[0], g["welch_seg0"]) < RTOL
    assert rel_err(segs[-1], g["welch_seg_last"]) < RTOL


def test_stft_golden(osz, golden):
    from openseize_amd.spectra.estimators import stft
    g = golden("g8_stft.npz")
    x = g["x"]
    for b in (True, False):
        for p in (True, False):
            for scaling in ("density", "spectrum"):
                f, t, X = stft(x, 256, axis=-1, resolution=1.0, boundary=b,
                               padded=p, scaling=scaling, asarray=True)
                key = f"b{int(b)}_p{int(p)}_{scaling}"
                assert X.shape == g[f"X_{key}"].shape
                assert np.allclose(t, g[f"t_{key}"], rtol=0, atol=1e-12)
                assert np.max(np.abs(X - g[f"X_{key}"])) < RTOL * np.max(np.abs(g[f"X_{key}"]))
                assert np.array_equal(f, g["freqs"])
    f, t, pro = stft(producer(x, 1000, -1), 256, axis=-1, resolution=0.5,
                     overlap=0.75, detrend="linear", window="hamming",
                     asarray=False)
    assert tuple(pro.shape) == tuple(g["pro_shape"])
    assert np.allclose(t, g["pro_t"])
    X = np.stack(list(pro), axis=-1)
    assert np.max(np.abs(X - g["pro_X"])) < RTOL * np.max(np.abs(g["pro_X"]))


def test_spectra_fused_4096(osz):
    """nfft = 4096 takes the fused on-chip path (pairs of segments per
    transform): check all three modes, both detrends, odd and even segment
    counts and ragged pushes against the oracle, the staged rocFFT route and the
    fft8 kernel."""
    import os
    from oracle import oracle as orc
    from openseize_amd.spectra.estimators import psd, stft
    rng = np.random.default_rng(21)
    x = rng.standard_normal((3, 47001)) + np.linspace(0, 2, 47001)
    fs = 4096
    for ov in (0.5, 0.0, 0.75):
        for detrend in ("constant", "linear"):
            cnt, f, p = psd(x, fs, axis=-1, resolution=1.0, overlap=ov, detrend=detrend)
            c2, f2, p2 = orc.psd(x, fs, resolution=1.0, overlap=ov, detrend=detrend)
            assert cnt == c2 and np.array_equal(f, f2)
            assert rel_err(p, p2) < RTOL
    # per-segment producers, chunksize that splits segments across pushes
    pro = producer(x, 5000, -1)
    f, wp = osz.welch(pro, fs, 4096, "hamming", 0.5, -1, "linear", "spectrum")
    segs = list(wp)
    f2, ref = orc.welch_segments(x, fs, 4096, "hamming", 0.5, "linear", "spectrum")
    assert len(segs) == len(ref)
    for a, b in zip(segs, ref):
        assert rel_err(a, b) < RTOL
    f, t, X = stft(x, fs, axis=-1, resolution=1.0, boundary=True, padded=True)
    f2, t2, X2 = orc.stft(x, fs, resolution=1.0, boundary=True, padded=True)
    assert X.shape == X2.shape and np.allclose(t, t2)
    assert np.max(np.abs(X - X2)) < RTOL * np.max(np.abs(X2))
    # the cube, the fft8 kernel and the staged rocFFT route agree; which one a psd() took is
    # read off its handle's launch report
    from openseize_amd import _device as dev

    def routed(**env):
        seen, plain = set(), dev.SpecStream.push

        def push(self, x2d):
            out = plain(self, x2d)
            seen.update(r["family"] for r in self.last_launches())
            return out

        os.environ.update(env)
        dev.SpecStream.push = push
        try:
            cnt, _, p = psd(x, fs, axis=-1, resolution=1.0)
        finally:
            dev.SpecStream.push = plain
            for k in env:
                del os.environ[k]
        return seen, cnt, p

    fam1, cnt1, p1 = routed()
    fam8, cnt8, p8 = routed(OSZ_SPEC_FUSED="0")
    fam0, cnt0, p0 = routed(OSZ_SPEC_FUSED="0", OSZ_SPEC_V8="0", OSZ_SPEC_MIX="0")
    assert (fam1, fam8, fam0) == ({"cube"}, {"fft8"}, {"staged"})
    assert cnt0 == cnt1 and rel_err(p1, p0) < 1e-12
    assert cnt8 == cnt1 and rel_err(p1, p8) < 1e-12


# ------------------------------------------- device-resident chain + masking
def test_device_resident_chain(osz, golden):
    """CUDA tensors in -> CUDA tensors out, FIR -> sosfiltfilt chained as
    producers, equal to the host-fed result and to the oracle."""
    import torch
    from functools import partial
    from oracle import oracle as orc
    g = golden("g4_sosfiltfilt.npz")
    x, sos = g["x"], g["sos_butter_bp6"]
    h = golden("g2_fir.npz")["h256"]
    xd = torch.from_numpy(x).cuda()
    fir = producer(partial(osz.oaconvolve, producer(xd, 1500, -1), h, -1, "same"),
                   1500, -1, shape=x.shape)
    out = list(osz.sosfiltfilt(fir, sos, -1))
    assert all(o.is_cuda for o in out)
    y = torch.cat(out, -1).cpu().numpy()
    ref = orc.sosfiltfilt(orc.convolve_direct(x, h, "same"), sos, 1500)
    assert rel_err(y, ref) < RTOL


def test_device_resident_api(osz, golden):
    """Every public entry point accepts a CUDA tensor and answers with CUDA
    tensors equal to the host-fed (ndarray) result."""
    import torch
    from openseize_amd.filtering.fir import Kaiser
    from openseize_amd.filtering.iir import Butter
    from openseize_amd.resampling.resampling import downsample, resample
    from openseize_amd.spectra.estimators import psd, stft
    rng = np.random.default_rng(41)
    x = rng.standard_normal((3, 30000))
    xd = torch.from_numpy(x).cuda()
    kais = Kaiser(fpass=200, fstop=400, fs=5000, gpass=0.5, gstop=40)
    butter = Butter(fpass=[8, 30], fstop=[3, 60], fs=500, gpass=1, gstop=40)
    pairs = [
        (kais(xd, 7000, axis=-1, mode="same"), kais(x, 7000, axis=-1, mode="same")),
        (butter(xd, 7000, axis=-1, dephase=True), butter(x, 7000, axis=-1, dephase=True)),
        (butter(xd, 7000, axis=-1, dephase=False), butter(x, 7000, axis=-1, dephase=False)),
        (downsample(xd, 5, 5000, 7000), downsample(x, 5, 5000, 7000)),
        (resample(xd, 3, 2, 5000, 7000), resample(x, 3, 2, 5000, 7000)),
        (psd(xd, 1000, resolution=2.0)[2], psd(x, 1000, resolution=2.0)[2]),
        (stft(xd, 500, resolution=1.0)[2], stft(x, 500, resolution=1.0)[2]),
    ]
    for got, want in pairs:
        assert torch.is_tensor(got) and got.is_cuda
        g = got.cpu().numpy()
        assert g.shape == want.shape
        assert np.max(np.abs(g - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300)
    # a producer over a device tensor stays a producer of device tensors
    pro = butter(producer(xd, 7000, -1), 7000, axis=-1)
    assert all(c.is_cuda for c in pro)


def test_c_abi_error_codes(osz):
    """Status codes of the C ABI map to the exception types of the Python
    boundary; handles refuse inconsistent arguments instead of faulting."""
    import ctypes
    import torch
    from openseize_amd import _device as dev, _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    bad = np.ones((1, 6))
    bad[0, 3] = 2.0                                   # a0 != 1
    assert lib.osz_sos_create(ctypes.byref(h), dev.host_dp(bad), 1, 4) == _lib.OSZ_ERR_INVALID
    assert b"should be all ones" in lib.osz_last_error()
    with pytest.raises(ValueError):
        dev.SosStream(np.ones((2, 5)), 4)             # wrong sos shape
    with pytest.raises(ValueError):
        dev.SosStream(np.array([[1.0, 0, 0, 1, 0, 0]]), 4).set_state(np.zeros((1, 3, 2)))
    with pytest.raises(ValueError):
        dev.SpecStream(128, 64, 32, np.ones(128), 1.0, "constant", 0, 2)   # nfft < nwin
    with pytest.raises(ValueError):
        dev.SpecStream(64, 64, 32, np.ones(64), 1.0, "cubic", 0, 2)        # unknown detrend
    fir = dev.FirStream(np.ones(8), 2)
    x = torch.zeros((2, 100), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        fir.push(x, skip=101)
    fir.close()
    with pytest.raises(NotImplementedError):
        dev.FirStream(np.ones(16 * 2048 + 1), 1)


def test_masked_producer_device(osz, golden):
    import torch
    g = golden("g1_producer.npz")
    x = g["x"]
    xd = torch.from_numpy(x).cuda()
    for name in ("rand", "hole", "short"):
        pro = producer(xd, 1000, -1, mask=g[f"mask_{name}"])
        chunks = list(pro)
        assert [c.shape[-1] for c in chunks] == list(g[f"masked_{name}_len_cs1000"])
        y = torch.cat(chunks, -1).cpu().numpy()
        assert np.array_equal(y, g[f"masked_{name}_cat_cs1000"])      # bit exact
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    y = torch.cat(list(producer(xt, 1000, 0, mask=g["mask_rand"])), 0).cpu().numpy()
    assert np.array_equal(y, g["masked_axis0_cat"])


# ------------------------------------------- full-size properties (cfg shapes)
def test_fullsize_properties(osz):
    """BASELINE chunk shape (256 ch x 2^20): linearity of the FIR and SOS
    paths, impulse response of the FIR = the taps, and chunking invariance of
    the carried state -- size-independent checks that need no CPU reference."""
    import scipy.signal as sps
    import torch
    from openseize_amd import _device as dev
    C, n = 256, 1 << 20
    h = sps.firwin(1024, 0.2)
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    a = dev.synth_normal(C, n, seed=1)
    b = dev.synth_normal(C, n, seed=2)

    def run_fir(x):
        f = dev.FirStream(h, C)
        y = f.push(x)
        f.close()
        return y

    def run_sos(x, pieces=1):
        s = dev.SosStream(sos, C)
        out = [s.forward(p.contiguous()) for p in torch.chunk(x, pieces, dim=1)]
        s.close()
        return torch.cat(out, 1)

    for run in (run_fir, run_sos):
        lhs = run(a + 2.0 * b)
        rhs = run(a) + 2.0 * run(b)
        assert float((lhs - rhs).abs().max()) < 1e-10 * float(rhs.abs().max())
    # impulse -> taps at every channel
    imp = torch.zeros((C, n), dtype=torch.float64, device="cuda")
    imp[:, 12345] = 1.0
    y = run_fir(imp)
    got = y[:, 12345:12345 + 1024].cpu().numpy()
    assert np.max(np.abs(got - h[None, :])) < 1e-14
    assert float(y[:, :12345].abs().max()) < 1e-14
    # carried state: one chunk == seven ragged chunks
    assert float((run_sos(a, 1) - run_sos(a, 7)).abs().max()) < 1e-10
    # order-independent checksum is reproducible
    assert dev.checksum(a)[0] == dev.checksum(dev.synth_normal(C, n, seed=1))[0]


def test_fullsize_properties_resample_spectra(osz):
    """BASELINE shapes for the other kernels (256 ch x 2^20 per GPU shard):
    size-independent properties that need no CPU reference.
    * decimation by 5 of a slow sinusoid (far inside the pass band) returns the
      sinusoid sampled every 5th point, and the resampler is linear;
    * Welch PSD (nfft 4096, 50 %): Parseval -- the one-sided density of white
      noise integrates to its variance; a pure tone puts its power in one bin;
    * the segment average is invariant to how the stream is cut into pushes."""
    import scipy.signal as sps
    import torch
    from openseize_amd import _device as dev, _lib
    from openseize_amd.filtering.fir import Kaiser
    C, n = 256, 1 << 20
    # ---- polyphase
    cutoff = 5000 / 10
    h = Kaiser(cutoff - cutoff / 10, cutoff + cutoff / 10, 5000, gpass=0.1, gstop=40).coeffs
    tt = torch.arange(n, dtype=torch.float64, device="cuda")
    tone = torch.sin(2 * np.pi * 3.0 / 5000 * tt).repeat(C, 1)     # 3 Hz at fs 5000
    a = dev.synth_normal(C, n, seed=5)

    def down(x):
        p = dev.PolyStream(h, 1, 5, C)
        y = p.push(x, final=True)
        p.close()
        return y

    yt = down(tone)
    assert yt.shape == (C, -(-n // 5))
    ref = tone[:, ::5]
    core = slice(200, yt.shape[1] - 200)                  # away from the zero-padded edges
    gain = float(np.sum(h))                               # DC gain of the Kaiser design
    assert float((yt[:, core] - gain * ref[:, core]).abs().max()) < 2e-3   # pass-band ripple 0.1 dB
    assert float((down(a + 3.0 * tone) - (down(a) + 3.0 * yt)).abs().max()) < 1e-11
    # ---- Welch
    nfft, fs = 4096, 4096.0
    w = sps.get_window("hann", nfft)
    scale = float(np.sqrt(1 / (fs * np.sum(w ** 2))))

    def welch(x, cuts):
        s = dev.SpecStream(nfft, nfft, nfft // 2, w, scale, "constant", _lib.SPEC_PSD_MEAN, C)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            s.push(x[:, lo:hi].contiguous())
        cnt, mean = s.mean()
        s.close()
        return cnt, mean

    cnt, p = welch(a, [0, n])
    assert cnt == (n - nfft) // (nfft // 2) + 1
    var = p.sum(axis=1) * (fs / nfft)                     # integral of the density
    assert np.all(np.abs(var - 1.0) < 0.02)               # N(0,1): variance 1 (511 segments)
    cnt2, p2 = welch(a, [0, 5000, 5001, 300000, 777777, n])
    assert cnt2 == cnt and np.max(np.abs(p2 - p)) < 1e-12 * np.max(p)
    tone2 = torch.sin(2 * np.pi * 512.0 / fs * tt).repeat(C, 1)    # exactly bin 512
    _, pt = welch(tone2, [0, n])
    assert np.all(np.argmax(pt, axis=1) == 512)
    assert np.all(np.abs(pt.sum(axis=1) * (fs / nfft) - 0.5) < 1e-6)    # power of a unit sine


def test_shapes_and_dtypes(osz):
    """1-D input, float32 input, a non-contiguous view and a 4-D array with the
    sample axis in the middle all go through the same (channels, samples)
    normalisation."""
    import scipy.signal as sps
    from oracle import oracle as orc
    rng = np.random.default_rng(51)
    sos = sps.butter(4, 0.2, output="sos")
    h = sps.firwin(31, 0.3)
    x1 = rng.standard_normal(5000)
    y = np.concatenate(list(osz.sosfilt(producer(x1, 1200, 0), sos, 0)))
    assert y.shape == x1.shape and rel_err(y, orc.sosfilt(x1[None], sos, 5000)[0][0]) < RTOL
    x32 = rng.standard_normal((2, 3000)).astype(np.float32)
    y = np.concatenate(list(osz.oaconvolve(producer(x32, 700, -1), h, -1, "same")), -1)
    assert y.dtype == np.float64
    assert rel_err(y, orc.convolve_direct(x32.astype(np.float64), h, "same")) < RTOL
    big = rng.standard_normal((4, 6000))
    view = big[::2, 1::2]                                     # non-contiguous
    y = np.concatenate(list(osz.sosfilt(producer(view, 1000, -1), sos, -1)), -1)
    assert rel_err(y, orc.sosfilt(np.ascontiguousarray(view), sos, 3000)[0]) < RTOL
    x4 = rng.standard_normal((2, 3, 2500, 2))
    y = np.concatenate(list(osz.oaconvolve(producer(x4, 600, 2), h, 2, "full")), 2)
    ref = orc.convolve_direct(np.moveaxis(x4, 2, -1), h, "full")
    assert rel_err(np.moveaxis(y, 2, -1), ref) < RTOL


def test_edf_reader_device_decode(osz, golden):
    """EDF records decoded on the device equal what the reference's Reader
    returns (bit exact: int16 * slope + offset with the reference's two
    roundings), including channels of different sample rates, padding, channel
    selection and the ReaderProducer path."""
    import os
    import torch
    from openseize_amd.file_io.edf import Reader
    g = golden("g11_edf.npz")
    path = os.path.join(os.path.dirname(__file__), "golden", "synthetic.edf")

    def same(a, b):
        return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)

    with Reader(path) as reader:
        assert same(reader.read(0), g["read_all"])
        assert same(reader.read(123, 4567), g["read_123_4567"])
        assert same(reader.read(4900, 5200), g["read_4900_5200"])
        assert same(reader.read(9990), g["read_9990_end"])
        assert same(reader.read(4000, 6000, padvalue=0.0), g["read_pad0"])
        assert reader.read(20000).shape == (4, 0)
        x = reader.read(123, 4567, device=True)
        assert torch.is_tensor(x) and x.is_cuda and same(x.cpu().numpy(), g["read_123_4567"])
        reader.channels = [0, 3]
        assert same(reader.read(250, 2750), g["read_ch03"])
        reader.channels = [2]
        assert same(reader.read(100, 4000), g["read_ch2"])
    pro = producer(Reader(path), 1700, axis=-1, start=300, stop=8000)
    assert [c.shape[-1] for c in pro] == list(g["pro2_len"])
    assert same(np.concatenate(list(pro), -1), g["pro2_cat"])
    # file -> device -> filter without float64 samples on the host
    import scipy.signal as sps
    dpro = producer(Reader(path), 1700, axis=-1, start=300, stop=5000, device=True)
    sos = sps.butter(2, 0.2, output="sos")
    chunks = list(osz.sosfilt(dpro, sos, -1))
    assert all(c.is_cuda for c in chunks)
    from oracle import oracle as orc
    ref, _ = orc.sosfilt(g["pro2_cat"][:, :4700], sos, 4700)
    assert rel_err(torch.cat(chunks, -1).cpu().numpy(), ref) < RTOL


def test_protools_device(osz, golden):
    """The producer-level glue keeps device-resident producers on the device
    and gives the reference's results."""
    import torch
    from openseize_amd.core import protools
    g = golden("g12_protools.npz")
    xd = torch.from_numpy(g["x"]).cuda()
    pro = producer(xd, 900, axis=-1)

    def eq(got, want):
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        return np.allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True)

    assert eq(protools.squeeze(pro).to_array(), g["x"][:, 0])
    assert eq(protools.add(pro, g["other"]).to_array(), g["add_arr"])
    assert eq(protools.multiply_along_axis(pro, g["w"], -1).to_array(), g["mul_along_prod"])
    assert eq(protools.slice_along_axis(pro, 10, 3000, 3, axis=-1).to_array(), g["slice_prod"])
    assert eq(protools.mean(pro, -1, True, keepdims=True), g["mean_prod_1"])
    assert eq(protools.std(pro, -1, True, keepdims=True), g["std_prod_1"])
    assert eq(protools.std(pro, 0), g["std_other"])
    out = protools.standardize(pro, -1)
    chunks = list(out)
    assert all(c.is_cuda for c in chunks)
    assert eq(torch.cat(chunks, -1), g["standardize_prod"])


def test_hilbert_analytic_signal(osz, golden):
    """Hilbert transformer (type III FIR) through the device FIR path: equals
    the reference's result; x + i*H(x) of a pass-band tone has unit envelope."""
    from openseize_amd.filtering.special import Hilbert
    g = golden("g13_hilbert.npz")
    filt = Hilbert(width=12.5, fs=500)
    y = filt(g["x"], chunksize=3000, axis=-1, mode="same")
    assert rel_err(y, g["imag_same"]) < RTOL
    t = np.arange(20000) / 500.0
    tone = np.cos(2 * np.pi * 60.0 * t)[None, :]
    env = np.abs(tone + 1j * filt(tone, chunksize=5000, axis=-1, mode="same"))
    core = slice(len(filt.coeffs), -len(filt.coeffs))
    assert np.max(np.abs(env[0, core] - 1.0)) < 2e-3        # gpass 0.01 dB


def test_analytic_transform_golden(osz, golden):
    """experimental.coupling.transforms.Analytic: x + i H(x)
    through the device FIR, amplitudes and phases in [0, 2 pi) equal the
    reference's."""
    from openseize_amd.experimental.coupling.transforms import Analytic
    g = golden("g14_metrics_analytic.npz")
    tr = Analytic(g["x"], fs=500, chunksize=2500, axis=-1, width=12.5)
    sig = tr.signal.to_array(dtype=complex)
    assert sig.shape == g["signal"].shape
    assert rel_err(sig.real, g["signal"].real) < RTOL
    assert rel_err(sig.imag, g["signal"].imag) < RTOL
    assert rel_err(tr.amplitudes.to_array(), g["amplitudes"]) < RTOL
    ph = tr.phases.to_array()
    assert ph.min() >= 0 and ph.max() < 2 * np.pi
    # compare on the unit circle (a phase next to 0 / 2 pi may wrap either way)
    assert np.max(np.abs(np.exp(1j * ph) - np.exp(1j * g["phases"]))) < 1e-8


def test_sos_alignment_paths(osz):
    """The SOS kernels stage 16 bytes per lane when a row is 16-byte aligned
    and 8 bytes otherwise: a device view that starts one sample into its
    buffer (8-byte aligned only) must give bit-identical results to an aligned
    copy of the same data, forward and zero-phase."""
    import torch
    import scipy.signal as sps
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    n = 4 * 8192
    buf = torch.randn((3, n + 2), dtype=torch.float64, device="cuda",
                      generator=torch.Generator(device="cuda").manual_seed(5))
    view = buf[:, 1:n + 1]                       # odd element offset
    aligned = view.clone()
    assert view.data_ptr() % 16 == 8 and aligned.data_ptr() % 16 == 0
    for fn in (osz.sosfilt, osz.sosfiltfilt):
        a = torch.cat(list(fn(producer(aligned, n // 2, -1), sos, -1)), -1)
        b = torch.cat(list(fn(producer(view, n // 2, -1), sos, -1)), -1)
        assert torch.equal(a, b)
    ref = sps.sosfilt(sos, aligned.cpu().numpy(), axis=-1)
    y = torch.cat(list(osz.sosfilt(producer(view, n // 2, -1), sos, -1)), -1).cpu().numpy()
    assert rel_err(y, ref) < RTOL


def test_long_stream_cfg3_direct(osz):
    """cfg-3 chain at the BASELINE chunksize (2^20) over a long stream, checked
    DIRECTLY against the CPU oracle on a 256-channel device-resident signal for
    three of its channels: 1024-tap FIR ('same') -> 6-section band-pass
    sosfiltfilt, 12 chunks (1.26e7 samples per channel), through the public
    producer API with CUDA tensors.  The oracle side uses SciPy's FFT
    convolution for the FIR (the direct form would take minutes) and the
    chunk-local zero-phase definition of the reference for the IIR."""
    import scipy.signal as sps
    import torch
    from functools import partial
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    C, cs, nchunks = 256, 1 << 20, 12
    n = cs * nchunks
    h = sps.firwin(1024, 0.2)
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    x = torch.cat([dev.synth_normal(C, cs, seed=11, n0=k * cs) for k in range(nchunks)], 1)
    fir = producer(partial(osz.oaconvolve, producer(x, cs, -1), h, -1, "same"), cs, -1,
                   shape=tuple(x.shape))
    pick = [0, 101, 255]
    got = []
    steps, plain = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.extend([1] * (a[2].shape[1] // cs)), plain(*a, **k))[1]
    try:
        for out in osz.sosfiltfilt(fir, sos, -1):
            assert out.is_cuda
            got.append(out[pick].cpu().numpy())
    finally:
        dev.chain_zp_step = plain
    assert len(steps) == nchunks - 2, len(steps)     # the headline's route: one zero-phase launch per chunk
    got = np.concatenate(got, -1)
    assert got.shape == (3, n)
    xh = x[pick].cpu().numpy()
    del x
    fir_ref = np.stack([sps.fftconvolve(row, h, mode="same") for row in xh])
    ref = orc.sosfiltfilt(fir_ref, sos, cs)
    assert rel_err(got, ref) < RTOL


def test_long_stream_cfg4_cfg5_direct(osz):
    """cfg-4 and cfg-5 at their BASELINE parameters over a long device-resident
    stream, checked DIRECTLY against the CPU oracle for three of 256 channels.
    cfg-4: psd(x, fs=4096, resolution=1.0, hann, 50 %, constant, density).
    cfg-5: downsample(x, M=5, fs=20480, chunksize=2^20) -> stft(y, fs=4096,
    resolution=1.0, boundary, padded) as a producer of segments."""
    import torch
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    from openseize_amd.resampling.resampling import downsample
    from openseize_amd.spectra.estimators import psd, stft
    C, cs, nchunks = 256, 1 << 20, 4
    n = cs * nchunks
    x = torch.cat([dev.synth_normal(C, cs, seed=12, n0=k * cs) for k in range(nchunks)], 1)
    pick = [0, 77, 255]
    xh = x[pick].cpu().numpy()
    # ---- cfg-4
    cnt, freqs, p = psd(x, fs=4096, axis=-1, resolution=1.0, window="hann", overlap=0.5,
                        detrend="constant", scaling="density")
    p = p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
    rc, rf, rp = orc.psd(xh, 4096, resolution=1.0)
    assert cnt == rc == (n - 4096) // 2048 + 1
    assert np.array_equal(freqs, rf)
    assert rel_err(p[pick], rp) < RTOL
    # ---- cfg-5
    y = downsample(producer(x, cs, -1), M=5, fs=20480, chunksize=cs, axis=-1)
    f, t, pro = stft(y, fs=4096, axis=-1, resolution=1.0, window="hann", overlap=0.5,
                     detrend="constant", scaling="density", boundary=True, padded=True,
                     asarray=False)
    yh = orc.polyphase_resample(xh, 1, 5, orc.resample_filter(1, 5, 20480))
    rf2, rt2, rX = orc.stft(yh, 4096, resolution=1.0)
    assert np.array_equal(f, rf2) and np.allclose(t, rt2, rtol=0, atol=1e-12)
    nseg = 0
    for k, seg in enumerate(pro):
        seg = seg[pick].cpu().numpy() if hasattr(seg, "cpu") else np.asarray(seg)[pick]
        assert np.max(np.abs(seg - rX[..., k])) < RTOL * np.max(np.abs(rX))
        nseg += 1
    assert nseg == rX.shape[-1]


def test_estimators_keep_producer_semantics(osz):
    """psd / stft set chunksize = int(fs) on the caller's producer (reference
    spectra/estimators.py:141) although the device work runs on a coarser copy;
    a masked producer goes through the same path and equals the estimate of
    the masked array."""
    from openseize_amd.spectra.estimators import psd, stft
    rng = np.random.default_rng(77)
    x = rng.standard_normal((3, 40000))
    pro = producer(x, 1000, -1)
    cnt, f, p = psd(pro, fs=256, axis=-1, resolution=1.0)
    assert pro.chunksize == 256
    cnt2, f2, p2 = psd(x, fs=256, axis=-1, resolution=1.0)
    assert cnt == cnt2 and rel_err(p, p2) < 1e-12
    mask = rng.random(40000) > 0.3
    mpro = producer(x, 1000, -1, mask=mask)
    cm, fm, pm = psd(mpro, fs=256, axis=-1, resolution=1.0)
    ca, fa, pa = psd(x[:, mask], fs=256, axis=-1, resolution=1.0)
    assert mpro.chunksize == 256 and cm == ca and rel_err(pm, pa) < 1e-12
    pro = producer(x, 1000, -1)
    f, t, X = stft(pro, fs=256, axis=-1, resolution=1.0)
    f2, t2, X2 = stft(x, fs=256, axis=-1, resolution=1.0)
    assert pro.chunksize == 256 and np.array_equal(t, t2) and rel_err(X, X2) < 1e-12


def test_handle_lifecycle_no_leak(osz):
    """Creating, using and destroying many iterator handles returns all the
    device memory the library allocated itself (tails workspace, states,
    tables of each handle): free memory before and after differs by less than
    a few MB."""
    import gc
    import scipy.signal as sps
    import torch
    from openseize_amd import _device as dev, _lib
    h = sps.firwin(300, 0.2)
    sos = sps.butter(4, 0.2, output="sos")
    w = sps.get_window("hann", 512)
    x = dev.synth_normal(8, 20000, seed=4)

    def cycle():
        f = dev.FirStream(h, 8); f.push(x); f.close()
        s = dev.SosStream(sos, 8); s.forward(x); s.close()
        p = dev.PolyStream(h, 3, 2, 8); p.push(x, final=True); p.close()
        sp = dev.SpecStream(512, 512, 256, w, 1.0, "constant", _lib.SPEC_PSD_MEAN, 8)
        sp.push(x); sp.close()

    for _ in range(5):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(150):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free0 - free1) < 64 << 20, (free0, free1)


def test_chain_forward_fused(osz):
    """osz_chain_forward (FIR feeding the forward SOS pass in one kernel, the
    FIR output never reaching HBM) equals osz_fir_push + osz_sos_forward, chunk
    after chunk with both carried states, for block lengths NR = 8, 12, 14,
    few and many channels (one and several runs per channel, i.e. with the
    zero-state pre-roll) and a ragged chunk end."""
    import scipy.signal as sps
    import torch
    from openseize_amd import _device as dev
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    for taps, C, n in ((1024, 256, 3 * 6144 * 30 + 777), (1024, 7, 1 << 20), (2049, 5, 400000),
                       (300, 3, 500000)):
        h = sps.firwin(taps, 0.2)
        xs = [dev.synth_normal(C, n, seed=9, n0=k * n) for k in range(3)]
        fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
        iir.set_state_scaled(xs[0], 0)
        ref = [iir.forward(fir.push(x, 0)) for x in xs]
        zref = iir.get_state()
        fir.close(); iir.close()
        fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
        iir.set_state_scaled(xs[0], 0)
        for k, x in enumerate(xs):
            f = dev.chain_forward(fir, iir, x)
            err = float((f - ref[k]).abs().max()) / float(ref[k].abs().max())
            assert err < 1e-12, (taps, C, n, k, err)
        assert np.allclose(iir.get_state(), zref, rtol=1e-10, atol=1e-12)
        fir.close(); iir.close()


def test_chain_step_overlapped(osz):
    """osz_chain_step (fused forward half on the caller's stream, backward pass of an
    earlier chunk beside it on the handle's own) against the single-stream kernel
    sequence osz_fir_push + osz_sosfiltfilt_step and against the CPU oracle, over a
    stream of chunks with a three-buffer ring (the next step's forward kernel
    reuses the buffer the previous backward pass read), ragged last chunk, few and
    many channels; carried states equal at the end."""
    import scipy.signal as sps
    import torch
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")
    for taps, C, cs, nchunks, last in ((1024, 256, 6144 * 24, 7, 6144 * 9 + 321),
                                       (300, 5, 200000, 6, 200000), (2049, 3, 120000, 5, 777)):
        h = sps.firwin(taps, 0.2)
        lens = [cs] * (nchunks - 1) + [last]
        xs, n0 = [], 0
        for n in lens:
            xs.append(dev.synth_normal(C, n, seed=31, n0=n0))
            n0 += n
        first = (xs[0][:, :1] * float(h[0])).contiguous()     # first sample of the FIR stream

        def run(mode):
            """'plain': fir.push + iir.step; 'step': osz_chain_step, stream ordered, ring of 3;
            'defer': osz_chain_step with OSZ_CHAIN_DEFER, ring of 3 (every step clashes with
            the pass in flight) and of 4 (none does); y taken one step late."""
            nring = 4 if mode == "defer4" else 3
            fir, iir = dev.FirStream(h, C), dev.SosStream(sos, C)
            iir.set_state_scaled(first, 0)
            ring = [torch.empty((C, cs), dtype=torch.float64, device="cuda") for _ in range(nring)]
            ys = [torch.empty((C, cs), dtype=torch.float64, device="cuda") for _ in range(2)]
            fwd, outs, late = [], [], None
            for k, x in enumerate(xs):
                buf = ring[k % nring][:, :x.shape[1]]
                if k < 2:
                    f = iir.forward(fir.push(x, 0), out=buf) if mode == "plain" else \
                        dev.chain_forward(fir, iir, x, out=buf)
                elif mode == "plain":
                    f, y = iir.step(fir.push(x, 0), fwd[k - 2], fwd[k - 1], f_out=buf)
                    outs.append(y.clone())
                elif mode == "step":
                    f, y = dev.chain_step(fir, iir, x, fwd[k - 2], fwd[k - 1], f_out=buf)
                    outs.append(y.clone())
                else:
                    yb = ys[k % 2][:, :fwd[k - 2].shape[1]]
                    f, y = dev.chain_step(fir, iir, x, fwd[k - 2], fwd[k - 1], f_out=buf, y_out=yb,
                                          defer=True)
                    if late is not None:
                        outs.append(late.clone())        # the previous step's y: ours now
                    late = y
                fwd.append(f)
            if late is not None:
                dev.chain_wait(iir)
                outs.append(late.clone())
            outs.append(iir.backward(fwd[-2], fwd[-1]).clone())
            outs.append(iir.backward(fwd[-1], None).clone())
            state = iir.get_state()
            fir.close()
            iir.close()
            return outs, state

        ref, zr = run("plain")
        for mode in ("step", "defer3", "defer4"):
            got, zg = run(mode)
            assert len(got) == len(ref) == len(xs)
            for k, (a, b) in enumerate(zip(got, ref)):
                err = float((a - b).abs().max()) / float(b.abs().max())
                assert err < 1e-11, (mode, taps, C, k, err)
            assert np.allclose(zg, zr, rtol=1e-10, atol=1e-12)
        # three channels against the oracle: the FIR stream (full mode, first N
        # samples), then the reference's chunk-local forward-backward filter
        pick = [0, C // 2, C - 1]
        xh = np.concatenate([x[pick].cpu().numpy() for x in xs], -1)
        fh = sps.oaconvolve(xh, h[None], axes=-1)[:, :xh.shape[1]]
        want = orc.sosfiltfilt(fh, sos, cs)
        gh = np.concatenate([g[pick].cpu().numpy() for g in got], -1)
        assert rel_err(gh, want) < RTOL, (taps, C)



def test_fir_then_sosfiltfilt_through_the_api_fused(osz):
    """FIR.__call__ feeding IIR.__call__ (dephase) on device-resident data takes the
    fused steady-state step (numerical._sosfiltfilt_after_fir) -- chunk for chunk
    the same as the two generators apart (OSZ_CHAIN_API=0), and the oracle's
    oaconvolve('same') -> chunk-local sosfiltfilt on three channels; odd and even
    left cuts, ragged last chunk, a stream ending exactly on a chunk, the ring's
    wrap (more than four chunks), few and many channels, sample axis first."""
    import os
    import scipy.signal as sps
    import torch
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    from openseize_amd.core import numerical as nm
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")

    def chain(x, taps, cs, axis):
        src = producer(x, cs, axis)
        fir = producer(partial(nm.oaconvolve, src, taps, axis, "same"), cs, axis, shape=src.shape)
        return [c for c in nm.sosfiltfilt(fir, sos, axis)]

    from functools import partial
    for taps_n, C, cs, total in ((1024, 256, 6144 * 24, 6144 * 24 * 6 + 6144 * 9 + 321),
                                 (301, 5, 100000, 100000 * 9), (2049, 3, 131072, 131072 * 4 + 777),
                                 # (2049 taps: blocks of 23 rows on the zero-phase kernel since round 5)
                                 (2049, 3, 131072, 131072 * 6 + 777), (64, 4, 70001, 70001 * 7 + 5)):
        taps = sps.firwin(taps_n, 0.2)
        x = dev.synth_normal(C, total, seed=44)
        steps, plain_step, plain_zp = [], dev.chain_step, dev.chain_zp_step
        dev.chain_step = lambda *a, **k: (steps.append("step"), plain_step(*a, **k))[1]
        dev.chain_zp_step = lambda *a, **k: (steps.extend(["zp"] * (a[2].shape[1] // cs)), plain_zp(*a, **k))[1]
        try:
            got = chain(x, taps, cs, -1)
        finally:
            dev.chain_step, dev.chain_zp_step = plain_step, plain_zp
        # the zero-phase kernel ran where it applies (six chunks or more, filters it takes: every
        # chunk but the last two, plus the head of the next for the seam); a shorter stream goes
        # through the two generators apart (round 5: no slower, and the reference FIR's NaN reach)
        nchunks = -(-total // cs)
        assert steps == (["zp"] * (nchunks - 2) if nchunks >= 6 else []), (taps_n, steps)
        os.environ["OSZ_CHAIN_API"] = "0"
        try:
            ref = chain(x, taps, cs, -1)
        finally:
            del os.environ["OSZ_CHAIN_API"]
        assert [g.shape for g in got] == [r.shape for r in ref], (taps_n, C)
        for k, (a, b) in enumerate(zip(got, ref)):
            err = float((a - b).abs().max()) / float(b.abs().max())
            assert err < 1e-11, (taps_n, C, k, err)
        pick = [0, C // 2, C - 1]
        xh = x[pick].cpu().numpy()
        want = orc.sosfiltfilt(np.concatenate(orc.oaconvolve(xh, taps, "same"), -1), sos, cs)
        gh = torch.cat(got, -1)[pick].cpu().numpy()
        assert rel_err(gh, want) < RTOL, (taps_n, C)
    # host-fed: ndarray chunks in, ndarray chunks out, one trip over PCIe each way
    taps = sps.firwin(513, 0.2)
    xh = np.random.default_rng(46).standard_normal((4, 90000 * 7 + 1234))
    steps, plain_zp = [], dev.chain_zp_step
    dev.chain_zp_step = lambda *a, **k: (steps.append(1), plain_zp(*a, **k))[1]
    try:
        got = chain(xh, taps, 90000, -1)
    finally:
        dev.chain_zp_step = plain_zp
    assert len(steps) == 8 - 2 and all(isinstance(g, np.ndarray) for g in got)
    assert [g.shape[-1] for g in got] == [90000] * 7 + [1234]
    want = orc.sosfiltfilt(np.concatenate(orc.oaconvolve(xh, taps, "same"), -1), sos, 90000)
    assert rel_err(np.concatenate(got, -1), want) < RTOL
    # sample axis first: (samples, channels)
    taps = sps.firwin(301, 0.2)
    xt = dev.synth_normal(6, 100000 * 6 + 31, seed=45).T.contiguous()
    got = torch.cat(chain(xt, taps, 100000, 0), 0)
    os.environ["OSZ_CHAIN_API"] = "0"
    try:
        ref = torch.cat(chain(xt, taps, 100000, 0), 0)
    finally:
        del os.environ["OSZ_CHAIN_API"]
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-11 * float(ref.abs().max())


@pytest.mark.gpu
def test_fir_then_sosfilt_through_the_api_fused(osz):
    """FIR.__call__ feeding IIR.__call__(phase-shifted: sosfilt) on device-resident data takes
    osz_chain_forward per chunk (numerical._sosfilt_after_fir) -- array for array the same as
    the two generators apart (OSZ_CHAIN_API=0), and the oracle's oaconvolve('same') -> sosfilt
    (core/numerical.py:158-298 feeding :301-335); odd and even left cuts, ragged last chunk, a
    stream ending exactly on a chunk, a start state zi, the scan-in-time route (2049 taps),
    sample axis first, host-fed data (ndarrays in and out); what the fused path does not take
    (a last chunk shorter than the cut) still comes out right."""
    import os
    from functools import partial
    import scipy.signal as sps
    import torch
    from oracle import oracle as orc
    from openseize_amd import _device as dev
    from openseize_amd.core import numerical as nm
    sos = sps.butter(6, [0.05, 0.3], "bandpass", output="sos")

    def chain(x, taps, cs, axis, zi=None):
        src = producer(x, cs, axis)
        fir = producer(partial(nm.oaconvolve, src, taps, axis, "same"), cs, axis, shape=src.shape)
        return [c for c in nm.sosfilt(fir, sos, axis, zi=zi)]

    def counted(x, taps, cs, axis, zi=None):
        calls, plain = [], dev.chain_forward
        dev.chain_forward = lambda *a, **k: (calls.append(1), plain(*a, **k))[1]
        try:
            return chain(x, taps, cs, axis, zi), len(calls)
        finally:
            dev.chain_forward = plain

    def apart(x, taps, cs, axis, zi=None):
        os.environ["OSZ_CHAIN_API"] = "0"
        try:
            return chain(x, taps, cs, axis, zi)
        finally:
            del os.environ["OSZ_CHAIN_API"]

    for taps_n, C, cs, total, fused in ((1024, 256, 6144 * 24, 6144 * 24 * 3 + 6144 * 9 + 321, True),
                                        (301, 5, 100000, 100000 * 5, True), (2049, 3, 131072, 131072 * 3 + 1777, True),
                                        (64, 4, 70001, 70001 * 4 + 45, True), (1024, 3, 70000, 70000 * 3 + 100, False)):
        taps = sps.firwin(taps_n, 0.2)
        x = dev.synth_normal(C, total, seed=47)
        zi = None if taps_n != 301 else np.random.default_rng(3).standard_normal((sos.shape[0], C, 2))
        got, ncalls = counted(x, taps, cs, -1, zi)
        nchunks = -(-total // cs)
        assert ncalls == (nchunks - 1 if fused else 0), (taps_n, ncalls)
        ref = apart(x, taps, cs, -1, zi)
        assert [g.shape for g in got] == [r.shape for r in ref], (taps_n, C)
        for k, (a, b) in enumerate(zip(got, ref)):
            err = float((a - b).abs().max()) / float(b.abs().max())
            assert err < 1e-11, (taps_n, C, k, err)
        # arrays of their own: no two of them share a sample (adjacent chunks of few channels may be
        # column ranges of ONE buffer since round 5 -- still memory nobody else writes)
        keep = [g.clone() for g in got]
        for k, g in enumerate(got):
            g.fill_(float(k))
        assert all(bool((g == float(k)).all()) for k, g in enumerate(got))
        for g, v in zip(got, keep):
            g.copy_(v)
        pick = [0, C // 2, C - 1]
        xh = x[pick].cpu().numpy()
        want, _ = orc.sosfilt(np.concatenate(orc.oaconvolve(xh, taps, "same"), -1), sos, cs,
                              zi=None if zi is None else zi[:, pick])
        gh = torch.cat(got, -1)[pick].cpu().numpy()
        assert rel_err(gh, want) < RTOL, (taps_n, C)
    # host-fed: ndarray chunks in, ndarray chunks out, one trip over PCIe each way
    taps = sps.firwin(513, 0.2)
    xh = np.random.default_rng(48).standard_normal((4, 90000 * 5 + 1234))
    got, ncalls = counted(xh, taps, 90000, -1)
    assert ncalls == 5 and all(isinstance(g, np.ndarray) for g in got)
    assert [g.shape[-1] for g in got] == [90000] * 5 + [1234]
    want, _ = orc.sosfilt(np.concatenate(orc.oaconvolve(xh, taps, "same"), -1), sos, 90000)
    assert rel_err(np.concatenate(got, -1), want) < RTOL
    # sample axis first: (samples, channels)
    taps = sps.firwin(301, 0.2)
    xt = dev.synth_normal(6, 100000 * 4 + 931, seed=49).T.contiguous()
    got, ncalls = counted(xt, taps, 100000, 0)
    assert ncalls == 4
    got, ref = torch.cat(got, 0), torch.cat(apart(xt, taps, 100000, 0), 0)
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-11 * float(ref.abs().max())


@pytest.mark.gpu
def test_polyphase_large_decimation_stays_on_the_tiled_kernel(osz):
    """Decimation by 13, 25 (the reference's tutorial: downsample(M=25), docs/tutorials/
    resampling.ipynb:650) and 40 with the default Kaiser design (293 / 561 / 895 taps): the
    window of the smallest tile takes 37 ... 113 KB of LDS and the tiled kernel still runs
    (one or two workgroups per CU) instead of the kernel that reads its window through the
    caches (60 ms instead of 0.93 per 256 x 2^20 at M = 25).  Ragged pushes against
    scipy.signal.resample_poly of the whole array (what core/numerical.py:597-632 assembles
    chunk by chunk)."""
    import scipy.signal as sps
    import torch
    from openseize_amd import _device as dev
    from openseize_amd.filtering.fir import Kaiser
    for M, cuts in ((13, (150001, 400000)), (25, (70000, 70025, 400000)), (40, (399999, 400000))):
        cut = 5000 / (2 * M)
        h = Kaiser(cut - cut / 10, cut + cut / 10, 5000, gpass=0.1, gstop=40).coeffs
        x = dev.synth_normal(5, 400000, seed=2)
        poly = dev.PolyStream(h, 1, M, 5)
        try:
            outs, lo = [], 0
            for hi in cuts:
                outs.append(poly.push(x[:, lo:hi].contiguous(), final=hi == cuts[-1]))
                lo = hi
        finally:
            poly.close()
        got = torch.cat(outs, 1).cpu().numpy()
        ref = sps.resample_poly(x.cpu().numpy(), 1, M, axis=-1, window=h)
        assert got.shape == ref.shape, (M, got.shape, ref.shape)
        assert np.max(np.abs(got - ref)) < 1e-12 * np.max(np.abs(ref)), M


@pytest.mark.parametrize("taps_n", [2, 257, 258, 1536, 2049, 2050])
def test_fir_block_heights_of_the_one_block_kernel(osz, taps_n):
    """fir_nega_kernel (csrc/fir.hip: one real block of 24 ... 31 rows per 4096-point transform)
    at the ends of its range of tap counts and just beyond (2050 taps: a partitioned filter on
    the pair kernel), three modes, ragged chunks, against numpy.convolve
    (core/numerical.py:158-298 equals it for every mode)."""
    import scipy.signal as sps
    from openseize_amd import _device as dev
    C, n, cs = 3, 200_003, 70_001
    x = dev.synth_normal(C, n, seed=800 + taps_n)
    h = sps.firwin(taps_n, 0.3) if taps_n > 2 else np.array([0.75, -0.25])
    xh = x.cpu().numpy()
    for mode in ("full", "same", "valid"):
        got = np.concatenate([c.cpu().numpy() for c in osz.oaconvolve(producer(x, cs, -1), h, -1, mode)], -1)
        want = np.stack([np.convolve(row, h, mode) for row in xh])
        assert got.shape == want.shape, (taps_n, mode)
        assert rel_err(got, want) < RTOL, (taps_n, mode)


@pytest.mark.gpu
def test_oaconvolve_few_channels_joined_chunks():
    """A resident stream of few channels goes through the FIR kernel several chunks per launch (round
    5: 256 / C adjacent views of one tensor at a time, as the zero-phase chain); the pieces the
    generator yields are the same chunk-aligned arrays as with one push per chunk (OSZ_ZP_GROUP=1),
    and their concatenation is np.convolve in every mode (core/numerical.py:158-298)."""
    import os
    import scipy.signal as sps
    import torch
    from openseize_amd import _device as dev
    from openseize_amd.core import numerical as nm
    C, cs, total = 4, 30000, 30000 * 9 + 1234
    x = dev.synth_normal(C, total, seed=9)
    xh = x.cpu().numpy()
    for taps_n in (64, 255, 1024):
        h = sps.firwin(taps_n, 0.3)
        for mode in ("same", "full", "valid"):
            pushes, plain = [], dev.FirStream.push

            def spy(self, x2d, *a, **k):
                pushes.append(x2d.shape[1])
                return plain(self, x2d, *a, **k)

            dev.FirStream.push = spy
            try:
                got = list(nm.oaconvolve(producer(x, cs, -1), h, -1, mode))
            finally:
                dev.FirStream.push = plain
            assert max(pushes) > cs, (mode, pushes)            # several chunks in one push
            os.environ["OSZ_ZP_GROUP"] = "1"
            try:
                one = list(nm.oaconvolve(producer(x, cs, -1), h, -1, mode))
            finally:
                del os.environ["OSZ_ZP_GROUP"]
            assert [g.shape[-1] for g in got] == [o.shape[-1] for o in one], (taps_n, mode)
            y = torch.cat(got, -1).cpu().numpy()
            want = np.stack([np.convolve(xh[c], h, mode) for c in range(C)])
            assert y.shape == want.shape and np.max(np.abs(y - want)) < 1e-12 * np.max(np.abs(want)), (taps_n, mode)


@pytest.mark.gpu
def test_reference_iir_chunksize_test_replayed():
    """The reference's own `test_sosfiltfilt_chunksizes` (/root/reference/tests/test_iir.py:132-158),
    statement for statement on the GPU path: a nine-section Chebyshev type I band-pass (200-600 Hz at
    fs 2500), a (101 400, 2, 4) array filtered along axis 0 at nine random chunksizes through the
    class API with dephase=True.  Its own bar -- allclose to SciPy's whole-array sosfiltfilt at
    atol 1e-4, the chunk-local backward passes being what they are (Q1) -- and this suite's: 1e-9 of
    the oracle's chunk-local scheme (core/numerical.py:338-411) at every one of them."""
    import scipy.signal as sps
    from oracle import oracle as orc
    from openseize_amd.filtering import iir
    rng = np.random.default_rng(9)
    axis, fs = 0, 2500
    arr = rng.random((101400, 2, 4))
    csizes = rng.integers(1000, 12300, size=9)
    filt = iir.Cheby1(fpass=[200, 600], fstop=[150, 650], fs=fs)
    assert filt.coeffs.shape == (9, 6)
    spresult = sps.sosfiltfilt(filt.coeffs, arr, axis=axis, padtype=None)
    flat = np.moveaxis(arr, axis, -1).reshape(8, -1)
    for csize in csizes:
        pro = producer(arr, chunksize=csize, axis=axis)
        pro_filt = filt(pro, chunksize=csize, axis=axis, dephase=True)
        oresult = np.concatenate([a for a in pro_filt], axis=axis)
        assert np.allclose(oresult, spresult, atol=1e-4), csize                 # the reference's assertion
        want = orc.sosfiltfilt(flat, filt.coeffs, int(csize))
        got = np.moveaxis(oresult, axis, -1).reshape(8, -1)
        assert np.max(np.abs(got - want)) < RTOL * np.max(np.abs(want)), csize
