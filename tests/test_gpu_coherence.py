"""GPU tests of window_coherence (K27) against ``window_coherence_measures``, the NumPy restatement
that tests/test_coherence_host.py pins.

Tolerances are those of tests/test_gpu_phase.py's header with N = nsub, per bin and averaged over the
band (``test_coherence_host.bounds``), with the suite's RTOL = 1e-9 of M = max|X| as the error of a
spectrum value: plv, imcoh and coh 4 RTOL M / min|X|; wpli 4 RTOL N M^2 / sum|d|; dwpli 16 RTOL N M^2
sum|d| / ((sum|d|)^2 - sum d^2); pli counts signs: entries with no unsafe segment (|d_s| < 20 RTOL
M^2) agree to 1e-12, an entry may differ by the band mean of 2 unsafe / N, and at most 1e-3 of the
(pair, bin) entries may be unsafe (the inputs stay ten times below that on the reference alone:
tests/test_coherence_host.py).  What must be the same bits is compared as bits.

The shapes (C, nperseg, h, nsub, m, nwin, bands in bins) are the smallest at which each part can go
wrong:
  (5, 64, 32, 7, 2, 6, ..)    overlapping windows; several windows per pass; three bands
  (17, 64, 32, 4, 1, 5, ..)   a one-bin band; one channel past two 8-channel blocks; m = 1
  (70, 128, 64, 3, 3, 3, ..)  several blocks with a partial last one; m = nsub; the least usable nsub
  (9, 256, 64, 5, 4, 3, ..)   a band of more than 64 bins (two passes per window); overlapping bands
  (6, 63, 21, 9, 1, 4, ..)    odd nperseg; a stride that is no power of two
  (2, 8, 4, 2, 2, 3, ..)      the least of everything
and a seventh here, (3, 64, 32, 2, 5, 3, ..), leaves gaps between the windows (m > nsub)."""

from functools import lru_cache

import numpy as np
import pytest

from test_coherence_host import NAMES, SHAPES, bounds, geometry, window_coherence_measures
from test_csd_host import signal
from test_phase_host import RTOL

pytestmark = pytest.mark.gpu

SAME = 1e-12
GAPS = (3, 64, 32, 2, 5, 3, ((2, 9), (9, 31)))
ALL = SHAPES + [GAPS]
IDS = [f"{s[0]}ch-L{s[1]}-h{s[2]}-nsub{s[3]}-m{s[4]}" for s in ALL]


@pytest.fixture(scope="module")
def wc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from openseize_amd import _lib
    _lib.load()      # fails loudly if the HIP library was not built
    from openseize_amd.features import coherence
    return coherence


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint64)


@lru_cache(maxsize=None)
def reference(shape):
    """(x, kwargs of the call, nwin, M, parts) of a shape; fs = nperseg, so bin k lies at k Hz.  Read-only."""
    nch, L, h, nsub, m, nwin, bands = shape
    overlap, W, step, n = geometry(shape)
    x = signal(nch, n, False, seed=nch)
    x.setflags(write=False)
    kw = dict(fs=float(L), winsize=W, step=step, bands=[(float(a), float(b)) for a, b in bands], nperseg=L,
              overlap=overlap)
    got, M, parts = window_coherence_measures(x, float(L), L, overlap, "hann", "constant", nsub, step, bands)
    assert got == nwin
    for m_ in M.values():
        m_.setflags(write=False)
    return x, kw, nwin, M, parts


def check(got, want, bound, unsafe, where, label, clean=None):
    """Every measure of ``got`` within its bound of ``want`` at ``where`` (pairs off the diagonal)."""
    for name in NAMES:
        err = np.abs(host(got[name]) - want[name])
        if name == "pli":
            safe = unsafe == 0
            worst = float(np.max(err[where & safe], initial=0.0))
            print(f"{label} pli: safe entries differ by {worst:.1e}; most allowed elsewhere {np.max(unsafe[where]):.2e}")
            assert worst <= SAME, name
            assert np.all(err[where] <= (unsafe + SAME)[where]), name
            continue
        limit = np.broadcast_to(bound[name], err.shape)
        print(f"{label} {name}: max err {np.max(err[where]):.2e}, bound {np.max(limit[where]):.2e}, "
              f"err / bound {np.max(err[where] / limit[where]):.2e}")
        assert np.all(err[where] <= limit[where]), name


@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_measures_are_the_restatement(wc, shape):
    nch, L, h, nsub, m, nwin, bands = shape
    x, kw, _, want, parts = reference(shape)
    count, got = wc.window_coherence(x, measures=NAMES, **kw)
    assert count == nwin and tuple(got) == NAMES
    bound, unsafe, share = bounds(parts, bands, nch)
    print(f"{shape[:6]}: {share:.2e} of the (pair, bin) entries sign-unsafe")
    assert share <= 1e-3
    diag = np.eye(nch, dtype=bool)
    where = np.broadcast_to(~diag, (nwin, len(bands), nch, nch))
    for name in NAMES:
        m_ = got[name]
        assert isinstance(m_, np.ndarray) and m_.dtype == np.float64 and m_.shape == (nwin, len(bands), nch, nch)
        assert np.array_equal(np.isnan(m_), np.isnan(want[name])), name
        assert np.all(m_[..., diag] == (1.0 if name in ("coh", "plv") else 0.0)), name
        if name == "imcoh":
            assert np.array_equal(m_.transpose(0, 1, 3, 2), -m_)
            assert not np.any(np.signbit(m_[m_ == 0.0]))
        else:
            assert np.array_equal(bits(m_.transpose(0, 1, 3, 2)), bits(m_)), name
    check(got, want, bound, unsafe, where, f"{shape[:6]}")


def test_bits_at_the_public_level(wc):
    shape = SHAPES[0]
    x, kw, nwin, _, _ = reference(shape)
    _, six = wc.window_coherence(x, measures=NAMES, **kw)
    _, again = wc.window_coherence(x, measures=NAMES[::-1], **kw)
    _, resident = wc.window_coherence(cuda(x), measures=NAMES, **kw)
    assert tuple(again) == NAMES[::-1]
    bands = kw["bands"]
    shuffled = [bands[2], (20.0, 25.0), bands[0]]
    _, other = wc.window_coherence(x, measures=NAMES, **dict(kw, bands=shuffled))
    import torch
    for name in NAMES:
        count, alone = wc.window_coherence(x, measures=name, **kw)
        assert count == nwin and isinstance(alone, np.ndarray)
        assert np.array_equal(bits(alone), bits(six[name])), name                 # one name = its entry of six
        assert np.array_equal(bits(again[name]), bits(six[name])), name           # two calls, the same bits
        assert torch.is_tensor(resident[name]) and resident[name].is_cuda
        assert np.array_equal(bits(resident[name]), bits(six[name])), name        # CUDA-fed = host-fed
        assert np.array_equal(bits(other[name][:, 0]), bits(six[name][:, 2])), name    # a band does not know the others
        assert np.array_equal(bits(other[name][:, 2]), bits(six[name][:, 0])), name
        _, single = wc.window_coherence(x, measures=name, **dict(kw, bands=bands[1]))
        assert single.shape == (nwin, shape[0], shape[0])
        assert np.array_equal(bits(single), bits(six[name][:, 1])), name
    # the step does not enter: the windows of step 2 h are every other window of step h
    _, dense = wc.window_coherence(x, measures=NAMES, **dict(kw, step=shape[2]))
    for name in NAMES:
        assert np.array_equal(bits(dense[name][::2][:nwin]), bits(six[name])), name
    # samples along axis 0
    _, turned = wc.window_coherence(np.ascontiguousarray(x.T), measures="wpli", axis=0, **kw)
    assert np.array_equal(bits(turned), bits(six["wpli"]))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], GAPS], ids=[IDS[0], IDS[4], IDS[6]])
def test_cuts_of_one_stream_agree(wc, shape, monkeypatch):
    """An array call against producers of odd chunk lengths, shorter than a segment, between a
    segment and a window, and longer than a window, with the caps so small that windows straddle
    pushes and launches: the same windows, within the bounds of the parity test scaled from the
    suite's RTOL = 1e-9 to spec.hip's cut guarantee of 1e-12 of the largest bin."""
    from openseize_amd import producer
    from openseize_amd.features import _stream
    nch, L, h, nsub, m, nwin, bands = shape
    x, kw, _, want, parts = reference(shape)
    _, whole = wc.window_coherence(x, measures=NAMES, **kw)
    bound, unsafe, _ = bounds(parts, bands, nch)
    cut = {name: b * (SAME / RTOL) + 1e-14 for name, b in bound.items()}        # (1e-14: the rounding of the measures)
    where = np.broadcast_to(~np.eye(nch, dtype=bool), (nwin, len(bands), nch, nch))
    monkeypatch.setattr(_stream, "_PUSH_BYTES", 2 * 8 * 6 * len(bands) * nch * nch)        # two windows a launch
    monkeypatch.setattr(wc, "_COHERENCE_PUSH_BYTES", 3 * 16 * nch * (L // 2 + 1))           # three segments a push
    W = kw["winsize"]
    for size in (L - 7, L + (W - L) // 2 + 1, W + 13):
        count, got = wc.window_coherence(producer(x, size, -1), measures=NAMES, **kw)
        assert count == nwin
        for name in NAMES:
            assert got[name].shape == whole[name].shape, (name, size)
            assert np.array_equal(np.isnan(got[name]), np.isnan(whole[name]))
        check(got, whole, cut, unsafe, where, f"{shape[:6]} chunks of {size}")
    count, got = wc.window_coherence(x, measures=NAMES, **kw)                    # the array itself, in small pushes
    assert count == nwin
    check(got, whole, cut, unsafe, where, f"{shape[:6]} small pushes")


# ---- the kernel alone, on fixed spectra: no transform is involved

def spectra(nseg, nch, nfreq, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nseg, nch, nfreq)) + 1j * rng.standard_normal((nseg, nch, nfreq))


def reduce(X, nsub, mstep, bands, mask=63):
    """_device.window_coherence of X (an ndarray) -> (planes, nwin, nbands, C, C) ndarray."""
    import torch
    from openseize_amd import _device as dev
    X = cuda(X)
    nwin = 0 if X.shape[0] < nsub else (X.shape[0] - nsub) // mstep + 1
    out = torch.full((bin(mask).count("1"), nwin, len(bands), X.shape[1], X.shape[1]), -7.0, dtype=torch.float64,
                     device="cuda")
    assert dev.window_coherence(X, nsub, mstep, bands, mask, out) == nwin
    return host(out)


def test_kernel_against_numpy(wc):
    """The six planes of random spectra against the sums written out in NumPy, at 1e-12."""
    nseg, nch, nfreq, nsub, mstep = 9, 5, 40, 4, 2
    bands = [(1, 4), (3, 40)]
    X = spectra(nseg, nch, nfreq, 0)
    got = reduce(X, nsub, mstep, bands)
    for k in range(3):
        Xw = X[k * mstep:k * mstep + nsub]
        z = np.conj(Xw)[:, :, None] * Xw[:, None]
        d = z.imag
        p = np.sum(np.abs(Xw) ** 2, axis=0)
        sa, sq = np.abs(d).sum(0), (d * d).sum(0)
        per_bin = [np.abs(z.sum(0)) ** 2 / (p[:, None] * p[None]), z.sum(0).imag / np.sqrt(p[:, None] * p[None]),
                   np.abs((z / np.abs(z)).sum(0)) / nsub, np.abs(np.sign(d).sum(0)) / nsub, np.abs(d.sum(0)) / sa,
                   (d.sum(0) ** 2 - sq) / (sa ** 2 - sq)]
        for p_, m in enumerate(per_bin):
            for b, (b0, b1) in enumerate(bands):
                want = m[..., b0:b1].mean(-1)
                want[np.eye(nch, dtype=bool)] = 1.0 if p_ in (0, 2) else 0.0
                assert np.max(np.abs(got[p_, k, b] - want)) < SAME, (k, NAMES[p_], b)


def test_kernel_bits(wc):
    nseg, nch, nfreq, nsub = 12, 11, 80, 3
    bands = [(1, 3), (5, 79), (7, 8)]
    X = spectra(nseg, nch, nfreq, 1)
    full = reduce(X, nsub, 1, bands)
    assert not np.any(full == -7.0)                                               # every entry is written
    # a channel subset, at the subset's entries
    keep = [1, 4, 9, 10]
    sub = reduce(X[:, keep], nsub, 1, bands)
    assert np.array_equal(bits(sub), bits(full[..., keep, :][..., keep]))
    # mstep 1 against 2, at the common windows
    assert np.array_equal(bits(reduce(X, nsub, 2, bands)), bits(full[:, ::2]))
    # one call against two calls on slices
    first, second = reduce(X[:7], nsub, 1, bands), reduce(X[5:], nsub, 1, bands)
    assert np.array_equal(bits(np.concatenate((first, second), axis=1)), bits(full))
    # a mask's planes do not know the other measures, nor a band the other bands
    for mask in (1, 2, 4, 8, 16, 32, 0b101001):
        planes = [p for p in range(6) if mask >> p & 1]
        assert np.array_equal(bits(reduce(X, nsub, 1, bands, mask)), bits(full[planes])), mask
    assert np.array_equal(bits(reduce(X, nsub, 1, bands[1:2])), bits(full[:, :, 1:2]))


def test_kernel_crosses_the_grid_limit(wc):
    """70 000 windows in one call equal the first and the last 100 computed alone: at nfreq = 5 with
    bands of 4, 2 and 1 bins (16, 32 and 64 windows a workgroup, the groups past a band's last window
    resting), and at nfreq = 40 with a band of 39 bins, one window a workgroup: 70 000 groups, more
    than the 65 535 of a grid's y, so the entry point's second batch."""
    nsub, nch = 2, 2
    for nfreq, cases in ((5, ([(1, 5)], [(1, 3), (4, 5)])), (40, ([(1, 40)],))):
        X = spectra(70001, nch, nfreq, 2)
        for bands in cases:
            full = reduce(X, nsub, 1, bands)
            assert full.shape[1] == 70000 and not np.any(full == -7.0)
            assert np.array_equal(bits(reduce(X[:101], nsub, 1, bands)), bits(full[:, :100]))
            assert np.array_equal(bits(reduce(X[-101:], nsub, 1, bands)), bits(full[:, -100:]))


def test_kernel_zero_and_nan_rows(wc):
    nseg, nch, nfreq, nsub = 6, 10, 70, 3
    bands = [(1, 3), (2, 69)]
    X = spectra(nseg, nch, nfreq, 3)
    clean = reduce(X, nsub, 1, bands)
    others = [c for c in range(nch) if c != 4]
    for value, lost in ((0.0, (0, 1, 2)), (np.nan, range(6))):
        Y = X.copy()
        Y[:, 4] = value
        got = reduce(Y, nsub, 1, bands)
        for p in lost:
            assert np.all(np.isnan(got[p][..., 4, :])) and np.all(np.isnan(got[p][..., :, 4])), (value, NAMES[p])
        assert np.array_equal(bits(got[..., others, :][..., others]), bits(clean[..., others, :][..., others]))
    # one segment, one bin: the windows that hold the segment and the bands that hold the bin, no other
    Y = X.copy()
    Y[3, 4, 2] = np.nan
    got = reduce(Y, nsub, 1, bands)
    hit = np.zeros(got.shape, bool)
    hit[:, 1:4, :, 4, :] = hit[:, 1:4, :, :, 4] = True                            # (windows 1 .. 3 hold segment 3)
    assert np.array_equal(np.isnan(got), hit)
    assert np.array_equal(bits(got[~hit]), bits(clean[~hit]))


# ---- non-finite samples and a coupling that comes and goes

def test_a_nonfinite_sample_stays_in_its_windows_row_and_column(wc):
    shape = SHAPES[0]
    nch, L, h, nsub, m, nwin, bands = shape
    x, kw, _, _, parts = reference(shape)
    _, clean = wc.window_coherence(x, measures=NAMES, **kw)
    y = x.copy()
    at = 5 * h + 3                                                                # in the segments 4 and 5
    y[2, at] = np.nan
    held = [k for k in range(nwin) if k * m <= 5 and k * m + nsub - 1 >= 4]
    assert 0 < len(held) < nwin
    hit = np.zeros((nwin, len(bands), nch, nch), bool)
    hit[held, :, 2, :] = hit[held, :, :, 2] = True
    bound, unsafe, _ = bounds(parts, bands, nch)
    where = ~hit & ~np.eye(nch, dtype=bool)
    for data in (y, cuda(y)):
        _, got = wc.window_coherence(data, measures=NAMES, **kw)
        for name in NAMES:
            assert np.array_equal(np.isnan(host(got[name])), hit), name
        check(got, clean, bound, unsafe, where, "beside a NaN")
        for measures in ("pli", NAMES):
            with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
                wc.window_coherence(data, measures=measures, **dict(kw, detrend="linear"))


def test_a_coupling_that_switches_off(wc):
    """Two channels share an 8 - 13 Hz rhythm at a 90 degree lag, plus noise, in the first half of the
    stream and not in the second (``test_coherence_host.coupled``); the windows' values follow."""
    from test_coherence_host import coupled
    x, fs, L, W = coupled()
    nwin = 8
    count, got = wc.window_coherence(x, fs, W, measures=("imcoh", "wpli", "coh"), bands=[(8, 13), (20, 40)], nperseg=L)
    assert count == nwin
    print({name: np.round(m[:, :, 0, 1], 2).tolist() for name, m in got.items()})
    for name in ("imcoh", "wpli", "coh"):
        assert np.all(np.abs(got[name][:nwin // 2, 0, 0, 1]) > 0.5), name         # the band that holds 10 Hz
        assert np.all(np.abs(got[name][nwin // 2:, 0, 0, 1]) < 0.5), name         # the coupling is off
    assert np.all(got["wpli"][:, 1, 0, 1] < 0.5)                                  # a band without it
    assert np.all(got["wpli"][:, 0, 0, 2] < 0.5)                                  # a channel without it
