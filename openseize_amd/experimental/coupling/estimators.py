"""Estimators of cross-frequency coupling: ``PhaseLock``, phase-to-power locking
between two bands of a 1-D signal, with the interface of the reference's
``experimental/coupling/estimators.py:26-420`` (``plot`` excepted), and
``ModulationIndex``, the phase-amplitude comodulogram (no counterpart in the reference).

The two hot loops are device kernels of ``csrc/coupling.hip``:
``osz_phase_index`` selects the samples whose analytic phase lies in a band
(``index``), and ``osz_lock_accumulate`` sums the power amp^2 over a window
around every selected sample and around every shifted (surrogate) copy of the
selection, all sets of one chunk in one launch (``estimate``).  The surrogate
shifts are drawn on the host from ``rng`` in the reference's order, so results
match it draw for draw; see ``estimate`` for the two ``ncores`` modes.

``ModulationIndex`` runs on ``csrc/pac.hip``: ``osz_phase_bins`` cuts the phase of every
phase band into bins, ``osz_pac_accumulate`` sums every amplitude band per phase bin for
the real pairing and every time-shifted surrogate of a chunk in one launch, and
``osz_pac_finish`` turns the sums into the modulation indices.
"""

import copy
import numbers
import time

import numpy as np
from scipy import stats
from scipy.stats import false_discovery_control as fdr

from openseize_amd import _device as dev
from openseize_amd import _lib
from openseize_amd.core import protools, resources
from openseize_amd.core.producer import producer
from openseize_amd.experimental.coupling.transforms import Analytic, _complex_rows
from openseize_amd.filtering import fir


class PhaseLock:
    """Phase-to-power locking estimator (Canolty et al. 2006) over chunks of a
    1-D signal: the phase comes from a band-limited Hilbert FIR (``hilbert``),
    windows that do not fit inside a chunk are dropped, as in the reference.

    Attributes:
        rng: numpy Generator of the surrogate shifts (``seed``).
        indices: the phase indices of ``index``, a list of int64 arrays, one per
            chunk (ndarrays for host input, CUDA tensors for CUDA input); None
            until ``index`` runs or after ``hilbert`` / ``chunksize`` / ``fs`` is
            set.  Assigned arrays must hold ascending positions within their
            chunk.
    """

    def __init__(self, hilbert, chunksize=int(10e6), seed=0):
        self._hilbert = hilbert
        self._chunksize = chunksize
        self.rng = np.random.default_rng(seed)
        self.indices = None

    @property
    def indices(self):
        return self._indices

    @indices.setter
    def indices(self, value):
        self._indices = value
        self._resident = None          # (sources, device copies) of what was uploaded

    @property
    def hilbert(self):
        return self._hilbert

    @hilbert.setter
    def hilbert(self, value):
        self._hilbert = value
        self.indices = None

    @property
    def fs(self):
        return self.hilbert.fs

    @fs.setter
    def fs(self, value):
        # the reference stores the value where nothing reads it (estimators.py:96-101)
        self._fs = value
        self.indices = None

    @property
    def chunksize(self):
        return self._chunksize

    @chunksize.setter
    def chunksize(self, value):
        self._chunksize = value
        self.indices = None

    def _analytic(self, x, axis):
        return Analytic(x, self.fs, self.chunksize, axis, width=self.hilbert.width,
                        gpass=self.hilbert.gpass, gstop=self.hilbert.gstop)

    def index(self, signal, fpass, fstop, firfilt=fir.Kaiser, phase=0, epsi=0.05, axis=-1,
              **kwargs):
        """Stores in ``indices`` the positions, per chunk, of the samples of the
        ``firfilt(fpass, fstop, fs, **kwargs)``-filtered signal whose analytic
        phase in [0, 2 pi) lies strictly between ``phase - epsi`` and
        ``phase + epsi`` (same units as the phases: radians)."""
        pro = producer(signal, chunksize=self.chunksize, axis=axis)
        if pro.ndim > 1:
            raise ValueError("Signal to estimate phase indices must be 1D")
        filt = firfilt(fpass, fstop, self.fs, **kwargs)
        analytic = self._analytic(filt(pro, chunksize=self.chunksize, axis=axis), axis)
        lo, hi = phase - epsi, phase + epsi
        indices, resident = [], []
        for arr in analytic.signal:
            z2d, host = _complex_rows(arr, dev.Layout(arr.shape, axis))
            idx = dev.phase_index(z2d[0], lo, hi)
            resident.append(idx)
            indices.append(idx.cpu().numpy() if host else idx)
        self.indices = indices
        self._resident = (list(indices), resident)

    def _device_indices(self):
        """Device copies of ``indices``; arrays assigned by the caller are uploaded
        here, once."""
        if self.indices is None:
            raise ValueError("no phase indices: call index() or assign indices first")
        if self._resident is not None:
            sources, resident = self._resident
            if len(sources) == len(self.indices) and all(
                    a is b for a, b in zip(sources, self.indices)):
                return resident
        import torch
        resident = []
        for arr in self.indices:
            if dev.is_tensor(arr):
                t = arr if arr.is_cuda else arr.cuda()
                t = t if t.dtype == torch.int64 else t.to(torch.int64)
            else:
                a = np.asarray(arr).astype(np.int64, copy=False).ravel()
                if a.size > 1 and np.any(np.diff(a) < 0):
                    raise ValueError("phase indices must be ascending within each chunk")
                t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            resident.append(t.reshape(-1).contiguous())
        self._resident = (list(self.indices), resident)
        return resident

    def shuffle(self, n_samples):
        """One random shift of every chunk's indices, modulo the smaller of
        ``n_samples`` and ``chunksize`` (host arrays)."""
        max_shift = min(self.chunksize, n_samples)
        shift = self.rng.integers(0, max_shift)
        return [np.mod(np.asarray(arr.cpu() if dev.is_tensor(arr) else arr) + shift, max_shift)
                for arr in self.indices]

    def _estimate(self, pro, center, bandwidth, winsize, shifts, max_shift, axis, **kwargs):
        """(power, unadjusted p-values or None) at one centre frequency."""
        import torch
        fpass = center + np.array([-bandwidth / 2, bandwidth / 2])
        fstop = fpass + np.array([-bandwidth / 2, bandwidth / 2])
        filt = fir.Kaiser(fpass, fstop, self.fs, **kwargs)
        z = protools.standardize(filt(pro, chunksize=self.chunksize, axis=axis), axis=axis)
        analytic = self._analytic(z, axis)
        nsets = len(shifts) + 1
        sums = dev.zeros((nsets, winsize), torch.float64)
        counts = dev.zeros((nsets,), torch.int64)
        dshifts = torch.from_numpy(np.asarray(shifts, dtype=np.int64)).cuda()
        for arr, idx in zip(analytic.signal, self._device_indices()):
            z2d, _ = _complex_rows(arr, dev.Layout(arr.shape, axis))
            amp, _ = dev.magphase(z2d, want_phase=False)
            dev.lock_accumulate(amp[0], idx, dshifts, max_shift, winsize, sums, counts)
        cnt = counts.cpu().numpy()
        empty = np.flatnonzero(cnt == 0)
        if empty.size:
            which = "the phase indices" if empty[0] == 0 else f"surrogate {empty[0]}"
            raise ValueError(f"no window of {winsize} samples fits around any index of "
                             f"{which} (index set {empty[0]}) at {center} Hz")
        dcnt = torch.from_numpy(cnt.astype(np.float64)).cuda()
        avg = dev.ew(_lib.EW_DIV, sums, dcnt, kind=_lib.BCAST_ROW)
        power = avg[0].cpu().numpy()
        if nsets == 1:
            return power, None
        mean, sd = (v.cpu().numpy() for v in dev.col_moments(avg[1:], ignore_nan=False))
        zscore = (power - mean) / (sd / np.sqrt(nsets - 1))
        return power, 1 - stats.norm.cdf(zscore)

    def printer(self, msg, verbose, end="\n", flush=True):
        if verbose:
            print(msg, end=end, flush=flush)

    def estimate(self, signal, centers, bandwidth=4, window=2, surrogates=300, in_memory=True,
                 ncores=None, verbose=True, axis=-1, **kwargs):
        """(powers, pvalues), each of shape (len(centers), window * fs): the mean
        power in a window around the phase indices at every centre frequency,
        and its false-discovery-rate adjusted p-value against ``surrogates``
        shifted copies of the indices (an object array of Nones when
        ``surrogates`` is falsy).

        The shifts follow the reference's ``ncores`` outcome: with one core they
        are drawn in sequence across centres and ``rng`` advances; with more,
        every centre gets the same shifts, drawn from ``rng``'s state at the
        call, and ``rng`` is left as it was (the reference's worker processes
        each draw from their own copy).  No process pool is used.
        ``in_memory`` is accepted and changes nothing.
        """
        pro = producer(signal, chunksize=self.chunksize, axis=axis)
        if pro.ndim > 1:
            raise ValueError("Signal must be 1-D array or Producer of 1-D arrays.")
        winsize = window * self.fs
        if isinstance(winsize, numbers.Integral):
            winsize = int(winsize)
        elif isinstance(winsize, numbers.Real) and float(winsize).is_integer():
            winsize = int(winsize)
        else:
            raise TypeError(f"window * fs = {winsize!r} must be a whole number of samples")
        if winsize < 1:
            raise ValueError(f"window * fs = {winsize} must be at least one sample")
        self._device_indices()
        cores = resources.allocate(len(centers), ncores)
        max_shift = min(self.chunksize, pro.shape[axis])
        nsur = int(surrogates) if surrogates else 0
        if cores > 1:
            rng = copy.deepcopy(self.rng)
            common = [rng.integers(0, max_shift) for _ in range(nsur)]
            self.printer(f"Initializing {type(self).__name__} with {cores} cores", verbose)

        t0 = time.perf_counter()
        result = {}
        for i, center in enumerate(centers, 1):
            if cores > 1:
                shifts = common
            else:
                shifts = [self.rng.integers(0, max_shift) for _ in range(nsur)]
            power, pvals = self._estimate(pro, center, bandwidth, winsize, shifts, max_shift,
                                          axis, **kwargs)
            result[center] = [power, fdr(pvals) if surrogates else None]
            self.printer(f"Frequency {i} / {len(centers)} completed", verbose, end="\r")
        delta = time.perf_counter() - t0
        self.printer(f"{type(self).__name__} estimate completed in {delta} secs", verbose)

        powers = np.stack([result[c][0] for c in centers])
        pvalues = np.stack([result[c][1] for c in centers])
        return powers, pvalues


class ModulationIndex:
    """Phase-amplitude comodulogram of a 1-D signal: the modulation index of Tort et al.
    (2010) -- the Kullback-Leibler distance from uniform of the mean amplitude per phase
    bin, over ln(nbins) -- for every pair of a phase band and an amplitude band, with
    time-shift surrogates for significance.  Phases and amplitudes come from Kaiser band
    filters followed by the band-limited Hilbert FIR ``hilbert``, chunk by chunk.

    Attributes:
        rng: numpy Generator of the surrogate shifts (``seed``).
        nbins: number of phase bins of [0, 2 pi), 2 to 64.
    """

    def __init__(self, hilbert, chunksize=int(10e6), nbins=18, seed=0):
        self.hilbert = hilbert
        self.chunksize = chunksize
        self.nbins = nbins
        self.rng = np.random.default_rng(seed)

    @property
    def fs(self):
        return self.hilbert.fs

    @fs.setter
    def fs(self, value):
        # as PhaseLock: the rate follows the Hilbert filter, the value is only kept
        self._fs = value

    def _bands(self, centers, bandwidth, what):
        """[(centre, Kaiser filter arguments)] of one axis of the grid, validated."""
        centers = list(np.atleast_1d(centers))
        if not centers:
            raise ValueError(f"no {what} centres given")
        widths = np.atleast_1d(bandwidth)
        if widths.size == 1:
            widths = np.repeat(widths, len(centers))
        if widths.ndim != 1 or widths.size != len(centers):
            raise ValueError(f"{what}_bandwidth holds {widths.size} values for {len(centers)} centres")
        bands = []
        for c, bw in zip(centers, widths):
            if not bw > 0:
                raise ValueError(f"{what} bandwidth {bw} at {c} Hz must be positive")
            fpass = c + np.array([-bw / 2, bw / 2])
            fstop = fpass + np.array([-bw / 2, bw / 2])
            if not (fstop[0] > 0 and fstop[1] < self.fs / 2):
                raise ValueError(f"{what} band at {c} Hz: the stop edges {fstop[0]:g} and {fstop[1]:g} Hz "
                                 f"must lie inside (0, {self.fs / 2:g}) Hz")
            bands.append((c, fpass, fstop))
        return bands

    def _analytic(self, pro, band, axis, kwargs):
        _, fpass, fstop = band
        filt = fir.Kaiser(fpass, fstop, self.fs, **kwargs)
        return Analytic(filt(pro, chunksize=self.chunksize, axis=axis), self.fs, self.chunksize,
                        axis, width=self.hilbert.width, gpass=self.hilbert.gpass,
                        gstop=self.hilbert.gstop).signal

    def printer(self, msg, verbose, end="\n", flush=True):
        if verbose:
            print(msg, end=end, flush=flush)

    def estimate(self, signal, phase_centers, amp_centers, phase_bandwidth=2, amp_bandwidth=20,
                 surrogates=200, min_shift=None, amplitude_signal=None, verbose=True, axis=-1,
                 **kwargs):
        """(mi, pvalues, dist) of shapes (P, A), (P, A) and (P, A, nbins), ndarrays for host
        and CUDA input alike: the modulation index of the amplitude around
        ``amp_centers[a]`` by the phase around ``phase_centers[p]``, its false-discovery-rate
        adjusted p-value over all P A cells, and the amplitude distribution over the phase
        bins.  The amplitudes are taken from ``amplitude_signal`` when given (a second 1-D
        source of the same length: cross-site coupling), else from ``signal``.

        A band of centre c and bandwidth bw (a scalar or one value per centre) is the filter
        ``fir.Kaiser(c -+ bw/2, c -+ bw, fs, **kwargs)``; its analytic signal comes from the
        Hilbert filter's ``width`` / ``gpass`` / ``gstop``.  Nothing is standardised: the
        index does not depend on the scale.

        Surrogates: ``surrogates`` shifts are drawn once per call, each as
        ``rng.integers(min_shift, max_shift - min_shift)`` with ``max_shift = min(chunksize,
        n)`` and ``min_shift = int(fs)`` unless given, and shared by all band pairs; within
        every chunk the amplitudes are rotated by the shift against the phases.  A last chunk
        shorter than a shift is rotated by the shift modulo its length.  The p-value of a
        cell is the upper normal tail of (mi - mean) / std (ddof 1) over its surrogates, 1.0
        where they do not vary.  With falsy ``surrogates`` nothing is drawn and ``pvalues`` is
        an object array of Nones.
        """
        import torch
        pro = producer(signal, chunksize=self.chunksize, axis=axis)
        if pro.ndim > 1:
            raise ValueError("Signal must be 1-D array or Producer of 1-D arrays.")
        amp_pro = pro
        if amplitude_signal is not None:
            amp_pro = producer(amplitude_signal, chunksize=self.chunksize, axis=axis)
            if amp_pro.ndim > 1:
                raise ValueError("amplitude_signal must be 1-D array or Producer of 1-D arrays.")
            if tuple(amp_pro.shape) != tuple(pro.shape):
                raise ValueError(f"amplitude_signal holds {amp_pro.shape[0]} samples, signal "
                                 f"{pro.shape[0]}")
        nbins = self.nbins
        if not (isinstance(nbins, numbers.Integral) and 2 <= nbins <= 64):
            raise ValueError(f"nbins = {nbins!r} is not a whole number from 2 to 64")
        nbins = int(nbins)
        pbands = self._bands(phase_centers, phase_bandwidth, "phase")
        abands = self._bands(amp_centers, amp_bandwidth, "amp")
        n = pro.shape[0]
        nsur = int(surrogates) if surrogates else 0
        if nsur < 0:
            raise ValueError(f"surrogates = {surrogates!r} is negative")
        if nsur:
            max_shift = min(self.chunksize, n)
            lo = int(self.fs) if min_shift is None else int(min_shift)
            if lo < 0 or lo >= max_shift - lo:
                raise ValueError(f"no shift lies in [{lo}, {max_shift - lo}): min_shift must be "
                                 f"below half of min(chunksize, samples) = {max_shift}")
        # (the filters are designed here, still before any source is pulled)
        streams = ([self._analytic(pro, b, axis, kwargs) for b in pbands]
                   + [self._analytic(amp_pro, b, axis, kwargs) for b in abands])
        shifts = [self.rng.integers(lo, max_shift - lo) for _ in range(nsur)]

        t0 = time.perf_counter()
        P, A = len(pbands), len(abands)
        sums = dev.zeros((P, A, nsur + 1, nbins), torch.float64)
        counts = dev.zeros((P, nbins), torch.int64)
        dshifts = torch.from_numpy(np.asarray(shifts, dtype=np.int64)).cuda()
        for k, chunks in enumerate(zip(*streams), 1):
            rows = [_complex_rows(arr, dev.Layout(arr.shape, axis))[0] for arr in chunks]
            L = rows[0].shape[1]
            bins = torch.empty((P, L), dtype=torch.uint8, device="cuda")
            amp = torch.empty((A, L), dtype=torch.float64, device="cuda")
            for p in range(P):
                dev.phase_bins(rows[p], nbins, out=bins[p:p + 1])
            for a in range(A):
                dev.magphase(rows[P + a], want_phase=False, mag_out=amp[a:a + 1])
            dev.pac_accumulate(bins, amp, dshifts, nbins, sums, counts)
            self.printer(f"Chunk {k} completed", verbose, end="\r")
        empty = np.flatnonzero((counts.cpu().numpy() == 0).any(axis=1))
        if empty.size:
            raise ValueError(f"a phase bin of the {nbins} stayed empty in the phase band at "
                             f"{pbands[empty[0]][0]} Hz: the signal is too short for nbins, or flat")
        dmi, ddist = dev.pac_finish(sums, counts)
        allmi, dist = dmi.cpu().numpy(), ddist.cpu().numpy()
        mi = np.ascontiguousarray(allmi[..., 0])
        if nsur:
            sur = allmi[..., 1:]
            mean = sur.mean(axis=-1)
            sd = sur.std(axis=-1, ddof=1) if nsur > 1 else np.zeros_like(mean)
            pvalues = np.ones_like(mi)
            ok = sd > 0
            pvalues[ok] = stats.norm.sf((mi[ok] - mean[ok]) / sd[ok])
            pvalues = fdr(pvalues.ravel()).reshape(mi.shape)
        else:
            pvalues = np.full(mi.shape, None, dtype=object)
        delta = time.perf_counter() - t0
        self.printer(f"{type(self).__name__} estimate completed in {delta} secs", verbose)
        return mi, pvalues, dist
