"""Generate tests/golden/g24_pair_bits.npz by RUNNING the channel-pair kernels on the GPU.

Run on a build of the commit BEFORE the kernels moved onto csrc/pair_tile.h, from the
repository root (the output directory is optional, tests/golden by default):

    python tests/golden/make_golden_pair_bits.py [outdir]

Only digests are written, ``sha256[k]`` under the name ``keys[k]``: per case ``in:<case>``, the
SHA-256 of the inputs' bytes (a changed random stream shows up as such, not as a kernel
failure), and per result ``out:<case>:<name>``, the SHA-256 of the result's bytes with every NaN
replaced by one canonical NaN first.
tests/test_gpu_pair_bits.py loads this file as a module, reruns ``CASES`` and compares.

The cases are the smallest shapes that reach every branch of the pair-tile skeleton; results come
from the openseize_amd._device wrappers directly.
  spec-<nch>ch-<pushes>   spectra (nseg, nch, 101) complex128: 101 bins are one full and one
        partial block of 64 lanes; 5 channels are a partial 4 x 4 tile inside one block, 17 are
        2 blocks of 16 (K10) and 3 of 8 (K11, K12): diagonal blocks with resting waves,
        off-diagonal blocks, a last block of one channel, more than one row of the triangle;
        pushes 1 (no prefetch), 7 (both stage buffers), 3+4 (accumulation from stored sums).
        Every accumulator starts as 0 on and above the diagonal and -7.0 below it, and is
        digested whole: the lower triangle is shown untouched.  cross_accumulate, cross_finish
        in both modes, lag_accumulate, unit_phasors + cross_accumulate, phase_finish for the
        five methods; with 7 segments jackknife_accumulate / jackknife_finish for the six
        methods at count 7, and dwpli once more on the first two segments at count 2.
  spec-5ch-nan, spec-5ch-zero   7 segments with a NaN in one channel of one segment, and with
        an exactly zero spectrum value (plv's 0 / 0).
  time-<nch>ch-<n>   analytic_accumulate with all four sum groups and analytic_finish for the
        five methods on (nch, n) complex128: n = 70 is one short time block whose second
        64-sample step is partial, n = 4096 + 70 two time blocks; time-5ch-70-zero has a zero
        sample.
  window-real, window-complex   window_pairs on 70 rows (two 64-row blocks; the 140 phasor rows
        of plv / ciplv three), n = 900, winsize 300, step 150, every measure of the data type.
"""

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NFREQ, NFFT = 101, 200
PHASE = ("imcoh", "plv", "pli", "wpli", "dwpli")
JACK = ("coherence", "imcoh", "plv", "pli", "wpli", "dwpli")
ANALYTIC = ("aec", "oaec", "plv", "ciplv", "wpli")


def digest(a):
    """SHA-256 of the bytes of a float64 / complex128 array, every NaN made the canonical one."""
    v = np.ascontiguousarray(a).view(np.float64).copy()
    v[np.isnan(v)] = np.nan
    return np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def complex_normal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def sums_tensor(planes, nch, tail, dtype):
    """Accumulator (planes..., nch, nch, tail...): 0 for i <= j, -7.0 below the diagonal."""
    a = np.zeros(planes + (nch, nch) + tail, dtype)
    lower = np.tril(np.ones((nch, nch), bool), -1)
    a[(slice(None),) * len(planes) + (lower,)] = -7.0
    return cuda(a)


def spectra_case(seed, nch, pushes, spoil=None):
    def run():
        from openseize_amd import _device as dev
        from openseize_amd import _lib
        nseg = sum(pushes)
        X = complex_normal(np.random.default_rng(seed), (nseg, nch, NFREQ))
        if spoil is not None:
            X[3, 2, 10] = spoil
        cuts = np.cumsum((0,) + pushes)
        Xd = cuda(X)
        U = dev.unit_phasors(Xd.clone())
        out = {}

        def totals(Xd, U, pushes_of):
            acc, accn = (sums_tensor((), nch, (NFREQ,), np.complex128) for _ in range(2))
            lag = sums_tensor((4,), nch, (NFREQ,), np.float64)
            for a, b in pushes_of:
                dev.cross_accumulate(Xd[a:b], acc)
                dev.lag_accumulate(Xd[a:b], lag)
                dev.cross_accumulate(U[a:b], accn)
            return acc, accn, lag

        spans = list(zip(cuts[:-1], cuts[1:]))
        acc, accn, lag = totals(Xd, U, spans)
        out.update(acc=acc, accn=accn, lag=lag, unit=U)
        out["coherence"] = dev.cross_finish(acc, nseg, NFFT, _lib.CROSS_COHERENCE)
        out["spectrum"] = dev.cross_finish(acc.clone(), nseg, NFFT, _lib.CROSS_SPECTRUM)
        for m in PHASE:
            out[f"phase-{m}"] = dev.phase_finish(m, nseg, NFFT, acc=acc, accn=accn, lag=lag)

        def jackknife(m, Xd, U, spans, count, acc, accn, lag, tag):
            dev2 = sums_tensor((2,), nch, (NFREQ,), np.float64)
            for a, b in spans:
                dev.jackknife_accumulate(m, (U if m == "plv" else Xd)[a:b], count, dev2, acc=acc, accn=accn, lag=lag)
            out[f"dev2-{tag}"] = dev2
            out[f"jack-{tag}"] = dev.jackknife_finish(m, dev2, count, NFFT, acc=acc, accn=accn, lag=lag)

        if nseg >= 2:
            for m in JACK:
                jackknife(m, Xd, U, spans, nseg, acc, accn, lag, m)
            two = totals(Xd[:2], U[:2], [(0, 2)])
            jackknife("dwpli", Xd, U, [(0, 2)], 2, *two, "dwpli-count2")
        return [X], {k: v.cpu().numpy() for k, v in out.items()}
    return run


def time_case(seed, nch, n, zero=False):
    def run():
        from openseize_amd import _device as dev
        groups = 15
        z = complex_normal(np.random.default_rng(seed), (nch, n))
        if zero:
            z[2, 13] = 0.0
        sums = sums_tensor((dev.analytic_planes(groups),), nch, (), np.float64)
        chan = cuda(np.zeros((3, nch)))
        dev.analytic_accumulate(cuda(z), groups, sums, chan)
        out = {"sums": sums, "chan": chan}
        for m in ANALYTIC:
            out[m] = dev.analytic_finish(m, n, groups, sums, chan)
        return [z], {k: v.cpu().numpy() for k, v in out.items()}
    return run


def window_case(seed, cplx):
    def run():
        import torch
        from openseize_amd import _device as dev
        from openseize_amd import _lib
        nch, n, winsize, step = 70, 900, 300, 150
        rng = np.random.default_rng(seed)
        x = complex_normal(rng, (nch, n)) if cplx else rng.standard_normal((nch, n))
        wc = _lib.WINDOW_CONNECTIVITY
        names = [k for k in wc if (k not in _lib.WC_REAL) == cplx]
        mask = sum(1 << wc[k] for k in names)
        nwin = (n - winsize) // step + 1
        out = torch.full((len(names), nwin, nch, nch), -7.0, dtype=torch.float64, device="cuda")
        assert dev.window_pairs(cuda(x), winsize, step, 1, mask, out) == nwin
        return [x], {"out": out.cpu().numpy()}
    return run


CASES = {}
for _nch in (5, 17):
    for _tag, _pushes in (("1", (1,)), ("7", (7,)), ("3+4", (3, 4))):
        CASES[f"spec-{_nch}ch-{_tag}"] = spectra_case(2400 + _nch, _nch, _pushes)
CASES["spec-5ch-nan"] = spectra_case(2431, 5, (7,), spoil=np.nan)
CASES["spec-5ch-zero"] = spectra_case(2432, 5, (7,), spoil=0.0)
for _nch in (5, 17):
    for _n in (70, 4096 + 70):
        CASES[f"time-{_nch}ch-{_n}"] = time_case(2440 + _nch, _nch, _n)
CASES["time-5ch-70-zero"] = time_case(2450, 5, 70, zero=True)
CASES["window-real"] = window_case(2460, False)
CASES["window-complex"] = window_case(2461, True)


def digests(case):
    """{key: digest} of one case, keyed as the fixture is."""
    inputs, results = CASES[case]()
    found = {f"in:{case}": digest(np.concatenate([np.ravel(a).view(np.float64) for a in inputs]))}
    found.update({f"out:{case}:{k}": digest(v) for k, v in results.items()})
    return found


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else HERE
    out = {}
    for case in CASES:
        out.update(digests(case))
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "g24_pair_bits.npz")
    np.savez_compressed(path, keys=np.array(list(out)), sha256=np.stack(list(out.values())))
    print(f"g24_pair_bits.npz: {os.path.getsize(path) / 1e3:.0f} kB, {len(out)} digests of {len(CASES)} cases")


if __name__ == "__main__":
    main()
