"""Generate tests/golden/g26_pairwin_bits.npz by RUNNING the channel-pair window kernels on the GPU.

Run on a build of the commit BEFORE windowpair.hip (K19), windowxcorr.hip (K23) and
windowgranger.hip (K24) moved onto csrc/pair_window.h, from the repository root (the output
directory is optional, tests/golden by default):

    python tests/golden/make_golden_pairwin_bits.py [outdir]

Only digests are written, ``sha256[k]`` under the name ``keys[k]``: per case ``in:<case>``, the
SHA-256 of the inputs' bytes (a changed random stream shows up as such, not as a kernel failure),
and per result ``out:<case>:<name>``, the SHA-256 of the result's bytes with every NaN replaced by
one canonical NaN first.  tests/test_gpu_pairwin_bits.py loads this file as a module, reruns
``CASES`` and compares.

Results come from the openseize_amd._device wrappers directly, into tensors that start as -7.0.
  xcorr-<W>-L<L>-<norm|raw>-<mask>   window_xcorr on 37 rows (two 32-row blocks, the second ragged;
        finishing tiles of 16, the third ragged), step 1, 5 windows.  Channel 5 is constant, channel
        11 has a NaN that window 0 alone holds and channel 20 +inf that the last window alone holds.
        W = 128 with L = 64 (129 lags: nine groups of 16, the last ragged, and the whole halo), L = 0
        and L = 5 (a partial first group), all four measures, normalised and not; L = 64 also with
        xcorr alone (mask 1) and lag alone (mask 4).  W = 9, L = 4: a window shorter than one
        64-sample step.
  xcorr-batches   70 rows, L = 64, W = 128, step 1, n = 187: 60 windows.  One window's G is 129 x
        70 x 70 = 632100 doubles, a batch holds at most 2^25 doubles (kGramCap) of G, which is 53
        windows: two batches, the second of 7.  The case asserts that from osz_window_xcorr_work's
        answer.  peak, lag and signed.
  granger-<W>-p<order>-<mask>   window_granger on 19 rows (tiles of 8, the third ragged), step 3, 5
        windows, orders 1, 4 (granger_pair_kernel<4>), 5, 8 (<8>), 9 and 16 (<16>) at W = 128 and order
        1 at W = 16, all three measures; order 5 also with each measure alone.  Channel 5 is
        constant, channel 11 has a NaN in window 0 alone and channel 7 is an exact copy of channel
        3: the values of the pair (3, 7) are unspecified, so its two entries are set to 0 before
        the digest.
  pairs-real-ddof<d>, pairs-complex   window_pairs on 70 rows with W = 1030, step 515, n = 2060: 3
        windows of two sub-blocks (OSZ_WC_BLOCK = 1024), the second of 6 samples.  Real: cov and
        corr with ddof 0 and 1.  Complex: aec, plv and ciplv, one sample of channel 9 is 0.
"""

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

GRAM_CAP = 1 << 25          # kGramCap of csrc/pair_window.h


def digest(a):
    """SHA-256 of the bytes of a float64 array, every NaN made the canonical one."""
    v = np.ascontiguousarray(a).view(np.float64).copy()
    v[np.isnan(v)] = np.nan
    return np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blank(*shape):
    import torch
    return torch.full(shape, -7.0, dtype=torch.float64, device="cuda")


def stream(seed, nch, W, step, nwin=5):
    """(nch, n) noise that holds ``nwin`` windows: channel 5 constant, a NaN in channel 11 that
    window 0 alone holds, +inf in channel 20 (if there is one) that the last window alone holds."""
    n = W + (nwin - 1) * step
    x = np.random.default_rng(seed).standard_normal((nch, n))
    x[5] = 2.5
    x[11, 0] = np.nan
    if nch > 20:
        x[20, n - 1] = np.inf
    return x


def xcorr_case(seed, nch, W, L, normalize, mask, n=None):
    def run():
        from openseize_amd import _device as dev
        x = stream(seed, nch, W, 1) if n is None else np.random.default_rng(seed).standard_normal((nch, n))
        nwin = x.shape[1] - W + 1
        planes = bin(mask >> 1).count("1")
        xc = blank(nwin, 2 * L + 1, nch, nch) if mask & 1 else None
        out = blank(planes, nwin, nch, nch) if planes else None
        if n is not None:                       # the case of two batches: see the module's docstring
            lib = dev.require_gpu()
            one = (2 * L + 1) * nch * nch
            batch = (lib.osz_window_xcorr_work(nch, x.shape[1], W, 1, L, mask) - nch * nwin) // one
            assert batch == GRAM_CAP // one and batch < nwin <= 2 * batch, (batch, nwin)
        assert dev.window_xcorr(cuda(x), W, 1, L, normalize, mask, xc, out) == nwin
        found = {}
        if xc is not None:
            found["xcorr"] = xc.cpu().numpy()
        if out is not None:
            found["out"] = out.cpu().numpy()
        return [x], found
    return run


def granger_case(seed, W, order, mask):
    def run():
        from openseize_amd import _device as dev
        nch, step, nwin = 19, 3, 5
        x = stream(seed, nch, W, step, nwin)
        x[7] = x[3]
        out = blank(bin(mask).count("1"), nwin, nch, nch)
        assert dev.window_granger(cuda(x), W, step, order, mask, out) == nwin
        got = out.cpu().numpy()
        got[:, :, 3, 7] = got[:, :, 7, 3] = 0.0
        return [x], {"out": got}
    return run


def pairs_case(seed, cplx, ddof):
    def run():
        from openseize_amd import _device as dev
        from openseize_amd import _lib
        nch, n, W, step = 70, 2060, 1030, 515
        assert _lib.WC_BLOCK < W < 2 * _lib.WC_BLOCK
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((nch, n))
        if cplx:
            x = x + 1j * rng.standard_normal((nch, n))
            x[9, 600] = 0.0
        wc = _lib.WINDOW_CONNECTIVITY
        names = [k for k in wc if (k not in _lib.WC_REAL) == cplx]
        mask = sum(1 << wc[k] for k in names)
        nwin = (n - W) // step + 1
        out = blank(len(names), nwin, nch, nch)
        assert dev.window_pairs(cuda(x), W, step, ddof, mask, out) == nwin
        return [x], {"out": out.cpu().numpy()}
    return run


def _cases():
    cases = {}
    for L in (64, 0, 5):
        for normalize in (True, False):
            cases[f"xcorr-128-L{L}-{'norm' if normalize else 'raw'}-15"] = xcorr_case(2600, 37, 128, L, normalize, 15)
    for mask in (1, 4):
        cases[f"xcorr-128-L64-norm-{mask}"] = xcorr_case(2600, 37, 128, 64, True, mask)
    for normalize in (True, False):
        cases[f"xcorr-9-L4-{'norm' if normalize else 'raw'}-15"] = xcorr_case(2601, 37, 9, 4, normalize, 15)
    cases["xcorr-batches"] = xcorr_case(2602, 70, 128, 64, True, 14, n=187)
    for order in (1, 4, 5, 8, 9, 16):
        cases[f"granger-128-p{order}-7"] = granger_case(2610, 128, order, 7)
    cases["granger-16-p1-7"] = granger_case(2611, 16, 1, 7)
    for mask in (1, 2, 4):
        cases[f"granger-128-p5-{mask}"] = granger_case(2610, 128, 5, mask)
    for ddof in (0, 1):
        cases[f"pairs-real-ddof{ddof}"] = pairs_case(2620, False, ddof)
    cases["pairs-complex"] = pairs_case(2621, True, 1)
    return cases


CASES = _cases()


def digests(case):
    """{key: digest} of one case, keyed as the fixture is."""
    inputs, results = CASES[case]()
    found = {f"in:{case}": digest(np.concatenate([np.ravel(a.view(np.float64)) for a in inputs]))}
    found.update({f"out:{case}:{k}": digest(v) for k, v in results.items()})
    return found


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else HERE
    out = {}
    for case in CASES:
        out.update(digests(case))
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "g26_pairwin_bits.npz")
    np.savez_compressed(path, keys=np.array(list(out)), sha256=np.stack(list(out.values())))
    print(f"g26_pairwin_bits.npz: {os.path.getsize(path) / 1e3:.0f} kB, {len(out)} digests of {len(CASES)} cases")


if __name__ == "__main__":
    main()
