"""Generate tests/golden/g25_window_bits.npz by RUNNING the per-channel window kernels on the GPU.

Run on a build of the commit BEFORE the kernels moved onto csrc/window_block.h, from the
repository root (the output directory is optional, tests/golden by default):

    python tests/golden/make_golden_window_bits.py [outdir]

Only digests are written, ``sha256[k]`` under the name ``keys[k]``: per case ``in:<case>``, the
SHA-256 of the inputs' bytes (a changed random stream shows up as such, not as a kernel
failure), and per result ``out:<case>:<name>``, the SHA-256 of the result's bytes with every NaN
replaced by one canonical NaN first.
tests/test_gpu_window_bits.py loads this file as a module, reruns ``CASES`` and compares.

Results come from the openseize_amd._device wrappers directly.  Every case has 3 channels whose
rows are a slice of a wider tensor (pitch > n), 5 overlapping windows with a step that is below W
and no divisor of it, and writes from win0 = 2 on into a result with room to spare that starts as
-7.0 and is digested whole: the cells no window owns are shown untouched.  Each case runs twice:
``clean`` on seeded normal noise, ``spoilt`` on the same noise with a NaN in channel 0 that only
window 0 holds, +inf in channel 1 that only the last window holds and -inf in channel 2 in windows
0 and 1.  W is the shortest window that reaches each compiled instance:
  features-<W>    100: the wave kernel; 4166: the workgroup kernel, whose last pass of 256 is
        partial; all thirteen features.  features-8-groups: W = 8, step 1, n = 16391, one channel:
        16384 windows, which the entry point hands out two to a wave.
  entropy-<W>     100: 64 threads; 600: 256; every measure.
  quantiles-<W>   50, 100, 200, 400, 600, 1500, 3000: the seven padded widths; median, mad and
        three quantiles.
  fractal-<W>     100, 600; every measure, kmax 8 and the default scales.
  wavelet-<W>-<taps>-<center>   W = 96 with 3 levels (one wave), W = 1024 with 4 levels (256
        threads); db2 and db4; every feature.  (It takes no win0: its result starts at 0.)
  ar-<W>-<method>-<center>      48, 100, 200, 400 (64 threads, 1, 2, 4, 8 samples a thread) and 512,
        600, 1500, 3000 (256 threads, 2, 4, 8, 16); order 8, all four measures.
  spectral-<nfft>   osz_spectral_features as tests/test_gpu_spectral.py drives it, all nine
        features: 250 (124 bins, one wave) and 8196 (4097 bins, 256 threads, two tiles); ``spoilt``
        has a NaN in one row and an all-zero row.
"""

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NCH, NWIN, WIN0, SPARE, LEFT, RIGHT = 3, 5, 2, 3, 5, 32
QUANTILES = (0.1, 0.5, 0.9)
SPECTRAL_EDGES = (0.5, 0.9, 0.95, 1.0)
SPECTRAL_DF = 0.37


def digest(a):
    """SHA-256 of the bytes of a float64 array, every NaN made the canonical one."""
    v = np.ascontiguousarray(a).view(np.float64).copy()
    v[np.isnan(v)] = np.nan
    return np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def streams(seed, W, step=None, nch=NCH, nwin=NWIN):
    """(step, {"clean": x, "spoilt": x}): (nch, n) noise that holds ``nwin`` windows and a few samples more."""
    step = W // 3 + 1 if step is None else step
    assert step < W and (W % step or step == 1)
    n = W + (nwin - 1) * step + min(step - 1, 7)
    x = np.random.default_rng(seed).standard_normal((nch, n))
    bad = x.copy()
    if nch == 1:
        bad[0, 3], bad[0, 5000], bad[0, 9000] = np.nan, np.inf, -np.inf
    else:
        bad[0, min(3, step - 1)] = np.nan                  # window 0 alone
        bad[1, (nwin - 1) * step + W - 1] = np.inf         # the last window alone
        bad[2, step + 1] = -np.inf                         # windows 0 and 1
    return step, {"clean": x, "spoilt": bad}


def sliced(x):
    """x as rows of a wider CUDA tensor: the pitch is LEFT + n + RIGHT."""
    wide = np.full((x.shape[0], LEFT + x.shape[1] + RIGHT), 1e300)
    wide[:, LEFT:LEFT + x.shape[1]] = x
    return cuda(wide)[:, LEFT:LEFT + x.shape[1]]


def result(planes, nch, nwin, win0=WIN0):
    import torch
    return torch.full((planes, nch, win0 + nwin + SPARE), -7.0, dtype=torch.float64, device="cuda")


def window_case(seed, W, planes, launch, extra=(), step=None, nch=NCH, nwin=NWIN, win0=WIN0):
    """``launch(dev, x2d, W, step, out, win0)`` on both streams."""
    def run():
        from openseize_amd import _device as dev
        s, xs = streams(seed, W, step, nch, nwin)
        found = {}
        for tag, x in xs.items():
            out = result(planes, nch, nwin, win0)
            assert launch(dev, sliced(x), W, s, out, win0) == nwin
            found[tag] = out.cpu().numpy()
        return list(xs.values()) + [np.asarray(e, dtype=np.float64) for e in extra], found
    return run


def features(dev, x, W, step, out, win0):
    from openseize_amd import _lib
    return dev.window_features(x, W, step, (1 << len(_lib.WINDOW_FEATURE)) - 1, out, win0)


def entropy(dev, x, W, step, out, win0):
    return dev.window_entropy(x, W, step, 15, 2, 0.2, "std", 3, 1, True, out, win0)


def quantiles(dev, x, W, step, out, win0):
    return dev.window_quantiles(x, W, step, 7, QUANTILES, out, win0)


def fractal(scales):
    def launch(dev, x, W, step, out, win0):
        return dev.window_fractal(x, W, step, 31, 8, scales, out, win0)
    return launch


def wavelet(lo, levels, center):
    def launch(dev, x, W, step, out, win0):
        return dev.window_wavelet(x, W, step, 31, lo, levels, center, True, out)
    return launch


def ar(method, center):
    def launch(dev, x, W, step, out, win0):
        return dev.window_ar(x, W, step, 15, 8, method, center, out, win0)
    return launch


def spectral_case(nfft):
    def run():
        from openseize_amd import _device as dev
        from openseize_amd import _lib
        nfreq = nfft // 2 + 1
        k0, k1 = 1, nfreq - 2
        n = k1 - k0 + 1
        a, b, c, d = k0, k0 + max(1, n // 4), k0 + max(2, n // 2), k1 + 1
        bands = ((a, b), (b, c), (c, d), (a, d), (b, d))
        P = 10.0 ** np.random.default_rng(nfft).uniform(-3, 3, (NWIN, NCH, nfreq))
        bad = P.copy()
        bad[1, 0, n // 2] = np.nan
        bad[3, 2] = 0.0
        mask = (1 << len(_lib.WINDOW_SPECTRAL)) - 1
        found = {}
        for tag, rows in (("clean", P), ("spoilt", bad)):
            out = result(dev.spectral_planes(mask, len(bands), len(SPECTRAL_EDGES)), NCH, NWIN)
            assert dev.spectral_features(cuda(rows), k0, k1, SPECTRAL_DF, bands, SPECTRAL_EDGES, True, mask, out,
                                         WIN0) == NWIN
            found[tag] = out.cpu().numpy()
        return [P, bad], found
    return run


def _cases():
    from openseize_amd.features.fractal import dfa_scales
    from openseize_amd.features.wavelet import wavelet_filters
    cases = {}
    for W in (100, 4166):
        cases[f"features-{W}"] = window_case(2500 + W, W, 13, features)
    cases["features-8-groups"] = window_case(2508, 8, 13, features, step=1, nch=1, nwin=16384)
    for W in (100, 600):
        cases[f"entropy-{W}"] = window_case(2510 + W, W, 4, entropy)
    for W in (50, 100, 200, 400, 600, 1500, 3000):
        cases[f"quantiles-{W}"] = window_case(2520 + W, W, 2 + len(QUANTILES), quantiles)
    for W in (100, 600):
        scales = dfa_scales(W)
        cases[f"fractal-{W}"] = window_case(2530 + W, W, 4 + len(scales), fractal(scales), extra=[scales])
    for W, levels in ((96, 3), (1024, 4)):
        for name in ("db2", "db4"):
            lo = wavelet_filters(name)[0]
            for center in (False, True):
                cases[f"wavelet-{W}-{len(lo)}-{'centred' if center else 'plain'}"] = window_case(
                    2540 + W, W, 4 * (levels + 1) + 1, wavelet(lo, levels, center), extra=[lo], win0=0)
    for W in (48, 100, 200, 400, 512, 600, 1500, 3000):
        for method in ("burg", "yule_walker"):
            for center in (False, True):
                cases[f"ar-{W}-{method}-{'centred' if center else 'plain'}"] = window_case(
                    2550 + W, W, 8 + 8 + 1 + 9, ar(method, center))
    for nfft in (250, 8196):
        cases[f"spectral-{nfft}"] = spectral_case(nfft)
    return cases


CASES = _cases()


def digests(case):
    """{key: digest} of one case, keyed as the fixture is."""
    inputs, results = CASES[case]()
    found = {f"in:{case}": digest(np.concatenate([np.ravel(a) for a in inputs]))}
    found.update({f"out:{case}:{k}": digest(v) for k, v in results.items()})
    return found


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else HERE
    out = {}
    for case in CASES:
        out.update(digests(case))
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "g25_window_bits.npz")
    np.savez_compressed(path, keys=np.array(list(out)), sha256=np.stack(list(out.values())))
    print(f"g25_window_bits.npz: {os.path.getsize(path) / 1e3:.0f} kB, {len(out)} digests of {len(CASES)} cases")


if __name__ == "__main__":
    main()
