"""CPU-only tests of window_features (K15): the names, the argument errors (raised with no GPU and
before the stream is touched), the window bookkeeping of the streaming loop as a pure function
of the chunk lengths, the C ABI of the entry points against the header, the register report of
csrc/windowfeat.hip (no scratch in any kernel), and ``window_measures``, the NumPy restatement
of the thirteen definitions that tests/test_gpu_features.py compares the device against.  The
restatement is pinned here against scipy.stats and NumPy, against closed forms (the Teager
energy, mobility and complexity of a sine, the line length of a ramp, the zero crossings of a
sine) and on the NaN rule."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.stats as sst

from openseize_amd import _lib, features
from openseize_amd.features import windowed
from openseize_amd.features.windowed import window_features

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mean", "var", "rms", "skew", "kurtosis", "min", "max", "ptp", "line_length", "zero_crossings",
         "mobility", "complexity", "teager")
EXACT = ("min", "max", "ptp", "zero_crossings")


def window_measures(x, W, step, dtype=np.float64):
    """The definitions: name -> (C, nwin) for x (C, N), the windows gathered by index, the moments
    two-pass about each window's own mean, every sum in ``dtype``.  A window that holds a NaN is
    NaN in every feature."""
    x = np.atleast_2d(np.asarray(x))
    n = x.shape[-1]
    nwin = 0 if n < W else (n - W) // step + 1
    idx = np.arange(nwin)[:, None] * step + np.arange(W)[None, :]
    raw = x[:, idx]                                        # (C, nwin, W), float64
    w = raw.astype(dtype)
    with np.errstate(all="ignore"):
        mu = w.mean(-1, dtype=dtype)
        d = w - mu[..., None]
        m2, m3, m4 = ((d ** k).mean(-1, dtype=dtype) for k in (2, 3, 4))
        dx = np.diff(w, axis=-1)
        ddx = np.diff(dx, axis=-1)
        v1, v2 = dx.var(-1, dtype=dtype), ddx.var(-1, dtype=dtype)
        mob = np.sqrt(v1 / m2)
        out = {"mean": mu, "var": m2, "rms": np.sqrt((w * w).mean(-1, dtype=dtype)),
               "skew": m3 / m2 ** dtype(1.5), "kurtosis": m4 / m2 ** 2,
               "min": raw.min(-1), "max": raw.max(-1), "ptp": raw.max(-1) - raw.min(-1),
               "line_length": np.abs(dx).sum(-1, dtype=dtype),
               "zero_crossings": ((raw[..., 1:] < 0) != (raw[..., :-1] < 0)).sum(-1).astype(np.float64),
               "mobility": mob, "complexity": np.sqrt(v2 / v1) / mob,
               "teager": (w[..., 1:-1] ** 2 - w[..., :-2] * w[..., 2:]).mean(-1, dtype=dtype)}
    holds_nan = np.isnan(raw).any(-1)
    for name in NAMES:
        out[name] = np.where(holds_nan, np.nan, out[name])
    return out


def scales(x, W, step):
    """(the long-double restatement, name -> the scale its 1e-9 bound is relative to): ``mean`` mean |x|,
    ``skew`` max(1, |skew|), ``teager`` mean(x_t^2 + |x_{t-1} x_{t+1}|), the value itself for the rest."""
    ref = window_measures(x, W, step, np.longdouble)
    n = x.shape[-1]
    idx = np.arange((n - W) // step + 1)[:, None] * step + np.arange(W)[None, :]
    w = np.atleast_2d(x)[:, idx].astype(np.longdouble)
    sc = {name: np.abs(ref[name]) for name in NAMES}
    sc["mean"] = np.abs(w).mean(-1)
    sc["skew"] = np.maximum(1, np.abs(ref["skew"]))
    sc["teager"] = (w[..., 1:-1] ** 2 + np.abs(w[..., :-2] * w[..., 2:])).mean(-1)
    return ref, sc


def test_names_are_public():
    assert features.window_features is window_features
    assert features.WINDOW_FEATURES == windowed.WINDOW_FEATURES == NAMES == tuple(_lib.WINDOW_FEATURE)
    assert list(_lib.WINDOW_FEATURE.values()) == list(range(13))
    doc = window_features.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name


def test_restatement_against_scipy_and_numpy():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 3000)) ** 3 + 0.5            # skewed, heavy-tailed, offset
    for W, step in ((250, 125), (4, 1), (67, 200)):
        M = window_measures(x, W, step)
        nwin = (3000 - W) // step + 1
        for k in (0, nwin // 2, nwin - 1):
            w = x[:, k * step:k * step + W]
            for name, want in (("mean", w.mean(-1)), ("var", np.var(w, axis=-1)),
                               ("rms", np.sqrt(np.mean(w * w, axis=-1))),
                               ("skew", sst.skew(w, axis=-1, bias=True)),
                               ("kurtosis", sst.kurtosis(w, axis=-1, fisher=False, bias=True)),
                               ("min", w.min(-1)), ("max", w.max(-1)), ("ptp", np.ptp(w, axis=-1)),
                               ("line_length", np.abs(np.diff(w, axis=-1)).sum(-1))):
                assert M[name].shape == (3, nwin)
                np.testing.assert_allclose(M[name][:, k], want, rtol=1e-11, atol=1e-13, err_msg=f"{name} {W} {k}")
            dx = np.diff(w, axis=-1)
            mob = np.sqrt(np.var(dx, axis=-1) / np.var(w, axis=-1))
            np.testing.assert_allclose(M["mobility"][:, k], mob, rtol=1e-11)
            np.testing.assert_allclose(M["complexity"][:, k],
                                       np.sqrt(np.var(np.diff(dx, axis=-1), axis=-1) / np.var(dx, axis=-1)) / mob,
                                       rtol=1e-11)


def test_closed_forms():
    W, step, periods = 400, 150, 8                            # whole periods per window, whatever its start
    om = 2 * np.pi * periods / W
    t = np.arange(4000)
    amp, phi = 1.7, 0.4
    M = window_measures(amp * np.sin(om * t + phi), W, step)
    np.testing.assert_allclose(M["teager"], (amp * np.sin(om)) ** 2, rtol=1e-12)
    np.testing.assert_allclose(M["mean"], 0.0, atol=1e-13)
    np.testing.assert_allclose(M["var"], amp ** 2 / 2, rtol=1e-12)
    # dx = 2 A sin(om / 2) cos(om (t + 1/2) + phi) is a sine again, though over W - 1 samples: the
    # missing sample moves var(dx) by O(1 / W)
    assert np.max(np.abs(M["mobility"] / (2 * np.sin(om / 2)) - 1)) < 2.0 / W
    assert np.max(np.abs(M["complexity"] - 1)) < 4.0 / W
    # a sine crosses zero twice a period; a window of whole periods sees 2 periods crossings, one
    # fewer when one of them falls between its last sample and the next window's first
    zc = M["zero_crossings"]
    assert np.all((zc == 2 * periods) | (zc == 2 * periods - 1)) and np.any(zc == 2 * periods)
    first = amp * np.sin(om * t[:W] + phi)
    assert zc[0, 0] == np.count_nonzero(np.diff(np.signbit(first).astype(int)))
    slope = 0.37
    R = window_measures(np.stack([slope * t - 50.0, -2 * slope * t - 1.0]), 100, 70)
    np.testing.assert_allclose(R["line_length"][0], 99 * slope, rtol=1e-12)
    np.testing.assert_allclose(R["line_length"][1], 99 * 2 * slope, rtol=1e-12)
    np.testing.assert_allclose(R["ptp"][0], 99 * slope, rtol=1e-12)
    assert R["zero_crossings"][0].sum() == 1 and np.all(R["zero_crossings"][1] == 0)
    np.testing.assert_allclose(R["teager"][0], slope ** 2, rtol=1e-7)     # x_t^2 - (x_t - s)(x_t + s)


def test_nan_rule_and_longdouble_margin():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 2000)) + 100.0
    clean = window_measures(x, 250, 125)
    y = x.copy()
    y[0, 700] = np.nan
    y[1, 1990:] = np.nan
    M = window_measures(y, 250, 125)
    nwin = (2000 - 250) // 125 + 1
    k = np.arange(nwin)
    hit = np.stack([(k * 125 <= 700) & (700 < k * 125 + 250), k * 125 + 250 > 1990])
    assert hit[0].sum() == 2 and hit[1].sum() == 1
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), hit), name
        assert np.array_equal(M[name][~hit], clean[name][~hit]), name
    # the float64 restatement against the long-double one under the scales of the GPU test
    ref, sc = scales(x, 250, 125)
    for name in NAMES:
        err = float(np.max(np.abs(clean[name] - ref[name]) / sc[name])) if name not in EXACT else \
            float(np.max(np.abs(clean[name] - ref[name])))
        assert err < (2e-12 if name not in EXACT else 1e-300), (name, err)


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_features(x + 1j * x, 100)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_features(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_features(x, 501)
    cases = (({"winsize": 3}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "features": "power"}, "mean.*line_length.*teager"),
             ({"winsize": 100, "features": ("var", "RMS")}, "RMS.*mean"),
             ({"winsize": 100, "features": ()}, "mean"), ({"winsize": 100, "features": 3}, "mean"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_features(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_features(x, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_features(src.pro, 100, features=NAMES)
        assert not src.started

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device (this test runs without one)
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    with pytest.raises(ValueError, match="real data.*complex128 chunks"):
        window_features(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_features(x, 100, fs=100)                                   # no such argument


@pytest.mark.parametrize("W,step", [(250, 125), (67, 200), (4, 1), (100, 100), (64, 1000), (300, 299)])
def test_window_bookkeeping_is_a_function_of_the_chunk_lengths(W, step):
    """Overlap, gaps, chunks smaller than a window: every push starts at the next unfinished
    window, holds exactly the samples the windows it completes need, and carries the rest."""
    rng = np.random.default_rng(W + step)
    for lengths in ([7] * 300, [249, 250, 251, 4099, 1, 1, 1, 700], [5000], [W - 1, 1, step, 3 * step + 2, 0, 900],
                    list(rng.integers(0, 3 * max(W, step), 40))):
        plan = windowed.window_plan(lengths, W, step)
        total, seen, done, have, skip = sum(lengths), 0, 0, 0, 0
        for m, (start, nwin, keep, left) in zip(lengths, plan):
            seen += m
            # the push's samples are [start, seen) (when it holds any); its windows are done .. done + nwin
            if nwin:
                assert start == done * step, (lengths, start, done)
                assert (done + nwin - 1) * step + W <= seen                 # every window is whole ...
            assert (done + nwin) * step + W > seen                          # ... and no whole window waits
            done += nwin
            nxt = done * step                                               # the next unfinished window
            assert keep == max(0, seen - nxt) and left == max(0, nxt - seen), (lengths, keep, left)
            assert keep < W
            assert windowed._advance(have, skip, m, W, step) == (min(skip, m), nwin, keep, left)
            have, skip = keep, left
        assert done == windowed.window_count(total, W, step)


C_TYPES = {"const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "const double *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def test_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, nargs in (("osz_window_count", "int64_t", 3), ("osz_window_features", "int", 12)):
        m = re.search(r"\b" + ret + " " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared"
        declared = []
        for arg in m.group(1).split(","):
            ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()   # drop the name
            declared.append(C_TYPES[ctype])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C_TYPES[ret] and len(declared) == nargs
        assert argtypes == declared, (name, argtypes, declared)
        assert hasattr(lib, name), f"{name} not exported"
    for name, value in _lib.WINDOW_FEATURE.items():
        assert re.search(rf"OSZ_WF_{name.upper()} = {value}\b", header), name
    assert re.search(r"OSZ_WF_COUNT = 13\b", header)
    assert re.search(rf"#define OSZ_WF_LONG {_lib.WF_LONG}\b", header)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowfeat\.hip\b", makefile, re.M)


def test_window_count_needs_no_device():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.osz_window_count.restype, lib.osz_window_count.argtypes = _lib.SIGNATURES["osz_window_count"]
    for n, W, step, want in ((99, 100, 10, 0), (100, 100, 10, 1), (109, 100, 10, 1), (110, 100, 10, 2),
                             (0, 4, 1, 0), (4, 4, 1, 1), (70000, 4, 1, 69997),
                             (1000, 67, 200, 5), (866, 67, 200, 4), (867, 67, 200, 5),          # gaps
                             (2 ** 40, 1024, 512, 2 ** 31 - 1),
                             (-1, 100, 10, -1), (100, 3, 1, -1), (100, 100, 0, -1), (100, 100, -2, -1)):
        assert lib.osz_window_count(n, W, step) == want, (n, W, step)
        if want >= 0:
            assert windowed.window_count(n, W, step) == want


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_window_kernels_use_no_scratch(tmp_path):
    """Both kernels of windowfeat.hip, compiled for gfx950 with the library's flags: no scratch, no
    spilled VGPR."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowfeat.hip"), "-o", str(tmp_path / "windowfeat.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=csrc)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\S+)", line)
        if not m:
            continue
        if m.group(1).strip() == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    assert len(kernels) == 2 and any("window_wave_kernel" in k for k in kernels) \
        and any("window_block_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0", (name, use)
        assert int(use["VGPRs"]) + int(use["AGPRs"]) <= 128           # four waves a SIMD at the least
