"""CPU-only tests of window_quantiles (K17): ``window_quantile_stats``, the NumPy restatement of the
definitions that tests/test_gpu_quantiles.py compares the device against bit for bit -- pinned
here against numpy.median, numpy.quantile(method="linear") and the median of the absolute
deviations, on closed forms, on signed zeros and on the rules for +-inf and NaN -- the argument
errors (raised with no GPU and before the stream is touched), the C ABI of the entry point against
the header, and the register report of csrc/windowquant.hip (no scratch in any kernel)."""

import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from openseize_amd import _lib, features
from openseize_amd.features import quantiles, windowed
from openseize_amd.features.quantiles import window_quantiles

from test_csd_host import Untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("median", "mad", "quantile")
Q = (0, 0.05, 0.25, 1 / 3, 0.5, 0.75, 0.9, 1)
# every padded width has a kernel instance of its own: a window is padded to the first that holds it
BOUNDS = tuple(2 ** e for e in range(_lib.WQ_NARROWEST.bit_length() - 1, _lib.WQ_LONGEST.bit_length()))


def total_order_keys(w):
    """uint64 keys whose order is the total order of the float64 ``w``: all bits of a negative value
    flipped, the sign bit of the others (-0.0 before +0.0)."""
    b = np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ np.uint64(1 << 63))


def sort_total(w):
    """``w`` ascending along its last axis in the total order."""
    return np.take_along_axis(w, np.argsort(total_order_keys(w), axis=-1, kind="stable"), axis=-1)


def median_of_sorted(s):
    W = s.shape[-1]
    with np.errstate(all="ignore"):
        return (s[..., (W - 1) // 2] + s[..., W // 2]) / 2.0


def quantile_of_sorted(s, p):
    W = s.shape[-1]
    h = float(p) * float(W - 1)
    lo = math.floor(h)
    g, hi = h - lo, min(lo + 1, W - 1)
    a, b = s[..., lo], s[..., hi]
    with np.errstate(all="ignore"):
        d = b - a
        v = a + d * g if g < 0.5 else b - d * (1.0 - g)
    return np.where(a == b, a, v)


def window_quantile_stats(x, W, step, q=Q):
    """The definitions: "median" and "mad" (C, nwin), "quantile" (len(q), C, nwin) for x (C, N).  A
    window that holds a NaN is NaN in every measure; so is the mad where a deviation is NaN."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    win = np.lib.stride_tricks.sliding_window_view(x, W, axis=-1)[:, ::step]
    wild = np.isnan(win).any(axis=-1)
    s = sort_total(win)
    med = median_of_sorted(s)
    with np.errstate(all="ignore"):
        dev = np.abs(win - med[..., None])
    lost = np.isnan(dev).any(axis=-1)
    mad = median_of_sorted(sort_total(np.where(lost[..., None], 0.0, dev)))
    out = {"median": np.where(wild, np.nan, med), "mad": np.where(lost, np.nan, mad),
           "quantile": np.stack([np.where(wild, np.nan, quantile_of_sorted(s, p)) for p in q])}
    return out


def one(w, q=Q):
    """The measures of one window: median and mad as floats, the quantiles as an array."""
    w = np.asarray(w, dtype=np.float64)
    M = window_quantile_stats(w, w.shape[0], 1, q)
    return float(M["median"][0, 0]), float(M["mad"][0, 0]), M["quantile"][:, 0, 0]


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_names_are_public():
    assert features.window_quantiles is window_quantiles
    assert features.WINDOW_QUANTILES == quantiles.WINDOW_QUANTILES == NAMES == tuple(_lib.WINDOW_QUANTILE)
    assert list(_lib.WINDOW_QUANTILE.values()) == list(range(3))
    assert quantiles.window_plan is windowed.window_plan and quantiles._advance is windowed._advance
    assert quantiles.window_count is windowed.window_count
    # one loop and one bound for the family: no module keeps a copy that a patch would miss
    assert quantiles._stream is windowed._stream and windowed._advance is quantiles._stream._advance
    assert not hasattr(quantiles, "_PUSH_BYTES") and not hasattr(windowed, "_PUSH_BYTES")
    assert BOUNDS[0] == _lib.WQ_NARROWEST and BOUNDS[-1] == _lib.WQ_LONGEST and _lib.WQ_WAVE in BOUNDS
    doc = window_quantiles.__doc__
    for name in NAMES:
        assert f'"{name}"' in doc, name


@pytest.mark.parametrize("W", [4, 5, 63, 64, 65, 250, 1000, 4096])
def test_restatement_is_numpy_bit_for_bit(W):
    rng = np.random.default_rng(17)
    n = W + 2 * max(W // 3, 1)
    x = np.cumsum(rng.standard_normal((3, n)), axis=-1) * 0.3 + rng.standard_normal((3, n)) + 100.0
    step = max(W // 3, 1)
    M = window_quantile_stats(x, W, step)
    win = np.lib.stride_tricks.sliding_window_view(x, W, axis=-1)[:, ::step]
    assert M["median"].shape == win.shape[:2] == (3, 3)
    assert same(M["median"], np.median(win, axis=-1))
    assert same(M["quantile"], np.quantile(win, Q, axis=-1, method="linear"))
    med = np.median(win, axis=-1)
    assert same(M["mad"], np.median(np.abs(win - med[..., None]), axis=-1))
    assert np.all(M["mad"] > 0)
    assert same(M["quantile"][4], M["median"]) or W % 2 == 0     # an odd window's middle sample
    assert np.all(np.diff(M["quantile"], axis=0) >= 0)


def test_closed_forms():
    for W in (4, 5, 64, 101):
        med, mad, qs = one(np.full(W, 3.25))
        assert med == 3.25 and mad == 0 and np.all(qs == 3.25)
        w = np.arange(W - 1, -1, -1.0)                           # 0 .. W - 1, reversed
        med, mad, qs = one(w)
        assert med == (W - 1) / 2
        assert mad == np.median(np.abs(np.arange(W) - (W - 1) / 2))
        assert mad == (W // 4 if W % 2 else W / 4)               # (these W) odd: 0 1 1 2 2 ..; even: .5 .5 1.5 1.5 ..
        assert qs[0] == 0 == w.min() and qs[-1] == W - 1 == w.max()
        assert qs[4] == med
        for p, v in zip(Q, qs):
            assert abs(v - p * (W - 1)) <= 2e-16 * W, (W, p)
    # even and odd W: the two middle samples and the one
    assert one([4.0, 1.0, 3.0, 2.0])[0] == 2.5 and one([5.0, 4.0, 1.0, 3.0, 2.0])[0] == 3.0
    assert one([4.0, 1.0, 3.0, 2.0])[1] == 1.0 and one([5.0, 4.0, 1.0, 3.0, 2.0])[1] == 1.0
    # _lerp: a + d g below one half, b - d (1 - g) from there on
    a, b = 1.0, 1.0 + 2.0 ** -20
    w = [a, b, a, b, b]                                          # sorted a a b b b
    _, _, qs = one(w, (0.3, 0.45))                               # h = 1.2, 1.8: lo = 1, hi = 2
    assert qs[0] == a + (b - a) * (1.2 - 1) and qs[1] == b - (b - a) * (1.0 - (0.45 * 4 - 1))


def test_signed_zeros_sort_by_their_bits():
    keys = total_order_keys(np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf]))
    assert np.all(np.diff(keys.astype(object)) > 0)
    w = np.array([0.0, -0.0, 0.0, -0.0])
    s = sort_total(w)
    assert same(s, [-0.0, -0.0, 0.0, 0.0])
    med, mad, qs = one(w, (0, 0.25, 1 / 3, 0.5, 1))
    assert same(med, 0.0) and same(mad, 0.0)                     # (-0.0 + 0.0) / 2 = +0.0
    assert same(qs, [-0.0, -0.0, -0.0, -0.0, 0.0])               # -0.0 == 0.0: a is returned, s_lo as it is
    assert same(one([-0.0, -0.0, -0.0, 0.0, 1.0])[0], -0.0)      # an odd window: (-0.0 + -0.0) / 2


def test_infinities_are_ordinary_values_and_nan_takes_the_window():
    inf = np.inf
    med, mad, qs = one([1.0, -inf, 3.0, 2.0, inf, 4.0, 5.0], (0, 0.5, 1))      # a minority
    assert med == 3.0 and mad == 2.0 and same(qs[1:], [3.0, inf])
    assert np.isnan(qs[0])                                       # a = -inf, b = 1, g = 0: -inf + inf 0
    med, mad, qs = one([inf, 1.0, inf, inf, 2.0], (0, 0.1, 0.5, 0.9, 1))        # a majority
    assert med == inf and np.isnan(mad)                          # inf - inf among the deviations
    assert qs[0] == 1.0 and qs[2] == inf and qs[4] == inf and qs[3] == inf      # a == b: a
    assert qs[1] == 1.0 + (2.0 - 1.0) * (0.1 * 4)
    # between 2 and 3; between 3 and inf below one half, a + inf g, and above it, inf - inf (1 - g)
    med, mad, qs = one([1.0, inf, 2.0, 3.0], (0.4, 0.7, 0.9))
    assert med == 2.5 and mad == 1.0
    assert qs[0] == 2.0 + 1.0 * (0.4 * 3 - 1) and qs[1] == inf and np.isnan(qs[2])
    med, mad, qs = one([-inf, -inf, inf, inf], (0.5,))
    assert np.isnan(med) and np.isnan(mad) and np.isnan(qs[0])   # -inf + inf
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 600))
    clean = window_quantile_stats(x, 100, 50)
    y = x.copy()
    y[0, 170] = np.nan
    y[1, 599] = -np.nan
    M = window_quantile_stats(y, 100, 50)
    k = np.arange(11)
    hit = np.stack([(k * 50 <= 170) & (170 < k * 50 + 100), k * 50 + 100 > 599])
    assert hit[0].sum() == 2 and hit[1].sum() == 1
    for name in NAMES:
        assert np.array_equal(np.isnan(M[name]), np.broadcast_to(hit, M[name].shape)), name
        assert same(M[name][..., ~hit], clean[name][..., ~hit]), name


def test_argument_errors_come_before_the_stream():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 500))
    with pytest.raises(ValueError, match="real data"):
        window_quantiles(x + 1j * x, 100)
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        window_quantiles(x.reshape(2, 2, 500), 100)
    with pytest.raises(ValueError, match="fewer than one window"):
        window_quantiles(x, 501)
    longest, qmost = _lib.WQ_LONGEST, _lib.WQ_QMOST
    cases = (({"winsize": 3}, "winsize"), ({"winsize": 0}, "winsize"), ({"winsize": 100.0}, "winsize"),
             ({"winsize": "100"}, "winsize"), ({"winsize": True}, "winsize"),
             ({"winsize": longest + 1}, f"winsize.*{longest}"),
             ({"winsize": 100, "step": 0}, "step"), ({"winsize": 100, "step": -5}, "step"),
             ({"winsize": 100, "step": 12.5}, "step"),
             ({"winsize": 100, "measures": "mean"}, "median.*mad.*quantile"),
             ({"winsize": 100, "measures": ("median", "Mad")}, "Mad.*median"),
             ({"winsize": 100, "measures": ()}, "median"), ({"winsize": 100, "measures": 3}, "median"),
             ({"winsize": 100, "measures": "quantile", "q": ()}, f"1 to {qmost}"),
             ({"winsize": 100, "measures": "quantile", "q": [0.5] * (qmost + 1)}, f"1 to {qmost}"),
             ({"winsize": 100, "measures": "quantile", "q": np.nan}, r"\[0, 1\]"),
             ({"winsize": 100, "measures": "quantile", "q": (0.5, np.inf)}, r"\[0, 1\]"),
             ({"winsize": 100, "measures": "quantile", "q": -1e-9}, r"\[0, 1\]"),
             ({"winsize": 100, "measures": ("median", "quantile"), "q": (0.5, 1.0000001)}, r"\[0, 1\]"),
             ({"winsize": 100, "measures": "quantile", "q": "0.5"}, r"\[0, 1\]"),
             ({"winsize": 100, "measures": "quantile", "q": (0.5, "0.7")}, r"\[0, 1\]"),
             ({"winsize": 100, "measures": "quantile", "q": None}, r"\[0, 1\]"))
    for kwargs, match in cases:
        src = Untouched((4, 5000))
        with pytest.raises(ValueError, match=match):
            window_quantiles(src.pro, **kwargs)
        assert not src.started, kwargs
        with pytest.raises(ValueError, match=match):
            window_quantiles(x, **kwargs)
    for shape, match in (((2, 2, 5000), "one- or two-dimensional"), ((4, 50), "fewer than one window")):
        src = Untouched(shape)
        with pytest.raises(ValueError, match=match):
            window_quantiles(src.pro, 100, measures=NAMES)
        assert not src.started

    # a producer shows what it holds only with its first chunk: complex chunks raise then, and
    # nothing has been asked of the device (this test runs without one)
    def gen():
        yield np.zeros((4, 5000), dtype=np.complex128)
    from openseize_amd import producer
    with pytest.raises(ValueError, match="real data.*complex128 chunks"):
        window_quantiles(producer(gen, chunksize=1000, axis=-1, shape=(4, 5000)), 100)
    with pytest.raises(TypeError):
        window_quantiles(x, 100, fs=100)                                  # no such argument


C_TYPES = {"void *": ctypes.c_void_p, "double *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}


def test_entry_point_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "osz_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "build libosz_hip.so first (__graft_entry__.build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    m = re.search(r"\bint osz_window_quantiles\(([^)]*)\);", header)
    assert m, "osz_window_quantiles is not declared"
    declared = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()).replace("*", "* ")).strip()       # drop the name
        declared.append(C_TYPES[ctype])
    restype, argtypes = _lib.SIGNATURES["osz_window_quantiles"]
    assert restype is ctypes.c_int and len(declared) == 14
    assert argtypes == declared, (argtypes, declared)
    assert hasattr(lib, "osz_window_quantiles"), "osz_window_quantiles not exported"
    for name, value in _lib.WINDOW_QUANTILE.items():
        assert re.search(rf"OSZ_WQ_{name.upper()} = {value}\b", header), name
    assert re.search(r"typedef enum \{[^}]*OSZ_WQ_COUNT = 3\s*\} osz_window_quantiles_measure;", header)
    for name in ("LONGEST", "QMOST", "NARROWEST", "WAVE"):
        assert re.search(rf"#define OSZ_WQ_{name} {getattr(_lib, 'WQ_' + name)}\b", header), name
    assert (_lib.WQ_LONGEST, _lib.WQ_QMOST) == (4096, 16)
    makefile = open(os.path.join(ROOT, "openseize_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwindowquant\.hip\b", makefile, re.M)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_quantile_kernels_use_no_scratch(tmp_path):
    """Every instance of the kernel of windowquant.hip -- one per padded width -- compiled for gfx950
    with the library's flags: no scratch, no spilled register."""
    csrc = os.path.join(ROOT, "openseize_amd", "csrc")
    res = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          os.path.join(csrc, "windowquant.hip"), "-o", str(tmp_path / "windowquant.o"),
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
    assert len(kernels) == len(BOUNDS) and all("window_quantiles_kernel" in k for k in kernels), sorted(kernels)
    for name, use in kernels.items():
        print(name, use)
        assert use["ScratchSize"] == "0" and use["VGPRs Spill"] == "0" and use["SGPRs Spill"] == "0", (name, use)
