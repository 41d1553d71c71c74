"""The argument checks of the three channel-pair window entry points -- osz_window_pairs (K19),
osz_window_xcorr (K23) and osz_window_granger (K24), csrc/pair_window.h -- and of their *_work
functions, driven through ctypes without a device: every check runs before the first HIP call, and
the library loads without a GPU.

The data pointers are small fake addresses that nothing dereferences, and every case has
n < winsize: no window, so a check that wrongly passed returns OSZ_OK -- which fails the assertion --
and cannot reach a launch.  (The checks of plane_pitch and of more than INT32_MAX windows need
windows and are not reached here; and without a window the work space is empty but for complex
K19's staged planes, so "work_len one short" is -1 everywhere else.)  For every class of bad argument the return is OSZ_ERR_INVALID
and osz_last_error() names the function and the offending value; where the plan refuses the sizes,
the matching *_work function returns -1."""

import re

import pytest

from openseize_amd import _lib

X, XC, OUT, WORK = 0x1000, 0x4000, 0x2000, 0x3000      # 16-byte aligned, never read
NCH, N, W, PITCH = 3, 10, 64, 16                        # n < winsize

# name -> (shortest, longest window (None: no limit), mask bits, the function's own parameter and
# its value in the accepted case)
ENTRIES = {
    "osz_window_pairs": (4, None, len(_lib.WINDOW_CONNECTIVITY), "is_complex", 0),
    "osz_window_xcorr": (8, _lib.WX_LONGEST, len(_lib.WINDOW_XCORR), "maxlag", 2),
    "osz_window_granger": (16, _lib.WG_LONGEST, len(_lib.WINDOW_GRANGER), "order", 2),
}
REAL, COMPLEX = 3, 28                                   # K19's masks: cov | corr, aec | plv | ciplv


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def arguments(name, **change):
    lo, hi, bits, own, value = ENTRIES[name]
    a = dict(x=X, pitch=PITCH, nch=NCH, n=N, winsize=W, step=5, mask=REAL if name == "osz_window_pairs" else (1 << bits) - 1,
             out=OUT, xcorr=XC, plane_pitch=0, work=WORK, work_len=None, ddof=1, normalize=1)
    a[own] = value
    a.update(change)
    assert a["n"] < a["winsize"], "every case is one without a window"
    return a, own


def work(lib, name, **change):
    """What ``name``_work answers for the arguments of ``call``."""
    a, own = arguments(name, **change)
    return getattr(lib, name + "_work")(a["nch"], a["n"], a["winsize"], a["step"],
                                        *((a["mask"], a[own]) if name == "osz_window_pairs" else (a[own], a["mask"])))


def call(lib, name, **change):
    """(status, message) of ``name`` on valid arguments with no window, but for ``change``;
    ``work_len`` is what ``name``_work asks for (0 where it refuses) plus ``short``."""
    short = change.pop("short", 0)
    a, own = arguments(name, **change)
    if a["work_len"] is None:
        a["work_len"] = max(work(lib, name, **change), 0) + short
    head = (a["x"], a["pitch"], a["nch"], a["n"])
    tail = (a["plane_pitch"], a["work"], a["work_len"], None)
    if name == "osz_window_pairs":
        args = head + (a[own], a["winsize"], a["step"], a["ddof"], a["mask"], a["out"]) + tail
    elif name == "osz_window_xcorr":
        args = head + (a["winsize"], a["step"], a[own], a["normalize"], a["mask"], a["xcorr"], a["out"]) + tail
    else:
        args = head + (a["winsize"], a["step"], a[own], a["mask"], a["out"]) + tail
    status = getattr(lib, name)(*args)
    return status, lib.osz_last_error().decode()


def cases(name):
    """label -> (the changed arguments, what the message says, whether the plan refuses them)."""
    lo, hi, bits, own, value = ENTRIES[name]
    found = {
        "null x": (dict(x=None), "null", False),
        "null out": (dict(out=None), "null", False),
        "null work": (dict(work=None), "null", False),
        "nch 1": (dict(nch=1), "nch 1,", True),
        "nch 16385": (dict(nch=16385), "nch 16385,", True),
        "negative n": (dict(n=-1), "n -1,", True),
        "winsize below": (dict(winsize=lo - 1, n=2, **({own: 1} if name == "osz_window_granger" else {})),
                          f"winsize {lo - 1},", True),
        "step 0": (dict(step=0), "step 0,", True),
        "mask 0": (dict(mask=0), "mask 0", True),
        "mask past the last bit": (dict(mask=1 << bits), f"mask {1 << bits}", True),
        "pitch < n": (dict(pitch=N - 1), f"pitch {N - 1} is less than n {N}", False),
        "x not aligned": (dict(x=X + 4), "aligned", False),
        "out not aligned": (dict(out=OUT + 4), "aligned", False),
        "work not aligned": (dict(work=WORK + 4), "aligned", False),
        "work_len one short": (dict(short=-1), "work holds -1 doubles", False),
    }
    if hi is not None:
        found["winsize above"] = (dict(winsize=hi + 1), f"winsize {hi + 1},", True)
    if name == "osz_window_pairs":
        found.update({
            "ddof 2": (dict(ddof=2), "ddof must be 0 or 1, got 2", False),
            "real measures of complex data": (dict(is_complex=1), "complex 1", True),
            "complex measures of real data": (dict(mask=COMPLEX), "complex 0", True),
            "real and complex measures": (dict(mask=REAL | COMPLEX, is_complex=1), "complex 1", True),
            "complex x not 16-byte aligned": (dict(is_complex=1, mask=COMPLEX, x=X + 8), "aligned", False),
            "complex work_len one short": (dict(is_complex=1, mask=COMPLEX, short=-1),
                                           f"work holds {3 * NCH * N - 1} doubles", False),
        })
    elif name == "osz_window_xcorr":
        found.update({
            "null xcorr": (dict(xcorr=None), "null", False),
            "null out, the lag alone": (dict(out=None, mask=4), "null", False),
            "maxlag -1": (dict(maxlag=-1), "maxlag -1", True),
            "maxlag 65": (dict(maxlag=_lib.WX_MAXLAG + 1, winsize=256), f"maxlag {_lib.WX_MAXLAG + 1}", True),
            "maxlag above W / 2": (dict(maxlag=W // 2 + 1), f"maxlag {W // 2 + 1}", True),
            "normalize 2": (dict(normalize=2), "normalize must be 0 or 1, got 2", False),
            "xcorr not aligned": (dict(xcorr=XC + 4), "aligned", False),
        })
    else:
        found.update({
            "order 0": (dict(order=0), "order 0", True),
            "order 17": (dict(order=_lib.WG_MAXORDER + 1, winsize=256), f"order {_lib.WG_MAXORDER + 1}", True),
            "order above W / 8": (dict(order=W // 8 + 1), f"order {W // 8 + 1}", True),
        })
    return found


@pytest.mark.parametrize("name", list(ENTRIES))
def test_valid_arguments_without_a_window_are_accepted(lib, name):
    status, msg = call(lib, name)
    assert status == _lib.OSZ_OK, msg
    assert work(lib, name) >= 0
    lo, hi, bits, own, value = ENTRIES[name]
    edge = dict(nch=16384, winsize=lo, n=lo - 1, pitch=lo)       # the ends of the ranges are inside them
    edge.update({"osz_window_xcorr": dict(maxlag=lo // 2), "osz_window_granger": dict(order=lo // 8)}.get(name, {}))
    status, msg = call(lib, name, **edge)
    assert status == _lib.OSZ_OK and work(lib, name, **edge) >= 0, msg


def test_the_arrays_a_mask_does_not_write_may_be_null(lib):
    for change in (dict(mask=1, out=None), dict(mask=14, xcorr=None)):
        status, msg = call(lib, "osz_window_xcorr", **change)
        assert status == _lib.OSZ_OK, msg


def test_complex_rows_are_accepted_and_their_stage_is_counted(lib):
    status, msg = call(lib, "osz_window_pairs", is_complex=1, mask=COMPLEX)
    assert status == _lib.OSZ_OK, msg
    assert work(lib, "osz_window_pairs", is_complex=1, mask=COMPLEX) == 3 * NCH * N


@pytest.mark.parametrize("name,label", [(name, label) for name in ENTRIES for label in cases(name)])
def test_a_bad_argument_is_refused(lib, name, label):
    change, says, planned = cases(name)[label]
    status, msg = call(lib, name, **change)
    assert status == _lib.OSZ_ERR_INVALID, (status, msg)
    assert msg.startswith(name + ": ") and re.search(re.escape(says) + r"(?!\d)", msg), msg
    change.pop("short", None)
    assert (work(lib, name, **change) == -1) == planned
