"""The argument checks that the six per-channel window entry points share (csrc/window_block.h),
driven through ctypes without a device: every check runs before the first HIP call, and the
library loads without a GPU.

The data pointers are small fake addresses that nothing dereferences, and every case has
n < winsize: no window, so a check that wrongly passed returns OSZ_OK -- which fails the assertion --
and cannot reach a launch.  (The check of the workgroup count needs windows and is not reached
here.)  For every class of bad argument the return is OSZ_ERR_INVALID and osz_last_error() names
the function and says what was wrong, in the wording the callers know."""

import ctypes

import pytest

from openseize_amd import _lib

X, OUT = 0x1000, 0x2000                 # 8-byte aligned, never read
NCH, N, W, PITCH = 3, 10, 64, 16        # n < winsize
ROW, WIN0 = 8, 2
Q = (ctypes.c_double * 3)(0.1, 0.5, 0.9)
SCALES = (ctypes.c_int * 3)(4, 8, 16)
TAPS = (ctypes.c_double * 4)(0.48296291314469025, 0.836516303737469, 0.22414386804185735, -0.12940952255092145)


def vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


# name -> (shortest, longest window, mask bits, the mask's noun, takes win0, the arguments between
# mask and out)
ENTRIES = {
    "osz_window_features": (4, 1 << 27, len(_lib.WINDOW_FEATURE), "feature", True, ()),
    "osz_window_entropy": (4, _lib.WE_LONGEST, len(_lib.WINDOW_ENTROPY), "measure", True, (2, 0.2, 0, 3, 1, 1)),
    "osz_window_quantiles": (4, _lib.WQ_LONGEST, len(_lib.WINDOW_QUANTILE), "measure", True, (vp(Q), 3)),
    "osz_window_fractal": (8, _lib.WR_LONGEST, len(_lib.WINDOW_FRACTAL), "measure", True, (8, vp(SCALES), 3)),
    "osz_window_wavelet": (8, _lib.WW_LONGEST, len(_lib.WINDOW_WAVELET), "feature", False, (vp(TAPS), 4, 2, 1, 1)),
    "osz_window_ar": (16, _lib.AR_LONGEST, len(_lib.WINDOW_AR), "measure", True, (8, 0, 1)),
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, name, **change):
    """(status, message) of ``name`` on valid arguments with no window, but for ``change``."""
    lo, hi, bits, noun, has_win0, own = ENTRIES[name]
    win0 = WIN0 if has_win0 else 0
    a = dict(x=X, pitch=PITCH, nch=NCH, n=N, winsize=W, step=5, mask=(1 << bits) - 1, out=OUT,
             plane_pitch=(NCH - 1) * ROW + win0, row_pitch=ROW, win0=win0)
    a.update(change)
    args = (a["x"], a["pitch"], a["nch"], a["n"], a["winsize"], a["step"], a["mask"]) + own + (
        a["out"], a["plane_pitch"], a["row_pitch"]) + ((a["win0"],) if has_win0 else ()) + (None,)
    assert a["n"] < a["winsize"], "every case is one without a window"
    status = getattr(lib, name)(*args)
    return status, lib.osz_last_error().decode()


def cases(name):
    """label -> (the changed arguments, what the message says)."""
    lo, hi, bits, noun, has_win0, own = ENTRIES[name]
    win0 = WIN0 if has_win0 else 0
    found = {
        "null x": (dict(x=None), "null argument"),
        "null out": (dict(out=None), "null argument"),
        "winsize below": (dict(winsize=lo - 1, n=2), f"winsize={lo - 1} ({lo} .. "),
        "winsize above": (dict(winsize=hi + 1), f"winsize={hi + 1} ({lo} .. {hi})"),
        "step 0": (dict(step=0), "step=0 (>= 1)"),
        "mask 0": (dict(mask=0), f"{noun} mask 0"),
        "mask past the last bit": (dict(mask=1 << bits), f"{noun} mask {1 << bits}"),
        "nch 0": (dict(nch=0), "bad sizes (nch=0"),
        "negative n": (dict(n=-1, pitch=PITCH), "bad sizes"),
        "pitch < n": (dict(pitch=N - 1), f"bad sizes (nch={NCH} n={N} pitch={N - 1})"),
        "row_pitch too small": (dict(row_pitch=win0 - 1, plane_pitch=1 << 20), "the result's pitches"),
        "plane_pitch too small": (dict(plane_pitch=(NCH - 1) * ROW + win0 - 1), "the result's pitches"),
        "plane_pitch too small, one row": (dict(nch=1, plane_pitch=win0 - 1), "the result's pitches"),
        "x not aligned": (dict(x=X + 4), "8-byte aligned"),
        "out not aligned": (dict(out=OUT + 4), "8-byte aligned"),
    }
    if has_win0:
        found["negative win0"] = (dict(win0=-1), "bad sizes")
    return found


@pytest.mark.parametrize("name", list(ENTRIES))
def test_valid_arguments_without_a_window_are_accepted(lib, name):
    status, msg = call(lib, name)
    assert status == _lib.OSZ_OK, msg
    status, msg = call(lib, name, nch=1, plane_pitch=WIN0 if ENTRIES[name][4] else 0)
    assert status == _lib.OSZ_OK, msg


@pytest.mark.parametrize("name,label", [(name, label) for name in ENTRIES for label in cases(name)])
def test_a_bad_common_argument_is_refused(lib, name, label):
    change, says = cases(name)[label]
    status, msg = call(lib, name, **change)
    assert status == _lib.OSZ_ERR_INVALID, (status, msg)
    assert msg.startswith(name + ": ") and says in msg, msg
