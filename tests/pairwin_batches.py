"""The corpus, the planner and the comparison of the channel-pair window kernels' batch walk (K19
osz_window_pairs, K23 osz_window_xcorr, K24 osz_window_granger, K25 osz_window_mi), shared by
tests/test_pairwin_batches_host.py and tests/test_gpu_pairwin_batches.py.  NumPy only.

* ``plan``: pw_plan of csrc/pair_window.h with wp_plan, wx_plan, wg_plan and wm_plan restated, so that
  the host test can show that every case crosses the batch edges it is here for and that the work
  space the library asks for is the one the restatement derives.
* ``CASES``: all at step 1.  Three batches (a middle batch: full, w0 > 0, not the last) of each
  kernel; two batches of K19's real plan; C = 2 with nwin = batch + 3 at the 65535-window clamp of a
  grid's y, every measure asked; K25's own cap by the staging in front of its count matrix.
* ``stream``: seeded rows of the kind each kernel's own parity test uses.
* ``picks`` and ``references``: the windows a reference is computed for -- both ends, both sides of
  every batch edge, one window inside every batch -- and the host modules' restatements at them,
  each from the window's own samples alone.
* ``check``: what both tests assert of a result.  No bound is set here: every one is imported from
  the kernel's own host module, and the rest is bit for bit.
"""

from collections import namedtuple
from functools import lru_cache

import numpy as np

from test_analytic_host import mixture
from test_connectivity_host import COMPLEX, REAL, RTOL
from test_connectivity_host import caps as pairs_caps
from test_granger_host import NAMES as GRANGER
from test_granger_host import coupled, window_granger_measures
from test_mi_host import NAMES as MI
from test_mi_host import mixed, window_mi_measures
from test_xcorr_host import NAMES as XCORR
from test_xcorr_host import caps as xcorr_caps
from test_xcorr_host import peak_margin

# ------------------------------------------------------------------ the planner, restated
GRAM_CAP = 1 << 25           # kGramCap: doubles of G a batch may hold
GRID_Y = 65535               # a batch is a grid's y
WC_BLOCK = 1024              # kWpBlock = OSZ_WC_BLOCK: a sub-block of a K19 window
MI_EDGES, MI_META, MI_STEP = 16, 18, 64      # kMiEdges, kMiMeta, kMiStep of csrc/windowmi.hip

Plan = namedtuple("Plan", "nwin one batch batches work binds")


def _ceil(a, b):
    return -(-a // b)


def window_count(n, W, step):
    return 0 if n < W else (n - W) // step + 1


def plan(kernel, nch, n, W, step, param, names, cplx=False):
    """Plan(nwin, one, batch, batches, work, binds) of one call: ``one`` the doubles of G a window
    takes, ``batches`` the list of (w0, count), ``work`` the doubles osz_window_*_work asks for and
    ``binds`` the limit that set ``batch``: "gram" (kGramCap), "grid" (65535), "staging" (K25's own
    cap) or "nwin" (one batch holds every window)."""
    nwin = window_count(n, W, step)
    stage = 0
    if kernel == "pairs":
        nsub = _ceil(W, WC_BLOCK)
        per = nsub * (4 if ("plv" in names or "ciplv" in names) else 1)
        chan = 2 * nch * nwin
        stage = 3 * nch * n if cplx else 0
    elif kernel == "xcorr":
        per, chan = 2 * param + 1, nch * nwin
    elif kernel == "granger":
        per, chan = 2 * param + 1, 2 * nch * nwin
    else:
        bp = 1
        while bp < param:
            bp *= 2
        per, chan = bp * bp // 2, 0
    one = per * nch * nch
    raw = GRAM_CAP // one
    batch, binds = max(1, min(raw, GRID_Y)), "grid" if raw > GRID_Y else "gram"
    if kernel == "mi":
        wpad = _ceil(W, MI_STEP) * MI_STEP
        front = (MI_EDGES + MI_META + wpad // 8) * nch
        if GRAM_CAP // front < min(batch, nwin):
            binds = "staging"
        batch = max(1, min(batch, nwin, GRAM_CAP // front))
        chan = ((W + 2) & ~1) + batch * front
    if nwin <= batch:
        batch, binds = batch if kernel == "mi" else nwin, "nwin"
    batches = [(w0, min(batch, nwin - w0)) for w0 in range(0, nwin, max(batch, 1))]
    return Plan(nwin, one, batch, batches, stage + chan + batch * one, binds)


# ------------------------------------------------------------------ the corpus
# kernel: pairs / xcorr / granger / mi.  param: ddof, maxlag, order or bins.  flag: xcorr's normalize,
# mi's binning.  want: what the case is here for -- (batches, binds, batch).
Case = namedtuple("Case", "key kernel nch W param flag names cplx nwin want")


def _case(key, kernel, nch, W, param, flag, names, cplx, batch, nbatch, binds, last=None):
    nwin = (nbatch - 1) * batch + ((1 if nbatch == 3 else 3) if last is None else last)    # `last`: the last batch
    return Case(key, kernel, nch, W, param, flag, tuple(names), cplx, nwin, (nbatch, binds, batch))


CASES = [
    # three batches: matrices only (the xcorr and counts arrays would be 0.5 GB)
    _case("three-xcorr", "xcorr", 34, 128, 64, True, XCORR[1:], False, 225, 3, "gram"),
    _case("three-granger", "granger", 34, 128, 16, None, GRANGER, False, 879, 3, "gram"),
    _case("three-mi", "mi", 34, 65, 16, "quantile", MI[1:], False, 226, 3, "gram"),
    _case("three-pairs-complex", "pairs", 18, 8193, 1, None, COMPLEX, True, 2876, 3, "gram"),
    # two batches of K19's real plan: another gram_per than the complex one
    _case("two-pairs-real-ddof0", "pairs", 18, 8193, 0, None, REAL, False, 11507, 2, "gram", 2),
    _case("two-pairs-real-ddof1", "pairs", 18, 8193, 1, None, REAL, False, 11507, 2, "gram", 2),
    # the grid clamp: C = 2, every measure
    _case("clamp-pairs-real", "pairs", 2, 4, 1, None, REAL, False, 65535, 2, "grid"),
    _case("clamp-pairs-complex", "pairs", 2, 4, 1, None, COMPLEX, True, 65535, 2, "grid"),
    _case("clamp-xcorr", "xcorr", 2, 8, 4, False, XCORR, False, 65535, 2, "grid"),
    _case("gram-xcorr-two-channels", "xcorr", 2, 128, 64, True, XCORR, False, 65027, 2, "gram"),
    _case("clamp-granger", "granger", 2, 16, 2, None, GRANGER, False, 65535, 2, "grid"),
    _case("clamp-mi-uniform", "mi", 2, 16, 4, "uniform", MI, False, 65535, 2, "grid"),
    _case("clamp-mi-quantile", "mi", 2, 16, 4, "quantile", MI, False, 65535, 2, "grid"),
    # K25's own cap: the staging in front of the count matrix
    _case("staging-mi", "mi", 2, 4096, 2, "quantile", MI, False, 30727, 2, "staging"),
]
BY_KEY = {c.key: c for c in CASES}
THREE = [c for c in CASES if c.want[0] == 3]
DIRECT = [c for c in CASES if c.nch == 2 and c.want[1] != "staging"]
STEP = 1


def samples(case, nwin=None):
    return ((case.nwin if nwin is None else nwin) - 1) * STEP + case.W


def plan_of(case, nwin=None):
    return plan(case.kernel, case.nch, samples(case, nwin), case.W, STEP, case.param, case.names, case.cplx)


@lru_cache(maxsize=None)
def _rows(kernel, cplx, nch, n, W):
    if kernel in ("xcorr", "granger"):
        return coupled(nch, n)                               # x[1:] += 0.7 roll(x[:-1], 3)
    if kernel == "mi":
        return mixed(nch, n)
    if not cplx:                                             # the real rows of test_gpu_connectivity.py
        x = np.random.default_rng(19).standard_normal((nch, n))
        x[1] = x[0] + 0.5 * x[1]
        return x
    if W >= 64:                                              # ... and its analytic rows
        return np.array(mixture(nch, n))
    rng = np.random.default_rng(23)
    return rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))


def stream(case):
    """The (C, n) rows of a case, of the kind its kernel's parity test uses.  Read-only."""
    x = _rows(case.kernel, case.cplx, case.nch, samples(case), case.W)
    x.setflags(write=False)
    return x


def batch_columns(case, w0, count):
    """The columns of the stream that the ``count`` windows from w0 on hold."""
    return slice(w0 * STEP, (w0 + count - 1) * STEP + case.W)


def shapes(case, nwin):
    """name -> shape of a result of ``nwin`` windows."""
    cc = (case.nch, case.nch)
    lead = {"xcorr": (2 * case.param + 1,) if case.kernel == "xcorr" else (),
            "counts": (case.param, case.param) if case.kernel == "mi" else ()}
    return {name: (nwin,) + lead.get(name, ()) + cc for name in case.names}


# ------------------------------------------------------------------ the windows a reference is computed for
def picks(batches):
    """Window 0, the last window, both sides of every batch edge and one window inside every batch."""
    nwin = batches[-1][0] + batches[-1][1]
    found = {0, nwin - 1}
    for w0, count in batches:
        if w0:
            found |= {w0 - 1, w0}
        found.add(w0 + count // 2)
    return sorted(found)


def references(case, x, at, dtype=np.longdouble):
    """(want, cap) at the windows ``at``, each from the window's own samples alone: name -> (len(at),
    ...) arrays, the restatement of the kernel's host module and the caps of its GPU parity test (None
    for a name that is compared exactly).  ``dtype``: K24's restatement also runs in float64."""
    want, cap = {}, {}
    for w in at:
        xw = np.asarray(x)[:, w * STEP:w * STEP + case.W]
        W = case.W
        if case.kernel == "pairs":
            M, c = pairs_caps(xw, W, W, case.param)
        elif case.kernel == "xcorr":
            M, c1 = xcorr_caps(xw, W, W, case.param, case.flag)
            c = {"xcorr": c1[:, None], "peak": c1, "signed": c1, "lag": None}
        elif case.kernel == "granger":
            M = window_granger_measures(xw, W, W, case.param, dtype)
            c = {name: np.full(M[name].shape, RTOL) for name in M}
        else:
            M = window_mi_measures(xw, W, W, case.param, case.flag)
            c = {name: None if name == "counts" else np.full(M[name].shape, RTOL) for name in M}
        for name in case.names:
            want.setdefault(name, []).append(M[name][0])
            cap.setdefault(name, []).append(None if c[name] is None else np.broadcast_to(c[name], M[name].shape)[0])
    return ({k: np.stack(v) for k, v in want.items()},
            {k: None if v[0] is None else np.stack(v) for k, v in cap.items()})


def lag_margin(case, x, at):
    """The smallest lead, in caps, of the largest |v| over the runner-up at the windows ``at``: above
    2, no rounding within the caps moves a peak to another lag (tests/test_gpu_xcorr.py)."""
    least = np.inf
    for w in at:
        xw = np.asarray(x)[:, w * STEP:w * STEP + case.W]
        M, c = xcorr_caps(xw, case.W, case.W, case.param, case.flag)
        least = min(least, peak_margin(M, c, case.param))
    return least


# ------------------------------------------------------------------ the comparison
def _is_host(a):
    return isinstance(a, np.ndarray)


def _bits(a):
    """The int64 view of a float64 array or tensor with every NaN made the canonical one."""
    if _is_host(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return np.where(np.isnan(a), np.nan, a).view(np.int64)
    import torch
    return torch.where(a.isnan(), torch.full((), float("nan"), dtype=a.dtype, device=a.device), a).contiguous().view(torch.int64)


def same_bits(a, b):
    """Whether two float64 arrays (or two tensors) agree bit for bit, any NaN equal to any NaN."""
    if tuple(a.shape) != tuple(b.shape):
        return False
    a, b = _bits(a), _bits(b)
    if _is_host(a):
        return bool(np.array_equal(a, b))
    import torch
    return bool(torch.equal(a, b))


def _host(a, at):
    return np.asarray(a[at] if _is_host(a) else a[at].cpu().numpy())


def check(case, whole, parts, at, refs, say=None):
    """What both tests assert of ``whole``, name -> (nwin, ...) results of one call over every window.

    (a) ``whole`` has the bits of ``parts`` laid end to end: an iterable of (w0, name -> results), one
        call per batch over that batch's own samples.  Nothing is left out.
    (b) At the windows ``at``, ``whole`` agrees with ``refs`` = (want, cap) of ``references`` under the
        comparison of the kernel's own GPU parity test.
    (c) Every result that the restatement says is finite is finite.
    Returns name -> the largest error at the picks as a fraction of its cap (``counts`` and ``lag``:
    the number of entries that differ)."""
    nwin = None
    for name in case.names:
        nwin = whole[name].shape[0] if nwin is None else nwin
        assert whole[name].shape[0] == nwin, (case.key, name, tuple(whole[name].shape))
    done = 0
    for w0, part in parts:                                   # (a)
        assert w0 == done, (case.key, "the parts are not in order", w0, done)
        for name in case.names:
            count = part[name].shape[0]
            assert w0 + count <= nwin, (case.key, name, w0, count, nwin)
            assert same_bits(whole[name][w0:w0 + count], part[name]), \
                (case.key, name, f"windows {w0} .. {w0 + count - 1} differ from the call over their own samples")
        done += part[case.names[0]].shape[0]
    assert done == nwin, (case.key, "the parts hold", done, "windows of", nwin)

    want, cap = refs
    ratios = {}
    for name in case.names:                                  # (b) and (c)
        g, w, c = _host(whole[name], list(at)), want[name], cap[name]
        assert g.shape == w.shape and g.dtype == np.float64, (case.key, name, g.shape, w.shape)
        finite = np.isfinite(w)
        assert np.all(np.isfinite(g[finite])), \
            (case.key, name, "not finite at windows", sorted({at[k] for k in np.argwhere(finite & ~np.isfinite(g))[:, 0]}))
        if c is None:                                        # counts, lag: exactly equal
            wrong = int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w)))))
            ratios[name] = wrong
            assert wrong == 0, (case.key, name, wrong, "entries differ")
            continue
        assert np.all(np.isfinite(c)) and np.all(c > 0), (case.key, name, "a cap is not finite")
        assert np.array_equal(np.isnan(g), np.isnan(w)), (case.key, name, "NaN where the restatement has none")
        err = np.where(finite, np.abs(g - np.where(finite, w, 0.0)), 0.0)
        ratios[name] = float(np.max(err / c))
        worst = at[int(np.argmax((err / c).reshape(len(at), -1).max(axis=1)))]
        assert np.all(err <= c), (case.key, name, f"{ratios[name]:.3e} of the cap at window {worst}")
        if name == "signed":
            assert np.array_equal(np.sign(g), np.sign(w)), (case.key, name)
    if say:
        say(f"{case.key}: " + ", ".join(f"{k} {v:.2e}" if cap[k] is not None else f"{k} {v} differ"
                                        for k, v in ratios.items()) + " of the cap")
    return ratios
