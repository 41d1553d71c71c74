"""The 80-bit reference, the filters and the corpus of tests/sos_routes.py, checked without a GPU:
the reference against SciPy and against itself, every filter's stored w and e64 re-measured, and
the corpus against the list of reachable kernel instances."""

import os

import numpy as np
import pytest

import sos_routes as R


@pytest.fixture(scope="module")
def measured():
    """key -> (w in tiles or None, e64), measured here."""
    out = {}
    for key in R.FILTERS:
        wl = R.warmup_len(R.design(key))
        out[key] = (None if wl == R.NEVER else wl / R.TILE, R.measure_e64(key))
    return out


def test_longdouble_is_80_bit():
    assert np.finfo(np.longdouble).nmant == 63


@pytest.mark.parametrize("key", list(R.FILTERS))
def test_filter_table(key, measured):
    """nsec, w and e64 stored beside the filter are what the design, the restated sos_warmup_len
    and the float64 serial recurrence give; 16 e64 stays within the loosest bound the project holds."""
    f = R.FILTERS[key]
    w, e64 = measured[key]
    print(f"{key}: nsec {f.nsec} w {w} e64 {e64:.3g} (stored {f.e64:.3g}) bound {R.bound(key):.3g}")
    assert R.design(key).shape == (f.nsec, 6)
    assert w == f.w
    assert f.e64 / 2 <= e64 <= f.e64 * 2
    assert 16 * f.e64 <= 1e-8


@pytest.mark.parametrize("key", list(R.FILTERS))
def test_reference_matches_scipy(key):
    """Zero state and a carried one: SciPy's float64 sosfilt stays within 4 e64 of the reference,
    outputs and final state."""
    import scipy.signal as sps
    sos, f = R.design(key), R.FILTERS[key]
    x = R.signal(2, 600000, 65)
    y, zf, peak = R.run_ref(x, sos)
    ys, zs = sps.sosfilt(sos, x, axis=-1, zi=np.zeros((f.nsec, 2, 2)))
    assert R.rel_err(ys, y).max() <= 4 * f.e64
    assert (np.abs(zs - zf).max(-1) / peak).max() <= 4 * f.e64
    head, rest = x[:, :1234], x[:, 1234:]
    y0, z0 = R.forward_ref(head, sos)
    y1, z1 = R.forward_ref(rest, sos, z0)
    assert np.array_equal(np.concatenate([y0, y1], -1), y) and np.array_equal(z1, zf)


def test_reversed_stride_is_flip_filter_flip():
    sos = R.design("bp6")
    x = R.signal(3, 20001, 66)
    zi = (R.zi_unit(sos)[:, None, :] * x[:, -1].astype(R.LD)[None, :, None])
    yr, zr, pr = R.run_ref(x, sos, zi, rev=True)
    yf, zf, pf = R.run_ref(x[:, ::-1], sos, zi)
    assert np.array_equal(yr, yf[:, ::-1]) and np.array_equal(zr, zf) and np.array_equal(pr, pf)
    assert np.array_equal(R.backward_ref(x, None, sos, R.TILE), yr)


def test_shortcut_past_a_nan_state_changes_nothing():
    """The reference stops doing arithmetic once the first section's state is NaN; built without
    that shortcut it gives the same bits, both directions, NaN and Inf inputs."""
    sos = R.design("bp9")
    x = R.signal(3, 3000, 71)
    x[0, 100] = np.nan
    x[1, -1] = np.inf
    x[2, 1500] = -np.inf
    for rev in (False, True):
        zi = R.backward_start(x, None, sos, 0) if rev else None
        fast, plain = R.run_ref(x, sos, zi, rev=rev), R.run_ref(x, sos, zi, rev=rev, plain=True)
        for a, b in zip(fast, plain):
            assert np.array_equal(a, b, equal_nan=True)
            assert np.array_equal(np.isinf(a), np.isinf(b))
        y = fast[0]
        if not rev:
            assert np.isfinite(y[0, :100]).all() and np.isnan(y[0, 100:]).all()
            assert np.isfinite(y[1, :-1]).all() and not np.isfinite(y[1, -1])
        else:
            assert np.isfinite(y[0, 101:]).all() and np.isnan(y[0, :101]).all()
            assert not np.isfinite(y[1]).any()


def test_zi_unit_is_sosfilt_zi():
    import scipy.signal as sps
    for key in R.FILTERS:
        sos = R.design(key)
        ref = sps.sosfilt_zi(sos)
        assert np.abs(R.zi_unit(sos) - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_backward_ref_is_the_chunk_local_scheme():
    """With fb the pass starts from the state a backward run over fb[:warm_len] leaves; SciPy's
    sosfilt on the flipped chunks, as core/numerical.py runs it, agrees to float64."""
    import scipy.signal as sps
    sos = R.design("bp6")
    fa, fb = R.signal(2, 30000, 67), R.signal(2, 9000, 68)
    zi = sps.sosfilt_zi(sos)[:, None, :]
    _, z = sps.sosfilt(sos, fb[:, ::-1], axis=-1, zi=zi * fb[:, -1][None, :, None])
    want = sps.sosfilt(sos, fa[:, ::-1], axis=-1, zi=z)[0][:, ::-1]
    assert R.rel_err(want, R.backward_ref(fa, fb, sos, R.NEVER)).max() < 1e-12
    cut = R.backward_ref(fa, fb, sos, 5000)
    assert np.array_equal(cut, R.backward_ref(fa, fb[:, :5000], sos, R.NEVER))
    assert not np.array_equal(cut, R.backward_ref(fa, fb, sos, 100))


def test_segmented_ref():
    """One segment is the plain pass; with a converged pre-roll the segments reproduce it; with one
    forced too short on the narrow band-pass a seam costs about 1e-2 -- and a segment start or a
    pre-roll that is one sample off is told apart just as clearly."""
    for rev in (False, True):
        sos = R.design("bp6")
        x = R.signal(2, 40000, 69)
        zi = np.random.default_rng(1).standard_normal((6, 2, 2)).astype(R.LD)
        y, zf, _ = R.run_ref(x, sos, zi, rev=rev)
        y1, z1 = R.segmented_ref(x, sos, zi, 1, 40000, 0, rev=rev)
        assert np.array_equal(y1, y) and np.array_equal(z1, zf)
        y3, z3 = R.segmented_ref(x, sos, zi, 3, 15000, 8192, rev=rev)
        assert R.rel_err(y3, y).max() < 1e-15 and np.abs(z3 - zf).max() < 1e-15
        sos = R.design("narrow2")
        x = R.signal(1, 8 * R.TILE, 70)
        y = R.run_ref(x, sos, rev=rev)[0]
        ys = R.segmented_ref(x, sos, None, 2, 4 * R.TILE, R.TILE, rev=rev)[0]
        assert 1e-3 < R.rel_err(ys, y)[0] < 1
        for seglen, pre in ((4 * R.TILE + 1, R.TILE), (4 * R.TILE, R.TILE - 1)):
            off = R.segmented_ref(x, sos, None, 2, seglen, pre, rev=rev)[0]
            assert R.rel_err(off, ys)[0] > 1e-4


def test_corpus_reaches_every_instance():
    got = {R.instance(r) for c in R.CASES for r in c.expect}
    assert got == R.REACHABLE, got ^ R.REACHABLE
    kernels = {r["kernel"] for c in R.CASES for r in c.expect}
    assert not kernels & R.UNREACHED_KERNELS
    for c in R.CASES:
        assert 1 <= len(c.expect) <= 4 and all(tuple(r) == R.FIELDS for r in c.expect), c.name
        assert R.FILTERS[c.key].w is not None or all(r["nseg"] == 1 for r in c.expect), c.name


def test_unreached_cites_the_source():
    text = open(os.path.join(R.ROOT, "openseize_amd", "csrc", "sos.hip")).read()
    for what, why, line in R.UNREACHED:
        assert what and why and text.count(line) == 1, line


def test_kernel_names_match_the_binding():
    from openseize_amd import _lib
    assert _lib.SOS_LAUNCH_FIELDS == R.FIELDS
    assert {k for k, *_ in R.REACHABLE} | R.UNREACHED_KERNELS == set(_lib.SOS_KERNEL)
    header = open(os.path.join(R.ROOT, "include", "osz_hip.h")).read()
    for i, name in enumerate(_lib.SOS_KERNEL):
        tag = "OSZ_SOSK_" + ("KERNEL" if name == "sos_kernel" else name.replace("sos_", "").upper())
        assert f"{tag} = {i}," in header or f"{tag} = {i} " in header, tag
    assert f"#define OSZ_SOS_LAUNCH_FIELDS {len(R.FIELDS)}\n" in header
    assert f"#define OSZ_SOS_LAUNCH_RECORDS {_lib.SOS_LAUNCH_RECORDS}\n" in header
