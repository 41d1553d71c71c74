"""The corpus and the references of tests/glue_cells.py checked without a GPU: (1) the corpus lengths sit
on the edges of the restated launch arithmetic; (2) the long-double moments reference is the reference's
formula (float64 NumPy, and the recorded results of G12: chunks of 900, a NaN-bearing signal, which pin
the n_k weighting and the NaN rule); (3) the Simpson reference is scipy.integrate.simpson; (4) the bounds
of tests/test_gpu_glue_cells.py would catch a dropped sample, a dropped last column of a block, swapped
Simpson weights, a missing even-count correction and a chunk weighted by its finite count, each by at
least 100 x; (5) the float64 formula itself keeps the kappa-scaled bound of the std on the corpus rows.

Sensitivity is measured per row and the best row counts: a dropped sample moves the mean by
|x_j - mean| / n, which the rows N(1000, 1) and N(1e5, 1) -- there for the conditioning of the std, kappa
1e6 and 1e10 -- hide behind their offset at the long lengths; the N(1, 3) row shows it at every length."""

import numpy as np
import pytest

import glue_cells as gc

LD = gc.LD


# ------------------------------------------------------------------ (1) planner edges
def test_corpus_sits_on_the_moments_partition_edges():
    part = gc.moments_partition
    assert gc.MOM_COLS in gc.N_MOM and gc.MOM_COLS + 1 in gc.N_MOM
    assert part(gc.MOM_COLS) == (1, 8192) and part(gc.MOM_COLS + 1) == (2, 4097)      # a ragged last block
    assert part(16385) == (3, 5462) and 3 * 5462 > 16385 > 2 * 5462
    cap = gc.MOM_COLS * gc.MOM_MAXBLK
    assert cap in gc.N_MOM and cap + 1 in gc.N_MOM
    assert part(cap) == (64, 8192) and part(cap - 8192 + 1)[0] == 64 and part(cap - 8192)[0] == 63
    assert part(cap + 1) == (64, 8193)                      # the first span past 8192
    assert [n for n in gc.N_MOM if part(n)[1] > gc.MOM_COLS] == [cap + 1]
    # a block of 256 threads: one trip or two, and a last trip that not every thread takes
    assert {255, 256, 257} <= set(gc.N_MOM)
    # every block of every corpus length has columns to sum (no block divides 0 by 0)
    for n in gc.N_MOM + tuple(n + sum(gc.STREAM_TAIL) for n in gc.N_MOM) + gc.STREAM_TAIL:
        if n:
            nblk, span = part(n)
            assert (nblk - 1) * span < n <= nblk * span, (n, nblk, span)


def test_corpus_sits_on_the_row_grid_and_take_edges():
    assert {gc.ROW_COLS - 1, gc.ROW_COLS, gc.ROW_COLS + 1} <= set(gc.N_ROW)
    assert gc.row_blocks(gc.ROW_COLS) == 1 and gc.row_blocks(gc.ROW_COLS + 1) == 2
    assert {63, 64, 65, 255, 256, 257} <= set(gc.N_ROW)      # a wave, a block, and one past each
    assert gc.N_FULL == 524288 and gc.row_blocks(gc.N_FULL) == gc.ROW_MAXBLK and gc.row_trips(gc.N_FULL) == 8
    assert gc.row_blocks(gc.N_FULL - gc.ROW_COLS) == gc.ROW_MAXBLK - 1
    assert gc.N_CAP == 526337 and gc.row_blocks(gc.N_CAP) == gc.ROW_MAXBLK and gc.row_trips(gc.N_CAP) == 9
    assert -(-gc.N_CAP // gc.ROW_COLS) > gc.ROW_MAXBLK + 1
    assert {gc.TAKE_COLS - 1, gc.TAKE_COLS, gc.TAKE_COLS + 1} <= set(gc.NIDX)
    assert gc.take_blocks(gc.TAKE_COLS) == 1 and gc.take_blocks(gc.TAKE_COLS + 1) == 2
    assert gc.NIDX_FULL == 524288 and gc.take_blocks(gc.NIDX_FULL) == gc.TAKE_MAXBLK
    assert gc.take_blocks(gc.NIDX_FULL - gc.TAKE_COLS) == gc.TAKE_MAXBLK - 1
    assert gc.NIDX_FULL + 1 in gc.NIDX and gc.take_blocks(gc.NIDX_FULL + 1) == gc.TAKE_MAXBLK   # a second trip
    assert gc.synth_blocks(gc.N_SYNTH) == gc.SYNTH_MAXBLK and gc.N_SYNTH > gc.SYNTH_COLS * gc.SYNTH_MAXBLK + 256
    # rows and columns by blockIdx.x * 256 + threadIdx.x: a second block with one thread at work
    assert max(gc.ROWS) == gc.CHAN_BLK + 1 and gc.moments_nrows(257) == 257 and gc.moments_nrows(8191) == 5
    assert {255, 256, 257, 1000} <= set(gc.NCOLS)


def test_corpus_sits_on_the_simpson_edges():
    m = set(gc.M_SIMPSON)
    assert {1, 2, 3, 4} <= m                                 # the two special cases, the first odd and even count
    for edge in (256, 512):
        assert {edge - 1, edge, edge + 1, edge + 2} <= m
    # the interior points 1 .. mo - 2 (an odd number of them) go over 256 threads: 255 of them are one
    # trip in which the last thread idles, 257 a second trip of one thread; odd and even counts of each
    interior = {mm: (mm if mm & 1 else mm - 1) - 2 for mm in m if mm >= 3}
    assert interior[257] == interior[258] == 255 and interior[259] == 257
    assert interior[3] == interior[4] == 1 and interior[5] == interior[6] == 3
    assert {2049, 2050} <= m                                 # the rfft of 4096 points, whole and less one


# ------------------------------------------------------------------ (2) the moments reference
def test_moments_reference_is_the_formula_in_float64():
    for n in (257, 8193):
        for stream in (False, True):
            x = gc.moments_data(n, stream)[[0, 3]]           # N(1, 3) and the row with 1 % NaN: kappa about 1.1
            chunks = gc.chunks_of(x, gc.moments_lens(n, stream))
            for ignore in (True, False):
                m, s, kappa = gc.moments_ref(chunks, ignore)
                fm, fs = gc.moments_f64(chunks, ignore)
                assert np.allclose(m.astype(np.float64), fm, rtol=1e-12, atol=1e-12, equal_nan=True)
                assert np.allclose(s.astype(np.float64), fs, rtol=1e-12, atol=1e-12, equal_nan=True)
                assert np.isnan(fm[1]) == (not ignore) and not np.isnan(fm[0])
                assert np.all((kappa[~np.isnan(kappa)] > 1) & (kappa[~np.isnan(kappa)] < 1.3))


def test_moments_reference_against_the_recorded_results(golden):
    g = golden("g12_protools.npz")
    x = g["x"].reshape(3, -1)
    assert np.isnan(x).sum() == 1
    chunks = [x[:, o:o + 900] for o in range(0, x.shape[1], 900)]
    assert [c.shape[1] for c in chunks] == [900, 900, 900, 900, 401]
    for ignore in (True, False):
        m, s, _ = gc.moments_ref(chunks, ignore)
        assert np.allclose(m.astype(np.float64), g[f"mean_prod_{int(ignore)}"].ravel(), rtol=1e-12, atol=1e-12,
                           equal_nan=True)
        assert np.allclose(s.astype(np.float64), g[f"std_prod_{int(ignore)}"].ravel(), rtol=1e-12, atol=1e-12,
                           equal_nan=True)
    # the recorded results tell the weightings apart: by finite count the NaN-bearing row moves by far more
    m, _, _ = gc.moments_ref(chunks, True)
    assert abs(_by_finite_count(chunks)[0][1] - m[1]) > 1e3 * 1e-12 * abs(m[1])


def test_all_nan_chunk_and_empty_push():
    x = gc.moments_data(8193, True)
    chunks = gc.chunks_of(x, gc.moments_lens(8193, True))
    assert chunks[3].shape[1] == 0 and bool(np.isnan(chunks[gc.NAN_CHUNK][4]).all())
    for ignore in (True, False):
        m, s, _ = gc.moments_ref(chunks, ignore)
        assert np.isnan(m[4]) and np.isnan(s[4])
        assert np.isnan(m[3]) == (not ignore)
        assert not np.isnan(m[:3]).any() and not np.isnan(s[:3]).any()


# ------------------------------------------------------------------ (3) Simpson against SciPy
@pytest.mark.parametrize("dx", gc.SIMPSON_DX)
def test_simpson_reference_against_scipy(dx):
    from scipy.integrate import simpson
    p = gc.simpson_data()
    for m in gc.M_SIMPSON:
        for a in gc.SIMPSON_A:
            seg = p[:, a:a + m]
            ref = gc.simpson_ref(seg, dx).astype(np.float64)
            if m == 1:
                assert not ref.any()
                continue
            want = simpson(seg, dx=dx, axis=-1)
            assert np.all(np.abs(ref - want) <= 1e-13 * dx * np.abs(seg).sum(-1)), (m, a)


# ------------------------------------------------------------------ (4) sensitivity
def _by_finite_count(chunks):
    """The mutant that weights a chunk by its count of finite samples instead of its length."""
    x = np.concatenate(chunks, axis=1).astype(LD)
    with np.errstate(all="ignore"):
        m = np.nanmean(x, axis=1)
        return m, np.sqrt(np.nanmean(x * x, axis=1) - m * m)


def _factor(got, chunks, ignore, ref):
    rm, rs = gc.moments_ratios(got[0].astype(np.float64), got[1].astype(np.float64), chunks, ignore, ref=ref)
    return rm, rs


def test_moments_bound_catches_a_dropped_sample_and_a_dropped_block_column():
    worst = np.inf
    for n in gc.N_MOM:
        x = gc.moments_data(n, False)[:5]
        ref = gc.moments_ref([x], True)
        nblk, span = gc.moments_partition(n)
        for what, j in (("sample", n // 3), ("last column of block 0", span - 1)):
            y = x.copy()
            y[:, j] = np.nan                                  # left out of both sums and of the count
            mut = gc.moments_ref([y], True)
            rm, rs = _factor(mut, [x], True, ref)
            best = max(rm[0], rs[0])                          # the N(1, 3) row
            print(f"moments n {n} dropped {what} ({j}): bound missed by {best:.3g} (mean {rm[0]:.3g}, "
                  f"std {rs[0]:.3g}; N(1000,1) {max(rm[1], rs[1]):.3g}, N(1e5,1) {max(rm[2], rs[2]):.3g})")
            worst = min(worst, best)
    assert worst >= 100, worst


def test_moments_bound_catches_the_finite_count_weighting():
    worst = np.inf
    for n in gc.N_MOM:
        x = gc.moments_data(n, True)[:5]
        chunks = gc.chunks_of(x, gc.moments_lens(n, True))
        ref = gc.moments_ref(chunks, True)
        assert not np.isnan(ref[0][3])
        rm, rs = _factor(_by_finite_count(chunks), chunks, True, ref)
        print(f"moments n {n} stream weighted by finite count: mean bound missed by {rm[3]:.3g}, std {rs[3]:.3g}")
        assert rm[0] < 1e-3 and rs[0] < 1e-3                  # no NaN in the row, no difference
        worst = min(worst, max(rm[3], rs[3]))
    assert worst >= 100, worst


def test_col_moments_bound_catches_a_dropped_sample():
    worst = np.inf
    for nred in gc.NRED[1:]:
        for ncols in gc.NCOLS:
            x = gc.col_data(nred, ncols)
            ref = gc.col_moments_ref(x, True)
            y = x.copy()
            y[nred // 2, 0] = np.nan
            mut = gc.col_moments_ref(y, True)
            rm, rs = gc.col_ratios(mut[0].astype(np.float64), mut[1].astype(np.float64), x, True, ref=ref)
            print(f"col_moments {nred} x {ncols} dropped sample: bound missed by mean {rm[0]:.3g}, std {rs[0]:.3g}")
            assert np.all(rm[2:] < 1e-3) and np.all(rs[2:] < 1e-3)      # the other columns: rounding to float64 only
            worst = min(worst, max(rm[0], rs[0]))
    assert worst >= 100, worst


def test_simpson_bound_catches_swapped_weights_and_a_missing_correction():
    p = gc.simpson_data()
    worst = np.inf
    for dx in gc.SIMPSON_DX:
        for m in gc.M_SIMPSON:
            if m < 3:
                continue
            seg = p[:, :m]
            ref, bound = gc.simpson_ref(seg, dx), gc.simpson_bound(seg, dx)
            muts = {"swapped": gc.simpson_ref(seg, dx, swap=True)}
            if not m & 1:
                muts["uncorrected"] = gc.simpson_ref(seg, dx, correct=False)
            for name, mut in muts.items():
                f = float(np.min(np.abs(mut - ref) / bound))
                print(f"simpson m {m} dx {dx} {name}: bound missed by {f:.3g}")
                worst = min(worst, f)
    assert worst >= 100, worst


# ------------------------------------------------------------------ (5) conditioning
def test_float64_formula_keeps_the_kappa_bound():
    """std = sqrt(E[x^2] - E[x]^2) loses kappa = E[x^2] / var to cancellation: in float64 NumPy it stays
    under 1e-12 * kappa of the long-double value on the corpus rows (kappa about 1.1, 1e6 and 1e10), so
    the bound of the GPU test is one the reference itself keeps."""
    worst = [0.0, 0.0, 0.0]
    for n in gc.N_MOM[1:]:
        for stream in (False, True):
            x = gc.moments_data(n, stream)[:3]
            chunks = gc.chunks_of(x, gc.moments_lens(n, stream))
            rm, rs, kappa = gc.moments_ref(chunks, True)
            fm, fs = gc.moments_f64(chunks, True)
            ratio = (np.abs(fs.astype(LD) - rs) / (gc.TOL * kappa * rs)).astype(np.float64)
            mratio = (np.abs(fm.astype(LD) - rm) / (gc.TOL * gc.mean_abs(chunks))).astype(np.float64)
            print(f"float64 formula n {n} stream {int(stream)}: kappa " + " ".join(f"{k:.3g}" for k in kappa.astype(float))
                  + " std ratio " + " ".join(f"{r:.2e}" for r in ratio) + " mean ratio " + " ".join(f"{r:.2e}" for r in mratio))
            assert np.all(ratio < 1) and np.all(mratio < 1), (n, stream, ratio, mratio)
            worst = [max(w, r) for w, r in zip(worst, ratio)]
    assert 1.05 < float(kappa[0]) < 1.2 and 0.9e6 < float(kappa[1]) < 1.1e6 and 0.9e10 < float(kappa[2]) < 1.1e10
    print("worst std ratio per row", worst)


def test_float64_formula_on_constant_rows():
    """What the reference's own formula gives on a flat channel in float64 NumPy (printed: 5.6e-9, 8.4e-8,
    3.3e-6 and 0 here; NaN whenever rounding leaves E[x^2] below E[x]^2): it keeps the bound the GPU test
    asks of the kernel, not (std > 1e-6 |c|)."""
    for c in gc.CONSTANTS:
        x = np.full((1, 600001), c)
        _, s = gc.moments_f64([x], True)
        print(f"float64 formula on a constant row of {c}: std {s[0]!r}")
        assert not (s[0] > 1e-6 * abs(c))


# ------------------------------------------------------------------ the exact references' own comparison
def test_same_bits_tells_signed_zeros_and_accepts_any_nan():
    a = np.array([0.0, np.nan, 1.0])
    assert gc.same_bits(a, a.copy())
    assert not gc.same_bits(a, np.array([-0.0, np.nan, 1.0]))
    assert gc.same_bits(a, np.array([0.0, -np.nan, 1.0]))
    assert not gc.same_bits(a, np.array([0.0, np.nan, np.nextafter(1.0, 2)]))
    assert not gc.same_bits(a, a[:2])


def test_ew_data_holds_the_special_operations():
    x, a, b = gc.ew_data(3, 257, 1)
    with np.errstate(all="ignore"):
        q = x / a
        assert np.isnan(q[(x == 0) & (a == 0)]).all() and ((x == 0) & (a == 0)).any()
        assert (np.isinf(x) & np.isinf(a)).any() and (a == 0).any() and np.isnan(x).any() and np.isnan(a).any()
        assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        assert np.isnan((x - a)[np.isinf(x) & (x == a)]).all()
    for kind in range(4):
        a1, b1 = gc.operands(kind, a, b)
        for op in range(4):
            y = gc.ew_ref(op, x, a1, b1, kind)
            assert y.shape == x.shape
            assert np.isfinite(y).mean() > (0.6 if kind else 0.9)       # mostly ordinary numbers
    for form in gc.TAKE_FORMS:
        for nidx in gc.NIDX[:4]:
            idx = gc.take_indices(form, nidx, 300)
            assert idx.dtype == np.int64 and (form == "empty" or (idx.min() >= 0 and idx.max() < 300 and len(idx) == nidx))
