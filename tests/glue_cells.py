"""The corpus and the references of the producer-level arithmetic (csrc/glue.hip: osz_moments_*,
osz_col_moments, the sixteen osz_ew instances, osz_complex_join, osz_magphase, osz_simpson; csrc/misc.hip:
osz_take), shared by tests/test_glue_cells_host.py and tests/test_gpu_glue_cells.py.  NumPy only.

* Restated planners: the launch arithmetic of glue.hip / misc.hip in Python, so that the host test can
  show that the corpus lengths sit on every edge of it.
* Long-double (x87, 64-bit mantissa) references for what is toleranced: the streaming moments with the
  reference's own chunk-length weighting, the two-pass column moments, Simpson's rule as simpson_kernel
  states it, hypot and the phase.
* Exact references for what is one correctly rounded IEEE operation or a copy (the four ew ops -- (x - a) / b
  is two operations with nothing to fuse --, complex_join, take): float64 NumPy, compared bit for bit
  by same_bits.
* The bounds of the GPU test, here so that the host test measures its mutants against the same figures.
"""

import functools
import warnings

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 80-bit format here"

# ------------------------------------------------------------------ the launch arithmetic, restated
MOM_COLS, MOM_MAXBLK = 8192, 64          # osz_moments_push: columns per block before the cap, kMomMaxBlk
ROW_COLS, ROW_MAXBLK = 256 * 8, 256      # row_grid: 256 threads x ~8 elements, at most 256 blocks
TAKE_COLS, TAKE_MAXBLK = 256, 2048       # osz_take
SYNTH_COLS, SYNTH_MAXBLK = 256, 1024     # osz_synth_normal
CHAN_BLK = 256                           # moments_fold / moments_finish / col_moments: one thread per row / column


def _ceil(a, b):
    return -(-a // b)


def moments_partition(n):
    """(nblk, span) of osz_moments_push: block b sums the columns [b * span, (b + 1) * span) of a row."""
    nblk = min(_ceil(n, MOM_COLS), MOM_MAXBLK)
    return nblk, _ceil(n, nblk)


def row_blocks(n):
    """gridDim.x of row_grid (ew, complex_join, magphase)."""
    return max(1, min(_ceil(n, ROW_COLS), ROW_MAXBLK))


def row_trips(n):
    """The most trips a thread of row_grid's grid-stride loop makes."""
    return _ceil(n, row_blocks(n) * 256)


def take_blocks(n):
    return min(_ceil(n, TAKE_COLS), TAKE_MAXBLK)


def synth_blocks(n):
    return min(_ceil(n, SYNTH_COLS), SYNTH_MAXBLK)


# ------------------------------------------------------------------ the corpus lengths
N_ROW = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
N_CAP = 524288 + 2048 + 1                # past the 256-block cap of row_grid; two rows only
N_FULL = ROW_COLS * ROW_MAXBLK           # the last length the capped grid covers in eight trips
N_MOM = (1, 255, 256, 257, 8191, 8192, 8193, 16385, 524288, 524289)
M_SIMPSON = (1, 2, 3, 4, 5, 6, 255, 256, 257, 258, 259, 511, 512, 513, 514, 2049, 2050)
NIDX = (1, 255, 256, 257, 524289)
NIDX_FULL = TAKE_COLS * TAKE_MAXBLK      # the last count the capped grid covers in one trip
ROWS = (1, 3, 257)                       # 257 only with n <= 257
N_SYNTH = SYNTH_COLS * SYNTH_MAXBLK + 1 + 256
NRED, NCOLS = (1, 2, 3, 65), (1, 255, 256, 257, 1000)

TOL = 1e-12                              # this suite's figure for mean / std / simpson (tests/test_gpu_glue.py)
TOL_MAG, TOL_PHASE = 1e-14, 1e-13        # test_analytic_amplitude_phase_kernels
U = 2.0 ** -53


# ------------------------------------------------------------------ bit-for-bit comparison
def same_bits(got, want):
    """True where two float64 (or complex128) arrays agree bit for bit; any NaN equals any NaN, signed
    zeros must match."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.complex128:
        got, want = got.view(np.float64), want.view(np.float64)
    assert got.dtype == np.float64
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | both_nan))


# ------------------------------------------------------------------ exact references (float64 NumPy)
EW_ADD, EW_MUL, EW_DIV, EW_STANDARDIZE = range(4)
BCAST_SCALAR, BCAST_ROW, BCAST_COL, BCAST_FULL = range(4)
OP_NAME = ("add", "mul", "div", "standardize")
KIND_NAME = ("scalar", "row", "col", "full")


def ew_ref(op, x, a, b, kind):
    """y = x (op) a [, b]; a / b: one value, (rows,), (n,) or (rows, n) as `kind` says."""
    def shaped(v):
        v = np.asarray(v, dtype=np.float64)
        if kind == BCAST_SCALAR:
            return v.reshape(1, 1)
        if kind == BCAST_ROW:
            return v.reshape(-1, 1)
        if kind == BCAST_COL:
            return v.reshape(1, -1)
        return v
    with np.errstate(all="ignore"):
        if op == EW_ADD:
            return x + shaped(a)
        if op == EW_MUL:
            return x * shaped(a)
        if op == EW_DIV:
            return x / shaped(a)
        return (x - shaped(a)) / shaped(b)


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, 1e300, -1e300, 3.0, 1e-300])


def ew_data(rows, n, seed):
    """(x, a_full, b_full): seeded normals with SPECIALS strewn over x, a and b so that +-0, +-inf, NaN, a
    zero divisor, 0 / 0, inf - inf and inf / inf all occur (from n = 63 on; shorter rows hold what fits)."""
    rng = np.random.default_rng([seed, rows, n])
    x, a, b = (rng.standard_normal((rows, n)) for _ in range(3))
    k = len(SPECIALS)
    for j in range(min(n, k * k)):
        # column j pairs special j // k of x with special j % k of the operand
        x[j % rows, j] = SPECIALS[j // k]
        a[j % rows, j] = SPECIALS[j % k]
        b[j % rows, j] = SPECIALS[(j + 1) % k]
    if n >= 3:
        x[-1, -1], a[-1, -1], b[-1, -1] = np.inf, np.inf, 0.0          # inf - inf, then NaN / 0
        x[0, -2], a[0, -2], b[0, -2] = 0.0, 0.0, 0.0                   # 0 / 0
    return x, a, b


def operands(kind, a_full, b_full):
    """The operands of `kind` cut from the full ones: an ordinary scalar (from the last row, which column 0
    leaves alone when there are two rows or more), row vectors whose first entries are +0 and -0 (a row
    divided by zero), column vectors with every special value."""
    if kind == BCAST_SCALAR:
        return a_full[-1, :1].copy(), b_full[-1, :1].copy()
    if kind == BCAST_ROW:
        return a_full[:, 0].copy(), b_full[:, 0].copy()
    if kind == BCAST_COL:
        return a_full[0].copy(), b_full[0].copy()
    return a_full, b_full


def take_indices(form, nidx, n, seed=0):
    """int64 indices into a row of n columns, every one inside it."""
    rng = np.random.default_rng([seed, nidx, n])
    if form == "mask":               # np.flatnonzero of a mask: ascending, distinct
        assert nidx <= n
        return np.sort(rng.choice(n, nidx, replace=False)).astype(np.int64)
    if form == "repeated":
        return rng.integers(0, max(n // 7, 1), nidx).astype(np.int64)
    if form == "descending":
        assert nidx <= n
        return np.sort(rng.choice(n, nidx, replace=False))[::-1].astype(np.int64)
    if form == "ends":
        return np.where(np.arange(nidx) % 2 == 0, 0, n - 1).astype(np.int64)
    assert form == "empty"
    return np.zeros(0, dtype=np.int64)


TAKE_FORMS = ("mask", "repeated", "descending", "ends", "empty")


# ------------------------------------------------------------------ streaming moments
ROW_KINDS = ("N(1,3)", "N(1000,1)", "N(1e5,1)", "1% NaN", "NaN chunk")
STREAM_TAIL = (1, 257, 0, 8193)          # the ragged pushes that follow the push of n
NAN_CHUNK = 2                            # the push (of 257) in which a "NaN chunk" row is all NaN


def moments_lens(n, stream):
    return (n,) + STREAM_TAIL if stream else (n,)


def moments_nrows(n):
    return 257 if n <= 257 else len(ROW_KINDS)


@functools.lru_cache(maxsize=None)
def moments_data(n, stream):
    """Rows of kind ROW_KINDS[r % 5] for the pushes moments_lens(n, stream), in one array (read-only)."""
    lens = moments_lens(n, stream)
    total, rows = sum(lens), moments_nrows(n)
    rng = np.random.default_rng([77, n, int(stream)])
    x = rng.standard_normal((rows, total))
    kind = np.arange(rows) % len(ROW_KINDS)
    x[kind == 0] = 1.0 + 3.0 * x[kind == 0]
    x[kind == 1] += 1000.0
    x[kind == 2] += 1e5
    x[kind == 3] = 1.0 + 3.0 * x[kind == 3]
    x[kind == 4] = 1.0 + 3.0 * x[kind == 4]
    holes = rng.random((rows, total)) < 0.01
    if total >= 2:
        holes[:, total // 2] = True
    holes[:, 0] = False                  # a push of one sample keeps it
    if stream:
        holes[:, n] = False
    x[(kind == 3)[:, None] & holes] = np.nan
    o = sum(lens[:NAN_CHUNK]) if stream else 0
    w = lens[NAN_CHUNK] if stream else n
    x[kind == 4, o:o + w] = np.nan
    x.setflags(write=False)
    return x


def chunks_of(x, lens):
    o, out = 0, []
    for n in lens:
        out.append(x[:, o:o + n])
        o += n
    assert o == x.shape[1]
    return out


def moments_ref(chunks, ignore_nan):
    """(mean, std, kappa) in long double, per row, of the chunks (rows, n_k) with the reference's weighting
    (core/protools.py mean / std): A = sum n_k (nan)mean(x_k), B = sum n_k (nan)mean(x_k^2), N = sum n_k with
    n_k the chunk LENGTH, not its count of finite samples; mean = A / N, std = sqrt(B / N - mean^2),
    kappa = (B / N) / (B / N - mean^2).  A row that is all NaN in one chunk gives NaN; a chunk of no
    samples adds nothing."""
    rows = chunks[0].shape[0]
    A, B, N = np.zeros(rows, LD), np.zeros(rows, LD), 0
    avg = np.nanmean if ignore_nan else np.mean
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        for x in chunks:
            n = x.shape[1]
            if n == 0:
                continue
            xl = x.astype(LD)
            A += n * avg(xl, axis=1)
            B += n * avg(xl * xl, axis=1)
            N += n
        mean = A / N
        var = B / N - mean * mean
        return mean, np.sqrt(var), (B / N) / var


def moments_f64(chunks, ignore_nan):
    """The same formula as the reference writes it, in float64 NumPy: (mean, std)."""
    rows = chunks[0].shape[0]
    A, B, N = np.zeros(rows), np.zeros(rows), 0
    avg = np.nanmean if ignore_nan else np.mean
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        for x in chunks:
            n = x.shape[1]
            if n == 0:
                continue
            A += n * avg(x, axis=1)
            B += n * avg(x ** 2, axis=1)
            N += n
        mean = A / N
        return mean, np.sqrt(B / N - mean ** 2)


def mean_abs(chunks):
    """mean |x| per row over the finite samples (0 where there are none): the scale of the mean's bound."""
    x = np.concatenate(chunks, axis=1)
    fin = np.isfinite(x)
    return np.where(fin, np.abs(x), 0.0).sum(1) / np.maximum(fin.sum(1), 1)


def moments_ratios(mean, sd, chunks, ignore_nan, ref=None):
    """(mean ratio, std ratio) per row: |got - ref| over the bound (TOL * mean|x|; TOL * kappa * ref).
    Where the reference is NaN the ratio is 0 if the result is NaN too and inf otherwise; where the
    reference variance is 0 (one sample) the std follows the constant-row rule: not (std > 1e-6 |c|)."""
    rm, rs, kappa = moments_ref(chunks, ignore_nan) if ref is None else ref
    scale = mean_abs(chunks)
    out = []
    with np.errstate(all="ignore"):
        for got, want, bound in ((mean, rm, TOL * scale), (sd, rs, TOL * kappa * rs)):
            got = np.asarray(got, dtype=np.float64)
            r = (np.abs(got.astype(LD) - want) / bound).astype(np.float64)
            both = np.isnan(got) & np.isnan(want)
            r = np.where(both, 0.0, np.where(np.isnan(r), np.inf, r))
            out.append(r)
        flat = (rs == 0) & ~np.isnan(rm)
        out[1] = np.where(flat, np.where(sd > 1e-6 * np.abs(rm.astype(np.float64)), np.inf, 0.0), out[1])
    return out[0], out[1]


CONSTANTS = (0.1, 7.7, 123.456, 0.0)


# ------------------------------------------------------------------ column moments
@functools.lru_cache(maxsize=None)
def col_data(nred, ncols):
    """(nred, ncols) normals of mixed scale; column 1 (if any) all NaN, a NaN in column ncols - 1 of row 0
    when nred > 1 (read-only)."""
    rng = np.random.default_rng([78, nred, ncols])
    x = rng.standard_normal((nred, ncols)) * rng.choice([1.0, 3.0, 1e3], ncols) + rng.choice([0.0, 1.0, 1e3], ncols)
    if ncols > 1:
        x[:, 1] = np.nan
    if nred > 1 and ncols > 2:
        x[0, ncols - 1] = np.nan
    x.setflags(write=False)
    return x


def col_moments_ref(x, ignore_nan):
    """Two-pass (nan)mean and (nan)std along axis 0 in long double."""
    xl = x.astype(LD)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        if ignore_nan:
            m = np.nanmean(xl, axis=0)
            return m, np.sqrt(np.nanmean((xl - m) ** 2, axis=0))
        m = np.mean(xl, axis=0)
        return m, np.sqrt(np.mean((xl - m) ** 2, axis=0))


def col_ratios(mean, sd, x, ignore_nan, ref=None):
    """(mean ratio, std ratio) per column; bounds TOL * mean|x| and TOL * sd + 4 U max|x| (the second term:
    the rounding of v - m, which the two-pass form cannot avoid)."""
    rm, rs = col_moments_ref(x, ignore_nan) if ref is None else ref
    fin = np.isfinite(x)
    ax = np.where(fin, np.abs(x), 0.0)
    scale = ax.sum(0) / np.maximum(fin.sum(0), 1)
    out = []
    with np.errstate(all="ignore"):
        for got, want, bound in ((mean, rm, TOL * scale), (sd, rs, TOL * rs + 4 * U * ax.max(0))):
            got = np.asarray(got, dtype=np.float64)
            r = (np.abs(got.astype(LD) - want) / bound).astype(np.float64)
            r = np.where((got.astype(LD) == want), 0.0, r)          # 0 / 0 where the bound itself is 0
            both = np.isnan(got) & np.isnan(want)
            out.append(np.where(both, 0.0, np.where(np.isnan(r), np.inf, r)))
    return out[0], out[1]


# ------------------------------------------------------------------ Simpson
SIMPSON_A, SIMPSON_DX, SIMPSON_ROWS = (0, 3), (1.0, 0.37), (1, 5)


@functools.lru_cache(maxsize=None)
def simpson_data():
    rng = np.random.default_rng(79)
    p = 0.5 + rng.standard_normal((max(SIMPSON_ROWS), max(SIMPSON_A) + max(M_SIMPSON)))
    p.setflags(write=False)
    return p


def simpson_ref(p, dx, swap=False, correct=True):
    """simpson_kernel's statement in long double over the last axis of p (rows, m): m = 1 gives 0, m = 2
    the trapezoid, else the composite rule on the odd count and, for an even count, the integral of the
    parabola through the last three points over the last interval (SciPy >= 1.11).  swap / correct:
    the mutants of the host test (odd and even weights swapped, the correction left out)."""
    p = np.asarray(p).astype(LD)
    m, dx = p.shape[-1], LD(dx)
    if m == 1:
        return np.zeros(p.shape[0], LD)
    if m == 2:
        return dx * (p[:, 0] + p[:, 1]) / 2
    mo = m if m & 1 else m - 1
    odd, even = p[:, 1:mo - 1:2].sum(1), p[:, 2:mo - 1:2].sum(1)
    if swap:
        odd, even = even, odd
    r = dx / 3 * (p[:, 0] + p[:, mo - 1] + 4 * odd + 2 * even)
    if not m & 1 and correct:
        r = r + dx * (5 * p[:, m - 1] + 8 * p[:, m - 2] - p[:, m - 3]) / 12
    return r


def simpson_bound(p, dx):
    return TOL * dx * np.abs(p).sum(-1)


# ------------------------------------------------------------------ magnitude and phase
def _pi_ld():
    return np.arctan2(LD(0), LD(-1))


def magphase_ref(z):
    """(hypot, atan2 mapped by "add 2 pi if negative") in long double."""
    re, im = z.real.astype(LD), z.imag.astype(LD)
    ph = np.arctan2(im, re)
    return np.hypot(re, im), np.where(ph < 0, ph + 2 * _pi_ld(), ph)


def magphase_numpy(z):
    """What float64 NumPy gives: np.abs, and np.angle followed by + 2 pi where negative."""
    with np.errstate(all="ignore"):
        ang = np.angle(z)
        return np.abs(z), np.where(ang < 0, ang + 2 * np.pi, ang)


SPECIAL_Z = np.array([complex(0.0, 0.0), complex(1.0, 0.0), complex(1.0, -0.0), complex(-1.0, 0.0),
                      complex(-1.0, -0.0), complex(0.0, 1.0), complex(0.0, -1.0), complex(1.0, -1e-20),
                      complex(1e300, 1e300), complex(5e-324, 0.0), complex(np.inf, np.nan),
                      complex(np.nan, 1.0), complex(np.inf, -np.inf)])


def magphase_data(rows, n, seed=80):
    rng = np.random.default_rng([seed, rows, n])
    return (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))) * \
        10.0 ** rng.integers(-3, 4, (rows, n))
