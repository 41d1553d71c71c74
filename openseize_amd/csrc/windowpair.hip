// windowpair.hip -- K19 per-window channel-pair matrices: for every window of W samples, `step`
// apart, the (C, C) covariance / correlation of real rows, or the amplitude-envelope correlation
// and the time-domain plv / ciplv of analytic (complex) rows.  The pair sums are bilinear: per
// window they are the Gram product G = R R^T of a row matrix R with time as the inner dimension,
// and they run on the float64 matrix pipe (v_mfma_f64_16x16x4_f64):
//   cov, corr    R = the C rows x - p, p the window's first sample of the row (the pivot);
//   aec          R = the C rows a - p of the envelope a = |z|;
//   plv, ciplv   R = the 2 C rows [u_x; u_y] of the unit phasor u = z / a, no pivot:
//                Re s_ij = G[i, j] + G[C + i, C + j],  Im s_ij = G[i, C + j] - G[j, C + i].
// Three steps: (1) window_stage_kernel writes a, u_x, u_y once per sample of a push (complex data
// only) and window_sums_kernel the per (row, window) sum of x - p (and of |u|^2, the flag of a
// zero-amplitude sample); (2) window_gram_kernel writes the block-upper triangle of G per window
// and sub-block of OSZ_WC_BLOCK samples; (3) window_finish_kernel folds the sub-blocks in order,
// applies the definitions and writes both mirrors.  DESIGN.md section 4, K19.
//
// Every sum has an order that is a function of W alone and nothing is atomic: an element of G is
// the MFMA's k-ordered chain over its own two rows, one chain per sub-block counted from the
// window's start; a row's sum is lane-strided and folded by wave_sum63.
#include "pair_window.h"

namespace osz {

constexpr int kWpBlock = OSZ_WC_BLOCK;        // samples per sub-block of a window
constexpr int kWpTile = kPwTile;              // rows per side of an MFMA tile
constexpr int kWpSide = 64;                   // rows per side of a workgroup's block of pairs
constexpr int kWpThreads = 256;               // 2 x 2 waves, each 2 x 2 tiles
constexpr int kWpPitch = kWave + 2;           // doubles per staged row: rows r and r + 1 are 2 (mod 32) apart,
                                              // so the 16 rows x 2 k of a half-wave's operand read cover 32
                                              // distinct 8-byte bank pairs
constexpr int kWpLoads = 2 * kWpSide * kWave / kWpThreads;   // 32 staged values per thread and step

static_assert(kWpBlock % kWave == 0, "a sub-block is a whole number of 64-sample steps");

__host__ __device__ inline bool wp_complex_mask(int mask) { return (mask & ~((1 << OSZ_WC_COV) | (1 << OSZ_WC_CORR))) != 0; }
__host__ __device__ inline bool wp_lock(int mask) { return (mask & ((1 << OSZ_WC_PLV) | (1 << OSZ_WC_CIPLV))) != 0; }

// a = |z|, u = z / a, once per sample: stage[0] = a, stage[1] = u_x, stage[2] = u_y, each (nch, n).
// A zero sample gives u = 0 / 0 = NaN.  One thread per sample.
__global__ void __launch_bounds__(256)
window_stage_kernel(const cx *__restrict__ z, int64_t ld, int nch, int64_t n, double *__restrict__ stage) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (t >= n) return;
    const cx v = z[(int64_t)c * ld + t];
    const double a = hypot(v.x, v.y);
    const int64_t plane = (int64_t)nch * n, at = (int64_t)c * n + t;
    stage[at] = a;
    stage[plane + at] = v.x / a;
    stage[2 * plane + at] = v.y / a;
}

// window_sums<2> (pair_window.h): the sums of x - p and of |u|^2 per (row, window)
__global__ void __launch_bounds__(kWave)
window_sums_kernel(const double *__restrict__ x, int64_t ld, int nch, int64_t W, int64_t step,
                   const double *__restrict__ ux, const double *__restrict__ uy, double *__restrict__ chan) {
    window_sums<2>(x, ld, nch, W, step, ux, uy, chan);
}

// G = R R^T of one sub-block of one window over one 64 x 64 block of row pairs (block row bi <=
// block column bj).  Per 64-sample step the workgroup stages the 64 + 64 rows (64 on the diagonal)
// in LDS, pivot subtracted and the samples past the sub-block's end zeroed: thread (wave w, lane
// l) fetches sample l of the slots 4 k + w, 512 B per row, one step ahead of the arithmetic.  Wave
// (wi, wj) keeps the 2 x 2 tiles of rows wi 32 .. + 31 against wj 32 .. + 31: per k-step of 4
// samples it reads two A and two B operands (one double per lane: row l & 15, sample l >> 4) and
// issues up to four MFMAs on four independent accumulators.  A tile below the diagonal or past
// the last row is neither computed nor written.
// Grid: x = triangular block index, y = window of the batch, z = sub-block.
template <bool PIVOT>
__global__ void __launch_bounds__(kWpThreads)
window_gram_kernel(const double *__restrict__ rows, int64_t ld, int nrows, int64_t W, int64_t step, int64_t win0,
                   int nblk, double *__restrict__ part) {
    __shared__ double tile[2 * kWpSide][kWpPitch];           // 67.6 KB: two workgroups per CU
    int bi, bj;
    pair_triangle(blockIdx.x, nblk, &bi, &bj);
    const bool diag = bi == bj;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int wi = w >> 1, wj = w & 1;
    const int64_t off = (int64_t)blockIdx.z * kWpBlock;      // < W by the grid
    const int64_t left = W - off;
    const int here = left < kWpBlock ? (int)left : kWpBlock;
    const int nsteps = (here + kWave - 1) / kWave;
    const int64_t first = ((int64_t)blockIdx.y + win0) * step;   // the window's first sample
    const int nslots = diag ? kWpSide : 2 * kWpSide;

    // slot e = 4 k + w of the staged rows: slots 0 .. 63 block row bi's, 64 .. 127 bj's.  The
    // slots' pivots wait in LDS and are subtracted on the way into the tile.  (The 32 row offsets
    // stay in vector registers: as scalars they spill.)
    __shared__ double pivot[2 * kWpSide];
    if (PIVOT && (int)threadIdx.x < nslots) {
        const int e = threadIdx.x, r = (e < kWpSide ? bi : bj) * kWpSide + (e & (kWpSide - 1));
        pivot[e] = r < nrows ? rows[(int64_t)r * ld + first] : 0.0;
    }
    // (a slot past the last row reads the last row instead: an element of G is formed from its
    // own two rows alone, and the elements of such a slot are not written)
    const double *mine = rows + first + off + lane;
    double g[kWpLoads];
#define WP_ROW(k) (mine + (int64_t)min(((k) < kWpLoads / 2 ? bi : bj) * kWpSide + ((4 * (k) + w) & (kWpSide - 1)), nrows - 1) * ld)
    bool act[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i0 = bi * kWpSide + wi * 32 + a * kWpTile, j0 = bj * kWpSide + wj * 32 + b * kWpTile;
            act[a][b] = i0 < nrows && j0 < nrows && i0 <= j0;
        }
    pair_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = pair_d4{0.0, 0.0, 0.0, 0.0};

    const int ra = wi * 32 + (lane & 15), rb = (diag ? 0 : kWpSide) + wj * 32 + (lane & 15), kq = lane >> 4;
#pragma unroll
    for (int k = 0; k < kWpLoads; ++k) g[k] = 4 * k + w < nslots && lane < here ? WP_ROW(k)[0] : 0.0;
    if (PIVOT) __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const bool inside = st * kWave + lane < here;        // past the end: +0.0 after the subtraction
#pragma unroll
        for (int k = 0; k < kWpLoads; ++k)
            if (4 * k + w < nslots) tile[4 * k + w][lane] = PIVOT ? (inside ? g[k] - pivot[4 * k + w] : 0.0) : g[k];
        __syncthreads();
        if (st + 1 < nsteps) {
            const int at = (st + 1) * kWave;
#pragma unroll
            for (int k = 0; k < kWpLoads; ++k) g[k] = 4 * k + w < nslots && at + lane < here ? WP_ROW(k)[at] : 0.0;
        }
        if (act[0][0] || act[0][1] || act[1][1]) {           // (act[1][0] implies act[0][0])
#pragma unroll
            for (int s = 0; s < kWave / 4; ++s) {
                const double a0 = tile[ra][4 * s + kq], a1 = tile[ra + kWpTile][4 * s + kq];
                const double b0 = tile[rb][4 * s + kq], b1 = tile[rb + kWpTile][4 * s + kq];
                if (act[0][0]) acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                if (act[0][1]) acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                if (act[1][0]) acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                if (act[1][1]) acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }

#undef WP_ROW

    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
    double *dst = part + ((int64_t)blockIdx.y * gridDim.z + blockIdx.z) * nrows * nrows;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (!act[a][b]) continue;
            const int j = bj * kWpSide + wj * 32 + b * kWpTile + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = bi * kWpSide + wi * 32 + a * kWpTile + kq + 4 * reg;
                if (i < nrows && j < nrows) dst[(int64_t)i * nrows + j] = acc[a][b][reg];
            }
        }
}

// the sub-blocks' partials of G[i, j] of one window, added in sub-block order
__device__ __forceinline__ double wp_fold(const double *__restrict__ g, int nsub, int64_t rr, int64_t at) {
    double t = g[at];
    for (int s = 1; s < nsub; ++s) t += g[s * rr + at];
    return t;
}

// One (i <= j, window) per thread: writes [i, j] and its mirror of every plane of `mask` that
// this Gram product serves (LOCK: plv and ciplv from the 2 C phasor rows; else cov and corr, or
// aec).  A channel whose own sums are not finite gives NaN, then come the fixed points of the
// diagonal, then the definitions.  Grid: x = pairs, y = window of the batch.
template <bool LOCK>
__global__ void __launch_bounds__(256)
window_finish_kernel(const double *__restrict__ part, int nsub, const double *__restrict__ chan, int nch, double cnt,
                     double div, int mask, double *__restrict__ out, int64_t out_plane, int64_t win0) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)nch * nch) return;
    const int i = (int)(k / nch), j = (int)(k % nch);
    if (i > j) return;
    const int64_t win = win0 + blockIdx.y;
    const int nrows = LOCK ? 2 * nch : nch;
    const int64_t rr = (int64_t)nrows * nrows;
    const double *g = part + (int64_t)blockIdx.y * nsub * rr;
    const double *ch = chan + win * 2 * nch;
    const double si = ch[i], sj = ch[j], fi = ch[nch + i], fj = ch[nch + j];
    double *o = out + win * nch * nch;
    const int64_t at = (int64_t)i * nch + j, mirror = (int64_t)j * nch + i;
    int plane = 0;
    if constexpr (LOCK) {
        const double re = wp_fold(g, nsub, rr, (int64_t)i * nrows + j) +
                          wp_fold(g, nsub, rr, (int64_t)(nch + i) * nrows + nch + j);
        const double im = wp_fold(g, nsub, rr, (int64_t)i * nrows + nch + j) -
                          wp_fold(g, nsub, rr, (int64_t)j * nrows + nch + i);
        const bool lost = !(__builtin_isfinite(si) && __builtin_isfinite(sj) && __builtin_isfinite(fi) &&
                            __builtin_isfinite(fj));
        plane = (mask & (1 << OSZ_WC_COV) ? 1 : 0) + (mask & (1 << OSZ_WC_CORR) ? 1 : 0) +
                (mask & (1 << OSZ_WC_AEC) ? 1 : 0);
        if (mask & (1 << OSZ_WC_PLV)) {
            double v = hypot(re, im) / cnt;
            if (lost) v = __builtin_nan("");
            else if (i == j) v = 1.0;
            o[plane * out_plane + at] = v;
            o[plane * out_plane + mirror] = v;
            ++plane;
        }
        if (mask & (1 << OSZ_WC_CIPLV)) {
            const double r = re / cnt, m = im / cnt;
            double v = __builtin_fabs(m) / sqrt(__builtin_fma(-r, r, 1.0));
            if (lost) v = __builtin_nan("");
            else if (i == j) v = 0.0;
            o[plane * out_plane + at] = v;
            o[plane * out_plane + mirror] = v;
        }
    } else {
        const double gij = wp_fold(g, nsub, rr, (int64_t)i * nrows + j);
        const double gii = wp_fold(g, nsub, rr, (int64_t)i * nrows + i);
        const double gjj = wp_fold(g, nsub, rr, (int64_t)j * nrows + j);
        const bool lost = !(__builtin_isfinite(si) && __builtin_isfinite(sj) && __builtin_isfinite(gii) &&
                            __builtin_isfinite(gjj) && __builtin_isfinite(fi) && __builtin_isfinite(fj));
        if (mask & (1 << OSZ_WC_COV)) {
            double v = __builtin_fma(cnt, gij, -(si * sj)) / (cnt * div);
            if (lost) v = __builtin_nan("");
            o[plane * out_plane + at] = v;
            o[plane * out_plane + mirror] = v;
            ++plane;
        }
        if (mask & (1 << OSZ_WC_CORR)) {
            double v = pearson(cnt, si, sj, gii, gjj, gij);
            v = v > 1.0 ? 1.0 : v < -1.0 ? -1.0 : v;         // (a NaN passes: a constant channel is 0 / 0)
            if (lost) v = __builtin_nan("");
            else if (i == j && v == v) v = 1.0;
            o[plane * out_plane + at] = v;
            o[plane * out_plane + mirror] = v;
            ++plane;
        }
        if (mask & (1 << OSZ_WC_AEC)) {
            double v = pearson(cnt, si, sj, gii, gjj, gij);
            if (lost) v = __builtin_nan("");
            else if (i == j) v = 1.0;
            o[plane * out_plane + at] = v;
            o[plane * out_plane + mirror] = v;
        }
    }
}

// The work space of one push: [stage: 3 nch n (complex)] [chan: 2 nch nwin] [G: batch nsub R R]
static bool wp_plan(const PwArgs &A, PwPlan *p) {
    const bool is_complex = A.value != 0;
    if (wp_complex_mask(A.mask) != is_complex || (is_complex && (A.mask & 3))) return false;
    p->nsub = (A.W + kWpBlock - 1) / kWpBlock;
    if (p->nsub > 65535) return false;
    if (!pw_plan(A, OSZ_WC_COUNT, 4, kAnyLength, 2, p->nsub * (wp_lock(A.mask) ? 4 : 1), p)) return false;
    p->stage = is_complex ? 3 * (int64_t)A.nch * A.n : 0;
    return true;
}

template <bool PIVOT>
static void wp_gram(const double *rows, int64_t ld, int nrows, int64_t W, int64_t step, int64_t win0, int64_t count,
                    int64_t nsub, double *part, hipStream_t st) {
    const int nblk = (nrows + kWpSide - 1) / kWpSide;
    hipLaunchKernelGGL(window_gram_kernel<PIVOT>, dim3((unsigned)(nblk * (nblk + 1) / 2), (unsigned)count, (unsigned)nsub),
                       dim3(kWpThreads), 0, st, rows, ld, nrows, W, step, win0, nblk, part);
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_pairs_work(int nch, int64_t n, int64_t winsize, int64_t step, int mask, int is_complex) {
    PwPlan p;
    return wp_plan({"osz_window_pairs", nch, n, winsize, step, mask, "complex", is_complex}, &p) ? p.work() : -1;
}

int osz_window_pairs(const void *x, int64_t pitch, int nch, int64_t n, int is_complex, int64_t winsize, int64_t step,
                     int ddof, int mask, double *out, int64_t plane_pitch, double *work, int64_t work_len,
                     void *stream) {
    const PwArgs A{"osz_window_pairs", nch, n, winsize, step, mask, "complex", is_complex, "ddof", ddof};
    PwPlan p;
    const int rc = pw_head(A, wp_plan(A, &p), p, {{x, is_complex ? 16u : 8u}, {out, 8}, {work, 8}}, pitch, true,
                           plane_pitch, work_len);
    if (rc != OSZ_OK) return rc;
    if (p.nwin == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    double *stage = work, *chan = work + p.stage, *part = chan + p.chan;
    const int64_t plane = (int64_t)nch * n, cc = (int64_t)nch * nch;
    const double *amp = is_complex ? stage : static_cast<const double *>(x);
    const int64_t ld = is_complex ? n : pitch;
    {
        KernelTimer timer("window_pair_prepare", st);
        if (is_complex)
            hipLaunchKernelGGL(window_stage_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)nch), dim3(256), 0, st,
                               static_cast<const cx *>(x), pitch, nch, n, stage);
        hipLaunchKernelGGL(window_sums_kernel, dim3((unsigned)p.nwin, (unsigned)nch), dim3(kWave), 0, st, amp, ld, nch,
                           winsize, step, is_complex ? stage + plane : nullptr, is_complex ? stage + 2 * plane : nullptr,
                           chan);
        OSZ_HIP(hipGetLastError());
    }
    const dim3 fgrid((unsigned)((cc + 255) / 256), 1);
    const double cnt = (double)winsize, div = (double)(winsize - ddof);
    const int pivoted = mask & ((1 << OSZ_WC_COV) | (1 << OSZ_WC_CORR) | (1 << OSZ_WC_AEC));
    return pw_batches(p, [&](int64_t w0, int64_t count) -> int {
        dim3 grid = fgrid;
        grid.y = (unsigned)count;
        if (pivoted) {
            {
                KernelTimer timer("window_gram", st);
                wp_gram<true>(amp, ld, nch, winsize, step, w0, count, p.nsub, part, st);
            }
            KernelTimer timer("window_pair_finish", st);
            hipLaunchKernelGGL(window_finish_kernel<false>, grid, dim3(256), 0, st, part, (int)p.nsub, chan, nch, cnt, div,
                               mask, out, plane_pitch, w0);
        }
        if (wp_lock(mask)) {
            {
                KernelTimer timer("window_gram", st);
                wp_gram<false>(stage + plane, n, 2 * nch, winsize, step, w0, count, p.nsub, part, st);
            }
            KernelTimer timer("window_pair_finish", st);
            hipLaunchKernelGGL(window_finish_kernel<true>, grid, dim3(256), 0, st, part, (int)p.nsub, chan, nch, cnt, div,
                               mask, out, plane_pitch, w0);
        }
        OSZ_HIP(hipGetLastError());
        return OSZ_OK;
    });
}

}  // extern "C"
