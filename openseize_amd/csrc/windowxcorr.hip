// windowxcorr.hip -- K23 lagged cross-correlation per window and channel pair: for every window of
// W samples, `step` apart, and every lag l of -L .. L the biased estimate
//   r_ij(l) = (1 / W) sum_t d_i[t] d_j[t + l],   d = the row minus its mean over the window,
// t over the samples for which both factors lie in the window, normalised or not, and from it the
// peak of |r| over the lags, the lag that attains it and the signed value there.  Per window the
// sums are K19's Gram product with one operand shifted in time, G(l) = D S_l D^T, and run on the
// float64 matrix pipe (v_mfma_f64_16x16x4_f64).  Three steps: (1) xcorr_sums_kernel writes per
// (row, window) the sum of x - p, p the window's first sample of the row (the mean is p + s / W);
// (2) xcorr_gram_kernel stages the centred rows in LDS, zeros outside the window, and writes the
// upper triangle of G(l) per window and lag; (3) xcorr_finish_kernel scales, normalises, clips,
// scans the lags with the tie rule and writes both mirrors.  DESIGN.md section 4, K23.
//
// Every sum has an order that is a function of (W, l) alone and nothing is atomic: an element of
// G(l) is the MFMA's k-ordered chain over t = 0 .. W - 1 in quads counted from the window's start
// (a factor outside the window is a staged +0.0), whichever lags share its workgroup; a row's sum
// is lane-strided and folded by wave_sum63.
#include "pair_window.h"

namespace osz {

constexpr int kWxTile = kPwTile;              // rows per side of an MFMA tile
constexpr int kWxSide = 32;                   // rows per side of a workgroup's block of pairs: 2 x 2 tiles
constexpr int kWxThreads = 256;               // 4 waves: each all 2 x 2 tiles of kWxLags lags
constexpr int kWxLags = 4;                    // lags per wave: 16 accumulator tiles, 128 registers
constexpr int kWxGroup = kWxLags * kWxThreads / kWave;   // lags per workgroup (grid z)
constexpr int kWxHalo = OSZ_WX_MAXLAG;        // samples the B rows are staged on either side of the step
constexpr int kWxPitchA = kWave + 2;          // doubles per staged row: 2 (mod 32), as K19's pitch, so that the
constexpr int kWxPitchB = kWave + 2 * kWxHalo + 2;   // 16 rows x 2 k of a half-wave's read cover 32 distinct
                                              // bank pairs; a lag shifts every lane alike and keeps that
constexpr int kWxFinish = 16;                 // pairs per side of a finishing workgroup's tile

static_assert(kWxPitchA % 32 == 2 && kWxPitchB % 32 == 2, "the staging pitches are 2 (mod 32) doubles");
static_assert(kWxSide % (kWxThreads / kWave) == 0, "the staged rows are dealt evenly to the waves");

// window_sums<1> (pair_window.h): the sum of x - p per (row, window), chan[w * nch + c]
__global__ void __launch_bounds__(kWave)
xcorr_sums_kernel(const double *__restrict__ x, int64_t ld, int nch, int64_t W, int64_t step,
                  double *__restrict__ chan) {
    window_sums<1>(x, ld, nch, W, step, nullptr, nullptr, chan);
}

// G(l) of one window over one 32 x 32 block of row pairs (block row bi <= block column bj) and
// one group of kWxGroup lags.  Per 64-sample step the workgroup stages in LDS the 32 A rows over
// the step and the 32 B rows over the step widened by kWxHalo samples on both sides, each value
// (x - p) - s / W or +0.0 outside the window: thread (wave w, lane l) fetches sample l of the rows
// 4 k + w.  Wave w keeps the 2 x 2 tiles of the lags m0 .. m0 + 3, m0 = 16 z + 4 w, lag l = m - L:
// per k-step of 4 samples it reads two A operands (one double per lane: row l & 15, sample l >> 4),
// and per lag two B operands l doubles further along, and issues up to four MFMAs a lag on
// independent accumulators.  A lag past L is neither computed nor written; a tile below the
// diagonal or past the last row is neither computed nor written, and of a tile on the diagonal the
// elements i <= j are written.
// Grid: x = triangular block index, y = window of the batch, z = group of lags.
__global__ void __launch_bounds__(kWxThreads)
xcorr_gram_kernel(const double *__restrict__ rows, int64_t ld, int nrows, int W, int64_t step, int64_t win0, int nblk,
                  int L, const double *__restrict__ chan, double *__restrict__ part) {
    __shared__ double ta[kWxSide][kWxPitchA];                // 16.5 KB
    __shared__ double tb[kWxSide][kWxPitchB];                // 48.5 KB: two workgroups per CU
    __shared__ double pivot[2 * kWxSide], mean[2 * kWxSide];
    int bi, bj;
    pair_triangle(blockIdx.x, nblk, &bi, &bj);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t win = (int64_t)blockIdx.y + win0;
    const int64_t first = win * step;                        // the window's first sample
    const int nl = 2 * L + 1;
    const int m0 = (int)blockIdx.z * kWxGroup + w * kWxLags; // the wave's first lag, counted from -L
    const int nq = nl - m0 < kWxLags ? nl - m0 : kWxLags;    // the wave's lags; <= 0: the wave rests
    const int nsteps = (W + kWave - 1) / kWave;

    // slots 0 .. 31 are block row bi's rows, 32 .. 63 bj's.  (A slot past the last row reads the
    // last row instead: an element of G is formed from its own two rows alone, and the elements
    // of such a slot are not written.)
    if ((int)threadIdx.x < 2 * kWxSide) {
        const int e = threadIdx.x;
        const int r = min((e < kWxSide ? bi : bj) * kWxSide + (e & (kWxSide - 1)), nrows - 1);
        pivot[e] = rows[(int64_t)r * ld + first];
        mean[e] = chan[win * nrows + r] / (double)W;
    }
    bool act[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i0 = bi * kWxSide + a * kWxTile, j0 = bj * kWxSide + b * kWxTile;
            act[a][b] = i0 < nrows && j0 < nrows && i0 <= j0;
        }
    pair_d4 acc[2][2][kWxLags];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < kWxLags; ++q) acc[a][b][q] = pair_d4{0.0, 0.0, 0.0, 0.0};
    int shift[kWxLags];                                      // where lag q's B operand starts in a staged row
#pragma unroll
    for (int q = 0; q < kWxLags; ++q) shift[q] = kWxHalo + min(m0 + q - L, L);

    const int rt = lane & 15, kq = lane >> 4;
    const double *mine = rows + first + lane;
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int t0 = st * kWave;
#pragma unroll
        for (int k = 0; k < kWxSide / 4; ++k) {
            const int e = 4 * k + w;
            const double *ra = mine + (int64_t)min(bi * kWxSide + e, nrows - 1) * ld;
            const double *rb = mine + (int64_t)min(bj * kWxSide + e, nrows - 1) * ld;
            ta[e][lane] = t0 + lane < W ? (ra[t0] - pivot[e]) - mean[e] : 0.0;
#pragma unroll
            for (int seg = 0; seg < 3; ++seg) {
                const int t = t0 + (seg - 1) * kWave;        // + lane: the sample of the window
                tb[e][seg * kWave + lane] =
                    t + lane >= 0 && t + lane < W ? (rb[t] - pivot[kWxSide + e]) - mean[kWxSide + e] : 0.0;
            }
        }
        __syncthreads();
        if (nq > 0 && (act[0][0] || act[0][1] || act[1][1])) {   // (act[1][0] implies act[0][0])
#pragma unroll 4
            for (int s = 0; s < kWave / 4; ++s) {
                const int c = 4 * s + kq;
                const double a0 = ta[rt][c], a1 = ta[rt + kWxTile][c];
#pragma unroll
                for (int q = 0; q < kWxLags; ++q) {
                    if (q >= nq) continue;
                    const double b0 = tb[rt][c + shift[q]], b1 = tb[rt + kWxTile][c + shift[q]];
                    if (act[0][0]) acc[0][0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0][q], 0, 0, 0);
                    if (act[0][1]) acc[0][1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1][q], 0, 0, 0);
                    if (act[1][0]) acc[1][0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0][q], 0, 0, 0);
                    if (act[1][1]) acc[1][1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1][q], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
    const int64_t rr = (int64_t)nrows * nrows;
    double *dst = part + (int64_t)blockIdx.y * nl * rr;
#pragma unroll
    for (int q = 0; q < kWxLags; ++q) {
        if (q >= nq) continue;
        double *plane = dst + (int64_t)(m0 + q) * rr;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (!act[a][b]) continue;
                const int j = bj * kWxSide + b * kWxTile + rt;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int i = bi * kWxSide + a * kWxTile + kq + 4 * reg;
                    if (i <= j && j < nrows) plane[(int64_t)i * nrows + j] = acc[a][b][q][reg];
                }
            }
    }
}

// One 16 x 16 tile of pairs (tile row bi <= tile column bj) and one window per workgroup, a thread
// per pair; the threads with i <= j compute.  v(l) = G_ij(l) / (sqrt G_ii(0) sqrt G_jj(0)) clipped
// to [-1, 1] (normalize) or G_ij(l) / W; a pair one of whose G_ii(0), G_jj(0) is not finite, or is
// 0 under normalize, is NaN in every measure.  i < j: v(l) goes to xcorr[L + l][i, j] and, through
// an LDS transpose that keeps the mirror's rows whole, to xcorr[L - l][j, i]; the lags are scanned
// in the order 0, +1, -1, +2, -2, ... and a candidate wins on a strictly larger |v| only, which is
// the tie rule; peak and signed go to both mirrors the same way, lag and 0 - lag.  i == j: the lags
// l >= 0 are written to both L + l and L - l, and lag 0, peak, lag and signed are the fixed points.
// Grid: x = triangular tile index, y = window of the batch.
__global__ void __launch_bounds__(kWxFinish * kWxFinish)
xcorr_finish_kernel(const double *__restrict__ part, int nch, int ntile, int L, double cnt, int normalize, int mask,
                    double *__restrict__ xc, double *__restrict__ out, int64_t out_plane, int64_t win0) {
    __shared__ double turn[kWxFinish][kWxFinish + 1];
    int bi, bj;
    pair_triangle(blockIdx.x, ntile, &bi, &bj);
    const int a = threadIdx.x / kWxFinish, b = threadIdx.x % kWxFinish;
    const int i = bi * kWxFinish + a, j = bj * kWxFinish + b;
    const bool mine = i < nch && j < nch && i <= j;          // this thread computes [i, j]
    // ... and writes the mirror [jm, im] of the pair that thread (b, a) computes
    const int jm = bj * kWxFinish + a, im = bi * kWxFinish + b;
    const bool mirrored = jm < nch && im < jm;
    const int64_t rr = (int64_t)nch * nch;
    const int64_t win = win0 + blockIdx.y;
    const int nl = 2 * L + 1;
    const double *g = part + (int64_t)blockIdx.y * nl * rr;
    const int64_t at = (int64_t)i * nch + j, mirror = (int64_t)jm * nch + im;
    const double nan = __builtin_nan("");
    double gii = 0.0, gjj = 0.0;
    if (mine) {
        gii = g[L * rr + (int64_t)i * nch + i];
        gjj = g[L * rr + (int64_t)j * nch + j];
    }
    const bool lost = !(__builtin_isfinite(gii) && __builtin_isfinite(gjj)) ||
                      (normalize && (gii == 0.0 || gjj == 0.0));
    const double den = normalize ? sqrt(gii) * sqrt(gjj) : cnt;
    const double d0 = lost ? nan : normalize ? 1.0 : gii / cnt;     // the diagonal's lag 0
    double *x = (mask & (1 << OSZ_WX_XCORR)) ? xc + win * nl * rr : nullptr;     // (the same for the whole grid)
    double best = -1.0, sgn = nan;
    int bl = 0;
    for (int n = 0; n < nl; ++n) {                           // l = 0, +1, -1, +2, -2, ...
        const int l = n & 1 ? (n + 1) >> 1 : -(n >> 1);
        double v = nan;
        if (mine && (i != j || l >= 0)) {
            v = g[(L + l) * rr + at] / den;
            if (normalize) v = v > 1.0 ? 1.0 : v < -1.0 ? -1.0 : v;
            if (lost) v = nan;
            if (i == j && l == 0) v = d0;
            if (x) {
                x[(L + l) * rr + at] = v;
                if (i == j) x[(L - l) * rr + at] = v;
            }
            const double av = __builtin_fabs(v);
            if (av > best) {
                best = av;
                bl = l;
                sgn = v;
            }
        }
        if (x) pw_mirror(turn, a, b, v, mirrored, x + (L - l) * rr + mirror);
    }
    double peak = lost ? nan : best, lag = lost ? nan : (double)bl;
    if (i == j) {
        peak = sgn = d0;
        lag = lost ? nan : 0.0;
    }
    double *o = out + win * rr;
    int plane = 0;
    const double vals[3] = {peak, lag, sgn};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (!(mask & (1 << (OSZ_WX_PEAK + m)))) continue;    // (the same for the whole grid)
        if (mine) o[plane * out_plane + at] = vals[m];
        pw_mirror(turn, a, b, m == 1 ? 0.0 - vals[m] : vals[m], mirrored, o + plane * out_plane + mirror);
        ++plane;
    }
}

int wx_window_sums(const double *x, int64_t pitch, int nch, int64_t W, int64_t step, int64_t w0, int64_t count,
                   double *chan, const char *timer, hipStream_t st) {
    OSZ_REQUIRE(w0 >= 0 && count >= 1 && count <= INT32_MAX && nch >= 1 && nch <= 16384, "wx_window_sums: bad sizes");
    KernelTimer t(timer, st);
    hipLaunchKernelGGL(xcorr_sums_kernel, dim3((unsigned)count, (unsigned)nch), dim3(kWave), 0, st, x + w0 * step, pitch,
                       nch, W, step, chan + w0 * nch);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int wx_lagged_gram(const double *x, int64_t pitch, int nch, int64_t W, int64_t step, int L, int64_t w0,
                   int64_t count, const double *chan, double *part, const char *timer, hipStream_t st) {
    OSZ_REQUIRE(count >= 1 && count <= 65535 && L >= 0 && L <= OSZ_WX_MAXLAG && L <= W / 2 && nch >= 1 &&
                    nch <= 16384 && W <= OSZ_WX_LONGEST,
                "wx_lagged_gram: bad sizes");
    const int nblk = (nch + kWxSide - 1) / kWxSide, ngroups = (2 * L + 1 + kWxGroup - 1) / kWxGroup;
    KernelTimer t(timer, st);
    hipLaunchKernelGGL(xcorr_gram_kernel, dim3((unsigned)(nblk * (nblk + 1) / 2), (unsigned)count, (unsigned)ngroups),
                       dim3(kWxThreads), 0, st, x, pitch, nch, (int)W, step, w0, nblk, L, chan, part);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

// The work space of one push: [chan: nch nwin] [G: batch (2 L + 1) nch nch]
static bool wx_plan(const PwArgs &A, PwPlan *p) {
    const int L = A.value;
    if (L < 0 || L > OSZ_WX_MAXLAG || L > A.W / 2) return false;
    return pw_plan(A, OSZ_WX_COUNT, 8, OSZ_WX_LONGEST, 1, 2 * L + 1, p);
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_xcorr_work(int nch, int64_t n, int64_t winsize, int64_t step, int maxlag, int mask) {
    PwPlan p;
    return wx_plan({"osz_window_xcorr", nch, n, winsize, step, mask, "maxlag", maxlag}, &p) ? p.work() : -1;
}

int osz_window_xcorr(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int maxlag,
                     int normalize, int mask, double *xcorr, double *out, int64_t plane_pitch, double *work,
                     int64_t work_len, void *stream) {
    const PwArgs A{"osz_window_xcorr", nch, n, winsize, step, mask, "maxlag", maxlag, "normalize", normalize};
    const bool full = mask & (1 << OSZ_WX_XCORR), matrices = mask & ~(1 << OSZ_WX_XCORR);
    PwPlan p;
    const int rc = pw_head(A, wx_plan(A, &p), p, {{x, 8}, {work, 8}, {xcorr, 8, true, full}, {out, 8, true, matrices}}, pitch,
                           matrices, plane_pitch, work_len);
    if (rc != OSZ_OK) return rc;
    if (p.nwin == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    double *chan = work, *part = work + p.chan;
    const int ntile = (nch + kWxFinish - 1) / kWxFinish;
    const int sums = wx_window_sums(x, pitch, nch, winsize, step, 0, p.nwin, chan, "window_xcorr_prepare", st);
    if (sums != OSZ_OK) return sums;
    return pw_batches(p, [&](int64_t w0, int64_t count) -> int {
        const int rc = wx_lagged_gram(x, pitch, nch, winsize, step, maxlag, w0, count, chan, part, "window_xcorr_gram", st);
        if (rc != OSZ_OK) return rc;
        KernelTimer timer("window_xcorr_finish", st);
        hipLaunchKernelGGL(xcorr_finish_kernel, dim3((unsigned)(ntile * (ntile + 1) / 2), (unsigned)count),
                           dim3(kWxFinish * kWxFinish), 0, st, part, nch, ntile, maxlag, (double)winsize, normalize, mask,
                           xcorr, out, plane_pitch, w0);
        OSZ_HIP(hipGetLastError());
        return OSZ_OK;
    });
}

}  // extern "C"
