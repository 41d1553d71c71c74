// windowgranger.hip -- K24 pairwise Granger causality per window (Geweke's time-domain measures):
// for every window of W samples, `step` apart, and every ordered pair (i, j) of channels, with d the
// row minus its window mean, r_ab(l) = (1 / W) sum_t d_a[t] d_b[t + l] the biased estimate of K23 and
// z_t = (d_i[t], d_j[t])^T,
//   C(l) = E[z_t z_{t-l}^T] = [[r_ii(l), r_ij(-l)], [r_ij(l), r_jj(l)]],   C(-l) = C(l)^T,
// the full model z_t = sum_{k=1..p} A_k z_{t-k} + e_t solves C(l) = sum_k A_k C(l - k), l = 1 .. p, its
// error covariance is S = C(0) - sum_k A_k C(k)^T, and the restricted models are the scalar
// Yule-Walker models of d_i and d_j alone, of the same order, with errors E_i and E_j:
//   granger[i, j] = F_{i->j} = ln(E_j / S_jj),  instant = ln(S_ii S_jj / det S),
//   total = (granger[i, j] + granger[j, i]) + instant.
// Three steps: (1) K23's sums and lagged Gram kernels with L = p (wx_window_sums, wx_lagged_gram)
// write the upper triangle of G(l) = W r(l), l = -p .. p, per window of a batch; (2)
// granger_auto_kernel, a thread per (window, channel), runs Levinson's recursion on G_cc(0 .. p) / W
// and writes E_c; (3) granger_pair_kernel, a lane per pair i < j, runs the block Levinson recursion
// (Whittle 1963; Wiggins and Robinson 1965) with 2 x 2 blocks, the coefficient blocks in LDS, and
// writes both mirrors.  DESIGN.md section 4, K24.
//
// The order of every operation is a function of p alone and nothing is atomic.
#include "pair_window.h"

namespace osz {

constexpr int kWgTile = 8;                    // pairs per side of a pair workgroup's tile: 64 lanes, one wave
constexpr int kWgAuto = 256;                  // (window, channel) threads per workgroup of the auto kernel

struct m2 {                                   // [[a, b], [c, d]]
    double a, b, c, d;
};

// acc - x y
__device__ __forceinline__ m2 m2_less(m2 acc, m2 x, m2 y) {
    return m2{__builtin_fma(-x.b, y.c, __builtin_fma(-x.a, y.a, acc.a)),
              __builtin_fma(-x.b, y.d, __builtin_fma(-x.a, y.b, acc.b)),
              __builtin_fma(-x.d, y.c, __builtin_fma(-x.c, y.a, acc.c)),
              __builtin_fma(-x.d, y.d, __builtin_fma(-x.c, y.b, acc.d))};
}
__device__ __forceinline__ m2 m2_t(m2 x) { return m2{x.a, x.c, x.b, x.d}; }
__device__ __forceinline__ double m2_det(m2 x) { return __builtin_fma(x.a, x.d, -(x.b * x.c)); }
// x u^-1, the inverse by the adjugate: x adj(u) times 1 / det u
__device__ __forceinline__ m2 m2_over(m2 x, m2 u) {
    const double s = 1.0 / m2_det(u);
    return m2{__builtin_fma(x.a, u.d, -(x.b * u.c)) * s, __builtin_fma(x.b, u.a, -(x.a * u.b)) * s,
              __builtin_fma(x.c, u.d, -(x.d * u.c)) * s, __builtin_fma(x.d, u.a, -(x.c * u.b)) * s};
}
__device__ __forceinline__ bool wg_good(double v) { return __builtin_isfinite(v) && v > 0.0; }
// a measure as it is written: a finite value below 0, which only rounding produces, is +0.0
__device__ __forceinline__ double wg_floor(double v) { return v <= 0.0 ? 0.0 : v; }

// One thread per (window of the batch, channel): E_p of the scalar Yule-Walker model of order p from
// r_l = G_cc(l) / W, l = 0 .. p, by Levinson's recursion (K22's arithmetic): E_0 = r_0, k_m = -(r_m +
// sum_{j=1}^{m-1} a_j r_{m-j}) / E_{m-1}, j ascending, a_j <- a_j + k_m a_{m-j}, a_m = k_m, E_m =
// E_{m-1} (1 - k_m^2).  The loops are unrolled to OSZ_WG_MAXORDER and the orders past p skipped (p is
// the same for the whole grid), so the coefficients stay in registers.
__global__ void __launch_bounds__(kWgAuto)
granger_auto_kernel(const double *__restrict__ part, int nch, int p, double cnt, int64_t count, int64_t win0,
                    double *__restrict__ err) {
    const int64_t at = (int64_t)blockIdx.x * kWgAuto + threadIdx.x;
    if (at >= count * nch) return;
    const int64_t w = at / nch;
    const int c = (int)(at - w * nch);
    const int64_t rr = (int64_t)nch * nch;
    const double *g = part + (w * (2 * p + 1) + p) * rr + (int64_t)c * nch + c;      // G_cc(0)
    double r[OSZ_WG_MAXORDER + 1], a[OSZ_WG_MAXORDER + 1];
#pragma unroll
    for (int l = 0; l <= OSZ_WG_MAXORDER; ++l) {
        r[l] = l <= p ? g[l * rr] / cnt : 0.0;
        a[l] = 0.0;
    }
    double e = r[0];
#pragma unroll
    for (int m = 1; m <= OSZ_WG_MAXORDER; ++m) {
        if (m > p) continue;
        double s = r[m];
#pragma unroll
        for (int j = 1; j < m; ++j) s = __builtin_fma(a[j], r[m - j], s);
        const double k = -s / e;
#pragma unroll
        for (int j = 1; 2 * j <= m; ++j) {                   // (j, m - j) together, both from the old values
            const double lo = a[j], hi = a[m - j];
            a[j] = __builtin_fma(k, hi, lo);
            if (j != m - j) a[m - j] = __builtin_fma(k, lo, hi);
        }
        a[m] = k;
        e *= __builtin_fma(-k, k, 1.0);
    }
    err[(win0 + w) * nch + c] = e;
}

// One 8 x 8 tile of pairs (tile row bi <= tile column bj) and one window per workgroup of one wave, a
// lane per pair; the lanes with i < j compute.  P is the largest order of the instance (its LDS).
//
// The recursion.  V = U = C(0), D = C(1); for m = 1 .. p:
//   Ar = D U^-1, Br = D^T V^-1                              (the two reflection matrices)
//   V <- V - Ar D^T, U <- U - Br D                          (the forward and backward error covariances)
//   and, for m < p, with D' = C(m + 1):
//     for k = 1 .. m - 1:  A_k <- A_k - Ar B_{m-k},  B_{m-k} <- B_{m-k} - Br A_k   (both from the old
//                          values; one sweep does it in place),  D' <- D' - A_k C(m + 1 - k)
//     A_m = Ar, B_m = Br, D' <- D' - Ar C(1), D = D'.
// S is V after order p: the coefficients of order p itself are never formed.  (The backward residual
// of order m is D^T exactly, so it is not computed a second time.)
//
// LDS, `[slot][lane]` so that a wave's access to a slot is 64 consecutive doubles: slots 8 (k - 1) ..
// 8 (k - 1) + 7 are A_k and B_k, k = 1 .. P - 1; then G_ij(l) / W and G_ij(-l) / W, l = 1 .. P.  The
// diagonal's r_ii(l) and r_jj(l), l = 0 .. P, are shared by the tile's rows and columns: `own`.
// Grid: x = triangular tile index, y = window of the batch.
template <int P>
__global__ void __launch_bounds__(kWave)
granger_pair_kernel(const double *__restrict__ part, const double *__restrict__ err, int nch, int ntile, int p,
                    double cnt, int mask, double *__restrict__ out, int64_t out_plane, int64_t win0) {
    constexpr int kCoef = 8 * (P - 1);
    __shared__ double slot[kCoef + 2 * P][kWave];
    __shared__ double own[P + 1][2 * kWgTile];
    __shared__ double turn[kWgTile][kWgTile + 1];
    int bi, bj;
    pair_triangle(blockIdx.x, ntile, &bi, &bj);
    const int lane = threadIdx.x, a = lane / kWgTile, b = lane % kWgTile;
    const int i = bi * kWgTile + a, j = bj * kWgTile + b;
    const bool inside = i < nch && j < nch;
    const bool mine = inside && i < j;                       // this lane computes [i, j]
    // ... and writes the mirror [jm, im] of the pair that lane (b, a) computes
    const int jm = bj * kWgTile + a, im = bi * kWgTile + b;
    const bool mirrored = jm < nch && im < jm;
    const int64_t rr = (int64_t)nch * nch;
    const int64_t win = win0 + blockIdx.y;
    const double *g = part + ((int64_t)blockIdx.y * (2 * p + 1) + p) * rr;           // lag 0 of the window
    const double nan = __builtin_nan("");

    for (int e = lane; e < (p + 1) * 2 * kWgTile; e += kWave) {
        const int l = e / (2 * kWgTile), s = e % (2 * kWgTile);
        const int c = min(s < kWgTile ? bi * kWgTile + s : bj * kWgTile + s - kWgTile, nch - 1);
        own[l][s] = g[l * rr + (int64_t)c * nch + c] / cnt;
    }
    __syncthreads();

    double gij = nan, gji = nan, ins = nan;                  // F_{i->j}, F_{j->i} and instant
    if (mine) {
        const double *gp = g + (int64_t)i * nch + j;
        for (int l = 1; l <= p; ++l) {
            slot[kCoef + 2 * (l - 1)][lane] = gp[l * rr] / cnt;
            slot[kCoef + 2 * (l - 1) + 1][lane] = gp[-l * rr] / cnt;
        }
        // C(l) = [[r_ii(l), r_ij(-l)], [r_ij(l), r_jj(l)]]
        auto C = [&](int l) {
            return m2{own[l][a], slot[kCoef + 2 * (l - 1) + 1][lane], slot[kCoef + 2 * (l - 1)][lane],
                      own[l][kWgTile + b]};
        };
        const double r0 = gp[0] / cnt;
        m2 V{own[0][a], r0, r0, own[0][kWgTile + b]};
        m2 U = V, D = C(1);
        for (int m = 1; m <= p; ++m) {
            const m2 Dt = m2_t(D);
            const m2 Ar = m2_over(D, U), Br = m2_over(Dt, V);
            V = m2_less(V, Ar, Dt);
            U = m2_less(U, Br, D);
            if (m == p) break;
            m2 Dn = C(m + 1);
            // (the blocks of step k + 1 are read before those of step k are written: they are other
            // slots, and the reads then wait behind the arithmetic, not in front of it)
            auto block = [&](int s) {
                const double *q = &slot[s][lane];
                return m2{q[0], q[kWave], q[2 * kWave], q[3 * kWave]};
            };
            m2 Ak = block(0), Bq = block(m > 1 ? 8 * (m - 2) + 4 : 4), Ck = C(m);    // (not used when m = 1)
#pragma unroll 2
            for (int k = 1; k < m; ++k) {
                double *pa = &slot[8 * (k - 1)][lane], *pb = &slot[8 * (m - k - 1) + 4][lane];
                const int kn = k + 1 < m ? k + 1 : k;
                const m2 Ak1 = block(8 * (kn - 1)), Bq1 = block(8 * (m - kn - 1) + 4), Ck1 = C(m + 1 - kn);
                const m2 An = m2_less(Ak, Ar, Bq), Bn = m2_less(Bq, Br, Ak);
                pa[0] = An.a, pa[kWave] = An.b, pa[2 * kWave] = An.c, pa[3 * kWave] = An.d;
                pb[0] = Bn.a, pb[kWave] = Bn.b, pb[2 * kWave] = Bn.c, pb[3 * kWave] = Bn.d;
                Dn = m2_less(Dn, An, Ck);
                Ak = Ak1, Bq = Bq1, Ck = Ck1;
            }
            double *pa = &slot[8 * (m - 1)][lane];
            pa[0] = Ar.a, pa[kWave] = Ar.b, pa[2 * kWave] = Ar.c, pa[3 * kWave] = Ar.d;
            pa[4 * kWave] = Br.a, pa[5 * kWave] = Br.b, pa[6 * kWave] = Br.c, pa[7 * kWave] = Br.d;
            D = m2_less(Dn, Ar, C(1));
        }
        const double ei = err[win * nch + i], ej = err[win * nch + j], det = m2_det(V);
        if (wg_good(ei) && wg_good(ej) && wg_good(V.a) && wg_good(V.d) && wg_good(det)) {
            gij = wg_floor(log(ej / V.d));
            gji = wg_floor(log(ei / V.a));
            ins = wg_floor(log(V.a * V.d / det));
        }
    }
    // the diagonal: the fixed point 0.0, NaN where the channel is lost
    const bool diag = inside && i == j;
    if (diag) gij = gji = ins = wg_good(err[win * nch + i]) ? 0.0 : nan;
    const double vals[3] = {gij, ins, (gij + gji) + ins}, back[3] = {gji, ins, (gij + gji) + ins};
    const int64_t at = (int64_t)i * nch + j, mirror = (int64_t)jm * nch + im;
    double *o = out + win * rr;
    int plane = 0;
#pragma unroll
    for (int q = 0; q < OSZ_WG_COUNT; ++q) {
        if (!(mask & (1 << q))) continue;                    // (the same for the whole grid)
        if (mine || diag) o[plane * out_plane + at] = vals[q];
        pw_mirror(turn, a, b, back[q], mirrored, o + plane * out_plane + mirror);
        ++plane;
    }
}

// The work space of one push: [chan: nch nwin] [E: nch nwin] [G: batch (2 p + 1) nch nch]
static bool wg_plan(const PwArgs &A, PwPlan *q) {
    const int p = A.value;
    if (p < 1 || p > OSZ_WG_MAXORDER || p > A.W / 8) return false;
    return pw_plan(A, OSZ_WG_COUNT, 16, OSZ_WG_LONGEST, 2, 2 * p + 1, q);
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_granger_work(int nch, int64_t n, int64_t winsize, int64_t step, int order, int mask) {
    PwPlan q;
    return wg_plan({"osz_window_granger", nch, n, winsize, step, mask, "order", order}, &q) ? q.work() : -1;
}

int osz_window_granger(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int order,
                       int mask, double *out, int64_t plane_pitch, double *work, int64_t work_len, void *stream) {
    const PwArgs A{"osz_window_granger", nch, n, winsize, step, mask, "order", order};
    PwPlan q;
    const int rc = pw_head(A, wg_plan(A, &q), q, {{x, 8}, {out, 8}, {work, 8}}, pitch, true, plane_pitch, work_len);
    if (rc != OSZ_OK || q.nwin == 0) return rc;
    hipStream_t st = as_stream(stream);
    double *chan = work, *err = work + q.chan / 2, *part = work + q.chan;     // (q.chan: the sums and E)
    const int ntile = (nch + kWgTile - 1) / kWgTile;
    const double cnt = (double)winsize;
    return pw_batches(q, [&](int64_t w0, int64_t count) -> int {
        // (the sums batch by batch: they bring the batch's samples in for the Gram kernel)
        int rc = wx_window_sums(x, pitch, nch, winsize, step, w0, count, chan, "window_granger_prepare", st);
        if (rc != OSZ_OK) return rc;
        rc = wx_lagged_gram(x, pitch, nch, winsize, step, order, w0, count, chan, part, "window_granger_gram", st);
        if (rc != OSZ_OK) return rc;
        {
            KernelTimer timer("window_granger_auto", st);
            hipLaunchKernelGGL(granger_auto_kernel, dim3((unsigned)((count * nch + kWgAuto - 1) / kWgAuto)), dim3(kWgAuto),
                               0, st, part, nch, order, cnt, count, w0, err);
            OSZ_HIP(hipGetLastError());
        }
        KernelTimer timer("window_granger_pair", st);
        const dim3 grid((unsigned)(ntile * (ntile + 1) / 2), (unsigned)count);
        if (order <= 4)
            hipLaunchKernelGGL(granger_pair_kernel<4>, grid, dim3(kWave), 0, st, part, err, nch, ntile, order, cnt, mask,
                               out, plane_pitch, w0);
        else if (order <= 8)
            hipLaunchKernelGGL(granger_pair_kernel<8>, grid, dim3(kWave), 0, st, part, err, nch, ntile, order, cnt, mask,
                               out, plane_pitch, w0);
        else
            hipLaunchKernelGGL(granger_pair_kernel<16>, grid, dim3(kWave), 0, st, part, err, nch, ntile, order, cnt, mask,
                               out, plane_pitch, w0);
        OSZ_HIP(hipGetLastError());
        return OSZ_OK;
    });
}

}  // extern "C"
