// windowar.hip -- K22 autoregressive models per window (features/ar.py window_ar): for every window
// of W samples, step apart, of every channel the coefficients a_1 .. a_p of x_t + sum_k a_k x_{t-k} =
// e_t, the reflection coefficients k_1 .. k_p and the innovation variances E_0 .. E_p, by Burg's
// recursion or from the biased autocorrelation (Yule-Walker).  DESIGN.md section 4, K22.
//
// One workgroup per (channel, window) -- 64 threads for W < OSZ_AR_WIDE, 256 from there on -- on a
// one-dimensional grid, one instance per R, the samples a thread holds: the least power of two with
// NT R >= W.
//   * the window is read once, lane-strided (t = tid + NT j): the same pass takes the ballot for
//     non-finite samples and the sum of x - p about the pivot p, the window's first sample, that
//     gives the mean; the window, centred or not, goes into LDS with zeros behind it;
//   * burg: slot s = 0 .. W - 1 - m holds, while k_m is formed, the pair F_s = f_{s+m} and B_s =
//     b_{s+m-1} -- the two errors that k_m multiplies -- so num and den are sums over a thread's
//     own registers and need no neighbour.  A thread owns R consecutive slots (read once from LDS,
//     one double of padding every 32: without it the lanes read at a stride of R doubles).  After
//     the update B' = B + k F stays where it is and F' = F + k B moves DOWN one slot: within a
//     thread that is the register the fused multiply-add writes to, and across threads one value
//     pair from the neighbour above.  The slots run against the lanes (thread tid owns the slots
//     of NT - 1 - tid) so that this neighbour is the lane below and the pair comes by wave_shr:1;
//     lane 0 of a wave takes it from LDS, where lane 63 of the wave before put it.  Slots past the
//     last valid one hold F = B = 0 and add exactly nothing: the update keeps zeros zero, the
//     shift brings a zero into the top slot, and the one B that an order retires (slot W - m) is
//     zeroed by the one lane that holds it.  No sum is masked.
//     Per order: 3 R fused multiply-adds for num and den, wave_sum63 of both, (256 threads) the
//     waves' pairs and the edge pairs through LDS behind ONE barrier -- the buffers alternate with
//     m -- then k_m in every thread and 2 R fused multiply-adds for the update;
//   * yule_walker: lag j is the sum over a thread's samples of x_t x_{t+j}, x_t its register and
//     x_{t+j} one LDS read at unit stride over the lanes, then wave_sum63 and the waves in order;
//     all lags are folded behind one barrier;
//   * the Levinson step runs in wave 0, lane j holding a_j (lane 0: a_0 = 1): a_{m-j} comes by
//     ds_bpermute, Yule-Walker's numerator sum_{j<m} a_j r_{m-j} is wave_sum63 of one product a
//     lane, and lane m keeps k_m and E_m.  The same lanes store the planes.
// Every sum is per-thread in the order of the thread's samples, then a fixed DPP sequence over the
// lanes, then the waves in wave order: a function of (W, m) or (W, j) alone, and nothing of order m
// reads anything of a later order, so the bits of k_m and E_m do not depend on p.  No floating-point
// operation is atomic.
#include <cmath>

#include "window_block.h"

namespace osz {

#pragma clang fp contract(off)

constexpr int kArLags = OSZ_AR_ORDER + 1;
static_assert(OSZ_AR_WIDE <= 8 * kWave && OSZ_AR_LONGEST <= 16 * 256, "window_ar_kernel: samples a thread");
static_assert(kArLags <= kWave, "window_ar_kernel: one lane a coefficient");

struct WaArgs : WinHead {
    int order, method, center;
};

// the v of the lane below (wave_shr:1); 0 in lane 0
__device__ __forceinline__ double wa_below(double v) { return dpp_mov0<0x138>(v); }

// The reflection coefficients of Burg's recursion, k_m into kk[m], m = 1 .. p.  The window is in
// `win`, padded, zeros from W to NT R + 1.
template <int NT, int R>
__device__ __forceinline__ void wa_burg(const double *win, int W, int p, int tid, int lane, int w, double *kk,
                                        double (*red)[NT / kWave][2], double (*edge)[NT / kWave][2]) {
    constexpr int NW = NT / kWave, LR = __builtin_ctz(R);
    const int rev = NT - 1 - tid, base = rev * R;
    double f[R], b[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        b[i] = win[lds_pad32(base + i)];
        f[i] = win[lds_pad32(base + i + 1)];
    }
    for (int m = 1; m <= p; ++m) {
        const int z = W - m;                               // the slot this order retires
        if ((z >> LR) == rev) {
#pragma unroll
            for (int i = 0; i < R; ++i) b[i] = i == (z & (R - 1)) ? 0.0 : b[i];
        }
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            num = __builtin_fma(f[i], b[i], num);
            den = __builtin_fma(f[i], f[i], den);
            den = __builtin_fma(b[i], b[i], den);
        }
        num = wave_sum63(num);
        den = wave_sum63(den);
        double rf = wa_below(f[0]), rb = wa_below(b[0]);   // the pair of the slot above this thread's last
        if (NW == 1) {
            num = lane63(num);
            den = lane63(den);
        } else {
            const int par = m & 1;
            if (lane == kWave - 1) {
                red[par][w][0] = num;
                red[par][w][1] = den;
                edge[par][w][0] = f[0];
                edge[par][w][1] = b[0];
            }
            __syncthreads();
            num = red[par][0][0];
            den = red[par][0][1];
#pragma unroll
            for (int v = 1; v < NW; ++v) {
                num += red[par][v][0];
                den += red[par][v][1];
            }
            if (lane == 0 && w > 0) {
                rf = edge[par][w - 1][0];
                rb = edge[par][w - 1][1];
            }
        }
        const double k = (-2.0 * num) / den;               // (den = 0: num = 0 and k is NaN)
        if (tid == 0) kk[m] = k;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const double nb = __builtin_fma(k, f[i], b[i]);
            f[i] = i + 1 < R ? __builtin_fma(k, b[i + 1], f[i + 1]) : __builtin_fma(k, rb, rf);
            b[i] = nb;
        }
    }
}

template <int NT, int R>
__global__ void __launch_bounds__(NT) window_ar_kernel(const WaArgs A) {
    constexpr int NW = NT / kWave;
    extern __shared__ double wa_win[];                     // the window and the zeros behind it
    __shared__ double e0[NW];                              // sum x^2
    __shared__ double red[2][NW][2], edge[2][NW][2];       // burg: (num, den) and (F, B) of a wave's last lane
    __shared__ double kk[kArLags];                         // burg: k_m
    __shared__ double lag[kArLags][NW], rr[kArLags];       // yule_walker: the waves' sums, r_j
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = A.W, mask = A.mask, p = A.order;
    const bool burg = A.method == OSZ_AR_BURG;
    const WinAt at = win_where(A);
    const double *__restrict__ row = at.row;
    double *__restrict__ dst = at.dst;

    // the window into registers (every load in flight at once), the sum about its first sample, the ballot
    const double x0 = row[0], piv = __builtin_isfinite(x0) ? x0 : 0.0;
    double xs[R];
#pragma unroll
    for (int j = 0; j < R; ++j) xs[j] = tid + j * NT < W ? row[tid + j * NT] : 0.0;
    double S1[1] = {0.0};
    bool wild = false;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        wild |= !__builtin_isfinite(xs[j]);
        S1[0] += tid + j * NT < W ? xs[j] - piv : 0.0;
    }
    const bool spoilt = win_fold<NW>(S1, wild, lane, w);
    const int pl_ref = (mask & 1) * p, pl_err = pl_ref + ((mask >> OSZ_AR_REFLECTION) & 1) * p;
    const int pl_path = pl_err + ((mask >> OSZ_AR_ERROR) & 1);
    if (spoilt) {                                          // (the whole workgroup)
        win_spoilt<NT>(dst, pl_path + ((mask >> OSZ_AR_ERROR_PATH) & 1) * (p + 1), A.plane_pitch, tid);
        return;
    }

    // the window, centred, into LDS; zeros from W to NT R + OSZ_AR_ORDER; burg's sum x^2
    const double mu = S1[0] / (double)W;
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int t = tid + j * NT;
        if (t < W) {
            xs[j] = A.center ? (xs[j] - piv) - mu : xs[j];
            wa_win[burg ? lds_pad32(t) : t] = xs[j];
        }
        s2 = __builtin_fma(xs[j], xs[j], s2);
    }
    for (int t = W + tid; t <= NT * R + OSZ_AR_ORDER; t += NT) wa_win[burg ? lds_pad32(t) : t] = 0.0;
    s2 = wave_sum63(s2);
    if (lane == kWave - 1) e0[w] = s2;
    __syncthreads();

    if (burg) {
        wa_burg<NT, R>(wa_win, W, p, tid, lane, w, kk, red, edge);
    } else {
        for (int j = 0; j <= p; ++j) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) s = __builtin_fma(xs[i], wa_win[tid + i * NT + j], s);
            s = wave_sum63(s);
            if (lane == kWave - 1) lag[j][w] = s;
        }
        if (NW > 1) __syncthreads();
    }
    if (w != 0) return;
    wave_lds_fence();                                      // kk, or lag of a one-wave workgroup: wave 0's own

    // the Levinson step, lane j holding a_j; lane m keeps k_m and E_m
    double E;
    if (burg) {
        E = e0[0];
#pragma unroll
        for (int v = 1; v < NW; ++v) E += e0[v];
        E /= (double)W;
    } else {
        if (lane <= p) {
            double r = lag[lane][0];
#pragma unroll
            for (int v = 1; v < NW; ++v) r += lag[lane][v];
            rr[lane] = r / (double)W;
        }
        wave_lds_fence();
        E = rr[0];
    }
    const double E0 = E;
    double a = lane == 0 ? 1.0 : 0.0, kr = 0.0, ep = E0;
    for (int m = 1; m <= p; ++m) {
        double k;
        if (burg) {
            k = kk[m];
        } else {
            const double term = lane < m ? a * rr[m - lane] : 0.0;
            k = -lane63(wave_sum63(term)) / E;
        }
        k = (E != 0.0 && E == E) ? k : __builtin_nan("");   // a spent or lost E ends the model here
        const double far = lane_from(a, (m - lane) & (kWave - 1));
        a = (lane >= 1 && lane < m) ? __builtin_fma(k, far, a) : lane == m ? k : a;
        E = E * (1.0 - k * k);
        if (lane == m) {
            kr = k;
            ep = E;
        }
    }
    if (E0 == 0.0) ep = 0.0;                               // nothing to model: the errors are 0, the rest NaN
    if (lane > p) return;
    if (lane >= 1) {
        if (mask & (1 << OSZ_AR_COEFFICIENTS)) dst[(int64_t)(lane - 1) * A.plane_pitch] = a;
        if (mask & (1 << OSZ_AR_REFLECTION)) dst[(int64_t)(pl_ref + lane - 1) * A.plane_pitch] = kr;
    }
    if ((mask & (1 << OSZ_AR_ERROR)) && lane == p) dst[(int64_t)pl_err * A.plane_pitch] = ep;
    if (mask & (1 << OSZ_AR_ERROR_PATH)) dst[(int64_t)(pl_path + lane) * A.plane_pitch] = ep;
}

template <int NT, int R>
static void wa_launch(unsigned nblk, size_t lds, hipStream_t st, const WaArgs &A) {
    hipLaunchKernelGGL((window_ar_kernel<NT, R>), dim3(nblk), dim3(NT), lds, st, A);
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_window_ar(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                  int order, int method, int center, double *out, int64_t plane_pitch, int64_t row_pitch,
                  int64_t win0, void *stream) {
    static const WinRule rule = {"osz_window_ar", "measure", OSZ_AR_COUNT, 16, OSZ_AR_LONGEST};
    const int planes = ((mask >> OSZ_AR_COEFFICIENTS) & 1) * order + ((mask >> OSZ_AR_REFLECTION) & 1) * order +
                       ((mask >> OSZ_AR_ERROR) & 1) + ((mask >> OSZ_AR_ERROR_PATH) & 1) * (order + 1);
    WaArgs A;
    if (int rc = win_head(rule, planes, x, pitch, nch, n, winsize, step, mask, out, plane_pitch, row_pitch, win0, A))
        return rc;
    OSZ_REQUIRE(order >= 1 && order <= OSZ_AR_ORDER && winsize >= 4 * (int64_t)order,
                "osz_window_ar: order=%d (1 .. %d, winsize=%lld >= 4 order)", order, OSZ_AR_ORDER, (long long)winsize);
    OSZ_REQUIRE(method == OSZ_AR_BURG || method == OSZ_AR_YULE_WALKER, "osz_window_ar: method %d", method);
    if (A.nwin == 0) return OSZ_OK;
    unsigned nblk;
    if (int rc = win_grid(rule, A, nch, nblk)) return rc;
    A.order = order;
    A.method = method;
    A.center = center != 0;
    const int W = (int)winsize, NT = W >= OSZ_AR_WIDE ? 256 : kWave;
    int R = 1;                                             // samples a thread: the least power of two with NT R >= W
    while (NT * R < W) R *= 2;
    const int cells = NT * R + OSZ_AR_ORDER + 1;           // the window and the zeros behind it; burg's padding
    const size_t lds = (size_t)(cells + (cells >> 5) + 1) * sizeof(double);
    hipStream_t st = as_stream(stream);
    KernelTimer timer("window_ar", st);
    if (NT == kWave) {
        if (R == 1) wa_launch<64, 1>(nblk, lds, st, A);
        else if (R == 2) wa_launch<64, 2>(nblk, lds, st, A);
        else if (R == 4) wa_launch<64, 4>(nblk, lds, st, A);
        else wa_launch<64, 8>(nblk, lds, st, A);
    } else {
        if (R == 2) wa_launch<256, 2>(nblk, lds, st, A);
        else if (R == 4) wa_launch<256, 4>(nblk, lds, st, A);
        else if (R == 8) wa_launch<256, 8>(nblk, lds, st, A);
        else wa_launch<256, 16>(nblk, lds, st, A);
    }
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
