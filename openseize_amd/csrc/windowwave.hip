// windowwave.hip -- K21 wavelet sub-band energies and statistics per window (features/wavelet.py
// window_wavelet): for every window of W samples, step apart, of every channel the numbers of
// osz_window_wavelet_feature over the bands d^1 .. d^J, a^J of an orthonormal discrete wavelet
// transform periodised within the window.  DESIGN.md section 4, K21.
//
// One workgroup per (channel, window) -- 64 threads for W <= OSZ_WW_WIDE, 256 above -- on a
// one-dimensional grid:
//   * the window is read once, every load of a thread in flight at the same time, into registers;
//     the same pass takes the ballot for non-finite samples and the sum of x - p about the pivot p,
//     the window's first sample, that gives the mean; a^0 -- x, or (x - p) - mean with center --
//     goes into LDS, W doubles;
//   * a second buffer of W / 2 doubles takes a^1, the first one a^2, and so on in turn: 1.5 W
//     doubles, 48 KB at W = 4096;
//   * per level a thread owns the outputs i = tid, tid + NT, .. < n_j / 2 and keeps their a_i and
//     d_i in registers (at most 8 of each).  The loop over the taps is the OUTER one, two taps a
//     step: h_k, h_{k+1}, g_k, g_{k+1} are uniform and shared by the thread's outputs.  They are
//     two 16-byte LDS reads at one address for all lanes, from a copy of the kernel's arguments
//     made once.  Read by the scalar unit from the arguments themselves, a step waited for the
//     scalar load and then for the window's read, and the 64 values do not fit the scalar
//     registers beside the rest (two steps' worth at a time already spilled); from LDS they
//     arrive with the window's values (measured together with the batched loads of the window:
//     DESIGN.md).  Per output the pair a^j[2i+k], a^j[2i+k+1] is one 16-byte LDS read and feeds
//     four fused multiply-adds.  n_j is
//     even at every level that is transformed, so (2i + k) mod n_j is even for even k and the pair
//     never straddles the wrap; k mod n_j is a scalar that advances by 2 and wraps by a compare
//     and a subtraction whatever n_j is (2 <= n_j), and 2i + (k mod n_j) < 2 n_j wraps by an
//     unsigned minimum: no level needs an integer remainder;
//   * only a^{j+1} goes back to LDS.  The statistics of d^{j+1} (and of a^J at the last level) are
//     taken from the registers that formed it: its sum first, folded over the workgroup, then
//     sum c^2, sum |c| and sum (c - mean)^2 -- the deviations about the band's mean, never
//     E[c^2] - E[c]^2.  The one barrier a level that publishes a^{j+1} publishes the sum too.
//     The sum and the deviations are taken only when std is asked and sum |c| only with mean_abs
//     (the default call folds one number a level, not four); the means and the averages are
//     products with the host's 1 / n_j, the kernel divides only for relative and entropy;
//   * a wave whose 64 outputs lie past n_j / 2 skips the level's arithmetic, and from the level
//     with n_j / 2 <= 64 on wave 0 goes on alone: the other waves wait at the last barrier, and
//     wave 0 hands a^{j+1} to itself through LDS behind a wave fence and takes the band's sum
//     from lane 63, with no barrier at all.  A one-wave workgroup runs every level this way.
// Every fold is per-thread in the order of the thread's outputs, then wave_sum63 over the lanes,
// then the waves in wave order: a function of (W, J) alone; a coefficient is a chain of fused
// multiply-adds in the order of k.  No floating-point operation is atomic.
#include <cmath>

#include "window_block.h"

namespace osz {

#pragma clang fp contract(off)

constexpr int kWwBands = OSZ_WW_LEVELS + 1;
static_assert(OSZ_WW_WIDE <= 2 * 4 * kWave && OSZ_WW_LONGEST <= 2 * 8 * 256, "window_wavelet_kernel: outputs a thread");
static_assert(OSZ_WW_TAPS % 2 == 0 && 2 * OSZ_WW_TAPS <= kWave && kWwBands <= kWave,
              "window_wavelet_kernel: taps in pairs, one lane a filter value, one lane a band");

struct WwArgs : WinHead {
    int pairs, levels;    // taps / 2, J
    int center, normalize;
    double ln_b;          // ln(J + 1), the host's
    double rw;            // 1 / W
    double rn[OSZ_WW_LEVELS + 1];   // 1 / the coefficients of band b
    double f[OSZ_WW_TAPS / 2][4];   // h_k, h_{k+1}, g_k, g_{k+1} for k = 0, 2, ..; zeros behind the taps
};

// The sum, over the wave's lanes that hold one, of the Q values of c: in lane 63.
template <int Q, int NT>
__device__ __forceinline__ double ww_sum(const double (&c)[Q], int tid, int half) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (q * NT >= half) break;
        s += tid + q * NT < half ? c[q] : 0.0;
    }
    return wave_sum63(s);
}

// sum c^2 and, where asked, sum |c| and sum (c - mean)^2 of the same values: the wave's in lane
// 63.  (What is asked is uniform, and no sum's arithmetic depends on the others.)
template <int Q, int NT>
__device__ __forceinline__ void ww_moments(const double (&c)[Q], int tid, int half, double mean, bool want_abs,
                                           bool want_std, double (&m)[3]) {
    double e2 = 0.0, e1 = 0.0, dv = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (q * NT >= half) break;
        const bool on = tid + q * NT < half;
        const double v = on ? c[q] : 0.0, d = on ? c[q] - mean : 0.0;
        e2 = __builtin_fma(v, v, e2);
        if (want_abs) e1 += __builtin_fabs(v);
        if (want_std) dv = __builtin_fma(d, d, dv);
    }
    m[0] = wave_sum63(e2);
    m[1] = want_abs ? wave_sum63(e1) : 0.0;
    m[2] = want_std ? wave_sum63(dv) : 0.0;
}

template <int NT, int Q>
__global__ void __launch_bounds__(NT) window_wavelet_kernel(const WwArgs A) {
    constexpr int NW = NT / kWave;
    extern __shared__ __align__(16) double ww_lds[];       // W + W / 2: the window, a^1; a^2, a^3 ..
    __shared__ double bsum[kWwBands][NW];                  // a band's sum
    __shared__ double bmom[kWwBands][NW][3];               // its sum c^2, sum |c|, sum (c - mean)^2
    __shared__ double eb[kWwBands], et[kWwBands];
    __shared__ __align__(16) double ww_taps[OSZ_WW_TAPS / 2][4];   // A.f
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = A.W, mask = A.mask, J = A.levels, B = J + 1, pairs = A.pairs;
    const bool want_abs = mask & (1 << OSZ_WW_MEAN_ABS), want_std = mask & (1 << OSZ_WW_STD);
    const WinAt at = win_where(A);
    const double *__restrict__ row = at.row;
    double *__restrict__ dst = at.dst;

    // the window into registers (every load in flight at once), the sum about its first sample, the
    // ballot; the filters into LDS
    const double x0 = row[0], p = __builtin_isfinite(x0) ? x0 : 0.0;
    double xr[2 * Q];
#pragma unroll
    for (int q = 0; q < 2 * Q; ++q) xr[q] = q * NT < W && tid + q * NT < W ? row[tid + q * NT] : 0.0;
    if (tid < 2 * OSZ_WW_TAPS) ww_taps[tid >> 2][tid & 3] = A.f[tid >> 2][tid & 3];
    double S1[1] = {0.0};
    bool wild = false;
#pragma unroll
    for (int q = 0; q < 2 * Q; ++q) {
        if (q * NT >= W) break;
        wild |= !__builtin_isfinite(xr[q]);
        S1[0] += tid + q * NT < W ? xr[q] - p : 0.0;
    }
    if (win_fold<NW>(S1, wild, lane, w)) {                 // (the whole workgroup)
        const int planes = __builtin_popcount(mask & ~(1 << OSZ_WW_ENTROPY)) * B + ((mask >> OSZ_WW_ENTROPY) & 1);
        win_spoilt<NT>(dst, planes, A.plane_pitch, tid);
        return;
    }
    const double mu = S1[0] * A.rw;
#pragma unroll
    for (int q = 0; q < 2 * Q; ++q) {                      // a^0
        if (q * NT >= W) break;
        if (tid + q * NT < W) ww_lds[tid + q * NT] = A.center ? (xr[q] - p) - mu : xr[q];
    }
    __syncthreads();

    double *src = ww_lds, *nxt = ww_lds + W;
    int n = W;
    for (int j = 0; j < J; ++j) {
        const int half = n >> 1;
        const bool last = j == J - 1;
        const bool solo = NW == 1 || half <= kWave;        // wave 0 alone from here on (uniform over the workgroup)
        if (solo && w != 0) break;                         // (to the last barrier)
        const bool mine = w * kWave < half;                // this wave has outputs
        double ca[Q], cd[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            ca[q] = 0.0;
            cd[q] = 0.0;
        }
        if (mine) {
            int at[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q)                     // (a lane without an output redoes output 0)
                at[q] = tid + q * NT < half ? 2 * (tid + q * NT) : 0;
            int kk = 0;                                    // k mod n
            for (int k2 = 0; k2 < pairs; ++k2) {
                const double2 h = *reinterpret_cast<const double2 *>(&ww_taps[k2][0]);
                const double2 g = *reinterpret_cast<const double2 *>(&ww_taps[k2][2]);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (q * NT >= half) break;
                    // (2i + k mod n) mod n of a value below 2 n: the smaller of it and it - n, unsigned
                    const unsigned idx = min((unsigned)(at[q] + kk), (unsigned)(at[q] + kk - n));
                    const double2 v = *reinterpret_cast<const double2 *>(src + idx);
                    ca[q] = __builtin_fma(h.x, v.x, ca[q]);
                    cd[q] = __builtin_fma(g.x, v.x, cd[q]);
                    ca[q] = __builtin_fma(h.y, v.y, ca[q]);
                    cd[q] = __builtin_fma(g.y, v.y, cd[q]);
                }
                kk += 2;
                kk -= kk >= n ? n : 0;
            }
            if (!last) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (q * NT >= half) break;
                    if (tid + q * NT < half) nxt[tid + q * NT] = ca[q];
                }
            }
        }
        // the band's sum, for its mean: only std reads it
        const double sd = want_std && mine ? ww_sum<Q, NT>(cd, tid, half) : 0.0;
        const double sa = want_std && mine && last ? ww_sum<Q, NT>(ca, tid, half) : 0.0;
        double md = 0.0, ma = 0.0;
        if (solo) {
            wave_lds_fence();                              // a^{j+1}, wave 0's own
            if (want_std) {
                md = lane63(sd);
                ma = lane63(sa);
            }
        } else {
            if (want_std && lane == kWave - 1) {
                bsum[j][w] = sd;
                if (last) bsum[J][w] = sa;
            }
            __syncthreads();                               // a^{j+1} and the sums; every read of a^j is done
            if (want_std) {
                md = bsum[j][0];
                ma = last ? bsum[J][0] : 0.0;
#pragma unroll
                for (int v = 1; v < NW; ++v) {
                    md += bsum[j][v];
                    ma += last ? bsum[J][v] : 0.0;
                }
            }
        }
        double m[3] = {0.0, 0.0, 0.0};
        if (mine) ww_moments<Q, NT>(cd, tid, half, md * A.rn[j], want_abs, want_std, m);
        if (lane == kWave - 1) {
#pragma unroll
            for (int v = 0; v < 3; ++v) bmom[j][w][v] = m[v];
            if (solo) {                                    // (the waves that left)
#pragma unroll
                for (int u = 1; u < NW; ++u) bmom[j][u][0] = bmom[j][u][1] = bmom[j][u][2] = 0.0;
            }
        }
        if (last) {
            double ml[3] = {0.0, 0.0, 0.0};
            if (mine) ww_moments<Q, NT>(ca, tid, half, ma * A.rn[J], want_abs, want_std, ml);
            if (lane == kWave - 1) {
#pragma unroll
                for (int v = 0; v < 3; ++v) bmom[J][w][v] = ml[v];
                if (solo) {
#pragma unroll
                    for (int u = 1; u < NW; ++u) bmom[J][u][0] = bmom[J][u][1] = bmom[J][u][2] = 0.0;
                }
            }
        }
        double *const t = src;
        src = nxt;
        nxt = t;
        n = half;
    }
    __syncthreads();

    // one lane a band (of wave 0: B <= 64); the planes are energy, relative, entropy, mean_abs and
    // std, of those asked
    if (tid >= B) return;
    const int pl_rel = (mask & 1) * B, pl_ent = pl_rel + ((mask >> OSZ_WW_RELATIVE) & 1) * B;
    const int pl_abs = pl_ent + ((mask >> OSZ_WW_ENTROPY) & 1), pl_std = pl_abs + ((mask >> OSZ_WW_MEAN_ABS) & 1) * B;
    double E = bmom[tid][0][0], e1 = bmom[tid][0][1], dv = bmom[tid][0][2];
#pragma unroll
    for (int v = 1; v < NW; ++v) {
        E += bmom[tid][v][0];
        e1 += bmom[tid][v][1];
        dv += bmom[tid][v][2];
    }
    eb[tid] = E;
    if (mask & (1 << OSZ_WW_ENERGY)) dst[(int64_t)tid * A.plane_pitch] = E;
    if (want_abs) dst[(int64_t)(pl_abs + tid) * A.plane_pitch] = e1 * A.rn[tid];
    if (want_std) dst[(int64_t)(pl_std + tid) * A.plane_pitch] = sqrt(dv * A.rn[tid]);
    if (!(mask & (1 << OSZ_WW_RELATIVE | 1 << OSZ_WW_ENTROPY))) return;
    wave_lds_fence();
    double total = 0.0;
    for (int b = 0; b < B; ++b) total += eb[b];
    const double pb = E / total;
    if (mask & (1 << OSZ_WW_RELATIVE)) dst[(int64_t)(pl_rel + tid) * A.plane_pitch] = pb;
    if (!(mask & (1 << OSZ_WW_ENTROPY))) return;
    et[tid] = pb > 0.0 ? pb * log(pb) : 0.0;               // (the logarithms side by side, the sum in the order of b)
    wave_lds_fence();
    if (tid != 0) return;
    double H = 0.0;
    for (int b = 0; b < B; ++b) H -= et[b];
    if (A.normalize) H /= A.ln_b;
    dst[(int64_t)pl_ent * A.plane_pitch] = total > 0.0 ? H : __builtin_nan("");
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_window_wavelet(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                       const double *lo, int taps, int levels, int center, int normalize, double *out,
                       int64_t out_plane, int64_t out_pitch, void *stream) {
    static const WinRule rule = {"osz_window_wavelet", "feature", OSZ_WW_COUNT, 8, OSZ_WW_LONGEST};
    const int B = levels + 1;
    const int planes = __builtin_popcount(mask & ~(1 << OSZ_WW_ENTROPY)) * B + ((mask >> OSZ_WW_ENTROPY) & 1);
    WwArgs A;
    if (int rc = win_head(rule, planes, x, pitch, nch, n, winsize, step, mask, out, out_plane, out_pitch, 0, A))
        return rc;
    OSZ_REQUIRE(lo, "osz_window_wavelet: null argument");
    OSZ_REQUIRE(taps >= 2 && taps <= OSZ_WW_TAPS && taps % 2 == 0, "osz_window_wavelet: %d taps (even, 2 .. %d)", taps,
                OSZ_WW_TAPS);
    OSZ_REQUIRE(levels >= 1 && levels <= OSZ_WW_LEVELS && winsize % ((int64_t)1 << levels) == 0,
                "osz_window_wavelet: levels=%d (1 .. %d, winsize=%lld a multiple of 2^levels)", levels, OSZ_WW_LEVELS,
                (long long)winsize);
    if (A.nwin == 0) return OSZ_OK;
    unsigned nblk;
    if (int rc = win_grid(rule, A, nch, nblk)) return rc;
    memset(A.f, 0, sizeof A.f);
    for (int k = 0; k < taps; ++k) {
        OSZ_REQUIRE(std::isfinite(lo[k]), "osz_window_wavelet: tap %d is not finite", k);
        A.f[k / 2][k % 2] = lo[k];
        A.f[k / 2][2 + k % 2] = (k % 2 ? -1.0 : 1.0) * lo[taps - 1 - k];     // g_k = (-1)^k h_{L-1-k}
    }
    A.pairs = taps / 2;
    A.levels = levels;
    A.center = center != 0;
    A.normalize = normalize != 0;
    A.ln_b = std::log((double)B);
    A.rw = 1.0 / (double)winsize;
    memset(A.rn, 0, sizeof A.rn);
    for (int b = 0; b < B; ++b) A.rn[b] = 1.0 / (double)(winsize >> (b < levels ? b + 1 : levels));
    const size_t lds = (size_t)(winsize + winsize / 2) * sizeof(double);
    hipStream_t st = as_stream(stream);
    KernelTimer timer("window_wavelet", st);
    if (winsize > OSZ_WW_WIDE) hipLaunchKernelGGL((window_wavelet_kernel<256, 8>), dim3(nblk), dim3(256), lds, st, A);
    else hipLaunchKernelGGL((window_wavelet_kernel<64, 4>), dim3(nblk), dim3(64), lds, st, A);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
