// windowfrac.hip -- K20 fractal dimensions and detrended fluctuation analysis per window
// (features/fractal.py window_fractal): for every window of W samples, step apart, of every channel
// the numbers of osz_window_fractal_measure -- the scaling family beside K15's sums and K16's
// pattern counts.  DESIGN.md section 4, K20.
//
// One workgroup per (channel, window) -- 64 threads for W < OSZ_WR_WIDE, 256 from there on -- on a
// one-dimensional grid.  Thread tid owns the samples t = tid + NT j, j < W / NT <= 16, and keeps
// them in registers:
//   * the window goes into LDS once; the same pass takes the ballot for non-finite samples and the
//     sum of x - p about the pivot p, the window's first sample, that gives the mean;
//   * katz and petrosian are one pass over the thread's samples: x_{t+1} and x_{t+2} from LDS at
//     unit stride over the lanes, a sum, a maximum and an integer count (the scalar unit counts
//     the bits of the wave's ballot);
//   * higuchi: every t in 0 .. W - 1 - k belongs to exactly one (m, k), m = t mod k, and n_mk takes
//     two values only -- q = (W - 1) / k for m <= (W - 1) mod k, q - 1 above -- so L(k) is two plain
//     sums of |x_{t+k} - x_t| with two weights.  x_t is the thread's register, x_{t+k} one LDS read
//     at unit stride over the lanes (no bank conflict); m advances by NT mod k a step;
//   * dfa: the lanes of a wave scan their 64 consecutive z = (x - p) - mean with DPP row shifts,
//     the waves' totals go through LDS and are taken in the order of t, and the profile replaces
//     the window in LDS, one double of padding every 32 (box b of n samples starts at b n: without
//     it a lane per box reads at a stride of n doubles, a 32-way bank conflict for n = 32; with it
//     the power-of-two strides are conflict-free).  Per scale the W / n boxes share the
//     workgroup's lanes: g consecutive lanes a box, g the largest power of two with g W / n <= NT
//     (a lane a box when there are more boxes than lanes, a wave a box at the most), so that a
//     scale of long boxes keeps as many lanes busy as one of short boxes: with a lane a box
//     whatever n, a scale costs its n steps for W / n lanes, and at W = 256 the scales of 16 to
//     55 samples were two thirds of the time.  A box is read twice -- sum y' and sum (i - ibar) y'
//     of y' = y - y_first, folded over the group by the first log2 g steps of wave_sum63 and handed
//     back by ds_bpermute, give the line; the second read sums the squared residuals themselves.
//     (The one-read form sum y'^2 - (sum y')^2 / n - (sum (i - ibar) y')^2 / sum (i - ibar)^2
//     cancels: on a random walk, whose profile is a steep line in every box, it loses the digits
//     the bound of the tests is made of.)
// Every fold is per-thread in the order of j or i, then a fixed DPP sequence over the lanes (of a
// box's group, of the wave), then the waves in wave order: a function of (W, k) or (W, n) alone.
// No floating-point operation is atomic.
#include <cmath>

#include "window_block.h"

namespace osz {

#pragma clang fp contract(off)

// doubles behind the window in LDS: higuchi's last step reads x_{t+k} for t up to NT - 1 past
// W - k and katz x_{t+2} (both are then discarded), and the padded profile ends at W + W / 32
constexpr int kWrPad = 264;
// OSZ_WR_WIDE = 512.  Below it one wave holds a window in 8 registers a lane, no fold crosses a
// wave and the barriers are a wave's own; every per-k and per-scale loop of such a window is at
// most 8 steps, about what a fold over four waves through LDS costs, so four waves would spend as
// much on folds as they save on steps.  From 512 on four waves cut the loops by four (16 steps a k
// at 4096 samples instead of 64) and a thread's samples stay within 16 registers.  (Reasoned from
// the instruction counts; the other values were not timed.)
static_assert(OSZ_WR_WIDE <= 8 * kWave && OSZ_WR_LONGEST <= 16 * 256, "window_fractal_kernel: samples a thread");
static_assert(kWrPad >= 256 + 2 && kWrPad >= OSZ_WR_LONGEST / 32 + 1, "kWrPad");
static_assert(OSZ_WR_KMAX <= kWave && OSZ_WR_SCALES <= kWave, "window_fractal_kernel: one lane a k, a scale");

struct WrArgs : WinHead {
    int kmax, nscale;
    double ln_n, log10_w; // ln(W - 1) and log10 W, the host's
    int scales[OSZ_WR_SCALES];
};

// Inclusive prefix sum over the 64 lanes: four row_shr steps scan the 16-lane rows, then a lane
// adds the totals of the rows below its own, in their order.  (Not ws_wave_scan of windowspec.hip,
// which adds what row_bcast hands on, row 0 + row 1 before row 2: other bits.  Each kernel's
// results are pinned to its own order.)
__device__ __forceinline__ double wave_scan(double v, int lane) {
    v += dpp_mov0<0x111>(v);
    v += dpp_mov0<0x112>(v);
    v += dpp_mov0<0x114>(v);
    v += dpp_mov0<0x118>(v);
    const double r0 = lane_of<15>(v), r1 = lane_of<31>(v), r2 = lane_of<47>(v);
    v += lane >= 16 ? r0 : 0.0;
    v += lane >= 32 ? r1 : 0.0;
    v += lane >= 48 ? r2 : 0.0;
    return v;
}

// Sum over every group of g consecutive lanes, g a power of two up to 64 and the wave's: valid in
// the LAST lane of each group -- the first log2 g steps of wave_sum63.
__device__ __forceinline__ double group_sum(double v, int g) {
    if (g >= 2) v += dpp_mov0<0x111>(v);
    if (g >= 4) v += dpp_mov0<0x112>(v);
    if (g >= 8) v += dpp_mov0<0x114>(v);
    if (g >= 16) v += dpp_mov0<0x118>(v);
    if (g >= 32) v += dpp_mov0<0x142>(v);
    if (g >= 64) v += dpp_mov0<0x143>(v);
    return v;
}

// the v of the last lane of its group of g, in every lane
__device__ __forceinline__ double group_last(double v, int lane, int g) { return lane_from(v, lane | (g - 1)); }

// Least-squares slope of v on u over n points, the abscissa centred (one thread).
__device__ __forceinline__ double wr_slope(const double *u, const double *v, int n) {
    double su = 0.0;
    for (int i = 0; i < n; ++i) su += u[i];
    const double ubar = su / (double)n;
    double num = 0.0, den = 0.0;
    for (int i = 0; i < n; ++i) {
        const double du = u[i] - ubar;
        num += du * v[i];
        den += du * du;
    }
    return num / den;
}

template <int NT, int JMAX>
__global__ void __launch_bounds__(NT) window_fractal_kernel(const WrArgs A) {
    constexpr int NW = NT / kWave;
    extern __shared__ double wr_win[];                     // W + kWrPad: the window, then its profile
    __shared__ double red[NW][2];                          // katz's L and d
    __shared__ int flips[NW];
    __shared__ double hred[OSZ_WR_KMAX][NW][2];
    __shared__ double tot[JMAX * NW];
    __shared__ double dred[OSZ_WR_SCALES][NW];
    __shared__ double hu[OSZ_WR_KMAX], hv[OSZ_WR_KMAX], du[OSZ_WR_SCALES], dv[OSZ_WR_SCALES];
    __shared__ int sc[OSZ_WR_SCALES];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = A.W, mask = A.mask;
    const WinAt at = win_where(A);
    const double *__restrict__ row = at.row;
    double *__restrict__ dst = at.dst;
    const bool higuchi = mask & (1 << OSZ_WR_HIGUCHI), dfa = mask & (1 << OSZ_WR_DFA | 1 << OSZ_WR_DFA_FLUCTUATIONS);
    const int S = dfa ? A.nscale : 0;

    // the window into LDS and registers, the sum about its first sample, the ballot
    const double x0 = row[0], p = __builtin_isfinite(x0) ? x0 : 0.0;
    double xr[JMAX];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) xr[j] = 0.0;
    double S1[1] = {0.0};
    bool wild = false;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        if (j * NT >= W) break;
        const int t = tid + j * NT;
        if (t < W) {
            const double v = row[t];
            wr_win[t] = v;
            xr[j] = v;
            wild |= !__builtin_isfinite(v);
            S1[0] += v - p;
        }
    }
    if (win_fold<NW>(S1, wild, lane, w)) {                 // (the whole workgroup)
        win_spoilt<NT>(dst, __builtin_popcount(mask & 15) + ((mask >> OSZ_WR_DFA_FLUCTUATIONS) & 1) * S, A.plane_pitch,
                       tid);
        return;
    }

    if (mask & (1 << OSZ_WR_KATZ | 1 << OSZ_WR_PETROSIAN)) {
        double kl = 0.0, kd = 0.0;
        int flip = 0;                                      // (the wave's)
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            if (j * NT >= W) break;
            const int t = tid + j * NT;
            const double a = wr_win[t + 1], b = wr_win[t + 2];
            const double d0 = a - xr[j], d1 = b - a;
            kl += t < W - 1 ? __builtin_fabs(d0) : 0.0;
            kd = __builtin_fmax(kd, t < W ? __builtin_fabs(xr[j] - x0) : 0.0);
            const bool turn = (t < W - 2) & (((d0 > 0.0) & (d1 < 0.0)) | ((d0 < 0.0) & (d1 > 0.0)));
            flip += __builtin_popcountll(__builtin_amdgcn_ballot_w64(turn));
        }
        kl = wave_sum63(kl);
        kd = wave_max63(kd);
        if (lane == kWave - 1) {
            red[w][0] = kl;
            red[w][1] = kd;
            flips[w] = flip;
        }
    }

    if (higuchi) {
        for (int k = 1; k <= A.kmax; ++k) {
            const int lim = W - k, r = (W - 1) % k, adv = NT % k;
            // tid mod k: tid + 0.5 is at least 0.5 / 64 from a multiple of k, the float product
            // within 256 * 2^-22 of the quotient
            int m = tid - k * (int)(((float)tid + 0.5f) * (1.0f / (float)k));
            double a0 = 0.0, a1 = 0.0;
            const double *far = wr_win + tid + k;
#pragma unroll
            for (int j = 0; j < JMAX; ++j) {
                if (j * NT >= lim) break;
                const double d = __builtin_fabs(far[j * NT] - xr[j]);
                const bool ok = tid + j * NT < lim, lo = m <= r;
                a0 += (ok & lo) ? d : 0.0;
                a1 += (ok & !lo) ? d : 0.0;
                m += adv;
                m -= m >= k ? k : 0;
            }
            a0 = wave_sum63(a0);
            a1 = wave_sum63(a1);
            if (lane == kWave - 1) {
                hred[k - 1][w][0] = a0;
                hred[k - 1][w][1] = a1;
            }
        }
    }

    if (dfa) {                                             // (uniform: the barriers are the workgroup's)
        // the scan of each wave's 64 consecutive samples, in place of the samples
        const double mu = S1[0] / (double)W;
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            if (j * NT >= W) break;
            const double z = tid + j * NT < W ? (xr[j] - p) - mu : 0.0;
            xr[j] = wave_scan(z, lane);
            if (lane == kWave - 1) tot[j * NW + w] = xr[j];
        }
        __syncthreads();                                   // (and every read of the window is done)
        double run = 0.0;
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            if (j * NT >= W) break;
            double base = 0.0;
#pragma unroll
            for (int v = 0; v < NW; ++v) {
                if (v == w) base = run;
                run += tot[j * NW + v];
            }
            const int t = tid + j * NT;
            if (t < W) wr_win[lds_pad32(t)] = base + xr[j];
        }
        __syncthreads();

        for (int s = 0; s < S; ++s) {
            const int n = A.scales[s], nb = W / n;
            // (1 / n and 1 / sum (i - ibar)^2 once a scale: a division a box costs what five samples cost)
            const double rn = (double)n, ibar = 0.5 * (double)(n - 1);
            const double rinv = 1.0 / rn, sinv = 12.0 / (rn * (rn * rn - 1.0));
            // lanes a box: the largest power of two with g nb <= NT, a wave at the most
            int g = 1, lg = 0;
            while (2 * g * nb <= NT && g < kWave) {
                g *= 2;
                ++lg;
            }
            const int per = NT >> lg, r = tid & (g - 1), grp = tid >> lg;
            double acc = 0.0;
            for (int b0 = 0; b0 < nb; b0 += per) {         // (one round unless g = 1)
                const bool on = b0 + grp < nb;             // (a group without a box redoes the last one)
                const int t0 = (on ? b0 + grp : nb - 1) * n;
                const double y0 = wr_win[lds_pad32(t0)];
                double sy = 0.0, sxy = 0.0;
                for (int i = r; i < n; i += g) {
                    const double d = wr_win[lds_pad32(t0 + i)] - y0;
                    sy += d;
                    sxy += ((double)i - ibar) * d;
                }
                if (g > 1) {
                    sy = group_last(group_sum(sy, g), lane, g);
                    sxy = group_last(group_sum(sxy, g), lane, g);
                }
                const double ic = sy * rinv, sl = sxy * sinv;
                double rss = 0.0;
                for (int i = r; i < n; i += g) {
                    const double e = ((wr_win[lds_pad32(t0 + i)] - y0) - ic) - sl * ((double)i - ibar);
                    rss += e * e;
                }
                rss = group_sum(rss, g);
                acc += (on & (r == g - 1)) ? rss : 0.0;
            }
            acc = wave_sum63(acc);
            if (lane == kWave - 1) dred[s][w] = acc;
            if (tid == 0) sc[s] = n;
        }
    }
    __syncthreads();

    // one lane a k and one a scale: the logarithms
    const int pl_dfa = __builtin_popcount(mask & 7), pl_fl = __builtin_popcount(mask & 15);
    if (higuchi && tid < A.kmax) {
        const int k = tid + 1, q = (W - 1) / k, r = (W - 1) % k;
        double a0 = hred[tid][0][0], a1 = hred[tid][0][1];
#pragma unroll
        for (int j = 1; j < NW; ++j) {
            a0 += hred[tid][j][0];
            a1 += hred[tid][j][1];
        }
        const double rk = (double)k;
        const double lo = a0 / (double)q, hi = r < k - 1 ? a1 / (double)(q - 1) : 0.0;
        const double L = (lo + hi) * (double)(W - 1) / rk / rk / rk;
        hu[tid] = log(1.0 / rk);
        hv[tid] = L > 0.0 ? log(L) : __builtin_nan("");
    }
    if (tid < S) {
        double sum = dred[tid][0];
#pragma unroll
        for (int j = 1; j < NW; ++j) sum += dred[tid][j];
        const int n = sc[tid];
        const double F = sqrt(__builtin_fmax(sum, 0.0) / (double)((W / n) * n));
        if (mask & (1 << OSZ_WR_DFA_FLUCTUATIONS)) dst[(int64_t)(pl_fl + tid) * A.plane_pitch] = F;
        du[tid] = log((double)n);
        dv[tid] = F > 0.0 ? log(F) : __builtin_nan("");
    }
    __syncthreads();
    if (tid != 0) return;
    if (higuchi) dst[0] = wr_slope(hu, hv, A.kmax);
    if (mask & (1 << OSZ_WR_KATZ)) {
        double L = red[0][0], d = red[0][1];
#pragma unroll
        for (int j = 1; j < NW; ++j) {
            L += red[j][0];
            d = __builtin_fmax(d, red[j][1]);
        }
        dst[(int64_t)__builtin_popcount(mask & 1) * A.plane_pitch] = A.ln_n / (A.ln_n + log(d / L));
    }
    if (mask & (1 << OSZ_WR_PETROSIAN)) {
        int N = flips[0];
#pragma unroll
        for (int j = 1; j < NW; ++j) N += flips[j];
        const double Wd = (double)W;
        dst[(int64_t)__builtin_popcount(mask & 3) * A.plane_pitch] =
            A.log10_w / (A.log10_w + log10(Wd / (Wd + 0.4 * (double)N)));
    }
    if (mask & (1 << OSZ_WR_DFA)) dst[(int64_t)pl_dfa * A.plane_pitch] = wr_slope(du, dv, S);
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_window_fractal(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                       int kmax, const int *scales, int nscales, double *out, int64_t plane_pitch, int64_t row_pitch,
                       int64_t win0, void *stream) {
    static const WinRule rule = {"osz_window_fractal", "measure", OSZ_WR_COUNT, 8, OSZ_WR_LONGEST};
    const int planes = __builtin_popcount(mask & 15) + ((mask >> OSZ_WR_DFA_FLUCTUATIONS) & 1) * nscales;
    WrArgs A;
    if (int rc = win_head(rule, planes, x, pitch, nch, n, winsize, step, mask, out, plane_pitch, row_pitch, win0, A))
        return rc;
    const bool higuchi = (mask & (1 << OSZ_WR_HIGUCHI)) != 0;
    const bool dfa = (mask & (1 << OSZ_WR_DFA | 1 << OSZ_WR_DFA_FLUCTUATIONS)) != 0;
    OSZ_REQUIRE(!higuchi || (kmax >= 2 && kmax <= OSZ_WR_KMAX && winsize >= 2 * (int64_t)kmax),
                "osz_window_fractal: kmax=%d (2 .. %d, winsize=%lld >= 2 kmax)", kmax, OSZ_WR_KMAX, (long long)winsize);
    memset(A.scales, 0, sizeof A.scales);
    if (dfa) {
        OSZ_REQUIRE(scales && nscales >= 2 && nscales <= OSZ_WR_SCALES, "osz_window_fractal: %d scales (2 .. %d)",
                    nscales, OSZ_WR_SCALES);
        for (int s = 0; s < nscales; ++s) {
            OSZ_REQUIRE(scales[s] >= 4 && scales[s] <= winsize / 2 && (s == 0 || scales[s] > scales[s - 1]),
                        "osz_window_fractal: scale %d is %d (strictly increasing, 4 .. winsize / 2 = %lld)", s,
                        scales[s], (long long)(winsize / 2));
            A.scales[s] = scales[s];
        }
    }
    if (A.nwin == 0) return OSZ_OK;
    unsigned nblk;
    if (int rc = win_grid(rule, A, nch, nblk)) return rc;
    A.kmax = higuchi ? kmax : 2;
    A.nscale = dfa ? nscales : 0;
    A.ln_n = std::log((double)(winsize - 1));
    A.log10_w = std::log10((double)winsize);
    const size_t lds = (size_t)(winsize + kWrPad) * sizeof(double);
    hipStream_t st = as_stream(stream);
    KernelTimer timer("window_fractal", st);
    if (winsize >= OSZ_WR_WIDE) hipLaunchKernelGGL((window_fractal_kernel<256, 16>), dim3(nblk), dim3(256), lds, st, A);
    else hipLaunchKernelGGL((window_fractal_kernel<64, 8>), dim3(nblk), dim3(64), lds, st, A);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
