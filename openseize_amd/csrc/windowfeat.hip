// windowfeat.hip -- K15 time-resolved per-channel features (features/windowed.py window_features):
// for every window of W samples, step apart, of every channel the thirteen numbers of
// osz_window_feature -- mean, variance, rms, skewness, kurtosis, min, max, peak to peak, line
// length, zero crossings, the Hjorth mobility and complexity, the mean Teager energy -- from ONE
// read of the window.  DESIGN.md section 4, K15.
//
// A window's bits depend on W and its own W samples only:
//   * thread `tid` of the `nthreads` that share a window (64: one wave, for W < OSZ_WF_LONG; 256:
//     one workgroup, from there on) owns the samples tid + nthreads k of it and sums them in that
//     order, a wave 64 consecutive samples a trip; x[t - 1] and x[t - 2] come from the two lanes
//     below (the first two lanes of a wave re-read them: cache hits).  The window is addressed as a
//     raw buffer, whose range check stands in for every predicate on a load, and four trips' loads
//     are in flight at a time;
//   * the 64 lanes are folded in the fixed order of wave_sum63, the four waves of a workgroup in
//     wave order through LDS; nothing is atomic;
//   * the central moments are one-pass sums of y = x - p about a pivot p, the window's own first
//     sample (0 where that is not finite), the variances of the first and second differences
//     about their own first value likewise: an offset of the data cancels in y exactly.
// How many windows one wave or workgroup works through in turn (`group`, at most 64) is a matter of
// filling the chip: each window's folded sums are parked in lane g (wave kernel) or in LDS row g
// (workgroup kernel), and when the group is done the lanes turn the sums into the features side
// by side -- the divisions and square roots cost one lane's time for up to 64 windows -- and
// store 64 consecutive windows of a plane in one instruction.
#include "window_block.h"

namespace osz {

#pragma clang fp contract(off)        // every fused multiply-add below is written out

constexpr int kWfSums = 13;           // folded doubles per window (the crossings and the NaN flag beside them)

// the lane-private sums of one window
struct WfAcc {
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;      // sum y, y^2, y^3, y^4,  y = x - p
    double sxx = 0.0;                                    // sum x^2
    double mn = __builtin_inf(), mx = -__builtin_inf();
    double ll = 0.0;                                     // sum |dx|
    double d1 = 0.0, d2 = 0.0;                           // sum u, u^2,  u = dx - dx_0
    double e1 = 0.0, e2 = 0.0;                           // sum v, v^2,  v = ddx - ddx_0
    double tg = 0.0;                                     // sum x[t-1]^2 - x[t-2] x[t]
    int zc = 0;
    unsigned long long nan = 0ull;                       // lanes that met a NaN (the same in every lane)
};

struct WfPivot {
    double p, pd, pe;
};

__device__ __forceinline__ double finite_or_zero(double v) { return __builtin_isfinite(v) ? v : 0.0; }

// (every lane reads the same three samples: one request)
__device__ __forceinline__ WfPivot wf_pivot(const double *__restrict__ row) {
    const double x0 = row[0], x1 = row[1], x2 = row[2];
    WfPivot pv;
    pv.p = finite_or_zero(x0);
    pv.pd = finite_or_zero(x1 - x0);
    pv.pe = finite_or_zero((x2 - x1) - (x1 - x0));
    return pv;
}

// One sample per lane: a = x[t], xm1 = x[t - 1], xm2 = x[t - 2].  EDGE: the wave's trip holds samples
// outside [2, W) -- t < 1 has no difference, t < 2 no second difference, t >= W nothing -- and what
// they would add is replaced by +0.0, which changes no bit of a sum that started at +0.0.
template <bool EDGE>
__device__ __forceinline__ void wf_step(double a, double xm1, double xm2, int64_t t, int64_t W, const WfPivot pv,
                                        WfAcc &s) {
    const bool in = !EDGE || t < W, in1 = !EDGE || (in && t >= 1), in2 = !EDGE || (in && t >= 2);
    s.nan |= __ballot(a != a);                             // (a sample outside the window reads as 0)
    const double y = in ? a - pv.p : 0.0, y2 = y * y;
    s.s1 += y;
    s.s2 += y2;
    s.s3 = __builtin_fma(y2, y, s.s3);
    s.s4 = __builtin_fma(y2, y2, s.s4);
    s.sxx = __builtin_fma(a, a, s.sxx);
    s.mn = __builtin_fmin(s.mn, in ? a : s.mn);
    s.mx = __builtin_fmax(s.mx, in ? a : s.mx);
    const double d = in1 ? a - xm1 : 0.0, u = in1 ? d - pv.pd : 0.0;
    s.ll += __builtin_fabs(d);
    s.d1 += u;
    s.d2 = __builtin_fma(u, u, s.d2);
    s.zc += in1 && ((a < 0.0) != (xm1 < 0.0));
    const double v = in2 ? (d - (xm1 - xm2)) - pv.pe : 0.0;
    s.e1 += v;
    s.e2 = __builtin_fma(v, v, s.e2);
    s.tg += in2 ? __builtin_fma(-xm2, a, xm1 * xm1) : 0.0;
}

// The window as a raw buffer of W doubles: a load at a byte offset outside [0, 8 W) touches no
// memory and returns 0 (the hardware's range check, offsets in the vector operand only), so no
// load of a trip is predicated and the compiler is free to issue the loads of several trips at once.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wf_rsrc(const double *row, int64_t W) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(row), 0, (int)(W * 8), 0x00020000);
}

// A wave's trip at samples t0 .. t0 + 63: x[t - 1] and x[t - 2] come from the lanes below, those of
// the first two lanes from a two-lane load of x[t0 - 2], x[t0 - 1] (a cache hit: another trip's
// line).  The loads (wf_load) and their use (wf_trip) are apart so that several trips' loads can
// be in flight.
struct WfTrip {
    double a, h;          // the lane's sample; in lanes 0 and 1 x[t0 - 2] and x[t0 - 1]
};
__device__ __forceinline__ WfTrip wf_load(__amdgpu_buffer_rsrc_t rs, int64_t t0, int lane) {
    const unsigned at = (unsigned)(t0 + lane) * 8u;
    WfTrip r;
    r.a = buf_load(rs, at, 0);
    r.h = buf_load(rs, lane < 2 ? at - 16u : 0x80000000u, 0);
    return r;
}
template <bool EDGE>
__device__ __forceinline__ void wf_trip(const WfTrip r, int64_t t0, int lane, int64_t W, const WfPivot pv, WfAcc &s) {
    const double h1 = lane_of<1>(r.h);
    double xm1 = __shfl_up(r.a, 1, kWave), xm2 = __shfl_up(r.a, 2, kWave);
    if (lane == 0) xm1 = h1;
    if (lane < 2) xm2 = r.h;
    wf_step<EDGE>(r.a, xm1, xm2, t0 + lane, W, pv, s);
}

// Four trips whose last starts inside the window: their loads are issued before the first of them
// is used -- that, and the waves beside this one, is what hides the memory's latency.  The first
// trip is an edge when it is the window's first, the last may end past the window.
template <int NT, bool FIRST>
__device__ __forceinline__ void wf_quad(__amdgpu_buffer_rsrc_t rs, int64_t t0, int lane, int64_t W, const WfPivot pv,
                                        WfAcc &s) {
    const WfTrip r0 = wf_load(rs, t0, lane), r1 = wf_load(rs, t0 + NT, lane);
    const WfTrip r2 = wf_load(rs, t0 + 2 * NT, lane), r3 = wf_load(rs, t0 + 3 * NT, lane);
    wf_trip<FIRST>(r0, t0, lane, W, pv, s);
    wf_trip<false>(r1, t0 + NT, lane, W, pv, s);
    wf_trip<false>(r2, t0 + 2 * NT, lane, W, pv, s);
    wf_trip<true>(r3, t0 + 3 * NT, lane, W, pv, s);
}

// Thread tid's share of the window: samples tid, tid + NT, ...  Whole waves take every trip
// together (the shuffles need all 64 lanes).  (The callers hand over the head's 32-bit W > 0
// zero-extended: the upper half of every 64-bit compare with it is then a constant.)
template <int NT>
__device__ __forceinline__ void wf_accumulate(const double *__restrict__ row, int64_t W, int tid, int lane,
                                              const WfPivot pv, WfAcc &s) {
    const __amdgpu_buffer_rsrc_t rs = wf_rsrc(row, W);
    int64_t t0 = tid - lane;                               // the wave's first sample of a trip
    if (t0 == 0 && 3 * NT < W) {
        wf_quad<NT, true>(rs, t0, lane, W, pv, s);
        t0 += 4 * NT;
    }
    for (; t0 != 0 && t0 + 3 * NT < W; t0 += 4 * NT) wf_quad<NT, false>(rs, t0, lane, W, pv, s);
    for (; t0 < W; t0 += NT) wf_trip<true>(wf_load(rs, t0, lane), t0, lane, W, pv, s);
}

__device__ __forceinline__ int wave_isum63(int v) {
    v += __builtin_amdgcn_mov_dpp(v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x142, 0xF, 0xF, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x143, 0xF, 0xF, true);
    return v;
}

// min / max over the wave in every lane (exact in any order)
__device__ __forceinline__ double wave_min(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = __builtin_fmin(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = __builtin_fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// The wave's fold of a window in q[0 .. kWfSums) (the same in every lane), the crossings in zc,
// "holds a NaN" in nan.
__device__ __forceinline__ void wf_fold_wave(const WfAcc &s, double q[kWfSums], int &zc, bool &nan) {
    q[0] = lane63(wave_sum63(s.s1));
    q[1] = lane63(wave_sum63(s.s2));
    q[2] = lane63(wave_sum63(s.s3));
    q[3] = lane63(wave_sum63(s.s4));
    q[4] = lane63(wave_sum63(s.sxx));
    q[5] = wave_min(s.mn);
    q[6] = wave_max(s.mx);
    q[7] = lane63(wave_sum63(s.ll));
    q[8] = lane63(wave_sum63(s.d1));
    q[9] = lane63(wave_sum63(s.d2));
    q[10] = lane63(wave_sum63(s.e1));
    q[11] = lane63(wave_sum63(s.e2));
    q[12] = lane63(wave_sum63(s.tg));
    zc = __builtin_amdgcn_readlane(wave_isum63(s.zc), kWave - 1);
    nan = s.nan != 0ull;
}

// One window's features from its folded sums, stored where `mask` asks: plane p of the result is
// the p-th feature present in mask, in the order of osz_window_feature.
__device__ __forceinline__ void wf_finish(const double q[kWfSums], double zc, bool nan, const WfPivot pv, int64_t W,
                                          int mask, double *__restrict__ dst, int64_t plane_pitch) {
    const double rn = 1.0 / (double)W, rn1 = 1.0 / (double)(W - 1), rn2 = 1.0 / (double)(W - 2);
    const double mu = q[0] * rn, a2 = q[1] * rn, a3 = q[2] * rn, a4 = q[3] * rn;
    const double mu2 = mu * mu;
    const double m2 = a2 - mu2;
    const double m3 = (a3 - 3.0 * mu * a2) + 2.0 * mu * mu2;
    const double m4 = ((a4 - 4.0 * mu * a3) + 6.0 * mu2 * a2) - 3.0 * mu2 * mu2;
    const double du = q[8] * rn1, vd = q[9] * rn1 - du * du;
    const double eu = q[10] * rn2, ve = q[11] * rn2 - eu * eu;
    const double mob = sqrt(vd / m2);
    double f[OSZ_WF_COUNT];
    f[OSZ_WF_MEAN] = pv.p + mu;
    f[OSZ_WF_VAR] = m2;
    f[OSZ_WF_RMS] = sqrt(q[4] * rn);
    f[OSZ_WF_SKEW] = m3 / (m2 * sqrt(m2));
    f[OSZ_WF_KURTOSIS] = m4 / (m2 * m2);
    f[OSZ_WF_MIN] = q[5];
    f[OSZ_WF_MAX] = q[6];
    f[OSZ_WF_PTP] = q[6] - q[5];
    f[OSZ_WF_LINE_LENGTH] = q[7];
    f[OSZ_WF_ZERO_CROSSINGS] = zc;
    f[OSZ_WF_MOBILITY] = mob;
    f[OSZ_WF_COMPLEXITY] = sqrt(ve / vd) / mob;
    f[OSZ_WF_TEAGER] = q[12] * rn2;
    int p = 0;
#pragma unroll
    for (int k = 0; k < OSZ_WF_COUNT; ++k) {
        if (mask & (1 << k)) {
            dst[(int64_t)p * plane_pitch] = nan ? __builtin_nan("") : f[k];
            ++p;
        }
    }
}

struct WfArgs : WinHead {
    int64_t ngroups;      // ceil(nwin / group)
    int64_t ntasks;       // nch * ngroups
    int group;            // windows one wave / workgroup works through, 1 .. 64
};

// W < OSZ_WF_LONG: one wave per (channel, group of windows); four independent waves a workgroup.
__global__ void __launch_bounds__(256) window_wave_kernel(const WfArgs A) {
    const int lane = threadIdx.x & (kWave - 1);
    // (the wave's index read back as a scalar: everything derived from it, the window's buffer
    // descriptor first of all, is uniform for the compiler too)
    const int64_t task = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (task >= A.ntasks) return;                          // (whole waves leave)
    const int64_t c = task / A.ngroups, k0 = (task % A.ngroups) * A.group;
    const int64_t left = A.nwin - k0;
    const int cnt = left < A.group ? (int)left : A.group;
    const double *ch = A.x + c * A.pitch;
    double keep[kWfSums];
    double keep_zc = 0.0;
    bool keep_nan = false;
    WfPivot keep_pv = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kWfSums; ++j) keep[j] = 0.0;
    for (int g = 0; g < cnt; ++g) {
        const double *row = ch + (k0 + g) * A.step;
        const WfPivot pv = wf_pivot(row);
        WfAcc s;
        wf_accumulate<kWave>(row, (unsigned)A.W, lane, lane, pv, s);
        double q[kWfSums];
        int zc;
        bool nan;
        wf_fold_wave(s, q, zc, nan);
        if (lane == g) {
#pragma unroll
            for (int j = 0; j < kWfSums; ++j) keep[j] = q[j];
            keep_zc = (double)zc;
            keep_nan = nan;
            keep_pv = pv;
        }
    }
    if (lane < cnt)
        wf_finish(keep, keep_zc, keep_nan, keep_pv, A.W, A.mask, A.out + c * A.row_pitch + k0 + lane, A.plane_pitch);
}

// W >= OSZ_WF_LONG: one workgroup of 256 per (channel, group of windows).
__global__ void __launch_bounds__(256) window_block_kernel(const WfArgs A) {
    __shared__ double red[4][kWfSums + 2];
    __shared__ double fin[kWave][kWfSums + 2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t task = blockIdx.x;
    const int64_t c = task / A.ngroups, k0 = (task % A.ngroups) * A.group;
    const int64_t left = A.nwin - k0;
    const int cnt = left < A.group ? (int)left : A.group;
    const double *ch = A.x + c * A.pitch;
    for (int g = 0; g < cnt; ++g) {
        const double *row = ch + (k0 + g) * A.step;
        const WfPivot pv = wf_pivot(row);
        WfAcc s;
        wf_accumulate<256>(row, (unsigned)A.W, w * kWave + lane, lane, pv, s);
        double q[kWfSums];
        int zc;
        bool nan;
        wf_fold_wave(s, q, zc, nan);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < kWfSums; ++j) red[w][j] = q[j];
            red[w][kWfSums] = (double)zc;
            red[w][kWfSums + 1] = nan ? 1.0 : 0.0;
        }
        __syncthreads();
        if (tid < kWfSums + 2) {
            const double r0 = red[0][tid], r1 = red[1][tid], r2 = red[2][tid], r3 = red[3][tid];
            double v;
            if (tid == 5) v = __builtin_fmin(__builtin_fmin(r0, r1), __builtin_fmin(r2, r3));
            else if (tid == 6) v = __builtin_fmax(__builtin_fmax(r0, r1), __builtin_fmax(r2, r3));
            else v = ((r0 + r1) + r2) + r3;
            fin[g][tid] = v;
        }
        __syncthreads();
    }
    if (tid < cnt) {
        double q[kWfSums];
#pragma unroll
        for (int j = 0; j < kWfSums; ++j) q[j] = fin[tid][j];
        const WfPivot pv = wf_pivot(ch + (k0 + tid) * A.step);
        wf_finish(q, fin[tid][kWfSums], fin[tid][kWfSums + 1] != 0.0, pv, A.W, A.mask,
                  A.out + c * A.row_pitch + k0 + tid, A.plane_pitch);
    }
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_count(int64_t n, int64_t winsize, int64_t step) {
    if (n < 0 || winsize < 4 || step < 1) return -1;
    return n < winsize ? 0 : (n - winsize) / step + 1;
}

int osz_window_features(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                        double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0, void *stream) {
    static const WinRule rule = {"osz_window_features", "feature", OSZ_WF_COUNT, 4, OSZ_WF_LONGEST};
    WfArgs A;
    if (int rc = win_head(rule, __builtin_popcount(mask), x, pitch, nch, n, winsize, step, mask, out, plane_pitch,
                          row_pitch, win0, A))
        return rc;
    const int64_t nwin = A.nwin;
    if (nwin == 0) return OSZ_OK;
    const bool longw = winsize >= OSZ_WF_LONG;
    // windows per wave / workgroup: as many as 64 while the launch still fills the chip
    const int64_t want = longw ? 2048 : 8192;
    int group = 64;
    while (group > 1 && nch * ((nwin + group - 1) / group) < want) group >>= 1;
    A.ngroups = (nwin + group - 1) / group;
    A.ntasks = nch * A.ngroups;
    A.group = group;
    const int64_t nblk = longw ? A.ntasks : (A.ntasks + 3) / 4;
    OSZ_REQUIRE(nblk <= INT32_MAX, "osz_window_features: %lld workgroups are too many for one launch", (long long)nblk);
    hipStream_t st = as_stream(stream);
    KernelTimer timer("window_features", st);
    if (longw) hipLaunchKernelGGL(window_block_kernel, dim3((unsigned)nblk), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(window_wave_kernel, dim3((unsigned)nblk), dim3(256), 0, st, A);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
