// windowquant.hip -- K17 order statistics per window (features/quantiles.py window_quantiles):
// for every window of W samples, step apart, of every channel the numbers of
// osz_window_quantiles_measure -- median, median absolute deviation, quantiles -- where K15's
// features are sums and K16's pattern counts.  DESIGN.md section 4, K17.
//
// One workgroup per (channel, window) on a one-dimensional grid -- one wave for W <= OSZ_WQ_WAVE,
// 256 threads above -- sorts the window on chip:
//   * the window is read once; a sample becomes a 64-bit key whose unsigned order is the total
//     order of the doubles (all bits of a negative value flipped, the sign bit of the others:
//     -0.0 < +0.0 without a special case); the same pass takes the ballot for NaN.  The window is
//     padded to Wpad, the power of two at or above max(W, OSZ_WQ_NARROWEST), with the largest key;
//     a thread holds K = Wpad / NT keys in registers, one kernel instance per Wpad;
//   * a bitonic network sorts element t K + r (thread t, register r).  A compare-exchange whose
//     partner is in the same thread (distance < K) runs in registers; a partner in the same wave
//     comes by a cross-lane move -- DPP quad_perm for lane ^ 1 and ^ 2, row_ror:8 for ^ 8,
//     ds_swizzle for ^ 4 and ^ 16, v_permlane32_swap for ^ 32; only the three stages of a
//     256-thread sort whose partner is in another wave go through LDS, two barriers each.  Which
//     sample starts where does not matter to a sort, so the load is the coalesced one;
//   * the sorted keys go to LDS once; median and quantiles are reads of at most two keys each.
//     For the mad the registers -- the sorted samples -- are replaced by the keys of
//     |x - median| and the same network runs again (the loop below: the network is emitted once).
// A key compares as an integer, every measure is a selection followed by at most four IEEE
// operations: a window's bits depend on W, q and its own samples only.
#include "window_block.h"

namespace osz {

#pragma clang fp contract(off)

typedef unsigned long long wq_key;
constexpr wq_key kWqSign = 1ull << 63;
constexpr wq_key kWqPad = ~0ull;          // above every key of a window without NaN (it is the key of a NaN)

static_assert(OSZ_WQ_NARROWEST == kWave && OSZ_WQ_WAVE == 8 * kWave && OSZ_WQ_LONGEST == 16 * 256 &&
                  OSZ_WQ_QMOST <= kWave,
              "window_quantiles_kernel");

struct WqArgs : WinHead {
    int nq;
    int lo[OSZ_WQ_QMOST];       // floor(q (W - 1))
    double g[OSZ_WQ_QMOST];     // q (W - 1) - lo
};

__device__ __forceinline__ wq_key wq_encode(double v) {
    const wq_key b = __builtin_bit_cast(wq_key, v);
    return (b & kWqSign) ? ~b : b ^ kWqSign;
}

__device__ __forceinline__ double wq_decode(wq_key k) {
    return __builtin_bit_cast(double, (k & kWqSign) ? k ^ kWqSign : ~k);
}

// v of lane `lane ^ M`
template <int M>
__device__ __forceinline__ unsigned wq_xor32(unsigned v, int lane) {
    if constexpr (M == 1) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);        // quad_perm:[1,0,3,2]
    else if constexpr (M == 2) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);   // quad_perm:[2,3,0,1]
    else if constexpr (M == 8) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);  // row_ror:8
    else if constexpr (M == 4 || M == 16) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (M << 10) | 0x1F);
    else {
        static_assert(M == 32, "wq_xor32");
        // lanes 32 .. 63 of the first result take lanes 0 .. 31 of v, lanes 0 .. 31 of the second
        // lanes 32 .. 63
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return lane < 32 ? r[1] : r[0];
    }
}

template <int M>
__device__ __forceinline__ wq_key wq_xor(wq_key v, int lane) {
    const unsigned lo = wq_xor32<M>((unsigned)v, lane), hi = wq_xor32<M>((unsigned)(v >> 32), lane);
    return ((wq_key)hi << 32) | lo;
}

// (equal keys are the same bits: which of the two a side keeps makes no difference)
__device__ __forceinline__ void wq_cswap(wq_key &a, wq_key &b, bool asc) {
    const bool sw = (a > b) == asc;
    const wq_key lo = sw ? b : a, hi = sw ? a : b;
    a = lo;
    b = hi;
}

// the stages of distance K / 2 .. 1 of a merge: both partners in this thread
template <int K>
__device__ __forceinline__ void wq_merge_regs(wq_key (&a)[K], bool asc) {
#pragma unroll
    for (int j = K / 2; j >= 1; j >>= 1)
#pragma unroll
        for (int r = 0; r < K; ++r)
            if ((r & j) == 0) wq_cswap(a[r], a[r | j], asc);
}

// one stage whose partner is lane ^ M: this side keeps the larger key when keepmax
template <int M, int K>
__device__ __forceinline__ void wq_stage_lanes(wq_key (&a)[K], bool keepmax, int lane) {
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const wq_key b = wq_xor<M>(a[r], lane);
        a[r] = ((b < a[r]) != keepmax) ? b : a[r];
    }
}

// one stage whose partner is thread `other` of another wave
template <int NT, int K>
__device__ __forceinline__ void wq_stage_waves(wq_key (&a)[K], wq_key *keys, int t, int other, bool keepmax) {
    __syncthreads();                                       // (the reads of what was there)
#pragma unroll
    for (int r = 0; r < K; ++r) keys[r * NT + t] = a[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const wq_key b = keys[r * NT + other];
        a[r] = ((b < a[r]) != keepmax) ? b : a[r];
    }
}

// Ascending over the elements t K + r.  The blocks of k elements of a bitonic sort alternate in
// direction, the last one, of all NT K, ascends.
template <int NT, int K>
__device__ __forceinline__ void wq_sort(wq_key (&a)[K], wq_key *keys, int t, int lane) {
#pragma unroll
    for (int k = 2; k <= K; k <<= 1)
#pragma unroll
        for (int j = k / 2; j >= 1; j >>= 1)
#pragma unroll
            for (int r = 0; r < K; ++r)
                if ((r & j) == 0) wq_cswap(a[r], a[r | j], k < K ? (r & k) == 0 : (t & 1) == 0);
#pragma nounroll
    for (int kk = 2; kk <= NT; kk <<= 1) {                 // blocks of kk threads
        const bool asc = (t & kk) == 0;
#pragma nounroll
        for (int m = kk >> 1; m >= 1; m >>= 1) {
            const bool keepmax = ((t & m) != 0) == asc;
            switch (m) {
            case 1: wq_stage_lanes<1, K>(a, keepmax, lane); break;
            case 2: wq_stage_lanes<2, K>(a, keepmax, lane); break;
            case 4: wq_stage_lanes<4, K>(a, keepmax, lane); break;
            case 8: wq_stage_lanes<8, K>(a, keepmax, lane); break;
            case 16: wq_stage_lanes<16, K>(a, keepmax, lane); break;
            case 32: wq_stage_lanes<32, K>(a, keepmax, lane); break;
            default:
                if constexpr (NT > kWave) wq_stage_waves<NT, K>(a, keys, t, t ^ m, keepmax);
                break;
            }
        }
        wq_merge_regs<K>(a, asc);
    }
}

// element i of the sorted window as publish left it
template <int NT, int K>
__device__ __forceinline__ double wq_rank(const wq_key *keys, int i) {
    return wq_decode(keys[(i % K) * NT + i / K]);
}

template <int NT, int K>
__device__ __forceinline__ double wq_median(const wq_key *keys, int W) {
    return (wq_rank<NT, K>(keys, (W - 1) / 2) + wq_rank<NT, K>(keys, W / 2)) / 2.0;
}

template <int NT, int K>
__global__ void __launch_bounds__(NT) window_quantiles_kernel(const WqArgs A) {
    constexpr int NW = NT / kWave;
    __shared__ wq_key keys[NT * K];
    __shared__ int bad[NW];
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int W = A.W;
    const WinAt at = win_where(A);
    const double *__restrict__ row = at.row;
    double *__restrict__ dst = at.dst;
    const bool want_median = A.mask & (1 << OSZ_WQ_MEDIAN), want_mad = A.mask & (1 << OSZ_WQ_MAD);
    const int nq = (A.mask & (1 << OSZ_WQ_QUANTILE)) ? A.nq : 0;
    const int p_mad = want_median ? 1 : 0, p_q = p_mad + (want_mad ? 1 : 0);

    // the window, coalesced; the ballot for NaN (an infinity sorts like any value, and there is no
    // sum to fold: not win_fold)
    wq_key a[K];
    bool wild = false;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int e = r * NT + t;
        a[r] = kWqPad;
        if (e < W) {
            const double v = row[e];
            wild |= v != v;
            a[r] = wq_encode(v);
        }
    }
    bool any = __ballot(wild) != 0ull;
    if constexpr (NW > 1) {
        if (lane == 0) bad[t >> 6] = any;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NW; ++j) any |= bad[j] != 0;
    }
    if (any) {                                             // (the whole workgroup)
        win_spoilt<NT>(dst, p_q + nq, A.plane_pitch, t);
        return;
    }

#pragma nounroll
    for (int pass = 0;; ++pass) {
        wq_sort<NT, K>(a, keys, t, lane);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < K; ++r) keys[r * NT + t] = a[r];
        __syncthreads();
        const double med = wq_median<NT, K>(keys, W);
        if (pass == 1) {
            if (t == 0) dst[(int64_t)p_mad * A.plane_pitch] = med;
            return;
        }
        if (t == 0 && want_median) dst[0] = med;
        if (t < nq) {
            const int lo = A.lo[t], hi = lo + 1 < W ? lo + 1 : W - 1;
            const double g = A.g[t], s = wq_rank<NT, K>(keys, lo), b = wq_rank<NT, K>(keys, hi);
            double v = s;
            if (s != b) {
                const double d = b - s;
                v = g < 0.5 ? s + d * g : b - d * (1.0 - g);
            }
            dst[(int64_t)(p_q + t) * A.plane_pitch] = v;
        }
        if (!want_mad) return;
        if (!__builtin_isfinite(med)) {                    // inf - inf: the deviations hold a NaN
            if (t == 0) dst[(int64_t)p_mad * A.plane_pitch] = __builtin_nan("");
            return;
        }
        // the sorted window is in the registers, element t K + r; the pad stays the pad
#pragma unroll
        for (int r = 0; r < K; ++r)
            if (t * K + r < W) a[r] = wq_encode(__builtin_fabs(wq_decode(a[r]) - med));
    }
}

template <int NT, int K>
static void wq_launch(const WqArgs &A, unsigned nblk, hipStream_t st) {
    hipLaunchKernelGGL((window_quantiles_kernel<NT, K>), dim3(nblk), dim3(NT), 0, st, A);
}

// osz_window_quantiles on a stream, timed under the caller's label (pair_window.h: K25 takes its bin
// edges from here)
int wq_quantiles(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                 const double *q, int nq, double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0,
                 const char *label, hipStream_t st) {
    static const WinRule rule = {"osz_window_quantiles", "measure", OSZ_WQ_COUNT, 4, OSZ_WQ_LONGEST};
    const int planes = __builtin_popcount(mask & 3) + ((mask >> OSZ_WQ_QUANTILE) & 1) * nq;
    WqArgs A;
    if (int rc = win_head(rule, planes, x, pitch, nch, n, winsize, step, mask, out, plane_pitch, row_pitch, win0, A))
        return rc;
    const bool quant = (mask & (1 << OSZ_WQ_QUANTILE)) != 0;
    OSZ_REQUIRE(!quant || (q && nq >= 1 && nq <= OSZ_WQ_QMOST), "osz_window_quantiles: %d quantiles (1 .. %d)%s", nq,
                OSZ_WQ_QMOST, quant && !q ? ", q is null" : "");
    A.nq = quant ? nq : 0;
    for (int j = 0; j < OSZ_WQ_QMOST; ++j) {
        A.lo[j] = 0;
        A.g[j] = 0.0;
    }
    for (int j = 0; j < A.nq; ++j) {
        OSZ_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0, "osz_window_quantiles: q[%d]=%g is not in [0, 1]", j, q[j]);
        const double h = q[j] * (double)(winsize - 1), lo = __builtin_floor(h);
        A.lo[j] = (int)lo;
        A.g[j] = h - lo;
    }
    if (A.nwin == 0) return OSZ_OK;
    unsigned nblk;
    if (int rc = win_grid(rule, A, nch, nblk)) return rc;
    int wpad = OSZ_WQ_NARROWEST;
    while (wpad < winsize) wpad <<= 1;
    KernelTimer timer(label, st);
    switch (wpad) {                                        // up to OSZ_WQ_WAVE one wave, 256 threads above
    case 64: wq_launch<64, 1>(A, nblk, st); break;
    case 128: wq_launch<64, 2>(A, nblk, st); break;
    case 256: wq_launch<64, 4>(A, nblk, st); break;
    case 512: wq_launch<64, 8>(A, nblk, st); break;
    case 1024: wq_launch<256, 4>(A, nblk, st); break;
    case 2048: wq_launch<256, 8>(A, nblk, st); break;
    default: wq_launch<256, 16>(A, nblk, st); break;
    }
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_window_quantiles(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                         const double *q, int nq, double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0,
                         void *stream) {
    return wq_quantiles(x, pitch, nch, n, winsize, step, mask, q, nq, out, plane_pitch, row_pitch, win0,
                        "window_quantiles", as_stream(stream));
}

}  // extern "C"
