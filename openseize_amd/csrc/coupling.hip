// coupling.hip -- the two hot loops of PhaseLock (experimental/coupling/estimators.py):
// selecting the samples whose analytic phase lies in a band, and the windowed power sums
// around those samples and around every shifted (surrogate) copy of them.
//
// Reference call sites replaced (src/openseize/experimental/coupling/estimators.py):
//   :172-177 index()'s per-chunk np.flatnonzero of the phase test;
//   :200-230 _avg(), run once for the real indices and once per surrogate (:289-292).
//
// osz_phase_index: count / scan / scatter over a fixed partition of the chunk (at most
// kPiMaxBlk blocks), so the positions come out in order and the same on every run.
//
// osz_lock_accumulate: a workgroup owns (set s, a tile of kLockTile consecutive window
// offsets k).  Set s's sorted positions q' split into an unwrapped and a wrapped range;
// binary searches trim each range to the positions whose whole window [q' - ceil(W/2),
// q' + floor(W/2)) lies in the chunk.  The workgroup walks the positions in order in
// batches whose span fits an LDS segment of p = amp^2: the segment is loaded once per batch
// (squared on load) and every thread adds, for each position of the batch, the segment
// values at its kLockPer offsets.  Each (s, k) is owned by one thread and summed in index
// order, then added to the persistent accumulator: no atomics on floating-point data.
#include "common.h"

namespace osz {

constexpr int kPiThreads = 256;
constexpr int kPiMaxBlk = 1024;

__device__ __forceinline__ bool in_band(const double2 *z, int64_t i, double lo, double hi) {
    const double p = phase_2pi(z[i]);
    return p > lo && p < hi;
}

// blkcnt[b] = number of samples in [b * span, (b + 1) * span) that pass
__global__ __launch_bounds__(kPiThreads) void phase_count_kernel(const double2 *__restrict__ z,
                                                                 int64_t n, int64_t span, double lo,
                                                                 double hi,
                                                                 int64_t *__restrict__ blkcnt) {
    __shared__ int64_t wsum[kPiThreads / 64];
    const int64_t a = (int64_t)blockIdx.x * span;
    const int64_t b = a + span < n ? a + span : n;
    int64_t c = 0;
    for (int64_t i = a + threadIdx.x; i < b; i += kPiThreads) c += in_band(z, i, lo, hi);
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int w = 0; w < kPiThreads / 64; ++w) t += wsum[w];
        blkcnt[blockIdx.x] = t;
    }
}

// exclusive scan of blkcnt[0, nblk) into blkoff, the total into *total (one block)
__global__ __launch_bounds__(kPiMaxBlk) void phase_scan_kernel(const int64_t *__restrict__ blkcnt,
                                                               int nblk,
                                                               int64_t *__restrict__ blkoff,
                                                               int64_t *__restrict__ total) {
    __shared__ int64_t wsum[kPiMaxBlk / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t v = t < nblk ? blkcnt[t] : 0;
    int64_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t u = __shfl_up(incl, off, 64);
        if (lane >= off) incl += u;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int64_t before = 0;
    for (int q = 0; q < w; ++q) before += wsum[q];
    if (t < nblk) blkoff[t] = before + incl - v;
    if (t == kPiMaxBlk - 1) *total = before + incl;
}

// out[blkoff[b] + rank] = i for every passing sample i of block b, in order
__global__ __launch_bounds__(kPiThreads) void phase_scatter_kernel(
    const double2 *__restrict__ z, int64_t n, int64_t span, double lo, double hi,
    const int64_t *__restrict__ blkoff, int64_t *__restrict__ out) {
    __shared__ int wcnt[kPiThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t a = (int64_t)blockIdx.x * span;
    const int64_t b = a + span < n ? a + span : n;
    int64_t base = blkoff[blockIdx.x];
    for (int64_t i0 = a; i0 < b; i0 += kPiThreads) {
        const int64_t i = i0 + threadIdx.x;
        const bool pass = i < b && in_band(z, i, lo, hi);
        const uint64_t m = __ballot(pass);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int q = 0; q < kPiThreads / 64; ++q) {
            before += q < w ? wcnt[q] : 0;
            all += wcnt[q];
        }
        if (pass) out[base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += all;
        __syncthreads();
    }
}

constexpr int kLockThreads = 512;
constexpr int kLockPer = 4;                                // offsets k per thread
constexpr int kLockTile = kLockThreads * kLockPer;         // offsets per workgroup
constexpr int kLockSeg = 8192;                             // p segment in LDS: 64 KiB
constexpr int kLockSpan = kLockSeg - kLockTile;            // largest q' span of a batch
constexpr int kLockQ = kLockThreads;                       // positions staged per round

// first position in [lo, hi) of the sorted idx with idx[i] >= v
__device__ int64_t lower_bound(const int64_t *idx, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (idx[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kLockThreads) void lock_accumulate_kernel(
    const double *__restrict__ amp, int64_t L, const int64_t *__restrict__ idx, int64_t nidx,
    const int64_t *__restrict__ shifts, int64_t max_shift, int64_t W, double *__restrict__ sums,
    int64_t ldsums, int64_t *__restrict__ counts) {
    __shared__ double seg[kLockSeg];
    __shared__ int64_t qs[kLockQ];
    __shared__ int64_t bounds[4];
    __shared__ int jend;
    const int t = threadIdx.x;
    const int s = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * kLockTile;
    const int64_t h = (W + 1) / 2;                 // ceil(W / 2): window starts at q' - h
    const int64_t qmax = L - W + h;                // last q' whose window ends inside the chunk
    const int64_t sigma = s == 0 ? 0 : shifts[s - 1];
    // range 0: q' = q + sigma (q < max_shift - sigma); range 1: q' = q + sigma - max_shift
    const int64_t off0 = sigma, off1 = sigma - max_shift;
    if (t == 0) {
        const int64_t split = s == 0 ? nidx : lower_bound(idx, 0, nidx, max_shift - sigma);
        int64_t a0 = 0, b0 = 0, a1 = split, b1 = split;
        if (qmax >= h) {
            a0 = lower_bound(idx, 0, split, h - off0);
            b0 = lower_bound(idx, a0, split, qmax + 1 - off0);
            a1 = lower_bound(idx, split, nidx, h - off1);
            b1 = lower_bound(idx, a1, nidx, qmax + 1 - off1);
        }
        bounds[0] = a0;
        bounds[1] = b0;
        bounds[2] = a1;
        bounds[3] = b1;
        if (blockIdx.x == 0) counts[s] += (b0 - a0) + (b1 - a1);
    }
    __syncthreads();
    const int kn = (int)(W - k0 < kLockTile ? W - k0 : kLockTile);
    double acc[kLockPer];
#pragma unroll
    for (int r = 0; r < kLockPer; ++r) acc[r] = 0.0;

    for (int rg = 0; rg < 2; ++rg) {
        const int64_t a = bounds[2 * rg], b = bounds[2 * rg + 1];
        const int64_t off = rg == 0 ? off0 : off1;
        for (int64_t i0 = a; i0 < b; i0 += kLockQ) {
            const int nq = (int)(b - i0 < kLockQ ? b - i0 : kLockQ);
            __syncthreads();
            if (t < nq) qs[t] = idx[i0 + t] + off;
            __syncthreads();
            int j0 = 0;
            while (j0 < nq) {
                const int64_t base = qs[j0];
                if (t == 0) jend = nq;
                __syncthreads();
                // the batch ends at the first position outside [base, base + kLockSpan)
                if (t > j0 && t < nq) {
                    const int64_t d = qs[t] - base;
                    if (d < 0 || d >= kLockSpan) atomicMin(&jend, t);
                }
                __syncthreads();
                const int j1 = jend;
                const int64_t seg0 = base - h + k0;
                const int len = (int)(qs[j1 - 1] - base) + kn;
                for (int e = t; e < len; e += kLockThreads) {
                    const int64_t pos = seg0 + e;
                    const double v = pos >= 0 && pos < L ? amp[pos] : 0.0;
                    seg[e] = v * v;
                }
                __syncthreads();
                for (int j = j0; j < j1; ++j) {
                    const int64_t q = qs[j];
                    if (q < h || q > qmax) continue;      // (only for unsorted input)
                    const int d = (int)(q - base);
#pragma unroll
                    for (int r = 0; r < kLockPer; ++r) {
                        const int kk = t + r * kLockThreads;
                        if (kk < kn) acc[r] += seg[d + kk];
                    }
                }
                __syncthreads();
                j0 = j1;
            }
        }
    }
    double *row = sums + (int64_t)s * ldsums + k0;
#pragma unroll
    for (int r = 0; r < kLockPer; ++r) {
        const int kk = t + r * kLockThreads;
        if (kk < kn) row[kk] += acc[r];
    }
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_phase_index(const double *z, int64_t n, double lo, double hi, int64_t *work,
                    int64_t *out, int64_t *count, void *stream) {
    OSZ_REQUIRE(work && count && (n == 0 || (z && out)), "osz_phase_index: null argument");
    OSZ_REQUIRE(n >= 0, "osz_phase_index: n=%lld", (long long)n);
    hipStream_t st = as_stream(stream);
    *count = 0;
    if (n == 0) return OSZ_OK;
    int64_t span = (n + kPiMaxBlk - 1) / kPiMaxBlk;
    if (span < 16 * kPiThreads) span = 16 * kPiThreads;
    span = (span + kPiThreads - 1) / kPiThreads * kPiThreads;
    const int nblk = (int)((n + span - 1) / span);
    const double2 *zc = reinterpret_cast<const double2 *>(z);
    int64_t *blkcnt = work, *blkoff = work + kPiMaxBlk, *total = work + 2 * kPiMaxBlk;
    {
        KernelTimer kt("phase_index", st);
        hipLaunchKernelGGL(phase_count_kernel, dim3(nblk), dim3(kPiThreads), 0, st, zc, n, span, lo,
                           hi, blkcnt);
        OSZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(phase_scan_kernel, dim3(1), dim3(kPiMaxBlk), 0, st, blkcnt, nblk, blkoff,
                           total);
        OSZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(phase_scatter_kernel, dim3(nblk), dim3(kPiThreads), 0, st, zc, n, span, lo,
                           hi, blkoff, out);
        OSZ_HIP(hipGetLastError());
    }
    OSZ_HIP(hipMemcpyAsync(count, total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    OSZ_HIP(hipStreamSynchronize(st));
    return OSZ_OK;
}

int osz_lock_accumulate(const double *amp, int64_t L, const int64_t *idx, int64_t nidx,
                        const int64_t *shifts, int nsur, int64_t max_shift, int64_t W, double *sums,
                        int64_t ldsums, int64_t *counts, void *stream) {
    OSZ_REQUIRE(sums && counts && (L == 0 || amp) && (nidx == 0 || idx) && (nsur == 0 || shifts),
                "osz_lock_accumulate: null argument");
    OSZ_REQUIRE(L >= 0 && nidx >= 0 && nsur >= 0 && nsur < 65535 && max_shift >= 1 && W >= 1 &&
                    ldsums >= W,
                "osz_lock_accumulate: bad sizes (L=%lld nidx=%lld nsur=%d max_shift=%lld W=%lld)",
                (long long)L, (long long)nidx, nsur, (long long)max_shift, (long long)W);
    hipStream_t st = as_stream(stream);
    const int64_t ntile = (W + kLockTile - 1) / kLockTile;
    OSZ_REQUIRE(ntile <= 0x7fffffff, "osz_lock_accumulate: W=%lld too large", (long long)W);
    KernelTimer kt("lock_accumulate", st);
    hipLaunchKernelGGL(lock_accumulate_kernel, dim3((unsigned)ntile, (unsigned)(nsur + 1)),
                       dim3(kLockThreads), 0, st, amp, L, idx, nidx, shifts, max_shift, W, sums,
                       ldsums, counts);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
