// window_block.h -- what the kernels with one workgroup per (channel, window) share: windowent,
// windowquant, windowfrac, windowwave and windowar (windowfeat, whose waves work through groups of
// windows, takes the host side only).  DESIGN.md section 4.
//
// Host side: WinHead, the arguments every such kernel reads, and win_head, the checks every entry
// point makes of them before anything else; an entry point keeps the checks of its own parameters
// and its dispatch.  Device side: win_where, a workgroup's window; win_fold, the sums about the
// pivot and the verdict on non-finite samples over the workgroup, behind ONE barrier; win_spoilt,
// NaN in every plane.  The pass that loads the window stays in each kernel: registers or LDS, the
// padding and a second moment differ on purpose.
#pragma once
#include "common.h"

namespace osz {

struct WinHead {
    const double *x;      // (nch, n) rows, row pitch `pitch`
    int64_t pitch, step;
    int64_t nwin;         // windows of this launch (per channel)
    int W, mask;
    double *out;          // already at the first window of this launch
    int64_t plane_pitch, row_pitch;
};

// an entry point's name, what it calls the bits of its mask ("feature", "measure") and how many
// there are, and the window lengths it takes
struct WinRule {
    const char *fn, *noun;
    int masks;
    int64_t shortest, longest;
};

// The common checks, in the order every entry point made them, and the head filled in: H.nwin
// says how many windows a row holds (0: nothing to launch).  `planes` is what the caller will
// write (it only words the message about the pitches: the caller checks its own parameters after
// this, with a mask and a window length it can rely on), `win0` the first window of `out` that is
// this launch's.
inline int win_head(const WinRule &R, int planes, const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize,
                    int64_t step, int mask, double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0,
                    WinHead &H) {
    OSZ_REQUIRE(x && out, "%s: null argument", R.fn);
    OSZ_REQUIRE(winsize >= R.shortest && winsize <= R.longest && step >= 1, "%s: winsize=%lld (%lld .. %lld) step=%lld (>= 1)",
                R.fn, (long long)winsize, (long long)R.shortest, (long long)R.longest, (long long)step);
    OSZ_REQUIRE(mask >= 1 && mask < (1 << R.masks), "%s: %s mask %d", R.fn, R.noun, mask);
    OSZ_REQUIRE(nch >= 1 && n >= 0 && pitch >= n && win0 >= 0, "%s: bad sizes (nch=%d n=%lld pitch=%lld)", R.fn, nch,
                (long long)n, (long long)pitch);
    const int64_t nwin = osz_window_count(n, winsize, step);
    OSZ_REQUIRE(row_pitch >= win0 + nwin && (nch == 1 || plane_pitch >= (int64_t)(nch - 1) * row_pitch + win0 + nwin) &&
                    plane_pitch >= win0 + nwin,
                "%s: the result's pitches (%lld, %lld) do not hold %d planes of %d rows of %lld + %lld windows", R.fn,
                (long long)plane_pitch, (long long)row_pitch, planes, nch, (long long)win0, (long long)nwin);
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 7) == 0,
                "%s: the arrays must be 8-byte aligned", R.fn);
    H.x = x;
    H.pitch = pitch;
    H.step = step;
    H.nwin = nwin;
    H.W = (int)winsize;
    H.mask = mask;
    H.out = out + win0;
    H.plane_pitch = plane_pitch;
    H.row_pitch = row_pitch;
    return OSZ_OK;
}

// One workgroup per (channel, window) on a one-dimensional grid: how many, fewer than 2^31.
inline int win_grid(const WinRule &R, const WinHead &H, int nch, unsigned &nblk) {
    OSZ_REQUIRE(H.nwin <= INT32_MAX / nch, "%s: %lld workgroups are too many for one launch", R.fn,
                (long long)H.nwin * nch);
    nblk = (unsigned)(H.nwin * nch);
    return OSZ_OK;
}

// the window of this workgroup and where its results go (plane 0)
struct WinAt {
    const double *row;
    double *dst;
};
__device__ __forceinline__ WinAt win_where(const WinHead &A) {
    // (the launch holds fewer than 2^31 workgroups, win_grid: a 32-bit division)
    const unsigned per_row = (unsigned)A.nwin;
    const int64_t c = blockIdx.x / per_row, kw = blockIdx.x % per_row;
    return {A.x + c * A.pitch + kw * A.step, A.out + c * A.row_pitch + kw};
}

// s[0 .. N), every thread's sums over its samples of the window, become the workgroup's -- the
// lanes by wave_sum63, lane 63 to LDS, one barrier, the waves added in wave order: the same bits
// in every thread -- and the return says whether any thread of the workgroup is `wild` (met a
// sample that spoils the window).  Uniform over the workgroup; every thread calls it once.
template <int NW, int N>
__device__ __forceinline__ bool win_fold(double (&s)[N], bool wild, int lane, int w) {
    __shared__ double sums[NW][N];
    __shared__ int bad[NW];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = wave_sum63(s[i]);
    const bool any = __ballot(wild) != 0ull;
    if (lane == kWave - 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) sums[w][i] = s[i];
        bad[w] = any;
    }
    __syncthreads();
    int wilds = bad[0];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = sums[0][i];
#pragma unroll
    for (int j = 1; j < NW; ++j) {
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] += sums[j][i];
        wilds |= bad[j];
    }
    return wilds != 0;
}

// a spoilt window: NaN in each of its `planes` planes (the whole workgroup of NT threads)
template <int NT>
__device__ __forceinline__ void win_spoilt(double *__restrict__ dst, int planes, int64_t plane_pitch, int tid) {
    for (int pl = tid; pl < planes; pl += NT) dst[(int64_t)pl * plane_pitch] = __builtin_nan("");
}

}  // namespace osz
