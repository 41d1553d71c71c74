// cross.hip -- K10 Welch cross-spectra over all channel pairs: the raw sums
// acc[i, j, f] += sum_s conj(X[s, i, f]) X[s, j, f] (i <= j) of the segment spectra a
// SPEC_DFT_SEGMENTS push wrote, and the finishing pass (mean, one-sided doubling, Hermitian
// mirror, or the magnitude-squared coherence).  DESIGN.md section 3, K10.
#include "common.h"

namespace osz {

typedef double cx __attribute__((ext_vector_type(2)));   // (re, im) of one complex128

constexpr int kCrossT = 4;                    // channels per side of a lane's register tile
constexpr int kCrossW = 4;                    // waves per side of a workgroup's tile
constexpr int kCrossB = kCrossT * kCrossW;    // channels per side of a workgroup's tile (16)
constexpr int kCrossThreads = kWave * kCrossW * kCrossW;   // 1024

// A lane is a frequency bin (nfreq is the fastest axis of X: a wave's load of one channel is
// 64 consecutive complex128, 16 B per lane), so the update at a bin never crosses lanes.  A
// workgroup owns 64 bins of a 16 x 16 block of channel pairs (block row <= block column); its
// 16 waves form a 4 x 4 grid and every lane keeps a 4 x 4 tile of complex sums in registers
// (64 VGPRs), walking the segments in order from the stored sum -- so the result does not
// depend on where the stream is cut into pushes, and nothing is atomic.  Per segment the
// workgroup needs 16 + 16 channel rows of 64 bins (32 KB): wave w fetches rows w of both sets
// (coalesced, once per workgroup instead of once per wave that uses them) one segment ahead
// of the arithmetic into registers, and hands them over through a double-buffered LDS stage,
// one barrier per segment.  Every wave then reads its 4 + 4 rows back as ds_read_b128 of
// consecutive lanes (conflict-free) for 16 complex multiply-adds = 64 FMAs.
// Grid: x = triangular block index (fastest: the workgroups resident together work on the
// same bins of different channel blocks and share the segment's rows in L2), y = bin block.
__global__ void __launch_bounds__(kCrossThreads)
cross_accumulate_kernel(const cx *__restrict__ X, int nseg, int nch, int nfreq, cx *__restrict__ acc,
                        int nblk) {
    __shared__ cx stage[2][2 * kCrossB][kWave];          // 64 KB
    int bi = 0, p = blockIdx.x;
    while (p >= nblk - bi) {                             // row bi of the triangle holds nblk - bi blocks
        p -= nblk - bi;
        ++bi;
    }
    const int bj = bi + p;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int wi = w / kCrossW, wj = w % kCrossW;
    const int f = blockIdx.y * kWave + lane;
    const bool inside = f < nfreq;
    // the two rows this wave stages
    const int ci = bi * kCrossB + w, cj = bj * kCrossB + w;
    const bool li = inside && ci < nch, lj = inside && cj < nch;
    // (a uniform base that moves from segment to segment plus a 32-bit offset per lane)
    const int64_t seg = (int64_t)nch * nfreq;
    const int oi = li ? ci * nfreq + f : 0, oj = lj ? cj * nfreq + f : 0;
    // the 4 x 4 pairs this lane sums; on a diagonal block the waves below the diagonal rest
    const int i0 = bi * kCrossB + wi * kCrossT, j0 = bj * kCrossB + wj * kCrossT;
    const bool active = i0 < nch && j0 < nch && (bi != bj || wi <= wj);
    const cx zero = {0.0, 0.0};

    cx sum[kCrossT][kCrossT];
#pragma unroll
    for (int a = 0; a < kCrossT; ++a)
#pragma unroll
        for (int b = 0; b < kCrossT; ++b) {
            const int i = i0 + a, j = j0 + b;
            sum[a][b] = (active && inside && j < nch && i <= j) ? acc[((int64_t)i * nch + j) * nfreq + f] : zero;
        }

    cx gi = li ? X[oi] : zero, gj = lj ? X[oj] : zero;
    stage[0][w][lane] = gi;
    stage[0][kCrossB + w][lane] = gj;
    __syncthreads();
    for (int s = 0; s < nseg; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < nseg;
        if (more) {
            X += seg;
            gi = li ? X[oi] : zero;
            gj = lj ? X[oj] : zero;
        }
        if (active) {
            cx u[kCrossT], v[kCrossT];
#pragma unroll
            for (int a = 0; a < kCrossT; ++a) u[a] = stage[cur][wi * kCrossT + a][lane];
#pragma unroll
            for (int b = 0; b < kCrossT; ++b) v[b] = stage[cur][kCrossB + wj * kCrossT + b][lane];
#pragma unroll
            for (int a = 0; a < kCrossT; ++a)
#pragma unroll
                for (int b = 0; b < kCrossT; ++b) {
                    // conj(u) v = (ur vr + ui vi) + i (ur vi - ui vr), four FMAs in a fixed order
                    double re = sum[a][b].x, im = sum[a][b].y;
                    re = __builtin_fma(u[a].x, v[b].x, re);
                    re = __builtin_fma(u[a].y, v[b].y, re);
                    im = __builtin_fma(u[a].x, v[b].y, im);
                    im = __builtin_fma(-u[a].y, v[b].x, im);
                    sum[a][b].x = re;
                    sum[a][b].y = im;
                }
        }
        if (more) {
            stage[cur ^ 1][w][lane] = gi;
            stage[cur ^ 1][kCrossB + w][lane] = gj;
        }
        __syncthreads();
    }

    if (active && inside) {
#pragma unroll
        for (int a = 0; a < kCrossT; ++a)
#pragma unroll
            for (int b = 0; b < kCrossT; ++b) {
                const int i = i0 + a, j = j0 + b;
                if (j < nch && i <= j) acc[((int64_t)i * nch + j) * nfreq + f] = sum[a][b];
            }
    }
}

// One (i <= j) pair per (blockIdx.z, blockIdx.y), a lane per bin; writes [i, j] and its mirror
// [j, i].  Spectrum: mean over the count, bins other than DC (and Nyquist for even nfft) doubled,
// the mirror conjugated, the diagonal's imaginary part set to 0 (the fused multiply-adds of the
// sum leave a residue there; the definition's ab - ba does not).  `out` may be `acc` itself: a
// pair is read by the one lane that writes it.  Coherence: |S_ij|^2 / (S_ii S_jj) from the raw
// sums (the count, the scaling and the doubling cancel), real.
__global__ void __launch_bounds__(256)
cross_finish_kernel(const cx *acc, double count, int nch, int nfreq, int nfft_is_even, int mode, void *out) {
    const int i = blockIdx.z, j = blockIdx.y;
    if (i > j) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nfreq) return;
    const int64_t ij = ((int64_t)i * nch + j) * nfreq + f, ji = ((int64_t)j * nch + i) * nfreq + f;
    const cx s = acc[ij];
    if (mode == OSZ_CROSS_SPECTRUM) {
        const double sides = (f == 0 || (nfft_is_even && f == nfreq - 1)) ? 1.0 : 2.0;
        cx *o = static_cast<cx *>(out);
        cx v = {s.x / count * sides, i == j ? 0.0 : s.y / count * sides};
        o[ij] = v;
        if (i != j) {
            v.y = -v.y;
            o[ji] = v;
        }
    } else {
        const double pi = acc[((int64_t)i * nch + i) * nfreq + f].x, pj = acc[((int64_t)j * nch + j) * nfreq + f].x;
        double *o = static_cast<double *>(out);
        const double c = (s.x * s.x + s.y * s.y) / (pi * pj);
        o[ij] = c;
        o[ji] = c;
    }
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_cross_accumulate(const void *X, int64_t nseg, int nch, int nfreq, void *acc, void *stream) {
    OSZ_REQUIRE(X && acc, "osz_cross_accumulate: null argument");
    OSZ_REQUIRE(nch >= 1 && nch <= 65535 && nfreq >= 1 && nseg >= 0 && nseg <= INT32_MAX &&
                    (int64_t)nch * nfreq < ((int64_t)1 << 27),
                "osz_cross_accumulate: bad sizes (nch * nfreq must stay below 2^27)");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0,
                "osz_cross_accumulate: X and acc must be 16-byte aligned");
    if (nseg == 0) return OSZ_OK;
    const int64_t nblk = (nch + kCrossB - 1) / kCrossB;
    const int64_t tri = nblk * (nblk + 1) / 2, fblk = ((int64_t)nfreq + kWave - 1) / kWave;
    OSZ_REQUIRE(tri <= INT32_MAX && fblk <= 65535, "osz_cross_accumulate: grid too large");
    KernelTimer timer("cross_accumulate", as_stream(stream));
    hipLaunchKernelGGL(cross_accumulate_kernel, dim3((unsigned)tri, (unsigned)fblk), dim3(kCrossThreads), 0,
                       as_stream(stream), static_cast<const cx *>(X), (int)nseg, nch, nfreq,
                       static_cast<cx *>(acc), (int)nblk);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_cross_finish(const void *acc, int64_t count, int nch, int nfreq, int nfft_is_even, int mode,
                     void *out, void *stream) {
    OSZ_REQUIRE(acc && out, "osz_cross_finish: null argument");
    OSZ_REQUIRE(nch >= 1 && nch <= 65535 && nfreq >= 1 && count >= 1, "osz_cross_finish: bad sizes");
    OSZ_REQUIRE(mode == OSZ_CROSS_SPECTRUM || mode == OSZ_CROSS_COHERENCE, "osz_cross_finish: unknown mode %d", mode);
    OSZ_REQUIRE(mode == OSZ_CROSS_SPECTRUM || out != acc, "osz_cross_finish: the coherence cannot overwrite the sums");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0,
                "osz_cross_finish: acc and out must be 16-byte aligned");
    KernelTimer timer("cross_finish", as_stream(stream));
    hipLaunchKernelGGL(cross_finish_kernel, dim3((unsigned)((nfreq + 255) / 256), nch, nch), dim3(256), 0,
                       as_stream(stream), static_cast<const cx *>(acc), (double)count, nch, nfreq,
                       nfft_is_even, mode, out);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
