// cross.hip -- K10 Welch cross-spectra over all channel pairs: the raw sums
// acc[i, j, f] += sum_s conj(X[s, i, f]) X[s, j, f] (i <= j) of the segment spectra a
// SPEC_DFT_SEGMENTS push wrote, and the finishing pass (mean, one-sided doubling, Hermitian
// mirror, or the magnitude-squared coherence).  DESIGN.md section 3, K10.
#include "pair_tile.h"

namespace osz {

// 4 x 4 waves: a 16 x 16 block of pairs; wave w stages row w of either set
using CrossTile = PairTile<4, 1, true>;

// The tile skeleton of pair_tile.h as it is: a lane is a frequency bin (nfreq is the fastest
// axis of X: a wave's load of one channel is 64 consecutive complex128, 16 B per lane) and keeps
// one complex sum per pair, 64 VGPRs, so the workgroup can be 16 waves.  Per segment it stages
// 16 + 16 channel rows of 64 bins (32 KB); every wave reads its 4 + 4 rows back as ds_read_b128
// for 16 complex multiply-adds = 64 FMAs.
// Grid: x = triangular block index, y = bin block.
__global__ void __launch_bounds__(CrossTile::Threads)
cross_accumulate_kernel(const cx *__restrict__ X, int nseg, int nch, int nfreq, cx *__restrict__ acc,
                        int nblk) {
    using P = CrossTile;
    __shared__ cx stage[2][2 * P::B][kWave];             // 64 KB
    const PairBlock<P> blk(blockIdx.x, nblk, nch);
    const int lane = blk.lane;
    const int f = blockIdx.y * kWave + lane;
    const bool inside = f < nfreq;
    // the rows this wave stages
    // (a uniform base that moves from segment to segment plus a 32-bit offset per lane)
    const int64_t seg = (int64_t)nch * nfreq;
    int off[P::Rows];
    bool have[P::Rows];
#pragma unroll
    for (int k = 0; k < P::Rows; ++k) {
        const int c = blk.channel(k);
        have[k] = inside && c < nch;
        off[k] = have[k] ? c * nfreq + f : 0;
    }
    const cx zero = {0.0, 0.0};

    cx sum[P::T][P::T];
    blk.pairs(nch, inside, [&](int a, int b, bool mine, int i, int j) {
        sum[a][b] = mine ? acc[pair_at(i, j, nch, nfreq, f)] : zero;
    });

    cx g[P::Rows];
    pair_walk(
        nseg, blk.active,
        [&](int s) {
            const cx *x = X + s * seg;
#pragma unroll
            for (int k = 0; k < P::Rows; ++k) g[k] = have[k] ? x[off[k]] : zero;
        },
        [&](int buf) {
#pragma unroll
            for (int k = 0; k < P::Rows; ++k) stage[buf][blk.entry(k)][lane] = g[k];
        },
        [&](int cur) {
            cx u[P::T], v[P::T];
#pragma unroll
            for (int a = 0; a < P::T; ++a) u[a] = stage[cur][blk.slot_i(a)][lane];
#pragma unroll
            for (int b = 0; b < P::T; ++b) v[b] = stage[cur][blk.slot_j(b)][lane];
#pragma unroll
            for (int a = 0; a < P::T; ++a)
#pragma unroll
                for (int b = 0; b < P::T; ++b) {
                    // conj(u) v = (ur vr + ui vi) + i (ur vi - ui vr), four FMAs in a fixed order
                    double re = sum[a][b].x, im = sum[a][b].y;
                    re = __builtin_fma(u[a].x, v[b].x, re);
                    re = __builtin_fma(u[a].y, v[b].y, re);
                    im = __builtin_fma(u[a].x, v[b].y, im);
                    im = __builtin_fma(-u[a].y, v[b].x, im);
                    sum[a][b].x = re;
                    sum[a][b].y = im;
                }
        });

    blk.pairs(nch, inside, [&](int a, int b, bool mine, int i, int j) {
        if (mine) acc[pair_at(i, j, nch, nfreq, f)] = sum[a][b];
    });
}

// One (i <= j) pair per (blockIdx.z, blockIdx.y), a lane per bin; writes [i, j] and its mirror
// [j, i].  Spectrum: mean over the count, bins other than DC (and Nyquist for even nfft) doubled,
// the mirror conjugated, the diagonal's imaginary part set to 0 (the fused multiply-adds of the
// sum leave a residue there; the definition's ab - ba does not).  `out` may be `acc` itself: a
// pair is read by the one lane that writes it.  Coherence: |S_ij|^2 / (S_ii S_jj) from the raw
// sums (the count, the scaling and the doubling cancel), real.
__global__ void __launch_bounds__(256)
cross_finish_kernel(const cx *acc, double count, int nch, int nfreq, int nfft_is_even, int mode, void *out) {
    const PairBin p(nch, nfreq, nfft_is_even);
    if (!p.valid) return;
    const cx s = acc[p.ij];
    if (mode == OSZ_CROSS_SPECTRUM) {
        const double sides = p.real_bin ? 1.0 : 2.0;
        cx *o = static_cast<cx *>(out);
        cx v = {s.x / count * sides, p.i == p.j ? 0.0 : s.y / count * sides};
        o[p.ij] = v;
        if (p.i != p.j) {
            v.y = -v.y;
            o[p.ji] = v;
        }
    } else {
        const double pi = acc[p.ii].x, pj = acc[p.jj].x;
        double *o = static_cast<double *>(out);
        const double c = (s.x * s.x + s.y * s.y) / (pi * pj);
        o[p.ij] = c;
        o[p.ji] = c;
    }
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_cross_accumulate(const void *X, int64_t nseg, int nch, int nfreq, void *acc, void *stream) {
    OSZ_REQUIRE(X && acc, "osz_cross_accumulate: null argument");
    int64_t nblk, tri;
    if (int rc = pair_grid("osz_cross_accumulate", nch, CrossTile::B, &nblk, &tri)) return rc;
    OSZ_REQUIRE(nfreq >= 1 && nseg >= 0 && nseg <= INT32_MAX && (int64_t)nch * nfreq < ((int64_t)1 << 27),
                "osz_cross_accumulate: bad sizes (nch * nfreq must stay below 2^27)");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0,
                "osz_cross_accumulate: X and acc must be 16-byte aligned");
    if (nseg == 0) return OSZ_OK;
    const int64_t fblk = ((int64_t)nfreq + kWave - 1) / kWave;
    OSZ_REQUIRE(fblk <= 65535, "osz_cross_accumulate: grid too large");
    KernelTimer timer("cross_accumulate", as_stream(stream));
    hipLaunchKernelGGL(cross_accumulate_kernel, dim3((unsigned)tri, (unsigned)fblk), dim3(CrossTile::Threads), 0,
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
