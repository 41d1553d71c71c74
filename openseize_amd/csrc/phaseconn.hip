// phaseconn.hip -- K11 phase-based connectivity over all channel pairs: the per-segment sums of
// d_s = Im(conj(X[s, i, f]) X[s, j, f]) that the phase-lag measures need (sum d, sum |d|, sum d^2,
// sum sign d), the in-place normalisation X / |X| whose cross-spectra (K10's kernel) are the
// phase-locking sums, and the finishing pass of imcoh / plv / pli / wpli / dwpli with their fixed
// points.  DESIGN.md section 3, K11.
#include "pair_tile.h"

namespace osz {

// 2 x 2 waves: an 8 x 8 block of pairs; wave w stages rows 4w .. 4w + 3 of the two sets taken as one list
using LagTile = PairTile<2, 1, false>;

// The tile skeleton of pair_tile.h with four real sums per pair instead of K10's one complex one:
// a lane is a frequency bin and keeps 64 doubles, 128 VGPRs, which is why the workgroup is 4
// waves and not K10's 16: at 256 threads a wave may hold 512 registers and several workgroups
// share a CU, each behind its own barrier.  Per segment the workgroup stages 8 + 8 channel rows
// of 64 bins (16 KB), 16 B per lane; every wave reads its 4 + 4 rows back as ds_read_b128.
// d comes from ONE expression, pair_im, and all four sums are fed from it.  A NaN d goes into
// all four (the sign of NaN is NaN here, not 0).
// Grid: x = triangular block index, y = bin block.
__global__ void __launch_bounds__(LagTile::Threads)
lag_accumulate_kernel(const cx *__restrict__ X, int nseg, int nch, int nfreq, double *__restrict__ lag,
                      int nblk) {
    using P = LagTile;
    __shared__ cx stage[2][2 * P::B][kWave];             // 32 KB
    const PairBlock<P> blk(blockIdx.x, nblk, nch);
    const int lane = blk.lane;
    const int f = blockIdx.y * kWave + lane;
    const bool inside = f < nfreq;
    // the rows this wave stages
    const int64_t seg = (int64_t)nch * nfreq;
    int off[P::Rows];
    bool have[P::Rows];
#pragma unroll
    for (int k = 0; k < P::Rows; ++k) {
        const int c = blk.channel(k);
        have[k] = inside && c < nch;
        off[k] = have[k] ? c * nfreq + f : 0;
    }
    const int64_t plane = (int64_t)nch * nch * nfreq;
    const cx zero = {0.0, 0.0};

    double sd[P::T][P::T], sa[P::T][P::T], sq[P::T][P::T], sg[P::T][P::T];
    blk.pairs(nch, inside, [&](int a, int b, bool mine, int i, int j) {
        const int64_t at = pair_at(i, j, nch, nfreq, f);
        sd[a][b] = mine ? lag[at] : 0.0;
        sa[a][b] = mine ? lag[plane + at] : 0.0;
        sq[a][b] = mine ? lag[2 * plane + at] : 0.0;
        sg[a][b] = mine ? lag[3 * plane + at] : 0.0;
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
                    const double d = pair_im(u[a], v[b]);
                    sd[a][b] += d;
                    sa[a][b] += __builtin_fabs(d);
                    sq[a][b] = __builtin_fma(d, d, sq[a][b]);
                    sg[a][b] += sign_of(d);
                }
        });

    blk.pairs(nch, inside, [&](int a, int b, bool mine, int i, int j) {
        if (mine) {
            const int64_t at = pair_at(i, j, nch, nfreq, f);
            lag[at] = sd[a][b];
            lag[plane + at] = sa[a][b];
            lag[2 * plane + at] = sq[a][b];
            lag[3 * plane + at] = sg[a][b];
        }
    });
}

// X <- X / |X|, one element per thread: 0 gives 0 / 0 = NaN, a NaN stays one.
__global__ void __launch_bounds__(256) unit_phasors_kernel(cx *X, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    cx v = X[k];
    const double r = hypot(v.x, v.y);
    v.x /= r;
    v.y /= r;
    X[k] = v;
}

// One (i <= j) pair per (blockIdx.z, blockIdx.y), a lane per bin; writes [i, j] and its mirror
// [j, i] (the same value; imcoh: the negated one).  In this order: a channel whose own sums (the
// diagonal entry of the accumulator the measure reads) are NaN gives NaN; the diagonal is 1.0
// for plv and 0.0 for the others; the real bins (DC, and Nyquist for even nfft) are 0.0 for all
// but plv; everything else is the definition, 0 / 0 left as the NaN it is.
__global__ void __launch_bounds__(256)
phase_finish_kernel(int mode, const cx *acc, const cx *accn, const double *lag, double count, int nch,
                    int nfreq, int nfft_is_even, double *out) {
    const PairBin p(nch, nfreq, nfft_is_even);
    if (!p.valid) return;
    double own_i, own_j, v;
    if (mode == OSZ_PHASE_IMCOH) {
        own_i = acc[p.ii].x;
        own_j = acc[p.jj].x;
        v = acc[p.ij].y / sqrt(own_i * own_j);
    } else if (mode == OSZ_PHASE_PLV) {
        own_i = accn[p.ii].x;
        own_j = accn[p.jj].x;
        const cx s = accn[p.ij];
        v = sqrt(s.x * s.x + s.y * s.y) / count;
    } else {
        own_i = lag[p.ii];
        own_j = lag[p.jj];
        const double d = lag[p.ij], a = lag[p.plane + p.ij], q = lag[2 * p.plane + p.ij];
        if (mode == OSZ_PHASE_PLI) v = __builtin_fabs(lag[3 * p.plane + p.ij]) / count;
        else if (mode == OSZ_PHASE_WPLI) v = __builtin_fabs(d) / a;
        else v = (d * d - q) / (a * a - q);
    }
    bool fixed = true;
    if (own_i != own_i || own_j != own_j) v = __builtin_nan("");
    else if (p.i == p.j) v = mode == OSZ_PHASE_PLV ? 1.0 : 0.0;
    else if (p.real_bin && mode != OSZ_PHASE_PLV) v = 0.0;
    else fixed = false;
    out[p.ij] = v;
    if (p.i != p.j) out[p.ji] = (mode == OSZ_PHASE_IMCOH && !fixed) ? -v : v;
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_lag_accumulate(const void *X, int64_t nseg, int nch, int nfreq, double *lag, void *stream) {
    OSZ_REQUIRE(X && lag, "osz_lag_accumulate: null argument");
    int64_t nblk, tri;
    if (int rc = pair_grid("osz_lag_accumulate", nch, LagTile::B, &nblk, &tri)) return rc;
    OSZ_REQUIRE(nfreq >= 1 && nseg >= 0 && nseg <= INT32_MAX && (int64_t)nch * nfreq < ((int64_t)1 << 27),
                "osz_lag_accumulate: bad sizes (nch * nfreq must stay below 2^27)");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(lag)) & 15) == 0,
                "osz_lag_accumulate: X and lag must be 16-byte aligned");
    if (nseg == 0) return OSZ_OK;
    const int64_t fblk = ((int64_t)nfreq + kWave - 1) / kWave;
    OSZ_REQUIRE(fblk <= 65535, "osz_lag_accumulate: grid too large");
    KernelTimer timer("lag_accumulate", as_stream(stream));
    hipLaunchKernelGGL(lag_accumulate_kernel, dim3((unsigned)tri, (unsigned)fblk), dim3(LagTile::Threads), 0,
                       as_stream(stream), static_cast<const cx *>(X), (int)nseg, nch, nfreq, lag, (int)nblk);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_unit_phasors(void *X, int64_t n, void *stream) {
    OSZ_REQUIRE(X, "osz_unit_phasors: null argument");
    OSZ_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * 256, "osz_unit_phasors: bad size");
    OSZ_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0, "osz_unit_phasors: X must be 16-byte aligned");
    if (n == 0) return OSZ_OK;
    KernelTimer timer("unit_phasors", as_stream(stream));
    hipLaunchKernelGGL(unit_phasors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<cx *>(X), n);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_phase_finish(int mode, const void *acc, const void *accn, const double *lag, int64_t count, int nch,
                     int nfreq, int nfft_is_even, double *out, void *stream) {
    OSZ_REQUIRE(mode >= OSZ_PHASE_IMCOH && mode <= OSZ_PHASE_DWPLI, "osz_phase_finish: unknown mode %d", mode);
    const void *sums = mode == OSZ_PHASE_IMCOH ? acc : mode == OSZ_PHASE_PLV ? accn : static_cast<const void *>(lag);
    OSZ_REQUIRE(sums && out, "osz_phase_finish: null argument (mode %d reads %s)", mode,
                mode == OSZ_PHASE_IMCOH ? "acc" : mode == OSZ_PHASE_PLV ? "accn" : "lag");
    OSZ_REQUIRE(nch >= 1 && nch <= 65535 && nfreq >= 1 && count >= 1, "osz_phase_finish: bad sizes");
    OSZ_REQUIRE(out != sums, "osz_phase_finish: the result cannot overwrite the sums");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(sums)) & 15) == 0,
                "osz_phase_finish: the sums and out must be 16-byte aligned");
    KernelTimer timer("phase_finish", as_stream(stream));
    hipLaunchKernelGGL(phase_finish_kernel, dim3((unsigned)((nfreq + 255) / 256), nch, nch), dim3(256), 0,
                       as_stream(stream), mode, static_cast<const cx *>(acc), static_cast<const cx *>(accn), lag,
                       (double)count, nch, nfreq, nfft_is_even, out);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
