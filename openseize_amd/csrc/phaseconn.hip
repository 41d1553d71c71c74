// phaseconn.hip -- K11 phase-based connectivity over all channel pairs: the per-segment sums of
// d_s = Im(conj(X[s, i, f]) X[s, j, f]) that the phase-lag measures need (sum d, sum |d|, sum d^2,
// sum sign d), the in-place normalisation X / |X| whose cross-spectra (K10's kernel) are the
// phase-locking sums, and the finishing pass of imcoh / plv / pli / wpli / dwpli with their fixed
// points.  DESIGN.md section 3, K11.
#include "common.h"

namespace osz {

typedef double cx __attribute__((ext_vector_type(2)));   // (re, im) of one complex128

constexpr int kLagT = 4;                      // channels per side of a lane's register tile
constexpr int kLagW = 2;                      // waves per side of a workgroup's tile
constexpr int kLagB = kLagT * kLagW;          // channels per side of a workgroup's tile (8)
constexpr int kLagWaves = kLagW * kLagW;      // 4
constexpr int kLagThreads = kWave * kLagWaves;            // 256
constexpr int kLagRows = 2 * kLagB / kLagWaves;           // rows a wave stages per segment (4)

// The structure of cross_accumulate_kernel (cross.hip) with four real sums per pair instead of
// one complex one: a lane is a frequency bin, a lane keeps a 4 x 4 tile of pairs -- 64 doubles,
// 128 VGPRs, which is why the workgroup is 4 waves (2 x 2: 64 bins of an 8 x 8 block of pairs,
// block row <= block column) and not K10's 16: at 256 threads a wave may hold 512 registers and
// several workgroups share a CU, each behind its own barrier.  Per segment the workgroup needs
// 8 + 8 channel rows of 64 bins (16 KB): wave w fetches rows 4w .. 4w + 3 of the two sets taken
// as one list (coalesced, 16 B per lane) one segment ahead of the arithmetic into registers and
// hands them over through a double-buffered LDS stage, one barrier per segment; every wave reads
// its 4 + 4 rows back as ds_read_b128 of consecutive lanes.  The segments are walked in order
// from the stored sums, nothing is atomic: the sums do not depend on where the stream is cut.
// d comes from ONE expression, fma(ur, vi, -(ui vr)), and all four sums are fed from it.  A NaN
// d goes into all four (the sign of NaN is NaN here, not 0).
// Grid: x = triangular block index (fastest), y = bin block.
__global__ void __launch_bounds__(kLagThreads)
lag_accumulate_kernel(const cx *__restrict__ X, int nseg, int nch, int nfreq, double *__restrict__ lag,
                      int nblk) {
    __shared__ cx stage[2][2 * kLagB][kWave];            // 32 KB
    int bi = 0, p = blockIdx.x;
    while (p >= nblk - bi) {                             // row bi of the triangle holds nblk - bi blocks
        p -= nblk - bi;
        ++bi;
    }
    const int bj = bi + p;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int wi = w / kLagW, wj = w % kLagW;
    const int f = blockIdx.y * kWave + lane;
    const bool inside = f < nfreq;
    // the rows this wave stages: entries 0 .. 7 of the list are block row bi's channels, 8 .. 15 bj's
    const int64_t seg = (int64_t)nch * nfreq;
    int off[kLagRows];
    bool have[kLagRows];
#pragma unroll
    for (int k = 0; k < kLagRows; ++k) {
        const int r = w * kLagRows + k;
        const int c = r < kLagB ? bi * kLagB + r : bj * kLagB + r - kLagB;
        have[k] = inside && c < nch;
        off[k] = have[k] ? c * nfreq + f : 0;
    }
    // the 4 x 4 pairs this lane sums; on a diagonal block the wave below the diagonal rests
    const int i0 = bi * kLagB + wi * kLagT, j0 = bj * kLagB + wj * kLagT;
    const bool active = i0 < nch && j0 < nch && (bi != bj || wi <= wj);
    const int64_t plane = (int64_t)nch * nch * nfreq;
    const cx zero = {0.0, 0.0};

    double sd[kLagT][kLagT], sa[kLagT][kLagT], sq[kLagT][kLagT], sg[kLagT][kLagT];
#pragma unroll
    for (int a = 0; a < kLagT; ++a)
#pragma unroll
        for (int b = 0; b < kLagT; ++b) {
            const int i = i0 + a, j = j0 + b;
            const bool mine = active && inside && j < nch && i <= j;
            const int64_t at = ((int64_t)i * nch + j) * nfreq + f;
            sd[a][b] = mine ? lag[at] : 0.0;
            sa[a][b] = mine ? lag[plane + at] : 0.0;
            sq[a][b] = mine ? lag[2 * plane + at] : 0.0;
            sg[a][b] = mine ? lag[3 * plane + at] : 0.0;
        }

    cx g[kLagRows];
#pragma unroll
    for (int k = 0; k < kLagRows; ++k) {
        g[k] = have[k] ? X[off[k]] : zero;
        stage[0][w * kLagRows + k][lane] = g[k];
    }
    __syncthreads();
    for (int s = 0; s < nseg; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < nseg;
        if (more) {
            X += seg;
#pragma unroll
            for (int k = 0; k < kLagRows; ++k) g[k] = have[k] ? X[off[k]] : zero;
        }
        if (active) {
            cx u[kLagT], v[kLagT];
#pragma unroll
            for (int a = 0; a < kLagT; ++a) u[a] = stage[cur][wi * kLagT + a][lane];
#pragma unroll
            for (int b = 0; b < kLagT; ++b) v[b] = stage[cur][kLagB + wj * kLagT + b][lane];
#pragma unroll
            for (int a = 0; a < kLagT; ++a)
#pragma unroll
                for (int b = 0; b < kLagT; ++b) {
                    // Im(conj(u) v) = ur vi - ui vr: one product rounded, one fused
                    const double t = u[a].y * v[b].x;
                    const double d = __builtin_fma(u[a].x, v[b].y, -t);
                    sd[a][b] += d;
                    sa[a][b] += __builtin_fabs(d);
                    sq[a][b] = __builtin_fma(d, d, sq[a][b]);
                    sg[a][b] += d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d);      // (+-0 adds 0, NaN adds NaN)
                }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < kLagRows; ++k) stage[cur ^ 1][w * kLagRows + k][lane] = g[k];
        }
        __syncthreads();
    }

    if (active && inside) {
#pragma unroll
        for (int a = 0; a < kLagT; ++a)
#pragma unroll
            for (int b = 0; b < kLagT; ++b) {
                const int i = i0 + a, j = j0 + b;
                if (j < nch && i <= j) {
                    const int64_t at = ((int64_t)i * nch + j) * nfreq + f;
                    lag[at] = sd[a][b];
                    lag[plane + at] = sa[a][b];
                    lag[2 * plane + at] = sq[a][b];
                    lag[3 * plane + at] = sg[a][b];
                }
            }
    }
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
    const int i = blockIdx.z, j = blockIdx.y;
    if (i > j) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nfreq) return;
    const int64_t ij = ((int64_t)i * nch + j) * nfreq + f, ji = ((int64_t)j * nch + i) * nfreq + f;
    const int64_t ii = ((int64_t)i * nch + i) * nfreq + f, jj = ((int64_t)j * nch + j) * nfreq + f;
    const int64_t plane = (int64_t)nch * nch * nfreq;
    const bool real_bin = f == 0 || (nfft_is_even && f == nfreq - 1);
    double own_i, own_j, v;
    if (mode == OSZ_PHASE_IMCOH) {
        own_i = acc[ii].x;
        own_j = acc[jj].x;
        v = acc[ij].y / sqrt(own_i * own_j);
    } else if (mode == OSZ_PHASE_PLV) {
        own_i = accn[ii].x;
        own_j = accn[jj].x;
        const cx s = accn[ij];
        v = sqrt(s.x * s.x + s.y * s.y) / count;
    } else {
        own_i = lag[ii];
        own_j = lag[jj];
        const double d = lag[ij], a = lag[plane + ij], q = lag[2 * plane + ij];
        if (mode == OSZ_PHASE_PLI) v = __builtin_fabs(lag[3 * plane + ij]) / count;
        else if (mode == OSZ_PHASE_WPLI) v = __builtin_fabs(d) / a;
        else v = (d * d - q) / (a * a - q);
    }
    bool fixed = true;
    if (own_i != own_i || own_j != own_j) v = __builtin_nan("");
    else if (i == j) v = mode == OSZ_PHASE_PLV ? 1.0 : 0.0;
    else if (real_bin && mode != OSZ_PHASE_PLV) v = 0.0;
    else fixed = false;
    out[ij] = v;
    if (i != j) out[ji] = (mode == OSZ_PHASE_IMCOH && !fixed) ? -v : v;
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_lag_accumulate(const void *X, int64_t nseg, int nch, int nfreq, double *lag, void *stream) {
    OSZ_REQUIRE(X && lag, "osz_lag_accumulate: null argument");
    OSZ_REQUIRE(nch >= 1 && nch <= 65535 && nfreq >= 1 && nseg >= 0 && nseg <= INT32_MAX &&
                    (int64_t)nch * nfreq < ((int64_t)1 << 27),
                "osz_lag_accumulate: bad sizes (nch * nfreq must stay below 2^27)");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(lag)) & 15) == 0,
                "osz_lag_accumulate: X and lag must be 16-byte aligned");
    if (nseg == 0) return OSZ_OK;
    const int64_t nblk = (nch + kLagB - 1) / kLagB;
    const int64_t tri = nblk * (nblk + 1) / 2, fblk = ((int64_t)nfreq + kWave - 1) / kWave;
    OSZ_REQUIRE(tri <= INT32_MAX && fblk <= 65535, "osz_lag_accumulate: grid too large");
    KernelTimer timer("lag_accumulate", as_stream(stream));
    hipLaunchKernelGGL(lag_accumulate_kernel, dim3((unsigned)tri, (unsigned)fblk), dim3(kLagThreads), 0,
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
