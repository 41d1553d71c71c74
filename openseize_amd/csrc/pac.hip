// pac.hip -- the phase-amplitude comodulogram of ModulationIndex
// (experimental/coupling/estimators.py): the Tort et al. (2010) modulation index over a grid of
// phase bands x amplitude bands, with time-shift surrogates.
//
// osz_phase_bins: the phase of each complex sample, computed as osz_magphase computes it
// (phase_2pi of common.h), cut into nbins equal bins of [0, 2 pi); one byte per sample.
//
// osz_pac_accumulate: a WAVE owns one (phase row p, amplitude row a, set s) for the whole chunk.
// Its lanes stride over time; lane t keeps a private column of nbins doubles in LDS at
// hist[b * threads + t] (consecutive lanes on consecutive banks for every b: no conflicts, no
// dynamic register indexing), adds its samples to it in time order, and the wave's 64 columns
// are then summed in lane order by the lane that owns bin b and added to the persistent
// accumulator.  Every addition has one owner and a fixed place in the order: no atomics on
// floating-point data, two runs give the same bits, and the sums do not depend on the grid.
// For set s the shifted amplitude row is two contiguous runs, amp[sigma, L) against
// bins[0, L - sigma) and amp[0, sigma) against bins[L - sigma, L): the lanes of a wave read
// consecutive bytes of bins and consecutive doubles of amp, nothing is gathered.  The waves of a
// workgroup are consecutive sets of one (p, a) and walk the same bins bytes.
// The bin counts do not depend on (a, s): a second small kernel counts them per phase row with
// integer atomics (exact in any order).
//
// osz_pac_finish: one thread per (p, a, s) turns the sums into the modulation index.
#include "common.h"

namespace osz {

constexpr int kPbThreads = 256;
constexpr int kPacNone = 255;                 // bin code of a sample that belongs to no bin

__global__ __launch_bounds__(kPbThreads) void phase_bins_kernel(const double2 *__restrict__ z,
                                                                int64_t ldz, int64_t n, int nbins,
                                                                uint8_t *__restrict__ bins,
                                                                int64_t ldb) {
    constexpr double kTwoPi = 6.283185307179586476925286766559;
    const int r = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double p = phase_2pi(z[(int64_t)r * ldz + i]);
        int code = kPacNone;
        if (p == p) {
            const int b = (int)floor(p * (double)nbins / kTwoPi);
            code = b < nbins - 1 ? b : nbins - 1;
        }
        bins[(int64_t)r * ldb + i] = (uint8_t)code;
    }
}

constexpr int kPacUnroll = 4;                 // samples per lane in flight: 256 per wave and step
constexpr int kPacCountThreads = 256;
constexpr int kPacCountTile = kPacCountThreads * 64;    // samples per block and step
constexpr int kPacCountMaxBlk = 1024;

// counts[p, b] += #{i < L : bins[p, i] = b}
__global__ __launch_bounds__(kPacCountThreads) void pac_count_kernel(
    const uint8_t *__restrict__ bins, int64_t ldb, int64_t L, int nbins,
    unsigned long long *__restrict__ counts) {
    __shared__ unsigned int h[64];
    const int t = threadIdx.x, p = blockIdx.y;
    if (t < 64) h[t] = 0;
    __syncthreads();
    const uint8_t *row = bins + (int64_t)p * ldb;
    for (int64_t i0 = (int64_t)blockIdx.x * kPacCountTile; i0 < L;
         i0 += (int64_t)gridDim.x * kPacCountTile) {
        const int64_t end = i0 + kPacCountTile < L ? i0 + kPacCountTile : L;
        for (int64_t i = i0 + t; i < end; i += kPacCountThreads) {
            const int b = row[i];
            if (b < nbins) atomicAdd(&h[b], 1u);
        }
        __syncthreads();
        // (a tile holds 16384 samples: the 32-bit partial counts cannot overflow)
        if (t < nbins && h[t]) {
            atomicAdd(&counts[(int64_t)p * nbins + t], (unsigned long long)h[t]);
            h[t] = 0;
        }
        __syncthreads();
    }
}

// one lane's share of a run: col[b * T] += amp[i] for i = lane, lane + 64, ... < len with
// bins[i] = b < nbins, in ascending i
template <int T>
__device__ __forceinline__ void pac_run(const uint8_t *__restrict__ bins,
                                        const double *__restrict__ amp, int64_t len, int lane,
                                        int nbins, double *col) {
    int64_t i = lane;
    for (; i + (kPacUnroll - 1) * kWave < len; i += kPacUnroll * kWave) {
        int b[kPacUnroll];
        double v[kPacUnroll];
#pragma unroll
        for (int u = 0; u < kPacUnroll; ++u) {
            b[u] = bins[i + u * kWave];
            v[u] = amp[i + u * kWave];
        }
#pragma unroll
        for (int u = 0; u < kPacUnroll; ++u)
            if (b[u] < nbins) col[b[u] * T] += v[u];
    }
    for (; i < len; i += kWave) {
        const int b = bins[i];
        if (b < nbins) col[b * T] += amp[i];
    }
}

template <int T>
__global__ __launch_bounds__(T) void pac_accumulate_kernel(
    const uint8_t *__restrict__ bins, int64_t ldb, const double *__restrict__ amp, int64_t lda,
    int64_t L, const int64_t *__restrict__ shifts, int nsets, int nbins,
    double *__restrict__ sums) {
    extern __shared__ double hist[];           // nbins x T
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const int s = blockIdx.x * (T / kWave) + w;
    const int a = blockIdx.y, p = blockIdx.z, na = gridDim.y;
    if (s >= nsets) return;                    // (whole waves: no workgroup barrier below)
    double *col = hist + t;
    for (int b = 0; b < nbins; ++b) col[b * T] = 0.0;
    int64_t sigma = 0;
    if (s > 0) {
        sigma = shifts[s - 1] % L;
        if (sigma < 0) sigma += L;
    }
    const uint8_t *brow = bins + (int64_t)p * ldb;
    const double *arow = amp + (int64_t)a * lda;
    pac_run<T>(brow, arow + sigma, L - sigma, lane, nbins, col);            // unwrapped
    pac_run<T>(brow + (L - sigma), arow, sigma, lane, nbins, col);          // wrapped
    wave_lds_fence();
    double *out = sums + (((int64_t)p * na + a) * nsets + s) * nbins;
    for (int b = lane; b < nbins; b += kWave) {
        const double *rowb = hist + b * T + w * kWave;
        double tot = 0.0;
        for (int l = 0; l < kWave; ++l) tot += rowb[l];
        out[b] += tot;
    }
}

// mi[p, a, s] = 1 + sum_b P_b ln P_b / ln nbins with P_b = m_b / sum m, m_b = sums / counts;
// dist[p, a, :] = P of set 0; a phase row with an empty bin gives NaN
__global__ __launch_bounds__(256) void pac_finish_kernel(const double *__restrict__ sums,
                                                         const int64_t *__restrict__ counts,
                                                         int na, int nsets, int nbins,
                                                         int64_t total, double *__restrict__ mi,
                                                         double *__restrict__ dist) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int s = (int)(g % nsets);
    const int64_t pa = g / nsets;
    const int64_t p = pa / na;
    const double *row = sums + g * nbins;
    const int64_t *cnt = counts + p * nbins;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    bool empty = false;
    double tot = 0.0;
    for (int b = 0; b < nbins; ++b) {
        if (cnt[b] == 0) empty = true;
        else tot += row[b] / (double)cnt[b];
    }
    // 1 + sum P ln P / ln n = sum (P ln(n P) - P + 1/n) / ln n, as sum P = 1.  Summed in the
    // second form: with x = n P - 1 a term is ((1 + x) ln(1 + x) - x) / n >= 0, of the size of
    // x^2 / 2, so nothing cancels between the bins, and an error e of sum P (the rounding of tot
    // and of the quotients) enters as e^2.  The first form loses the index (1e-4 for a
    // surrogate) in the rounding of a sum close to -1, and sum P ln(n P) alone still takes e
    // in full: 1e-12 of such an index.
    double kl = 0.0;
    for (int b = 0; b < nbins; ++b) {
        const double pb = empty ? nan : row[b] / (double)cnt[b] / tot;
        const double x = fma((double)nbins, pb, -1.0);
        kl += pb != 0.0 ? (double)nbins * pb * log1p(x) - x : 1.0;
        if (s == 0) dist[pa * nbins + b] = pb;
    }
    mi[g] = empty ? nan : kl / ((double)nbins * log((double)nbins));
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_phase_bins(const double *z, int rows, int64_t n, int64_t ldz, int nbins, uint8_t *bins,
                   int64_t ldb, void *stream) {
    OSZ_REQUIRE(n == 0 || (z && bins), "osz_phase_bins: null argument");
    OSZ_REQUIRE(rows >= 1 && rows <= 65535 && n >= 0 && ldz >= n && ldb >= n,
                "osz_phase_bins: bad shape (rows=%d n=%lld ldz=%lld ldb=%lld)", rows, (long long)n,
                (long long)ldz, (long long)ldb);
    OSZ_REQUIRE(nbins >= 2 && nbins <= 64, "osz_phase_bins: nbins=%d is not in [2, 64]", nbins);
    if (n == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    int64_t nblk = (n + kPbThreads - 1) / kPbThreads;
    if (nblk > 4096) nblk = 4096;
    KernelTimer kt("phase_bins", st);
    hipLaunchKernelGGL(phase_bins_kernel, dim3((unsigned)nblk, (unsigned)rows), dim3(kPbThreads), 0,
                       st, reinterpret_cast<const double2 *>(z), ldz, n, nbins, bins, ldb);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_pac_accumulate(const uint8_t *bins, int np, int64_t ldb, const double *amp, int na,
                       int64_t lda, int64_t L, const int64_t *shifts, int nsur, int nbins,
                       double *sums, int64_t *counts, void *stream) {
    OSZ_REQUIRE(sums && counts && (L == 0 || (bins && amp)) && (nsur == 0 || shifts),
                "osz_pac_accumulate: null argument");
    OSZ_REQUIRE(np >= 1 && np <= 65535 && na >= 1 && na <= 65535 && L >= 0 && ldb >= L && lda >= L &&
                    nsur >= 0 && nsur < 0x7fffff00,
                "osz_pac_accumulate: bad sizes (np=%d na=%d L=%lld ldb=%lld lda=%lld nsur=%d)", np,
                na, (long long)L, (long long)ldb, (long long)lda, nsur);
    OSZ_REQUIRE(nbins >= 2 && nbins <= 64, "osz_pac_accumulate: nbins=%d is not in [2, 64]", nbins);
    if (L == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    const int nsets = nsur + 1;
    {
        KernelTimer kt("pac_count", st);
        int64_t nblk = (L + kPacCountTile - 1) / kPacCountTile;
        if (nblk > kPacCountMaxBlk) nblk = kPacCountMaxBlk;
        hipLaunchKernelGGL(pac_count_kernel, dim3((unsigned)nblk, (unsigned)np),
                           dim3(kPacCountThreads), 0, st, bins, ldb, L, nbins,
                           reinterpret_cast<unsigned long long *>(counts));
        OSZ_HIP(hipGetLastError());
    }
    KernelTimer kt("pac_accumulate", st);
    // the columns of a workgroup fill at most 64 KiB of LDS: 256 threads up to 32 bins, 128 above
    if (nbins <= 32) {
        constexpr int T = 256;
        const size_t lds = (size_t)nbins * T * sizeof(double);
        OSZ_DYN_LDS(pac_accumulate_kernel<T>, lds);
        hipLaunchKernelGGL(pac_accumulate_kernel<T>,
                           dim3((unsigned)((nsets + T / kWave - 1) / (T / kWave)), (unsigned)na,
                                (unsigned)np),
                           dim3(T), lds, st, bins, ldb, amp, lda, L, shifts, nsets, nbins, sums);
    } else {
        constexpr int T = 128;
        const size_t lds = (size_t)nbins * T * sizeof(double);
        OSZ_DYN_LDS(pac_accumulate_kernel<T>, lds);
        hipLaunchKernelGGL(pac_accumulate_kernel<T>,
                           dim3((unsigned)((nsets + T / kWave - 1) / (T / kWave)), (unsigned)na,
                                (unsigned)np),
                           dim3(T), lds, st, bins, ldb, amp, lda, L, shifts, nsets, nbins, sums);
    }
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_pac_finish(const double *sums, const int64_t *counts, int np, int na, int nsets, int nbins,
                   double *mi, double *dist, void *stream) {
    OSZ_REQUIRE(sums && counts && mi && dist, "osz_pac_finish: null argument");
    OSZ_REQUIRE(np >= 1 && na >= 1 && nsets >= 1, "osz_pac_finish: bad sizes (np=%d na=%d nsets=%d)",
                np, na, nsets);
    OSZ_REQUIRE(nbins >= 2 && nbins <= 64, "osz_pac_finish: nbins=%d is not in [2, 64]", nbins);
    hipStream_t st = as_stream(stream);
    const int64_t total = (int64_t)np * na * nsets;
    const int64_t nblk = (total + 255) / 256;
    OSZ_REQUIRE(nblk <= 0x7fffffff, "osz_pac_finish: %lld cells are too many", (long long)total);
    KernelTimer kt("pac_finish", st);
    hipLaunchKernelGGL(pac_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, st, sums, counts, na,
                       nsets, nbins, total, mi, dist);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
