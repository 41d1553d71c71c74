// windowspec.hip -- K18 spectral features per window (features/spectral.py window_spectral): every
// periodogram row that a SPEC_PSD_SEGMENTS push of spec.hip wrote is reduced to the numbers of
// osz_window_spectral_feature -- band power, peak, centroid, spread, edge frequencies, entropy,
// flatness -- where K15 .. K17 reduce the samples themselves.  DESIGN.md section 4, K18.
//
// One workgroup per row on a two-dimensional grid (row = y gridDim.x + x: more rows than one grid
// dimension holds) -- one wave for a range of n <= OSZ_WS_WAVE bins, 256 threads above:
//   * the range is cut into tiles of CAP = NT BMAX bins (one tile up to OSZ_WS_WAVE for the wave,
//     up to OSZ_WS_LDS for the workgroup; longer ranges take ceil(n / OSZ_WS_LDS) tiles).  A tile
//     comes into LDS by coalesced loads and leaves it lane-blocked: thread t holds the B
//     consecutive bins t B .. t B + B - 1 in registers (B = ceil(n / NT) for one tile, BMAX for
//     more; the LDS pitch B | 1 is odd, so both sides are free of bank conflicts).  LDS is the
//     transposer only: every sum, the arg-max and the search read registers;
//   * pass 1 takes per thread, in bin order, sum P, sum f P, the largest bin and the part of every
//     band the thread holds; the threads' sums meet in a fixed order (wave_sum63, then the waves
//     in turn);
//   * pass 2 -- only when spread, edge, entropy or flatness is asked -- needs the total and the
//     centroid: sum (f - c)^2 P, sum p ln p, sum ln p, and for the edges a DPP scan of the
//     threads' sums; the one thread whose block crosses p S walks its own bins.  A one-tile row
//     still holds its bins in registers; a longer row reads its tiles again (from L2).
// Sums have a fixed order that is a function of n alone, the only atomic is an integer minimum in
// LDS: a row's bits depend on its own bins and the arguments only.
#include <climits>

#include "common.h"

namespace osz {

#pragma clang fp contract(off)

static_assert(OSZ_WS_WAVE == 8 * kWave && OSZ_WS_LDS == 16 * 256 && OSZ_WS_BANDS_MOST == 16 &&
                  OSZ_WS_EDGES_MOST == 16 && OSZ_WS_COUNT == 9,
              "spectral_features_kernel");

struct WsArgs {
    const double *P;      // (nrows, nfreq) rows
    int64_t nfreq, nrows;
    int nch, k0, n;       // the range: bins k0 .. k0 + n - 1
    double df, lnn;       // ln n
    int nbands, nedges, normalize, mask;
    int b0[OSZ_WS_BANDS_MOST], b1[OSZ_WS_BANDS_MOST];
    double edge[OSZ_WS_EDGES_MOST];
    double *out;          // already at win0
    int64_t plane_pitch, row_pitch;
};

// The sums of v[0 .. N) over the workgroup, in every thread: wave_sum63, then the waves in turn.
template <int NT, int N>
__device__ __forceinline__ void ws_block_sum(double (&v)[N], double *red, int lane, int w) {
    constexpr int NW = NT / kWave;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = lane63(wave_sum63(v[i]));
    if constexpr (NW > 1) {
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < N; ++i) red[i * NW + w] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double s = red[i * NW];
#pragma unroll
            for (int j = 1; j < NW; ++j) s += red[i * NW + j];
            v[i] = s;
        }
        __syncthreads();
    }
}

// Inclusive sums over the lanes of a wave: row_shr 1, 2, 4, 8 inside the rows of 16 (lanes without
// a source add 0), then row_bcast:15 into the odd rows and row_bcast:31 into the upper half.
// (Not wave_scan of windowfrac.hip, which adds the totals of the rows below by readlane, in row
// order: other bits.  Each kernel's results are pinned to its own order.)
__device__ __forceinline__ double ws_wave_scan(double v, int lane) {
    v += dpp_mov0<0x111>(v);
    v += dpp_mov0<0x112>(v);
    v += dpp_mov0<0x114>(v);
    v += dpp_mov0<0x118>(v);
    const double a = dpp_mov0<0x142>(v);
    if (lane & 16) v += a;
    const double b = dpp_mov0<0x143>(v);
    if (lane & 32) v += b;
    return v;
}

// (exclusive sum of s over the threads before this one, the sum over all of them)
template <int NT>
__device__ __forceinline__ void ws_block_scan(double s, double *red, int lane, int w, double &excl, double &total) {
    constexpr int NW = NT / kWave;
    const double inc = ws_wave_scan(s, lane);
    // the lane below: row_shr:1 inside a row, the last lane of the row before across rows
    const double below = lane_from(inc, (lane + 63) & 63);
    excl = lane ? below : 0.0;
    total = lane63(inc);
    if constexpr (NW > 1) {
        if (lane == 0) red[w] = total;
        __syncthreads();
        double off = 0.0, all = red[0];
#pragma unroll
        for (int j = 1; j < NW; ++j) {
            if (j <= w) off = all;
            all += red[j];
        }
        __syncthreads();
        excl = w ? off + excl : excl;
        total = all;
    }
}

template <int NT, int BMAX>
__global__ void __launch_bounds__(NT) spectral_features_kernel(const WsArgs A) {
    constexpr int NW = NT / kWave, CAP = NT * BMAX;
    __shared__ double tile[NT * (BMAX | 1)];
    __shared__ double red[4 * NW];
    __shared__ int redk[NW];
    __shared__ double bandsum[OSZ_WS_BANDS_MOST];
    __shared__ int edgek[OSZ_WS_EDGES_MOST];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
    const int64_t r = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (r >= A.nrows) return;                              // (the whole workgroup)
    const double *__restrict__ row = A.P + r * A.nfreq + A.k0;
    const int n = A.n, ntiles = (n + CAP - 1) / CAP;
    const int B = ntiles == 1 ? (n + NT - 1) / NT : BMAX, bs = B | 1;
    const unsigned magic = (65536u + B - 1) / B;           // e / B = e magic >> 16 for e < 65536 / B
    const double df = A.df;
    const int mask = A.mask;
    const bool w_total = mask & (1 << OSZ_WS_TOTAL), w_band = mask & (1 << OSZ_WS_BAND),
               w_rel = mask & (1 << OSZ_WS_RELATIVE), w_peak = mask & (1 << OSZ_WS_PEAK),
               w_cent = mask & (1 << OSZ_WS_CENTROID), w_spread = mask & (1 << OSZ_WS_SPREAD),
               w_edge = mask & (1 << OSZ_WS_EDGE), w_ent = mask & (1 << OSZ_WS_ENTROPY),
               w_flat = mask & (1 << OSZ_WS_FLATNESS);
    const int nb = (w_band || w_rel) ? A.nbands : 0, ne = w_edge ? A.nedges : 0;
    const int p_band = w_total ? 1 : 0, p_rel = p_band + (w_band ? nb : 0), p_peak = p_rel + (w_rel ? nb : 0),
              p_cent = p_peak + (w_peak ? 1 : 0), p_spread = p_cent + (w_cent ? 1 : 0),
              p_edge = p_spread + (w_spread ? 1 : 0), p_ent = p_edge + ne, p_flat = p_ent + (w_ent ? 1 : 0),
              nplanes = p_flat + (w_flat ? 1 : 0);
    const unsigned seg = (unsigned)r / (unsigned)A.nch;    // (r < 2^31: the entry point checks)
    double *__restrict__ dst = A.out + (int64_t)((unsigned)r - seg * (unsigned)A.nch) * A.row_pitch + seg;
    const double nan = __builtin_nan("");

    if (t < OSZ_WS_EDGES_MOST) edgek[t] = INT_MAX;

    double p[BMAX];
    int cnt = 0, klo = 0;                                  // this thread's bins of the tile: klo .. klo + cnt - 1
    auto load_tile = [&](int tb, int tn) {
        __syncthreads();                                   // (the reads of the tile before)
#pragma unroll
        for (int q = 0; q < BMAX; ++q) {
            const int e = q * NT + t;
            if (e < tn) {
                const int own = (int)(((unsigned)e * magic) >> 16);
                tile[own * bs + (e - own * B)] = row[tb + e];
            }
        }
        __syncthreads();
        cnt = tn - t * B;
        cnt = cnt < 0 ? 0 : (cnt > B ? B : cnt);
        klo = A.k0 + tb + t * B;
#pragma unroll
        for (int j = 0; j < BMAX; ++j) p[j] = j < cnt ? tile[t * bs + j] : 0.0;
    };

    // ---- pass 1: sum P, sum f P, the largest bin, the bands ----
    double sacc = 0.0, m1 = 0.0, best = -1.0;
    int bk = INT_MAX;
    for (int it = 0; it < ntiles; ++it) {
        const int tb = it * CAP, tn = n - tb < CAP ? n - tb : CAP;
        load_tile(tb, tn);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if (j < cnt) {
                const double v = p[j], f = (double)(klo + j) * df;
                s += v;
                m1 += f * v;
                if (v > best) {
                    best = v;
                    bk = klo + j;
                }
            }
        sacc += s;
        for (int bb = 0; bb < nb; bb += 4) {
            double c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[i] = 0.0;
                if (bb + i < nb) {
                    const int lo = A.b0[bb + i] > klo ? A.b0[bb + i] : klo;
                    const int hi = A.b1[bb + i] < klo + cnt ? A.b1[bb + i] : klo + cnt;
                    if (lo < hi) {
                        if (hi - lo == cnt) c[i] = s;      // (the same additions in the same order)
                        else
#pragma unroll
                            for (int j = 0; j < BMAX; ++j)
                                if (klo + j >= lo && klo + j < hi) c[i] += p[j];
                    }
                }
            }
            ws_block_sum<NT, 4>(c, red, lane, w);
            if (t == 0)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (bb + i < nb) bandsum[bb + i] = it ? bandsum[bb + i] + c[i] : c[i];
        }
    }
    double a[2] = {sacc, m1};
    ws_block_sum<NT, 2>(a, red, lane, w);
    const double S = a[0], M1 = a[1];
    if (w_peak) {                                          // the largest bin, ties to the lowest
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m);
            const int ok = __shfl_xor(bk, m);
            if (ob > best || (ob == best && ok < bk)) {
                best = ob;
                bk = ok;
            }
        }
        if constexpr (NW > 1) {
            if (lane == 0) {
                red[w] = best;
                redk[w] = bk;
            }
            __syncthreads();
            best = red[0];
            bk = redk[0];
#pragma unroll
            for (int j = 1; j < NW; ++j)
                if (red[j] > best || (red[j] == best && redk[j] < bk)) {
                    best = red[j];
                    bk = redk[j];
                }
            __syncthreads();
        }
    }
    __syncthreads();                                       // bandsum
    const bool wild = S != S, zero = S == 0.0;
    const double total = df * S;
    if (t == 0) {
        if (w_total) dst[0] = wild ? nan : total;
        for (int b = 0; b < nb; ++b) {
            const double band = df * bandsum[b];
            if (w_band) dst[(int64_t)(p_band + b) * A.plane_pitch] = wild ? nan : band;
            if (w_rel) dst[(int64_t)(p_rel + b) * A.plane_pitch] = (wild || zero) ? nan : band / total;
        }
        if (w_peak) dst[(int64_t)p_peak * A.plane_pitch] = (wild || zero) ? nan : (double)bk * df;
        if (w_cent) dst[(int64_t)p_cent * A.plane_pitch] = (wild || zero) ? nan : M1 / S;
    }
    if (!(w_spread || w_edge || w_ent || w_flat)) return;
    if (wild || zero) {                                    // (the whole workgroup)
        if (t >= p_spread && t < nplanes) dst[(int64_t)t * A.plane_pitch] = nan;
        return;
    }

    // ---- pass 2: about the centroid and the total ----
    const double cen = M1 / S;
    const bool logs = w_ent || w_flat;
    double m2 = 0.0, H = 0.0, L = 0.0, nz = 0.0, carry = 0.0;
    for (int it = 0; it < ntiles; ++it) {
        const int tb = it * CAP, tn = n - tb < CAP ? n - tb : CAP;
        if (ntiles > 1) load_tile(tb, tn);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if (j < cnt) {
                const double v = p[j], d = (double)(klo + j) * df - cen;
                s += v;
                m2 += (d * d) * v;
                if (logs) {
                    const double q = v / S;
                    if (q > 0.0) {
                        const double lq = log(q);
                        H += q * lq;
                        L += lq;
                    } else
                        nz += 1.0;
                }
            }
        if (ne) {
            double excl, all;
            ws_block_scan<NT>(s, red, lane, w, excl, all);
            const double base = carry + excl, incl = base + s;
            for (int e = 0; e < ne; ++e) {
                const double thr = A.edge[e] * S;
                if (incl >= thr && !(base >= thr)) {       // this thread's block crosses p S
                    double run = 0.0;
                    int k = INT_MAX;
#pragma unroll
                    for (int j = 0; j < BMAX; ++j)
                        if (j < cnt) {
                            run += p[j];
                            if (k == INT_MAX && base + run >= thr) k = klo + j;
                        }
                    atomicMin(&edgek[e], k);
                }
            }
            carry += all;
        }
    }
    double z[4] = {m2, H, L, nz};
    ws_block_sum<NT, 4>(z, red, lane, w);
    __syncthreads();                                       // edgek
    if (t == 0) {
        if (w_spread) dst[(int64_t)p_spread * A.plane_pitch] = sqrt(z[0] / S);
        for (int e = 0; e < ne; ++e) {
            // (no cumulative sum reached p S: the last bin's does but for the rounding)
            const int k = edgek[e] == INT_MAX ? A.k0 + n - 1 : edgek[e];
            dst[(int64_t)(p_edge + e) * A.plane_pitch] = (double)k * df;
        }
        if (w_ent) {
            const double h = 0.0 - z[1];
            dst[(int64_t)p_ent * A.plane_pitch] = n == 1 ? 0.0 : (A.normalize ? h / A.lnn : h);
        }
        if (w_flat) dst[(int64_t)p_flat * A.plane_pitch] = z[3] > 0.0 ? 0.0 : (double)n * exp(z[2] / (double)n);
    }
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_spectral_features(const double *P, int64_t nrows, int nch, int64_t nfreq, int64_t k0, int64_t k1, double df,
                          const int *bands, int nbands, const double *edges, int nedges, int normalize, int mask,
                          double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0, void *stream) {
    OSZ_REQUIRE(P && out, "osz_spectral_features: null argument");
    OSZ_REQUIRE(nch >= 1 && nrows >= 0 && nrows % nch == 0 && nfreq >= 1 && nfreq <= INT32_MAX / 2 && win0 >= 0,
                "osz_spectral_features: bad sizes (nrows=%lld nch=%d nfreq=%lld)", (long long)nrows, nch,
                (long long)nfreq);
    OSZ_REQUIRE(k0 >= 0 && k0 <= k1 && k1 < nfreq,
                "osz_spectral_features: the bin range %lld .. %lld is not in 0 .. %lld", (long long)k0, (long long)k1,
                (long long)nfreq - 1);
    OSZ_REQUIRE(mask >= 1 && mask < (1 << OSZ_WS_COUNT), "osz_spectral_features: feature mask %d", mask);
    OSZ_REQUIRE(df == df, "osz_spectral_features: df is NaN");
    const bool banded = (mask & ((1 << OSZ_WS_BAND) | (1 << OSZ_WS_RELATIVE))) != 0;
    const bool edged = (mask & (1 << OSZ_WS_EDGE)) != 0;
    OSZ_REQUIRE(!banded || (bands && nbands >= 1 && nbands <= OSZ_WS_BANDS_MOST),
                "osz_spectral_features: %d bands (1 .. %d)%s", nbands, OSZ_WS_BANDS_MOST,
                banded && !bands ? ", bands is null" : "");
    OSZ_REQUIRE(!edged || (edges && nedges >= 1 && nedges <= OSZ_WS_EDGES_MOST),
                "osz_spectral_features: %d edge fractions (1 .. %d)%s", nedges, OSZ_WS_EDGES_MOST,
                edged && !edges ? ", edges is null" : "");
    WsArgs A;
    A.nbands = banded ? nbands : 0;
    A.nedges = edged ? nedges : 0;
    for (int j = 0; j < OSZ_WS_BANDS_MOST; ++j) A.b0[j] = A.b1[j] = 0;
    for (int j = 0; j < OSZ_WS_EDGES_MOST; ++j) A.edge[j] = 1.0;
    for (int j = 0; j < A.nbands; ++j) {
        OSZ_REQUIRE(bands[2 * j] >= k0 && bands[2 * j] < bands[2 * j + 1] && bands[2 * j + 1] <= k1 + 1,
                    "osz_spectral_features: band %d, bins [%d, %d), is empty or not inside %lld .. %lld", j,
                    bands[2 * j], bands[2 * j + 1], (long long)k0, (long long)k1);
        A.b0[j] = bands[2 * j];
        A.b1[j] = bands[2 * j + 1];
    }
    for (int j = 0; j < A.nedges; ++j) {
        OSZ_REQUIRE(edges[j] > 0.0 && edges[j] <= 1.0, "osz_spectral_features: edges[%d]=%g is not in (0, 1]", j,
                    edges[j]);
        A.edge[j] = edges[j];
    }
    const int64_t nseg = nrows / nch;
    const int planes = __builtin_popcount(mask & ~((1 << OSZ_WS_BAND) | (1 << OSZ_WS_RELATIVE) | (1 << OSZ_WS_EDGE))) +
                       A.nbands * __builtin_popcount(mask & ((1 << OSZ_WS_BAND) | (1 << OSZ_WS_RELATIVE))) + A.nedges;
    OSZ_REQUIRE(row_pitch >= win0 + nseg && (nch == 1 || plane_pitch >= (int64_t)(nch - 1) * row_pitch + win0 + nseg) &&
                    plane_pitch >= win0 + nseg,
                "osz_spectral_features: the result's pitches (%lld, %lld) do not hold %d rows of %lld + %lld windows "
                "in each of %d planes",
                (long long)plane_pitch, (long long)row_pitch, nch, (long long)win0, (long long)nseg, planes);
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(out)) & 7) == 0,
                "osz_spectral_features: the arrays must be 8-byte aligned");
    if (nrows == 0) return OSZ_OK;
    constexpr int64_t kGridX = 32768;
    OSZ_REQUIRE(nrows <= kGridX * 65535, "osz_spectral_features: %lld rows are too many for one launch",
                (long long)nrows);
    A.P = P;
    A.nfreq = nfreq;
    A.nrows = nrows;
    A.nch = nch;
    A.k0 = (int)k0;
    A.n = (int)(k1 - k0 + 1);
    A.df = df;
    A.lnn = __builtin_log((double)A.n);
    A.normalize = normalize != 0;
    A.mask = mask;
    A.out = out + win0;
    A.plane_pitch = plane_pitch;
    A.row_pitch = row_pitch;
    const dim3 grid((unsigned)(nrows < kGridX ? nrows : kGridX), (unsigned)((nrows + kGridX - 1) / kGridX));
    hipStream_t st = as_stream(stream);
    KernelTimer timer("spectral_features", st);
    if (A.n <= OSZ_WS_WAVE) hipLaunchKernelGGL((spectral_features_kernel<64, 8>), grid, dim3(64), 0, st, A);
    else hipLaunchKernelGGL((spectral_features_kernel<256, 16>), grid, dim3(256), 0, st, A);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
