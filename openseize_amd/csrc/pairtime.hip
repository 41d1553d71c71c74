// pairtime.hip -- K13 time-domain connectivity of analytic signals over all channel pairs: the
// sums over TIME that amplitude-envelope correlation, its orthogonalised form, and the
// time-domain plv / ciplv / wpli need.  With z[c, t] = x + i y, a = |z|, r = 1 / a, u = z / a and,
// per pair, d = Im(conj(z_i) z_j), m = |d|:
//   group AMP   sum a_i a_j                                                     (aec)
//   group ORTH  sum m, sum m r_i, sum m r_j, sum (m r_i)^2, sum (m r_j)^2       (oaec)
//   group LOCK  Re, Im of sum conj(u_i) u_j                                     (plv, ciplv)
//   group LAG   sum d, sum m                                                    (wpli)
// and per channel sum a, sum a^2, sum |u|^2.  DESIGN.md section 3, K13.
//
// Unlike K10 / K11 the only reduction axis is the fastest axis of the data.  The stream is cut
// into blocks of OSZ_ANALYTIC_BLOCK samples counted from its first sample; a workgroup owns one
// block of pairs and ONE time block (grid y), a lane the samples lane + 64 k of it, summed in
// that order; the 64 lanes are then reduced in the fixed order of wave_sum63 and the block's
// partial is written, nothing is atomic.  pair_fold_kernel adds the partials to the totals in
// block order.  The sums therefore do not depend on how the stream is cut into pushes.
#include "pair_tile.h"

namespace osz {

constexpr int kPtWaves = 4;                   // waves of a workgroup, of either kernel
constexpr int kPtBlock = OSZ_ANALYTIC_BLOCK;  // samples per time block
constexpr int kPtPlanes = 6;                  // prepared planes: x, y, r, a, ux, uy
constexpr int kPtChan = 3;                    // per-channel sums: a, a^2, |u|^2

// A sum group: the prepared planes [first, first + nv) it reads and the ns sums it keeps.
template <int G> struct PtGroup;
template <> struct PtGroup<OSZ_ANALYTIC_AMP> { static constexpr int first = 3, nv = 1, ns = 1; };
template <> struct PtGroup<OSZ_ANALYTIC_ORTH> { static constexpr int first = 0, nv = 3, ns = 5; };
template <> struct PtGroup<OSZ_ANALYTIC_LOCK> { static constexpr int first = 4, nv = 2, ns = 2; };
template <> struct PtGroup<OSZ_ANALYTIC_LAG> { static constexpr int first = 0, nv = 2, ns = 2; };

__host__ __device__ inline int pt_planes(int groups) {
    return (groups & OSZ_ANALYTIC_AMP ? 1 : 0) + (groups & OSZ_ANALYTIC_ORTH ? 5 : 0) +
           (groups & OSZ_ANALYTIC_LOCK ? 2 : 0) + (groups & OSZ_ANALYTIC_LAG ? 2 : 0);
}
// the first plane of group g among the planes of `groups` (order: AMP, ORTH, LOCK, LAG)
__host__ __device__ inline int pt_first(int groups, int g) { return pt_planes(groups & (g - 1)); }

// Staging, once per (channel, sample) so that the pair loop holds no sqrt and no division:
// prep[p, c, t] for the six planes, and the block's per-channel sums.  Grid: x = time block,
// y = channel; thread k owns the samples k + 256 m of the block.  A zero sample gives r = inf and
// u = 0 / 0 = NaN: sum |u|^2 is the channel's flag for it (its own sum a stays finite).
__global__ void __launch_bounds__(256)
pair_prepare_kernel(const cx *__restrict__ z, int64_t ld, int nch, int64_t n, double *__restrict__ prep,
                    double *__restrict__ cpart) {
    __shared__ double red[kPtWaves][kPtChan];
    const int c = blockIdx.y, lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * kPtBlock, plane = (int64_t)nch * n;
    const cx *row = z + (int64_t)c * ld;
    double *out = prep + (int64_t)c * n;
    double sa = 0.0, sq = 0.0, su = 0.0;
    for (int m = 0; m < kPtBlock / 256; ++m) {
        const int64_t t = t0 + m * 256 + threadIdx.x;
        if (t < n) {
            const cx v = row[t];
            const double a = hypot(v.x, v.y);
            const double ux = v.x / a, uy = v.y / a;
            out[t] = v.x;
            out[plane + t] = v.y;
            out[2 * plane + t] = 1.0 / a;
            out[3 * plane + t] = a;
            out[4 * plane + t] = ux;
            out[5 * plane + t] = uy;
            sa += a;
            sq = __builtin_fma(a, a, sq);
            su += __builtin_fma(ux, ux, uy * uy);
        }
    }
    sa = wave_sum63(sa);
    sq = wave_sum63(sq);
    su = wave_sum63(su);
    if (lane == kWave - 1) {
        red[w][0] = sa;
        red[w][1] = sq;
        red[w][2] = su;
    }
    __syncthreads();
    if (threadIdx.x < kPtChan) {
        double s = red[0][threadIdx.x];
        for (int k = 1; k < kPtWaves; ++k) s += red[k][threadIdx.x];
        cpart[((int64_t)blockIdx.x * kPtChan + threadIdx.x) * nch + c] = s;
    }
}

// K11's workgroup (2 x 2 waves, an 8 x 8 block of pairs; 256 threads, so a wave may hold 512
// registers -- ORTH keeps 80 doubles of sums) whose staged rows carry the group's nv planes;
// wave w stages its quarter of the list, 8 B per lane
template <int G> using PtTile = PairTile<2, PtGroup<G>::nv, false>;

// The tile skeleton of pair_tile.h turned onto the time axis: a lane is a sample of a 64-sample
// step and keeps ns sums per pair; the 64 lanes are reduced at the end.  d comes from ONE
// expression, pair_im, in ORTH and in LAG: their sums of m carry the same bits.
// Samples past the end of a short last block are staged as 0 and add +0.0.
// Grid: x = triangular block index, y = time block.
template <int G>
__global__ void __launch_bounds__(PtTile<G>::Threads)
pair_accumulate_kernel(const double *__restrict__ prep, int nch, int64_t n, double *__restrict__ part, int nblk,
                       int nplanes, int plane0) {
    using P = PtTile<G>;
    constexpr int NV = P::NV, NS = PtGroup<G>::ns;
    __shared__ double stage[2][2 * P::B * NV][kWave];    // ORTH: 48 KB
    const PairBlock<P> blk(blockIdx.x, nblk, nch);
    const int lane = blk.lane;
    const int64_t t0 = (int64_t)blockIdx.y * kPtBlock;
    const int64_t left = n - t0;                         // >= 1 by the grid
    const int here = left < kPtBlock ? (int)left : kPtBlock;
    const int nsteps = (here + kWave - 1) / kWave;
    const int64_t plane = (int64_t)nch * n;
    // the rows this wave stages
    const double *src[P::Rows];
    bool have[P::Rows];
#pragma unroll
    for (int k = 0; k < P::Rows; ++k) {
        const int c = blk.channel(k);
        have[k] = c < nch;
        src[k] = prep + (PtGroup<G>::first + blk.value(k)) * plane + (have[k] ? (int64_t)c * n : 0) + t0 + lane;
    }

    double s[NS][P::T][P::T];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
        for (int a = 0; a < P::T; ++a)
#pragma unroll
            for (int b = 0; b < P::T; ++b) s[q][a][b] = 0.0;

    double g[P::Rows];
    pair_walk(
        nsteps, blk.active,
        [&](int st) {
            const int at = st * kWave;
#pragma unroll
            for (int k = 0; k < P::Rows; ++k) g[k] = have[k] && at + lane < here ? src[k][at] : 0.0;
        },
        [&](int buf) {
#pragma unroll
            for (int k = 0; k < P::Rows; ++k) stage[buf][blk.entry(k)][lane] = g[k];
        },
        [&](int cur) {
            double u[P::T][NV], v[P::T][NV];
#pragma unroll
            for (int a = 0; a < P::T; ++a)
#pragma unroll
                for (int q = 0; q < NV; ++q) u[a][q] = stage[cur][blk.slot_i(a) * NV + q][lane];
#pragma unroll
            for (int b = 0; b < P::T; ++b)
#pragma unroll
                for (int q = 0; q < NV; ++q) v[b][q] = stage[cur][blk.slot_j(b) * NV + q][lane];
#pragma unroll
            for (int a = 0; a < P::T; ++a)
#pragma unroll
                for (int b = 0; b < P::T; ++b) {
                    if constexpr (G == OSZ_ANALYTIC_AMP) {
                        s[0][a][b] = __builtin_fma(u[a][0], v[b][0], s[0][a][b]);
                    } else if constexpr (G == OSZ_ANALYTIC_LOCK) {
                        // conj(u_i) u_j
                        s[0][a][b] += pair_re(u[a][0], u[a][1], v[b][0], v[b][1]);
                        s[1][a][b] += pair_im(u[a][0], u[a][1], v[b][0], v[b][1]);
                    } else {
                        const double d = pair_im(u[a][0], u[a][1], v[b][0], v[b][1]);
                        const double m = __builtin_fabs(d);
                        if constexpr (G == OSZ_ANALYTIC_LAG) {
                            s[0][a][b] += d;
                            s[1][a][b] += m;
                        } else {
                            const double pi = m * u[a][2], pj = m * v[b][2];
                            s[0][a][b] += m;
                            s[1][a][b] += pi;
                            s[2][a][b] += pj;
                            s[3][a][b] = __builtin_fma(pi, pi, s[3][a][b]);
                            s[4][a][b] = __builtin_fma(pj, pj, s[4][a][b]);
                        }
                    }
                }
        });

    if (blk.active) {
        const int64_t cc = (int64_t)nch * nch;
        double *dst = part + ((int64_t)blockIdx.y * nplanes + plane0) * cc;
#pragma unroll
        for (int q = 0; q < NS; ++q)
            blk.pairs(nch, true, [&](int a, int b, bool mine, int i, int j) {
                const double total = wave_sum63(s[q][a][b]);
                if (lane == kWave - 1 && mine) dst[q * cc + (int64_t)i * nch + j] = total;
            });
    }
}

// tot[k] += part[0, k] + part[1, k] + ... in block order, one element per thread: read once,
// written once.  With tri != 0 the elements are (plane, i, j) and those with i > j are left alone.
__global__ void __launch_bounds__(256)
pair_fold_kernel(const double *__restrict__ part, int64_t nb, int64_t count, int tri, double *__restrict__ tot) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    if (tri && (k / tri) % tri > k % tri) return;
    double t = tot[k];
    for (int64_t b = 0; b < nb; ++b) t += part[b * count + k];
    tot[k] = t;
}

// One (i <= j) pair per thread; writes [i, j] and its mirror.  In this order: a channel one of
// whose own sums is not finite gives NaN; the diagonal is 1.0 for aec and plv and 0.0 for the
// others; everything else is the definition.
__global__ void __launch_bounds__(256)
analytic_finish_kernel(int mode, const double *__restrict__ sums, int groups, const double *__restrict__ chan,
                       double cnt, int nch, double *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)nch * nch) return;
    const int i = (int)(k / nch), j = (int)(k % nch);
    if (i > j) return;
    const int64_t cc = (int64_t)nch * nch;
    const double ai = chan[i], aj = chan[j], qi = chan[nch + i], qj = chan[nch + j];
    const bool lost = !(__builtin_isfinite(ai) && __builtin_isfinite(aj) && __builtin_isfinite(qi) &&
                        __builtin_isfinite(qj) && __builtin_isfinite(chan[2 * nch + i]) &&
                        __builtin_isfinite(chan[2 * nch + j]));
    double v;
    if (mode == OSZ_ANALYTIC_AEC) {
        v = pearson(cnt, ai, aj, qi, qj, sums[pt_first(groups, OSZ_ANALYTIC_AMP) * cc + k]);
    } else if (mode == OSZ_ANALYTIC_OAEC) {
        const double *o = sums + pt_first(groups, OSZ_ANALYTIC_ORTH) * cc + k;
        const double m = o[0];
        v = 0.5 * (pearson(cnt, ai, o[cc], qi, o[3 * cc], m) + pearson(cnt, aj, o[2 * cc], qj, o[4 * cc], m));
    } else if (mode == OSZ_ANALYTIC_WPLI) {
        const double *o = sums + pt_first(groups, OSZ_ANALYTIC_LAG) * cc + k;
        v = __builtin_fabs(o[0]) / o[cc];
    } else {
        const double *o = sums + pt_first(groups, OSZ_ANALYTIC_LOCK) * cc + k;
        if (mode == OSZ_ANALYTIC_PLV) {
            v = hypot(o[0], o[cc]) / cnt;
        } else {
            const double re = o[0] / cnt, im = o[cc] / cnt;
            v = __builtin_fabs(im) / sqrt(__builtin_fma(-re, re, 1.0));
        }
    }
    if (lost) v = __builtin_nan("");
    else if (i == j) v = (mode == OSZ_ANALYTIC_AEC || mode == OSZ_ANALYTIC_PLV) ? 1.0 : 0.0;
    out[k] = v;
    if (i != j) out[(int64_t)j * nch + i] = v;
}

static int pt_group_of(int mode) {
    return mode == OSZ_ANALYTIC_AEC ? OSZ_ANALYTIC_AMP : mode == OSZ_ANALYTIC_OAEC ? OSZ_ANALYTIC_ORTH
         : mode == OSZ_ANALYTIC_WPLI ? OSZ_ANALYTIC_LAG : OSZ_ANALYTIC_LOCK;
}

template <int G>
static void pt_launch(const double *prep, int nch, int64_t n, double *part, int nblk, int groups, dim3 grid,
                      hipStream_t st) {
    hipLaunchKernelGGL(pair_accumulate_kernel<G>, grid, dim3(PtTile<G>::Threads), 0, st, prep, nch, n, part, nblk,
                       pt_planes(groups), pt_first(groups, G));
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_analytic_work(int nch, int64_t n, int groups) {
    if (nch < 1 || n < 0 || groups < 1 || groups > OSZ_ANALYTIC_ALL) return -1;
    const int64_t nb = (n + kPtBlock - 1) / kPtBlock;
    return kPtPlanes * (int64_t)nch * n + nb * ((int64_t)pt_planes(groups) * nch * nch + kPtChan * (int64_t)nch);
}

int osz_analytic_accumulate(const void *z, int64_t ld, int nch, int64_t n, int groups, double *sums, double *chan,
                            double *work, int64_t work_len, void *stream) {
    OSZ_REQUIRE(z && sums && chan && work, "osz_analytic_accumulate: null argument");
    OSZ_REQUIRE(groups >= 1 && groups <= OSZ_ANALYTIC_ALL, "osz_analytic_accumulate: unknown sum groups %d", groups);
    int64_t nblk, tri;
    if (int rc = pair_grid("osz_analytic_accumulate", nch, PtTile<OSZ_ANALYTIC_AMP>::B, &nblk, &tri)) return rc;
    OSZ_REQUIRE(n >= 0 && ld >= n && n <= (int64_t)65535 * kPtBlock && (int64_t)nch * n < ((int64_t)1 << 40),
                "osz_analytic_accumulate: bad sizes");
    OSZ_REQUIRE((reinterpret_cast<uintptr_t>(z) & 15) == 0 &&
                    ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(chan) |
                      reinterpret_cast<uintptr_t>(work)) & 7) == 0,
                "osz_analytic_accumulate: z must be 16-byte aligned, the float64 arrays 8-byte aligned");
    OSZ_REQUIRE(work_len >= osz_analytic_work(nch, n, groups),
                "osz_analytic_accumulate: work holds %lld doubles, osz_analytic_work asks for %lld",
                (long long)work_len, (long long)osz_analytic_work(nch, n, groups));
    if (n == 0) return OSZ_OK;
    const int64_t nb = (n + kPtBlock - 1) / kPtBlock;
    const int np = pt_planes(groups);
    const int64_t cc = (int64_t)nch * nch;
    OSZ_REQUIRE((np * cc + 255) / 256 <= INT32_MAX, "osz_analytic_accumulate: grid too large");
    double *prep = work, *part = prep + kPtPlanes * (int64_t)nch * n, *cpart = part + nb * np * cc;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer timer("pair_prepare", st);
        hipLaunchKernelGGL(pair_prepare_kernel, dim3((unsigned)nb, (unsigned)nch), dim3(256), 0, st,
                           static_cast<const cx *>(z), ld, nch, n, prep, cpart);
        OSZ_HIP(hipGetLastError());
    }
    {
        KernelTimer timer("pair_accumulate", st);
        const dim3 grid((unsigned)tri, (unsigned)nb);
        if (groups & OSZ_ANALYTIC_AMP) pt_launch<OSZ_ANALYTIC_AMP>(prep, nch, n, part, (int)nblk, groups, grid, st);
        if (groups & OSZ_ANALYTIC_ORTH) pt_launch<OSZ_ANALYTIC_ORTH>(prep, nch, n, part, (int)nblk, groups, grid, st);
        if (groups & OSZ_ANALYTIC_LOCK) pt_launch<OSZ_ANALYTIC_LOCK>(prep, nch, n, part, (int)nblk, groups, grid, st);
        if (groups & OSZ_ANALYTIC_LAG) pt_launch<OSZ_ANALYTIC_LAG>(prep, nch, n, part, (int)nblk, groups, grid, st);
        OSZ_HIP(hipGetLastError());
    }
    KernelTimer timer("pair_fold", st);
    hipLaunchKernelGGL(pair_fold_kernel, dim3((unsigned)((np * cc + 255) / 256)), dim3(256), 0, st, part, nb,
                       np * cc, nch, sums);
    hipLaunchKernelGGL(pair_fold_kernel, dim3((unsigned)((kPtChan * nch + 255) / 256)), dim3(256), 0, st, cpart, nb,
                       (int64_t)kPtChan * nch, 0, chan);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_analytic_finish(int mode, const double *sums, int groups, const double *chan, int64_t count, int nch,
                        double *out, void *stream) {
    OSZ_REQUIRE(mode >= OSZ_ANALYTIC_AEC && mode <= OSZ_ANALYTIC_WPLI, "osz_analytic_finish: unknown mode %d", mode);
    OSZ_REQUIRE(groups >= 1 && groups <= OSZ_ANALYTIC_ALL && (groups & pt_group_of(mode)),
                "osz_analytic_finish: mode %d reads sum group %d, which groups = %d does not hold", mode,
                pt_group_of(mode), groups);
    OSZ_REQUIRE(sums && chan && out, "osz_analytic_finish: null argument");
    OSZ_REQUIRE(nch >= 1 && nch <= 65535 && count >= 1, "osz_analytic_finish: bad sizes");
    OSZ_REQUIRE(out != sums, "osz_analytic_finish: the result cannot overwrite the sums");
    KernelTimer timer("analytic_finish", as_stream(stream));
    const int64_t cc = (int64_t)nch * nch;
    hipLaunchKernelGGL(analytic_finish_kernel, dim3((unsigned)((cc + 255) / 256)), dim3(256), 0, as_stream(stream),
                       mode, sums, groups, chan, (double)count, nch, out);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
