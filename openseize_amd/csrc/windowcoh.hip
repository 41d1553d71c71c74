// windowcoh.hip -- K27 banded spectral connectivity per window: for every window of nsub consecutive
// segment spectra (a SPEC_DFT_SEGMENTS push), mstep apart, every channel pair and every band of bins
// the band mean of coh / imcoh (K10's sums), plv (K10's sums of the unit phasors) and pli / wpli /
// dwpli (K11's sums), each taken over the window's segments alone.  DESIGN.md section 4, K27.
#include <algorithm>

#include "pair_tile.h"

namespace osz {

// 2 x 2 waves: an 8 x 8 block of pairs, K11's tile; wave w stages rows 4w .. 4w + 3 of the two sets
using CohTile = PairTile<2, 1, false>;

constexpr int kCohPairs = CohTile::B * CohTile::B;       // the pairs of a block
constexpr int kCohPitch = kWave + 1;                     // doubles per pair in the fold's LDS: an odd pitch
enum { kCohCross = 0, kCohLock = 1, kCohLag = 2 };       // the sum groups, one kernel instance each

struct CohBands {
    int b[2 * OSZ_WK_BANDS_MOST];                        // [b0, b1) per band
};

// The tile skeleton of pair_tile.h with a lane that is one (window, bin of the band): a workgroup
// owns whole windows of one band, so no band sum crosses workgroups.  A band of nb <= 64 bins takes
// g = 64 / nb windows per workgroup, lane l the bin l % nb of window l / nb (g nb lanes busy); a
// longer one takes one window in ceil(nb / 64) passes, the band sum carried from pass to pass in
// bin order.  The walk is the window's nsub segments in order through K11's double-buffered stage
// (32 KB, one barrier per segment); the sums are K10's (CROSS; LOCK: of X / |X|, normalised on the
// way into the stage) with the sum |X|^2 of the tile's 4 + 4 channels taken from the staged values,
// or K11's four (LAG) with K11's own-channel sum.  After the walk the stage is free: measure by
// measure the lanes put their per-bin values there, 65 doubles per pair, and one thread per (pair,
// window) adds its band's bins in bin order, multiplies by 1 / nb once and writes [i, j]; the
// mirror goes through `turn` so that its rows stay whole.  The fold order is a function of nb alone.
// Grid: x = triangular block index, y = group of windows (from group0 on), z = band.
template <int G>
__global__ void __launch_bounds__(CohTile::Threads)
window_coherence_kernel(const cx *__restrict__ X, int nch, int nfreq, int nsub, int mstep, int64_t nwin,
                        int64_t group0, CohBands bands, int nbands, int mask, double *__restrict__ out,
                        int64_t plane_pitch, int nblk) {
    using P = CohTile;
    __shared__ __attribute__((aligned(16))) unsigned char raw[kCohPairs * kCohPitch * sizeof(double)];   // 32.5 KB
    __shared__ double turn[P::Threads];
    typedef cx StageRow[kWave];
    StageRow *stage = reinterpret_cast<StageRow *>(raw);             // [2][2 B][64], the first 32 KB
    double *vals = reinterpret_cast<double *>(raw);                  // [pair][65]

    const int band = blockIdx.z;
    const int b0 = bands.b[2 * band], nb = bands.b[2 * band + 1] - b0;
    const bool narrow = nb <= kWave;
    const int g = narrow ? kWave / nb : 1;
    const int64_t k0 = (group0 + blockIdx.y) * g;
    if (k0 >= nwin) return;                                          // (the grid's y is the widest band's)
    const int gwin = (int)(nwin - k0 < g ? nwin - k0 : g);           // the windows of this workgroup
    const int npass = narrow ? 1 : (nb + kWave - 1) / kWave;
    const PairBlock<P> blk(blockIdx.x, nblk, nch);
    const int lane = blk.lane, tid = threadIdx.x;
    const int wl = narrow ? lane / nb : 0;
    const int fl0 = narrow ? lane - wl * nb : lane;
    const bool busy = wl < gwin;
    const bool on_diagonal = blk.bi == blk.bj && blk.wi == blk.wj;   // the tile's (a, a) are (i, i)
    const int64_t seg = (int64_t)nch * nfreq;
    const cx *xk = X + (k0 + (busy ? wl : 0)) * mstep * seg;         // the window's first segment
    const double count = nsub, inv = 1.0 / nb;
    const int64_t square = (int64_t)nch * nch;
    const cx zero = {0.0, 0.0};
    double carry[3] = {0.0, 0.0, 0.0};                               // a long band's sums so far, per measure

    for (int pass = 0; pass < npass; ++pass) {
        const int fl = fl0 + pass * kWave;
        const bool inside = busy && fl < nb;
        const bool last = pass == npass - 1;
        const int span = narrow ? nb : (nb - pass * kWave < kWave ? nb - pass * kWave : kWave);
        int off[P::Rows];                                            // (-1: a row or a lane without a value)
#pragma unroll
        for (int k = 0; k < P::Rows; ++k) {
            const int c = blk.channel(k);
            off[k] = inside && c < nch ? c * nfreq + b0 + fl : -1;
        }

        // CROSS, LOCK: s0 = sum Re z, s1 = sum Im z; LAG: sum d, sum |d|, sum d^2, sum sign d
        double s0[P::T][P::T], s1[P::T][P::T], s2[P::T][P::T], s3[P::T][P::T];   // (CROSS, LOCK: two of them)
        double own_i[P::T], own_j[P::T];                             // sum |X|^2; LAG: K11's sum of pair_im(x, x)
#pragma unroll
        for (int a = 0; a < P::T; ++a) {
            own_i[a] = own_j[a] = 0.0;
#pragma unroll
            for (int b = 0; b < P::T; ++b) {
                s0[a][b] = s1[a][b] = s2[a][b] = s3[a][b] = 0.0;
            }
        }

        cx got[P::Rows];
        pair_walk(
            nsub, blk.active,
            [&](int s) {
                const cx *x = xk + s * seg;
#pragma unroll
                for (int k = 0; k < P::Rows; ++k) {
                    cx v = off[k] >= 0 ? x[off[k]] : zero;
                    if (G == kCohLock && off[k] >= 0) {                  // X / |X| as osz_unit_phasors: 0 gives NaN
                        const double r = hypot(v.x, v.y);
                        v.x /= r;
                        v.y /= r;
                    }
                    got[k] = v;
                }
            },
            [&](int buf) {
#pragma unroll
                for (int k = 0; k < P::Rows; ++k) stage[buf * 2 * P::B + blk.entry(k)][lane] = got[k];
            },
            [&](int cur) {
                cx u[P::T], v[P::T];
#pragma unroll
                for (int a = 0; a < P::T; ++a) u[a] = stage[cur * 2 * P::B + blk.slot_i(a)][lane];
#pragma unroll
                for (int b = 0; b < P::T; ++b) v[b] = stage[cur * 2 * P::B + blk.slot_j(b)][lane];
#pragma unroll
                for (int a = 0; a < P::T; ++a) {
                    if (G == kCohLag) {
                        own_i[a] += pair_im(u[a], u[a]);
                        own_j[a] += pair_im(v[a], v[a]);
                    } else {
                        own_i[a] = __builtin_fma(u[a].y, u[a].y, __builtin_fma(u[a].x, u[a].x, own_i[a]));
                        own_j[a] = __builtin_fma(v[a].y, v[a].y, __builtin_fma(v[a].x, v[a].x, own_j[a]));
                    }
                }
#pragma unroll
                for (int a = 0; a < P::T; ++a)
#pragma unroll
                    for (int b = 0; b < P::T; ++b) {
                        if (G == kCohLag) {                          // K11's arithmetic
                            const double d = pair_im(u[a], v[b]);
                            s0[a][b] += d;
                            s1[a][b] += __builtin_fabs(d);
                            s2[a][b] = __builtin_fma(d, d, s2[a][b]);
                            s3[a][b] += sign_of(d);
                        } else {                                     // K10's: four FMAs in a fixed order
                            double re = s0[a][b], im = s1[a][b];
                            re = __builtin_fma(u[a].x, v[b].x, re);
                            re = __builtin_fma(u[a].y, v[b].y, re);
                            im = __builtin_fma(u[a].x, v[b].y, im);
                            im = __builtin_fma(-u[a].y, v[b].x, im);
                            s0[a][b] = re;
                            s1[a][b] = im;
                        }
                    }
            });
        // (the walk ends behind a barrier: the stage is free)

        // One measure: the per-bin values of `value(a, b)` go to vals, the diagonal's as 0.0 or, for
        // a channel that is `lost(a)`, NaN; the fold; with the last pass the plane of measure m.
        auto measure = [&](int slot, int m, double diagonal, bool negated, auto lost, auto value) {
            // (every lane of an active wave writes its whole tile: what is no pair, or no bin of a
            // window, lies where the fold does not read)
            if (blk.active) {
#pragma unroll
                for (int a = 0; a < P::T; ++a)
#pragma unroll
                    for (int b = 0; b < P::T; ++b)
                        vals[((blk.wi * P::T + a) * P::B + blk.wj * P::T + b) * kCohPitch + lane] =
                            a == b && on_diagonal ? (lost(a) ? __builtin_nan("") : 0.0) : value(a, b);
            }
            __syncthreads();
            double *plane = out + (int64_t)__builtin_popcount(mask & ((1 << m) - 1)) * plane_pitch;
            const int rounds = (kCohPairs * gwin + P::Threads - 1) / P::Threads;
            for (int r = 0; r < rounds; ++r) {
                const int t = tid + r * P::Threads;
                const int q = t & (kCohPairs - 1), wloc = t / kCohPairs;
                const bool task = wloc < gwin;
                const int a = q / P::B, b = q % P::B;
                const int i = blk.bi * P::B + a, j = blk.bj * P::B + b;
                double s = narrow ? 0.0 : carry[slot];
                if (task) {
                    const double *p = vals + q * kCohPitch + (narrow ? wloc * nb : 0);
                    for (int e = 0; e < span; ++e) s += p[e];
                }
                if (!narrow) carry[slot] = s;
                if (!last) continue;                                 // (uniform: a long band's pass before its last)
                double v = s * inv;
                if (i == j) v = s != s ? s : diagonal;
                else if (negated && v == 0.0) v = 0.0;
                const int64_t at = ((k0 + wloc) * nbands + band) * square;
                if (task && j < nch && i <= j) plane[at + (int64_t)i * nch + j] = v;
                turn[tid] = negated && v != 0.0 ? -v : v;
                __syncthreads();
                const int i2 = blk.bi * P::B + b, j2 = blk.bj * P::B + a;    // the pair (b, a) of the block
                if (task && j2 < nch && i2 < j2) plane[at + (int64_t)j2 * nch + i2] = turn[(tid & ~(kCohPairs - 1)) | (b * P::B + a)];
                __syncthreads();
            }
            if (!last) __syncthreads();
        };

        if (G == kCohCross) {
            const auto lost = [&](int a) { return !(own_i[a] > 0.0); };
            if (mask & 1 << OSZ_WK_COH)
                measure(0, OSZ_WK_COH, 1.0, false, lost, [&](int a, int b) {
                    return (s0[a][b] * s0[a][b] + s1[a][b] * s1[a][b]) / (own_i[a] * own_j[b]);
                });
            if (mask & 1 << OSZ_WK_IMCOH)
                measure(1, OSZ_WK_IMCOH, 0.0, true, lost, [&](int a, int b) { return s1[a][b] / sqrt(own_i[a] * own_j[b]); });
        } else if (G == kCohLock) {
            measure(0, OSZ_WK_PLV, 1.0, false, [&](int a) { return own_i[a] != own_i[a]; },
                    [&](int a, int b) { return sqrt(s0[a][b] * s0[a][b] + s1[a][b] * s1[a][b]) / count; });
        } else {
            const auto lost = [&](int a) { return own_i[a] != own_i[a]; };
            if (mask & 1 << OSZ_WK_PLI)
                measure(0, OSZ_WK_PLI, 0.0, false, lost, [&](int a, int b) { return __builtin_fabs(s3[a][b]) / count; });
            if (mask & 1 << OSZ_WK_WPLI)
                measure(1, OSZ_WK_WPLI, 0.0, false, lost, [&](int a, int b) { return __builtin_fabs(s0[a][b]) / s1[a][b]; });
            if (mask & 1 << OSZ_WK_DWPLI)
                measure(2, OSZ_WK_DWPLI, 0.0, false, lost, [&](int a, int b) {
                    const double d = s0[a][b], q = s2[a][b], w = s1[a][b];
                    return (d * d - q) / (w * w - q);
                });
        }
    }
}

// the sizes both entry points refuse
inline bool wk_sizes(int64_t nseg, int nch, int nfreq, int nsub, int mstep, int nbands, int mask) {
    return nseg >= 0 && nseg <= INT32_MAX && nch >= 2 && nch <= 16384 && nfreq >= 2 &&
           (int64_t)nch * nfreq < ((int64_t)1 << 27) && nsub >= 2 && mstep >= 1 && nbands >= 1 &&
           nbands <= OSZ_WK_BANDS_MOST && mask >= 1 && mask < 1 << OSZ_WK_COUNT;
}

template <int G>
int wk_launch(const char *label, const cx *X, int nch, int nfreq, int nsub, int mstep, int64_t nwin, int64_t groups,
              const CohBands &bands, int nbands, int mask, double *out, int64_t plane_pitch, hipStream_t st) {
    int64_t nblk, tri;
    if (int rc = pair_grid("osz_window_coherence", nch, CohTile::B, &nblk, &tri)) return rc;
    KernelTimer timer(label, st);
    for (int64_t y0 = 0; y0 < groups; y0 += 65535) {                 // (a grid's y)
        const int64_t ny = std::min<int64_t>(65535, groups - y0);
        hipLaunchKernelGGL(window_coherence_kernel<G>, dim3((unsigned)tri, (unsigned)ny, (unsigned)nbands),
                           dim3(CohTile::Threads), 0, st, X, nch, nfreq, nsub, mstep, nwin, y0, bands, nbands, mask, out,
                           plane_pitch, (int)nblk);
        OSZ_HIP(hipGetLastError());
    }
    return OSZ_OK;
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_coherence_work(int64_t nseg, int nch, int nfreq, int nsub, int mstep, int nbands, int mask) {
    return wk_sizes(nseg, nch, nfreq, nsub, mstep, nbands, mask) ? 0 : -1;
}

int osz_window_coherence(const void *X, int64_t nseg, int nch, int nfreq, int nsub, int mstep, const int *bands,
                         int nbands, int mask, double *out, int64_t plane_pitch, double *work, int64_t work_len,
                         void *stream) {
    const char *fn = "osz_window_coherence";
    OSZ_REQUIRE(X && bands && out, "%s: null argument", fn);
    OSZ_REQUIRE(wk_sizes(nseg, nch, nfreq, nsub, mstep, nbands, mask),
                "%s: bad sizes or measures (nseg %lld, nch %d, nfreq %d, nsub %d, mstep %d, nbands %d, mask %d)", fn,
                (long long)nseg, nch, nfreq, nsub, mstep, nbands, mask);
    CohBands B;
    int64_t groups = 0;
    const int64_t nwin = nseg < nsub ? 0 : (nseg - nsub) / mstep + 1;    // (osz_window_count's, from nsub = 2 on)
    for (int b = 0; b < nbands; ++b) {
        const int b0 = bands[2 * b], b1 = bands[2 * b + 1];
        OSZ_REQUIRE(b0 >= 1 && b0 < b1 && b1 <= nfreq, "%s: band %d, bins [%d, %d), is empty or outside 1 .. %d", fn, b, b0,
                    b1, nfreq - 1);
        B.b[2 * b] = b0;
        B.b[2 * b + 1] = b1;
        const int nb = b1 - b0, g = nb <= kWave ? kWave / nb : 1;
        groups = std::max(groups, (nwin + g - 1) / g);
    }
    for (int b = 2 * nbands; b < 2 * OSZ_WK_BANDS_MOST; ++b) B.b[b] = 0;
    OSZ_REQUIRE(plane_pitch >= 0 && plane_pitch / ((int64_t)nbands * nch * nch) >= nwin, "%s: plane_pitch %lld holds fewer than %lld windows", fn,
                (long long)plane_pitch, (long long)nwin);
    OSZ_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(work) & 7) == 0,
                "%s: an array is not aligned (X: 16 bytes, out and work: 8)", fn);
    OSZ_REQUIRE(work_len >= 0, "%s: work holds %lld doubles, %s_work asks for 0", fn, (long long)work_len, fn);
    OSZ_REQUIRE(nwin <= INT32_MAX, "%s: too many windows in one push", fn);
    if (nwin == 0) return OSZ_OK;
    const cx *x = static_cast<const cx *>(X);
    hipStream_t st = as_stream(stream);
    if (mask & (1 << OSZ_WK_COH | 1 << OSZ_WK_IMCOH))
        if (int rc = wk_launch<kCohCross>("window_coherence_cross", x, nch, nfreq, nsub, mstep, nwin, groups, B, nbands, mask,
                                          out, plane_pitch, st))
            return rc;
    if (mask & 1 << OSZ_WK_PLV)
        if (int rc = wk_launch<kCohLock>("window_coherence_lock", x, nch, nfreq, nsub, mstep, nwin, groups, B, nbands, mask,
                                         out, plane_pitch, st))
            return rc;
    if (mask & (1 << OSZ_WK_PLI | 1 << OSZ_WK_WPLI | 1 << OSZ_WK_DWPLI))
        if (int rc = wk_launch<kCohLag>("window_coherence_lag", x, nch, nfreq, nsub, mstep, nwin, groups, B, nbands, mask, out,
                                        plane_pitch, st))
            return rc;
    return OSZ_OK;
}

}  // extern "C"
