// jackknife.hip -- K12 delete-one jackknife over the Welch segments for coherence and the five
// phase measures of K11: a second pass over the segment spectra that, per (pair, bin), forms the
// measure without segment s from the downdated totals (the totals of K10 / K11 minus segment s's
// contribution) and adds d_s = theta_(s) - theta and d_s^2 in segment order, and the finishing
// pass se = sqrt((N - 1) / N (sum d^2 - (sum d)^2 / N)) with its fixed points.  DESIGN.md
// section 3, K12.
#include "pair_tile.h"

namespace osz {

// K11's workgroup: 2 x 2 waves, an 8 x 8 block of pairs, wave w stages rows 4w .. 4w + 3 of the list
using JackTile = PairTile<2, 1, false>;
constexpr int kJackT = JackTile::T, kJackB = JackTile::B, kJackRows = JackTile::Rows;

// The tile shape of pair_tile.h, a lane a frequency bin, with the walk and the tile loops written
// out: five of the six instances hold 256 VGPRs and more in AGPRs at one wave per SIMD, where
// the compiler's schedule decides their speed, and on pair_walk / PairBlock::pairs four of them
// ran 1.3 to 3.7 % slower (profiles/pair_tile_ab.txt).  Per pair the lane holds the totals the
// measure reads (1 to 3 doubles), theta from all segments and the two running sums, loaded from
// dev2 at the start and stored at the end.  One measure per launch, MODE a template argument, so
// a launch carries only its own registers (4 to 6 doubles per pair).
// coherence / imcoh: the staging wave also stages, next to each row, 1 / (P_c - |X_c|^2)
// (coherence) or its square root (imcoh), P_c = Re acc[c, c] -- one division (and one square
// root) per (channel, segment, bin) instead of one per (pair, segment, bin); the pair loop
// multiplies.  theta is formed by the same expression as theta_(s), with nothing taken away.
// plv reads spectra that osz_unit_phasors normalised and the sums of K10 over those.
// d = Im(conj(u) v) is pair_im, the expression of lag_accumulate_kernel.
// Grid: x = triangular block index, y = bin block.
template <int MODE>
__global__ void __launch_bounds__(JackTile::Threads)
jackknife_accumulate_kernel(const cx *__restrict__ X, int nseg, int nch, int nfreq, const cx *__restrict__ csum,
                            const double *__restrict__ lag, double count, double *__restrict__ dev2, int nblk) {
    constexpr bool kPower = MODE == OSZ_JACK_COHERENCE || MODE == OSZ_JACK_IMCOH;
    constexpr bool kComplex = MODE == OSZ_JACK_COHERENCE || MODE == OSZ_JACK_PLV;      // both parts of z
    __shared__ cx stage[2][2 * kJackB][kWave];                                          // 32 KB
    __shared__ double aux[kPower ? 2 : 1][kPower ? 2 * kJackB : 1][kPower ? kWave : 1]; // 16 KB
    const PairBlock<JackTile> blk(blockIdx.x, nblk, nch);
    const int lane = blk.lane, i0 = blk.i0, j0 = blk.j0;
    const bool active = blk.active;
    const int f = blockIdx.y * kWave + lane;
    const bool inside = f < nfreq;
    // the rows this wave stages
    const int64_t seg = (int64_t)nch * nfreq;
    int off[kJackRows];
    bool have[kJackRows];
    double own[kJackRows];                               // P_c of the staged rows (coherence, imcoh)
#pragma unroll
    for (int k = 0; k < kJackRows; ++k) {
        const int c = blk.channel(k);
        have[k] = inside && c < nch;
        off[k] = have[k] ? c * nfreq + f : 0;
        own[k] = 0.0;
        if constexpr (kPower) own[k] = have[k] ? csum[pair_at(c, c, nch, nfreq, f)].x : 0.0;
    }
    const int64_t plane = (int64_t)nch * nch * nfreq;
    const cx zero = {0.0, 0.0};
    const double rn = 1.0 / count, rn1 = 1.0 / (count - 1.0);

    // what a staged row carries beside the spectrum value x, from its channel's total P
    auto beside = [](double P, cx x) {
        const double left = P - __builtin_fma(x.x, x.x, x.y * x.y);
        return MODE == OSZ_JACK_COHERENCE ? 1.0 / left : 1.0 / sqrt(left);
    };

    // the totals of the pair (t0, t1, t2: as many as the measure reads), theta, the running sums
    double t0[kJackT][kJackT], t1[kJackT][kJackT], t2[kJackT][kJackT];
    double th[kJackT][kJackT], s1[kJackT][kJackT], s2[kJackT][kJackT];
    double pu[kJackT], pv[kJackT];                       // (coherence, imcoh) 1 / P or 1 / sqrt(P)
#pragma unroll
    for (int a = 0; a < kJackT; ++a) {
        pu[a] = pv[a] = 0.0;
        if constexpr (kPower) {
            const int i = i0 + a, j = j0 + a;
            const bool hi = active && inside && i < nch, hj = active && inside && j < nch;
            pu[a] = beside(hi ? csum[((int64_t)i * nch + i) * nfreq + f].x : 0.0, zero);
            pv[a] = beside(hj ? csum[((int64_t)j * nch + j) * nfreq + f].x : 0.0, zero);
        }
    }
#pragma unroll
    for (int a = 0; a < kJackT; ++a)
#pragma unroll
        for (int b = 0; b < kJackT; ++b) {
            const int i = i0 + a, j = j0 + b;
            const bool mine = active && inside && j < nch && i <= j;
            const int64_t at = ((int64_t)i * nch + j) * nfreq + f;
            s1[a][b] = mine ? dev2[at] : 0.0;
            s2[a][b] = mine ? dev2[plane + at] : 0.0;
            t0[a][b] = t1[a][b] = t2[a][b] = 0.0;
            if constexpr (MODE == OSZ_JACK_COHERENCE) {
                const cx A = mine ? csum[at] : zero;
                t0[a][b] = A.x;
                t1[a][b] = A.y;
                th[a][b] = __builtin_fma(A.x, A.x, A.y * A.y) * (pu[a] * pv[b]);
            } else if constexpr (MODE == OSZ_JACK_IMCOH) {
                t0[a][b] = mine ? csum[at].y : 0.0;
                th[a][b] = t0[a][b] * (pu[a] * pv[b]);
            } else if constexpr (MODE == OSZ_JACK_PLV) {
                const cx U = mine ? csum[at] : zero;
                t0[a][b] = U.x;
                t1[a][b] = U.y;
                th[a][b] = sqrt(__builtin_fma(U.x, U.x, U.y * U.y)) * rn;
            } else if constexpr (MODE == OSZ_JACK_PLI) {
                t0[a][b] = mine ? lag[3 * plane + at] : 0.0;
                th[a][b] = __builtin_fabs(t0[a][b]) * rn;
            } else if constexpr (MODE == OSZ_JACK_WPLI) {
                t0[a][b] = mine ? lag[at] : 0.0;
                t1[a][b] = mine ? lag[plane + at] : 0.0;
                th[a][b] = __builtin_fabs(t0[a][b]) / t1[a][b];
            } else {
                t0[a][b] = mine ? lag[at] : 0.0;
                t1[a][b] = mine ? lag[plane + at] : 0.0;
                t2[a][b] = mine ? lag[2 * plane + at] : 0.0;
                th[a][b] = __builtin_fma(t0[a][b], t0[a][b], -t2[a][b]) /
                           __builtin_fma(t1[a][b], t1[a][b], -t2[a][b]);
            }
        }

    cx g[kJackRows];
#pragma unroll
    for (int k = 0; k < kJackRows; ++k) {
        g[k] = have[k] ? X[off[k]] : zero;
        stage[0][blk.entry(k)][lane] = g[k];
        if constexpr (kPower) aux[0][blk.entry(k)][lane] = beside(own[k], g[k]);
    }
    __syncthreads();
    for (int s = 0; s < nseg; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < nseg;
        if (more) {
            X += seg;
#pragma unroll
            for (int k = 0; k < kJackRows; ++k) g[k] = have[k] ? X[off[k]] : zero;
        }
        if (active) {
            cx u[kJackT], v[kJackT];
            double ru[kJackT], rv[kJackT];
#pragma unroll
            for (int a = 0; a < kJackT; ++a) {
                u[a] = stage[cur][blk.slot_i(a)][lane];
                v[a] = stage[cur][blk.slot_j(a)][lane];
                ru[a] = rv[a] = 0.0;
                if constexpr (kPower) {
                    ru[a] = aux[cur][blk.slot_i(a)][lane];
                    rv[a] = aux[cur][blk.slot_j(a)][lane];
                }
            }
#pragma unroll
            for (int a = 0; a < kJackT; ++a)
#pragma unroll
                for (int b = 0; b < kJackT; ++b) {
                    const double d = pair_im(u[a], v[b]);            // (as K11 sums it)
                    double re = 0.0;
                    if constexpr (kComplex) re = pair_re(u[a], v[b]);
                    double left;                                     // theta without segment s
                    if constexpr (MODE == OSZ_JACK_COHERENCE) {
                        const double ar = t0[a][b] - re, ai = t1[a][b] - d;
                        left = __builtin_fma(ar, ar, ai * ai) * (ru[a] * rv[b]);
                    } else if constexpr (MODE == OSZ_JACK_IMCOH) {
                        left = (t0[a][b] - d) * (ru[a] * rv[b]);
                    } else if constexpr (MODE == OSZ_JACK_PLV) {
                        const double ar = t0[a][b] - re, ai = t1[a][b] - d;
                        left = sqrt(__builtin_fma(ar, ar, ai * ai)) * rn1;
                    } else if constexpr (MODE == OSZ_JACK_PLI) {
                        left = __builtin_fabs(t0[a][b] - sign_of(d)) * rn1;
                    } else if constexpr (MODE == OSZ_JACK_WPLI) {
                        left = __builtin_fabs(t0[a][b] - d) / (t1[a][b] - __builtin_fabs(d));
                    } else {
                        const double dn = t0[a][b] - d, bn = t1[a][b] - __builtin_fabs(d);
                        const double qn = __builtin_fma(-d, d, t2[a][b]);
                        left = __builtin_fma(dn, dn, -qn) / __builtin_fma(bn, bn, -qn);
                        // (one segment left: d^2 - d^2 over |d|^2 - d^2, which the downdate only rounds to)
                        if (count == 2.0) left = __builtin_nan("");
                    }
                    const double dev = left - th[a][b];
                    s1[a][b] += dev;
                    s2[a][b] = __builtin_fma(dev, dev, s2[a][b]);
                }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < kJackRows; ++k) {
                stage[cur ^ 1][blk.entry(k)][lane] = g[k];
                if constexpr (kPower) aux[cur ^ 1][blk.entry(k)][lane] = beside(own[k], g[k]);
            }
        }
        __syncthreads();
    }

    if (active && inside) {
#pragma unroll
        for (int a = 0; a < kJackT; ++a)
#pragma unroll
            for (int b = 0; b < kJackT; ++b) {
                const int i = i0 + a, j = j0 + b;
                if (j < nch && i <= j) {
                    const int64_t at = pair_at(i, j, nch, nfreq, f);
                    dev2[at] = s1[a][b];
                    dev2[plane + at] = s2[a][b];
                }
            }
    }
}

// One (i <= j) pair per (blockIdx.z, blockIdx.y), a lane per bin; writes [i, j] and its mirror
// [j, i], the same value for every measure (imcoh's deviations change sign together).  In the
// order of phase_finish_kernel: a channel whose own sums (the diagonal entry of the totals the
// measure reads) are NaN gives NaN; the diagonal is 0.0; the real bins (DC, and Nyquist for even
// nfft) are 0.0 for all but plv; everything else is the definition, the variance clamped at the
// rounding of its own subtraction before the square root, a NaN left as it is.
__global__ void __launch_bounds__(256)
jackknife_finish_kernel(int mode, const double *dev2, const cx *csum, const double *lag, double count, int nch,
                        int nfreq, int nfft_is_even, double *out) {
    const PairBin p(nch, nfreq, nfft_is_even);
    if (!p.valid) return;
    const bool on_lag = mode >= OSZ_JACK_PLI;
    const double own_i = on_lag ? lag[p.ii] : csum[p.ii].x, own_j = on_lag ? lag[p.jj] : csum[p.jj].x;
    const double sum = dev2[p.ij], squares = dev2[p.plane + p.ij];
    // sum d^2 - (sum d)^2 / N carries up to (3 N + 1) roundings of sum d^2: what does not exceed
    // them is the 0 of deviations that are equal to within rounding (and a negative value is)
    double v = squares - sum * sum / count;
    v = v <= 4.0 * count * 0x1p-53 * squares ? 0.0 : v;              // (false for a NaN: it stays)
    v = sqrt((count - 1.0) / count * v);
    if (own_i != own_i || own_j != own_j) v = __builtin_nan("");
    else if (p.i == p.j) v = 0.0;
    else if (p.real_bin && mode != OSZ_JACK_PLV) v = 0.0;
    out[p.ij] = v;
    if (p.i != p.j) out[p.ji] = v;
}

static const char *jack_reads(int mode) {
    return mode <= OSZ_JACK_IMCOH ? "acc" : mode == OSZ_JACK_PLV ? "accn" : "lag";
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_jackknife_accumulate(int mode, const void *X, int64_t nseg, int nch, int nfreq, const void *acc,
                             const void *accn, const double *lag, int64_t count, double *dev2, void *stream) {
    OSZ_REQUIRE(mode >= OSZ_JACK_COHERENCE && mode <= OSZ_JACK_DWPLI, "osz_jackknife_accumulate: unknown mode %d", mode);
    const void *csum = mode <= OSZ_JACK_IMCOH ? acc : accn;
    const void *sums = mode <= OSZ_JACK_PLV ? csum : static_cast<const void *>(lag);
    OSZ_REQUIRE(X && sums && dev2, "osz_jackknife_accumulate: null argument (mode %d reads %s)", mode, jack_reads(mode));
    int64_t nblk, tri;
    if (int rc = pair_grid("osz_jackknife_accumulate", nch, JackTile::B, &nblk, &tri)) return rc;
    OSZ_REQUIRE(nfreq >= 1 && nseg >= 0 && nseg <= INT32_MAX && (int64_t)nch * nfreq < ((int64_t)1 << 27),
                "osz_jackknife_accumulate: bad sizes (nch * nfreq must stay below 2^27)");
    OSZ_REQUIRE(count >= 2 && nseg <= count, "osz_jackknife_accumulate: the totals must be those of at least two "
                                             "segments and of no fewer than this push holds");
    OSZ_REQUIRE(static_cast<const void *>(dev2) != sums && static_cast<const void *>(dev2) != X,
                "osz_jackknife_accumulate: dev2 cannot be the totals or the spectra");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(dev2)) & 15) == 0,
                "osz_jackknife_accumulate: X, the totals and dev2 must be 16-byte aligned");
    if (nseg == 0) return OSZ_OK;
    const int64_t fblk = ((int64_t)nfreq + kWave - 1) / kWave;
    OSZ_REQUIRE(fblk <= 65535, "osz_jackknife_accumulate: grid too large");
    KernelTimer timer("jackknife_accumulate", as_stream(stream));
    const dim3 grid((unsigned)tri, (unsigned)fblk), block(JackTile::Threads);
    const cx *x = static_cast<const cx *>(X), *c = static_cast<const cx *>(csum);
#define OSZ_JACK_LAUNCH(M)                                                                                        \
    case M:                                                                                                       \
        hipLaunchKernelGGL(jackknife_accumulate_kernel<M>, grid, block, 0, as_stream(stream), x, (int)nseg, nch, \
                           nfreq, c, lag, (double)count, dev2, (int)nblk);                                        \
        break;
    switch (mode) {
        OSZ_JACK_LAUNCH(OSZ_JACK_COHERENCE)
        OSZ_JACK_LAUNCH(OSZ_JACK_IMCOH)
        OSZ_JACK_LAUNCH(OSZ_JACK_PLV)
        OSZ_JACK_LAUNCH(OSZ_JACK_PLI)
        OSZ_JACK_LAUNCH(OSZ_JACK_WPLI)
        OSZ_JACK_LAUNCH(OSZ_JACK_DWPLI)
    }
#undef OSZ_JACK_LAUNCH
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_jackknife_finish(int mode, const double *dev2, const void *acc, const void *accn, const double *lag,
                         int64_t count, int nch, int nfreq, int nfft_is_even, double *out, void *stream) {
    OSZ_REQUIRE(mode >= OSZ_JACK_COHERENCE && mode <= OSZ_JACK_DWPLI, "osz_jackknife_finish: unknown mode %d", mode);
    const void *csum = mode <= OSZ_JACK_IMCOH ? acc : accn;
    const void *sums = mode <= OSZ_JACK_PLV ? csum : static_cast<const void *>(lag);
    OSZ_REQUIRE(dev2 && sums && out, "osz_jackknife_finish: null argument (mode %d reads %s)", mode, jack_reads(mode));
    OSZ_REQUIRE(nch >= 1 && nch <= 65535 && nfreq >= 1 && count >= 2, "osz_jackknife_finish: bad sizes");
    OSZ_REQUIRE(out != dev2 && static_cast<const void *>(out) != sums,
                "osz_jackknife_finish: the result cannot overwrite the sums");
    OSZ_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(dev2)) & 15) == 0,
                "osz_jackknife_finish: the sums and out must be 16-byte aligned");
    KernelTimer timer("jackknife_finish", as_stream(stream));
    hipLaunchKernelGGL(jackknife_finish_kernel, dim3((unsigned)((nfreq + 255) / 256), nch, nch), dim3(256), 0,
                       as_stream(stream), mode, dev2, static_cast<const cx *>(csum), lag, (double)count, nch, nfreq,
                       nfft_is_even, out);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
