// bispec.hip -- K14 Welch bispectrum per channel: with T = X[k1] X[k2] conj(X[k1 + k2]) of one
// segment spectrum, the raw sums over the segments
//   sums[0], sums[1] = Re, Im of sum T      sums[2] = sum |X[k1] X[k2]|^2
//   sums[3] = sum |X[k1]| |X[k2]| |X[k1 + k2]|  (= sum |T|)       power = sum |X|^2
// for the bin pairs k2 <= k1 of a band with k1 + k2 <= nfreq - 1 (the principal domain of a real
// signal), and the finishing pass (the mean bispectrum, the two bicoherences, both mirrors, NaN
// outside the domain).  DESIGN.md section 3, K14.
#include "common.h"

namespace osz {

typedef double cx __attribute__((ext_vector_type(2)));   // (re, im) of one complex128

constexpr int kBsR = 8;                          // k1 rows of a wave's register tile
constexpr int kBsH = 4;                          // rows whose X[k1] a wave asks for together
constexpr int kBsW = 4;                          // waves of a workgroup
constexpr int kBsRows = kBsR * kBsW;             // k1 rows of a workgroup's tile (32)
constexpr int kBsThreads = kWave * kBsW;         // 256
constexpr int kBsWin = kWave + kBsRows - 1;      // bins k1 + k2 a workgroup's tile reaches (95)

// Staging, once per (segment, channel, bin) so that the pair loop holds no square root: the plane
// mag = |X|, and power[c, k] += |X[s, c, k]|^2 in segment order from the stored sum.  A thread
// per (channel, bin); a wave's loads are 64 consecutive complex128.
__global__ void __launch_bounds__(256)
bispec_prepare_kernel(const cx *__restrict__ X, int nseg, int64_t plane, double *__restrict__ mag,
                      double *__restrict__ power) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= plane) return;
    double p = power[k];
    for (int s = 0; s < nseg; ++s) {
        const cx v = X[s * plane + k];
        mag[s * plane + k] = hypot(v.x, v.y);
        p += __builtin_fma(v.x, v.x, v.y * v.y);
    }
    power[k] = p;
}

// A lane is a k2 (the band's bins are the fastest axis of the sums: a wave's load of X[k2] is 64
// consecutive complex128), a wave keeps kBsR consecutive k1 rows x 4 sums in registers (64
// VGPRs), a workgroup is 4 such waves over the same 64 k2 of one channel, and the segments are
// walked in order from the stored sums: nothing is atomic and the result does not depend on
// where the stream is cut into pushes.  Per segment a wave needs
//   X[k1], |X[k1]| of its rows   wave-uniform: scalar loads, they occupy no vector register
//   X[k2], |X[k2]|               one coalesced load, fetched a segment ahead
//   X[k1 + k2], |X[k1 + k2]|     row r of lane l reads bin base + r + l: the 32 rows of the
//                                workgroup share ONE window of 95 consecutive bins, which the
//                                first 95 threads fetch a segment ahead and hand over through a
//                                double-buffered LDS stage, one barrier per segment; a row then
//                                reads it back at consecutive lanes (conflict-free).
// Twelve float64 instructions per (entry, segment), in this order: P = X1 X2 (2 mul, 2 fma),
// sum T += P conj(X3) (4 fma), sum |P|^2 (2 fma), sum |T| += (|X1| |X2|) |X3| (1 mul, 1 fma).
// Grid: x = block of 64 k2 (fastest), y = tile of 32 k1, z = channel.  A tile wholly above the
// diagonal (k2 > k1) or wholly outside the domain returns at once, a wave of that kind only
// helps with the staging; entries above the diagonal or outside the domain are not stored.
__global__ void __launch_bounds__(kBsThreads)
bispec_accumulate_kernel(const cx *__restrict__ X, const double *__restrict__ mag, int nseg, int nch, int nfreq,
                         int k_lo, int nb, double *__restrict__ sums) {
    __shared__ cx winx[2][kBsWin + 1];
    __shared__ double winm[2][kBsWin + 1];
    const int b0 = blockIdx.x * kWave, a0 = blockIdx.y * kBsRows, c = blockIdx.z;
    const int last = nfreq - 1;                           // the largest k1 + k2 of the domain
    if (b0 > a0 + kBsRows - 1 || 2 * k_lo + a0 + b0 > last) return;
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int aw = a0 + w * kBsR;                         // the wave's first row
    const bool active = aw < nb && b0 <= aw + kBsR - 1 && 2 * k_lo + aw + b0 <= last;
    const int b = b0 + lane;
    const bool have2 = b < nb;
    const int k3 = 2 * k_lo + a0 + b0 + t;                // the window bin this thread stages
    const bool havew = t < kBsWin && k3 <= last;
    // (a uniform base that moves from segment to segment plus a 32-bit offset)
    const int64_t seg = (int64_t)nch * nfreq;
    const int row = c * nfreq;
    const int o2 = row + (have2 ? k_lo + b : 0), ow = row + (havew ? k3 : 0);
    unsigned o1[kBsR];                                    // byte offsets into the plane |X| (below 2^30)
#pragma unroll
    for (int r = 0; r < kBsR; ++r) o1[r] = 8u * (unsigned)(row + min(k_lo + aw + r, last));   // (rows past the band are not stored)
    const int64_t nn = (int64_t)nb * nb, cnn = (int64_t)nch * nn;
    const cx zero = {0.0, 0.0};

    // the entries of row a this lane owns: below the diagonal, inside the band and the domain
    auto keep = [&](int a) { return active && have2 && a < nb && b <= a && 2 * k_lo + a + b <= last; };
    double sre[kBsR], sim[kBsR], spp[kBsR], smm[kBsR];
#pragma unroll
    for (int r = 0; r < kBsR; ++r) {
        const int a = aw + r;
        const bool mine = keep(a);
        const int64_t at = c * nn + (int64_t)a * nb + b;
        sre[r] = mine ? sums[at] : 0.0;
        sim[r] = mine ? sums[cnn + at] : 0.0;
        spp[r] = mine ? sums[2 * cnn + at] : 0.0;
        smm[r] = mine ? sums[3 * cnn + at] : 0.0;
    }

    cx x2 = have2 ? X[o2] : zero, gw = havew ? X[ow] : zero;
    double m2 = have2 ? mag[o2] : 0.0, gm = havew ? mag[ow] : 0.0;
    cx g2 = x2;
    double gm2 = m2;
    if (t < kBsWin) {
        winx[0][t] = gw;
        winm[0][t] = gm;
    }
    __syncthreads();
    for (int s = 0; s < nseg; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < nseg;
        const cx *Xs = X + s * seg;
        const double *ms = mag + s * seg;
        if (more) {
            g2 = have2 ? Xs[seg + o2] : zero;
            gm2 = have2 ? ms[seg + o2] : 0.0;
            gw = havew ? Xs[seg + ow] : zero;
            gm = havew ? ms[seg + ow] : 0.0;
        }
        if (active) {
#pragma unroll
            for (int h = 0; h < kBsR; h += kBsH) {
                cx x1[kBsH];                              // wave-uniform: half the rows asked for at once
                double m1[kBsH];
#pragma unroll
                for (int q = 0; q < kBsH; ++q) {
                    x1[q] = *reinterpret_cast<const cx *>(reinterpret_cast<const char *>(Xs) + 2 * o1[h + q]);
                    m1[q] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(ms) + o1[h + q]);
                }
#pragma unroll
                for (int q = 0; q < kBsH; ++q) {
                    const int r = h + q;
                    const cx x3 = winx[cur][w * kBsR + r + lane];
                    const double m3 = winm[cur][w * kBsR + r + lane];
                    double pr = x1[q].x * x2.x, pi = x1[q].x * x2.y;
                    pr = __builtin_fma(-x1[q].y, x2.y, pr);
                    pi = __builtin_fma(x1[q].y, x2.x, pi);
                    // P conj(X3) = (pr x3r + pi x3i) + i (pi x3r - pr x3i)
                    sre[r] = __builtin_fma(pr, x3.x, sre[r]);
                    sre[r] = __builtin_fma(pi, x3.y, sre[r]);
                    sim[r] = __builtin_fma(pi, x3.x, sim[r]);
                    sim[r] = __builtin_fma(-pr, x3.y, sim[r]);
                    spp[r] = __builtin_fma(pr, pr, spp[r]);
                    spp[r] = __builtin_fma(pi, pi, spp[r]);
                    smm[r] = __builtin_fma(m1[q] * m2, m3, smm[r]);
                }
            }
        }
        if (more) {
            if (t < kBsWin) {
                winx[cur ^ 1][t] = gw;
                winm[cur ^ 1][t] = gm;
            }
            x2 = g2;
            m2 = gm2;
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < kBsR; ++r) {
        if (!keep(aw + r)) continue;
        const int64_t at = c * nn + (int64_t)(aw + r) * nb + b;
        sums[at] = sre[r];
        sums[cnn + at] = sim[r];
        sums[2 * cnn + at] = spp[r];
        sums[3 * cnn + at] = smm[r];
    }
}

// One band-bin pair b <= a per thread (grid: x = block of 256 b, y = a, z = channel); writes
// [a, b] and its mirror [b, a].  Outside the domain both are NaN, written and not computed.
// Spectrum: sum T / count.  Kim: |sum T|^2 / (sum |X1 X2|^2 sum |X3|^2).  Hagihira: |sum T| /
// sum |T|.  A zero denominator gives what IEEE gives.
__global__ void __launch_bounds__(256)
bispec_finish_kernel(int mode, const double *__restrict__ sums, const double *__restrict__ power, double count,
                     int nch, int nfreq, int k_lo, int nb, void *__restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y, c = blockIdx.z;
    if (b > a) return;
    const int64_t nn = (int64_t)nb * nb, cnn = (int64_t)nch * nn;
    const int64_t ab = c * nn + (int64_t)a * nb + b, ba = c * nn + (int64_t)b * nb + a;
    const int k3 = 2 * k_lo + a + b;
    const bool inside = k3 <= nfreq - 1;
    const double nan = __builtin_nan("");
    const double re = inside ? sums[ab] : nan, im = inside ? sums[cnn + ab] : nan;
    if (mode == OSZ_BISPEC_SPECTRUM) {
        cx *o = static_cast<cx *>(out);
        const cx v = {re / count, im / count};
        o[ab] = v;
        o[ba] = v;
        return;
    }
    double v = nan;
    if (inside) {
        if (mode == OSZ_BISPEC_KIM)
            v = __builtin_fma(re, re, im * im) / (sums[2 * cnn + ab] * power[(int64_t)c * nfreq + k3]);
        else
            v = hypot(re, im) / sums[3 * cnn + ab];
    }
    double *o = static_cast<double *>(out);
    o[ab] = v;
    o[ba] = v;
}

static bool bs_sizes_ok(int64_t nseg, int nch, int nfreq) {
    return nseg >= 0 && nseg <= INT32_MAX && nch >= 1 && nch <= 65535 && nfreq >= 1 &&
           (int64_t)nch * nfreq < ((int64_t)1 << 27);
}

static bool bs_band_ok(int nch, int nfreq, int k_lo, int nb) {
    // (k_lo + nb <= nfreq bounds nb; the offsets of the sums are 64-bit)
    return k_lo >= 0 && nb >= 1 && (int64_t)k_lo + nb <= nfreq && (nb + kBsRows - 1) / kBsRows <= 65535 && nb <= 65535;
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_bispec_work(int64_t nseg, int nch, int nfreq) {
    if (!bs_sizes_ok(nseg, nch, nfreq)) return -1;
    return nseg * nch * nfreq;
}

int osz_bispec_accumulate(const void *X, int64_t nseg, int nch, int nfreq, int k_lo, int nb, double *sums,
                          double *power, double *work, int64_t work_len, void *stream) {
    OSZ_REQUIRE(X && sums && power && work, "osz_bispec_accumulate: null argument");
    OSZ_REQUIRE(bs_sizes_ok(nseg, nch, nfreq),
                "osz_bispec_accumulate: bad sizes (nch * nfreq must stay below 2^27)");
    OSZ_REQUIRE(bs_band_ok(nch, nfreq, k_lo, nb),
                "osz_bispec_accumulate: the band [%d, %d + %d) does not lie in the %d bins", k_lo, k_lo, nb, nfreq);
    OSZ_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
                    ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(power) |
                      reinterpret_cast<uintptr_t>(work)) & 7) == 0,
                "osz_bispec_accumulate: X must be 16-byte aligned, the float64 arrays 8-byte aligned");
    OSZ_REQUIRE(work_len >= osz_bispec_work(nseg, nch, nfreq),
                "osz_bispec_accumulate: work holds %lld doubles, osz_bispec_work asks for %lld",
                (long long)work_len, (long long)osz_bispec_work(nseg, nch, nfreq));
    if (nseg == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    const int64_t plane = (int64_t)nch * nfreq;
    {
        KernelTimer timer("bispec_prepare", st);
        hipLaunchKernelGGL(bispec_prepare_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st,
                           static_cast<const cx *>(X), (int)nseg, plane, work, power);
        OSZ_HIP(hipGetLastError());
    }
    // tiles below the diagonal only: the row tiles reach the band's end, a row tile's k2 blocks its last row
    KernelTimer timer("bispec_accumulate", st);
    const dim3 grid((unsigned)((nb + kWave - 1) / kWave), (unsigned)((nb + kBsRows - 1) / kBsRows), (unsigned)nch);
    hipLaunchKernelGGL(bispec_accumulate_kernel, grid, dim3(kBsThreads), 0, st, static_cast<const cx *>(X),
                       static_cast<const double *>(work), (int)nseg, nch, nfreq, k_lo, nb, sums);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int osz_bispec_finish(int mode, const double *sums, const double *power, int64_t count, int nch, int nfreq,
                      int k_lo, int nb, void *out, void *stream) {
    OSZ_REQUIRE(mode == OSZ_BISPEC_SPECTRUM || mode == OSZ_BISPEC_KIM || mode == OSZ_BISPEC_HAGIHIRA,
                "osz_bispec_finish: unknown mode %d", mode);
    OSZ_REQUIRE(sums && power && out, "osz_bispec_finish: null argument");
    OSZ_REQUIRE(bs_sizes_ok(0, nch, nfreq) && count >= 1, "osz_bispec_finish: bad sizes");
    OSZ_REQUIRE(bs_band_ok(nch, nfreq, k_lo, nb),
                "osz_bispec_finish: the band [%d, %d + %d) does not lie in the %d bins", k_lo, k_lo, nb, nfreq);
    OSZ_REQUIRE(out != sums, "osz_bispec_finish: the result cannot overwrite the sums");
    OSZ_REQUIRE((reinterpret_cast<uintptr_t>(out) & (mode == OSZ_BISPEC_SPECTRUM ? 15 : 7)) == 0,
                "osz_bispec_finish: out is not aligned");
    KernelTimer timer("bispec_finish", as_stream(stream));
    hipLaunchKernelGGL(bispec_finish_kernel, dim3((unsigned)((nb + 255) / 256), (unsigned)nb, (unsigned)nch), dim3(256),
                       0, as_stream(stream), mode, sums, power, (double)count, nch, nfreq, k_lo, nb, out);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
