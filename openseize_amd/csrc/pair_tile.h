// pair_tile.h -- the tile skeleton of the all-pairs accumulate kernels (K10 cross.hip, K11
// phaseconn.hip, K12 jackknife.hip, K13 pairtime.hip) and the small pieces their finishing
// passes and host entry points share.  DESIGN.md section 3, K10.
//
// A lane is one position of the axis that pairs do not cross (a frequency bin; in K13 a sample
// of a 64-sample step) and keeps a T x T = 4 x 4 tile of channel pairs in registers.  A
// workgroup of W x W waves owns 64 such positions of a B x B block of pairs, B = 4 W, block row
// bi <= block column bj: grid x is the index of the block in the upper triangle (fastest, so the
// workgroups resident together share the step's rows in L2).  On a diagonal block the waves
// below the diagonal rest.  Per step (a segment, 64 samples) the workgroup needs the B + B
// channel rows of the two sets, NV values each: the 2 B NV staged entries are dealt to the
// waves, every wave fetches its Rows entries one step ahead of the arithmetic into registers
// (coalesced, once per workgroup instead of once per wave that uses them) and hands them over
// through a double-buffered LDS stage, one barrier per step; every wave then reads its T + T
// rows back as consecutive lanes (conflict-free).  The steps are walked in order from the stored
// sums and nothing is atomic, so the sums do not depend on where a stream is cut into pushes.
// The kernels keep what differs: the LDS arrays and their sizes, the sums, the arithmetic.  (K12
// takes the tile and the block but writes the walk out: jackknife.hip says why.)
#pragma once
#include "common.h"

namespace osz {

typedef double cx __attribute__((ext_vector_type(2)));   // (re, im) of one complex128

// Im and Re of conj(u) v, each one product rounded and one fused.  Every sum of d = Im(conj(u) v)
// in K11, K12 and K13 is fed from pair_im: they carry the same bits.
__device__ __forceinline__ double pair_im(double ur, double ui, double vr, double vi) {
    return __builtin_fma(ur, vi, -(ui * vr));
}
__device__ __forceinline__ double pair_re(double ur, double ui, double vr, double vi) {
    return __builtin_fma(ur, vr, ui * vi);
}
__device__ __forceinline__ double pair_im(cx u, cx v) { return pair_im(u.x, u.y, v.x, v.y); }
__device__ __forceinline__ double pair_re(cx u, cx v) { return pair_re(u.x, u.y, v.x, v.y); }

// sign(d) as the sums of K11 take it: +-0 gives 0 (d itself), NaN gives NaN
__device__ __forceinline__ double sign_of(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d); }

// Pearson r from the five sums over `cnt` samples; a zero variance gives what IEEE gives.
__device__ __forceinline__ double pearson(double cnt, double sp, double sq, double spp, double sqq, double spq) {
    const double cov = __builtin_fma(cnt, spq, -(sp * sq));
    const double vp = __builtin_fma(cnt, spp, -(sp * sp));
    const double vq = __builtin_fma(cnt, sqq, -(sq * sq));
    return cov / (sqrt(vp) * sqrt(vq));
}

// Block p of the upper triangle of nblk x nblk blocks, rows first: row bi holds nblk - bi blocks.
__device__ __forceinline__ void pair_triangle(int p, int nblk, int *bi, int *bj) {
    int r = 0;
    while (p >= nblk - r) {
        p -= nblk - r;
        ++r;
    }
    *bi = r;
    *bj = r + p;
}

// [i, j, f] of an (nch, nch, nfreq) plane
__device__ __forceinline__ int64_t pair_at(int i, int j, int nch, int nfreq, int f) {
    return ((int64_t)i * nch + j) * nfreq + f;
}

// The constants of a W x W-wave workgroup whose staged rows carry NV values each.  The staged
// entries are a list: entry e is value e % NV of slot e / NV, slots 0 .. B - 1 block row bi's
// channels, B .. 2 B - 1 bj's.  DEALT says which entries a wave fetches, which decides the
// global-load pattern: wave w takes entries w, Waves + w, ... (K10: row w of either set), or
// else the run w Rows .. w Rows + Rows - 1 (K11 - K13).
template <int W_, int NV_, bool DEALT>
struct PairTile {
    static constexpr int T = 4, W = W_, NV = NV_, B = T * W, Waves = W * W, Threads = kWave * Waves;
    static constexpr int Rows = 2 * B * NV / Waves;      // staged entries per wave and step
    static_assert(2 * B * NV % Waves == 0, "the staged entries divide evenly among the waves");
    __device__ static __forceinline__ int entry(int w, int k) { return DEALT ? k * Waves + w : w * Rows + k; }
};

// Where a thread stands in its workgroup's block of pairs.
template <class P>
struct PairBlock {
    int bi, bj, lane, w, wi, wj;
    int i0, j0;                                          // the first pair of the lane's 4 x 4 tile
    bool active;                                         // false for a wave that rests
    __device__ __forceinline__ PairBlock(int p, int nblk, int nch) {
        pair_triangle(p, nblk, &bi, &bj);
        lane = threadIdx.x & (kWave - 1);
        w = threadIdx.x >> 6;
        wi = w / P::W;
        wj = w % P::W;
        i0 = bi * P::B + wi * P::T;
        j0 = bj * P::B + wj * P::T;
        active = i0 < nch && j0 < nch && (bi != bj || wi <= wj);
    }
    // the k-th staged entry of this wave: its place in the list, its value and its channel
    __device__ __forceinline__ int entry(int k) const { return P::entry(w, k); }
    __device__ __forceinline__ int value(int k) const { return entry(k) % P::NV; }
    __device__ __forceinline__ int channel(int k) const {
        const int r = entry(k) / P::NV;
        return r < P::B ? bi * P::B + r : bj * P::B + r - P::B;
    }
    // the staged slots the tile's rows a and columns b are read back from
    __device__ __forceinline__ int slot_i(int a) const { return wi * P::T + a; }
    __device__ __forceinline__ int slot_j(int b) const { return P::B + wj * P::T + b; }
    // f(a, b, mine, i, j) over the tile; `mine` is the one predicate under which a pair's sums
    // are loaded and stored: the lane is `inside` its axis and (i, j) is a pair with i <= j.
    template <class F>
    __device__ __forceinline__ void pairs(int nch, bool inside, F f) const {
#pragma unroll
        for (int a = 0; a < P::T; ++a)
#pragma unroll
            for (int b = 0; b < P::T; ++b) {
                const int i = i0 + a, j = j0 + b;
                f(a, b, active && inside && j < nch && i <= j, i, j);
            }
    }
};

// The walk over nsteps steps: fetch(s) loads step s's entries into registers, put(buf) writes
// them to stage buffer buf, work(buf) is the arithmetic on buffer buf.  Loads run one step
// ahead, one barrier per step.
template <class Fetch, class Put, class Work>
__device__ __forceinline__ void pair_walk(int nsteps, bool active, Fetch fetch, Put put, Work work) {
    fetch(0);
    put(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < nsteps;
        if (more) fetch(s + 1);
        if (active) work(cur);
        if (more) put(cur ^ 1);
        __syncthreads();
    }
}

// The finishing passes: one (i <= j) pair per (blockIdx.z, blockIdx.y), a lane per bin.
struct PairBin {
    int i, j, f;
    bool valid;                                          // i <= j and a bin of the spectrum
    int64_t ij, ji, ii, jj, plane;
    bool real_bin;                                       // DC, and Nyquist for even nfft
    __device__ __forceinline__ PairBin(int nch, int nfreq, int nfft_is_even)
        : i(blockIdx.z), j(blockIdx.y), f(blockIdx.x * 256 + threadIdx.x), valid(i <= j && f < nfreq),
          ij(pair_at(i, j, nch, nfreq, f)), ji(pair_at(j, i, nch, nfreq, f)), ii(pair_at(i, i, nch, nfreq, f)),
          jj(pair_at(j, j, nch, nfreq, f)), plane((int64_t)nch * nch * nfreq),
          real_bin(f == 0 || (nfft_is_even && f == nfreq - 1)) {}
};

// The triangular grid of an accumulate entry point `who` over nch channels in blocks of B.
inline int pair_grid(const char *who, int nch, int B, int64_t *nblk, int64_t *tri) {
    OSZ_REQUIRE(nch >= 1 && nch <= 65535, "%s: bad sizes", who);
    *nblk = (nch + B - 1) / B;
    *tri = *nblk * (*nblk + 1) / 2;
    OSZ_REQUIRE(*tri <= INT32_MAX, "%s: grid too large", who);
    return OSZ_OK;
}

}  // namespace osz
