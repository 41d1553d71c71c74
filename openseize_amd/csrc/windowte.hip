// windowte.hip -- K26 binned transfer entropy per window and ordered channel pair: for every window
// of W samples, `step` apart, every row is cut into B bins exactly as K25 cuts it (windowmi.hip: the
// same edges, the same bytes), and with u = lag and T = W - u, n_abc(i, j) counts the t = u .. W - 1
// with the target, row j, in bin a at t and in bin b at t - 1 and the source, row i, in bin c at
// t - u.  With phi(n) = n ln n
//   S3 = sum phi(n_abc),  Sab = sum phi(n_ab.),  Sbc = sum phi(n_.bc),  Sb = sum phi(n_.b.)
//   TE_{i -> j} = I(Y_t ; X_{t-u} | Y_{t-1}) = ((S3 - Sab) - (Sbc - Sb)) / T,  Hc_j = (Sb - Sab) / T.
// The three-way histograms of all ordered pairs are one rectangular product N = Z R^T of one-hot
// rows: Z[j Bp^2 + (a Bp + b)][t'] = (the target's symbol at t' is (a, b)), R[i Bp + c][t'] = (the
// bin of row i at t' is c), t' = t - u, Bp = B rounded up to a power of two: 0 / 1 bytes in, exact
// int32 out, on the int8 matrix pipe (v_mfma_i32_16x16x64_i8).  Per batch of windows:
// (1) K25's edges and codes, through its launchers (wm_codes; phi(0 .. W) once per call, wm_phi);
// (2) te_symbol_kernel writes a symbol per t' < T, code[t' + u] << lb | code[t' + u - 1], and 0xFF
//     from T to the next multiple of 64.  The source operand is the code array itself, read from
//     t' = 0: where it runs past T the target's 0xFF has no one-hot row, so the product drops it;
// (3) te_gram_kernel expands symbols and codes to one-hot rows while it stages them in LDS and
//     writes the whole (nch Bp^2) x (nch Bp) rectangle of N;
// (4) te_finish_kernel sums phi by table lookup, both directions of a pair in one thread, forms
//     the measures and writes both entries; te_counts_kernel copies N out as float64.
// The finish is not fused onto the accumulators: a pair's cells lie across Bp^2 / 16 .. 4 tiles of
// a wave and its reverse direction in another workgroup (as in K25).  DESIGN.md section 4, K26.
//
// The counts are integers; phi is read from one table, so it is a function of n alone; the sums
// of phi run in one thread with b outermost, then a, then c: an order that is a function of B
// alone.  Nothing is atomic.
#include "pair_window.h"

namespace osz {

#pragma clang fp contract(off)

typedef int te_i4 __attribute__((ext_vector_type(4)));
typedef unsigned te_u4 __attribute__((ext_vector_type(4)));
typedef int te_i2 __attribute__((ext_vector_type(2)));

constexpr int kTeEdges = OSZ_WM_MAXBINS;      // K25's doubles of edges per (row, window)
constexpr int kTeMeta = OSZ_WM_MAXBINS + 2;   // K25's doubles per (window, row); the flag is the last
constexpr int kTeFlag = OSZ_WM_MAXBINS + 1;
constexpr int kTeSide = 64;                   // one-hot rows per side of a workgroup's block: 2 x 2 waves
constexpr int kTeThreads = 256;               // 4 waves, each 2 x 2 tiles of 16 x 16
constexpr int kTeStep = 64;                   // samples per matrix step: the k of the instruction
constexpr int kTeFinish = 16;                 // pairs per side of a finishing workgroup's tile
constexpr unsigned char kTeNoBin = 0xFF;      // K25's code of a sample past the window; the symbol past T

static_assert(OSZ_WT_MAXBINS * OSZ_WT_MAXBINS <= kTeSide && OSZ_WT_MAXBINS <= OSZ_WM_MAXBINS &&
                  OSZ_WT_LONGEST == OSZ_WM_LONGEST,
              "a target channel's symbols fill at most one block side, below the no-bin byte; the bins are K25's");

// The symbols of one (window, row): thread t writes the symbols t, t + 256, ..
// Grid: x = window of the batch, y = row.
__global__ void __launch_bounds__(256)
te_symbol_kernel(const unsigned char *__restrict__ codes, int nch, int wpad, int T, int tpad, int u, int lb,
                 unsigned char *__restrict__ syms) {
    const int64_t at = ((int64_t)blockIdx.x * nch + blockIdx.y) * wpad;
    const unsigned char *__restrict__ src = codes + at;
    unsigned char *__restrict__ dst = syms + at;
    for (int t = threadIdx.x; t < tpad; t += 256) {
        unsigned char z = kTeNoBin;
        if (t < T) {
            const unsigned now = src[t + u], before = src[t + u - 1];
            if (now != kTeNoBin && before != kTeNoBin) z = (unsigned char)(now << lb | before);
        }
        dst[t] = z;
    }
}

// N of one window over one 64 x 64 block: block row bi of the target operand against block column
// bj of the source operand.  Target row r is symbol r & (Bp^2 - 1) of channel r >> 2 lb; source row
// r is bin r & (Bp - 1) of channel r >> lb.  Per 64-sample step thread (e = t >> 2, seg = t & 3)
// fetches 16 bytes of the channel of row e of either side and stores the 16 one-hot bytes of that
// row; wave (wi, wj) then reads, per 16 x 16 tile side, row l & 15, bytes 16 (l >> 4) .. + 15 -- the
// same 16 samples of k in both operands -- and issues up to four MFMAs on independent
// accumulators.  A tile past the last row of either side is neither computed nor written.
// Grid: x = bi * nbj + bj, y = window of the batch.
__global__ void __launch_bounds__(kTeThreads)
te_gram_kernel(const unsigned char *__restrict__ syms, const unsigned char *__restrict__ codes, int nch, int wpad,
               int tpad, int lb, int nbj, int *__restrict__ part) {
    __shared__ te_u4 stage[2][kTeSide][kTeStep / 16];        // 8 KB
    const int bi = blockIdx.x / nbj, bj = blockIdx.x % nbj;
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6, wi = w >> 1, wj = w & 1;
    const int64_t wb = blockIdx.y;
    const int RA = nch << (2 * lb), RB = nch << lb;
    const int rt = lane & 15, kq = lane >> 4;

    bool act[2][2];
    te_i4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i0 = bi * kTeSide + wi * 32 + a * kPwTile, j0 = bj * kTeSide + wj * 32 + b * kPwTile;
            act[a][b] = i0 < RA && j0 < RB;
            acc[a][b] = te_i4{0, 0, 0, 0};
        }
    const bool busy = act[0][0];                             // (the first tile of a wave: the others imply it)

    const int e = t >> 2, seg = t & 3;
    const unsigned char *src[2];
    unsigned same[2];
    bool have[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = (h ? bj : bi) * kTeSide + e, shift = h ? lb : 2 * lb;
        have[h] = r < (h ? RB : RA);
        const int ch = have[h] ? r >> shift : 0;
        same[h] = (unsigned)(r & ((1 << shift) - 1)) * 0x01010101u;
        src[h] = (h ? codes : syms) + (wb * nch + ch) * wpad + seg * 16;
    }
    for (int s0 = 0; s0 < tpad; s0 += kTeStep) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            te_u4 o = {0u, 0u, 0u, 0u};
            if (have[h]) {
                const te_u4 cw = *reinterpret_cast<const te_u4 *>(src[h] + s0);
                o = te_u4{mi_onehot(cw.x, same[h]), mi_onehot(cw.y, same[h]), mi_onehot(cw.z, same[h]),
                          mi_onehot(cw.w, same[h])};
            }
            stage[h][e][seg] = o;
        }
        __syncthreads();
        if (busy) {
            te_i4 fa[2], fb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fa[a] = __builtin_bit_cast(te_i4, stage[0][wi * 32 + a * kPwTile + rt][kq]);
                fb[a] = __builtin_bit_cast(te_i4, stage[1][wj * 32 + a * kPwTile + rt][kq]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    if (act[a][b]) acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D of the 16 x 16 forms: column (the B operand's row) = lane & 15, row (the A operand's) = 4 (lane >> 4) + reg
    int *__restrict__ dst = part + wb * RA * RB;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (!act[a][b]) continue;
            const int j = bj * kTeSide + wj * 32 + b * kPwTile + rt;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = bi * kTeSide + wi * 32 + a * kPwTile + 4 * kq + reg;
                if (i < RA && j < RB) dst[(int64_t)i * RB + j] = acc[a][b][reg];
            }
        }
}

// The sums of one direction: g at the cells of (target, source), RB ints a row.  te = ((S3 - Sab) -
// (Sbc - Sb)) / T, below 0 (and the -0.0 no subtraction here gives) +0.0; hc = (Sb - Sab) / T.
template <int LB>
__device__ __forceinline__ void te_direction(const int *__restrict__ g, int64_t RB, int B, int T,
                                             const double *__restrict__ phi, double *te, double *hc) {
    constexpr int BP = 1 << LB;
    double S3 = 0.0, Sab = 0.0, Sbc = 0.0, Sb = 0.0;
    for (int b = 0; b < B; ++b) {
        int nbc[BP], nb = 0;
#pragma unroll
        for (int c = 0; c < BP; ++c) nbc[c] = 0;
        for (int a = 0; a < B; ++a) {
            const int *row = g + (int64_t)(a << LB | b) * RB;
            int nv[BP];
            if constexpr (BP >= 4) {
#pragma unroll
                for (int q = 0; q < BP / 4; ++q) {
                    const te_i4 four = reinterpret_cast<const te_i4 *>(row)[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) nv[4 * q + k] = four[k];
                }
            } else {
                const te_i2 two = *reinterpret_cast<const te_i2 *>(row);
                nv[0] = two.x;
                nv[1] = two.y;
            }
            int nab = 0;
#pragma unroll
            for (int c = 0; c < BP; ++c) {
                if (c >= B) continue;                        // (the same for the whole grid)
                const int n = nv[c] < 0 ? 0 : nv[c] > T ? T : nv[c];
                S3 += phi[n];                                // (phi(0) = +0.0 moves nothing)
                nab += n;
                nbc[c] += n;
            }
            Sab += phi[nab > T ? T : nab];
            nb += nab;
        }
#pragma unroll
        for (int c = 0; c < BP; ++c)
            if (c < B) Sbc += phi[nbc[c] > T ? T : nbc[c]];
        Sb += phi[nb > T ? T : nb];
    }
    const double cnt = (double)T;
    double v = ((S3 - Sab) - (Sbc - Sb)) / cnt;
    if (!(v > 0.0)) v = 0.0;
    *te = v;
    *hc = (Sb - Sab) / cnt;
}

__device__ __forceinline__ double te_normalised(double te, double hc) {
    double v = te / hc;
    v = v > 1.0 ? 1.0 : v < 0.0 ? 0.0 : v;
    return hc == 0.0 ? __builtin_nan("") : v;
}

// One 16 x 16 tile of pairs (tile row bi <= tile column bj) and one window per workgroup, a thread
// per pair; the thread of i < j computes i -> j and j -> i, each from its own Bp^3 cells, writes
// [i, j] and hands [j, i] through the LDS turn that keeps the mirror's rows whole.  i == j: +0.0.
// A pair with a flagged row is NaN in every measure.
// Grid: x = triangular tile index, y = window of the batch.
template <int LB>
__global__ void __launch_bounds__(kTeFinish * kTeFinish)
te_finish_kernel(const int *__restrict__ part, const double *__restrict__ meta, const double *__restrict__ table,
                 int nch, int ntile, int B, int W, int T, int mask, double *__restrict__ out, int64_t out_plane,
                 int64_t win0) {
    extern __shared__ double phi[];                          // phi(0 .. W)
    __shared__ double turn[kTeFinish][kTeFinish + 1];
    for (int n = threadIdx.x; n <= W; n += kTeFinish * kTeFinish) phi[n] = table[n];
    __syncthreads();
    int bi, bj;
    pair_triangle(blockIdx.x, ntile, &bi, &bj);
    const int ta = threadIdx.x / kTeFinish, tb = threadIdx.x % kTeFinish;
    const int i = bi * kTeFinish + ta, j = bj * kTeFinish + tb;
    const bool mine = i < nch && j < nch && i <= j;          // this thread computes [i, j]
    const bool pair = mine && i < j;
    // ... and writes the mirror [jm, im] of the pair that thread (tb, ta) computes
    const int jm = bj * kTeFinish + ta, im = bi * kTeFinish + tb;
    const bool mirrored = jm < nch && im < jm;
    const int64_t rr = (int64_t)nch * nch, wb = blockIdx.y, win = win0 + wb;
    const int64_t RB = (int64_t)nch << LB, RA = RB << LB;
    const int64_t at = (int64_t)i * nch + j, mirror = (int64_t)jm * nch + im;
    const double nan = __builtin_nan("");
    const double *mi_ = meta + (wb * nch + (mine ? i : 0)) * kTeMeta, *mj_ = meta + (wb * nch + (mine ? j : 0)) * kTeMeta;
    const bool lost = mine && (mi_[kTeFlag] != 0.0 || mj_[kTeFlag] != 0.0);

    double fwd = 0.0, hf = 0.0, rev = 0.0, hr = 0.0;         // i -> j with Hc_j, j -> i with Hc_i
    if (pair) {
        const int *g = part + wb * RA * RB;
        te_direction<LB>(g + ((int64_t)j << (2 * LB)) * RB + ((int64_t)i << LB), RB, B, T, phi, &fwd, &hf);
        te_direction<LB>(g + ((int64_t)i << (2 * LB)) * RB + ((int64_t)j << LB), RB, B, T, phi, &rev, &hr);
    }
    // (the diagonal: +0.0 in all three)
    double vals[3] = {fwd, pair ? te_normalised(fwd, hf) : 0.0, fwd - rev};
    double back[3] = {rev, pair ? te_normalised(rev, hr) : 0.0, rev - fwd};
#pragma unroll
    for (int m = 0; m < 3; ++m)
        if (lost) vals[m] = back[m] = nan;
    double *o = out + win * rr;
    int plane = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (!(mask & (1 << (OSZ_WT_TE + m)))) continue;      // (the same for the whole grid)
        if (mine) o[plane * out_plane + at] = vals[m];
        pw_mirror(turn, ta, tb, back[m], mirrored, o + plane * out_plane + mirror);
        ++plane;
    }
}

// counts[k, a, b, c, i, j] = N[j Bp^2 + a Bp + b][i Bp + c], NaN for a flagged row: a thread per
// (i, j), j fastest.  Grid: x = blocks of 256 pairs, y = window of the batch, z = (a B + b) B + c.
__global__ void __launch_bounds__(256)
te_counts_kernel(const int *__restrict__ part, const double *__restrict__ meta, int nch, int B, int lb, int T,
                 double *__restrict__ counts, int64_t win0) {
    const int64_t rr = (int64_t)nch * nch, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= rr) return;
    const int i = (int)(p / nch), j = (int)(p % nch);
    const int cell = blockIdx.z, c = cell % B, b = cell / B % B, a = cell / (B * B);
    const int64_t wb = blockIdx.y, RB = (int64_t)nch << lb, RA = RB << lb;
    const double *mw = meta + wb * nch * kTeMeta;
    const bool lost = mw[(int64_t)i * kTeMeta + kTeFlag] != 0.0 || mw[(int64_t)j * kTeMeta + kTeFlag] != 0.0;
    int n = part[(wb * RA + ((int64_t)j << (2 * lb)) + (a << lb | b)) * RB + ((int64_t)i << lb) + c];
    n = n < 0 ? 0 : n > T ? T : n;
    counts[(((win0 + wb) * B * B * B) + cell) * rr + p] = lost ? __builtin_nan("") : (double)n;
}

static int wt_log2(int bins) {
    int lb = 1;
    while ((1 << lb) < bins) ++lb;
    return lb;
}

// The work space of one push: [phi: W + 1, rounded up to even] and for one batch of windows [edges:
// 16 nch] [meta: 18 nch] [codes: nch Wpad bytes] [symbols: nch Wpad bytes] [N: (nch Bp^2) (nch Bp)
// int32] each.  The batch is also held to kGramCap doubles of what goes in front of N.
struct WtPlan : PwPlan {
    int lb, T, tpad;
    int64_t wpad, phi, edges, meta, codes;                   // the parts' lengths in doubles (codes: and symbols')
};
static bool wt_plan(const PwArgs &A, int lag, WtPlan *p) {
    const int B = A.value;
    if (B < 2 || B > OSZ_WT_MAXBINS || lag < 1 || lag > OSZ_WT_MAXLAG) return false;
    p->lb = wt_log2(B);
    const int64_t bp = (int64_t)1 << p->lb;
    if (!pw_plan(A, OSZ_WT_COUNT, 16, OSZ_WT_LONGEST, 0, bp * bp * bp / 2, p)) return false;
    if (lag > A.W / 2) return false;
    p->T = (int)A.W - lag;
    p->tpad = (p->T + kTeStep - 1) / kTeStep * kTeStep;
    p->wpad = (A.W + kTeStep - 1) / kTeStep * kTeStep;
    const int64_t per = (kTeEdges + kTeMeta + 2 * (p->wpad / 8)) * A.nch;   // doubles per window in front of N
    p->batch = std::max<int64_t>(1, std::min(p->batch, kGramCap / per));
    p->gram = p->batch * p->one;
    p->phi = (A.W + 2) & ~(int64_t)1;
    p->edges = p->batch * kTeEdges * A.nch;
    p->meta = p->batch * kTeMeta * A.nch;
    p->codes = p->batch * A.nch * (p->wpad / 8);
    p->chan = p->phi + p->edges + p->meta + 2 * p->codes;
    return true;
}

template <int LB>
static void wt_finish(unsigned tri, unsigned count, size_t lds, hipStream_t st, const int *part, const double *meta,
                      const double *table, int nch, int ntile, int B, int W, int T, int mask, double *out,
                      int64_t out_plane, int64_t win0) {
    hipLaunchKernelGGL((te_finish_kernel<LB>), dim3(tri, count), dim3(kTeFinish * kTeFinish), lds, st, part, meta, table,
                       nch, ntile, B, W, T, mask, out, out_plane, win0);
}

// "lag <u>, bins": what pw_head's message of refused sizes names in front of the bins
struct WtOwn {
    char text[32];
    explicit WtOwn(int lag) { snprintf(text, sizeof text, "lag %d, bins", lag); }
};

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_te_work(int nch, int64_t n, int64_t winsize, int64_t step, int bins, int lag, int mask) {
    WtPlan p;
    return wt_plan({"osz_window_te", nch, n, winsize, step, mask, "bins", bins}, lag, &p) ? p.work() : -1;
}

int osz_window_te(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int bins,
                  int lag, int binning, int mask, double *counts, double *out, int64_t plane_pitch, double *work,
                  int64_t work_len, void *stream) {
    const WtOwn own(lag);
    const PwArgs A{"osz_window_te", nch, n, winsize, step, mask, own.text, bins, "binning", binning};
    const bool full = mask & (1 << OSZ_WT_COUNTS), matrices = mask & ~(1 << OSZ_WT_COUNTS);
    WtPlan p;
    const int rc = pw_head(A, wt_plan(A, lag, &p), p, {{x, 8}, {work, 16}, {counts, 8, true, full}, {out, 8, true, matrices}},
                           pitch, matrices, plane_pitch, work_len);
    if (rc != OSZ_OK) return rc;
    if (p.nwin == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    const int W = (int)winsize;
    double *phi = work, *edges = phi + p.phi, *meta = edges + p.edges;
    unsigned char *codes = reinterpret_cast<unsigned char *>(meta + p.meta);
    unsigned char *syms = codes + p.codes * 8;
    int *part = reinterpret_cast<int *>(work + p.chan);
    const int ra = nch << (2 * p.lb), rb = nch << p.lb;
    const int nbi = (ra + kTeSide - 1) / kTeSide, nbj = (rb + kTeSide - 1) / kTeSide;
    const int ntile = (nch + kTeFinish - 1) / kTeFinish;
    const int rc_phi = wm_phi(phi, W, "window_te_phi", st);
    if (rc_phi != OSZ_OK) return rc_phi;
    return pw_batches(p, [&](int64_t w0, int64_t count) -> int {
        const int rc = wm_codes(x + w0 * step, pitch, nch, W, step, count, bins, binning, phi, edges, meta, codes,
                                (int)p.wpad, "window_te_edges", "window_te_code", st);
        if (rc != OSZ_OK) return rc;
        {
            KernelTimer timer("window_te_symbol", st);
            hipLaunchKernelGGL(te_symbol_kernel, dim3((unsigned)count, (unsigned)nch), dim3(256), 0, st, codes, nch,
                               (int)p.wpad, p.T, p.tpad, lag, p.lb, syms);
            OSZ_HIP(hipGetLastError());
        }
        {
            KernelTimer timer("window_te_gram", st);
            hipLaunchKernelGGL(te_gram_kernel, dim3((unsigned)((int64_t)nbi * nbj), (unsigned)count), dim3(kTeThreads), 0, st,
                               syms, codes, nch, (int)p.wpad, p.tpad, p.lb, nbj, part);
            OSZ_HIP(hipGetLastError());
        }
        KernelTimer timer("window_te_finish", st);
        if (matrices) {
            const unsigned tri = (unsigned)(ntile * (ntile + 1) / 2);
            const size_t lds = (size_t)(W + 1) * sizeof(double);
            switch (p.lb) {
            case 1: wt_finish<1>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, p.T, mask, out, plane_pitch, w0); break;
            case 2: wt_finish<2>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, p.T, mask, out, plane_pitch, w0); break;
            default: wt_finish<3>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, p.T, mask, out, plane_pitch, w0); break;
            }
            OSZ_HIP(hipGetLastError());
        }
        if (full) {
            const int64_t pairs = (int64_t)nch * nch;
            hipLaunchKernelGGL(te_counts_kernel, dim3((unsigned)((pairs + 255) / 256), (unsigned)count,
                                                      (unsigned)(bins * bins * bins)),
                               dim3(256), 0, st, part, meta, nch, bins, p.lb, p.T, counts, w0);
            OSZ_HIP(hipGetLastError());
        }
        return OSZ_OK;
    });
}

}  // extern "C"
