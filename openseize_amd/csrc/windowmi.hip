// windowmi.hip -- K25 binned mutual information per window and channel pair: for every window of W
// samples, `step` apart, every row is cut into B bins (at its own k / B quantiles, K17's, or at B
// equal parts of its range), n_ab(i, j) counts the samples with row i in bin a and row j in bin b,
// and with phi(n) = n ln n
//   H_i = (phi(W) - sum_a phi(n_a)) / W,  H_ij = (phi(W) - sum_ab phi(n_ab)) / W,  MI = H_i + H_j - H_ij.
// The joint histograms of all pairs are one Gram product, N = R R^T over the nch Bp one-hot rows
// R[c Bp + a][t] = (bin of row c at t is a), Bp = B rounded up to a power of two: 0 / 1 bytes in,
// exact int32 out, on the int8 matrix pipe (v_mfma_i32_16x16x64_i8).  Per batch of windows:
// (1) the edges: K17's launcher (wq_quantiles), or the row's extremes inside step 2;
// (2) mi_code_kernel reads a window once, writes a bin code per sample (one byte; the samples
//     past W up to the next multiple of 64 get a code no bin has), the marginal counts, their
//     sum of phi and the non-finite flag;
// (3) mi_gram_kernel expands the codes to one-hot rows while it stages them in LDS -- once per
//     workgroup, not once per operand register -- and writes the block-upper triangle of N;
// (4) mi_finish_kernel sums phi(n_ab) by table lookup per pair i < j, forms the measures and
//     writes both mirrors.  phi(0 .. W) is computed once per call (mi_phi_kernel).
// Steps (1) and (2) and the table are also host launchers, wm_codes and wm_phi (pair_window.h): K26
// (windowte.hip) starts from the same bytes.
// DESIGN.md section 4, K25.
//
// The counts are integers; phi is read from one table, so it is a function of n alone; a sum of
// phi runs over a, then b, in one thread: an order that is a function of B alone.  Nothing is
// atomic.  H uses phi(W) / W for ln W, so that a constant row has H = +0.0 exactly.
#include "pair_window.h"

namespace osz {

#pragma clang fp contract(off)

typedef int mi_i4 __attribute__((ext_vector_type(4)));
typedef unsigned mi_u4 __attribute__((ext_vector_type(4)));
typedef int mi_i2 __attribute__((ext_vector_type(2)));

constexpr int kMiEdges = OSZ_WM_MAXBINS;      // doubles of edges per (row, window): B - 1 <= 15 used
constexpr int kMiMeta = OSZ_WM_MAXBINS + 2;   // per (window, row): the counts n_a, their sum of phi, the flag
constexpr int kMiSphi = OSZ_WM_MAXBINS, kMiFlag = OSZ_WM_MAXBINS + 1;
constexpr int kMiSide = 64;                   // one-hot rows per side of a workgroup's block: 2 x 2 waves
constexpr int kMiThreads = 256;               // 4 waves, each 2 x 2 tiles of 16 x 16
constexpr int kMiStep = 64;                   // samples per matrix step: the k of the instruction
constexpr int kMiFinish = 16;                 // pairs per side of a finishing workgroup's tile
constexpr unsigned char kMiNoBin = 0xFF;      // the code of a sample past the window

static_assert(OSZ_WM_MAXBINS == kPwTile && OSZ_WM_MAXBINS - 1 <= OSZ_WQ_QMOST && OSZ_WM_LONGEST <= OSZ_WQ_LONGEST,
              "a row's bins fill at most one tile, its edges one K17 call");

__global__ void __launch_bounds__(256) mi_phi_kernel(double *__restrict__ phi, int W) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n <= W) phi[n] = n ? (double)n * log((double)n) : 0.0;
}

struct MiCode {
    const double *x;          // already at the batch's first window
    int64_t pitch, step, count;
    int nch, W, wpad, B, uniform;
    const double *phi, *edges;
    double *meta;
    unsigned char *codes;
};

// One workgroup per (window, row): thread t holds the samples r NT + t in registers.
// Grid: x = window of the batch, y = row.
template <int NT, int K>
__global__ void __launch_bounds__(NT) mi_code_kernel(const MiCode A) {
    constexpr int NW = NT / kWave;
    __shared__ double ext[2][NW];
    __shared__ int hist[NW][OSZ_WM_MAXBINS], bad[NW];
    __shared__ double edge[kMiEdges];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
    const int64_t wb = blockIdx.x;
    const int c = blockIdx.y, W = A.W, B = A.B;
    const double *__restrict__ row = A.x + (int64_t)c * A.pitch + wb * A.step;
    const double inf = __builtin_inf();

    double v[K];
    double lo = inf, hi = -inf;
    bool wild = false;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int e = r * NT + t;
        v[r] = 0.0;
        if (e < W) {
            v[r] = row[e];
            wild |= !__builtin_isfinite(v[r]);
            lo = __builtin_fmin(lo, v[r]);
            hi = __builtin_fmax(hi, v[r]);
        }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {                    // (min and max: any order gives the same bits)
        lo = __builtin_fmin(lo, __shfl_xor(lo, m));
        hi = __builtin_fmax(hi, __shfl_xor(hi, m));
    }
    const bool any = __ballot(wild) != 0ull;
    if (lane == 0) {
        ext[0][w] = lo;
        ext[1][w] = hi;
        bad[w] = any;
    }
    __syncthreads();
    int wilds = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        lo = __builtin_fmin(lo, ext[0][j]);
        hi = __builtin_fmax(hi, ext[1][j]);
        wilds |= bad[j];
    }
    if (t < kMiEdges) {
        double e = inf;                                      // (an edge no finite sample reaches)
        if (t < B - 1) {
            if (A.uniform) e = lo + (double)(t + 1) * ((hi - lo) / (double)B);
            else e = A.edges[((int64_t)t * A.nch + c) * A.count + wb];
        }
        edge[t] = e;
    }
    if (A.uniform && !__builtin_isfinite(hi - lo)) wilds = 1;
    __syncthreads();

    // the bin: the number of edges <= the sample
    unsigned char *__restrict__ dst = A.codes + (wb * A.nch + c) * A.wpad;
    int code[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int e = r * NT + t;
        int n = 0;
#pragma unroll
        for (int k = 0; k < kMiEdges - 1; ++k) n += edge[k] <= v[r] ? 1 : 0;
        code[r] = e < W ? n : -1;
        if (e < A.wpad) dst[e] = e < W ? (unsigned char)n : kMiNoBin;
    }
    for (int a = 0; a < B; ++a) {
        int n = 0;
#pragma unroll
        for (int r = 0; r < K; ++r) n += __popcll(__ballot(code[r] == a));
        if (lane == 0) hist[w][a] = n;
    }
    __syncthreads();
    if (t == 0) {
        double *__restrict__ meta = A.meta + (wb * A.nch + c) * kMiMeta;
        double s = 0.0;
        for (int a = 0; a < OSZ_WM_MAXBINS; ++a) {
            int n = 0;
            if (a < B)
#pragma unroll
                for (int j = 0; j < NW; ++j) n += hist[j][a];
            n = n < 0 ? 0 : n > W ? W : n;
            meta[a] = (double)n;
            s += A.phi[n];                                   // (phi(0) = +0.0 moves nothing)
        }
        meta[kMiSphi] = s;
        meta[kMiFlag] = wilds ? 1.0 : 0.0;
    }
}

// N of one window over one 64 x 64 block of one-hot rows (block row bi <= block column bj).  Row r
// is bin r & (Bp - 1) of channel r >> lb.  Per 64-sample step thread (e = t >> 2, seg = t & 3)
// fetches 16 codes of the channels of slot e of either side and stores the 16 one-hot bytes of its
// rows; wave (wi, wj) then reads, per 16 x 16 tile side, row l & 15, bytes 16 (l >> 4) .. + 15 --
// the same 16 samples of k in both operands, whatever their order inside the instruction -- and
// issues up to four MFMAs on independent accumulators.  A tile below the diagonal or past the
// last row is neither computed nor written.
// Grid: x = triangular block index, y = window of the batch.
__global__ void __launch_bounds__(kMiThreads)
mi_gram_kernel(const unsigned char *__restrict__ codes, int nch, int wpad, int lb, int nblk, int *__restrict__ part) {
    __shared__ mi_u4 stage[2][kMiSide][kMiStep / 16];        // 8 KB
    int bi, bj;
    pair_triangle(blockIdx.x, nblk, &bi, &bj);
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6, wi = w >> 1, wj = w & 1;
    const int64_t wb = blockIdx.y;
    const int R = nch << lb;
    const int rt = lane & 15, kq = lane >> 4;

    bool act[2][2];
    mi_i4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i0 = bi * kMiSide + wi * 32 + a * kPwTile, j0 = bj * kMiSide + wj * 32 + b * kPwTile;
            act[a][b] = i0 < R && j0 < R && i0 <= j0;
            acc[a][b] = mi_i4{0, 0, 0, 0};
        }
    const bool busy = act[0][0] || act[0][1] || act[1][1];   // (act[1][0] implies act[0][0])

    const int e = t >> 2, seg = t & 3;
    const unsigned char *src[2];
    unsigned same[2];
    bool have[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = (h ? bj : bi) * kMiSide + e;
        have[h] = r < R;
        const int ch = have[h] ? r >> lb : 0;
        same[h] = (unsigned)(r & ((1 << lb) - 1)) * 0x01010101u;
        src[h] = codes + (wb * nch + ch) * wpad + seg * 16;
    }
    for (int s0 = 0; s0 < wpad; s0 += kMiStep) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            mi_u4 o = {0u, 0u, 0u, 0u};
            if (have[h]) {
                const mi_u4 cw = *reinterpret_cast<const mi_u4 *>(src[h] + s0);
                o = mi_u4{mi_onehot(cw.x, same[h]), mi_onehot(cw.y, same[h]), mi_onehot(cw.z, same[h]),
                          mi_onehot(cw.w, same[h])};
            }
            stage[h][e][seg] = o;
        }
        __syncthreads();
        if (busy) {
            mi_i4 fa[2], fb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fa[a] = __builtin_bit_cast(mi_i4, stage[0][wi * 32 + a * kPwTile + rt][kq]);
                fb[a] = __builtin_bit_cast(mi_i4, stage[1][wj * 32 + a * kPwTile + rt][kq]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    if (act[a][b]) acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D of the 16 x 16 forms: column = lane & 15, row = 4 (lane >> 4) + reg
    int *__restrict__ dst = part + wb * R * R;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (!act[a][b]) continue;
            const int j = bj * kMiSide + wj * 32 + b * kPwTile + rt;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = bi * kMiSide + wi * 32 + a * kPwTile + 4 * kq + reg;
                if (i < R && j < R) dst[(int64_t)i * R + j] = acc[a][b][reg];
            }
        }
}

// One 16 x 16 tile of pairs (tile row bi <= tile column bj) and one window per workgroup, a thread
// per pair; the threads with i <= j compute.  i < j: S = sum over a, then b, of phi(n_ab), phi from
// the table in LDS, the Bp counts of a row of cells read at once; then the definitions, and every
// value goes to [i, j] and, through the LDS turn that keeps the mirror's rows whole, to [j, i]
// (counts[a, b, i, j] to counts[b, a, j, i]).  i == j: the fixed points, from the marginal counts.
// A pair with a flagged row is NaN in every measure.
// Grid: x = triangular tile index, y = window of the batch.
template <int LB>
__global__ void __launch_bounds__(kMiFinish * kMiFinish)
mi_finish_kernel(const int *__restrict__ part, const double *__restrict__ meta, const double *__restrict__ table,
                 int nch, int ntile, int B, int W, int mask, double *__restrict__ counts, double *__restrict__ out,
                 int64_t out_plane, int64_t win0) {
    constexpr int BP = 1 << LB;
    extern __shared__ double phi[];                          // phi(0 .. W)
    __shared__ double turn[kMiFinish][kMiFinish + 1];
    for (int n = threadIdx.x; n <= W; n += kMiFinish * kMiFinish) phi[n] = table[n];
    __syncthreads();
    int bi, bj;
    pair_triangle(blockIdx.x, ntile, &bi, &bj);
    const int ta = threadIdx.x / kMiFinish, tb = threadIdx.x % kMiFinish;
    const int i = bi * kMiFinish + ta, j = bj * kMiFinish + tb;
    const bool mine = i < nch && j < nch && i <= j;          // this thread computes [i, j]
    const bool pair = mine && i < j;
    // ... and writes the mirror [jm, im] of the pair that thread (tb, ta) computes
    const int jm = bj * kMiFinish + ta, im = bi * kMiFinish + tb;
    const bool mirrored = jm < nch && im < jm;
    const int64_t rr = (int64_t)nch * nch, wb = blockIdx.y, win = win0 + wb;
    const int64_t R = (int64_t)nch << LB;
    const int64_t at = (int64_t)i * nch + j, mirror = (int64_t)jm * nch + im;
    const double nan = __builtin_nan("");
    const double *mi_ = meta + (wb * nch + (mine ? i : 0)) * kMiMeta, *mj_ = meta + (wb * nch + (mine ? j : 0)) * kMiMeta;
    const bool lost = mine && (mi_[kMiFlag] != 0.0 || mj_[kMiFlag] != 0.0);
    const int *g = part + (wb * R + ((int64_t)(pair ? i : 0) << LB)) * R + ((int64_t)(pair ? j : 0) << LB);
    double *c = (mask & (1 << OSZ_WM_COUNTS)) ? counts + win * B * B * rr : nullptr;   // (the same for the whole grid)

    double S = 0.0;
    for (int a = 0; a < B; ++a) {
        int nv[BP];
#pragma unroll
        for (int b = 0; b < BP; ++b) nv[b] = 0;
        if (pair) {
            if constexpr (BP >= 4) {
#pragma unroll
                for (int q = 0; q < BP / 4; ++q) {
                    const mi_i4 four = reinterpret_cast<const mi_i4 *>(g + a * R)[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) nv[4 * q + k] = four[k];
                }
            } else {
                const mi_i2 two = *reinterpret_cast<const mi_i2 *>(g + a * R);
                nv[0] = two.x;
                nv[1] = two.y;
            }
        } else if (mine) {
#pragma unroll
            for (int b = 0; b < BP; ++b) nv[b] = b == a ? (int)mi_[a] : 0;
        }
#pragma unroll
        for (int b = 0; b < BP; ++b) {
            if (b >= B) continue;                            // (the same for the whole grid)
            const int n = nv[b] < 0 ? 0 : nv[b] > W ? W : nv[b];
            S += phi[n];
            if (c) {
                const double v = lost ? nan : (double)n;
                if (mine) c[(int64_t)(a * B + b) * rr + at] = v;
                pw_mirror(turn, ta, tb, v, mirrored, c + (int64_t)(b * B + a) * rr + mirror);
            }
        }
    }

    const double cnt = (double)W, top = phi[W];
    const double hi = (top - mi_[kMiSphi]) / cnt, hj = (top - mj_[kMiSphi]) / cnt, hij = (top - S) / cnt;
    double mi = (hi + hj) - hij;
    if (mi < 0.0) mi = 0.0;
    const double prod = hi * hj;
    double nmi = mi / sqrt(prod);
    nmi = nmi > 1.0 ? 1.0 : nmi < 0.0 ? 0.0 : nmi;
    if (prod == 0.0) nmi = nan;
    double joint = hij;
    if (i == j) {
        mi = joint = hi;
        nmi = hi == 0.0 ? nan : 1.0;
    }
    if (lost) mi = nmi = joint = nan;
    if (!(mask & ~(1 << OSZ_WM_COUNTS))) return;             // (the same for the whole grid)
    double *o = out + win * rr;
    int plane = 0;
    const double vals[3] = {mi, nmi, joint};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (!(mask & (1 << (OSZ_WM_MI + m)))) continue;      // (the same for the whole grid)
        if (mine) o[plane * out_plane + at] = vals[m];
        pw_mirror(turn, ta, tb, vals[m], mirrored, o + plane * out_plane + mirror);
        ++plane;
    }
}

static int wm_log2(int bins) {
    int lb = 1;
    while ((1 << lb) < bins) ++lb;
    return lb;
}

// The work space of one push: [phi: W + 1, rounded up to even] and for one batch of windows [edges:
// 16 nch] [meta: 18 nch] [codes: nch Wpad bytes] [N: (nch Bp)^2 int32] each.  The batch is also
// held to kGramCap doubles of what goes in front of N.
struct WmPlan : PwPlan {
    int lb;
    int64_t wpad, phi, edges, meta, codes;                   // the parts' lengths in doubles
};
static bool wm_plan(const PwArgs &A, WmPlan *p) {
    const int B = A.value;
    if (B < 2 || B > OSZ_WM_MAXBINS) return false;
    p->lb = wm_log2(B);
    const int64_t bp = (int64_t)1 << p->lb;
    if (!pw_plan(A, OSZ_WM_COUNT, 16, OSZ_WM_LONGEST, 0, bp * bp / 2, p)) return false;
    p->wpad = (A.W + kMiStep - 1) / kMiStep * kMiStep;
    const int64_t per = (kMiEdges + kMiMeta + p->wpad / 8) * A.nch;      // doubles per window in front of N
    p->batch = std::max<int64_t>(1, std::min(p->batch, kGramCap / per));
    p->gram = p->batch * p->one;
    p->phi = (A.W + 2) & ~(int64_t)1;
    p->edges = p->batch * kMiEdges * A.nch;
    p->meta = p->batch * kMiMeta * A.nch;
    p->codes = p->batch * A.nch * (p->wpad / 8);
    p->chan = p->phi + p->edges + p->meta + p->codes;
    return true;
}

template <int NT, int K>
static void wm_code(const MiCode &A, hipStream_t st) {
    hipLaunchKernelGGL((mi_code_kernel<NT, K>), dim3((unsigned)A.count, (unsigned)A.nch), dim3(NT), 0, st, A);
}

int wm_phi(double *phi, int W, const char *label, hipStream_t st) {
    KernelTimer timer(label, st);
    hipLaunchKernelGGL(mi_phi_kernel, dim3((unsigned)(W / 256 + 1)), dim3(256), 0, st, phi, W);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

int wm_codes(const double *x, int64_t pitch, int nch, int W, int64_t step, int64_t count, int bins, int binning,
             const double *phi, double *edges, double *meta, unsigned char *codes, int wpad, const char *edges_label,
             const char *code_label, hipStream_t st) {
    if (binning == OSZ_WM_QUANTILE) {
        double q[OSZ_WQ_QMOST];
        for (int k = 1; k < bins; ++k) q[k - 1] = (double)k / (double)bins;
        const int rc = wq_quantiles(x, pitch, nch, (count - 1) * step + W, W, step, 1 << OSZ_WQ_QUANTILE, q, bins - 1, edges,
                                    nch * count, count, 0, edges_label, st);
        if (rc != OSZ_OK) return rc;
    }
    const MiCode C{x, pitch, step, count, nch, W, wpad, bins, binning == OSZ_WM_UNIFORM, phi, edges, meta, codes};
    KernelTimer timer(code_label, st);
    if (W <= 64) wm_code<64, 1>(C, st);
    else if (W <= 256) wm_code<64, 4>(C, st);
    else if (W <= 1024) wm_code<256, 4>(C, st);
    else wm_code<1024, 4>(C, st);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

template <int LB>
static void wm_finish(unsigned tri, unsigned count, size_t lds, hipStream_t st, const int *part, const double *meta,
                      const double *table, int nch, int ntile, int B, int W, int mask, double *counts, double *out,
                      int64_t out_plane, int64_t win0) {
    hipLaunchKernelGGL((mi_finish_kernel<LB>), dim3(tri, count), dim3(kMiFinish * kMiFinish), lds, st, part, meta, table,
                       nch, ntile, B, W, mask, counts, out, out_plane, win0);
}

}  // namespace osz

using namespace osz;

extern "C" {

int64_t osz_window_mi_work(int nch, int64_t n, int64_t winsize, int64_t step, int bins, int mask) {
    WmPlan p;
    return wm_plan({"osz_window_mi", nch, n, winsize, step, mask, "bins", bins}, &p) ? p.work() : -1;
}

int osz_window_mi(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int bins,
                  int binning, int mask, double *counts, double *out, int64_t plane_pitch, double *work,
                  int64_t work_len, void *stream) {
    const PwArgs A{"osz_window_mi", nch, n, winsize, step, mask, "bins", bins, "binning", binning};
    const bool full = mask & (1 << OSZ_WM_COUNTS), matrices = mask & ~(1 << OSZ_WM_COUNTS);
    WmPlan p;
    const int rc = pw_head(A, wm_plan(A, &p), p, {{x, 8}, {work, 16}, {counts, 8, true, full}, {out, 8, true, matrices}},
                           pitch, matrices, plane_pitch, work_len);
    if (rc != OSZ_OK) return rc;
    if (p.nwin == 0) return OSZ_OK;
    hipStream_t st = as_stream(stream);
    const int W = (int)winsize;
    double *phi = work, *edges = phi + p.phi, *meta = edges + p.edges;
    unsigned char *codes = reinterpret_cast<unsigned char *>(meta + p.meta);
    int *part = reinterpret_cast<int *>(work + p.chan);
    const int rows = nch << p.lb;
    const int nblk = (rows + kMiSide - 1) / kMiSide, ntile = (nch + kMiFinish - 1) / kMiFinish;
    const int rc_phi = wm_phi(phi, W, "window_mi_phi", st);
    if (rc_phi != OSZ_OK) return rc_phi;
    return pw_batches(p, [&](int64_t w0, int64_t count) -> int {
        const int rc = wm_codes(x + w0 * step, pitch, nch, W, step, count, bins, binning, phi, edges, meta, codes,
                                (int)p.wpad, "window_mi_edges", "window_mi_code", st);
        if (rc != OSZ_OK) return rc;
        {
            KernelTimer timer("window_mi_gram", st);
            hipLaunchKernelGGL(mi_gram_kernel, dim3((unsigned)(nblk * (nblk + 1) / 2), (unsigned)count), dim3(kMiThreads), 0,
                               st, codes, nch, (int)p.wpad, p.lb, nblk, part);
            OSZ_HIP(hipGetLastError());
        }
        KernelTimer timer("window_mi_finish", st);
        const unsigned tri = (unsigned)(ntile * (ntile + 1) / 2);
        const size_t lds = (size_t)(W + 1) * sizeof(double);
        switch (p.lb) {
        case 1: wm_finish<1>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, mask, counts, out, plane_pitch, w0); break;
        case 2: wm_finish<2>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, mask, counts, out, plane_pitch, w0); break;
        case 3: wm_finish<3>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, mask, counts, out, plane_pitch, w0); break;
        default: wm_finish<4>(tri, (unsigned)count, lds, st, part, meta, phi, nch, ntile, bins, W, mask, counts, out, plane_pitch, w0); break;
        }
        OSZ_HIP(hipGetLastError());
        return OSZ_OK;
    });
}

}  // extern "C"
