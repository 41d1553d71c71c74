// pair_window.h -- what the channel-pair window kernels share: K19 windowpair.hip, K23
// windowxcorr.hip, K24 windowgranger.hip, K25 windowmi.hip and K26 windowte.hip.  DESIGN.md section 4.
//
// Host side: PwPlan and pw_plan, the work space of one push and the windows of a batch; pw_head,
// the checks every entry point makes of its arguments; pw_batches, the walk over the batches; and
// wx_window_sums and wx_lagged_gram, K23's sums and Gram launches, which K24 starts from too, and
// wm_phi and wm_codes, K25's table and bin codes, which K26 starts from too.  An
// entry point keeps the conditions of its own parameters and its launches.  Device side: the sums
// kernel and the LDS turn that writes a mirror.  The Gram kernels keep their staging and MFMA
// loops, 64 against 32 rows a side, sub-blocks against groups of lags, and with them their tile
// predicate and tile store: shared, either moved the registers or the instructions of one of them.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "pair_tile.h"

namespace osz {

constexpr int64_t kGramCap = (int64_t)1 << 25;   // doubles of G one batch of windows may hold (256 MiB)
constexpr int64_t kAnyLength = INT64_MAX;        // pw_plan's `longest` of a kernel without one

// The work space of one push, [stage] [chan] [G of one batch], in doubles, and its windows.
struct PwPlan {
    int64_t nwin, chan, one, batch, gram;        // `one`: a window's G; `batch`: the windows of a batch
    int64_t stage = 0, nsub = 1;                 // K19's alone: the staged phasors, the sub-blocks of a window
    int64_t work() const { return stage + chan + gram; }
};

// What every entry point and its *_work function take: `fn` the entry point's name, `own` and `value`
// its own parameter as a message names it, `flag` and `flag_value` its 0-or-1 argument if it has one.
struct PwArgs {
    const char *fn;
    int nch;
    int64_t n, W, step;
    int mask;
    const char *own;
    int value;
    const char *flag = nullptr;
    int flag_value = 0;
};

// The plan of A's rows in windows of W (shortest .. longest) for a mask of `bits` bits: chan_per
// doubles per (row, window) and gram_per doubles of G per window and pair of rows.  False for the
// sizes every pair window kernel refuses.
inline bool pw_plan(const PwArgs &A, int bits, int64_t shortest, int64_t longest, int chan_per, int64_t gram_per,
                    PwPlan *p) {
    if (A.nch < 2 || A.nch > 16384 || A.n < 0 || A.W < shortest || A.W > longest || A.step < 1 || A.mask < 1 ||
        A.mask >= 1 << bits)
        return false;
    if ((int64_t)A.nch * A.n >= ((int64_t)1 << 40)) return false;
    p->nwin = osz_window_count(A.n, A.W, A.step);
    p->chan = chan_per * (int64_t)A.nch * p->nwin;
    p->one = gram_per * A.nch * A.nch;
    const int64_t batch = kGramCap / p->one;                 // (a grid's y)
    p->batch = std::min(batch < 1 ? 1 : batch > 65535 ? 65535 : batch, p->nwin);
    p->gram = p->batch * p->one;
    return true;
}

// An array of an entry point: its address, the alignment of its elements and, for an array that only
// some masks write, whether this one does.
struct PwArray {
    const void *at;
    unsigned align;
    bool by_mask = false, needed = true;
};

// The checks of an entry point, in the order every entry point made them: the arrays every mask
// needs are not null, the plan took the sizes (`planned`), the flag is 0 or 1, the arrays this mask
// needs are not null, pitch, plane_pitch (if `planes`: the mask writes (nch, nch) planes), the
// alignments, work_len, and fewer than 2^31 windows.  `arrays` are x, the results and the work
// space.  OSZ_OK leaves P.nwin for the caller to look at: 0 is nothing to launch.
inline int pw_head(const PwArgs &A, bool planned, const PwPlan &P, std::initializer_list<PwArray> arrays, int64_t pitch,
                   bool planes, int64_t plane_pitch, int64_t work_len) {
    for (const PwArray &a : arrays) OSZ_REQUIRE(a.at || a.by_mask, "%s: null argument", A.fn);
    OSZ_REQUIRE(planned, "%s: bad sizes or measures (nch %d, n %lld, winsize %lld, step %lld, mask %d, %s %d)", A.fn, A.nch,
                (long long)A.n, (long long)A.W, (long long)A.step, A.mask, A.own, A.value);
    OSZ_REQUIRE(!A.flag || A.flag_value == 0 || A.flag_value == 1, "%s: %s must be 0 or 1, got %d", A.fn, A.flag,
                A.flag_value);
    for (const PwArray &a : arrays) OSZ_REQUIRE(a.at || !a.needed, "%s: null argument (mask %d)", A.fn, A.mask);
    OSZ_REQUIRE(pitch >= A.n, "%s: pitch %lld is less than n %lld", A.fn, (long long)pitch, (long long)A.n);
    OSZ_REQUIRE(!planes || plane_pitch >= P.nwin * A.nch * A.nch, "%s: plane_pitch %lld holds fewer than %lld windows",
                A.fn, (long long)plane_pitch, (long long)P.nwin);
    for (const PwArray &a : arrays)
        OSZ_REQUIRE((reinterpret_cast<uintptr_t>(a.at) & (a.align - 1)) == 0, "%s: an array is not %u-byte aligned", A.fn,
                    a.align);
    OSZ_REQUIRE(work_len >= P.work(), "%s: work holds %lld doubles, %s_work asks for %lld", A.fn, (long long)work_len,
                A.fn, (long long)P.work());
    OSZ_REQUIRE(P.nwin <= INT32_MAX, "%s: too many windows in one push", A.fn);
    return OSZ_OK;
}

// launch(w0, count) for every batch of the plan's windows, in order; the first failure ends the walk
template <class Launch>
inline int pw_batches(const PwPlan &P, Launch launch) {
    for (int64_t w0 = 0; w0 < P.nwin; w0 += P.batch) {
        const int rc = launch(w0, std::min(P.batch, P.nwin - w0));
        if (rc != OSZ_OK) return rc;
    }
    return OSZ_OK;
}

// K23's sums and Gram kernels (windowxcorr.hip), which K24 starts from too, for x (nch rows of pitch
// `pitch`, windows of W samples, `step` apart) and its `count` windows from window w0 on, each timed
// under the caller's label.  wx_window_sums (K23: once per push; K24: per batch): chan[w * nch + c]
// takes the sum of row c over window w about the window's first sample.  wx_lagged_gram: part[((w -
// w0) * (2 L + 1) + L + l) * nch * nch + i * nch + j], i <= j, takes G_ij(l) = sum_t d_i[t] d_j[t + l];
// count <= 65535, 0 <= L <= min(OSZ_WX_MAXLAG, W / 2).
int wx_window_sums(const double *x, int64_t pitch, int nch, int64_t W, int64_t step, int64_t w0, int64_t count,
                   double *chan, const char *timer, hipStream_t st);
int wx_lagged_gram(const double *x, int64_t pitch, int nch, int64_t W, int64_t step, int L, int64_t w0,
                   int64_t count, const double *chan, double *part, const char *timer, hipStream_t st);

// K17's launcher (windowquant.hip), which K25 takes its quantile edges from: osz_window_quantiles
// with its arguments and checks, on stream st, timed under the caller's label.
int wq_quantiles(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                 const double *q, int nq, double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0,
                 const char *label, hipStream_t st);

// K25's phi table, edges and bin codes (windowmi.hip), which K26 starts from too, each launch timed
// under the caller's label.  wm_phi: phi[n] = n ln n for n = 0 .. W.  wm_codes, for x (nch rows of
// pitch `pitch`) at the first of `count` <= 65535 windows of W samples, `step` apart: the edges of
// the `bins` bins (binning OSZ_WM_QUANTILE: through wq_quantiles into `edges`, OSZ_WM_MAXBINS
// doubles per (row, window); OSZ_WM_UNIFORM: inside the code kernel), then per (window w, row c)
// the codes, codes[(w * nch + c) * wpad + t] = the bin of sample t, 0xFF for W <= t < wpad (wpad: W
// rounded up to a multiple of 64), and meta[(w * nch + c) * (OSZ_WM_MAXBINS + 2) + ..]: the
// marginal counts, at OSZ_WM_MAXBINS their sum of phi, at OSZ_WM_MAXBINS + 1 the non-finite flag.
int wm_phi(double *phi, int W, const char *label, hipStream_t st);
int wm_codes(const double *x, int64_t pitch, int nch, int W, int64_t step, int64_t count, int bins, int binning,
             const double *phi, double *edges, double *meta, unsigned char *codes, int wpad, const char *edges_label,
             const char *code_label, hipStream_t st);

// where the bytes of the word w equal those of `same` (a byte repeated four times): 1, else 0
__device__ __forceinline__ unsigned mi_onehot(unsigned w, unsigned same) {
    const unsigned x = w ^ same, low = 0x7F7F7F7Fu;
    return (~(((x & low) + low) | x | low)) >> 7;
}

typedef double pair_d4 __attribute__((ext_vector_type(4)));   // one lane's share of a 16 x 16 MFMA tile
constexpr int kPwTile = 16;                                   // rows per side of an MFMA tile

// The body of the two sums kernels, one wave per (window, row): chan[(w * NS) * nch + c] = sum over
// the window of x - p, p the window's first sample; NS = 2 (K19) adds chan[(w * 2 + 1) * nch + c] =
// sum |u|^2 of the phasor (ux, uy) of complex data, 0 without one.  Lane l owns the samples l + 64 k
// in that order; wave_sum63 folds the lanes.
template <int NS>
__device__ __forceinline__ void window_sums(const double *__restrict__ x, int64_t ld, int nch, int64_t W, int64_t step,
                                            const double *__restrict__ ux, const double *__restrict__ uy,
                                            double *__restrict__ chan) {
    const int64_t w = blockIdx.x;
    const int c = blockIdx.y, lane = threadIdx.x;
    const int64_t at = (int64_t)c * ld + w * step;
    const double p = x[at];
    double s = 0.0, f = 0.0;
    for (int64_t t = lane; t < W; t += kWave) {
        s += x[at + t] - p;
        if (NS == 2 && ux) {
            const double a = ux[at + t], b = uy[at + t];
            f += __builtin_fma(a, a, b * b);
        }
    }
    s = wave_sum63(s);
    if (NS == 2) f = wave_sum63(f);
    if (lane == kWave - 1) {
        chan[(w * NS) * nch + c] = s;
        if (NS == 2) chan[(w * 2 + 1) * nch + c] = f;
    }
}

// Thread (a, b) of a T x T tile of pairs hands v to thread (b, a), which writes it to *dst if it is
// `mirrored`: the mirror's rows stay whole.  Two barriers; every thread of the workgroup calls it.
template <int T>
__device__ __forceinline__ void pw_mirror(double (&turn)[T][T + 1], int a, int b, double v, bool mirrored,
                                          double *dst) {
    turn[a][b] = v;
    __syncthreads();
    if (mirrored) *dst = turn[b][a];
    __syncthreads();
}

}  // namespace osz
