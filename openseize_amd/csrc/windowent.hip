// windowent.hip -- K16 sample and permutation entropy per window (features/entropy.py
// window_entropy): for every window of W samples, step apart, of every channel the numbers of
// osz_window_entropy_measure -- pattern counts, where K15's features are sums.  DESIGN.md
// section 4, K16.
//
// One workgroup per (channel, window) -- 64 threads for W < OSZ_WE_WIDE, 256 from there on -- on a
// one-dimensional grid:
//   * the window goes into LDS once; the same pass takes the ballot for non-finite samples and the
//     sums of y = x - p and y^2 about the pivot p, the window's first sample, that give the std;
//     thread tid sums the samples tid + NT k in that order, the lanes are folded by wave_sum63 and
//     the waves in wave order: a function of W alone;
//   * sample entropy walks diagonals of the pair matrix: a lane owns a lag L = j - i and steps t
//     along it, x_{t+L} from LDS, consecutive over the lanes, x_t -- the same for every lane --
//     from the row itself through the scalar cache, eight samples a load: it arrives in scalar
//     registers, costs the LDS nothing and is an operand of the subtraction as it stands.  `run`, the number of
//     consecutive t' <= t with |x_t' - x_{t'+L}| <= rho, says in one compare whether the template
//     pair that ends at t matches over m and over m + 1 samples, so any m costs the same.  A lane
//     takes lag L and then lag W - m - L: W + m steps whatever L is; a wave walks 64 consecutive
//     lags to the end of the longest, W + m + 63 steps, of which all but 63 carry no predicate.
//     The counts are integers;
//   * permutation entropy takes the Lehmer code of each vector from order (order - 1) / 2 compares
//     and counts it in an LDS histogram with 32-bit integer adds; one wave folds -sum p log2 p,
//     lane l the bins l + 64 k in that order, the lanes by wave_sum63.
// No floating-point operation is atomic, so a window's bits depend on W, the parameters and its
// own samples only.
#include "window_block.h"

namespace osz {

#pragma clang fp contract(off)

constexpr int kWePad = 64;            // doubles behind the window in LDS: a wave's walk reads up to 63 past its end
constexpr int kWeBins = 720;          // 6!
constexpr int kWeOrder = 6;

// the lane counts of a window's matching pairs fit 32 bits: there are fewer than W^2 / 2 pairs
static_assert((int64_t)OSZ_WE_LONGEST * OSZ_WE_LONGEST / 2 < ((int64_t)1 << 32), "OSZ_WE_LONGEST");
static_assert(OSZ_WE_WIDE >= 2 * kWave && kWePad >= kWave, "window_entropy_kernel");

struct WeArgs : WinHead {
    int m, tol;
    double r;
    int order, delay, normalize;
};

// One step t along a diagonal of lag L: xt = x_t, xf = x_{t+L}.  With run the matches in a row up
// to t - 1, the templates i = t - m, j = i + L match over m samples when run >= m (both are
// templates: j + m = t + L <= W - 1) and over m + 1 when x_t and x_{t+L} match as well.  b counts
// for the lane, a for the whole wave: the two compares leave their lanes as scalar masks, and
// the scalar unit counts the bits of their intersection beside the vector work -- one counter on
// each unit keeps both under the five vector instructions of the step itself (counting both on
// the scalar unit ran 11 .. 20 % slower: it issues one instruction where the vector unit issues
// two).  (A lane with rho < 0 never matches and counts nothing.)
__device__ __forceinline__ void we_step(double xt, double xf, bool valid, int m, double rho, int &run, unsigned &a,
                                        unsigned &b) {
    const bool hit = (__builtin_fabs(xt - xf) <= rho) & valid;
    const bool had = run >= m;
    b += (unsigned)(had & valid);
    a += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(had) & __builtin_amdgcn_ballot_w64(hit));
    run = hit ? run + 1 : 0;
}

// The diagonal of lag L, steps t = 0 .. steps - 1 (`steps` and `full` are the wave's): the lane's
// own diagonal ends at t = end - 1 = W - 1 - L, no lane's before t = full - 1.  The first `full`
// steps carry no predicate, and the loads of eight steps are issued before the first is used.
__device__ __forceinline__ void we_walk(const double *__restrict__ row, const double *win, int L, int end, int full,
                                        int steps, int m, double rho, unsigned &a, unsigned &b) {
    const double *far = win + L;
    int run = 0, t = 0;
    for (; t + 8 <= full; t += 8) {
        double xt[8], xf[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            xt[u] = row[t + u];
            xf[u] = far[t + u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) we_step(xt[u], xf[u], true, m, rho, run, a, b);
    }
    for (; t < steps; ++t) we_step(row[t], far[t], t < end, m, rho, run, a, b);
}

template <int NT>
__global__ void __launch_bounds__(NT) window_entropy_kernel(const WeArgs A) {
    constexpr int NW = NT / kWave;
    extern __shared__ double we_win[];                     // W + kWePad
    __shared__ unsigned hist[kWeBins];
    __shared__ unsigned cnt[2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = A.W;
    const WinAt at = win_where(A);
    const double *__restrict__ row = at.row;
    double *__restrict__ dst = at.dst;
    const int planes = __builtin_popcount(A.mask);

    // the window into LDS, the sums about its first sample, the ballot
    const double x0 = row[0], p = __builtin_isfinite(x0) ? x0 : 0.0;
    double S[2] = {0.0, 0.0};                              // sum y, sum y^2
    bool wild = false;
    for (int t = tid; t < W; t += NT) {
        const double v = row[t];
        we_win[t] = v;
        wild |= !__builtin_isfinite(v);
        const double y = v - p;
        S[0] += y;
        S[1] += y * y;
    }
    if (tid < kWePad) we_win[W + tid] = 0.0;
    for (int i = tid; i < kWeBins; i += NT) hist[i] = 0u;
    if (tid < 2) cnt[tid] = 0u;
    if (win_fold<NW>(S, wild, lane, w)) {                  // (the whole workgroup; its barrier publishes the window too)
        win_spoilt<NT>(dst, planes, A.plane_pitch, tid);
        return;
    }

    if (A.mask & 7) {
        double rho = A.r;
        if (A.tol == OSZ_WE_TOL_STD) {
            const double rn = 1.0 / (double)W, mu = S[0] * rn;
            rho = A.r * sqrt(__builtin_fmax(S[1] * rn - mu * mu, 0.0));
        }
        // The templates are 0 .. N - 1, the lags 1 .. N - 1; task q of the N / 2 takes lag q + 1
        // and then lag N - (q + 1) (the same lag once, for the middle one of an even N).  A wave
        // takes 64 consecutive tasks at a time.
        const int m = A.m, N = W - m, T = N / 2;
        // A lane without a diagonal of its own walks lag 0 with rho = -1: it matches nothing.  a is
        // the wave's count, b the lane's.
        unsigned a = 0u, b = 0u;
        for (int q0 = w * kWave; q0 < T; q0 += NT) {
            const int L = q0 + lane + 1, L2 = N - L, last = q0 + kWave < T ? q0 + kWave : T;   // (the group's last lag)
            const bool on = L <= T, on2 = on && L2 != L;
            we_walk(row, we_win, on ? L : 0, on ? W - L : 0, W - last, W - q0 - 1, m, on ? rho : -1.0, a, b);
            we_walk(row, we_win, on2 ? L2 : 0, on2 ? m + L : 0, m + q0 + 1, m + last, m, on2 ? rho : -1.0, a, b);
        }
        if (lane == 0) atomicAdd(&cnt[0], a);
        atomicAdd(&cnt[1], b);
    }

    int nvec = 0, nbins = 1;
    if (A.mask & (1 << OSZ_WE_PERMUTATION)) {
        // weight of element k's Lehmer digit, (order - 1 - k)!; a vector is padded to six
        // elements with +inf, which no element is greater than: their digits are 0
        const int d = A.order, tau = A.delay;
        int wt[kWeOrder];
#pragma unroll
        for (int j = kWeOrder - 1; j >= 0; --j) {
            wt[j] = j < d ? nbins : 0;
            if (j < d) nbins *= d - j;
        }
        nvec = W - (d - 1) * tau;
        for (int t = tid; t < nvec; t += NT) {
            double v[kWeOrder];
#pragma unroll
            for (int j = 0; j < kWeOrder; ++j) {
                const double u = we_win[j < d ? t + j * tau : t];
                v[j] = j < d ? u : __builtin_inf();
            }
            int idx = 0;
#pragma unroll
            for (int j = 0; j < kWeOrder - 1; ++j) {
                int less = 0;                              // later elements below element j (a tie goes to the earlier)
#pragma unroll
                for (int l = j + 1; l < kWeOrder; ++l) less += v[l] < v[j];
                idx += less * wt[j];
            }
            atomicAdd(&hist[idx], 1u);
        }
    }
    __syncthreads();

    if (w != 0) return;
    if (A.mask & (1 << OSZ_WE_PERMUTATION)) {
        double acc = 0.0;
        for (int i = lane; i < nbins; i += kWave) {
            const unsigned n = hist[i];
            if (n) {
                const double pr = (double)n / (double)nvec;
                acc += pr * log2(pr);
            }
        }
        acc = wave_sum63(acc);
        if (lane == kWave - 1) {
            double h = 0.0 - acc;
            if (A.normalize) h /= log2((double)nbins);
            dst[(int64_t)__builtin_popcount(A.mask & 7) * A.plane_pitch] = h;
        }
    }
    if (lane == 0 && (A.mask & 7)) {
        const double a = (double)cnt[0], b = (double)cnt[1];
        int pl = 0;
        if (A.mask & (1 << OSZ_WE_SAMPLE)) dst[(int64_t)pl++ * A.plane_pitch] = 0.0 - log(a / b);
        if (A.mask & (1 << OSZ_WE_SAMPLE_A)) dst[(int64_t)pl++ * A.plane_pitch] = a;
        if (A.mask & (1 << OSZ_WE_SAMPLE_B)) dst[(int64_t)pl * A.plane_pitch] = b;
    }
}

}  // namespace osz

using namespace osz;

extern "C" {

int osz_window_entropy(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                       int m, double r, int tolerance, int order, int64_t delay, int normalize, double *out,
                       int64_t plane_pitch, int64_t row_pitch, int64_t win0, void *stream) {
    static const WinRule rule = {"osz_window_entropy", "measure", OSZ_WE_COUNT, 4, OSZ_WE_LONGEST};
    WeArgs A;
    if (int rc = win_head(rule, __builtin_popcount(mask), x, pitch, nch, n, winsize, step, mask, out, plane_pitch,
                          row_pitch, win0, A))
        return rc;
    OSZ_REQUIRE(m >= 1 && m <= 8 && r >= 0.0 && __builtin_isfinite(r) &&
                    (tolerance == OSZ_WE_TOL_STD || tolerance == OSZ_WE_TOL_ABSOLUTE),
                "osz_window_entropy: m=%d (1 .. 8) r=%g (finite, >= 0) tolerance=%d (0, 1)", m, r, tolerance);
    OSZ_REQUIRE(order >= 2 && order <= kWeOrder && delay >= 1,
                "osz_window_entropy: order=%d (2 .. %d) delay=%lld (>= 1)", order, kWeOrder, (long long)delay);
    const bool sample = (mask & 7) != 0, perm = (mask & (1 << OSZ_WE_PERMUTATION)) != 0;
    OSZ_REQUIRE(!sample || winsize >= m + 2, "osz_window_entropy: winsize=%lld holds no pair of templates of m=%d",
                (long long)winsize, m);
    OSZ_REQUIRE(!perm || (delay < winsize && (order - 1) * delay < winsize),
                "osz_window_entropy: winsize=%lld holds no vector of order=%d, delay=%lld", (long long)winsize, order,
                (long long)delay);
    if (A.nwin == 0) return OSZ_OK;
    unsigned nblk;
    if (int rc = win_grid(rule, A, nch, nblk)) return rc;
    A.m = m;
    A.tol = tolerance;
    A.r = r;
    A.order = order;
    A.delay = perm ? (int)delay : 1;
    A.normalize = normalize;
    const size_t lds = (size_t)(winsize + kWePad) * sizeof(double);
    hipStream_t st = as_stream(stream);
    KernelTimer timer("window_entropy", st);
    if (winsize >= OSZ_WE_WIDE) hipLaunchKernelGGL(window_entropy_kernel<256>, dim3(nblk), dim3(256), lds, st, A);
    else hipLaunchKernelGGL(window_entropy_kernel<64>, dim3(nblk), dim3(64), lds, st, A);
    OSZ_HIP(hipGetLastError());
    return OSZ_OK;
}

}  // extern "C"
