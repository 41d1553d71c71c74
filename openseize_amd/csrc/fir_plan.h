// fir_plan.h -- host-side planning of the stand-alone overlap-add FIR (fir.hip): how a filter is
// cut into pieces, which kernel a piece runs (fir_nega_kernel<NB> or fir_oa_kernel<NR, 16, PF>)
// at which block length, and how a push of n samples is cut into blocks and runs.  Plain C++
// (no HIP): fir.hip calls it, and tests/host/fir_plan_check.cpp builds the same plans with g++.
// The run partition itself (fir_run_start) is in fir_pair.h, where the device code needs it.
#pragma once

#include <cstdint>

namespace osz {

constexpr int kFirN = 4096;        // the transform length (fft::N)
constexpr int kFirMaxTaps = 2049;  // NFFT - ntaps + 1 >= ntaps - 1
constexpr int kFirPart = 2048;     // taps per piece of a partitioned filter
constexpr int kFirMaxParts = 16;   // => up to 32768 taps

// ---- the piece split: one piece up to kFirMaxTaps taps, pieces of kFirPart taps beyond
inline int fir_nparts(int ntaps) { return ntaps <= kFirMaxTaps ? 1 : (ntaps + kFirPart - 1) / kFirPart; }
inline int fir_piece_off(int nparts, int q) { return nparts == 1 ? 0 : q * kFirPart; }
inline int fir_piece_len(int ntaps, int nparts, int q) {
    const int off = fir_piece_off(nparts, q);
    return nparts == 1 ? ntaps : (ntaps - off < kFirPart ? ntaps - off : kFirPart);
}

// ---- per piece
// fir_oa_kernel: two blocks per transform, whole rows of 256 with step + ntaps - 1 <= 4096,
// 8 (2049 taps) .. 15 (<= 257 taps) rows
inline int fir_pair_step(int ntaps) {
    int step = ((kFirN - ntaps + 1) / 256) * 256;
    if (step > 15 * 256) step = 15 * 256;
    return step;
}
// fir_nega_kernel: one block per transform of twice the window, 24 (2049 taps) .. 31 (<= 257
// taps) rows; 0: the piece has no such tables (a single tap has no tail to carry)
inline int fir_nega_step(int ntaps) {
    if (ntaps < 2 || ntaps > kFirMaxTaps) return 0;
    int nb = (2 * kFirN + 1 - ntaps) / 256;
    if (nb > 31) nb = 31;
    return 256 * nb;
}

struct FirPiecePlan {
    int nega;   // 1: fir_nega_kernel<rows>, 0: fir_oa_kernel<rows, 16, PF of fir_pf_table.h>
    int rows;   // NB or NR
    int step;   // 256 rows
};

// one real block per transform (fir_nega_kernel) where its tables exist
inline FirPiecePlan fir_piece_plan(int ntaps) {
    const int stepn = fir_nega_step(ntaps);
    FirPiecePlan p;
    p.nega = stepn != 0 && ntaps - 1 >= 1;
    p.step = p.nega ? stepn : fir_pair_step(ntaps);
    p.rows = p.step / 256;
    return p;
}

// ---- per push
struct FirPushPlan {
    int64_t nblocks, R, nruns;
};

// cus: the device's compute units
inline FirPushPlan fir_push_plan(int64_t n, int step, int nch, int cus) {
    FirPushPlan p;
    const int64_t nblocks = (n + step - 1) / step;
    // run length: long runs (every workgroup pays for its twiddle loads, its tail
    // and its seam) as long as about 3/4 of the 512 workgroup slots stay busy --
    // measured at 16..256 channels, runs of an even number of blocks
    int64_t R = (nblocks * nch) / 384;
    if (R > 32) R = 32;
    if (R < 2) R = 2;
    R &= ~1LL;
    int64_t nruns = (nblocks + R - 1) / R;       // balanced runs of <= R blocks
    {
        // whole "rounds" of resident workgroups: with W workgroups on S slots the
        // launch takes ceil(W / S) rounds, so prefer a run count that wastes
        // little of the last round (slots = CUs x workgroups per CU by LDS)
        const int64_t slots = (int64_t)cus * 2;   // 64 KB of LDS per workgroup
        int64_t best = nruns;
        double best_waste = 2.0;
        for (int64_t cand = nruns; cand < nruns + 8; ++cand) {
            const int64_t w = cand * nch, rounds = (w + slots - 1) / slots;
            const double waste = 1.0 - (double)w / (double)(rounds * slots);
            if (waste < best_waste - 1e-9) {
                best_waste = waste;
                best = cand;
            }
        }
        nruns = best;
    }
    // every run must hold at least one whole block (>= ntaps - 1 samples) so that
    // tails never reach past the run that follows: at most one run per pair of
    // blocks whose first block is whole
    if (nruns > nblocks / 2) nruns = nblocks / 2;
    if (nruns < 1) nruns = 1;
    p.nblocks = nblocks;
    p.R = R;
    p.nruns = nruns;
    return p;
}

}  // namespace osz
