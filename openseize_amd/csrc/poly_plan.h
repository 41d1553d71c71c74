// poly_plan.h -- host-side planning of the polyphase resampler (poly.hip): which tile the block
// kernel takes, how many phase groups share it, the pitch of a phase stream in LDS, and the
// blocked sub-filter table G[r][e][a].  Plain C++ (no HIP): poly.hip calls it, and
// tests/host/poly_host_check.cpp builds the same plans and tables with g++.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace osz {
namespace polyplan {

constexpr int kR = 4;                     // consecutive outputs per thread (kPolyR)
constexpr int kBlk = 8;                   // taps per coefficient block (kPolyBlk)
constexpr size_t kLdsShared = 53 * 1024;  // a window three workgroups per CU have room for
constexpr size_t kLdsAlone = 150 * 1024;  // the smallest tile may take most of a CU's 160 KB

struct Plan {
    int H = 0;        // input samples of history the handle carries
    int apad = 0;     // taps per phase stream, multiple of kBlk
    int nt = 0;       // output threads per tile (256, 128 or 64); 0: the window of no tile fits LDS
    int se = 0;       // LDS doubles per phase stream
    int eg = 1;       // phase groups per workgroup (1, 2 or 4): nt * eg threads
    int stepw = 0;    // staging: threads of the workgroup rounded down to a multiple of M
    int dqs = 0;      // stepw / M
    size_t lds = 0;   // dynamic LDS bytes of a workgroup
};

inline size_t lds_bytes(int L, int M, int nt, int se) {
    return ((size_t)M * se + (L == 1 ? 0 : (size_t)nt * kR * L)) * sizeof(double);
}

inline size_t lds_limit(int nt) { return nt == 64 ? kLdsAlone : kLdsShared; }

// Phase groups of a workgroup whose window takes `bytes` of LDS: decimators on a 128- or
// 64-thread tile only; two (four measured no faster), four when the window leaves room for one
// or two workgroups per CU only.
inline int phase_groups(int L, int M, int nt, size_t bytes) {
    if (L != 1 || nt > 128) return 1;
    const int eg_on = bytes > kLdsShared ? 4 : 2;
    return eg_on >= 4 && M >= 4 ? 4 : M >= 2 ? 2 : 1;
}

inline Plan plan(int ntaps, int L, int M) {
    Plan p;
    p.H = (ntaps - 1 + L - 1) / L + 1;
    const int msub_max = (ntaps + L - 1) / L;
    int apad = (msub_max + M - 1) / M;                       // taps per phase stream
    apad = (apad + kBlk - 1) / kBlk * kBlk;
    p.apad = apad;
    for (int nt = 256; nt >= 64 && !p.nt; nt >>= 1) {
        const int nstream = nt * kR + apad;
        const int se = (nstream + (nstream >> 2) + 2) | 1;   // odd: spreads the staging writes
        // (the smallest tile may take most of a CU's 160 KB: one workgroup per CU then, still
        // fifty times the rate of the kernel that reads its window through the caches)
        if (lds_bytes(L, M, nt, se) <= lds_limit(nt)) {
            p.nt = nt;
            p.se = se;
        }
    }
    if (!p.nt) return p;
    // The stream pitch decides how the staging writes fall on the banks: a ds_write_b64
    // is served in groups of 16 consecutive lanes, conflict free when their 16 double
    // addresses e * se + pad(i) differ mod 16 (MI355X_MICROARCH.md, LDS).  Lanes walk
    // (i, e) = (w div M, w mod M), so the best pitch depends on M: take, among the 16
    // pitches from the needed one up, the one with the fewest extra LDS cycles over the
    // first steps of a tile (it was "any odd pitch": 30 % of the LDS cycles were conflicts).
    // (threads per workgroup by the phase-group rule at the needed pitch)
    const int nth = p.nt * phase_groups(L, M, p.nt, lds_bytes(L, M, p.nt, p.se));
    const int stepw = nth - nth % M, dqs = M <= nth ? stepw / M : 0;
    auto extra_cycles = [&](int se) {
        long cost = 0;
        for (int u = 0; u < 8; ++u)
            for (int g0 = 0; g0 < nth; g0 += 16) {
                int cnt[16] = {0}, worst = 0;
                for (int tw = g0; tw < g0 + 16 && tw < nth; ++tw) {
                    const int i = tw / M + u * dqs, e = tw % M;
                    const int bank = (int)(((long)e * se + i + (i >> 2)) & 15);
                    worst = std::max(worst, ++cnt[bank]);
                }
                cost += worst - 1;
            }
        return cost;
    };
    if (M <= nth) {
        int best = p.se;
        long best_cost = extra_cycles(best);
        for (int cand = p.se + 1; cand < p.se + 16 && best_cost > 0; ++cand) {
            if (lds_bytes(L, M, p.nt, cand) > lds_limit(p.nt)) break;
            const long c = extra_cycles(cand);
            if (c < best_cost) {
                best_cost = c;
                best = cand;
            }
        }
        p.se = best;
    }
    // what a push launches: the phase-group rule at the pitch taken
    p.lds = lds_bytes(L, M, p.nt, p.se);
    p.eg = phase_groups(L, M, p.nt, p.lds);
    p.stepw = p.eg * p.nt - (p.eg * p.nt) % M;
    p.dqs = p.stepw / M;
    return p;
}

// Blocked sub-filters G[r][e][a] = hsub_r[msub_r - 1 - (M a + e)], zero padded to apad taps per
// phase stream; hsub_r[k'] = hL[phi_r + L k'], phi_r = (r M + centre) mod L.
inline std::vector<double> build_G(const double *hL, int ntaps, int centre, int L, int M, int apad) {
    std::vector<double> G((size_t)L * M * apad, 0.0);
    for (int r = 0; r < L; ++r) {
        const int phi = (int)(((int64_t)r * M + centre) % L);
        const int msub = phi < ntaps ? (ntaps - phi + L - 1) / L : 0;
        for (int kk = 0; kk < msub; ++kk) {
            const int u = msub - 1 - kk, aa = u / M, e = u % M;
            G[((size_t)r * M + e) * apad + aa] = hL[phi + (size_t)L * kk];
        }
    }
    return G;
}

}  // namespace polyplan
}  // namespace osz
