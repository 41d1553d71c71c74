// Builds the plans and blocked tables of the polyphase resampler (csrc/poly_plan.h) with g++
// and writes them out for tests/poly_cells.py.
//   poly_host_check <in.bin> <out.bin>
// in:  int32 ncases, then per case int32 ntaps, centre, L, M and double taps[ntaps]
// out: per case int32 kernel (0 fallback, 1 block), ONE, NT, EG, apad, se, lds_bytes, H, half,
//      stepw, dqs, 0, then int64 count and the doubles of G[L][M][apad] (count 0 for the fallback)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "poly_plan.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    int32_t ncases;
    if (fread(&ncases, sizeof(int32_t), 1, f) != 1) return 2;
    for (int32_t c = 0; c < ncases; ++c) {
        int32_t hdr[4];
        if (fread(hdr, sizeof(int32_t), 4, f) != 4) return 2;
        const int ntaps = hdr[0], centre = hdr[1], L = hdr[2], M = hdr[3];
        if (ntaps < 1 || L < 1 || M < 1 || centre < 0 || centre >= ntaps) return 3;
        std::vector<double> hL(ntaps);
        if (fread(hL.data(), sizeof(double), hL.size(), f) != hL.size()) return 2;
        for (double &v : hL) v *= (double)L;              // as osz_poly_create_centred
        const osz::polyplan::Plan p = osz::polyplan::plan(ntaps, L, M);
        const int32_t out[12] = {p.nt ? 1 : 0, p.nt ? (int32_t)(L == 1) : 0, p.nt,     p.nt ? p.eg : 0,
                                 p.nt ? p.apad : 0, p.se, (int32_t)p.lds, p.H, centre, p.stepw, p.dqs, 0};
        fwrite(out, sizeof(int32_t), 12, g);
        std::vector<double> G;
        if (p.nt) G = osz::polyplan::build_G(hL.data(), ntaps, centre, L, M, p.apad);
        const int64_t n = (int64_t)G.size();
        fwrite(&n, sizeof(int64_t), 1, g);
        if (n) fwrite(G.data(), sizeof(double), G.size(), g);
    }
    fclose(f);
    fclose(g);
    return 0;
}
