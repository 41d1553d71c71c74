// fir_plan_check.cpp -- the planner of the stand-alone FIR (csrc/fir_plan.h) on the host, built by
// g++ (tests/fir_cells.py: build_host_exe).
//   fir_plan_check plan   reads "ntaps nch cus n" lines; prints, per case and piece,
//                         "case kernel rows pf piece taps step nblocks R nruns" (kernel: 0 nega, 1 pair)
//   fir_plan_check grid   the invariant fir_seam_kernel rests on, over piece lengths at both ends of
//                         every block height, nblocks 1 ... 200, nch in {1, 2, 3, 64, 256, 65535},
//                         cus in {1, 80, 256, 304} and last blocks of 1, ntaps - 1 and step samples:
//                         1 <= nruns <= max(1, nblocks / 2); every run holds a block; every run after
//                         the first begins at least ntaps - 1 samples before n and at least
//                         ntaps - 1 samples behind the start of the run before it.  Prints the
//                         failures and "checked <count>"; exit status 1 if there are any.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fir_pf_table.h"
#include "fir_plan.h"

using namespace osz;

// fir_run_start of fir_pair.h (device code, not for g++): run r starts at block
// 2 floor(r ceil(nblocks / 2) / nruns)
static int64_t run_start(int64_t r, int64_t nblocks, int64_t nruns) {
    const int64_t npairs = (nblocks + 1) / 2;
    const int64_t b = 2 * ((r * npairs) / nruns);
    return b < nblocks ? b : nblocks;
}

static int plan_mode() {
    static const int pf_table[8] = OSZ_FIR_PF_TABLE;
    long long ntaps, nch, cus, n;
    int idx = 0;
    while (scanf("%lld %lld %lld %lld", &ntaps, &nch, &cus, &n) == 4) {
        const int nparts = fir_nparts((int)ntaps);
        if (nparts > kFirMaxParts) return 2;
        for (int q = 0; q < nparts; ++q) {
            const int taps = fir_piece_len((int)ntaps, nparts, q);
            if (fir_piece_off(nparts, q) != (nparts == 1 ? 0 : q * kFirPart)) return 3;
            const FirPiecePlan pp = fir_piece_plan(taps);
            const FirPushPlan pl = fir_push_plan(n, pp.step, (int)nch, (int)cus);
            const int pf = pp.nega ? 0 : pf_table[pp.rows - 8];
            printf("%d %d %d %d %d %d %d %lld %lld %lld\n", idx, pp.nega ? 0 : 1, pp.rows, pf, q, taps, pp.step,
                   (long long)pl.nblocks, (long long)pl.R, (long long)pl.nruns);
        }
        ++idx;
    }
    return 0;
}

static int grid_mode() {
    static const int chans[] = {1, 2, 3, 64, 256, 65535}, cuss[] = {1, 80, 256, 304};
    long long checked = 0, bad = 0;
    int taps[18], nt = 0;
    taps[nt++] = 1;
    taps[nt++] = 2;
    for (int k = 257; k <= 2049; k += 256) {
        taps[nt++] = k;
        if (k < 2049) taps[nt++] = k + 1;
    }
    taps[nt++] = kFirPart;
    for (int it = 0; it < nt; ++it) {
        const FirPiecePlan pp = fir_piece_plan(taps[it]);
        const int64_t w = taps[it] - 1, S = pp.step;
        if (w > S) { printf("taps %d: tail %lld longer than a block %lld\n", taps[it], (long long)w, (long long)S); ++bad; }
        const int64_t lasts[3] = {1, w > 0 ? w : 1, S};
        for (int64_t nb = 1; nb <= 200; ++nb)
            for (int nch : chans)
                for (int cus : cuss)
                    for (int64_t last : lasts) {
                        const int64_t n = (nb - 1) * S + last;
                        const FirPushPlan pl = fir_push_plan(n, (int)S, nch, cus);
                        ++checked;
                        bool ok = pl.nblocks == nb && pl.nruns >= 1 && pl.nruns <= (nb / 2 > 1 ? nb / 2 : 1) &&
                                  pl.R >= 2 && pl.R <= 32 && pl.R % 2 == 0;
                        ok = ok && run_start(0, nb, pl.nruns) == 0 && run_start(pl.nruns, nb, pl.nruns) == nb;
                        for (int64_t r = 1; ok && r < pl.nruns; ++r) {
                            const int64_t b = run_start(r, nb, pl.nruns), prev = run_start(r - 1, nb, pl.nruns);
                            ok = b > prev && b < nb && b * S + w <= n && (b - prev) * S >= w;
                        }
                        if (!ok) {
                            if (bad < 20)
                                printf("taps %d step %lld nblocks %lld nch %d cus %d last %lld: R %lld nruns %lld\n",
                                       taps[it], (long long)S, (long long)nb, nch, cus, (long long)last,
                                       (long long)pl.R, (long long)pl.nruns);
                            ++bad;
                        }
                    }
    }
    printf("checked %lld\n", checked);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_mode();
    if (argc == 2 && !strcmp(argv[1], "grid")) return grid_mode();
    fprintf(stderr, "usage: fir_plan_check plan|grid\n");
    return 64;
}
