/* sos_ref_ld.c -- the definition the SOS launch routes are tested against
 * (tests/sos_routes.py): a cascade of second-order sections as a SERIAL
 * transposed direct form II recurrence in long double (x87 80-bit, 64-bit
 * mantissa).  Coefficients and input are widened, the state stays in long
 * double from call to call, and an output is rounded once, to the double it is
 * returned as.  Compile WITHOUT fast-math: the order of operations below is the
 * definition.
 *
 *   per section, per sample:  y  = b0 x + z0
 *                             z0 = b1 x - a1 y + z1
 *                             z1 = b2 x - a2 y
 *
 * sos     nsec x 6 doubles (b0 b1 b2 a0 a1 a2), a0 divided out in long double
 * x, y    (nch, n) with row pitches ldx, ldy; y may be NULL (state only)
 * stride  +1: samples 0 .. n-1 in this order;  -1: n-1 down to 0 (the backward
 *         pass; the output lands where its input was)
 * zi, zf  (nsec, nch, 2) long double, the layout of osz_sos_set_state; zi NULL: zero
 * peak    (nsec, nch) long double or NULL: max over the run of |input|, |output|
 *         of the section -- the scale a state's error is judged against
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define SOS_REF_MAXSEC 64

int sos_ref_ld(const double *sos, int nsec, int nch, const double *x, int64_t ldx, double *y,
               int64_t ldy, int64_t n, int64_t stride, const long double *zi, long double *zf,
               long double *peak)
{
    long double b0[SOS_REF_MAXSEC], b1[SOS_REF_MAXSEC], b2[SOS_REF_MAXSEC];
    long double a1[SOS_REF_MAXSEC], a2[SOS_REF_MAXSEC];
    long double z0[SOS_REF_MAXSEC], z1[SOS_REF_MAXSEC], pk[SOS_REF_MAXSEC];
    int s, c;
    int64_t i;
    if (nsec < 1 || nsec > SOS_REF_MAXSEC || nch < 1 || n < 0 || (stride != 1 && stride != -1))
        return -1;
    for (s = 0; s < nsec; ++s) {
        const long double a0 = (long double)sos[6 * s + 3];
        b0[s] = (long double)sos[6 * s + 0] / a0;
        b1[s] = (long double)sos[6 * s + 1] / a0;
        b2[s] = (long double)sos[6 * s + 2] / a0;
        a1[s] = (long double)sos[6 * s + 4] / a0;
        a2[s] = (long double)sos[6 * s + 5] / a0;
    }
    for (c = 0; c < nch; ++c) {
        const double *xr = x + (int64_t)c * ldx;
        double *yr = y ? y + (int64_t)c * ldy : NULL;
        for (s = 0; s < nsec; ++s) {
            z0[s] = zi ? zi[((size_t)s * nch + c) * 2 + 0] : 0.0L;
            z1[s] = zi ? zi[((size_t)s * nch + c) * 2 + 1] : 0.0L;
            pk[s] = 0.0L;
        }
        for (i = 0; i < n; ++i) {
            const int64_t k = stride > 0 ? i : n - 1 - i;
            long double u;
#ifndef SOS_REF_PLAIN   /* tests/test_sos_routes_host.py builds both and compares them */
            if (z0[0] != z0[0]) {
                /* Not an approximation, only time saved (x87 arithmetic on NaN is about a hundred
                 * times slower): a NaN in the first section's z0 makes v NaN, which keeps that z0
                 * NaN and feeds NaN to every later section, for every sample still to come.  So
                 * all of them are NaN, and after one more sample so is every state. */
                for (; i < n; ++i) {
                    const int64_t kk = stride > 0 ? i : n - 1 - i;
                    if (fabsl((long double)xr[kk]) > pk[0]) pk[0] = fabsl((long double)xr[kk]);
                    if (yr) yr[kk] = (double)z0[0];
                }
                for (s = 0; s < nsec; ++s) z0[s] = z1[s] = z0[0];
                break;
            }
#endif
            u = (long double)xr[k];
            for (s = 0; s < nsec; ++s) {
                const long double v = b0[s] * u + z0[s];
                z0[s] = b1[s] * u - a1[s] * v + z1[s];
                z1[s] = b2[s] * u - a2[s] * v;
                if (fabsl(u) > pk[s]) pk[s] = fabsl(u);
                if (fabsl(v) > pk[s]) pk[s] = fabsl(v);
                u = v;
            }
            if (yr) yr[k] = (double)u;
        }
        for (s = 0; s < nsec; ++s) {
            if (zf) {
                zf[((size_t)s * nch + c) * 2 + 0] = z0[s];
                zf[((size_t)s * nch + c) * 2 + 1] = z1[s];
            }
            if (peak) peak[(size_t)s * nch + c] = pk[s];
        }
    }
    return 0;
}
