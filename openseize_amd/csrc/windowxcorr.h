// windowxcorr.h -- what windowxcorr.hip (K23) lends to the kernels that start from its lagged Gram
// products (K24 windowgranger.hip).
#pragma once
#include "common.h"

namespace osz {

// The doubles of G one batch of windows may hold, and the windows of a batch of `one` doubles each.
int64_t wx_batch(int64_t one);

// xcorr_sums_kernel and xcorr_gram_kernel for the `count` windows from window w0 on of x (nch rows of
// pitch `pitch`, windows of W samples, `step` apart): chan[w * nch + c] takes the sum of row c over
// window w about the window's first sample, part[((w - w0) * (2 L + 1) + L + l) * nch * nch + i * nch
// + j], i <= j, takes G_ij(l) = sum_t d_i[t] d_j[t + l] -- the bits osz_window_xcorr works from.  The
// Gram launch is timed as `timer`.  count <= 65535, 0 <= L <= min(OSZ_WX_MAXLAG, W / 2).
int wx_lagged_gram(const double *x, int64_t pitch, int nch, int64_t W, int64_t step, int L, int64_t w0,
                   int64_t count, double *chan, double *part, const char *timer, hipStream_t st);

}  // namespace osz
