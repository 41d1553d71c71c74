/*
 * osz_hip.h -- C ABI of libosz_hip.so: the MI355X (gfx950) implementation of
 * Openseize's chunked DSP hot path.
 *
 * The reference (mscaudill/openseize, 100 % Python) has no FFI of its own: its
 * hot loops are calls into SciPy/NumPy compiled code from
 * src/openseize/core/numerical.py.  Each entry point below replaces one of
 * those call sites (cited per function) and is what a ctypes binding inside
 * the reference would bind -- see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - plain C, no exceptions, no ownership crossing the ABI;
 *   - every function returns 0 on success and a negative osz_status otherwise;
 *     osz_last_error() gives a thread-local message;
 *   - all signal data is float64, device resident, laid out (channels, samples)
 *     row-major with a row pitch `ld` given in ELEMENTS.  Complex outputs are
 *     interleaved (re, im) float64 pairs; their pitch is in complex elements;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls
 *     only enqueue work unless documented otherwise;
 *   - one opaque handle per ITERATOR (the reference's generators each own
 *     their carried state); handles are not thread-safe.
 */
#ifndef OSZ_HIP_H
#define OSZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OSZ_OK = 0,
    OSZ_ERR_INVALID = -1,   /* bad argument            -> ValueError   */
    OSZ_ERR_HIP = -2,       /* HIP / rocFFT failure    -> RuntimeError */
    OSZ_ERR_NOMEM = -3,     /* allocation failure      -> MemoryError  */
    OSZ_ERR_STATE = -4,     /* call order violated     -> RuntimeError */
    OSZ_ERR_UNSUPPORTED = -5
} osz_status;

typedef struct osz_sos_s *osz_sos_t;
typedef struct osz_fir_s *osz_fir_t;
typedef struct osz_poly_s *osz_poly_t;
typedef struct osz_spec_s *osz_spec_t;

/* ---- library / device ------------------------------------------------- */
int osz_version(void);
const char *osz_last_error(void);
/* name may be NULL; reports the current HIP device. */
int osz_device_info(int *cu_count, size_t *hbm_bytes, char *name, int name_len);

/* Memory and stream helpers so that a host without PyTorch can drive the
 * library (the Python host uses torch tensors' data_ptr() instead). */
int osz_malloc(void **dptr, size_t bytes);
int osz_free(void *dptr);
int osz_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int osz_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int osz_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int osz_memset(void *dst, int value, size_t bytes, void *stream);
int osz_stream_sync(void *stream);
/* HIP-event timing on `stream` (torch.cuda.Event only sees torch's stream). */
int osz_event_create(void **ev);
int osz_event_destroy(void *ev);
int osz_event_record(void *ev, void *stream);
int osz_event_elapsed_ms(void *start, void *stop, float *ms); /* syncs stop */

/* Per-kernel timing with HIP events on the launch stream.  While enabled every
 * kernel launch of the library is bracketed by two events; query syncs and
 * returns the launches and summed milliseconds recorded under `name`
 * ("fir_oa", "fir_seam", "sos_fwd", "sos_warmup", "sos_bwd", "poly",
 * "spec_prep", "spec_rocfft", "spec_post"). */
int osz_profile_enable(int on);
int osz_profile_reset(void);
int osz_profile_query(const char *name, int64_t *launches, double *total_ms);

/* ---- K2/K3: cascaded second-order sections ---------------------------- */
/*
 * Replaces scipy.signal.sosfilt as called by the reference at
 *   core/numerical.py:334        (sosfilt: forward, zi carried per chunk)
 *   core/numerical.py:399,402,410 (sosfiltfilt: backward passes on flips)
 * sos: nsec x 6 host doubles (b0 b1 b2 a0 a1 a2; a0 is divided out).
 * The handle owns the carried state z (nsec, nch, 2) on the device.
 */
int osz_sos_create(osz_sos_t *h, const double *sos, int nsec, int nch);
int osz_sos_destroy(osz_sos_t h);
/* zi/zf host arrays laid out (nsec, nch, 2) like the reference's zi argument
 * (core/numerical.py:313-329).  zi == NULL zeroes the state.  Synchronous -- or, handed a
 * DEVICE array of the same layout, a copy ordered on `stream` that nothing waits for (a
 * snapshot the caller may never need: core/numerical.py's zero-phase stream, before its end). */
int osz_sos_set_state(osz_sos_t h, const double *zi, void *stream);
int osz_sos_get_state(osz_sos_t h, double *zf, void *stream);
/* zi_unit (nsec, 2) is the steady-state unit-step state the reference gets from
 * scipy.signal.sosfilt_zi at core/numerical.py:378.  The library derives it
 * from the coefficients at create time; this call overrides it (host doubles).
 * Synchronous. */
int osz_sos_set_zi_unit(osz_sos_t h, const double *zi_unit);
/* state[s, c, :] = zi_unit[s, :] * x[c, col]  -- the steady-state start the
 * reference builds at core/numerical.py:374-386 (zi * x0). x: device. */
int osz_sos_set_state_scaled(osz_sos_t h, const double *x, int64_t ldx,
                             int64_t col, void *stream);
/* y[c, 0:n] = cascade(x[c, 0:n]) continuing from the carried state, which is
 * advanced (core/numerical.py:332-335). x == y (in place) is allowed. */
int osz_sos_forward(osz_sos_t h, const double *x, int64_t ldx, double *y,
                    int64_t ldy, int64_t n, void *stream);
/*
 * Backward sweep of sosfiltfilt for one chunk (core/numerical.py:390-411).
 *   fa (nch, na): forward-filtered chunk i;  fb (nch, nb): forward-filtered
 *   chunk i+1 or NULL for the last chunk.
 * fb != NULL: warm-up = back-filter fb from zi_unit * fb[:, nb-1], keep only
 * its final state (:397-399), then back-filter fa from that state (:401-403).
 * fb == NULL: back-filter fa from zi_unit * fa[:, na-1] (:408-411).
 * y (nch, na) receives the result in natural sample order. The handle's
 * carried forward state is not touched.
 */
/* Samples of forward chunk i+1 (counted from its start) that the chunk-local
 * backward warm-up of chunk i reads: beyond them the state has forgotten its start
 * to below 1e-16 (1 << 62: the whole chunk).  fb / nb of the calls below may be cut
 * to this length. */
int64_t osz_sos_warm_len(osz_sos_t h);

/* The warm-up over fb stops once further samples cannot change a float64
 * state: after warmup_len samples, the smallest multiple of the kernel tile
 * with ||M^len||_inf < 1e-18 (M: state-transition matrix of the cascade).
 * For slowly decaying cascades warmup_len exceeds the chunk and the whole of
 * fb is used, exactly as the reference does.  set(0) forces the full chunk. */
int64_t osz_sos_warmup_len(osz_sos_t h);
int osz_sos_set_warmup_len(osz_sos_t h, int64_t len);
int osz_sosfiltfilt_chunk(osz_sos_t h, const double *fa, int64_t ldfa,
                          int64_t na, const double *fb, int64_t ldfb,
                          int64_t nb, double *y, int64_t ldy, void *stream);

/*
 * One steady-state step of sosfiltfilt in a single launch: forward-filter the
 * incoming chunk x (nch, nx) -> f (advancing the carried state) AND back-filter
 * an earlier forward chunk fa with the warm-up over fb (as
 * osz_sosfiltfilt_chunk) -> y.  The two passes are independent and share the
 * GPU (two workgroups per CU).  Equivalent to osz_sos_forward followed by
 * osz_sosfiltfilt_chunk, which it falls back to for ragged chunk lengths.
 */
int osz_sosfiltfilt_step(osz_sos_t h, const double *x, int64_t ldx, int64_t nx,
                         double *f, int64_t ldf, const double *fa, int64_t ldfa,
                         int64_t na, const double *fb, int64_t ldfb, int64_t nb,
                         double *y, int64_t ldy, void *stream);

/*
 * What the handle's most recent osz_sos_forward, osz_sosfiltfilt_chunk or
 * osz_sosfiltfilt_step call launched, in launch order: each launch site of the
 * cascade notes what it launches, as it launches it.  A record is OSZ_SOS_LAUNCH_FIELDS
 * int64 values:
 *   [0] kernel      OSZ_SOSK_*
 *   [1] rev         1 a backward pass, 0 a forward one, -1 one of each (the dual launches)
 *   [2] guard       1 the bounds-checked body (a ragged length), 0 whole tiles
 *   [3] al16        1 / 0 the instance for 16-byte aligned rows or the other; -1 the
 *                   kernel has no such instances
 *   [4] nseg        time segments per pass (1: one workgroup per channel)
 *   [5] seglen      samples per segment but the last (the dual launches: of the
 *                   forward pass; OSZ_SOSK_SEAL: of the runs it seals)
 *   [6] seglen_b    the dual launches: samples per segment of the backward pass; else 0
 *   [7] pre         samples segment s > 0 starts early, from a zero state
 *   [8] prex        1 the chunk-local warm-up rides the launch as a pre-roll
 *   [9] warmup      1 the state-only warm-up launch (nothing is written but a state)
 *   [10] n          samples per channel (the dual launches: of the forward pass)
 *   [11] n_b        the dual launches: samples per channel of the backward pass; else 0
 * Up to `cap` records go to `out` (host, cap * OSZ_SOS_LAUNCH_FIELDS values); *count
 * is the number of launches noted (at most OSZ_SOS_LAUNCH_RECORDS are kept).
 */
#define OSZ_SOS_LAUNCH_FIELDS 12
#define OSZ_SOS_LAUNCH_RECORDS 8
enum {
    OSZ_SOSK_KERNEL = 0,      /* sos_kernel: one workgroup per channel           */
    OSZ_SOSK_SPLIT = 1,       /* sos_split_kernel                                */
    OSZ_SOSK_SPLIT_LEAN = 2,  /* sos_split_lean_kernel                           */
    OSZ_SOSK_SPLIT2 = 3,      /* sos_split2_kernel                               */
    OSZ_SOSK_DUAL = 4,        /* sos_dual_kernel                                 */
    OSZ_SOSK_DUAL_LEAN = 5,   /* sos_dual_lean_kernel                            */
    OSZ_SOSK_DUAL2 = 6,       /* sos_dual2_kernel                                */
    OSZ_SOSK_SEAL = 7         /* sos_seal_kernel: NaN reach behind a cut forward pass */
};
int osz_sos_last_launches(osz_sos_t h, int64_t *out, int cap, int *count);

/* ---- K1: streaming FFT overlap-add FIR -------------------------------- */
/*
 * Replaces the np.fft.rfft / irfft circular convolution and overlap add of
 * oaconvolve (core/numerical.py:229-251, hot loop :254-298).  The handle
 * carries the (nch, ntaps-1) overlap tail.  The stream of FULL linear
 * convolution samples is produced; boundary modes (:143-150) are applied by
 * the caller through `skip` (left cut) and by trimming the flush.
 */
int osz_fir_create(osz_fir_t *h, const double *taps, int ntaps, int nch);
int osz_fir_destroy(osz_fir_t h);
int osz_fir_reset(osz_fir_t h, void *stream);
/* Checkpoint / resume (the de-facto state of the reference's
 * generator is the overlap tail, core/numerical.py:223, :269): the carried
 * tail(s) as osz_fir_state_size() host doubles.  Synchronous; with a device array instead,
 * ordered on `stream` and not waited for (as osz_sos_get_state). */
int64_t osz_fir_state_size(osz_fir_t h);
int osz_fir_get_state(osz_fir_t h, double *state, void *stream);
int osz_fir_set_state(osz_fir_t h, const double *state, void *stream);
/* Consumes x (nch, n) and writes the n next samples of the full convolution,
 * minus the first `skip` of them, to y (nch, n - skip); 0 <= skip <= n. */
int osz_fir_push(osz_fir_t h, const double *x, int64_t ldx, int64_t n,
                 double *y, int64_t ldy, int64_t skip, void *stream);
/* Writes tail[skip : ntaps-1-drop] (the samples after the last input) to y.
 * Does not modify the carried tail. */
int osz_fir_flush(osz_fir_t h, double *y, int64_t ldy, int64_t skip,
                  int64_t drop, void *stream);
/*
 * What the handle's most recent osz_fir_push launched, in launch order: one record per
 * main-kernel launch, that is one per piece of the filter (one piece up to 2049 taps, pieces
 * of 2048 taps beyond).  The seam kernel behind each launch and the work-row kernels of a
 * partitioned filter are not noted.  A record is OSZ_FIR_LAUNCH_FIELDS int64 values:
 *   [0] kernel      OSZ_FIRK_*
 *   [1] rows        rows of 256 samples per block: NB of fir_nega_kernel<NB> (24 ... 31),
 *                   NR of fir_oa_kernel<NR, 16, PF> (8 ... 15)
 *   [2] pf          OSZ_FIRK_PAIR: the variant PF (fir_pf_table.h); OSZ_FIRK_NEGA: 0
 *   [3] piece       index of the piece
 *   [4] taps        taps of the piece
 *   [5] step        samples per block, 256 rows
 *   [6] nblocks     blocks of the push, the last one may be ragged
 *   [7] R           the run length the planner aimed at, in blocks
 *   [8] nruns       runs (workgroups per channel); run r starts at block
 *                   min(2 floor(r ceil(nblocks / 2) / nruns), nblocks)
 *   [9] accum       1 the launch adds into the work row of a partitioned filter, 0 it writes
 *   [10] n          samples per channel
 *   [11] skip       leading output samples not written (a piece of a partitioned filter: 0,
 *                   the cut is made when the work row is drained)
 * Up to `cap` records go to `out` (host, cap * OSZ_FIR_LAUNCH_FIELDS values); *count is the
 * number of launches noted (at most OSZ_FIR_LAUNCH_RECORDS, one per piece, are kept).  A push
 * of no samples launches nothing.
 */
#define OSZ_FIR_LAUNCH_FIELDS 12
#define OSZ_FIR_LAUNCH_RECORDS 16
enum {
    OSZ_FIRK_NEGA = 0,        /* fir_nega_kernel: one real block per transform    */
    OSZ_FIRK_PAIR = 1         /* fir_oa_kernel: a pair of blocks per transform    */
};
int osz_fir_last_launches(osz_fir_t h, int64_t *out, int cap, int *count);

/* ---- K1 + K2 fused: FIR feeding the forward pass of a cascade --------- */
/*
 * The forward half of the chain the reference builds from two generators --
 * oaconvolve (core/numerical.py:158-298, 'full' stream, no left cut) into
 * sosfilt / the forward pass of sosfiltfilt (:301-335, :374-386) -- in one
 * kernel: f = sosfilt(fir(x)) for the next n samples of every channel, both
 * handles' carried states advanced exactly as osz_fir_push(skip = 0) followed
 * by osz_sos_forward would.  The FIR output never reaches HBM (16 instead of
 * 32 B per channel-sample).  Which kernel takes the chunk: osz_chain_forward_route
 * below.  What no fused kernel takes (partitioned FIRs, chunks of fewer than four
 * block pairs on route 0, the ragged head of a chunk there) runs through the
 * separate kernels inside the call: same results, same carried states.
 */
int osz_chain_forward(osz_fir_t fir, osz_sos_t sos, const double *x, int64_t ldx,
                      int64_t n, double *f, int64_t ldf, void *stream);
/* Which kernel osz_chain_forward runs the whole blocks of this pair of handles on:
 * 2 = FIR and cascade as one multiplication per bin, one 8192-sample block per 4096-point
 * transform (chain_zpn_kernel<.., ZP = false>); 1 = the same with a pair of blocks per
 * transform (chain_spec_kernel: cascades the first does not take); 0 = the FIR in the
 * spectrum and the cascade as a scan in time (chain_kernel); -1 on error.  Builds the
 * pair's tables on first use (cached on the handles); a handle paired otherwise before
 * gets its own carried state back on `stream`.  Diagnostic: tests and coverage tables. */
int osz_chain_forward_route(osz_fir_t fir, osz_sos_t sos, void *stream);
/* The plan behind osz_chain_forward_route, for tests that check every compiled instance
 * (read-only: it builds the pair's tables as the route does and decides nothing).  Fills
 * out[0 .. n), n >= 6, with: route (as osz_chain_forward_route), rows (NB on route 2, NR on
 * routes 1 and 0 -- route 0: the FIR part's rows, 0 when the fused scan cannot run), NM and
 * NS (modes, slow modes; 0 on route 0, NS 0 on route 1), lane_table (route 0: 1 when the
 * cascade has the lane tables of chain_kernel<NR, true>, at most 8 sections), has_instance
 * (1 when the dispatcher finds a compiled kernel for this plan); the rest 0.  0 or an
 * osz_status_t. */
int osz_chain_forward_plan(osz_fir_t fir, osz_sos_t sos, void *stream, int32_t *out, int n);

/*
 * One steady-state step of the FIR -> sosfiltfilt chain: osz_chain_forward of the
 * incoming chunk x -> f on `stream` and, BESIDE it on a stream of the SOS handle's
 * own, osz_sosfiltfilt_chunk of an earlier forward chunk fa (warmed up over fb, or
 * NULL) -> y.  The backward pass starts behind everything queued on `stream` before
 * the call.  f must not alias fa or fb.
 *   flags = 0: `stream` is ordered behind the backward pass when the call returns --
 *     one stream-ordered operation for the caller.
 *   flags = OSZ_CHAIN_DEFER: the backward pass is left running: y, and the right to
 *     overwrite fa / fb, are the caller's only after the NEXT osz_chain_step or an
 *     osz_chain_wait on this handle has been queued on `stream`.  The next step
 *     waits for the pass only if its f overlaps fa or fb (a ring of four forward
 *     buffers never does).
 * Replaces, for a FIR producer feeding sosfiltfilt, core/numerical.py:158-298 +
 * :374-411 of the reference.
 */
#define OSZ_CHAIN_DEFER 1
int osz_chain_step(osz_fir_t fir, osz_sos_t sos, const double *x, int64_t ldx,
                   int64_t n, double *f, int64_t ldf, const double *fa,
                   int64_t ldfa, int64_t na, const double *fb, int64_t ldfb,
                   int64_t nb, double *y, int64_t ldy, int flags, void *stream);

/* `stream` is ordered behind the deferred backward pass of the last osz_chain_step. */
int osz_chain_wait(osz_sos_t sos, void *stream);

/* ---- K1 + K2 + K3 as one multiplication per bin: FIR -> sosfiltfilt ----- */
/*
 * The whole chain the reference builds from oaconvolve (core/numerical.py:158-298) and
 * sosfiltfilt (:338-411), for streams whose chunks are much longer than the cascade's
 * memory (osz_sos_warm_len): there the chunk-local backward pass of the reference equals,
 * to 1e-18, the backward pass over the whole rest of the stream, and FIR, forward and
 * backward cascade are the zero-phase filter H_fir |H_iir|^2 -- one spectrum multiply in
 * the FIR's 4096-point transform plus the cascade's ringing on both sides of each block,
 * put back by mode bursts (csrc/chain_zp.hip).  The forward stream never exists: 8 B read
 * and 8 B written per channel-sample for what SURVEY 8d books at 48.
 *
 * The output stream runs osz_chain_zp_lag() samples behind the input: a block's backward
 * ringing reaches that far into what the previous block has produced.  The two ends of a
 * stream (where the reference's start state sosfilt_zi * x[0] and its last chunk's
 * backward start matter) are the caller's, with the separate kernels: open after the
 * start state has been set on the SOS handle, finish before the last chunks.
 *
 *   osz_chain_zp_lag        samples of delay (a multiple of 256), or -1 when the pair
 *                           of filters does not take this kernel (poles that repeat,
 *                           ringing longer than the transform's guard rows -- twelve rows
 *                           of 256 samples at most --, a partitioned FIR, i.e. one of more
 *                           than 2049 taps)
 *   osz_chain_zp_tolerance  where the bursts are cut, relative to the norm of the composite
 *                           impulse response (0: the default, 1e-15; before osz_chain_zp_lag /
 *                           _open; also the cut of osz_chain_forward's spectral kernels for
 *                           this cascade).  What is cut off scales with the INPUT's magnitude,
 *                           about 0.3 tol max|x|: the default keeps it at float64's own
 *                           rounding on any input; a caller whose streams are zero-mean may
 *                           relax it (1e-12: one burst row less each way, 2 % less time, 6e-13
 *                           of the output scale on such data).
 *   osz_chain_zp_reach      how far a non-finite INPUT sample reaches in the reference's FIR: it works
 *                           in segments of `step` input samples, one FFT each (core/numerical.py:
 *                           202-217, 258-283), so the forward stream is bad from the start of the
 *                           segment that holds the sample -- osz_chain_zp_seal then counts chunks
 *                           from there (0, the default: from the sample itself; the kernels record
 *                           the exact sample)
 *   osz_chain_zp_min_chunk  shortest chunk osz_chain_zp_step takes (two blocks)
 *   osz_chain_zp_open       starts a stream at sample 0: the FIR's overlap tail must be
 *                           zero; the forward cascade starts from the state on the SOS
 *                           handle (osz_sos_set_state*) at stream sample `skip` -- the
 *                           FIR's left cut, which the cascade never sees -- and that state
 *                           is consumed
 *   osz_chain_zp_step       the next n input samples; the n output samples
 *                           [pos - lag, pos + n - lag) of the stream (pos: samples stepped
 *                           before; the first lag outputs of a stream mean nothing) go to
 *                           y0[0, n0) and y[0, n - n0): a caller that cuts the output into
 *                           chunks of its own passes the tail of the previous chunk and
 *                           the head of the current one (n0 = 0: everything to y).
 *                           Non-finite input: the step records where the forward stream
 *                           went bad, every later step writes NaN only, and
 *                           osz_chain_zp_seal settles the chunk it happened in and the one
 *                           before -- outputs are final once sealed
 *   osz_chain_zp_seal       NaN reach of sosfiltfilt: y holds output samples [s0, s0 + n)
 *                           of a stream cut into chunks of cs samples from `origin` on; a
 *                           chunk is NaN as a whole when the forward stream went bad in it
 *                           or in the chunk after it (positions the steps so far have seen)
 *   osz_chain_zp_finish     ends the zero-phase part: the handles' own states (FIR overlap
 *                           tail, forward section states) become those at the end of the
 *                           samples stepped -- osz_fir_push / osz_sos_forward /
 *                           osz_chain_forward continue the forward stream from there --
 *                           and y[0, ny) receives the next ny output samples, for which
 *                           the first m samples of what follows are read (m >= min_chunk,
 *                           ny <= m - min_chunk / 2: the last pair of blocks of those m
 *                           samples is not what the continued stream would have there)
 */
int64_t osz_chain_zp_lag(osz_fir_t fir, osz_sos_t sos);
/* The zero-phase plan of this pair (read-only, as osz_chain_zp_lag: it builds the tables and
 * decides nothing), for tests that check every compiled instance.  Fills out[0 .. n), n >= 8,
 * with: kernel (0 refused, 1 the pair kernel chain_zp_kernel, 2 one block per transform,
 * chain_zpn_kernel), rows (NR or NB), NM, NS (0 for the pair kernel), R, Rf (burst rows
 * backwards / forwards), RM (rows the instance holds: 5, 8 or 12), has_instance (1 when the
 * dispatcher finds a compiled kernel); the rest 0.  0 or an osz_status_t. */
int osz_chain_zp_plan(osz_fir_t fir, osz_sos_t sos, int32_t *out, int n);
int osz_chain_zp_tolerance(osz_fir_t fir, osz_sos_t sos, double tol);
int osz_chain_zp_reach(osz_fir_t fir, osz_sos_t sos, int64_t step);
int64_t osz_chain_zp_min_chunk(osz_fir_t fir, osz_sos_t sos);
int osz_chain_zp_open(osz_fir_t fir, osz_sos_t sos, int64_t skip, void *stream);
int osz_chain_zp_step(osz_fir_t fir, osz_sos_t sos, const double *x, int64_t ldx,
                      int64_t n, double *y0, int64_t ldy0, int64_t n0, double *y,
                      int64_t ldy, void *stream);
int osz_chain_zp_seal(osz_fir_t fir, osz_sos_t sos, double *y, int64_t ldy, int64_t n,
                      int64_t s0, int64_t origin, int64_t cs, void *stream);
int osz_chain_zp_finish(osz_fir_t fir, osz_sos_t sos, const double *x, int64_t ldx,
                        int64_t m, double *y, int64_t ldy, int64_t ny, void *stream);

/* ---- K4: polyphase rational resampler --------------------------------- */
/*
 * Replaces scipy.signal.resample_poly(padded, L, M, window=h) as called at
 * core/numerical.py:610,631 together with the overhang bookkeeping :590-632.
 * Output sample j of the whole stream is
 *    sum_k L*h[k] * xup[j*M + half - k],  half = (ntaps-1)/2
 * The handle carries the input history it still needs.
 */
int osz_poly_create(osz_poly_t *h, const double *taps, int ntaps, int L, int M,
                    int nch);
/* The same with the tap that lines up with an output named (`half` above = centre): what
 * resample_poly does to the window before it filters -- zeros in front (n_pre_pad) and behind
 * (n_post_pad, every phase to one count of taps; scipy/signal/_signaltools.py, resample_poly) --
 * handed in as taps.  The kernels multiply every tap they are given, zero-valued ones included,
 * and no other: a non-finite sample is lost to exactly the outputs SciPy (and so the reference,
 * core/numerical.py:610,631) loses it to.  osz_poly_create(taps, n) = ..._centred(taps, n, (n-1)/2). */
int osz_poly_create_centred(osz_poly_t *h, const double *taps, int ntaps, int centre, int L, int M,
                            int nch);
int osz_poly_destroy(osz_poly_t h);
int osz_poly_reset(osz_poly_t h, void *stream);
/* Checkpoint / resume: [samples consumed, samples produced, input history]
 * as osz_poly_state_size() host doubles.  Synchronous. */
int64_t osz_poly_state_size(osz_poly_t h);
int osz_poly_get_state(osz_poly_t h, double *state, void *stream);
int osz_poly_set_state(osz_poly_t h, const double *state, void *stream);
/* Number of output samples a push of n more input samples will produce
 * (final != 0: the stream ends with this push, total = ceil(N*L/M)). */
int64_t osz_poly_out_count(osz_poly_t h, int64_t n, int final);
/* The plan of this handle (read-only), for tests that check every compiled instance.  Fills
 * out[0 .. n), n >= 9, with: kernel (0 the cache-path poly_kernel, 1 poly_block_kernel), ONE
 * (L == 1), NT (output threads per tile), EG (phase groups), apad (taps per phase stream of the
 * blocked table), se (LDS doubles per phase stream), lds_bytes -- the block kernel's, 0 for the
 * fallback -- then H (samples of history carried) and half (the centre tap); the rest 0.
 * 0 or an osz_status_t. */
int osz_poly_plan(osz_poly_t h, int32_t *out, int n);
int osz_poly_push(osz_poly_t h, const double *x, int64_t ldx, int64_t n,
                  int final, double *y, int64_t ldy, int64_t *n_out,
                  void *stream);

/* ---- K5/K6: segmenter + detrend + window + rFFT (+ power, + average) -- */
/*
 * Replaces _spectra_estimatives' FIFO segmenter (core/numerical.py:799-849),
 * modified_dft (:635-718: scipy.signal.detrend, get_window, np.fft.rfft,
 * scaling) and periodogram (:721-796), and the running segment average of
 * spectra/estimators.py:149-152.
 */
typedef enum {
    OSZ_SPEC_PSD_MEAN = 0,     /* accumulate sum of periodograms (psd)        */
    OSZ_SPEC_PSD_SEGMENTS = 1, /* one (nch, nfreq) f64 periodogram / segment  */
    OSZ_SPEC_DFT_SEGMENTS = 2  /* one (nch, nfreq) c128 modified DFT / segment */
} osz_spec_mode;
enum { OSZ_DETREND_CONSTANT = 0, OSZ_DETREND_LINEAR = 1 };

/* Segments are nwin samples long, `stride` apart, zero-padded to nfft >= nwin
 * (welch/stft: nwin == nfft; periodogram with nfft > samples: :697-699).
 * window: nwin host doubles (scipy.signal.get_window, periodic);
 * scale: sqrt(norm) of core/numerical.py:703-716, computed by the caller. */
int osz_spec_create(osz_spec_t *h, int nwin, int nfft, int stride,
                    const double *window, double scale, int detrend, int mode,
                    int nch);
int osz_spec_destroy(osz_spec_t h);
int osz_spec_reset(osz_spec_t h, void *stream);
/* Number of complete segments a push of n more samples will emit. */
int64_t osz_spec_seg_count(osz_spec_t h, int64_t n);
/* Consumes x (nch, n).  SEGMENTS modes: writes nseg estimates to out laid out
 * (nseg, nch, nfreq) contiguous (f64 or interleaved c128).  PSD_MEAN: out is
 * ignored and the handle's accumulator advances. */
int osz_spec_push(osz_spec_t h, const double *x, int64_t ldx, int64_t n,
                  void *out, int64_t *nseg, void *stream);
/*
 * What the handle's most recent osz_spec_push launched, in launch order: each launch
 * site of the engine notes what it launches, as it launches it (the small kernels
 * that build the head buffer, fold partial sums and move the carry are not noted).
 * Read-only.  A record is OSZ_SPEC_LAUNCH_FIELDS int64 values:
 *   [0] family    OSZ_SPECK_*
 *   [1] size      the instance's size parameter: N (cube, fft8), NT threads (mix,
 *                 split), the convolution length M (blue); staged: nfft
 *   [2] mode      osz_spec_mode
 *   [3] linear    1 / 0: OSZ_DETREND_LINEAR or _CONSTANT
 *   [4] half      cube, fft8: 1 / 0 the HALF instance (a pair shares a half); mix,
 *                 split: the half-carry of the trend sums; -1: no such parameter
 *   [5] nseg      segments of this launch (staged: of this batch)
 *   [6] R         segments (mix, split) or segment pairs (cube, fft8, blue) per run,
 *                 as the launch site planned it; staged: segments per batch
 *   [7] nruns     runs per channel (staged: 1)
 *   [8] head      1: the segments that begin in the carry, out of the head buffer;
 *                 0: those inside the chunk; -1: one launch reads the carry itself
 *   [9] npass     mix, split: passes of the radix plan; else 0
 *   [10] R0, [11] S0   split: nfft / 2 = R0 S0; else 0
 *   [12 ...]      radix[0 .. npass), zeros behind
 * Up to `cap` records go to `out` (host, cap * OSZ_SPEC_LAUNCH_FIELDS values); *count
 * is the number of launches noted (at most OSZ_SPEC_LAUNCH_RECORDS are kept).
 */
#define OSZ_SPEC_LAUNCH_FIELDS 26
#define OSZ_SPEC_LAUNCH_RECORDS 8
enum {
    OSZ_SPECK_CUBE = 0,    /* spec_cube_kernel                       */
    OSZ_SPECK_FFT8 = 1,    /* spec8_kernel                           */
    OSZ_SPECK_MIX = 2,     /* specmix_kernel                         */
    OSZ_SPECK_SPLIT = 3,   /* specsplit_kernel                       */
    OSZ_SPECK_BLUE = 4,    /* spec_blue_kernel                       */
    OSZ_SPECK_STAGED = 5   /* spec_prep_kernel, rocFFT, spec_post_kernel */
};
int osz_spec_last_launches(osz_spec_t h, int64_t *out, int cap, int *count);
/* PSD_MEAN: raw sum of periodograms (nch, nfreq) f64 on the device and the
 * segment count so far -- a multi-GPU time split reduces these (RCCL) before
 * dividing.  The pointer stays owned by the handle. */
int osz_spec_sum(osz_spec_t h, double **dsum, int64_t *count);
/* PSD_MEAN: copies the raw sum into a caller-owned device buffer (nch, nfreq),
 * e.g. a tensor handed to an RCCL all-reduce. Asynchronous on `stream`. */
int osz_spec_export_sum(osz_spec_t h, double *dst, int64_t *count, void *stream);
/* PSD_MEAN: mean = sum / count into host array (nch, nfreq). Synchronous. */
int osz_spec_mean(osz_spec_t h, double *mean, int64_t *count, void *stream);

/* PSD_MEAN: mean = sum / count into a caller-owned DEVICE buffer (nch, nfreq):
 * the estimate never leaves HBM.  Asynchronous on `stream`. */
int osz_spec_mean_device(osz_spec_t h, double *dmean, int64_t *count, void *stream);
/* Checkpoint / resume: [carried samples, segment count, FIFO remainder
 * (core/numerical.py:821), periodogram sum] as osz_spec_state_size() host
 * doubles.  Synchronous. */
int64_t osz_spec_state_size(osz_spec_t h);
int osz_spec_get_state(osz_spec_t h, double *state, void *stream);
int osz_spec_set_state(osz_spec_t h, const double *state, void *stream);

/* ---- the one collective: Welch segment average over a time split ------ */
/*
 * The reference averages the periodograms of the whole stream with a running
 * mean (spectra/estimators.py:149-152).  When the stream of a channel block is
 * split in time across GPUs (one process per GPU), each rank's PSD_MEAN handle
 * holds the sum over its own segments; osz_welch_reduce all-reduces (sum) the
 * (nch, nfreq) accumulator and the segment count over the ranks of an RCCL
 * communicator, in place: afterwards osz_spec_mean / _mean_device /
 * _export_sum on ANY rank give the average over the whole stream.
 * comm is an ncclComm_t (void*) of the RCCL instance this library binds at run
 * time: the one already mapped in the process (a PyTorch host), else
 * /opt/rocm/lib/librccl.so.1.  A host without PyTorch creates the
 * communicator through the three helpers below; the 128-byte unique id
 * travels from rank 0 to the others by the host's own means (file, socket).
 * osz_welch_reduce synchronises `stream` (the count comes back to the host).
 */
#define OSZ_RCCL_ID_BYTES 128
int osz_rccl_bind(const char *librccl_path /* NULL: default search */);
int osz_rccl_unique_id(char *id128);
int osz_rccl_comm_create(void **comm, int nranks, int rank, const char *id128);
int osz_rccl_comm_destroy(void *comm);
int osz_rccl_comm_size(void *comm, int *nranks);
int osz_welch_reduce(osz_spec_t h, void *comm, void *stream);

/* ---- host side of host-fed streams -------------------------------------- */
/* dst[r][0, row_bytes) = src[r][0, row_bytes), r < rows; rows dst_pitch / src_pitch bytes
 * apart, host memory both: packs a chunk of a host ndarray -- a column range of a C-ordered
 * array, what the reference's ArrayProducer slices (core/producer.py:289-295) -- into a
 * pinned staging buffer over a few persistent threads; returns when the rows are in place. */
int osz_host_copy2d(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch,
                    int64_t rows, int64_t row_bytes);

/* ---- K7: mask compaction ---------------------------------------------- */
/* y[c, j] = x[c, idx[j]], j < nidx: np.take(arr, np.flatnonzero(mask), axis)
 * of MaskedProducer.__iter__ (core/producer.py:432). idx: device int64. */
int osz_take(const double *x, int64_t ldx, int nch, const int64_t *idx,
             int64_t nidx, double *y, int64_t ldy, void *stream);

/* ---- producer-level arithmetic on device chunks -- */
/*
 * Streaming per-channel moments: replaces the chunk loops of protools.mean /
 * protools.std (core/protools.py:500-545, :547-592).  push folds one chunk
 * x (nch, n): per channel the sum, the sum of squares and the count of its
 * samples (NaNs skipped when ignore_nan, numpy.nanmean; deterministic order),
 * then A += n * sum/count, B += n * sumsq/count, L += n -- the reference
 * weights every chunk's (nan)mean by the chunk length.  finish writes
 * mean = A/L and std = sqrt(B/L - mean^2) (:592) to device arrays (nch);
 * either may be NULL.
 */
typedef struct osz_moments_s *osz_moments_t;
int osz_moments_create(osz_moments_t *h, int nch);
int osz_moments_destroy(osz_moments_t h);
int osz_moments_reset(osz_moments_t h, void *stream);
int osz_moments_push(osz_moments_t h, const double *x, int64_t ldx, int64_t n,
                     int ignore_nan, void *stream);
int osz_moments_finish(osz_moments_t h, double *dmean, double *dstd, void *stream);

/* Mean / standard deviation along the FIRST axis of a (nred, ncols) matrix
 * (numpy.(nan)mean, numpy.(nan)std per column): what protools.mean / std do
 * chunk by chunk when the reduced axis is not the production axis
 * (core/protools.py:538-545, :586-592).  Device outputs (ncols); either NULL. */
int osz_col_moments(const double *x, int64_t ldx, int nred, int64_t ncols, int ignore_nan,
                    double *dmean, double *dstd, void *stream);

/* Elementwise y = x (op) operand with NumPy-style broadcasting reduced to the
 * (channels, samples) layout: protools.add / multiply / multiply_along_axis
 * (core/protools.py:72-180, :334-384), standardize's (x - mean) / std
 * (:660-671) and power_norm's division (spectra/metrics.py:141).  a (and b
 * for STANDARDIZE) are DEVICE arrays: one value, one per channel (row), one
 * per sample (column), or a full (nch, n) matrix with pitch ldab. */
enum { OSZ_EW_ADD = 0, OSZ_EW_MUL = 1, OSZ_EW_DIV = 2, OSZ_EW_STANDARDIZE = 3 };
enum { OSZ_BCAST_SCALAR = 0, OSZ_BCAST_ROW = 1, OSZ_BCAST_COL = 2, OSZ_BCAST_FULL = 3 };
int osz_ew(int op, const double *x, int64_t ldx, int nch, int64_t n, const double *a,
           const double *b, int kind, int64_t ldab, double *y, int64_t ldy, void *stream);

/* z = re + i im (interleaved c128, pitch in complex elements): the analytic
 * signal x + i H(x) of experimental/coupling/transforms.py:186-192. */
int osz_complex_join(const double *re, int64_t ldre, const double *im, int64_t ldim,
                     int nch, int64_t n, double *z, int64_t ldz, void *stream);
/* mag = |z| (numpy.abs), phase = numpy.angle(z) mapped to [0, 2 pi)
 * (transforms.py:75-107); either output may be NULL. */
int osz_magphase(const double *z, int64_t ldz, int nch, int64_t n, double *mag,
                 double *phase, int64_t ldo, void *stream);
/* out[c] = scipy.integrate.simpson(p[c, a : a + m], dx = dx): the band power
 * of spectra/metrics.py:80-87 on the (nch, nfreq) device estimate. */
int osz_simpson(const double *p, int64_t ldp, int nch, int64_t a, int64_t m, double dx,
                double *out, void *stream);

/* ---- phase-locked power (experimental/coupling/estimators.py) -------- */
/*
 * PhaseLock.index (reference estimators.py:172-177): out[0, *count) = the
 * positions i < n, in ascending order, of the 1-D complex chunk z (interleaved
 * c128, device) whose phase -- numpy.angle mapped to [0, 2 pi), computed as
 * osz_magphase computes it -- satisfies lo < phase < hi.  out: device int64 of
 * capacity n; work: device int64 scratch of 2049 elements; *count is written
 * to HOST memory (the call synchronises `stream`).
 */
int osz_phase_index(const double *z, int64_t n, double lo, double hi, int64_t *work,
                    int64_t *out, int64_t *count, void *stream);
/*
 * PhaseLock._avg (estimators.py:200-230) for the real index set and nsur
 * shifted copies of it in one call, on one chunk: amp (L), device f64, the
 * Hilbert amplitudes of the chunk; idx (nidx), device int64, the chunk's phase
 * indices in ascending order.  Set 0 is idx itself; set s in 1..nsur is
 * (idx + shifts[s - 1]) mod max_shift.  With h = ceil(W/2), a position q of a
 * set contributes iff h <= q and q + floor(W/2) <= L, and then
 *   sums[s, k] += sum over those q of amp[q - h + k]^2   (k < W, pitch ldsums)
 *   counts[s]  += their number                           (device int64)
 * sums and counts are accumulators the caller zeroes once and carries across
 * the chunks of a signal.  Fixed summation order, no atomics on sums: two runs
 * give the same bits.
 */
int osz_lock_accumulate(const double *amp, int64_t L, const int64_t *idx, int64_t nidx,
                        const int64_t *shifts, int nsur, int64_t max_shift, int64_t W,
                        double *sums, int64_t ldsums, int64_t *counts, void *stream);

/* ---- phase-amplitude comodulogram (experimental/coupling/estimators.py ModulationIndex) -- */
/*
 * z: `rows` rows of n interleaved c128 samples, pitch ldz in complex elements (device).
 * bins[r, i] (device uint8, pitch ldb) = min(nbins - 1, floor(phase * nbins / (2 pi))) with the
 * phase in [0, 2 pi) computed as osz_magphase computes it; a NaN phase gives 255: the sample
 * belongs to no bin.  2 <= nbins <= 64.
 */
int osz_phase_bins(const double *z, int rows, int64_t n, int64_t ldz, int nbins, uint8_t *bins,
                   int64_t ldb, void *stream);
/*
 * One chunk of length L of the Tort et al. (2010) amplitude-by-phase sums, for the real pairing
 * (set 0) and nsur time-shifted copies of the amplitudes (set s, shifted by sigma_s =
 * shifts[s - 1] mod L; sigma_0 = 0), all (p, a, s) in one launch.  bins: (np, L) uint8 of
 * osz_phase_bins, pitch ldb; amp: (na, L) f64, pitch lda; shifts: nsur int64 (all device).
 *   sums[p, a, s, b] += sum over i with bins[p, i] = b of amp[a, (i + sigma_s) mod L]
 *   counts[p, b]     += #{i : bins[p, i] = b}
 * sums: contiguous (np, na, nsur + 1, nbins) f64, counts: (np, nbins) int64, accumulators the
 * caller zeroes once and carries across the chunks of a signal.  Codes >= nbins (255) are
 * skipped; a non-finite amplitude propagates into the sums it falls into; L = 0 is a no-op.
 * Every sum is owned by one wave and added in a fixed order, no atomics on sums: two runs give
 * the same bits.
 */
int osz_pac_accumulate(const uint8_t *bins, int np, int64_t ldb, const double *amp, int na,
                       int64_t lda, int64_t L, const int64_t *shifts, int nsur, int nbins,
                       double *sums, int64_t *counts, void *stream);
/*
 * The modulation index of every (p, a, set): with m_b = sums / counts and P_b = m_b / sum m,
 *   mi[p, a, s] = 1 + sum_b P_b ln P_b / ln nbins        (0 ln 0 = 0)
 *   dist[p, a, :] = P of set 0
 * mi: (np, na, nsets) f64, dist: (np, na, nbins) f64 (device).  A phase row with an empty bin
 * gives NaN for that whole row.  The index is summed as
 * sum_b (P_b ln(nbins P_b) - P_b + 1 / nbins) / ln nbins, the same number as sum P = 1, with
 * terms that are all >= 0 and second order in the rounding of sum P, so that an index of 1e-4
 * keeps its digits.
 */
int osz_pac_finish(const double *sums, const int64_t *counts, int np, int na, int nsets, int nbins,
                   double *mi, double *dist, void *stream);

/* ---- Welch cross-spectra over all channel pairs (spectra/estimators.py csd, coherence) -- */
/*
 * X: the (nseg, nch, nfreq) interleaved c128 block an OSZ_SPEC_DFT_SEGMENTS push wrote
 * (device); acc: (nch, nch, nfreq) c128 raw sums (device), owned and zeroed by the caller and
 * carried across the pushes of a stream:
 *   acc[i, j, f] += sum over s of conj(X[s, i, f]) X[s, j, f]        for i <= j
 * summed segment by segment from the stored value, so the sums do not depend on where the
 * stream is cut; no atomics: two runs give the same bits.  Entries with i > j are not touched.
 */
int osz_cross_accumulate(const void *X, int64_t nseg, int nch, int nfreq, void *acc, void *stream);
typedef enum {
    OSZ_CROSS_SPECTRUM = 0,    /* out: (nch, nch, nfreq) c128                 */
    OSZ_CROSS_COHERENCE = 1    /* out: (nch, nch, nfreq) f64                  */
} osz_cross_mode;
/*
 * Spectrum: out[i, j] = acc[i, j] / count, every bin but DC (and the last one when
 * nfft_is_even) doubled; out[j, i] = conj(out[i, j]); the imaginary part of out[i, i] is 0.
 * `out` may be `acc`.  Coherence: out[i, j] = out[j, i] = |acc[i, j]|^2 / (Re acc[i, i] Re acc[j, j]).
 */
int osz_cross_finish(const void *acc, int64_t count, int nch, int nfreq, int nfft_is_even, int mode,
                     void *out, void *stream);

/* ---- phase-based connectivity over all channel pairs (spectra/estimators.py phase_connectivity) -- */
/*
 * X as for osz_cross_accumulate; lag: four (nch, nch, nfreq) f64 planes (device), owned and
 * zeroed by the caller and carried across the pushes of a stream.  With
 * d = Im(conj(X[s, i, f]) X[s, j, f]) = fma(Re X_i, Im X_j, -(Im X_i Re X_j)), for i <= j:
 *   lag[0, i, j, f] += sum over s of d          lag[1, i, j, f] += sum over s of |d|
 *   lag[2, i, j, f] += sum over s of d^2        lag[3, i, j, f] += sum over s of sign(d)
 * sign(+-0) = 0 and sign(NaN) = NaN.  Summed segment by segment from the stored value, no
 * atomics: the sums do not depend on where the stream is cut and two runs give the same bits.
 * Entries with i > j are not touched.
 */
int osz_lag_accumulate(const void *X, int64_t nseg, int nch, int nfreq, double *lag, void *stream);
/*
 * X[k] <- X[k] / |X[k]| for the n interleaved c128 values at X (device), in place; 0 gives NaN.
 * osz_cross_accumulate on the result adds z / |z| of every pair, z = conj(X_i) X_j.
 */
int osz_unit_phasors(void *X, int64_t n, void *stream);
typedef enum {
    OSZ_PHASE_IMCOH = 0,   /* Im acc[i, j] / sqrt(Re acc[i, i] Re acc[j, j])      reads acc  */
    OSZ_PHASE_PLV = 1,     /* |accn[i, j]| / count                                 reads accn */
    OSZ_PHASE_PLI = 2,     /* |lag[3]| / count                                     reads lag  */
    OSZ_PHASE_WPLI = 3,    /* |lag[0]| / lag[1]                                    reads lag  */
    OSZ_PHASE_DWPLI = 4    /* (lag[0]^2 - lag[2]) / (lag[1]^2 - lag[2])            reads lag  */
} osz_phase_mode;
/*
 * out (nch, nch, nfreq) f64 from the sums of `count` segments: acc the sums of
 * osz_cross_accumulate, accn those of the spectra osz_unit_phasors normalised, lag those of
 * osz_lag_accumulate; the ones `mode` does not read may be null.  out[j, i] = out[i, j], for
 * imcoh -out[i, j].  In this order: where the diagonal sums of channel i or j are NaN the entry
 * is NaN; the diagonal is 1.0 for plv and 0.0 for the others; at bin 0, and at the last bin
 * when nfft_is_even, every measure but plv is 0.0 (and its mirror 0.0); elsewhere 0 / 0 is NaN.
 */
int osz_phase_finish(int mode, const void *acc, const void *accn, const double *lag, int64_t count,
                     int nch, int nfreq, int nfft_is_even, double *out, void *stream);

/* ---- delete-one jackknife over the Welch segments (spectra/estimators.py jackknife) ------ */
typedef enum {             /* theta without segment s, from the totals minus its contribution  */
    OSZ_JACK_COHERENCE = 0, /* |A - z|^2 / ((P_i - p_i)(P_j - p_j))               reads acc  */
    OSZ_JACK_IMCOH = 1,     /* Im(A - z) / sqrt((P_i - p_i)(P_j - p_j))           reads acc  */
    OSZ_JACK_PLV = 2,       /* |U - u| / (count - 1)                              reads accn */
    OSZ_JACK_PLI = 3,       /* |G - sign d| / (count - 1)                         reads lag  */
    OSZ_JACK_WPLI = 4,      /* |D - d| / (B - |d|)                                reads lag  */
    OSZ_JACK_DWPLI = 5      /* ((D - d)^2 - (Q - d^2)) / ((B - |d|)^2 - (Q - d^2)) reads lag  */
} osz_jack_mode;
/*
 * The second pass.  X: (nseg, nch, nfreq) c128 segment spectra (device) as for
 * osz_cross_accumulate -- for OSZ_JACK_PLV the spectra osz_unit_phasors normalised; acc / accn /
 * lag: the FINISHED totals of all `count` >= 2 segments of the stream (osz_cross_accumulate of the
 * spectra, of the unit phasors, osz_lag_accumulate), the ones `mode` does not read may be null.
 * With z = conj(X_i) X_j of segment s, d = Im z (the expression of osz_lag_accumulate),
 * p_i = |X_i|^2, A = acc[i, j], P_i = Re acc[i, i], U = accn[i, j], (D, B, Q, G) = lag[0 .. 3]:
 * theta_(s) as the table says, theta the same expression with nothing taken away, and for i <= j
 *   dev2[0, i, j, f] += sum over s of (theta_(s) - theta)
 *   dev2[1, i, j, f] += sum over s of (theta_(s) - theta)^2
 * dev2: two (nch, nch, nfreq) f64 planes (device), owned and zeroed by the caller and carried
 * across the pushes; one such array per mode.  Summed segment by segment from the stored value,
 * no atomics: the sums do not depend on where the stream is cut and two runs give the same bits.
 * Entries with i > j are not touched.  A zero denominator gives inf or NaN, as IEEE does; with
 * count = 2 dwpli's theta_(s) is 0 / 0 by definition and is written as NaN.
 */
int osz_jackknife_accumulate(int mode, const void *X, int64_t nseg, int nch, int nfreq, const void *acc,
                             const void *accn, const double *lag, int64_t count, double *dev2, void *stream);
/*
 * out (nch, nch, nfreq) f64, out[j, i] = out[i, j] =
 *   sqrt((count - 1) / count v),  v = dev2[1] - dev2[0]^2 / count         (a NaN stays one)
 * with v taken as 0 where it does not exceed 4 count 2^-53 dev2[1], the rounding the subtraction
 * itself may carry (which covers v < 0): the deviations are then equal to within rounding -- with
 * two segments, coherence, plv, pli and wpli of the one segment left are 1 whichever is left out.
 * In this order: where the diagonal totals of channel i or j (of the array `mode` reads) are NaN
 * the entry is NaN; the diagonal is 0.0; at bin 0, and at the last bin when nfft_is_even, every
 * measure but plv is 0.0.
 */
int osz_jackknife_finish(int mode, const double *dev2, const void *acc, const void *accn, const double *lag,
                         int64_t count, int nch, int nfreq, int nfft_is_even, double *out, void *stream);

/* ---- time-domain connectivity of analytic signals over all channel pairs ------------------ */
/* (experimental/coupling/connectivity.py analytic_connectivity; csrc/pairtime.hip, K13) */
#define OSZ_ANALYTIC_BLOCK 4096   /* samples per time block, counted from the stream's first sample */
typedef enum {                    /* sum groups, a bit each; their planes follow in this order      */
    OSZ_ANALYTIC_AMP = 1,         /* 1 plane:  sum a_i a_j                                           */
    OSZ_ANALYTIC_ORTH = 2,        /* 5 planes: sum m, m / a_i, m / a_j, (m / a_i)^2, (m / a_j)^2     */
    OSZ_ANALYTIC_LOCK = 4,        /* 2 planes: Re, Im of sum conj(u_i) u_j                           */
    OSZ_ANALYTIC_LAG = 8,         /* 2 planes: sum d, sum m                                          */
    OSZ_ANALYTIC_ALL = 15
} osz_analytic_group;
typedef enum {
    OSZ_ANALYTIC_AEC = 0,         /* Pearson r of (a_i, a_j)                             reads AMP  */
    OSZ_ANALYTIC_OAEC = 1,        /* (r(a_i, m / a_i) + r(a_j, m / a_j)) / 2             reads ORTH */
    OSZ_ANALYTIC_PLV = 2,         /* |sum conj(u_i) u_j| / count                         reads LOCK */
    OSZ_ANALYTIC_CIPLV = 3,       /* |Im s| / sqrt(1 - (Re s)^2), s = sum / count        reads LOCK */
    OSZ_ANALYTIC_WPLI = 4         /* |sum d| / sum m                                     reads LAG  */
} osz_analytic_mode;
/*
 * The doubles of work space one push of n samples of nch channels with these groups needs
 * (the staged planes, the block partials); -1 for arguments out of range.
 */
int64_t osz_analytic_work(int nch, int64_t n, int groups);
/*
 * z: nch rows of n c128 samples (device, interleaved re/im), row pitch ld samples.  With
 * a = |z|, u = z / a, d = Im(conj(z_i) z_j) = fma(x_i, y_j, -(y_i x_j)) and m = |d|, adds for i <= j
 * the sums over the n samples that `groups` names to sums -- (planes, nch, nch) f64 (device), the
 * planes of the groups present in the order above, owned and zeroed by the caller -- and sum a,
 * sum a^2 and sum |u|^2 of every channel to chan (3, nch).  Entries of sums with i > j are not
 * touched.  The samples are summed in blocks of OSZ_ANALYTIC_BLOCK in a fixed order and the
 * blocks' partials added to the stored sums in block order, no atomics: when every push but a
 * stream's last holds a whole number of blocks, the sums do not depend on where the stream is
 * cut and two runs give the same bits.  work: at least work_len >= the doubles the work-space
 * query above asks for (device), contents undefined afterwards.
 */
int osz_analytic_accumulate(const void *z, int64_t ld, int nch, int64_t n, int groups, double *sums,
                            double *chan, double *work, int64_t work_len, void *stream);
/*
 * out (nch, nch) f64 from the sums of `count` samples; out[j, i] = out[i, j].  In this order:
 * where one of the sums in chan of channel i or j is not finite the entry is NaN; the diagonal is
 * 1.0 for aec and plv and 0.0 for the others; elsewhere the definition, 0 / 0 left as NaN.
 */
int osz_analytic_finish(int mode, const double *sums, int groups, const double *chan, int64_t count,
                        int nch, double *out, void *stream);

/* ---- Welch bispectrum and bicoherence per channel (spectra/estimators.py bispectrum) ----- */
/* (csrc/bispec.hip, K14) */
typedef enum {
    OSZ_BISPEC_SPECTRUM = 0,   /* out: (nch, nb, nb) c128   sum T / count                         */
    OSZ_BISPEC_KIM = 1,        /* out: (nch, nb, nb) f64    |sum T|^2 / (sum |X1 X2|^2 sum |X3|^2) */
    OSZ_BISPEC_HAGIHIRA = 2    /* out: (nch, nb, nb) f64    |sum T| / sum |T|                      */
} osz_bispec_mode;
/*
 * The doubles of work space one push of nseg segments needs (the plane |X|); -1 for arguments
 * out of range (nch * nfreq must stay below 2^27).
 */
int64_t osz_bispec_work(int64_t nseg, int nch, int nfreq);
/*
 * X: the (nseg, nch, nfreq) interleaved c128 block an OSZ_SPEC_DFT_SEGMENTS push wrote (device).
 * The band is the nb bins k_lo .. k_lo + nb - 1 (k_lo + nb <= nfreq).  With k1 = k_lo + a,
 * k2 = k_lo + b, X1 = X[s, c, k1], X2 = X[s, c, k2], X3 = X[s, c, k1 + k2] and T = X1 X2 conj(X3),
 * for b <= a and k1 + k2 <= nfreq - 1 (the third factor is read from the whole spectrum):
 *   sums[0, c, a, b] += sum over s of Re T         sums[1, c, a, b] += sum over s of Im T
 *   sums[2, c, a, b] += sum over s of |X1 X2|^2    sums[3, c, a, b] += sum over s of |X1| |X2| |X3|
 * and for every bin  power[c, k] += sum over s of |X[s, c, k]|^2.
 * sums: (4, nch, nb, nb) f64, power: (nch, nfreq) f64 (device), owned and zeroed by the caller and
 * carried across the pushes of a stream; entries of sums with b > a or outside the domain are
 * not touched.  Summed segment by segment from the stored value, fused multiply-adds in a fixed
 * order, no atomics: the sums do not depend on where the stream is cut and two runs give the
 * same bits.  work: at least work_len >= the doubles the work-space query above asks for (device),
 * contents undefined afterwards.
 */
int osz_bispec_accumulate(const void *X, int64_t nseg, int nch, int nfreq, int k_lo, int nb, double *sums,
                          double *power, double *work, int64_t work_len, void *stream);
/*
 * out (nch, nb, nb), c128 for OSZ_BISPEC_SPECTRUM and f64 otherwise, from the sums of `count`
 * segments as the table of modes says; out[c, b, a] = out[c, a, b] bit for bit.  Entries with
 * k1 + k2 > nfreq - 1 are NaN (both parts of a c128).  A zero denominator gives what IEEE gives.
 */
int osz_bispec_finish(int mode, const double *sums, const double *power, int64_t count, int nch, int nfreq,
                      int k_lo, int nb, void *out, void *stream);

/* ---- time-resolved per-channel features (features/windowed.py window_features) ------------ */
/* (csrc/windowfeat.hip, K15) */
#define OSZ_WF_LONG 4096          /* windows of at least this many samples take a workgroup each, shorter ones a wave */
#define OSZ_WF_LONGEST 134217728      /* the longest window, 2^27 samples: a window is addressed with 32-bit byte offsets  */
typedef enum {                    /* dx_t = x_{t+1} - x_t, ddx_t = dx_{t+1} - dx_t, m_k the k-th central moment / W  */
    OSZ_WF_MEAN = 0,
    OSZ_WF_VAR = 1,               /* m_2                                                                 */
    OSZ_WF_RMS = 2,               /* sqrt(mean x^2)                                                      */
    OSZ_WF_SKEW = 3,              /* m_3 / m_2^1.5                                                       */
    OSZ_WF_KURTOSIS = 4,          /* m_4 / m_2^2 (Pearson, not excess)                                   */
    OSZ_WF_MIN = 5,
    OSZ_WF_MAX = 6,
    OSZ_WF_PTP = 7,               /* max - min                                                           */
    OSZ_WF_LINE_LENGTH = 8,       /* sum |dx_t|                                                          */
    OSZ_WF_ZERO_CROSSINGS = 9,    /* the number of t with (x_t < 0) != (x_{t+1} < 0)                     */
    OSZ_WF_MOBILITY = 10,         /* sqrt(var(dx) / var(x))                                              */
    OSZ_WF_COMPLEXITY = 11,       /* sqrt(var(ddx) / var(dx)) / mobility                                 */
    OSZ_WF_TEAGER = 12,           /* mean over t = 1 .. W - 2 of x_t^2 - x_{t-1} x_{t+1}                 */
    OSZ_WF_COUNT = 13
} osz_window_feature;
/*
 * The windows of winsize samples, step apart, that n samples hold: 0 for n < winsize, else
 * (n - winsize) / step + 1; -1 for n < 0, winsize < 4 or step < 1.  Touches no device.
 */
int64_t osz_window_count(int64_t n, int64_t winsize, int64_t step);
/*
 * x: nch rows of n f64 samples (device), row pitch `pitch` samples.  Window k of a row covers its
 * samples k step .. k step + winsize - 1; for the nwin windows the n samples hold and every
 * feature f whose bit 1 << f is set in mask (an osz_window_feature), in the order of the enum,
 *   out[p * plane_pitch + c * row_pitch + win0 + k] = feature of window k of row c      (f64, device)
 * with p the feature's rank among those present: successive pushes of a stream fill one result.
 * Nothing else of out is touched.  A window that holds a NaN gives NaN in every feature; +-inf and
 * a zero variance give what IEEE arithmetic gives from the definitions.  A window's bits depend
 * on winsize and its own samples only -- not on step, the window's index, nch, mask or how the
 * stream is cut into pushes: the partition of a window over lanes and the order of the fold are
 * functions of winsize alone, and nothing is atomic.  winsize <= OSZ_WF_LONGEST.  One launch, no work space.
 */
int osz_window_features(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step,
                        int mask, double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0,
                        void *stream);

/* ---- sample and permutation entropy per window (features/entropy.py window_entropy) -------- */
/* (csrc/windowent.hip, K16) */
#define OSZ_WE_LONGEST 4096       /* the longest window: it is held in LDS, 32 KB                             */
#define OSZ_WE_WIDE 512           /* windows of at least this many samples take 256 threads, shorter ones 64  */
typedef enum {
    OSZ_WE_SAMPLE = 0,            /* -ln(A / B), Richman & Moorman 2000                                   */
    OSZ_WE_SAMPLE_A = 1,          /* A: template pairs i < j that match over m + 1 samples, as f64, exact */
    OSZ_WE_SAMPLE_B = 2,          /* B: the pairs that match over m samples                               */
    OSZ_WE_PERMUTATION = 3,       /* -sum p log2 p over the order! rank patterns, Bandt & Pompe 2002      */
    OSZ_WE_COUNT = 4
} osz_window_entropy_measure;
enum { OSZ_WE_TOL_STD = 0, OSZ_WE_TOL_ABSOLUTE = 1 };
/*
 * x, the windows, mask (bit 1 << e of an osz_window_entropy_measure) and out are those of
 * osz_window_features: out[p * plane_pitch + c * row_pitch + win0 + k], p the measure's rank among
 * those present; nothing else of out is touched.  With x_0 .. x_{W-1} one window, W = winsize:
 *   sample       the templates are i = 0 .. W - m - 1 for both lengths; B counts the pairs i < j
 *                with max_{k < m} |x_{i+k} - x_{j+k}| <= rho, A the same with k <= m (<= in f64);
 *                rho = r std(window) (divisor W, from sums about the window's first sample) for
 *                OSZ_WE_TOL_STD, rho = r for OSZ_WE_TOL_ABSOLUTE.  A = 0 < B gives +inf, B = 0 NaN.
 *   permutation  the vectors (x_t, x_{t+delay}, .., x_{t+(order-1) delay}), t = 0 .. W - 1 -
 *                (order - 1) delay; the rank of element k is #{l : x_l < x_k} + #{l < k : x_l = x_k};
 *                p the histogram of the order! patterns over the number of vectors; the result is
 *                -sum p log2 p, over log2 order! when normalize is not 0.
 * 4 <= winsize <= OSZ_WE_LONGEST, 1 <= m <= 8, r finite and >= 0, 2 <= order <= 6, delay >= 1;
 * winsize >= m + 2 when a sample measure is asked, winsize > (order - 1) delay when permutation is.
 * A window that holds a NaN or +-inf is NaN in every measure.  A window's bits depend on winsize,
 * the parameters and its own samples only: the counts are integers, the sums for the std and the
 * fold of the histogram run in an order that is a function of winsize alone, and no
 * floating-point operation is atomic.  One launch, one workgroup per window, no work space.
 */
int osz_window_entropy(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step,
                       int mask, int m, double r, int tolerance, int order, int64_t delay, int normalize,
                       double *out, int64_t plane_pitch, int64_t row_pitch, int64_t win0, void *stream);

/* ---- median, MAD and quantiles per window (features/quantiles.py window_quantiles) -------- */
/* (csrc/windowquant.hip, K17) */
#define OSZ_WQ_LONGEST 4096       /* the longest window: it is sorted on chip, 16 keys in each of 256 threads     */
#define OSZ_WQ_QMOST 16           /* the most quantiles of one call: they travel in the kernel's arguments        */
#define OSZ_WQ_NARROWEST 64       /* the least padded width; one kernel instance per power of two from here to    */
                                  /* OSZ_WQ_LONGEST: a window is padded to the first of them that holds it         */
#define OSZ_WQ_WAVE 512           /* windows of up to this many samples are sorted by one wave, longer ones by 256 threads */
typedef enum {
    OSZ_WQ_MEDIAN = 0,            /* the mean of the two middle samples of the sorted window (of the one) */
    OSZ_WQ_MAD = 1,               /* the median of |x_t - median|, unscaled                               */
    OSZ_WQ_QUANTILE = 2,          /* Hyndman & Fan type 7 for each of the nq values of q                  */
    OSZ_WQ_COUNT = 3
} osz_window_quantiles_measure;
/*
 * x, the windows, mask (bit 1 << e of an osz_window_quantiles_measure) and out are those of
 * osz_window_features: out[p * plane_pitch + c * row_pitch + win0 + k]; the planes are, of those
 * present in mask, median, mad and then the nq quantiles in the order of q; nothing else of out is
 * touched.  q: nq values in [0, 1] in HOST memory (read only when OSZ_WQ_QUANTILE is asked, 1 <= nq
 * <= OSZ_WQ_QMOST; any order, duplicates give duplicate planes).  With s_0 <= .. <= s_{W-1} the
 * samples of one window, W = winsize, in ascending total order (-0.0 before +0.0: the order of
 * the bits):
 *   median    (s_{(W-1)/2} + s_{W/2}) / 2: one addition, one division.
 *   quantile  h = p (W - 1), lo = floor(h), g = h - lo, hi = min(lo + 1, W - 1) -- computed here,
 *             on the host, once; a = s_lo, b = s_hi; a where a == b, else with d = b - a
 *             a + d g for g < 0.5 and b - d (1 - g) otherwise (numpy's linear method).
 *   mad       the median, by the rule above, of |x_t - median| over the window.  NaN where the
 *             median is not finite (inf - inf is among the deviations).
 * Every operation is one IEEE operation, none contracted.  4 <= winsize <= OSZ_WQ_LONGEST.  A
 * window that holds a NaN is NaN in every measure; +-inf are ordinary values of the sort.  A
 * window's bits depend on winsize, q and its own samples only: the sort compares integer keys,
 * and nothing is atomic.  One launch, one workgroup per window, no work space.
 */
int osz_window_quantiles(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step,
                         int mask, const double *q, int nq, double *out, int64_t plane_pitch, int64_t row_pitch,
                         int64_t win0, void *stream);

/* ---- spectral features per window (features/spectral.py window_spectral) ------------------ */
/* (csrc/windowspec.hip, K18) */
#define OSZ_WS_BANDS_MOST 16      /* the most bands of one call: they travel in the kernel's arguments            */
#define OSZ_WS_EDGES_MOST 16      /* the most edge fractions of one call: they travel in the kernel's arguments   */
#define OSZ_WS_WAVE 512           /* ranges of up to this many bins are reduced by one wave, longer ones by 256 threads */
#define OSZ_WS_LDS 4096           /* ranges of up to this many bins are one tile and are read once; longer ones   */
                                  /* are cut into tiles of this many bins and read twice, the second time from L2 */
typedef enum {
    OSZ_WS_TOTAL = 0,             /* df sum P_k: a rectangle sum (osz_simpson is the Simpson rule)              */
    OSZ_WS_BAND = 1,              /* df sum of P_k over b0 <= k < b1, one plane per band                        */
    OSZ_WS_RELATIVE = 2,          /* band / total, one plane per band                                           */
    OSZ_WS_PEAK = 3,              /* f_k of the largest P_k, ties to the lowest k                               */
    OSZ_WS_CENTROID = 4,          /* c = sum f_k P_k / sum P_k                                                  */
    OSZ_WS_SPREAD = 5,            /* sqrt(sum (f_k - c)^2 P_k / sum P_k), the two-pass form                     */
    OSZ_WS_EDGE = 6,              /* the lowest f_k whose cumulative sum reaches p sum P, one plane per p       */
    OSZ_WS_ENTROPY = 7,           /* -sum p_k ln p_k, p_k = P_k / sum P; over ln n when normalize is set        */
    OSZ_WS_FLATNESS = 8,          /* n exp(mean ln p_k): geometric over arithmetic mean; 0 where a p_k is 0     */
    OSZ_WS_COUNT = 9
} osz_window_spectral_feature;
/*
 * P: nrows = nseg * nch contiguous rows of nfreq float64 periodogram bins on the device, row
 * s * nch + c that of segment s and channel c -- what an OSZ_SPEC_PSD_SEGMENTS push wrote.  One
 * launch reduces the bins k0 .. k1 (inclusive; n = k1 - k0 + 1 of them) of every row to the
 * features in mask (bit 1 << e of an osz_window_spectral_feature) and writes
 * out[p * plane_pitch + c * row_pitch + win0 + s]; the planes are, of those present in mask and in
 * the enum's order, total, nbands of band, nbands of relative, peak, centroid, spread, nedges of
 * edge, entropy, flatness; nothing else of out is touched.  f_k = k * df, one multiply.  bands:
 * nbands pairs of bins [b0, b1) in HOST memory, each not empty and inside k0 .. k1 + 1 (read only
 * when BAND or RELATIVE is asked, 1 <= nbands <= OSZ_WS_BANDS_MOST; they may overlap).  edges:
 * nedges fractions in (0, 1] in HOST memory (read only when EDGE is asked, 1 <= nedges <=
 * OSZ_WS_EDGES_MOST); an edge is bin-valued, nothing is interpolated, and p = 1 gives a bin whose
 * cumulative sum reaches the total (the last bin where rounding keeps every sum below it).  For n
 * = 1 the entropy is 0.
 * A row that holds a NaN in the range is NaN in every feature, peak and edge included.  A row
 * whose range sums to exactly 0 gives total and band 0 and every other feature NaN.  A row's bits
 * depend on its own bins k0 .. k1 and the arguments only -- not on nrows, the row's place, win0 or
 * the other features in mask: every sum has an order that is a function of n alone, and the only
 * atomic operation is an integer minimum.  Ranges of up to OSZ_WS_WAVE bins take one wave per row,
 * longer ones 256 threads; up to OSZ_WS_LDS bins a row is read once, beyond that twice.  One
 * launch, one workgroup per row, no work space.
 */
int osz_spectral_features(const double *P, int64_t nrows, int nch, int64_t nfreq, int64_t k0, int64_t k1,
                          double df, const int *bands, int nbands, const double *edges, int nedges,
                          int normalize, int mask, double *out, int64_t plane_pitch, int64_t row_pitch,
                          int64_t win0, void *stream);

/* ---- channel-pair matrices per window (features/connectivity.py window_connectivity) ------ */
/* (csrc/windowpair.hip, K19) */
#define OSZ_WC_BLOCK 1024         /* a window's pair sums are chains over sub-blocks of this many samples counted */
                                  /* from the window's start, folded in order                                      */
typedef enum {
    OSZ_WC_COV = 0,               /* real rows: numpy.cov of the window, divisor winsize - ddof                    */
    OSZ_WC_CORR = 1,              /* real rows: numpy.corrcoef, clipped to [-1, 1]; diagonal 1.0                   */
    OSZ_WC_AEC = 2,               /* complex rows: Pearson r of the envelopes |z|; diagonal 1.0                    */
    OSZ_WC_PLV = 3,               /* complex rows: |s|, s = mean conj(u_i) u_j, u = z / |z|; diagonal 1.0          */
    OSZ_WC_CIPLV = 4,             /* complex rows: |Im s| / sqrt(1 - (Re s)^2); diagonal 0.0                       */
    OSZ_WC_COUNT = 5
} osz_window_pair_measure;
/*
 * The float64 work space of one osz_window_pairs call with these arguments, in doubles: the staged
 * planes |z|, u_x, u_y of complex data (3 nch n), two sums per (channel, window), and the Gram
 * products of a batch of windows (at most 2^25 doubles, or one window's).  -1 for nch < 2 or >
 * 16384, n < 0, winsize < 4, step < 1, an empty or unknown mask, or a mask that mixes the real
 * measures (COV, CORR) with the complex ones or does not suit is_complex.  Touches no device.
 */
int64_t osz_window_pairs_work(int nch, int64_t n, int64_t winsize, int64_t step, int mask, int is_complex);
/*
 * x: nch rows of n samples on the device, row pitch `pitch` samples: float64 for is_complex = 0,
 * complex128 (16-byte aligned) otherwise.  Window k covers the samples k step .. k step + winsize
 * - 1 of every row; for the nwin = osz_window_count(n, winsize, step) windows and every measure m
 * whose bit 1 << m is set in mask (an osz_window_pair_measure), in the order of the enum,
 *   out[p * plane_pitch + (k * nch + i) * nch + j] = measure of rows i and j over window k   (f64)
 * with p the measure's rank among those present.  Nothing else of out is touched.  ddof (0 or 1)
 * enters COV alone.  [i, j] and [j, i] are written from one value.  An entry's bits depend on
 * winsize, ddof and the window's samples of rows i and j only -- not on step, k, nch, the other
 * rows, mask or how a stream is cut into pushes: the pair sums are the float64 MFMA's k-ordered
 * chains over sub-blocks of OSZ_WC_BLOCK samples counted from the window's start, about the rows'
 * first samples of the window, and nothing is atomic.  A row whose own sums over the window are
 * not finite (a NaN or +-inf sample; for complex rows also a zero sample) is NaN in its row and
 * column, the diagonal included; a constant real row gives COV exactly 0 and CORR NaN there.
 * work: work_len >= osz_window_pairs_work(...) doubles on the device, the caller's.
 */
int osz_window_pairs(const void *x, int64_t pitch, int nch, int64_t n, int is_complex, int64_t winsize, int64_t step,
                     int ddof, int mask, double *out, int64_t plane_pitch, double *work, int64_t work_len,
                     void *stream);

/* ---- fractal dimensions and DFA per window (features/fractal.py window_fractal) ----------- */
/* (csrc/windowfrac.hip, K20) */
#define OSZ_WR_LONGEST 4096       /* the longest window: it is held in LDS, 32 KB                             */
#define OSZ_WR_WIDE 512           /* windows of at least this many samples take 256 threads, shorter ones 64  */
#define OSZ_WR_KMAX 64            /* the largest kmax of higuchi                                              */
#define OSZ_WR_SCALES 32          /* the most scales of dfa: they travel in the kernel's arguments            */
typedef enum {
    OSZ_WR_HIGUCHI = 0,           /* slope of ln L(k) on ln(1 / k), Higuchi 1988                           */
    OSZ_WR_KATZ = 1,              /* ln n / (ln n + ln(d / L)), Katz 1988                                  */
    OSZ_WR_PETROSIAN = 2,         /* log10 W / (log10 W + log10(W / (W + 0.4 N))), Petrosian 1995          */
    OSZ_WR_DFA = 3,               /* slope of ln F(n) on ln n, detrended fluctuation analysis              */
    OSZ_WR_DFA_FLUCTUATIONS = 4,  /* the F(n) themselves, one plane per scale                              */
    OSZ_WR_COUNT = 5
} osz_window_fractal_measure;
/*
 * x, the windows, mask (bit 1 << e of an osz_window_fractal_measure) and out are those of
 * osz_window_features: out[p * plane_pitch + c * row_pitch + win0 + k], p the plane's rank among
 * those present -- higuchi, katz, petrosian, dfa and then the nscales planes of dfa_fluctuations;
 * nothing else of out is touched.  With x_0 .. x_{W-1} one window, W = winsize:
 *   higuchi    for k = 1 .. kmax and m = 0 .. k - 1: n_mk = floor((W - 1 - m) / k),
 *              L_m(k) = (sum_{i=1..n_mk} |x_{m+ik} - x_{m+(i-1)k}|) (W - 1) / (n_mk k) / k, L(k) the
 *              mean of L_m(k) over m; the result is the least-squares slope of v = ln L(k) on u =
 *              ln(1 / k) with the abscissa centred, sum (u - mean u) v / sum (u - mean u)^2.  An
 *              L(k) = 0 gives NaN.
 *   katz       L = sum |x_{i+1} - x_i|, d = max_i |x_i - x_0|, n = W - 1: ln n / (ln n + ln(d / L));
 *              a constant window gives NaN.
 *   petrosian  N the number of i with d_i = x_{i+1} - x_i and d_{i+1} of strictly opposite sign (a
 *              zero difference is no sign): log10 W / (log10 W + log10(W / (W + 0.4 N))).
 *   dfa        y_t = sum_{j<=t} (x_j - mean), the mean from sums about x_0.  For each scale n the
 *              floor(W / n) boxes of n samples counted from the window's first sample (the tail is
 *              dropped); in each box the least-squares line of y about the box's first value;
 *              F(n) = sqrt(mean over all boxed samples of the squared residual).  The result is the
 *              slope of ln F(n) on ln n, centred as above; an F(n) = 0 gives NaN.
 *   dfa_fluctuations  F(n), plane s that of scales[s].
 * scales: nscales ints in HOST memory, read only when a dfa measure is asked: 2 <= nscales <=
 * OSZ_WR_SCALES, strictly increasing, 4 <= n <= winsize / 2.  8 <= winsize <= OSZ_WR_LONGEST, 2 <=
 * kmax <= OSZ_WR_KMAX and winsize >= 2 kmax when higuchi is asked.
 * A window that holds a NaN or +-inf is NaN in every plane.  A window's bits depend on winsize,
 * kmax, scales and its own samples only: every sum runs in an order that is a function of
 * (winsize, k) or (winsize, n) alone, the count of petrosian is an integer, and no floating-point
 * operation is atomic.  One launch, one workgroup per window, no work space.
 */
int osz_window_fractal(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step,
                       int mask, int kmax, const int *scales, int nscales, double *out, int64_t plane_pitch,
                       int64_t row_pitch, int64_t win0, void *stream);

/* ---- wavelet sub-band energies and statistics per window (features/wavelet.py window_wavelet) */
/* (csrc/windowwave.hip, K21) */
#define OSZ_WW_LONGEST 4096       /* the longest window: it and its approximations are held in LDS, 48 KB     */
#define OSZ_WW_WIDE 512           /* windows of up to this many samples take one wave, longer ones 256 threads */
#define OSZ_WW_TAPS 32            /* the longest filter: h and g travel in the kernel's arguments             */
#define OSZ_WW_LEVELS 12          /* the most levels of the transform                                         */
typedef enum {
    OSZ_WW_ENERGY = 0,            /* E_b = sum c^2 over the band's coefficients, one plane per band        */
    OSZ_WW_RELATIVE = 1,          /* p_b = E_b / sum_b E_b, one plane per band                             */
    OSZ_WW_ENTROPY = 2,           /* -sum_b p_b ln p_b (/ ln B with normalize), Rosso et al. 2001          */
    OSZ_WW_MEAN_ABS = 3,          /* mean |c| over the band's coefficients, one plane per band             */
    OSZ_WW_STD = 4,               /* population standard deviation of the band's coefficients, per band    */
    OSZ_WW_COUNT = 5
} osz_window_wavelet_feature;
/*
 * x, the windows and mask (bit 1 << e of an osz_window_wavelet_feature) are those of
 * osz_window_features; out[p * out_plane + c * out_pitch + k], p the plane's rank among those
 * present in enum order, a per-band feature taking B = levels + 1 consecutive planes in the order
 * d^1, d^2, .., d^J, a^J; nothing else of out is touched.
 * The transform is the orthonormal discrete wavelet transform periodised within the window.  With
 * a^0 the window of W = winsize samples (minus its mean when center is not 0, the mean from sums
 * about the window's first sample), n_j the length of a^j, h = lo (taps values in HOST memory, taps
 * even, 2 .. OSZ_WW_TAPS) and g_k = (-1)^k h_{taps-1-k}:
 *   a^{j+1}_i = sum_k h_k a^j_{(2i+k) mod n_j},  d^{j+1}_i = sum_k g_k a^j_{(2i+k) mod n_j},
 * i = 0 .. n_j / 2 - 1, j = 0 .. J - 1, J = levels (1 .. OSZ_WW_LEVELS), winsize a multiple of 2^J
 * and 8 <= winsize <= OSZ_WW_LONGEST.  n_j < taps is allowed: the filter wraps more than once.  The
 * sum over k runs in the order of k, fused multiply-adds.
 *   energy    sum c^2.            relative  E_b / sum_b E_b (NaN when the sum is 0).
 *   entropy   -sum_b p_b ln p_b, a term with p_b = 0 being 0, divided by ln B when normalize is not
 *             0; NaN when sum_b E_b = 0.
 *   mean_abs  (sum |c|) / count.  std  sqrt(sum (c - mean)^2 / count), the band's mean taken first.
 * A window that holds a NaN or +-inf is NaN in every plane.  A window's bits depend on winsize, h,
 * levels, center, normalize and its own samples only: every sum runs in an order that is a function
 * of (winsize, levels, taps) alone and no floating-point operation is atomic.  One launch, one
 * workgroup per (channel, window), no work space.
 */
int osz_window_wavelet(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step,
                       int mask, const double *lo, int taps, int levels, int center, int normalize,
                       double *out, int64_t out_plane, int64_t out_pitch, void *stream);

/* ---- autoregressive models per window (features/ar.py window_ar) -------------------------- */
/* (csrc/windowar.hip, K22) */
#define OSZ_AR_LONGEST 4096       /* the longest window: it is held on chip, in LDS and in registers          */
#define OSZ_AR_WIDE 512           /* windows of at least this many samples take 256 threads, shorter ones 64  */
#define OSZ_AR_ORDER 32           /* the largest model order: one lane a coefficient                          */
typedef enum {
    OSZ_AR_COEFFICIENTS = 0,      /* a_1 .. a_p of the order-p model, one plane each                       */
    OSZ_AR_REFLECTION = 1,        /* k_1 .. k_p, one plane each                                            */
    OSZ_AR_ERROR = 2,             /* E_p, the innovation variance of the order-p model                     */
    OSZ_AR_ERROR_PATH = 3,        /* E_0 .. E_p, one plane each                                            */
    OSZ_AR_COUNT = 4
} osz_window_ar_measure;
typedef enum {
    OSZ_AR_BURG = 0,              /* Burg 1968: k_m from the forward and backward prediction errors        */
    OSZ_AR_YULE_WALKER = 1        /* k_m from the biased autocorrelation                                   */
} osz_window_ar_method;
/*
 * x, the windows, mask (bit 1 << e of an osz_window_ar_measure) and out are those of
 * osz_window_features: out[q * plane_pitch + c * row_pitch + win0 + k], q the plane's rank among
 * those present -- the p planes of coefficients, the p of reflection, error and then the p + 1 of
 * error_path, p = order; nothing else of out is touched.  With x_0 .. x_{W-1} one window, W =
 * winsize, minus its mean when center is not 0 (the mean from sums about the window's first
 * sample), the model is x_t + sum_{k=1..p} a_k x_{t-k} = e_t (the signs of arburg):
 *   burg         f_t = b_t = x_t, E_0 = (1 / W) sum x_t^2.  For m = 1 .. p: num = sum_{t=m}^{W-1}
 *                f_t b_{t-1}, den = sum_{t=m}^{W-1} (f_t^2 + b_{t-1}^2) -- the direct sum, not its
 *                downdating recursion -- k_m = -2 num / den; then for t = m .. W - 1, both from the
 *                old values, f_t <- f_t + k_m b_{t-1} and b_t <- b_{t-1} + k_m f_t.
 *   yule_walker  r_j = (1 / W) sum_{t=0}^{W-1-j} x_t x_{t+j}, j = 0 .. p (biased: |k| < 1), E_0 =
 *                r_0 and k_m = -(r_m + sum_{j=1}^{m-1} a^(m-1)_j r_{m-j}) / E_{m-1}.
 *   both         a^(m)_j = a^(m-1)_j + k_m a^(m-1)_{m-j} for j < m, a^(m)_m = k_m, E_m = E_{m-1}
 *                (1 - k_m^2).
 * 16 <= winsize <= OSZ_AR_LONGEST, 1 <= order <= OSZ_AR_ORDER, winsize >= 4 order; method is an
 * osz_window_ar_method.
 * A window that holds a NaN or +-inf is NaN in every plane.  A window with E_0 = 0 gives error and
 * error_path 0 and coefficients and reflection NaN.  An E_{m-1} that is 0 (or a den that is 0) at a
 * later order makes k_m and everything of the orders from m on NaN, error_path included, and moves
 * nothing before it.  A window's bits depend on winsize, method, center and its own samples only,
 * and those of k_m and E_m not on order: every sum runs in an order that is a function of (winsize,
 * m) or (winsize, j) alone and no floating-point operation is atomic.  One launch, one workgroup per
 * (channel, window), no work space.
 */
int osz_window_ar(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int mask,
                  int order, int method, int center, double *out, int64_t plane_pitch, int64_t row_pitch,
                  int64_t win0, void *stream);

/* ---- lagged cross-correlation per window and pair (features/xcorr.py window_xcorr) -------- */
/* (csrc/windowxcorr.hip, K23) */
#define OSZ_WX_LONGEST 4096       /* the longest window                                                       */
#define OSZ_WX_MAXLAG 64          /* the largest maxlag: the halo of the staged rows                          */
typedef enum {
    OSZ_WX_XCORR = 0,             /* v_ij(l) for every lag l of -maxlag .. maxlag                             */
    OSZ_WX_PEAK = 1,              /* max over l of |v_ij(l)|                                                  */
    OSZ_WX_LAG = 2,               /* the l that attains it (the smallest |l| of equal maxima, then l > 0)     */
    OSZ_WX_SIGNED = 3,            /* v_ij at that lag                                                         */
    OSZ_WX_COUNT = 4
} osz_window_xcorr_measure;
/*
 * The float64 work space of one osz_window_xcorr call with these arguments, in doubles: one sum per
 * (channel, window) and the lagged Gram products of a batch of windows, (2 maxlag + 1) nch nch
 * doubles a window (at most 2^25 doubles, or one window's).  -1 for nch < 2 or > 16384, n < 0,
 * winsize < 8 or > OSZ_WX_LONGEST, step < 1, maxlag < 0 or > min(OSZ_WX_MAXLAG, winsize / 2), or an
 * empty or unknown mask.  Touches no device.
 */
int64_t osz_window_xcorr_work(int nch, int64_t n, int64_t winsize, int64_t step, int maxlag, int mask);
/*
 * x: nch float64 rows of n samples on the device, row pitch `pitch` samples.  Window k covers the
 * samples k step .. k step + winsize - 1 of every row.  With W = winsize, L = maxlag, d_i row i
 * minus its mean over the window and, for -L <= l <= L,
 *   r_ij(l) = (1 / W) sum_t d_i[t] d_j[t + l],  t over max(0, -l) .. min(W, W - l) - 1,
 * v_ij(l) is r_ij(l) / sqrt(r_ii(0) r_jj(0)) clipped to [-1, 1] (normalize = 1) or r_ij(l)
 * (normalize = 0).  For the nwin = osz_window_count(n, winsize, step) windows, with XCORR in mask
 *   xcorr[((k * (2 L + 1) + L + l) * nch + i) * nch + j] = v_ij(l)                          (f64)
 * and for every other measure m of mask (an osz_window_xcorr_measure), in the order of the enum,
 *   out[p * plane_pitch + (k * nch + i) * nch + j] = measure of rows i and j over window k  (f64)
 * with p the measure's rank among those present, XCORR not counted.  xcorr is read only with XCORR
 * in mask, out only with another measure; nothing else of either is touched.  v_ij(l) and v_ji(-l)
 * are written from one value, PEAK and SIGNED to both mirrors, LAG[j, i] = -LAG[i, j].  Of equal
 * |v| the smallest |l| wins, then the positive l (i < j).  The diagonal: lag 0, PEAK and SIGNED are
 * 1.0 (normalize) or r_ii(0), LAG 0.0, and the lags l and -l are written from one value.  An
 * entry's bits depend on winsize, normalize and the window's samples of rows i and j only -- not on
 * step, k, nch, the other rows, mask, maxlag (a lag's plane) or how a stream is cut into pushes: a
 * sum is the float64 MFMA's k-ordered chain over t = 0 .. W - 1 counted from the window's start
 * (the factors outside the window are +0.0), about the row's mean p + s / W, p the row's first
 * sample of the window and s the sum of x - p; nothing is atomic.  A row with a NaN or +-inf
 * sample is NaN in its row and column in every measure; a constant row is NaN there with
 * normalize = 1 and 0 (LAG 0) with normalize = 0.
 * work: work_len >= osz_window_xcorr_work(...) doubles on the device, the caller's.
 */
int osz_window_xcorr(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int maxlag,
                     int normalize, int mask, double *xcorr, double *out, int64_t plane_pitch, double *work,
                     int64_t work_len, void *stream);

/* ---- pairwise Granger causality per window (features/granger.py window_granger) --------- */
/* (csrc/windowgranger.hip, K24) */
#define OSZ_WG_LONGEST 4096       /* the longest window                                                       */
#define OSZ_WG_MAXORDER 16        /* the largest model order: the coefficient blocks of a pair fill the LDS   */
typedef enum {
    OSZ_WG_GRANGER = 0,           /* F_{i->j} = ln(E_j / S_jj): row the source, column the target            */
    OSZ_WG_INSTANT = 1,           /* ln(S_ii S_jj / det S)                                                    */
    OSZ_WG_TOTAL = 2,             /* (F_{i->j} + F_{j->i}) + instant                                          */
    OSZ_WG_COUNT = 3
} osz_window_granger_measure;
/*
 * The float64 work space of one osz_window_granger call with these arguments, in doubles: a sum and
 * a restricted model's error per (channel, window) and the lagged Gram products of a batch of
 * windows, (2 order + 1) nch nch doubles a window (at most 2^25 doubles, or one window's).  -1 for
 * nch < 2 or > 16384, n < 0, winsize < 16 or > OSZ_WG_LONGEST, step < 1, order < 1 or >
 * min(OSZ_WG_MAXORDER, winsize / 8), or an empty or unknown mask.  Touches no device.
 */
int64_t osz_window_granger_work(int nch, int64_t n, int64_t winsize, int64_t step, int order, int mask);
/*
 * x and the windows are those of osz_window_xcorr.  With W = winsize, p = order, d_i row i minus its
 * mean over the window, r_ab(l) = (1 / W) sum_t d_a[t] d_b[t + l] as there and z_t = (d_i[t],
 * d_j[t])^T for the ordered pair (i, j):
 *   C(l) = E[z_t z_{t-l}^T], C(l)_ab = r_ba(l), C(-l) = C(l)^T;
 *   A_1 .. A_p solve C(l) = sum_{k=1..p} A_k C(l - k), l = 1 .. p (the bivariate Yule-Walker
 *   equations, by the block Levinson recursion);  S = C(0) - sum_k A_k C(k)^T;
 *   E_i, E_j: the errors of the scalar Yule-Walker models of order p of d_i and d_j alone;
 *   GRANGER[i, j] = ln(E_j / S_jj),  INSTANT[i, j] = ln(S_ii S_jj / det S),
 *   TOTAL[i, j] = (GRANGER[i, j] + GRANGER[j, i]) + INSTANT[i, j].
 * For the nwin = osz_window_count(n, winsize, step) windows and every measure m of mask (bit 1 << m),
 * in the order of the enum,
 *   out[q * plane_pitch + (k * nch + i) * nch + j] = measure of rows i and j over window k  (f64)
 * with q the measure's rank among those present; nothing else of out is touched.  A finite value
 * below 0 is written as +0.0.  INSTANT and TOTAL are written to both mirrors from one value.  The
 * diagonal is 0.0, and NaN where E_i is not finite and > 0.  A pair is NaN in every measure and both
 * directions when one of E_i, E_j, S_ii, S_jj, det S is not finite and > 0: a row with a NaN or
 * +-inf sample, or a constant row, is NaN in its row and column.  An entry's bits depend on winsize,
 * order and the window's samples of rows i and j only -- not on step, k, nch, the other rows, mask
 * or how a stream is cut into pushes: the sums are osz_window_xcorr's, the order of every operation
 * after them is a function of p alone, and nothing is atomic.
 * work: work_len >= osz_window_granger_work(...) doubles on the device, the caller's.
 */
int osz_window_granger(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int order,
                       int mask, double *out, int64_t plane_pitch, double *work, int64_t work_len, void *stream);

/* ---- binned mutual information per window and pair (features/mutual_info.py window_mutual_info) */
/* (csrc/windowmi.hip, K25) */
#define OSZ_WM_LONGEST 4096       /* the longest window: an int32 count is exact, phi(0 .. W) is a table      */
#define OSZ_WM_MAXBINS 16         /* the most bins: the one-hot rows of a channel fill one matrix tile        */
typedef enum {
    OSZ_WM_COUNTS = 0,            /* n_ab(i, j): the joint histogram itself                                   */
    OSZ_WM_MI = 1,                /* H_i + H_j - H_ij, nats                                                   */
    OSZ_WM_NMI = 2,               /* MI / sqrt(H_i H_j) clipped to [0, 1]                                     */
    OSZ_WM_JOINT = 3,             /* H_ij                                                                     */
    OSZ_WM_COUNT = 4
} osz_window_mi_measure;
typedef enum {
    OSZ_WM_QUANTILE = 0,          /* edges at the k / bins quantiles of the window (Hyndman & Fan type 7)     */
    OSZ_WM_UNIFORM = 1            /* edges lo + k ((hi - lo) / bins), lo and hi the window's extremes         */
} osz_window_mi_binning;
/*
 * The float64 work space of one osz_window_mi call with these arguments, in doubles: the table
 * phi(0 .. winsize), and for a batch of windows the edges, marginal counts and bin codes per
 * (channel, window) and the int32 joint counts, (nch Bp)^2 a window with Bp = bins rounded up to a
 * power of two (at most 2^25 doubles, or one window's).  -1 for nch < 2 or > 16384, n < 0, winsize
 * < 16 or > OSZ_WM_LONGEST, step < 1, bins < 2 or > OSZ_WM_MAXBINS, or an empty or unknown mask.
 * Touches no device.
 */
int64_t osz_window_mi_work(int nch, int64_t n, int64_t winsize, int64_t step, int bins, int mask);
/*
 * x and the windows are those of osz_window_xcorr.  With W = winsize and B = bins, a window of a row
 * has the edges e_1 <= .. <= e_{B-1}: the k / B quantiles of its samples, osz_window_quantiles'
 * arithmetic to the bit (binning OSZ_WM_QUANTILE), or lo + k ((hi - lo) / B), each operation one
 * IEEE operation (OSZ_WM_UNIFORM).  A sample's bin is the number of edges <= it; n_ab(i, j) counts
 * the samples t with row i in bin a and row j in bin b; n_a(i) are the marginal counts.  With
 * phi(n) = n ln n, phi(0) = 0, and S(.) the sum of phi over the cells in the order a, then b:
 *   H_i = (phi(W) - S(n_a)) / W,  H_ij = (phi(W) - S(n_ab)) / W,  MI_ij = (H_i + H_j) - H_ij.
 * For the nwin = osz_window_count(n, winsize, step) windows, with COUNTS in mask
 *   counts[(((k * B + a) * B + b) * nch + i) * nch + j] = n_ab(i, j)                       (f64)
 * and for every other measure m of mask (an osz_window_mi_measure), in the order of the enum,
 *   out[p * plane_pitch + (k * nch + i) * nch + j] = measure of rows i and j over window k  (f64)
 * with p the measure's rank among those present, COUNTS not counted.  counts is read only with
 * COUNTS in mask, out only with another measure.  MI below 0 is written as +0.0; NMI is NaN where
 * H_i H_j = 0.  Every measure is computed for i < j and written to both mirrors, counts[a, b, i, j]
 * and counts[b, a, j, i] from one value.  The diagonal: MI = JOINT = H_i, NMI = 1.0 (NaN for H_i =
 * 0), counts n_a for a = b and 0 elsewhere.  A row with a NaN or +-inf sample (under UNIFORM also
 * one whose hi - lo is not finite) is NaN in its row and column in every measure, counts included.
 * An entry's bits depend on winsize, bins, binning and the window's samples of rows i and j only:
 * the counts are the int8 MFMA's exact int32 sums, phi is read from one table, the sums of phi run
 * in an order that is a function of B alone, nothing is atomic.
 * work: work_len >= osz_window_mi_work(...) doubles on the device, the caller's.
 */
int osz_window_mi(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int bins,
                  int binning, int mask, double *counts, double *out, int64_t plane_pitch, double *work,
                  int64_t work_len, void *stream);

/* ---- binned transfer entropy per window and ordered pair (features/transfer_entropy.py) */
/* (csrc/windowte.hip, K26) */
#define OSZ_WT_LONGEST 4096       /* the longest window, osz_window_mi's                                      */
#define OSZ_WT_MAXBINS 8          /* the most bins: a (bin now, bin before) symbol is one byte below 0xFF     */
#define OSZ_WT_MAXLAG 64          /* the largest lag of the source                                            */
typedef enum {
    OSZ_WT_COUNTS = 0,            /* n_abc(i, j): the three-way histogram itself                              */
    OSZ_WT_TE = 1,                /* I(Y_t ; X_{t-u} | Y_{t-1}), nats, source i (row) to target j (column)    */
    OSZ_WT_NTE = 2,               /* TE / H(Y_t | Y_{t-1}) clipped to [0, 1]                                  */
    OSZ_WT_NET = 3,               /* TE[i, j] - TE[j, i]                                                      */
    OSZ_WT_COUNT = 4
} osz_window_te_measure;
/*
 * The float64 work space of one osz_window_te call with these arguments, in doubles: the table
 * phi(0 .. winsize), and for a batch of windows osz_window_mi's edges, marginal counts and bin
 * codes per (channel, window), as many bytes of symbols again and the int32 counts, (nch Bp^2) x
 * (nch Bp) a window with Bp = bins rounded up to a power of two (at most 2^25 doubles, or one
 * window's).  -1 for nch < 2 or > 16384, n < 0, winsize < 16 or > OSZ_WT_LONGEST, step < 1, bins
 * < 2 or > OSZ_WT_MAXBINS, lag < 1 or > min(OSZ_WT_MAXLAG, winsize / 2), or an empty or unknown
 * mask.  Touches no device.
 */
int64_t osz_window_te_work(int nch, int64_t n, int64_t winsize, int64_t step, int bins, int lag, int mask);
/*
 * x, the windows, the edges and the bins (binning: an osz_window_mi_binning) are those of
 * osz_window_mi: the bins of a window are cut from all W = winsize samples.  With B = bins, u = lag
 * and T = W - u, n_abc(i, j) counts the t = u .. W - 1 of the window with the target, row j, in bin
 * a at t and in bin b at t - 1 and the source, row i, in bin c at t - u.  With phi(n) = n ln n,
 * phi(0) = 0, every sum in one thread, b outermost, then a, then c:
 *   S3 = sum_bac phi(n_abc)          Sab = sum_ba phi(sum_c n_abc)
 *   Sbc = sum_bc phi(sum_a n_abc)    Sb = sum_b phi(sum_ac n_abc)     (the inner sums are integers)
 *   TE = ((S3 - Sab) - (Sbc - Sb)) / T,   Hc = (Sb - Sab) / T.
 * For the nwin = osz_window_count(n, winsize, step) windows, with COUNTS in mask
 *   counts[((((k * B + a) * B + b) * B + c) * nch + i) * nch + j] = n_abc(i, j)            (f64)
 * and for every other measure m of mask (an osz_window_te_measure), in the order of the enum,
 *   out[p * plane_pitch + (k * nch + i) * nch + j] = measure from row i to row j, window k  (f64)
 * with p the measure's rank among those present, COUNTS not counted.  counts is read only with
 * COUNTS in mask, out only with another measure.  A finite TE below 0 is written as +0.0; NTE is
 * TE / Hc clipped to [0, 1], NaN where Hc = 0; NET[i, j] is TE[i, j] - TE[j, i] and NET[j, i] is
 * TE[j, i] - TE[i, j], each one subtraction.  The diagonal of TE, NTE and NET is +0.0; counts[..,
 * i, i] is what the definition gives.  A row with a NaN or +-inf sample (under UNIFORM also one
 * whose hi - lo is not finite) is NaN in its row and column in every measure, counts included.
 * An entry's bits depend on winsize, bins, lag, binning and the window's samples of rows i and j
 * only: the counts are the int8 MFMA's exact int32 sums, phi is read from one table, the sums of
 * phi run in an order that is a function of B alone, nothing is atomic.
 * work: work_len >= osz_window_te_work(...) doubles on the device, the caller's.
 */
int osz_window_te(const double *x, int64_t pitch, int nch, int64_t n, int64_t winsize, int64_t step, int bins,
                  int lag, int binning, int mask, double *counts, double *out, int64_t plane_pitch, double *work,
                  int64_t work_len, void *stream);

/* ---- banded spectral connectivity per window (features/coherence.py) */
/* (csrc/windowcoh.hip, K27) */
#define OSZ_WK_BANDS_MOST 16      /* the most bands of one call                                               */
typedef enum {
    OSZ_WK_COH = 0,               /* |sum z|^2 / (sum |X_i|^2 sum |X_j|^2), z = conj(X_i) X_j                 */
    OSZ_WK_IMCOH = 1,             /* Im sum z / sqrt(sum |X_i|^2 sum |X_j|^2)                                 */
    OSZ_WK_PLV = 2,               /* |sum z / |z|| / N                                                        */
    OSZ_WK_PLI = 3,               /* |sum sign d| / N, d = Im z                                               */
    OSZ_WK_WPLI = 4,              /* |sum d| / sum |d|                                                        */
    OSZ_WK_DWPLI = 5,             /* ((sum d)^2 - sum d^2) / ((sum |d|)^2 - sum d^2)                          */
    OSZ_WK_COUNT = 6
} osz_window_coherence_measure;
/*
 * The float64 work space of one osz_window_coherence call with these arguments, in doubles: 0, the
 * sums of a window stay in registers and its bins are folded in LDS.  -1 for nseg < 0 or >= 2^31,
 * nch < 2 or > 16384, nfreq < 2, nch * nfreq >= 2^27, nsub < 2, mstep < 1, nbands < 1 or >
 * OSZ_WK_BANDS_MOST, or an empty or unknown mask.  Touches no device.
 */
int64_t osz_window_coherence_work(int64_t nseg, int nch, int nfreq, int nsub, int mstep, int nbands, int mask);
/*
 * X: the contiguous complex128 (nseg, nch, nfreq) segment spectra of an OSZ_SPEC_DFT_SEGMENTS
 * push, on the device.  Window k is the N = nsub segments k * mstep .. k * mstep + nsub - 1, nwin =
 * (nseg - nsub) / mstep + 1 of them (0 for nseg < nsub: osz_window_count's rule, from nsub = 2 on).  bands: nbands pairs [b0, b1) of bins on the host,
 * 1 <= b0 < b1 <= nfreq (the caller keeps a real Nyquist bin out).  Per window, pair and bin the
 * sums over the window's segments, in segment order, are osz_cross_accumulate's (of X for COH and
 * IMCOH, of X / |X| for PLV) and osz_lag_accumulate's (PLI, WPLI, DWPLI), and the measure is the
 * definition above with N = nsub; a band's value is the sum of its bins' values in bin order times
 * 1 / (b1 - b0).  For every measure m of mask (bit 1 << m), in the order of the enum,
 *   out[p * plane_pitch + (((k * nbands + b) * nch + i) * nch + j)] = measure of band b, window k (f64)
 * with p the measure's rank among those present; plane_pitch >= nwin * nbands * nch * nch.  [j, i]
 * is written from the value of [i, j], i < j (IMCOH: negated, a zero +0.0 on both sides).  The
 * diagonal is 1.0 for COH and PLV and 0.0 for the others.  A channel whose own sums are NaN in a
 * bin of the band -- a non-finite spectrum value; for COH, IMCOH and PLV also one without power --
 * is NaN in its row and column, the diagonal included; a zero denominator gives the NaN it gives.
 * An entry's bits depend on nsub, the band's bins and the window's spectra of channels i and j
 * only; nothing is atomic.  Arguments that hold no window return OSZ_OK and launch nothing.
 * work: work_len >= osz_window_coherence_work(...) doubles, the caller's; it may be null.
 */
int osz_window_coherence(const void *X, int64_t nseg, int nch, int nfreq, int nsub, int mstep, const int *bands,
                         int nbands, int mask, double *out, int64_t plane_pitch, double *work, int64_t work_len,
                         void *stream);

/* ---- EDF record decode ----------------------------- */
/*
 * Replaces the host-side unpacking of edf.Reader (reference
 * file_io/edf.py:452-483 _records, :382-419 _decipher, :506-556 _read_array):
 * the file's little-endian int16 records go to the device as they are (2 B per
 * sample over PCIe instead of 8) and are de-interleaved and scaled there.
 * raw: device int16, records [rec0, ...) of `reclen` samples each; per-channel
 * device arrays choff/spr (int32), slope/offset (f64), len (int64: samples the
 * channel can fill; the rest of the `width` columns get padvalue*slope+offset,
 * as the reference pads before deciphering).  out: (nch, width) f64.
 */
int osz_edf_decode(const int16_t *raw, int reclen, int nch, const int32_t *choff,
                   const int32_t *spr, const double *slope, const double *offset,
                   const int64_t *len, int64_t rec0, int64_t start, int64_t width,
                   double padvalue, double *out, int64_t ldo, void *stream);

/* ---- EDF record encode ------------------------------------------------- */
/*
 * The inverse of osz_edf_decode, for edf.Writer (reference file_io/edf.py:660-697
 * _records, _encipher): physical float64 samples -> the little-endian int16 data
 * records of an EDF file.  Row c of the source is the first h[c] columns of `carry`
 * (nch rows of pitch ldc, nc columns; null: none) followed by the nx columns of x
 * (nch rows of pitch ldx).  Per-channel device arrays spr / choff (int32: samples per
 * record, offset inside an output record; reclen = sum of spr) and slope / offset
 * (f64).  out: device int16, nrec * reclen values, 8-byte aligned; record r holds for
 * each channel in turn rint((row_c[r spr[c] + j] - offset[c]) / slope[c]), j < spr[c]:
 * one IEEE subtraction, one IEEE division, round half to even.  Results above 32767
 * (and +inf) write 32767, below -32768 (and -inf) -32768, NaN writes 0 -- where the
 * reference's cast is undefined -- and counter[0] (saturated) and counter[1] (NaN),
 * two device uint64 the caller zeroes, are added to.  A sample neither source holds
 * reads as NaN.  10 bytes of HBM traffic per sample.
 */
int osz_edf_encode(const double *x, int64_t ldx, int64_t nx, const double *carry, int64_t ldc,
                   int64_t nc, const int32_t *h, int nch, const int32_t *spr, const int32_t *choff,
                   const double *slope, const double *offset, int reclen, int64_t nrec,
                   int16_t *out, uint64_t *counter, void *stream);

/* ---- synthetic device-resident source (benchmarks, tests) ------------- */
/* x[c, j] = N(0,1) keyed by (seed, ch0 + c, n0 + j): counter-based, so any
 * shard or chunk is reproducible on CPU and GPU alike. */
int osz_synth_normal(double *x, int64_t ldx, int nch, int64_t n, uint64_t seed,
                     int64_t ch0, int64_t n0, void *stream);
/* 64-bit order-independent checksum of a (nch, n) block: sum of the bit
 * patterns, plus the float sum; both written to host. Synchronous. */
int osz_checksum(const double *x, int64_t ldx, int nch, int64_t n,
                 uint64_t *bits, double *fsum, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OSZ_HIP_H */
