"""ctypes binding of libosz_hip.so (the C ABI declared in include/osz_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or cannot
be loaded, every numerical entry point raises ``OszLibraryError``.
"""

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# OSZ_HIP_LIB points the binding at another build of the same C ABI
LIB_PATH = os.environ.get("OSZ_HIP_LIB") or os.path.join(_HERE, "lib", "libosz_hip.so")
CSRC = os.path.join(_HERE, "csrc")

OSZ_OK = 0
OSZ_ERR_INVALID = -1
OSZ_ERR_HIP = -2
OSZ_ERR_NOMEM = -3
OSZ_ERR_STATE = -4
OSZ_ERR_UNSUPPORTED = -5

SPEC_PSD_MEAN, SPEC_PSD_SEGMENTS, SPEC_DFT_SEGMENTS = 0, 1, 2
EW_ADD, EW_MUL, EW_DIV, EW_STANDARDIZE = 0, 1, 2, 3
BCAST_SCALAR, BCAST_ROW, BCAST_COL, BCAST_FULL = 0, 1, 2, 3
DETREND = {"constant": 0, "linear": 1}
CROSS_SPECTRUM, CROSS_COHERENCE = 0, 1
PHASE_MODE = {"imcoh": 0, "plv": 1, "pli": 2, "wpli": 3, "dwpli": 4}
JACK_MODE = {"coherence": 0, "imcoh": 1, "plv": 2, "pli": 3, "wpli": 4, "dwpli": 5}
ANALYTIC_MODE = {"aec": 0, "oaec": 1, "plv": 2, "ciplv": 3, "wpli": 4}
# the sum group (a bit) each analytic measure reads, and the (nch, nch) planes a group keeps
ANALYTIC_AMP, ANALYTIC_ORTH, ANALYTIC_LOCK, ANALYTIC_LAG = 1, 2, 4, 8
ANALYTIC_GROUP = {"aec": ANALYTIC_AMP, "oaec": ANALYTIC_ORTH, "plv": ANALYTIC_LOCK, "ciplv": ANALYTIC_LOCK,
                  "wpli": ANALYTIC_LAG}
ANALYTIC_PLANES = {ANALYTIC_AMP: 1, ANALYTIC_ORTH: 5, ANALYTIC_LOCK: 2, ANALYTIC_LAG: 2}
ANALYTIC_BLOCK = 4096
BISPEC_MODE = {"spectrum": 0, "kim": 1, "hagihira": 2}
# OSZ_WF_*: a feature's bit in the mask of osz_window_features is 1 << its value
WINDOW_FEATURE = {"mean": 0, "var": 1, "rms": 2, "skew": 3, "kurtosis": 4, "min": 5, "max": 6, "ptp": 7,
                  "line_length": 8, "zero_crossings": 9, "mobility": 10, "complexity": 11, "teager": 12}
WF_LONG = 4096       # OSZ_WF_LONG: windows of at least this many samples take the workgroup kernel
# OSZ_WE_*: a measure's bit in the mask of osz_window_entropy is 1 << its value
WINDOW_ENTROPY = {"sample": 0, "sample_a": 1, "sample_b": 2, "permutation": 3}
WE_TOLERANCE = {"std": 0, "absolute": 1}      # OSZ_WE_TOL_*
WE_LONGEST = 4096    # OSZ_WE_LONGEST: the longest window of osz_window_entropy (it is held in LDS)
WE_WIDE = 512        # OSZ_WE_WIDE: windows of at least this many samples take a workgroup of 256, shorter ones a wave
# OSZ_WQ_*: a measure's bit in the mask of osz_window_quantiles is 1 << its value
WINDOW_QUANTILE = {"median": 0, "mad": 1, "quantile": 2}
WQ_LONGEST = 4096    # OSZ_WQ_LONGEST: the longest window of osz_window_quantiles (it is sorted on chip)
WQ_QMOST = 16        # OSZ_WQ_QMOST: the most quantiles of one call
WQ_NARROWEST = 64    # OSZ_WQ_NARROWEST: the least padded width; one kernel instance per power of two up to WQ_LONGEST
WQ_WAVE = 512        # OSZ_WQ_WAVE: windows of up to this many samples are sorted by one wave, longer ones by 256 threads
# OSZ_WS_*: a feature's bit in the mask of osz_spectral_features is 1 << its value
WINDOW_SPECTRAL = {"total": 0, "band": 1, "relative": 2, "peak": 3, "centroid": 4, "spread": 5, "edge": 6,
                   "entropy": 7, "flatness": 8}
WS_BANDS_MOST = 16   # OSZ_WS_BANDS_MOST: the most bands of one call
WS_EDGES_MOST = 16   # OSZ_WS_EDGES_MOST: the most edge fractions of one call
WS_WAVE = 512        # OSZ_WS_WAVE: ranges of up to this many bins are reduced by one wave, longer ones by 256 threads
WS_LDS = 4096        # OSZ_WS_LDS: ranges of up to this many bins are one tile, read once; longer ones are read twice
# OSZ_WC_*: a measure's bit in the mask of osz_window_pairs is 1 << its value; the first two take real data
WINDOW_CONNECTIVITY = {"cov": 0, "corr": 1, "aec": 2, "plv": 3, "ciplv": 4}
WC_REAL = ("cov", "corr")
WC_BLOCK = 1024      # OSZ_WC_BLOCK: a window's pair sums are chains over sub-blocks of this many samples, folded in order
# OSZ_WR_*: a measure's bit in the mask of osz_window_fractal is 1 << its value
WINDOW_FRACTAL = {"higuchi": 0, "katz": 1, "petrosian": 2, "dfa": 3, "dfa_fluctuations": 4}
WR_LONGEST = 4096    # OSZ_WR_LONGEST: the longest window of osz_window_fractal (it is held in LDS)
WR_WIDE = 512        # OSZ_WR_WIDE: windows of at least this many samples take a workgroup of 256, shorter ones a wave
WR_KMAX = 64         # OSZ_WR_KMAX: the largest kmax of higuchi
WR_SCALES = 32       # OSZ_WR_SCALES: the most scales of dfa
# OSZ_WW_*: a feature's bit in the mask of osz_window_wavelet is 1 << its value
WINDOW_WAVELET = {"energy": 0, "relative": 1, "entropy": 2, "mean_abs": 3, "std": 4}
WW_LONGEST = 4096    # OSZ_WW_LONGEST: the longest window of osz_window_wavelet (it is held in LDS)
WW_WIDE = 512        # OSZ_WW_WIDE: windows of up to this many samples take one wave, longer ones a workgroup of 256
WW_TAPS = 32         # OSZ_WW_TAPS: the longest filter
WW_LEVELS = 12       # OSZ_WW_LEVELS: the most levels of the transform
# OSZ_AR_*: a measure's bit in the mask of osz_window_ar is 1 << its value
WINDOW_AR = {"coefficients": 0, "reflection": 1, "error": 2, "error_path": 3}
AR_METHOD = {"burg": 0, "yule_walker": 1}     # osz_window_ar_method
AR_LONGEST = 4096    # OSZ_AR_LONGEST: the longest window of osz_window_ar (it is held on chip)
AR_WIDE = 512        # OSZ_AR_WIDE: windows of at least this many samples take a workgroup of 256, shorter ones a wave
AR_ORDER = 32        # OSZ_AR_ORDER: the largest model order
# OSZ_WX_*: a measure's bit in the mask of osz_window_xcorr is 1 << its value
WINDOW_XCORR = {"xcorr": 0, "peak": 1, "lag": 2, "signed": 3}
WX_LONGEST = 4096    # OSZ_WX_LONGEST: the longest window of osz_window_xcorr
WX_MAXLAG = 64       # OSZ_WX_MAXLAG: the largest maxlag (the halo of the rows staged on chip)
# OSZ_WG_*: a measure's bit in the mask of osz_window_granger is 1 << its value
WINDOW_GRANGER = {"granger": 0, "instant": 1, "total": 2}
WG_LONGEST = 4096    # OSZ_WG_LONGEST: the longest window of osz_window_granger
WG_MAXORDER = 16     # OSZ_WG_MAXORDER: the largest model order (a pair's coefficient blocks are held in LDS)
# OSZ_WM_*: a measure's bit in the mask of osz_window_mi is 1 << its value
WINDOW_MI = {"counts": 0, "mi": 1, "nmi": 2, "joint": 3}
MI_BINNING = {"quantile": 0, "uniform": 1}    # osz_window_mi_binning
WM_LONGEST = 4096    # OSZ_WM_LONGEST: the longest window of osz_window_mi
WM_MAXBINS = 16      # OSZ_WM_MAXBINS: the most bins (a channel's one-hot rows fill one matrix tile)
# OSZ_WT_*: a measure's bit in the mask of osz_window_te is 1 << its value; the binnings are MI_BINNING
WINDOW_TE = {"counts": 0, "te": 1, "nte": 2, "net": 3}
WT_LONGEST = 4096    # OSZ_WT_LONGEST: the longest window of osz_window_te
WT_MAXBINS = 8       # OSZ_WT_MAXBINS: the most bins (a (bin now, bin before) symbol is one byte below 0xFF)
WT_MAXLAG = 64       # OSZ_WT_MAXLAG: the largest lag of the source
# OSZ_WK_*: a measure's bit in the mask of osz_window_coherence is 1 << its value
WINDOW_COHERENCE = {"coh": 0, "imcoh": 1, "plv": 2, "pli": 3, "wpli": 4, "dwpli": 5}
WK_BANDS_MOST = 16   # OSZ_WK_BANDS_MOST: the most bands of one call
# OSZ_SOSK_*: the kernel of a record of osz_sos_last_launches, and the record's fields in order
SOS_KERNEL = ("sos_kernel", "sos_split", "sos_split_lean", "sos_split2", "sos_dual", "sos_dual_lean",
              "sos_dual2", "seal")
SOS_LAUNCH_FIELDS = ("kernel", "rev", "guard", "al16", "nseg", "seglen", "seglen_b", "pre", "prex",
                     "warmup", "n", "n_b")
SOS_LAUNCH_RECORDS = 8
# OSZ_FIRK_*: the kernel of a record of osz_fir_last_launches, and the record's fields in order
FIR_KERNEL = ("nega", "pair")
FIR_LAUNCH_FIELDS = ("kernel", "rows", "pf", "piece", "taps", "step", "nblocks", "R", "nruns", "accum",
                     "n", "skip")
FIR_LAUNCH_RECORDS = 16
# OSZ_SPECK_*: the family of a record of osz_spec_last_launches, and the record's scalar fields in
# order; SPEC_LAUNCH_RADIX values of the radix plan follow them
SPEC_FAMILY = ("cube", "fft8", "mix", "split", "blue", "staged")
SPEC_LAUNCH_SCALARS = ("family", "size", "mode", "linear", "half", "nseg", "R", "nruns", "head", "npass",
                       "R0", "S0")
SPEC_LAUNCH_RADIX = 14
SPEC_LAUNCH_FIELDS = len(SPEC_LAUNCH_SCALARS) + SPEC_LAUNCH_RADIX
SPEC_LAUNCH_RECORDS = 8


class OszLibraryError(RuntimeError):
    """libosz_hip.so is missing or failed to load."""


c_dp = ctypes.POINTER(ctypes.c_double)
c_i64 = ctypes.c_int64
c_vp = ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/osz_hip.h one to one
CHAIN_DEFER = 1

SIGNATURES = {
    "osz_version": (ctypes.c_int, []),
    "osz_last_error": (ctypes.c_char_p, []),
    "osz_device_info": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_size_t),
                                       ctypes.c_char_p, ctypes.c_int]),
    "osz_malloc": (ctypes.c_int, [ctypes.POINTER(c_vp), ctypes.c_size_t]),
    "osz_free": (ctypes.c_int, [c_vp]),
    "osz_memcpy_h2d": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "osz_memcpy_d2h": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "osz_memcpy_d2d": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "osz_memset": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_size_t, c_vp]),
    "osz_stream_sync": (ctypes.c_int, [c_vp]),
    "osz_event_create": (ctypes.c_int, [ctypes.POINTER(c_vp)]),
    "osz_event_destroy": (ctypes.c_int, [c_vp]),
    "osz_event_record": (ctypes.c_int, [c_vp, c_vp]),
    "osz_event_elapsed_ms": (ctypes.c_int, [c_vp, c_vp,
                                            ctypes.POINTER(ctypes.c_float)]),
    "osz_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "osz_profile_reset": (ctypes.c_int, []),
    "osz_profile_query": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(c_i64),
                                         ctypes.POINTER(ctypes.c_double)]),
    "osz_sos_create": (ctypes.c_int, [ctypes.POINTER(c_vp), c_dp, ctypes.c_int,
                                      ctypes.c_int]),
    "osz_sos_destroy": (ctypes.c_int, [c_vp]),
    "osz_sos_set_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_sos_get_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_sos_set_zi_unit": (ctypes.c_int, [c_vp, c_dp]),
    "osz_sos_set_state_scaled": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_vp]),
    "osz_sos_forward": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, c_i64,
                                       c_vp]),
    "osz_sos_warmup_len": (c_i64, [c_vp]),
    "osz_sos_set_warmup_len": (ctypes.c_int, [c_vp, c_i64]),
    "osz_sosfiltfilt_chunk": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_vp,
                                             c_i64, c_i64, c_vp, c_i64, c_vp]),
    "osz_sosfiltfilt_step": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_vp, c_i64,
                                            c_vp, c_i64, c_i64, c_vp, c_i64, c_i64,
                                            c_vp, c_i64, c_vp]),
    "osz_chain_forward": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp]),
    "osz_chain_forward_route": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "osz_chain_forward_plan": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int]),
    "osz_chain_step": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64,
                                      c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64,
                                      ctypes.c_int, c_vp]),
    "osz_chain_wait": (ctypes.c_int, [c_vp, c_vp]),
    "osz_chain_zp_lag": (c_i64, [c_vp, c_vp]),
    "osz_chain_zp_plan": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int]),
    "osz_chain_zp_tolerance": (ctypes.c_int, [c_vp, c_vp, ctypes.c_double]),
    "osz_chain_zp_reach": (ctypes.c_int, [c_vp, c_vp, c_i64]),
    "osz_chain_zp_min_chunk": (c_i64, [c_vp, c_vp]),
    "osz_chain_zp_open": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp]),
    "osz_chain_zp_step": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp]),
    "osz_chain_zp_seal": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp]),
    "osz_chain_zp_finish": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp]),
    "osz_sos_warm_len": (c_i64, [c_vp]),
    "osz_sos_last_launches": (ctypes.c_int, [c_vp, ctypes.POINTER(c_i64), ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int)]),
    "osz_fir_create": (ctypes.c_int, [ctypes.POINTER(c_vp), c_dp, ctypes.c_int,
                                      ctypes.c_int]),
    "osz_fir_destroy": (ctypes.c_int, [c_vp]),
    "osz_fir_reset": (ctypes.c_int, [c_vp, c_vp]),
    "osz_fir_state_size": (c_i64, [c_vp]),
    "osz_fir_get_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_fir_set_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_fir_push": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_vp, c_i64,
                                    c_i64, c_vp]),
    "osz_fir_flush": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp]),
    "osz_fir_last_launches": (ctypes.c_int, [c_vp, ctypes.POINTER(c_i64), ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int)]),
    "osz_poly_create": (ctypes.c_int, [ctypes.POINTER(c_vp), c_dp, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int]),
    "osz_poly_create_centred": (ctypes.c_int, [ctypes.POINTER(c_vp), c_dp, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "osz_poly_destroy": (ctypes.c_int, [c_vp]),
    "osz_poly_reset": (ctypes.c_int, [c_vp, c_vp]),
    "osz_poly_state_size": (c_i64, [c_vp]),
    "osz_poly_get_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_poly_set_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_poly_out_count": (c_i64, [c_vp, c_i64, ctypes.c_int]),
    "osz_poly_plan": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int]),
    "osz_poly_push": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, ctypes.c_int,
                                     c_vp, c_i64, ctypes.POINTER(c_i64), c_vp]),
    "osz_spec_create": (ctypes.c_int, [ctypes.POINTER(c_vp), ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, c_dp,
                                       ctypes.c_double, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int]),
    "osz_spec_destroy": (ctypes.c_int, [c_vp]),
    "osz_spec_reset": (ctypes.c_int, [c_vp, c_vp]),
    "osz_spec_seg_count": (c_i64, [c_vp, c_i64]),
    "osz_spec_push": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, c_vp,
                                     ctypes.POINTER(c_i64), c_vp]),
    "osz_spec_last_launches": (ctypes.c_int, [c_vp, ctypes.POINTER(c_i64), ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int)]),
    "osz_spec_sum": (ctypes.c_int, [c_vp, ctypes.POINTER(c_vp),
                                    ctypes.POINTER(c_i64)]),
    "osz_spec_export_sum": (ctypes.c_int, [c_vp, c_vp, ctypes.POINTER(c_i64), c_vp]),
    "osz_spec_mean": (ctypes.c_int, [c_vp, c_dp, ctypes.POINTER(c_i64), c_vp]),
    "osz_spec_mean_device": (ctypes.c_int, [c_vp, c_vp, ctypes.POINTER(c_i64), c_vp]),
    "osz_spec_state_size": (c_i64, [c_vp]),
    "osz_spec_get_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_spec_set_state": (ctypes.c_int, [c_vp, c_dp, c_vp]),
    "osz_rccl_bind": (ctypes.c_int, [ctypes.c_char_p]),
    "osz_rccl_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "osz_rccl_comm_create": (ctypes.c_int, [ctypes.POINTER(c_vp), ctypes.c_int, ctypes.c_int,
                                            ctypes.c_char_p]),
    "osz_rccl_comm_destroy": (ctypes.c_int, [c_vp]),
    "osz_rccl_comm_size": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_int)]),
    "osz_welch_reduce": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "osz_moments_create": (ctypes.c_int, [ctypes.POINTER(c_vp), ctypes.c_int]),
    "osz_moments_destroy": (ctypes.c_int, [c_vp]),
    "osz_moments_reset": (ctypes.c_int, [c_vp, c_vp]),
    "osz_moments_push": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, ctypes.c_int, c_vp]),
    "osz_moments_finish": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "osz_col_moments": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, ctypes.c_int, c_vp, c_vp,
                                       c_vp]),
    "osz_ew": (ctypes.c_int, [ctypes.c_int, c_vp, c_i64, ctypes.c_int, c_i64, c_vp, c_vp,
                              ctypes.c_int, c_i64, c_vp, c_i64, c_vp]),
    "osz_complex_join": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, ctypes.c_int, c_i64, c_vp,
                                        c_i64, c_vp]),
    "osz_magphase": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "osz_phase_index": (ctypes.c_int, [c_vp, c_i64, ctypes.c_double, ctypes.c_double, c_vp, c_vp,
                                       ctypes.POINTER(c_i64), c_vp]),
    "osz_lock_accumulate": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, ctypes.c_int, c_i64,
                                           c_i64, c_vp, c_i64, c_vp, c_vp]),
    "osz_phase_bins": (ctypes.c_int, [c_vp, ctypes.c_int, c_i64, c_i64, ctypes.c_int, c_vp, c_i64,
                                      c_vp]),
    "osz_pac_accumulate": (ctypes.c_int, [c_vp, ctypes.c_int, c_i64, c_vp, ctypes.c_int, c_i64,
                                          c_i64, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                          c_vp]),
    "osz_pac_finish": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, c_vp, c_vp, c_vp]),
    "osz_cross_accumulate": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "osz_cross_finish": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, c_vp, c_vp]),
    "osz_lag_accumulate": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "osz_unit_phasors": (ctypes.c_int, [c_vp, c_i64, c_vp]),
    "osz_phase_finish": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_vp, c_i64, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "osz_jackknife_accumulate": (ctypes.c_int, [ctypes.c_int, c_vp, c_i64, ctypes.c_int, ctypes.c_int,
                                                c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "osz_jackknife_finish": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_vp, c_vp, c_i64, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "osz_analytic_work": (c_i64, [ctypes.c_int, c_i64, ctypes.c_int]),
    "osz_analytic_accumulate": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, ctypes.c_int, c_vp, c_vp, c_vp,
                                               c_i64, c_vp]),
    "osz_analytic_finish": (ctypes.c_int, [ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_i64, ctypes.c_int, c_vp,
                                           c_vp]),
    "osz_bispec_work": (c_i64, [c_i64, ctypes.c_int, ctypes.c_int]),
    "osz_bispec_accumulate": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             c_vp, c_vp, c_vp, c_i64, c_vp]),
    "osz_bispec_finish": (ctypes.c_int, [ctypes.c_int, c_vp, c_vp, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, c_vp, c_vp]),
    "osz_window_count": (c_i64, [c_i64, c_i64, c_i64]),
    "osz_window_features": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, c_vp, c_i64,
                                           c_i64, c_i64, c_vp]),
    "osz_window_entropy": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_double, ctypes.c_int, ctypes.c_int, c_i64, ctypes.c_int, c_vp,
                                          c_i64, c_i64, c_i64, c_vp]),
    "osz_window_quantiles": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, c_vp,
                                            ctypes.c_int, c_vp, c_i64, c_i64, c_i64, c_vp]),
    "osz_spectral_features": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_double, c_vp,
                                             ctypes.c_int, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                             c_i64, c_i64, c_i64, c_vp]),
    "osz_window_pairs_work": (c_i64, [ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int]),
    "osz_window_pairs": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, ctypes.c_int, c_i64, c_i64, ctypes.c_int,
                                        ctypes.c_int, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "osz_window_fractal": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                          c_vp, ctypes.c_int, c_vp, c_i64, c_i64, c_i64, c_vp]),
    "osz_window_wavelet": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, c_vp,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_i64, c_i64,
                                          c_vp]),
    "osz_window_ar": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, c_vp, c_i64, c_i64, c_i64, c_vp]),
    "osz_window_xcorr_work": (c_i64, [ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int]),
    "osz_window_xcorr": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "osz_window_granger_work": (c_i64, [ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int]),
    "osz_window_granger": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                          c_vp, c_i64, c_vp, c_i64, c_vp]),
    "osz_window_mi_work": (c_i64, [ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int]),
    "osz_window_mi": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "osz_window_te_work": (c_i64, [ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "osz_window_te": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "osz_window_coherence_work": (c_i64, [c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int]),
    "osz_window_coherence": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp,
                                            ctypes.c_int, ctypes.c_int, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "osz_simpson": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_i64, ctypes.c_double,
                                   c_vp, c_vp]),
    "osz_host_copy2d": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i64]),
    "osz_take": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_vp, c_i64, c_vp,
                                c_i64, c_vp]),
    "osz_edf_decode": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp,
                                      c_vp, c_vp, c_i64, c_i64, c_i64, ctypes.c_double,
                                      c_vp, c_i64, c_vp]),
    "osz_edf_encode": (ctypes.c_int, [c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, ctypes.c_int,
                                      c_vp, c_vp, c_vp, c_vp, ctypes.c_int, c_i64, c_vp, c_vp,
                                      c_vp]),
    "osz_synth_normal": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64,
                                        ctypes.c_uint64, c_i64, c_i64, c_vp]),
    "osz_checksum": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64,
                                    ctypes.POINTER(ctypes.c_uint64),
                                    ctypes.POINTER(ctypes.c_double), c_vp]),
}

_lib = None


def build(verbose=False):
    """Compile libosz_hip.so for gfx950 with hipcc (make in csrc/)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode:
        raise OszLibraryError("building libosz_hip.so failed")


def load():
    """Returns the loaded library with argtypes set; raises OszLibraryError
    if it is absent -- there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OszLibraryError(
            f"{LIB_PATH} not found: build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc, gfx950). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise OszLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


_EXC = {OSZ_ERR_INVALID: ValueError, OSZ_ERR_HIP: RuntimeError,
        OSZ_ERR_NOMEM: MemoryError, OSZ_ERR_STATE: RuntimeError,
        OSZ_ERR_UNSUPPORTED: NotImplementedError}


def check(status):
    """Maps a C status code back to the Python exception types the reference
    raises at this boundary (SURVEY 8b 'Errors')."""
    if status == OSZ_OK:
        return
    msg = load().osz_last_error().decode("utf-8", "replace")
    raise _EXC.get(status, RuntimeError)(msg)
