"""ctypes binding of ``libqbp.so`` (C ABI: ``include/qbp.h``).

There is no CPU fallback: if the shared library is missing, or no MI355X is visible, every
entry point raises (``QbpError``) instead of computing something else.
"""
from __future__ import annotations

import ctypes as C
import functools
import importlib.util
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB_PATH = os.path.join(_HERE, "csrc", "libqbp.so")
LIB_PATH = os.environ.get("QBP_LIB_PATH") or _DEFAULT_LIB_PATH   # override: experiments

SUM_PRODUCT, DAMPED_SP, MIN_SUM = 0, 1, 2
FLAG_FORCE_FULL = 1
FLAG_OSD0 = 2
FLAG_PAIRWISE_COLSUM = 4     # np.sum order of the loop form (beliefPropagation.py:68)
FLAG_DENSE_F_COLSUM = 8      # np.sum(R, axis=0) order of the dense forms on a Fortran-ordered H (include/qbp.h)
FLAG_DENSE_F_COLSUM_ITER0 = 16   # ... at iteration 0 only (damped variants, F-ordered H below 256 KiB)
FLAG_FAST_MATH = 32          # opt-in: round 2's tanh / arctanh approximations on the on-chip kernel (include/qbp.h)
FLAG_OSD_CS = 64             # order-w OSD, combination sweep (qbp_osd_batch; with FLAG_OSD0 in qbp_mc_run)
FLAG_OSD_E = 128             # order-w OSD, exhaustive over the w least reliable non-pivot columns
FLAG_OSD_LARGE = 256         # order-w OSD also on matrices beyond the one-wavefront kernel (up to 8192 rows)
FLAG_RELAY = 512             # Monte-Carlo calls: Relay-BP (qbp_relay_configure) instead of OSD on the trials BP leaves
FLAG_LAYERED = 1024          # the layered (check-serial) schedule instead of flooding (qbp_layered_configure)
FLAG_GD = 2048               # Monte-Carlo calls: BP guided decimation (qbp_gd_configure) on the trials BP leaves
FLAG_LSD = 4096              # Monte-Carlo calls: localized statistics decoding (qbp_lsd_configure) on those trials
FLAG_QUANT = 8192            # Monte-Carlo calls: fixed-point min-sum (qbp_quant_configure) as the first stage
OSD_ORDER_SHIFT = 16         # QBP_OSD_ORDER_FLAGS(w) = w << 16
OSD_MAX_ORDER = {"cs": 64, "e": 12}
MC_OSD_MAX_TRIALS = 1 << 20
MC_MAX_BUDGETS = 16          # QBP_MC_MAX_BUDGETS: rows of one qbp_mc_run_budgets call
SPECTRUM_ROWS = 4            # QBP_SPECTRUM_ROWS: weights_found_BP, _OSD, _BP_error, _OSD_error (rework/main.py)
MC_SPECTRUM_MAX_ITER = 1024  # QBP_MC_SPECTRUM_MAX_ITER: iteration limit of qbp_mc_run_spectrum
LLR_HIST_ROWS = 4            # QBP_LLR_HIST_ROWS: 2 * (BP did not converge) + (the bit's true value)
LLR_HIST_MAX_WORDS = 8192    # QBP_LLR_HIST_MAX_WORDS: n_budgets * LLR_HIST_ROWS * (bins + 3) of one qbp_mc_run_llr_hist call
FAULT_WEIGHT_MAX = 256       # QBP_FAULT_WEIGHT_MAX: firing sites of one trial of qbp_mc_run_fault_weight
NUM_COUNTERS = 12
COUNTER_NAMES = ("trials", "logical_error", "BPs_fault", "BPs_miscorrected", "incorrectable",
                 "degenerateErrors", "not_converged", "sum_iterations",
                 "logical_error_not_converged", "exact_recoveries", "osd_invalid", "reserved1")
OPT_SLOTS_PER_BLOCK, OPT_BLOCKS_PER_CU, OPT_FORCE_GENERIC, OPT_KERNEL, OPT_GENERAL_THREADS, OPT_OSD_BIG, OPT_GENERAL_NO_LDS_TABLES, OPT_GENERAL_NO_R_SPLIT, OPT_GENERAL_MEM = 1, 2, 4, 5, 6, 7, 8, 9, 10
OPT_FORCED_TWO_BARRIERS = 11
OPT_NO_FIRST_STEP_TABLE = 12
OPT_EARLY_EXIT_FULL_WG = 13
OPT_MC_WEIGHT_CHUNK = 14     # qbp_mc_run_weight: trials sampled and decoded per chunk (0 = default)
OPT_LAYERED_SLOTS = 15       # layered BP: records decoded at once by one workgroup (0 = auto)
# Relay-BP, layered BP, BP guided decimation: where a record's messages live -- 0 LDS only, 1 global workspace, 2 automatic
OPT_RELAY_MEM, OPT_LAYERED_MEM, OPT_GD_MEM = 16, 17, 18
OPT_LSD_MEM = 19             # localized statistics decoding: where a record's rows live, the same three values
OPT_QUANT_SLOTS = 121        # fixed-point min-sum: records decoded at once by one workgroup (0 = auto)
OPT_LLR_HIST_CHUNK = 120     # qbp_mc_run_llr_hist: trials per launch (0 = default: the most 32-bit counts allow)
# family: (the option, ``large=`` -> its value, the accepted spellings in words).  ``relay.RelayConfig.large``,
# ``Decoder.layered_configure(large=)`` and ``gd.GDConfig.large`` spell the same three values differently (README.md);
# ``Decoder.lsd_configure(large=)`` spells them as Relay-BP does
MSG_MEM = {
    "relay":   (OPT_RELAY_MEM,   {False: 0, True: 2, "force": 1}, "False, True or 'force'"),
    "layered": (OPT_LAYERED_MEM, {False: 0, True: 2},             "False or True"),
    "gd":      (OPT_GD_MEM,      {False: 0, True: 1, "auto": 2},  "False, True or 'auto'"),
    "lsd":     (OPT_LSD_MEM,     {False: 0, True: 2, "force": 1}, "False, True or 'force'"),
}
RELAY_MEM, LAYERED_MEM, GD_MEM = (MSG_MEM[family][1] for family in ("relay", "layered", "gd"))


def msg_mem_value(family, large, spelled=None):
    """The option value of a family's ``large=``; ValueError for what the family does not accept (``spelled``: the
    accepted spellings in words, where the caller accepts more than the table)."""
    _, table, words = MSG_MEM[family]
    if not isinstance(large, (bool, str)) or large not in table:        # (1 == True: no plain lookup)
        raise ValueError(f"large must be {spelled or words}, got {large!r}")
    return table[large]


KERNEL_AUTO, KERNEL_ON_CHIP, KERNEL_GENERAL, KERNEL_STREAM = 0, 1, 2, 3
INFO = dict(m=100, n=101, edges=102, max_row_deg=103, max_col_deg=104, kernel_kind=105,
            threads=106, lds_bytes=107, grid=108, num_cu=109, last_kernel=110, one_barrier=111)

# every symbol include/qbp.h declares: (restype, argtypes)
_VP = C.c_void_p
SIGNATURES = {
    "qbp_create": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_VP)]),
    "qbp_destroy": (None, [_VP]),
    "qbp_plan": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "qbp_plan_r_layout": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP]),
    "qbp_column_order": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    "qbp_decode_batch": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                   C.c_double, C.c_double, C.c_uint32, _VP, _VP, _VP, _VP]),
    "qbp_decode_batch_device": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_double, C.c_double, C.c_double, C.c_uint32, _VP,
                                          _VP, _VP, _VP, _VP]),
    "qbp_mc_run": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_uint64,
                             C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double,
                             C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_mc_run_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                    C.c_uint64, C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32,
                                    C.c_double, C.c_double, C.c_double, C.c_uint32, _VP, _VP]),
    "qbp_mc_run_errors": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, C.c_int32, C.c_int32,
                                    C.c_double, C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_mc_sample_errors": (C.c_int, [_VP, C.c_double, C.c_int32, C.c_uint64, C.c_int64,
                                       C.c_int64, _VP]),
    "qbp_mc_run_probs": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_uint64,
                                   C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double,
                                   C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_mc_run_probs_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32,
                                          C.c_uint64, C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32,
                                          C.c_double, C.c_double, C.c_double, C.c_uint32, _VP, _VP]),
    "qbp_mc_run_budgets": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_uint64,
                                     C.c_int64, C.c_int64, _VP, _VP, C.c_int32, C.c_int32, C.c_double,
                                     C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_mc_run_budgets_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32,
                                            C.c_uint64, C.c_int64, C.c_int64, _VP, _VP, C.c_int32, C.c_int32,
                                            C.c_double, C.c_double, C.c_double, C.c_uint32, _VP, _VP]),
    "qbp_mc_run_llr_hist": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_uint64,
                                      C.c_int64, C.c_int64, _VP, _VP, C.c_int32, C.c_int32, C.c_double,
                                      C.c_double, C.c_double, C.c_uint32, C.c_double, C.c_double, C.c_int32, _VP, _VP]),
    "qbp_mc_run_llr_hist_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32,
                                             C.c_uint64, C.c_int64, C.c_int64, _VP, _VP, C.c_int32, C.c_int32,
                                             C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_double, C.c_double,
                                             C.c_int32, _VP, _VP, _VP]),
    "qbp_mc_run_errors_llr_hist": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, _VP, C.c_int32,
                                             C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_double,
                                             C.c_double, C.c_int32, _VP, _VP]),
    "qbp_mc_run_spectrum": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_uint64,
                                      C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double,
                                      C.c_double, C.c_double, C.c_uint32, _VP, _VP, _VP]),
    "qbp_mc_run_spectrum_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32,
                                             C.c_uint64, C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32,
                                             C.c_double, C.c_double, C.c_double, C.c_uint32, _VP, _VP, _VP, _VP]),
    "qbp_mc_run_errors_spectrum": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, C.c_int32,
                                             C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, _VP, _VP,
                                             _VP]),
    "qbp_decode_shots": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double,
                                   C.c_double, C.c_double, C.c_uint32, _VP, _VP, _VP]),
    "qbp_decode_shots_device": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.c_int64, _VP, C.c_int32, C.c_int32,
                                          C.c_double, C.c_double, C.c_double, C.c_uint32, _VP, _VP, _VP, _VP]),
    "qbp_mc_sample_errors_probs": (C.c_int, [_VP, _VP, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP]),
    "qbp_mc_run_weight": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int64,
                                    _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_mc_run_weight_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int64,
                                           C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                           C.c_double, C.c_uint32, _VP, _VP]),
    "qbp_mc_sample_errors_weight": (C.c_int, [_VP, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP]),
    "qbp_enum_count": (C.c_int, [C.c_int32, C.c_int32, _VP]),
    "qbp_mc_run_enum": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _VP, C.c_int32,
                                  C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_mc_run_enum_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _VP,
                                         C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, _VP,
                                         _VP]),
    "qbp_mc_sample_errors_enum": (C.c_int, [_VP, C.c_int32, C.c_int64, C.c_int64, _VP]),
    "qbp_enum_failures": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _VP, C.c_int32, C.c_int32,
                                    C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_int32, C.c_int64, _VP, _VP, _VP,
                                    _VP]),
    "qbp_enum_failures_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _VP, C.c_int32,
                                           C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_int32,
                                           C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "qbp_fault_table_set": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int64, _VP]),
    "qbp_mc_run_fault_weight": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int64,
                                          _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                          _VP]),
    "qbp_mc_run_fault_weight_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int64,
                                                 C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                 C.c_double, C.c_uint32, _VP, _VP]),
    "qbp_mc_sample_errors_fault_weight": (C.c_int, [_VP, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP]),
    "qbp_fault_weight_failures": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP,
                                            C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                            C.c_int32, C.c_int64, _VP, _VP, _VP, _VP]),
    "qbp_fault_weight_failures_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int64,
                                                   _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                                   C.c_uint32, C.c_int32, C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "qbp_check_messages": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                     C.c_double, C.c_int32, C.c_uint32, _VP]),
    "qbp_message_histograms": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                         C.c_double, C.c_int32, C.c_uint32, C.c_int32, _VP, _VP, _VP]),
    "qbp_osd0_batch": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "qbp_osd0_batch_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP]),
    "qbp_osd_batch": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, C.c_int64, _VP]),
    "qbp_osd_batch_device": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, C.c_int64, _VP, _VP]),
    "qbp_osd_batch_ordered": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "qbp_osd_batch_ordered_device": (C.c_int, [_VP, C.c_uint32, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP]),
    "qbp_relay_configure": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, C.c_double, C.c_double]),
    "qbp_relay_decode_batch": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "qbp_relay_decode_batch_device": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "qbp_gd_configure": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_double]),
    "qbp_gd_decode_batch": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "qbp_gd_decode_batch_device": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "qbp_lsd_configure": (C.c_int, [_VP, C.c_int32]),
    "qbp_lsd_batch": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP]),
    "qbp_lsd_batch_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "qbp_distance_search": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP, _VP, _VP,
                                      _VP]),
    "qbp_frame_create": (C.c_int, [C.c_int32, _VP, C.c_int64, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32,
                                   C.POINTER(_VP)]),
    "qbp_frame_destroy": (None, [_VP]),
    "qbp_frame_sample": (C.c_int, [_VP, _VP, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP, _VP]),
    "qbp_frame_sample_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, _VP, _VP, _VP]),
    "qbp_frame_faults": (C.c_int, [_VP, C.c_int64, C.c_int64, _VP, _VP]),
    "qbp_frame_faults_device": (C.c_int, [_VP, C.c_int64, C.c_int64, _VP, _VP, _VP]),
    "qbp_frame_set_option": (C.c_int, [_VP, C.c_int32, C.c_int64]),
    "qbp_frame_get_info": (C.c_int64, [_VP, C.c_int32]),
    "qbp_layered_plan": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "qbp_layered_configure": (C.c_int, [_VP, _VP]),
    "qbp_quant_configure": (C.c_int, [_VP, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32]),
    "qbp_quant_decode_batch": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_uint32, _VP, _VP, _VP, _VP, _VP]),
    "qbp_quant_decode_batch_device": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_uint32, _VP, _VP, _VP, _VP, _VP,
                                                _VP]),
    "qbp_window_plan": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                  _VP]),
    "qbp_window_create": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(_VP)]),
    "qbp_window_destroy": (None, [_VP]),
    "qbp_window_decode_batch": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                          C.c_double, C.c_uint32, _VP, _VP, _VP, _VP, _VP]),
    "qbp_window_decode_batch_device": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                 C.c_double, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "qbp_window_mc_run_probs": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_uint64, C.c_int64,
                                          C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                          C.c_uint32, _VP]),
    "qbp_window_mc_run_probs_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_uint64, C.c_int64,
                                                 C.c_int64, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                 C.c_double, C.c_uint32, _VP, _VP]),
    "qbp_window_mc_run_errors": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, C.c_int32, C.c_int32,
                                           C.c_double, C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_window_get_info": (C.c_int64, [_VP, C.c_int32, C.c_int32]),
    "qbp_window_set_option": (C.c_int, [_VP, C.c_int32, C.c_int64]),
    "qbp_decode_batch_cond": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                        C.c_uint32, _VP, _VP, _VP, _VP]),
    "qbp_decode_batch_cond_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                               C.c_double, C.c_uint32, _VP, _VP, _VP, _VP, _VP]),
    "qbp_css_create": (C.c_int, [_VP, _VP, C.POINTER(_VP)]),
    "qbp_css_destroy": (None, [_VP]),
    "qbp_css_set_option": (C.c_int, [_VP, C.c_int32, C.c_int64]),
    "qbp_css_sample_errors": (C.c_int, [_VP, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.c_int64, _VP,
                                        _VP]),
    "qbp_css_decode_batch": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_double,
                                       C.c_double, C.c_double, C.c_uint32, _VP, _VP, _VP, _VP]),
    "qbp_css_mc_run": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                 C.c_uint64, C.c_int64, C.c_int64, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_double,
                                 C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_css_mc_run_errors": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, C.c_int32, _VP, _VP, C.c_int64, _VP, _VP, _VP,
                                        C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_uint32, _VP]),
    "qbp_set_option": (C.c_int, [_VP, C.c_int32, C.c_int64]),
    "qbp_get_info": (C.c_int64, [_VP, C.c_int32]),
    "qbp_debug_math": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int64]),
    "qbp_last_error": (C.c_char_p, []),
    "qbp_version": (C.c_char_p, []),
}


def osd_flags(method="cs", order=0, large=False):
    """Flags of an OSD pass: order 0 -> ``FLAG_OSD0`` (OSD-0); order w >= 1 -> ``FLAG_OSD0 | FLAG_OSD_CS`` (method
    "cs", 1 <= w <= 64) or ``| FLAG_OSD_E`` ("e", 1 <= w <= 12) with the order in bits 16..23.  The same value
    serves ``Decoder.osd`` and the Monte-Carlo calls.  ``large``: ``| FLAG_OSD_LARGE``, order w >= 1 also on
    matrices beyond the one-wavefront OSD kernel; with order 0 a ValueError.  Raises ValueError for anything else."""
    m = str(method).lower()
    if m not in OSD_MAX_ORDER:
        raise ValueError(f"OSD method must be 'cs' or 'e', got {method!r}")
    if isinstance(order, bool) or int(order) != order:
        raise ValueError(f"OSD order must be an integer, got {order!r}")
    w = int(order)
    if w == 0:
        if large:
            raise ValueError("large=True needs an OSD order >= 1 (OSD-0 runs on every matrix)")
        return FLAG_OSD0
    if not 1 <= w <= OSD_MAX_ORDER[m]:
        raise ValueError(f"OSD-{m.upper()} order must be in [0, {OSD_MAX_ORDER[m]}], got {w}")
    return (FLAG_OSD0 | (FLAG_OSD_CS if m == "cs" else FLAG_OSD_E) | (w << OSD_ORDER_SHIFT)
            | (FLAG_OSD_LARGE if large else 0))


def check_budgets(budgets):
    """The ladder of ``qbp_mc_run_budgets`` as int32[K]: 1 <= K <= MC_MAX_BUDGETS integers >= 1, strictly ascending
    (ValueError otherwise -- the library refuses the same lists with QBP_E_INVALID)."""
    b = np.asarray(budgets)
    if b.ndim != 1 or not 1 <= b.size <= MC_MAX_BUDGETS:
        raise ValueError(f"budgets must be a list of 1 to {MC_MAX_BUDGETS} iteration limits, got {budgets!r}")
    if b.dtype.kind not in "iu" or np.any(b < 1) or np.any(b > np.iinfo(np.int32).max):
        raise ValueError(f"budgets must be integers >= 1, got {budgets!r}")
    if np.any(np.diff(b.astype(np.int64)) <= 0):
        raise ValueError(f"budgets must be strictly ascending, got {budgets!r}")
    return np.ascontiguousarray(b, np.int32)


def check_llr_hist(bins, lo, hi, n_budgets):
    """The table of ``qbp_mc_run_llr_hist`` as ``(bins, lo, hi)``: an integer ``bins`` >= 1, a finite range with
    lo < hi, and ``n_budgets * LLR_HIST_ROWS * (bins + 3)`` words within ``LLR_HIST_MAX_WORDS`` (ValueError otherwise
    -- the library refuses the same values with QBP_E_INVALID)."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
        raise ValueError(f"bins must be an integer >= 1, got {bins!r}")
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"the LLR range must be two numbers, got {(lo, hi)!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"the LLR range must be finite with lo < hi, got ({lo}, {hi})")
    words = int(n_budgets) * LLR_HIST_ROWS * (int(bins) + 3)
    if words > LLR_HIST_MAX_WORDS:
        raise ValueError(f"{n_budgets} budgets x {LLR_HIST_ROWS} rows x ({bins} bins + 3) = {words} words exceed "
                         f"LLR_HIST_MAX_WORDS = {LLR_HIST_MAX_WORDS}")
    return int(bins), lo, hi


def llr_hist_edges(bins, lo, hi):
    """The bin edges of ``qbp_mc_run_llr_hist``: ``np.linspace(lo, hi, bins + 1)``, as the library computes them."""
    return np.linspace(float(lo), float(hi), int(bins) + 1)


class QbpError(RuntimeError):
    """A libqbp call failed; ``code`` is the QBP_E_* value of include/qbp.h."""
    code = 0


E_INVALID = -1
E_UNSUPPORTED = -4


_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own ``libamdhip64.so.7``
    (plus a matching HSA runtime); the system ROCm has a library of the same SONAME.  Whichever is
    loaded first serves both libqbp and torch -- and torch cannot initialise on the system copy
    ("No HIP GPUs are available").  So if torch is installed (it need not be imported, and is not
    imported here), load its copy first; libqbp's DT_NEEDED entry then resolves to it."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _missing(name):
    def fn(*args):
        raise QbpError(f"{LIB_PATH} has no {name} (a build from before that entry point)")
    return fn


def load():
    """Load libqbp.so (built by ``__graft_entry__.build()`` / ``make -C qldpc_amd/csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QbpError(f"{LIB_PATH} is missing: build it with `python -c 'import "
                           f"__graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        _preload_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if (fn is None and (name.startswith(("qbp_window_", "qbp_quant_", "qbp_frame_")) or name == "qbp_plan_r_layout")
                    and LIB_PATH != _DEFAULT_LIB_PATH):
                # a QBP_LIB_PATH build from before sliding-window decoding (tools/bench_window.py times its
                # whole-matrix path), from before the variable-major message layout (A/B runs against it) or from
                # before fixed-point min-sum (tools/bench_quant.py times its double-precision rows on it), or from
                # before the Pauli-frame simulator (tools/bench_circuit.py times run_dem on it):
                # everything else works, such a call raises QbpError
                setattr(lib, name, _missing(name))
                continue
            if fn is None:
                raise AttributeError(f"{LIB_PATH} has no {name}: rebuild it")
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _check(rc):
    if rc != 0:
        err = QbpError(f"libqbp error {rc}: {load().qbp_last_error().decode()}")
        err.code = int(rc)
        raise err


def _ptr(a):
    return None if a is None else a.ctypes.data


def layered_plan(row_ptr, col_idx, m, n, order=None):
    """Host-only: the layered schedule of a CSR matrix (qbp_layered_plan) -> ``(order, level_ptr)``: the checks level
    after level and the level boundaries int32[n_levels + 1].  ``order``: a permutation of the checks, None = the
    default (greedy colouring, by colour then index)."""
    rp = np.ascontiguousarray(row_ptr, np.int32)
    ci = np.ascontiguousarray(col_idx, np.int32)
    if rp.shape != (int(m) + 1,):
        raise ValueError(f"row_ptr must have shape ({int(m) + 1},)")
    oin = None
    if order is not None:
        oin = np.ascontiguousarray(order, np.int32)
        if oin.shape != (int(m),):
            raise ValueError(f"order must have shape ({int(m)},), got {oin.shape}")
    out = np.zeros(int(m), np.int32)
    lptr = np.zeros(int(m) + 1, np.int32)
    nl = C.c_int32(0)
    _check(load().qbp_layered_plan(rp.ctypes.data, _ptr(ci), int(m), int(n), _ptr(oin), out.ctypes.data,
                                   lptr.ctypes.data, C.byref(nl)))
    return out, lptr[:nl.value + 1].copy()


def _locked(method):
    """Serialise the host-buffer entry points of one Decoder: a qbp_handle owns one set of device
    scratch buffers and one stream (include/qbp.h: "not thread-safe"), while the reference's
    functions are pure and may be called from a thread pool.  ctypes drops the GIL during the call,
    so without this two threads decoding the same matrix would share that scratch."""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return method(self, *args, **kwargs)
    return wrapper


WINDOW_INFO = dict(windows=1, classes=2, rounds=3)     # QBP_WINDOW_INFO_*


def _window_args(row_ptr, col_idx, m, n, check_round):
    rp = np.ascontiguousarray(row_ptr, np.int32)
    ci = np.ascontiguousarray(col_idx, np.int32)
    if rp.shape != (int(m) + 1,):
        raise ValueError(f"row_ptr must have shape ({int(m) + 1},)")
    cr = np.ascontiguousarray(check_round, np.int32)
    if cr.shape != (int(m),):
        raise ValueError(f"check_round must have shape ({int(m)},), got {cr.shape}")
    return rp, ci, cr


def window_plan(row_ptr, col_idx, m, n, check_round, W, F):
    """Host-only: the partition of sliding-window decoding (qbp_window_plan) as a dict -- ``K`` windows;
    ``check_ptr`` int32[K + 1] into ``checks``; ``var_ptr`` int32[K + 1] into ``vars``; ``commit`` uint8 per entry of
    ``vars``; ``cls`` int32[K], the class of identical local CSR of every window."""
    rp, ci, cr = _window_args(row_ptr, col_idx, m, n, check_round)
    lib = load()
    sizes = np.zeros(3, np.int32)
    head = (rp.ctypes.data, _ptr(ci), int(m), int(n), cr.ctypes.data, int(W), int(F), sizes.ctypes.data)
    _check(lib.qbp_window_plan(*head, None, None, None, None, None, None))
    K, nc, nv = (int(x) for x in sizes)
    out = dict(K=K, check_ptr=np.zeros(K + 1, np.int32), checks=np.zeros(nc, np.int32), var_ptr=np.zeros(K + 1, np.int32),
               vars=np.zeros(nv, np.int32), commit=np.zeros(nv, np.uint8), cls=np.zeros(K, np.int32))
    _check(lib.qbp_window_plan(*head, *(out[k].ctypes.data for k in ("check_ptr", "checks", "var_ptr", "vars", "commit",
                                                                      "cls"))))
    return out


class WindowDecoder:
    """Sliding-window decoder of one multi-round matrix on one GPU (wraps a ``qbp_window``; include/qbp.h states the
    rule).  Methods taking host arrays are serialised per object; the ``*_device`` methods only enqueue work."""

    def __init__(self, row_ptr, col_idx, m, n, check_round, W, F, device=0):
        self.row_ptr, self.col_idx, self.check_round = _window_args(row_ptr, col_idx, m, n, check_round)
        self.m, self.n, self.W, self.F = int(m), int(n), int(W), int(F)
        h = _VP()
        _check(load().qbp_window_create(self.row_ptr.ctypes.data, _ptr(self.col_idx), self.m, self.n,
                                        self.check_round.ctypes.data, self.W, self.F, int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._lock = threading.RLock()

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.qbp_window_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, what, index=0):
        """``what``: "windows", "classes", "rounds", or a key of ``INFO`` for the sub-handle of class ``index``."""
        code = WINDOW_INFO[what] if what in WINDOW_INFO else INFO[what]
        return int(load().qbp_window_get_info(self._h, code, int(index)))

    @_locked
    def set_option(self, option, value):
        _check(load().qbp_window_set_option(self._h, int(option), int(value)))

    @_locked
    def decode(self, syndromes, prior, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0,
               want_llr=True):
        """-> (correction uint8[B, n], converged bool[B], iters int32[B], llr float64[B, n] or None,
        window_fails int32[B]).  ``flags``: FLAG_FORCE_FULL and the OSD bits (``osd_flags``)."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m}), got {syn.shape}")
        pr = np.ascontiguousarray(prior, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},), got {pr.shape}")
        B = syn.shape[0]
        x = np.empty((B, self.n), np.uint8)
        conv = np.empty(B, np.uint8)
        iters = np.empty(B, np.int32)
        llr = np.empty((B, self.n), np.float64) if want_llr else None
        fails = np.empty(B, np.int32)
        _check(load().qbp_window_decode_batch(self._h, syn.ctypes.data, pr.ctypes.data, B, int(max_iter), int(variant),
                                              float(alpha), float(damping), float(clip_llr), int(flags), x.ctypes.data,
                                              conv.ctypes.data, iters.ctypes.data, _ptr(llr), fails.ctypes.data))
        return x, conv.astype(bool), iters, llr, fails

    def decode_device(self, d_syndromes, d_prior, B, max_iter, variant, alpha, damping, clip_llr, flags, d_correction,
                      d_converged, d_iters, d_llr, d_window_fails, stream=0):
        _check(load().qbp_window_decode_batch_device(
            self._h, d_syndromes, d_prior, int(B), int(max_iter), int(variant), float(alpha), float(damping),
            float(clip_llr), int(flags), d_correction or None, d_converged or None, d_iters or None, d_llr or None,
            d_window_fails or None, stream or None))

    def _lx(self, Lx):
        L = np.ascontiguousarray(Lx, np.uint8)
        if L.ndim != 2 or L.shape[1] != self.n:
            raise ValueError(f"Lx must have shape (k, {self.n}), got {L.shape}")
        return L

    @_locked
    def mc_run_probs(self, Lx, distance, probs, prior, trial_begin, trial_end, draws=1, seed=0, max_iter=50,
                     variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, counters=None):
        """qbp_window_mc_run_probs -> int64[12], ADDED to ``counters`` if given."""
        L = self._lx(Lx)
        pb = np.ascontiguousarray(probs, np.float64)
        pr = np.ascontiguousarray(prior, np.float64)
        if pb.shape != (self.n,) or pr.shape != (self.n,):
            raise ValueError(f"probs and prior must have shape ({self.n},)")
        cnt = np.zeros(NUM_COUNTERS, np.int64) if counters is None else counters
        _check(load().qbp_window_mc_run_probs(self._h, L.ctypes.data, L.shape[0], int(distance), pb.ctypes.data, int(draws),
                                              int(seed), int(trial_begin), int(trial_end), pr.ctypes.data, int(max_iter),
                                              int(variant), float(alpha), float(damping), float(clip_llr), int(flags),
                                              cnt.ctypes.data))
        return cnt

    def mc_run_probs_device(self, Lx, distance, probs, d_prior, trial_begin, trial_end, d_counters, draws=1, seed=0,
                            max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, stream=0):
        L = self._lx(Lx)
        pb = np.ascontiguousarray(probs, np.float64)
        if pb.shape != (self.n,):
            raise ValueError(f"probs must have shape ({self.n},)")
        _check(load().qbp_window_mc_run_probs_device(
            self._h, L.ctypes.data, L.shape[0], int(distance), pb.ctypes.data, int(draws), int(seed), int(trial_begin),
            int(trial_end), d_prior, int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr),
            int(flags), d_counters, stream or None))

    @_locked
    def mc_run_errors(self, Lx, distance, errors, prior, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
                      clip_llr=20.0, flags=0):
        """qbp_window_mc_run_errors -> int64[12] (SET)."""
        L = self._lx(Lx)
        err = np.ascontiguousarray(errors, np.uint8)
        if err.ndim != 2 or err.shape[1] != self.n:
            raise ValueError(f"errors must have shape (T, {self.n}), got {err.shape}")
        pr = np.ascontiguousarray(prior, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},), got {pr.shape}")
        cnt = np.zeros(NUM_COUNTERS, np.int64)
        _check(load().qbp_window_mc_run_errors(self._h, L.ctypes.data, L.shape[0], int(distance), err.ctypes.data,
                                               err.shape[0], pr.ctypes.data, int(max_iter), int(variant), float(alpha),
                                               float(damping), float(clip_llr), int(flags), cnt.ctypes.data))
        return cnt


FRAME_INFO = dict(qubits=0, sites=1, faults=2, records=3, detectors=4, observables=5, chunk_lanes=6, workspace_bytes=7,
                  chunks=8, classes=9)                 # QBP_FRAME_INFO_*
FRAME_OPT_CHUNK_LANES = 1


class FrameSim:
    """GPU Pauli-frame simulator of one circuit on one GPU (wraps a ``qbp_frame``; include/qbp.h states the rules).
    ``ops`` int32 [rows, 4]: (kind, q0, q1, rate class) per target or pair; detectors and observables as CSR lists of
    measurement-record indices (``circuit.Circuit`` builds all of it).  Methods taking host arrays are serialised per
    object; the ``*_device`` methods only enqueue work."""

    def __init__(self, nq, ops, det_ptr, det_idx, obs_ptr, obs_idx, device=0):
        self.ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 4)
        self.det_ptr, self.det_idx = np.ascontiguousarray(det_ptr, np.int32), np.ascontiguousarray(det_idx, np.int32)
        self.obs_ptr, self.obs_idx = np.ascontiguousarray(obs_ptr, np.int32), np.ascontiguousarray(obs_idx, np.int32)
        self.m, self.k = self.det_ptr.size - 1, self.obs_ptr.size - 1
        h = _VP()
        _check(load().qbp_frame_create(int(nq), _ptr(self.ops), self.ops.shape[0], _ptr(self.det_ptr), _ptr(self.det_idx),
                                       self.m, _ptr(self.obs_ptr), _ptr(self.obs_idx), self.k, int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._lock = threading.RLock()

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.qbp_frame_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, what):
        return int(load().qbp_frame_get_info(self._h, FRAME_INFO[what]))

    @_locked
    def set_option(self, option, value):
        _check(load().qbp_frame_set_option(self._h, int(option), int(value)))

    def _outputs(self, T, want_det, want_obs):
        det = np.zeros((int(T), (self.m + 7) // 8), np.uint8) if want_det else None
        obs = np.zeros(int(T), np.uint64) if want_obs else None
        return det, obs

    @_locked
    def sample(self, rates, T, seed=0, shot_begin=0, want_det=True, want_obs=True):
        """Shots ``shot_begin .. shot_begin + T - 1`` (qbp_frame_sample) -> ``(det_bits uint8 [T, ceil(m / 8)], masks
        uint64 [T])``; ``rates`` float64 per rate class."""
        r = np.ascontiguousarray(rates, np.float64)
        det, obs = self._outputs(T, want_det, want_obs)
        _check(load().qbp_frame_sample(self._h, r.ctypes.data, r.size, int(seed), int(shot_begin), int(T), _ptr(det),
                                       _ptr(obs)))
        return det, obs

    def sample_device(self, rates, T, d_det_bits, d_obs, seed=0, shot_begin=0, stream=0):
        """``sample`` into device buffers (pointers as ints, either may be 0), enqueued on ``stream``."""
        r = np.ascontiguousarray(rates, np.float64)
        _check(load().qbp_frame_sample_device(self._h, r.ctypes.data, r.size, int(seed), int(shot_begin), int(T),
                                              d_det_bits or None, d_obs or None, stream or None))

    @_locked
    def faults(self, fault_begin, T, want_det=True, want_obs=True):
        """Single faults ``fault_begin .. fault_begin + T - 1`` (qbp_frame_faults): the rows of ``sample``'s layout."""
        det, obs = self._outputs(T, want_det, want_obs)
        _check(load().qbp_frame_faults(self._h, int(fault_begin), int(T), _ptr(det), _ptr(obs)))
        return det, obs

    def faults_device(self, fault_begin, T, d_det_bits, d_obs, stream=0):
        _check(load().qbp_frame_faults_device(self._h, int(fault_begin), int(T), d_det_bits or None, d_obs or None,
                                              stream or None))


class CssDecoder:
    """Two-stage decoder of a CSS code under Pauli noise (wraps a ``qbp_css`` over two ``Decoder`` objects it keeps
    alive; include/qbp.h states the rule).  Sector A is ``dec_a`` (for the codes of codes/: Hx, which detects Z and Y),
    sector B ``dec_b`` (Hz: X and Y).  Methods are serialised per object and hold both decoders' locks."""

    def __init__(self, dec_a, dec_b):
        if dec_a.n != dec_b.n:
            raise ValueError(f"the two matrices have {dec_a.n} and {dec_b.n} columns")
        self.a, self.b = dec_a, dec_b
        self.n, self.ma, self.mb = dec_a.n, dec_a.m, dec_b.m
        h = _VP()
        _check(load().qbp_css_create(dec_a._h, dec_b._h, C.byref(h)))
        self._h = h
        self.device = dec_a.device
        self._lock = threading.RLock()

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.qbp_css_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, *args):
        with self._lock, self.a._lock, self.b._lock:
            _check(fn(self._h, *args))

    def set_option(self, option, value):
        self._call(load().qbp_css_set_option, int(option), int(value))

    def _priors(self, *priors):
        out = [np.ascontiguousarray(p, np.float64) for p in priors]
        for p in out:
            if p.shape != (self.n,):
                raise ValueError(f"a prior must have shape ({self.n},), got {p.shape}")
        return out

    def _logicals(self, L):
        L = np.ascontiguousarray(L, np.uint8)
        if L.ndim != 2 or L.shape[1] != self.n:
            raise ValueError(f"logical operators must have shape (k, {self.n}), got {L.shape}")
        return L

    def sample_errors(self, px, py, pz, trial_begin, T, seed=0):
        """qbp_css_sample_errors -> (errors_a, errors_b) uint8[T, n]: Z or Y, X or Y."""
        ea = np.empty((int(T), self.n), np.uint8)
        eb = np.empty((int(T), self.n), np.uint8)
        self._call(load().qbp_css_sample_errors, float(px), float(py), float(pz), int(seed), int(trial_begin), int(T),
                   ea.ctypes.data, eb.ctypes.data)
        return ea, eb

    def decode(self, syn_a, syn_b, prior_a, prior_b0, prior_b1, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
               clip_llr=20.0, flags=0):
        """qbp_css_decode_batch -> (x_a, x_b uint8[B, n], conv_a, conv_b bool[B])."""
        sa = np.ascontiguousarray(syn_a, np.uint8)
        sb = np.ascontiguousarray(syn_b, np.uint8)
        if sa.ndim != 2 or sa.shape[1] != self.ma or sb.shape != (sa.shape[0], self.mb):
            raise ValueError(f"syndromes must have shapes (B, {self.ma}) and (B, {self.mb}), got {sa.shape}, {sb.shape}")
        pa, p0, p1 = self._priors(prior_a, prior_b0, prior_b1)
        B = sa.shape[0]
        xa = np.empty((B, self.n), np.uint8)
        xb = np.empty((B, self.n), np.uint8)
        ca = np.empty(B, np.uint8)
        cb = np.empty(B, np.uint8)
        self._call(load().qbp_css_decode_batch, sa.ctypes.data, sb.ctypes.data, B, pa.ctypes.data, p0.ctypes.data,
                   p1.ctypes.data, int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr), int(flags),
                   xa.ctypes.data, xb.ctypes.data, ca.ctypes.data, cb.ctypes.data)
        return xa, xb, ca.astype(bool), cb.astype(bool)

    def mc_run(self, La, Lb, distance, px, py, pz, prior_a, prior_b0, prior_b1, trial_begin, trial_end, seed=0, max_iter=50,
               variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, counters=None):
        """qbp_css_mc_run -> int64[3, 12] (sector A, sector B, the trial), ADDED to ``counters`` if given."""
        La, Lb = self._logicals(La), self._logicals(Lb)
        pa, p0, p1 = self._priors(prior_a, prior_b0, prior_b1)
        cnt = np.zeros((3, NUM_COUNTERS), np.int64) if counters is None else counters
        self._call(load().qbp_css_mc_run, La.ctypes.data, La.shape[0], Lb.ctypes.data, Lb.shape[0], int(distance),
                   float(px), float(py), float(pz), int(seed), int(trial_begin), int(trial_end), pa.ctypes.data,
                   p0.ctypes.data, p1.ctypes.data, int(max_iter), int(variant), float(alpha), float(damping),
                   float(clip_llr), int(flags), cnt.ctypes.data)
        return cnt

    def mc_run_errors(self, La, Lb, distance, errors_a, errors_b, prior_a, prior_b0, prior_b1, max_iter=50,
                      variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        """qbp_css_mc_run_errors -> int64[3, 12] (SET)."""
        La, Lb = self._logicals(La), self._logicals(Lb)
        ea = np.ascontiguousarray(errors_a, np.uint8)
        eb = np.ascontiguousarray(errors_b, np.uint8)
        if ea.ndim != 2 or ea.shape[1] != self.n or eb.shape != ea.shape:
            raise ValueError(f"errors must both have shape (T, {self.n}), got {ea.shape}, {eb.shape}")
        pa, p0, p1 = self._priors(prior_a, prior_b0, prior_b1)
        cnt = np.zeros((3, NUM_COUNTERS), np.int64)
        self._call(load().qbp_css_mc_run_errors, La.ctypes.data, La.shape[0], Lb.ctypes.data, Lb.shape[0], int(distance),
                   ea.ctypes.data, eb.ctypes.data, ea.shape[0], pa.ctypes.data, p0.ctypes.data, p1.ctypes.data,
                   int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr), int(flags), cnt.ctypes.data)
        return cnt


class Decoder:
    """One parity-check matrix on one GPU (wraps a ``qbp_handle``).  Methods taking host arrays
    are serialised per Decoder (thread-safe); the ``*_device`` methods only enqueue work on the
    caller's stream and are ordered by the caller."""

    def __init__(self, row_ptr, col_idx, m, n, device=0):
        lib = load()
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        self.col_idx = np.ascontiguousarray(col_idx, np.int32)
        self.m, self.n = int(m), int(n)
        h = _VP()
        _check(lib.qbp_create(self.row_ptr.ctypes.data, _ptr(self.col_idx), self.m, self.n,
                              int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._lock = threading.RLock()
        self._layered = None          # the order of the last layered_configure (bytes; b"" = default), None = none

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.qbp_destroy(h)

    def __del__(self):
        try:                      # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass

    def info(self, what):
        return int(load().qbp_get_info(self._h, INFO[what]))

    @_locked
    def set_option(self, option, value):
        _check(load().qbp_set_option(self._h, int(option), int(value)))

    def set_msg_mem(self, family, large, spelled=None):
        """Write a family's option of MSG_MEM from its ``large=`` (``msg_mem_value``)."""
        self.set_option(MSG_MEM[family][0], msg_mem_value(family, large, spelled))

    # ---- host buffers ----------------------------------------------------------------------
    @_locked
    def layered_configure(self, order=None, large=None):
        """Store the level tables of the layered schedule in the handle (qbp_layered_configure).  ``order``: a
        permutation of the checks, None = the default order.  ``large``: None leaves the handle's OPT_LAYERED_MEM as
        it is; False writes 0 (a record's state in LDS only: matrices beyond 160 KiB are refused); True writes 2
        (the messages in a global workspace where the LDS does not hold them)."""
        if large is not None:
            self.set_msg_mem("layered", large, "None, False or True")
        oin = None
        if order is not None:
            oin = np.ascontiguousarray(order, np.int32)
            if oin.shape != (self.m,):
                raise ValueError(f"order must have shape ({self.m},), got {oin.shape}")
        key = b"" if oin is None else oin.tobytes()
        if self._layered != key:
            self._layered = None
            _check(load().qbp_layered_configure(self._h, _ptr(oin)))
            self._layered = key

    @_locked
    def decode(self, syndromes, prior, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
               clip_llr=20.0, flags=0, want_llr=True, layered=False):
        """``layered``: True -- the layered schedule (FLAG_LAYERED) in the configured order, the default one if none
        was configured; an array -- in that order of the checks."""
        if layered is not False and layered is not None:
            if layered is True:
                if self._layered is None:
                    self.layered_configure(None)
            else:
                self.layered_configure(layered)
            flags = int(flags) | FLAG_LAYERED
        syn = np.ascontiguousarray(syndromes, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m}), got {syn.shape}")
        pr = np.ascontiguousarray(prior, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"initialBelief must have shape ({self.n},), got {pr.shape}")
        B = syn.shape[0]
        hard = np.empty((B, self.n), np.uint8)
        conv = np.empty(B, np.uint8)
        iters = np.empty(B, np.int32)
        llr = np.empty((B, self.n), np.float64) if want_llr else None
        _check(load().qbp_decode_batch(self._h, syn.ctypes.data, pr.ctypes.data, B, int(max_iter),
                                       int(variant), float(alpha), float(damping),
                                       float(clip_llr), int(flags), hard.ctypes.data,
                                       conv.ctypes.data, iters.ctypes.data, _ptr(llr)))
        return hard, conv.astype(bool), iters, llr

    @_locked
    def quant_configure(self, cfg):
        """Store a fixed-point min-sum configuration (``quant.QuantConfig``) in the handle (qbp_quant_configure)."""
        num, shift = cfg.alpha
        _check(load().qbp_quant_configure(self._h, int(cfg.bits), float(cfg.scale), int(num), int(shift), int(cfg.beta)))

    @_locked
    def quant_decode(self, syndromes, prior, max_iter=50, flags=0, want_posterior=True, want_llr=True):
        """qbp_quant_decode_batch in the stored configuration -> (hard, converged, iters, posterior_q int32[B, n] or
        None, llr float64[B, n] = posterior_q as doubles, or None)."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m}), got {syn.shape}")
        pr = np.ascontiguousarray(prior, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"initialBelief must have shape ({self.n},), got {pr.shape}")
        B = syn.shape[0]
        hard = np.empty((B, self.n), np.uint8)
        conv = np.empty(B, np.uint8)
        iters = np.empty(B, np.int32)
        post = np.empty((B, self.n), np.int32) if want_posterior else None
        llr = np.empty((B, self.n), np.float64) if want_llr else None
        _check(load().qbp_quant_decode_batch(self._h, syn.ctypes.data, pr.ctypes.data, B, int(max_iter), int(flags),
                                             hard.ctypes.data, conv.ctypes.data, iters.ctypes.data, _ptr(post), _ptr(llr)))
        return hard, conv.astype(bool), iters, post, llr

    def quant_decode_device(self, d_syndromes, d_prior, B, max_iter, flags, d_hard, d_converged, d_iters, d_posterior_q,
                            d_llr, stream=0):
        _check(load().qbp_quant_decode_batch_device(
            self._h, d_syndromes, d_prior, int(B), int(max_iter), int(flags), d_hard or None, d_converged or None,
            d_iters or None, d_posterior_q or None, d_llr or None, stream or None))

    # ---- device buffers (raw pointers, e.g. torch tensors' data_ptr()) ----------------------
    def decode_device(self, d_syndromes, d_prior, B, max_iter, variant, alpha, damping, clip_llr,
                      flags, d_hard, d_converged, d_iters, d_llr, stream=0):
        _check(load().qbp_decode_batch_device(
            self._h, d_syndromes, d_prior, int(B), int(max_iter), int(variant), float(alpha),
            float(damping), float(clip_llr), int(flags), d_hard or None, d_converged or None,
            d_iters or None, d_llr or None, stream or None))

    @_locked
    def decode_cond(self, syndromes, sel, prior0, prior1, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, clip_llr=20.0,
                    flags=0, want_llr=True):
        """qbp_decode_batch_cond: record b decodes with ``np.where(sel[b] & 1, prior1, prior0)`` as its prior ->
        (hard, converged, iters, llr or None) with ``decode``'s meaning."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m}), got {syn.shape}")
        B = syn.shape[0]
        sl = np.ascontiguousarray(sel, np.uint8)
        if sl.shape != (B, self.n):
            raise ValueError(f"sel must have shape ({B}, {self.n}), got {sl.shape}")
        p0 = np.ascontiguousarray(prior0, np.float64)
        p1 = np.ascontiguousarray(prior1, np.float64)
        if p0.shape != (self.n,) or p1.shape != (self.n,):
            raise ValueError(f"prior0 and prior1 must have shape ({self.n},)")
        hard = np.empty((B, self.n), np.uint8)
        conv = np.empty(B, np.uint8)
        iters = np.empty(B, np.int32)
        llr = np.empty((B, self.n), np.float64) if want_llr else None
        _check(load().qbp_decode_batch_cond(self._h, syn.ctypes.data, sl.ctypes.data, p0.ctypes.data, p1.ctypes.data, B,
                                            int(max_iter), int(variant), float(alpha), float(clip_llr), int(flags),
                                            hard.ctypes.data, conv.ctypes.data, iters.ctypes.data, _ptr(llr)))
        return hard, conv.astype(bool), iters, llr

    def decode_cond_device(self, d_syndromes, d_sel, d_prior0, d_prior1, B, max_iter, variant, alpha, clip_llr, flags,
                           d_hard, d_converged, d_iters, d_llr, stream=0):
        _check(load().qbp_decode_batch_cond_device(
            self._h, d_syndromes, d_sel, d_prior0, d_prior1, int(B), int(max_iter), int(variant), float(alpha),
            float(clip_llr), int(flags), d_hard or None, d_converged or None, d_iters or None, d_llr or None,
            stream or None))

    @_locked
    def relay_configure(self, cfg):
        """Store a Relay-BP configuration (``relay.RelayConfig``) in the handle: OPT_RELAY_MEM from ``cfg.large``, then
        qbp_relay_configure."""
        if cfg.n != self.n:
            raise ValueError(f"the relay configuration is for {cfg.n} variables, the matrix has {self.n}")
        self.set_msg_mem("relay", cfg.large)
        _check(load().qbp_relay_configure(self._h, cfg.gammas.ctypes.data, cfg.gammas.shape[0],
                                          cfg.leg_iters.ctypes.data, cfg.stop_after, cfg.alpha, cfg.clip_llr))

    @_locked
    def relay_decode(self, syndromes, prior, cfg=None, want_llr=True):
        """Relay-BP of B syndromes (qbp_relay_decode_batch) -> ``(hard, converged, iters, llr, legs, solutions)``;
        ``cfg``: configure first (None: the handle's configuration)."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m}), got {syn.shape}")
        pr = np.ascontiguousarray(prior, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},), got {pr.shape}")
        if cfg is not None:
            self.relay_configure(cfg)
        B = syn.shape[0]
        hard = np.empty((B, self.n), np.uint8)
        conv = np.empty(B, np.uint8)
        iters, legs, sols = (np.empty(B, np.int32) for _ in range(3))
        llr = np.empty((B, self.n), np.float64) if want_llr else None
        _check(load().qbp_relay_decode_batch(self._h, syn.ctypes.data, pr.ctypes.data, B, hard.ctypes.data,
                                             conv.ctypes.data, iters.ctypes.data, _ptr(llr), legs.ctypes.data,
                                             sols.ctypes.data))
        return hard, conv.astype(bool), iters, llr, legs, sols

    def relay_decode_device(self, d_syndromes, d_prior, B, d_hard, d_converged, d_iters, d_llr, d_legs, d_solutions,
                            stream=0):
        """``relay_decode`` on device buffers (pointers as ints; outputs may be 0), enqueued on `stream`."""
        _check(load().qbp_relay_decode_batch_device(self._h, d_syndromes, d_prior, int(B), d_hard or None,
                                                    d_converged or None, d_iters or None, d_llr or None, d_legs or None,
                                                    d_solutions or None, stream or None))

    @_locked
    def gd_configure(self, cfg):
        """Store a BP guided decimation configuration (``gd.GDConfig``) in the handle: OPT_GD_MEM from ``cfg.large``,
        then qbp_gd_configure."""
        self.set_msg_mem("gd", cfg.large)
        _check(load().qbp_gd_configure(self._h, cfg.iters_per_round, cfg.max_rounds, cfg.decim_llr, cfg.variant,
                                       cfg.alpha, cfg.clip_llr))

    @_locked
    def gd_decode(self, syndromes, prior, cfg=None, want_llr=True):
        """BP guided decimation of B syndromes (qbp_gd_decode_batch) -> ``(hard, converged, iters, llr, rounds)``;
        ``cfg``: configure first (None: the handle's configuration)."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m}), got {syn.shape}")
        pr = np.ascontiguousarray(prior, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},), got {pr.shape}")
        if cfg is not None:
            self.gd_configure(cfg)
        B = syn.shape[0]
        hard = np.empty((B, self.n), np.uint8)
        conv = np.empty(B, np.uint8)
        iters, rounds = (np.empty(B, np.int32) for _ in range(2))
        llr = np.empty((B, self.n), np.float64) if want_llr else None
        _check(load().qbp_gd_decode_batch(self._h, syn.ctypes.data, pr.ctypes.data, B, hard.ctypes.data,
                                          conv.ctypes.data, iters.ctypes.data, _ptr(llr), rounds.ctypes.data))
        return hard, conv.astype(bool), iters, llr, rounds

    def gd_decode_device(self, d_syndromes, d_prior, B, d_hard, d_converged, d_iters, d_llr, d_rounds, stream=0):
        """``gd_decode`` on device buffers (pointers as ints; outputs may be 0), enqueued on `stream`."""
        _check(load().qbp_gd_decode_batch_device(self._h, d_syndromes, d_prior, int(B), d_hard or None,
                                                 d_converged or None, d_iters or None, d_llr or None, d_rounds or None,
                                                 stream or None))

    @_locked
    def lsd_configure(self, bits_per_step, large=False):
        """Store the bits_per_step of localized statistics decoding in the handle: OPT_LSD_MEM from ``large`` -- False
        the LDS kernel only, True the large build (rows in a global workspace) where the LDS kernel does not take the
        matrix, "force" the large build always --, then qbp_lsd_configure.  The option is rewritten on EVERY call: the
        default ``large=False`` puts back 0 whatever ``set_option(OPT_LSD_MEM, ...)`` wrote before (set the option
        after this call, or pass ``large``)."""
        self.set_msg_mem("lsd", large)
        _check(load().qbp_lsd_configure(self._h, int(bits_per_step)))

    @_locked
    def lsd(self, syndromes, llr, hard, bits_per_step=None, want_stats=True, large=False):
        """Localized statistics decoding of B decoder outputs (host arrays; qbp_lsd_batch) -> ``(solution uint8[B, n],
        stats int32[B, 4])``; ``bits_per_step``: configure first, with ``large`` as in ``lsd_configure``, which
        rewrites OPT_LSD_MEM (None: the handle's configuration and option stay, ``large`` is not looked at)."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        l = np.ascontiguousarray(llr, np.float64)
        hd = np.ascontiguousarray(hard, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m})")
        if l.shape != (syn.shape[0], self.n) or hd.shape != l.shape:
            raise ValueError(f"llr and hard must have shape ({syn.shape[0]}, {self.n})")
        if bits_per_step is not None:
            self.lsd_configure(bits_per_step, large)
        sol = np.empty_like(hd)
        stats = np.empty((syn.shape[0], 4), np.int32) if want_stats else None
        _check(load().qbp_lsd_batch(self._h, syn.ctypes.data, l.ctypes.data, hd.ctypes.data, syn.shape[0],
                                    sol.ctypes.data, _ptr(stats)))
        return sol, stats

    def lsd_device(self, d_syndromes, d_llr, d_hard, B, d_solution, d_stats=0, stream=0):
        """``lsd`` on device buffers (pointers as ints; d_stats may be 0), enqueued on `stream`."""
        _check(load().qbp_lsd_batch_device(self._h, d_syndromes, d_llr, d_hard, int(B), d_solution, d_stats or None,
                                           stream or None))

    @_locked
    def distance_search(self, G, L, trial_begin, trial_end, seed=0, hist=None, want_codeword=True):
        """Randomized information-set search over ker H for the lightest vector a row of ``L`` detects
        (qbp_distance_search; include/qbp.h states the trial).  ``G`` uint8[r, n]: rows of ker H (the library checks
        them); ``L`` uint8[k, n], 1 <= k <= 64.  Returns ``(result int64[4], hist int64[n + 1], codeword uint8[n] or
        None, logical_mask int or None)``: result = (trials run, smallest weight or -1, the first trial that reached
        it, its row); ``hist`` is added to when given (in place), else starts from zero; the last two are None when
        no trial had a result or ``want_codeword`` is False."""
        G = np.ascontiguousarray(G, np.uint8)
        L = np.ascontiguousarray(L, np.uint8)
        if G.ndim != 2 or G.shape[1] != self.n:
            raise ValueError(f"G must have shape (r, {self.n}), got {G.shape}")
        if L.ndim != 2 or L.shape[1] != self.n:
            raise ValueError(f"L must have shape (k, {self.n}), got {L.shape}")
        if hist is None:
            hist = np.zeros(self.n + 1, np.int64)
        elif not (isinstance(hist, np.ndarray) and hist.dtype == np.int64 and hist.shape == (self.n + 1,)
                  and hist.flags.c_contiguous):
            raise ValueError(f"hist must be a contiguous int64 array of shape ({self.n + 1},)")
        result = np.zeros(4, np.int64)
        codeword = np.zeros(self.n, np.uint8) if want_codeword else None
        mask = np.zeros(1, np.uint64) if want_codeword else None
        _check(load().qbp_distance_search(self._h, G.ctypes.data, G.shape[0], L.ctypes.data, L.shape[0],
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(trial_begin), int(trial_end),
                                          result.ctypes.data, hist.ctypes.data, _ptr(codeword), _ptr(mask)))
        if not want_codeword or result[1] < 0:
            return result, hist, None, None
        return result, hist, codeword, int(mask[0])

    def mc_osd_step(self):
        """Trials one qbp_mc_run call may cover with FLAG_OSD0, FLAG_RELAY, FLAG_GD or FLAG_LSD (per-trial records:
        m + 10 n bytes)."""
        return max(1, min(MC_OSD_MAX_TRIALS, (8 << 30) // (self.m + 10 * self.n)))

    def mc_step(self, flags, whole, n_budgets=1):
        """Trials one Monte-Carlo or shot call may cover: with FLAG_OSD0, FLAG_RELAY, FLAG_GD or FLAG_LSD it keeps
        per-trial records, ``n_budgets`` of them in a ladder call, so ``mc_osd_step() // n_budgets`` (at least 1);
        without them ``whole``, the caller's whole range (at least 1: the value is the step of a ``range``)."""
        if int(flags) & (FLAG_OSD0 | FLAG_RELAY | FLAG_GD | FLAG_LSD):
            return max(1, self.mc_osd_step() // int(n_budgets))
        return max(1, int(whole))

    def _mc_sampled(self, fn, Lx, distance, source, trial_begin, trial_end, prior, limit, decoder, outputs, n_budgets=1,
                    after=()):
        """The host form ``fn`` of a sampled Monte-Carlo entry over [trial_begin, trial_end): ``source`` are its
        arguments between distance and the range, ``limit`` those between the prior and the variant, ``decoder`` is
        (variant, alpha, damping, clip_llr, flags), ``after`` the arguments between the flags and the outputs, and
        ``outputs`` the int64 arrays it adds to, which are returned."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        if Lx.ndim != 2 or Lx.shape[1] != self.n:
            raise ValueError(f"Lx must have shape (k, {self.n})")
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},)")
        variant, alpha, damping, clip_llr, flags = decoder
        begin, end = int(trial_begin), int(trial_end)
        step = self.mc_step(flags, end - begin, n_budgets)
        for a in range(begin, end, step):
            _check(getattr(load(), fn)(self._h, Lx.ctypes.data, Lx.shape[0], int(distance), *source, a, min(a + step, end),
                                       pr.ctypes.data, *limit, int(variant), float(alpha), float(damping),
                                       float(clip_llr), int(flags), *after, *(o.ctypes.data for o in outputs)))
        return outputs

    def _mc_stored(self, fn, Lx, distance, errors, prior, max_iter, decoder, tables=(), rows=None, after=(),
                   n_budgets=1):
        """The host form ``fn`` of a stored-error entry on error patterns uint8[T, n]: the counters, summed over the
        parts of a long list (a call SETS its counters); ``tables`` are added to by every part.  ``max_iter``: the
        limit, or the tuple of arguments that stands in its place (a ladder: budgets, their number) with ``rows``
        counter rows; ``after``: arguments between the flags and the counters."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        err = np.ascontiguousarray(errors, np.uint8)
        if Lx.ndim != 2 or Lx.shape[1] != self.n or pr.shape != (self.n,) or err.ndim != 2 or err.shape[1] != self.n:
            raise ValueError("bad shapes")
        variant, alpha, damping, clip_llr, flags = decoder
        shape = NUM_COUNTERS if rows is None else (int(rows), NUM_COUNTERS)
        limit = max_iter if isinstance(max_iter, tuple) else (int(max_iter),)
        total = np.zeros(shape, np.int64)
        step = self.mc_step(flags, len(err), n_budgets)
        for a in range(0, len(err), step):
            part = np.zeros(shape, np.int64)
            chunk = err[a:a + step]
            _check(getattr(load(), fn)(self._h, Lx.ctypes.data, Lx.shape[0], int(distance), chunk.ctypes.data, len(chunk),
                                       pr.ctypes.data, *limit, int(variant), float(alpha), float(damping),
                                       float(clip_llr), int(flags), *after, part.ctypes.data,
                                       *(t.ctypes.data for t in tables)))
            total += part
        return total

    @_locked
    def mc_run(self, Lx, distance, p, prior, trial_begin, trial_end, draws=1, seed=0, max_iter=50,
               variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        return self._mc_sampled("qbp_mc_run", Lx, distance, (float(p), int(draws), int(seed)), trial_begin, trial_end,
                                prior, (int(max_iter),), (variant, alpha, damping, clip_llr, flags),
                                [np.zeros(NUM_COUNTERS, np.int64)])[0]

    @_locked
    def mc_run_errors(self, Lx, distance, errors, prior, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
                      clip_llr=20.0, flags=0):
        """Counters int64[12] of the device pipeline (syndrome = H e, BP, [OSD-0,] classification) on GIVEN
        error patterns uint8[T, n] instead of sampled ones (qbp_mc_run_errors)."""
        return self._mc_stored("qbp_mc_run_errors", Lx, distance, errors, prior, max_iter,
                               (variant, alpha, damping, clip_llr, flags))

    def mc_run_device(self, Lx, distance, p, d_prior, trial_begin, trial_end, d_counters, draws=1,
                      seed=0, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
                      clip_llr=20.0, flags=0, stream=0):
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_mc_run_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), float(p), int(draws), int(seed),
            int(trial_begin), int(trial_end), d_prior, int(max_iter), int(variant), float(alpha),
            float(damping), float(clip_llr), int(flags), d_counters, stream or None))

    def _probs(self, probs):
        pr = np.ascontiguousarray(probs, np.float64)
        if pr.shape != (self.n,):
            raise ValueError(f"probs must have shape ({self.n},), got {pr.shape}")
        return pr

    @_locked
    def mc_run_probs(self, Lx, distance, probs, prior, trial_begin, trial_end, draws=1, seed=0, max_iter=50,
                     variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        """``mc_run`` with a probability per column (detector error models: qbp_mc_run_probs)."""
        probs = self._probs(probs)
        return self._mc_sampled("qbp_mc_run_probs", Lx, distance, (probs.ctypes.data, int(draws), int(seed)), trial_begin,
                                trial_end, prior, (int(max_iter),), (variant, alpha, damping, clip_llr, flags),
                                [np.zeros(NUM_COUNTERS, np.int64)])[0]

    def mc_run_probs_device(self, Lx, distance, probs, d_prior, trial_begin, trial_end, d_counters, draws=1,
                            seed=0, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
                            clip_llr=20.0, flags=0, stream=0):
        """``mc_run_device`` with a probability per column (host array; uploaded once, re-uploaded when it
        changes).  One call: with FLAG_OSD0 the caller splits ranges by ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        probs = self._probs(probs)
        _check(load().qbp_mc_run_probs_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), probs.ctypes.data, int(draws), int(seed),
            int(trial_begin), int(trial_end), d_prior, int(max_iter), int(variant), float(alpha),
            float(damping), float(clip_llr), int(flags), d_counters, stream or None))

    @_locked
    def mc_run_weight(self, Lx, distance, weight, prior, trial_begin, trial_end, seed=0, max_iter=50,
                      variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        """``mc_run`` on errors of exactly ``weight`` ones, uniform among the C(n, weight) patterns
        (qbp_mc_run_weight): counters int64[12] of trials [trial_begin, trial_end)."""
        return self._mc_sampled("qbp_mc_run_weight", Lx, distance, (int(weight), int(seed)), trial_begin, trial_end,
                                prior, (int(max_iter),), (variant, alpha, damping, clip_llr, flags),
                                [np.zeros(NUM_COUNTERS, np.int64)])[0]

    def mc_run_weight_device(self, Lx, distance, weight, d_prior, trial_begin, trial_end, d_counters, seed=0,
                             max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0,
                             stream=0):
        """``mc_run_weight`` on device buffers: d_counters int64[12] is added to.  One call: with FLAG_OSD0 the
        caller splits ranges by ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_mc_run_weight_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), int(weight), int(seed), int(trial_begin),
            int(trial_end), d_prior, int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr),
            int(flags), d_counters, stream or None))

    @_locked
    def mc_run_enum(self, Lx, distance, weight, prior, rank_begin, rank_end, max_iter=50, variant=SUM_PRODUCT,
                    alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        """``mc_run_weight`` on ENUMERATED patterns (qbp_mc_run_enum): counters int64[12] of the weight-``weight``
        patterns of ranks [rank_begin, rank_end) in the order of ``itertools.combinations(range(n), weight)``.
        [0] of the whole class is C(n, weight) and [1] / [0] its exact failure fraction."""
        return self._mc_sampled("qbp_mc_run_enum", Lx, distance, (int(weight),), rank_begin, rank_end, prior,
                                (int(max_iter),), (variant, alpha, damping, clip_llr, flags),
                                [np.zeros(NUM_COUNTERS, np.int64)])[0]

    def mc_run_enum_device(self, Lx, distance, weight, d_prior, rank_begin, rank_end, d_counters, max_iter=50,
                           variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, stream=0):
        """``mc_run_enum`` on device buffers: d_counters int64[12] is added to.  One call: with FLAG_OSD0 the
        caller splits ranges by ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_mc_run_enum_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), int(weight), int(rank_begin), int(rank_end), d_prior,
            int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr), int(flags), d_counters,
            stream or None))

    @_locked
    def enum_failures(self, Lx, weight, prior, rank_begin, rank_end, what=1, cap=1 << 20, max_iter=50,
                      variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, counters=None):
        """The failing patterns of ranks [rank_begin, rank_end) of weight ``weight`` (qbp_enum_failures): decoded as
        ``decode_shots`` decodes their syndromes, kind = (Lx x != Lx e) | 2 (BP did not converge); captured when
        ``kind & what`` (1 logical, 2 unconverged, 3 either).  Returns ``(ranks int64[F], kinds uint8[F], found,
        counters int64[12])`` with F = min(found, cap), ascending in rank when found <= cap; a given ``counters``
        array is added to."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        if Lx.ndim != 2 or Lx.shape[1] != self.n:
            raise ValueError(f"Lx must have shape (k, {self.n})")
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},)")
        if counters is None:
            counters = np.zeros(NUM_COUNTERS, np.int64)
        elif not (isinstance(counters, np.ndarray) and counters.dtype == np.int64 and
                  counters.shape == (NUM_COUNTERS,) and counters.flags.c_contiguous):
            raise ValueError(f"counters must be a C-contiguous int64 array of shape ({NUM_COUNTERS},)")
        cap = int(cap)
        room = max(0, min(cap, int(rank_end) - int(rank_begin)))       # (no more can be captured)
        ranks = np.zeros(room, np.int64)
        kinds = np.zeros(room, np.uint8)
        found = np.zeros(1, np.int64)
        _check(load().qbp_enum_failures(
            self._h, Lx.ctypes.data, Lx.shape[0], int(weight), int(rank_begin), int(rank_end), pr.ctypes.data,
            int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr), int(flags), int(what),
            cap if cap < 0 else room, ranks.ctypes.data if room else None, kinds.ctypes.data if room else None,
            found.ctypes.data, counters.ctypes.data))
        kept = min(int(found[0]), room)
        return ranks[:kept], kinds[:kept], int(found[0]), counters

    def enum_failures_device(self, Lx, weight, d_prior, rank_begin, rank_end, what, cap, d_ranks, d_kinds, d_found,
                             d_counters, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0,
                             flags=0, stream=0):
        """``enum_failures`` on device buffers (pointers as ints): d_ranks int64[cap] and d_kinds uint8[cap] in no
        particular order, d_found int64[1] and d_counters int64[12] added to."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_enum_failures_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(weight), int(rank_begin), int(rank_end), d_prior, int(max_iter),
            int(variant), float(alpha), float(damping), float(clip_llr), int(flags), int(what), int(cap),
            d_ranks or None, d_kinds or None, d_found or None, d_counters, stream or None))

    @_locked
    def fault_table_set(self, first_fault, K, fault_column):
        """The fault table of the fixed-weight fault sampler (qbp_fault_table_set): ``first_fault`` int64 [N] and ``K``
        [N] of the active sites (``circuit.fault_sites``), ``fault_column`` [faults] the column of every fault, -1 for
        one that flips nothing (``CircuitDem.fault_column``).  Replaces an earlier table; N = 0 clears it."""
        first = np.ascontiguousarray(first_fault, np.int64)
        k = np.ascontiguousarray(K, np.uint8)
        if first.ndim != 1 or k.shape != first.shape or not np.array_equal(k, np.asarray(K).ravel()):
            raise ValueError("first_fault and K must be one-dimensional, of one length, K within a byte")
        col = np.asarray(fault_column)
        if col.ndim != 1 or np.any(col < -1) or np.any(col >= self.n):
            raise ValueError(f"fault_column must be one-dimensional with entries in [-1, {self.n})")
        col = np.ascontiguousarray(col, np.int32)
        _check(load().qbp_fault_table_set(self._h, first.size, first.ctypes.data, k.ctypes.data, col.size,
                                          col.ctypes.data))

    @_locked
    def mc_run_fault_weight(self, Lx, distance, weight, prior, trial_begin, trial_end, seed=0, max_iter=50,
                            variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        """``mc_run_weight`` on exactly ``weight`` firing fault sites of the table of ``fault_table_set``, uniform among
        the site sets, each with one of its codes (qbp_mc_run_fault_weight): counters int64[12] of trials
        [trial_begin, trial_end)."""
        return self._mc_sampled("qbp_mc_run_fault_weight", Lx, distance, (int(weight), int(seed)), trial_begin,
                                trial_end, prior, (int(max_iter),), (variant, alpha, damping, clip_llr, flags),
                                [np.zeros(NUM_COUNTERS, np.int64)])[0]

    def mc_run_fault_weight_device(self, Lx, distance, weight, d_prior, trial_begin, trial_end, d_counters, seed=0,
                                   max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0,
                                   stream=0):
        """``mc_run_fault_weight`` on device buffers: d_counters int64[12] is added to.  One call: with FLAG_OSD0 the
        caller splits ranges by ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_mc_run_fault_weight_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), int(weight), int(seed), int(trial_begin),
            int(trial_end), d_prior, int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr),
            int(flags), d_counters, stream or None))

    @_locked
    def fault_weight_failures(self, Lx, weight, prior, trial_begin, trial_end, seed=0, what=1, cap=1 << 20, max_iter=50,
                              variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, counters=None):
        """The failing trials of [trial_begin, trial_end) of a fixed-weight fault run (qbp_fault_weight_failures):
        ``enum_failures`` with the fault sampler as the filler.  Returns ``(trials int64[F], kinds uint8[F], found,
        counters int64[12])`` with F = min(found, cap), ascending when found <= cap; ``circuit.fault_sets`` names the
        faults of a trial."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        if Lx.ndim != 2 or Lx.shape[1] != self.n:
            raise ValueError(f"Lx must have shape (k, {self.n})")
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},)")
        if counters is None:
            counters = np.zeros(NUM_COUNTERS, np.int64)
        elif not (isinstance(counters, np.ndarray) and counters.dtype == np.int64 and
                  counters.shape == (NUM_COUNTERS,) and counters.flags.c_contiguous):
            raise ValueError(f"counters must be a C-contiguous int64 array of shape ({NUM_COUNTERS},)")
        cap = int(cap)
        room = max(0, min(cap, int(trial_end) - int(trial_begin)))       # (no more can be captured)
        trials = np.zeros(room, np.int64)
        kinds = np.zeros(room, np.uint8)
        found = np.zeros(1, np.int64)
        _check(load().qbp_fault_weight_failures(
            self._h, Lx.ctypes.data, Lx.shape[0], int(weight), int(seed), int(trial_begin), int(trial_end),
            pr.ctypes.data, int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr), int(flags),
            int(what), cap if cap < 0 else room, trials.ctypes.data if room else None,
            kinds.ctypes.data if room else None, found.ctypes.data, counters.ctypes.data))
        kept = min(int(found[0]), room)
        return trials[:kept], kinds[:kept], int(found[0]), counters

    def fault_weight_failures_device(self, Lx, weight, d_prior, trial_begin, trial_end, what, cap, d_trials, d_kinds,
                                     d_found, d_counters, seed=0, max_iter=50, variant=SUM_PRODUCT, alpha=1.0,
                                     damping=1.0, clip_llr=20.0, flags=0, stream=0):
        """``fault_weight_failures`` on device buffers (pointers as ints): d_trials int64[cap] and d_kinds uint8[cap] in
        no particular order, d_found int64[1] and d_counters int64[12] added to."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_fault_weight_failures_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(weight), int(seed), int(trial_begin), int(trial_end), d_prior,
            int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr), int(flags), int(what), int(cap),
            d_trials or None, d_kinds or None, d_found or None, d_counters, stream or None))

    def _spectrum_tables(self, max_iter, spectrum, iter_hist):
        """The two tables of the spectrum calls (new zeroed ones, or the caller's, which are added to)."""
        if int(max_iter) < 1:       # (beyond MC_SPECTRUM_MAX_ITER the library answers QBP_E_INVALID)
            raise ValueError(f"max_iter must be >= 1, got {max_iter}")
        if spectrum is None:
            spectrum = np.zeros((SPECTRUM_ROWS, self.n + 1), np.int64)
        if iter_hist is None:
            iter_hist = np.zeros(int(max_iter) + 1, np.int64)
        for name, a, shape in (("spectrum", spectrum, (SPECTRUM_ROWS, self.n + 1)),
                               ("iter_hist", iter_hist, (int(max_iter) + 1,))):
            if not (isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == shape and a.flags.c_contiguous):
                raise ValueError(f"{name} must be a C-contiguous int64 array of shape {shape}")
        return spectrum, iter_hist

    @_locked
    def mc_run_spectrum(self, Lx, distance, probs, prior, trial_begin, trial_end, draws=1, seed=0, max_iter=50,
                        variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, spectrum=None,
                        iter_hist=None):
        """``mc_run_probs`` plus two distributions (qbp_mc_run_spectrum): returns ``(counters int64[12], spectrum
        int64[4, n + 1], iter_hist int64[max_iter + 1])``.  Row r of ``spectrum`` is the histogram of residual
        weights of rework/main.py's list r (weights_found_BP, _OSD, _BP_error, _OSD_error); bin k of ``iter_hist``
        counts the trials first satisfied in iteration k, bin max_iter those BP did not converge on.  ``probs``: one
        probability per column, or a scalar p.  Given ``spectrum`` / ``iter_hist`` arrays are added to."""
        probs = self._probs(np.full(self.n, float(probs)) if np.ndim(probs) == 0 else probs)
        spectrum, iter_hist = self._spectrum_tables(max_iter, spectrum, iter_hist)
        return tuple(self._mc_sampled("qbp_mc_run_spectrum", Lx, distance, (probs.ctypes.data, int(draws), int(seed)),
                                      trial_begin, trial_end, prior, (int(max_iter),),
                                      (variant, alpha, damping, clip_llr, flags),
                                      [np.zeros(NUM_COUNTERS, np.int64), spectrum, iter_hist]))

    def mc_run_spectrum_device(self, Lx, distance, probs, d_prior, trial_begin, trial_end, d_counters, d_spectrum,
                               d_iter_hist=0, draws=1, seed=0, max_iter=50, variant=SUM_PRODUCT, alpha=1.0,
                               damping=1.0, clip_llr=20.0, flags=0, stream=0):
        """``mc_run_spectrum`` on device buffers: d_counters int64[12], d_spectrum int64[4, n + 1] and d_iter_hist
        int64[max_iter + 1] (0: none) are added to.  One call: with FLAG_OSD0 the caller splits ranges by
        ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        probs = self._probs(np.full(self.n, float(probs)) if np.ndim(probs) == 0 else probs)
        _check(load().qbp_mc_run_spectrum_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), probs.ctypes.data, int(draws), int(seed),
            int(trial_begin), int(trial_end), d_prior, int(max_iter), int(variant), float(alpha),
            float(damping), float(clip_llr), int(flags), d_counters, d_spectrum or None, d_iter_hist or None,
            stream or None))

    @_locked
    def mc_run_errors_spectrum(self, Lx, distance, errors, prior, max_iter=50, variant=SUM_PRODUCT, alpha=1.0,
                               damping=1.0, clip_llr=20.0, flags=0):
        """``mc_run_errors`` plus the two tables of ``mc_run_spectrum`` on GIVEN error patterns uint8[T, n]
        (qbp_mc_run_errors_spectrum): ``(counters, spectrum, iter_hist)``."""
        spectrum, iter_hist = self._spectrum_tables(max_iter, None, None)
        total = self._mc_stored("qbp_mc_run_errors_spectrum", Lx, distance, errors, prior, max_iter,
                                (variant, alpha, damping, clip_llr, flags), (spectrum, iter_hist))
        return total, spectrum, iter_hist

    @_locked
    def decode_shots(self, Lx, det_bits, prior, actual=None, max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
                     clip_llr=20.0, flags=0, counters=None):
        """Decode recorded shots to observable predictions (qbp_decode_shots).  ``det_bits`` uint8[T, ceil(m / 8)]:
        detection events in stim's b8 layout (``shots.pack_bits``); ``actual`` uint64[T] or None: the recorded
        observables, bit l = observable l (``shots.masks_of``); ``Lx`` uint8[k, n], 1 <= k <= 64.  Returns
        ``(counters int64[12], predictions uint64[T], converged bool[T])``; a given ``counters`` array is added to.
        With FLAG_OSD0 a call keeps per-shot records: T is split by ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        det = np.ascontiguousarray(det_bits, np.uint8)
        rb = (self.m + 7) // 8
        if Lx.ndim != 2 or Lx.shape[1] != self.n:
            raise ValueError(f"Lx must have shape (k, {self.n})")
        if pr.shape != (self.n,):
            raise ValueError(f"prior must have shape ({self.n},)")
        if det.ndim != 2 or det.shape[1] != rb:
            raise ValueError(f"det_bits must have shape (T, {rb}) (bit-packed rows of {self.m} detectors), "
                             f"got {det.shape}")
        T = det.shape[0]
        act = None
        if actual is not None:
            act = np.ascontiguousarray(actual, np.uint64)
            if act.shape != (T,):
                raise ValueError(f"actual must have shape ({T},), got {act.shape}")
        if counters is None:
            counters = np.zeros(NUM_COUNTERS, np.int64)
        elif not (isinstance(counters, np.ndarray) and counters.dtype == np.int64 and
                  counters.shape == (NUM_COUNTERS,) and counters.flags.c_contiguous):
            raise ValueError(f"counters must be a C-contiguous int64 array of shape ({NUM_COUNTERS},)")
        pred = np.zeros(T, np.uint64)
        conv = np.zeros(T, np.uint8)
        step = self.mc_step(flags, T)
        for a in range(0, T, step):
            b = min(a + step, T)
            _check(load().qbp_decode_shots(
                self._h, Lx.ctypes.data, Lx.shape[0], det[a:b].ctypes.data, None if act is None else act[a:b].ctypes.data,
                b - a, pr.ctypes.data, int(max_iter), int(variant), float(alpha), float(damping), float(clip_llr),
                int(flags), pred[a:b].ctypes.data, conv[a:b].ctypes.data, counters.ctypes.data))
        return counters, pred, conv.astype(bool)

    def decode_shots_device(self, Lx, d_det_bits, d_actual, T, d_prior, d_predictions, d_converged, d_counters,
                            max_iter=50, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, stream=0):
        """``decode_shots`` on device buffers (pointers as ints; d_actual, d_predictions, d_converged may be 0):
        d_counters int64[12] is added to.  One call: with FLAG_OSD0 the caller splits by ``mc_osd_step()``."""
        Lx = np.ascontiguousarray(Lx, np.uint8)
        _check(load().qbp_decode_shots_device(
            self._h, Lx.ctypes.data, Lx.shape[0], d_det_bits, d_actual or None, int(T), d_prior, int(max_iter),
            int(variant), float(alpha), float(damping), float(clip_llr), int(flags), d_predictions or None,
            d_converged or None, d_counters, stream or None))

    def mc_budgets_step(self, n_budgets):
        """Trials one qbp_mc_run_budgets call may cover with FLAG_OSD0: the records are kept per budget."""
        return self.mc_step(FLAG_OSD0, 0, n_budgets)

    @_locked
    def mc_run_budgets(self, Lx, distance, probs, prior, budgets, trial_begin, trial_end, draws=1, seed=0,
                       variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0):
        """Counters int64[K, 12] of ONE pass over the trials: row j is ``mc_run_probs(..., max_iter=budgets[j])``
        (qbp_mc_run_budgets; ``probs``: one probability per column, or a scalar p for all of them)."""
        bud = check_budgets(budgets)
        probs = self._probs(np.full(self.n, float(probs)) if np.ndim(probs) == 0 else probs)
        return self._mc_sampled("qbp_mc_run_budgets", Lx, distance, (probs.ctypes.data, int(draws), int(seed)),
                                trial_begin, trial_end, prior, (bud.ctypes.data, len(bud)),
                                (variant, alpha, damping, clip_llr, flags),
                                [np.zeros((len(bud), NUM_COUNTERS), np.int64)], n_budgets=len(bud))[0]

    def mc_run_budgets_device(self, Lx, distance, probs, d_prior, budgets, trial_begin, trial_end, d_counters,
                              draws=1, seed=0, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0,
                              stream=0):
        """``mc_run_budgets`` on device buffers: d_counters int64[K, 12] is added to.  One call: with FLAG_OSD0 the
        caller splits ranges by ``mc_budgets_step(K)``."""
        bud = check_budgets(budgets)
        Lx = np.ascontiguousarray(Lx, np.uint8)
        probs = self._probs(np.full(self.n, float(probs)) if np.ndim(probs) == 0 else probs)
        _check(load().qbp_mc_run_budgets_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), probs.ctypes.data, int(draws), int(seed),
            int(trial_begin), int(trial_end), d_prior, bud.ctypes.data, len(bud), int(variant), float(alpha),
            float(damping), float(clip_llr), int(flags), d_counters, stream or None))

    def _llr_hist_table(self, n_budgets, bins, hist):
        """The table of the LLR-histogram calls (a new zeroed one, or the caller's, which is added to)."""
        shape = (int(n_budgets), LLR_HIST_ROWS, int(bins) + 3)
        if hist is None:
            return np.zeros(shape, np.int64)
        if not (isinstance(hist, np.ndarray) and hist.dtype == np.int64 and hist.shape == shape and hist.flags.c_contiguous):
            raise ValueError(f"hist must be a C-contiguous int64 array of shape {shape}")
        return hist

    @_locked
    def mc_run_llr_hist(self, Lx, distance, probs, prior, budgets, bins, llr_range, trial_begin, trial_end, draws=1,
                        seed=0, variant=SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, hist=None):
        """``mc_run_budgets`` plus the posterior-LLR histograms per budget (qbp_mc_run_llr_hist): returns ``(counters
        int64[K, 12], hist int64[K, 4, bins + 3])``.  ``hist[j, 2 * (not converged) + true bit, c]`` counts the
        posterior values of budget j in column c: 0 below ``llr_range[0]``, 1 .. bins the bins of ``np.histogram(x,
        bins, range=llr_range)``, bins + 1 above ``llr_range[1]``, bins + 2 NaN.  A given ``hist`` is added to."""
        bud = check_budgets(budgets)
        bins, lo, hi = check_llr_hist(bins, *llr_range, len(bud))
        probs = self._probs(np.full(self.n, float(probs)) if np.ndim(probs) == 0 else probs)
        hist = self._llr_hist_table(len(bud), bins, hist)
        return tuple(self._mc_sampled("qbp_mc_run_llr_hist", Lx, distance, (probs.ctypes.data, int(draws), int(seed)),
                                      trial_begin, trial_end, prior, (bud.ctypes.data, len(bud)),
                                      (variant, alpha, damping, clip_llr, flags),
                                      [np.zeros((len(bud), NUM_COUNTERS), np.int64), hist],
                                      n_budgets=len(bud), after=(lo, hi, bins)))

    def mc_run_llr_hist_device(self, Lx, distance, probs, d_prior, budgets, bins, llr_range, trial_begin, trial_end,
                               d_counters, d_hist, draws=1, seed=0, variant=SUM_PRODUCT, alpha=1.0, damping=1.0,
                               clip_llr=20.0, flags=0, stream=0):
        """``mc_run_llr_hist`` on device buffers: d_counters int64[K, 12] and d_hist int64[K, 4, bins + 3] are added
        to.  One call: with FLAG_OSD0 the caller splits ranges by ``mc_budgets_step(K)``."""
        bud = check_budgets(budgets)
        bins, lo, hi = check_llr_hist(bins, *llr_range, len(bud))
        Lx = np.ascontiguousarray(Lx, np.uint8)
        probs = self._probs(np.full(self.n, float(probs)) if np.ndim(probs) == 0 else probs)
        _check(load().qbp_mc_run_llr_hist_device(
            self._h, Lx.ctypes.data, Lx.shape[0], int(distance), probs.ctypes.data, int(draws), int(seed),
            int(trial_begin), int(trial_end), d_prior, bud.ctypes.data, len(bud), int(variant), float(alpha),
            float(damping), float(clip_llr), int(flags), lo, hi, bins, d_counters, d_hist or None, stream or None))

    @_locked
    def mc_run_errors_llr_hist(self, Lx, distance, errors, prior, budgets, bins, llr_range, variant=SUM_PRODUCT,
                               alpha=1.0, damping=1.0, clip_llr=20.0, flags=0, hist=None):
        """``mc_run_llr_hist`` on GIVEN error patterns uint8[T, n] (qbp_mc_run_errors_llr_hist): ``(counters int64[K,
        12], hist int64[K, 4, bins + 3])``."""
        bud = check_budgets(budgets)
        bins, lo, hi = check_llr_hist(bins, *llr_range, len(bud))
        hist = self._llr_hist_table(len(bud), bins, hist)
        total = self._mc_stored("qbp_mc_run_errors_llr_hist", Lx, distance, errors, prior, (bud.ctypes.data, len(bud)),
                                (variant, alpha, damping, clip_llr, flags), (hist,), rows=len(bud), after=(lo, hi, bins),
                                n_budgets=len(bud))
        return total, hist

    @_locked
    def check_messages(self, syndromes, prior, variant, alpha=1.0, damping=1.0, clip_llr=20.0,
                       iteration=0, flags=0):
        """Check->variable messages float64[B, E] (CSR edge order) after iteration `iteration`
        (`flags`: column-sum order of the iterations before it)."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        if syn.ndim != 2 or syn.shape[1] != self.m or pr.shape != (self.n,):
            raise ValueError("bad shapes")
        out = np.empty((syn.shape[0], len(self.col_idx)), np.float64)
        _check(load().qbp_check_messages(self._h, syn.ctypes.data, pr.ctypes.data, syn.shape[0],
                                         int(variant), float(alpha), float(damping),
                                         float(clip_llr), int(iteration), int(flags), out.ctypes.data))
        return out

    @_locked
    def message_histograms(self, syndromes, errors, prior, variant, alpha=1.0, damping=1.0,
                           clip_llr=20.0, iteration=0, bins=50, flags=0):
        """(edges float64[bins + 1], hist0 int64[bins], hist1 int64[bins]): the check->variable
        messages of `check_messages`, binned on the device by the true value of their bit."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        err = np.ascontiguousarray(errors, np.uint8)
        pr = np.ascontiguousarray(prior, np.float64)
        if syn.ndim != 2 or syn.shape[1] != self.m or err.shape != (syn.shape[0], self.n) or pr.shape != (self.n,):
            raise ValueError("bad shapes")
        edges = np.empty(int(bins) + 1, np.float64)
        h0 = np.empty(int(bins), np.int64)
        h1 = np.empty(int(bins), np.int64)
        _check(load().qbp_message_histograms(self._h, syn.ctypes.data, err.ctypes.data, pr.ctypes.data,
                                             syn.shape[0], int(variant), float(alpha), float(damping),
                                             float(clip_llr), int(iteration), int(flags), int(bins), edges.ctypes.data,
                                             h0.ctypes.data, h1.ctypes.data))
        return edges, h0, h1

    @_locked
    def osd0(self, syndromes, llr, hard):
        """OSD-0 on B decoder outputs (host arrays) -> solution uint8[B, n]."""
        syn = np.ascontiguousarray(syndromes, np.uint8)
        l = np.ascontiguousarray(llr, np.float64)
        hd = np.ascontiguousarray(hard, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m})")
        if l.shape != (syn.shape[0], self.n) or hd.shape != l.shape:
            raise ValueError(f"llr and hard must have shape ({syn.shape[0]}, {self.n})")
        sol = np.empty_like(hd)
        _check(load().qbp_osd0_batch(self._h, syn.ctypes.data, l.ctypes.data, hd.ctypes.data,
                                     syn.shape[0], sol.ctypes.data))
        return sol

    def osd0_device(self, d_syndromes, d_llr, d_hard, B, d_solution, stream=0):
        """OSD-0 on device buffers (pointers as ints), enqueued on `stream`."""
        _check(load().qbp_osd0_batch_device(self._h, d_syndromes, d_llr, d_hard, int(B), d_solution,
                                            stream or None))

    @_locked
    def osd(self, syndromes, llr, hard, method="cs", order=7, column_order=None, large=False):
        """Order-w OSD (include/qbp.h, qbp_osd_batch) on B decoder outputs (host arrays) -> solution
        uint8[B, n]; order 0 is OSD-0.  ``column_order`` int[B, n]: every record's columns from the least reliable
        on, a permutation of 0..n-1 per row (qbp_osd_batch_ordered); None: sorted by (|llr|, column).  ``large``:
        FLAG_OSD_LARGE, order >= 1 also on matrices beyond the one-wavefront kernel."""
        fl = osd_flags(method, order, large)
        syn = np.ascontiguousarray(syndromes, np.uint8)
        l = np.ascontiguousarray(llr, np.float64)
        hd = np.ascontiguousarray(hard, np.uint8)
        if syn.ndim != 2 or syn.shape[1] != self.m:
            raise ValueError(f"syndromes must have shape (B, {self.m})")
        if l.shape != (syn.shape[0], self.n) or hd.shape != l.shape:
            raise ValueError(f"llr and hard must have shape ({syn.shape[0]}, {self.n})")
        sol = np.empty_like(hd)
        if column_order is None:
            _check(load().qbp_osd_batch(self._h, fl, syn.ctypes.data, l.ctypes.data, hd.ctypes.data,
                                        syn.shape[0], sol.ctypes.data))
            return sol
        co = np.asarray(column_order)
        if co.dtype.kind not in "iu" or co.shape != l.shape:
            raise ValueError(f"column_order must be an integer array of shape ({syn.shape[0]}, {self.n})")
        if co.size and (co.min() < -2**31 or co.max() >= 2**31):   # (the cast to int32 must not wrap a value into
            raise ValueError("column_order entries do not fit int32")   # range; the library checks the rows)
        co = np.ascontiguousarray(co, np.int32)
        _check(load().qbp_osd_batch_ordered(self._h, fl, syn.ctypes.data, l.ctypes.data, hd.ctypes.data,
                                            co.ctypes.data, syn.shape[0], sol.ctypes.data))
        return sol

    def osd_device(self, d_syndromes, d_llr, d_hard, B, d_solution, method="cs", order=7, stream=0, d_order=0,
                   large=False):
        """Order-w OSD on device buffers (pointers as ints), enqueued on `stream`.  ``d_order``: int32[B, n] column
        orders on the device (qbp_osd_batch_ordered_device: not validated there), 0: sorted by (|llr|, column)."""
        if d_order:
            _check(load().qbp_osd_batch_ordered_device(self._h, osd_flags(method, order, large), d_syndromes, d_llr, d_hard,
                                                       d_order, int(B), d_solution, stream or None))
            return
        _check(load().qbp_osd_batch_device(self._h, osd_flags(method, order, large), d_syndromes, d_llr, d_hard, int(B),
                                           d_solution, stream or None))

    @_locked
    def mc_sample_errors(self, p, trial_begin, T, draws=1, seed=0):
        out = np.empty((int(T), self.n), np.uint8)
        _check(load().qbp_mc_sample_errors(self._h, float(p), int(draws), int(seed),
                                           int(trial_begin), int(T), out.ctypes.data))
        return out

    @_locked
    def mc_sample_errors_probs(self, probs, trial_begin, T, draws=1, seed=0):
        probs = self._probs(probs)
        out = np.empty((int(T), self.n), np.uint8)
        _check(load().qbp_mc_sample_errors_probs(self._h, probs.ctypes.data, int(draws), int(seed),
                                                 int(trial_begin), int(T), out.ctypes.data))
        return out

    @_locked
    def mc_sample_errors_weight(self, weight, trial_begin, T, seed=0):
        """Errors uint8[T, n] the sampler of ``mc_run_weight`` draws for trials trial_begin .. + T (tests)."""
        out = np.empty((int(T), self.n), np.uint8)
        _check(load().qbp_mc_sample_errors_weight(self._h, int(weight), int(seed), int(trial_begin), int(T),
                                                  out.ctypes.data))
        return out

    @_locked
    def mc_sample_errors_fault_weight(self, weight, trial_begin, T, seed=0):
        """Rows uint8[T, n] the sampler of ``mc_run_fault_weight`` fills for trials trial_begin .. + T (tests)."""
        out = np.empty((int(T), self.n), np.uint8)
        _check(load().qbp_mc_sample_errors_fault_weight(self._h, int(weight), int(seed), int(trial_begin), int(T),
                                                        out.ctypes.data))
        return out

    @_locked
    def mc_sample_errors_enum(self, weight, rank_begin, T):
        """Patterns uint8[T, n] of ranks rank_begin .. + T of weight ``weight``, as ``mc_run_enum`` fills them (tests)."""
        out = np.empty((int(T), self.n), np.uint8)
        _check(load().qbp_mc_sample_errors_enum(self._h, int(weight), int(rank_begin), int(T), out.ctypes.data))
        return out

    @_locked
    def debug_math(self, kind, x):
        x = np.ascontiguousarray(x, np.float64)
        y = np.empty_like(x)
        _check(load().qbp_debug_math(self._h, int(kind), x.ctypes.data, y.ctypes.data, x.size))
        return y
