"""ctypes binding of the C-ABI kernel library (include/dctn_amd.h).

The library is the product path.  There is deliberately NO fallback: if the shared object is
missing, or no MI355X is visible, the call raises (CPU tensors are staged to the GPU, see `placement`).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdctn_amd.so")
CSRC = os.path.join(_HERE, "csrc")

F32, F64, BF16 = 0, 1, 2
PREC_EXACT, PREC_BF16, PREC_SPLIT, PREC_MASK = 0, 1, 2, 0xFF
OPT_F32_PREFER_HALVES, OPT_SMALL_CHUNKS, OPT_MAIN_KERNEL_ONLY, OPT_GENERIC_KERNELS = 1 << 8, 1 << 9, 1 << 10, 1 << 11
OPT_HEAD_FEATURES_BLOCKED4 = 1 << 12   # dctn_eps_head_fwd / _bwd only: sample-blocked feature layout
ERR_BAD_SHAPE, ERR_BAD_DTYPE, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_LAUNCH, ERR_NULL = -1, -2, -3, -4, -5, -6
SAVED, PARTIAL = 1, 2   # positive success codes (include/dctn_amd.h)
# what dctn_eps_family answers (DCTN_EPS_FAMILY_*; -1: the shape or policy is invalid)
(EPS_FAMILY_GENERIC, EPS_FAMILY_Q2REG, EPS_FAMILY_BIGCORE_F32, EPS_FAMILY_HALVES, EPS_FAMILY_Q2REG_F32,
 EPS_FAMILY_BIGCORE_BF16X3) = range(6)
SBS_MATRIX_CORE_SWEEP = 1 << 8   # OR-ed into the dtype argument of the dctn_convsbs_* calls
SBS_WIDE_SWEEP = 1 << 9   # likewise: the backward on the wide family (convsbs_wide.hip) for any string it covers
# DCTN_BATCH_SRC_*: `src_kind` of dctn_batch_call_t; dctn_batch_draw / dctn_batch_gather take the first two
BATCH_SRC_U8_TABLE, BATCH_SRC_ROWS, BATCH_SRC_COLOUR = 0, 1, 2
BATCH_IDENTITY_ORDER, BATCH_PAD_TAIL = 1, 2  # `flags` of a draw
TRACE_HAS_REG, TRACE_HAS_GUARD, TRACE_HAS_ADAM, TRACE_HAS_SOURCE = 1, 2, 4, 8   # DCTN_TRACE_HAS_*: a record's `present`
AUG_HFLIP = 1   # DCTN_AUG_HFLIP: `aug_flags` of dctn_batch_draw_aug / dctn_batch_draw_cols_aug

_DTYPE_CODE = {torch.float32: F32, torch.float64: F64, torch.bfloat16: BF16}

c_int, c_i64, c_void, c_size = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
c_u32 = ctypes.c_uint32
_I64x5 = ctypes.POINTER(c_i64)
_I64P = ctypes.POINTER(c_i64)
_IntP = ctypes.POINTER(c_int)
_PtrP = ctypes.POINTER(c_void)


class FlatStep(ctypes.Structure):
    """dctn_flat_step_t: every buffer and block of one flat-optimizer step; an option that is off is None (NULL)."""
    _fields_ = [("params", c_void), ("master", c_void), ("grads", c_void), ("sq_sum", c_void), ("state", c_void),
                ("guard", c_void), ("schedule", c_void), ("groups", c_void), ("n", c_i64), ("n_reg", c_i64),
                ("l2", ctypes.c_float), ("dtype", c_int)]


_FlatStepP = ctypes.POINTER(FlatStep)


class WeightEma(ctypes.Structure):
    """dctn_weight_ema_t: the n float32 averages and the 32-byte block of a weight average, both device pointers."""
    _fields_ = [("ema", c_void), ("block", c_void)]


_WeightEmaP = ctypes.POINTER(WeightEma)


class BatchCall(ctypes.Structure):
    """dctn_batch_call_t: every buffer, shape and option of one batch-source launch; what a kind or an operation does not
    use stays None / 0."""
    _fields_ = [("src", c_void), ("table", c_void), ("labels", c_void), ("sample_idx", c_void), ("x", c_void), ("y", c_void),
                ("indices", c_void), ("state", c_void), ("n", c_i64), ("global_batch", c_i64), ("count", c_i64),
                ("rank_offset", c_i64), ("row_len", c_i64), ("height", c_i64), ("width_px", c_i64), ("src_kind", c_int),
                ("src_channels", c_int), ("width", c_int), ("flags", c_int), ("dtype", c_int), ("augment", c_int),
                ("max_shift", c_int), ("aug_flags", c_int), ("fill", c_u32)]


_BatchCallP = ctypes.POINTER(BatchCall)


class TTString(ctypes.Structure):
    """dctn_tt_string_t: one ConvSBS string as dctn_tt_stats takes it; the bonds are cyclic (bond_sizes[0] == 1: open)."""
    _fields_ = [("n_cores", c_int), ("C", c_int), ("q", c_int), ("reserved", c_int), ("out_sizes", c_int * 16),
                ("bond_sizes", c_int * 16)]


_TTStringP = ctypes.POINTER(TTString)


class BatchMonitorCall(ctypes.Structure):
    """dctn_batch_monitor_t: every buffer, shape and option of one batch-monitor launch; ``indices`` may be None."""
    _fields_ = [("x", c_void), ("logits", c_void), ("y", c_void), ("indices", c_void), ("edges", c_void), ("block", c_void),
                ("workspace", c_void), ("workspace_bytes", c_size), ("B", c_i64), ("C", c_int), ("H", c_int), ("W", c_int),
                ("Q", c_int), ("K", c_int), ("L", c_int), ("n_edges", c_int), ("period", c_int), ("capacity", c_int),
                ("x_dtype", c_int), ("logits_dtype", c_int), ("reserved", c_int)]


_BatchMonitorP = ctypes.POINTER(BatchMonitorCall)

# name -> (restype, argtypes); mirrors include/dctn_amd.h one to one
SIGNATURES = {
    "dctn_version": (c_int, []),
    "dctn_strerror": (ctypes.c_char_p, [c_int]),
    "dctn_last_kernel": (ctypes.c_char_p, []),
    "dctn_device_limits": (c_int, [_IntP, _IntP]),
    "dctn_eps_family": (c_int, [c_int] * 9),
    "dctn_eps_fwd_workspace_bytes": (c_size, [c_int] * 7 + [c_int] * 2),
    "dctn_eps_fwd": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_size] + [c_int] * 7 + [c_int, c_int, c_void]),
    "dctn_eps_saved_bytes": (c_size, [c_int] * 7 + [c_int] * 2),
    "dctn_eps_fwd_save": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_size, c_void, c_size] + [c_int] * 7 + [c_int, c_int, c_void]),
    "dctn_eps_bwd_saved": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_size, c_void, c_void, c_void, c_size]
                           + [c_int] * 7 + [c_int, c_int, c_void]),
    "dctn_eps_fwd_stats_workspace_bytes": (c_size, [c_int] * 7 + [c_int] * 2),
    "dctn_eps_fwd_stats": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_size] + [c_int] * 7 + [c_int, c_int, c_void]),
    "dctn_eps_bwd_workspace_bytes": (c_size, [c_int] * 7 + [c_int] * 4),
    "dctn_eps_bwd": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_void, c_void, c_size]
                     + [c_int] * 7 + [c_int, c_int, c_void]),
    "dctn_eps_head_fwd": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_void, c_void] + [c_int] * 8 + [c_int, c_int, c_void]),
    "dctn_eps_head_bwd_workspace_bytes": (c_size, [c_int] * 8 + [c_int, c_int]),
    "dctn_eps_head_bwd": (c_int, [c_void, _I64x5, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_size]
                          + [c_int] * 8 + [c_int, c_int, c_void]),
    "dctn_ce_loss_fwd": (c_int, [c_void, c_void, c_void, c_i64, c_int, c_int, c_void]),
    "dctn_ce_loss_fwd_grad": (c_int, [c_void, c_void, c_void, c_void, c_i64, c_int, c_int, c_void]),
    "dctn_ce_loss_bwd": (c_int, [c_void, c_void, c_void, c_void, c_i64, c_int, c_int, c_void]),
    "dctn_sgd_l2_num_partials": (c_int, [c_i64]),
    "dctn_sgd_l2_step": (c_int, [c_void, c_void, c_void, c_void, c_i64, c_i64, ctypes.c_float, ctypes.c_float,
                                 ctypes.c_float, c_int, c_int, c_void]),
    "dctn_sgd_l2_step_master": (c_int, [c_void] * 5 + [c_i64, c_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        c_int, c_void]),
    "dctn_adam_state_bytes": (c_size, []),
    "dctn_adam_l2_num_partials": (c_int, [c_i64]),
    "dctn_adam_l2_step": (c_int, [c_void] * 6 + [c_i64, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                  ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_adam_l2_step_master": (c_int, [c_void] * 7 + [c_i64, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                         ctypes.c_float, ctypes.c_float, c_void]),
    "dctn_grad_guard_state_bytes": (c_size, []),
    "dctn_grad_guard_num_partials": (c_int, [c_i64]),
    "dctn_grad_guard_check": (c_int, [c_void, c_i64, c_int, c_void, c_void, c_void, c_void]),
    "dctn_adam_l2_step_guarded": (c_int, [c_void] * 7 + [c_i64, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_adam_l2_step_master_guarded": (c_int, [c_void] * 8 + [c_i64, c_i64, ctypes.c_double, ctypes.c_double,
                                                 ctypes.c_float, ctypes.c_float, ctypes.c_float, c_void]),
    "dctn_sgd_l2_step_guarded": (c_int, [c_void] * 5 + [c_i64, c_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                         c_int, c_int, c_void]),
    "dctn_sgd_l2_step_master_guarded": (c_int, [c_void] * 6 + [c_i64, c_i64, ctypes.c_float, ctypes.c_float,
                                                ctypes.c_float, c_int, c_void]),
    "dctn_lr_schedule_bytes": (c_size, []),
    "dctn_lr_schedule_value": (c_int, [c_void, c_i64, ctypes.POINTER(ctypes.c_float)]),
    "dctn_adam_l2_step_scheduled": (c_int, [c_void] * 9 + [c_i64, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                            ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_sgd_l2_step_scheduled": (c_int, [c_void] * 8 + [c_i64, c_i64, ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_param_groups_bytes": (c_size, []),
    "dctn_param_groups_check": (c_int, [c_void, c_i64]),
    "dctn_adam_l2_step_grouped": (c_int, [c_void] * 10 + [c_i64, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                          ctypes.c_float, c_int, c_void]),
    "dctn_sgd_l2_step_grouped": (c_int, [c_void] * 9 + [c_i64, c_i64, ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_flat_step_bytes": (c_size, []),
    "dctn_adam_flat_step": (c_int, [_FlatStepP, c_void, c_void, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                    ctypes.c_float, c_void]),
    "dctn_sgd_flat_step": (c_int, [_FlatStepP, c_void, ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_weight_ema_bytes": (c_size, []),
    "dctn_weight_ema_weight": (c_int, [c_void, c_i64, ctypes.POINTER(ctypes.c_float)]),
    "dctn_adam_flat_step_ema": (c_int, [_FlatStepP, _WeightEmaP, c_void, c_void, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_float, ctypes.c_float, c_void]),
    "dctn_sgd_flat_step_ema": (c_int, [_FlatStepP, _WeightEmaP, c_void, ctypes.c_float, ctypes.c_float, c_int, c_void]),
    "dctn_rmsprop_num_partials": (c_int, [c_i64]),
    "dctn_rmsprop_flat_step": (c_int, [_FlatStepP, _WeightEmaP, c_void, c_void, ctypes.c_double, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_float, c_void]),
    "dctn_sgd_flat_step_decay": (c_int, [_FlatStepP, _WeightEmaP, c_void, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                         c_int, c_void]),
    "dctn_weight_ema_apply": (c_int, [c_void, c_void, c_void, c_i64, c_int, c_void]),
    "dctn_weight_ema_restore": (c_int, [c_void, c_void, c_i64, c_int, c_void]),
    "dctn_step_trace_head_bytes": (c_size, []),
    "dctn_step_trace_record_bytes": (c_size, []),
    "dctn_step_trace_record": (c_int, [c_void] * 9 + [c_int, c_i64, c_int, c_int, c_void]),
    "dctn_ce_score_accumulate": (c_int, [c_void, c_void, c_void, c_i64, c_int, c_int, c_void]),
    "dctn_core_dropout_state_bytes": (c_size, []),
    "dctn_core_dropout_fwd": (c_int, [_PtrP, _PtrP, _I64P, c_int, c_void, c_void, c_void, c_int, c_void]),
    "dctn_core_dropout_bwd": (c_int, [_PtrP, _PtrP, _I64P, c_int, c_void, c_void, c_int, c_void]),
    "dctn_core_dropout_mask": (c_int, [_PtrP, _I64P, c_int, c_void, c_void, c_int, c_void]),
    "dctn_batch_state_bytes": (c_size, []),
    "dctn_batch_draw": (c_int, [c_void] * 7 + [c_i64] * 5 + [c_int] * 4 + [c_void]),
    "dctn_batch_gather": (c_int, [c_void] * 7 + [c_i64] * 3 + [c_int] * 3 + [c_void]),
    "dctn_batch_draw_cols": (c_int, [c_void] * 7 + [c_i64] * 5 + [c_int] * 4 + [c_void]),
    "dctn_batch_gather_cols": (c_int, [c_void] * 7 + [c_i64] * 3 + [c_int] * 3 + [c_void]),
    "dctn_batch_draw_aug": (c_int, [c_void] * 7 + [c_i64] * 6 + [c_int] * 5 + [c_u32, c_void]),
    "dctn_batch_draw_cols_aug": (c_int, [c_void] * 7 + [c_i64] * 6 + [c_int] * 6 + [c_u32, c_void]),
    "dctn_batch_call_bytes": (c_size, []),
    "dctn_batch_draw_call": (c_int, [_BatchCallP, c_void]),
    "dctn_batch_gather_call": (c_int, [_BatchCallP, c_void]),
    "dctn_state_max_regions": (c_int, []),
    "dctn_state_arena_bytes": (c_size, [_I64P, c_int]),
    "dctn_state_gather": (c_int, [_PtrP, _I64P, c_int, c_void, c_size, c_void, c_void]),
    "dctn_state_scatter": (c_int, [c_void, _PtrP, _I64P, c_int, c_void, c_void]),
    "dctn_window_stats": (c_int, [c_void, _I64x5, c_void] + [c_int] * 6 + [c_int, c_void]),
    "dctn_phi_window_stats": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "dctn_phi_expand": (c_int, [c_void, c_void, c_i64, ctypes.c_float, c_int, c_void]),
    "dctn_byte_histogram": (c_int, [c_void, c_i64, c_int, c_void, c_void]),
    "dctn_byte_window_stats_workspace_bytes": (c_size, [c_i64]),
    "dctn_byte_window_stats": (c_int, [c_void, c_i64, c_int, c_int, c_int, c_void, ctypes.c_double, ctypes.c_double, c_int,
                                       c_void, c_void, c_void]),
    "dctn_convsbs_workspace_bytes": (c_size, [c_int, _IntP, _IntP] + [c_int] * 5 + [_IntP, _IntP, c_int, c_int]),
    "dctn_convsbs_fwd": (c_int, [c_void, _I64x5, _PtrP, c_void, c_int, _IntP, _IntP, _IntP, _IntP]
                         + [c_int] * 5 + [c_void, c_size, c_int, c_void]),
    "dctn_convsbs_bwd": (c_int, [c_void, _I64x5, _PtrP, c_void, c_void, _PtrP, c_int, _IntP, _IntP, _IntP, _IntP]
                         + [c_int] * 5 + [c_void, c_size, c_int, c_void]),
    "dctn_convsbs_saved_states_bytes": (c_size, [c_int, _IntP, _IntP] + [c_int] * 5 + [_IntP, _IntP, c_int]),
    "dctn_convsbs_bwd_saved": (c_int, [c_void, _I64x5, _PtrP, c_void, c_void, _PtrP, c_int, _IntP, _IntP, _IntP, _IntP]
                               + [c_int] * 5 + [c_void, c_size, c_void, c_size, c_int, c_void]),
    "dctn_convsbs_many_workspace_bytes": (c_size, [c_int, c_int, _IntP, _IntP] + [c_int] * 5 + [_IntP, _IntP, c_int]),
    "dctn_convsbs_many_fwd": (c_int, [c_void, _I64x5, _PtrP, _PtrP, c_int, c_int, _IntP, _IntP, _IntP, _IntP] + [c_int] * 5 + [c_int, c_void]),
    "dctn_convsbs_many_bwd": (c_int, [c_void, _I64x5, _PtrP, _PtrP, c_void, _PtrP, c_int, c_int, _IntP, _IntP, _IntP, _IntP]
                              + [c_int] * 5 + [c_void, c_size, c_int, c_void]),
    "dctn_logmatmulexp_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_i64, c_i64, c_int]),
    "dctn_logmatmulexp_fwd": (c_int, [c_void, c_void, c_void, c_void, c_size, c_i64, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void]),
    "dctn_logmatmulexp_bwd": (c_int, [c_void] * 7 + [c_size, c_i64, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void]),
    "dctn_logmatmulexp_fold_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_int]),
    "dctn_logmatmulexp_fold_fwd": (c_int, [c_void, c_void, c_i64, c_int, c_int, c_int, c_void]),
    "dctn_linear_head_fwd": (c_int, [c_void, c_void, c_void, c_void, c_i64, c_int, c_int, c_int, c_void]),
    "dctn_linear_head_bwd_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int]),
    "dctn_linear_head_bwd": (c_int, [c_void] * 7 + [c_size, c_i64, c_int, c_int, c_int, c_void]),
    "dctn_position_mean_fwd": (c_int, [c_void, c_void, c_i64, c_i64, c_int, c_int, c_void]),
    "dctn_position_mean_bwd": (c_int, [c_void, c_void, c_i64, c_i64, c_int, c_int, c_void]),
    "dctn_tensor_stats_record_bytes": (c_size, []),
    "dctn_tensor_stats_workspace_bytes": (c_size, [c_int]),
    "dctn_tensor_stats": (c_int, [_PtrP, _I64P, c_int, c_void, c_void, c_size, c_int, c_void]),
    "dctn_tensor_hist_block_bytes": (c_size, [c_int]),
    "dctn_tensor_hist": (c_int, [_PtrP, _I64P, c_int, c_void, c_int, c_void, c_int, c_int, c_void]),
    "dctn_tensor_hist_reset": (c_int, [c_void, c_int, c_int, c_void]),
    "dctn_tt_stats_block_bytes": (c_size, [c_int, c_int]),
    "dctn_tt_stats_workspace_bytes": (c_size, [_TTStringP, c_int]),
    "dctn_tt_stats": (c_int, [_PtrP, _TTStringP, c_int, c_void, c_int, c_int, c_void, c_size, c_int, c_void]),
    "dctn_param_stats_block_bytes": (c_size, [c_int, c_int]),
    "dctn_param_stats_workspace_bytes": (c_size, [_I64P, c_int]),
    "dctn_param_stats": (c_int, [c_void, c_void, c_void, _I64P, c_int, c_void, c_int, c_int, c_void, c_size, c_int, c_void]),
    "dctn_batch_monitor_block_bytes": (c_size, [c_i64, c_int, c_int]),
    "dctn_batch_monitor_workspace_bytes": (c_size, [c_i64]),
    "dctn_batch_monitor": (c_int, [_BatchMonitorP, c_void]),
    "dctn_mode_product": (c_int, [c_void, c_void, c_void, c_i64, c_int, c_int, c_i64, c_int, c_void]),
    "dctn_fiber_gram_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_i64, c_int]),
    "dctn_fiber_gram": (c_int, [c_void, c_void, c_void, c_void, c_size, c_i64, c_int, c_int, c_i64, c_int, c_void]),
    "dctn_logmatmulexp_fold_bwd": (c_int, [c_void, c_void, c_void, c_void, c_size, c_i64, c_int, c_int, c_int, c_void]),
    "dctn_ar_handle_bytes": (c_size, []),
    "dctn_ar_create": (c_int, [c_int, c_int, c_size, _PtrP]),
    "dctn_ar_export": (c_int, [c_void, c_void]),
    "dctn_ar_connect": (c_int, [c_void, c_void]),
    "dctn_ar_allreduce": (c_int, [c_void, c_void, c_i64, c_int, c_int, c_void]),
    "dctn_ar_allreduce_algo": (c_int, [c_void, c_void, c_i64, c_int, c_int, c_int, c_void]),
    "dctn_ar_status": (c_int, [c_void]),
    "dctn_ar_destroy": (c_int, [c_void]),
}

_lib: Optional[ctypes.CDLL] = None


def build(verbose: bool = False) -> str:
    """Compile dctn_amd/csrc/*.hip for gfx950 into dctn_amd/libdctn_amd.so (hipcc cross-compiles
    without a GPU)."""
    res = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise RuntimeError("building libdctn_amd.so failed")
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP kernel library is the only implementation of the "
                "contraction path (no fallback).  Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C dctn_amd/csrc`."
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so does not export it
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def last_kernel() -> str:
    return lib().dctn_last_kernel().decode()


def dtype_code(t: torch.Tensor) -> int:
    try:
        return _DTYPE_CODE[t.dtype]
    except KeyError:
        raise TypeError(f"dctn_amd supports float32, float64 and bfloat16 tensors, got {t.dtype}") from None


def require_device(*tensors: torch.Tensor) -> torch.device:
    """Device of a kernel-library call: every tensor must already live on the same MI355X device (the
    autograd Functions are only ever reached through `on_device`, which stages CPU tensors first)."""
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "dctn_amd: the contraction path runs on an MI355X device only; got a tensor on "
                f"'{t.device}'.  There is deliberately no CPU fallback."
            )
        if t.device != dev:
            raise RuntimeError(f"dctn_amd: tensors on different devices ({dev} vs {t.device})")
    return dev


def placement(*tensors: torch.Tensor):
    """(device to compute on, staged?).  "Device follows the tensors" (SURVEY 8b): tensors that all live on
    one GPU compute there; tensors that all live on the CPU - how the reference's own tests build them
    (tests/test_eps.py:10-13) - are STAGED to the current GPU, run through the same HIP kernels and the
    results come back as CPU tensors of the same dtype.  Without a GPU there is nothing to stage to, and
    no CPU implementation to fall back on: RuntimeError.  Mixed placements raise like torch does."""
    devs = {t.device for t in tensors}
    if len(devs) > 1:
        raise RuntimeError(f"dctn_amd: expected all tensors on one device, got {sorted(str(d) for d in devs)}")
    dev = tensors[0].device
    if dev.type == "cuda":
        return dev, False
    if dev.type != "cpu":
        raise RuntimeError(f"dctn_amd: unsupported device '{dev}'")
    if not torch.cuda.is_available():
        raise RuntimeError(
            "dctn_amd: CPU tensors are staged to an MI355X for the contraction, but no GPU is visible. "
            "There is deliberately no CPU implementation of this path."
        )
    return torch.device("cuda", torch.cuda.current_device()), True


def on_device(fn, *tensors: torch.Tensor):
    """``fn(*tensors)`` with CPU tensors staged to the GPU and the result(s) brought back (see `placement`).
    The copies are ordinary differentiable ``.to()`` calls, so gradients arrive on the CPU leaves."""
    dev, staged = placement(*tensors)
    if not staged:
        return fn(*tensors)
    out = fn(*(t.to(dev) for t in tensors))
    if isinstance(out, torch.Tensor):
        return out.cpu()
    return type(out)(o.cpu() for o in out)


def check(rc: int, what: str) -> int:
    """Raises for the negative DCTN_ERR_* codes; returns the (non-negative) success code: DCTN_OK, DCTN_SAVED, DCTN_PARTIAL."""
    if rc >= 0:
        return rc
    msg = lib().dctn_strerror(rc).decode()
    if rc == ERR_BAD_SHAPE:
        raise AssertionError(f"{what}: {msg}")  # the reference signals shape errors with `assert`
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg} (code {rc})")


def stream_ptr(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def strides5(t: torch.Tensor):
    return (c_i64 * 5)(*t.stride())


def int_array(values: Sequence[int]):
    return (c_int * len(values))(*[int(v) for v in values])


def i64_array(values: Sequence[int]):
    return (c_i64 * len(values))(*[int(v) for v in values])


def ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    return (c_void * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


_ws_cache: dict = {}


def workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    """Scratch for one kernel-library call.  Small requests come from the caching allocator; large
    ones (ConvSBS backward states: tens of MB) reuse one grow-only buffer per (device, stream) —
    calls on a stream are ordered, so consecutive calls can share it — because re-requesting big
    blocks every call makes the allocator release and re-map them.  Under graph capture the
    allocation must come from the graph's pool, so the cache is bypassed."""
    nbytes = max(int(nbytes), 256)
    if nbytes < (8 << 20) or torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _ws_cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf


# precision policy for float32 tensors on the MFMA paths (bf16 tensors always use bf16 MFMA)
_precision = PREC_EXACT


# mode names of set_float32_matmul_precision: PyTorch's three ("highest", "high", "medium") and the project's own
PRECISION_MODES = {"exact": PREC_EXACT, "highest": PREC_EXACT, "high": PREC_SPLIT, "bf16": PREC_BF16, "medium": PREC_BF16}


def set_float32_matmul_precision(mode: str) -> None:
    """'exact' / 'highest' (default): f32 in / f32 accumulate.

    'high' (DCTN_PREC_SPLIT, bf16x3): each float32 operand value is the sum of two bf16 values, hi + lo, and each
    product hi*hi + hi*lo + lo*hi with float32 accumulation (about 3 * 2^-18 relative error per product).  Float32 EPS
    calls whose shape the bf16x3 large-core family plans run it, forward and backward; every other shape runs exactly
    as under 'exact' - the same kernels and the same bits (the register-resident exact-f32 family and its fused head,
    the two-halves path, float64, the generic kernels).  Like PyTorch's "high" it permits the faster arithmetic and
    does not force it.

    'bf16' / 'medium': operands rounded to bf16, f32 accumulate.  Any other name raises KeyError."""
    global _precision
    _precision = PRECISION_MODES[mode]


_options = 0


def precision() -> int:
    """The `policy` argument of the EPS entry points: precision | option flags (include/dctn_amd.h)."""
    return _precision | _options


class options:
    """``with L.options(L.OPT_SMALL_CHUNKS): ...`` - DCTN_OPT_* flags OR-ed into the policy of every EPS call inside
    the block (tests and measurement tools; the flags travel to the library as an explicit argument)."""

    def __init__(self, flags: int):
        self.flags = int(flags)

    def __enter__(self):
        global _options
        self._saved = _options
        _options |= self.flags
        return self

    def __exit__(self, *exc):
        global _options
        _options = self._saved
        return False
