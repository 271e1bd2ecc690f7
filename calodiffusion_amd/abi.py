"""ctypes binding of ``lib/libcalodiff_hip.so`` (C ABI: ``include/calodiff.h``): the constants, structs and signatures of the
header, the loader, the helpers every caller of the library shares, the process-wide calls and the workspace cache.

PyTorch is used here for device memory, streams and parameter storage only.  There is no fallback of
any kind: if the library is missing, or no gfx950 GPU is visible, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CALODIFF_LIB") or os.path.join(_HERE, "lib", "libcalodiff_hip.so")  # override: A/B builds

CD_MAX_SIZES = 8
CD_ABI_VERSION = 3  # include/calodiff.h; load_library refuses a library that reports another one
TIME_KINDS = {"log": 0, "sigma": 1, "raw": 2}
OBJECTIVES = {"hybrid": 0, "noise_pred": 1, "mean_pred": 2}
LOSS_TYPES = {"l2": 0, "l1": 1, "mse": 2, "huber": 3}  # CD_LOSS_* (Loss._loss, models/loss.py:97-116)


class CdUnetDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("grid", C.c_int32 * 3),
        ("in_channels", C.c_int32),
        ("n_sizes", C.c_int32),
        ("layer_sizes", C.c_int32 * CD_MAX_SIZES),
        ("groups", C.c_int32),
        ("block_attn", C.c_int32),
        ("mid_attn", C.c_int32),
        ("compress_z", C.c_int32),
        ("cond_size", C.c_int32),
        ("cond_dim", C.c_int32),
        ("rz_input", C.c_int32),
        ("phi_input", C.c_int32),
        ("time_embed_kind", C.c_int32),
        ("objective", C.c_int32),
        ("sigma_data", C.c_float),
        ("time_sin", C.c_int32),
        ("cond_sin", C.c_int32),
    ]


SOP_LINCOMB, SOP_DENOISE, SOP_RANDN, SOP_RECORD, SOP_LINDIV, SOP_DENOISE_PS = 0, 1, 2, 3, 4, 5


class CdSamplerOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dst", C.c_int32), ("nsrc", C.c_int32), ("src", C.c_int32 * 6), ("col", C.c_int32)]


class CdLayerMlpDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("dim_in", C.c_int32), ("hidden", C.c_int32), ("cond_emb", C.c_int32), ("cond_size", C.c_int32),
                ("n_res", C.c_int32), ("time_embed_kind", C.c_int32), ("objective", C.c_int32), ("sigma_data", C.c_float)]


class CdHlfDesc(C.Structure):
    """Host tables of one binning geometry (cd_hlf_create copies them to the device)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_layers", C.c_int32), ("layer_offset", C.POINTER(C.c_int32)),
                ("eta", C.POINTER(C.c_double)), ("phi", C.POINTER(C.c_double)), ("with_centres", C.POINTER(C.c_int32))]


class CdShowerStatsDesc(C.Structure):
    """Host tables of one shower geometry (cd_shower_stats_create copies them to the device)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_layers", C.c_int32), ("n_cells", C.c_int32), ("n_rbins", C.c_int32),
                ("n_abins", C.c_int32), ("r_bin", C.POINTER(C.c_int32)), ("a_bin", C.POINTER(C.c_int32)),
                ("r_coord", C.POINTER(C.c_double)), ("angle", C.POINTER(C.c_double))]


class CdGeneratorRun(C.Structure):
    """The arguments of cd_generator_run_ex."""
    _fields_ = [("struct_size", C.c_uint32), ("batch", C.c_int32), ("energy", C.c_void_p), ("energy_is_normalised", C.c_int32),
                ("sparse_mode", C.c_int32), ("layers", C.c_void_p), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("first_row", C.c_int32), ("global_batch", C.c_int32), ("showers", C.c_void_p), ("layers_out", C.c_void_p),
                ("next_offset", C.POINTER(C.c_uint64)), ("decode_seed", C.c_uint64), ("decode_offset", C.c_uint64),
                ("next_decode_offset", C.POINTER(C.c_uint64)), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class CdClassifierDesc(C.Structure):
    """The classifier test's DNN (calodiffusion_amd.classifier)."""
    _fields_ = [("struct_size", C.c_uint32), ("input_dim", C.c_int32), ("hidden", C.c_int32), ("num_layer", C.c_int32),
                ("negative_slope", C.c_float), ("dropout_p", C.c_float)]


class CdStep(C.Structure):
    _fields_ = [("sigma", C.c_float), ("sigma_prev_masked", C.c_float), ("ddim_sigma", C.c_float), ("denom", C.c_float)]


# every symbol include/calodiff.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SIGNATURES = {
    "cd_last_error": (C.c_char_p, []),
    "cd_abi_version": (C.c_int, []),
    "cd_device_check": (C.c_int, [C.c_char_p, C.c_int]),
    "cd_plan_create": (C.c_int, [C.POINTER(CdUnetDesc), C.POINTER(_P)]),
    "cd_plan_destroy": (C.c_int, [_P]),
    "cd_plan_num_weights": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "cd_plan_weight_name": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]),
    "cd_plan_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "cd_plan_set_weights": (C.c_int, [_P, C.c_int, C.POINTER(_P), _P]),
    "cd_plan_set_coords": (C.c_int, [_P, _P, _P, _P, _P]),
    "cd_plan_workspace_bytes": (C.c_int, [_P, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_unet_forward": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_denoise": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_denoise_safe": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_int), _P]),
    "cd_ddim_sample": (C.c_int, [_P, C.c_int, _P, _P, C.POINTER(CdStep), C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P,
                                 C.c_int, _P, C.c_size_t, _P]),
    "cd_plan_sampler_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_sampler_run": (C.c_int, [_P, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, C.POINTER(CdSamplerOp), C.c_int,
                                 C.POINTER(C.c_int32), _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P, C.c_int,
                                 _P, C.c_size_t, _P]),
    "cd_randn": (C.c_int, [_P, C.c_int64, C.c_uint64, C.c_uint64, _P]),
    "cd_plan_grad_layout": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "cd_plan_train_workspace_bytes": (C.c_int, [_P, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_plan_status": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
    "cd_layer_forward": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "cd_layer_denoise": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "cd_layer_sample": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "cd_layer_sampler_run": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, _P, C.c_int,
                                       _P, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    "cd_layer_train_workspace_bytes": (C.c_int, [_P, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_layer_train_step": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_layer_train_step_loss": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_size_t,
                                           _P]),
    "cd_layer_loss": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "cd_layer_vjp_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_layer_denoise_vjp": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_reverse_norm": (C.c_int, [_P, _P, _P, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_float, C.c_float, _P]),
    "cd_reverse_norm_staged": (C.c_int, [_P, _P, _P, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_int, _P]),
    "cd_preprocess": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_float, C.c_float,
                                C.c_float, C.c_int, C.c_float, _P]),
    "cd_preprocess_hgcal": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_double), C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_float, _P]),
    "cd_geom_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P), _P]),
    "cd_geom_create_ex": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P), _P]),
    "cd_geom_create_csr": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P), _P]),
    "cd_geom_refresh": (C.c_int, [_P, _P, _P]),
    "cd_geom_destroy": (C.c_int, [_P]),
    "cd_geom_apply_vjp": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P]),
    "cd_geom_apply": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P]),
    "cd_geom_sparse_workspace_bytes": (C.c_int, [_P, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_geom_decode_sparse": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "cd_radial_create": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.POINTER(_P), _P]),
    "cd_radial_destroy": (C.c_int, [_P]),
    "cd_radial_enc": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "cd_radial_dec": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "cd_radial_enc_vjp": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "cd_radial_dec_vjp": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "cd_preprocess_ds1": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_float, C.c_float, C.c_float,
                                    C.c_int, C.c_float, _P]),
    "cd_reverse_norm_ds1": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_float, C.c_float, _P]),
    "cd_plan_set_radial": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "cd_plan_set_geom": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "cd_adam_step": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                               C.POINTER(C.c_int64), C.c_double, C.c_double, C.c_double, C.c_float, C.c_float, C.c_int, _P]),
    "cd_train_step": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "cd_train_step_target": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "cd_ode_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int64, _P]),
    "cd_ema_step": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_double, _P]),
    "cd_plan_vjp_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_denoise_vjp": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_plan_bns_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_bns_theta_grad": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_generator_create": (C.c_int, [_P, C.c_size_t, C.POINTER(_P), _P]),
    "cd_generator_destroy": (C.c_int, [_P]),
    "cd_generator_checksum": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "cd_generator_info": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cd_generator_geometry": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cd_generator_workspace_bytes": (C.c_int, [_P, C.c_int, C.POINTER(C.c_size_t)]),
    "cd_generator_run": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_uint64),
                                   _P, C.c_size_t, _P]),
    "cd_generator_run_ex": (C.c_int, [_P, C.POINTER(CdGeneratorRun)]),
    "cd_hlf_create": (C.c_int, [C.POINTER(CdHlfDesc), C.POINTER(_P), _P]),
    "cd_hlf_destroy": (C.c_int, [_P]),
    "cd_hlf_compute": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, _P, _P]),
    "cd_shower_stats_create": (C.c_int, [C.POINTER(CdShowerStatsDesc), C.POINTER(_P), _P]),
    "cd_shower_stats_destroy": (C.c_int, [_P]),
    "cd_shower_stats_compute": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
    "cd_threshold_conserve": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "cd_fpd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "cd_fpd_moments": (C.c_int, [_P, C.c_int64, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int32), C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_kpd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "cd_kpd_sums": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, _P, _P, _P, C.c_size_t,
                              _P]),
    "cd_column_histograms_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "cd_column_histograms": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "cd_classifier_num_params": (C.c_int, [C.POINTER(CdClassifierDesc), C.POINTER(C.c_int64)]),
    "cd_classifier_workspace_bytes": (C.c_int, [C.POINTER(CdClassifierDesc), C.c_int, C.POINTER(C.c_size_t)]),
    "cd_classifier_forward": (C.c_int, [C.POINTER(CdClassifierDesc), C.POINTER(C.c_void_p), _P, C.c_int64, _P, C.c_int64, _P, C.c_int, _P,
                                        C.c_size_t, _P]),
    "cd_classifier_train_step": (C.c_int, [C.POINTER(CdClassifierDesc), C.POINTER(C.c_void_p), _P, _P, C.c_int64, _P, C.c_int, C.c_uint64,
                                           C.c_uint64, _P, _P, C.c_int, _P, _P, C.c_double, C.c_double, C.c_double, C.c_float, C.c_int, _P,
                                           C.c_size_t, _P]),
    "cd_classifier_train_epoch": (C.c_int, [C.POINTER(CdClassifierDesc), C.POINTER(C.c_void_p), _P, _P, C.c_int64, _P, C.c_int64, C.c_int,
                                            C.c_uint64, C.c_uint64, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_float, _P, _P,
                                            C.c_size_t, _P]),
    "cd_classifier_dropout_mask": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P]),
    "cd_set_conv_precision": (C.c_int, [C.c_char_p]),
    "cd_get_conv_precision": (C.c_char_p, []),
    "cd_profile_begin": (C.c_int, []),
    "cd_profile_end": (C.c_int, [C.c_char_p, C.c_int]),
    "cd_loss_hybrid_l2": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cd_loss_hybrid": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "cd_op_to_channels_last": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, _P]),
    "cd_op_to_ncdhw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, _P]),
    "cd_op_axpy_sigma": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int64, _P]),
    "cd_op_cyl_conv": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P]),
    "cd_op_zslide_conv": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                    _P, _P]),
    "cd_op_cyl_conv_transpose": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                           C.POINTER(C.c_int32), _P, _P]),
    "cd_op_init_conv": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _P, _P]),
    "cd_op_init_pair_conv": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int), C.c_int,
                                       C.POINTER(C.c_int32), C.c_int, _P, _P]),
    "cd_op_group_norm": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    "cd_op_resnet_block": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(_P), _P, _P, C.c_int, C.c_int,
                                     C.POINTER(C.c_int32), C.c_int, _P, C.c_size_t, _P]),
    "cd_op_linear_attention": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.POINTER(C.c_int32), _P, C.c_size_t, _P]),
    "cd_op_conv_backward": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.c_size_t, _P]),
    "cd_op_conv_transpose_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                                C.POINTER(C.c_int32), _P, C.c_size_t, _P]),
    "cd_op_group_norm_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _P,
                                            C.c_size_t, _P]),
    "cd_op_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int64]),
    "cd_op_linear_act": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.c_int,
                                   _P]),
    "cd_op_linear_act_backward": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P,
                                            C.c_size_t, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the HIP library and bind every declared symbol; fails loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m calodiffusion_amd.build` (hipcc, --offload-arch=gfx950). "
            "calodiffusion_amd has no CPU or PyTorch fallback.")
    _check_built_from_these_sources()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    if lib.cd_abi_version() != CD_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} reports ABI version {lib.cd_abi_version()}, this binding is written against "
                           f"{CD_ABI_VERSION} (include/calodiff.h): rebuild with `python -m calodiffusion_amd.build`")
    _lib = lib
    return lib


def _check_built_from_these_sources():
    """The library is git-ignored and travels between boxes as a built file: refuse one that was not built from the sources
    next to it (a stale .so with an older argument list shifts every pointer argument).  build.py writes `<lib>.srchash`
    after every link; CALODIFF_LIB (an explicit A/B build) and CD_SKIP_SRCHASH=1 bypass the check."""
    if os.environ.get("CALODIFF_LIB") or os.environ.get("CD_SKIP_SRCHASH"):
        return
    from . import build
    stamp = LIB_PATH + ".srchash"
    have = open(stamp).read().strip() if os.path.exists(stamp) else None
    want = build.source_hash()
    if have != want:
        raise RuntimeError(f"{LIB_PATH} was not built from the sources in {build.CSRC} (stamp {str(have)[:12]}, sources "
                           f"{want[:12]}): run `python -m calodiffusion_amd.build`")


def _check(code: int):
    if code != 0:
        msg = load_library().cd_last_error().decode(errors="replace")
        exc = ValueError if code == -1 else RuntimeError
        raise exc(f"calodiff[{code}]: {msg}")


def require_gpu() -> str:
    lib = load_library()
    if not torch.cuda.is_available():
        raise RuntimeError("calodiffusion_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False and "
                           "there is no CPU fallback")
    buf = C.create_string_buffer(256)
    _check(lib.cd_device_check(buf, 256))
    return buf.value.decode()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(ROCm) tensor: calodiffusion_amd computes on the GPU only")
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t


_NP_DTYPES = {torch.float32: np.float32, torch.float64: np.float64}


def _upload(a, dtype: torch.dtype, name: str, need_gpu: bool = False, keep_device: bool = False) -> torch.Tensor:
    """A NumPy array, sequence or tensor (host or device) as a contiguous device tensor of ``dtype``; the values are not touched.
    A tensor is converted by torch in the move; anything else is converted by NumPy on the host and then uploaded.
    ``need_gpu``: without a GPU the refusal names the argument (else it is torch's own).  ``keep_device``: a CUDA tensor
    stays on its device (else everything lands on the current one)."""
    if need_gpu and not torch.cuda.is_available():
        raise RuntimeError(f"{name}: calodiffusion_amd computes on the GPU only and torch.cuda.is_available() is False")
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype == object:
            raise TypeError(f"{name} must be a numeric array")
        # ("CW": torch wraps writable arrays only; a copy is made only where one is needed)
        a = torch.from_numpy(np.require(a, _NP_DTYPES[dtype], "CW"))
    return a.detach().to(device=a.device if keep_device and a.is_cuda else "cuda", dtype=dtype).contiguous()


def _i32x3(v: Sequence[int]):
    return (C.c_int32 * 3)(*[int(a) for a in v])


def _nbytes(sizing_fn, *args) -> int:
    """What a ``cd_*_workspace_bytes(*args, size_t *out)`` entry point reports."""
    n = C.c_size_t()
    _check(sizing_fn(*args, C.byref(n)))
    return n.value


class Handle:
    """A ``void*`` of the library: ``handle`` is null until a ``cd_*_create`` call fills it (``C.byref(self.handle)``), and is what
    the C calls take.  ``destroy`` (the ``cd_*_destroy`` of its kind) is called at most once and never for a null handle, so an
    owner whose create call failed frees nothing.  After ``close()`` the handle is null again."""

    def __init__(self, destroy):
        self.handle, self._destroy = C.c_void_p(), destroy

    def close(self):
        handle, self.handle = self.handle, C.c_void_p()
        if handle:
            self._destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter teardown: the library may be gone before its last handle
            pass


class WorkspaceCache:
    """The workspaces one owner hands to the library: at most ONE uint8 tensor per kind (the large ones are ~1 GB each at the
    headline batch: alternating calls of two kinds must not reallocate, a ragged last batch must not double the footprint).
    A request for another key of a kind drops the kept tensor first, then sizes and allocates the new one, so the two never
    coexist.  Iterating yields (kind, *key)."""

    def __init__(self):
        self._kept = {}  # kind -> (key, tensor)

    def get(self, kind, key, device, nbytes) -> torch.Tensor:
        """``nbytes`` a callable: the workspace of exactly that size, the callable evaluated on a miss only (everything keyed by
        shape).  ``nbytes`` an int: one of at least that size (grow on demand)."""
        key = tuple(key)
        kept = self._kept.get(kind)
        if kept is not None and kept[0] == key and (callable(nbytes) or kept[1].numel() >= nbytes):
            return kept[1]
        del kept  # (every reference to the old tensor goes before the next one is sized and allocated)
        self._kept.pop(kind, None)
        ws = torch.empty(int(nbytes() if callable(nbytes) else nbytes), dtype=torch.uint8, device=device)
        self._kept[kind] = (key, ws)
        return ws

    def drop(self, *kinds):
        for kind in kinds:
            self._kept.pop(kind, None)

    def clear(self):
        self._kept.clear()

    def __iter__(self):
        return iter([(kind,) + key for kind, (key, _) in self._kept.items()])

    def __len__(self):
        return len(self._kept)


def set_conv_precision(mode: str):
    """'f16x2' (default), 'bf16x3' or 'f32' arithmetic of the convolutions, process-wide (cd_set_conv_precision)."""
    _check(load_library().cd_set_conv_precision(mode.encode()))


def get_conv_precision() -> str:
    return load_library().cd_get_conv_precision().decode()


def profile_begin():
    _check(load_library().cd_profile_begin())


def profile_end() -> dict:
    import json
    buf = C.create_string_buffer(1 << 18)
    _check(load_library().cd_profile_end(buf, 1 << 18))
    return json.loads(buf.value.decode())


def randn(shape, device, seed: int, offset: int = 0) -> torch.Tensor:
    """Unit normals from the device Philox stream (element i is a function of (seed, offset + i) only)."""
    lib = load_library()
    require_gpu()
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _check(lib.cd_randn(out.data_ptr(), out.numel(), int(seed), int(offset), _stream()))
    return out
