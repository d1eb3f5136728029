"""ctypes binding of libdsdiff.so (the C ABI in include/dsdiff.h).

There is NO fallback: if the shared library is missing or no gfx950 device is usable the product
raises.  The oracle under /oracle is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSD_LIBRARY") or os.path.join(_HERE, "libdsdiff.so")   # DSD_LIBRARY: A/B builds (tools/)
CSRC = os.path.join(_HERE, "csrc")

DSD_MAX_LEVELS = 8
DSD_NCOEF = 8
DSD_DPM_NCOEF = 9
(DPM_MS0, DPM_MS1, DPM_MS2, DPM_MS3, DPM_SS_S1, DPM_SS_S2, DPM_SS_T2, DPM_SS_T3, DPM_SS_T3_TAYLOR) = range(9)
MODE_A_DDPM, MODE_A_DDIM, MODE_B_DDPM, MODE_B_DDIM, MODE_B_PLMS = 0, 1, 2, 3, 4
PLMS_PREDICT, PLMS_CORRECT, PLMS_AB2, PLMS_AB3, PLMS_AB4 = 0, 1, 2, 3, 4
PRED_EPS, PRED_X0, PRED_V = 0, 1, 2
LOSS_L2, LOSS_L1, LOSS_CHARBONNIER = 0, 1, 2
LOSS_TERM_MSE, LOSS_TERM_VB, LOSS_TERM_COM, LOSS_TERM_DIST, LOSS_NTERMS = 0, 1, 2, 3, 4
CONTRAST_CL, CONTRAST_EU, CONTRAST_EU_CL, CONTRAST_L1 = 0, 1, 2, 3
CONTRAST_MAX_VIEWS, CONTRAST_MAX_ROWS = 8, 256
METRICS_MAX_SCALES, METRICS_TILE_W, METRICS_TILE_H = 5, 32, 16
VOLUME_TILE_W, VOLUME_TILE_H, VOLUME_MAX_LOG2 = 32, 16, 27
# DSD_VOLUME_* slots of dsd_volume_metrics.out, in the header's order, and the status bits
VOLUME_SLOTS = ("nrmse", "mape", "smape", "logac", "medsymac", "psnr", "ssim3d", "status", "n_M", "lo_d", "hi_d", "lo_h", "hi_h", "lo_w",
                "hi_w", "mean_t_M", "std_t_M", "mean_p_M", "std_p_M", "mean_t_Z", "std_t_Z", "mean_p_Z", "std_p_Z", "mean_t_R", "std_t_R",
                "mean_p_R", "std_p_R")
VOLUME_NOUT = len(VOLUME_SLOTS)
VOLUME_EMPTY_MASK, VOLUME_EMPTY_CROP, VOLUME_ZERO_STD, VOLUME_ZERO_RANGE, VOLUME_SMALL_R = 1, 2, 4, 8, 16
PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16x6": 2, "f16x3": 3, "f16": 4, "bf16": 5}
(BLOCK_RES, BLOCK_ATTN, BLOCK_UPSAMPLE, BLOCK_DOWNSAMPLE, BLOCK_DISENTANGLE, BLOCK_SE, BLOCK_CROSSATTN,
 BLOCK_FF_GEGLU, BLOCK_BASIC_TRANSFORMER, BLOCK_SPATIAL_TRANSFORMER, BLOCK_VAE_ENCODER, BLOCK_VAE_DECODER,
 BLOCK_DIT, BLOCK_UNET, BLOCK_VAE_ATTN) = range(15)

# every symbol include/dsdiff.h declares (tests/test_abi.py checks the header against this list)
EXPORTS = [
    "dsd_last_error", "dsd_device_info", "dsd_create", "dsd_destroy", "dsd_param_count", "dsd_param_info",
    "dsd_set_param", "dsd_set_timestep_freqs", "dsd_set_precision", "dsd_get_precision", "dsd_set_share_zero_streams", "dsd_params_ready", "dsd_plan", "dsd_workspace_bytes", "dsd_device_bytes", "dsd_set_graph", "dsd_graph_stats", "dsd_set_fuse_gn_stats", "dsd_set_fuse_gn_apply", "dsd_set_stream_lanes", "dsd_set_winograd", "dsd_set_vae_fused_attention", "dsd_set_slice_ids", "dsd_plan_launches", "dsd_plan_flops",
    "dsd_profile_enable", "dsd_profile_count", "dsd_profile_get", "dsd_profile_op_count", "dsd_profile_op_get", "dsd_profile_op_name", "dsd_forward", "dsd_sample", "dsd_op_sampler_update", "dsd_sample_dpm", "dsd_op_dpm_step", "dsd_op_dpm_threshold", "dsd_block_create", "dsd_block_forward", "dsd_bench_conv2d", "dsd_bench_conv2d_stamps", "dsd_bench_mfma_peak", "dsd_conv_plan", "dsd_subpixel_weights_host", "dsd_set_conv_mfma16", "dsd_op_conv2d", "dsd_op_conv2d_prec", "dsd_op_conv2d_ex", "dsd_op_conv2d_gn", "dsd_op_gn_finalize", "dsd_op_avg_into_stats", "dsd_op_gn_small", "dsd_op_gn_silu_conv_out1",
    "dsd_op_gaussian_sample", "dsd_op_group_norm", "dsd_op_qkv_attention", "dsd_op_attention", "dsd_op_gemm_half", "dsd_bench_gemm_half", "dsd_bench_attention_half", "dsd_op_attention_half", "dsd_op_timestep_embedding", "dsd_op_linear", "dsd_op_philox_normal",
    "dsd_op_posterior_sample_scaled", "dsd_op_sampler_update_guided", "dsd_op_dpm_step_guided",
    "dsd_invert", "dsd_op_mask_blend", "dsd_op_q_sample", "dsd_op_ddim_invert_step",
    "dsd_sample_plms", "dsd_op_plms_step", "dsd_sample_dpm_program", "dsd_op_dpm_eval",
    "dsd_sample_dpm_adaptive_trial", "dsd_op_dpm_adaptive_error",
    "dsd_set_conditioning", "dsd_set_trace",
    "dsd_calc_bpd", "dsd_op_vlb_terms", "dsd_op_prior_bpd", "dsd_op_ddim_reverse_step",
    "dsd_create_disc", "dsd_op_disc_bottleneck",
    "dsd_eval_loss", "dsd_op_loss_rows", "dsd_op_pair_mse_rows", "dsd_op_vlb_terms_rows",
    "dsd_set_disentangle", "dsd_op_contrast_rows",
    "dsd_op_tail",
    "dsd_op_image_metrics",
    "dsd_op_volume_metrics", "dsd_op_kth_double",
]
# DSD_TAIL_* of include/dsdiff.h, in its order
TAIL_KINDS = ("se_scale", "avg_into", "nchw_to_nhwc", "nhwc_to_nchw", "avgpool2", "upsample2", "geglu", "softmax_rows", "ln_modulate",
              "ln_modulate16", "layer_norm", "gated_residual", "gelu_tanh", "patchify", "unpatchify", "add_rows_broadcast", "embed_add",
              "add2", "cast16", "uncast16")


class DsdConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("model_channels", C.c_int32), ("out_channels", C.c_int32),
        ("n_levels", C.c_int32), ("channel_mult", C.c_int32 * DSD_MAX_LEVELS),
        ("num_res_blocks", C.c_int32 * DSD_MAX_LEVELS), ("n_attention_resolutions", C.c_int32),
        ("attention_resolutions", C.c_int32 * DSD_MAX_LEVELS), ("num_heads", C.c_int32),
        ("num_head_channels", C.c_int32), ("num_heads_upsample", C.c_int32), ("use_scale_shift_norm", C.c_int32),
        ("resblock_updown", C.c_int32), ("use_new_attention_order", C.c_int32), ("legacy", C.c_int32),
    ]


class DsdSchedule(C.Structure):
    _fields_ = [
        ("steps", C.c_int32), ("mode", C.c_int32), ("pred", C.c_int32), ("learned_range", C.c_int32),
        ("clip_denoised", C.c_int32), ("eta", C.c_float), ("coef", C.POINTER(C.c_float)),
        ("t_model", C.POINTER(C.c_float)), ("nonzero", C.POINTER(C.c_int32)),
    ]


class DsdDpmSchedule(C.Structure):
    _fields_ = [
        ("steps", C.c_int32), ("pred", C.c_int32), ("data_pred", C.c_int32), ("thresholding", C.c_int32),
        ("threshold_ratio", C.c_float), ("threshold_max", C.c_float), ("coef", C.POINTER(C.c_float)),
        ("t_input", C.POINTER(C.c_float)), ("order", C.POINTER(C.c_int32)),
    ]


class DsdDpmProgram(C.Structure):
    _fields_ = [
        ("n_eval", C.c_int32), ("pred", C.c_int32), ("data_pred", C.c_int32), ("thresholding", C.c_int32),
        ("threshold_ratio", C.c_float), ("threshold_max", C.c_float), ("kind", C.POINTER(C.c_int32)),
        ("t_input", C.POINTER(C.c_float)), ("alpha", C.POINTER(C.c_float)), ("sigma", C.POINTER(C.c_float)),
        ("coef", C.POINTER(C.c_float)), ("slot", C.POINTER(C.c_int32)), ("keep", C.POINTER(C.c_int32)),
    ]


class DsdGuidance(C.Structure):
    _fields_ = [("uncond", C.c_void_p), ("scale", C.POINTER(C.c_float)), ("n_scale", C.c_int32)]


class DsdConditioning(C.Structure):
    _fields_ = [("context", C.c_void_p), ("context_uncond", C.c_void_p), ("tokens", C.c_int32), ("y", C.c_void_p),
                ("y_uncond", C.c_void_p), ("y_width", C.c_int32), ("B", C.c_int32)]


class DsdTrace(C.Structure):
    _fields_ = [("keep", C.POINTER(C.c_int32)), ("n_keep", C.c_int32), ("x", C.c_void_p), ("pred_x0", C.c_void_p)]


class DsdInpaint(C.Structure):
    _fields_ = [("x0", C.c_void_p), ("mask", C.c_void_p), ("mask_channels", C.c_int32), ("noise", C.c_void_p)]


class DsdInvertSchedule(C.Structure):
    _fields_ = [("steps", C.c_int32), ("coef", C.POINTER(C.c_float)), ("t_model", C.POINTER(C.c_float))]


class DsdBpd(C.Structure):
    _fields_ = [("post_log_var", C.POINTER(C.c_float)), ("vb", C.c_void_p), ("xstart_mse", C.c_void_p), ("mse", C.c_void_p),
                ("prior", C.c_void_p), ("prior_log_var", C.c_float)]


class DsdLoss(C.Structure):
    _fields_ = [("target", C.c_int32), ("pred", C.c_int32), ("kind", C.c_int32), ("learned_range", C.c_int32), ("t_model", C.c_void_p), ("a", C.c_void_p),
                ("s", C.c_void_p), ("vlb_coef", C.c_void_p), ("post_log_var", C.c_void_p), ("decoder", C.c_void_p),
                ("terms", C.c_void_p)]


class DsdDisentangle(C.Structure):
    _fields_ = [("mode", C.c_int32), ("temperature_cs", C.c_float), ("temperature_sal", C.c_float), ("labels_cs", C.c_void_p),
                ("n_labels_cs", C.c_int32), ("labels_sal", C.c_void_p), ("n_labels_sal", C.c_int32), ("loss", C.c_void_p),
                ("logits_cs", C.c_void_p), ("logits_sal", C.c_void_p)]


class DsdImageMetrics(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("target", C.c_void_p), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("scales", C.c_int32), ("data_range", C.c_double), ("pre", C.POINTER(C.c_double)), ("scale_out", C.c_void_p),
                ("elem_out", C.c_void_p)]


class DsdVolumeMetrics(C.Structure):
    _fields_ = [("target", C.c_void_p), ("pred", C.c_void_p), ("elem_is_double", C.c_int32), ("mask", C.c_void_p), ("D", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("win", C.c_int32), ("out", C.c_void_p)]


class DsdConvEx(C.Structure):
    _fields_ = [("x_batch_stride", C.c_int64), ("pad_lo", C.c_int32), ("pad_total", C.c_int32), ("y_ld", C.c_int32),
                ("out_nchw", C.c_int32), ("emb_stride", C.c_int32), ("no_scratch", C.c_int32), ("ksplit", C.c_int32),
                ("reserved", C.c_int32), ("kernel", C.c_char * 64)]


class DsdConvGn(C.Structure):
    _fields_ = [("gn_scale", C.c_void_p), ("gn_shift", C.c_void_p), ("stats", C.c_void_p), ("stats_doubles", C.c_int64),
                ("stats_chunks", C.c_int32), ("query", C.c_int32)]


class DsdError(RuntimeError):
    pass


_lib = None


def build(verbose: bool = False) -> str:
    """Compile libdsdiff.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise DsdError("building libdsdiff.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DsdError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"(or make -C {CSRC}); there is no CPU fallback")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; load torch FIRST so both share that one HIP runtime
    # (loading /opt/rocm's copy first leaves torch with "No HIP GPUs are available").
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32p = C.c_void_p, C.c_int, C.c_int64, C.c_void_p
    L.dsd_last_error.restype = C.c_char_p
    L.dsd_device_info.argtypes = [i32, C.c_char_p, i32, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.dsd_create.argtypes = [C.POINTER(DsdConfig), i32, C.POINTER(vp)]
    L.dsd_destroy.argtypes = [vp]
    L.dsd_destroy.restype = None
    L.dsd_param_count.argtypes = [vp]
    L.dsd_param_info.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.dsd_set_param.argtypes = [vp, C.c_char_p, f32p, C.POINTER(C.c_int64), i32, i32, vp]
    L.dsd_set_timestep_freqs.argtypes = [vp, f32p, i32]
    L.dsd_set_precision.argtypes = [vp, i32]
    L.dsd_get_precision.argtypes = [vp]
    L.dsd_set_share_zero_streams.argtypes = [vp, i32]
    L.dsd_params_ready.argtypes = [vp]
    L.dsd_plan.argtypes = [vp, i32, i32, i32, i32]
    L.dsd_workspace_bytes.argtypes = [vp]
    L.dsd_workspace_bytes.restype = i64
    L.dsd_device_bytes.argtypes = [vp]
    L.dsd_device_bytes.restype = i64
    L.dsd_set_graph.argtypes = [vp, i32]
    L.dsd_set_fuse_gn_stats.argtypes = [vp, i32]
    L.dsd_set_fuse_gn_apply.argtypes = [vp, i32]
    L.dsd_set_stream_lanes.argtypes = [vp, i32, i32]
    L.dsd_set_winograd.argtypes = [vp, i32]
    L.dsd_set_vae_fused_attention.argtypes = [vp, i32]
    L.dsd_graph_stats.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dsd_set_slice_ids.argtypes = [vp, C.POINTER(C.c_int64), i32]
    L.dsd_plan_launches.argtypes = [vp]
    L.dsd_plan_flops.argtypes = [vp]
    L.dsd_plan_flops.restype = C.c_double
    L.dsd_profile_enable.argtypes = [vp, i32]
    L.dsd_profile_count.argtypes = [vp]
    L.dsd_op_gn_silu_conv_out1.argtypes = [vp, i32, i32, i32, i32, vp, vp, C.c_float, vp, vp, vp, vp]
    L.dsd_profile_op_count.argtypes = [vp]
    L.dsd_profile_op_name.argtypes = [vp, i32, C.POINTER(C.c_char_p)]
    L.dsd_profile_op_get.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dsd_profile_get.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.dsd_forward.argtypes = [vp, f32p, vp, i32, i32, i32, i32, i32, f32p, C.POINTER(vp), vp]
    # The six device loops: one entry point each, the handle picks the denoiser, g / inp are NULL for unguided / unmasked.  A
    # library from before this layout, loaded through DSD_LIBRARY, still exports dsd_sample & co. but with the older, shorter
    # signatures: it no longer matches these and must not be used for A/B runs of the loops.
    sp, gp, ip = C.POINTER(DsdSchedule), C.POINTER(DsdGuidance), C.POINTER(DsdInpaint)
    L.dsd_sample.argtypes = [vp, sp, gp, ip, f32p, i32, f32p, i32, f32p, C.c_uint64, i32, i32, i32, i32, i32, vp]
    L.dsd_sample_dpm.argtypes = [vp, C.POINTER(DsdDpmSchedule), gp, f32p, i32, f32p, i32, i32, i32, i32, vp]
    L.dsd_sample_dpm_program.argtypes = [vp, C.POINTER(DsdDpmProgram), gp, f32p, i32, f32p, i32, i32, i32, i32, f32p, vp]
    L.dsd_sample_plms.argtypes = [vp, sp, gp, ip, C.c_float, f32p, i32, f32p, i32, C.c_uint64, i32, i32, i32, i32, i32, vp]
    L.dsd_invert.argtypes = [vp, C.POINTER(DsdInvertSchedule), gp, f32p, i32, f32p, i32, i32, i32, i32, i32, i32, vp]
    L.dsd_calc_bpd.argtypes = [vp, sp, C.POINTER(DsdBpd), f32p, i32, f32p, i32, f32p, C.c_uint64, i32, i32, i32, i32, i32, vp]
    L.dsd_op_sampler_update.argtypes = [C.POINTER(DsdSchedule), i32, f32p, f32p, f32p, C.c_uint64, i32, i32, i32, f32p, vp]
    L.dsd_op_dpm_step.argtypes = [C.POINTER(DsdDpmSchedule), i32, f32p, i32, f32p, f32p, f32p, i32, i32, i32, vp]
    L.dsd_op_dpm_threshold.argtypes = [f32p, i32, i32, C.c_float, C.c_float, f32p, f32p, vp]
    L.dsd_block_create.argtypes = [i32, C.POINTER(C.c_int32), i32, i32, C.POINTER(vp)]
    L.dsd_block_forward.argtypes = [vp, f32p, i32, i32, i32, i32, f32p, i32, f32p, i32, f32p, vp]
    L.dsd_op_conv2d.argtypes = [f32p, i32, i32, i32, i32, f32p, f32p, i32, i32, i32, i32, f32p, f32p, f32p, vp]
    L.dsd_bench_conv2d.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.dsd_bench_conv2d_stamps.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_longlong), i32, C.POINTER(C.c_int)]
    L.dsd_bench_mfma_peak.argtypes = [i32, i32, C.c_float, i32, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.dsd_conv_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.dsd_op_conv2d_prec.argtypes = [f32p, i32, i32, i32, i32, f32p, f32p, i32, i32, i32, i32, f32p, f32p, i32, f32p, vp]
    L.dsd_op_conv2d_ex.argtypes = [f32p, i32, i32, i32, i32, f32p, f32p, i32, i32, i32, i32, f32p, f32p, i32, C.POINTER(DsdConvEx),
                                   f32p, vp]
    L.dsd_op_conv2d_gn.argtypes = [f32p, i32, i32, i32, i32, f32p, f32p, i32, i32, i32, i32, f32p, f32p, i32, C.POINTER(DsdConvEx),
                                   C.POINTER(DsdConvGn), f32p, vp]
    L.dsd_op_gn_finalize.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, i32, f32p, f32p, C.c_float, f32p, i32, f32p, f32p, vp]
    L.dsd_op_avg_into_stats.argtypes = [f32p, f32p, f32p, f32p, C.c_float, i32, i32, i32, f32p, i32, i32, i32, i32, vp, i64,
                                        C.POINTER(C.c_int), vp]
    L.dsd_op_gn_small.argtypes = [f32p, i32, i32, i32, f32p, f32p, C.c_float, f32p, i32, i32, f32p, vp]
    L.dsd_op_attention.argtypes = [f32p, f32p, f32p, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float,
                                   C.c_float, i32, f32p, vp]
    L.dsd_op_group_norm.argtypes = [f32p, i32, i32, i32, f32p, f32p, C.c_float, i32, f32p, vp]
    L.dsd_op_qkv_attention.argtypes = [f32p, i32, i32, i32, i32, i32, i32, f32p, vp]
    L.dsd_set_conv_mfma16.argtypes = [i32]
    L.dsd_subpixel_weights_host.argtypes = [f32p, i32, i32, f32p]
    L.dsd_op_gemm_half.argtypes = [f32p, f32p, f32p, i32, i32, i32, i32, i32, f32p, i32, f32p, vp]
    L.dsd_bench_gemm_half.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_float)]
    L.dsd_bench_attention_half.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_float)]
    L.dsd_op_attention_half.argtypes = [f32p, i32, i32, i32, i32, i32, C.c_float, f32p, vp]
    L.dsd_op_timestep_embedding.argtypes = [vp, i32, i32, i32, f32p, f32p, vp]
    L.dsd_op_linear.argtypes = [f32p, i32, i32, f32p, f32p, i32, i32, f32p, vp]
    L.dsd_op_gaussian_sample.argtypes = [f32p, f32p, C.c_uint64, i32, i32, i32, i32, f32p, vp]
    L.dsd_op_philox_normal.argtypes = [f32p, i64, C.c_uint64, C.c_uint64, vp]
    L.dsd_op_posterior_sample_scaled.argtypes = [f32p, f32p, C.c_uint64, i32, i32, i32, i32, C.c_float, f32p, vp]
    L.dsd_op_sampler_update_guided.argtypes = [C.POINTER(DsdSchedule), i32, f32p, f32p, C.c_float, f32p, i64, f32p, C.c_uint64,
                                               i32, i32, i32, i32, f32p, vp]
    L.dsd_op_dpm_step_guided.argtypes = [C.POINTER(DsdDpmSchedule), i32, f32p, f32p, i32, C.c_float, f32p, i64, f32p, f32p,
                                         i32, i32, i32, i32, vp]
    L.dsd_op_mask_blend.argtypes = [C.c_float, C.c_float, f32p, f32p, i32, f32p, i64, i32, f32p, C.c_uint64, C.c_uint64, i32, i32,
                                    i32, i32, vp]
    L.dsd_op_q_sample.argtypes = [f32p, f32p, f32p, f32p, C.c_uint64, C.c_uint64, f32p, i64, i32, i32, i32, i32, vp]
    L.dsd_op_ddim_invert_step.argtypes = [C.c_float, C.c_float, f32p, f32p, C.c_float, f32p, i64, i32, i32, i32, i32, vp]
    L.dsd_op_plms_step.argtypes = [i32, C.c_float, C.c_float, C.c_float, f32p, f32p, C.c_float, f32p, f32p, f32p, f32p, f32p, i64,
                                   C.c_float, i32, i32, i32, i32, vp]
    L.dsd_op_dpm_eval.argtypes = [C.POINTER(DsdDpmProgram), i32, f32p, f32p, i32, C.c_float, f32p, i64, f32p, f32p, i32, i32, i32, i32, vp]
    if hasattr(L, "dsd_sample_dpm_adaptive_trial"):   # (absent from an older build under DSD_LIBRARY)
        L.dsd_sample_dpm_adaptive_trial.argtypes = [vp, C.POINTER(DsdDpmProgram), gp, f32p, i32, C.POINTER(C.c_float), C.c_float,
                                                    C.c_float, f32p, f32p, f32p, i32, i32, i32, i32, C.POINTER(C.c_float), vp]
        L.dsd_op_dpm_adaptive_error.argtypes = [i32, C.POINTER(C.c_float), C.c_float, C.c_float, f32p, f32p, f32p, f32p, i64, f32p,
                                                f32p, f32p, i32, i32, i32, i32, vp]
    L.dsd_op_vlb_terms.argtypes = [sp, i32, C.c_float, f32p, i64, f32p, i64, f32p, f32p, C.c_uint64, f32p, f32p, f32p, i64, f32p, f32p,
                                   f32p, i32, i32, i32, i32, vp]
    L.dsd_op_prior_bpd.argtypes = [C.c_float, C.c_float, f32p, f32p, i32, i32, i32, i32, vp]
    L.dsd_op_ddim_reverse_step.argtypes = [sp, i32, C.c_float, f32p, i64, f32p, i64, f32p, i32, i32, i32, i32, vp]
    if hasattr(L, "dsd_create_disc"):          # (likewise absent from an older build under DSD_LIBRARY)
        L.dsd_create_disc.argtypes = [C.POINTER(DsdConfig), i32, C.POINTER(vp)]
        L.dsd_op_disc_bottleneck.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, f32p,
                                             C.POINTER(vp), i32, vp]
    if hasattr(L, "dsd_eval_loss"):            # (likewise)
        L.dsd_eval_loss.argtypes = [vp, C.POINTER(DsdLoss), f32p, i32, f32p, i32, f32p, C.c_uint64, C.c_uint64, i32, i32, i32, vp]
        L.dsd_op_loss_rows.argtypes = [i32, i32, f32p, i64, f32p, f32p, C.c_uint64, C.c_uint64, f32p, f32p, f32p, i64, i32, i32, i32,
                                       i32, vp]
        L.dsd_op_pair_mse_rows.argtypes = [C.POINTER(vp), i32, i32, i64, f32p, vp]
        L.dsd_op_vlb_terms_rows.argtypes = [i32, i32, i32, f32p, f32p, vp, f32p, i64, f32p, i64, f32p, f32p, C.c_uint64, C.c_uint64,
                                            f32p, f32p, f32p, i64, i32, i32, i32, i32, vp]
    if hasattr(L, "dsd_set_disentangle"):      # (likewise)
        L.dsd_set_disentangle.argtypes = [vp, C.POINTER(DsdDisentangle)]
        L.dsd_op_contrast_rows.argtypes = [C.POINTER(vp), i32, i32, i64, i64, vp, i32, C.c_float, f32p, f32p, vp]
    if hasattr(L, "dsd_op_tail"):              # (likewise)
        L.dsd_op_tail.argtypes = [i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(C.c_float), vp]
    if hasattr(L, "dsd_op_image_metrics"):     # (likewise)
        L.dsd_op_image_metrics.argtypes = [C.POINTER(DsdImageMetrics), vp]
    if hasattr(L, "dsd_op_volume_metrics"):    # (likewise)
        L.dsd_op_volume_metrics.argtypes = [C.POINTER(DsdVolumeMetrics), vp]
        L.dsd_op_kth_double.argtypes = [vp, i64, i64, vp, vp]
    if hasattr(L, "dsd_set_conditioning"):     # (an older build under DSD_LIBRARY, for A/B timing of the loops it has)
        L.dsd_set_conditioning.argtypes = [vp, C.POINTER(DsdConditioning)]
    if hasattr(L, "dsd_set_trace"):            # (likewise)
        L.dsd_set_trace.argtypes = [vp, C.POINTER(DsdTrace)]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise DsdError(lib().dsd_last_error().decode("utf-8", "replace"))


def require_gpu(device: int = 0):
    """Fail loudly unless a gfx950 device is usable (no silent eager/CPU fallback)."""
    name = C.create_string_buffer(256)
    ncu, mem = C.c_int(0), C.c_int64(0)
    check(lib().dsd_device_info(device, name, 256, C.byref(ncu), C.byref(mem)))
    return name.value.decode(), ncu.value, mem.value


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t):
    """Device pointer of a contiguous fp32 CUDA tensor (or None)."""
    if t is None:
        return None
    import torch
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous CUDA tensor"
    return C.c_void_p(t.data_ptr())
