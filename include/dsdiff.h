/*
 * dsdiff.h — C ABI of libdsdiff.so: the MI355X (gfx950) implementation of the conditional-DDPM
 * sampling hot path of larrybb626/diffusion_models_dsdiff.
 *
 * Plain C: pointers, sizes, ints.  No torch types.  Every tensor pointer is a DEVICE pointer to
 * contiguous fp32 unless stated otherwise; the caller owns inputs/outputs, the library owns the
 * packed weights and the workspace.  Every entry point returns 0 on success, <0 on error
 * (dsd_last_error() gives the message, thread-local).  All work is enqueued on the caller's
 * hipStream_t (passed as void*; NULL = default stream) and is asynchronous w.r.t. the host.
 * Calls on one handle are not re-entrant.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   dsd_create / dsd_set_param     <- DSUnetModel.__init__           UNet_DS_Diff/model.py:172-611
 *                                     + nn.Module.load_state_dict (names = reference state_dict keys)
 *   dsd_forward                    <- DSUnetModel.forward            UNet_DS_Diff/model.py:629-756
 *   dsd_create_disc                <- UNet_disc_Model.__init__ / SuperResModelNew   Disc_diff/guided_diffusion/unet.py:726-967,1063-1076
 *                                     (the four-stream DisC-Diff denoiser of configs/disc-diff.yaml and disc-diff-origin.yaml);
 *                                     dsd_forward on such a handle <- UNet_disc_Model.forward :985-1044, and every four-stream
 *                                     loop (dsd_sample ... dsd_calc_bpd) takes it with Cc = 3 (t1, t2, dwi behind the state,
 *                                     Disc_diff/guided_diffusion/gaussian_diffusion.py:271-278)
 *   dsd_op_disc_bottleneck         <- the bottleneck head of that forward, :1015-1033 (csrc/disc.hip)
 *   dsd_sample                     <- GaussianDiffusion.p_sample_loop / ddim_sample_loop
 *                                        Disc_diff/guided_diffusion/gaussian_diffusion.py:524-616,705-786
 *                                     DDPMModel.p_sample_loop        trainers/trainer_ddpm.py:447-482
 *                                     DDIMSampler.ddim_sampling      ldm/models/diffusion/ddim.py:128-261
 *                                     the same two on VAE latents (a DSD_BLOCK_UNET / DSD_BLOCK_DIT handle)
 *                                        ldm/models/diffusion/ddim.py:128-261, ldm/models/diffusion/ddpm.py:1048-1115
 *                                        (call sites trainers/trainer_latent_diffusion.py:492-544)
 *                                     with g: unconditional_guidance_scale / unconditional_conditioning
 *                                        ldm/models/diffusion/ddim.py:194-219 (p_sample_ddim, ucg_schedule :165-167)
 *   dsd_sample_dpm                 <- DPMSolverSampler.sample  ldm/models/diffusion/dpm_solver_new/sampler.py:35-103
 *                                     with g: model_wrapper guidance_type="classifier-free"
 *                                        ldm/models/diffusion/dpm_solver_new/dpm_solver_pytorch.py:324-332
 *   dsd_sample_plms / dsd_op_plms_step
 *                                  <- PLMSSampler.sample / p_sample_plms  ldm/models/diffusion/plms.py:59-245
 *                                        with sampling_util.norm_thresholding (dynamic_threshold)
 *   dsd_set_trace                  <- the intermediates those samplers return (x_inter / pred_x0 every log_every_t steps)
 *                                        ldm/models/diffusion/ddim.py:149,178-183, plms.py likewise, ddpm.py:1062,1089-1092,
 *                                        trainers/trainer_ddpm.py:451-456
 *   dsd_set_disentangle / dsd_op_contrast_rows
 *                                  <- training_losses(disentangle=) / get_disentangle_loss / ContrastiveLoss
 *                                        training_project/utils/gaussian_diffusion.py:907-975,1056-1094,
 *                                        loss_function/contrastive_loss.py (csrc/contrast.hip)
 *   dsd_op_image_metrics           <- monai.metrics MAEMetric / SSIMMetric at the end of validation_step
 *                                        trainers/trainer_ddpm.py:501-565, and the per-slice MS-SSIM of
 *                                        inference/test_metrics.py:249-274 (csrc/metrics.hip)
 *   dsd_op_sampler_update_guided / dsd_op_dpm_step_guided <- one guided step of those loops (kernel-level tests, host loops)
 *   dsd_sample_dpm_adaptive_trial / dsd_op_dpm_adaptive_error
 *                                  <- one trial of DPM_Solver.dpm_solver_adaptive  sampler.py:921-980 (the loop stays on the host)
 *   dsd_sample_dpm_program / dsd_op_dpm_eval
 *                                  <- DPM_Solver.sample / .inverse with method "multistep" order 1..3, "singlestep",
 *                                        "singlestep_fixed", return_intermediate, guided or not
 *                                        Disc_diff/guided_diffusion/sampler.py:445-501,555-868,1001-1217
 *   dsd_op_posterior_sample_scaled <- LatentDiffusion.get_first_stage_encoding(encode_first_stage(x))
 *                                        ldm/models/diffusion/ddpm.py:660-667 with distributions.py:24-37
 *   dsd_block_*                    <- ResBlock / AttentionBlock / Upsample / Downsample
 *                                        ldm/modules/diffusionmodules/openaimodel.py:93-164,167-284,426-473
 *                                     FeatureDisentangle             UNet_DS_Diff/model.py:152-168
 *                                     SE_Attention                   Disc_diff/guided_diffusion/unet.py:82-109
 *                                     CrossAttention / BasicTransformerBlock / SpatialTransformer
 *                                        ldm/modules/attention.py:145-194,302-331,366-428
 *   dsd_op_*                       <- the stock torch ops those modules call (kernel-level tests)
 */
#ifndef DSDIFF_H
#define DSDIFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsd_handle dsd_handle;

#define DSD_MAX_LEVELS 8

/* ctor kwargs of DSUnetModel that shape the graph (UNet_DS_Diff/model.py:172-202). */
typedef struct dsd_config {
    int32_t in_channels;        /* per-stream input channels (yaml: 1) */
    int32_t model_channels;
    int32_t out_channels;
    int32_t n_levels;           /* len(channel_mult) */
    int32_t channel_mult[DSD_MAX_LEVELS];
    int32_t num_res_blocks[DSD_MAX_LEVELS];
    int32_t n_attention_resolutions;
    int32_t attention_resolutions[DSD_MAX_LEVELS];
    int32_t num_heads;          /* -1 if unset */
    int32_t num_head_channels;  /* -1 if unset */
    int32_t num_heads_upsample; /* -1 if unset */
    int32_t use_scale_shift_norm;
    int32_t resblock_updown;
    int32_t use_new_attention_order;
    int32_t legacy;
} dsd_config;

/* Error text of the last failing call on this thread ("" if none). */
const char* dsd_last_error(void);
/* Library / device probe: returns 0 and fills name (<=255 chars) if a gfx950 device is usable. */
int dsd_device_info(int device, char* name, int name_len, int* n_cu, int64_t* hbm_bytes);

/* ---- model handle ------------------------------------------------------------------------ */
/* device < 0 creates a table-only handle (parameter names/shapes, no GPU needed; compute calls fail). */
int dsd_create(const dsd_config* cfg, int device, dsd_handle** out);
/* UNet_disc_Model (Disc_diff/guided_diffusion/unet.py:726-1044): four single-channel encoder streams with their own weights
 * (input_blocks, input_blocks_T1, _T2, _DWI), every skip the four-stream mean, a bottleneck head — conv_common / conv_distinct
 * (one weight set each, applied to all four streams), SE gates, Conv1x1 + SiLU — then middle block, decoder and out.  The
 * parameter table carries the reference state_dict's names, shapes and order.  Of dsd_config, `legacy` is ignored (this network
 * has only the openai-style AttentionBlock); num_heads_upsample and use_new_attention_order are honoured; in_channels and
 * channel_mult[0] must be 1.  The handle is a model handle: dsd_plan / dsd_forward take C = 4 (x, T1, T2, DWI), the sampling
 * loops take it wherever they take dsd_create's with Cc = 3 (any other count fails before device work), graph replay,
 * first_step / n_steps and dsd_set_slice_ids included; dsd_set_share_zero_streams(on) fails (all four streams are live).
 * dsd_forward's feats: NULL or 8 device pointers to [B,half,H/2^(L-1),W/2^(L-1)] NCHW buffers, com_h1..4 (after the SiLU,
 * before any SE) then dist_h1..4 (after their SE): with `out` the 9-tuple the reference returns.
 * The head runs as three launches of csrc/disc.hip; with the environment variable DSD_DISC_UNFUSED set (read when a plan is
 * built) it is composed from the older ops instead (SiLU copies, four-way mean, the one-workgroup-per-sample SE, concat
 * copies): A/B timing and cross-check. */
int dsd_create_disc(const dsd_config* cfg, int device, dsd_handle** out);
void dsd_destroy(dsd_handle* h);

/* Parameter table (names/shapes identical to the reference state_dict, OIHW conv weights). */
int dsd_param_count(dsd_handle* h);
int dsd_param_info(dsd_handle* h, int idx, const char** name, int64_t shape[4], int* ndim);
/* Upload one parameter. src is fp32 in the reference layout; src_is_device selects the copy kind.
 * 3x3 conv weights are re-packed OIHW -> OHWI on device.  With src_is_device the copy is asynchronous on `stream`;
 * later plan-time work of the library (splitting the weights into bf16 / fp16 pieces, on whatever stream the planning
 * call is given) waits on an event recorded here, so uploads on a non-blocking stream need no extra synchronisation. */
int dsd_set_param(dsd_handle* h, const char* name, const float* src, const int64_t* shape, int ndim,
                  int src_is_device, void* stream);
/* Optional: the sinusoidal-embedding frequency table exp(-ln(1e4)*k/half), k < model_channels/2
 * (util.py:172-174), as evaluated by the caller's own fp32 exp.  sin/cos of t*f with t up to 1e3 amplify a
 * 1-ulp difference in f to ~6e-5, so a host that wants bit-identical arguments supplies its table; without
 * it the library evaluates exp in fp64 and rounds once. */
int dsd_set_timestep_freqs(dsd_handle* h, const float* freqs_host, int n);
/* Arithmetic of the convolutions (99 % of the FLOPs): DSD_PREC_F32 = v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fma
 * chain); DSD_PREC_BF16X6 = every fp32 operand split exactly into three bf16 pieces, six bf16 MFMA products with fp32
 * accumulation (drops only terms <= 2^-24: fp32-grade, ~1e-6 on the network output); DSD_PREC_BF16X3 = two pieces, three
 * products (~1.5e-5 on the network output, still inside the 1e-4 bar of the sampled image).
 * DSD_PREC_F16X3 = two fp16 pieces (11 + 11 bits), three products: ~1.4x the fp32 kernel's error at 1.5x the speed of
 * bf16x6, but fp16's range: if a conv operand exceeds 65504 the call FAILS (device flag, checked with one stream
 * synchronisation at the end of dsd_forward / dsd_sample) instead of returning inf/NaN, and operands that are uniformly
 * tiny lose accuracy (absolute floor 3e-8: |x|~1e-3 -> 2e-5 relative).  Meant for GroupNorm-normalised activations.
 * Default: DSD_PREC_BF16X6 (all parity tests hold at the fp32 tolerances); shapes the split kernel cannot take
 * (Cin % 32 != 0, operands >= 4 GiB) use the fp32 kernels in every mode.
 * DSD_PREC_F16 / DSD_PREC_BF16 (DSD_BLOCK_DIT handles only; any other handle refuses them): the reference's autocast
 * arithmetic for the transformer backbone (BASELINE configs[4] "512x512 fp16"; UNet_DS_Diff/DiT_models.py:101-122 under
 * torch.autocast) — the four Linears of every DiTBlock and both attention products take 16-bit operands rounded ONCE
 * (round to nearest even) and run ONE MFMA per product with fp32 accumulation; LayerNorm, adaLN modulation, softmax
 * statistics, the gated residual stream, patch embedding, conditioning MLPs and the final layer stay fp32 as autocast keeps
 * them.  fp16 has fp16's range (activations beyond 65504 become inf exactly as in the reference); bf16 does not. */
enum { DSD_PREC_F32 = 0, DSD_PREC_BF16X3 = 1, DSD_PREC_BF16X6 = 2, DSD_PREC_F16X3 = 3, DSD_PREC_F16 = 4, DSD_PREC_BF16 = 5 };
int dsd_set_precision(dsd_handle* h, int precision);
int dsd_get_precision(dsd_handle* h);
/* dsd_sample only, OFF by default.  In the 2-channel branch (model.py:654-658) the `al` and `l` encoder streams get
 * zeros_like(x) as input and, inside a sampling loop, the same timestep for every slice: their activations are identical
 * across the batch.  With this option they are evaluated once per step (batch of one) and broadcast where they join the
 * other streams — the same output (bit-identical when the per-layer kernel choice does not change with the batch,
 * otherwise equal to fp32 rounding, ~1e-7), 28 % fewer FLOPs at batch 16.  It is work the reference performs redundantly, so
 * it is never enabled silently and bench.py reports it as a separate line; dsd_plan_flops() counts what is executed. */
int dsd_set_share_zero_streams(dsd_handle* h, int on);
/* GroupNorm statistics (ON by default): every tensor a GroupNorm32 normalises is written by a convolution, or is the
 * concatenation of a convolution output and the skip average (model.py:743-746), so the per-channel sums are accumulated
 * in the epilogue of the kernel that writes the tensor and the separate statistics pass over HBM disappears
 * (openaimodel.py:264-284: "fused GroupNorm" of the north star).  0 = always run the standalone pass (A/B, tests). */
int dsd_set_fuse_gn_stats(dsd_handle* h, int on);
/* GroupNorm + SiLU in front of a 3x3 convolution (ResBlock in_layers / out_layers, openaimodel.py:264-284), ON by default in
 * the bf16x6 mode: the large layers — those the tap-reuse kernel takes — apply the normalisation while they stage their input
 * rows into LDS, so the apply pass (one read + one write of the tensor through HBM per GroupNorm) disappears.  An element is
 * then activated once per filter row and column tile (6x on a 320-channel layer) in VALU slots of the convolution, with the
 * hardware exp2 / reciprocal (~1 ulp each) instead of expf and an IEEE division: the outputs agree with the apply-pass route
 * to fp32 rounding (measured 1e-7 relative on the network output), not bit for bit.  0 = always the separate pass. */
int dsd_set_fuse_gn_apply(dsd_handle* h, int on);
/* The four encoder streams of DSUnetModel (noise, a, al, l: UNet_DS_Diff/model.py:674-686) are independent chains until the
 * skip average.  ON by default: from the first encoder block whose input has at most `max_pixels` pixels (batch x H x W;
 * <= 0 keeps the current value, default 16384) the four streams are launched on four HIP streams (the caller's + three of
 * the library's, forked and joined through events inside dsd_forward / dsd_sample, also under hipGraph capture), so that
 * four grids too small to fill 256 CUs share the chip instead of queueing.  The convolutions of those levels are PLANNED for
 * a quarter of the chip each (tile width / split-K: a layer that would take narrow tiles alone takes the wide tap-reuse kernel
 * with the fused GroupNorm when its three siblings run beside it), so on = 1 and on = 0 agree to fp32 rounding, not bit for
 * bit; on = 2 keeps the lanes' plan and launches it on the caller's stream alone — bit-identical to on = 1 (the check that no
 * dependency between the lanes is missing).  The caller sees one stream: work submitted to it after the call is ordered
 * after the join. */
int dsd_set_stream_lanes(dsd_handle* h, int on, int max_pixels);
/* bf16x6 mode only, OFF by default: 3x3 stride-1 convolutions whose grid fills the chip at least twice (>= 512 workgroups),
 * with an output width that is a power of two <= 256, Cin % 32 == 0 and Cout = 0 or 64 (mod 128), run as Winograd F(2,3)
 * ALONG THE WIDTH — 4 instead of 6 products per pair of outputs and filter row, i.e. 1.5x fewer MFMAs.  The input transform
 * (sums / differences of neighbouring pixels) is done in fp32, the weight transform once in fp64, and both operands are then
 * split into three bf16 pieces exactly as in the direct kernel, so every operand still carries 24 significant bits; the
 * result differs from the direct form by an fp32 re-association of the convolution sum (measured: 0.75x the direct
 * kernel's error against fp64, tests/test_ops_gpu.py).  Opt-in because it is only 6-20 % faster than the direct kernel on
 * the layers it takes (its operand feeding costs what the saved MFMAs gain: conv_wino.hip header) — 2 % on a whole
 * denoising step — and stays below the 300 TF/s go / no-go set for it. */
int dsd_set_winograd(dsd_handle* h, int on);
/* KL-VAE handles, OFF by default: AttnBlock (one head over all C <= 512 channels) as ONE fused attention launch — online
 * softmax, the T x T score matrix never leaves the chip (csrc/attention_wide.hip for C > 128) — instead of the materialised
 * route (two GEMMs around a row softmax, per sample).  With it on the plan holds neither the 4 T^2-byte score buffer nor the
 * V transpose nor the split planes, so dsd_workspace_bytes shrinks.  Both routes are fp32-grade (exact fp32 MFMA in
 * DSD_PREC_F32, bf16x6 otherwise) and agree to fp32 rounding, not bit for bit.  A block with C > 512 or C % 4 != 0 keeps
 * the materialised route. */
int dsd_set_vae_fused_attention(dsd_handle* h, int on);
/* 0 if every parameter has been set, else -1 with the first missing name in dsd_last_error(). */
int dsd_params_ready(dsd_handle* h);

/* Build (or re-use) the launch plan + workspace for an input shape.  Allocation happens here,
 * never inside dsd_forward/dsd_sample once the plan for that shape exists. */
int dsd_plan(dsd_handle* h, int B, int C, int H, int W);
int64_t dsd_workspace_bytes(dsd_handle* h);
/* Everything the handle holds on the device right now: parameter slab, upload staging, workspace arena, the bf16 / fp16
 * weight pieces of the split arithmetic modes (6 B per convolution weight; only the family of the current mode is kept),
 * sampling scratch. */
int64_t dsd_device_bytes(dsd_handle* h);
/* Number of kernel launches in the current plan's forward. */
int dsd_plan_launches(dsd_handle* h);
/* Algorithmic FLOPs (2*MAC of conv/linear/attention matmuls) of one forward of the current plan:
 * executed = what the kernels really compute. */
double dsd_plan_flops(dsd_handle* h);

/* One denoising-network evaluation.  x: [B,C,H,W] (C in {2,4}, NCHW as the reference passes it),
 * t: [B] int64 (t_is_float=0) or fp32 (t_is_float=1) on device, out: [B,out_channels,H,W].
 * feats: NULL, or 14 device pointers to [B,half,H/2^(L-1),W/2^(L-1)] NCHW buffers in the order
 * style[3], content[3], anatomy[2], lesion[2], n_style_content[4] (model.py:751-756). */
int dsd_forward(dsd_handle* h, const float* x, const void* t, int t_is_float, int B, int C, int H, int W,
                float* out, float* const* feats, void* stream);

/* Per-kernel timing of the plan, measured with hipEvents on the stream the kernels are launched on (one
 * pair per op; forces a stream sync per forward, so never leave it on in a throughput run).  Totals
 * accumulate over forwards until re-enabled.  kind = kernel name, flops / bytes = the algorithmic work of
 * those launches (2*MAC; fp32 read+write bytes for the memory-bound kernels). */
int dsd_profile_enable(dsd_handle* h, int on);
int dsd_profile_count(dsd_handle* h);
int dsd_profile_get(dsd_handle* h, int idx, const char** kind, double* total_ms, double* flops, double* bytes,
                    int64_t* calls, int* runs);
/* The same per op of the plan, in launch order, for the last profiled forward (kind = the op's kernel kind). */
int dsd_profile_op_count(dsd_handle* h);
int dsd_profile_op_get(dsd_handle* h, int idx, const char** kind, double* ms, double* flops, double* bytes);
/* The layer op `idx` of the current plan belongs to: the name of the last parameter the graph builder looked up before it
 * emitted the op ("input_blocks.4.0.in_layers.2.bias", ...; "" for ops in front of the first parameter). */
int dsd_profile_op_name(dsd_handle* h, int idx, const char** name);

/* ---- sampling loop ----------------------------------------------------------------------- */
/* Whole-forward hipGraph replay inside dsd_sample / dsd_sample_dpm (OFF by default): the network evaluation of a step is
 * a fixed list of ~800 launches whose arguments do not change while the loop runs on the same buffers, so it can be captured
 * once (after the plan's first host-launched forward) and replayed per step; the reference's Python loop
 * (gaussian_diffusion.py:569-616) pays the launches every step.  Results are bit-identical either way.  Measured on MI355X:
 * the asynchronous host launches already keep the GPU busy (batch 16: 443.7 vs 445.4 ms per step, batch 1: 39.0 vs 40.3), so
 * replay only takes the launch work off the host thread; hence opt-in.  dsd_forward and dsd_profile_* always launch from
 * the host. */
int dsd_set_graph(dsd_handle* h, int on);
int dsd_graph_stats(dsd_handle* h, int* captures, int* launches);
/* Optional: the global slice index of every row of the next sampling batches (host array, n = batch size; n = 0 clears).
 * With it the on-device Philox noise of a slice is keyed by (seed, step, slice index, pixel) instead of its position in
 * the batch, so a volume gives the same samples however its slices are sharded over GPUs or grouped into batches. */
int dsd_set_slice_ids(dsd_handle* h, const int64_t* ids_host, int n);
enum { DSD_MODE_A_DDPM = 0, DSD_MODE_A_DDIM = 1, DSD_MODE_B_DDPM = 2, DSD_MODE_B_DDIM = 3,
       /* PLMSSampler: dsd_sample_plms only; every other entry point rejects it */
       DSD_MODE_B_PLMS = 4 };
enum { DSD_PRED_EPS = 0, DSD_PRED_X0 = 1, DSD_PRED_V = 2 };
#define DSD_NCOEF 8
/* Host-side schedule for `steps` loop iterations, iteration k = 0 is the FIRST executed (largest t).
 * coef[k*DSD_NCOEF + j] fp32, meaning per mode (tables are produced in float64 on the host exactly as
 * the reference does and rounded to fp32 once, gaussian_diffusion.py:1003 / ddpm.py:155-178):
 *   A (guided-diffusion):  0 sqrt_acp  1 sqrt_1m_acp  2 sqrt_recip_acp  3 sqrt_recipm1_acp
 *                          4 post_coef1  5 post_coef2  6 log_var(fixed) or min_log(learned range)  7 max_log
 *        A_DDIM re-uses 0-3 and:  4 alpha_bar  5 alpha_bar_prev
 *   B_DDPM (ldm):          0 sqrt_acp 1 sqrt_1m_acp 2 sqrt_recip_acp 3 sqrt_recipm1_acp 4 coef1 5 coef2 6 post_log_var
 *   B_DDIM (ldm):          0 sqrt_acp 1 sqrt_1m_acp 4 a_t 5 a_prev 6 sigma_t 7 sqrt_1m_at
 *   B_PLMS (ldm):          the slots of B_DDIM; sigma_t must be 0 (PLMS takes eta = 0 only).  The second network evaluation of
 *                          iteration 0 runs at t_model[min(1, steps - 1)] (plms.py:150)
 * t_model[k]: the timestep value handed to the network at iteration k (timestep_map[t], optionally
 * rescaled, respace.py:123-128); nonzero[k]: 0 only where the reference masks the noise (t == 0). */
typedef struct dsd_schedule {
    int32_t steps;
    int32_t mode;          /* DSD_MODE_* */
    int32_t pred;          /* DSD_PRED_* */
    int32_t learned_range; /* model emits 2*C channels, LEARNED_RANGE variance (gaussian_diffusion.py:280-294) */
    int32_t clip_denoised;
    float eta;             /* DDIM eta (A_DDIM computes sigma on device from alpha_bar, alpha_bar_prev) */
    const float* coef;     /* host, steps*DSD_NCOEF */
    const float* t_model;  /* host, steps */
    const int32_t* nonzero;/* host, steps */
} dsd_schedule;

/* ---- the two kinds of denoiser ---------------------------------------------------------------
 * Every loop below (dsd_sample, dsd_sample_dpm, dsd_sample_dpm_program, dsd_sample_plms, dsd_invert, dsd_calc_bpd) runs whole on
 * the device and takes the same (h, ..., cond, Cc, x, Cz, ..., B, H, W, ...): the HANDLE picks the denoiser, the call does not.
 *   - A model handle (dsd_create: DSUnetModel; dsd_create_disc: UNet_disc_Model) is the four-stream model.  x: [B,1,H,W], so
 *     Cz must be 1 (anything else is rejected before device work).  cond: [B,Cc,H,W] (Cc in {1,3}; 3 for UNet_disc_Model)
 *     concatenated after x every step (DiffusionWrapper 'concat', ddpm.py:1331-1333); the planes are read in place.
 *   - A DSD_BLOCK_UNET handle (the plain UNetModel; with a spatial transformer or a label_emb its context / y come through
 *     dsd_set_conditioning, below, and Cc may be 0) or a DSD_BLOCK_DIT handle reads the state from its own input.  x: [B,Cz,H,W]
 *     (VAE latents).  The UNetModel has in_channels = Cz + Cc and out_channels = Cz (2 with a learned-range variance, which needs
 *     Cz = 1).  cond [B,Cc,H,W] is concatenated after the state: both are copied ONCE into the denoiser's persistent NCHW input,
 *     and every update writes x_{t-1} straight into its state channels.  dsd_set_graph replay runs on one stream, no forks; the
 *     Philox counter is (seed, step, slice, channel, pixel).  Replaces DDIMSampler.sample / ddim_sampling
 *     (ldm/models/diffusion/ddim.py:57-261) and LatentDiffusion.p_sample_loop (ddpm.py:1048-1115) as
 *     trainers/trainer_latent_diffusion.py:492-544 calls them.
 *     The DiT is the network the reference's trainer swaps in for the U-Net behind the same DiffusionWrapper
 *     (trainers/trainer_use_gaussian_diff.py:84-86): in_channels = Cz + Cc (Cc = 0 and cond = NULL for an unconditional DiT),
 *     H = W = input_size, t as the handle's aux and no labels (none reaches the DiT through the wrapper).  Its output has Cz
 *     channels, or 2*Cz with learn_sigma (in_channels // 3 * 2, sic): the prediction is channels [0,Cz), the learned-range
 *     variance of (b, c, p) is channel Cz + c — read by DSD_MODE_A_DDPM with learned_range for any Cz, left unread by every other
 *     mode and loop (gaussian_diffusion.py:484-485).  DSD_PREC_F16 / DSD_PREC_BF16 apply to the network only: the state, the
 *     updates and the model output stay fp32.
 *     Any other block handle is rejected.  Each misfit (channels, size, output channels, learned_range without a variance half)
 *     is rejected with its numbers before any device work.
 * x is updated in place (in = x_T, out = the sample).  Schedules, first_step / n_steps (a sub-range of iterations, n_steps <= 0
 * = all, so a caller can time or checkpoint part of the chain), dsd_set_slice_ids and dsd_set_graph work alike for both kinds.
 * g: NULL, or classifier-free guidance (dsd_guidance, below).  inp: NULL, or the mask (dsd_inpaint, below). */
/* ---- classifier-free guidance -------------------------------------------------------------
 * The reference's unconditional_guidance_scale / unconditional_conditioning (DDIMSampler.sample, DPMSolverSampler.sample,
 * model_wrapper(guidance_type="classifier-free")).  Per step the denoiser is evaluated in ONE pass over 2B rows —
 * x_in = cat([x]*2), c_in = cat([uncond, cond]) (ddim.py:197-218) — in library-owned buffers, and the two output halves are
 * combined in front of the update, each sampler in its reference's order (fp32, nothing contracted):
 *   DDIM        out   = out_u   + s*(out_c   - out_u)    on the raw network outputs (ddim.py:219), then the B_DDIM update
 *   DPM-Solver  noise = noise_u + s*(noise_c - noise_u)  on the noise predictions each half forms from its own output and the
 *               shared x_t (dpm_solver_pytorch.py:324-332), then data prediction / thresholding (quantile per logical sample) /
 *               multistep update
 * The update writes x_{t-1} to both state rows of a sample.  Noise (fed: [steps,B,..]; Philox) and dsd_set_slice_ids are keyed by
 * the B logical samples, never by the 2B rows: a guided run with seed S draws the normals of the unguided run with seed S.
 * dsd_set_share_zero_streams, the stream lanes and dsd_set_graph replay work as in the unguided loops.
 * uncond: device, laid out like cond ([B,Cc,H,W]).  scale: host, one fp32 scale per executed step (a constant
 * unconditional_guidance_scale is the array filled with it; ucg_schedule is the array itself, ddim.py:165-167); n_scale must
 * equal the schedule's steps.  A step whose scale is 1.0 still runs the guided arithmetic.  The callers keep guidance OFF
 * (uncond None or scale 1.0, ddim.py:194) by passing g = NULL.  Where a loop takes g: dsd_sample in DSD_MODE_B_DDIM only (the
 * reference has no guidance in the family-A loops or the DDPM loop) and without a learned-range variance; dsd_sample_dpm,
 * dsd_sample_dpm_program (scale[k] belongs to network evaluation k), dsd_sample_plms and dsd_invert; dsd_calc_bpd takes none. */
typedef struct dsd_guidance {
    const float* uncond;   /* device, [B,Cc,H,W] like cond */
    const float* scale;    /* host, n_scale */
    int32_t n_scale;
} dsd_guidance;
/* ---- masked sampling (image-to-image, inpainting) --------------------------------------------
 * Masked sampling (DDIMSampler.sample(mask=, x0=), ddim.py:160-163; LatentDiffusion.p_sample_loop(mask=, x0=), ddpm.py:1085-1087):
 *   img_orig = sqrt_acp[t]*x0 + sqrt_1m_acp[t]*z        (q_sample, ddpm.py:356-359; coef[k][0], coef[k][1] of the iteration)
 *   x        = img_orig*mask + (1 - mask)*x             (mask 1 keeps x0, 0 samples)
 * DSD_MODE_B_DDIM blends BEFORE the network evaluation of every executed iteration (none after the last update);
 * DSD_MODE_B_DDPM blends AFTER every update, the last included, so the kept region ends as q_sample(x0, 0).  The family-A
 * loops have no mask in the reference and are rejected; so is a masked B_DDPM loop with guidance.
 * z: noise[k] of the fed [steps,B,Cz,H,W], or Philox normals of the stream (philox_seed, k + 2^32) — the update of iteration k
 * draws from (philox_seed, k) — keyed by logical sample and dsd_set_slice_ids like the update's noise.
 * The blend runs outside the captured network (dsd_set_graph), next to the update.  inp = NULL: unmasked.  dsd_sample and
 * dsd_sample_plms take inp (the latter blends in front of the first network evaluation of every iteration, as B_DDIM does). */
typedef struct dsd_inpaint {
    const float* x0;        /* device, [B,Cz,H,W] like the state */
    const float* mask;      /* device, [B,mask_channels,H,W] */
    int32_t mask_channels;  /* 1 (broadcast over the state's channels) or Cz */
    const float* noise;     /* device, [steps,B,Cz,H,W] blend noise, or NULL: Philox */
} dsd_inpaint;
/* ---- cross-attention and vector conditioning of the latent loops ----------------------------
 * The conditioning keys beside 'concat' that the reference's latent inference runs on: trainers/trainer_latent_diffusion.py:153-189
 * builds {"c_crossattn": [c], "c_adm": c_adm, "c_concat": [...]}, :492-524 samples with an unconditional_conditioning dict that
 * replaces c_crossattn and keeps c_adm / c_concat, DiffusionWrapper.forward (ldm/models/diffusion/ddpm.py:1328-1365) dispatches
 * 'crossattn', 'hybrid', 'adm', 'hybrid-adm', 'crossattn-adm', and UNetModel.forward
 * (ldm/modules/diffusionmodules/openaimodel.py:926-958) adds label_emb(y) (:696-712) to the time embedding.
 * dsd_set_conditioning installs one bundle on a DSD_BLOCK_UNET handle; NULL clears it.  The struct holds DEVICE pointers that
 * must stay valid until the bundle is cleared or replaced; the library reads them when a call binds:
 *   - every loop (dsd_sample ... dsd_calc_bpd, masked and guided alike) copies the parts once per call into buffers of its own
 *     of `rows` rows (rows = B, or 2B under a dsd_guidance: the unconditional twins first, as for the denoiser's input), which the network
 *     reads every step; a cached plan or a replayed graph sees stable addresses, a different `tokens` re-plans.  The context
 *     projections run every step, as in the reference.
 *   - dsd_block_forward on a DSD_BLOCK_UNET handle with label_emb reads y (B rows) from the bundle; its context stays aux2.
 * Checked before any device work, each misfit with its numbers: a spatial-transformer handle without a context and a context
 * for a handle without one; y if and only if the handle has label_emb; y_width against the handle's kind (0 for int classes,
 * 1 for "continuous", adm_in_channels for "sequential"); B against the call's; int labels outside [0, num_classes).  Under a
 * dsd_guidance every part that is set needs its unconditional twin (a twin equal to the conditional part is legal: the
 * reference's c_adm), and Cc = 0 is allowed when a context or y is there to be replaced (g->uncond may then be NULL).  DSD_BLOCK_DIT
 * and four-stream handles refuse any bundle. */
typedef struct dsd_conditioning {
    const float* context;        /* [B,tokens,context_dim], or NULL */
    const float* context_uncond; /* [B,tokens,context_dim], or NULL */
    int32_t tokens;              /* context length */
    const void* y;               /* int64 [B] (y_width 0) or fp32 [B,y_width], or NULL */
    const void* y_uncond;        /* like y, or NULL */
    int32_t y_width;             /* 0 = int64 labels, else fp32 floats per row */
    int32_t B;                   /* batch size */
} dsd_conditioning;
int dsd_set_conditioning(dsd_handle* h, const dsd_conditioning* c);
/* ---- intermediates of a loop ------------------------------------------------------------------
 * What the reference's samplers return beside the sample: the state every log_every_t steps and, from DDIM and PLMS, pred_x0
 * (intermediates of DDIMSampler.ddim_sampling ddim.py:149,178-183 and plms_sampling; LatentDiffusion.p_sample_loop
 * ddpm.py:1062,1089-1092; progressive_denoising's x0_partial :1034-1040; DDPMModel.p_sample_loop trainer_ddpm.py:451-456).
 * dsd_set_trace installs a trace on the handle, NULL clears it; the loops' own signatures stay as they are.  dsd_sample (all four
 * modes) and dsd_sample_plms honour it — unguided, guided and masked, for every denoiser they take:
 *   x[j]        the B logical rows of the state after the update of iteration keep[j], dense [B,Cz,H,W] whatever row stride
 *               the loop keeps its state at; under guidance one half of the 2B rows (both hold the same value).  A masked
 *               DSD_MODE_B_DDPM loop blends after the update and the entry is taken after that blend (ddpm.py:1085-1090);
 *               DSD_MODE_B_DDIM and PLMS blend in front of the evaluation, so theirs is the update's own result.
 *   pred_x0[j]  what the update kernel of iteration keep[j] forms anyway, written by that kernel (no extra pass): DDIM's
 *               pred_x0 from the guided e_t (v-models: predict_start_from_z_and_v), family B DDPM's clipped x_recon
 *               (p_sample(return_x0=True)), family A's clipped pred_xstart (the Cz state channels only under a learned-range
 *               variance), PLMS's pred_x0 of the step's final get_x_prev_and_pred_x0, after norm thresholding.
 * A call with first_step / n_steps writes the entries whose keep[j] lies in its window and no others: a split run fills the
 * buffers an unsplit one fills.  The snapshots lie outside the network graph of dsd_set_graph; with or without replay the
 * buffers hold the same bits, and so does the sample with or without a trace.  With no trace installed the loops launch what
 * they launch without this feature.
 * Rejected by dsd_set_trace, which then leaves the installed trace in place: n_keep < 1, keep not strictly ascending,
 * keep[0] < 0, both buffers NULL.  Rejected by the loop before any device work: a keep entry >= the schedule's steps.  (PLMS
 * with samples of a multiple of four floats wants pred_x0 16-byte aligned and says so.)  Every other loop (dsd_sample_dpm, dsd_sample_dpm_program, dsd_sample_dpm_adaptive_trial,
 * dsd_invert, dsd_calc_bpd) fails while a trace is installed instead of ignoring it.  The buffers must stay valid until the
 * trace is cleared or replaced. */
typedef struct dsd_trace {
    const int32_t* keep;  /* HOST, n_keep strictly ascending loop iterations k in [0, steps); copied by the call */
    int32_t n_keep;
    float* x;             /* DEVICE [n_keep,B,Cz,H,W] or NULL: the state as the reference appends it after iteration keep[j] */
    float* pred_x0;       /* DEVICE [n_keep,B,Cz,H,W] or NULL: the pred_x0 the reference's step returns at iteration keep[j] */
} dsd_trace;
int dsd_set_trace(dsd_handle* h, const dsd_trace* t);   /* NULL clears */

/* DDPM / DDIM (dsd_schedule).  noise: NULL -> on-device Philox4x32-10 N(0,1) from philox_seed; else [steps,B,Cz,H,W] pre-drawn
 * normals, noise[k] used at iteration k (parity mode). */
int dsd_sample(dsd_handle* h, const dsd_schedule* sched, const dsd_guidance* g, const dsd_inpaint* inp, const float* cond, int Cc,
               float* x, int Cz, const float* noise, uint64_t philox_seed, int B, int H, int W, int first_step, int n_steps,
               void* stream);
/* The fused sampler update alone (iteration k): model_out [B,Cm,H,W]; x updated in place; pred_xstart
 * (optional, [B,1,H,W]) receives the clipped x_0 prediction (the reference's out["pred_xstart"]).  A state of Cz channels is B*Cz
 * one-channel images; with a learned-range variance it is B images of (Cz*H) x W: the output row [mean(Cz), variance(Cz)] is
 * the one-channel layout at that height, and element (b, c, p) keeps its Philox counter b*Cz*H*W + c*H*W + p. */
int dsd_op_sampler_update(const dsd_schedule* sched, int k, const float* model_out, float* x, const float* noise,
                          uint64_t philox_seed, int B, int H, int W, float* pred_xstart, void* stream);

/* ---- DPM-Solver(++) multistep sampler -----------------------------------------------------
 * Replaces DPM_Solver(...).sample(method="multistep", order<=2) of Disc_diff/guided_diffusion/sampler.py:1017-1222
 * (call site GaussianDiffusion.dpm_solver_sample_loop, gaussian_diffusion.py:467-522) and of its twin
 * ldm/models/diffusion/dpm_solver_new/dpm_solver_pytorch.py (call site DPMSolverSampler.sample, sampler.py:86-101).
 * Iteration k evaluates the network once at model time t_input[k] and applies one update:
 *   m_k  = data prediction (x - sigma_k*eps)/alpha_k [data_pred=1, "dpmsolver++"] or eps [data_pred=0, "dpmsolver"],
 *          eps from the network output per `pred` (model_wrapper, sampler.py:247-265); with `thresholding` the data
 *          prediction is dynamically thresholded per sample (sampler.py:379-388)
 *   order[k] = 1:  x <- cx*x - cm*m_k                                   (dpm_solver_first_update :509-553)
 *   order[k] = 2:  x <- (cx*x - cm*m_k) - cd*(ir0*(m_k - m_{k-1}))      (multistep_dpm_solver_second_update :760-816)
 *   order[k] = 0:  x <- thresholded data prediction                     (denoise_to_zero_fn :503-507; forces data_pred)
 * coef[k*DSD_NCOEF + j]: 0 alpha_k  1 sigma_k  2 cx  3 cm  4 cd  5 ir0 (= 1/r0), all produced on the host with the
 * reference's fp32 torch expressions (NoiseScheduleVP, sampler.py:76-149). */
typedef struct dsd_dpm_schedule {
    int32_t steps;            /* network evaluations (= updates) */
    int32_t pred;             /* DSD_PRED_* : what the network predicts */
    int32_t data_pred;        /* 1 = dpmsolver++ (data prediction), 0 = dpmsolver (noise prediction) */
    int32_t thresholding;     /* dynamic thresholding of the data prediction */
    float threshold_ratio;    /* 0.995 */
    float threshold_max;      /* 1.0 */
    const float* coef;        /* host, steps*DSD_NCOEF */
    const float* t_input;     /* host, steps: fp32 model time (t - 1/N)*1000, sampler.py:236-245 */
    const int32_t* order;     /* host, steps */
} dsd_dpm_schedule;
/* A four-stream network with 2 output channels (learned sigma) contributes its first only (gaussian_diffusion.py:484-485); a DiT
 * its first Cz.  Dynamic thresholding takes the quantile per sample over all Cz*H*W elements (dynamic_thresholding_fn,
 * ldm/models/diffusion/dpm_solver_new/dpm_solver_pytorch.py:418). */
int dsd_sample_dpm(dsd_handle* h, const dsd_dpm_schedule* sched, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz,
                   int B, int H, int W, void* stream);
/* Iteration k's post-network part alone: model_out [B,Cm,H,W], x updated in place, m_cur [B,1,H,W] receives m_k,
 * m_prev = m_{k-1} (may be NULL when order[k] < 2). */
int dsd_op_dpm_step(const dsd_dpm_schedule* sched, int k, const float* model_out, int Cm, float* x, float* m_cur,
                    const float* m_prev, int B, int H, int W, void* stream);
/* One guided update alone (iteration k, DSD_MODE_B_DDIM).  out_uncond / out_cond: the two [B,Cz,H,W] halves of the network
 * output.  x: the 2B-row state, logical sample b at x + b*x_row_stride and x + (B+b)*x_row_stride (x_row_stride = 0: Cz*H*W,
 * i.e. a contiguous [2B,Cz,H,W]); the first B rows are read, all 2B receive x_{t-1}.  noise [B,Cz,H,W] or NULL (Philox),
 * pred_xstart (optional) [B,Cz,H,W]. */
int dsd_op_sampler_update_guided(const dsd_schedule* sched, int k, const float* out_uncond, const float* out_cond, float scale,
                                 float* x, int64_t x_row_stride, const float* noise, uint64_t philox_seed, int B, int Cz, int H,
                                 int W, float* pred_xstart, void* stream);
/* Iteration k's post-network part of the guided DPM-Solver loop: out_uncond / out_cond [B,Cm*Cz,H,W] (Cm = 2 needs Cz = 1), x
 * as in dsd_op_sampler_update_guided, m_cur / m_prev [B,Cz,H,W]; the thresholding quantile is per logical sample over Cz*H*W. */
int dsd_op_dpm_step_guided(const dsd_dpm_schedule* sched, int k, const float* out_uncond, const float* out_cond, int Cm, float scale,
                           float* x, int64_t x_row_stride, float* m_cur, const float* m_prev, int B, int Cz, int H, int W,
                           void* stream);
/* ---- the DPM-Solver family as a program of evaluations -------------------------------------
 * Replaces DPM_Solver(...).sample / .inverse of Disc_diff/guided_diffusion/sampler.py:1001-1217 (and of the twin
 * dpm_solver_pytorch.py) for method = "multistep" with order 1..3 (:818-868 adds the third), "singlestep" and "singlestep_fixed"
 * (:555-758, orders and times from get_orders_and_timesteps_for_singlestep_solver :445-501), with return_intermediate.
 * dsd_sample_dpm and its schedule stay as they are; this is a second way in, for everything they do not cover.
 * The program is a host array of network EVALUATIONS.  Evaluation k runs the network at model time t_input[k] on the current
 * state, forms the model value m from the output as DPM_Solver.model_fn does — noise prediction per `pred` with alpha[k] /
 * sigma[k] and the state the network read, data prediction with `data_pred` (always for DSD_DPM_MS0), dynamic thresholding per
 * logical sample — stores it in history plane slot[4k] (three planes, 0..2; nothing is rotated) and writes the next state:
 *   kind                 ma, mb, mc = planes slot[4k+1..3]          c = coef + k*DSD_DPM_NCOEF
 *   DSD_DPM_MS0          x = ma                                                          (denoise_to_zero_fn :503-507)
 *   DSD_DPM_MS1          x = c0*x - c1*ma                                                (:509-553)
 *   DSD_DPM_MS2          x = (c0*x - c1*ma) - c2*(c3*(ma - mb))                          (:760-816; ma = m_k, mb = m_{k-1})
 *   DSD_DPM_MS3          D1_0 = c4*(ma - mb), D1_1 = c5*(mb - mc), D1 = D1_0 + c6*(D1_0 - D1_1), D2 = c7*(D1_0 - D1_1)
 *                        x = ((c0*x - c1*ma) + c2*D1) - c3*D2                            (:818-868; mc = m_{k-2})
 *   DSD_DPM_SS_S1        base = x;  x = c0*base - c1*ma                                  (x_s1; ma = model_s)
 *   DSD_DPM_SS_S2        x = (c0*base - c1*ma) - c2*(mb - ma)                            (x_s2 of the third order; mb = model_s1)
 *   DSD_DPM_SS_T2 / _T3  x = (c0*base - c1*ma) - c2*(mb - ma)                            (x_t, 'dpmsolver'; mb = model_s1 / model_s2)
 *   DSD_DPM_SS_T3_TAYLOR D1_0 = c4*(mb - ma), D1_1 = c5*(mc - ma), D1 = (c7*D1_0 - c6*D1_1)/c8, D2 = 2*(D1_1 - D1_0)/c8
 *                        x = ((c0*base - c1*ma) + c2*D1) - c3*D2                         (x_t, 'taylor' :705-714; c6 r1, c7 r2, c8 r2-r1)
 * A singlestep step of order 1 is DSD_DPM_MS1.  The base state x_s of a singlestep step lives in a library plane from SS_S1
 * until the step's x_t is written.  Every coefficient is a host scalar: the value of the reference's fp32 torch expression on
 * its (1,)-tensors, with the sign the reference writes in front of a term folded in where the two algorithm types differ.
 * keep[k] != 0: the state after evaluation k is an intermediate (sample(return_intermediate=True) appends it, :1147-1213).
 * Rejected before any device work, each with its numbers: a kind outside the table, a slot outside 0..2, a multistep update
 * that reads a plane no earlier evaluation wrote, stage kinds out of sequence (SS_S2 / SS_T2 not after SS_S1, SS_T3* not after
 * SS_S2, anything but the next stage inside a step, a program that ends inside a step), null arrays, threshold_ratio outside
 * [0,1], a guidance whose n_scale differs from n_eval. */
enum { DSD_DPM_MS0 = 0, DSD_DPM_MS1 = 1, DSD_DPM_MS2 = 2, DSD_DPM_MS3 = 3, DSD_DPM_SS_S1 = 4, DSD_DPM_SS_S2 = 5, DSD_DPM_SS_T2 = 6,
       DSD_DPM_SS_T3 = 7, DSD_DPM_SS_T3_TAYLOR = 8 };
#define DSD_DPM_NCOEF 9   /* the widest row: DSD_DPM_SS_T3_TAYLOR, c0..c8 */
typedef struct dsd_dpm_program {
    int32_t n_eval;           /* network evaluations */
    int32_t pred;             /* DSD_PRED_* */
    int32_t data_pred;        /* 1 = dpmsolver++, 0 = dpmsolver */
    int32_t thresholding;
    float threshold_ratio;
    float threshold_max;
    const int32_t* kind;      /* host, n_eval: DSD_DPM_* */
    const float* t_input;     /* host, n_eval: fp32 model time of the evaluation */
    const float* alpha;       /* host, n_eval: marginal alpha / sigma at the evaluation's time */
    const float* sigma;
    const float* coef;        /* host, n_eval*DSD_DPM_NCOEF */
    const int32_t* slot;      /* host, n_eval*4: plane written, planes read as ma, mb, mc (unread ones: any value in 0..2) */
    const int32_t* keep;      /* host, n_eval, or NULL = none kept */
} dsd_dpm_program;
/* g carries one scale per evaluation.  intermediates: NULL, or device [n_kept,B,Cz,H,W] (n_kept = the nonzero keep entries),
 * filled in order. */
int dsd_sample_dpm_program(dsd_handle* h, const dsd_dpm_program* prog, const dsd_guidance* g, const float* cond, int Cc, float* x,
                           int Cz, int B, int H, int W, float* intermediates, void* stream);
/* Evaluation k's post-network part alone (host loops, kernel-level tests).  out_cond [B,Cm*Cz,H,W] is the network output
 * (Cm = 1, or 2 with a learned sigma in the second half of the channels, which is left unread; any Cz); out_uncond NULL, or the unconditional half: then x holds 2B rows as in dsd_op_dpm_step_guided and both rows of a sample are
 * written.  hist: the three history planes [3,B,Cz,H,W]; base [B,Cz,H,W] (may be NULL for the multistep kinds). */
int dsd_op_dpm_eval(const dsd_dpm_program* prog, int k, const float* out_uncond, const float* out_cond, int Cm, float scale, float* x,
                    int64_t x_row_stride, float* hist, float* base, int B, int Cz, int H, int W, void* stream);
/* ---- adaptive step-size DPM-Solver: one trial ------------------------------------------------
 * Replaces the body of the while loop of DPM_Solver.dpm_solver_adaptive (sampler.py:921-980 and the twin dpm_solver_pytorch.py:
 * 958-1012); the loop itself — the step size h, accept or reject, the end test — stays with the host, which needs the error of
 * every trial to decide the next.  prog is exactly ONE singlestep step from s to t: DSD_DPM_SS_S1, DSD_DPM_SS_T2 (order 2, r1 =
 * 0.5) or DSD_DPM_SS_S1, DSD_DPM_SS_S2, DSD_DPM_SS_T3 / _T3_TAYLOR (order 3, r1 = 1/3, r2 = 2/3), i.e. `order` network
 * evaluations, run by the driver of dsd_sample_dpm_program for every denoiser it takes, guided (g carries `order` scales) or
 * not, with thresholding, with or without graph replay of the network.  lower_coef = {c0, c1, c2} is the update of order - 1
 * from the same model values: x_lower = c0*x_s - c1*model_s (order 2; c2 = 0), or (c0*x_s - c1*model_s) - c2*(model_s1 - model_s)
 * (order 3: the second-order singlestep update with r1 = 1/3, 'dpmsolver' or 'taylor' coefficient in c2); c0 and c1 are those
 * of the step's last row.  After the step one pass forms x_lower, delta = max(atol, rtol*max(|x_lower|, |x_prev|)) and, per
 * sample b, err[b] = sqrt(mean(((x_higher - x_lower)/delta)^2)) (fp64 sums in a fixed order: two runs give the same bits).
 * x [B,Cz,H,W] (device): x_s on entry, x_higher on return — also when the caller then rejects the trial, so a caller that may
 * reject passes a copy.  x_prev (device, in), x_lower (device, out): [B,Cz,H,W].  err (HOST, B floats) is copied back through a
 * pinned buffer of the handle: the one synchronisation of the trial, outside any graph capture.  The trial is accepted when
 * max_b err[b] <= 1.
 * Rejected before any device work, each with its numbers: everything dsd_sample_dpm_program rejects; a program that is not
 * exactly one singlestep step of order 2 or 3 (one that keeps intermediates has no output for them); a lower-order row whose c0 / c1 differ from the
 * step's or whose c2 is non-zero for order 2 / not finite for order 3; atol <= 0; rtol < 0; null arrays. */
int dsd_sample_dpm_adaptive_trial(dsd_handle* h, const dsd_dpm_program* prog, const dsd_guidance* g, const float* cond, int Cc,
                                  const float* lower_coef, float atol, float rtol, float* x, const float* x_prev, float* x_lower, int Cz,
                                  int B, int H, int W, float* err, void* stream);
/* The error estimate alone on caller-supplied planes (kernel-level tests): lower_order 1 or 2, base / ma / mb (NULL for lower_order
 * 1) / x_prev / x_lower [B,Cz,H,W], x_higher row b at x_higher + b*x_row_stride (0 = Cz*H*W; the first B rows of a guided 2B-row
 * state), err: DEVICE array of B floats. */
int dsd_op_dpm_adaptive_error(int lower_order, const float* lower_coef, float atol, float rtol, const float* base, const float* ma,
                              const float* mb, const float* x_higher, int64_t x_row_stride, const float* x_prev, float* x_lower,
                              float* err, int B, int Cz, int H, int W, void* stream);
/* ---- DDIM inversion (DDIMSampler.encode, ddim.py:263-308) ----------------------------------
 * Iteration i evaluates the network at model time t_model[i] — the reference passes the loop index i itself (:282), not a
 * timestep of the schedule; the caller fills t_model accordingly — and applies x <- coef[2i]*x + coef[2i+1]*e  (xt_weighted + weighted_noise_pred, :292-295), e the network output or, with guidance,
 * e_u + s*(e_c - e_u) (:287-290).  coef: host, produced with the reference's expressions and dtypes, rounded to fp32 once. */
typedef struct dsd_invert_schedule {
    int32_t steps;
    const float* coef;      /* host, steps*2: cx, ce */
    const float* t_model;   /* host, steps */
} dsd_invert_schedule;
/* x: in = x0, out = the encoded state, in place. */
int dsd_invert(dsd_handle* h, const dsd_invert_schedule* sched, const dsd_guidance* g, const float* cond, int Cc, float* x, int Cz,
               int B, int H, int W, int first_step, int n_steps, void* stream);
/* The blend alone.  x: state rows at x + b*x_row_stride (0: Cz*H*W); guided != 0: the 2B-row state, row b is read, rows b and
 * B+b are written.  noise [B,Cz,H,W] or NULL: Philox stream (philox_seed, step + 2^32). */
int dsd_op_mask_blend(float a, float s, const float* x0, const float* mask, int mask_channels, float* x, int64_t x_row_stride,
                      int guided, const float* noise, uint64_t philox_seed, uint64_t step, int B, int Cz, int H, int W,
                      void* stream);
/* q_sample with per-row coefficients (LatentDiffusion.q_sample, DDIMSampler.stochastic_encode): out_b = a[b]*x0_b + s[b]*z_b;
 * a, s: device [B]; out rows at out + b*out_row_stride (0: contiguous). */
int dsd_op_q_sample(const float* a, const float* s, const float* x0, const float* noise, uint64_t philox_seed, uint64_t step,
                    float* out, int64_t out_row_stride, int B, int Cz, int H, int W, void* stream);
/* One inversion step.  out_uncond == NULL: x (B rows) <- cx*x + ce*out_cond; else the guided step on the 2B-row state. */
int dsd_op_ddim_invert_step(float cx, float ce, const float* out_uncond, const float* out_cond, float scale, float* x,
                            int64_t x_row_stride, int B, int Cz, int H, int W, void* stream);
/* ---- variational bound in bits per dimension ------------------------------------------------
 * Replaces GaussianDiffusion.calc_bpd_loop / _vb_terms_bpd / _prior_bpd (Disc_diff/guided_diffusion/gaussian_diffusion.py:
 * 788-819, 922-991; losses.py) on a DSD_MODE_A_DDPM schedule.  Iteration k (t = steps-1-k) forms x_t = c0*x_start + c1*z in a
 * state of the loop's own (x_start is read only and comes out untouched), evaluates the network once at t_model[k] and reduces,
 * per sample, over the Cz*H*W elements:
 *   vb          mean normal_kl(true posterior mean / post_log_var[k], model mean / model log-variance) / ln 2, or at t = 0
 *               mean -discretized_gaussian_log_likelihood(x_start, model mean, 0.5 * model log-variance) / ln 2
 *   xstart_mse  mean (pred_xstart - x_start)^2
 *   mse         mean (eps - z)^2,  eps = (c2*x_t - pred_xstart) / c3
 * pred_xstart (clipped with clip_denoised), the model mean and the fixed or learned-range log-variance are the values of
 * dsd_sample's update; every product and sum is one rounded fp32 operation in the reference's order.  The sums are formed in
 * fp64 from fixed per-block partials added in index order (no atomics): two runs are bit-identical.
 * z: noise[k] of the fed [steps,B,Cz,H,W], or the Philox normals of stream (philox_seed, k + 2^32), keyed by logical sample and
 * dsd_set_slice_ids.  Column k of the [B,steps] outputs is iteration k: the reference's stack order.  first_step / n_steps
 * and dsd_set_graph work as in dsd_sample; columns outside the range are left as they are.
 * Rejected before any device work: a mode other than DSD_MODE_A_DDPM, null outputs or a null post_log_var, learned_range on a
 * model without a variance half, and the channel / shape / slice-id misfits of the sampling loops.  It takes no dsd_guidance:
 * the reference evaluates the bound unguided. */
typedef struct dsd_bpd {
    const float* post_log_var; /* host, steps: posterior_log_variance_clipped[t] in iteration order (fp32 of the float64 table) */
    float* vb;                 /* device, [B,steps] */
    float* xstart_mse;         /* device, [B,steps] */
    float* mse;                /* device, [B,steps] */
    float* prior;              /* device, [B], or NULL: _prior_bpd from coef[0] (sqrt_acp at T-1) and prior_log_var */
    float prior_log_var;       /* log(1 - alphas_cumprod[T-1]) */
} dsd_bpd;
int dsd_calc_bpd(dsd_handle* h, const dsd_schedule* sched, const dsd_bpd* bpd, const float* cond, int Cc, const float* x_start,
                 int Cz, const float* noise, uint64_t philox_seed, int B, int H, int W, int first_step, int n_steps, void* stream);
/* The terms of iteration k alone, on caller buffers: model_out rows at model_out + b*out_row_stride (0: Cz*H*W, or 2*Cz*H*W
 * with learned_range), x_t rows at x_t + b*x_row_stride (0: Cz*H*W), x_start and noise [B,Cz,H,W] (noise NULL: Philox stream
 * (philox_seed, k + 2^32)).  Sample b's scalars go to vb / xstart_mse / mse [b*term_stride] (0: 1; each may be NULL); mean /
 * log_variance / pred_xstart ([B,Cz,H,W], each may be NULL) receive p_mean_variance's planes. */
int dsd_op_vlb_terms(const dsd_schedule* sched, int k, float post_log_var, const float* model_out, int64_t out_row_stride,
                     const float* x_t, int64_t x_row_stride, const float* x_start, const float* noise, uint64_t philox_seed,
                     float* vb, float* xstart_mse, float* mse, int64_t term_stride, float* mean, float* log_variance,
                     float* pred_xstart, int B, int Cz, int H, int W, void* stream);
/* _prior_bpd: prior[b] = mean normal_kl(sqrt_acp*x_start_b, log_1m_acp, 0, 0) / ln 2. */
int dsd_op_prior_bpd(float sqrt_acp, float log_1m_acp, const float* x_start, float* prior, int B, int Cz, int H, int W,
                     void* stream);
/* ddim_reverse_sample (:667-703) after the network evaluation of iteration k of a family-A schedule: x (rows at x +
 * b*x_row_stride, 0: Cz*H*W) <- pred_xstart*sqrt(alpha_bar_next) + sqrt(1 - alpha_bar_next)*eps, eps = (c2*x - pred_xstart)/c3,
 * in place; pred_xstart (optional, [B,Cz,H,W]) receives the clipped prediction. */
int dsd_op_ddim_reverse_step(const dsd_schedule* sched, int k, float alpha_bar_next, const float* model_out,
                             int64_t out_row_stride, float* x, int64_t x_row_stride, float* pred_xstart, int B, int Cz, int H,
                             int W, void* stream);
/* ---- the denoising loss, forward only --------------------------------------------------------
 * Replaces GaussianDiffusion.training_losses (Disc_diff/guided_diffusion/gaussian_diffusion.py:821-920 and
 * training_project/utils/gaussian_diffusion.py:824-), DDPM.p_losses / get_loss / get_v (ldm/models/diffusion/ddpm.py:361-415)
 * and LatentDiffusion.p_losses (:892-927) as an evaluation: no gradient, no optimiser.  It is the one evaluation with a
 * timestep per SAMPLE, so whatever depends on t arrives as device rows of B values, gathered by the caller from its tables.
 * One call: x_t[b] = a[b]*x_start[b] + s[b]*z[b] in a state of the call's own, one network evaluation with t_model[b] per row,
 * then per sample, over the Cz*H*W elements, into row b of terms [B, DSD_LOSS_NTERMS]:
 *   DSD_LOSS_TERM_MSE   mean kind(target - prediction); target: z, x_start, or a[b]*z - s[b]*x_start (get_v);
 *                       kind: DSD_LOSS_L2 d^2, DSD_LOSS_L1 |d|, DSD_LOSS_CHARBONNIER sqrt(d^2 + 1e-6) (L1_Charbonnier_loss)
 *   DSD_LOSS_TERM_VB    (vlb_coef != NULL) _vb_terms_bpd with clip_denoised = False: sample b's DSD_MODE_A_DDPM coefficient row
 *                       vlb_coef[b], post_log_var[b], and the decoder NLL where decoder[b] != 0 (t == 0); with learned_range the
 *                       variance half of the output is read in place
 *   DSD_LOSS_TERM_COM / DSD_LOSS_TERM_DIST   (dsd_create_disc handles) the sums over the six pairs of the four com_h / dist_h
 *                       bottleneck tensors of mean (f_i - f_j)^2, read straight from the workspace
 * Columns a call does not compute are left as they are.  z: noise [B,Cz,H,W], or NULL: the Philox normals of stream
 * (philox_seed, step + 2^32) — the ones dsd_op_q_sample draws with the same seed and step.  Every reduction adds fixed
 * per-block fp64 partials in index order (no atomics): two calls agree bit for bit.  The handle picks the denoiser as in the
 * loops (cond / Cc / Cz as there; dsd_set_conditioning applies); after the first call of a shape nothing is allocated.
 * Rejected before any device work: null rows or results, an unknown pred / kind, learned_range on a model without a variance
 * half, an installed trace, and the channel / shape / slice-id misfits of the loops. */
enum { DSD_LOSS_L2 = 0, DSD_LOSS_L1 = 1, DSD_LOSS_CHARBONNIER = 2 };
enum { DSD_LOSS_TERM_MSE = 0, DSD_LOSS_TERM_VB = 1, DSD_LOSS_TERM_COM = 2, DSD_LOSS_TERM_DIST = 3, DSD_LOSS_NTERMS = 4 };
typedef struct dsd_loss {
    int32_t target;            /* DSD_PRED_*: the target of the mse term (training_losses reads it off `parameterization`) */
    int32_t pred;              /* DSD_PRED_*: what the vb term's p_mean_variance reads the output as (model_mean_type; the two
                                * differ in the reference for predict_xstart with parameterization "eps") */
    int32_t kind;              /* DSD_LOSS_* */
    int32_t learned_range;     /* the output carries a variance half [Cz,2Cz) (read by the vb term only) */
    const float* t_model;      /* device, [B]: the value the network receives as t */
    const float* a;            /* device, [B]: sqrt_alphas_cumprod[t] */
    const float* s;            /* device, [B]: sqrt_one_minus_alphas_cumprod[t] */
    const float* vlb_coef;     /* device, [B,DSD_NCOEF], or NULL: no vb term */
    const float* post_log_var; /* device, [B]: posterior_log_variance_clipped[t] (with vlb_coef) */
    const int32_t* decoder;    /* device, [B]: t == 0 (with vlb_coef) */
    float* terms;              /* device, [B,DSD_LOSS_NTERMS] */
} dsd_loss;
int dsd_eval_loss(dsd_handle* h, const dsd_loss* spec, const float* cond, int Cc, const float* x_start, int Cz, const float* noise,
                  uint64_t philox_seed, uint64_t step, int B, int H, int W, void* stream);
/* The mse term alone, on caller buffers: model_out rows at model_out + b*out_row_stride (0: Cz*H*W); x_start (unread by the eps
 * target) and noise (unread by the x0 target; NULL: Philox as above) [B,Cz,H,W]; a, s device [B] (v target only); loss[b*loss_stride]
 * (0: 1). */
int dsd_op_loss_rows(int pred, int kind, const float* model_out, int64_t out_row_stride, const float* x_start, const float* noise,
                     uint64_t philox_seed, uint64_t step, const float* a, const float* s, float* loss, int64_t loss_stride, int B,
                     int Cz, int H, int W, void* stream);
/* out[b] = sum over the pairs of the n_feats (2, 3 or 4) device tensors feats[i] [B,n] of mean (f_i - f_j)^2, pairs and fp32 sums in
 * the reference's order: (1,2) + (2,3) + (1,3), then + ((1,4) + (2,4) + (3,4)). */
int dsd_op_pair_mse_rows(const float* const* feats, int n_feats, int B, int64_t n, float* out, void* stream);
/* dsd_op_vlb_terms with a timestep per sample: coef device [B,DSD_NCOEF], post_log_var device [B], decoder device [B] (t == 0).
 * Same device functions; with one t shared by the batch the results are dsd_op_vlb_terms' bits. */
int dsd_op_vlb_terms_rows(int pred, int learned_range, int clip_denoised, const float* coef, const float* post_log_var,
                          const int32_t* decoder, const float* model_out, int64_t out_row_stride, const float* x_t,
                          int64_t x_row_stride, const float* x_start, const float* noise, uint64_t philox_seed, uint64_t step,
                          float* vb, float* xstart_mse, float* mse, int64_t term_stride, int B, int Cz, int H, int W, void* stream);
/* ---- the disentanglement losses over the bottleneck heads, forward only ------------------------
 * Replaces training_losses(disentangle=) (training_project/utils/gaussian_diffusion.py:907-975), get_disentangle_loss
 * (:1056-1094), ContrastiveLoss(contrast_mode='all', contrastive_method='cl') (loss_function/contrastive_loss.py) and the p = 1
 * distance of trainers/trainer_ds_diff.py:341-354 as an evaluation.  n_views device tensors views[v] [B,n], sample b of view v at
 * views[v] + b*row_stride (0: n), are the R = n_views*B rows r = v*B + b of torch.cat(torch.unbind(features, 1), 0); labels is
 * device int32 [R] in that order.  One pass over the features forms the R x R matrix of fp64 dot products G (DSD_CONTRAST_L1: of
 * sum |x_i - x_j|) from fixed per-slice fp64 partials added in index order (no atomics: two calls agree bit for bit), then
 *   cos_ij = G_ij / (max(sqrt G_ii, 1e-8) * max(sqrt G_jj, 1e-8)),   d_ij = sqrt(max(G_ii + G_jj - 2 G_ij, 0))   (fp64)
 *   DSD_CONTRAST_CL     logits = fp32(cos) / temperature;  loss = -mean_i [ sum_{j != i, label_j == label_i} (logits_ij -
 *                       log sum_{j != i} exp(logits_ij)) / (#positives_i + 1e-6) ]  (no maximum is subtracted, as the reference)
 *   DSD_CONTRAST_EU     l = fp32(d) / n;  loss = sum_{same label, i != j} l / sum_{different label} l;  logits = 2 l - 1
 *   DSD_CONTRAST_EU_CL  loss = loss_eu + 0.05 * loss_cl;  logits = the cosine logits
 *   DSD_CONTRAST_L1     the EU ratio on l = fp32(G) / n;  logits = l
 * into loss[1] and logits [R,R] (fp32, device).  R is at most DSD_CONTRAST_MAX_ROWS (seven views of a batch of 32 are 224),
 * n_views at most DSD_CONTRAST_MAX_VIEWS.  Rejected before any device work: null pointers, an unknown mode, temperature <= 0 in
 * the two cosine modes, fewer than 2 or more than DSD_CONTRAST_MAX_ROWS rows, row_stride < n. */
enum { DSD_CONTRAST_CL = 0, DSD_CONTRAST_EU = 1, DSD_CONTRAST_EU_CL = 2, DSD_CONTRAST_L1 = 3 };
enum { DSD_CONTRAST_MAX_VIEWS = 8, DSD_CONTRAST_MAX_ROWS = 256 };
int dsd_op_contrast_rows(const float* const* views, int n_views, int B, int64_t n, int64_t row_stride, const int32_t* labels,
                         int mode, float temperature, float* loss, float* logits, void* stream);
/* A rider on dsd_eval_loss, as dsd_set_trace is one on the loops: with it installed, dsd_eval_loss on a dsd_create handle
 * (DSUnetModel) keeps the ten head tensors of the forward in the workspace (style[3], content[3], anatomy[2], lesion[2]; nothing
 * is exported and the two n_style / n_content heads of dsd_forward's feature mode are not evaluated), plans without zero-stream
 * sharing, and after the forward runs the op above twice, in the reference's view order (:917-918, :940):
 *   loss[0], logits_cs  [6B,6B]   content[3] + style[3]               labels_cs  [6B], temperature_cs  (the reference: 0.05)
 *   loss[1], logits_sal [7B,7B]   style[3] + anatomy[2] + lesion[2]   labels_sal [7B], temperature_sal (the reference: 0.1)
 * The dsd_loss terms are computed as without it.  NULL clears.  dsd_set_disentangle rejects null pointers, an unknown mode
 * (DSD_CONTRAST_L1 included: the reference's training_losses has no such form) and non-positive temperatures in the cosine
 * modes; dsd_eval_loss then fails before any device work on every other handle kind (dsd_create_disc, block handles), when
 * n_labels_cs != 6B or n_labels_sal != 7B, and when 7B exceeds DSD_CONTRAST_MAX_ROWS.  Without a rider dsd_eval_loss launches
 * exactly what it launched before there was one. */
typedef struct dsd_disentangle {
    int32_t mode;                  /* DSD_CONTRAST_CL / _EU / _EU_CL */
    float temperature_cs;
    float temperature_sal;
    const int32_t* labels_cs;      /* device, [n_labels_cs] */
    int32_t n_labels_cs;           /* 6B of the dsd_eval_loss calls that follow */
    const int32_t* labels_sal;     /* device, [n_labels_sal] */
    int32_t n_labels_sal;          /* 7B */
    float* loss;                   /* device, [2]: c_s, s_a_l */
    float* logits_cs;              /* device, [6B,6B] */
    float* logits_sal;             /* device, [7B,7B] */
} dsd_disentangle;
int dsd_set_disentangle(dsd_handle* h, const dsd_disentangle* spec);   /* NULL clears */
/* ---- validation metrics of a batch of samples: MAE / MSE sums, Gaussian SSIM, the MS-SSIM scale table ------------
 * Replaces, as an evaluation, monai.metrics.MAEMetric and SSIMMetric(spatial_dims=2[, data_range=2.0]) at the end of every
 * trainer's validation_step (trainers/trainer_ddpm.py:79-80,529-532, trainers/trainer_use_gaussian_diff.py:99-102,519-584 and
 * the other five trainers) and the per-slice MS-SSIM behind the "ssim" column of the inference metric table
 * (inference/test_metrics.py:249-274).  PARITY UNPINNED: neither MONAI nor torchmetrics can be run beside this library; the
 * formulas below are their published definitions, pinned against the float64 host restatements host_io.ssim_gaussian and
 * host_io.multiscale_structural_similarity.
 * pred / target: device fp32 [B,C,H,W].  Everything from the load onward is fp64.
 *   pre (host, NULL or 7 doubles mean_p, div_p, mean_t, div_t, add, lo, hi):  x <- min(max((x - mean) / div + add, lo), hi) at
 *       the load, one (mean, div) for pred and one for target; the 12-bit rescale of test_metrics.py:21-26 is
 *       (mean, std / 400, 2048, 1e-10, 4095) and gives the host's bits.  elem and the range are taken after it.
 *   elem_out (device fp64 [B,6]):  sum |p - t|, sum (p - t)^2, min t, max t, min p, max p over the C*H*W elements of a sample.
 *   R = data_range, or with data_range == 0 the sample's own max(max p - min p, max t - min t);  c1 = (0.01 R)^2, c2 = (0.03 R)^2.
 *   window g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum, 11 taps, applied along the rows, then along the columns, at the
 *       (H - 10) x (W - 10) positions where it lies inside the image.  With E[.] that blur:
 *       mx = E[x], my = E[y], sx = E[xx] - mx^2, sy = E[yy] - my^2, sxy = E[xy] - mx my               (biased)
 *       cs = (2 sxy + c2) / (sx + sy + c2),   ssim = (2 mx my + c1) / (mx^2 + my^2 + c1) * cs
 *   scale_out (device fp64 [B,scales,2]):  per sample and scale the mean of ssim and the mean of cs over all channels and
 *       window positions, NOT clamped (MS-SSIM clamps at 0, SSIMMetric does not: that stays with the caller).  Scale s + 1 is
 *       the 2 x 2 average of scale s, a trailing odd row / column dropped (F.avg_pool2d), kept in fp64.
 * A map workgroup owns DSD_METRICS_TILE_W x DSD_METRICS_TILE_H window positions of one channel.  Every sum is formed from fixed
 * per-workgroup fp64 partials folded in a fixed order; no atomics: two calls agree bit for bit.  Scratch is allocated and
 * released by the call.  Rejected before any device work: null pointers, scales outside 1..DSD_METRICS_MAX_SCALES,
 * min(H, W) >> (scales - 1) below 11, B > 65535, C*H*W > 2^30, data_range negative or not finite, pre with a div of 0 or
 * lo > hi. */
enum { DSD_METRICS_MAX_SCALES = 5, DSD_METRICS_TILE_W = 32, DSD_METRICS_TILE_H = 16 };
typedef struct dsd_image_metrics {
    const float* pred;             /* device, [B,C,H,W] */
    const float* target;           /* device, [B,C,H,W] */
    int32_t B, C, H, W;
    int32_t scales;                /* 1..DSD_METRICS_MAX_SCALES */
    double data_range;             /* > 0, or 0: per sample */
    const double* pre;             /* host, NULL or [7] */
    double* scale_out;             /* device, [B,scales,2] */
    double* elem_out;              /* device, [B,6] */
} dsd_image_metrics;
int dsd_op_image_metrics(const dsd_image_metrics* spec, void* stream);
/* ---- The metric table of a volume on the device: masked errors, exact median, PSNR, box-window SSIM ----------------------------
 * The columns inference/get_metric.py, get_metric_BraTs.py, get_metric_lh.py and get_metric_rm.py fill per volume id from the array
 * functions of inference/test_metrics.py (:21-26,149-246,378-400), restated from the float64 host functions of host_io.py (nrmse,
 * mape, smape, logac, medsymac, psnr, ssim); where this text and such a function differ, the function wins.
 * target / pred: device [D,H,W], float (elem_is_double 0) or double (1).  mask: device uint8 [D,H,W], non-zero = inside, or NULL.
 * Everything from the load onward is fp64.
 *   M = the voxels with mask != 0 (every voxel without a mask); per axis lo / hi = the smallest / largest index holding a voxel
 *       of M.  The crop is [lo, hi) on every axis: the upper bound is EXCLUSIVE, as the reference slices, so the last plane that
 *       holds mask voxels is dropped (without a mask the crop is [0, n - 1)).
 *   Z = the crop of where(m, x, 0);  R = the crop of the raw volume with a mask, the whole volume without one.
 *   s12(x) = min(max(((x - mean) / (std / 400.)) + 2048., 1e-10), 4095), mean and population std of the domain's own values, pred
 *       and target each their own;  ts, ps = s12 of target and pred over M.
 *   nrmse = sqrt(mean_M (t - p)^2) / (max_M t - min_M t)           mape  = mean_M |ts - ps| / |ts|
 *   smape = mean_M |ps - ts| / (|ts| + |ps|)                       logac = mean_M l,  l = |log(ps / ts)|
 *   medsymac = exp(median_M l) - 1, the median the middle order statistic, or half the sum of the two middle ones for an even n_M
 *   psnr = 10 log10((max_Z tz - min_Z tz)^2 / mean_Z (tz - pz)^2)
 *   ssim3d (win > 0) = the mean over every window position inside R of
 *       ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  x = s12_R(t), y = s12_R(p), u the plain win^3 window
 *       means, v the sample (co)variances win^3 / (win^3 - 1) (uxx - ux^2), C = (K (max x - min x))^2, K = 0.01, 0.03.
 * out (device fp64 [DSD_VOLUME_NOUT]): the slots below; DSD_VOLUME_STATUS holds the status bits as a double.  A condition that
 * leaves a value undefined sets its bit and the affected slots are NaN: an empty mask (all but n_M), a crop with a side of 0
 * (psnr, the Z values and with a mask ssim3d and the R values), a zero std of target or pred in M (mape, smape, logac, medsymac) or,
 * with win > 0, in R (ssim3d), a zero range under nrmse or psnr, with win > 0 a side of R below win (ssim3d).
 * The median is an exact selection (dsd_op_kth_double's kernels on the l array, padded with +inf outside M).  A workgroup of the
 * ssim3d row kernel owns DSD_VOLUME_TILE_W x DSD_VOLUME_TILE_H window positions of one slice.  Every sum is formed from fixed
 * per-workgroup fp64 partials folded in a fixed order; no floating-point atomics: two calls agree bit for bit.  Scratch is
 * allocated and released by the call: 8 bytes per voxel for l and, with win > 0, 40 bytes per (z, window position in the plane)
 * of the whole volume, since the box is known on the device only.  Rejected before any device work: a null target, pred or out, a dimension below 1,
 * D*H*W > 2^DSD_VOLUME_MAX_LOG2, win even or outside 0, 3..11, elem_is_double not 0 or 1. */
enum { DSD_VOLUME_TILE_W = 32, DSD_VOLUME_TILE_H = 16, DSD_VOLUME_MAX_LOG2 = 27 };
enum {
    DSD_VOLUME_NRMSE = 0, DSD_VOLUME_MAPE, DSD_VOLUME_SMAPE, DSD_VOLUME_LOGAC, DSD_VOLUME_MEDSYMAC, DSD_VOLUME_PSNR, DSD_VOLUME_SSIM3D,
    DSD_VOLUME_STATUS, DSD_VOLUME_N_M,
    DSD_VOLUME_LO_D, DSD_VOLUME_HI_D, DSD_VOLUME_LO_H, DSD_VOLUME_HI_H, DSD_VOLUME_LO_W, DSD_VOLUME_HI_W,   /* hi: the largest index */
    DSD_VOLUME_MEAN_T_M, DSD_VOLUME_STD_T_M, DSD_VOLUME_MEAN_P_M, DSD_VOLUME_STD_P_M,
    DSD_VOLUME_MEAN_T_Z, DSD_VOLUME_STD_T_Z, DSD_VOLUME_MEAN_P_Z, DSD_VOLUME_STD_P_Z,
    DSD_VOLUME_MEAN_T_R, DSD_VOLUME_STD_T_R, DSD_VOLUME_MEAN_P_R, DSD_VOLUME_STD_P_R,
    DSD_VOLUME_NOUT
};
enum { DSD_VOLUME_EMPTY_MASK = 1, DSD_VOLUME_EMPTY_CROP = 2, DSD_VOLUME_ZERO_STD = 4, DSD_VOLUME_ZERO_RANGE = 8, DSD_VOLUME_SMALL_R = 16 };
typedef struct dsd_volume_metrics {
    const void* target;            /* device, [D,H,W] */
    const void* pred;              /* device, [D,H,W] */
    int32_t elem_is_double;        /* 0: float, 1: double */
    const uint8_t* mask;           /* device, [D,H,W], or NULL */
    int32_t D, H, W;
    int32_t win;                   /* 0: no ssim3d; else odd, 3..11 (the reference: 9) */
    double* out;                   /* device, [DSD_VOLUME_NOUT] */
} dsd_volume_metrics;
int dsd_op_volume_metrics(const dsd_volume_metrics* spec, void* stream);
/* out[0] (device) = the k-th smallest, 0-based, of the n doubles x (device; no NaN among them), exactly: most-significant-first
 * radix selection on the order-preserving uint64 image of the bits (sign flipped for non-negative values, complement for negative
 * ones), six histogram passes of 11-bit digits; the result is the element itself.  Rejected: null pointers, n outside 1..2^31,
 * k outside 0..n-1. */
int dsd_op_kth_double(const double* x, int64_t n, int64_t k, double* out, void* stream);
/* ---- PLMS sampler with norm thresholding ---------------------------------------------------
 * Replaces PLMSSampler.sample / plms_sampling / p_sample_plms (ldm/models/diffusion/plms.py:59-245) on a DSD_MODE_B_PLMS
 * schedule.  Iteration k evaluates the network once at t_model[k] (guided: 2B rows, e_t = e_u + s*(e_c - e_u), as in
 * the guided dsd_sample) and combines the noise prediction e_t with the up to three earlier ones (plms.py:228-241, fp32, left to
 * right, true division):
 *   k = 0   x' = upd(e_t); e_next = network(x', t_model[min(1, steps-1)]); e' = (e_t + e_next) / 2     (two evaluations)
 *   k = 1   e' = (3 e_t - o1) / 2          k = 2   e' = (23 e_t - 16 o1 + 5 o2) / 12
 *   k >= 3  e' = (55 e_t - 59 o1 + 37 o2 - 9 o3) / 24
 *   upd(e): pred_x0 = (x - sqrt_1m_at*e) / sqrt(a_t);  dynamic_threshold v > 0: pred_x0 *= v / max(rms(pred_x0), v), the rms over
 *           the Cz*H*W elements of each logical sample (sampling_util.norm_thresholding);  x <- sqrt(a_prev)*pred_x0 +
 *           sqrt(1 - a_prev)*e.  No update noise: sigma is 0, so temperature and noise_dropout act on a zero tensor.
 * The history receives the raw (guided) e_t.  It lives in the handle: first_step = 0 starts it, first_step = k > 0 continues
 * the history the previous call on this handle left for iteration k (same B, state shape and schedule length), and fails
 * otherwise; split runs are bit-identical to the whole run.  The threshold's per-sample sum is formed from fixed per-block
 * partial sums in fp64, combined in a fixed order: two runs are bit-identical.
 * inp is blended with inp->noise / Philox stream (philox_seed, k + 2^32).  dynamic_threshold <= 0: off.
 * Rejected: any other mode, sigma != 0, learned_range, a prediction type other than DSD_PRED_EPS (the reference feeds the
 * network output to the update as a noise prediction whatever the parameterization). */
int dsd_sample_plms(dsd_handle* h, const dsd_schedule* sched, const dsd_guidance* g, const dsd_inpaint* inp,
                    float dynamic_threshold, const float* cond, int Cc, float* x, int Cz, uint64_t philox_seed, int B, int H, int W,
                    int first_step, int n_steps, void* stream);
/* One PLMS update (with its norm pass) on caller buffers.  order: DSD_PLMS_PREDICT / DSD_PLMS_CORRECT are the two halves of
 * iteration 0 around its second network evaluation, DSD_PLMS_AB2..AB4 the multistep updates on 1..3 earlier predictions.
 * out_uncond == NULL: e = out_cond [B,Cz,H,W], x has B rows; else the guided combination and x is the 2B-row state (row b
 * read, rows b and B+b written), rows at x + b*x_row_stride (0: Cz*H*W).  History planes are [B,Cz,H,W]:
 *   PREDICT  h_new <- e_t, x_saved <- x, x <- upd(e_t)
 *   CORRECT  e_t = h_new, e_next = the network output, x <- upd((e_t + e_next)/2) applied to x_saved; h_new stays e_t
 *   AB2..4   h_new <- e_t (AB4: h_new holds o3, read first), o1 / o2 the newest / second-newest earlier predictions (read only)
 * a_t, a_prev, sqrt_1m_at: coefficient slots 4, 5, 7 of the iteration. */
enum { DSD_PLMS_PREDICT = 0, DSD_PLMS_CORRECT = 1, DSD_PLMS_AB2 = 2, DSD_PLMS_AB3 = 3, DSD_PLMS_AB4 = 4 };
int dsd_op_plms_step(int order, float a_t, float a_prev, float sqrt_1m_at, const float* out_uncond, const float* out_cond,
                     float scale, float* h_new, const float* o1, const float* o2, float* x_saved, float* x,
                     int64_t x_row_stride, float dynamic_threshold, int B, int Cz, int H, int W, void* stream);
/* Dynamic thresholding alone: y = clamp(x0,-s,s)/s with s_b = max(quantile_ratio(|x0_b|), max_val); x0,y [B,n], s [B]. */
int dsd_op_dpm_threshold(const float* x0, int B, int n, float ratio, float max_val, float* y, float* s_out, void* stream);

/* ---- single blocks (own parameter namespace, names relative to the block) ----------------- */
enum { DSD_BLOCK_RES = 0, DSD_BLOCK_ATTN = 1, DSD_BLOCK_UPSAMPLE = 2, DSD_BLOCK_DOWNSAMPLE = 3,
       DSD_BLOCK_DISENTANGLE = 4, DSD_BLOCK_SE = 5, DSD_BLOCK_CROSSATTN = 6, DSD_BLOCK_FF_GEGLU = 7,
       DSD_BLOCK_BASIC_TRANSFORMER = 8, DSD_BLOCK_SPATIAL_TRANSFORMER = 9,
       /* latent path (SURVEY f-3): the KL-VAE of ldm/models/autoencoder.py:26-147 — Encoder / Decoder of
        * ldm/modules/diffusionmodules/model.py:452-655 with quant_conv / post_quant_conv; parameter names are the
        * AutoencoderKL state_dict's ("encoder.down.0.block.0.norm1.weight", "quant_conv.weight", ...) */
       DSD_BLOCK_VAE_ENCODER = 10, DSD_BLOCK_VAE_DECODER = 11,
       /* transformer backbone (SURVEY f-4): DiT of UNet_DS_Diff/DiT_models.py:145-262 (adaLN-Zero blocks, timm-style
        * PatchEmbed / Attention / Mlp); parameter names are the DiT state_dict's */
       DSD_BLOCK_DIT = 12,
       /* the plain single-stream UNetModel of ldm/modules/diffusionmodules/openaimodel.py:571-958: the
        * denoiser that consumes the VAE latents in the latent path; optionally with a SpatialTransformer on `context` in
        * every attention slot (use_spatial_transformer=True, :761-765,818-822,872-876) and with label_emb on y (:696-712) */
       DSD_BLOCK_UNET = 13,
       /* the KL-VAE's AttnBlock alone (ldm/modules/diffusionmodules/model.py:185-209): one head over all channels; parameter
        * names norm / q / k / v / proj_out.  Takes dsd_set_vae_fused_attention like the encoder and the decoder. */
       DSD_BLOCK_VAE_ATTN = 14 };
/* iargs by kind:
 *   RES: cin, cout, emb_ch, use_scale_shift_norm, up, down      ATTN: ch, heads, new_order
 *   UPSAMPLE/DOWNSAMPLE: ch     DISENTANGLE: ch, half_ch       SE: ch, reduction
 *   CROSSATTN: query_dim, context_dim, heads, dim_head          FF_GEGLU: dim, mult
 *   BASIC_TRANSFORMER: dim, heads, dim_head, context_dim
 *   SPATIAL_TRANSFORMER: in_ch, heads, dim_head, depth, context_dim, use_linear
 *   VAE_ENCODER / VAE_DECODER: ch, out_ch, in_channels, resolution, z_channels, double_z, embed_dim, num_res_blocks,
 *        with_quant (1: AutoencoderKL.encode / decode incl. quant_conv / post_quant_conv, 0: bare Encoder / Decoder),
 *        len(ch_mult), ch_mult..., len(attn_resolutions), attn_resolutions...    (configs/autoencoder_kl_64x64x3.yaml:14-24)
 *        encoder: x [B,in_channels,H,W] -> moments [B,2*embed_dim,H/f,W/f];  decoder: z [B,embed_dim,h,w] -> [B,out_ch,h*f,w*f]
 *   VAE_ATTN: in_channels
 *   DIT: input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_hidden, num_classes, learn_sigma,
 *        use_cfg_embedding.  x [B,in_channels,S,S] (x and cond already concatenated), aux = timesteps [B] fp32 (aux_len 1),
 *        aux2 = class labels [B] int64 or NULL (aux_len2 1 / 0); out [B, out_channels, S, S].  dsd_set_timestep_freqs
 *        (128 entries) installs the caller's frequency table as for the U-Net.
 *   UNET: in_channels, model_channels, out_channels, num_heads, num_head_channels, num_heads_upsample, use_scale_shift_norm,
 *        resblock_updown, use_new_attention_order, legacy, len(channel_mult), channel_mult..., num_res_blocks per level...,
 *        len(attention_resolutions), attention_resolutions...  (the ctor kwargs of openaimodel.py:601-633), optionally followed by
 *        use_spatial_transformer, transformer_depth (1), context_dim, use_linear_in_transformer, and behind those by the
 *        label_emb kind (0 none, 1 int num_classes, 2 "continuous", 3 "sequential") and its width (num_classes /
 *        adm_in_channels; openaimodel.py:696-712).  Parameters: label_emb.weight (kind 1, [num_classes, 4*model_channels]),
 *        label_emb.weight / .bias (kind 2), label_emb.0.0.* and label_emb.0.2.* (kind 3).
 *        x [B,in_channels,H,W], aux = timesteps [B] fp32 (aux_len 1), aux2 = context [B,tokens,context_dim] with
 *        aux_len2 = tokens (spatial-transformer variant only, else NULL / 0); y of a label_emb handle comes through
 *        dsd_set_conditioning; out [B,out_channels,H,W]. */
int dsd_block_create(int kind, const int32_t* iargs, int n_iargs, int device, dsd_handle** out);
/* x: NCHW [B,C,H,W] (token blocks: [B,N,C] passed as H=N, W=1 "NHWC"), aux: emb [B,emb_ch] for RES,
 * context [B,Nc,Cc] for cross-attention kinds (aux2/aux_len2 = second context for depth-2 spatial
 * transformer), else NULL.  out sized as the block's output. */
int dsd_block_forward(dsd_handle* h, const float* x, int B, int C, int H, int W, const float* aux, int aux_len,
                      const float* aux2, int aux_len2, float* out, void* stream);

/* ---- kernel-level ops (NHWC activations; used by tests and micro-benchmarks) -------------- */
/* y[N,OH,OW,Cout] = conv(x[N,H,W,Cin], w OIHW ks x ks, pad ks/2, stride) + bias (+ emb[N,Cout]) (+ res) ;
 * upsample=1 folds a nearest x2 in front of the conv (Upsample, openaimodel.py:111-121). */
int dsd_op_conv2d(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                  int ks, int stride, int upsample, const float* emb, const float* res, float* y, void* stream);
/* Same with an explicit arithmetic mode: 0 = fp32 MFMA, 1 = bf16x3, 2 = bf16x6 (fp32 operands split into bf16 pieces,
 * fp32 accumulation; conv_split.hip).  Shapes the split kernel cannot take fall back to fp32.  OR-ing 16 / 32 / 64
 * into `precision` forces the A-direct / fully staged / 256-row A-direct kernel structure (tests); otherwise the library
 * chooses; OR-ing 128 (with precision 2) runs the F(2,3) kernel of dsd_set_winograd and fails if the shape cannot take it. */
int dsd_op_conv2d_prec(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                       int ks, int stride, int upsample, const float* emb, const float* res, int precision, float* y,
                       void* stream);
/* The launch arguments the networks set and dsd_op_conv2d_prec cannot express (ConvArgs, csrc/kernels.h); everything else as
 * in dsd_op_conv2d_prec, including the precision | structure bits, the F(2,3) / sub-pixel weight preparation and the f16x3
 * overflow flag.  Inputs:
 *   x_batch_stride  elements between the samples of x: -1 = H*W*Cin, 0 = ONE plane shared by the batch, else >= H*W*Cin
 *   pad_lo, pad_total  zero rows / columns before the first one and in total per axis (-1, -1 = ks/2 on every side;
 *                   0, 1 = the VAE's Downsample)
 *   y_ld            row stride of y in elements (0 = Cout): y is a channel slice of a wider NHWC tensor; y itself points
 *                   at the slice's first channel (16-byte aligned; y_ld % 4 == 0 unless y_ld == Cout)
 *   out_nchw        y is [N,Cout,OH,OW] (needs y_ld == Cout)
 *   emb_stride      row stride of emb in elements (0 = Cout): emb[n*emb_stride + co], emb pointing at the layer's first column
 *   no_scratch      launch without split-K workspace (what a caller outside the planned graph does)
 * Outputs: kernel = the name of the kernel that was launched (conv2d_route_name), ksplit = the split-K factor that ran (1
 * without scratch).  y is caller-allocated; arguments are validated before anything is launched. */
typedef struct dsd_conv_ex {
    int64_t x_batch_stride;
    int32_t pad_lo, pad_total;
    int32_t y_ld;
    int32_t out_nchw;
    int32_t emb_stride;
    int32_t no_scratch;
    int32_t ksplit;
    int32_t reserved;
    char kernel[64];
} dsd_conv_ex;
int dsd_op_conv2d_ex(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                     int ks, int stride, int upsample, const float* emb, const float* res, int precision, dsd_conv_ex* ex,
                     float* y, void* stream);
/* dsd_op_conv2d_ex with the remaining ConvArgs fields: GroupNorm + SiLU of the INPUT applied inside the kernel, and the GroupNorm
 * statistics of the OUTPUT from the epilogue.  Inputs:
 *   gn_scale, gn_shift  [N][Cin] per-(sample, channel) coefficients (dsd_op_gn_finalize's), both or neither; x is then the tensor
 *                   BEFORE the normalisation and the layer computes conv(silu(x * scale + shift)) with zero padding of the
 *                   activated tensor.  Refused unless the launch runs the tap-reuse kernel (kernel name ".../tr+gn")
 *   stats           optional output, [N][stats_chunks][Cout][2] doubles: (sum, sum of squares) of every output column over a
 *                   chunk = a run of OH*OW / stats_chunks consecutive output pixels of one sample (sub-pixel form: chunk =
 *                   (2 py + px) * (H*W / 256) + run of 256 low-resolution pixels whose phase-(py, px) outputs it covers)
 *   stats_doubles   doubles the stats buffer holds (checked against N * stats_chunks * Cout * 2)
 *   query           1: fill ex->kernel, ex->ksplit and stats_chunks, launch nothing (y is not written)
 * Output: stats_chunks = chunks per sample the kernel of exactly these arguments (no_scratch included) emits; 0 = it cannot,
 * and a call with stats is then refused.  Every refusal comes before the first launch. */
typedef struct dsd_conv_gn {
    const float* gn_scale;
    const float* gn_shift;
    double* stats;
    int64_t stats_doubles;
    int32_t stats_chunks;
    int32_t query;
} dsd_conv_gn;
int dsd_op_conv2d_gn(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                     int ks, int stride, int upsample, const float* emb, const float* res, int precision, dsd_conv_ex* ex,
                     dsd_conv_gn* gn, float* y, void* stream);
/* gn_finalize on caller-supplied statistics: source 0 covers channels [0, c0) with chunks0 chunks per sample
 * (p0[N][chunks0][c0][2] doubles), the optional source 1 (p1 != NULL) channels [c0, c0 + c1); c0 (+ c1) must equal C.  film
 * (optional): [N][film_stride] rows holding the FiLM scale in columns [0, C) and the shift in [C, 2C).  scale / shift: [N][C],
 * GroupNorm32(x) (* (1 + film scale) + film shift) = x * scale + shift. */
int dsd_op_gn_finalize(const double* p0, int chunks0, int c0, const double* p1, int chunks1, int c1, int N, int HW, int C,
                       const float* gamma, const float* beta, float eps, const float* film, int film_stride, float* scale,
                       float* shift, void* stream);
/* dst[n, p, coff:coff+C] = act((a [+ b] [+ c] [+ d]) / div) on [N][HW][C] sources (bit k of bmask: source k is ONE sample
 * [HW][C] broadcast over the batch), dst rows of dstC floats, and the per-column statistics of what was written:
 * partial[N][*nchunk][C][2] doubles (the chunking of the standalone statistics pass; *nchunk is an output, partial_doubles the
 * room the caller gave).  act: 0 none, 1 SiLU. */
int dsd_op_avg_into_stats(const float* a, const float* b, const float* c, const float* d, float div, int N, int HW, int C,
                          float* dst, int dstC, int coff, int act, int bmask, double* partial, int64_t partial_doubles,
                          int* nchunk, void* stream);
/* The bottleneck head of UNet_disc_Model without a network (Disc_diff/guided_diffusion/unet.py:1015-1033).  com[4] / dist[4]:
 * the PRE-activation outputs of conv_common / conv_distinct on the four streams, NHWC [B][HW][half] each; w1[5] / w2[5]: the
 * bias-free SE linears [Cr][half] / [half][Cr] of SE_Attention_com and SE_Attention_dist_1..4, in that order (all device
 * pointers, the pointer arrays themselves on the host).  cat [B][HW][5*half] receives
 * [SE_com(mean_i SiLU(com_i)), SE_dist_1(SiLU(dist_1)), ..., SE_dist_4(SiLU(dist_4))]; feats: NULL, or 8 device pointers to
 * NHWC [B][HW][half] buffers for SiLU(com_1..4) and the four scaled dist_i.  half % 4 == 0 and 16-byte aligned pointers, else
 * the call fails.  unfused: 0 the three launches of csrc/disc.hip (fp64 pooling partials added in index order, no atomics: two
 * runs are bit-identical), 1 the composition of older ops, -1 as the environment variable DSD_DISC_UNFUSED says. */
int dsd_op_disc_bottleneck(const float* const* com, const float* const* dist, const float* const* w1, const float* const* w2,
                           int B, int HW, int half, int Cr, float* cat, float* const* feats, int unfused, void* stream);
/* The one-launch GroupNorm32 (+ FiLM, + activation) of small maps, called directly (the DSD_GN_SMALL switch of the networks is
 * not consulted): x, y [N][HW][C], C % 32 == 0, HW * C / 32 <= 32768; film as in dsd_op_gn_finalize; act: 0 none, 1 SiLU. */
int dsd_op_gn_small(const float* x, int N, int HW, int C, const float* gamma, const float* beta, float eps, const float* film,
                    int film_stride, int act, float* y, void* stream);
/* Micro-benchmark of the convolution kernel on random data (library-owned buffers): average ms per launch over
 * `iters` back-to-back launches (hipEvents) and the algorithmic FLOPs of one launch.  variant: -1/0 default fp32
 * kernel, 1 flat-load fp32 kernel, 10 bf16x3, 11 bf16x6, 12 f16x3 (library's choice of structure), 20/21 both operands staged
 * through LDS, 30/31 activations read straight into registers (128-row tile), 40/41/42 the same on the 256-row tile,
 * 50 bf16x6 as F(2,3) along the width (FLOPs reported are those of the direct form: "fp32-equivalent"). */
int dsd_bench_conv2d(int N, int H, int W, int Cin, int Cout, int ks, int stride, int variant, int iters, float* avg_ms,
                     double* flops);
/* Diagnostic build of the dominant kernel (bf16x6, 256-row tile, Cout = 320 -> 160-column tiles): `warm` untimed launches
 * of the product kernel, then ONE launch of an instantiation that stamps (s_memtime, s_memrealtime) at entry, in front of
 * the k-loop, behind it and after the epilogue.  out: 8 int64 per workgroup (host memory, room for max_wgs workgroups);
 * *n_wgs = workgroups launched.  tools/conv_stamps.py turns this into prologue / loop / epilogue / gap times and the
 * in-kernel clock.  whatif != 0 runs an instantiation with one cost of the k-loop removed (output garbage; timing only):
 * 2 no activation loads, 4 no weight loads / LDS writes, 8 no barrier, 16 no weight fragment reads, 31 all of them and no
 * activation split (the bare MFMA stream of this kernel), 32 loads issued in bursts of eight (the schedule before round 2;
 * results stay correct), 256 activations read as pre-split bf16 planes (12 piece loads per tile, no split VALU), 512 the tap-reuse
 * instantiation the library uses for these layers by default (0 stamps the plain A-direct kernel).  Other values fail (conv_split.hip lists what else was measured). */
int dsd_bench_conv2d_stamps(int N, int H, int W, int Cin, int Cout, int warm, int whatif, long long* out, int max_wgs,
                            int* n_wgs);
/* What the bf16 matrix pipes of this device sustain: a bare v_mfma_f32_32x32x16_bf16 loop on the dominant convolution's
 * accumulator tile (one wave per SIMD, 160 accumulators, six products per group), `workgroups_per_cu` x 256 workgroups
 * (<= 0: 8), about `ms_target` milliseconds per launch, average of `iters` launches (hipEvents).  variant 0: operands in
 * registers (nothing but MFMAs: the upper bound at the clock the chip holds); 1: weight fragments re-read from LDS as the
 * convolution does; 2 / 3: the same two on all-zero operands; 4 .. 7: the same four with the work issued as
 * v_mfma_f32_16x16x32_bf16 (the same output tile per wave, the same matrix-pipe cycles: the two shapes can hold different
 * clocks under load).  *tflops = issued bf16 MFMA TFLOP/s.  (peak.hip) */
int dsd_bench_mfma_peak(int variant, int workgroups_per_cu, float ms_target, int iters, float* avg_ms, double* tflops);
/* How the library would run a convolution (host-side query, no GPU work): kernel structure (0 both operands staged
 * through LDS, 1 / 2 activations read straight into registers with a 128 / 256-row tile; -1 for the fp32 kernel), N-tile
 * width in 32-column units, split-K factor and the scratch bytes the split needs.  precision as in dsd_op_conv2d_prec;
 * + 256: planned as inside a stream-lane region (dsd_set_stream_lanes), i.e. for a quarter of the chip. */
/* Process-wide switch (experiment): the dominant convolution kernel (256 x 160 tile, bf16x6, tap reuse,
 * optional fused GroupNorm) with its matrix work issued as v_mfma_f32_16x16x32_bf16 (conv_tr16.hip) instead of
 * v_mfma_f32_32x32x16_bf16.  Same results up to fp32 summation order.  Default: the environment variable
 * DSD_CONV_MFMA16 (0).  Returns the previous setting. */
int dsd_set_conv_mfma16(int on);
/* Phase weights of the sub-pixel form of conv3x3(nearest_x2(x)) (host-side, no GPU work): w_oihw [Cout][Cin][3][3] ->
 * out [4 phases (py, px)][Cout][2][2][Cin], each phase tap the fp64 sum of the original taps it covers.  Output pixel
 * (2i + py, 2j + px) is then sum over (a, b) of x[i + py - 1 + a][j + px - 1 + b] . out[py, px][:, a, b, :] (zero outside).
 * The library's bf16x6 mode runs upsample layers this way where the tap-reuse kernel takes the low-resolution map. */
int dsd_subpixel_weights_host(const float* w_oihw, int Cout, int Cin, double* out);
int dsd_conv_plan(int N, int H, int W, int Cin, int Cout, int ks, int stride, int precision, int* structure, int* nt,
                  int* ksplit, uint64_t* scratch_bytes);
/* GroupNorm(32, C, eps) [+ SiLU] on x[N,HW,C]. */
int dsd_op_group_norm(const float* x, int N, int HW, int C, const float* gamma, const float* beta, float eps,
                      int silu, float* y, void* stream);
/* The model's last layer as one pass: y[N,H,W] = Conv3x3(SiLU(GroupNorm32(x))) with ONE output channel, x NHWC [N,H,W,C],
 * C a multiple of 64 up to 320, w_oihw [1,C,3,3] (UNet_DS_Diff/model.py:511-515 `self.out`, applied at :751). */
int dsd_op_gn_silu_conv_out1(const float* x, int N, int H, int W, int C, const float* gamma, const float* beta, float eps,
                             const float* w_oihw, const float* bias, float* y, void* stream);
/* QKVAttention / QKVAttentionLegacy (openaimodel.py:496-555) on qkv[N,T,3C] -> a[N,T,C].  split = 0: both products on
 * the fp32 matrix cores (what DSD_PREC_F32 runs); 1: operands split exactly into three bf16 pieces, six bf16 MFMA products
 * each (what every other mode runs); the softmax is fp32 either way. */
int dsd_op_qkv_attention(const float* qkv, int N, int T, int C, int heads, int new_order, int split, float* a, void* stream);
/* The fp32-grade attention kernels with every launch argument of AttnArgs (csrc/kernels.h): out[n,t,h*d + :] =
 * softmax((q scale_q)(k scale_k)^T scale_s) v per head.  q rows [N*Tq] of ldq floats with head h at +h*q_hs (k, v alike over
 * N*Tk rows), out rows of ldo floats with head h at +h*d.  Strides and pointers must keep rows 16-byte aligned.  split as in
 * dsd_op_qkv_attention.  d % 4 == 0 and d <= 512: up to 128 one wave owns a query's whole head (csrc/attention.hip, the kernels
 * every network uses), above it the head dim is sliced across the four waves of a workgroup (csrc/attention_wide.hip: this entry
 * and the KL-VAE's fused AttnBlock, dsd_set_vae_fused_attention); anything else is an error.  The networks' own attention slots
 * (U-Net, SpatialTransformer, DiT) still stop at d = 128. */
int dsd_op_attention(const float* q, const float* k, const float* v, int N, int Tq, int Tk, int heads, int d, int ldq, int ldk,
                     int ldv, int ldo, int q_hs, int k_hs, int v_hs, float scale_q, float scale_k, float scale_s, int split,
                     float* out, void* stream);
/* The half-precision kernels of DSD_PREC_F16 / DSD_PREC_BF16 on fp32 device buffers (the entry rounds the inputs to 16 bits
 * once, runs the kernel, and widens the 16-bit result): y[M,N] = x[M,K] w[N,K]^T + bias (nn.Linear; timm Mlp / Attention
 * projections, DiT_models.py:101-122).  epi 0: y = round16(acc + bias); 1: y = round16(gelu_tanh(round16(acc + bias)));
 * 2: y (fp32, in/out) += gate[(m / T), :] * round16(acc + bias) — the adaLN-Zero gated residual (:120-121). */
int dsd_op_gemm_half(const float* x, const float* w, const float* bias, int M, int N, int K, int bf16, int epi,
                     const float* gate, int T, float* y, void* stream);
/* Timing of the half-precision GEMM kernel on random operands (hipEvents, average of `iters` launches after one warm-up).
 * whatif < 0: the product kernel with epilogue `epi`; whatif >= 0: a diagnostic instantiation with costs removed (bits: 1 no
 * LDS-DMA staging in the loop, 2 fragments read from LDS only once, 4 no epilogue, 8 no barrier; instantiated: 0, 1, 2, 3, 4,
 * 7, 15) whose results are garbage — tools/gemm_whatif.py. */
int dsd_bench_gemm_half(int M, int N, int K, int bf16, int epi, int whatif, int iters, float* avg_ms);
/* The same for the half-precision attention kernel on a random qkv[N,T,3C].  whatif bits: 1 no softmax arithmetic, 2 no K / V
 * staging after the first tile, 4 no second product, 8 no first product (instantiated for fp16, head dim 64: 0, 1, 2, 3, 4, 8,
 * 13) — tools/attn_whatif.py. */
int dsd_bench_attention_half(int N, int T, int C, int heads, int bf16, int whatif, int iters, float* avg_ms);
/* softmax(q k^T * d^-1/2) v of timm Attention on qkv[N,T,3C] (q | k | v, heads inside each) -> a[N,T,C], 16-bit operands,
 * fp32 softmax statistics; thr: running-maximum threshold in log2 units (< 0: the library's default). */
int dsd_op_attention_half(const float* qkv, int N, int T, int C, int heads, int bf16, float thr, float* a, void* stream);
/* timestep_embedding (util.py:161-181): t[N] (int64 or fp32) -> [N,dim].  freqs (device, [dim/2], may be NULL): the
 * frequency table as the caller's own fp32 exp evaluates it (what dsd_set_timestep_freqs installs in a model handle);
 * with it the sin/cos arguments are bit-identical to the reference's. */
int dsd_op_timestep_embedding(const void* t, int t_is_float, int N, int dim, const float* freqs, float* y, void* stream);
/* y[N,O] = act_in(x[N,K]) @ w[O,K]^T + bias ; act_in: 0 none, 1 SiLU. */
int dsd_op_linear(const float* x, int N, int K, const float* w, const float* bias, int O, int act_in, float* y,
                  void* stream);
/* DiagonalGaussianDistribution(moments).sample() (ldm/modules/distributions/distributions.py:24-37): moments [B,2E,H,W]
 * -> z [B,E,H,W] = mean + exp(0.5*clamp(logvar,-30,20)) * eps; eps = noise [B,E,H,W] or on-device Philox normals. */
int dsd_op_gaussian_sample(const float* moments, const float* noise_or_null, uint64_t philox_seed, int B, int E, int H, int W,
                           float* z, void* stream);
/* scale * DiagonalGaussianDistribution(moments).sample(): LatentDiffusion.get_first_stage_encoding (ddpm.py:660-667), the sample
 * formed first, then scaled.  moments [B,2E,H,W] -> z [B,E,H,W].  With the B rows ordered (sample, key) — K condition images
 * per sample encoded in ONE pass of B = batch*K one-channel images (trainers/trainer_latent_diffusion.py:177-189) — z is the
 * [batch,K*E,H,W] 'concat' conditioning, key k in channels [k*E,(k+1)*E). */
int dsd_op_posterior_sample_scaled(const float* moments, const float* noise_or_null, uint64_t philox_seed, int B, int E, int H,
                                   int W, float scale, float* z, void* stream);
/* Philox4x32-10 + Box-Muller stream used by dsd_sample when noise == NULL: fills n normals. */
int dsd_op_philox_normal(float* y, int64_t n, uint64_t seed, uint64_t step, void* stream);
/* The small kernels around the convolutions and the transformer blocks (csrc/misc.hip, layer_norm of csrc/norm.hip, the casts and
 * ln_modulate16 of csrc/gemm16.hip), each launched alone exactly as the networks launch it (test plumbing: no arithmetic
 * here).  All buffers are device pointers; a kind reads its arguments in the order of its launcher in csrc/kernels.h:
 *   kind                 ptrs                  ints                                                         floats
 *   SE_SCALE             x, w1, w2, y          N, HW, C, Cr
 *   AVG_INTO             a, b, c, d, dst       pixels, C, dstC, coff, act, per_sample_pixels, bmask         div
 *   NCHW_TO_NHWC         x, y                  N, C, HW             (NHWC_TO_NCHW alike)
 *   AVGPOOL2             x, y                  N, H, W, C           (UPSAMPLE2 alike; x NHWC)
 *   GEGLU                x, y                  rows, inner
 *   SOFTMAX_ROWS         s (in place)          rows, cols                                                   scale
 *   LN_MODULATE          x, mod, y             N, T, C, mod_stride, shift_off, scale_off                    eps
 *   LN_MODULATE16        x, mod, y (16-bit)    N, T, C, mod_stride, shift_off, scale_off, bf16              eps
 *   LAYER_NORM           x, gamma, beta, y     rows, C                                                      eps
 *   GATED_RESIDUAL       x (in place), y, mod  N, T, C, mod_stride, gate_off
 *   GELU_TANH            x (in place)          n
 *   PATCHIFY             x, y                  N, C, H, W, p        (token channels in the order c, ph, pw)
 *   UNPATCHIFY           x, y                  N, c, h, w, p        (token channels in the order ph, pw, c)
 *   ADD_ROWS_BROADCAST   x (in place), pos     N, TC
 *   EMBED_ADD            a (or NULL), table, idx (int64), y         N, C
 *   ADD2                 a, b, y               n
 *   CAST16               x, y (16-bit)         n, bf16              (UNCAST16: x 16-bit, y fp32)
 * Unused trailing arrays may be NULL. */
enum { DSD_TAIL_SE_SCALE = 0, DSD_TAIL_AVG_INTO, DSD_TAIL_NCHW_TO_NHWC, DSD_TAIL_NHWC_TO_NCHW, DSD_TAIL_AVGPOOL2, DSD_TAIL_UPSAMPLE2,
       DSD_TAIL_GEGLU, DSD_TAIL_SOFTMAX_ROWS, DSD_TAIL_LN_MODULATE, DSD_TAIL_LN_MODULATE16, DSD_TAIL_LAYER_NORM,
       DSD_TAIL_GATED_RESIDUAL, DSD_TAIL_GELU_TANH, DSD_TAIL_PATCHIFY, DSD_TAIL_UNPATCHIFY, DSD_TAIL_ADD_ROWS_BROADCAST,
       DSD_TAIL_EMBED_ADD, DSD_TAIL_ADD2, DSD_TAIL_CAST16, DSD_TAIL_UNCAST16, DSD_TAIL_NKINDS };
int dsd_op_tail(int kind, void* const* ptrs, const int64_t* ints, const float* floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSDIFF_H */
