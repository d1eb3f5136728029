// Launcher declarations for the hand-written gfx950 kernels of libdsdiff.
#pragma once
#include "common.h"

namespace dsd {

// ---------------------------------------------------------------- conv.hip
// Implicit-GEMM convolution on NHWC fp32, f32 MFMA (v_mfma_f32_32x32x2_f32), M = N*OH*OW, N = Cout, K = ks*ks*Cin.
struct ConvArgs {
    const float* x = nullptr;   // input, NHWC within a sample
    int N = 0, H = 0, W = 0, Cin = 0;
    int64_t x_bs = -1;          // batch stride of x in elements (<0 -> H*W*Cin; 0 = one plane shared by all samples)
    const float* w = nullptr;   // packed OHWI: [Cout][ks*ks*Cin]
    const float* bias = nullptr;
    int Cout = 0, ks = 3, stride = 1;
    int pad_lo = -1, pad_total = -1;   // padding before the first row/column and in total per axis (-1: ks/2 and 2*(ks/2))
    int ups = 0;                // nearest x2 folded into the gather (Upsample, openaimodel.py:111-121)
    const float* emb = nullptr; // per-(n,co) add: emb[n*emb_stride + co]   (ResBlock h + emb_out, openaimodel.py:282)
    int emb_stride = 0;
    const float* res = nullptr; // residual NHWC [N,OH,OW,Cout] added in the epilogue (skip_connection(x) + h)
    float* y = nullptr;
    int y_ld = 0;               // row stride of y in elements (0 -> Cout): lets a conv write a channel slice of a wider
                                // NHWC tensor, e.g. the decoder's concat buffer (torch.cat([h, skip]) never copied)
    int out_nchw = 0;           // store as [N,Cout,OH,OW] (final layer with out_channels > 1)
    int variant = -1;           // kernel variant override (-1 = default / env DSD_CONV_VARIANT)
    int precision = 0;          // PREC_F32 | PREC_BF16X3 | PREC_BF16X6 (conv_split.hip)
    const void* w_split = nullptr;  // [3][Cout][ks*ks*Cin] bf16 pieces of w (needed for the split precisions)
    const void* w_wino = nullptr;   // transformed + split + packed weights of the F(2,3) kernel (conv_wino.hip), optional
    // sub-pixel form of an upsample layer (conv2d_subpixel_ok): [3][4 phases][Cout][2][2][Cin] bf16 pieces of the phase weights
    // (subpixel_weights); when present, conv2d() runs the layer as four 2x2 convolutions on the low-resolution map
    const void* w_subpixel = nullptr;
    int* ovf = nullptr;             // device flag set by the f16x3 kernels when an operand exceeds the fp16 range
    float* scratch = nullptr;       // split-K partial sums (ConvRoute::scratch_bytes); without it small grids run unsplit
    size_t scratch_bytes = 0;
    // GroupNorm statistics of the OUTPUT, accumulated in the epilogue: stats[n][chunk][co][2] doubles (GnSrc layout),
    // stats_chunks = ConvRoute::stats_chunks chunks per sample; nullptr = not wanted
    double* stats = nullptr;
    int stats_chunks = 0;
    // diagnostic build of the dominant kernel only (tools/conv_stamps.py): 8 int64 per workgroup — (s_memtime,
    // s_memrealtime) at entry, in front of the k-loop, behind it, and after the epilogue
    long long* stamps = nullptr;
    int diag = 0;   // what-if bits (conv_split.hip, DIAG)
    // GroupNorm + SiLU of the INPUT applied while the filter rows are staged (tap-reuse kernel only: ConvRoute::fuses_gn):
    // x is then the tensor BEFORE the normalisation and gn_scale / gn_shift are gn_finalize's per-(sample, channel)
    // coefficients [N][Cin]; the separate apply pass over HBM disappears
    const float* gn_scale = nullptr;
    const float* gn_shift = nullptr;
    // launches of this shape that run side by side on other HIP streams (the four encoder streams' lanes, net.cpp): the planner
    // sizes tile width / split-K for 1/lanes of the chip — a grid that would leave three quarters of the CUs idle alone fills them
    // together, so the wide tap-reuse kernel (with the fused GroupNorm) is the right choice where a lone launch takes narrow tiles
    int lanes = 1;
};
// Output size.  Default padding is ks/2 on every side (the U-Net's convolutions); pad_lo / pad_total describe the VAE's
// Downsample (ldm/modules/diffusionmodules/model.py:78-83: F.pad (0,1,0,1) then a stride-2 conv with padding 0), i.e. no
// padding before the first row / column and one zero row / column after the last.
inline void conv_out_hw(const ConvArgs& a, int* OH, int* OW) {
    const int IHg = a.ups ? a.H * 2 : a.H, IWg = a.ups ? a.W * 2 : a.W;
    const int pt = a.pad_total >= 0 ? a.pad_total : 2 * (a.ks / 2);
    *OH = (IHg + pt - a.ks) / a.stride + 1;
    *OW = (IWg + pt - a.ks) / a.stride + 1;
}
// What conv2d() launches for a set of arguments and what that launch offers its caller (the fields: conv.hip, conv2d_route)
enum ConvFamily { CONV_DIRECT_COLS, CONV_DIRECT_LDS, CONV_SCALAR, CONV_SUBPIXEL, CONV_WINO, CONV_MFMA_BUF, CONV_MFMA, CONV_SPLIT };
struct ConvRoute { ConvFamily family = CONV_MFMA; int precision = 0, nt = 1, ksplit = 1, structure = -1; bool tap_reuse = false, fuses_gn = false;
                   int stats_chunks = 0, launches = 1; size_t scratch_bytes = 0; int OH = 0, OW = 0; int64_t M = 0; };
ConvRoute conv2d_route(const ConvArgs& a, bool replan);   // replan: split-K scratch will be passed; conv2d(a) launches conv2d_route(a, a.scratch != nullptr)
const char* conv2d_route_name(const ConvRoute& r, bool gn_applied);
// out = Conv3x3(SiLU(x * scale + shift)) with ONE output channel (conv_out1.hip): x NHWC [N,H,W,C] BEFORE the normalisation,
// scale / shift = gn_finalize's coefficients [N][C], w = [3][3][C] (the packed OHWI weight of a 1-channel conv), y = [N,H,W]
struct ConvOut1Args {
    const float* x = nullptr;
    int N = 0, H = 0, W = 0, C = 0;
    const float* scale = nullptr;
    const float* shift = nullptr;
    const float* w = nullptr;
    const float* bias = nullptr;
    float* y = nullptr;
};
bool conv_out1_ok(int C, int cout, int ks, int stride);
void conv_out1(const ConvOut1Args& a, hipStream_t s);
enum { PREC_F32 = 0, PREC_BF16X3 = 1, PREC_BF16X6 = 2, PREC_F16X3 = 3, PREC_F16 = 4, PREC_BF16 = 5 };
void conv2d(ConvArgs a, hipStream_t s);
// conv_split.hip: fp32 operands as sums of bf16 pieces on the bf16 matrix cores
void split_weights(const float* w, int64_t n, int np, void* planes, hipStream_t s, bool f16 = false, int* ovf = nullptr);
bool conv2d_split_eligible(const ConvArgs& a);
bool conv2d_split_tr(const ConvArgs& a, int nt, int ksplit, int ad);   // the tap-reuse instantiation would take it
// Sub-pixel upsample convolution (conv_split.hip): output pixel (2i + py, 2j + px) of conv3x3(nearest_x2(x)) reads input rows
// i + py - 1 + {0, 1} and columns j + px - 1 + {0, 1}; original filter row (column) k of phase p lands on phase tap
// subpixel_tap(p, k) (p = 0: k = 0 -> 0, k = 1, 2 -> 1;  p = 1: k = 0, 1 -> 0, k = 2 -> 1).  The zero padding maps exactly.
__host__ __device__ inline int subpixel_tap(int p, int k) { return (p + k + 1) / 2 - p; }
bool conv2d_subpixel_shape_ok(const ConvArgs& a);   // the sub-pixel kernel can take this problem
bool conv2d_subpixel_ok(const ConvArgs& a);         // the planner runs it that way (bf16x6, no structure forced): build w_subpixel
size_t subpixel_weight_bytes(int Cout, int Cin);
void subpixel_weights(const float* w_ohwi, int Cout, int Cin, void* planes, hipStream_t s);
void conv2d_subpixel(const ConvArgs& a, hipStream_t s);
// process-wide switch of the tap-reuse kernel's MFMA shape (0: 32x32x16, 1: 16x16x32 — conv_tr16.hip); A/B runs in one process
void conv2d_set_mfma16(int on);
int conv2d_get_mfma16();
void conv2d_split(const ConvArgs& a, int nt, int ksplit, int structure, hipStream_t s);
double conv2d_flops(const ConvArgs& a);        // the layer's algorithmic count (3x3 over the upsampled map for an upsample layer)
double conv2d_exec_flops(const ConvArgs& a);   // what the launched kernel multiplies (4/9 of that in the sub-pixel form)
// N-tile width (in 32-column units) and split-K factor the split-precision path runs this problem with; nt_default is the
// width the generic cost model (conv.hip pick_nt) would take
void conv2d_split_plan(const ConvArgs& a, int nt_default, int* nt, int* ksplit, int* structure = nullptr, bool allow_split = true);
void pack_ohwi(const float* w_oihw, float* w_ohwi, int Cout, int Cin, int ks, hipStream_t s);
// conv_wino.hip: 3x3 stride-1 convolution as F(2,3) along the width (1.5x fewer MFMAs), bf16x6 arithmetic
bool conv2d_wino_shape_ok(const ConvArgs& a);      // could run there if it had packed weights
bool conv2d_wino_eligible(const ConvArgs& a);      // shape_ok and a.w_wino present
bool conv2d_wino_worthwhile(const ConvArgs& a);    // shape_ok and a grid big enough to beat the direct kernel (the planner's rule)
size_t wino_packed_bytes(int Cout, int Cin);
// peak.hip: bare MFMA loops (diagnostic)
int64_t mfma_peak_src_bytes();
void mfma_peak_fill(void* src, bool zero, hipStream_t s);
double mfma_peak_launch(int variant, const void* src, float* sink, int workgroups, int loops, hipStream_t s);
void wino_pack_weights(const float* w_ohwi, int Cout, int Cin, void* packed, hipStream_t s);
void conv2d_wino(const ConvArgs& a, hipStream_t s);
int conv2d_wino_stats_chunks(const ConvArgs& a);

// ---------------------------------------------------------------- norm.hip
int gn_nchunks(int HW, int C);
// Per-column statistics of the channels [c0, c0+c) of a tensor: p[n][chunk][col][2] doubles (sum, sumsq over the chunk's
// pixels), `chunks` chunks per sample.  Written by gn_stats, by avg_into_stats and by the convolution epilogues.
struct GnSrc {
    const double* p = nullptr;
    int chunks = 0, c0 = 0, c = 0;
};
// partial: [N][nchunk][C][2] doubles
void gn_stats(const float* x, int N, int HW, int C, double* partial, int nchunk, hipStream_t s);
// scale/shift: [N][C] so that GN(x) = x*scale + shift; film (optional, [N][film_stride] = scale|shift halves):
// (GN(x))*(1+fs)+fsh folded in (ResBlock use_scale_shift_norm, openaimodel.py:276-280).  s0 covers channels [0, s0.c),
// s1 (optional: p == nullptr) the rest — a concatenated tensor has one source per part.
void gn_finalize(const GnSrc& s0, const GnSrc& s1, int N, int HW, int C, const float* gamma, const float* beta,
                 float eps, const float* film, int film_stride, float* scale, float* shift, hipStream_t s);
// whole GroupNorm32 (+ FiLM, + activation) of a small map in one launch: one workgroup per (group, sample)
bool gn_small_ok(int HW, int C);
void gn_small(const float* x, int N, int HW, int C, const float* gamma, const float* beta, float eps, const float* film,
              int film_stride, int act, float* y, hipStream_t s);
// avg_into (misc.hip) on [N][HW][C] sources + the per-column statistics of what it wrote: partial [N][gn_nchunks(HW,C)][C][2]
void avg_into_stats(const float* a, const float* b, const float* c, const float* d, float div, int N, int HW, int C,
                    float* dst, int dstC, int coff, int act, int bmask, double* partial, int nchunk, hipStream_t s);
enum { ACT_NONE = 0, ACT_SILU = 1 };
void affine_act(const float* x, int N, int HW, int C, const float* scale, const float* shift, int act, float* y,
                hipStream_t s);
void layer_norm(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* y,
                hipStream_t s);

// ---------------------------------------------------------------- attention.hip
struct AttnArgs {
    const float *q = nullptr, *k = nullptr, *v = nullptr;  // rows of ld* floats, head h at +h*hs*
    int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
    int q_hs = 0, k_hs = 0, v_hs = 0;
    int N = 0, Tq = 0, Tk = 0, heads = 0, d = 0;
    float scale_q = 1.f, scale_k = 1.f, scale_s = 1.f;
    float* out = nullptr;  // [N][Tq][ldo], head h at +h*d
    int split = 0;         // 1: both products on the bf16 matrix cores with operands split into 3 bf16 pieces (bf16x6), 0: fp32 MFMA
};
void attention(const AttnArgs& a, hipStream_t s);        // d % 4 == 0, d <= 128
void attention_wide(const AttnArgs& a, hipStream_t s);   // attention_wide.hip: 128 < d <= 512, d % 4 == 0
void attention_any(const AttnArgs& a, hipStream_t s);    // attention_wide.hip: dispatches on d between the two (d <= 512)

// ---------------------------------------------------------------- gemm16.hip / attention16.hip
// Single-product half-precision arithmetic of the transformer backbone (PREC_F16 / PREC_BF16: 16-bit operands, one MFMA per
// product, fp32 accumulation) — what the reference's DiT runs under fp16 autocast (BASELINE configs[4]).
enum { EPI16_STORE = 0, EPI16_GELU = 1, EPI16_GATED = 2 };
struct Gemm16Args {
    const void* x = nullptr;   // [M][ldx] 16-bit activations
    int ldx = 0;
    const void* w = nullptr;   // [N][K] 16-bit weights (nn.Linear layout)
    const float* bias = nullptr;
    int M = 0, N = 0, K = 0;
    int bf16 = 0;              // 0: fp16, 1: bf16
    int epi = EPI16_STORE;
    void* y16 = nullptr;       // EPI16_STORE / EPI16_GELU: [M][ldy] 16-bit
    int ldy = 0;
    float* x32 = nullptr;      // EPI16_GATED: x32[m][n] += gate[(m / T) * gate_stride + n] * round16(acc + bias)
    int ldx32 = 0;
    const float* gate = nullptr;
    int gate_stride = 0, T = 1;
    int qcols = 0;             // EPI16_STORE: columns < qcols are multiplied by qscale in fp32 before the rounding
    float qscale = 1.f;
};
bool gemm16_shape_ok(int M, int N, int K);
void gemm16(const Gemm16Args& a, hipStream_t s);
void gemm16_whatif(const Gemm16Args& a, int whatif, hipStream_t s);   // diagnostic instantiations (timing only), -1 = the product kernel
void cast16(const float* x, int64_t n, void* y, int bf16, hipStream_t s);      // fp32 -> fp16 / bf16, round to nearest even
void uncast16(const void* x, int64_t n, float* y, int bf16, hipStream_t s);
// ln_modulate (misc.hip) with a 16-bit result: the A operand of the following Linear
void ln_modulate16(const float* x, int N, int T, int C, const float* mod, int mod_stride, int shift_off, int scale_off, float eps,
                   void* y, int bf16, hipStream_t s);
struct Attn16Args {
    const void *q = nullptr, *k = nullptr, *v = nullptr;   // 16-bit rows of ld* elements, head h at +h*hs*
    int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
    int q_hs = 0, k_hs = 0, v_hs = 0;
    int N = 0, Tq = 0, Tk = 0, heads = 0, d = 0;
    float scale_q = 1.f;   // q * scale_q (fp32, rounded back) — 1 when q arrives pre-scaled by hd^-1/2 * log2(e); scores are base-2 logits
    float thr = -1.f;      // running-maximum threshold in log2 units (< 0: default 8; 0: move the maximum on every increase)
    int bf16 = 0;
    void* out = nullptr;   // [N][Tq][ldo] 16-bit, head h at +h*d
};
bool attention16_shape_ok(int d);
void attention16(const Attn16Args& a, hipStream_t s);
void attention16_whatif(const Attn16Args& a, int whatif, hipStream_t s);   // diagnostic instantiations (timing only), -1 = the product kernel

// ---------------------------------------------------------------- misc.hip
void timestep_embedding(const void* t, int t_is_float, int N, int dim, float* y, hipStream_t s,
                        const float* freqs = nullptr);
void linear(const float* x, int N, int K, int ldx, const float* w, const float* bias, int O, int act_in, float* y,
            int ldy, hipStream_t s);
void se_scale(const float* x, int N, int HW, int C, const float* w1, const float* w2, int Cr, float* y, hipStream_t s);
// dst[p, coff:coff+C] = act((a+b+c+d) * scale), sources NHWC [pixels][C]
// bmask bit k: source k is ONE sample ([per_sample_pixels][C]) broadcast over the batch of dst
void avg_into(const float* a, const float* b, const float* c, const float* d, float scale, int64_t pixels, int C,
              float* dst, int dstC, int coff, int act, hipStream_t s, int64_t per_sample_pixels = 0, int bmask = 0);
void nchw_to_nhwc(const float* x, int N, int C, int HW, float* y, hipStream_t s);
void nhwc_to_nchw(const float* x, int N, int C, int HW, float* y, hipStream_t s);
void avgpool2(const float* x, int N, int H, int W, int C, float* y, hipStream_t s);
void upsample2(const float* x, int N, int H, int W, int C, float* y, hipStream_t s);
void geglu(const float* x, int64_t rows, int inner, float* y, hipStream_t s);
// ---- DiT pieces (UNet_DS_Diff/DiT_models.py)
// LayerNorm without affine (eps) then modulate: y[n,t,:] = ((x - mean) * rstd) * (1 + scale[n,:]) + shift[n,:]; mod rows have
// stride mod_stride, shift at +shift_off, scale at +scale_off   (DiTBlock.forward :119-121, FinalLayer.forward :139-141)
void ln_modulate(const float* x, int N, int T, int C, const float* mod, int mod_stride, int shift_off, int scale_off, float eps,
                 float* y, hipStream_t s);
// x[n,t,:] += gate[n,:] * y[n,t,:]   (gate = mod + gate_off, the adaLN-Zero residual :120-121); in place on x
void gated_residual(float* x, const float* y, int N, int T, int C, const float* mod, int mod_stride, int gate_off, hipStream_t s);
// in place: GELU(approximate="tanh")
void gelu_tanh(float* x, int64_t n, hipStream_t s);
// x [N,C,H,W] -> tokens [N, (H/p)*(W/p), C*p*p] in Conv2d weight order (c, ph, pw)   (timm PatchEmbed = Conv2d(k = stride = p))
void patchify(const float* x, int N, int C, int H, int W, int p, float* y, hipStream_t s);
// tokens [N, h*w, p*p*c] (order ph, pw, c) -> [N, c, h*p, w*p]   (DiT.unpatchify :209-222)
void unpatchify(const float* x, int N, int c, int h, int w, int p, float* y, hipStream_t s);
// x[n,t,:] += pos[t,:]
void add_rows_broadcast(float* x, const float* pos, int N, int64_t TC, hipStream_t s);
// y[n,:] = (a ? a[n,:] : 0) + table[idx[n], :]   (LabelEmbedder: c = t_emb + y_emb :241-244); idx int64 on device
void embed_add(const float* a, const float* table, const long long* idx, int N, int C, float* y, hipStream_t s);
// in place: s[r][:] = softmax(s[r][:] * scale) over `cols` contiguous fp32 (one workgroup per row; max-subtracted, fp32)
void softmax_rows(float* s, int64_t rows, int cols, float scale, hipStream_t st);
void add2(const float* a, const float* b, int64_t n, float* y, hipStream_t s);

// ---------------------------------------------------------------- disc.hip
// Bottleneck head of UNet_disc_Model (Disc_diff/guided_diffusion/unet.py:1015-1033).  com / dist: the PRE-activation outputs of
// conv_common / conv_distinct on the four streams, NHWC [B][HW][half]; w1[k] [Cr][half] / w2[k] [half][Cr]: the SE linears of
// SE_Attention_com (k = 0) and SE_Attention_dist_1..4; cat [B][HW][5*half] = [SE_com(mean_i SiLU(com_i)), SE_dist_i(SiLU(dist_i))];
// feat (all eight or none), NHWC [B][HW][half]: SiLU(com_i) and the four scaled dist_i — the first eight values the forward returns.
struct DiscArgs {
    const float* com[4] = {};
    const float* dist[4] = {};
    const float* w1[5] = {};
    const float* w2[5] = {};
    int B = 0, HW = 0, half = 0, Cr = 0;
    float* cat = nullptr;
    float* feat[8] = {};
    void* scratch = nullptr;   // disc_scratch_bytes(B, HW, half, unfused) bytes
};
int disc_nchunks(int HW);
size_t disc_scratch_bytes(int B, int HW, int half, bool unfused);
bool disc_unfused_env();                                       // DSD_DISC_UNFUSED set (and not "0"), read at every call
void disc_bottleneck(const DiscArgs& a, hipStream_t s);          // three launches: pool, gate, scale
void disc_bottleneck_unfused(const DiscArgs& a, hipStream_t s);  // avg_into / se_scale / concat copies (A/B, cross-check)

// ---------------------------------------------------------------- sampler.hip
struct StepCoef {
    float c[8];
    int mode, pred, learned_range, clip, nonzero;
    float eta;
};
// out_c: the model output, row b at out_c + b*o_bs (0 = Cz*HW, or 2*Cz*HW with learned_range): channels [0,Cz) the prediction,
// [Cz,2Cz) the learned-range variance (read with learned_range only); x in/out [B,Cz,HW] with row stride x_bs (0 = Cz*HW);
// noise [B,Cz,HW] or null (Philox)
// slice_ids (optional, device [B]): global slice index of every batch row — the Philox counter of element r = c*HW + p of row b
// is slice_ids[b]*Cz*HW + r instead of b*Cz*HW + r, so a slice's noise does not depend on how the volume was sharded or batched
// Classifier-free guidance (out_u != nullptr, DSD_MODE_B_DDIM): the network ran on 2B rows (uncond half first), out_u / out_c are
// the two [B,..] halves of its output and x is the 2B-row state (logical sample b at rows b and B+b, row stride x_bs); the
// update runs on out = out_u + scale*(out_c - out_u) and both rows receive x_{t-1}.  noise, x0_out and slice_ids stay per
// logical sample.
void sampler_update(const StepCoef& sc, const float* out_u, const float* out_c, float scale, float* x, const float* noise,
                    uint64_t seed, uint64_t step, int B, int HW, hipStream_t s, float* x0_out = nullptr,
                    const int64_t* slice_ids = nullptr, int Cz = 1, int64_t x_bs = 0, int64_t o_bs = 0);
// DPM-Solver(++) multistep: coefficients of one network evaluation + update (host tables, include/dsdiff.h dsd_dpm_schedule)
struct DpmCoef {
    float alpha, sigma;      // marginal alpha_t, sigma_t at the evaluation time
    float cx, cm, cd, ir0;   // x <- (cx*x - cm*m0) - cd*(ir0*(m0 - m1))
    int order;               // 0: x <- m0 (denoise to zero), 1, 2
    int pred;                // DSD_PRED_* of the network
    int data_pred, thresh;
};
// out_u != nullptr: guided as in sampler_update, noise = noise_u + scale*(noise_c - noise_u) on the two noise predictions;
// m_cur / m_prev and s_buf are per logical sample
void dpm_step(const DpmCoef& c, const float* out_u, const float* out_c, int Cm, float scale, float* x, float* m_cur,
              const float* m_prev, float* s_buf, float ratio, float max_val, int B, int HW, hipStream_t s, int64_t x_bs = 0);
// One evaluation of a DPM-Solver program (include/dsdiff.h dsd_dpm_program; forms in sampler.hip): after the model value of
// the evaluation is in plane mw (dpm_model / dpm_quantile with `c`), dpm_eval_kernel thresholds it there and writes the next
// state from ma / mb / mc (history planes [B,HW]; mb, mc null where the kind reads none) and the base state — the state
// itself, or for the singlestep kinds from SS_S2 on the plane `base`, which SS_S1 fills.
struct DpmEval {
    float c[9] = {};               // DSD_DPM_NCOEF (sampler.hip asserts it)
    int kind = 0;                  // DSD_DPM_*
    float* mw = nullptr;
    const float* ma = nullptr;
    const float* mb = nullptr;
    const float* mc = nullptr;
    const float* s_thr = nullptr;  // set by dpm_eval
    float* x = nullptr;            // state row b at x + b*x_bs (0 = HW); dup (set by dpm_eval when guided): also row B+b
    float* base = nullptr;
    int64_t x_bs = 0;
    int dup = 0;
};
void dpm_eval(const DpmCoef& c, const DpmEval& e, const float* out_u, const float* out_c, int Cm, float scale, float* s_buf,
              float ratio, float max_val, int B, int HW, hipStream_t s);
// The error estimate of one adaptive DPM-Solver trial (dpm_solver_adaptive, sampler.py:965-977) on B logical samples of n
// elements, from the planes a singlestep step leaves behind: x_lower = c0*base - c1*ma (lower_order 1) or (c0*base - c1*ma) -
// c2*(mb - ma) (lower_order 2) through dpm_eval_value, written to x_lower [B,n]; delta = max(atol, rtol*max(|x_lower|,
// |x_prev|)); err[b] = sqrt(mean(((x_higher - x_lower)/delta)^2)).  base / ma / mb / x_prev are [B,n]; x_higher row b sits at
// xh + b*x_bs (0 = n; the first B rows of a guided 2B-row state).  part: dpm_adaptive_part_doubles(B) doubles of scratch.
struct DpmAdaptiveErr {
    float c[3] = {};
    int lower_order = 1;
    float atol = 0.f, rtol = 0.f;
    const float* base = nullptr;
    const float* ma = nullptr;
    const float* mb = nullptr;     // null for lower_order 1
    const float* xh = nullptr;
    const float* x_prev = nullptr;
    float* x_lower = nullptr;
    int64_t x_bs = 0;
    double* part = nullptr;
    float* err = nullptr;          // device [B]
};
size_t dpm_adaptive_part_doubles(int B);
void dpm_adaptive_error(const DpmAdaptiveErr& a, int B, int64_t n, hipStream_t s);
// Image-to-image.  q_sample (+ mask blend): img_orig = a*x0 + s*z with a, s scalars or per row from the device arrays a_row /
// s_row; mask != nullptr ([B,mask_ch,HW], mask_ch 1 or Cz): x = img_orig*mask + (1 - mask)*x, else x = img_orig.  x0 / noise are
// [B,Cz,HW]; the state row b is x + b*x_bs (0 = Cz*HW); dup: also written to row B+b (guided 2B-row state).  noise == nullptr:
// Philox stream (seed, step + 2^32), counter keyed by slice_ids like the update's.
void q_sample_blend(float a, float s, const float* a_row, const float* s_row, const float* x0, const float* mask, int mask_ch,
                    float* x, const float* noise, uint64_t seed, uint64_t step, int B, int Cz, int HW, hipStream_t st,
                    int64_t x_bs = 0, bool dup = false, const int64_t* slice_ids = nullptr);
// DDIM inversion step: x = cx*x + ce*e, e = out_c or (out_u != nullptr) out_u + scale*(out_c - out_u), then written to both rows
// (output rows of o_bs elements, 0 = Cz*HW: the prediction is their first Cz*HW)
void ddim_invert_step(float cx, float ce, const float* out_u, const float* out_c, float scale, float* x, int B, int Cz, int HW,
                      hipStream_t st, int64_t x_bs = 0, int64_t o_bs = 0);
// PLMS (sampler.hip): one update of PLMSSampler.p_sample_plms (ldm/models/diffusion/plms.py:206-243) on B logical samples of
// n = Cz*HW elements.  order (DSD_PLMS_*): 0 predict / 1 correct = the two halves of the first step around its second network
// evaluation, 2..4 = Adams-Bashforth on 1..3 earlier noise predictions.  out_u == nullptr: e_t = out_c, else e_t = out_u +
// scale*(out_c - out_u) and x_{t-1} goes to rows b and B+b.  h_new: the history plane that receives e_t (order 0, 2, 3, 4; for
// order 4 it holds the oldest prediction, which the same thread reads first) and from which order 1 reads it back; o1 / o2: the
// newest and second-newest earlier predictions; x_saved [B,n]: written with x_t by order 0, read by order 1.  thr > 0:
// pred_x0 *= thr / max(rms(pred_x0), thr) per sample; `part` then needs plms_norm_doubles(B, n) doubles of scratch.
struct PlmsStep {
    float a_t = 0.f, a_prev = 0.f, sigma = 0.f, s1m = 0.f;
    int order = 0;
    float thr = 0.f, scale = 1.f;
    const float* out_u = nullptr;
    const float* out_c = nullptr;
    float* h_new = nullptr;
    const float* o1 = nullptr;
    const float* o2 = nullptr;
    float* x_saved = nullptr;
    float* x = nullptr;
    int64_t x_bs = 0;
    int64_t o_bs = 0;        // row stride of out_u / out_c (0 = n; 2n for a model with a variance half, left unread)
    double* part = nullptr;
    float* x0_out = nullptr; // optional [B,n]: the pred_x0 this update forms (after the threshold), get_x_prev_and_pred_x0's second value
};
size_t plms_norm_doubles(int B, int64_t n);
void plms_step(const PlmsStep& a, int B, int Cz, int HW, hipStream_t s);
// Variational bound (sampler.hip; gaussian_diffusion.py:788-819, 938-991): the terms of one timestep on B samples of n = Cz*HW
// elements from the network output of x_t = q_sample(x_start, t, noise).  sc: the DSD_MODE_A_DDPM coefficients of the step;
// post_log_var: posterior_log_variance_clipped[t] (c[6] except under FIXED_LARGE).  x_start / noise and the optional planes
// mean / log_variance / pred_xstart are [B,n]; x_t row b at xt + b*x_bs (0 = n); output row b at out + b*o_bs (0 = n, 2n with
// learned_range: the variance half follows the prediction).  noise == nullptr: the normals of Philox stream (seed, step + 2^32),
// counter keyed by slice_ids — the ones q_sample_blend drew x_t from.  part: vlb_part_doubles(B, n) doubles of scratch.
struct VlbStep {
    StepCoef sc;
    float post_log_var = 0.f;
    const float* x_start = nullptr;
    const float* xt = nullptr;
    const float* out = nullptr;
    const float* noise = nullptr;
    int64_t x_bs = 0, o_bs = 0;
    uint64_t seed = 0, step = 0;
    const int64_t* slice_ids = nullptr;
    double* part = nullptr;
    float* mean = nullptr;
    float* log_variance = nullptr;
    float* pred_xstart = nullptr;
};
size_t vlb_part_doubles(int B, int64_t n);
// the one finalize of every per-sample reduction (vlb_terms, prior_bpd, loss.hip): out_q[b*stride] = fp32(sum_q / n) from
// part[b][nblk][nq] (nq <= 3; null outputs skipped), added in index order by one wave; bits: quantity 0 is divided by ln 2
void rows_finalize(const double* part, int nblk, int nq, int n, float* o0, float* o1, float* o2, int64_t stride, int bits, int B,
                   hipStream_t s);
// decoder: t == 0, the term is the discretised decoder NLL instead of the KL.  Sample b's vb (bits), mean (pred_xstart - x_start)^2
// and mean (eps - noise)^2 go to vb / xstart_mse / mse [b*term_stride] (each optional; all null: the planes only).
void vlb_terms(const VlbStep& a, bool decoder, float* vb, float* xstart_mse, float* mse, int64_t term_stride, int B, int Cz, int HW,
               hipStream_t s);
// _prior_bpd (:922-936): mean normal_kl(c0*x_start, logvar, 0, 0) / ln 2 per sample; part: vlb_part_doubles(B, n) doubles
void prior_bpd(float c0, float logvar, const float* x_start, double* part, float* prior, int B, int64_t n, hipStream_t s);
// ddim_reverse_sample (:691-701) in place on the state rows; x0_out (optional, [B,Cz*HW]) receives the clipped pred_xstart
void ddim_reverse_step(const StepCoef& sc, float abar_next, const float* out, float* x, float* x0_out, int B, int Cz, int HW,
                       hipStream_t st, int64_t x_bs = 0, int64_t o_bs = 0);
void dpm_threshold(const float* x0, float* y, float* s_buf, float ratio, float max_val, int B, int n, hipStream_t s);
void philox_normal(float* y, int64_t n, uint64_t seed, uint64_t step, hipStream_t s);
// DiagonalGaussianDistribution.sample (ldm/modules/distributions/distributions.py:24-37): moments [B,2E,HW] (NCHW) ->
// z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps), eps = noise[B,E,HW] or Philox normals (noise == nullptr)
void gaussian_sample(const float* moments, const float* noise, uint64_t seed, int B, int E, int HW, float* z, hipStream_t s,
                     float scale = 1.0f);
void fill_t(float* t, int B, float v, hipStream_t s);

// ---------------------------------------------------------------- loss.hip
// The denoising losses (training_losses / p_losses, forward only): one scalar per sample, every timestep-dependent value a
// device row [B].  Reductions as vlb_terms': fixed per-block fp64 partials, one finalize, no atomics.
// loss[b*stride] = mean over the n = Cz*HW elements of kind(target - out): target (DSD_PRED_*) = the noise, x_start, or
// a_row[b]*noise - s_row[b]*x_start (get_v); kind (DSD_LOSS_*) = d^2, |d| or sqrt(d^2 + 1e-6).  Output row b at out + b*o_bs
// (0 = n; 2n reads the prediction half of an output with a variance half in place); x_start / noise [B,n] (each read only by
// the targets that need it); noise == nullptr: the normals q_sample_blend drew x_t from (Philox stream (seed, step + 2^32),
// counter keyed by slice_ids).  part: loss_part_doubles(B, n) doubles of scratch.
struct LossRows {
    const float* out = nullptr;
    int64_t o_bs = 0;
    const float* x_start = nullptr;
    const float* noise = nullptr;
    const float* a_row = nullptr;
    const float* s_row = nullptr;
    int target = 0, kind = 0;
    uint64_t seed = 0, step = 0;
    const int64_t* slice_ids = nullptr;
    double* part = nullptr;
    float* loss = nullptr;
    int64_t stride = 1;
};
size_t loss_part_doubles(int B, int64_t n);
void loss_rows(const LossRows& a, int B, int Cz, int HW, hipStream_t s);
// out[b*stride] = sum over the pairs (i, j) of the nf (2..4) feature tensors of mean((f_i - f_j)^2) over n elements, each pair's
// mean rounded to fp32 and added in the reference's order: (1,2) + (2,3) + (1,3), then + ((1,4) + (2,4) + (3,4)).  Row b of
// tensor i at f[i] + b*bs (0 = n).  part: pair_part_doubles(B, n) doubles.
struct PairMse {
    const float* f[4] = {};
    int nf = 0;
    int64_t bs = 0;
    double* part = nullptr;
    float* out = nullptr;
    int64_t stride = 1;
};
size_t pair_part_doubles(int B, int64_t n);
void pair_mse_rows(const PairMse& a, int B, int64_t n, hipStream_t s);
// vlb_terms with a timestep per sample: coef [B,DSD_NCOEF] (the DSD_MODE_A_DDPM rows), post_log_var [B], decoder [B] (t == 0:
// the discretised decoder NLL instead of the KL), all on the device; a.sc gives pred / learned_range / clip, its c is unread.
struct VlbRows {
    const float* coef = nullptr;
    const float* post_log_var = nullptr;
    const int32_t* decoder = nullptr;
};
void vlb_terms_rows(const VlbStep& a, const VlbRows& r, float* vb, float* xstart_mse, float* mse, int64_t term_stride, int B, int Cz,
                    int HW, hipStream_t s);

// ---------------------------------------------------------------- contrast.hip
// The disentanglement losses over R = n_views*B feature rows of n elements (row view*B + b at v[view] + b*bs, bs 0 = n): the
// R x R matrix of fp64 dot products (or L1 distances) from fixed per-slice partials added in index order, then one workgroup
// that turns the matrix and labels [R] into loss[1] and the fp32 logits [R,R] of `mode` (DSD_CONTRAST_*).  part:
// contrast_part_doubles(R, n) doubles.  No atomics: two runs agree bit for bit.
struct ContrastRows {
    const float* v[8] = {};   // DSD_CONTRAST_MAX_VIEWS
    int64_t bs = 0;
    const int32_t* labels = nullptr;
    double* part = nullptr;
    float* loss = nullptr;
    float* logits = nullptr;
};
size_t contrast_part_doubles(int R, int64_t n);
// the argument checks that need no pointer (the callers of the C ABI run them before any device work)
void contrast_check(int n_views, int B, int64_t n, int mode, float temperature);
void contrast_rows(const ContrastRows& a, int n_views, int B, int64_t n, int mode, float temperature, hipStream_t s);

// ---------------------------------------------------------------- metrics.hip
// MAE / MSE sums, Gaussian SSIM (11 taps, sigma 1.5, valid interior) and the MS-SSIM scale table of pred against target, fp32
// [B,C,H,W], in fp64 from the load onward: scale_out[B][scales][2] = the mean of the ssim map and of the contrast-structure map
// per sample and scale (over the channels and the interior, unclamped), elem_out[B][6] = sum |p - t|, sum (p - t)^2, min t,
// max t, min p, max p.  data_range 0: each sample's own max(range(pred), range(target)).  pre: NULL or the host's seven doubles
// (mean_p, div_p, mean_t, div_t, add, lo, hi) of y = clip((x - mean) / div + add, lo, hi), applied at the load.  scratch:
// image_metrics_scratch_doubles(...) doubles.  Fixed per-tile partials, a fixed fold: two runs agree bit for bit.
static constexpr int kMtTileW = 32, kMtTileH = 16;   // outputs one workgroup of the map kernel owns (DSD_METRICS_TILE_W / _H)
struct ImageMetrics {
    const float* pred = nullptr;
    const float* target = nullptr;
    int B = 0, C = 0, H = 0, W = 0, scales = 1;
    double data_range = 1.0;
    const double* pre = nullptr;
    double* scratch = nullptr;
    double* scale_out = nullptr;
    double* elem_out = nullptr;
};
size_t image_metrics_scratch_doubles(int B, int C, int H, int W, int scales);
// the argument checks that need no device pointer (the C ABI runs them before any device work)
void image_metrics_check(int B, int C, int H, int W, int scales, double data_range, const double* pre);
void image_metrics(const ImageMetrics& a, hipStream_t s);

// ---------------------------------------------------------------- volume_metrics.hip
// The metric table of one volume pair [D,H,W] (float or double elements, fp64 from the load onward): NRMSE, MAPE, sMAPE, logac,
// medsymac over the mask M, PSNR over the masked crop Z, the win^3 box-window SSIM over R, and the auxiliary values, into
// out[DSD_VOLUME_NOUT] (device) with a status word among them; definitions in include/dsdiff.h.  scratch:
// volume_metrics_scratch_bytes(...) bytes.  Fixed per-workgroup partials, a fixed fold, integer atomics in the histograms only:
// two runs agree bit for bit.
static constexpr int kVmTileW = 32, kVmTileH = 16;   // window positions one workgroup of the ssim3d row kernel owns (DSD_VOLUME_TILE_W / _H)
struct VolumeMetrics {
    const void* target = nullptr;
    const void* pred = nullptr;
    int elem_is_double = 0;
    const uint8_t* mask = nullptr;
    int D = 0, H = 0, W = 0, win = 0;
    void* scratch = nullptr;
    double* out = nullptr;
};
size_t volume_metrics_scratch_bytes(int D, int H, int W, int win);
// the argument checks that need no device pointer (the C ABI runs them before any device work)
void volume_metrics_check(int D, int H, int W, int win, int elem_is_double);
void volume_metrics(const VolumeMetrics& a, hipStream_t s);
// out[0] = the k-th smallest (0-based) of x[n] (device, no NaN), exactly: radix selection on the order-preserving image of the bits
size_t kth_double_scratch_bytes();
void kth_double_check(int64_t n, int64_t k);
void kth_double(const double* x, int64_t n, int64_t k, void* scratch, double* out, hipStream_t s);

}  // namespace dsd
