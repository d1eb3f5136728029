// loss.hip — the denoising losses, one scalar per sample.
//
// GaussianDiffusion.training_losses (Disc_diff/guided_diffusion/gaussian_diffusion.py:821-920 and its training_project twin),
// DDPM.get_v / get_loss / p_losses (ldm/models/diffusion/ddpm.py:361-415) and LatentDiffusion.p_losses (:892-927), forward only.
// Unlike every loop of sampler.hip these draw a timestep per SAMPLE, so whatever depends on t arrives as device rows [B].
//
// All three reductions follow the variational bound's (sampler.hip): grid x over the 1024-element pieces of one sample, y = the
// sample; a thread owns four consecutive elements (no grid-stride loop), sums in fp64, the block folds in a fixed LDS tree into
// part[b][piece][quantity]; a one-wave finalize adds the pieces in index order.  No atomics: two runs agree bit for bit.
#include "sampler_dev.h"

#pragma clang fp contract(off)

namespace dsd {

static int row_blocks(int64_t n) { return (int)((n + kVlbPiece - 1) / kVlbPiece); }
static void check_rows(const char* what, int B, int64_t n) {
    DSD_CHECK(n <= (int64_t)1 << 30, "%s: one sample has %lld elements; up to 2^30 are taken", what, (long long)n);
    DSD_CHECK(B <= 65535, "%s: %d samples; up to 65535 are taken", what, B);
}

// ------------------------------------------------------------------------------------------------------------------ loss_rows
// target - pred per element: the noise (eps), x_start (x0) or get_v's a*noise - s*x_start; then (target - pred)^2, |target - pred|
// or L1_Charbonnier_loss's sqrt(d*d + 1e-6) with d = X + (-Y) = target - pred.
template <int V>
__global__ __launch_bounds__(256) void loss_rows_kernel(LossRows a, int n) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    const int64_t row = (int64_t)b * n;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int valid = n - p;
    double acc[1] = {0.0};
    if (valid > 0) {
        const Pack<4> out = ld_quad<V>(a.out + (int64_t)b * a.o_bs + p, valid);
        Pack<4> xs = {}, z = {};
        if (a.target != DSD_PRED_EPS) xs = ld_quad<V>(a.x_start + row + p, valid);
        if (a.target != DSD_PRED_X0) {
            if (a.noise)
                z = ld_quad<V>(a.noise + row + p, valid);
            else
                z = philox_quad<V>((a.slice_ids ? a.slice_ids[b] * n : row) + p, a.seed, a.step, valid);
        }
        float ca = 0.f, cs = 0.f;
        if (a.target == DSD_PRED_V) { ca = a.a_row[b]; cs = a.s_row[b]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float target;
            if (a.target == DSD_PRED_EPS) target = z.v[j];
            else if (a.target == DSD_PRED_X0) target = xs.v[j];
            else target = ca * z.v[j] - cs * xs.v[j];                        // get_v ddpm.py:361-365
            const float d = target - out.v[j];
            float e;
            if (a.kind == DSD_LOSS_L2) e = d * d;
            else if (a.kind == DSD_LOSS_L1) e = fabsf(d);
            else e = sqrtf(d * d + 1e-6f);                                   // L1_Charbonnier_loss :18-28
            if (j < valid) acc[0] += (double)e;
        }
    }
    vlb_block_fold<1>(acc, red, a.part + (int64_t)b * gridDim.x + blockIdx.x);
}

size_t loss_part_doubles(int B, int64_t n) { return (size_t)B * row_blocks(n); }

void loss_rows(const LossRows& arg, int B, int Cz, int HW, hipStream_t s) {
    LossRows a = arg;
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    check_rows("loss_rows", B, n);
    DSD_CHECK(a.out && a.part && a.loss, "loss_rows: null argument");
    DSD_CHECK(a.target >= DSD_PRED_EPS && a.target <= DSD_PRED_V, "loss_rows: unknown target %d", a.target);
    DSD_CHECK(a.kind >= DSD_LOSS_L2 && a.kind <= DSD_LOSS_CHARBONNIER, "loss_rows: unknown loss kind %d", a.kind);
    DSD_CHECK(a.target == DSD_PRED_EPS || a.x_start, "loss_rows: the x0 and v targets read x_start (null)");
    DSD_CHECK(a.target != DSD_PRED_V || (a.a_row && a.s_row), "loss_rows: the v target reads the rows a and s (null)");
    if (a.o_bs <= 0) a.o_bs = n;
    DSD_CHECK(a.o_bs >= n, "loss_rows: output rows of %lld elements, a sample has %lld", (long long)a.o_bs, (long long)n);
    if (a.stride <= 0) a.stride = 1;
    const int nblk = row_blocks(n);
    launch_vec(can_vec4(n, a.o_bs, a.out, a.x_start, a.noise), [&](auto V) {
        hipLaunchKernelGGL(loss_rows_kernel<decltype(V)::value>, dim3(nblk, B), dim3(256), 0, s, a, (int)n);
    });
    check_launch("loss_rows");
    rows_finalize(a.part, nblk, 1, (int)n, a.loss, nullptr, nullptr, a.stride, 0, B, s);
}

// -------------------------------------------------------------------------------------------------------------- pair_mse_rows
// The DisC-Diff com / dist terms (:898-910): per sample the sum over the pairs of nf feature tensors of mean_flat((f_i - f_j)^2).
// Quantity q of the reduction is one pair, in the reference's order: (1,2), (2,3), (1,3), then with a fourth (1,4), (2,4), (3,4).
template <int V>
__global__ __launch_bounds__(256) void pair_mse_kernel(PairMse a, int n) {
    __shared__ double red[6 * 256];
    const int b = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int valid = n - p;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (valid > 0) {
        Pack<4> f[4] = {};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < a.nf) f[i] = ld_quad<V>(a.f[i] + (int64_t)b * a.bs + p, valid);
        const int npair = a.nf == 2 ? 1 : a.nf == 3 ? 3 : 6;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            if (q >= npair) break;
            const int i = q == 1 ? 1 : q == 4 ? 1 : q == 5 ? 2 : 0;          // the pair (i, k) of quantity q; q is unrolled
            const int k = q == 0 ? 1 : q <= 2 ? 2 : 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = f[i].v[j] - f[k].v[j];
                if (j < valid) acc[q] += (double)(d * d);
            }
        }
    }
    vlb_block_fold<6>(acc, red, a.part + ((int64_t)b * gridDim.x + blockIdx.x) * 6);
}

// every pair's mean rounded to fp32 (mean_flat), then the reference's fp32 sums: (m12 + m23) + m13, += (m14 + m24) + m34
__global__ __launch_bounds__(64) void pair_finalize_kernel(const double* __restrict__ part, int nblk, int nf, int n, float* out,
                                                           int64_t stride) {
    __shared__ double red[6 * 64];
    const int b = blockIdx.x;
    rows_fold_partials(part, b, nblk, 6, red);
    if (threadIdx.x == 0) {
        float m[6];
        for (int q = 0; q < 6; ++q) m[q] = rows_mean_value(red[q * 64], n, false);
        float v = m[0];
        if (nf >= 3) v = m[0] + m[1] + m[2];
        if (nf == 4) v = v + (m[3] + m[4] + m[5]);
        out[(int64_t)b * stride] = v;
    }
}

size_t pair_part_doubles(int B, int64_t n) { return (size_t)B * row_blocks(n) * 6; }

void pair_mse_rows(const PairMse& arg, int B, int64_t n, hipStream_t s) {
    PairMse a = arg;
    if (!B || !n) return;
    check_rows("pair_mse_rows", B, n);
    DSD_CHECK(a.nf >= 2 && a.nf <= 4, "pair_mse_rows takes 2, 3 or 4 feature tensors, got %d", a.nf);
    for (int i = 0; i < a.nf; ++i) DSD_CHECK(a.f[i], "pair_mse_rows: feature tensor %d is null", i);
    DSD_CHECK(a.part && a.out, "pair_mse_rows: null argument");
    if (a.bs <= 0) a.bs = n;
    if (a.stride <= 0) a.stride = 1;
    const int nblk = row_blocks(n);
    launch_vec(can_vec4(n, a.bs, a.f[0], a.f[1], a.f[2], a.f[3]), [&](auto V) {
        hipLaunchKernelGGL(pair_mse_kernel<decltype(V)::value>, dim3(nblk, B), dim3(256), 0, s, a, (int)n);
    });
    check_launch("pair_mse_rows");
    hipLaunchKernelGGL(pair_finalize_kernel, dim3(B), dim3(64), 0, s, a.part, nblk, a.nf, (int)n, a.out, a.stride);
    check_launch("pair_mse_finalize");
}

// ------------------------------------------------------------------------------------------------------------- vlb_terms_rows
// vlb_terms (sampler.hip) with everything that depends on t per sample: the coefficient row, the true posterior's log-variance
// and the t == 0 select.  The block is one sample's, so the select is block-uniform; both arms are the device functions of
// vlb_terms_kernel, and with one t shared by the batch the results are its bits.
template <int V>
__global__ __launch_bounds__(256) void vlb_terms_rows_kernel(VlbStep a, VlbRows r, int n) {
    __shared__ double red[3 * 256];
    const int b = blockIdx.y;
    StepCoef sc = a.sc;
#pragma unroll
    for (int j = 0; j < DSD_NCOEF; ++j) sc.c[j] = r.coef[(int64_t)b * DSD_NCOEF + j];
    const float plv = r.post_log_var[b];
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    double acc[3] = {0.0, 0.0, 0.0};
    if (r.decoder[b])
        vlb_thread_terms<V, true>(a, sc, plv, b, n, p, acc);
    else
        vlb_thread_terms<V, false>(a, sc, plv, b, n, p, acc);
    vlb_block_fold<3>(acc, red, a.part + ((int64_t)b * gridDim.x + blockIdx.x) * 3);
}

void vlb_terms_rows(const VlbStep& step, const VlbRows& r, float* vb, float* xstart_mse, float* mse, int64_t term_stride, int B,
                    int Cz, int HW, hipStream_t s) {
    VlbStep a = step;
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    check_rows("variational bound (rows)", B, n);
    DSD_CHECK(a.part, "variational bound (rows): the reduction needs its scratch");
    DSD_CHECK(r.coef && r.post_log_var && r.decoder, "variational bound (rows): null coefficient rows");
    const int64_t need = (a.sc.learned_range ? 2 : 1) * n;
    if (a.x_bs <= 0) a.x_bs = n;
    if (a.o_bs <= 0) a.o_bs = need;
    DSD_CHECK(a.o_bs >= need, "variational bound (rows): output rows of %lld elements, the terms read %lld", (long long)a.o_bs,
              (long long)need);
    const bool v4 = can_vec4(n, a.x_bs, a.x_start, a.xt, a.out, a.noise, a.mean, a.log_variance, a.pred_xstart) && a.o_bs % 4 == 0;
    const int nblk = row_blocks(n);
    launch_vec(v4, [&](auto V) {
        hipLaunchKernelGGL(vlb_terms_rows_kernel<decltype(V)::value>, dim3(nblk, B), dim3(256), 0, s, a, r, (int)n);
    });
    check_launch("vlb_terms_rows");
    if (!vb && !xstart_mse && !mse) return;
    rows_finalize(a.part, nblk, 3, (int)n, vb, xstart_mse, mse, term_stride > 0 ? term_stride : (int64_t)1, 1, B, s);
}

}  // namespace dsd
