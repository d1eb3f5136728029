// sampler.hip — the per-step sampler update as ONE fused elementwise kernel (+ on-device Philox noise).
//
// Mode A  = guided-diffusion: p_mean_variance / p_sample / ddim_sample
//           (Disc_diff/guided_diffusion/gaussian_diffusion.py:244-350, 422-465, 618-665)
// Mode B  = LDM: DDPMModel.p_sample / p_mean_variance (trainers/trainer_ddpm.py:461-482, with
//           ldm/models/diffusion/ddpm.py:284-311) and DDIMSampler.p_sample_ddim (ldm/models/diffusion/ddim.py:187-261);
//           PLMSSampler.p_sample_plms with norm thresholding (ldm/models/diffusion/plms.py:178-245), further down.
// The arithmetic is written in the reference's fp32 operation order; coefficient tables come from the host
// (float64 there, rounded to fp32 once, like _extract_into_tensor(...).float() / the registered fp32 buffers).
#include "sampler_dev.h"

// The reference evaluates these updates as separate fp32 torch ops, so nothing in this file may be contracted into an
// FMA: plain operators under contract(off) (HIP's __fmul_rn/__fsub_rn are header inlines that stay contractable);
// fmaf() is written where torch itself fuses.
#pragma clang fp contract(off)

namespace dsd {

__global__ void philox_normal_kernel(float* __restrict__ y, int64_t n, uint64_t seed, uint64_t step) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        y[i] = philox_normal_at(i, seed, step);
}

void philox_normal(float* y, int64_t n, uint64_t seed, uint64_t step, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65535)), dim3(256), 0, s, y, n, seed, step);
    check_launch("philox_normal");
}

static int ew_blocks(int64_t work) { return (int)std::min<int64_t>((work + 255) / 256, 2048); }

// p_sample_ddim after the network output is formed (ddim.py:222-260): returns x_{t-1}, x0 = the (clipped) pred_x0
__device__ __forceinline__ float ddim_update(const StepCoef& sc, float out, float xt, float z, float& x0) {
    const float* c = sc.c;
    float e_t;
    if (sc.pred == DSD_PRED_V) {
        e_t = c[0] * out + c[1] * xt;   // predict_eps_from_z_and_v ddpm.py:298-302
        x0 = c[0] * xt - c[1] * out;    // predict_start_from_z_and_v ddpm.py:290-296
    } else {
        e_t = out;
        x0 = (xt - c[7] * e_t) / sqrtf(c[4]);
    }
    if (sc.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const float dir = sqrtf(1.f - c[5] - c[6] * c[6]) * e_t;
    return sqrtf(c[5]) * x0 + dir + c[6] * z;
}

// x_{t-1} of one element in any of the four modes; var = the learned-range variance channel (read only with learned_range)
__device__ __forceinline__ float sampler_update_value(const StepCoef& sc, float out, float xt, float z, float var, float& x0) {
    if (sc.mode == DSD_MODE_B_DDIM) return ddim_update(sc, out, xt, z, x0);
    const float* c = sc.c;
    x0 = pred_xstart_value(sc, out, xt);
    const float nz = sc.nonzero ? 1.f : 0.f;
    if (sc.mode == DSD_MODE_A_DDIM) {
        // gaussian_diffusion.py:646-664
        const float eps = (c[2] * xt - x0) / c[3];
        const float ab = c[4], abp = c[5];
        const float sigma = sc.eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
        const float mean_pred = x0 * sqrtf(abp) + sqrtf(1.f - abp - sigma * sigma) * eps;
        return mean_pred + nz * sigma * z;
    }
    // DDPM: q_posterior mean + exp(0.5 logvar) z   (gaussian_diffusion.py:220-223,464; trainer_ddpm.py:467)
    const float mean = c[4] * x0 + c[5] * xt;
    const float logvar = model_log_variance(sc, var);
    return mean + nz * expf(0.5f * logvar) * z;
}

// One sample is n = Cz*HW elements (r = c*HW + p inside it).  The state row b lives at x + b*x_bs: x_bs = n for a state of its
// own, (Cz+Cc)*HW when the state is the first Cz channels of the denoiser's NCHW input (the latent loop writes x_{t-1} straight
// into the buffer the network reads next).  Noise and x0_out are contiguous [B,Cz,HW].  The model output row b lives at
// mo + b*o_bs: its first n elements are the prediction (channels [0,Cz)), the n after them the learned-range variance (channels
// [Cz,2Cz): frac of (b, c, p) at o_bs*b + n + c*HW + p, gaussian_diffusion.py:280-294); o_bs = n, or 2n for a model with a
// variance half, which every mode without learned variance leaves unread.  The
// Philox counter of (row b, channel c, pixel p) is (slice_ids ? slice_ids[b] : b)*n + r: distinct channels never share a normal.
// Classifier-free guidance (mo_u != nullptr; ddim.py:194-219): the network ran on 2B rows — x_in = cat([x]*2), c_in =
// cat([uncond, cond]) — so its output arrives as the halves mo_u / mo_c and the state occupies 2B rows, logical sample b at rows
// b and B+b.  Both hold x_t on entry; the kernel forms out = out_u + gs*(out_c - out_u) on the raw outputs (ddim.py:219), reads
// row b and writes x_{t-1} to both, so the next evaluation needs no copy.  Everything else — noise, Philox counters, slice_ids,
// x0_out — is indexed by the B logical samples.
template <int V>
__global__ __launch_bounds__(256) void sampler_update_kernel(StepCoef sc, const float* __restrict__ mo_u,
                                                             const float* __restrict__ mo_c, float gs, float* __restrict__ x,
                                                             const float* __restrict__ noise, uint64_t seed, uint64_t step,
                                                             int B, int64_t n, int64_t x_bs, int64_t o_bs,
                                                             float* __restrict__ x0_out,
                                                             const int64_t* __restrict__ slice_ids) {
    const int64_t nv = n / V;
    // One pack per thread and no grid-stride loop: out of a loop the compiler hoists the constants of the inlined logf / sinf /
    // cosf into scalar registers, more than there are once all four modes and both output halves are live (it spilled them).
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * nv) return;
    const int64_t b = i / nv;
    const int64_t p = (i - b * nv) * V;
    const int64_t li = b * n + p;                                // in the [B,n] tensors
    const int64_t oi = b * o_bs + p;                             // in the model output
    const int64_t xi = b * x_bs + p;
    Pack<V> out = ld_pack<V>(mo_c + oi);
    if (mo_u) {
        const Pack<V> ou = ld_pack<V>(mo_u + oi);
#pragma unroll
        for (int j = 0; j < V; ++j) out.v[j] = ou.v[j] + gs * (out.v[j] - ou.v[j]);
    }
    const Pack<V> xt = ld_pack<V>(x + xi);
    const Pack<V> z = noise ? ld_pack<V>(noise + li) : philox_normal_pack<V>(slice_ids ? slice_ids[b] * n + p : li, seed, step);
    Pack<V> var = {};
    if (sc.learned_range && (sc.mode == DSD_MODE_A_DDPM || sc.mode == DSD_MODE_B_DDPM)) var = ld_pack<V>(mo_c + oi + n);
    Pack<V> res, x0;
#pragma unroll
    for (int j = 0; j < V; ++j) res.v[j] = sampler_update_value(sc, out.v[j], xt.v[j], z.v[j], var.v[j], x0.v[j]);
    st_pack<V>(x + xi, res);
    if (mo_u) st_pack<V>(x + xi + (int64_t)B * x_bs, res);
    if (x0_out) st_pack<V>(x0_out + li, x0);
}

void sampler_update(const StepCoef& sc, const float* out_u, const float* out_c, float scale, float* x, const float* noise,
                    uint64_t seed, uint64_t step, int B, int HW, hipStream_t s, float* x0_out, const int64_t* slice_ids, int Cz,
                    int64_t x_bs, int64_t o_bs) {
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    if (x_bs <= 0) x_bs = n;
    if (o_bs <= 0) o_bs = (sc.learned_range ? 2 : 1) * n;
    DSD_CHECK(o_bs >= (sc.learned_range ? 2 : 1) * n, "sampler update: output rows of %lld elements, the update reads %lld",
              (long long)o_bs, (long long)((sc.learned_range ? 2 : 1) * n));
    const bool v4 = can_vec4(n, x_bs, out_u, out_c, x, noise, x0_out) && o_bs % 4 == 0;
    launch_vec(v4, [&](auto V) {
        hipLaunchKernelGGL(sampler_update_kernel<decltype(V)::value>, dim3((unsigned)((B * (n / decltype(V)::value) + 255) / 256)),
                           dim3(256), 0, s, sc, out_u, out_c, scale, x, noise, seed, step, B, n, x_bs, o_bs, x0_out, slice_ids);
    });
    check_launch("sampler_update");
}

// ------------------------------------------------------------------------------------------------------------------
// DPM-Solver(++) multistep (Disc_diff/guided_diffusion/sampler.py; twin ldm/models/diffusion/dpm_solver_new/
// dpm_solver_pytorch.py).  Per network evaluation k:
//   dpm_model   m_k = data prediction x0 (dpmsolver++, sampler.py:396-405) or noise prediction (:390-394) from the
//               network output, for model types noise / x_start / v (model_wrapper :247-265)
//   dpm_quantile  s_b = max(quantile_0.995(|x0_b|), max_val) per sample (dynamic thresholding :379-388, torch.quantile
//               'linear': sorted[floor(r)] lerp sorted[ceil(r)], r = q*(n-1) in fp32) by an exact 4-pass radix select
//   dpm_update  m_k <- clamp(m_k,-s,s)/s ; x <- first-order (:509-553) or second-order multistep update (:760-816)
// Every product/sum is a separately rounded fp32 op in the reference's order (file-wide contract(off)).
// HW = elements per sample (Cz*h*w for a latent state); x row b at x + b*x_bs (x_bs = HW, or (Cz+Cc)*h*w inside the
// denoiser's input buffer); m and the model output are contiguous.  Guided (mo_u != nullptr): the 2B-row state and the two
// output halves of sampler_update_kernel; m and the thresholding quantile stay per logical sample.
// noise prediction from the network output (model_wrapper.noise_pred_fn :247-265)
__device__ __forceinline__ float dpm_noise_pred(const DpmCoef& c, float out, float xt) {
    if (c.pred == DSD_PRED_EPS) return out;
    if (c.pred == DSD_PRED_X0) return (xt - c.alpha * out) / c.sigma;
    return c.alpha * out + c.sigma * xt;
}
// first-order (:509-553) / second-order multistep (:760-816) update from m = m_k, m1 = m_{k-1}
__device__ __forceinline__ float dpm_update_value(const DpmCoef& c, float m, float m1, float xt) {
    if (c.order == 0) return m;                               // denoise_to_zero_fn :503-507
    float res = c.cx * xt - c.cm * m;
    if (c.order == 2) res = res - c.cd * (c.ir0 * (m - m1));
    return res;
}

// guided: each half becomes a noise prediction from its own output and the shared x_t, then
// noise = noise_u + gs * (noise_c - noise_u) (dpm_solver_pytorch.py:324-332)
template <int V>
__global__ __launch_bounds__(256) void dpm_model_kernel(DpmCoef c, const float* __restrict__ mo_u, const float* __restrict__ mo_c,
                                                        int Cm, float gs, const float* __restrict__ x, float* __restrict__ m,
                                                        int B, int HW, int64_t x_bs) {
    const int64_t nv = HW / V, total = (int64_t)B * nv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / nv;
        const int64_t p = (i - b * nv) * V;
        const int64_t oi = (b * Cm) * HW + p;                 // a learned-sigma model: first channel only (gaussian_diffusion.py:484-485)
        const Pack<V> oc = ld_pack<V>(mo_c + oi), xt = ld_pack<V>(x + b * x_bs + p);
        Pack<V> ou = oc;
        if (mo_u) ou = ld_pack<V>(mo_u + oi);
        Pack<V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float eps = dpm_noise_pred(c, oc.v[j], xt.v[j]);
            if (mo_u) {
                const float eu = dpm_noise_pred(c, ou.v[j], xt.v[j]);
                eps = eu + gs * (eps - eu);
            }
            r.v[j] = c.data_pred ? (xt.v[j] - c.sigma * eps) / c.alpha : eps;
        }
        st_pack<V>(m + b * HW + p, r);
    }
}

// One block per sample.  |v| bit patterns of non-negative floats order like unsigned integers, so the element of rank k
// is found digit by digit (8 bits per pass) with an LDS histogram; the rank k+1 element is either the same value or the
// smallest value above it.
__global__ __launch_bounds__(1024) void dpm_quantile_kernel(const float* __restrict__ m, int n, float ratio, float max_val,
                                                            float* __restrict__ s_out) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh_prefix, sh_k, sh_cnt, sh_min;
    const float* v = m + (int64_t)blockIdx.x * n;
    const float rank = ratio * (float)(n - 1);
    const float fl = floorf(rank);
    const uint32_t k_below = (uint32_t)fl;
    const bool need_above = ceilf(rank) != fl;
    const float w = rank - fl;
    if (threadIdx.x == 0) { sh_prefix = 0; sh_k = k_below; sh_min = 0xFFFFFFFFu; }
    uint32_t mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t prefix = sh_prefix;
        for (int i = threadIdx.x; i < n; i += 1024) {
            const uint32_t u = __float_as_uint(v[i]) & 0x7FFFFFFFu;
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t k = sh_k, d = 0;
            while (d < 255 && k >= hist[d]) { k -= hist[d]; ++d; }
            sh_k = k;
            sh_cnt = hist[d];
            sh_prefix = prefix | (d << shift);
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const uint32_t ubelow = sh_prefix;
    uint32_t uabove = ubelow;
    if (need_above && sh_k + 1 >= sh_cnt) {      // rank k+1 lies beyond the run of equal values
        uint32_t loc = 0xFFFFFFFFu;
        for (int i = threadIdx.x; i < n; i += 1024) {
            const uint32_t u = __float_as_uint(v[i]) & 0x7FFFFFFFu;
            if (u > ubelow && u < loc) loc = u;
        }
        atomicMin(&sh_min, loc);
        __syncthreads();
        uabove = sh_min;
    }
    if (threadIdx.x == 0) {
        const float a = __uint_as_float(ubelow), b = __uint_as_float(uabove);
        // at::lerp (ATen/native/Lerp.h, vectorised CPU form): fma(w<0.5 ? w : w-1, b-a, w<0.5 ? a : b)
        const float diff = b - a;
        const float q = (fabsf(w) < 0.5f) ? fmaf(w, diff, a) : fmaf(w - 1.0f, diff, b);
        s_out[blockIdx.x] = fmaxf(q, max_val);
    }
}

// thresholds m_k in place, then writes x_{t-1} to row b and, with dup (the guided 2B-row state), to row B+b
template <int V>
__global__ __launch_bounds__(256) void dpm_update_kernel(DpmCoef c, float* __restrict__ m0, const float* __restrict__ m1,
                                                         const float* __restrict__ s_thr, float* __restrict__ x, int B, int HW,
                                                         int64_t x_bs, int dup) {
    const int64_t nv = HW / V, total = (int64_t)B * nv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / nv;
        const int64_t p = (i - b * nv) * V;
        const int64_t li = b * HW + p, xi = b * x_bs + p;
        Pack<V> m = ld_pack<V>(m0 + li);
        if (s_thr) {
            const float s = s_thr[b];
#pragma unroll
            for (int j = 0; j < V; ++j) m.v[j] = fminf(fmaxf(m.v[j], -s), s) / s;
            st_pack<V>(m0 + li, m);
        }
        if (!x) continue;                                     // thresholding only (dsd_op_dpm_threshold)
        const Pack<V> xt = ld_pack<V>(x + xi);
        Pack<V> mp = m;
        if (c.order == 2) mp = ld_pack<V>(m1 + li);
        Pack<V> res;
#pragma unroll
        for (int j = 0; j < V; ++j) res.v[j] = dpm_update_value(c, m.v[j], mp.v[j], xt.v[j]);
        st_pack<V>(x + xi, res);
        if (dup) st_pack<V>(x + xi + (int64_t)B * x_bs, res);
    }
}

static void dpm_update(bool v4, const DpmCoef& c, float* m0, const float* m1, const float* s_thr, float* x, int B, int HW,
                       int64_t x_bs, bool dup, hipStream_t s) {
    launch_vec(v4, [&](auto V) {
        hipLaunchKernelGGL(dpm_update_kernel<decltype(V)::value>, dim3(ew_blocks((int64_t)B * (HW / decltype(V)::value))), dim3(256),
                           0, s, c, m0, m1, s_thr, x, B, HW, x_bs, dup ? 1 : 0);
    });
    check_launch("dpm_update");
}

// The front half of every DPM evaluation: the model value of the network output into m, and with thresholding on a data
// prediction the per-sample scale into s_buf.  Returns the scales the update kernel applies, or null.
static const float* dpm_model_value(bool v4, const DpmCoef& c, const float* out_u, const float* out_c, int Cm, float scale,
                                    const float* x, float* m, float* s_buf, float ratio, float max_val, int B, int HW, int64_t x_bs,
                                    hipStream_t s) {
    launch_vec(v4, [&](auto V) {
        hipLaunchKernelGGL(dpm_model_kernel<decltype(V)::value>, dim3(ew_blocks((int64_t)B * (HW / decltype(V)::value))), dim3(256),
                           0, s, c, out_u, out_c, Cm, scale, x, m, B, HW, x_bs);
    });
    check_launch("dpm_model");
    if (!(c.thresh && c.data_pred)) return nullptr;
    hipLaunchKernelGGL(dpm_quantile_kernel, dim3(B), dim3(1024), 0, s, m, HW, ratio, max_val, s_buf);   // per logical sample: m is [B,HW]
    check_launch("dpm_quantile");
    return s_buf;
}

void dpm_step(const DpmCoef& c, const float* out_u, const float* out_c, int Cm, float scale, float* x, float* m_cur,
              const float* m_prev, float* s_buf, float ratio, float max_val, int B, int HW, hipStream_t s, int64_t x_bs) {
    if (!B || !HW) return;
    if (x_bs <= 0) x_bs = HW;
    const bool v4 = can_vec4(HW, x_bs, out_u, out_c, x, m_cur, m_prev);
    const float* thr = dpm_model_value(v4, c, out_u, out_c, Cm, scale, x, m_cur, s_buf, ratio, max_val, B, HW, x_bs, s);
    dpm_update(v4, c, m_cur, m_prev, thr, x, B, HW, x_bs, out_u != nullptr, s);
}

void dpm_threshold(const float* x0, float* y, float* s_buf, float ratio, float max_val, int B, int n, hipStream_t s) {
    if (!B || !n) return;
    DSD_HIP(hipMemcpyAsync(y, x0, (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(dpm_quantile_kernel, dim3(B), dim3(1024), 0, s, y, n, ratio, max_val, s_buf);
    check_launch("dpm_quantile");
    DpmCoef c{};
    c.order = 0;
    dpm_update(can_vec4(n, n, y), c, y, nullptr, s_buf, nullptr, B, n, n, false, s);
    DSD_HIP(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------------------------------------------
// The DPM-Solver family as a program of evaluations (include/dsdiff.h dsd_dpm_program): multistep up to third order
// (multistep_dpm_solver_third_update, sampler.py:818-868) and the singlestep solvers of second (:555-635) and third order
// (:637-758).  Every evaluation forms its model value with dpm_model_kernel / dpm_quantile_kernel above — from the alpha and
// sigma of ITS time and the state the network just read, stage states included — and dpm_eval_kernel thresholds it in its
// history plane and writes the next state.  The history is three planes [B,HW] addressed by slot (nothing is copied or rotated:
// the program names the plane an evaluation writes and the ones it reads).  A singlestep stage reads the BASE state x_s: the
// first stage (SS_S1) copies it from the state into the base plane before it overwrites the state with x_s1, the later ones read
// it there.  c[] holds host scalars only (the reference's fp32 torch expressions on its (1,)-tensors); a sign the reference
// writes as "+ c*D" against "- c*D" between the two algorithm types is folded into c (a - (-c)*D == a + c*D bit for bit).
//   MS0              x = ma                                                       denoise_to_zero_fn :503-507
//   MS1, SS_S1       x = c0*xb - c1*ma                                            :509-553 / x_s1
//   MS2              x = (c0*xb - c1*ma) - c2*(c3*(ma - mb))                      :760-816
//   MS3              D1_0 = c4*(ma - mb); D1_1 = c5*(mb - mc); D1 = D1_0 + c6*(D1_0 - D1_1); D2 = c7*(D1_0 - D1_1)
//                    x = ((c0*xb - c1*ma) + c2*D1) - c3*D2                        :840-867
//   SS_S2/T2/T3      x = (c0*xb - c1*ma) - c2*(mb - ma)                           x_s2, x_t of 'dpmsolver' (:592-631, :692-742)
//   SS_T3_TAYLOR     D1_0 = c4*(mb - ma); D1_1 = c5*(mc - ma); D1 = (c7*D1_0 - c6*D1_1)/c8; D2 = 2*(D1_1 - D1_0)/c8
//                    x = ((c0*xb - c1*ma) + c2*D1) - c3*D2                        :705-714, :744-753 (two IEEE divisions)
static_assert(sizeof(DpmEval::c) == DSD_DPM_NCOEF * sizeof(float), "DpmEval::c is one dsd_dpm_program coefficient row");
__device__ __forceinline__ float dpm_eval_value(const DpmEval& e, float xb, float ma, float mb, float mc) {
    const float* c = e.c;
    if (e.kind == DSD_DPM_MS0) return ma;
    const float lin = c[0] * xb - c[1] * ma;
    switch (e.kind) {
        case DSD_DPM_MS2: return lin - c[2] * (c[3] * (ma - mb));
        case DSD_DPM_MS3: {
            const float d10 = c[4] * (ma - mb), d11 = c[5] * (mb - mc);
            const float dd = d10 - d11;
            const float d1 = d10 + c[6] * dd, d2 = c[7] * dd;
            return (lin + c[2] * d1) - c[3] * d2;
        }
        case DSD_DPM_SS_S2:
        case DSD_DPM_SS_T2:
        case DSD_DPM_SS_T3: return lin - c[2] * (mb - ma);
        case DSD_DPM_SS_T3_TAYLOR: {
            const float d10 = c[4] * (mb - ma), d11 = c[5] * (mc - ma);
            const float d1 = (c[7] * d10 - c[6] * d11) / c[8];
            const float d2 = 2.f * (d11 - d10) / c[8];
            return (lin + c[2] * d1) - c[3] * d2;
        }
        default: return lin;                                  // MS1, SS_S1
    }
}

// mw (the plane this evaluation's model value was written to) may be one of ma / mb / mc: the planes are not __restrict__, and
// a thread reads its own elements of mw back only through the registers it thresholded.
template <int V>
__global__ __launch_bounds__(256) void dpm_eval_kernel(DpmEval e, int B, int HW) {
    const int64_t nv = HW / V, total = (int64_t)B * nv;
    const bool from_base = e.kind >= DSD_DPM_SS_S2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / nv;
        const int64_t p = (i - b * nv) * V;
        const int64_t li = b * HW + p, xi = b * e.x_bs + p;
        Pack<V> mw = ld_pack<V>(e.mw + li);
        if (e.s_thr) {
            const float s = e.s_thr[b];
#pragma unroll
            for (int j = 0; j < V; ++j) mw.v[j] = fminf(fmaxf(mw.v[j], -s), s) / s;
            st_pack<V>(e.mw + li, mw);
        }
        const Pack<V> ma = e.ma == e.mw ? mw : ld_pack<V>(e.ma + li);
        Pack<V> mb = ma, mc = ma;
        if (e.mb) mb = e.mb == e.mw ? mw : ld_pack<V>(e.mb + li);
        if (e.mc) mc = e.mc == e.mw ? mw : ld_pack<V>(e.mc + li);
        const Pack<V> xb = from_base ? ld_pack<V>(e.base + li) : ld_pack<V>(e.x + xi);
        if (e.kind == DSD_DPM_SS_S1) st_pack<V>(e.base + li, xb);
        Pack<V> res;
#pragma unroll
        for (int j = 0; j < V; ++j) res.v[j] = dpm_eval_value(e, xb.v[j], ma.v[j], mb.v[j], mc.v[j]);
        st_pack<V>(e.x + xi, res);
        if (e.dup) st_pack<V>(e.x + xi + (int64_t)B * e.x_bs, res);
    }
}

void dpm_eval(const DpmCoef& c, const DpmEval& ev, const float* out_u, const float* out_c, int Cm, float scale, float* s_buf,
              float ratio, float max_val, int B, int HW, hipStream_t s) {
    if (!B || !HW) return;
    DpmEval e = ev;
    if (e.x_bs <= 0) e.x_bs = HW;
    const bool v4 = can_vec4(HW, e.x_bs, out_u, out_c, e.x, e.mw, e.ma, e.mb, e.mc, e.base);
    e.s_thr = dpm_model_value(v4, c, out_u, out_c, Cm, scale, e.x, e.mw, s_buf, ratio, max_val, B, HW, e.x_bs, s);
    e.dup = out_u != nullptr;
    launch_vec(v4, [&](auto V) {
        hipLaunchKernelGGL(dpm_eval_kernel<decltype(V)::value>, dim3(ew_blocks((int64_t)B * (HW / decltype(V)::value))), dim3(256), 0,
                           s, e, B, HW);
    });
    check_launch("dpm_eval");
}

// ------------------------------------------------------------------------------------------------------------------
// Image-to-image: q_sample / mask blend (ddim.py:160-163, ddpm.py:356-359,1085-1087) and the DDIM inversion step (ddim.py:282-295).
// Logical sample b: x0 and noise rows are contiguous [B,n] (n = Cz*HW), the state row sits at x + b*x_bs, and with `dup` (a guided
// loop's 2B-row state) the result also goes to row B+b.
//   img_orig = a*x0 + s*z                       a, s: the iteration's scalars, or per row from a_row / s_row (q_sample, t is [B])
//   x        = img_orig*mask + (1 - mask)*x     mask [B,mc,HW], mc = 1 (broadcast over the channels) or Cz; mask == nullptr: x = img_orig
// z is fed, or normal slice*n + p of the Philox stream (seed, step + 2^32): the update of iteration `step` draws from (seed, step),
// so the two never share a counter block.  V = 4 needs n % 4 == 0 and, for a one-channel mask, HW % 4 == 0 (a pack stays inside
// one channel); the launcher checks.

// Grid: x over the packs of one sample (capped, strided), y = the sample — the row's coefficients and its slice id are
// block-uniform and no 64-bit division is left.  BLEND selects the mask blend (scalar a, s) or the plain q_sample (a_row, s_row,
// or without them the scalars: one timestep for the whole batch): one kernel with every argument live spilled scalar registers.
template <int V, bool BLEND>
__global__ __launch_bounds__(256) void q_sample_blend_kernel(float a, float s, const float* __restrict__ a_row,
                                                             const float* __restrict__ s_row, const float* __restrict__ x0,
                                                             const float* __restrict__ mask, int mc, float* __restrict__ x,
                                                             const float* __restrict__ noise, uint64_t seed, uint64_t step, int B,
                                                             int n, int hw, int64_t x_bs, int dup,
                                                             const int64_t* __restrict__ slice_ids) {
    const int b = blockIdx.y;
    const float ca = (BLEND || !a_row) ? a : a_row[b], cs = (BLEND || !s_row) ? s : s_row[b];
    const int64_t row = (int64_t)b * n;                                       // in the [B,n] tensors
    const int64_t ctr = slice_ids ? slice_ids[b] * n : row;                   // Philox counter of the row's first element
    float* xr = x + (int64_t)b * x_bs;
    for (int p = (blockIdx.x * 256 + threadIdx.x) * V; p < n; p += gridDim.x * 256 * V) {
        const Pack<V> xs = ld_pack<V>(x0 + row + p);
        const Pack<V> z = noise ? ld_pack<V>(noise + row + p) : philox_normal_pack<V>(ctr + p, seed, step + kBlendStream);
        Pack<V> res;
#pragma unroll
        for (int j = 0; j < V; ++j) res.v[j] = ca * xs.v[j] + cs * z.v[j];            // q_sample ddpm.py:358-359
        if constexpr (BLEND) {
            const Pack<V> m = ld_pack<V>(mask + (mc == 1 ? (int64_t)b * hw + p % hw : row + p));
            const Pack<V> xt = ld_pack<V>(xr + p);
#pragma unroll
            for (int j = 0; j < V; ++j) res.v[j] = res.v[j] * m.v[j] + (1.f - m.v[j]) * xt.v[j];   // ddim.py:163
        }
        st_pack<V>(xr + p, res);
        if (BLEND && dup) st_pack<V>(xr + p + (int64_t)B * x_bs, res);
    }
}

void q_sample_blend(float a, float s, const float* a_row, const float* s_row, const float* x0, const float* mask, int mask_ch,
                    float* x, const float* noise, uint64_t seed, uint64_t step, int B, int Cz, int HW, hipStream_t st, int64_t x_bs,
                    bool dup, const int64_t* slice_ids) {
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    DSD_CHECK(n <= (int64_t)1 << 30, "q_sample / mask blend: one sample has %lld elements; up to 2^30 are taken", (long long)n);
    if (x_bs <= 0) x_bs = n;
    const bool v4 = can_vec4(n, x_bs, x0, mask, x, noise) && (!mask || mask_ch != 1 || HW % 4 == 0);
    DSD_CHECK(B <= 65535, "q_sample / mask blend: %d samples; up to 65535 are taken", B);
    const dim3 grid((unsigned)std::min<int64_t>((n / (v4 ? 4 : 1) + 255) / 256, 2048), (unsigned)B);
    launch_vec(v4, [&](auto V) {
        auto kern = mask ? q_sample_blend_kernel<decltype(V)::value, true> : q_sample_blend_kernel<decltype(V)::value, false>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a, s, a_row, s_row, x0, mask, mask_ch, x, noise, seed, step, B, (int)n, HW,
                           x_bs, dup ? 1 : 0, slice_ids);
    });
    check_launch("q_sample_blend");
}

// DDIM inversion (ddim.py:292-295): x_next = cx*x + ce*e as xt_weighted + weighted_noise_pred, e the raw network output or,
// guided (mo_u != nullptr), e_u + gs*(e_c - e_u) from the two output halves (:287-290); x_next goes to rows b and, guided, B+b.
template <int V>
__global__ __launch_bounds__(256) void ddim_invert_kernel(float cx, float ce, const float* __restrict__ mo_u,
                                                          const float* __restrict__ mo_c, float gs, float* __restrict__ x, int B,
                                                          int64_t n, int64_t x_bs, int64_t o_bs) {
    const int64_t nv = n / V, total = (int64_t)B * nv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / nv;
        const int64_t p = (i - b * nv) * V;
        const int64_t oi = b * o_bs + p, xi = b * x_bs + p;      // output rows of o_bs: the prediction is their first n elements
        Pack<V> e = ld_pack<V>(mo_c + oi);
        const Pack<V> xt = ld_pack<V>(x + xi);
        if (mo_u) {
            const Pack<V> eu = ld_pack<V>(mo_u + oi);
#pragma unroll
            for (int j = 0; j < V; ++j) e.v[j] = eu.v[j] + gs * (e.v[j] - eu.v[j]);
        }
        Pack<V> res;
#pragma unroll
        for (int j = 0; j < V; ++j) res.v[j] = cx * xt.v[j] + ce * e.v[j];
        st_pack<V>(x + xi, res);
        if (mo_u) st_pack<V>(x + xi + (int64_t)B * x_bs, res);
    }
}

void ddim_invert_step(float cx, float ce, const float* out_u, const float* out_c, float scale, float* x, int B, int Cz, int HW,
                      hipStream_t st, int64_t x_bs, int64_t o_bs) {
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    if (x_bs <= 0) x_bs = n;
    if (o_bs <= 0) o_bs = n;
    launch_vec(can_vec4(n, x_bs, out_u, out_c, x) && o_bs % 4 == 0, [&](auto V) {
        hipLaunchKernelGGL(ddim_invert_kernel<decltype(V)::value>, dim3(ew_blocks(B * (n / decltype(V)::value))), dim3(256), 0, st, cx,
                           ce, out_u, out_c, scale, x, B, n, x_bs, o_bs);
    });
    check_launch("ddim_invert");
}

// ------------------------------------------------------------------------------------------------------------------
// PLMS (ldm/models/diffusion/plms.py:206-243; PlmsStep in kernels.h).  Grid as the blend's: x over the packs of one sample, y =
// the sample, so the threshold's scale is block-uniform.  The history planes and x_saved are contiguous [B,n]; row b of the two
// output halves sits at out + b*o_bs (o_bs = n, or 2n for a model with a variance half, which PLMS leaves unread); the state row
// b sits at x + b*x_bs and, guided, the result also goes to row B+b.
// plms_form: e_t, e' and the pred_x0 before thresholding of one pack — the one place both kernels take them from, so the norm
// kernel sums exactly the values the update kernel scales.  The combinations are the reference's expressions, left to right,
// every product and sum rounded on its own (file-wide contract(off)), the divisors literals with an IEEE division.
template <int V>
__device__ __forceinline__ void plms_form(const PlmsStep& a, int b, int p, int n, Pack<V>& et, Pack<V>& ep, Pack<V>& xt,
                                          Pack<V>& x0) {
    const int64_t li = (int64_t)b * n + p, oi = b * a.o_bs + p;               // output rows of o_bs, the prediction first
    Pack<V> e = ld_pack<V>(a.out_c + oi);
    if (a.out_u) {                                                            // plms.py:189-193
        const Pack<V> eu = ld_pack<V>(a.out_u + oi);
#pragma unroll
        for (int j = 0; j < V; ++j) e.v[j] = eu.v[j] + a.scale * (e.v[j] - eu.v[j]);
    }
    if (a.order == DSD_PLMS_CORRECT) {                                        // :231-232, e = e_t_next
        et = ld_pack<V>(a.h_new + li);
        xt = ld_pack<V>(a.x_saved + li);
#pragma unroll
        for (int j = 0; j < V; ++j) ep.v[j] = (et.v[j] + e.v[j]) / 2.f;
    } else {
        et = e;
        xt = ld_pack<V>(a.x + (int64_t)b * a.x_bs + p);
        if (a.order == DSD_PLMS_PREDICT) {                                    // :230
            ep = e;
        } else if (a.order == DSD_PLMS_AB2) {                                 // :235
            const Pack<V> o1 = ld_pack<V>(a.o1 + li);
#pragma unroll
            for (int j = 0; j < V; ++j) ep.v[j] = (3.f * et.v[j] - o1.v[j]) / 2.f;
        } else if (a.order == DSD_PLMS_AB3) {                                 // :238
            const Pack<V> o1 = ld_pack<V>(a.o1 + li), o2 = ld_pack<V>(a.o2 + li);
#pragma unroll
            for (int j = 0; j < V; ++j) ep.v[j] = (23.f * et.v[j] - 16.f * o1.v[j] + 5.f * o2.v[j]) / 12.f;
        } else {                                                              // :241, o3 in the plane this step retires
            const Pack<V> o1 = ld_pack<V>(a.o1 + li), o2 = ld_pack<V>(a.o2 + li), o3 = ld_pack<V>(a.h_new + li);
#pragma unroll
            for (int j = 0; j < V; ++j)
                ep.v[j] = (55.f * et.v[j] - 59.f * o1.v[j] + 37.f * o2.v[j] - 9.f * o3.v[j]) / 24.f;
        }
    }
    const float sa = sqrtf(a.a_t);
#pragma unroll
    for (int j = 0; j < V; ++j) x0.v[j] = (xt.v[j] - a.s1m * ep.v[j]) / sa;    // :214
}

// Per-sample sum of pred_x0^2 for norm_thresholding (sampling_util.py:14-16), read-only, launched in front of the update.
// Deterministic: every thread sums its strided packs in fp64, the block folds its 256 sums in a fixed tree, and block j of
// sample b writes part[b*gridDim.x + j]; the update kernel adds the partials in index order.  No atomics.
static constexpr int kPlmsNormBlocks = 32;
template <int V>
__global__ __launch_bounds__(256) void plms_x0_norm_kernel(PlmsStep a, int n) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    double acc = 0.0;
    for (int p = (blockIdx.x * 256 + threadIdx.x) * V; p < n; p += gridDim.x * 256 * V) {
        Pack<V> et, ep, xt, x0;
        plms_form<V>(a, b, p, n, et, ep, xt, x0);
#pragma unroll
        for (int j = 0; j < V; ++j) acc += (double)x0.v[j] * (double)x0.v[j];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.part[(int64_t)b * gridDim.x + blockIdx.x] = red[0];
}

template <int V>
__global__ __launch_bounds__(256) void plms_update_kernel(PlmsStep a, int B, int n, int nblk) {
    const int b = blockIdx.y;
    float thr_scale = 1.f;
    if (a.thr > 0.f) {                                                        // value / max(sqrt(mean(x0^2)), value)
        double sum = 0.0;
        for (int j = 0; j < nblk; ++j) sum += a.part[(int64_t)b * nblk + j];
        thr_scale = a.thr / fmaxf(sqrtf((float)(sum / (double)n)), a.thr);
    }
    const float sp = sqrtf(a.a_prev), sd = sqrtf(1.f - a.a_prev - a.sigma * a.sigma);   // :220,224; sigma = 0: no noise term
    float* xr = a.x + (int64_t)b * a.x_bs;
    for (int p = (blockIdx.x * 256 + threadIdx.x) * V; p < n; p += gridDim.x * 256 * V) {
        const int64_t li = (int64_t)b * n + p;
        Pack<V> et, ep, xt, x0, res;
        plms_form<V>(a, b, p, n, et, ep, xt, x0);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (a.thr > 0.f) x0.v[j] = x0.v[j] * thr_scale;
            res.v[j] = sp * x0.v[j] + sd * ep.v[j];
        }
        if (a.order != DSD_PLMS_CORRECT) st_pack<V>(a.h_new + li, et);        // the history takes the raw (guided) e_t (:165-166)
        if (a.order == DSD_PLMS_PREDICT) st_pack<V>(a.x_saved + li, xt);
        st_pack<V>(xr + p, res);
        if (a.out_u) st_pack<V>(xr + p + (int64_t)B * a.x_bs, res);
        if (a.x0_out) st_pack<V>(a.x0_out + li, x0);
    }
}

size_t plms_norm_doubles(int B, int64_t) { return (size_t)B * kPlmsNormBlocks; }

void plms_step(const PlmsStep& step, int B, int Cz, int HW, hipStream_t s) {
    PlmsStep a = step;
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    DSD_CHECK(n <= (int64_t)1 << 30, "PLMS update: one sample has %lld elements; up to 2^30 are taken", (long long)n);
    DSD_CHECK(B <= 65535, "PLMS update: %d samples; up to 65535 are taken", B);
    if (a.x_bs <= 0) a.x_bs = n;
    if (a.o_bs <= 0) a.o_bs = n;
    const bool v4 = can_vec4(n, a.x_bs, a.out_u, a.out_c, a.h_new, a.o1, a.o2, a.x_saved, a.x) && a.o_bs % 4 == 0;
    // x0_out does not choose the pack width: the threshold's partial sums follow it, and an update with the output must give the
    // bits of the update without
    DSD_CHECK(!v4 || ((uintptr_t)a.x0_out & 15u) == 0, "PLMS update: the pred_x0 output %p must be 16-byte aligned (samples of %lld floats)",
              (const void*)a.x0_out, (long long)n);
    const int64_t blocks = (n / (v4 ? 4 : 1) + 255) / 256;
    const int nblk = (int)std::min<int64_t>(blocks, kPlmsNormBlocks);
    if (a.thr > 0.f) {
        DSD_CHECK(a.part, "PLMS update: the threshold needs its scratch");
        launch_vec(v4, [&](auto V) {
            hipLaunchKernelGGL(plms_x0_norm_kernel<decltype(V)::value>, dim3(nblk, B), dim3(256), 0, s, a, (int)n);
        });
        check_launch("plms_x0_norm");
    }
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 2048), (unsigned)B);
    launch_vec(v4, [&](auto V) { hipLaunchKernelGGL(plms_update_kernel<decltype(V)::value>, grid, dim3(256), 0, s, a, B, (int)n, nblk); });
    check_launch("plms_update");
}

// ------------------------------------------------------------------------------------------------------------------
// Variational bound (gaussian_diffusion.py:788-819, 922-991; losses.py).  One read-only pass after the network evaluation of
// iteration k forms, per element and in the reference's fp32 operation order, the KL of the true posterior against the model's
// (DECODER, t == 0: the negated discretised log-likelihood), (pred_xstart - x_start)^2 and (eps - noise)^2, and sums the three
// per sample as plms_x0_norm_kernel sums its norm: every thread in fp64, the block in a fixed LDS tree, block j of sample b into
// part[(b*gridDim.x + j)*3 + q]; vlb_finalize_kernel adds the partials in a fixed order.  No atomics: two runs are bit-identical.
// Grid: x over the 1024-element pieces of one sample, y = the sample.  A thread owns four consecutive elements and there is NO
// grid-stride loop: out of a loop the compiler hoists the constants of the inlined logf / sinf / cosf / expf / tanhf into scalar
// registers and spilled them (12-38 per instantiation), as it did in sampler_update_kernel.  V only selects how the four are
// loaded and stored (one 16-byte access, or guarded scalar ones), so both forms add the same values in the same order.
template <int V, bool DECODER>
__global__ __launch_bounds__(256) void vlb_terms_kernel(VlbStep a, int n) {
    __shared__ double red[3 * 256];
    const int b = blockIdx.y;
    double acc[3] = {0.0, 0.0, 0.0};
    vlb_thread_terms<V, DECODER>(a, a.sc, a.post_log_var, b, n, (blockIdx.x * 256 + threadIdx.x) * 4, acc);
    vlb_block_fold<3>(acc, red, a.part + ((int64_t)b * gridDim.x + blockIdx.x) * 3);
}

// _prior_bpd's kl_prior (:932-935): normal_kl(c0*x_start, log(1 - acp[T-1]), 0.0, 0.0) per element
template <int V>
__global__ __launch_bounds__(256) void prior_kl_kernel(float c0, float logvar, const float* __restrict__ x_start, int n,
                                                       double* __restrict__ part) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int valid = n - p;
    double acc[1] = {0.0};
    if (valid > 0) {
        const Pack<4> xs = ld_quad<V>(x_start + (int64_t)b * n + p, valid);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float kl = normal_kl_value(c0 * xs.v[j], logvar, 0.0f, 0.0f);
            if (j < valid) acc[0] += (double)kl;
        }
    }
    vlb_block_fold<1>(acc, red, part + (int64_t)b * gridDim.x + blockIdx.x);
}

// One wave per sample: lane l adds the partials l, l+64, ... in index order, the 64 lane sums fold in a fixed tree; mean_flat
// in fp64 rounded to fp32 once, then (quantity 0) the reference's fp32 division by np.log(2.0).  Quantity q of sample b goes to
// out[q][b*stride].
__global__ __launch_bounds__(64) void vlb_finalize_kernel(const double* __restrict__ part, int nblk, int nq, int n, float* o0,
                                                          float* o1, float* o2, int64_t stride, int bits) {
    __shared__ double red[3 * 64];
    const int b = blockIdx.x;
    rows_fold_partials(part, b, nblk, nq, red);
    if (threadIdx.x == 0) {
        float* outs[3] = {o0, o1, o2};
        for (int q = 0; q < nq; ++q) {
            if (!outs[q]) continue;
            outs[q][(int64_t)b * stride] = rows_mean_value(red[q * 64], n, bits && q == 0);
        }
    }
}

// bits: quantity 0 is a bound term (divided by ln 2); loss.hip's means pass 0
void rows_finalize(const double* part, int nblk, int nq, int n, float* o0, float* o1, float* o2, int64_t stride, int bits, int B,
                   hipStream_t s) {
    hipLaunchKernelGGL(vlb_finalize_kernel, dim3(B), dim3(64), 0, s, part, nblk, nq, n, o0, o1, o2, stride, bits);
    check_launch("vlb_finalize");
}

static int vlb_blocks(int64_t n) { return (int)((n + kVlbPiece - 1) / kVlbPiece); }
size_t vlb_part_doubles(int B, int64_t n) { return (size_t)B * vlb_blocks(n) * 3; }

void vlb_terms(const VlbStep& step, bool decoder, float* vb, float* xstart_mse, float* mse, int64_t term_stride, int B, int Cz, int HW,
               hipStream_t s) {
    VlbStep a = step;
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    DSD_CHECK(n <= (int64_t)1 << 30, "variational bound: one sample has %lld elements; up to 2^30 are taken", (long long)n);
    DSD_CHECK(B <= 65535, "variational bound: %d samples; up to 65535 are taken", B);
    DSD_CHECK(a.part, "variational bound: the reduction needs its scratch");
    const int64_t need = (a.sc.learned_range ? 2 : 1) * n;
    if (a.x_bs <= 0) a.x_bs = n;
    if (a.o_bs <= 0) a.o_bs = need;
    DSD_CHECK(a.o_bs >= need, "variational bound: output rows of %lld elements, the terms read %lld", (long long)a.o_bs, (long long)need);
    const bool v4 = can_vec4(n, a.x_bs, a.x_start, a.xt, a.out, a.noise, a.mean, a.log_variance, a.pred_xstart) && a.o_bs % 4 == 0;
    const int nblk = vlb_blocks(n);
    launch_vec(v4, [&](auto V) {
        auto kern = decoder ? vlb_terms_kernel<decltype(V)::value, true> : vlb_terms_kernel<decltype(V)::value, false>;
        hipLaunchKernelGGL(kern, dim3(nblk, B), dim3(256), 0, s, a, (int)n);
    });
    check_launch("vlb_terms");
    if (!vb && !xstart_mse && !mse) return;
    rows_finalize(a.part, nblk, 3, (int)n, vb, xstart_mse, mse, term_stride > 0 ? term_stride : (int64_t)1, 1, B, s);
}

void prior_bpd(float c0, float logvar, const float* x_start, double* part, float* prior, int B, int64_t n, hipStream_t s) {
    if (!B || !n) return;
    DSD_CHECK(n <= (int64_t)1 << 30, "prior bpd: one sample has %lld elements; up to 2^30 are taken", (long long)n);
    DSD_CHECK(B <= 65535, "prior bpd: %d samples; up to 65535 are taken", B);
    const int nblk = vlb_blocks(n);
    launch_vec(can_vec4(n, n, x_start), [&](auto V) {
        hipLaunchKernelGGL(prior_kl_kernel<decltype(V)::value>, dim3(nblk, B), dim3(256), 0, s, c0, logvar, x_start, (int)n, part);
    });
    check_launch("prior_kl");
    rows_finalize(part, nblk, 1, (int)n, prior, nullptr, nullptr, 1, 1, B, s);
}

// ddim_reverse_sample (gaussian_diffusion.py:691-701): eps re-derived from the clipped pred_xstart, x_{t+1} written in place
template <int V>
__global__ __launch_bounds__(256) void ddim_reverse_kernel(StepCoef sc, float abar_next, const float* __restrict__ mo,
                                                           float* __restrict__ x, float* __restrict__ x0_out, int B, int64_t n,
                                                           int64_t x_bs, int64_t o_bs) {
    const int64_t nv = n / V, total = (int64_t)B * nv;
    const float sa = sqrtf(abar_next), sb = sqrtf(1.f - abar_next);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / nv;
        const int64_t p = (i - b * nv) * V;
        const int64_t oi = b * o_bs + p, xi = b * x_bs + p;
        const Pack<V> out = ld_pack<V>(mo + oi), xt = ld_pack<V>(x + xi);
        Pack<V> res, x0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            x0.v[j] = pred_xstart_value(sc, out.v[j], xt.v[j]);
            const float eps = (sc.c[2] * xt.v[j] - x0.v[j]) / sc.c[3];
            res.v[j] = x0.v[j] * sa + sb * eps;
        }
        st_pack<V>(x + xi, res);
        if (x0_out) st_pack<V>(x0_out + b * n + p, x0);
    }
}

void ddim_reverse_step(const StepCoef& sc, float abar_next, const float* out, float* x, float* x0_out, int B, int Cz, int HW,
                       hipStream_t st, int64_t x_bs, int64_t o_bs) {
    const int64_t n = (int64_t)Cz * HW;
    if (!B || !n) return;
    if (x_bs <= 0) x_bs = n;
    if (o_bs <= 0) o_bs = n;
    launch_vec(can_vec4(n, x_bs, out, x, x0_out) && o_bs % 4 == 0, [&](auto V) {
        hipLaunchKernelGGL(ddim_reverse_kernel<decltype(V)::value>, dim3(ew_blocks(B * (n / decltype(V)::value))), dim3(256), 0, st, sc,
                           abar_next, out, x, x0_out, B, n, x_bs, o_bs);
    });
    check_launch("ddim_reverse");
}

// ------------------------------------------------------------------------------------------------------------------
// Adaptive DPM-Solver (dpm_solver_adaptive, sampler.py:921-980): the error estimate of one trial (DpmAdaptiveErr in kernels.h).
// One pass over the sample recomputes the lower-order result from the planes the singlestep step left — dpm_eval_value with
// kind MS1 (c0*base - c1*ma, dpm_solver_first_update) or SS_T2 ((c0*base - c1*ma) - c2*(mb - ma), the second-order singlestep
// update on the model_s1 the third-order step evaluated) — writes it out, and sums ((x_higher - x_lower)/delta)^2 per sample,
// delta = max(atol, rtol*max(|x_lower|, |x_prev|)) (:969-971), every operation a single fp32 one in the reference's order.
// The sum follows plms_x0_norm_kernel: fp64 per thread, a fixed LDS tree per block, block j of sample b into part[b*gridDim.x +
// j], at most kAdaptiveBlocks partials per sample, which dpm_adaptive_finish_kernel adds in index order.  No atomics: two runs
// are bit-identical.  As in vlb_terms_kernel a thread owns four consecutive elements and V only selects how they are loaded and
// stored, so the scalar path adds the same values in the same order as the 16-byte one.
static constexpr int kAdaptiveBlocks = 32;
template <int V>
__global__ __launch_bounds__(256) void dpm_adaptive_error_kernel(DpmAdaptiveErr a, DpmEval lo, int n) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    const int64_t row = (int64_t)b * n;
    const float* xh = a.xh + (int64_t)b * a.x_bs;
    double acc = 0.0;
    for (int p = (blockIdx.x * 256 + threadIdx.x) * 4; p < n; p += gridDim.x * 1024) {
        const int valid = n - p < 4 ? n - p : 4;
        const Pack<4> xb = ld_quad<V>(a.base + row + p, valid), ma = ld_quad<V>(a.ma + row + p, valid);
        const Pack<4> mb = a.mb ? ld_quad<V>(a.mb + row + p, valid) : ma;
        const Pack<4> hi = ld_quad<V>(xh + p, valid), xp = ld_quad<V>(a.x_prev + row + p, valid);
        Pack<4> xl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xl.v[j] = dpm_eval_value(lo, xb.v[j], ma.v[j], mb.v[j], ma.v[j]);
            const float delta = fmaxf(a.atol, a.rtol * fmaxf(fabsf(xl.v[j]), fabsf(xp.v[j])));
            const float q = (hi.v[j] - xl.v[j]) / delta;
            if (j < valid) acc += (double)q * (double)q;
        }
        st_quad<V>(a.x_lower + row + p, xl, valid);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.part[(int64_t)b * gridDim.x + blockIdx.x] = red[0];
}

__global__ void dpm_adaptive_finish_kernel(const double* __restrict__ part, int nblk, int n, float* __restrict__ err, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sum = 0.0;
    for (int j = 0; j < nblk; ++j) sum += part[(int64_t)b * nblk + j];
    err[b] = (float)sqrt(sum / (double)n);
}

size_t dpm_adaptive_part_doubles(int B) { return (size_t)B * kAdaptiveBlocks; }

void dpm_adaptive_error(const DpmAdaptiveErr& arg, int B, int64_t n, hipStream_t s) {
    DpmAdaptiveErr a = arg;
    if (!B || !n) return;
    DSD_CHECK(n <= (int64_t)1 << 30, "adaptive error estimate: one sample has %lld elements; up to 2^30 are taken", (long long)n);
    DSD_CHECK(B <= 65535, "adaptive error estimate: %d samples; up to 65535 are taken", B);
    DSD_CHECK(a.part && a.err, "adaptive error estimate: it needs its scratch and its output");
    if (a.x_bs <= 0) a.x_bs = n;
    if (a.lower_order == 1) a.mb = nullptr;
    DpmEval lo;
    for (int j = 0; j < 3; ++j) lo.c[j] = a.c[j];
    lo.kind = a.lower_order == 1 ? DSD_DPM_MS1 : DSD_DPM_SS_T2;
    const bool v4 = can_vec4(n, a.x_bs, a.base, a.ma, a.mb, a.xh, a.x_prev, a.x_lower);
    const int nblk = (int)std::min<int64_t>((n + 1023) / 1024, kAdaptiveBlocks);
    launch_vec(v4, [&](auto V) {
        hipLaunchKernelGGL(dpm_adaptive_error_kernel<decltype(V)::value>, dim3(nblk, B), dim3(256), 0, s, a, lo, (int)n);
    });
    check_launch("dpm_adaptive_error");
    hipLaunchKernelGGL(dpm_adaptive_finish_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, a.part, nblk, (int)n, a.err, B);
    check_launch("dpm_adaptive_finish");
}

// scale: LatentDiffusion.get_first_stage_encoding's scale_factor * z (ddpm.py:660-667), applied after the sample is formed
// (1.0 for the plain DiagonalGaussianDistribution.sample: x * 1.0f is exact).  With B = batch*K rows ordered (sample, key),
// z [B*K,E,HW] IS the [batch,K*E,HW] 'concat' conditioning: key k of a sample lands in channels [k*E,(k+1)*E).
__global__ void gaussian_sample_kernel(const float* __restrict__ mo, const float* __restrict__ noise, uint64_t seed, int B, int E,
                                       int HW, float scale, float* __restrict__ z) {
    const int64_t total = (int64_t)B * E * HW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / ((int64_t)E * HW);
        const int64_t r = i - b * E * HW;                       // (e, p) inside the sample
        const float mean = mo[b * 2 * E * HW + r];
        float logvar = mo[b * 2 * E * HW + (int64_t)E * HW + r];
        logvar = fminf(fmaxf(logvar, -30.f), 20.f);             // distributions.py:28
        const float std = expf(0.5f * logvar);
        const float eps = noise ? noise[i] : philox_normal_at(i, seed, 0);
        z[i] = scale * (mean + std * eps);                      // :36, then ddpm.py:667
    }
}
void gaussian_sample(const float* moments, const float* noise, uint64_t seed, int B, int E, int HW, float* z, hipStream_t s,
                     float scale) {
    const int64_t total = (int64_t)B * E * HW;
    if (!total) return;
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, moments,
                       noise, seed, B, E, HW, scale, z);
    check_launch("gaussian_sample");
}

__global__ void fill_t_kernel(float* t, int B, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) t[i] = v;
}
void fill_t(float* t, int B, float v, hipStream_t s) {
    hipLaunchKernelGGL(fill_t_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, t, B, v);
    check_launch("fill_t");
}

}  // namespace dsd
