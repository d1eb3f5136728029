// sampler_dev.h — device functions shared by sampler.hip and loss.hip: the Philox normal stream, the packed loads, the pieces of
// p_mean_variance and the variational-bound term with its deterministic reduction.  Both files include it under
// `#pragma clang fp contract(off)` (the reference evaluates these as separate fp32 torch ops), which this header repeats so the
// functions never depend on where they are included from.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "../../include/dsdiff.h"

#pragma clang fp contract(off)

namespace dsd {

// ---- Philox4x32-10 (Salmon et al. 2011): counter = (idx, step), key = seed
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                               uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// element i of the normal stream for (seed, step): Box-Muller on the Philox block i/4... each block yields 4 normals
__device__ __forceinline__ float philox_normal_at(int64_t i, uint64_t seed, uint64_t step) {
    uint32_t r[4];
    const uint64_t blk = (uint64_t)i >> 2;
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    const int lane = (int)(i & 3);
    const uint32_t a = r[lane & 2], b = r[(lane & 2) + 1];
    const float u1 = ((float)a + 1.0f) * 2.3283064365386963e-10f;  // (0,1]
    const float u2 = (float)b * 2.3283064365386963e-10f;           // [0,1)
    const float rad = sqrtf(-2.0f * logf(u1));
    const float ang = 6.283185307179586f * u2;
    return (lane & 1) ? rad * sinf(ang) : rad * cosf(ang);
}

// V = 4: 16-byte accesses (n, x_bs multiples of 4 and 16-byte aligned pointers; the launchers check), V = 1 otherwise.
template <int V> struct alignas(4 * V) Pack { float v[V]; };
template <int V> __device__ __forceinline__ Pack<V> ld_pack(const float* p) { return *reinterpret_cast<const Pack<V>*>(p); }
template <int V> __device__ __forceinline__ void st_pack(float* p, const Pack<V>& a) { *reinterpret_cast<Pack<V>*>(p) = a; }

// normals i .. i+V-1 of the (seed, step) stream; i % V == 0.  V = 4 is one Philox block: the values philox_normal_at gives
template <int V> __device__ __forceinline__ Pack<V> philox_normal_pack(int64_t i, uint64_t seed, uint64_t step) {
    Pack<V> z;
    if constexpr (V == 4) {
        uint32_t r[4];
        const uint64_t blk = (uint64_t)i >> 2;
        philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed,
                      (uint32_t)(seed >> 32), r);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float u1 = ((float)r[2 * h] + 1.0f) * 2.3283064365386963e-10f;
            const float u2 = (float)r[2 * h + 1] * 2.3283064365386963e-10f;
            const float rad = sqrtf(-2.0f * logf(u1));
            const float ang = 6.283185307179586f * u2;
            z.v[2 * h] = rad * cosf(ang);
            z.v[2 * h + 1] = rad * sinf(ang);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) z.v[j] = philox_normal_at(i + j, seed, step);
    }
    return z;
}

// The launchers' side of V: 16-byte accesses when one sample (n elements) and the state's row stride are multiples of four
// floats and every pointer the kernel takes packs from is 16-byte aligned (a null one counts as aligned).
template <class... P> static bool can_vec4(int64_t n, int64_t x_bs, const P*... ptrs) {
    return n % 4 == 0 && x_bs % 4 == 0 && (... && (((uintptr_t)ptrs & 15u) == 0));
}
// launch(std::integral_constant<int, V>) with V = 4 or 1
template <class F> static void launch_vec(bool v4, F&& launch) {
    if (v4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 1>{});
}

// pred_xstart of the guided-diffusion family and of ldm's DDPM (gaussian_diffusion.py:311-341): the network output as v, eps or
// x_start, then process_xstart's clip
__device__ __forceinline__ float pred_xstart_value(const StepCoef& sc, float out, float xt) {
    const float* c = sc.c;
    float x0;
    if (sc.pred == DSD_PRED_V)
        x0 = c[0] * xt - c[1] * out;
    else if (sc.pred == DSD_PRED_EPS)
        x0 = c[2] * xt - c[3] * out;
    else
        x0 = out;
    if (sc.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    return x0;
}
// the learned-range log-variance (gaussian_diffusion.py:287-293) from the variance channel, or the step's fixed one
__device__ __forceinline__ float model_log_variance(const StepCoef& sc, float var) {
    if (!sc.learned_range) return sc.c[6];
    const float frac = (var + 1.f) / 2.f;
    return frac * sc.c[7] + (1.f - frac) * sc.c[6];
}

// q_sample draws from stream (seed, step + 2^32): the update of iteration `step` draws from (seed, step)
static constexpr uint64_t kBlendStream = 1ull << 32;

// ---- the per-sample reductions: a block owns kVlbPiece consecutive elements of one sample, a thread four of them
static constexpr int kVlbPiece = 1024;

template <int V> __device__ __forceinline__ Pack<4> ld_quad(const float* p, int valid) {
    if constexpr (V == 4) return ld_pack<4>(p);
    Pack<4> r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = j < valid ? p[j] : 0.f;
    return r;
}
template <int V> __device__ __forceinline__ void st_quad(float* p, const Pack<4>& a, int valid) {
    if constexpr (V == 4) {
        st_pack<4>(p, a);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) p[j] = a.v[j];
    }
}
// the four normals of elements ctr .. ctr+3 of q_sample's stream (those past `valid` are 0)
template <int V> __device__ __forceinline__ Pack<4> philox_quad(int64_t ctr, uint64_t seed, uint64_t step, int valid) {
    if constexpr (V == 4) return philox_normal_pack<4>(ctr, seed, step + kBlendStream);
    Pack<4> z;
#pragma unroll
    for (int j = 0; j < 4; ++j) z.v[j] = j < valid ? philox_normal_at(ctr + j, seed, step + kBlendStream) : 0.f;
    return z;
}

// the NQ sums of a block: the 256 threads' sums folded in the fixed tree, thread 0 writes them
template <int NQ>
__device__ __forceinline__ void vlb_block_fold(const double (&acc)[NQ], double* red, double* dst) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[q * 256 + threadIdx.x] = acc[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) red[q * 256 + threadIdx.x] += red[q * 256 + threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) dst[q] = red[q * 256];
    }
}

// normal_kl (losses.py:32-38), left to right
__device__ __forceinline__ float normal_kl_value(float mean1, float logvar1, float mean2, float logvar2) {
    const float d = mean1 - mean2;
    return 0.5f * (-1.0f + logvar2 - logvar1 + expf(logvar1 - logvar2) + (d * d) * expf(-logvar2));
}
// approx_standard_normal_cdf (losses.py:41-46); pow(x, 3) is x*x*x in torch
__device__ __forceinline__ float approx_normal_cdf(float x) {
    return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * (x * x * x))));
}
// discretized_gaussian_log_likelihood (losses.py:49-77)
__device__ __forceinline__ float discretized_log_likelihood(float x, float mean, float log_scale) {
    const float centered = x - mean;
    const float inv_stdv = expf(-log_scale);
    const float cdf_plus = approx_normal_cdf(inv_stdv * (centered + (float)(1.0 / 255.0)));
    const float cdf_min = approx_normal_cdf(inv_stdv * (centered - (float)(1.0 / 255.0)));
    float arg = fmaxf(cdf_plus - cdf_min, 1e-12f);
    if (x > 0.999f) arg = fmaxf(1.0f - cdf_min, 1e-12f);
    if (x < -0.999f) arg = fmaxf(cdf_plus, 1e-12f);
    return logf(arg);                                          // one logf: the selects choose its argument
}

// One thread's share of the bound's terms of sample b (VlbStep, kernels.h): its four elements from p on, under the step
// coefficients sc and the true posterior's log-variance post_log_var — the call's (vlb_terms_kernel) or the sample's own
// (vlb_terms_rows_kernel).  Adds the KL (DECODER: the negated discretised log-likelihood), (pred_xstart - x_start)^2 and
// (eps - noise)^2 to acc and writes the optional planes.
template <int V, bool DECODER>
__device__ __forceinline__ void vlb_thread_terms(const VlbStep& a, const StepCoef& sc, float post_log_var, int b, int n, int p,
                                                 double (&acc)[3]) {
    const int64_t row = (int64_t)b * n;
    const int valid = n - p;                                   // <= 0: nothing of this thread's lies inside the sample
    if (valid > 0) {
        const float* orow = a.out + (int64_t)b * a.o_bs + p;
        const Pack<4> xs = ld_quad<V>(a.x_start + row + p, valid), xt = ld_quad<V>(a.xt + (int64_t)b * a.x_bs + p, valid);
        const Pack<4> out = ld_quad<V>(orow, valid);
        Pack<4> z, var = {};
        if (a.noise) {
            z = ld_quad<V>(a.noise + row + p, valid);
        } else {
            const int64_t ctr = (a.slice_ids ? a.slice_ids[b] * n : row) + p;
            if constexpr (V == 4) {
                z = philox_normal_pack<4>(ctr, a.seed, a.step + kBlendStream);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) z.v[j] = j < valid ? philox_normal_at(ctr + j, a.seed, a.step + kBlendStream) : 0.f;
            }
        }
        if (sc.learned_range) var = ld_quad<V>(orow + n, valid);
        Pack<4> mean, lv, x0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x0.v[j] = pred_xstart_value(sc, out.v[j], xt.v[j]);
            mean.v[j] = sc.c[4] * x0.v[j] + sc.c[5] * xt.v[j];                 // q_posterior_mean_variance :220-223
            lv.v[j] = model_log_variance(sc, var.v[j]);
            float term;
            if constexpr (DECODER) {
                term = -discretized_log_likelihood(xs.v[j], mean.v[j], 0.5f * lv.v[j]);
            } else {
                const float true_mean = sc.c[4] * xs.v[j] + sc.c[5] * xt.v[j];
                term = normal_kl_value(true_mean, post_log_var, mean.v[j], lv.v[j]);
            }
            const float dx = x0.v[j] - xs.v[j];
            const float eps = (sc.c[2] * xt.v[j] - x0.v[j]) / sc.c[3];         // _predict_eps_from_xstart :369-373
            const float de = eps - z.v[j];
            if (j < valid) {
                acc[0] += (double)term;
                acc[1] += (double)(dx * dx);
                acc[2] += (double)(de * de);
            }
        }
        if (a.mean) st_quad<V>(a.mean + row + p, mean, valid);
        if (a.log_variance) st_quad<V>(a.log_variance + row + p, lv, valid);
        if (a.pred_xstart) st_quad<V>(a.pred_xstart + row + p, x0, valid);
    }
}

// One wave per sample (64 threads): lane l adds the partials l, l+64, ... of sample b in index order, the 64 lane sums fold in
// a fixed tree (red: nq*64 doubles of LDS); on thread 0, red[q*64] then holds the sum of quantity q.
__device__ __forceinline__ void rows_fold_partials(const double* __restrict__ part, int b, int nblk, int nq, double* red) {
    for (int q = 0; q < nq; ++q) {
        double sum = 0.0;
        for (int j = threadIdx.x; j < nblk; j += 64) sum += part[((int64_t)b * nblk + j) * nq + q];
        red[q * 64 + threadIdx.x] = sum;
    }
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < nq; ++q) red[q * 64 + threadIdx.x] += red[q * 64 + threadIdx.x + w];
        __syncthreads();
    }
}
// mean_flat in fp64 rounded to fp32 once, then (bits) the reference's fp32 division by np.log(2.0)
__device__ __forceinline__ float rows_mean_value(double sum, int n, bool bits) {
    float v = (float)(sum / (double)n);
    if (bits) v = v / 0.6931471805599453f;
    return v;
}

}  // namespace dsd
