// attention_wide.hip — fused softmax(Q K^T) V with online softmax for head dims 132..512 (attention.hip stops at 128).
//
// Widths of the SD-v1 U-Net's SpatialTransformer heads (160), of AttentionBlock / CrossAttention with one head on >= 160
// channels and of the KL-VAE's AttnBlock (one head over 512 channels, ldm/modules/diffusionmodules/model.py:185-209).
// Reached through attention_any() below: the VAE's fused AttnBlock (dsd_set_vae_fused_attention) and dsd_op_attention.
//
// One workgroup = (sample, head, 32 queries).  O for 32 queries at d = 512 is 256 accumulator registers per lane, so one
// wave cannot own a whole head: the head dim is SLICED across the four waves, wave w owns d in [w*SW, w*SW + SW) with
// SW = 32 DT = 64 / 96 / 128 (zero-padded: 4 SW >= d), i.e. the register footprint of the narrow kernels at d = SW.
//   * Every wave multiplies its slice of K into a partial S^T tile (32 keys x 32 queries, the transposed-score layout of
//     attention.hip: lane = query, 16 keys per lane).  The four partials are exchanged through LDS (4 KB per wave and
//     sub-tile, double-buffered: one barrier per sub-tile) and EVERY wave adds them in the same order ((p0+p1)+p2)+p3, so
//     all four hold a bit-identical S, hence identical running maxima, identical rescale decisions and identical l: the
//     slices of one output row are scaled alike.
//   * Every wave then runs the same softmax and multiplies P (in registers, B-operand layout) into its slice of V.
//   * With 32 queries per workgroup and the head dim sliced, a K or V element is used by exactly ONE wave, once: LDS would
//     only re-lay it out.  Both operands therefore go global -> registers directly in A-operand layout (K: lane = key, 8
//     resp. 4 consecutive d per load; V: lane = d, one key per load, 128 contiguous bytes per 32 lanes) and are split into
//     bf16 pieces there.  The only LDS is the 32 KB score exchange; the score matrix never leaves the chip.
//   * Padding costs no predicated load.  Q is zero beyond d and beyond Tq, which alone makes the padded part of every
//     score sum vanish; scores of keys beyond Tk are masked to -inf after the exchange, so their P is exactly 0; rows of
//     O^T beyond d are never stored.  K and V addresses past the head dim or past Tk are therefore CLAMPED to the last
//     valid element rather than zero-filled: what they fetch is multiplied by an exact zero or lands in an unwritten row
//     (as in the narrow kernels, a non-finite input poisons its head either way).
// Two arithmetics, as the narrow kernels: exact fp32 MFMA (split == 0) and bf16x6 (split == 1: split8 / mfma6 of
// device_common.h).
#include "device_common.h"

namespace dsd {

// S = ((p0 + p1) + p2) + p3 of the four waves' partial tiles; xs is this sub-tile's buffer [wave][register][lane].
__device__ __forceinline__ void w_exchange(float* xs, int wave, int lane, f32x16& sacc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(wave * 16 + r) * 64 + lane] = sacc[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p0 = xs[(0 * 16 + r) * 64 + lane], p1 = xs[(1 * 16 + r) * 64 + lane];
        const float p2 = xs[(2 * 16 + r) * 64 + lane], p3 = xs[(3 * 16 + r) * 64 + lane];
        sacc[r] = ((p0 + p1) + p2) + p3;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// exact fp32: v_mfma_f32_32x32x2_f32 for both products, plain online softmax (attention_kernel's arithmetic)
template <int DT>
__global__ __launch_bounds__(256, 1) void attention_wide_kernel(AttnArgs a) {
    constexpr int SW = DT * 32;   // this wave's slice of the (padded) head dim
    constexpr int DH = SW / 2;    // per lane-half k range of the QK^T product
    __shared__ __attribute__((aligned(16))) float xs[2 * 4 * 16 * 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, half = lane >> 5;
    const int n = blockIdx.z, head = blockIdx.y;
    const int q = blockIdx.x * 32 + lrow;
    const bool q_ok = q < a.Tq;
    const int dbase = wave * SW;

    // Q^T fragment (B operand): this lane's query, d in dbase + [half*DH, half*DH + DH), pre-scaled like the reference
    float qf[DH];
    {
        const float* qp = a.q + ((int64_t)n * a.Tq + (q_ok ? q : 0)) * a.ldq + (int64_t)head * a.q_hs;
#pragma unroll
        for (int i = 0; i < DH; i += 4) {
            const int d = dbase + half * DH + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q_ok && d < a.d) v = *reinterpret_cast<const float4*>(qp + d);
            qf[i] = v.x * a.scale_q;
            qf[i + 1] = v.y * a.scale_q;
            qf[i + 2] = v.z * a.scale_q;
            qf[i + 3] = v.w * a.scale_q;
        }
    }
    f32x16 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const float* kbase = a.k + (int64_t)n * a.Tk * a.ldk + (int64_t)head * a.k_hs;
    const float* vbase = a.v + (int64_t)n * a.Tk * a.ldv + (int64_t)head * a.v_hs;
    // K fragment (A operand of S^T = K Q^T): lane = key k0 + lrow, the same d range as qf; fetched one sub-tile ahead
    float4 kreg[DH / 4];
    auto fetch_k = [&](int k0) {
        const float* kp = kbase + (int64_t)min(k0 + lrow, a.Tk - 1) * a.ldk;
#pragma unroll
        for (int i = 0; i < DH; i += 4) kreg[i / 4] = *reinterpret_cast<const float4*>(kp + min(dbase + half * DH + i, a.d - 4));
    };
    fetch_k(0);
    int buf = 0;
    for (int k0 = 0; k0 < a.Tk; k0 += 32, buf ^= 1) {
        // V fragments (A operand of O^T = V^T P^T): lane = d, register s = key k0 + (s&3) + 8 (s>>2) + 4 half — the key
        // order of the S^T accumulator.  Issued before the first product, which hides their latency.
        float vf[DT][16];
        const float* vtile = vbase + (int64_t)k0 * a.ldv;   // in-tile offsets fit 32 bits (checked at launch)
        const int klast = a.Tk - 1 - k0;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const unsigned dcl = min(dbase + t * 32 + lrow, a.d - 1);
#pragma unroll
            for (int s = 0; s < 16; ++s) vf[t][s] = vtile[(unsigned)min((s & 3) + 8 * (s >> 2) + 4 * half, klast) * (unsigned)a.ldv + dcl];
        }
        // partial S^T[key][q] = sum over this wave's d of K[key][d] Q[q][d]
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int i = 0; i < DH; i += 4) {
            const float4 k4 = kreg[i / 4];
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x * a.scale_k, qf[i], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y * a.scale_k, qf[i + 1], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z * a.scale_k, qf[i + 2], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w * a.scale_k, qf[i + 3], sacc, 0, 0, 0);
        }
        if (k0 + 32 < a.Tk) fetch_k(k0 + 32);
        w_exchange(xs + buf * (4 * 16 * 64), wave, lane, sacc);
        // mask + online softmax, identical in all four waves
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float sv = sacc[r] * a.scale_s;
            sv = key < a.Tk ? sv : -INFINITY;
            sacc[r] = sv;
            tmax = fmaxf(tmax, sv);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m_run, tmax);
        const float corr = expf(m_run - m_new);  // m_run = -inf on the first tile -> 0
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = expf(sacc[r] - m_new);
            sacc[r] = pv;
            psum += pv;
        }
        psum += __shfl_xor(psum, 32);
        l_run = l_run * corr + psum;
        m_run = m_new;
        // O^T[d][q] = corr * O^T + sum_key V[key][d] P[key][q]
#pragma unroll
        for (int t = 0; t < DT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] *= corr;
#pragma unroll
            for (int s = 0; s < 16; ++s) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[t][s], sacc[s], o[t], 0, 0, 0);
        }
    }
    if (!q_ok) return;
    const float inv = 1.f / l_run;
    float* op = a.out + ((int64_t)n * a.Tq + q) * a.ldo + (int64_t)head * a.d;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = dbase + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (d < a.d) op[d] = o[t][r] * inv;
        }
}

// ------------------------------------------------------------------------------------------------------------------
// bf16x6: operands split exactly into three bf16 pieces, six v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation;
// base-2 logits and the optimistic running maximum of attention_split_kernel.
template <int DT>
__global__ __launch_bounds__(256, 1) void attention_wide_split_kernel(AttnArgs a) {
    constexpr int SW = DT * 32;   // this wave's slice of the (padded) head dim
    constexpr int NKS = SW / 16;  // 16-wide k-steps of the QK^T product per wave
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ __attribute__((aligned(16))) float xs[2 * 4 * 16 * 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, half = lane >> 5;
    const int n = blockIdx.z, head = blockIdx.y;
    const int q = blockIdx.x * 32 + lrow;
    const bool q_ok = q < a.Tq;
    const int dbase = wave * SW;

    // Q pieces (B operand): this lane's query, k-step s covers d = dbase + 16 s + 8 half .. + 8; base-2 logits
    bf16x8 qf[NKS][3];
    {
        const float qs = a.scale_q * a.scale_s * LOG2E;
        const float* qp = a.q + ((int64_t)n * a.Tq + (q_ok ? q : 0)) * a.ldq + (int64_t)head * a.q_hs;
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; i += 4) {
                const int d = dbase + s * 16 + half * 8 + i;
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q_ok && d < a.d) t = *reinterpret_cast<const float4*>(qp + d);
                v[i] = t.x * qs; v[i + 1] = t.y * qs; v[i + 2] = t.z * qs; v[i + 3] = t.w * qs;
            }
            split8(v, qf[s]);
        }
    }
    f32x16 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = 0.f, l_run = 0.f;   // l_run: this lane's 16 keys of every sub-tile (the halves are added at the end)

    const float* kbase = a.k + (int64_t)n * a.Tk * a.ldk + (int64_t)head * a.k_hs;
    const float* vbase = a.v + (int64_t)n * a.Tk * a.ldv + (int64_t)head * a.v_hs;
    // K (A operand of S^T = K Q^T): lane = key k0 + lrow, k-step s = the 8 floats at d = dbase + 16 s + 8 half; fetched
    // one sub-tile ahead and split when it is multiplied
    float4 kreg[NKS][2];
    auto fetch_k = [&](int k0) {
        const float* kp = kbase + (int64_t)min(k0 + lrow, a.Tk - 1) * a.ldk;
#pragma unroll
        for (int s = 0; s < NKS; ++s)
#pragma unroll
            for (int e = 0; e < 2; ++e) kreg[s][e] = *reinterpret_cast<const float4*>(kp + min(dbase + s * 16 + half * 8 + e * 4, a.d - 4));
    };
    constexpr float THR = 8.f;

    fetch_k(0);
    bool first = true;
    int buf = 0;
    for (int k0 = 0; k0 < a.Tk; k0 += 32, buf ^= 1) {
        // V (A operand of O^T = V^T P^T): lane = d = dbase + 32 t + lrow; element j of k-step s2 is key
        // k0 + 16 s2 + 4 half + (j & 3) + 8 (j >> 2), the key that register 8 s2 + j of the S^T accumulator holds.  Issued
        // before the first product, which hides their latency.
        float vf[DT][2][8];
        const float* vtile = vbase + (int64_t)k0 * a.ldv;   // in-tile offsets fit 32 bits (checked at launch)
        const int klast = a.Tk - 1 - k0;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const unsigned dcl = min(dbase + t * 32 + lrow, a.d - 1);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    vf[t][s2][j] = vtile[(unsigned)min(16 * s2 + 4 * half + (j & 3) + 8 * (j >> 2), klast) * (unsigned)a.ldv + dcl];
        }
        // partial S^T[key][q] = sum over this wave's d of K[key][d] Q[q][d]
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const float kv[8] = {kreg[s][0].x * a.scale_k, kreg[s][0].y * a.scale_k, kreg[s][0].z * a.scale_k, kreg[s][0].w * a.scale_k,
                                 kreg[s][1].x * a.scale_k, kreg[s][1].y * a.scale_k, kreg[s][1].z * a.scale_k, kreg[s][1].w * a.scale_k};
            bf16x8 kp[3];
            split8(kv, kp);
            mfma6(kp, qf[s], sacc);
        }
        if (k0 + 32 < a.Tk) fetch_k(k0 + 32);
        w_exchange(xs + buf * (4 * 16 * 64), wave, lane, sacc);
        // S - m, keys beyond Tk take no part; identical in all four waves from here on
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            sacc[r] = key < a.Tk ? sacc[r] - m_run : -INFINITY;
        }
        float tmax = sacc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sacc[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const bool need = first || !(tmax <= THR);
        if (__any(need)) {
            const float delta = need ? tmax : 0.f;
            const float corr = first ? 0.f : __builtin_amdgcn_exp2f(-delta);
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= corr;
            l_run *= corr;
            m_run += delta;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] -= delta;
            first = false;
        }
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sacc[r] = __builtin_amdgcn_exp2f(sacc[r]);
            psum += sacc[r];
        }
        l_run += psum;
        // O^T[d][q] += sum_key V[key][d] P[key][q];  k-step s2 = registers 8 s2 .. 8 s2 + 7 of P, split exactly into 3 pieces
        bf16x8 pf[2][3];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = sacc[8 * s2 + e];
            split8(v, pf[s2]);
        }
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 vp[3];
                split8(vf[t][s2], vp);
                mfma6(vp, pf[s2], o[t]);
            }
    }
    if (!q_ok) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.f / l_tot;
    float* op = a.out + ((int64_t)n * a.Tq + q) * a.ldo + (int64_t)head * a.d;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int d = dbase + t * 32 + 8 * r4 + 4 * half;
            if (d < a.d)   // head dim % 4 == 0 and d % 4 == 0: the four values are valid together
                *reinterpret_cast<float4*>(op + d) = make_float4(o[t][4 * r4] * inv, o[t][4 * r4 + 1] * inv, o[t][4 * r4 + 2] * inv, o[t][4 * r4 + 3] * inv);
        }
}

// 128 < d <= 512
void attention_wide(const AttnArgs& a, hipStream_t s) {
    DSD_CHECK(a.d % 4 == 0 && a.d > 128 && a.d <= 512, "attention: head dim %d unsupported (need multiple of 4, <=512)", a.d);
    DSD_CHECK(a.Tk >= 1 && a.Tq >= 1, "attention: empty sequence");
    DSD_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.q_hs % 4 == 0 && a.k_hs % 4 == 0 && a.v_hs % 4 == 0,
              "attention: rows must be 16-byte aligned");
    DSD_CHECK(!a.split || a.ldo % 4 == 0, "attention: output rows must be 16-byte aligned");
    DSD_CHECK(a.ldv <= (1 << 26), "attention: V row stride %d too large for the wide-head kernels", a.ldv);   // 32 ldv in an int
    const dim3 grid(cdiv(a.Tq, 32), a.heads, a.N), block(256);
    const int dt = cdiv(a.d, 128);   // 32-wide d tiles per wave
    if (a.split) {
        switch (dt) {
            case 2: hipLaunchKernelGGL(attention_wide_split_kernel<2>, grid, block, 0, s, a); break;
            case 3: hipLaunchKernelGGL(attention_wide_split_kernel<3>, grid, block, 0, s, a); break;
            default: hipLaunchKernelGGL(attention_wide_split_kernel<4>, grid, block, 0, s, a); break;
        }
        check_launch("attention_wide_split");
        return;
    }
    switch (dt) {
        case 2: hipLaunchKernelGGL(attention_wide_kernel<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(attention_wide_kernel<3>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(attention_wide_kernel<4>, grid, block, 0, s, a); break;
    }
    check_launch("attention_wide");
}

// attention() up to d = 128, attention_wide() up to 512; anything else is refused by name.  The entry of the callers that take
// wide heads today: the KL-VAE's fused AttnBlock and dsd_op_attention.
void attention_any(const AttnArgs& a, hipStream_t s) {
    DSD_CHECK(a.d % 4 == 0 && a.d >= 4 && a.d <= 512, "attention: head dim %d unsupported (need multiple of 4, <=512)", a.d);
    if (a.d > 128)
        attention_wide(a, s);
    else
        attention(a, s);
}

}  // namespace dsd
