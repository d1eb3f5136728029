// conv.hip — NHWC fp32 convolution as an implicit GEMM on the gfx950 f32 matrix cores.
//
// Replaces every nn.Conv2d / nn.Conv1d(k=1) call site on the hot path
// (ldm/modules/diffusionmodules/util.py:229-239 conv_nd; openaimodel.py:109,155,208,234,245,452,460;
//  UNet_DS_Diff/model.py:158,163,285,514,569-601).
//
//   M = N*OH*OW (output pixels), Ngemm = Cout, K = ks*ks*Cin, A gathered on the fly (im2col never
//   materialised), B = weights packed OHWI so both operands are K-contiguous.
//   Block = 256 threads = 4 waves; block tile 128 (M) x 32*NT (N) x 32 (K); each wave owns 32 rows and
//   all NT 32-wide column tiles -> NT accumulators of v_mfma_f32_32x32x2_f32 (exact fp32 fma chain).
//   LDS tiles are [row][36] floats (pad 4): the ds_read_b128 fragment reads (lane = row, 4 k's) and the
//   ds_write_b128 staging writes are both bank-conflict free with that stride.
//   K order inside a group of 8 is permuted (lane half h takes k = 8g+4h+j for MFMA j) identically for A
//   and B, so one 16-byte LDS read feeds four MFMAs.
//   Global -> register prefetch of tile kt+1 is issued before the MFMAs of tile kt (single LDS buffer,
//   2 blocks per CU hide the barriers).  Epilogue fuses bias, the per-(sample,channel) timestep-embedding
//   add and the residual add.
//   Two kernels share the tile code: conv_mfma_buf_kernel (default; buffer loads, hardware range check for
//   padding) and conv_mfma_kernel (flat loads + masks; any Cin % 4 == 0, operands >= 4 GiB).
//   Measured on the way here (tools/bench_conv.py, 16x256x256x320->320): flat loads 125 TF/s; + fragment
//   reads issued one group ahead and a branch-free epilogue 129; MFMA + LDS reads alone 151, + barriers and
//   LDS writes 147, i.e. the flat kernel lost 12 % to address arithmetic / branches in the load phase;
//   buffer loads 143 (91 % of the 157.3 TF/s fp32 matrix peak).  A double-buffered BK=16 / one-barrier
//   variant and an accumulator-interleaved MFMA order were tried and are not faster (142 / 127).
#include "device_common.h"

#include <string>

#include <cstdlib>

namespace dsd {

static constexpr size_t DIRECT_LDS_MAX = 128 * 1024;   // weights of the small-K direct kernel, [K][Cout] fp32 in LDS
static constexpr int BM = 128;
static constexpr int BK = 32;
static constexpr int LDS_STRIDE = 36;

struct ConvP {
    const float* x;
    const float* w;
    const float* bias;
    const float* emb;
    const float* res;
    float* y;
    int64_t x_bs;
    int N, H, W, Cin, Cout, OH, OW, ks, stride, pad, ups, emb_stride, out_nchw;
    int M, Ktot, cchunks, IHg, IWg, tiles_m, tiles_n, ohw;
    unsigned x_bytes, w_bytes;  // buffer-descriptor extents (buffer-load kernel only)
    int y_ld;                   // row stride of y (>= Cout)
};


// ---- accumulator tile -> memory.  C/D map of a 32x32 tile: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
// Interior tiles (the common case) take a branch-free path: bias once per column, then per group of 4 rows all
// residual / embedding loads are issued together before the adds and stores (one vmcnt wait per group instead of
// one dependent global load per element).
template <int NT>
__device__ __forceinline__ void conv_epilogue(const ConvP& p, const f32x16 (&acc)[NT], int m0, int n0, int wave, int lrow,
                                              int half) {
    const bool interior = (m0 + BM <= p.M) && (n0 + NT * 32 <= p.Cout) && !p.out_nchw;
    if (interior) {
        float bj[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) bj[j] = p.bias ? p.bias[n0 + j * 32 + lrow] : 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int mb = m0 + wave * 32 + 8 * g + 4 * half;  // rows mb .. mb+3  <->  regs 4g .. 4g+3
            float ev[4][NT], rv[4][NT];
            if (p.emb) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float* er = p.emb + (int64_t)((mb + rr) / p.ohw) * p.emb_stride + n0 + lrow;
#pragma unroll
                    for (int j = 0; j < NT; ++j) ev[rr][j] = er[j * 32];
                }
            }
            if (p.res) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float* rp = p.res + (int64_t)(mb + rr) * p.Cout + n0 + lrow;
#pragma unroll
                    for (int j = 0; j < NT; ++j) rv[rr][j] = rp[j * 32];
                }
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                float* yp = p.y + (int64_t)(mb + rr) * p.y_ld + n0 + lrow;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    float v = acc[j][4 * g + rr] + bj[j];
                    if (p.emb) v += ev[rr][j];
                    if (p.res) v += rv[rr][j];
                    yp[j * 32] = v;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= p.M) continue;
        const int nb = m / p.ohw;
        const float* embrow = p.emb ? p.emb + (int64_t)nb * p.emb_stride : nullptr;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + j * 32 + lrow;
            if (n >= p.Cout) continue;
            float v = acc[j][r];
            if (p.bias) v += p.bias[n];
            if (embrow) v += embrow[n];
            if (p.res) v += p.res[(int64_t)m * p.Cout + n];
            if (p.out_nchw) {
                const int pix = m - nb * p.ohw;
                p.y[((int64_t)nb * p.Cout + n) * p.ohw + pix] = v;
            } else {
                p.y[(int64_t)m * p.y_ld + n] = v;
            }
        }
    }
}

// ---- MFMAs of NKG k-groups (8 k each) of one staged tile, fragment reads software-pipelined ONE group ahead:
// the ds_read_b128 of group g+1 is issued before the four MFMAs of group g, so its latency hides behind 256 cycles
// of matrix work instead of being waited for in front of every group.
template <int NT, int NKG, int LSTRIDE>
__device__ __forceinline__ void conv_tile_mfma(const float* a_frag, const float* b_frag, f32x16 (&acc)[NT]) {
    float4 a_cur = *reinterpret_cast<const float4*>(a_frag);
    float4 b_cur = *reinterpret_cast<const float4*>(b_frag);
    float4 a_nxt = a_cur, b_nxt = b_cur;
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (j + 1 < NT) {
                b_nxt = *reinterpret_cast<const float4*>(b_frag + (j + 1) * 32 * LSTRIDE + 8 * kg);
            } else if (kg + 1 < NKG) {
                b_nxt = *reinterpret_cast<const float4*>(b_frag + 8 * (kg + 1));
                a_nxt = *reinterpret_cast<const float4*>(a_frag + 8 * (kg + 1));
            }
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.x, b_cur.x, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.y, b_cur.y, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.z, b_cur.z, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.w, b_cur.w, acc[j], 0, 0, 0);
            b_cur = b_nxt;
            if (j == NT - 1) a_cur = a_nxt;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(ConvP p) {
    __shared__ __attribute__((aligned(16))) float lds[(BM + NT * 32) * LDS_STRIDE];
    float* As = lds;
    float* Bs = lds + BM * LDS_STRIDE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // XCD-aware tile order: blocks that share A rows / the weight panel run on one XCD (one L2).
    const int nwg = gridDim.x;
    int L = blockIdx.x;
    {
        const int cpx = nwg >> 3;
        if (L < (cpx << 3)) L = (L & 7) * cpx + (L >> 3);
    }
    const int tile_n = L % p.tiles_n;
    const int tile_m = L / p.tiles_n;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * (NT * 32);

    // ---- staging map: thread -> (row = tid>>3 (+32 i), 4 consecutive k = 4*(tid&7))
    const int col4 = tid & 7;
    const int srow = tid >> 3;
    int a_h[4], a_w[4];
    int64_t a_nb[4];
    bool a_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int m = m0 + srow + 32 * i;
        a_ok[i] = m < p.M;
        m = a_ok[i] ? m : 0;
        const int n = m / p.ohw;
        const int r = m - n * p.ohw;
        const int oh = r / p.OW;
        const int ow = r - oh * p.OW;
        a_h[i] = oh * p.stride - p.pad;
        a_w[i] = ow * p.stride - p.pad;
        a_nb[i] = (int64_t)n * p.x_bs;
    }
    const float* wrow[NT];
    bool b_ok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + srow + 32 * j;
        b_ok[j] = n < p.Cout;
        wrow[j] = p.w + (int64_t)(b_ok[j] ? n : 0) * p.Ktot;
    }

    float4 ra[4], rb[NT];
    auto load_tile = [&](int kh, int kw, int cc) {
        const int c = cc * BK + col4 * 4;
        const bool cok = c < p.Cin;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int ih = a_h[i] + kh, iw = a_w[i] + kw;
            const bool ok = a_ok[i] && cok && (unsigned)ih < (unsigned)p.IHg && (unsigned)iw < (unsigned)p.IWg;
            if (p.ups) {
                ih >>= 1;
                iw >>= 1;
            }
            ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) ra[i] = *reinterpret_cast<const float4*>(p.x + a_nb[i] + ((int64_t)ih * p.W + iw) * p.Cin + c);
        }
        const int kofs = (kh * p.ks + kw) * p.Cin + c;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b_ok[j] && cok) rb[j] = *reinterpret_cast<const float4*>(wrow[j] + kofs);
        }
    };

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int lrow = lane & 31;
    const int half = lane >> 5;
    const float* a_frag = As + (wave * 32 + lrow) * LDS_STRIDE + 4 * half;
    const float* b_frag = Bs + lrow * LDS_STRIDE + 4 * half;
    float* a_st = As + srow * LDS_STRIDE + col4 * 4;
    float* b_st = Bs + srow * LDS_STRIDE + col4 * 4;

    const int KT = p.ks * p.ks * p.cchunks;
    int kh = 0, kw = 0, cc = 0;
    load_tile(kh, kw, cc);
    for (int kt = 0; kt < KT; ++kt) {
        __syncthreads();  // all waves finished reading the previous tile
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(a_st + 32 * i * LDS_STRIDE) = ra[i];
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<float4*>(b_st + 32 * j * LDS_STRIDE) = rb[j];
        __syncthreads();
        if (kt + 1 < KT) {  // prefetch next tile into registers; lands while the MFMAs below run
            if (++cc == p.cchunks) {
                cc = 0;
                if (++kw == p.ks) {
                    kw = 0;
                    ++kh;
                }
            }
            load_tile(kh, kw, cc);
        }
        conv_tile_mfma<NT, 4, LDS_STRIDE>(a_frag, b_frag, acc);
    }

    conv_epilogue<NT>(p, acc, m0, n0, wave, lrow, half);
}

// Default kernel: same tiling/loop as conv_mfma_kernel, but the operand gathers use BUFFER loads: a 32-bit per-lane
// byte offset that is recomputed only when the filter tap changes (every Cin/32 tiles), a scalar per-tile offset, and
// the hardware range check instead of exec-masked branches for padding / ragged rows (an out-of-range offset returns
// zeros).  The flat-load kernel spends ~12 % of its time issuing address arithmetic and branches (tools/bench_conv.py
// diagnostics); this one issues 9 loads and two scalar adds per tile.  Needs Cin % 32 == 0 and < 4 GiB operands.
template <int NT>
__global__ __launch_bounds__(256, 2) void conv_mfma_buf_kernel(ConvP p) {
    __shared__ __attribute__((aligned(16))) float lds[(BM + NT * 32) * LDS_STRIDE];
    float* As = lds;
    float* Bs = lds + BM * LDS_STRIDE;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwg = gridDim.x;
    int L = blockIdx.x;
    {
        const int cpx = nwg >> 3;
        if (L < (cpx << 3)) L = (L & 7) * cpx + (L >> 3);
    }
    const int tile_n = L % p.tiles_n;
    const int tile_m = L / p.tiles_n;
    const int m0 = tile_m * BM;
    const int n0 = tile_n * (NT * 32);

    const int col4 = tid & 7;
    const int srow = tid >> 3;
    int a_h[4], a_w[4];
    unsigned a_nb[4];
    bool a_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int m = m0 + srow + 32 * i;
        a_ok[i] = m < p.M;
        m = a_ok[i] ? m : 0;
        const int n = m / p.ohw;
        const int r = m - n * p.ohw;
        const int oh = r / p.OW;
        const int ow = r - oh * p.OW;
        a_h[i] = oh * p.stride - p.pad;
        a_w[i] = ow * p.stride - p.pad;
        a_nb[i] = (unsigned)n * (unsigned)p.x_bs + (unsigned)(col4 * 4);
    }
    unsigned b_voff[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + srow + 32 * j;
        b_voff[j] = n < p.Cout ? ((unsigned)n * (unsigned)p.Ktot + (unsigned)(col4 * 4)) * 4u : OOB;
    }
    unsigned a_voff[4];
    auto tap_offsets = [&](int kh, int kw) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int ih = a_h[i] + kh, iw = a_w[i] + kw;
            const bool ok = a_ok[i] && (unsigned)ih < (unsigned)p.IHg && (unsigned)iw < (unsigned)p.IWg;
            if (p.ups) {
                ih >>= 1;
                iw >>= 1;
            }
            a_voff[i] = ok ? (a_nb[i] + (unsigned)(ih * p.W + iw) * (unsigned)p.Cin) * 4u : OOB;
        }
    };
    f32x4 ra[4], rb[NT];
    auto load_tile = [&](int soff_a, int soff_b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, a_voff[i], soff_a, 0));
#pragma unroll
        for (int j = 0; j < NT; ++j) rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, b_voff[j], soff_b, 0));
    };

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int lrow = lane & 31;
    const int half = lane >> 5;
    const float* a_frag = As + (wave * 32 + lrow) * LDS_STRIDE + 4 * half;
    const float* b_frag = Bs + lrow * LDS_STRIDE + 4 * half;
    float* a_st = As + srow * LDS_STRIDE + col4 * 4;
    float* b_st = Bs + srow * LDS_STRIDE + col4 * 4;

    const int KT = p.ks * p.ks * p.cchunks;
    int kh = 0, kw = 0, cc = 0, tap = 0;
    tap_offsets(0, 0);
    load_tile(0, 0);
    for (int kt = 0; kt < KT; ++kt) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(a_st + 32 * i * LDS_STRIDE) = ra[i];
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(b_st + 32 * j * LDS_STRIDE) = rb[j];
        __syncthreads();
        if (kt + 1 < KT) {
            if (++cc == p.cchunks) {
                cc = 0;
                ++tap;
                if (++kw == p.ks) {
                    kw = 0;
                    ++kh;
                }
                tap_offsets(kh, kw);
            }
            load_tile(cc * (BK * 4), (tap * p.Cin + cc * BK) * 4);
        }
        conv_tile_mfma<NT, 4, LDS_STRIDE>(a_frag, b_frag, acc);
    }
    conv_epilogue<NT>(p, acc, m0, n0, wave, lrow, half);
}

// Direct kernel for tiny K (first layer: Cin = 1, K = 9): output-write bound, weights staged in LDS as [k][Cout].
__global__ __launch_bounds__(256) void conv_direct_lds_kernel(ConvP p) {
    extern __shared__ float wl[];  // [Ktot][Cout]
    const int tid = threadIdx.x;
    for (int i = tid; i < p.Ktot * p.Cout; i += 256) {
        const int k = i / p.Cout, co = i - k * p.Cout;
        wl[i] = p.w[(int64_t)co * p.Ktot + k];
    }
    __syncthreads();
    const int c4n = p.Cout >> 2;
    const int PIX = 64;
    const int64_t pix0 = (int64_t)blockIdx.x * PIX;
    for (int idx = tid; idx < PIX * c4n; idx += 256) {
        const int pl = idx / c4n, c4 = idx - pl * c4n;
        const int64_t m = pix0 + pl;
        if (m >= p.M) break;
        const int nb = (int)(m / p.ohw);
        const int r = (int)(m - (int64_t)nb * p.ohw);
        const int oh = r / p.OW, ow = r - oh * p.OW;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int k = 0;
        for (int kh = 0; kh < p.ks; ++kh)
            for (int kw = 0; kw < p.ks; ++kw) {
                int ih = oh * p.stride - p.pad + kh, iw = ow * p.stride - p.pad + kw;
                const bool ok = (unsigned)ih < (unsigned)p.IHg && (unsigned)iw < (unsigned)p.IWg;
                if (p.ups) {
                    ih >>= 1;
                    iw >>= 1;
                }
                const float* src = p.x + (int64_t)nb * p.x_bs + ((int64_t)ih * p.W + iw) * p.Cin;
                for (int ci = 0; ci < p.Cin; ++ci, ++k) {
                    const float xv = ok ? src[ci] : 0.f;
                    const float4 w4 = *reinterpret_cast<const float4*>(wl + k * p.Cout + c4 * 4);
                    acc.x = fmaf(xv, w4.x, acc.x);
                    acc.y = fmaf(xv, w4.y, acc.y);
                    acc.z = fmaf(xv, w4.z, acc.z);
                    acc.w = fmaf(xv, w4.w, acc.w);
                }
            }
        float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = c4 * 4 + q;
            if (p.bias) v[q] += p.bias[n];
            if (p.emb) v[q] += p.emb[(int64_t)nb * p.emb_stride + n];
            if (p.res) v[q] += p.res[m * p.Cout + n];
        }
        if (p.out_nchw) {
            for (int q = 0; q < 4; ++q) p.y[((int64_t)nb * p.Cout + c4 * 4 + q) * p.ohw + r] = v[q];
        } else {
            *reinterpret_cast<float4*>(p.y + m * p.y_ld + c4 * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// First layer (Cin = 1, K = 9 -> 320 channels at 256x256): pure output-write traffic.  A thread owns four fixed output
// channels, keeps their K x 4 weights and bias in registers and walks over pixels: per pixel K broadcast loads, 4K FMAs and
// one 16-byte store, no LDS and no per-element index divisions (the LDS version above reaches 1.9 TB/s, this one the
// store rate of the elementwise kernels).
// STATS [r3]: the workgroup's pixels are one chunk of ONE sample (ppb divides OH*OW) and it also leaves that chunk's per-channel
// (sum, sum of squares) in stats[n][chunk][co][2] (fp64, the GnSrc layout gn_finalize reads): the GroupNorm that follows the
// first convolution of every encoder stream no longer re-reads the 1.3 GB it just wrote.
template <int KMAX, bool STATS>
__global__ __launch_bounds__(256) void conv_direct_cols_kernel(ConvP p, int W4, int ppb, double* __restrict__ stats, int chunks) {
    __shared__ double sm[STATS ? 1024 : 1][2];   // [row][co] partials of rows 1.. (rpi * Cout <= 1024)
    const int rpi = blockDim.x / W4;
    const int row = threadIdx.x / W4;
    const int c4 = threadIdx.x - row * W4;
    double ss[4] = {0.0, 0.0, 0.0, 0.0}, qq[4] = {0.0, 0.0, 0.0, 0.0};
    float4 w[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < p.Ktot) {
            w[k].x = p.w[(int64_t)(c4 * 4 + 0) * p.Ktot + k];
            w[k].y = p.w[(int64_t)(c4 * 4 + 1) * p.Ktot + k];
            w[k].z = p.w[(int64_t)(c4 * 4 + 2) * p.Ktot + k];
            w[k].w = p.w[(int64_t)(c4 * 4 + 3) * p.Ktot + k];
        } else {
            w[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    int dh[KMAX], dw[KMAX], dc[KMAX];   // filter-tap offsets of k, once per thread (no divisions in the pixel loop)
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int tap = k / p.Cin;
        dc[k] = k - tap * p.Cin;
        dh[k] = tap / p.ks - p.pad;
        dw[k] = tap - (tap / p.ks) * p.ks - p.pad;
    }
    const float4 b4 = p.bias ? *reinterpret_cast<const float4*>(p.bias + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t m_end = min((int64_t)p.M, ((int64_t)blockIdx.x + 1) * ppb);
    int64_t m = (int64_t)blockIdx.x * ppb + row;
    int nb = (int)(m / p.ohw);
    int oh = (int)(m - (int64_t)nb * p.ohw) / p.OW;
    int ow = (int)(m - (int64_t)nb * p.ohw) - oh * p.OW;
    for (; m < m_end; m += rpi, ow += rpi) {
        while (ow >= p.OW) {   // pixel coordinates advance incrementally: no division per pixel
            ow -= p.OW;
            if (++oh == p.OH) {
                oh = 0;
                ++nb;
            }
        }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* xb = p.x + (int64_t)nb * p.x_bs;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            int ih = oh * p.stride + dh[k], iw = ow * p.stride + dw[k];
            const bool ok = (k < p.Ktot) & ((unsigned)ih < (unsigned)p.IHg) & ((unsigned)iw < (unsigned)p.IWg);
            ih >>= p.ups;
            iw >>= p.ups;
            const float xv = ok ? xb[((int64_t)ih * p.W + iw) * p.Cin + dc[k]] : 0.f;
            acc.x = fmaf(xv, w[k].x, acc.x);
            acc.y = fmaf(xv, w[k].y, acc.y);
            acc.z = fmaf(xv, w[k].z, acc.z);
            acc.w = fmaf(xv, w[k].w, acc.w);
        }
        acc.x += b4.x; acc.y += b4.y; acc.z += b4.z; acc.w += b4.w;   // bias after the fma chain, like every other epilogue
        if (p.emb) {
            const float4 e = *reinterpret_cast<const float4*>(p.emb + (int64_t)nb * p.emb_stride + c4 * 4);
            acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
        }
        if (p.res) {
            const float4 e = *reinterpret_cast<const float4*>(p.res + m * p.Cout + c4 * 4);
            acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
        }
        *reinterpret_cast<float4*>(p.y + m * p.y_ld + c4 * 4) = acc;
        if (STATS) {
            const double a = acc.x, b = acc.y, c = acc.z, d = acc.w;
            ss[0] += a; qq[0] = fma(a, a, qq[0]);
            ss[1] += b; qq[1] = fma(b, b, qq[1]);
            ss[2] += c; qq[2] = fma(c, c, qq[2]);
            ss[3] += d; qq[3] = fma(d, d, qq[3]);
        }
    }
    if (STATS) {   // rows 1.. hand their sums to row 0, which adds them in row order (deterministic)
        if (row > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sm[row * p.Cout + c4 * 4 + e][0] = ss[e];
                sm[row * p.Cout + c4 * 4 + e][1] = qq[e];
            }
        }
        __syncthreads();
        if (row == 0) {
            for (int r = 1; r < rpi; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ss[e] += sm[r * p.Cout + c4 * 4 + e][0];
                    qq[e] += sm[r * p.Cout + c4 * 4 + e][1];
                }
            const int64_t m0 = (int64_t)blockIdx.x * ppb;
            const int n0 = (int)(m0 / p.ohw), chunk = (int)((m0 - (int64_t)n0 * p.ohw) / ppb);
            double* o = stats + (((int64_t)n0 * chunks + chunk) * p.Cout + c4 * 4) * 2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[2 * e] = ss[e];
                o[2 * e + 1] = qq[e];
            }
        }
    }
}

// Fully generic scalar fallback (odd channel counts; never on the hot configs).
__global__ __launch_bounds__(256) void conv_scalar_kernel(ConvP p) {
    const int64_t total = (int64_t)p.M * p.Cout;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / p.Cout;
        const int n = (int)(i - m * p.Cout);
        const int nb = (int)(m / p.ohw);
        const int r = (int)(m - (int64_t)nb * p.ohw);
        const int oh = r / p.OW, ow = r - oh * p.OW;
        float acc = 0.f;
        const float* wr = p.w + (int64_t)n * p.Ktot;
        for (int kh = 0; kh < p.ks; ++kh)
            for (int kw = 0; kw < p.ks; ++kw) {
                int ih = oh * p.stride - p.pad + kh, iw = ow * p.stride - p.pad + kw;
                if (!((unsigned)ih < (unsigned)p.IHg && (unsigned)iw < (unsigned)p.IWg)) continue;
                if (p.ups) {
                    ih >>= 1;
                    iw >>= 1;
                }
                const float* src = p.x + (int64_t)nb * p.x_bs + ((int64_t)ih * p.W + iw) * p.Cin;
                const float* wk = wr + (kh * p.ks + kw) * p.Cin;
                for (int ci = 0; ci < p.Cin; ++ci) acc = fmaf(src[ci], wk[ci], acc);
            }
        if (p.bias) acc += p.bias[n];
        if (p.emb) acc += p.emb[(int64_t)nb * p.emb_stride + n];
        if (p.res) acc += p.res[m * p.Cout + n];
        if (p.out_nchw)
            p.y[((int64_t)nb * p.Cout + n) * p.ohw + r] = acc;
        else
            p.y[m * p.y_ld + n] = acc;
    }
}

__global__ void pack_ohwi_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cout, int Cin, int kk) {
    const int64_t total = (int64_t)Cout * Cin * kk;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        // dst index: ((co*kk + t)*Cin + ci)
        const int ci = (int)(i % Cin);
        const int64_t r = i / Cin;
        const int t = (int)(r % kk);
        const int co = (int)(r / kk);
        dst[i] = src[((int64_t)co * Cin + ci) * kk + t];
    }
}

void pack_ohwi(const float* w_oihw, float* w_ohwi, int Cout, int Cin, int ks, hipStream_t s) {
    const int64_t total = (int64_t)Cout * Cin * ks * ks;
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(pack_ohwi_kernel, dim3(blocks), dim3(256), 0, s, w_oihw, w_ohwi, Cout, Cin, ks * ks);
    check_launch("pack_ohwi");
}

double conv2d_flops(const ConvArgs& a) {
    int OH, OW;
    conv_out_hw(a, &OH, &OW);
    return 2.0 * a.N * OH * OW * (double)a.Cout * a.ks * a.ks * a.Cin;
}

// what the launched kernel multiplies: the sub-pixel form does 4 of the 9 taps per output pixel (conv2d_flops stays the
// layer's algorithmic 3x3-over-the-upsampled-map count)
double conv2d_exec_flops(const ConvArgs& a) { return a.w_subpixel ? conv2d_flops(a) * 4.0 / 9.0 : conv2d_flops(a); }

// kernel variant: 0 = default (buffer-load kernel when eligible), 1 = force the flat-load kernel.
// ConvArgs.variant >= 0 wins, else env DSD_CONV_VARIANT, else 0.
static int conv_variant(const ConvArgs& a) {
    if (a.variant >= 0) return a.variant;
    static const int env = [] {
        const char* e = getenv("DSD_CONV_VARIANT");
        return e ? atoi(e) : 0;
    }();
    return env;
}

// Column-tile count NT (block tile = 128 x 32*NT) by a small cost model fitted to tools/bench_conv.py measurements:
//   time ~ ceil(blocks / (256 CUs x 2 resident)) x K-tiles x (t_fix + NT x t_mfma)
// t_fix = per-tile staging/barrier cycles that do not shrink with NT, t_mfma = matrix-pipe cycles per 32 columns per
// tile (fp32: 16 x 64, bf16x6: 12 x 32, bf16x3: 6 x 32).  Big layers get NT = 5 (weights and A staging amortised over the
// widest tile); small-M layers get narrower tiles so the grid still fills the chip.
static int pick_nt(int Cout, int tiles_m, int precision, int lanes = 1) {
    static const int force = [] {
        const char* e = getenv("DSD_FORCE_NT");   // experiments only
        return e ? atoi(e) : 0;
    }();
    if (force >= 1 && force <= 5) return force;
    const int t32 = cdiv(Cout, 32);
    const double t_fix = precision == PREC_F32 ? 500.0 : 700.0;
    const double t_mf = precision == PREC_F32 ? 1024.0 : (precision == PREC_BF16X6 ? 384.0 : 192.0);   // bf16x3 = f16x3
    int best = 1;
    double best_t = 1e300;
    for (int nt = 5; nt >= 1; --nt) {
        const int64_t blocks = (int64_t)tiles_m * cdiv(t32, nt) * std::max(1, lanes);   // (what shares the chip with this launch)
        const double t = (double)cdiv(blocks, 512) * (t_fix + nt * t_mf);
        if (t < best_t * 0.999) {
            best_t = t;
            best = nt;
        }
    }
    return best;
}

// pixels per workgroup of the first-layer kernel; with_stats: a divisor of OH*OW (one chunk of one sample), 0 = none suitable
static int direct_cols_ppb(const ConvArgs& a, int64_t M, int ohw, bool with_stats) {
    const int W4 = a.Cout / 4, rpi = 256 / W4;
    if (!with_stats) return std::max(rpi * 8, cdiv(cdiv(M, 8192), rpi) * rpi);
    for (int ppb = 128; ppb >= 16; ppb >>= 1)
        if (ohw % ppb == 0) return ppb;
    return 0;
}

// The one routing decision: which kernel conv2d() launches for `a`, with what tiling, and what that kernel can do for the
// caller.  replan = split-K scratch is available, so a grid that leaves CUs idle may be re-planned (conv2d_split_plan).
//   precision      the arithmetic that runs (PREC_F32 where the split kernels cannot take the problem)
//   nt, ksplit     column tile in 32-column units (MFMA and split kernels), split-K factor
//   structure      split kernels: 0 staged, 1 / 2 A-direct with 128 / 256-row tiles; -1 elsewhere
//   tap_reuse      the tap-reuse instantiation of the 256-row kernel
//   fuses_gn       the launch can apply GroupNorm + SiLU to its input itself (a.gn_scale / a.gn_shift)
//   stats_chunks   chunks per sample it can emit output statistics with (0 = it cannot: the caller runs gn_stats on the output)
//   scratch_bytes  split-K workspace it needs;  launches: kernels per call (2 = with the split-K reduction);  M = N * OH * OW
ConvRoute conv2d_route(const ConvArgs& a, bool replan) {
    ConvRoute r;
    conv_out_hw(a, &r.OH, &r.OW);
    r.M = (int64_t)a.N * r.OH * r.OW;
    const int ohw = r.OH * r.OW, Ktot = a.ks * a.ks * a.Cin;
    // split-bf16 arithmetic requested and usable for this problem?  (Until the A-direct kernel was software-pipelined, grids
    // of at most one block per CU were faster on the fp32 kernel and stayed there; now the 128-row A-direct kernel ties it in
    // bf16x6 and beats it in the 3-product modes on those layers — tools/bench_conv.py 0 31 30 with DSD_SHAPES=small.)
    r.precision = a.precision == PREC_F32 || !conv2d_split_eligible(a) ? PREC_F32 : a.precision;
    r.nt = pick_nt(a.Cout, cdiv(r.M, BM), r.precision, a.lanes);
    if (a.w_subpixel) {   // the caller built the phase weights because conv2d_subpixel_ok() chose this form: one kernel, one tile width
        r.family = CONV_SUBPIXEL;
        r.precision = PREC_BF16X6;
        r.nt = 5;
        r.structure = 2;
        r.tap_reuse = true;
        r.stats_chunks = conv2d_subpixel_shape_ok(a) ? 4 * a.H * a.W / (2 * BM) : 0;   // (phase, 256-pixel chunk)
        return r;
    }
    if (a.Cin % 4 != 0 || Ktot < 32) {   // small K: the first layers
        if (a.Cout % 4 == 0 && a.Cout / 4 <= 256 && Ktot <= 9 && !a.out_nchw && (!a.emb || a.emb_stride % 4 == 0)) {
            r.family = CONV_DIRECT_COLS;
            const int ppb = direct_cols_ppb(a, r.M, ohw, true);
            r.stats_chunks = ppb ? ohw / ppb : 0;
        } else {
            r.family = a.Cout % 4 == 0 && (size_t)Ktot * a.Cout * sizeof(float) <= DIRECT_LDS_MAX ? CONV_DIRECT_LDS : CONV_SCALAR;
        }
        return r;
    }
    if (r.precision == PREC_BF16X6 && conv2d_wino_eligible(a)) {
        r.family = CONV_WINO;
        r.stats_chunks = conv2d_wino_stats_chunks(a);
        return r;
    }
    if (r.precision == PREC_F32) {
        // buffer-load kernel when the operands are addressable with 32-bit byte offsets
        const int64_t x_bs = a.x_bs >= 0 ? a.x_bs : (int64_t)a.H * a.W * a.Cin;
        const int64_t xb = ((int64_t)(a.N - 1) * x_bs + (int64_t)a.H * a.W * a.Cin) * 4, wb = (int64_t)a.Cout * Ktot * 4;
        r.family = a.Cin % BK == 0 && xb < 0xFFFFFF00ll && wb < 0xFFFFFF00ll && conv_variant(a) == 0 ? CONV_MFMA_BUF : CONV_MFMA;
        return r;
    }
    r.family = CONV_SPLIT;
    // the plan a launch with scratch gets (p) and the one a launch without it gets (d): default structure and tile width, unsplit
    int nt_p, ks_p, ad_p, nt_d, ks_d, ad_d;
    conv2d_split_plan(a, r.nt, &nt_p, &ks_p, &ad_p, true);
    conv2d_split_plan(a, r.nt, &nt_d, &ks_d, &ad_d, false);
    r.nt = replan ? nt_p : nt_d;
    r.ksplit = replan ? ks_p : ks_d;
    r.structure = replan ? ad_p : ad_d;
    r.launches = r.ksplit > 1 ? 2 : 1;
    r.scratch_bytes = r.ksplit > 1 ? (size_t)r.ksplit * r.M * a.Cout * sizeof(float) : 0;
    r.tap_reuse = conv2d_split_tr(a, r.nt, r.ksplit, r.structure);   // tap reuse through LDS: an instantiation (kernel symbol) of its own
    // What the kernel offers the caller is answered for BOTH plans and granted only where they agree: the planner asks before it
    // knows whether scratch will be passed (none is when plan p does not split), and the answer decides what the network fuses.
    static const bool no_gn_fuse = getenv("DSD_NO_GN_FUSE") != nullptr;   // A/B
    r.fuses_gn = !no_gn_fuse && r.tap_reuse && conv2d_split_tr(a, nt_p, ks_p, ad_p);
    // statistics epilogue: not in the split-K form (the reduction kernel writes the output), not in the 128-row kernels with
    // >= 4 column tiles (no registers for it), and only when both plans tile the rows alike (the f = 8 VAE's 64x64 layers do not)
    const int rows = ad_p == 2 ? 2 * BM : BM;
    if (!a.out_nchw && ks_p == 1 && ad_d == ad_p && !(ad_p == 1 && (nt_p >= 4 || nt_d >= 4)) && ohw % rows == 0) r.stats_chunks = ohw / rows;
    return r;
}

// The 256-row A-direct kernel keeps the plain name; the other structures, split-K runs, tap reuse and the instantiation that
// also applies GroupNorm + SiLU to its input (gn_applied) are kinds of their own, so that a kind's average launch time is one
// kernel's (bench.py roofline vs the rocprofv3 kernel trace)
const char* conv2d_route_name(const ConvRoute& r, bool gn_applied) {
    switch (r.family) {
        case CONV_DIRECT_COLS: return "conv_direct_cols";
        case CONV_DIRECT_LDS: return "conv_direct_lds";
        case CONV_SCALAR: return "conv_scalar";
        case CONV_SUBPIXEL: return "conv_bf16x6<5>/tr+subpixel";
        case CONV_WINO: return "conv_wino_bf16x6";
        default: break;
    }
    static const char* base[4] = {"conv_mfma", "conv_bf16x3", "conv_bf16x6", "conv_f16x3"};
    static std::string pool[4][6][4][2][2][2];
    const int ad = r.family == CONV_SPLIT ? r.structure : 3;
    const bool gn = r.tap_reuse && gn_applied;
    std::string& n = pool[r.precision][r.nt][ad][r.ksplit > 1][r.tap_reuse][gn];
    if (n.empty())
        n = std::string(base[r.precision]) + "<" + std::to_string(r.nt) + ">" + (ad >= 2 ? "" : (ad == 1 ? "/r128" : "/staged")) +
            (r.ksplit > 1 ? "+splitk" : "") + (r.tap_reuse ? "/tr" : "") + (gn ? "+gn" : "");
    return n.c_str();
}

template <int NT> static void launch_mfma(bool buf, dim3 grid, hipStream_t s, const ConvP& p) {
    if (buf)
        hipLaunchKernelGGL(conv_mfma_buf_kernel<NT>, grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(conv_mfma_kernel<NT>, grid, dim3(256), 0, s, p);
}

void conv2d(ConvArgs a, hipStream_t s) {
    DSD_CHECK(a.ks == 1 || a.ks == 3, "conv2d: kernel size %d unsupported", a.ks);
    DSD_CHECK(a.stride == 1 || a.stride == 2, "conv2d: stride %d unsupported", a.stride);
    const ConvRoute r = conv2d_route(a, a.scratch != nullptr);   // a caller without scratch (never the planned graph) gets the unsplit configuration
    DSD_CHECK(a.gn_scale == nullptr || r.fuses_gn, "conv2d: GroupNorm coefficients given, but this problem does not run on the kernel that applies them");
    DSD_CHECK(r.M < (1ll << 31) && r.M * std::max(a.Cout, a.Cin) < (1ll << 40), "conv2d: problem too large");
    if (r.M == 0 || a.Cout == 0) return;
    if (r.family == CONV_SUBPIXEL) return conv2d_subpixel(a, s);
    if (r.family == CONV_WINO) return conv2d_wino(a, s);
    if (r.family == CONV_SPLIT) return conv2d_split(a, r.nt, r.ksplit, r.structure, s);
    ConvP p{};
    p.x = a.x; p.w = a.w; p.bias = a.bias; p.emb = a.emb; p.res = a.res; p.y = a.y;
    p.N = a.N; p.H = a.H; p.W = a.W; p.Cin = a.Cin; p.Cout = a.Cout; p.ks = a.ks; p.stride = a.stride;
    p.y_ld = a.y_ld > 0 ? a.y_ld : a.Cout;
    p.pad = a.pad_lo >= 0 ? a.pad_lo : a.ks / 2; p.ups = a.ups; p.emb_stride = a.emb_stride; p.out_nchw = a.out_nchw;
    p.x_bs = a.x_bs >= 0 ? a.x_bs : (int64_t)a.H * a.W * a.Cin;
    p.IHg = a.ups ? a.H * 2 : a.H;
    p.IWg = a.ups ? a.W * 2 : a.W;
    p.OH = r.OH; p.OW = r.OW;
    p.ohw = p.OH * p.OW;
    p.M = (int)r.M;
    p.Ktot = a.ks * a.ks * a.Cin;
    p.cchunks = cdiv(a.Cin, BK);
    p.tiles_m = cdiv(p.M, BM);
    if (r.family == CONV_DIRECT_COLS) {
        const int W4 = a.Cout / 4, rpi = 256 / W4;
        if (a.stats) {
            const int ppb = direct_cols_ppb(a, p.M, p.ohw, true);
            DSD_CHECK(ppb > 0 && r.stats_chunks == a.stats_chunks, "conv2d: statistics chunks %d do not match this launch", a.stats_chunks);
            hipLaunchKernelGGL((conv_direct_cols_kernel<9, true>), dim3(p.M / ppb), dim3(rpi * W4), 0, s, p, W4, ppb, a.stats, a.stats_chunks);
        } else {
            const int ppb = direct_cols_ppb(a, p.M, p.ohw, false);
            hipLaunchKernelGGL((conv_direct_cols_kernel<9, false>), dim3(cdiv(p.M, ppb)), dim3(rpi * W4), 0, s, p, W4, ppb, nullptr, 0);
        }
        check_launch("conv_direct_cols");
    } else if (r.family == CONV_DIRECT_LDS) {
        // (beyond the 64 KB default the dynamic LDS size has to be allowed once per process; the latent U-Net's first layer,
        // 6 -> 320 channels, needs 69 KB and used to fall to the scalar kernel: ~1 ms per evaluation)
        static const hipError_t lds_attr = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_direct_lds_kernel),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)DIRECT_LDS_MAX);
        DSD_CHECK(lds_attr == hipSuccess, "hipFuncSetAttribute(conv_direct_lds_kernel): %s", hipGetErrorString(lds_attr));
        hipLaunchKernelGGL(conv_direct_lds_kernel, dim3(cdiv(p.M, 64)), dim3(256), (size_t)p.Ktot * a.Cout * sizeof(float), s, p);
        check_launch("conv_direct_lds");
    } else if (r.family == CONV_SCALAR) {
        const int blocks = (int)std::min<int64_t>(((int64_t)p.M * a.Cout + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(conv_scalar_kernel, dim3(blocks), dim3(256), 0, s, p);
        check_launch("conv_scalar");
    } else {   // fp32 MFMA
        const bool buf = r.family == CONV_MFMA_BUF;
        p.tiles_n = cdiv(a.Cout, r.nt * 32);
        p.x_bytes = buf ? (unsigned)((((int64_t)(a.N - 1) * p.x_bs + (int64_t)a.H * a.W * a.Cin)) * 4) : 0;
        p.w_bytes = buf ? (unsigned)((int64_t)a.Cout * p.Ktot * 4) : 0;
        const dim3 grid((unsigned)(p.tiles_m * p.tiles_n));
        switch (r.nt) {
            case 1: launch_mfma<1>(buf, grid, s, p); break;
            case 2: launch_mfma<2>(buf, grid, s, p); break;
            case 3: launch_mfma<3>(buf, grid, s, p); break;
            case 4: launch_mfma<4>(buf, grid, s, p); break;
            default: launch_mfma<5>(buf, grid, s, p); break;
        }
        check_launch(buf ? "conv_mfma_buf" : "conv_mfma");
    }
}

}  // namespace dsd
