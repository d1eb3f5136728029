// disc.hip — the bottleneck head of UNet_disc_Model (Disc_diff/guided_diffusion/unet.py:1015-1033): from the eight
// pre-activation outputs of conv_common / conv_distinct (four streams each) to the [B, HW, 5*half] concat buffer that
// dim_reduction_non_zeros reads.
//
//   com_i  = SiLU(common_i)                       dist_i = SE_dist_i(SiLU(distinct_i))
//   com    = SE_com(mean_i com_i)                 cat    = [com, dist_1, dist_2, dist_3, dist_4]
//   SE(v)  = v * sigmoid(W2 relu(W1 avgpool(v)))  (unet.py:82-109, bias-free linears)
//
// Three launches over (pixel chunk, branch 0..4, sample); branch 0 is the common one, whose value is the four-stream mean:
//   pool   per-chunk sums of the activated values, fp64, written (never accumulated) to part[n][branch][chunk][half]
//   gate   adds the chunks in index order, pooled -> W1 -> relu -> W2 -> sigmoid, one workgroup per (branch, sample)
//   scale  value * gate into the branch's channel slice of cat (and, on request, the eight feature tensors)
// No atomics and a fixed summation order everywhere: two runs are bit-identical.  All global accesses are 16 bytes wide
// (half % 4 == 0); the activated values are recomputed by the scale pass instead of stored (one expf against 4 bytes through HBM).
#include "device_common.h"

namespace dsd {

namespace {

__device__ __forceinline__ float4 silu4(float4 v) { return make_float4(silu_f(v.x), silu_f(v.y), silu_f(v.z), silu_f(v.w)); }

// what the kernels read of DiscArgs (by value: no array is indexed with a run-time value, so nothing lands in scratch)
struct DiscK {
    const float4 *c0, *c1, *c2, *c3, *d0, *d1, *d2, *d3;
    int HW, half, ppc, nchunk;
};

// activated value of branch br at float4 index i of a [B][HW][half] tensor; branch 0: mean of the four activated commons
__device__ __forceinline__ float4 disc_value(const DiscK& a, int br, int64_t i) {
    if (br == 0) {
        const float4 v0 = silu4(a.c0[i]), v1 = silu4(a.c1[i]), v2 = silu4(a.c2[i]), v3 = silu4(a.c3[i]);
        return make_float4((((v0.x + v1.x) + v2.x) + v3.x) * 0.25f, (((v0.y + v1.y) + v2.y) + v3.y) * 0.25f,
                           (((v0.z + v1.z) + v2.z) + v3.z) * 0.25f, (((v0.w + v1.w) + v2.w) + v3.w) * 0.25f);
    }
    const float4* d = br == 1 ? a.d0 : (br == 2 ? a.d1 : (br == 3 ? a.d2 : a.d3));
    return silu4(d[i]);
}

// grid (nchunk, 5, B).  Threads form `rows` pixel rows of TW float4 columns; the rows' sums meet in LDS and are added in row order.
__global__ __launch_bounds__(256) void disc_pool_kernel(DiscK a, double* __restrict__ part) {
    __shared__ double sm[256 * 4];
    const int chunk = blockIdx.x, br = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const int cols = a.half >> 2;
    const int TW = cols < 256 ? cols : 256, rows = 256 / TW;
    const int tc = tid % TW, tr = tid / TW;
    const int p0 = chunk * a.ppc, p1 = min(p0 + a.ppc, a.HW);
    const int64_t base = (int64_t)n * a.HW * cols;
    double* out = part + (((int64_t)n * 5 + br) * a.nchunk + chunk) * a.half;
    for (int c0 = 0; c0 < cols; c0 += TW) {   // (one trip unless half > 1024)
        const int c4 = c0 + tc;
        double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
        if (tr < rows && c4 < cols)
            for (int p = p0 + tr; p < p1; p += rows) {
                const float4 v = disc_value(a, br, base + (int64_t)p * cols + c4);
                sx += (double)v.x; sy += (double)v.y; sz += (double)v.z; sw += (double)v.w;
            }
        sm[tid * 4 + 0] = sx; sm[tid * 4 + 1] = sy; sm[tid * 4 + 2] = sz; sm[tid * 4 + 3] = sw;
        __syncthreads();
        if (tr == 0 && c4 < cols) {
            for (int r = 1; r < rows; ++r) {
                const double* q = sm + (r * TW + tc) * 4;
                sx += q[0]; sy += q[1]; sz += q[2]; sw += q[3];
            }
            double* o = out + c4 * 4;
            o[0] = sx; o[1] = sy; o[2] = sz; o[3] = sw;
        }
        __syncthreads();
    }
}

struct DiscW {
    const float *w1_0, *w1_1, *w1_2, *w1_3, *w1_4;   // [Cr][half]
    const float *w2_0, *w2_1, *w2_2, *w2_3, *w2_4;   // [half][Cr]
};

// grid (5, B); dynamic LDS: pooled[half], hid[Cr]
__global__ __launch_bounds__(256) void disc_gate_kernel(const double* __restrict__ part, DiscW w, int HW, int half, int Cr, int nchunk,
                                                        float* __restrict__ gate) {
    extern __shared__ float gsm[];
    float* pooled = gsm;
    float* hid = gsm + half;
    const int br = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* w1 = br == 0 ? w.w1_0 : (br == 1 ? w.w1_1 : (br == 2 ? w.w1_2 : (br == 3 ? w.w1_3 : w.w1_4)));
    const float* w2 = br == 0 ? w.w2_0 : (br == 1 ? w.w2_1 : (br == 2 ? w.w2_2 : (br == 3 ? w.w2_3 : w.w2_4)));
    const double* pp = part + ((int64_t)n * 5 + br) * nchunk * half;
    for (int c = tid; c < half; c += 256) {
        double s = 0.0;
        for (int k = 0; k < nchunk; ++k) s += pp[(int64_t)k * half + c];
        pooled[c] = (float)(s / (double)HW);
    }
    __syncthreads();
    for (int j = wave; j < Cr; j += 4) {   // one wave per hidden unit: lanes stride the channels, butterfly sum (fixed order)
        float s = 0.f;
        for (int c = lane; c < half; c += 64) s = fmaf(w1[(int64_t)j * half + c], pooled[c], s);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) hid[j] = fmaxf(s, 0.f);
    }
    __syncthreads();
    float* g = gate + ((int64_t)n * 5 + br) * half;
    for (int c = tid; c < half; c += 256) {
        float s = 0.f;
        for (int j = 0; j < Cr; ++j) s = fmaf(w2[(int64_t)c * Cr + j], hid[j], s);
        g[c] = 1.f / (1.f + expf(-s));
    }
}

struct DiscF {
    float4 *f0, *f1, *f2, *f3, *f4, *f5, *f6, *f7;   // com_h1..4 (after SiLU), dist_h1..4 (after their SE); all null: not wanted
};

// grid (nchunk, 5, B)
__global__ __launch_bounds__(256) void disc_scale_kernel(DiscK a, const float* __restrict__ gate, float* __restrict__ cat, DiscF f) {
    const int chunk = blockIdx.x, br = blockIdx.y, n = blockIdx.z;
    const int cols = a.half >> 2;
    const int p0 = chunk * a.ppc, p1 = min(p0 + a.ppc, a.HW);
    const int64_t base = (int64_t)n * a.HW * cols;
    const float4* g4 = reinterpret_cast<const float4*>(gate + ((int64_t)n * 5 + br) * a.half);
    const int total = (p1 - p0) * cols;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int pl = i / cols, c4 = i - pl * cols;
        const int64_t p = (int64_t)n * a.HW + p0 + pl;          // pixel index over the batch
        const int64_t idx = base + (int64_t)(p0 + pl) * cols + c4;
        const float4 g = g4[c4];
        float4 v;
        if (br == 0 && f.f0) {   // the four activated commons are outputs of their own
            const float4 v0 = silu4(a.c0[idx]), v1 = silu4(a.c1[idx]), v2 = silu4(a.c2[idx]), v3 = silu4(a.c3[idx]);
            f.f0[idx] = v0; f.f1[idx] = v1; f.f2[idx] = v2; f.f3[idx] = v3;
            v = make_float4((((v0.x + v1.x) + v2.x) + v3.x) * 0.25f, (((v0.y + v1.y) + v2.y) + v3.y) * 0.25f,
                            (((v0.z + v1.z) + v2.z) + v3.z) * 0.25f, (((v0.w + v1.w) + v2.w) + v3.w) * 0.25f);
        } else {
            v = disc_value(a, br, idx);
        }
        v.x *= g.x; v.y *= g.y; v.z *= g.z; v.w *= g.w;
        *reinterpret_cast<float4*>(cat + p * (5 * (int64_t)a.half) + (int64_t)br * a.half + c4 * 4) = v;
        if (br > 0 && f.f0) {
            float4* fd = br == 1 ? f.f4 : (br == 2 ? f.f5 : (br == 3 ? f.f6 : f.f7));
            fd[idx] = v;
        }
    }
}

}  // namespace

// pixels per chunk: at least 64, at most 32 chunks per sample (a function of HW alone: the summation order never depends on the batch)
static int disc_ppc(int HW) { return std::max(64, cdiv(HW, 32)); }
int disc_nchunks(int HW) { return cdiv(HW, disc_ppc(HW)); }

bool disc_unfused_env() {
    const char* e = getenv("DSD_DISC_UNFUSED");   // A/B and cross-check: the head composed from avg_into / se_scale / concat copies
    return e != nullptr && e[0] != 0 && e[0] != '0';
}

size_t disc_scratch_bytes(int B, int HW, int half, bool unfused) {
    if (unfused) return (size_t)6 * B * HW * half * sizeof(float);   // four activated commons, their mean, one SE result
    const size_t part = (size_t)B * 5 * disc_nchunks(HW) * half * sizeof(double);
    return part + (size_t)B * 5 * half * sizeof(float);
}

static void disc_check(const DiscArgs& a) {
    DSD_CHECK(a.B >= 1 && a.HW >= 1 && a.half >= 4 && a.Cr >= 1, "disc bottleneck: bad shape (B %d, HW %d, half %d, Cr %d)", a.B, a.HW, a.half, a.Cr);
    DSD_CHECK(a.half % 4 == 0, "disc bottleneck: half = %d is not a multiple of 4 (the kernels move 16 bytes per access)", a.half);
    DSD_CHECK((int64_t)a.B * a.HW * a.half < ((int64_t)1 << 40), "disc bottleneck: tensor too large");
    for (int i = 0; i < 4; ++i) DSD_CHECK(a.com[i] && a.dist[i], "disc bottleneck: null input");
    for (int i = 0; i < 5; ++i) DSD_CHECK(a.w1[i] && a.w2[i], "disc bottleneck: null SE weight");
    DSD_CHECK(a.cat && a.scratch, "disc bottleneck: null output / scratch");
    bool any = false, all = true;
    for (int i = 0; i < 8; ++i) { any |= a.feat[i] != nullptr; all &= a.feat[i] != nullptr; }
    DSD_CHECK(!any || all, "disc bottleneck: the eight feature outputs come together or not at all");
}

void disc_bottleneck(const DiscArgs& a, hipStream_t s) {
    disc_check(a);
    DiscK k;
    k.c0 = (const float4*)a.com[0]; k.c1 = (const float4*)a.com[1]; k.c2 = (const float4*)a.com[2]; k.c3 = (const float4*)a.com[3];
    k.d0 = (const float4*)a.dist[0]; k.d1 = (const float4*)a.dist[1]; k.d2 = (const float4*)a.dist[2]; k.d3 = (const float4*)a.dist[3];
    k.HW = a.HW; k.half = a.half; k.ppc = disc_ppc(a.HW); k.nchunk = disc_nchunks(a.HW);
    double* part = reinterpret_cast<double*>(a.scratch);
    float* gate = reinterpret_cast<float*>(part + (size_t)a.B * 5 * k.nchunk * a.half);
    DiscW w{a.w1[0], a.w1[1], a.w1[2], a.w1[3], a.w1[4], a.w2[0], a.w2[1], a.w2[2], a.w2[3], a.w2[4]};
    DiscF f{(float4*)a.feat[0], (float4*)a.feat[1], (float4*)a.feat[2], (float4*)a.feat[3],
            (float4*)a.feat[4], (float4*)a.feat[5], (float4*)a.feat[6], (float4*)a.feat[7]};
    const dim3 grid(k.nchunk, 5, a.B);
    hipLaunchKernelGGL(disc_pool_kernel, grid, dim3(256), 0, s, k, part);
    check_launch("disc_pool");
    const size_t lds = (size_t)(a.half + a.Cr) * sizeof(float);
    DSD_CHECK(lds <= 48 * 1024, "disc bottleneck: half = %d does not fit the gate kernel's LDS", a.half);
    hipLaunchKernelGGL(disc_gate_kernel, dim3(5, a.B), dim3(256), lds, s, part, w, a.HW, a.half, a.Cr, k.nchunk, gate);
    check_launch("disc_gate");
    hipLaunchKernelGGL(disc_scale_kernel, grid, dim3(256), 0, s, k, gate, a.cat, f);
    check_launch("disc_scale");
}

// the same head from the library's existing ops: SiLU copies, four-way mean, se_scale (one workgroup per sample), concat copies
void disc_bottleneck_unfused(const DiscArgs& a, hipStream_t s) {
    disc_check(a);
    const int64_t px = (int64_t)a.B * a.HW, n = px * a.half;
    float* tmp = reinterpret_cast<float*>(a.scratch);
    float* ca[4];
    for (int i = 0; i < 4; ++i) {
        ca[i] = a.feat[0] ? a.feat[i] : tmp + i * n;
        avg_into(a.com[i], nullptr, nullptr, nullptr, 1.f, px, a.half, ca[i], a.half, 0, ACT_SILU, s);
    }
    float* mean = tmp + 4 * n;
    float* se = tmp + 5 * n;
    avg_into(ca[0], ca[1], ca[2], ca[3], 4.f, px, a.half, mean, a.half, 0, ACT_NONE, s);
    se_scale(mean, a.B, a.HW, a.half, a.w1[0], a.w2[0], a.Cr, se, s);
    avg_into(se, nullptr, nullptr, nullptr, 1.f, px, a.half, a.cat, 5 * a.half, 0, ACT_NONE, s);
    for (int i = 0; i < 4; ++i) {
        avg_into(a.dist[i], nullptr, nullptr, nullptr, 1.f, px, a.half, mean, a.half, 0, ACT_SILU, s);
        float* d = a.feat[0] ? a.feat[4 + i] : se;
        se_scale(mean, a.B, a.HW, a.half, a.w1[1 + i], a.w2[1 + i], a.Cr, d, s);
        avg_into(d, nullptr, nullptr, nullptr, 1.f, px, a.half, a.cat, 5 * a.half, (1 + i) * a.half, ACT_NONE, s);
    }
}

}  // namespace dsd
