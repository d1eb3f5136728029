// contrast.hip — the disentanglement losses over the bottleneck heads (content / style / anatomy / lesion).
//
// training_project/utils/gaussian_diffusion.py:907-975 (training_losses(disentangle=)), :1056-1094 (get_disentangle_loss),
// loss_function/contrastive_loss.py (ContrastiveLoss, contrast_mode 'all', method 'cl') and the p = 1 form of
// trainers/trainer_ds_diff.py:341-354, forward only.  R = n_views*B feature rows of n elements, row r = view*B + b
// (torch.cat(torch.unbind(features, 1), 0)).
//
// Pass 1 forms the R x R matrix of fp64 dot products (or of L1 distances) where the reference materialises an R x R x n
// broadcast: a workgroup owns a 128 x 128 tile of the matrix and one slice of n, stages 32 elements of its rows in LDS at a time
// and keeps an 8 x 8 patch of fp64 sums per thread.  Up to R = 128 (seven views at batch 16 is 112) one tile is the matrix and
// every feature element is read from memory once; above it the 2 x 2 tiles each read their own rows.  Products of fp32 values
// are exact in fp64, so the squared distance G_ii + G_jj - 2 G_ij only loses what the fp64 sums lose.  Every workgroup writes
// its patch to part[slice][R][R]; contrast_reduce adds the slices in index order.  No atomics: two runs agree bit for bit.
// Pass 2 (one workgroup, thread i = row i) turns the matrix and the labels into the loss and the fp32 logits.
#include "../../include/dsdiff.h"
#include "kernels.h"

namespace dsd {

static_assert(DSD_CONTRAST_MAX_VIEWS == 8, "ContrastRows::v");
static constexpr int kCtTile = 128;          // rows (and columns) of the matrix one workgroup owns
static constexpr int kCtK = 32;              // elements of n staged per step
static constexpr int kCtLd = kCtTile + 1;    // LDS row pitch of the [k][row] staging (odd: the transposing store is conflict-free)
static constexpr int kCtSlices = 64;         // at most this many slices of n (the partials are slices * R * R doubles)

static int ct_slice(int64_t n) {
    const int64_t per = (n + kCtSlices - 1) / kCtSlices;
    return (int)((per + kCtK - 1) / kCtK * kCtK);
}
static int ct_nslice(int64_t n) { return (int)((n + ct_slice(n) - 1) / ct_slice(n)); }

size_t contrast_part_doubles(int R, int64_t n) { return ((size_t)ct_nslice(n) + 1) * R * R; }

// element k of feature row r (zero outside the matrix and past n: both metrics add nothing there)
__device__ __forceinline__ float ct_load(const ContrastRows& a, int B, int R, int n, int r, int k) {
    if (r >= R || k >= n) return 0.f;
    const int view = r / B, b = r - view * B;
    const float* p = a.v[0];
#pragma unroll
    for (int q = 1; q < DSD_CONTRAST_MAX_VIEWS; ++q)     // (a select chain: a dynamic index into the argument would go through scratch)
        if (view == q) p = a.v[q];
    return p[(int64_t)b * a.bs + k];
}

// L1 false: part[slice][i][j] = sum over the slice of x_i[k] * x_j[k];  L1 true: of |x_i[k] - x_j[k]|
template <bool L1>
__global__ __launch_bounds__(256) void contrast_gram_kernel(ContrastRows a, int B, int R, int n, int slice) {
    __shared__ float sA[kCtK * kCtLd];
    __shared__ float sB[kCtK * kCtLd];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * kCtTile, j0 = blockIdx.z * kCtTile;
    const bool diag = blockIdx.y == blockIdx.z;
    const int k0 = blockIdx.x * slice, k1 = min(n, k0 + slice);
    const float* pb = diag ? sA : sB;
    double acc[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;
    for (int kk = k0; kk < k1; kk += kCtK) {
        __syncthreads();
        for (int idx = tid; idx < kCtTile * kCtK; idx += 256) {
            const int r = idx / kCtK, k = idx % kCtK;
            sA[k * kCtLd + r] = ct_load(a, B, R, n, i0 + r, kk + k);
            if (!diag) sB[k * kCtLd + r] = ct_load(a, B, R, n, j0 + r, kk + k);
        }
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < kCtK; ++k) {
            double av[8], bv[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                av[p] = (double)sA[k * kCtLd + ty + 16 * p];
                bv[p] = (double)pb[k * kCtLd + tx + 16 * p];
            }
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (L1)
                        acc[p][q] += fabs(av[p] - bv[q]);
                    else
                        acc[p][q] = fma(av[p], bv[q], acc[p][q]);
                }
        }
    }
    double* dst = a.part + (size_t)blockIdx.x * R * R;
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
            if (i < R && j < R) dst[(size_t)i * R + j] = acc[p][q];
        }
}

// G[i][j] = part[0][i][j] + part[1][i][j] + ... in index order
__global__ __launch_bounds__(256) void contrast_reduce_kernel(const double* __restrict__ part, int nslice, int rr, double* __restrict__ G) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rr) return;
    double s = 0.0;
    for (int p = 0; p < nslice; ++p) s += part[(size_t)p * rr + idx];
    G[idx] = s;
}

// One workgroup; thread i owns row i of the matrix.  Sums run in fp64 over the fp32 logits the reference forms (and returns) and
// are rounded where the reference holds an fp32 scalar.
//   cl (contrastive_loss.py:98-131): logits = cos / temperature (:98-100); the diagonal leaves the sum of exp(logits) and the
//       positives (logits_mask :105-111); log_prob = logits - log(sum) with no max subtracted (cal_log_prob :139-142);
//       mean_log_prob_pos = sum(mask * log_prob) / (sum(mask) + 1e-6) (:116); loss = -mean over the rows (:120-121, the factor
//       temperature / base_temperature of the module is 0.1 / 0.1 whatever the call passes).
//   eu (gaussian_diffusion.py:1060-1075): logits = float(cdist64) / n (:1066-1067); numerator over same label without the
//       diagonal, denominator over different labels (:1072-1073); loss = numerator / denominator; returned logits * 2 - 1.
//   eu&cl (:1076-1092): loss_eu + 0.05 * loss_cl, the cosine logits returned.   l1 (trainer_ds_diff.py:341-354): eu on L1 / n.
__global__ __launch_bounds__(256) void contrast_loss_kernel(const double* __restrict__ G, const int32_t* __restrict__ labels, int R, int n,
                                                            int mode, float temperature, float* loss, float* logits) {
    __shared__ double red[3 * 256];
    const int i = threadIdx.x;
    double s_cl = 0.0, s_num = 0.0, s_den = 0.0;
    if (i < R) {
        const int li = labels[i];
        const double gii = G[(size_t)i * R + i];
        float* row = logits + (size_t)i * R;
        if (mode == DSD_CONTRAST_CL || mode == DSD_CONTRAST_EU_CL) {
            const double ni = fmax(sqrt(gii), 1e-8);                      // CosineSimilarity(dim=-1, eps=1e-8)
            double se = 0.0;
            for (int j = 0; j < R; ++j) {
                const double nj = fmax(sqrt(G[(size_t)j * R + j]), 1e-8);
                const float c = (float)(G[(size_t)i * R + j] / (ni * nj));
                const float lg = c / temperature;
                row[j] = lg;
                if (j != i) se += exp((double)lg);
            }
            const double lse = log(se);
            double sp = 0.0;
            int np = 0;
            for (int j = 0; j < R; ++j)
                if (j != i && labels[j] == li) {
                    sp += (double)row[j] - lse;
                    ++np;
                }
            s_cl = sp / (double)((float)np + 1e-6f);                      // the mask is fp32 (:63), and so is mask.sum(1) + 1e-6
        }
        if (mode != DSD_CONTRAST_CL) {
            for (int j = 0; j < R; ++j) {
                const double g = G[(size_t)i * R + j];
                const double d = mode == DSD_CONTRAST_L1 ? g : sqrt(fmax(gii + G[(size_t)j * R + j] - 2.0 * g, 0.0));
                const float lg = (float)d / (float)n;
                if (labels[j] != li)
                    s_den += (double)lg;
                else if (j != i)
                    s_num += (double)lg;
                if (mode == DSD_CONTRAST_EU) row[j] = lg * 2.f - 1.f;
                if (mode == DSD_CONTRAST_L1) row[j] = lg;
            }
        }
    }
    red[i] = s_cl; red[256 + i] = s_num; red[512 + i] = s_den;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (i < w) {
            red[i] += red[i + w]; red[256 + i] += red[256 + i + w]; red[512 + i] += red[512 + i + w];
        }
        __syncthreads();
    }
    if (i == 0) {
        const float l_cl = (float)(-(red[0] / (double)R));
        const float l_eu = (float)red[256] / (float)red[512];
        loss[0] = mode == DSD_CONTRAST_CL ? l_cl : mode == DSD_CONTRAST_EU_CL ? l_eu + 0.05f * l_cl : l_eu;
    }
}

void contrast_check(int n_views, int B, int64_t n, int mode, float temperature) {
    DSD_CHECK(mode >= DSD_CONTRAST_CL && mode <= DSD_CONTRAST_L1, "contrast_rows: unknown mode %d (DSD_CONTRAST_CL / _EU / _EU_CL / _L1)", mode);
    DSD_CHECK(n_views >= 1 && n_views <= DSD_CONTRAST_MAX_VIEWS, "contrast_rows takes 1 to %d views, got %d", DSD_CONTRAST_MAX_VIEWS, n_views);
    DSD_CHECK(B >= 1 && n >= 1, "contrast_rows: bad shape: B %d n %lld", B, (long long)n);
    DSD_CHECK(n <= (int64_t)1 << 30, "contrast_rows: one row has %lld elements; up to 2^30 are taken", (long long)n);
    DSD_CHECK((int64_t)n_views * B >= 2 && (int64_t)n_views * B <= DSD_CONTRAST_MAX_ROWS,
              "contrast_rows: %d views of %d samples are %lld rows; 2 to %d are taken", n_views, B, (long long)n_views * B, DSD_CONTRAST_MAX_ROWS);
    const bool cosine = mode == DSD_CONTRAST_CL || mode == DSD_CONTRAST_EU_CL;
    DSD_CHECK(!cosine || temperature > 0.f, "contrast_rows: the cosine modes divide by the temperature, got %g", (double)temperature);
}

void contrast_rows(const ContrastRows& arg, int n_views, int B, int64_t n, int mode, float temperature, hipStream_t s) {
    ContrastRows a = arg;
    contrast_check(n_views, B, n, mode, temperature);
    for (int i = 0; i < n_views; ++i) DSD_CHECK(a.v[i], "contrast_rows: view %d is null", i);
    DSD_CHECK(a.labels && a.part && a.loss && a.logits, "contrast_rows: null argument");
    if (a.bs <= 0) a.bs = n;
    DSD_CHECK(a.bs >= n, "contrast_rows: rows of %lld elements in a stride of %lld", (long long)n, (long long)a.bs);
    const int R = n_views * B, slice = ct_slice(n), nslice = ct_nslice(n), tiles = (R + kCtTile - 1) / kCtTile;
    const dim3 grid(nslice, tiles, tiles);
    if (mode == DSD_CONTRAST_L1)
        hipLaunchKernelGGL(contrast_gram_kernel<true>, grid, dim3(256), 0, s, a, B, R, (int)n, slice);
    else
        hipLaunchKernelGGL(contrast_gram_kernel<false>, grid, dim3(256), 0, s, a, B, R, (int)n, slice);
    check_launch("contrast_gram");
    double* G = a.part + (size_t)nslice * R * R;
    hipLaunchKernelGGL(contrast_reduce_kernel, dim3((R * R + 255) / 256), dim3(256), 0, s, a.part, nslice, R * R, G);
    check_launch("contrast_reduce");
    hipLaunchKernelGGL(contrast_loss_kernel, dim3(1), dim3(256), 0, s, G, a.labels, R, (int)n, mode, temperature, a.loss, a.logits);
    check_launch("contrast_loss");
}

}  // namespace dsd
