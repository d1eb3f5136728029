// metrics.hip — the validation metrics of a batch of samples: MAE / MSE sums, Gaussian SSIM and the MS-SSIM scale table.
//
// MONAI's MAEMetric and SSIMMetric(spatial_dims=2) as every trainer's validation_step calls them (trainers/trainer_ddpm.py:501-565,
// trainers/trainer_use_gaussian_diff.py:99-102,519-584) and torchmetrics' MS-SSIM per axial slice of the inference metric table
// (inference/test_metrics.py:249-274), forward only.  pred / target are fp32 [B,C,H,W]; everything from the load onward is fp64:
// with an fp32 window E[x^2] - m^2 of a 12-bit image (mean 2048, std 400) keeps four digits, and a pyramid stored as fp32 does
// not reach the 1e-10 the tests ask for either.
//
//   elem pass    grid (pieces of 2048 elements, B): sum |p - t|, sum (p - t)^2, min / max of t and of p -> part[b][piece][6];
//                the finalize adds the pieces in a fixed order into elem[b][6] and writes the sample's c1 = (0.01 R)^2 and
//                c2 = (0.03 R)^2, R the fixed data range or (R = 0) max(max p - min p, max t - min t) of THAT sample.
//   pool         scale s + 1 = 2x2 average of scale s, a trailing odd row / column dropped (F.avg_pool2d), stored as fp64.
//   map          a workgroup owns 32 x 16 outputs of one channel: the 42 x 26 inputs go to LDS as fp64 (the optional pre-transform
//                applied once, at this load), the row blur of x, y, xx, yy, xy into five 32 x 26 planes, then the column blur, the
//                two maps, a fixed LDS fold -> part[b][tile][2].  About 55 KB of LDS, two to three workgroups per CU.
//   finalize     adds the tiles of (b, scale) in a fixed order and divides by C * (H - 10) * (W - 10).
// No atomics anywhere: two calls agree bit for bit.
#include "../../include/dsdiff.h"
#include "kernels.h"

#include <cmath>

namespace dsd {

static constexpr int kMtWin = 11;                  // taps of the window
static constexpr int kMtHalo = kMtWin - 1;
static constexpr int kMtIW = kMtTileW + kMtHalo;   // 42 input columns of a tile
static constexpr int kMtIH = kMtTileH + kMtHalo;   // 26 input rows
static constexpr int kMtPiece = 2048;              // elements one workgroup of the elem pass owns
static_assert(kMtTileW == DSD_METRICS_TILE_W && kMtTileH == DSD_METRICS_TILE_H, "dsdiff.h names the tile");
static_assert(kMtTileW == 32 && kMtTileH == 16,"metrics_map_kernel: a thread owns column tid & 31 of rows tid >> 5 and (tid >> 5) + 8");

// g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum, evaluated in double (host_io._gauss1d(11, 1.5), digit for digit)
static __constant__ const double kMtG[kMtWin] = {
    0.0010283800844791092, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537, 0.26601172486179436,
    0.2130055377112537,    0.10936068950970002,  0.03600077212843083, 0.007598758135239185, 0.0010283800844791092};

// y = clip((x - mean) / div + add, lo, hi), the expression of host_io.scale12bit: no product, so nothing to contract, and the
// IEEE division gives the host's bits
struct MtPre {
    int on = 0;
    double mean_p = 0, div_p = 1, mean_t = 0, div_t = 1, add = 0, lo = 0, hi = 0;
};
__device__ __forceinline__ double mt_in(float v, const MtPre& q, double mean, double div) {
    const double x = (double)v;
    return q.on ? fmin(fmax((x - mean) / div + q.add, q.lo), q.hi) : x;
}
__device__ __forceinline__ double mt_in(double v, const MtPre&, double, double) { return v; }   // a pooled scale: transformed already

// red holds Q runs of 256; sums for q < NSUM, then minima and maxima alternating (elem: |d|, d^2, min t, max t, min p, max p)
template <int Q, int NSUM>
__device__ __forceinline__ void mt_fold(double* red, int tid) {
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double a = red[q * 256 + tid], b = red[q * 256 + tid + w];
                red[q * 256 + tid] = q < NSUM ? a + b : ((q - NSUM) & 1) ? fmax(a, b) : fmin(a, b);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------ elem pass
__global__ __launch_bounds__(256) void metrics_elem_kernel(const float* __restrict__ pred, const float* __restrict__ target, int n, MtPre q,
                                                           double* __restrict__ part) {
    __shared__ double red[6 * 256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t row = (int64_t)b * n;
    double sa = 0.0, ss = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < kMtPiece / 256; ++j) {
        const int i = blockIdx.x * kMtPiece + j * 256 + tid;              // n <= 2^30: no overflow
        if (i < n) {
            const double p = mt_in(pred[row + i], q, q.mean_p, q.div_p), t = mt_in(target[row + i], q, q.mean_t, q.div_t);
            const double d = p - t;
            sa += fabs(d);
            ss += d * d;
            tmin = fmin(tmin, t); tmax = fmax(tmax, t);
            pmin = fmin(pmin, p); pmax = fmax(pmax, p);
        }
    }
    red[tid] = sa; red[256 + tid] = ss; red[512 + tid] = tmin; red[768 + tid] = tmax; red[1024 + tid] = pmin; red[1280 + tid] = pmax;
    mt_fold<6, 2>(red, tid);
    if (tid < 6) part[((int64_t)b * gridDim.x + blockIdx.x) * 6 + tid] = red[tid * 256];
}

// one workgroup per sample: thread t takes the pieces t, t + 256, ... in that order, then the fixed fold
__global__ __launch_bounds__(256) void metrics_elem_finalize_kernel(const double* __restrict__ part, int npiece, double data_range,
                                                                    double* __restrict__ elem, double* __restrict__ cc) {
    __shared__ double red[6 * 256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double sa = 0.0, ss = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY;
    for (int p = tid; p < npiece; p += 256) {
        const double* v = part + ((int64_t)b * npiece + p) * 6;
        sa += v[0]; ss += v[1];
        tmin = fmin(tmin, v[2]); tmax = fmax(tmax, v[3]);
        pmin = fmin(pmin, v[4]); pmax = fmax(pmax, v[5]);
    }
    red[tid] = sa; red[256 + tid] = ss; red[512 + tid] = tmin; red[768 + tid] = tmax; red[1024 + tid] = pmin; red[1280 + tid] = pmax;
    mt_fold<6, 2>(red, tid);
    if (tid < 6) elem[b * 6 + tid] = red[tid * 256];
    if (tid == 0) {
        const double R = data_range > 0.0 ? data_range : fmax(red[1280] - red[1024], red[768] - red[512]);
        const double k1 = 0.01 * R, k2 = 0.03 * R;
        cc[b * 2] = k1 * k1;
        cc[b * 2 + 1] = k2 * k2;
    }
}

// ----------------------------------------------------------------------------------------------------------------------- pool
// grid (ceil(C*H2*W2 / 256), B): out[b][c][i][j] = mean of in[b][c][2i..2i+1][2j..2j+1]
template <typename T>
__global__ __launch_bounds__(256) void metrics_pool_kernel(const T* __restrict__ x, const T* __restrict__ y, int C, int H, int W, MtPre q,
                                                           double* __restrict__ xo, double* __restrict__ yo) {
    const int H2 = H / 2, W2 = W / 2;
    const int per = C * H2 * W2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= per) return;
    const int j = idx % W2, i = (idx / W2) % H2, c = idx / (W2 * H2);
    const int64_t src = ((int64_t)blockIdx.y * C + c) * H * W + (int64_t)(2 * i) * W + 2 * j;
    const T* px = x + src;
    const T* py = y + src;
    const double a = mt_in(px[0], q, q.mean_p, q.div_p) + mt_in(px[1], q, q.mean_p, q.div_p) + mt_in(px[W], q, q.mean_p, q.div_p) +
                     mt_in(px[W + 1], q, q.mean_p, q.div_p);
    const double t = mt_in(py[0], q, q.mean_t, q.div_t) + mt_in(py[1], q, q.mean_t, q.div_t) + mt_in(py[W], q, q.mean_t, q.div_t) +
                     mt_in(py[W + 1], q, q.mean_t, q.div_t);
    const int64_t dst = (int64_t)blockIdx.y * per + idx;
    xo[dst] = 0.25 * a;
    yo[dst] = 0.25 * t;
}

// ------------------------------------------------------------------------------------------------------------------------ map
// grid (tilesX * tilesY * C, B).  x is the prediction, y the target; part is this scale's [B][tiles][2] (ssim sum, cs sum).
template <typename T>
__global__ __launch_bounds__(256) void metrics_map_kernel(const T* __restrict__ x, const T* __restrict__ y, int C, int H, int W, int tilesX,
                                                          int tilesY, MtPre q, const double* __restrict__ cc, double* __restrict__ part) {
    __shared__ double sx[kMtIH * kMtIW];
    __shared__ double sy[kMtIH * kMtIW];
    __shared__ double rb[5][kMtIH * kMtTileW];
    __shared__ double red[2 * 256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tile = blockIdx.x;
    const int x0 = (tile % tilesX) * kMtTileW, y0 = ((tile / tilesX) % tilesY) * kMtTileH, c = tile / (tilesX * tilesY);
    const int64_t plane = ((int64_t)b * C + c) * H * W;
    const T* px = x + plane;
    const T* py = y + plane;
    for (int idx = tid; idx < kMtIH * kMtIW; idx += 256) {               // zero outside the image: only masked outputs read it
        const int r = idx / kMtIW, k = idx % kMtIW;
        const int gy = y0 + r, gx = x0 + k;
        const bool in = gy < H && gx < W;
        sx[idx] = in ? mt_in(px[(int64_t)gy * W + gx], q, q.mean_p, q.div_p) : 0.0;
        sy[idx] = in ? mt_in(py[(int64_t)gy * W + gx], q, q.mean_t, q.div_t) : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < kMtIH * kMtTileW; idx += 256) {
        const int r = idx / kMtTileW, k = idx % kMtTileW;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
        for (int t = 0; t < kMtWin; ++t) {
            const double g = kMtG[t], a = sx[r * kMtIW + k + t], v = sy[r * kMtIW + k + t];
            mx += g * a; my += g * v;
            xx += g * (a * a); yy += g * (v * v); xy += g * (a * v);
        }
        rb[0][idx] = mx; rb[1][idx] = my; rb[2][idx] = xx; rb[3][idx] = yy; rb[4][idx] = xy;
    }
    __syncthreads();
    const double c1 = cc[b * 2], c2 = cc[b * 2 + 1];
    const int Wo = W - kMtHalo, Ho = H - kMtHalo;
    const int lx = tid & (kMtTileW - 1), ly = tid / kMtTileW;
    double s_ssim = 0.0, s_cs = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int oy = ly + 8 * h;
        if (x0 + lx < Wo && y0 + oy < Ho) {
            double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
            for (int t = 0; t < kMtWin; ++t) {
                const double g = kMtG[t];
                const int at = (oy + t) * kMtTileW + lx;
                mx += g * rb[0][at]; my += g * rb[1][at];
                xx += g * rb[2][at]; yy += g * rb[3][at]; xy += g * rb[4][at];
            }
            const double vx = xx - mx * mx, vy = yy - my * my, vxy = xy - mx * my;      // biased
            const double cs = (2.0 * vxy + c2) / (vx + vy + c2);
            s_cs += cs;
            s_ssim += (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * cs;
        }
    }
    red[tid] = s_ssim; red[256 + tid] = s_cs;
    mt_fold<2, 2>(red, tid);
    if (tid < 2) part[((int64_t)b * gridDim.x + tile) * 2 + tid] = red[tid * 256];
}

struct MtScales {
    int64_t off[DSD_METRICS_MAX_SCALES];   // of scale s' partials in the scratch, in doubles
    int tiles[DSD_METRICS_MAX_SCALES];
    double count[DSD_METRICS_MAX_SCALES];  // C * Ho * Wo
};

// grid (S, B): scale_out[b][s] = (sum of the ssim map, sum of the cs map) / count, unclamped
__global__ __launch_bounds__(256) void metrics_map_finalize_kernel(const double* __restrict__ scratch, MtScales sc, int S,
                                                                   double* __restrict__ out) {
    __shared__ double red[2 * 256];
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int64_t off = sc.off[0];
    int tiles = sc.tiles[0];
    double count = sc.count[0];
#pragma unroll
    for (int i = 1; i < DSD_METRICS_MAX_SCALES; ++i)      // (a select chain: a dynamic index into the argument would go through scratch)
        if (s == i) { off = sc.off[i]; tiles = sc.tiles[i]; count = sc.count[i]; }
    const double* part = scratch + off + (int64_t)b * tiles * 2;
    double a = 0.0, c = 0.0;
    for (int p = tid; p < tiles; p += 256) { a += part[p * 2]; c += part[p * 2 + 1]; }
    red[tid] = a; red[256 + tid] = c;
    mt_fold<2, 2>(red, tid);
    if (tid < 2) out[((int64_t)b * S + s) * 2 + tid] = red[tid * 256] / count;
}

// ----------------------------------------------------------------------------------------------------------------------- host
namespace {
struct MtLayout {
    int h[DSD_METRICS_MAX_SCALES], w[DSD_METRICS_MAX_SCALES], tx[DSD_METRICS_MAX_SCALES], ty[DSD_METRICS_MAX_SCALES];
    int npiece;
    size_t elem_part, cc, map_part[DSD_METRICS_MAX_SCALES], pyr_x[DSD_METRICS_MAX_SCALES], pyr_y[DSD_METRICS_MAX_SCALES], total;
};
MtLayout mt_layout(int B, int C, int H, int W, int S) {
    MtLayout l = {};
    const int64_t n = (int64_t)C * H * W;
    l.npiece = (int)((n + kMtPiece - 1) / kMtPiece);
    size_t at = 0;
    l.elem_part = at; at += (size_t)B * l.npiece * 6;
    l.cc = at; at += (size_t)B * 2;
    for (int s = 0; s < S; ++s) {
        l.h[s] = s ? l.h[s - 1] / 2 : H;
        l.w[s] = s ? l.w[s - 1] / 2 : W;
        l.tx[s] = (l.w[s] - kMtHalo + kMtTileW - 1) / kMtTileW;
        l.ty[s] = (l.h[s] - kMtHalo + kMtTileH - 1) / kMtTileH;
        l.map_part[s] = at; at += (size_t)B * l.tx[s] * l.ty[s] * C * 2;
        if (s) {
            const size_t img = (size_t)B * C * l.h[s] * l.w[s];
            l.pyr_x[s] = at; at += img;
            l.pyr_y[s] = at; at += img;
        }
    }
    l.total = at;
    return l;
}
}  // namespace

void image_metrics_check(int B, int C, int H, int W, int scales, double data_range, const double* pre) {
    DSD_CHECK(scales >= 1 && scales <= DSD_METRICS_MAX_SCALES, "image_metrics: scales is %d; 1 to %d are taken", scales, DSD_METRICS_MAX_SCALES);
    DSD_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1, "image_metrics: bad shape: B %d C %d H %d W %d", B, C, H, W);
    const int least = (H < W ? H : W) >> (scales - 1);
    DSD_CHECK(least >= kMtWin, "image_metrics: scale %d of a %d x %d image has a side of %d; the %d-tap window needs %d", scales, H, W, least,
              kMtWin, kMtWin);
    DSD_CHECK(B <= 65535, "image_metrics: B is %d; up to 65535 samples are taken", B);
    const int64_t n = (int64_t)C * H * W;
    DSD_CHECK(n <= (int64_t)1 << 30, "image_metrics: one sample has C*H*W = %lld elements; up to 2^30 are taken", (long long)n);
    DSD_CHECK(std::isfinite(data_range) && data_range >= 0.0, "image_metrics: data_range is %g; a positive value, or 0 for each sample's own range",
              data_range);
    if (pre) {
        DSD_CHECK(pre[1] != 0.0, "image_metrics: pre divides the prediction by div = %g", pre[1]);
        DSD_CHECK(pre[3] != 0.0, "image_metrics: pre divides the target by div = %g", pre[3]);
        DSD_CHECK(pre[5] <= pre[6], "image_metrics: pre clips to lo = %g above hi = %g", pre[5], pre[6]);
    }
}

size_t image_metrics_scratch_doubles(int B, int C, int H, int W, int scales) { return mt_layout(B, C, H, W, scales).total; }

void image_metrics(const ImageMetrics& a, hipStream_t s) {
    image_metrics_check(a.B, a.C, a.H, a.W, a.scales, a.data_range, a.pre);
    DSD_CHECK(a.pred && a.target && a.scratch && a.scale_out && a.elem_out, "image_metrics: null argument");
    const int B = a.B, C = a.C, S = a.scales;
    const MtLayout l = mt_layout(B, C, a.H, a.W, S);
    MtPre q;
    if (a.pre) {
        q.on = 1;
        q.mean_p = a.pre[0]; q.div_p = a.pre[1]; q.mean_t = a.pre[2]; q.div_t = a.pre[3];
        q.add = a.pre[4]; q.lo = a.pre[5]; q.hi = a.pre[6];
    }
    const MtPre none;
    double* w = a.scratch;
    const int n = C * a.H * a.W;
    hipLaunchKernelGGL(metrics_elem_kernel, dim3(l.npiece, B), dim3(256), 0, s, a.pred, a.target, n, q, w + l.elem_part);
    check_launch("metrics_elem");
    hipLaunchKernelGGL(metrics_elem_finalize_kernel, dim3(B), dim3(256), 0, s, w + l.elem_part, l.npiece, a.data_range, a.elem_out, w + l.cc);
    check_launch("metrics_elem_finalize");
    MtScales sc = {};
    for (int i = 0; i < S; ++i) {
        const int tiles = l.tx[i] * l.ty[i] * C;
        sc.off[i] = (int64_t)l.map_part[i];
        sc.tiles[i] = tiles;
        sc.count[i] = (double)C * (l.h[i] - kMtHalo) * (l.w[i] - kMtHalo);
        if (i == 0) {
            hipLaunchKernelGGL(metrics_map_kernel<float>, dim3(tiles, B), dim3(256), 0, s, a.pred, a.target, C, a.H, a.W, l.tx[0], l.ty[0], q,
                               w + l.cc, w + l.map_part[0]);
        } else {
            const int per = C * l.h[i] * l.w[i];
            if (i == 1)
                hipLaunchKernelGGL(metrics_pool_kernel<float>, dim3((per + 255) / 256, B), dim3(256), 0, s, a.pred, a.target, C, a.H, a.W, q,
                                   w + l.pyr_x[1], w + l.pyr_y[1]);
            else
                hipLaunchKernelGGL(metrics_pool_kernel<double>, dim3((per + 255) / 256, B), dim3(256), 0, s, (const double*)(w + l.pyr_x[i - 1]),
                                   (const double*)(w + l.pyr_y[i - 1]), C, l.h[i - 1], l.w[i - 1], none, w + l.pyr_x[i], w + l.pyr_y[i]);
            check_launch("metrics_pool");
            hipLaunchKernelGGL(metrics_map_kernel<double>, dim3(tiles, B), dim3(256), 0, s, (const double*)(w + l.pyr_x[i]),
                               (const double*)(w + l.pyr_y[i]), C, l.h[i], l.w[i], l.tx[i], l.ty[i], none, w + l.cc, w + l.map_part[i]);
        }
        check_launch("metrics_map");
    }
    hipLaunchKernelGGL(metrics_map_finalize_kernel, dim3(S, B), dim3(256), 0, s, (const double*)w, sc, S, a.scale_out);
    check_launch("metrics_map_finalize");
}

}  // namespace dsd
