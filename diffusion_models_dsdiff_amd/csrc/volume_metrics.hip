// volume_metrics.hip — the per-id metric table of a predicted volume against its reference, and an exact order statistic.
//
// The array metrics of inference/test_metrics.py as inference/get_metric*.py call them per volume id — NRMSE, MAPE, sMAPE, logac,
// medsymac over the mask (:149-224), PSNR over the mask's bounding box (:378-400), the 9^3 box-window SSIM (:227-246) — restated
// from the float64 host functions of host_io.py, which are what the tests hold this file to.  target / pred are [D,H,W] of float or
// of double (one templated load); everything from the load onward is fp64.
//
//   domains   M = the voxels with mask != 0 (all, without a mask); per axis lo / hi = the smallest / largest index holding one;
//             the crop is [lo, hi) per axis, the upper bound EXCLUSIVE as the reference slices; Z = the crop of where(m, x, 0);
//             R = the crop of the raw volume with a mask, the whole volume without one.
//   pass 1    n_M, the box, sum t, sum p, min t, max t over M.
//   pass 2    centred squares of t and p and sum (t - p)^2 over M; sums, min / max of tz and sum (tz - pz)^2 over Z; sums and
//             min / max of t over R.
//   pass 3    centred squares over Z and R; ts / ps = the 12-bit rescale with M's mean and std, the three M sums, and
//             l = |log(ps / ts)| stored per voxel, +inf outside M.
//   select    the two middle order statistics of l by most-significant-first radix selection (kth_*: 11-bit digits, six histogram
//             passes, both ranks side by side); the padding is the largest key, so a rank below n_M never reaches it.
//   ssim3d    (win > 0) per z-slice of R the win x win window sums of x, y, xx, yy, xy through LDS into [d, h - win + 1,
//             w - win + 1, 5]; a second kernel adds win slices along z, forms the map and folds it.  Sums are re-added per window.
// Every pass writes one partial per workgroup and quantity; a one-workgroup kernel adds them in a fixed order (thread t takes the
// pieces t, t + 256, ..., then a fixed LDS fold) and leaves means, stds and the box in a state array in device memory that the
// next pass reads: no value returns to the host before the end.  No floating-point atomics; the histograms count with integer
// atomics, whose result does not depend on order: two calls agree bit for bit.  The box is known on the device only, so grids
// and scratch are sized for the whole volume and workgroups outside R leave at once.
#include "../../include/dsdiff.h"
#include "kernels.h"

#include <cmath>

namespace dsd {

static constexpr int kVmPiece = 2048;                        // voxels one workgroup of a pass owns
static constexpr int kVmWinMax = 11;
static constexpr int kVmIW = kVmTileW + kVmWinMax - 1;       // LDS row stride of a tile's inputs
static constexpr int kVmIH = kVmTileH + kVmWinMax - 1;
static constexpr int kVmQ = 12;                              // partials per workgroup, the widest pass
static constexpr int kKthDigit = 11, kKthBins = 1 << kKthDigit, kKthPasses = 6, kKthPiece = 4096;
static_assert(kVmTileW == DSD_VOLUME_TILE_W && kVmTileH == DSD_VOLUME_TILE_H, "dsdiff.h names the tile");
static_assert(kVmTileW == 32 && kVmTileH == 16, "volume_ssim_rows_kernel: a thread owns column tid & 31 of rows tid >> 5 and (tid >> 5) + 8");
static_assert(kKthDigit * (kKthPasses - 1) < 64 && kKthDigit * kKthPasses >= 64, "six digits cover the 64 key bits");

// the state the passes hand on, in device memory (doubles)
enum {
    S_N = 0, S_LO_D, S_HI_D, S_LO_H, S_HI_H, S_LO_W, S_HI_W,             // lo / hi: the crop [lo, hi), 0 / 0 for an empty mask
    S_MIN_TM, S_MAX_TM, S_MEAN_TM, S_MEAN_PM, S_STD_TM, S_STD_PM, S_NRMSE,
    S_NZ, S_MEAN_TZ, S_MEAN_PZ, S_STD_TZ, S_STD_PZ, S_MIN_TZ, S_MAX_TZ, S_PSNR,
    S_NR, S_MEAN_TR, S_MEAN_PR, S_STD_TR, S_STD_PR, S_MIN_TR, S_MAX_TR, S_C1, S_C2,
    S_MAPE, S_SMAPE, S_LOGAC, S_COUNT
};

struct KthSel {
    unsigned long long prefix;   // the digits chosen so far, in place
    long long k;                 // the rank among the elements that share them
};

template <typename T>
__device__ __forceinline__ double vm_load(const T* __restrict__ x, int64_t i) { return (double)x[i]; }

// host_io.scale12bit, in its expression order: no product, so nothing to contract, and the IEEE division gives the host's bits
__device__ __forceinline__ double vm_s12(double x, double mean, double div) { return fmin(fmax(((x - mean) / div) + 2048., 1e-10), 4095.); }

// red holds Q runs of 256; sums for q < NSUM, then minima and maxima alternating
template <int Q, int NSUM>
__device__ __forceinline__ void vm_fold(double* red, int tid) {
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

// one workgroup: thread t takes the pieces t, t + 256, ... of part[npiece][Q] in that order, then the fixed fold; red[q * 256]
template <int Q, int NSUM>
__device__ __forceinline__ void vm_fold_parts(const double* __restrict__ part, int npiece, double* red, int tid) {
    double v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = q < NSUM ? 0.0 : ((q - NSUM) & 1) ? -INFINITY : INFINITY;
    for (int p = tid; p < npiece; p += 256) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double b = part[(int64_t)p * Q + q];
            v[q] = q < NSUM ? v[q] + b : ((q - NSUM) & 1) ? fmax(v[q], b) : fmin(v[q], b);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q * 256 + tid] = v[q];
    vm_fold<Q, NSUM>(red, tid);
}

struct VmBox {
    int z0, y0, x0, z1, y1, x1;   // the crop [lo, hi)
};
__device__ __forceinline__ VmBox vm_box(const double* __restrict__ st) {
    VmBox b;
    b.z0 = (int)st[S_LO_D]; b.z1 = (int)st[S_HI_D];
    b.y0 = (int)st[S_LO_H]; b.y1 = (int)st[S_HI_H];
    b.x0 = (int)st[S_LO_W]; b.x1 = (int)st[S_HI_W];
    return b;
}
// R: the crop with a mask, the whole volume without one
__device__ __forceinline__ VmBox vm_box_r(const double* __restrict__ st, int has_mask, int D, int H, int W) {
    if (has_mask) return vm_box(st);
    VmBox b;
    b.z0 = b.y0 = b.x0 = 0;
    b.z1 = D; b.y1 = H; b.x1 = W;
    return b;
}

// --------------------------------------------------------------------------------------------------------------------- pass 1
// part[piece][11]: n, sum t, sum p | min t, max t, lo z, hi z, lo y, hi y, lo x, hi x  (indices as doubles: exact)
template <typename T>
__global__ __launch_bounds__(256) void volume_pass1_kernel(const T* __restrict__ t, const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                           int n, int H, int W, double* __restrict__ part) {
    __shared__ double red[11 * 256];
    const int tid = threadIdx.x;
    double v[11] = {0.0, 0.0, 0.0, INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < kVmPiece / 256; ++j) {
        const int i = blockIdx.x * kVmPiece + j * 256 + tid;                 // n <= 2^27: no overflow
        if (i < n && (!mask || mask[i])) {
            const double a = vm_load(t, i), b = vm_load(p, i);
            const double x = (double)(i % W), y = (double)((i / W) % H), z = (double)(i / (W * H));
            v[0] += 1.0; v[1] += a; v[2] += b;
            v[3] = fmin(v[3], a); v[4] = fmax(v[4], a);
            v[5] = fmin(v[5], z); v[6] = fmax(v[6], z);
            v[7] = fmin(v[7], y); v[8] = fmax(v[8], y);
            v[9] = fmin(v[9], x); v[10] = fmax(v[10], x);
        }
    }
#pragma unroll
    for (int q = 0; q < 11; ++q) red[q * 256 + tid] = v[q];
    vm_fold<11, 3>(red, tid);
    if (tid < 11) part[(int64_t)blockIdx.x * 11 + tid] = red[tid * 256];
}

__global__ __launch_bounds__(256) void volume_final1_kernel(const double* __restrict__ part, int npiece, int has_mask, int n_all,
                                                            double* __restrict__ st, KthSel* __restrict__ sel) {
    __shared__ double red[11 * 256];
    const int tid = threadIdx.x;
    vm_fold_parts<11, 3>(part, npiece, red, tid);
    if (tid == 0) {
        const double n = red[0];
        const bool any = n > 0.0;
        st[S_N] = n;
        double side[3];
        for (int a = 0; a < 3; ++a) {
            const double lo = any ? red[(5 + 2 * a) * 256] : 0.0, hi = any ? red[(6 + 2 * a) * 256] : 0.0;
            st[S_LO_D + 2 * a] = lo;
            st[S_HI_D + 2 * a] = hi;
            side[a] = hi - lo;
        }
        st[S_MIN_TM] = red[3 * 256];
        st[S_MAX_TM] = red[4 * 256];
        st[S_MEAN_TM] = red[1 * 256] / n;
        st[S_MEAN_PM] = red[2 * 256] / n;
        st[S_NZ] = side[0] * side[1] * side[2];
        st[S_NR] = has_mask ? st[S_NZ] : (double)n_all;
        const long long ni = (long long)n;
        sel[0].prefix = 0; sel[0].k = ni > 0 ? (ni - 1) / 2 : 0;        // the two middle ranks: one and the same for an odd n
        sel[1].prefix = 0; sel[1].k = ni / 2;
    }
}

// --------------------------------------------------------------------------------------------------------------------- pass 2
// part[piece][12]: M: sum (t - mt)^2, sum (p - mp)^2, sum (t - p)^2;  Z: sum tz, sum pz, sum (tz - pz)^2;  R: sum t, sum p |
// min tz, max tz, min tR, max tR
template <typename T>
__global__ __launch_bounds__(256) void volume_pass2_kernel(const T* __restrict__ t, const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                           int n, int D, int H, int W, const double* __restrict__ st, double* __restrict__ part) {
    __shared__ double red[12 * 256];
    const int tid = threadIdx.x;
    const VmBox bz = vm_box(st), br = vm_box_r(st, mask != nullptr, D, H, W);
    const double mt = st[S_MEAN_TM], mp = st[S_MEAN_PM];
    double v[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY, INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < kVmPiece / 256; ++j) {
        const int i = blockIdx.x * kVmPiece + j * 256 + tid;
        if (i < n) {
            const double a = vm_load(t, i), b = vm_load(p, i);
            const int x = i % W, y = (i / W) % H, z = i / (W * H);
            const bool m = !mask || mask[i];
            if (m) {
                const double da = a - mt, db = b - mp, d = a - b;
                v[0] += da * da; v[1] += db * db; v[2] += d * d;
            }
            if (z >= bz.z0 && z < bz.z1 && y >= bz.y0 && y < bz.y1 && x >= bz.x0 && x < bz.x1) {
                const double az = m ? a : 0.0, pz = m ? b : 0.0, d = az - pz;
                v[3] += az; v[4] += pz; v[5] += d * d;
                v[8] = fmin(v[8], az); v[9] = fmax(v[9], az);
            }
            if (z >= br.z0 && z < br.z1 && y >= br.y0 && y < br.y1 && x >= br.x0 && x < br.x1) {
                v[6] += a; v[7] += b;
                v[10] = fmin(v[10], a); v[11] = fmax(v[11], a);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) red[q * 256 + tid] = v[q];
    vm_fold<12, 8>(red, tid);
    if (tid < 12) part[(int64_t)blockIdx.x * 12 + tid] = red[tid * 256];
}

__global__ __launch_bounds__(256) void volume_final2_kernel(const double* __restrict__ part, int npiece, double* __restrict__ st) {
    __shared__ double red[12 * 256];
    const int tid = threadIdx.x;
    vm_fold_parts<12, 8>(part, npiece, red, tid);
    if (tid == 0) {
        const double n = st[S_N], nz = st[S_NZ], nr = st[S_NR];
        st[S_STD_TM] = sqrt(red[0] / n);
        st[S_STD_PM] = sqrt(red[1 * 256] / n);
        st[S_NRMSE] = sqrt(red[2 * 256] / n) / (st[S_MAX_TM] - st[S_MIN_TM]);
        st[S_MEAN_TZ] = red[3 * 256] / nz;
        st[S_MEAN_PZ] = red[4 * 256] / nz;
        st[S_MIN_TZ] = red[8 * 256];
        st[S_MAX_TZ] = red[9 * 256];
        const double range = red[9 * 256] - red[8 * 256];
        st[S_PSNR] = 10.0 * log10(range * range / (red[5 * 256] / nz));
        st[S_MEAN_TR] = red[6 * 256] / nr;
        st[S_MEAN_PR] = red[7 * 256] / nr;
        st[S_MIN_TR] = red[10 * 256];
        st[S_MAX_TR] = red[11 * 256];
    }
}

// --------------------------------------------------------------------------------------------------------------------- pass 3
// part[piece][7]: Z: sum (tz - mtz)^2, sum (pz - mpz)^2;  R: sum (t - mtr)^2, sum (p - mpr)^2;  M: sum |ts - ps| / |ts|,
// sum |ps - ts| / (|ts| + |ps|), sum l.   lval[i] = l inside M, +inf outside.
template <typename T>
__global__ __launch_bounds__(256) void volume_pass3_kernel(const T* __restrict__ t, const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                           int n, int D, int H, int W, const double* __restrict__ st, double* __restrict__ lval,
                                                           double* __restrict__ part) {
    __shared__ double red[7 * 256];
    const int tid = threadIdx.x;
    const VmBox bz = vm_box(st), br = vm_box_r(st, mask != nullptr, D, H, W);
    const double mt = st[S_MEAN_TM], mp = st[S_MEAN_PM], dt = st[S_STD_TM] / 400., dp = st[S_STD_PM] / 400.;
    const double mtz = st[S_MEAN_TZ], mpz = st[S_MEAN_PZ], mtr = st[S_MEAN_TR], mpr = st[S_MEAN_PR];
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kVmPiece / 256; ++j) {
        const int i = blockIdx.x * kVmPiece + j * 256 + tid;
        if (i < n) {
            const double a = vm_load(t, i), b = vm_load(p, i);
            const int x = i % W, y = (i / W) % H, z = i / (W * H);
            const bool m = !mask || mask[i];
            if (z >= bz.z0 && z < bz.z1 && y >= bz.y0 && y < bz.y1 && x >= bz.x0 && x < bz.x1) {
                const double da = (m ? a : 0.0) - mtz, db = (m ? b : 0.0) - mpz;
                v[0] += da * da; v[1] += db * db;
            }
            if (z >= br.z0 && z < br.z1 && y >= br.y0 && y < br.y1 && x >= br.x0 && x < br.x1) {
                const double da = a - mtr, db = b - mpr;
                v[2] += da * da; v[3] += db * db;
            }
            double l = INFINITY;
            if (m) {
                const double ts = vm_s12(a, mt, dt), ps = vm_s12(b, mp, dp);
                l = fabs(log(ps / ts));
                v[4] += fabs(ts - ps) / fabs(ts);
                v[5] += fabs(ps - ts) / (fabs(ts) + fabs(ps));
                v[6] += l;
            }
            lval[i] = l;
        }
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) red[q * 256 + tid] = v[q];
    vm_fold<7, 7>(red, tid);
    if (tid < 7) part[(int64_t)blockIdx.x * 7 + tid] = red[tid * 256];
}

__global__ __launch_bounds__(256) void volume_final3_kernel(const double* __restrict__ part, int npiece, double* __restrict__ st) {
    __shared__ double red[7 * 256];
    const int tid = threadIdx.x;
    vm_fold_parts<7, 7>(part, npiece, red, tid);
    if (tid == 0) {
        const double n = st[S_N], nz = st[S_NZ], nr = st[S_NR];
        st[S_STD_TZ] = sqrt(red[0] / nz);
        st[S_STD_PZ] = sqrt(red[1 * 256] / nz);
        const double sr = sqrt(red[2 * 256] / nr);
        st[S_STD_TR] = sr;
        st[S_STD_PR] = sqrt(red[3 * 256] / nr);
        st[S_MAPE] = red[4 * 256] / n;
        st[S_SMAPE] = red[5 * 256] / n;
        st[S_LOGAC] = red[6 * 256] / n;
        // the rescale is monotone: the range of the rescaled reference is the rescaled max less the rescaled min
        const double R = vm_s12(st[S_MAX_TR], st[S_MEAN_TR], sr / 400.) - vm_s12(st[S_MIN_TR], st[S_MEAN_TR], sr / 400.);
        const double k1 = 0.01 * R, k2 = 0.03 * R;
        st[S_C1] = k1 * k1;
        st[S_C2] = k2 * k2;
    }
}

// ------------------------------------------------------------------------------------------------------------------ selection
// the order-preserving image of a double's bits: the sign flipped for non-negative values, the complement for negative ones
__device__ __forceinline__ unsigned long long kth_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : u ^ 0x8000000000000000ull;
}
__device__ __forceinline__ double kth_value(unsigned long long key) {
    const unsigned long long u = (key >> 63) ? key ^ 0x8000000000000000ull : ~key;
    return __longlong_as_double((long long)u);
}
__device__ __forceinline__ int kth_shift(int pass) { return pass < kKthPasses - 1 ? 64 - kKthDigit * (pass + 1) : 0; }
__device__ __forceinline__ int kth_bits(int pass) { return pass < kKthPasses - 1 ? kKthDigit : 64 - kKthDigit * (kKthPasses - 1); }

__global__ void kth_init_kernel(KthSel* __restrict__ sel, long long k) {
    sel[0].prefix = 0;
    sel[0].k = k;
}

// grid (pieces of 4096, lanes): digit `pass` of the elements that carry lane's prefix, counted in LDS, then added to hist[lane][pass]
__global__ __launch_bounds__(256) void kth_hist_kernel(const double* __restrict__ x, int64_t n, int pass, const KthSel* __restrict__ sel,
                                                       unsigned* __restrict__ hist) {
    __shared__ unsigned h[kKthBins];
    const int tid = threadIdx.x, lane = blockIdx.y;
    for (int b = tid; b < kKthBins; b += 256) h[b] = 0u;
    __syncthreads();
    const int shift = kth_shift(pass), above = shift + kth_bits(pass);     // above < 64 from the second pass on
    const unsigned long long want = pass ? sel[lane].prefix >> above : 0ull;
    const unsigned mask = (1u << kth_bits(pass)) - 1u;
    const int64_t base = (int64_t)blockIdx.x * kKthPiece;
#pragma unroll 4
    for (int j = 0; j < kKthPiece / 256; ++j) {
        const int64_t i = base + j * 256 + tid;
        if (i < n) {
            const unsigned long long key = kth_key(x[i]);
            if (pass == 0 || (key >> above) == want) atomicAdd(&h[(unsigned)(key >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    unsigned* g = hist + ((int64_t)lane * kKthPasses + pass) * kKthBins;
    for (int b = tid; b < kKthBins; b += 256)
        if (h[b]) atomicAdd(&g[b], h[b]);
}

// grid (lanes): the bin of hist[lane][pass] that holds rank k; k becomes the rank inside it.  A rank past the count (n_M = 0)
// stops in the last bin: nothing is indexed by it.
__global__ __launch_bounds__(256) void kth_scan_kernel(const unsigned* __restrict__ hist, int pass, KthSel* __restrict__ sel) {
    __shared__ unsigned long long cs[256];
    const int tid = threadIdx.x, lane = blockIdx.x;
    const unsigned* g = hist + ((int64_t)lane * kKthPasses + pass) * kKthBins;
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < kKthBins / 256; ++j) s += g[tid * (kKthBins / 256) + j];
    cs[tid] = s;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long k = (unsigned long long)sel[lane].k;
        unsigned long long acc = 0;
        int c = 0;
        for (; c < 255; ++c) {
            if (acc + cs[c] > k) break;
            acc += cs[c];
        }
        int b = c * (kKthBins / 256);
        for (int j = 0; j < kKthBins / 256 - 1; ++j) {
            const unsigned v = g[b];
            if (acc + v > k) break;
            acc += v;
            ++b;
        }
        sel[lane].k = (long long)(k - acc);
        sel[lane].prefix |= (unsigned long long)b << kth_shift(pass);
    }
}

__global__ void kth_result_kernel(const KthSel* __restrict__ sel, double* __restrict__ out) { out[0] = kth_value(sel[0].prefix); }

static void kth_select(const double* x, int64_t n, int lanes, KthSel* sel, unsigned* hist, hipStream_t s) {
    DSD_HIP(hipMemsetAsync(hist, 0, (size_t)lanes * kKthPasses * kKthBins * sizeof(unsigned), s));
    const unsigned pieces = (unsigned)((n + kKthPiece - 1) / kKthPiece);
    for (int pass = 0; pass < kKthPasses; ++pass) {
        hipLaunchKernelGGL(kth_hist_kernel, dim3(pieces, lanes), dim3(256), 0, s, x, n, pass, (const KthSel*)sel, hist);
        check_launch("kth_hist");
        hipLaunchKernelGGL(kth_scan_kernel, dim3(lanes), dim3(256), 0, s, (const unsigned*)hist, pass, sel);
        check_launch("kth_scan");
    }
}

// --------------------------------------------------------------------------------------------------------------------- ssim3d
// grid (tilesX * tilesY * D), sized for the whole volume: slice zr of R, a tile of 32 x 16 window positions.  rows[zr][oy][ox][5] =
// the win x win sums of x, y, xx, yy, xy (x the rescaled reference, y the rescaled prediction), hp = h - win + 1, wp = w - win + 1.
template <typename T>
__global__ __launch_bounds__(256) void volume_ssim_rows_kernel(const T* __restrict__ t, const T* __restrict__ p, int has_mask, int D, int H, int W,
                                                               int win, int tilesX, int tilesY, const double* __restrict__ st,
                                                               double* __restrict__ rows) {
    __shared__ double sx[kVmIH * kVmIW];
    __shared__ double sy[kVmIH * kVmIW];
    __shared__ double rb[5][kVmIH * kVmTileW];
    const int tid = threadIdx.x;
    const VmBox br = vm_box_r(st, has_mask, D, H, W);
    const int d = br.z1 - br.z0, h = br.y1 - br.y0, w = br.x1 - br.x0;
    const int hp = h - win + 1, wp = w - win + 1;
    const int tile = blockIdx.x % (tilesX * tilesY), zr = blockIdx.x / (tilesX * tilesY);
    const int ox0 = (tile % tilesX) * kVmTileW, oy0 = (tile / tilesX) * kVmTileH;
    if (d < win || hp < 1 || wp < 1 || zr >= d || ox0 >= wp || oy0 >= hp) return;      // uniform over the workgroup
    const double mt = st[S_MEAN_TR], mp = st[S_MEAN_PR], dt = st[S_STD_TR] / 400., dp = st[S_STD_PR] / 400.;
    const int ih = kVmTileH + win - 1, iw = kVmTileW + win - 1;
    const int64_t slice = (int64_t)(br.z0 + zr) * H * W;
    for (int idx = tid; idx < ih * iw; idx += 256) {                                   // zero outside R: only masked outputs read it
        const int r = idx / iw, k = idx % iw;
        const int gy = oy0 + r, gx = ox0 + k;
        const bool in = gy < h && gx < w;
        const int64_t at = slice + (int64_t)(br.y0 + gy) * W + br.x0 + gx;
        sx[r * kVmIW + k] = in ? vm_s12(vm_load(t, at), mt, dt) : 0.0;
        sy[r * kVmIW + k] = in ? vm_s12(vm_load(p, at), mp, dp) : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < ih * kVmTileW; idx += 256) {
        const int r = idx / kVmTileW, k = idx % kVmTileW;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
        for (int j = 0; j < win; ++j) {
            const double a = sx[r * kVmIW + k + j], b = sy[r * kVmIW + k + j];
            mx += a; my += b;
            xx += a * a; yy += b * b; xy += a * b;
        }
        rb[0][idx] = mx; rb[1][idx] = my; rb[2][idx] = xx; rb[3][idx] = yy; rb[4][idx] = xy;
    }
    __syncthreads();
    const int lx = tid & (kVmTileW - 1), ly = tid / kVmTileW;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int oy = ly + 8 * half;
        if (ox0 + lx < wp && oy0 + oy < hp) {
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < win; ++j) {
                const int at = (oy + j) * kVmTileW + lx;
#pragma unroll
                for (int q = 0; q < 5; ++q) v[q] += rb[q][at];
            }
            double* o = rows + (((int64_t)zr * hp + oy0 + oy) * wp + ox0 + lx) * 5;
#pragma unroll
            for (int q = 0; q < 5; ++q) o[q] = v[q];
        }
    }
}

// a thread owns one window position of R: win slices of rows added along z, the map, a fixed fold -> part[workgroup]
__global__ __launch_bounds__(256) void volume_ssim_map_kernel(const double* __restrict__ rows, int has_mask, int D, int H, int W, int win,
                                                              const double* __restrict__ st, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const VmBox br = vm_box_r(st, has_mask, D, H, W);
    const int dq = br.z1 - br.z0 - win + 1, hp = br.y1 - br.y0 - win + 1, wp = br.x1 - br.x0 - win + 1;
    const int64_t plane = (int64_t)hp * wp, npos = (dq < 1 || hp < 1 || wp < 1) ? 0 : dq * plane;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    double val = 0.0;
    if (i < npos) {
        const int64_t oz = i / plane, rem = i % plane;
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < win; ++j) {
            const double* r = rows + ((oz + j) * plane + rem) * 5;
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] += r[q];
        }
        const double npix = (double)(win * win * win), cov = npix / (npix - 1.0);
        const double ux = v[0] / npix, uy = v[1] / npix, uxx = v[2] / npix, uyy = v[3] / npix, uxy = v[4] / npix;
        const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
        const double c1 = st[S_C1], c2 = st[S_C2];
        val = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
    red[tid] = val;
    vm_fold<1, 1>(red, tid);
    if (tid == 0) part[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------------------------------------ out
// one workgroup: folds the ssim partials, takes the median from the two selected ranks, decides the status, writes out[]
__global__ __launch_bounds__(256) void volume_out_kernel(const double* __restrict__ st, const KthSel* __restrict__ sel,
                                                         const double* __restrict__ ssim_part, int nssim, int has_mask, int D, int H, int W,
                                                         int win, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    vm_fold_parts<1, 1>(ssim_part, nssim, red, tid);
    if (tid != 0) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double n = st[S_N];
    int status = 0;
    for (int i = 0; i < DSD_VOLUME_NOUT; ++i) out[i] = qnan;
    out[DSD_VOLUME_N_M] = n;
    if (n <= 0.0) {
        out[DSD_VOLUME_STATUS] = (double)DSD_VOLUME_EMPTY_MASK;
        return;
    }
    for (int a = 0; a < 6; ++a) out[DSD_VOLUME_LO_D + a] = st[S_LO_D + a];
    out[DSD_VOLUME_MEAN_T_M] = st[S_MEAN_TM]; out[DSD_VOLUME_STD_T_M] = st[S_STD_TM];
    out[DSD_VOLUME_MEAN_P_M] = st[S_MEAN_PM]; out[DSD_VOLUME_STD_P_M] = st[S_STD_PM];
    if (st[S_MAX_TM] == st[S_MIN_TM]) status |= DSD_VOLUME_ZERO_RANGE;
    else out[DSD_VOLUME_NRMSE] = st[S_NRMSE];
    if (st[S_STD_TM] == 0.0 || st[S_STD_PM] == 0.0) {
        status |= DSD_VOLUME_ZERO_STD;
    } else {
        out[DSD_VOLUME_MAPE] = st[S_MAPE];
        out[DSD_VOLUME_SMAPE] = st[S_SMAPE];
        out[DSD_VOLUME_LOGAC] = st[S_LOGAC];
        // the middle order statistic, or half the sum of the two middle ones (np.median); for an odd n both ranks are one
        out[DSD_VOLUME_MEDSYMAC] = exp(0.5 * (kth_value(sel[0].prefix) + kth_value(sel[1].prefix))) - 1.0;
    }
    const bool crop = st[S_NZ] > 0.0;
    if (!crop) {
        status |= DSD_VOLUME_EMPTY_CROP;
    } else {
        out[DSD_VOLUME_MEAN_T_Z] = st[S_MEAN_TZ]; out[DSD_VOLUME_STD_T_Z] = st[S_STD_TZ];
        out[DSD_VOLUME_MEAN_P_Z] = st[S_MEAN_PZ]; out[DSD_VOLUME_STD_P_Z] = st[S_STD_PZ];
        if (st[S_MAX_TZ] == st[S_MIN_TZ]) status |= DSD_VOLUME_ZERO_RANGE;
        else out[DSD_VOLUME_PSNR] = st[S_PSNR];
    }
    if (crop || !has_mask) {
        out[DSD_VOLUME_MEAN_T_R] = st[S_MEAN_TR]; out[DSD_VOLUME_STD_T_R] = st[S_STD_TR];
        out[DSD_VOLUME_MEAN_P_R] = st[S_MEAN_PR]; out[DSD_VOLUME_STD_P_R] = st[S_STD_PR];
        if (win > 0) {
            const VmBox br = vm_box_r(st, has_mask, D, H, W);
            const int dq = br.z1 - br.z0 - win + 1, hp = br.y1 - br.y0 - win + 1, wp = br.x1 - br.x0 - win + 1;
            if (dq < 1 || hp < 1 || wp < 1) status |= DSD_VOLUME_SMALL_R;
            else if (st[S_STD_TR] == 0.0 || st[S_STD_PR] == 0.0) status |= DSD_VOLUME_ZERO_STD;
            else out[DSD_VOLUME_SSIM3D] = red[0] / ((double)dq * hp * wp);
        }
    }
    out[DSD_VOLUME_STATUS] = (double)status;
}

// ----------------------------------------------------------------------------------------------------------------------- host
namespace {
struct VmLayout {
    int npiece, tx, ty;
    int64_t nrows_wg, nmap_wg;
    size_t part, st, lval, sel, hist, rows, ssim_part, total;    // byte offsets, each a multiple of 16
};
size_t vm_up(size_t b) { return (b + 255) & ~(size_t)255; }
VmLayout vm_layout(int D, int H, int W, int win) {
    VmLayout l = {};
    const int64_t n = (int64_t)D * H * W;
    l.npiece = (int)((n + kVmPiece - 1) / kVmPiece);
    size_t at = 0;
    l.part = at; at += vm_up((size_t)l.npiece * kVmQ * sizeof(double));
    l.st = at; at += vm_up(S_COUNT * sizeof(double));
    l.lval = at; at += vm_up((size_t)n * sizeof(double));
    l.sel = at; at += vm_up(2 * sizeof(KthSel));
    l.hist = at; at += vm_up((size_t)2 * kKthPasses * kKthBins * sizeof(unsigned));
    const bool ssim = win > 0 && D >= win && H >= win && W >= win;      // else no slice of R takes the window: the status says so
    if (ssim) {
        const int hp = H - win + 1, wp = W - win + 1;
        l.tx = (wp + kVmTileW - 1) / kVmTileW;
        l.ty = (hp + kVmTileH - 1) / kVmTileH;
        l.nrows_wg = (int64_t)l.tx * l.ty * D;
        l.nmap_wg = ((int64_t)(D - win + 1) * hp * wp + 255) / 256;
        l.rows = at; at += vm_up((size_t)D * hp * wp * 5 * sizeof(double));
    }
    l.ssim_part = at; at += vm_up((size_t)(l.nmap_wg ? l.nmap_wg : 1) * sizeof(double));
    l.total = at;
    return l;
}

template <typename T>
void vm_run(const VolumeMetrics& a, const VmLayout& l, char* w, hipStream_t s) {
    const T* t = (const T*)a.target;
    const T* p = (const T*)a.pred;
    const int D = a.D, H = a.H, W = a.W, n = D * H * W, has_mask = a.mask != nullptr;
    double* part = (double*)(w + l.part);
    double* st = (double*)(w + l.st);
    double* lval = (double*)(w + l.lval);
    KthSel* sel = (KthSel*)(w + l.sel);
    double* ssim_part = (double*)(w + l.ssim_part);
    hipLaunchKernelGGL(volume_pass1_kernel<T>, dim3(l.npiece), dim3(256), 0, s, t, p, a.mask, n, H, W, part);
    check_launch("volume_pass1");
    hipLaunchKernelGGL(volume_final1_kernel, dim3(1), dim3(256), 0, s, (const double*)part, l.npiece, has_mask, n, st, sel);
    check_launch("volume_final1");
    hipLaunchKernelGGL(volume_pass2_kernel<T>, dim3(l.npiece), dim3(256), 0, s, t, p, a.mask, n, D, H, W, (const double*)st, part);
    check_launch("volume_pass2");
    hipLaunchKernelGGL(volume_final2_kernel, dim3(1), dim3(256), 0, s, (const double*)part, l.npiece, st);
    check_launch("volume_final2");
    hipLaunchKernelGGL(volume_pass3_kernel<T>, dim3(l.npiece), dim3(256), 0, s, t, p, a.mask, n, D, H, W, (const double*)st, lval, part);
    check_launch("volume_pass3");
    hipLaunchKernelGGL(volume_final3_kernel, dim3(1), dim3(256), 0, s, (const double*)part, l.npiece, st);
    check_launch("volume_final3");
    kth_select(lval, n, 2, sel, (unsigned*)(w + l.hist), s);
    if (l.nmap_wg) {
        double* rows = (double*)(w + l.rows);
        hipLaunchKernelGGL(volume_ssim_rows_kernel<T>, dim3((unsigned)l.nrows_wg), dim3(256), 0, s, t, p, has_mask, D, H, W, a.win, l.tx, l.ty,
                           (const double*)st, rows);
        check_launch("volume_ssim_rows");
        hipLaunchKernelGGL(volume_ssim_map_kernel, dim3((unsigned)l.nmap_wg), dim3(256), 0, s, (const double*)rows, has_mask, D, H, W, a.win,
                           (const double*)st, ssim_part);
        check_launch("volume_ssim_map");
    }
    hipLaunchKernelGGL(volume_out_kernel, dim3(1), dim3(256), 0, s, (const double*)st, (const KthSel*)sel, (const double*)ssim_part,
                       (int)l.nmap_wg, has_mask, D, H, W, a.win, a.out);
    check_launch("volume_out");
}
}  // namespace

void volume_metrics_check(int D, int H, int W, int win, int elem_is_double) {
    DSD_CHECK(D >= 1 && H >= 1 && W >= 1, "volume_metrics: bad shape: D %d H %d W %d", D, H, W);
    const int64_t n = (int64_t)D * H * W;
    DSD_CHECK(n <= (int64_t)1 << DSD_VOLUME_MAX_LOG2, "volume_metrics: D*H*W = %lld voxels; up to 2^%d are taken", (long long)n,
              DSD_VOLUME_MAX_LOG2);
    DSD_CHECK(win == 0 || (win >= 3 && win <= kVmWinMax && (win & 1)), "volume_metrics: win is %d; 0 (no ssim3d) or an odd value from 3 to %d",
              win, kVmWinMax);
    DSD_CHECK(elem_is_double == 0 || elem_is_double == 1, "volume_metrics: elem_is_double is %d; 0 (float) or 1 (double)", elem_is_double);
}

size_t volume_metrics_scratch_bytes(int D, int H, int W, int win) { return vm_layout(D, H, W, win).total; }

void volume_metrics(const VolumeMetrics& a, hipStream_t s) {
    volume_metrics_check(a.D, a.H, a.W, a.win, a.elem_is_double);
    DSD_CHECK(a.target && a.pred && a.out && a.scratch, "volume_metrics: null argument");
    const VmLayout l = vm_layout(a.D, a.H, a.W, a.win);
    if (a.elem_is_double) vm_run<double>(a, l, (char*)a.scratch, s);
    else vm_run<float>(a, l, (char*)a.scratch, s);
}

void kth_double_check(int64_t n, int64_t k) {
    DSD_CHECK(n >= 1 && n <= (int64_t)1 << 31, "kth_double: n is %lld; 1 to 2^31 elements are taken", (long long)n);
    DSD_CHECK(k >= 0 && k < n, "kth_double: k is %lld; a rank from 0 to n - 1 = %lld", (long long)k, (long long)(n - 1));
}

size_t kth_double_scratch_bytes() { return vm_up(sizeof(KthSel)) + (size_t)kKthPasses * kKthBins * sizeof(unsigned); }

void kth_double(const double* x, int64_t n, int64_t k, void* scratch, double* out, hipStream_t s) {
    kth_double_check(n, k);
    DSD_CHECK(x && out && scratch, "kth_double: null argument");
    KthSel* sel = (KthSel*)scratch;
    hipLaunchKernelGGL(kth_init_kernel, dim3(1), dim3(1), 0, s, sel, (long long)k);
    check_launch("kth_init");
    kth_select(x, n, 1, sel, (unsigned*)((char*)scratch + vm_up(sizeof(KthSel))), s);
    hipLaunchKernelGGL(kth_result_kernel, dim3(1), dim3(1), 0, s, (const KthSel*)sel, out);
    check_launch("kth_result");
}

}  // namespace dsd
