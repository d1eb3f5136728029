// device_common.h — what the device code of every translation unit shares: the vector types, the split-MFMA arithmetic
// (bf16x6 / bf16x3 / f16x3, the library's default arithmetic), the buffer-resource idiom, the LDS-DMA wrapper, exact SiLU.
// One definition each; a kernel's own design notes stay with the kernel.
//
// The split.  gfx950 has no TF32/xf32; its fp32-input MFMA runs at 1/16 of the bf16 rate.  An fp32 value is written EXACTLY
// as a sum of three bf16 values (8 + 8 + 8 significand bits): piece 1 = round(a), piece 2 = round(a - piece 1), piece 3 =
// round(a - piece 1 - piece 2); each subtraction is exact in fp32, so a = a1 + a2 + a3 up to 2^-24 |a|.  With fp32 accumulation
//   bf16x6:  a1w1 + a1w2 + a2w1 + a2w2 + a1w3 + a3w1   drops only terms <= 2^-24 |a w|  -> fp32-grade result
//            (measured on the CPU oracle: 9e-7 rel-L2 on the full network's output, the same as fp32 re-ordering noise)
//   bf16x3:  a1w1 + a1w2 + a2w1                         drops terms ~2^-16..2^-17 |a w| -> 1.5e-5 on the network output
// at 6 (resp. 3) v_mfma_f32_32x32x16_bf16 per 16 k instead of 8 v_mfma_f32_32x32x2_f32: 2.67x (5.3x) fewer matrix-pipe
// cycles.  f16x3 is the three-product form on fp16 pieces (11 significand bits each, but range +-65504 only: an operand
// beyond it cannot be represented, and split4 raises the caller's overflow flag instead of silently producing inf).
// Term order: the products are accumulated SMALLEST TERMS FIRST (mfma6), so that the small terms are not absorbed one by
// one into an accumulator that already holds the large one.  Every parity bar of the test suite rests on this order and on
// the rounding sequence of split4 being the same in every kernel: change them here or nowhere.
#pragma once
#include "kernels.h"

#include <type_traits>

namespace dsd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- 16-bit piece / fragment traits: bf16 (8 significand bits, fp32's exponent range) or fp16 (11 bits, range +-65504).
// pk packs two floats (rounded) into one dword, lo / hi widen its halves back; mfma is v_mfma_f32_32x32x16 on an f32x16
// accumulator and v_mfma_f32_16x16x32 on an f32x4 one.
template <typename T> struct Piece;
template <> struct Piece<__bf16> {
    typedef bf16x8 v8;
    typedef bf16x4 v4;
    static __device__ __forceinline__ unsigned pk(float a, float b) {
        bf16x2 t;
        t[0] = (__bf16)a;
        t[1] = (__bf16)b;
        return __builtin_bit_cast(unsigned, t);
    }
    static __device__ __forceinline__ float lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
    static __device__ __forceinline__ float hi(unsigned p) { return __builtin_bit_cast(float, p & 0xFFFF0000u); }
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Piece<_Float16> {
    typedef f16x8 v8;
    typedef f16x4 v4;
    static __device__ __forceinline__ unsigned pk(float a, float b) {
        f16x2 t;
        t[0] = (_Float16)a;
        t[1] = (_Float16)b;
        return __builtin_bit_cast(unsigned, t);
    }
    static __device__ __forceinline__ float lo(unsigned p) { return (float)__builtin_bit_cast(f16x2, p)[0]; }
    static __device__ __forceinline__ float hi(unsigned p) { return (float)__builtin_bit_cast(f16x2, p)[1]; }
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <bool F16> using Elt = Piece<std::conditional_t<F16, _Float16, __bf16>>;                       // by arithmetic flag
template <typename V8> using PieceOf = Piece<std::conditional_t<std::is_same<V8, f16x8>::value, _Float16, __bf16>>;   // by fragment type

// ---- the split: 4 fp32 -> NP pieces each; out[p] = 4 packed 16-bit values (8 bytes)
template <int NP, bool F16 = false>
__device__ __forceinline__ void split4(f32x4 v, u32x2 (&out)[NP], int* ovf = nullptr) {
    float a = v.x, b = v.y, c = v.z, d = v.w;
    if (F16 && ovf) {   // fp16 pieces cannot hold |x| > 65504: flag it instead of silently producing inf
        const float m = fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d)));
        if (!(m <= 65504.f)) *ovf = 1;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const unsigned p01 = Elt<F16>::pk(a, b), p23 = Elt<F16>::pk(c, d);
        out[p].x = p01;
        out[p].y = p23;
        if (p + 1 < NP) {
            a -= Elt<F16>::lo(p01);
            b -= Elt<F16>::hi(p01);
            c -= Elt<F16>::lo(p23);
            d -= Elt<F16>::hi(p23);
        }
    }
}
// 8 fp32 (the 8 consecutive k of one MFMA operand fragment) -> NP fragments of 8 pieces
template <int NP, bool F16>
__device__ __forceinline__ void split8(f32x4 lo, f32x4 hi, typename Elt<F16>::v8 (&out)[NP], int* ovf) {
    typedef typename Elt<F16>::v8 v8;
    u32x2 pl[NP], ph[NP];
    split4<NP, F16>(lo, pl, ovf);
    split4<NP, F16>(hi, ph, ovf);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        u32x4 v;
        v.x = pl[q].x; v.y = pl[q].y; v.z = ph[q].x; v.w = ph[q].y;
        out[q] = __builtin_bit_cast(v8, v);
    }
}
// The bf16x6 split of the attention and Winograd kernels (attention.hip, attention_wide.hip, conv_wino.hip; three copies
// before).  The same roundings and subtractions as split8<3, false> above, value by value, but stated pair by pair
// instead of four floats at a time — and KEPT APART for that: forwarded to the body above, the eleven attention_split /
// attention_wide_split kernels and conv_wino_kernel come out with another instruction schedule (4 to 28 bytes longer), and
// a single body written over arrays changes the convolution kernels as well.  Every kernel must stay byte-identical
// (tools/kernel_resources.py --compare), so the statement order of each family is part of what is preserved here.
__device__ __forceinline__ void split8(const float (&v0)[8], bf16x8 (&out)[3]) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v0[i];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        u32x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned pk = Elt<false>::pk(v[2 * i], v[2 * i + 1]);
            w[i] = pk;
            if (q < 2) {
                v[2 * i] -= Elt<false>::lo(pk);
                v[2 * i + 1] -= Elt<false>::hi(pk);
            }
        }
        out[q] = __builtin_bit_cast(bf16x8, w);
    }
}
__device__ __forceinline__ void split8(f32x4 lo, f32x4 hi, bf16x8 (&out)[3]) {
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    split8(v, out);
}

// ---- c += a * b on pieces, smallest terms first: the six products of NP = 3, the three of NP = 2 (the three-product
// arithmetics keep two pieces per operand).  ACC = f32x16 (32x32x16) or f32x4 (16x16x32).
template <int NP, typename V8, typename ACC>
__device__ __forceinline__ void mfma6(const V8 (&a)[NP], const V8 (&b)[NP], ACC& c) {
    typedef PieceOf<V8> E;
    if constexpr (NP == 3) {
        c = E::mfma(a[2], b[0], c);
        c = E::mfma(a[0], b[2], c);
        c = E::mfma(a[1], b[1], c);
    }
    c = E::mfma(a[1], b[0], c);
    c = E::mfma(a[0], b[1], c);
    c = E::mfma(a[0], b[0], c);
}

// ---- the scalar split of the weight-preparation kernels: dst[i] = the 16 bits of the next piece of the residual r
// (carried in fp32 or fp64), r -= piece.  (wino_pack_kernel, conv_wino.hip, keeps these three lines written out: through
// this function its index arithmetic is scheduled ahead of the conversion and the kernel's bytes change.)
template <typename T, typename R, typename I>
__device__ __forceinline__ void store_piece(unsigned short* dst, I i, R& r) {
    const T b = (T)(float)r;
    dst[i] = __builtin_bit_cast(unsigned short, b);
    r -= (R)(float)b;
}

// ---- raw buffer addressing: a lane whose byte offset is out of range reads zeros (the hardware range check is the
// kernels' padding); OOB must not wrap when a small immediate or scalar offset is added to it
static constexpr unsigned OOB = 0xFFFFFFF0u;
static constexpr int RSRC_DWORD3 = 0x00020000;   // fourth dword of the resource: DATA_FORMAT = 32 bit, no stride, no swizzle
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, RSRC_DWORD3);
}
// 16 B per lane from a buffer resource straight into LDS (lane-linear from the wave-uniform `lds`).  A __device__ function of
// its own: the target builtin directly inside a __global__ template makes the HOST pass drop the instantiation silently.
static __device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, unsigned char* lds, unsigned voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (void __attribute__((address_space(3)))*)lds, 16, voff, soff, 0, 0);
}

// ---- exact SiLU (expf and an IEEE division).  A hardware exp2 / reciprocal form was measured in the GroupNorm apply pass:
// 18.9 -> 18.4 ms per step for ~3e-7 of extra error; not taken.  (conv_out1.hip keeps such a form, silu_fast_f, for itself.)
__device__ __forceinline__ float silu_f(float v) { return v / (1.f + expf(-v)); }

}  // namespace dsd
