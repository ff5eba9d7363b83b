// bf16 matrix-core helpers shared by the 2-D convolutions (conv2d_tiled.h) and the fused FeatureNet kernels (dmvs_ring.h): the operand type of
// v_mfma_f32_16x16x32_bf16, round-to-nearest conversions, the three-way split of fp32 values behind DMVS_ARITH_SPLIT, and one K = 32 step of
// a split product.
#pragma once
#include "dmvs_common.h"

typedef float f32x4_bf __attribute__((ext_vector_type(4)));

// 8 bf16 operand values of a lane for v_mfma_f32_16x16x32_bf16 (k-slots 8*(lane>>4) .. +7), as raw 16-bit patterns
#ifdef DMVS_HOST_EMULATION
typedef hipemu_s16x8 bf16x8;
__device__ __forceinline__ bf16x8 dmvs_pack_bf16x8(const float (&v)[8]) {
    bf16x8 r;
    for (int j = 0; j < 8; ++j) r[j] = (short)dmvs_f32_to_bf16(v[j]);
    return r;
}
__device__ __forceinline__ f32x4_bf dmvs_mfma_bf16(bf16x8 a, bf16x8 b, f32x4_bf c) { return hipemu_mfma_f32_16x16x32_bf16(a, b, c); }
#else
typedef short bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 dmvs_pack_bf16x8(const float (&v)[8]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const bf16x2 p = __builtin_convertvector(f32x2{v[j], v[j + 1]}, bf16x2);       // v_cvt_pk_bf16_f32: round to nearest even
        const s16x2 q = __builtin_bit_cast(s16x2, p);
        r[j] = q[0];
        r[j + 1] = q[1];
    }
    return r;
}
__device__ __forceinline__ f32x4_bf dmvs_mfma_bf16(bf16x8 a, bf16x8 b, f32x4_bf c) {
    typedef __bf16 mfma_bf16x8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mfma_bf16x8, a), __builtin_bit_cast(mfma_bf16x8, b), c, 0, 0, 0);
}
#endif

// DMVS_ARITH_SPLIT: an fp32 value as the sum of three bf16 values, hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), each rounded to
// nearest even: the two remainders are exact in fp32, |mid| <= 2^-9 |x|, |lo| <= 2^-18 |x|, and x - (hi + mid + lo) is below 2^-27 |x|.  (Splitting
// by truncation is exact but gives all three parts the sign of x: the dropped partial products then all have the product's sign and add up to
// a bias of ~1e-7 x sum |a b| -- measured 2.4x the fma chain's error on a 7x7 layer.  Rounded parts have independent signs.)  For 8 values at
// once, packed as the three k-slot operands of v_mfma_f32_16x16x32_bf16: 1.5 conversions + 2 unpacks + 2 subtractions per value.  (inf -> NaN.)
__device__ __forceinline__ void dmvs_bf16x8_to_f32(const bf16x8& p, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = __uint_as_float((uint32_t)(uint16_t)p[j] << 16);
}
__device__ __forceinline__ void dmvs_split3_bf16x8(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    float f[8], r1[8], r2[8];
    h = dmvs_pack_bf16x8(v);
    dmvs_bf16x8_to_f32(h, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) r1[j] = v[j] - f[j];
    m = dmvs_pack_bf16x8(r1);
    dmvs_bf16x8_to_f32(m, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) r2[j] = r1[j] - f[j];
    l = dmvs_pack_bf16x8(r2);
}

// One K = 32 step of a split product, for NG independent accumulators that share the weight operand: THE ORDER of the six partial products
// (pixel part * weight part), smallest first: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi; the three dropped ones are below 2^-26 of the product.
// The partial product is outermost, so that an accumulator is re-used NG instructions later.  PIX_FIRST: the pixels are the first MFMA operand
// (D[pixel][cout]), else the weights (D[cout][pixel]).  Bit-equality between the fused kernels and the launches they replace rests on every
// split kernel issuing this order per accumulator: conv2d_tiled.h (DMVS_SPLIT_PRODUCT) and conv1_pair.hip (conv_group, which interleaves its
// operand reads with the six instructions) spell it out by hand.
template <int NG, bool PIX_FIRST>
__device__ __forceinline__ void dmvs_split_step(const bf16x8* ph, const bf16x8* pm, const bf16x8* pl, const bf16x8& wh, const bf16x8& wm, const bf16x8& wl, f32x4_bf* acc) {
    auto mf = [&](const bf16x8* p, const bf16x8& w) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = PIX_FIRST ? dmvs_mfma_bf16(p[g], w, acc[g]) : dmvs_mfma_bf16(w, p[g], acc[g]);
    };
    mf(pl, wh);
    mf(ph, wl);
    mf(pm, wm);
    mf(pm, wh);
    mf(ph, wm);
    mf(ph, wh);
}

// Four fp32 values as bf16 triples into k-slots 0-3 or 4-7 of a [plane hi / mid / lo][position][8 channels] image: one 8-byte store per plane.
// dst = the half entry of the hi plane, plane_u32x2 = a plane's size in 8-byte units.
typedef uint32_t dmvs_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dmvs_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dmvs_store_split4(const float (&v4)[4], dmvs_u32x2* dst, int plane_u32x2) {
    const float v[8] = {v4[0], v4[1], v4[2], v4[3], 0.0f, 0.0f, 0.0f, 0.0f};
    bf16x8 h8, m8, l8;
    dmvs_split3_bf16x8(v, h8, m8, l8);
    const dmvs_u32x4 hh = __builtin_bit_cast(dmvs_u32x4, h8), mm = __builtin_bit_cast(dmvs_u32x4, m8), ll = __builtin_bit_cast(dmvs_u32x4, l8);
    dst[0] = dmvs_u32x2{hh[0], hh[1]};
    dst[plane_u32x2] = dmvs_u32x2{mm[0], mm[1]};
    dst[2 * plane_u32x2] = dmvs_u32x2{ll[0], ll[1]};
}
