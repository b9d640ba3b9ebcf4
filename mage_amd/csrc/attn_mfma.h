// Operand helpers of the matrix-core attention kernels (norm_attn.hip: attention_mfma_kernel and its few-query form) -- shared with the
// fused Q K / P V epilogues of gemm4.hip, which must produce the same bits from the same values: ONE definition of the P = hi + lo split
// and of the two MFMA calls.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 abf16x8;
typedef __attribute__((ext_vector_type(4))) short ashort4;
typedef __attribute__((ext_vector_type(4))) _Float16 ahalf4;
// HT = the 16-bit element type of q, k, v and out: unsigned short (bf16) or f16_t (MAGE_F16).  P = hi + lo in that type -- bf16: hi = the
// truncation of p, lo = the truncated residue (8 + 8 bits); f16: hi = round(p), lo = round(p - hi) (11 + 11 bits; p <= 1, the residue is
// >= 2^-24 p: inside the f16 subnormal grid's 6e-8) -- so that P V keeps fp32-class weights in both.
template <typename HT> __device__ __forceinline__ void attn_p_split(float p, short& hi, short& lo) {
    if constexpr (std::is_same<HT, f16_t>::value) {
        const _Float16 h = (_Float16)p;
        hi = __builtin_bit_cast(short, h);
        lo = __builtin_bit_cast(short, (_Float16)(p - (float)h));
    } else {
        const unsigned hb = __float_as_uint(p) & 0xffff0000u;
        hi = (short)(hb >> 16);
        lo = (short)(__float_as_uint(p - __uint_as_float(hb)) >> 16);
    }
}
template <typename HT> __device__ __forceinline__ f32x4 attn_mfma_pv(const ashort4& vt, const ashort4& p, const f32x4& o) {
    if constexpr (std::is_same<HT, f16_t>::value)
        return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(ahalf4, vt), __builtin_bit_cast(ahalf4, p), o, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vt, p, o, 0, 0, 0);
}
template <typename HT> __device__ __forceinline__ f32x4 attn_mfma_qk(const uint4& k, const uint4& q) {
    return mfma16x16x32<HT>(__builtin_bit_cast(u32x4, k), __builtin_bit_cast(u32x4, q), f32x4{0.f, 0.f, 0.f, 0.f});
}

}  // namespace
