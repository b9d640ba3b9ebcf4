// Operand helpers of the matrix-core attention kernels (attention.hip: attention_mfma_kernel and its few-query form) -- shared with the
// fused Q K / P V epilogues of gemm4.hip, which must produce the same bits from the same values: ONE definition of the P = hi + lo split
// and of the two MFMA calls -- and the two operand policies (bf16 / f16 rows, f16x3 split rows) attention_mfma_kernel is written over.
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

// Logical column c of a split row (common.h) sits at 16-bit index (c / 64) * 128 + piece * 64 + c % 64.
__device__ __forceinline__ int split_col(int c, int piece) { return ((c >> 6) << 7) + (piece << 6) + (c & 63); }

// Operand policies of attention_mfma_kernel and of the f16x3 few-query kernel (attention.hip): everything in which the f16x3 mode
// differs from the bf16 / f16 one, and nothing else -- how a Q / K / V fragment is loaded, the Q K product, the exponent's argument, the
// P = hi + lo split, how V^T is read from staged V rows, the P V product with its accumulation order over the key blocks, and the
// output rows.
//   frag           8 consecutive logical columns of a row, as PIECES 16-byte pieces;  load(row, c): c = the first logical column
//   qk(k, q)       the 16 x 16 block of S^T = K Q^T
//   exp_arg<NKB>   the argument of a probability's exponential from the raw score s: s * scale - mx, with its roundings fixed here
//                  (contraction off) instead of left to what the compiler makes of a kernel's shape; the few-query kernels call it too
//   pe, p4         one piece of a probability, and four of them (the B operand of the P V product);  psplit(p, hi, lo)
//   vt4            V^T of 4 keys x this lane's column;  vt(p, pitch, lo): p = the staged row of the first key at the column's (hi) piece,
//                  pitch = 16-bit elements between rows, lo = elements from a hi piece to its lo piece (unused without one)
//   pv<NKB>        O^T = V^T P^T over the NKB key blocks
//   out_t, ldo()   the output rows' store8 type and their leading dimension in it
//   COLS           physical 16-bit columns per head;  LO = the hi -> lo distance inside a row of q, k, v;  col(c): where logical column
//                  c's (hi) piece sits in such a row
template <typename HT>                                   // HT = unsigned short (bf16 rows) or f16_t (f16 rows)
struct attn_ops_plain {
    static constexpr int PIECES = 1, COLS = 32, LO = 0;
    struct frag { uint4 p[1]; };
    typedef short pe;
    typedef ashort4 p4;
    typedef ashort4 vt4;
    typedef HT out_t;
    static __device__ __forceinline__ int ldo(int ld) { return ld; }
    static __device__ __forceinline__ int col(int c) { return c; }
    static __device__ __forceinline__ frag load(const unsigned short* row, int c) { return frag{{*(const uint4*)(row + c)}}; }
    static __device__ __forceinline__ f32x4 qk(const frag& k, const frag& q) { return attn_mfma_qk<HT>(k.p[0], q.p[0]); }
    template <int NKB> static __device__ __forceinline__ float exp_arg(float s, float scale, float mx) {
#pragma clang fp contract(off)
        return s * scale - mx;
    }
    static __device__ __forceinline__ void psplit(float p, pe& hi, pe& lo) { attn_p_split<HT>(p, hi, lo); }
    static __device__ __forceinline__ vt4 vt(const unsigned short* p, int pitch, int) {
        vt4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (short)p[e * pitch];
        return v;
    }
    template <int NKB> static __device__ __forceinline__ f32x4 pv(const vt4 (&v)[NKB], const p4 (&phi)[NKB], const p4 (&plo)[NKB]) {
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            o = attn_mfma_pv<HT>(v[kb], phi[kb], o);
            o = attn_mfma_pv<HT>(v[kb], plo[kb], o);
        }
        return o;
    }
};

// f16x3 (the fast parity mode: q, k, v and out are SPLIT rows of f16 pieces): every product as three f16 MFMA passes -- S^T = (K_hi Q_lo^T
// + K_lo Q_hi^T) 2^-11 + K_hi Q_hi^T by v_mfma_f32_16x16x32_f16, P = hi + lo 2^-11 in f16 pieces, O^T = (V_hi^T P_lo^T + V_lo^T P_hi^T)
// 2^-11 + V_hi^T P_hi^T by 16x16x16 (all cross terms of all key blocks, the rescale, then all hi terms) -- 22-bit operands, fp32
// accumulation: fp32-class like the split GEMMs.
struct attn_ops_f16x3 {
    static constexpr int PIECES = 2, COLS = 64, LO = 64;
    static constexpr float LO_SCALE = 1.0f / MAGE_F16_LO_SCALE;
    struct frag { uint4 p[2]; };                         // hi, lo
    typedef _Float16 pe;
    typedef ahalf4 p4;
    struct vt4 { ahalf4 hi, lo; };
    typedef split_f16 out_t;
    static __device__ __forceinline__ int ldo(int ld) { return ld >> 1; }
    static __device__ __forceinline__ int col(int c) { return split_col(c, 0); }
    static __device__ __forceinline__ frag load(const unsigned short* row, int c) {
        return frag{{*(const uint4*)(row + split_col(c, 0)), *(const uint4*)(row + split_col(c, 1))}};
    }
    static __device__ __forceinline__ f32x4 qk(const frag& k, const frag& q) {
        const f16x8 kh = __builtin_bit_cast(f16x8, k.p[0]), kl = __builtin_bit_cast(f16x8, k.p[1]);
        const f16x8 qh = __builtin_bit_cast(f16x8, q.p[0]), ql = __builtin_bit_cast(f16x8, q.p[1]);
        f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh, a, 0, 0, 0);
        a *= LO_SCALE;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh, a, 0, 0, 0);
    }
    // With two key blocks s * scale - mx is ONE fma here, and two roundings everywhere else: the contraction the compiler used to find
    // in the f16x3 kernels at NKB = 2 and nowhere else, written down because the rows of this mode are pinned bit for bit.
    template <int NKB> static __device__ __forceinline__ float exp_arg(float s, float scale, float mx) {
#pragma clang fp contract(off)
        if constexpr (NKB == 2) return __builtin_fmaf(s, scale, -mx);
        else return s * scale - mx;
    }
    static __device__ __forceinline__ void psplit(float p, pe& hi, pe& lo) {
        hi = (_Float16)p;
        lo = (_Float16)((p - (float)hi) * MAGE_F16_LO_SCALE);
    }
    static __device__ __forceinline__ vt4 vt(const unsigned short* p, int pitch, int lo) {
        vt4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v.hi[e] = __builtin_bit_cast(_Float16, p[e * pitch]);
            v.lo[e] = __builtin_bit_cast(_Float16, p[e * pitch + lo]);
        }
        return v;
    }
    template <int NKB> static __device__ __forceinline__ f32x4 pv(const vt4 (&v)[NKB], const p4 (&phi)[NKB], const p4 (&plo)[NKB]) {
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            a = __builtin_amdgcn_mfma_f32_16x16x16f16(v[kb].hi, plo[kb], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x16f16(v[kb].lo, phi[kb], a, 0, 0, 0);
        }
        a *= LO_SCALE;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) a = __builtin_amdgcn_mfma_f32_16x16x16f16(v[kb].hi, phi[kb], a, 0, 0, 0);
        return a;
    }
};

}  // namespace
