// Short-sequence multi-head attention (axial / text / cross), forward: the thread-per-(query, head) kernel, the matrix-core kernel over an
// operand policy and its two few-query forms, behind mage_attention.  The backward kernels are in attention_bwd.hip.
// All HBM-bound: one pass over the data, 16-byte vector accesses, fp32 arithmetic.
#include <type_traits>

#include "common.h"
#include "attn_mfma.h"      // the MFMA attention kernels' operand helpers, shared with the fused Q K / P V epilogues of gemm4.hip

namespace {

// ------------------------------------------------------------------------------------ attention
// Workgroup = (sequence, head group).  K and V of the head group are staged once in LDS in their storage type
// (bf16 stays bf16: half the LDS bytes and half the ds_read_b128 per key, twice the resident workgroups);
// each thread then owns (query i, head h) pairs: q in registers, scores in registers (NK_MAX <= 64), softmax in
// registers, output accumulated in registers, all fp32.  Lanes of a wave that share h read the same LDS address
// (broadcast); the (up to 4) distinct heads of a wave sit 64/128 B apart: conflict-free b128 reads.
__device__ __forceinline__ void load8f(const float* p, f32x4& a, f32x4& b) {
    a = *(const f32x4*)p;
    b = *(const f32x4*)(p + 4);
}
__device__ __forceinline__ void load8f(const unsigned short* p, f32x4& a, f32x4& b) {
    const uint4 r = *(const uint4*)p;
    a = f32x4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
    b = f32x4{__uint_as_float(r.z << 16), __uint_as_float(r.z & 0xffff0000u), __uint_as_float(r.w << 16), __uint_as_float(r.w & 0xffff0000u)};
}
__device__ __forceinline__ void copy8(const float* src, float* dst) {
    *(f32x4*)dst = *(const f32x4*)src;
    *(f32x4*)(dst + 4) = *(const f32x4*)(src + 4);
}
__device__ __forceinline__ void copy8(const unsigned short* src, unsigned short* dst) { *(uint4*)dst = *(const uint4*)src; }
__device__ __forceinline__ void load8f(const f16_t* p, f32x4& a, f32x4& b) {
    const uint4 r = *(const uint4*)p;
    a = widen4<f16_t>(uint2{r.x, r.y});
    b = widen4<f16_t>(uint2{r.z, r.w});
}
__device__ __forceinline__ void copy8(const f16_t* src, f16_t* dst) { *(uint4*)dst = *(const uint4*)src; }

template <typename T, int NK_MAX, typename OT = T>   // OT: T, or (T = float) split_bf16 / split_f16: the output leaves as split rows (common.h)
__global__ __launch_bounds__(256) void attention_kernel(const mage_attn_desc d, int hg) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* ks = (T*)smem_raw;                            // [nk][hg*32]
    const int rowf = hg * 32;
    T* vs = ks + (long)d.nk * rowf;
    const int s = blockIdx.x;
    const int h0 = blockIdx.y * hg;
    const int outer = s / d.inner, in = s - outer * d.inner;
    const long q_base = (long)outer * d.q_outer_stride + in;
    const long o_base = d.o_axis_stride ? (long)outer * d.o_outer_stride + in : q_base;      // out: q's row map unless the descriptor gives its own
    const long o_step = d.o_axis_stride ? d.o_axis_stride : d.q_axis_stride;
    const long kv_base = (long)outer * d.kv_outer_stride + in;
    const T* kp = (const T*)d.k;
    const T* vp = (const T*)d.v;
    // stage K, V: nk rows x (hg*32) columns, 8 elements per thread-step
    const int vec_per_row = rowf / 8;
    for (int e = threadIdx.x; e < d.nk * vec_per_row; e += 256) {
        const int j = e / vec_per_row, c = (e - j * vec_per_row) * 8;
        const long row = kv_base + (long)j * d.kv_axis_stride;
        copy8(kp + row * d.ldk + h0 * 32 + c, ks + j * rowf + c);
        copy8(vp + row * d.ldv + h0 * 32 + c, vs + j * rowf + c);
    }
    __syncthreads();
    int klen = d.nk;
    if (d.kv_len) klen = min(klen, d.kv_len[s / d.kv_len_div]);
    const unsigned drop_thresh = d.drop_p > 0.f ? (unsigned)((double)d.drop_p * 4294967296.0) : 0u;
    const float inv_keep = 1.0f / (1.0f - d.drop_p);
    const T* qp = (const T*)d.q;
    OT* op = (OT*)d.out;
    const int ldo = std::is_same<OT, T>::value ? d.ldo : d.ldo >> 1;   // split rows: ldo counts 16-bit elements, a logical element is 4 bytes
    for (int p = threadIdx.x; p < d.nq * hg; p += 256) {
        const int hl = p / d.nq, i = p - hl * d.nq;
        const long row = q_base + (long)i * d.q_axis_stride;
        f32x4 q[8];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            load8f(qp + row * d.ldq + (h0 + hl) * 32 + c * 8, q[2 * c], q[2 * c + 1]);
            q[2 * c] *= d.scale;
            q[2 * c + 1] *= d.scale;
        }
        const int jmax = d.causal ? min(klen, i + 1 + (d.nk - d.nq)) : klen;   // bottom-right aligned causal mask
        float sc[NK_MAX];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NK_MAX; ++j) {
            float a = -INFINITY;
            if (j < jmax) {
                const T* kr = ks + j * rowf + hl * 32;
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f32x4 k0, k1;
                    load8f(kr + c * 8, k0, k1);
                    a0 += q[2 * c][0] * k0[0] + q[2 * c][1] * k0[1] + q[2 * c][2] * k0[2] + q[2 * c][3] * k0[3];
                    a1 += q[2 * c + 1][0] * k1[0] + q[2 * c + 1][1] * k1[1] + q[2 * c + 1][2] * k1[2] + q[2 * c + 1][3] * k1[3];
                }
                a = a0 + a1;
            }
            sc[j] = a;
            mx = fmaxf(mx, a);
        }
        float den = 0.f;
        f32x4 o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NK_MAX; ++j) {
            if (j < jmax) {
                float pj = expf(sc[j] - mx);
                den += pj;
                if (drop_thresh) {                   // dropout on the probabilities (train() of the text encoder): the sum stays unmasked
                    const unsigned long long idx = (((unsigned long long)s * d.n_head + (h0 + hl)) * d.nq + i) * d.nk + j;
                    pj = drop_keep(d.drop_seed * 0x9e3779b97f4a7c15ULL, idx, drop_thresh) ? pj * inv_keep : 0.f;
                }
                const T* vr = vs + j * rowf + hl * 32;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f32x4 v0, v1;
                    load8f(vr + c * 8, v0, v1);
                    o[2 * c] += pj * v0;
                    o[2 * c + 1] += pj * v1;
                }
            }
        }
        const float inv = 1.0f / den;
        OT* orow = op + (o_base + (long)i * o_step) * ldo + (h0 + hl) * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) store8(orow + c * 8, o[2 * c] * inv, o[2 * c + 1] * inv);
    }
}

// ------------------------------------------------------------------------------------ attention on the matrix cores
// 16-bit or f16x3 rows, nq <= 32 and nk <= 32 (every axial attention of the decoder, frames_length up to 32): one wave per (sequence,
// head), three MFMA steps per block of 16 queries (and per block of 16 keys).  The workgroup-per-sequence kernel is written once over
// an operand policy (attn_mfma.h) and described here with the bf16 policy's instructions; its wave-per-sequence forms for nq <= 2 follow.
//   S^T = K Q^T   (v_mfma_f32_16x16x32_bf16, operands straight from global: lane (r = lane&15, g = lane>>4) loads the 16
//                  bytes [g*8, g*8+8) of row r of K resp. Q): the result lane (i = lane&15, g) holds S^T[j = 4g+e][i], e=0..3,
//                  i.e. four consecutive keys of ITS query -- exactly the B-operand layout of the next MFMA (swapped-QK idiom).
//   softmax over j: 4 values in the lane, then across the 4 lane groups (two xor-shuffles).
//   O^T = V^T P^T (v_mfma_f32_16x16x16_bf16 per 16-dim half; P split into bf16 hi + lo so that P V keeps fp32-class weights;
//                  A operand = V^T: lane (n = lane&15, g) needs V[j = 4g+e][n]: four 2-byte reads of the V rows staged in LDS).
// Only V goes through LDS (16.5 KB per workgroup: 9 workgroups per CU keep HBM busy); the thread-per-(query, head) kernel
// below converts every K/V element to fp32 once per query (VALU time ~ HBM time at bf16); here the arithmetic is ~40
// vector instructions per (sequence, head).  Output: a lane swap gives every lane 8 consecutive dims -> one 16-byte store.
// NKB = key blocks of 16 (nk <= 16*NKB); queries are walked in blocks of 16 (nq <= 32 at the call sites: frames_length 32).
// MAXH = heads per wave (ceil(n_head / 4) rounded up to 2, 4 or 8): sizes the preloaded fragment registers; 16 heads -> 4, which
// keeps the kernel at a register count that lets 4-5 workgroups share a CU (a memory-bound kernel lives off that).
// Ops = the operand policy (attn_mfma.h): attn_ops_plain<unsigned short | f16_t> for bf16 / f16 rows, attn_ops_f16x3 for split rows of
// f16 pieces (the fast parity mode, in place of the thread-per-(query, head) fp32 kernel: 540 vs ~200 us per launch at cfg2).  The
// geometry, the mask, the softmax and the row store below are the same code for all three.
template <int NKB, int MAXH, typename Ops>
__global__ __launch_bounds__(256) void attention_mfma_kernel(const mage_attn_desc d) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned short* vs = (unsigned short*)smem_raw;     // [16*NKB][n_head*COLS + 16]: V rows as they lie in memory; rows >= nk are zero
    const int rowf = d.n_head * Ops::COLS, vpitch = rowf + 16;
    const int s = blockIdx.x;
    const int outer = s / d.inner, in = s - outer * d.inner;
    const long q_base = (long)outer * d.q_outer_stride + in;
    const long o_base = d.o_axis_stride ? (long)outer * d.o_outer_stride + in : q_base;      // out: q's row map unless the descriptor gives its own
    const long o_step = d.o_axis_stride ? d.o_axis_stride : d.q_axis_stride;
    const long kv_base = (long)outer * d.kv_outer_stride + in;
    const unsigned short* qp = (const unsigned short*)d.q;
    const unsigned short* kp = (const unsigned short*)d.k;
    const unsigned short* vp = (const unsigned short*)d.v;
    typename Ops::out_t* op = (typename Ops::out_t*)d.out;
    const int ldo = Ops::ldo(d.ldo);
    const int vec_per_row = rowf / 8;
    for (int e = threadIdx.x; e < 16 * NKB * vec_per_row; e += 256) {
        const int j = e / vec_per_row, c = (e - j * vec_per_row) * 8;
        uint4 val = uint4{0u, 0u, 0u, 0u};
        if (j < d.nk) val = *(const uint4*)(vp + (kv_base + (long)j * d.kv_axis_stride) * d.ldv + c);
        *(uint4*)(vs + j * vpitch + c) = val;
    }
    int klen = d.nk;
    if (d.kv_len) klen = min(klen, d.kv_len[s / d.kv_len_div]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    // all of this wave's K fragments up front (independent 16-byte loads; out-of-range keys clamped, masked below)
    typename Ops::frag kf[MAXH][NKB];
#pragma unroll
    for (int t = 0; t < MAXH; ++t) {
        const int h = wave + 4 * t;
        if (h < d.n_head) {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const long krow = kv_base + (long)min(kb * 16 + r, d.nk - 1) * d.kv_axis_stride;
                kf[t][kb] = Ops::load(kp + krow * d.ldk, h * 32 + g * 8);
            }
        }
    }
    __syncthreads();
    const int nqb = (d.nq + 15) >> 4;
    for (int qb = 0; qb < nqb; ++qb) {
        const int qi = qb * 16 + r;                                           // this lane's query
        const long qrow = q_base + (long)min(qi, d.nq - 1) * d.q_axis_stride;
        const int jmax = d.causal ? min(klen, qi + 1 + (d.nk - d.nq)) : klen;  // query qi sees keys j < jmax
        typename Ops::frag qf[MAXH];
#pragma unroll
        for (int t = 0; t < MAXH; ++t) {
            const int h = wave + 4 * t;
            if (h < d.n_head) qf[t] = Ops::load(qp + qrow * d.ldq, h * 32 + g * 8);
        }
#pragma unroll
        for (int t = 0; t < MAXH; ++t) {
            const int h = wave + 4 * t;
            if (h >= d.n_head) break;
            f32x4 st[NKB];
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                st[kb] = Ops::qk(kf[t][kb], qf[t]);
#pragma unroll
                for (int e = 0; e < 4; ++e) mx = fmaxf(mx, (kb * 16 + 4 * g + e < jmax) ? st[kb][e] * d.scale : -INFINITY);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float den = 0.f;
            typename Ops::p4 phi[NKB], plo[NKB];                              // P = hi + lo (lo = the residue, in the policy's pieces)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = (kb * 16 + 4 * g + e < jmax) ? expf(Ops::template exp_arg<NKB>(st[kb][e], d.scale, mx)) : 0.f;
                    den += p;
                    typename Ops::pe ph, pl;
                    Ops::psplit(p, ph, pl);
                    phi[kb][e] = ph;
                    plo[kb][e] = pl;
                }
            den += __shfl_xor(den, 16);
            den += __shfl_xor(den, 32);
            f32x4 o[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                typename Ops::vt4 vt[NKB];
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
                    vt[kb] = Ops::vt(vs + (kb * 16 + 4 * g) * vpitch + Ops::col(h * 32 + b * 16 + r), vpitch, Ops::LO);
                o[b] = Ops::template pv<NKB>(vt, phi, plo);
            }
            // lane (i = r, g) holds O[i][b*16 + 4g + e]; swap halves between neighbouring lane groups: 8 consecutive dims per lane
            const float inv = 1.0f / den;
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[0][e]), __float_as_uint(o[1][e]), false, false);
                v0[e] = __uint_as_float(sw[0]) * inv;
                v1[e] = __uint_as_float(sw[1]) * inv;
            }
            if (qi < d.nq) {
                const int col = h * 32 + 16 * (g & 1) + 8 * (g >> 1);
                store8(op + (o_base + (long)qi * o_step) * ldo + col, v0, v1);
            }
        }
    }
}

// Few queries, many sequences (the incremental AR step's temporal attention: nq = 1 or 2 new positions against a K,V cache of up to
// 32, 16384 sequences at cfg2): one WAVE per sequence, no workgroup barrier.  Per (sequence, head) the SAME instruction sequence on the
// same operand values as attention_mfma_kernel (S^T = K Q^T by one 16x16x32 MFMA, in-lane softmax + two xor-shuffles, P = hi + lo,
// O^T = V^T P^T by 16x16x16 MFMAs) -- the incremental loop's tokens stay bit-identical to the full pass's -- with the V rows in a
// wave-private LDS tile (rows beyond nk are clamped copies: their probabilities are exactly 0) and four heads' loads in flight before
// the first MFMA.  The workgroup-per-sequence kernel
// spends its time in per-workgroup latency at this shape (V staging + barrier for ONE query): 107 us per launch at cfg2 against
// ~55 us of K,V cache bytes.
// DPP row shifts (within each 16-lane row): row_shr<N>: lane r takes src of lane r - N (lanes r < N keep old); row_shl<N>: lane r takes
// lane r + N (lanes r >= 16 - N: themselves).  N = 0: src.
template <int N> __device__ __forceinline__ float row_shr_f(float old, float src) {
    if constexpr (N == 0) return src;
    else return __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(old), __float_as_uint(src), 0x110 + N, 0xf, 0xf, false));
}
template <int N> __device__ __forceinline__ unsigned row_shl_u(unsigned src) {
    if constexpr (N == 0) return src;
    else return __builtin_amdgcn_update_dpp(src, src, 0x100 + N, 0xf, 0xf, false);
}
template <int N> __device__ __forceinline__ float row_shl_f(float src) { return __uint_as_float(row_shl_u<N>(__float_as_uint(src))); }
template <int N> __device__ __forceinline__ ashort4 row_shl_s4(ashort4 src) {
    const uint2 u = __builtin_bit_cast(uint2, src);
    return __builtin_bit_cast(ashort4, uint2{row_shl_u<N>(u.x), row_shl_u<N>(u.y)});
}

template <int NKB, typename HT = unsigned short>
__global__ __launch_bounds__(256) void attention_mfma_fewq_kernel(const mage_attn_desc d) {
    typedef attn_ops_plain<HT> Ops;
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= d.n_seq) return;
    const int outer = s / d.inner, in = s - outer * d.inner;
    const long q_base = (long)outer * d.q_outer_stride + in;
    const long o_base = d.o_axis_stride ? (long)outer * d.o_outer_stride + in : q_base;      // out: q's row map unless the descriptor gives its own
    const long o_step = d.o_axis_stride ? d.o_axis_stride : d.q_axis_stride;
    const long kv_base = (long)outer * d.kv_outer_stride + in;
    const unsigned short* qp = (const unsigned short*)d.q;
    const unsigned short* kp = (const unsigned short*)d.k;
    const unsigned short* vp = (const unsigned short*)d.v;
    HT* op = (HT*)d.out;
    int klen = d.nk;
    if (d.kv_len) klen = min(klen, d.kv_len[s / d.kv_len_div]);
    const int r = lane & 15, g = lane >> 4;
    const int qi = r;                                                         // nq <= 16: one query block
    const long qrow = q_base + (long)min(qi, d.nq - 1) * d.q_axis_stride;
    long krow[NKB], krow_v[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        krow[kb] = (kv_base + (long)min(kb * 16 + r, d.nk - 1) * d.kv_axis_stride) * d.ldk;
        krow_v[kb] = (kv_base + (long)min(kb * 16 + r, d.nk - 1) * d.kv_axis_stride) * d.ldv;
    }
    // chunks of CH heads: their loads are all in flight before the first MFMA.  (Measured: a software-pipelined variant -- chunk c+1's
    // loads under chunk c's arithmetic -- needs 168 VGPRs, 2 waves per SIMD, and is SLOWER: 105 us at nk = 2 against 74; this kernel
    // lives off occupancy.)
    // V^T fragments (lane (n, g) needs V[4g+e][n], e = 0..3: a column walk): each lane loads 16 bytes of a V row like a K fragment,
    // parks them in a WAVE-PRIVATE LDS tile (no barrier: one wave's DS operations execute in order) and reads its four 2-byte values
    // back.  (Fetched as 2-byte global loads the kernel was bound by the texture addresser: 75 us at nk = 2.)
    constexpr int CH = 4, VP = 40;                                           // 80-byte LDS rows
    __shared__ unsigned short vsm[4][CH][NKB * 16][VP];
    const int wv = threadIdx.x >> 6;
    uint4 kf[1][CH][NKB], qf[1][CH];
    ashort4 vt[1][CH][2][NKB];
    auto load_chunk = [&](int buf, int h0) {
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            const int h = min(h0 + t, d.n_head - 1);
            qf[buf][t] = *(const uint4*)(qp + qrow * d.ldq + h * 32 + g * 8);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                kf[buf][t][kb] = *(const uint4*)(kp + krow[kb] + h * 32 + g * 8);
                *(uint4*)&vsm[wv][t][kb * 16 + r][g * 8] = *(const uint4*)(vp + krow_v[kb] + h * 32 + g * 8);
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < CH; ++t)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e) vt[buf][t][b][kb][e] = (short)vsm[wv][t][kb * 16 + 4 * g + e][b * 16 + r];
        __builtin_amdgcn_wave_barrier();
    };
    // One softmax for the CH heads of a chunk.  With nq <= 2 only result columns (lanes l15 =) 0, 1 of a head's 16 x 16 score block
    // are queries; the other 14 repeat them.  Every VALU instruction costs a wave 4 cycles whatever its useful lanes, and the softmax
    // (exp, max / sum trees, the hi + lo split) is ~100 of a head's ~200 instructions: so the CH heads' two columns are moved side by
    // side (head t -> lanes 2t, 2t+1 of each 16-lane row: one DPP row shift per register), scaled / masked / exponentiated / summed ONCE,
    // and moved back as each head's P operand.  Per element the same operations in the same order as the one-head form (the xor-16 /
    // xor-32 partners are the same lanes of the other key groups): bit-identical rows.
    const int jmax_p = d.causal ? min(klen, (r & 1) + 1 + (d.nk - d.nq)) : klen;      // packed lanes: query = lane parity
    auto compute_chunk = [&](int buf, int h0) {
        f32x4 sp[NKB];                                                        // packed scores
        auto gather = [&](auto T) {
            constexpr int t = decltype(T)::value;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const f32x4 stt = attn_mfma_qk<HT>(kf[buf][t][kb], qf[buf][t]);
#pragma unroll
                for (int e = 0; e < 4; ++e) sp[kb][e] = row_shr_f<2 * t>(sp[kb][e], stt[e]);
            }
        };
        gather(std::integral_constant<int, 0>{});
        gather(std::integral_constant<int, 1>{});
        gather(std::integral_constant<int, 2>{});
        gather(std::integral_constant<int, 3>{});
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, (kb * 16 + 4 * g + e < jmax_p) ? sp[kb][e] * d.scale : -INFINITY);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float den = 0.f;
        ashort4 phi_p[NKB], plo_p[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = (kb * 16 + 4 * g + e < jmax_p) ? expf(Ops::template exp_arg<NKB>(sp[kb][e], d.scale, mx)) : 0.f;
                den += p;
                short ph, pl;
                attn_p_split<HT>(p, ph, pl);
                phi_p[kb][e] = ph;
                plo_p[kb][e] = pl;
            }
        den += __shfl_xor(den, 16);
        den += __shfl_xor(den, 32);
        const float inv_p = 1.0f / den;
        auto finish = [&](auto T) {
            constexpr int t = decltype(T)::value;
            const int h = h0 + t;
            if (h >= d.n_head) return;
            ashort4 phi[NKB], plo[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                phi[kb] = row_shl_s4<2 * t>(phi_p[kb]);
                plo[kb] = row_shl_s4<2 * t>(plo_p[kb]);
            }
            const float inv = row_shl_f<2 * t>(inv_p);
            f32x4 o[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                o[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    o[b] = attn_mfma_pv<HT>(vt[buf][t][b][kb], phi[kb], o[b]);
                    o[b] = attn_mfma_pv<HT>(vt[buf][t][b][kb], plo[kb], o[b]);
                }
            }
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[0][e]), __float_as_uint(o[1][e]), false, false);
                v0[e] = __uint_as_float(sw[0]) * inv;
                v1[e] = __uint_as_float(sw[1]) * inv;
            }
            if (qi < d.nq) {
                const int col = h * 32 + 16 * (g & 1) + 8 * (g >> 1);
                store8(op + (o_base + (long)qi * o_step) * d.ldo + col, v0, v1);
            }
        };
        finish(std::integral_constant<int, 0>{});
        finish(std::integral_constant<int, 1>{});
        finish(std::integral_constant<int, 2>{});
        finish(std::integral_constant<int, 3>{});
    };
    for (int h0 = 0; h0 < d.n_head; h0 += CH) {
        load_chunk(0, h0);
        compute_chunk(0, h0);
    }
}

// The few-query form of attention_mfma_kernel over attn_ops_f16x3 (the incremental step's temporal attention in f16x3 mode): wave per
// sequence, the V pieces in a wave-private LDS tile, per (sequence, head) the policy's operations in the workgroup kernel's order (the
// incremental loop's tokens stay bit-identical to the full pass's).  Chunks of two heads; the V^T fragments are read where a head's P V
// product needs them (read in the load phase as above they cost this kernel two of its seven waves per SIMD).
template <int NKB>
__global__ __launch_bounds__(256) void attention_mfma_split_fewq_kernel(const mage_attn_desc d) {
    typedef attn_ops_f16x3 Ops;
    constexpr int CH = 2, VP = 40;
    __shared__ unsigned short vsm[4][CH][2][NKB * 16][VP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wv;
    if (s >= d.n_seq) return;
    const int outer = s / d.inner, in = s - outer * d.inner;
    const long q_base = (long)outer * d.q_outer_stride + in;
    const long o_base = d.o_axis_stride ? (long)outer * d.o_outer_stride + in : q_base;      // out: q's row map unless the descriptor gives its own
    const long o_step = d.o_axis_stride ? d.o_axis_stride : d.q_axis_stride;
    const long kv_base = (long)outer * d.kv_outer_stride + in;
    const unsigned short* qp = (const unsigned short*)d.q;
    const unsigned short* kp = (const unsigned short*)d.k;
    const unsigned short* vp = (const unsigned short*)d.v;
    Ops::out_t* op = (Ops::out_t*)d.out;
    const int ldo = Ops::ldo(d.ldo);
    int klen = d.nk;
    if (d.kv_len) klen = min(klen, d.kv_len[s / d.kv_len_div]);
    const int r = lane & 15, g = lane >> 4;
    const int qi = r;
    const long qrow = (q_base + (long)min(qi, d.nq - 1) * d.q_axis_stride) * d.ldq;
    const int jmax_p = d.causal ? min(klen, (r & 1) + 1 + (d.nk - d.nq)) : klen;      // packed lanes: query = lane parity
    long krow[NKB], vrow[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        krow[kb] = (kv_base + (long)min(kb * 16 + r, d.nk - 1) * d.kv_axis_stride) * d.ldk;
        vrow[kb] = (kv_base + (long)min(kb * 16 + r, d.nk - 1) * d.kv_axis_stride) * d.ldv;
    }
    for (int h0 = 0; h0 < d.n_head; h0 += CH) {
        Ops::frag kf[CH][NKB], qf[CH];
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            const int h = min(h0 + t, d.n_head - 1);
            qf[t] = Ops::load(qp + qrow, h * 32 + g * 8);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                kf[t][kb] = Ops::load(kp + krow[kb], h * 32 + g * 8);
                const Ops::frag vf = Ops::load(vp + vrow[kb], h * 32 + g * 8);
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) *(uint4*)&vsm[wv][t][pc][kb * 16 + r][g * 8] = vf.p[pc];
            }
        }
        __builtin_amdgcn_wave_barrier();
        // one softmax for the chunk's CH = 2 heads (their query columns side by side: attention_mfma_fewq_kernel)
        f32x4 sp[NKB];
        auto gather = [&](auto T) {
            constexpr int t = decltype(T)::value;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const f32x4 a = Ops::qk(kf[t][kb], qf[t]);
#pragma unroll
                for (int e = 0; e < 4; ++e) sp[kb][e] = row_shr_f<2 * t>(sp[kb][e], a[e]);
            }
        };
        gather(std::integral_constant<int, 0>{});
        gather(std::integral_constant<int, 1>{});
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, (kb * 16 + 4 * g + e < jmax_p) ? sp[kb][e] * d.scale : -INFINITY);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float den = 0.f;
        Ops::p4 phi_p[NKB], plo_p[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = (kb * 16 + 4 * g + e < jmax_p) ? expf(Ops::exp_arg<NKB>(sp[kb][e], d.scale, mx)) : 0.f;
                den += p;
                Ops::pe ph, pl;
                Ops::psplit(p, ph, pl);
                phi_p[kb][e] = ph;
                plo_p[kb][e] = pl;
            }
        den += __shfl_xor(den, 16);
        den += __shfl_xor(den, 32);
        const float inv_p = 1.0f / den;
        auto finish = [&](auto T) {
            constexpr int t = decltype(T)::value;
            const int h = h0 + t;
            if (h >= d.n_head) return;
            Ops::p4 phi[NKB], plo[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                phi[kb] = __builtin_bit_cast(ahalf4, row_shl_s4<2 * t>(__builtin_bit_cast(ashort4, phi_p[kb])));
                plo[kb] = __builtin_bit_cast(ahalf4, row_shl_s4<2 * t>(__builtin_bit_cast(ashort4, plo_p[kb])));
            }
            const float inv = row_shl_f<2 * t>(inv_p);
            f32x4 o[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                Ops::vt4 vt[NKB];                                             // hi at piece 0 of the tile, lo one piece further
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) vt[kb] = Ops::vt(&vsm[wv][t][0][kb * 16 + 4 * g][b * 16 + r], VP, NKB * 16 * VP);
                o[b] = Ops::pv<NKB>(vt, phi, plo);
            }
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[0][e]), __float_as_uint(o[1][e]), false, false);
                v0[e] = __uint_as_float(sw[0]) * inv;
                v1[e] = __uint_as_float(sw[1]) * inv;
            }
            if (qi < d.nq) {
                const int col = h * 32 + 16 * (g & 1) + 8 * (g >> 1);
                store8(op + (o_base + (long)qi * o_step) * ldo + col, v0, v1);
            }
        };
        finish(std::integral_constant<int, 0>{});
        finish(std::integral_constant<int, 1>{});
        __builtin_amdgcn_wave_barrier();
    }
}

// The matrix-core kernels (nq, nk, n_head <= 32), for either operand policy: the few-query kernel of the policy's mode for the incremental
// step's temporal attention, else the workgroup kernel on its (NKB, MAXH) ladder.  n_head = 32 with nk > 16 stages more than 64 KiB of
// V: the kernel's dynamic LDS limit is raised for such a launch.
template <typename Ops>
int attn_mfma_launch(const mage_attn_desc* d, hipStream_t s) {
    const int nkb = d->nk <= 16 ? 1 : 2;
    if (d->nq <= 2 && d->n_seq >= 1024 && !mage_options().attn_no_fewq) {      // the incremental step's temporal attention
        const dim3 grid((unsigned)((d->n_seq + 3) / 4));
        if constexpr (Ops::PIECES == 2) {
            if (nkb == 1) hipLaunchKernelGGL((attention_mfma_split_fewq_kernel<1>), grid, dim3(256), 0, s, *d);
            else hipLaunchKernelGGL((attention_mfma_split_fewq_kernel<2>), grid, dim3(256), 0, s, *d);
        } else {
            if (nkb == 1) hipLaunchKernelGGL((attention_mfma_fewq_kernel<1, typename Ops::out_t>), grid, dim3(256), 0, s, *d);
            else hipLaunchKernelGGL((attention_mfma_fewq_kernel<2, typename Ops::out_t>), grid, dim3(256), 0, s, *d);
        }
        MAGE_CHECK_LAUNCH("mage_attention");
        return MAGE_OK;
    }
    const size_t lds = (size_t)16 * nkb * (d->n_head * Ops::COLS + 16) * 2;
    const int hpw = (d->n_head + 3) / 4;
#define ATTN_MFMA(NKB, MH) \
    do { \
        if (lds > 64 * 1024) \
            (void)hipFuncSetAttribute((const void*)attention_mfma_kernel<NKB, MH, Ops>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
        hipLaunchKernelGGL((attention_mfma_kernel<NKB, MH, Ops>), dim3(d->n_seq), dim3(256), lds, s, *d); \
    } while (0)
    if (nkb == 1) { if (hpw <= 2) ATTN_MFMA(1, 2); else if (hpw <= 4) ATTN_MFMA(1, 4); else ATTN_MFMA(1, 8); }
    else { if (hpw <= 2) ATTN_MFMA(2, 2); else if (hpw <= 4) ATTN_MFMA(2, 4); else ATTN_MFMA(2, 8); }
#undef ATTN_MFMA
    MAGE_CHECK_LAUNCH("mage_attention");
    return MAGE_OK;
}

template <typename T>
int attn_launch(const mage_attn_desc* d, hipStream_t s) {
    if constexpr (sizeof(T) == 2) {
        // the axial attentions: short sequences on the matrix cores
        if (d->nq <= 32 && d->nk <= 32 && d->n_head <= 32 && !mage_options().attn_no_mfma) return attn_mfma_launch<attn_ops_plain<T>>(d, s);
    }
    // heads per workgroup: all of them if K,V fit 64 KiB of LDS, else halved while even; an odd group that still does not fit takes
    // its largest divisor that does (1 always does: nk <= 64), so every head count runs
    auto too_big = [&](int g) { return (long)d->nk * g * 32 * 2 * sizeof(T) > 64 * 1024; };
    int hg = d->n_head;
    while (too_big(hg) && hg > 1 && hg % 2 == 0) hg /= 2;
    if (too_big(hg)) {
        int g = hg - 1;
        while (hg % g != 0 || too_big(g)) --g;
        hg = g;
    }
    const size_t lds = (size_t)d->nk * hg * 32 * 2 * sizeof(T);
    MAGE_CHECK_ARG(lds <= 64 * 1024 && d->n_head % hg == 0, "mage_attention: nk=%d too large for LDS staging", d->nk);
    const dim3 grid(d->n_seq, d->n_head / hg), blk(256);
    if constexpr (sizeof(T) == 4) {
        if (d->out_split == MAGE_BF16X3 || d->out_split == MAGE_F16X3) {
#define ATTN_SPLIT(NK) \
    do { \
        if (d->out_split == MAGE_BF16X3) hipLaunchKernelGGL((attention_kernel<float, NK, split_bf16>), grid, blk, lds, s, *d, hg); \
        else hipLaunchKernelGGL((attention_kernel<float, NK, split_f16>), grid, blk, lds, s, *d, hg); \
    } while (0)
            if (d->nk <= 16) ATTN_SPLIT(16); else if (d->nk <= 32) ATTN_SPLIT(32); else ATTN_SPLIT(64);
#undef ATTN_SPLIT
            MAGE_CHECK_LAUNCH("mage_attention");
            return MAGE_OK;
        }
    }
    if (d->nk <= 16) hipLaunchKernelGGL((attention_kernel<T, 16>), grid, blk, lds, s, *d, hg);
    else if (d->nk <= 32) hipLaunchKernelGGL((attention_kernel<T, 32>), grid, blk, lds, s, *d, hg);
    else hipLaunchKernelGGL((attention_kernel<T, 64>), grid, blk, lds, s, *d, hg);
    MAGE_CHECK_LAUNCH("mage_attention");
    return MAGE_OK;
}

}  // namespace

namespace {
int attn_split_launch(const mage_attn_desc* d, hipStream_t s) {
    MAGE_CHECK_ARG(d->nq <= 32 && d->nk <= 32 && d->n_head <= 32 && d->n_head % 2 == 0 && d->out_split == MAGE_F16X3 && d->drop_p == 0.f,
                   "mage_attention: split (f16x3) q/k/v: nq, nk <= 32, an even head count, split output");
    MAGE_CHECK_ARG((d->ldq | d->ldk | d->ldv | d->ldo) % 128 == 0 && ((((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->out) & 255) == 0),
                   "mage_attention: split operands need leading dimensions that are multiples of 128 16-bit elements and 256-byte aligned bases");
    return attn_mfma_launch<attn_ops_f16x3>(d, s);
}
}  // namespace

extern "C" int mage_attention(const mage_attn_desc* d, void* stream) {
    MAGE_CHECK_ARG(d && d->q && d->k && d->v && d->out, "mage_attention: null pointer");
    MAGE_CHECK_ARG(d->nk >= 1 && d->nk <= 64, "mage_attention: nk=%d outside [1, 64]", d->nk);
    MAGE_CHECK_ARG(d->nq >= 1 && d->n_seq >= 1 && d->n_head >= 1 && d->inner >= 1, "mage_attention: bad sizes");
    MAGE_CHECK_ARG((d->ldq | d->ldk | d->ldv | d->ldo) % 8 == 0, "mage_attention: leading dims must be multiples of 8");
    MAGE_CHECK_ARG((((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->out) & 15) == 0,
                   "mage_attention: q, k, v and out must be 16-byte aligned (every kernel reads and writes them in 16-byte vectors)");
    MAGE_CHECK_ARG(!d->kv_len || d->kv_len_div >= 1, "mage_attention: kv_len_div must be >= 1");
    MAGE_CHECK_ARG((d->o_axis_stride == 0 && d->o_outer_stride == 0) || d->o_axis_stride > 0, "mage_attention: o_axis_stride must be > 0 when an output row map is given");
    MAGE_CHECK_ARG(d->drop_p >= 0.f && d->drop_p < 1.f && (d->drop_p == 0.f || (d->dtype == MAGE_F32 && d->out_split == 0)),
                   "mage_attention: drop_p=%g needs fp32 q/k/v (the thread-per-query kernel) and 0 <= p < 1", (double)d->drop_p);
    MAGE_CHECK_ARG(d->out_split == 0 || ((d->out_split == MAGE_BF16X3 || d->out_split == MAGE_F16X3) && (d->dtype == MAGE_F32 || d->dtype == MAGE_F16X3) &&
                                         (d->n_head * 32) % 64 == 0 && d->ldo % 128 == 0 && (((uintptr_t)d->out) & 255) == 0),
                   "mage_attention: out_split needs fp32 q/k/v, an even head count, ldo a multiple of 128 16-bit elements, out 256-byte aligned");
    if (d->dtype == MAGE_F32) return attn_launch<float>(d, (hipStream_t)stream);
    if (d->dtype == MAGE_BF16) return attn_launch<unsigned short>(d, (hipStream_t)stream);
    if (d->dtype == MAGE_F16) return attn_launch<f16_t>(d, (hipStream_t)stream);
    if (d->dtype == MAGE_F16X3) return attn_split_launch(d, (hipStream_t)stream);
    mage_set_error("mage_attention: bad dtype %d", d->dtype);
    return MAGE_EINVAL;
}
