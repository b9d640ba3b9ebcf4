// Codebook quantiser (nearest neighbour), embedding gathers, row argmax and cross entropy.
// Integer/index outputs here must be bit-exact against the reference, so the distance follows the
// reference FORMULA (vqvae_model.py:14-21): fl32(fl32(|c|^2 + |z|^2) - 2*<z,c>), first minimum wins.
#include "common.h"
#include "../../include/mage_hip_ext.h"

namespace {

__global__ __launch_bounds__(256) void vq_prepare_kernel(const float* __restrict__ cb, int K, int D,
                                                         float* __restrict__ cbt, float* __restrict__ c2) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const float v = cb[(long)k * D + d];
        cbt[(long)d * K + k] = v;
        s += (double)v * (double)v;
    }
    c2[k] = (float)s;
}

struct Best {
    float d0; int i0; float d1;     // best distance, its index, second-best distance
};
__device__ __forceinline__ void best_push(Best& b, float d, int i) {
    if (d < b.d0 || (d == b.d0 && i < b.i0)) { b.d1 = b.d0; b.d0 = d; b.i0 = i; }
    else if (d < b.d1) b.d1 = d;
}
__device__ __forceinline__ Best best_wave_reduce(Best b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od0 = __shfl_xor(b.d0, o, 64), od1 = __shfl_xor(b.d1, o, 64);
        const int oi0 = __shfl_xor(b.i0, o, 64);
        if (od0 < b.d0 || (od0 == b.d0 && oi0 < b.i0)) { b.d1 = fminf(b.d0, od1); b.d0 = od0; b.i0 = oi0; }
        else b.d1 = fminf(b.d1, od0);
    }
    return b;
}

// 16 rows of z per workgroup; every thread owns KPT codes (k = tid + 256*kk) for all 16 rows.
// Dot products are accumulated in fp64 (FP64 vector rate on CDNA4 is half the fp32 rate; this kernel is
// tiny) and rounded once, so the only fp32 roundings left are the ones the reference formula itself has.
template <int KPT>
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* __restrict__ z, const float* __restrict__ cbt,
                                                         const float* __restrict__ c2, long M, int D, int K,
                                                         int64_t* __restrict__ idx, float* __restrict__ margin) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* zs = (float*)smem_raw;                    // [16][D]
    float* x2s = zs + 16 * D;                        // [16]
    float* ds = x2s + 16;                            // [16][K]
    const long r0 = (long)blockIdx.x * 16;
    for (int e = threadIdx.x; e < 16 * D / 4; e += 256) {
        const int r = e / (D / 4), c = (e - r * (D / 4)) * 4;
        *(f32x4*)(zs + r * D + c) = (r0 + r < M) ? *(const f32x4*)(z + (r0 + r) * D + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s += (double)zs[threadIdx.x * D + d] * (double)zs[threadIdx.x * D + d];
        x2s[threadIdx.x] = (float)s;
    }
    double acc[KPT][16];
#pragma unroll
    for (int kk = 0; kk < KPT; ++kk)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kk][r] = 0.0;
    for (int d = 0; d < D; d += 4) {
        float c[KPT][4];
#pragma unroll
        for (int kk = 0; kk < KPT; ++kk) {
            const int k = threadIdx.x + 256 * kk;
#pragma unroll
            for (int e = 0; e < 4; ++e) c[kk][e] = (k < K) ? cbt[(long)(d + e) * K + k] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x4 zv = *(const f32x4*)(zs + r * D + d);
#pragma unroll
            for (int kk = 0; kk < KPT; ++kk)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[kk][r] = fma((double)zv[e], (double)c[kk][e], acc[kk][r]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KPT; ++kk) {
        const int k = threadIdx.x + 256 * kk;
        if (k < K) {
            const float ck = c2[k];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = ck + x2s[r];                       // fl32(|c|^2 + |z|^2)
                ds[r * K + k] = fmaf(-2.0f, (float)acc[kk][r], s); // fl32(s - 2*dot)
            }
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < 16; r += 4) {
        if (r0 + r >= M) break;
        Best b{INFINITY, 0x7fffffff, INFINITY};
        for (int k = lane; k < K; k += 64) best_push(b, ds[r * K + k], k);
        b = best_wave_reduce(b);
        if (lane == 0) {
            idx[r0 + r] = b.i0;
            if (margin) margin[r0 + r] = b.d1 - b.d0;
        }
    }
}

// The same quantiser on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: D[m][n] += sum_k A[m][k] B[n][k], A lane (m = lane & 15,
// g = lane >> 4) feeds A[m][k = g], B lane (n, g) feeds B[n][g], result lane (n, g) holds D[g + 4e][n], e = 0..3 -- the fp64
// variant interleaves the rows, unlike the 32-bit MFMAs' D[4g + e][n]).  A = 16 rows of z
// (straight from global: a lane re-reads its row 4 bytes at a time, L1-resident), B = 16 codes of the transposed codebook (64-byte
// segments per k), so a lane ends up with the fp64 dot products of ITS code with four rows; the distance keeps the reference formula
// fl32(fl32(|c|^2 + |z|^2) - 2 <z, c>) and the first minimum wins.  Workgroup = RT x 16 rows; its NWV waves split the codebook
// (NT tiles of 16 codes each); the per-row (best, index, second best) triples are merged across the 16 lanes of a code group, then
// across the waves through LDS.  The dot products differ from the VALU kernel's only in fp64 summation order (1e-16 relative).
// The thread-per-code kernel above converted every operand to fp64 per use: 5.9 ms for 40 960 vectors at D = 1024, K = 512.
typedef __attribute__((ext_vector_type(4))) double f64x4;

__device__ __forceinline__ void best_merge(Best& b, float od0, int oi0, float od1) {
    if (od0 < b.d0 || (od0 == b.d0 && oi0 < b.i0)) { b.d1 = fminf(b.d0, od1); b.d0 = od0; b.i0 = oi0; }
    else b.d1 = fminf(b.d1, od0);
}

template <int NT, int RT, int NWV>
__global__ __launch_bounds__(64 * NWV) void vq_nearest_mfma_kernel(const float* __restrict__ z, const float* __restrict__ cbt,
                                                              const float* __restrict__ c2, long M, int D, int K,
                                                              int64_t* __restrict__ idx, float* __restrict__ margin) {
    __shared__ float sd0[NWV][RT * 16], sd1[NWV][RT * 16];
    __shared__ int si0[NWV][RT * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const long r0 = (long)blockIdx.x * (RT * 16);
    const int code0 = wave * NT * 16;                                  // this wave's slice of the codebook
    const float* zrow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) zrow[rt] = z + min(r0 + rt * 16 + l15, M - 1) * (long)D + g;
    int ccol[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) ccol[t] = min(code0 + t * 16 + l15, K - 1);
    f64x4 acc[RT][NT];
    double x2[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        x2[rt] = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int d = 0; d < D; d += 4) {
        double a[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            a[rt] = (double)zrow[rt][d];
            x2[rt] = fma(a[rt], a[rt], x2[rt]);
        }
        const float* cb = cbt + (long)(d + g) * K;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double b = (double)cb[ccol[t]];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], b, acc[rt][t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        // |z|^2 of row l15: this lane summed its k = g slice
        double s = x2[rt];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float x2f = (float)s;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xr = __shfl(x2f, g + 4 * e);                   // |z|^2 of the row this accumulator element belongs to
            Best b{INFINITY, 0x7fffffff, INFINITY};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int code = code0 + t * 16 + l15;
                if (code < K) {
                    const float sck = c2[code] + xr;                                    // fl32(|c|^2 + |z|^2)
                    best_push(b, fmaf(-2.0f, (float)acc[rt][t][e], sck), code);         // fl32(s - 2*dot)
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {                          // across the 16 lanes (codes) of this lane group
                const float od0 = __shfl_xor(b.d0, o), od1 = __shfl_xor(b.d1, o);
                const int oi0 = __shfl_xor(b.i0, o);
                best_merge(b, od0, oi0, od1);
            }
            if (l15 == 0) {
                const int r = rt * 16 + g + 4 * e;
                sd0[wave][r] = b.d0;
                si0[wave][r] = b.i0;
                sd1[wave][r] = b.d1;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < RT * 16 && r0 + threadIdx.x < M) {
        Best b{sd0[0][threadIdx.x], si0[0][threadIdx.x], sd1[0][threadIdx.x]};
#pragma unroll
        for (int w = 1; w < NWV; ++w) best_merge(b, sd0[w][threadIdx.x], si0[w][threadIdx.x], sd1[w][threadIdx.x]);
        idx[r0 + threadIdx.x] = b.i0;
        if (margin) margin[r0 + threadIdx.x] = b.d1 - b.d0;
    }
}

template <typename OT>
__global__ __launch_bounds__(256) void embedding_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                        OT* __restrict__ out, long n, int C, int n_table, int relu,
                                                        long group, long group_stride, long off, long inner, long inner_stride,
                                                        int* __restrict__ err) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    long id = ids[i];
    if (id < 0 || id >= n_table) {          // the reference raises IndexError here: reported by mage_check_device_errors
        if (lane == 0) mage_raise(err, MAGE_DEVERR_EMBEDDING_ID, id, n_table);
        id = id < 0 ? 0 : n_table - 1;      // stay memory-safe meanwhile
    }
    const long ig = i % group;
    const long orow = (i / group) * group_stride + (ig / inner) * inner_stride + (ig % inner) + off;
    const float* src = table + id * C;
    OT* dst = out + orow * C;
    for (int c = lane * 4; c < C; c += 256) {
        f32x4 v = *(const f32x4*)(src + c);
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        store4(dst + c, v);
    }
}

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group,
                                                     long in_stride, long in_off, int64_t* __restrict__ out,
                                                     long out_stride, long out_off, float* __restrict__ margin) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const long gi = i / group, gr = i - gi * group;
    const float* p = logits + (gi * in_stride + gr + in_off) * ld;
    Best b{INFINITY, 0x7fffffff, INFINITY};          // minimise the negated logit: first maximum wins
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 v = *(const f32x4*)(p + k);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) best_push(b, -v[e], k + e);
    }
    b = best_wave_reduce(b);
    if (lane == 0) {
        out[gi * out_stride + gr + out_off] = b.i0;
        if (margin) margin[i] = b.d1 - b.d0;
    }
}

// ---- seeded token sampling (mage_sample_tokens): temperature, top-k, top-p, Gumbel-max.  The rule, for one row:
//   inputs: fp32 logits z[0..K), inv_t = (float)(1.0 / temperature) (host), top_k (0 = off), top_p in (0, 1] (1 = off), the row's clip
//   seed (uint64) and the token position pos = frame * h*w + pixel (frame = index of the generated frame, 0 .. L-2).
//   1. s_j = z_j * inv_t (one fp32 multiply).  A NaN logit is never selected (it is in no set below).
//   2. top-k: if 0 < top_k < K, A = { j : s_j >= the top_k-th largest s } (ties at the boundary kept: |A| may exceed top_k; fewer than
//      top_k non-NaN logits: A = all of them); otherwise A = every code.
//   3. top-p: if top_p < 1, w_j = exp(s_j - max_A s) for j in A, W = sum_A w_j, tau = the largest value v among { s_j : j in A } with
//      sum_{j in A, s_j >= v} w_j >= top_p * W, N = { j in A : s_j >= tau } (ties kept); otherwise N = A.
//   4. Gumbel-max on a stateless counter (hash32, common.h):
//      u_j = ((hash32(seed * 0x9e3779b97f4a7c15 + (pos * K + j)) >> 8) + 0.5) * 2^-24   (uint64 wrap-around arithmetic),
//      g_j = -log(-log(u_j)), token = the smallest j in N that maximises s_j + g_j (no selectable code at all: token 0).
// A token's random stream depends on its clip's seed, frame, pixel and code only: not on the batch size, the clip's place in the batch,
// the AR mode, the number of streams or graph replay.  top_k == 1 is greedy by definition: mage_argmax's kernel (first maximum wins).
// One wave per row, the row in registers (NV values per lane, 16-byte loads; code k = c*256 + lane*4 + e of chunk c).  The selections are
// bit-by-bit bisections over order-preserving uint keys of s: top-k counts with ballots (a scalar count, no shuffles), top-p sums the w_j
// with fixed-order butterflies (every lane holds the same bits).  Where the sums are rounded (W, the masses) a row whose boundary mass is
// within fp32 rounding of top_p * W may keep one value more or less than the exact rule; nothing else is approximate.
__device__ __forceinline__ unsigned sample_key(float s) {       // order-preserving; -0 == +0; NaN -> 0 (below every number: never kept)
    unsigned u = __float_as_uint(s);
    if (s != s) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// -log(u) of the 24-bit uniform u = (m + 0.5) 2^-24, never rounded: u itself is exact in fp32 below 1/2, 1 - u above (where log1p takes it)
__device__ __forceinline__ float sample_neglog_u(unsigned m) {
    return m < (1u << 23) ? -logf(((float)m + 0.5f) * 0x1p-24f) : -log1pf(-(((float)((1u << 24) - 1u - m) + 0.5f) * 0x1p-24f));
}
// g = -log(-log(u))
__device__ __forceinline__ float sample_gumbel(unsigned long long ctr) {
    return -logf(sample_neglog_u(hash32(ctr) >> 8));
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// Chunk c of a row in sample_kernel's layout: one 16-byte load, codes k = c*256 + lane*4 + e, 0 past K.
__device__ __forceinline__ f32x4 sample_row_chunk(const float* __restrict__ p, int lane, int K, int c) {
    const int k = c * 256 + lane * 4;
    return k < K ? *(const f32x4*)(p + k) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// Steps 1-3 of the rule for one row: s (the scaled logits), key (0: not selectable -- NaN, or past K) and the returned threshold lo >= 1
// with N = { j : key_j >= lo }.  row(c) gives chunk c of the row (sample_kernel loads it there and then, token_stats_kernel hands over the
// registers it read once).  THE filter: mage_sample_tokens draws from this set and mage_token_stats reports on it, so the two agree bit
// for bit on every row, the ones whose rounded top-p masses keep a value more or less than the exact rule included.
template <int NV, bool TOPK, bool TOPP, typename ROW>
__device__ __forceinline__ unsigned sample_filter(ROW row, int lane, int K, float inv_t, int top_k, float top_p, float (&s)[NV],
                                                  unsigned (&key)[NV]) {
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const int k = c * 256 + lane * 4;
        const f32x4 v = row(c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s[c * 4 + e] = __fmul_rn(v[e], inv_t);
            key[c * 4 + e] = k < K ? sample_key(s[c * 4 + e]) : 0u;
        }
    }
    unsigned lo = 1u;                                   // the candidate set: key >= lo
    if constexpr (TOPK) {                               // the largest t with #{key >= t} >= top_k: the top_k-th largest key
        unsigned t = 0u;
        auto bit = [&](int b) {
            const unsigned c = t | (1u << b);
            int n = 0;
#pragma unroll
            for (int e = 0; e < NV; ++e) n += __popcll(__ballot(key[e] >= c));
            if (n >= top_k) t = c;
        };
        // NV = 4, 32 x 4 ballots: straight-line code, which the compiler chose by itself while this loop stood in sample_kernel (K = 256,
        // top-k only: 40 against 43 us as a loop); every other instance is the loop it always was
        if constexpr (NV == 4) {
#pragma unroll
            for (int b = 31; b >= 0; --b) bit(b);
        } else {
            for (int b = 31; b >= 0; --b) bit(b);
        }
        lo = max(t, 1u);
    }
    if constexpr (TOPP) {
        unsigned km = 0u;
#pragma unroll
        for (int e = 0; e < NV; ++e) km = max(km, key[e]);
        km = wave_max_u32(km);
        if (km >= lo) {                                 // else: nothing selectable
            const float smax = sample_key_value(km);
            float w[NV], wl = 0.f;
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                w[e] = key[e] >= lo ? expf(s[e] - smax) : 0.f;
                wl += w[e];
            }
            const float target = __fmul_rn(top_p, wave_sum(wl));
            // the largest key t in [lo, km] with mass(key >= t) >= target; mass(>= lo) = W >= target.  The bits above the highest one in which
            // lo and km differ are common to every key in between: the bisection starts below them (mass(>= t) = W there too).
            const unsigned d = lo ^ km;
            const int hb = d ? 31 - __builtin_clz(d) : -1;
            unsigned t = hb >= 0 ? (km & ~((2u << hb) - 1u)) : km;
            for (int b = hb; b >= 0; --b) {
                const unsigned c = t | (1u << b);
                float ml = 0.f;
#pragma unroll
                for (int e = 0; e < NV; ++e) ml += key[e] >= c ? w[e] : 0.f;
                const float m = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wave_sum(ml))));
                if (m >= target) t = c;
            }
            lo = max(t, lo);
        }
    }
    return lo;
}

template <int NV, bool TOPK, bool TOPP>
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group,
                                                     long in_stride, long in_off, int64_t* __restrict__ out, long out_stride,
                                                     long out_off, const int64_t* __restrict__ seeds, long pos_off, float inv_t,
                                                     int top_k, float top_p) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const long gi = i / group, gr = i - gi * group;
    const float* p = logits + (gi * in_stride + gr + in_off) * ld;
    float s[NV];
    unsigned key[NV];
    const unsigned lo = sample_filter<NV, TOPK, TOPP>([=](int c) { return sample_row_chunk(p, lane, K, c); }, lane, K, inv_t, top_k, top_p,
                                                      s, key);                                    // the candidate set: key >= lo
    const unsigned long long ctr = (unsigned long long)seeds[gi] * 0x9e3779b97f4a7c15ULL
                                   + (unsigned long long)(pos_off + gr) * (unsigned long long)K;
    float best = -INFINITY;
    int bj = 0x7fffffff;
    if constexpr (TOPK || TOPP) {
        // a filtered set is small: each lane draws for its own candidates one at a time (the wave runs as many rounds as the fullest lane
        // holds), instead of paying the Gumbel transform -- the dominant cost -- in every slot some lane of the wave needs
        unsigned long long pend = 0;
#pragma unroll
        for (int e = 0; e < NV; ++e) pend |= (unsigned long long)(key[e] >= lo) << e;
        while (pend) {
            const int e0 = __builtin_ctzll(pend);
            pend &= pend - 1;
            float sv = 0.f;
#pragma unroll
            for (int e = 0; e < NV; ++e) sv = e == e0 ? s[e] : sv;
            const int j = (e0 >> 2) * 256 + lane * 4 + (e0 & 3);
            const float v = sv + sample_gumbel(ctr + (unsigned long long)j);
            if (v > best || (v == best && j < bj)) { best = v; bj = j; }
        }
    } else {
        // nothing filtered: lo == 1, and key >= 1 says no more than "a code of the row, not NaN" (sample_key) -- asked of s itself, so that
        // this instance holds no key registers through the Gumbel transforms
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int j = (e >> 2) * 256 + lane * 4 + (e & 3);
            if (j < K && s[e] == s[e]) {
                const float v = s[e] + sample_gumbel(ctr + (unsigned long long)j);
                if (v > best || (v == best && j < bj)) { best = v; bj = j; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (lane == 0) out[gi * out_stride + gr + out_off] = bj == 0x7fffffff ? 0 : bj;
}

__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                      long rows, int K, float* __restrict__ row_loss, int* __restrict__ err) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + i * K;
    float mx = -INFINITY;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, p[k]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(p[k] - mx);
    s = wave_sum(s);
    if (lane == 0) {
        long tg = target[i];
        if (tg < 0 || tg >= K) {
            mage_raise(err, MAGE_DEVERR_CE_TARGET, tg, K);
            tg = 0;
        }
        row_loss[i] = (logf(s) + mx) - p[tg];
    }
}

__global__ __launch_bounds__(1024) void sum_kernel(const float* __restrict__ v, long n, float* __restrict__ out, double inv) {
    __shared__ double red[16];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) s += (double)v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        out[0] = (float)(t * inv);
    }
}

// ---- token log-probabilities (mage_token_logprob) and per-clip scores (mage_clip_scores).
// lp = z_t - (m + log sum_j exp(z_j - m)), m = max_j z_j: the log-softmax of a row gathered at its token.  One wave per row, the row in
// registers in sample_kernel's layout (code k = c*256 + lane*4 + e of chunk c).  Every reduction has a fixed order (a lane adds its own
// terms in register order, the lanes meet in an xor butterfly), so a row's bits depend on the row alone.  -inf logits add exp(-inf) = 0;
// a NaN logit, or a row whose maximum is not finite (inf - inf), makes the sum NaN and so the result; z_t = -inf gives -inf.  expf / logf
// are the accurate ones.
template <int NV>
__global__ __launch_bounds__(256) void token_logprob_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group,
                                                            long in_stride, long in_off, const int64_t* __restrict__ tokens,
                                                            float* __restrict__ logprob, long tok_stride, long tok_off,
                                                            int* __restrict__ err) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const long gi = i / group, gr = i - gi * group;
    const float* p = logits + (gi * in_stride + gr + in_off) * ld;
    float z[NV];
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const int k = c * 256 + lane * 4;
        const f32x4 v = k < K ? *(const f32x4*)(p + k) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            z[c * 4 + e] = v[e];
            mx = fmaxf(mx, v[e]);                       // (a NaN is skipped here and caught by the sum)
        }
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) s = __fadd_rn(s, expf(z[e] - mx));
    s = wave_sum(s);
    if (lane == 0) {
        const long ti = gi * tok_stride + gr + tok_off;
        long tg = tokens[ti];
        if (tg < 0 || tg >= K) {                        // reported by mage_check_device_errors, as mage_cross_entropy's targets are
            mage_raise(err, MAGE_DEVERR_TOKEN_ID, tg, K);
            tg = tg < 0 ? 0 : K - 1;
        }
        logprob[ti] = p[tg] - (mx + logf(s));
    }
}

// ---- per-token statistics of the sampling policy (mage_token_stats, include/mage_hip_ext.h): what mage_sample_tokens' filter kept and how
// the kept set weighs the given token.  Per row, with s, A, N of steps 1-3 of the sampling rule above (sample_filter: the sampler's own code,
// so N is the sampler's bit for bit), s_max = max_N s, w_j = exp(s_j - s_max), Z = sum_{j in N} w_j:
//   kept           = |N|                                                (a ballot count: exact)
//   policy_logprob = s_t - (s_max + log Z) for t in N, -inf otherwise   (s_t = z_t * inv_t, the sampler's multiply)
//   policy_entropy = log Z - (sum_{j in N} w_j (s_j - s_max)) / Z       (nats; exactly 0 when |N| = 1)
//   entropy        = the same formula over the whole row of z itself: temperature 1, no filter -- the distribution mage_token_logprob scores under
// top_k == 1 is greedy by definition, as in the sampler: N = { mage_argmax's first maximum of z }, kept = 1, policy_logprob = 0 for that code
// and -inf for any other, policy_entropy = 0.
// Special values: a NaN logit is in no set and adds nothing to Z (it makes `entropy` NaN, as it does mage_token_logprob's result); a -inf
// logit in N counts in `kept` and adds a zero term to both sums (never 0 * inf); a row with no selectable code (every logit NaN) gives
// kept = 0 and NaN for policy_logprob and policy_entropy; s_max = +-inf (a +inf logit, a row of -inf only) gives NaN through
// inf - inf, as in mage_token_logprob; a token outside [0, K) is raised (MAGE_DEVERR_TOKEN_ID) and clamped.
// One wave per row, the row read once into registers in sample_kernel's layout whatever outputs are asked for (a null output costs a
// wave-uniform branch), one instance per filter combination.  Every sum has a fixed order: a lane adds its own terms in register order (adding
// 0 for a code outside N), the lanes meet in an xor butterfly; expf / logf are the accurate ones.  With temperature 1 and no filter, s = z,
// s_max = the row maximum and Z is token_logprob_kernel's sum operation for operation: policy_logprob equals mage_token_logprob's result bit
// for bit on NaN-free rows.
enum { STATS_TOPK = 1, STATS_TOPP = 2, STATS_GREEDY = 4 };
template <int NV, int MODE>
__global__ __launch_bounds__(256) void token_stats_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group, long in_stride,
                                                          long in_off, const int64_t* __restrict__ tokens, long tok_stride, long tok_off,
                                                          float inv_t, int top_k, float top_p, float* __restrict__ policy_logprob,
                                                          float* __restrict__ policy_entropy, int32_t* __restrict__ kept,
                                                          float* __restrict__ entropy, int* __restrict__ err) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const long gi = i / group, gr = i - gi * group;
    const float* p = logits + (gi * in_stride + gr + in_off) * ld;
    const long ti = gi * tok_stride + gr + tok_off;
    f32x4 zc[NV / 4];
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) zc[c] = sample_row_chunk(p, lane, K, c);
    if (entropy) {                                      // the whole row at temperature 1: token_logprob_kernel's maximum and sum
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < NV; ++e)
            if ((e >> 2) * 256 + lane * 4 < K) mx = fmaxf(mx, zc[e >> 2][e & 3]);          // (a NaN is skipped here and caught by the sum)
        mx = wave_max(mx);
        float zs = 0.f, ts = 0.f;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const float d = zc[e >> 2][e & 3] - mx;
            const float w = (e >> 2) * 256 + lane * 4 < K ? expf(d) : 0.f;
            zs = __fadd_rn(zs, w);
            ts = w == 0.f ? ts : __fmaf_rn(w, d, ts);   // exp(-inf) = 0 adds nothing: not 0 * inf
        }
        zs = wave_sum(zs);
        ts = wave_sum(ts);
        if (lane == 0) entropy[ti] = logf(zs) - ts / zs;
    }
    if (!policy_logprob && !policy_entropy && !kept) return;
    float s[NV];
    unsigned key[NV];
    const unsigned lo = sample_filter<NV, (MODE & STATS_TOPK) != 0, (MODE & STATS_TOPP) != 0>([&](int c) { return zc[c]; }, lane, K, inv_t, top_k,
                                                                                              top_p, s, key);
    unsigned km = 0u;
#pragma unroll
    for (int e = 0; e < NV; ++e) km = max(km, key[e]);
    km = wave_max_u32(km);                              // km >= lo unless nothing is selectable (then every key is 0)
    if constexpr (MODE == STATS_GREEDY) {               // (inv_t = 1 here: s = z) N = the first maximum, NaNs skipped: argmax_kernel's pick
        int bj = 0x7fffffff;
#pragma unroll
        for (int e = NV - 1; e >= 0; --e)
            if (key[e] == km) bj = (e >> 2) * 256 + lane * 4 + (e & 3);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bj = min(bj, __shfl_xor(bj, o, 64));
        if (lane == 0) {
            const bool any = km != 0u;
            if (kept) kept[ti] = any ? 1 : 0;
            if (policy_entropy) policy_entropy[ti] = any ? 0.f : __builtin_nanf("");
            if (policy_logprob) {
                long tg = tokens[ti];
                if (tg < 0 || tg >= K) {
                    mage_raise(err, MAGE_DEVERR_TOKEN_ID, tg, K);
                    tg = tg < 0 ? 0 : K - 1;
                }
                policy_logprob[ti] = !any ? __builtin_nanf("") : tg == bj ? 0.f : -INFINITY;
            }
        }
    } else {
        int n = 0;
#pragma unroll
        for (int e = 0; e < NV; ++e) n += __popcll(__ballot(key[e] >= lo));
        float zs = 0.f, ts = 0.f;
        const float smax = sample_key_value(km);
        if (policy_logprob || policy_entropy) {
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const float d = s[e] - smax;
                const float w = key[e] >= lo ? expf(d) : 0.f;
                zs = __fadd_rn(zs, w);
                ts = w == 0.f ? ts : __fmaf_rn(w, d, ts);
            }
            zs = wave_sum(zs);
            if (policy_entropy) ts = wave_sum(ts);
        }
        if (lane == 0) {
            if (kept) kept[ti] = n;
            const float lz = logf(zs);
            if (policy_entropy) policy_entropy[ti] = n ? lz - ts / zs : __builtin_nanf("");
            if (policy_logprob) {
                long tg = tokens[ti];
                if (tg < 0 || tg >= K) {
                    mage_raise(err, MAGE_DEVERR_TOKEN_ID, tg, K);
                    tg = tg < 0 ? 0 : K - 1;
                }
                const float st = __fmul_rn(p[tg], inv_t);
                policy_logprob[ti] = !n ? __builtin_nanf("") : sample_key(st) >= lo ? st - (smax + lz) : -INFINITY;
            }
        }
    }
}

// ---- policy-gradient loss over given tokens (mage_policy_loss / mage_policy_loss_bwd, include/mage_hip_ext.h states the rule).  The policy
// is the sampler's: s, N of steps 1-3 of the sampling rule above by sample_filter itself, logprob and entropy by token_stats_kernel's
// operations in token_stats_kernel's order, so on the same inputs they carry mage_token_stats' bits.  One wave per row, the row read once
// into registers in sample_kernel's layout, one instance per filter combination; the forward kernel leaves the filter's threshold in cut[i]
// and the backward kernel keeps j iff sample_key(s_j) >= cut[i]: no second bisection, and the same set bit for bit.

// w_j = exp(s_j - smax) over the kept set (0 outside it), Z = sum w_j and sum w_j (s_j - smax): token_stats_kernel's sums, term for term
template <int NV>
__device__ __forceinline__ void policy_sums(const float (&s)[NV], const unsigned (&key)[NV], unsigned lo, float smax, float (&w)[NV], float& zs,
                                            float& ts) {
    zs = 0.f;
    ts = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const float d = s[e] - smax;
        w[e] = key[e] >= lo ? expf(d) : 0.f;
        zs = __fadd_rn(zs, w[e]);
        ts = w[e] == 0.f ? ts : __fmaf_rn(w[e], d, ts);
    }
    zs = wave_sum(zs);
    ts = wave_sum(ts);
}

// One row's loss term and the factor g of its gradient from logprob lp, entropy H, advantage A and (clipped form) the behaviour
// log-probability b.  rho = expf(lp - b) is the one fp32 value both passes use to decide which branch of the surrogate is active; the
// products and the final sum are taken in fp64 and rounded once.  An outside row (lp = -inf: a token the filter cannot draw) gives 0, 0.
struct PolicyTerm { float loss, g; bool outside, off; double sum; };   // sum: the loss before its one rounding (the anchored form adds to it)
__device__ __forceinline__ PolicyTerm policy_term(float lp, float H, float A, bool clipped, float b, float cmin, float cmax, float ent_coef) {
    PolicyTerm t{0.f, 0.f, lp == -INFINITY, false, 0.0};
    if (t.outside) return t;
    double surr;
    if (!clipped) {
        surr = (double)A * (double)lp;
        t.g = -A;
    } else {
        const float rho = expf(lp - b);
        const bool active = (A >= 0.f && rho <= cmax) || (A < 0.f && rho >= cmin);
        const double u = (double)rho * (double)A, c = (double)fminf(fmaxf(rho, cmin), cmax) * (double)A;
        surr = u < c ? u : (c < u ? c : (u != u ? u : c));              // min; a NaN stays a NaN
        t.g = active ? -(A * rho) : 0.f;
        t.off = !active;
    }
    t.sum = -surr - (double)ent_coef * (double)H;
    t.loss = (float)t.sum;
    return t;
}

// The anchor of mage_policy_loss_anchored: d = r - lp (one fp32 subtraction) against the reference log-probability r, in fp64
//   kl = exp(d) - d - 1 (the k3 estimator, >= 0)   and   gfac = 1 - exp(d) = d kl / d lp.
// gfac = -expm1(d) has no cancellation anywhere.  kl = expm1(d) - d for |d| >= 2^-8: the subtraction cancels at most the leading
// 2 / |d| <= 2^9 of the operands, a relative error below 2^-42; below 2^-8 the series d^2 (1/2 + d (1/6 + d (1/24 + d (1/120 + d / 720))))
// whose first dropped term d^7 / 5040 is below 2^-51 of the sum.  Both are far inside one fp32 ulp (2^-24), and d = 0 gives 0, 0 exactly.
// An outside row (lp = -inf) and a row whose r is not finite (an unanchored row) have no anchor: kl = 0, no gradient.
struct PolicyAnchor { double kl, gfac; bool on; };
__device__ __forceinline__ PolicyAnchor policy_anchor(float lp, float r) {
    PolicyAnchor a{0.0, 0.0, false};
    if (lp == -INFINITY || !__builtin_isfinite(r)) return a;
    a.on = true;
    const double d = (double)(r - lp), em = expm1(d);
    a.gfac = -em;
    a.kl = fabs(d) < 0x1p-8 ? d * d * (1.0 / 2 + d * (1.0 / 6 + d * (1.0 / 24 + d * (1.0 / 120 + d * (1.0 / 720))))) : em - d;
    return a;
}

// policy_term plus kl_coef times the anchor: the loss from the fp64 sum, g from g's fp32 value and the fp64 factor, one rounding each.  A
// zero term is not added at all (kl_coef = 0, d = 0, no anchor), so such a row carries policy_term's bits -- also its -0 and its NaN.
__device__ __forceinline__ PolicyTerm policy_term_anchored(PolicyTerm t, const PolicyAnchor& a, float kl_coef) {
    if (!a.on || kl_coef == 0.f) return t;
    if (a.kl != 0.0) t.loss = (float)(t.sum + (double)kl_coef * a.kl);
    if (a.gfac != 0.0) t.g = (float)((double)t.g + (double)kl_coef * a.gfac);
    return t;
}

__device__ __forceinline__ long policy_token(const int64_t* __restrict__ tokens, long i, int K, int* err) {
    long tg = tokens[i];
    if (tg < 0 || tg >= K) {
        if (err) mage_raise(err, MAGE_DEVERR_TOKEN_ID, tg, K);          // (the backward pass clamps alike and leaves the report to the forward one)
        tg = tg < 0 ? 0 : K - 1;
    }
    return tg;
}

// mage_policy_loss_masked's per-row byte, one scalar value per wave (the row index is the wave's); a null mask (the unmasked entry points) has
// no given row
__device__ __forceinline__ bool policy_row_given(const uint8_t* __restrict__ given, long i) {
    return given && __builtin_amdgcn_readfirstlane((int)given[i]) != 0;
}

template <int NV, bool TOPK, bool TOPP, bool ANCH>
__global__ __launch_bounds__(256) void policy_loss_kernel(const float* __restrict__ logits, long rows, int K, long ld,
                                                          const int64_t* __restrict__ tokens, const float* __restrict__ adv, long adv_div,
                                                          const float* __restrict__ blp, float inv_t, int top_k, float top_p, float cmin,
                                                          float cmax, float ent_coef, float* __restrict__ row_loss,
                                                          float* __restrict__ logprob, float* __restrict__ entropy,
                                                          unsigned* __restrict__ cut, int* __restrict__ err,
                                                          const float* __restrict__ ref, float kl_coef, float* __restrict__ kl,
                                                          const uint8_t* __restrict__ given) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    if (policy_row_given(given, i)) {                   // (wave-uniform) mage_policy_loss_masked: nothing of the row is read
        if (lane == 0) {
            cut[i] = 0u;
            logprob[i] = 0.f;
            entropy[i] = 0.f;
            row_loss[i] = 0.f;
            if (kl) kl[i] = 0.f;
        }
        return;
    }
    const float* p = logits + i * ld;
    float s[NV], w[NV];
    unsigned key[NV];
    const unsigned lo = sample_filter<NV, TOPK, TOPP>([=](int c) { return sample_row_chunk(p, lane, K, c); }, lane, K, inv_t, top_k, top_p, s,
                                                      key);
    unsigned km = 0u;
#pragma unroll
    for (int e = 0; e < NV; ++e) km = max(km, key[e]);
    km = wave_max_u32(km);                              // km >= lo unless nothing is selectable (then every key is 0)
    int n = 0;
#pragma unroll
    for (int e = 0; e < NV; ++e) n += __popcll(__ballot(key[e] >= lo));
    const float smax = sample_key_value(km);
    float zs, ts;
    policy_sums<NV>(s, key, lo, smax, w, zs, ts);
    if (lane == 0) {
        const float lz = logf(zs);
        const float H = n ? lz - ts / zs : __builtin_nanf("");
        const long tg = policy_token(tokens, i, K, err);
        const float st = __fmul_rn(p[tg], inv_t);
        const float lp = !n ? __builtin_nanf("") : sample_key(st) >= lo ? st - (smax + lz) : -INFINITY;
        cut[i] = lo;
        logprob[i] = lp;
        entropy[i] = H;
        const PolicyTerm t = policy_term(lp, H, adv[i / adv_div], blp != nullptr, blp ? blp[i] : 0.f, cmin, cmax, ent_coef);
        if constexpr (ANCH) {
            const PolicyAnchor a = policy_anchor(lp, ref[i]);
            kl[i] = (float)a.kl;
            row_loss[i] = policy_term_anchored(t, a, kl_coef).loss;
        } else {
            row_loss[i] = t.loss;
        }
    }
}

// summary, stage 1 of 2: workgroup b owns rows [b * chunk, (b + 1) * chunk) and leaves W fp64 sums in part[b * W ..]: the loss terms, the
// entropies, b - logprob, the rows whose gradient the clip switched off, the outside rows (an outside row counts in the last one only) and,
// for the anchored call (W = 7), the KL estimates and the unanchored rows (a reference log-probability that is not finite).
// A thread adds its rows in ascending order, the lanes meet in an xor butterfly, thread 0 adds the four waves in order: a fixed order.
// The masked call (W = 8) adds the free rows only, in the same order, and counts the given ones in an eighth sum; its kl and ref may be null
// (the plain rule: sums 5 and 6 stay 0).
enum { POLICY_PARTS = 256, POLICY_MEANS = 7, POLICY_MASKED = 8 };
__device__ double g_policy_part[POLICY_PARTS * POLICY_MASKED];     // stage 1 -> stage 2, within one mage_policy_loss* call (stream order)
template <int W>
__global__ __launch_bounds__(256) void policy_part_kernel(const float* __restrict__ row_loss, const float* __restrict__ logprob,
                                                          const float* __restrict__ entropy, const float* __restrict__ adv, long adv_div,
                                                          const float* __restrict__ blp, float cmin, float cmax, long rows, long chunk,
                                                          const float* __restrict__ kl, const float* __restrict__ ref,
                                                          const uint8_t* __restrict__ given) {
    __shared__ double red[4][W];
    const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    double a[W] = {};
    for (long i = r0 + threadIdx.x; i < r1; i += 256) {
        if constexpr (W == POLICY_MASKED) {
            if (given[i]) {
                a[7] += 1.0;
                continue;
            }
        }
        const float lp = logprob[i];
        if (lp == -INFINITY) {
            a[4] += 1.0;
            continue;
        }
        a[0] += (double)row_loss[i];
        a[1] += (double)entropy[i];
        if (blp) {
            const float b = blp[i];
            a[2] += (double)b - (double)lp;
            a[3] += policy_term(lp, 0.f, adv[i / adv_div], true, b, cmin, cmax, 0.f).off ? 1.0 : 0.0;
        }
        if constexpr (W >= POLICY_MEANS) {
            if (W == POLICY_MEANS || ref) {
                a[5] += (double)kl[i];
                a[6] += __builtin_isfinite(ref[i]) ? 0.0 : 1.0;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < W; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_xor(a[q], o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = a[q];
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int q = threadIdx.x;
        g_policy_part[blockIdx.x * W + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// stage 2: thread t holds workgroup t's sums; the same butterfly and wave order, one multiply by 1 / rows, one rounding to fp32
template <int W>
__global__ __launch_bounds__(256) void policy_summary_kernel(float* __restrict__ summary, double inv) {
    __shared__ double red[4][W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
        double v = g_policy_part[threadIdx.x * W + q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int q = threadIdx.x;
        summary[q] = (float)((((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]) * inv);
    }
}

// stage 2 of the masked call: the same sums; the eighth one is the number of given rows (exact in fp64), so n_free = rows - given.  The seven
// means are multiplied by 1 / n_free (the unmasked call's 1.0 / rows when nothing is given; 0 when everything is), summary[7] is the given
// share, and norm[0] = 1.0f / (float)n_free is left for the backward call: the value the unmasked one forms on the host for its `rows`.
__global__ __launch_bounds__(256) void policy_summary_masked_kernel(float* __restrict__ summary, float* __restrict__ norm, long rows) {
    constexpr int W = POLICY_MASKED;
    __shared__ double red[4][W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
        double v = g_policy_part[threadIdx.x * W + q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int q = threadIdx.x;
        const double ng = ((red[0][7] + red[1][7]) + red[2][7]) + red[3][7];
        const long n_free = rows - (long)ng;
        if (q < POLICY_MEANS) {
            const double inv = n_free > 0 ? 1.0 / (double)n_free : 0.0;
            summary[q] = (float)((((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]) * inv);
        } else {
            summary[7] = (float)(ng / (double)rows);
            norm[0] = n_free > 0 ? __fdiv_rn(1.0f, (float)n_free) : 0.f;
        }
    }
}

// dlogits_ij = scale * [ g_i (1[j = t] - p_j) + ent_coef p_j (log p_j + H_i) ] for j in N, 0 outside N and in outside rows; scale =
// grad_out[0] / rows * inv_t, p_j = w_j / Z, log p_j + H_i = (s_j - smax) - (sum_N w (s - smax)) / Z; a p_j = 0 term is 0.  Z, H, logprob are
// recomputed with the forward kernel's operations (policy_sums), so g_i is decided by the forward pass's rho.
template <int NV, typename OT, bool ANCH>
__global__ __launch_bounds__(256) void policy_loss_bwd_kernel(const float* __restrict__ logits, long rows, int K, long ld,
                                                              const int64_t* __restrict__ tokens, const float* __restrict__ adv, long adv_div,
                                                              const float* __restrict__ blp, const unsigned* __restrict__ cut, float inv_t,
                                                              float cmin, float cmax, float ent_coef, const float* __restrict__ gout,
                                                              float inv_rows, OT* __restrict__ dl, const float* __restrict__ ref,
                                                              float kl_coef, const uint8_t* __restrict__ given,
                                                              const float* __restrict__ norm) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + i * ld;
    OT* o = dl + i * (long)K;
    if (policy_row_given(given, i)) {                                   // (wave-uniform) a zero row by the free rows' stores, nothing read
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
            const int k = c * 256 + lane * 4;
            if (k < K) store4(o + k, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    if (norm) inv_rows = norm[0];                                       // the masked call: 1 / n_free, left by its forward call
    const unsigned lo = cut[i];
    float s[NV], w[NV];
    unsigned key[NV];
    unsigned km = 0u;
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const int k = c * 256 + lane * 4;
        const f32x4 v = sample_row_chunk(p, lane, K, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s[c * 4 + e] = __fmul_rn(v[e], inv_t);                      // sample_filter's s and key
            key[c * 4 + e] = k < K ? sample_key(s[c * 4 + e]) : 0u;
            km = max(km, key[c * 4 + e]);
        }
    }
    km = wave_max_u32(km);
    const float smax = sample_key_value(km);
    float zs, ts;
    policy_sums<NV>(s, key, lo, smax, w, zs, ts);
    const long tg = policy_token(tokens, i, K, nullptr);
    const float st = __fmul_rn(p[tg], inv_t);
    const bool out_n = sample_key(st) < lo;                             // t outside N (or no selectable code at all: st is NaN, key 0)
    const float lz = logf(zs);
    const float H = lz - ts / zs;
    const float lp = st - (smax + lz);
    PolicyTerm t = policy_term(lp, H, adv[i / adv_div], blp != nullptr, blp ? blp[i] : 0.f, cmin, cmax, ent_coef);
    if constexpr (ANCH) {
        // (lp is only the forward pass's logprob where the token is in N: any other row is zeroed below whatever g is)
        if (!out_n) t = policy_term_anchored(t, policy_anchor(lp, ref[i]), kl_coef);
    }
    // 1 - p_t = (Z - w_t) / Z from the sum of the OTHER kept terms (same fixed order): no cancellation where the token holds nearly all the mass
    float zo = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) zo = __fadd_rn(zo, (e >> 2) * 256 + lane * 4 + (e & 3) == tg ? 0.f : w[e]);
    zo = wave_sum(zo);
    const float scale = gout[0] * inv_rows * inv_t, inv_z = 1.0f / zs;
    const float hx = ts / zs;                                           // log p_j + H = (s_j - smax) - hx: log Z drops out
    const bool zero = out_n || t.outside;                               // an outside row (t.outside: a kept token of logit -inf)
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const int k = c * 256 + lane * 4;
        if (k >= K) break;
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = c * 4 + e;
            const float pj = w[j] * inv_z;
            float v = t.g * (k + e == tg ? zo * inv_z : -pj);
            if (ent_coef != 0.f && pj != 0.f) v += ent_coef * pj * ((s[j] - smax) - hx);
            d[e] = (zero || key[j] < lo) ? 0.f : v * scale;
        }
        store4(o + k, d);
    }
}

// One workgroup per clip: wave w sums candidates w, w + 4, ... (a lane adds values lane, lane + 64, ... in fp64, the lanes meet in an xor
// butterfly, one rounding to fp32), then thread 0 picks the largest score: first on ties, a NaN only if every score is NaN.
__global__ __launch_bounds__(256) void clip_scores_kernel(const float* __restrict__ logprob, int n_cand, long per_clip,
                                                          float* __restrict__ scores, int64_t* __restrict__ best) {
    const long clip = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = wave; c < n_cand; c += 4) {
        const float* v = logprob + (clip * n_cand + c) * per_clip;
        double s = 0.0;
        for (long j = lane; j < per_clip; j += 64) s += (double)v[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) scores[clip * n_cand + c] = (float)s;
    }
    if (!best) return;
    __syncthreads();                                    // (workgroup-uniform: `best` is a kernel argument)
    if (threadIdx.x == 0) {
        int bi = 0;
        float bs = scores[clip * n_cand];
        for (int c = 1; c < n_cand; ++c) {
            const float sc = scores[clip * n_cand + c];
            if (sc > bs || (bs != bs && sc == sc)) { bs = sc; bi = c; }
        }
        best[clip] = bi;
    }
}

}  // namespace

extern "C" int mage_vq_prepare(const float* codebook, int32_t K, int32_t D, float* codebook_t, float* c2, void* stream) {
    MAGE_CHECK_ARG(codebook && codebook_t && c2 && K > 0 && D > 0, "mage_vq_prepare: bad arguments");
    hipLaunchKernelGGL(vq_prepare_kernel, dim3((K + 255) / 256), dim3(256), 0, (hipStream_t)stream, codebook, K, D,
                       codebook_t, c2);
    MAGE_CHECK_LAUNCH("mage_vq_prepare");
    return MAGE_OK;
}

extern "C" int mage_vq_nearest(const float* z, const float* codebook_t, const float* c2, int64_t M, int32_t D, int32_t K,
                               int64_t* idx, float* margin, void* stream) {
    MAGE_CHECK_ARG(z && codebook_t && c2 && idx, "mage_vq_nearest: null pointer");
    MAGE_CHECK_ARG(M > 0 && D > 0 && D % 4 == 0 && K > 0 && K <= 1024, "mage_vq_nearest: M=%ld D=%d K=%d unsupported", (long)M, D, K);
    hipStream_t s = (hipStream_t)stream;
    if (!mage_options().vq_no_mfma) {                                       // the fp64 matrix-core kernel: any D % 4 == 0, K <= 1024
        const dim3 g32((unsigned)((M + 31) / 32));        // 4 tiles of 16 codes per wave: 92 + 64 registers, 3 waves per SIMD
        if (K <= 256) hipLaunchKernelGGL((vq_nearest_mfma_kernel<4, 2, 4>), g32, dim3(256), 0, s, z, codebook_t, c2, (long)M, D, K, idx, margin);
        else if (K <= 512) hipLaunchKernelGGL((vq_nearest_mfma_kernel<4, 2, 8>), g32, dim3(512), 0, s, z, codebook_t, c2, (long)M, D, K, idx, margin);
        else hipLaunchKernelGGL((vq_nearest_mfma_kernel<8, 2, 8>), g32, dim3(512), 0, s, z, codebook_t, c2, (long)M, D, K, idx, margin);
        MAGE_CHECK_LAUNCH("mage_vq_nearest");
        return MAGE_OK;
    }
    const size_t lds = (size_t)(16 * D + 16 + 16 * K) * 4;
    MAGE_CHECK_ARG(lds <= 144 * 1024, "mage_vq_nearest: D=%d K=%d exceed the LDS budget", D, K);
    static bool attr_set[MAGE_MAX_DEVICES] = {false};      // the attribute is per device (idempotent: a racing second call is harmless)
    const int dev = mage_device_index();
    MAGE_CHECK_ARG(dev >= 0, "mage_vq_nearest: no current device");
    if (!attr_set[dev]) {
        (void)hipFuncSetAttribute((const void*)vq_nearest_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        (void)hipFuncSetAttribute((const void*)vq_nearest_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        (void)hipFuncSetAttribute((const void*)vq_nearest_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        attr_set[dev] = true;
    }
    const dim3 grid((unsigned)((M + 15) / 16)), blk(256);
    if (K <= 256) hipLaunchKernelGGL((vq_nearest_kernel<1>), grid, blk, lds, s, z, codebook_t, c2, (long)M, D, K, idx, margin);
    else if (K <= 512) hipLaunchKernelGGL((vq_nearest_kernel<2>), grid, blk, lds, s, z, codebook_t, c2, (long)M, D, K, idx, margin);
    else hipLaunchKernelGGL((vq_nearest_kernel<4>), grid, blk, lds, s, z, codebook_t, c2, (long)M, D, K, idx, margin);
    MAGE_CHECK_LAUNCH("mage_vq_nearest");
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------ convolution of an embedding as a table sum
// A k x k convolution (stride 1, zero padding (k-1)/2) over nn.Embedding rows has only n_codes distinct input vectors, so it is
//     y[img, p, :] = pos[p, :] + sum over taps (ky, kx) of T[tap][ids[img, p + (ky, kx) - centre], :]      (taps outside the image: nothing)
// with T[tap][code] = W_tap emb[code] precomputed once per weights (and any Linear applied to the result folded into T and pos).
// One wave per output pixel: taps_h*taps_w rows of C floats gathered from a table that lives in L2 / Infinity Cache (9 x 512 x 512
// fp32 = 9.4 MB at the MNIST config), summed in a fixed order in fp32, + a broadcast row table (the T positions), written to row
// yrow = (m / group) * y_group_stride + m % group + y_off of y (m = img*H*W + p): the frame slots of the decoder's residual stream.
namespace {
template <typename TT_, typename OT, int VPL>
__global__ __launch_bounds__(256) void table_conv_kernel(const int64_t* __restrict__ ids, const TT_* __restrict__ table, const float* __restrict__ pos,
                                                         const float* __restrict__ bias, int relu,
                                                         const float* __restrict__ rowadd, OT* __restrict__ y, long n_pix, int H, int W,
                                                         int th, int tw, int n_codes, int C, long group, long y_group_stride, long y_off,
                                                         long rowadd_div, int rowadd_mod, long ldy, int* __restrict__ err) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n_pix) return;
    const int lane = threadIdx.x & 63;
    const int plane = H * W;
    const long img = m / plane;
    const int p = (int)(m - img * plane);
    const int py = p / W, px = p - py * W;
    f32x4 acc[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        acc[j] = (pos && c < C) ? *(const f32x4*)(pos + (long)p * C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (bias && c < C) acc[j] += *(const f32x4*)(bias + c);
    }
    const int64_t* img_ids = ids + img * plane;
    for (int ky = 0; ky < th; ++ky) {
        const int iy = py + ky - (th >> 1);
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < tw; ++kx) {
            const int ix = px + kx - (tw >> 1);
            if ((unsigned)ix >= (unsigned)W) continue;
            long id = img_ids[iy * W + ix];
            if (id < 0 || id >= n_codes) {      // the reference's nn.Embedding raises IndexError: reported by mage_check_device_errors
                if (lane == 0) mage_raise(err, MAGE_DEVERR_EMBEDDING_ID, id, n_codes);
                id = id < 0 ? 0 : n_codes - 1;
            }
            MAGE_DASSERT(id >= 0 && id < n_codes);
            const TT_* row = table + ((long)(ky * tw + kx) * n_codes + id) * C;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int c = j * 256 + lane * 4;
                if (c < C) acc[j] += load4(row + c);
            }
        }
    }
    const long yrow = (m / group) * y_group_stride + m % group + y_off;
    if (rowadd) {
        const float* rp = rowadd + ((yrow / rowadd_div) % rowadd_mod) * (long)C;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * 256 + lane * 4;
            if (c < C) acc[j] += *(const f32x4*)(rp + c);
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        if (c < C) {
            if (relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = fmaxf(acc[j][e], 0.f);
            }
            store4(y + yrow * ldy + c, acc[j]);
        }
    }
}
// The same sums for 16-bit tables and rows of exactly 512 channels (the decoder's frame fill: 245 760 pixels per call at cfg2): a lane owns 8
// channels, so a table row is ONE 16-byte load per lane (the kernel above takes two 8-byte loads per row: twice the load instructions at
// 0.54-0.70x the bytes per instruction).  Same order of additions per element: pos (+ bias), the taps in (ky, kx) order, the row table.
template <typename T16>
__global__ __launch_bounds__(256) void table_conv512_kernel(const int64_t* __restrict__ ids, const T16* __restrict__ table, const float* __restrict__ pos,
                                                            const float* __restrict__ bias, int relu, const float* __restrict__ rowadd,
                                                            T16* __restrict__ y, long n_pix, int H, int W, int th, int tw, int n_codes, long group,
                                                            long y_group_stride, long y_off, long rowadd_div, int rowadd_mod, long ldy,
                                                            int* __restrict__ err) {
    constexpr int C = 512;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n_pix) return;
    const int lane = threadIdx.x & 63, c = lane * 8;
    const int plane = H * W;
    const long img = m / plane;
    const int p = (int)(m - img * plane);
    const int py = p / W, px = p - py * W;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    if (pos) {
        a0 = *(const f32x4*)(pos + (long)p * C + c);
        a1 = *(const f32x4*)(pos + (long)p * C + c + 4);
    }
    if (bias) {
        a0 += *(const f32x4*)(bias + c);
        a1 += *(const f32x4*)(bias + c + 4);
    }
    const int64_t* img_ids = ids + img * plane;
    for (int ky = 0; ky < th; ++ky) {
        const int iy = py + ky - (th >> 1);
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < tw; ++kx) {
            const int ix = px + kx - (tw >> 1);
            if ((unsigned)ix >= (unsigned)W) continue;
            long id = img_ids[iy * W + ix];
            if (id < 0 || id >= n_codes) {
                if (lane == 0) mage_raise(err, MAGE_DEVERR_EMBEDDING_ID, id, n_codes);
                id = id < 0 ? 0 : n_codes - 1;
            }
            const u32x4 r = *(const u32x4*)(table + ((long)(ky * tw + kx) * n_codes + id) * C + c);
            a0 += widen4<T16>(uint2{r[0], r[1]});
            a1 += widen4<T16>(uint2{r[2], r[3]});
        }
    }
    const long yrow = (m / group) * y_group_stride + m % group + y_off;
    if (rowadd) {
        const float* rp = rowadd + ((yrow / rowadd_div) % rowadd_mod) * (long)C;
        a0 += *(const f32x4*)(rp + c);
        a1 += *(const f32x4*)(rp + c + 4);
    }
    if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a0[e] = fmaxf(a0[e], 0.f);
            a1[e] = fmaxf(a1[e], 0.f);
        }
    }
    store8(y + yrow * ldy + c, a0, a1);
}
}  // namespace

extern "C" int mage_table_conv(const int64_t* ids, int64_t n_img, int32_t H, int32_t W, int32_t taps_h, int32_t taps_w, const void* table,
                               int32_t table_dtype, int32_t n_codes, int32_t C, const float* pos, const float* bias, int32_t relu,
                               const float* rowadd, int64_t rowadd_div, int32_t rowadd_mod, void* y, int32_t y_dtype, int64_t ldy, int64_t group,
                               int64_t y_group_stride, int64_t y_off, void* stream) {
    MAGE_CHECK_ARG(ids && table && y, "mage_table_conv: null pointer");
    MAGE_CHECK_ARG(n_img > 0 && H > 0 && W > 0 && taps_h >= 1 && taps_w >= 1 && (taps_h & 1) && (taps_w & 1) && n_codes > 0 && C > 0 && C % 4 == 0 &&
                       C <= 2048 && ldy >= C && ldy % 4 == 0 && group > 0,
                   "mage_table_conv: bad sizes (odd taps, C %% 4 == 0, C <= 2048)");
    MAGE_CHECK_ARG(!rowadd || (rowadd_div >= 1 && rowadd_mod >= 1), "mage_table_conv: bad rowadd div/mod");
    const bool ysplit = y_dtype == MAGE_BF16X3 || y_dtype == MAGE_F16X3;
    MAGE_CHECK_ARG((table_dtype == MAGE_F32 || table_dtype == MAGE_BF16 || table_dtype == MAGE_F16) &&
                       (y_dtype == MAGE_F32 || y_dtype == MAGE_BF16 || y_dtype == MAGE_F16 || ysplit) &&
                       (table_dtype == MAGE_F32 || y_dtype == MAGE_F32 || table_dtype == y_dtype),
                   "mage_table_conv: bad table / y dtype %d %d (fp32, bf16 or f16; a 16-bit table writes fp32 or its own type)", table_dtype, y_dtype);
    MAGE_CHECK_ARG(!ysplit || (C % 64 == 0 && ldy == C && (((uintptr_t)y) & 255) == 0 && table_dtype == MAGE_F32),
                   "mage_table_conv: split output needs an fp32 table, C %% 64 == 0, packed rows, y 256-byte aligned");
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_table_conv: mage_init() has not been called");
    const long n_pix = (long)n_img * H * W;
    const dim3 grid((unsigned)((n_pix + 3) / 4)), blk(256);
    hipStream_t s = (hipStream_t)stream;
#define TC(T_, O_, V) hipLaunchKernelGGL((table_conv_kernel<T_, O_, V>), grid, blk, 0, s, ids, (const T_*)table, pos, bias, relu, rowadd, (O_*)y, n_pix, H, W, \
                                         taps_h, taps_w, n_codes, C, (long)group, (long)y_group_stride, (long)y_off, (long)rowadd_div, rowadd_mod, (long)ldy, err)
#define TCV(T_, O_) do { if (vpl <= 1) TC(T_, O_, 1); else if (vpl <= 2) TC(T_, O_, 2); else if (vpl <= 4) TC(T_, O_, 4); else TC(T_, O_, 8); } while (0)
    const int vpl = (C + 255) / 256;
    if (C == 512 && table_dtype == y_dtype && (y_dtype == MAGE_BF16 || y_dtype == MAGE_F16) && ldy % 8 == 0 &&
        (((uintptr_t)table | (uintptr_t)y | (uintptr_t)pos | (uintptr_t)bias | (uintptr_t)rowadd) & 15) == 0) {
        if (y_dtype == MAGE_BF16)
            hipLaunchKernelGGL((table_conv512_kernel<unsigned short>), grid, blk, 0, s, ids, (const unsigned short*)table, pos, bias, relu, rowadd,
                               (unsigned short*)y, n_pix, H, W, taps_h, taps_w, n_codes, (long)group, (long)y_group_stride, (long)y_off, (long)rowadd_div,
                               rowadd_mod, (long)ldy, err);
        else
            hipLaunchKernelGGL((table_conv512_kernel<f16_t>), grid, blk, 0, s, ids, (const f16_t*)table, pos, bias, relu, rowadd, (f16_t*)y, n_pix, H, W,
                               taps_h, taps_w, n_codes, (long)group, (long)y_group_stride, (long)y_off, (long)rowadd_div, rowadd_mod, (long)ldy, err);
        MAGE_CHECK_LAUNCH("mage_table_conv");
        return MAGE_OK;
    }
    if (y_dtype == MAGE_F16X3) TCV(float, split_f16);
    else if (y_dtype == MAGE_BF16X3) TCV(float, split_bf16);
    else if (table_dtype == MAGE_F32 && y_dtype == MAGE_F32) TCV(float, float);
    else if (table_dtype == MAGE_F32 && y_dtype == MAGE_F16) TCV(float, f16_t);
    else if (table_dtype == MAGE_F16 && y_dtype == MAGE_F32) TCV(f16_t, float);
    else if (table_dtype == MAGE_F16) TCV(f16_t, f16_t);
    else if (table_dtype == MAGE_F32) TCV(float, unsigned short);
    else if (y_dtype == MAGE_F32) TCV(unsigned short, float);
    else TCV(unsigned short, unsigned short);
#undef TCV
#undef TC
    MAGE_CHECK_LAUNCH("mage_table_conv");
    return MAGE_OK;
}

extern "C" int mage_embedding(const int64_t* ids, const float* table, void* out, int32_t out_dtype, int64_t n, int32_t C,
                              int32_t n_table, int32_t relu, int64_t group, int64_t group_stride, int64_t off, int64_t inner,
                              int64_t inner_stride, void* stream) {
    MAGE_CHECK_ARG(ids && table && out, "mage_embedding: null pointer");
    MAGE_CHECK_ARG(n > 0 && C > 0 && C % 4 == 0 && n_table > 0 && group > 0, "mage_embedding: bad sizes n=%ld C=%d", (long)n, C);
    if (inner <= 0) {                      // one-level grouping
        inner = group;
        inner_stride = group;
    }
    const dim3 grid((unsigned)((n + 3) / 4)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_embedding: mage_init() has not been called");
    if (out_dtype == MAGE_F32)
        hipLaunchKernelGGL((embedding_kernel<float>), grid, blk, 0, s, ids, table, (float*)out, (long)n, C, n_table, relu,
                           (long)group, (long)group_stride, (long)off, (long)inner, (long)inner_stride, err);
    else if (out_dtype == MAGE_BF16)
        hipLaunchKernelGGL((embedding_kernel<unsigned short>), grid, blk, 0, s, ids, table, (unsigned short*)out, (long)n, C,
                           n_table, relu, (long)group, (long)group_stride, (long)off, (long)inner, (long)inner_stride, err);
    else if (out_dtype == MAGE_F16)
        hipLaunchKernelGGL((embedding_kernel<f16_t>), grid, blk, 0, s, ids, table, (f16_t*)out, (long)n, C, n_table, relu, (long)group,
                           (long)group_stride, (long)off, (long)inner, (long)inner_stride, err);
    else if (out_dtype == MAGE_BF16X3 || out_dtype == MAGE_F16X3) {     // split rows (common.h): the frame convolution's A operand in the fast parity mode
        MAGE_CHECK_ARG(C % 64 == 0 && (((uintptr_t)out) & 255) == 0, "mage_embedding: split output needs C %% 64 == 0 and out 256-byte aligned");
        if (out_dtype == MAGE_BF16X3)
            hipLaunchKernelGGL((embedding_kernel<split_bf16>), grid, blk, 0, s, ids, table, (split_bf16*)out, (long)n, C, n_table, relu,
                               (long)group, (long)group_stride, (long)off, (long)inner, (long)inner_stride, err);
        else
            hipLaunchKernelGGL((embedding_kernel<split_f16>), grid, blk, 0, s, ids, table, (split_f16*)out, (long)n, C, n_table, relu,
                               (long)group, (long)group_stride, (long)off, (long)inner, (long)inner_stride, err);
    } else {
        mage_set_error("mage_embedding: bad out_dtype %d", out_dtype);
        return MAGE_EINVAL;
    }
    MAGE_CHECK_LAUNCH("mage_embedding");
    return MAGE_OK;
}

extern "C" int mage_argmax(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride,
                           int64_t in_off, int64_t* out, int64_t out_group_stride, int64_t out_off, float* margin,
                           void* stream) {
    MAGE_CHECK_ARG(logits && out, "mage_argmax: null pointer");
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && ld % 4 == 0 && group > 0, "mage_argmax: bad sizes rows=%ld K=%d", (long)rows, K);
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, (long)rows,
                       K, (long)ld, (long)group, (long)in_group_stride, (long)in_off, out, (long)out_group_stride,
                       (long)out_off, margin);
    MAGE_CHECK_LAUNCH("mage_argmax");
    return MAGE_OK;
}

template <int NV>
static void sample_launch(bool topk, bool topp, dim3 grid, hipStream_t s, const float* logits, long rows, int K, long ld, long group,
                          long in_stride, long in_off, int64_t* out, long out_stride, long out_off, const int64_t* seeds, long pos_off,
                          float inv_t, int top_k, float top_p) {
#define MAGE_SAMPLE(TK, TP)                                                                                                          \
    hipLaunchKernelGGL((sample_kernel<NV, TK, TP>), grid, dim3(256), 0, s, logits, rows, K, ld, group, in_stride, in_off, out,   \
                       out_stride, out_off, seeds, pos_off, inv_t, top_k, top_p)
    if (topk && topp) MAGE_SAMPLE(true, true);
    else if (topk) MAGE_SAMPLE(true, false);
    else if (topp) MAGE_SAMPLE(false, true);
    else MAGE_SAMPLE(false, false);
#undef MAGE_SAMPLE
}

extern "C" int mage_sample_tokens(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride,
                                  int64_t in_off, int64_t* out, int64_t out_group_stride, int64_t out_off, const int64_t* seeds,
                                  int64_t pos_off, float temperature, int32_t top_k, float top_p, void* stream) {
    MAGE_CHECK_ARG(logits && out && seeds, "mage_sample_tokens: null pointer");
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && K <= MAGE_SAMPLE_MAX_K && ld % 4 == 0 && ld >= K && group > 0 && pos_off >= 0 &&
                   (((uintptr_t)logits) & 15) == 0,
                   "mage_sample_tokens: bad sizes rows=%ld K=%d ld=%ld (K %% 4 == 0, K <= %d, 16-byte aligned rows)", (long)rows, K,
                   (long)ld, MAGE_SAMPLE_MAX_K);
    MAGE_CHECK_ARG(top_k >= 0 && top_k <= K, "mage_sample_tokens: top_k=%d outside [0, K=%d]", top_k, K);
    MAGE_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "mage_sample_tokens: top_p=%g outside (0, 1]", (double)top_p);
    const float inv_t = (float)(1.0 / (double)temperature);
    MAGE_CHECK_ARG(__builtin_isfinite(temperature) && temperature > 0.f && __builtin_isfinite(inv_t),
                   "mage_sample_tokens: temperature=%g must be finite and > 0", (double)temperature);
    if (top_k == 1)                                     // greedy by definition: first maximum of the logits
        return mage_argmax(logits, rows, K, ld, group, in_group_stride, in_off, out, out_group_stride, out_off, nullptr, stream);
    const bool topk = top_k > 0 && top_k < K, topp = top_p < 1.f;
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const long a[] = {(long)rows, (long)ld, (long)group, (long)in_group_stride, (long)in_off, (long)out_group_stride, (long)out_off,
                      (long)pos_off};
    if (K <= 256) sample_launch<4>(topk, topp, grid, s, logits, a[0], K, a[1], a[2], a[3], a[4], out, a[5], a[6], seeds, a[7], inv_t, top_k, top_p);
    else if (K <= 512) sample_launch<8>(topk, topp, grid, s, logits, a[0], K, a[1], a[2], a[3], a[4], out, a[5], a[6], seeds, a[7], inv_t, top_k, top_p);
    else if (K <= 1024) sample_launch<16>(topk, topp, grid, s, logits, a[0], K, a[1], a[2], a[3], a[4], out, a[5], a[6], seeds, a[7], inv_t, top_k, top_p);
    else if (K <= 2048) sample_launch<32>(topk, topp, grid, s, logits, a[0], K, a[1], a[2], a[3], a[4], out, a[5], a[6], seeds, a[7], inv_t, top_k, top_p);
    else sample_launch<64>(topk, topp, grid, s, logits, a[0], K, a[1], a[2], a[3], a[4], out, a[5], a[6], seeds, a[7], inv_t, top_k, top_p);
    MAGE_CHECK_LAUNCH("mage_sample_tokens");
    return MAGE_OK;
}

// ---- seeded standard-normal noise of the randomness branch (mage_video_noise; include/mage_hip_ext.h states the rule).  Element
// e = channel * hw + pixel of a clip with seed s takes the two counters base + 2e and base + 2e + 1, base = (s ^ 2^63) * 0x9e3779b97f4a7c15
// (uint64 wrap-around): the sampler's counters of the same seed start at s * 0x9e3779b97f4a7c15, exactly 2^63 away (the constant is odd), so
// the two streams of one seed cannot meet while either is shorter than 2^63.  Box-Muller, one normal per element: the radius from the 24-bit
// uniform of the first counter through sample_neglog_u (never rounded), the angle from the 23-bit one of the second through cospif of the
// exactly representable (m2 + 0.5) 2^-22.
// One lane owns a tile of 4 channels x 4 pixels and computes its 16 values ONCE: four 16-byte stores along the pixels into the NCHW tensor
// and / or four along the channels into the channel-last rows, so the two layouts hold the same bits by construction.  Lanes run along the
// channel quads first: the rows output is written in runs of 4 C bytes (whole rows), the NCHW output in runs of 64 bytes per channel.  A
// quad that crosses the end of its axis, or whose address is not 16-byte aligned (hw or C no multiple of 4), is stored element by element.
namespace {

constexpr unsigned long long NOISE_SEPARATION = 0x8000000000000000ULL;

__device__ __forceinline__ float video_noise_value(unsigned long long base, unsigned long long e) {
    const unsigned long long ctr = base + 2ULL * e;
    const float nl = sample_neglog_u(hash32(ctr) >> 8);                     // -log(u1), in (2^-25, 25 log 2]
    const unsigned m2 = hash32(ctr + 1ULL) >> 9;
    return __fmul_rn(sqrtf(2.0f * nl), cospif(((float)m2 + 0.5f) * 0x1p-22f));
}

__global__ __launch_bounds__(256) void video_noise_kernel(const int64_t* __restrict__ seeds, long tiles, int C, int hw, int CQ, int PQ,
                                                          float* __restrict__ nchw, float* __restrict__ rows) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= tiles) return;
    const int c0 = (int)(t % CQ) * 4;
    const long r = t / CQ;
    const int p0 = (int)(r % PQ) * 4;
    const long b = r / PQ;
    const unsigned long long base = ((unsigned long long)seeds[b] ^ NOISE_SEPARATION) * 0x9e3779b97f4a7c15ULL;
    float v[4][4];                                                          // [channel][pixel] of the tile
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int pi = 0; pi < 4; ++pi)
            v[ci][pi] = (c0 + ci < C && p0 + pi < hw) ? video_noise_value(base, (unsigned long long)(c0 + ci) * (unsigned)hw + (unsigned)(p0 + pi))
                                                      : 0.f;
    if (nchw) {
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            if (c0 + ci >= C) break;
            const long i = (b * C + c0 + ci) * (long)hw + p0;
            if (p0 + 3 < hw && (i & 3) == 0) {
                store4(nchw + i, f32x4{v[ci][0], v[ci][1], v[ci][2], v[ci][3]});
            } else {
#pragma unroll
                for (int pi = 0; pi < 4; ++pi)
                    if (p0 + pi < hw) nchw[i + pi] = v[ci][pi];
            }
        }
    }
    if (rows) {
#pragma unroll
        for (int pi = 0; pi < 4; ++pi) {
            if (p0 + pi >= hw) break;
            const long i = (b * hw + p0 + pi) * (long)C + c0;
            if (c0 + 3 < C && (i & 3) == 0) {
                store4(rows + i, f32x4{v[0][pi], v[1][pi], v[2][pi], v[3][pi]});
            } else {
#pragma unroll
                for (int ci = 0; ci < 4; ++ci)
                    if (c0 + ci < C) rows[i + ci] = v[ci][pi];
            }
        }
    }
}

}  // namespace

extern "C" int mage_video_noise(const int64_t* seeds, int64_t B, int32_t C, int64_t hw, float* nchw, float* rows, void* stream) {
    MAGE_CHECK_ARG(seeds && (((uintptr_t)seeds) & 7) == 0, "mage_video_noise: seeds must be a non-null, 8-byte aligned int64 pointer");
    MAGE_CHECK_ARG(B > 0 && C > 0 && hw > 0, "mage_video_noise: bad sizes B=%ld C=%d hw=%ld (all must be > 0)", (long)B, C, (long)hw);
    MAGE_CHECK_ARG(nchw || rows, "mage_video_noise: no output (give the NCHW tensor, the channel-last rows, or both)");
    MAGE_CHECK_ARG((((uintptr_t)nchw) & 15) == 0 && (((uintptr_t)rows) & 15) == 0, "mage_video_noise: outputs must be 16-byte aligned");
    // a clip's counters are base + 2e + {0, 1} with e < C*hw <= 2^30 (the kernel's 32-bit tile coordinates cannot wrap, the counters stay
    // below 2^31); the launch is one lane per 4 x 4 tile, at most 2^38 of them
    MAGE_CHECK_ARG(hw <= (1LL << 30) && (int64_t)C * hw <= (1LL << 30) && B <= (1LL << 38) / ((int64_t)C * hw),
                   "mage_video_noise: B=%ld C=%d hw=%ld is past the counter range (C*hw <= 2^30, B*C*hw <= 2^38)", (long)B, C, (long)hw);
    const int CQ = (C + 3) / 4, PQ = (int)((hw + 3) / 4);
    const long tiles = (long)B * CQ * PQ;
    video_noise_kernel<<<dim3((unsigned)((tiles + 255) / 256)), 256, 0, (hipStream_t)stream>>>(seeds, tiles, C, (int)hw, CQ, PQ, nchw, rows);
    MAGE_CHECK_LAUNCH("mage_video_noise");
    return MAGE_OK;
}

extern "C" int mage_token_logprob(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride,
                                  int64_t in_off, const int64_t* tokens, float* logprob, int64_t tok_group_stride, int64_t tok_off,
                                  void* stream) {
    MAGE_CHECK_ARG(logits && tokens && logprob, "mage_token_logprob: null pointer");
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && K <= MAGE_SAMPLE_MAX_K && ld % 4 == 0 && ld >= K && group > 0 && in_group_stride >= 0 &&
                   in_off >= 0 && tok_group_stride >= 0 && tok_off >= 0 && (((uintptr_t)logits) & 15) == 0,
                   "mage_token_logprob: bad sizes rows=%ld K=%d ld=%ld (K %% 4 == 0, K <= %d, 16-byte aligned rows)", (long)rows, K, (long)ld,
                   MAGE_SAMPLE_MAX_K);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_token_logprob: mage_init() has not been called");
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_LOGPROB(NV)                                                                                                             \
    hipLaunchKernelGGL((token_logprob_kernel<NV>), grid, dim3(256), 0, s, logits, (long)rows, K, (long)ld, (long)group,              \
                       (long)in_group_stride, (long)in_off, tokens, logprob, (long)tok_group_stride, (long)tok_off, err)
    if (K <= 256) MAGE_LOGPROB(4);
    else if (K <= 512) MAGE_LOGPROB(8);
    else if (K <= 1024) MAGE_LOGPROB(16);
    else if (K <= 2048) MAGE_LOGPROB(32);
    else MAGE_LOGPROB(64);
#undef MAGE_LOGPROB
    MAGE_CHECK_LAUNCH("mage_token_logprob");
    return MAGE_OK;
}

template <int NV>
static void stats_launch(int mode, dim3 grid, hipStream_t s, const float* logits, long rows, int K, long ld, long group, long in_stride, long in_off,
                         const int64_t* tokens, long tok_stride, long tok_off, float inv_t, int top_k, float top_p, float* policy_logprob,
                         float* policy_entropy, int32_t* kept, float* entropy, int* err) {
#define MAGE_STATS(M)                                                                                                                 \
    hipLaunchKernelGGL((token_stats_kernel<NV, M>), grid, dim3(256), 0, s, logits, rows, K, ld, group, in_stride, in_off, tokens, tok_stride, \
                       tok_off, inv_t, top_k, top_p, policy_logprob, policy_entropy, kept, entropy, err)
    if (mode == STATS_GREEDY) MAGE_STATS(STATS_GREEDY);
    else if (mode == (STATS_TOPK | STATS_TOPP)) MAGE_STATS(STATS_TOPK | STATS_TOPP);
    else if (mode == STATS_TOPK) MAGE_STATS(STATS_TOPK);
    else if (mode == STATS_TOPP) MAGE_STATS(STATS_TOPP);
    else MAGE_STATS(0);
#undef MAGE_STATS
}

extern "C" int mage_token_stats(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride, int64_t in_off,
                                const int64_t* tokens, int64_t tok_group_stride, int64_t tok_off, float temperature, int32_t top_k, float top_p,
                                float* policy_logprob, float* policy_entropy, int32_t* kept, float* entropy, void* stream) {
    MAGE_CHECK_ARG(logits && (policy_logprob || policy_entropy || kept || entropy), "mage_token_stats: null logits, or no output asked for");
    MAGE_CHECK_ARG(tokens || !policy_logprob, "mage_token_stats: policy_logprob needs tokens");
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && K <= MAGE_SAMPLE_MAX_K && ld % 4 == 0 && ld >= K && group > 0 && in_group_stride >= 0 &&
                   in_off >= 0 && tok_group_stride >= 0 && tok_off >= 0 && (((uintptr_t)logits) & 15) == 0,
                   "mage_token_stats: bad sizes rows=%ld K=%d ld=%ld (K %% 4 == 0, K <= %d, 16-byte aligned rows)", (long)rows, K, (long)ld,
                   MAGE_SAMPLE_MAX_K);
    MAGE_CHECK_ARG(top_k >= 0 && top_k <= K, "mage_token_stats: top_k=%d outside [0, K=%d]", top_k, K);
    MAGE_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "mage_token_stats: top_p=%g outside (0, 1]", (double)top_p);
    const float inv_t = (float)(1.0 / (double)temperature);
    MAGE_CHECK_ARG(__builtin_isfinite(temperature) && temperature > 0.f && __builtin_isfinite(inv_t),
                   "mage_token_stats: temperature=%g must be finite and > 0", (double)temperature);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_token_stats: mage_init() has not been called");
    const int mode = top_k == 1 ? STATS_GREEDY : (top_k > 0 && top_k < K ? STATS_TOPK : 0) | (top_p < 1.f ? STATS_TOPP : 0);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_STATS_NV(NV)                                                                                                              \
    stats_launch<NV>(mode, grid, s, logits, (long)rows, K, (long)ld, (long)group, (long)in_group_stride, (long)in_off, tokens,         \
                     (long)tok_group_stride, (long)tok_off, mode == STATS_GREEDY ? 1.f : inv_t, top_k, top_p, policy_logprob, policy_entropy, kept, entropy, err)
    if (K <= 256) MAGE_STATS_NV(4);
    else if (K <= 512) MAGE_STATS_NV(8);
    else if (K <= 1024) MAGE_STATS_NV(16);
    else if (K <= 2048) MAGE_STATS_NV(32);
    else MAGE_STATS_NV(64);
#undef MAGE_STATS_NV
    MAGE_CHECK_LAUNCH("mage_token_stats");
    return MAGE_OK;
}

// ---- classifier-free guidance of the logits (mage_guide_logits; include/mage_hip_ext.h states the rule): z = c + (s - 1)(c - u) per element,
// one explicit fma behind two selects that make scale 1 and u == c return c's bits.  Pure streaming, 12 bytes per element: no reduction, no
// LDS, no atomics.  A workgroup owns RB whole rows (RB * K/4 quads, about 1024: four per lane); consecutive lanes take consecutive quads, so a
// wave-instruction moves 1 KiB of one row (or of adjacent rows), and a lane issues all of its up to eight 16-byte loads before the first
// store: ~32 KiB in flight per workgroup.  A lane reads the quads it writes and no other, before it writes them: out may be cond itself.
namespace {

constexpr int GUIDE_QUADS = 4;                                              // quads per lane

__global__ __launch_bounds__(256) void guide_logits_kernel(const float* cond, const float* uncond, float* out, long rows, int KQ, long ld, long group,
                                                           long in_stride, long in_off, const float* __restrict__ scale, long scale_div, int RB) {
    const long row0 = (long)blockIdx.x * RB;
    const long left = rows - row0;
    const int n = (int)(left < RB ? left : RB) * KQ;                        // this workgroup's quads
    long at[GUIDE_QUADS];
    float w[GUIDE_QUADS];
    f32x4 c[GUIDE_QUADS], u[GUIDE_QUADS];
#pragma unroll
    for (int j = 0; j < GUIDE_QUADS; ++j) {
        const int idx = (int)threadIdx.x + j * 256;
        if (idx < n) {
            const int r = idx / KQ;
            const long row = row0 + r;
            at[j] = ((row / group) * in_stride + row % group + in_off) * ld + 4 * (idx - r * KQ);
            w[j] = __fsub_rn(scale[row / scale_div], 1.0f);
            c[j] = load4(cond + at[j]);
            u[j] = load4(uncond + at[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < GUIDE_QUADS; ++j) {
        if ((int)threadIdx.x + j * 256 < n) {
            f32x4 z;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = __fsub_rn(c[j][e], u[j][e]);
                z[e] = (w[j] == 0.f || d == 0.f) ? c[j][e] : __fmaf_rn(w[j], d, c[j][e]);
            }
            store4(out + at[j], z);
        }
    }
}

}  // namespace

extern "C" int mage_guide_logits(const float* cond, const float* uncond, float* out, int64_t rows, int32_t K, int64_t ld, int64_t group,
                                 int64_t in_group_stride, int64_t in_off, const float* scale, int64_t scale_div, void* stream) {
    MAGE_CHECK_ARG(cond && uncond && out && scale, "mage_guide_logits: null pointer");
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && K <= MAGE_SAMPLE_MAX_K && ld % 4 == 0 && ld >= K && group > 0 && in_group_stride >= 0 &&
                   in_off >= 0 && scale_div > 0,
                   "mage_guide_logits: bad sizes rows=%ld K=%d ld=%ld group=%ld scale_div=%ld (K %% 4 == 0, K <= %d, ld %% 4 == 0, ld >= K)",
                   (long)rows, K, (long)ld, (long)group, (long)scale_div, MAGE_SAMPLE_MAX_K);
    MAGE_CHECK_ARG(((((uintptr_t)cond) | ((uintptr_t)uncond) | ((uintptr_t)out)) & 15) == 0 && (((uintptr_t)scale) & 3) == 0,
                   "mage_guide_logits: cond, uncond and out must be 16-byte aligned, scale 4-byte aligned");
    const int KQ = K / 4;
    const int RB = KQ >= 256 * GUIDE_QUADS ? 1 : 256 * GUIDE_QUADS / KQ;    // whole rows per workgroup, RB * KQ <= 1024 quads
    const int64_t blocks = (rows + RB - 1) / RB;
    MAGE_CHECK_ARG(blocks <= 0x7fffffffLL, "mage_guide_logits: rows=%ld is more than one launch covers", (long)rows);
    guide_logits_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(cond, uncond, out, (long)rows, KQ, (long)ld, (long)group,
                                                                                (long)in_group_stride, (long)in_off, scale, (long)scale_div, RB);
    MAGE_CHECK_LAUNCH("mage_guide_logits");
    return MAGE_OK;
}

// ---- given tokens over picked ones (mage_apply_known_tokens; include/mage_hip_ext.h states the rule).  One thread per row: it reads its
// `known` value and, where that is >= 0, stores it and the certain policy's results (log-probabilities 0, entropies 0, kept 1) at the row's
// token index.  A free row stores nothing.  8 bytes read and at most 28 written per row: launch-bound at a frame's size.  No LDS, no atomics.
namespace {

__global__ __launch_bounds__(256) void apply_known_kernel(int64_t* __restrict__ tokens, long rows, long group, long tok_stride, long tok_off,
                                                          const int64_t* __restrict__ known, long known_stride, long known_off, long known_div,
                                                          int K, float* __restrict__ logprob, float* __restrict__ policy_logprob,
                                                          float* __restrict__ entropy, float* __restrict__ policy_entropy,
                                                          int32_t* __restrict__ kept, int* __restrict__ err) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const long c = i / group, j = i - c * group;
    long k = known[(c / known_div) * known_stride + j + known_off];
    if (k < 0) return;
    if (k >= K) {                                       // reported by mage_check_device_errors, as mage_token_logprob's bad token is
        mage_raise(err, MAGE_DEVERR_TOKEN_ID, k, K);
        k = K - 1;
    }
    const long t = c * tok_stride + j + tok_off;
    tokens[t] = k;
    if (logprob) logprob[t] = 0.f;
    if (policy_logprob) policy_logprob[t] = 0.f;
    if (entropy) entropy[t] = 0.f;
    if (policy_entropy) policy_entropy[t] = 0.f;
    if (kept) kept[t] = 1;
}

}  // namespace

extern "C" int mage_apply_known_tokens(int64_t* tokens, int64_t rows, int64_t group, int64_t tok_group_stride, int64_t tok_off,
                                       const int64_t* known, int64_t known_group_stride, int64_t known_off, int64_t known_clip_div, int32_t K,
                                       float* logprob, float* policy_logprob, float* entropy, float* policy_entropy, int32_t* kept,
                                       void* stream) {
    MAGE_CHECK_ARG(tokens && known, "mage_apply_known_tokens: null pointer");
    MAGE_CHECK_ARG(rows >= 0 && group > 0 && known_clip_div > 0 && tok_group_stride >= 0 && tok_off >= 0 && known_group_stride >= 0 &&
                   known_off >= 0 && K > 0,
                   "mage_apply_known_tokens: bad sizes rows=%ld group=%ld known_clip_div=%ld K=%d (strides and offsets >= 0)", (long)rows,
                   (long)group, (long)known_clip_div, K);
    if (rows == 0) return MAGE_OK;
    const int64_t blocks = (rows + 255) / 256;
    MAGE_CHECK_ARG(blocks <= 0x7fffffffLL, "mage_apply_known_tokens: rows=%ld is more than one launch covers", (long)rows);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_apply_known_tokens: mage_init() has not been called");
    apply_known_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(tokens, (long)rows, (long)group, (long)tok_group_stride,
                                                                               (long)tok_off, known, (long)known_group_stride, (long)known_off,
                                                                               (long)known_clip_div, K, logprob, policy_logprob, entropy,
                                                                               policy_entropy, kept, err);
    MAGE_CHECK_LAUNCH("mage_apply_known_tokens");
    return MAGE_OK;
}

extern "C" int mage_clip_scores(const float* logprob, int64_t n_clips, int32_t n_cand, int64_t per_clip, float* scores, int64_t* best,
                                void* stream) {
    MAGE_CHECK_ARG(logprob && scores, "mage_clip_scores: null pointer");
    MAGE_CHECK_ARG(n_clips > 0 && n_clips <= 0x7fffffffL && n_cand > 0 && per_clip > 0, "mage_clip_scores: bad sizes n_clips=%ld n_cand=%d per_clip=%ld",
                   (long)n_clips, n_cand, (long)per_clip);
    MAGE_CHECK_ARG(n_cand == 1 || best, "mage_clip_scores: n_cand=%d > 1 needs `best`", n_cand);
    hipLaunchKernelGGL(clip_scores_kernel, dim3((unsigned)n_clips), dim3(256), 0, (hipStream_t)stream, logprob, n_cand, (long)per_clip, scores,
                       n_cand > 1 ? best : nullptr);
    MAGE_CHECK_LAUNCH("mage_clip_scores");
    return MAGE_OK;
}

extern "C" int mage_cross_entropy(const float* logits, const int64_t* target, int64_t rows, int32_t K, float* row_loss,
                                  float* loss_mean, void* stream) {
    MAGE_CHECK_ARG(logits && target && row_loss && loss_mean, "mage_cross_entropy: null pointer");
    MAGE_CHECK_ARG(rows > 0 && K > 0, "mage_cross_entropy: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_cross_entropy: mage_init() has not been called");
    hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, target, (long)rows, K, row_loss, err);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, s, row_loss, (long)rows, loss_mean, 1.0 / (double)rows);
    MAGE_CHECK_LAUNCH("mage_cross_entropy");
    return MAGE_OK;
}

// the argument rules mage_policy_loss and mage_policy_loss_bwd share (mage_token_stats' sizes and temperature, the clip and the entropy weight)
static int policy_check(const char* who, const void* logits, int64_t rows, int32_t K, int64_t ld, int64_t adv_div, float temperature,
                        float inv_t, float clip_lo, float clip_hi, float entropy_coef) {
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && K <= MAGE_SAMPLE_MAX_K && ld % 4 == 0 && ld >= K && adv_div > 0 &&
                   (((uintptr_t)logits) & 15) == 0,
                   "%s: bad sizes rows=%ld K=%d ld=%ld adv_div=%ld (K %% 4 == 0, K <= %d, 16-byte aligned rows)", who, (long)rows, K, (long)ld,
                   (long)adv_div, MAGE_SAMPLE_MAX_K);
    MAGE_CHECK_ARG(__builtin_isfinite(temperature) && temperature > 0.f && __builtin_isfinite(inv_t),
                   "%s: temperature=%g must be finite and > 0", who, (double)temperature);
    MAGE_CHECK_ARG(clip_lo >= 0.f && clip_lo <= 1.f && clip_hi >= 0.f, "%s: clip_lo=%g outside [0, 1] or clip_hi=%g < 0", who, (double)clip_lo,
                   (double)clip_hi);
    MAGE_CHECK_ARG(__builtin_isfinite(entropy_coef), "%s: entropy_coef=%g must be finite", who, (double)entropy_coef);
    return MAGE_OK;
}

// what the anchored pair asks in addition: a reference log-probability per row and a weight that is a number
static int policy_anchor_check(const char* who, const float* reference_logprob, float kl_coef) {
    MAGE_CHECK_ARG(reference_logprob && (((uintptr_t)reference_logprob) & 3) == 0, "%s: reference_logprob must be a 4-byte aligned pointer", who);
    MAGE_CHECK_ARG(__builtin_isfinite(kl_coef) && kl_coef >= 0.f, "%s: kl_coef=%g must be finite and >= 0", who, (double)kl_coef);
    return MAGE_OK;
}

template <int NV, bool ANCH>
static void policy_launch(bool topk, bool topp, dim3 grid, hipStream_t s, const float* logits, long rows, int K, long ld, const int64_t* tokens,
                          const float* adv, long adv_div, const float* blp, float inv_t, int top_k, float top_p, float cmin, float cmax,
                          float ent_coef, float* row_loss, float* logprob, float* entropy, uint32_t* cut, int* err, const float* ref,
                          float kl_coef, float* kl, const uint8_t* given) {
#define MAGE_POLICY(TK, TP)                                                                                                                  \
    hipLaunchKernelGGL((policy_loss_kernel<NV, TK, TP, ANCH>), grid, dim3(256), 0, s, logits, rows, K, ld, tokens, adv, adv_div, blp, inv_t, \
                       top_k, top_p, cmin, cmax, ent_coef, row_loss, logprob, entropy, cut, err, ref, kl_coef, kl, given)
    if (topk && topp) MAGE_POLICY(true, true);
    else if (topk) MAGE_POLICY(true, false);
    else if (topp) MAGE_POLICY(false, true);
    else MAGE_POLICY(false, false);
#undef MAGE_POLICY
}

// mage_policy_loss (ANCH false: reference_logprob, kl_coef and kl unused) and mage_policy_loss_anchored behind their own argument rules;
// given non-null: mage_policy_loss_masked in either form (the masked reduction, norm written)
template <bool ANCH>
static int policy_forward(const char* who, const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                          int64_t adv_div, const float* behaviour_logprob, float temperature, int32_t top_k, float top_p, float clip_lo,
                          float clip_hi, float entropy_coef, float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* summary,
                          const float* reference_logprob, float kl_coef, float* kl, void* stream, const uint8_t* given = nullptr,
                          float* norm = nullptr) {
    MAGE_CHECK_ARG(logits && tokens && advantage && row_loss && logprob && entropy && cut && summary, "%s: null pointer", who);
    const float inv_t = (float)(1.0 / (double)temperature);
    if (int rc = policy_check(who, logits, rows, K, ld, adv_div, temperature, inv_t, clip_lo, clip_hi, entropy_coef)) return rc;
    MAGE_CHECK_ARG(top_k >= 0 && top_k <= K, "%s: top_k=%d outside [0, K=%d]", who, top_k, K);
    MAGE_CHECK_ARG(top_k != 1, "%s: top_k=1 is greedy decoding: its log-probability is 0 and has no gradient", who);
    MAGE_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "%s: top_p=%g outside (0, 1]", who, (double)top_p);
    if (ANCH)
        if (int rc = policy_anchor_check(who, reference_logprob, kl_coef)) return rc;
    MAGE_CHECK_ARG(!ANCH || (kl && (((uintptr_t)kl) & 3) == 0), "%s: kl must be a 4-byte aligned pointer", who);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "%s: mage_init() has not been called", who);
    const bool topk = top_k > 0 && top_k < K, topp = top_p < 1.f;
    const float cmin = (float)(1.0 - (double)clip_lo), cmax = (float)(1.0 + (double)clip_hi);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_POLICY_NV(NV)                                                                                                                   \
    policy_launch<NV, ANCH>(topk, topp, grid, s, logits, (long)rows, K, (long)ld, tokens, advantage, (long)adv_div, behaviour_logprob, inv_t, \
                            top_k, top_p, cmin, cmax, entropy_coef, row_loss, logprob, entropy, cut, err, reference_logprob, kl_coef, kl, \
                            given)
    if (K <= 256) MAGE_POLICY_NV(4);
    else if (K <= 512) MAGE_POLICY_NV(8);
    else if (K <= 1024) MAGE_POLICY_NV(16);
    else if (K <= 2048) MAGE_POLICY_NV(32);
    else MAGE_POLICY_NV(64);
#undef MAGE_POLICY_NV
    constexpr int W = ANCH ? POLICY_MEANS : 5;
    const long chunk = (long)((rows + POLICY_PARTS - 1) / POLICY_PARTS);
    if (given) {
        hipLaunchKernelGGL(policy_part_kernel<POLICY_MASKED>, dim3(POLICY_PARTS), dim3(256), 0, s, row_loss, logprob, entropy, advantage,
                           (long)adv_div, behaviour_logprob, cmin, cmax, (long)rows, chunk, kl, reference_logprob, given);
        hipLaunchKernelGGL(policy_summary_masked_kernel, dim3(1), dim3(POLICY_PARTS), 0, s, summary, norm, (long)rows);
    } else {
        hipLaunchKernelGGL(policy_part_kernel<W>, dim3(POLICY_PARTS), dim3(256), 0, s, row_loss, logprob, entropy, advantage, (long)adv_div,
                           behaviour_logprob, cmin, cmax, (long)rows, chunk, kl, reference_logprob, given);
        hipLaunchKernelGGL(policy_summary_kernel<W>, dim3(1), dim3(POLICY_PARTS), 0, s, summary, 1.0 / (double)rows);
    }
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

template <bool ANCH>
static int policy_backward(const char* who, const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                           const float* advantage, int64_t adv_div, const float* behaviour_logprob, const uint32_t* cut, float temperature,
                           float clip_lo, float clip_hi, float entropy_coef, const float* grad_out, void* dlogits, int32_t dl_dtype,
                           const float* reference_logprob, float kl_coef, void* stream, const uint8_t* given = nullptr,
                           const float* norm = nullptr) {
    MAGE_CHECK_ARG(logits && tokens && advantage && cut && grad_out && dlogits, "%s: null pointer", who);
    const float inv_t = (float)(1.0 / (double)temperature);
    if (int rc = policy_check(who, logits, rows, K, ld, adv_div, temperature, inv_t, clip_lo, clip_hi, entropy_coef)) return rc;
    MAGE_CHECK_ARG((dl_dtype == MAGE_F32 || dl_dtype == MAGE_BF16) && (((uintptr_t)dlogits) & 15) == 0,
                   "%s: dlogits must be 16-byte aligned fp32 or bf16 (dtype %d)", who, dl_dtype);
    if (ANCH)
        if (int rc = policy_anchor_check(who, reference_logprob, kl_coef)) return rc;
    const float cmin = (float)(1.0 - (double)clip_lo), cmax = (float)(1.0 + (double)clip_hi);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_POLICY_BWD(NV, OT)                                                                                                            \
    hipLaunchKernelGGL((policy_loss_bwd_kernel<NV, OT, ANCH>), grid, dim3(256), 0, s, logits, (long)rows, K, (long)ld, tokens, advantage, \
                       (long)adv_div, behaviour_logprob, cut, inv_t, cmin, cmax, entropy_coef, grad_out, 1.0f / (float)rows, (OT*)dlogits, \
                       reference_logprob, kl_coef, given, norm)
#define MAGE_POLICY_BWD_NV(NV)                                  \
    do {                                                        \
        if (dl_dtype == MAGE_F32) MAGE_POLICY_BWD(NV, float);   \
        else MAGE_POLICY_BWD(NV, unsigned short);               \
    } while (0)
    if (K <= 256) MAGE_POLICY_BWD_NV(4);
    else if (K <= 512) MAGE_POLICY_BWD_NV(8);
    else if (K <= 1024) MAGE_POLICY_BWD_NV(16);
    else if (K <= 2048) MAGE_POLICY_BWD_NV(32);
    else MAGE_POLICY_BWD_NV(64);
#undef MAGE_POLICY_BWD_NV
#undef MAGE_POLICY_BWD
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

extern "C" int mage_policy_loss(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                int64_t adv_div, const float* behaviour_logprob, float temperature, int32_t top_k, float top_p, float clip_lo,
                                float clip_hi, float entropy_coef, float* row_loss, float* logprob, float* entropy, uint32_t* cut,
                                float* summary, void* stream) {
    return policy_forward<false>("mage_policy_loss", logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, top_k, top_p,
                                 clip_lo, clip_hi, entropy_coef, row_loss, logprob, entropy, cut, summary, nullptr, 0.f, nullptr, stream);
}

extern "C" int mage_policy_loss_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                    int64_t adv_div, const float* behaviour_logprob, const uint32_t* cut, float temperature, float clip_lo,
                                    float clip_hi, float entropy_coef, const float* grad_out, void* dlogits, int32_t dl_dtype, void* stream) {
    return policy_backward<false>("mage_policy_loss_bwd", logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, cut, temperature,
                                  clip_lo, clip_hi, entropy_coef, grad_out, dlogits, dl_dtype, nullptr, 0.f, stream);
}

extern "C" int mage_policy_loss_anchored(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                         int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                                         int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef,
                                         float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary,
                                         void* stream) {
    return policy_forward<true>("mage_policy_loss_anchored", logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, top_k,
                                top_p, clip_lo, clip_hi, entropy_coef, row_loss, logprob, entropy, cut, summary, reference_logprob, kl_coef, kl,
                                stream);
}

extern "C" int mage_policy_loss_anchored_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                             const float* advantage, int64_t adv_div, const float* behaviour_logprob,
                                             const float* reference_logprob, const uint32_t* cut, float temperature, float clip_lo,
                                             float clip_hi, float entropy_coef, float kl_coef, const float* grad_out, void* dlogits,
                                             int32_t dl_dtype, void* stream) {
    return policy_backward<true>("mage_policy_loss_anchored_bwd", logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, cut,
                                 temperature, clip_lo, clip_hi, entropy_coef, grad_out, dlogits, dl_dtype, reference_logprob, kl_coef, stream);
}

// the mask and the normaliser of the masked pair, and its one rule about the anchor: reference_logprob and kl come together or not at all
static int policy_masked_check(const char* who, const uint8_t* given, const float* norm, bool has_ref, bool has_kl, float kl_coef) {
    MAGE_CHECK_ARG(given != nullptr, "%s: given must not be null (the unmasked entry points take no mask)", who);
    MAGE_CHECK_ARG(norm && (((uintptr_t)norm) & 3) == 0, "%s: norm must be a 4-byte aligned pointer", who);
    MAGE_CHECK_ARG(has_ref == has_kl, "%s: reference_logprob and kl are given together (the anchored rule) or both null (the plain rule)", who);
    MAGE_CHECK_ARG(has_ref || kl_coef == 0.f, "%s: kl_coef=%g needs reference_logprob", who, (double)kl_coef);
    return MAGE_OK;
}

extern "C" int mage_policy_loss_masked(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                       int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                                       int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef,
                                       float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary, float* norm,
                                       const uint8_t* given, void* stream) {
    const char* who = "mage_policy_loss_masked";
    if (int rc = policy_masked_check(who, given, norm, reference_logprob != nullptr, kl != nullptr, kl_coef)) return rc;
    if (reference_logprob)
        return policy_forward<true>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, top_k, top_p, clip_lo,
                                    clip_hi, entropy_coef, row_loss, logprob, entropy, cut, summary, reference_logprob, kl_coef, kl, stream, given,
                                    norm);
    return policy_forward<false>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, top_k, top_p, clip_lo,
                                 clip_hi, entropy_coef, row_loss, logprob, entropy, cut, summary, nullptr, 0.f, nullptr, stream, given, norm);
}

extern "C" int mage_policy_loss_masked_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                           const float* advantage, int64_t adv_div, const float* behaviour_logprob,
                                           const float* reference_logprob, const uint32_t* cut, float temperature, float clip_lo, float clip_hi,
                                           float entropy_coef, float kl_coef, const float* grad_out, const float* norm, void* dlogits,
                                           int32_t dl_dtype, const uint8_t* given, void* stream) {
    const char* who = "mage_policy_loss_masked_bwd";
    if (int rc = policy_masked_check(who, given, norm, reference_logprob != nullptr, reference_logprob != nullptr, kl_coef)) return rc;
    if (reference_logprob)
        return policy_backward<true>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, cut, temperature, clip_lo, clip_hi,
                                     entropy_coef, grad_out, dlogits, dl_dtype, reference_logprob, kl_coef, stream, given, norm);
    return policy_backward<false>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, cut, temperature, clip_lo, clip_hi,
                                  entropy_coef, grad_out, dlogits, dl_dtype, nullptr, 0.f, stream, given, norm);
}
