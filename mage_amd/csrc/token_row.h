// One row of logits in the registers of one wave: the layout, the sampling filter and the fixed-order sums that the token heads share
// (token_heads.hip: sampling, log-probabilities, statistics; policy_loss.hip; preference.hip: the log-probabilities' backward; distill.hip: two rows per wave; xent.hip: the supervised loss).
// A workgroup of 256 threads takes four rows, wave by wave.  A lane holds NV values of its row as NV/4 chunks of 16 bytes: code
// k = c*256 + lane*4 + e is element e of chunk c, register c*4 + e.  NV = 4, 8, 16, 32, 64 covers K <= 256 .. 4096 (MAGE_ROW_LADDER).
// Every sum has one order: a lane adds its own terms in register order with explicit roundings, the lanes meet in an xor butterfly, so
// every lane holds the same bits and a row's bits depend on the row alone.  expf / logf are the accurate ones.  The heads promise each other
// equal bits (the sampler never draws what the statistics call impossible; policy_logprob equals mage_token_logprob; a backward pass keeps
// its forward pass's set) BECAUSE they call the functions below: change an operation here and every head changes with it.
#pragma once
#include "common.h"
#include "../../include/mage_hip_ext.h"

// ---- the sampling rule (mage_sample_tokens): temperature, top-k, top-p, Gumbel-max.  For one row:
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
// the AR mode, the number of streams or graph replay.  top_k == 1 is greedy by definition: mage_argmax's kernel (first maximum wins; step 4's
// "token 0" does not apply on that path: a row of NaNs yields mage_argmax's 0x7fffffff).
// The selections are bit-by-bit bisections over order-preserving uint keys of s: top-k counts with ballots (a scalar count, no shuffles),
// top-p sums the w_j with fixed-order butterflies.  Where the sums are rounded (W, the masses) a row whose boundary mass is within fp32
// rounding of top_p * W may keep one value more or less than the exact rule; nothing else is approximate.

// ---- addressing: row i of the call is row gr of group gi; a group's rows are contiguous, the groups in_stride rows apart
struct RowIndex { long gi, gr; };
__device__ __forceinline__ RowIndex row_index(long i, long group) {
    const long gi = i / group;
    return RowIndex{gi, i - gi * group};
}
__device__ __forceinline__ const float* row_logits(const float* __restrict__ logits, RowIndex r, long in_stride, long in_off, long ld) {
    return logits + (r.gi * in_stride + r.gr + in_off) * ld;
}
// the row's place in a token-shaped array (tokens, outputs)
__device__ __forceinline__ long row_slot(RowIndex r, long stride, long off) { return r.gi * stride + r.gr + off; }

// Chunk c of a row: one 16-byte load, 0 past K (the filter's form: its keys say what lies past K) ...
__device__ __forceinline__ f32x4 sample_row_chunk(const float* __restrict__ p, int lane, int K, int c) {
    const int k = c * 256 + lane * 4;
    return k < K ? *(const f32x4*)(p + k) : f32x4{0.f, 0.f, 0.f, 0.f};
}
// ... and -inf past K, the form row_logsumexp takes: a padding code is one more -inf logit (it leaves the maximum alone and adds
// exp(-inf) = 0).  token_stats_kernel once loaded zeros and skipped them behind k < K guards inside its sums; the sums are the same bit
// for bit, and this form needs no guard.  It serves sample_filter as well (s = -inf there, the key 0 as for any code past K), which is how
// token_stats_kernel reads its row once for both.
__device__ __forceinline__ f32x4 row_chunk_inf(const float* __restrict__ p, int lane, int K, int c) {
    const int k = c * 256 + lane * 4;
    return k < K ? *(const f32x4*)(p + k) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
}

// The row's token.  CLAMP: a token outside [0, K) is raised (MAGE_DEVERR_TOKEN_ID, reported by mage_check_device_errors; a null err leaves
// the report to the pass that ran before) and clamped into range, to stay memory-safe meanwhile.  !CLAMP: -1, no one-hot.
template <bool CLAMP = true>
__device__ __forceinline__ long row_token(const int64_t* __restrict__ tokens, long i, int K, int* err) {
    long tg = tokens[i];
    if (tg < 0 || tg >= K) {
        if (err) mage_raise(err, MAGE_DEVERR_TOKEN_ID, tg, K);
        tg = !CLAMP ? -1 : tg < 0 ? 0 : K - 1;
    }
    return tg;
}
// the masked entry points' per-row byte, one scalar value per wave (the row index is the wave's); a null mask has no given row
__device__ __forceinline__ bool row_given(const uint8_t* __restrict__ given, long i) {
    return given && __builtin_amdgcn_readfirstlane((int)given[i]) != 0;
}

// ---- keys
__device__ __forceinline__ unsigned sample_key(float s) {       // order-preserving; -0 == +0; NaN -> 0 (below every number: never kept)
    unsigned u = __float_as_uint(s);
    if (s != s) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
// the key of the row's largest s: >= the filter's threshold unless nothing is selectable (then every key is 0)
template <int NV>
__device__ __forceinline__ unsigned row_key_max(const unsigned (&key)[NV]) {
    unsigned km = 0u;
#pragma unroll
    for (int e = 0; e < NV; ++e) km = max(km, key[e]);
    return wave_max_u32(km);
}
// |N| by ballots: exact
template <int NV>
__device__ __forceinline__ int kept_count(const unsigned (&key)[NV], unsigned lo) {
    int n = 0;
#pragma unroll
    for (int e = 0; e < NV; ++e) n += __popcll(__ballot(key[e] >= lo));
    return n;
}

// Steps 1-3 of the rule for one row: s, key and the returned threshold lo >= 1 with N = { j : key_j >= lo }.  THE filter:
// mage_sample_tokens draws from this set, mage_token_stats reports on it and mage_policy_loss differentiates over it, so they agree bit
// for bit on every row, the ones whose rounded top-p masses keep a value more or less than the exact rule included.
template <int NV, bool TOPK, bool TOPP, typename ROW>
__device__ __forceinline__ unsigned sample_filter(ROW row, int lane, int K, float inv_t, int top_k, float top_p, float (&s)[NV],
                                                  unsigned (&key)[NV]) {
    // step 1, stated here and nowhere else (row_keys below is this function with nothing to filter).  As a helper called from here it
    // changed the machine code of the sampler's NV = 4 instances, and their top-p form measured 1.1 % slower (566 against 560 us for
    // 245 760 rows of 256, outside the 0.6 us repeat-to-repeat spread)
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
    unsigned lo = 1u;                                  // the candidate set: key >= lo
    if constexpr (TOPK) {                               // the largest t with #{key >= t} >= top_k: the top_k-th largest key
        unsigned t = 0u;
        auto bit = [&](int b) {
            const unsigned c = t | (1u << b);
            if (kept_count<NV>(key, c) >= top_k) t = c;
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
        const unsigned km = row_key_max<NV>(key);
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

// step 1 alone -- s and key of the row, what a backward pass recomputes before it applies its forward pass's threshold: the filter with
// neither top-k nor top-p
template <int NV, typename ROW>
__device__ __forceinline__ void row_keys(ROW row, int lane, int K, float inv_t, float (&s)[NV], unsigned (&key)[NV]) {
    sample_filter<NV, false, false>(row, lane, K, inv_t, 0, 1.f, s, key);
}

// ---- sums
// The whole row at temperature 1: mx = max_j z_j (a NaN is skipped there and caught by the sum), w_j = exp(z_j - mx), zs = sum_j w_j and,
// ENT, ts = sum_j w_j (z_j - mx) for the entropy (a zero weight adds nothing: never 0 * inf).  row(c) gives chunk c padded with -inf.
// mage_token_logprob, its backward pass and mage_token_stats' `entropy` are this one function.
struct RowLse { float mx, zs, ts; };
template <int NV, bool ENT = false, typename ROW>
__device__ __forceinline__ RowLse row_logsumexp(ROW row, float (&w)[NV]) {
    RowLse r{-INFINITY, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const f32x4 v = row(c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[c * 4 + e] = v[e];
            r.mx = fmaxf(r.mx, v[e]);
        }
    }
    r.mx = wave_max(r.mx);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const float d = w[e] - r.mx;
        w[e] = expf(d);
        r.zs = __fadd_rn(r.zs, w[e]);
        if constexpr (ENT) r.ts = w[e] == 0.f ? r.ts : __fmaf_rn(w[e], d, r.ts);
    }
    r.zs = wave_sum(r.zs);
    if constexpr (ENT) r.ts = wave_sum(r.ts);
    return r;
}
// The kept set: w_j = exp(s_j - smax) for key_j >= lo (0 outside), zs = sum w_j, ts = sum w_j (s_j - smax).  With temperature 1 and no
// filter this is row_logsumexp's sum operation for operation (s = z, smax = mx, every key of a NaN-free row >= lo = 1).
template <int NV>
__device__ __forceinline__ void kept_sums(const float (&s)[NV], const unsigned (&key)[NV], unsigned lo, float smax, float (&w)[NV], float& zs,
                                          float& ts, bool want_ts = true) {
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
    if (want_ts) ts = wave_sum(ts);                     // (wave-uniform; without it ts is one lane's part: not a result)
}
// the same sums for a caller that has no use for the weights (mage_token_stats; want_ts: whether the entropy is asked for)
template <int NV>
__device__ __forceinline__ void kept_sums(const float (&s)[NV], const unsigned (&key)[NV], unsigned lo, float smax, float& zs, float& ts,
                                          bool want_ts) {
    float w[NV];
    kept_sums<NV>(s, key, lo, smax, w, zs, ts, want_ts);
}
// The policy's log-probability of the token (zt = its logit, st = zt * inv_t: the sampler's multiply) and its entropy over the kept set of
// n codes:   lp = st - (smax + log Z) for a token in N, -inf outside it;   H = log Z - ts / Z (nats; exactly 0 when n = 1);   n = 0: both NaN.
// smax = +-inf (a +inf logit, a row of -inf only) gives NaN through inf - inf.  A backward pass, which has no count, passes n = 1: a row
// with n = 0 has no key >= lo, so its token is outside and its gradient is zero whatever lp and H are.
// lp rounds zt * inv_t - (smax + log Z) ONCE: the compiler has contracted the multiply into the difference in every kernel since these
// heads exist, so those are the bits the entry points return; the explicit fma pins them (the rounded product st decides membership).
struct RowScore { float lp, H; };
__device__ __forceinline__ RowScore row_score(int n, float zt, float inv_t, unsigned lo, float smax, float zs, float ts) {
    const float lz = logf(zs), st = __fmul_rn(zt, inv_t);
    const float lp = __fmaf_rn(zt, inv_t, -(smax + lz));
    return RowScore{!n ? __builtin_nanf("") : sample_key(st) >= lo ? lp : -INFINITY, n ? lz - ts / zs : __builtin_nanf("")};
}

// ---- host side
// the instance for K: NV = 4 .. 64 values per lane
#define MAGE_ROW_LADDER(K, CALL)        \
    do {                                \
        if ((K) <= 256) CALL(4);        \
        else if ((K) <= 512) CALL(8);   \
        else if ((K) <= 1024) CALL(16); \
        else if ((K) <= 2048) CALL(32); \
        else CALL(64);                  \
    } while (0)

// The size and alignment rule of every entry point that reads rows in this layout.  `more`: the caller's own conditions on the arguments the
// message does not name (group, strides, offsets, a second pointer's alignment); div_name / div: the divisor the message does name, if any.
static inline int token_rows_check(const char* who, const void* logits, int64_t rows, int32_t K, int64_t ld, bool more,
                                   const char* div_name = nullptr, int64_t div = 1) {
    if (rows > 0 && K > 0 && K % 4 == 0 && K <= MAGE_SAMPLE_MAX_K && ld % 4 == 0 && ld >= K && div > 0 && more && (((uintptr_t)logits) & 15) == 0)
        return MAGE_OK;
    if (div_name)
        mage_set_error("%s: bad sizes rows=%ld K=%d ld=%ld %s=%ld (K %% 4 == 0, K <= %d, 16-byte aligned rows)", who, (long)rows, K, (long)ld,
                       div_name, (long)div, MAGE_SAMPLE_MAX_K);
    else
        mage_set_error("%s: bad sizes rows=%ld K=%d ld=%ld (K %% 4 == 0, K <= %d, 16-byte aligned rows)", who, (long)rows, K, (long)ld,
                       MAGE_SAMPLE_MAX_K);
    return MAGE_EINVAL;
}
