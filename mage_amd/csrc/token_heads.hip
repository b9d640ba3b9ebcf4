// The token heads over one row of logits per wave (token_row.h states the layout, the sampling rule and the shared sums): argmax, seeded
// sampling, log-probabilities, policy statistics, guidance, given tokens, per-clip scores and cross entropy.
#include "token_row.h"

namespace {

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group,
                                                     long in_stride, long in_off, int64_t* __restrict__ out,
                                                     long out_stride, long out_off, float* __restrict__ margin) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const RowIndex r = row_index(i, group);
    const float* p = row_logits(logits, r, in_stride, in_off, ld);
    Best b{INFINITY, 0x7fffffff, INFINITY};          // minimise the negated logit: first maximum wins
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 v = *(const f32x4*)(p + k);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) best_push(b, -v[e], k + e);
    }
    b = best_wave_reduce(b);
    if (lane == 0) {
        out[row_slot(r, out_stride, out_off)] = b.i0;
        if (margin) margin[i] = b.d1 - b.d0;
    }
}

// g = -log(-log(u))
__device__ __forceinline__ float sample_gumbel(unsigned long long ctr) {
    return -logf(sample_neglog_u(hash32(ctr) >> 8));
}

template <int NV, bool TOPK, bool TOPP>
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group,
                                                     long in_stride, long in_off, int64_t* __restrict__ out, long out_stride,
                                                     long out_off, const int64_t* __restrict__ seeds, long pos_off, float inv_t,
                                                     int top_k, float top_p) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const RowIndex r = row_index(i, group);
    const float* p = row_logits(logits, r, in_stride, in_off, ld);
    float s[NV];
    unsigned key[NV];
    const unsigned lo = sample_filter<NV, TOPK, TOPP>([=](int c) { return sample_row_chunk(p, lane, K, c); }, lane, K, inv_t, top_k, top_p,
                                                      s, key);                                    // the candidate set: key >= lo
    const unsigned long long ctr = (unsigned long long)seeds[r.gi] * 0x9e3779b97f4a7c15ULL
                                   + (unsigned long long)(pos_off + r.gr) * (unsigned long long)K;
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
    if (lane == 0) out[row_slot(r, out_stride, out_off)] = bj == 0x7fffffff ? 0 : bj;
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
// lp = z_t - (m + log sum_j exp(z_j - m)), m = max_j z_j: the log-softmax of a row gathered at its token: row_logsumexp (token_row.h).
// -inf logits add exp(-inf) = 0; a NaN logit, or a row whose maximum is not finite (inf - inf), makes the sum NaN and so the result;
// z_t = -inf gives -inf.  A token outside [0, K) is raised and clamped, as mage_cross_entropy's targets are.
template <int NV>
__global__ __launch_bounds__(256) void token_logprob_kernel(const float* __restrict__ logits, long rows, int K, long ld, long group,
                                                            long in_stride, long in_off, const int64_t* __restrict__ tokens,
                                                            float* __restrict__ logprob, long tok_stride, long tok_off,
                                                            int* __restrict__ err) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const RowIndex r = row_index(i, group);
    const float* p = row_logits(logits, r, in_stride, in_off, ld);
    float w[NV];
    const RowLse l = row_logsumexp<NV>([=](int c) { return row_chunk_inf(p, lane, K, c); }, w);
    if (lane == 0) {
        const long ti = row_slot(r, tok_stride, tok_off);
        logprob[ti] = p[row_token(tokens, ti, K, err)] - (l.mx + logf(l.zs));
    }
}

// ---- per-token statistics of the sampling policy (mage_token_stats, include/mage_hip_ext.h): what mage_sample_tokens' filter kept and how
// the kept set weighs the given token.  Per row, with s, A, N of steps 1-3 of the sampling rule (token_row.h; sample_filter: the sampler's own
// code, so N is the sampler's bit for bit), s_max = max_N s, w_j = exp(s_j - s_max), Z = sum_{j in N} w_j:
//   kept           = |N|                                                (a ballot count: exact)
//   policy_logprob = z_t * inv_t - (s_max + log Z) for t in N, -inf otherwise   (rounded once, an fma: row_score, token_row.h, says why;
//                    include/mage_hip_ext.h still words it as s_t - (...) with a rounded s_t: its wording needs a follow-up)
//   policy_entropy = log Z - (sum_{j in N} w_j (s_j - s_max)) / Z       (nats; exactly 0 when |N| = 1)
//   entropy        = the same formula over the whole row of z itself: temperature 1, no filter -- the distribution mage_token_logprob scores under
// top_k == 1 is greedy by definition, as in the sampler: N = { mage_argmax's first maximum of z }, kept = 1, policy_logprob = 0 for that code
// and -inf for any other, policy_entropy = 0.
// Special values: a NaN logit is in no set and adds nothing to Z (it makes `entropy` NaN, as it does mage_token_logprob's result); a -inf
// logit in N counts in `kept` and adds a zero term to both sums (never 0 * inf); a row with no selectable code (every logit NaN) gives
// kept = 0 and NaN for policy_logprob and policy_entropy; s_max = +-inf (a +inf logit, a row of -inf only) gives NaN through
// inf - inf, as in mage_token_logprob; a token outside [0, K) is raised (MAGE_DEVERR_TOKEN_ID) and clamped.
// The row is read once into registers whatever outputs are asked for (a null output costs a wave-uniform branch), one instance per filter
// combination.  The sums are kept_sums and row_logsumexp (token_row.h): with temperature 1 and no filter, policy_logprob equals
// mage_token_logprob's result bit for bit on NaN-free rows.
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
    const RowIndex r = row_index(i, group);
    const float* p = row_logits(logits, r, in_stride, in_off, ld);
    const long ti = row_slot(r, tok_stride, tok_off);
    f32x4 zc[NV / 4];
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) zc[c] = row_chunk_inf(p, lane, K, c);   // -inf past K: row_logsumexp's form; the filter's keys do not look there
    if (entropy) {                                      // the whole row at temperature 1: token_logprob_kernel's maximum and sum
        float w[NV];
        const RowLse l = row_logsumexp<NV, true>([&](int c) { return zc[c]; }, w);
        if (lane == 0) entropy[ti] = logf(l.zs) - l.ts / l.zs;
    }
    if (!policy_logprob && !policy_entropy && !kept) return;
    float s[NV];
    unsigned key[NV];
    const unsigned lo = sample_filter<NV, (MODE & STATS_TOPK) != 0, (MODE & STATS_TOPP) != 0>([&](int c) { return zc[c]; }, lane, K, inv_t, top_k,
                                                                                              top_p, s, key);
    const unsigned km = row_key_max<NV>(key);
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
                const long tg = row_token(tokens, ti, K, err);
                policy_logprob[ti] = !any ? __builtin_nanf("") : tg == bj ? 0.f : -INFINITY;
            }
        }
    } else {
        const int n = kept_count<NV>(key, lo);
        const float smax = sample_key_value(km);
        float zs = 0.f, ts = 0.f;
        if (policy_logprob || policy_entropy) kept_sums<NV>(s, key, lo, smax, zs, ts, policy_entropy != nullptr);
        if (lane == 0) {
            if (kept) kept[ti] = n;
            const float zt = policy_logprob ? p[row_token(tokens, ti, K, err)] : 0.f;
            const RowScore sc = row_score(n, zt, inv_t, lo, smax, zs, ts);
            if (policy_entropy) policy_entropy[ti] = sc.H;
            if (policy_logprob) policy_logprob[ti] = sc.lp;
        }
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

extern "C" int mage_argmax(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride,
                           int64_t in_off, int64_t* out, int64_t out_group_stride, int64_t out_off, float* margin,
                           void* stream) {
    MAGE_CHECK_ARG(logits && out, "mage_argmax: null pointer");
    MAGE_CHECK_ARG(rows > 0 && K > 0 && K % 4 == 0 && ld % 4 == 0 && group > 0, "mage_argmax: bad sizes rows=%ld K=%d", (long)rows, K);
    // the rows are read as 16-byte vectors, K values of each: no K <= MAGE_SAMPLE_MAX_K here (token_rows_check), the kernel sweeps any K
    MAGE_CHECK_ARG(ld >= K && (((uintptr_t)logits) & 15) == 0, "mage_argmax: K=%d ld=%ld logits=%p (ld >= K, logits 16-byte aligned)", K, (long)ld,
                   (const void*)logits);
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
    if (int rc = token_rows_check("mage_sample_tokens", logits, rows, K, ld, group > 0 && pos_off >= 0)) return rc;
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
#define MAGE_SAMPLE_NV(NV) \
    sample_launch<NV>(topk, topp, grid, s, logits, a[0], K, a[1], a[2], a[3], a[4], out, a[5], a[6], seeds, a[7], inv_t, top_k, top_p)
    MAGE_ROW_LADDER(K, MAGE_SAMPLE_NV);
#undef MAGE_SAMPLE_NV
    MAGE_CHECK_LAUNCH("mage_sample_tokens");
    return MAGE_OK;
}

extern "C" int mage_token_logprob(const float* logits, int64_t rows, int32_t K, int64_t ld, int64_t group, int64_t in_group_stride,
                                  int64_t in_off, const int64_t* tokens, float* logprob, int64_t tok_group_stride, int64_t tok_off,
                                  void* stream) {
    MAGE_CHECK_ARG(logits && tokens && logprob, "mage_token_logprob: null pointer");
    if (int rc = token_rows_check("mage_token_logprob", logits, rows, K, ld,
                                  group > 0 && in_group_stride >= 0 && in_off >= 0 && tok_group_stride >= 0 && tok_off >= 0))
        return rc;
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_token_logprob: mage_init() has not been called");
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_LOGPROB(NV)                                                                                                             \
    hipLaunchKernelGGL((token_logprob_kernel<NV>), grid, dim3(256), 0, s, logits, (long)rows, K, (long)ld, (long)group,              \
                       (long)in_group_stride, (long)in_off, tokens, logprob, (long)tok_group_stride, (long)tok_off, err)
    MAGE_ROW_LADDER(K, MAGE_LOGPROB);
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
    if (int rc = token_rows_check("mage_token_stats", logits, rows, K, ld,
                                  group > 0 && in_group_stride >= 0 && in_off >= 0 && tok_group_stride >= 0 && tok_off >= 0))
        return rc;
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
    MAGE_ROW_LADDER(K, MAGE_STATS_NV);
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
