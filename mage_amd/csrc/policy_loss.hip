// Policy-gradient loss over given tokens (mage_policy_loss / mage_policy_loss_bwd and their anchored and masked forms; include/mage_hip_ext.h
// states the rule).  The policy is the sampler's: s, N of steps 1-3 of the sampling rule by sample_filter itself, logprob and entropy by the
// functions mage_token_stats calls (token_row.h), so on the same inputs they carry its bits.  One wave per row, the row read once into
// registers, one instance per filter combination; the forward kernel leaves the filter's threshold in cut[i] and the backward kernel keeps j
// iff sample_key(s_j) >= cut[i]: no second bisection, and the same set bit for bit.
#include "token_row.h"

namespace {

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

// mage_policy_loss_grouped: policy_term's clipped rule with the group's rho_g = expf(m_g) in place of the row's own expf(lp - b).  The same
// operations in the same order, so a group of one row (m_g = lp - b) carries policy_term's bits.  Stated beside policy_term and not inside
// it: the instances of the existing entry points keep their code.
__device__ __forceinline__ PolicyTerm policy_term_group(float lp, float H, float A, float rho, float cmin, float cmax, float ent_coef) {
    PolicyTerm t{0.f, 0.f, lp == -INFINITY, false, 0.0};
    if (t.outside) return t;
    const bool active = (A >= 0.f && rho <= cmax) || (A < 0.f && rho >= cmin);
    const double u = (double)rho * (double)A, c = (double)fminf(fmaxf(rho, cmin), cmax) * (double)A;
    const double surr = u < c ? u : (c < u ? c : (u != u ? u : c));     // min; a NaN stays a NaN
    t.g = active ? -(A * rho) : 0.f;
    t.off = !active;
    t.sum = -surr - (double)ent_coef * (double)H;
    t.loss = (float)t.sum;
    return t;
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
    if (row_given(given, i)) {                          // (wave-uniform) mage_policy_loss_masked: nothing of the row is read
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
    const unsigned km = row_key_max<NV>(key);
    const int n = kept_count<NV>(key, lo);
    const float smax = sample_key_value(km);
    float zs, ts;
    kept_sums<NV>(s, key, lo, smax, w, zs, ts);
    if (lane == 0) {
        const auto [lp, H] = row_score(n, p[row_token(tokens, i, K, err)], inv_t, lo, smax, zs, ts);
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

// mage_policy_loss_grouped, between the row kernel and the summary: group g owns rows [g * ratio_div, (g + 1) * ratio_div).  Its T threads
// (T = 64: one wave per group, four groups per workgroup; T = 1024: one workgroup of sixteen waves per group) add d_i = logprob_i - b_i
// (one fp32 subtraction) of the counted rows (free, logprob != -inf) in fp64 -- a thread its rows in ascending order, the lanes in the
// xor butterfly, the waves in order -- and count them; m_g = (float)(sum / n_g), +0 for n_g = 0.  Every thread then holds
// rho_g = expf(m_g) and rewrites row_loss of its counted rows (the row kernel left the token rule's value there); a given row and an
// outside row keep the row kernel's +0.  A clip of 3840 rows on 256 threads measured 31 us over its price (15 dependent rows per thread,
// twice, with the anchor's fp64 expm1): hence 1024.
template <int T>
__global__ __launch_bounds__(T == 64 ? 256 : T) void policy_group_kernel(
    const float* __restrict__ logprob, const float* __restrict__ entropy, const float* __restrict__ blp, const uint8_t* __restrict__ given,
    const float* __restrict__ adv, long adv_div, const float* __restrict__ ref, float kl_coef, float cmin, float cmax, float ent_coef,
    long groups, long ratio_div, float* __restrict__ glr, int* __restrict__ gcount, float* __restrict__ row_loss) {
    const long g = T == 64 ? (long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long)blockIdx.x;
    const int t = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    if (g >= groups) return;                            // (T = 64 only, wave-uniform: that form has no barrier)
    const long r0 = g * ratio_div;
    double sum = 0.0;
    int n = 0;
    for (long j = t; j < ratio_div; j += T) {
        const long i = r0 + j;
        if (given && given[i]) continue;
        const float lp = logprob[i];
        if (lp == -INFINITY) continue;
        sum += (double)(lp - blp[i]);
        ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        n += __shfl_xor(n, o, 64);
    }
    if constexpr (T != 64) {
        __shared__ double red[T / 64];
        __shared__ int redn[T / 64];
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6] = sum;
            redn[threadIdx.x >> 6] = n;
        }
        __syncthreads();
        sum = red[0];
        n = redn[0];
#pragma unroll
        for (int w = 1; w < T / 64; ++w) {
            sum += red[w];
            n += redn[w];
        }
    }
    const float m = n ? (float)(sum / (double)n) : 0.f;
    if (t == 0) {
        glr[g] = m;
        gcount[g] = n;
    }
    const float rho = expf(m), A = adv[r0 / adv_div];
    for (long j = t; j < ratio_div; j += T) {
        const long i = r0 + j;
        if (given && given[i]) continue;
        const float lp = logprob[i];
        if (lp == -INFINITY) continue;
        PolicyTerm tm = policy_term_group(lp, entropy[i], A, rho, cmin, cmax, ent_coef);
        if (ref) tm = policy_term_anchored(tm, policy_anchor(lp, ref[i]), kl_coef);
        row_loss[i] = tm.loss;
    }
}

// summary, stage 1 of 2: workgroup b owns rows [b * chunk, (b + 1) * chunk) and leaves W fp64 sums in part[b * W ..]: the loss terms, the
// entropies, b - logprob, the rows whose gradient the clip switched off, the outside rows (an outside row counts in the last one only) and,
// for the anchored call (W = 7), the KL estimates and the unanchored rows (a reference log-probability that is not finite).
// A thread adds its rows in ascending order, the lanes meet in an xor butterfly, thread 0 adds the four waves in order: a fixed order.
// The masked call (W = 8) adds the free rows only, in the same order, and counts the given ones in an eighth sum; its kl and ref may be null
// (the plain rule: sums 5 and 6 stay 0).
enum { POLICY_PARTS = 256, POLICY_MEANS = 7, POLICY_MASKED = 8, POLICY_GROUP_WAVE = 1024 };   // GROUP_WAVE: the largest group one wave takes
__device__ double g_policy_part[POLICY_PARTS * POLICY_MASKED];     // stage 1 -> stage 2, within one mage_policy_loss* call (stream order)
// The grouped call (GRP, W = 8): given may be null, and a row's gradient is switched off by its group's rho_g = expf(glr[i / ratio_div]).
template <int W, bool GRP = false>
__global__ __launch_bounds__(256) void policy_part_kernel(const float* __restrict__ row_loss, const float* __restrict__ logprob,
                                                          const float* __restrict__ entropy, const float* __restrict__ adv, long adv_div,
                                                          const float* __restrict__ blp, float cmin, float cmax, long rows, long chunk,
                                                          const float* __restrict__ kl, const float* __restrict__ ref,
                                                          const uint8_t* __restrict__ given, const float* __restrict__ glr = nullptr,
                                                          long ratio_div = 1) {
    __shared__ double red[4][W];
    const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    double a[W] = {};
    for (long i = r0 + threadIdx.x; i < r1; i += 256) {
        if constexpr (W == POLICY_MASKED) {
            if (GRP ? given && given[i] : given[i]) {
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
            if constexpr (GRP) a[3] += policy_term_group(lp, 0.f, adv[i / adv_div], expf(glr[i / ratio_div]), cmin, cmax, 0.f).off ? 1.0 : 0.0;
            else a[3] += policy_term(lp, 0.f, adv[i / adv_div], true, b, cmin, cmax, 0.f).off ? 1.0 : 0.0;
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
// recomputed with the forward kernel's operations (row_keys, kept_sums, row_score), so g_i is decided by the forward pass's rho.
// GRP (mage_policy_loss_grouped_bwd): one more wave-uniform load, the group's m_g, and rho_g = expf(m_g) in place of the row's own ratio.
template <int NV, typename OT, bool ANCH, bool GRP = false>
__global__ __launch_bounds__(256) void policy_loss_bwd_kernel(const float* __restrict__ logits, long rows, int K, long ld,
                                                              const int64_t* __restrict__ tokens, const float* __restrict__ adv, long adv_div,
                                                              const float* __restrict__ blp, const unsigned* __restrict__ cut, float inv_t,
                                                              float cmin, float cmax, float ent_coef, const float* __restrict__ gout,
                                                              float inv_rows, OT* __restrict__ dl, const float* __restrict__ ref,
                                                              float kl_coef, const uint8_t* __restrict__ given,
                                                              const float* __restrict__ norm, const float* __restrict__ glr = nullptr,
                                                              long ratio_div = 1) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + i * ld;
    OT* o = dl + i * (long)K;
    if (row_given(given, i)) {                                          // (wave-uniform) a zero row by the free rows' stores, nothing read
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
    row_keys<NV>([=](int c) { return sample_row_chunk(p, lane, K, c); }, lane, K, inv_t, s, key);
    const float smax = sample_key_value(row_key_max<NV>(key));
    float zs, ts;
    kept_sums<NV>(s, key, lo, smax, w, zs, ts);
    const long tg = row_token(tokens, i, K, nullptr);                   // (clamped alike; the report is the forward pass's)
    // n = 1: no count here.  lp = -inf (t.outside below) for a token outside N, a row without a selectable code (st is NaN, key 0) included
    const auto [lp, H] = row_score(1, p[tg], inv_t, lo, smax, zs, ts);
    PolicyTerm t;
    if constexpr (GRP) t = policy_term_group(lp, H, adv[i / adv_div], expf(glr[i / ratio_div]), cmin, cmax, ent_coef);
    else t = policy_term(lp, H, adv[i / adv_div], blp != nullptr, blp ? blp[i] : 0.f, cmin, cmax, ent_coef);
    if constexpr (ANCH) {
        if (!t.outside) t = policy_term_anchored(t, policy_anchor(lp, ref[i]), kl_coef);        // (the guard spares an outside row its fp64 expm1)
    }
    // 1 - p_t = (Z - w_t) / Z from the sum of the OTHER kept terms (same fixed order): no cancellation where the token holds nearly all the mass
    float zo = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) zo = __fadd_rn(zo, (e >> 2) * 256 + lane * 4 + (e & 3) == tg ? 0.f : w[e]);
    zo = wave_sum(zo);
    const float scale = gout[0] * inv_rows * inv_t, inv_z = 1.0f / zs;
    const float hx = ts / zs;                                           // log p_j + H = (s_j - smax) - hx: log Z drops out
    const bool zero = t.outside;                                        // an outside row (a kept token of logit -inf too)
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

}  // namespace

// the argument rules mage_policy_loss and mage_policy_loss_bwd share (mage_token_stats' sizes and temperature, the clip and the entropy weight)
static int policy_check(const char* who, const void* logits, int64_t rows, int32_t K, int64_t ld, int64_t adv_div, float temperature,
                        float inv_t, float clip_lo, float clip_hi, float entropy_coef) {
    if (int rc = token_rows_check(who, logits, rows, K, ld, true, "adv_div", adv_div)) return rc;
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
// given non-null: mage_policy_loss_masked in either form (the masked reduction, norm written); ratio_div > 0: mage_policy_loss_grouped (the
// group kernel between the row kernel and the masked reduction, given or not)
template <bool ANCH>
static int policy_forward(const char* who, const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                          int64_t adv_div, const float* behaviour_logprob, float temperature, int32_t top_k, float top_p, float clip_lo,
                          float clip_hi, float entropy_coef, float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* summary,
                          const float* reference_logprob, float kl_coef, float* kl, void* stream, const uint8_t* given = nullptr,
                          float* norm = nullptr, int64_t ratio_div = 0, float* group_logratio = nullptr, int32_t* group_count = nullptr) {
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
    MAGE_ROW_LADDER(K, MAGE_POLICY_NV);
#undef MAGE_POLICY_NV
    constexpr int W = ANCH ? POLICY_MEANS : 5;
    const long chunk = (long)((rows + POLICY_PARTS - 1) / POLICY_PARTS);
    if (ratio_div > 0) {
        const long groups = (long)(rows / ratio_div);
        const float* ref = ANCH ? reference_logprob : nullptr;
#define MAGE_POLICY_GROUP(T, GRID)                                                                                                   \
    hipLaunchKernelGGL(policy_group_kernel<T>, dim3((unsigned)(GRID)), dim3(T == 64 ? 256 : T), 0, s, logprob, entropy, behaviour_logprob, \
                       given, advantage, (long)adv_div, ref, kl_coef, cmin, cmax, entropy_coef, groups, (long)ratio_div, group_logratio,    \
                       group_count, row_loss)
        if (ratio_div <= POLICY_GROUP_WAVE) MAGE_POLICY_GROUP(64, (groups + 3) / 4);
        else MAGE_POLICY_GROUP(1024, groups);
#undef MAGE_POLICY_GROUP
        hipLaunchKernelGGL((policy_part_kernel<POLICY_MASKED, true>), dim3(POLICY_PARTS), dim3(256), 0, s, row_loss, logprob, entropy, advantage,
                           (long)adv_div, behaviour_logprob, cmin, cmax, (long)rows, chunk, kl, reference_logprob, given, group_logratio,
                           (long)ratio_div);
        hipLaunchKernelGGL(policy_summary_masked_kernel, dim3(1), dim3(POLICY_PARTS), 0, s, summary, norm, (long)rows);
    } else if (given) {
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
                           const float* norm = nullptr, int64_t ratio_div = 0, const float* group_logratio = nullptr) {
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
#define MAGE_POLICY_BWD(NV, OT, GRP)                                                                                                          \
    hipLaunchKernelGGL((policy_loss_bwd_kernel<NV, OT, ANCH, GRP>), grid, dim3(256), 0, s, logits, (long)rows, K, (long)ld, tokens, advantage, \
                       (long)adv_div, behaviour_logprob, cut, inv_t, cmin, cmax, entropy_coef, grad_out, 1.0f / (float)rows, (OT*)dlogits,    \
                       reference_logprob, kl_coef, given, norm, group_logratio, (long)ratio_div)
#define MAGE_POLICY_BWD_NV(NV)                                                      \
    do {                                                                            \
        if (ratio_div > 0) {                                                        \
            if (dl_dtype == MAGE_F32) MAGE_POLICY_BWD(NV, float, true);             \
            else MAGE_POLICY_BWD(NV, unsigned short, true);                         \
        } else if (dl_dtype == MAGE_F32) MAGE_POLICY_BWD(NV, float, false);         \
        else MAGE_POLICY_BWD(NV, unsigned short, false);                            \
    } while (0)
    MAGE_ROW_LADDER(K, MAGE_POLICY_BWD_NV);
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

// what the grouped pair asks beyond the masked pair's rules (given may be null here): a behaviour policy to form the ratio against, groups
// that tile the rows and lie inside one advantage each, and somewhere to leave m_g
static int policy_grouped_check(const char* who, const float* behaviour_logprob, int64_t rows, int64_t adv_div, int64_t ratio_div,
                                const float* group_logratio, const int32_t* group_count, bool want_count, const float* norm, bool has_ref,
                                bool has_kl, float kl_coef) {
    MAGE_CHECK_ARG(behaviour_logprob != nullptr, "%s: behaviour_logprob must not be null (there is no ratio to group)", who);
    MAGE_CHECK_ARG(ratio_div >= 1 && ratio_div <= 0x7fffffff, "%s: ratio_div=%ld must be in [1, 2^31)", who, (long)ratio_div);
    MAGE_CHECK_ARG(rows > 0 && rows % ratio_div == 0, "%s: rows=%ld is not a multiple of ratio_div=%ld", who, (long)rows, (long)ratio_div);
    MAGE_CHECK_ARG(adv_div > 0 && adv_div % ratio_div == 0, "%s: adv_div=%ld is not a multiple of ratio_div=%ld (a group has one advantage)", who,
                   (long)adv_div, (long)ratio_div);
    MAGE_CHECK_ARG(group_logratio && (((uintptr_t)group_logratio) & 3) == 0, "%s: group_logratio must be a 4-byte aligned pointer", who);
    MAGE_CHECK_ARG(!want_count || (group_count && (((uintptr_t)group_count) & 3) == 0), "%s: group_count must be a 4-byte aligned pointer", who);
    MAGE_CHECK_ARG(norm && (((uintptr_t)norm) & 3) == 0, "%s: norm must be a 4-byte aligned pointer", who);
    MAGE_CHECK_ARG(has_ref == has_kl, "%s: reference_logprob and kl are given together (the anchored rule) or both null (the plain rule)", who);
    MAGE_CHECK_ARG(has_ref || kl_coef == 0.f, "%s: kl_coef=%g needs reference_logprob", who, (double)kl_coef);
    return MAGE_OK;
}

extern "C" int mage_policy_loss_grouped(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                        int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                                        int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef,
                                        float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary, float* norm,
                                        const uint8_t* given, int64_t ratio_div, float* group_logratio, int32_t* group_count, void* stream) {
    const char* who = "mage_policy_loss_grouped";
    if (int rc = policy_grouped_check(who, behaviour_logprob, rows, adv_div, ratio_div, group_logratio, group_count, true, norm,
                                      reference_logprob != nullptr, kl != nullptr, kl_coef))
        return rc;
    if (reference_logprob)
        return policy_forward<true>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, top_k, top_p, clip_lo,
                                    clip_hi, entropy_coef, row_loss, logprob, entropy, cut, summary, reference_logprob, kl_coef, kl, stream, given,
                                    norm, ratio_div, group_logratio, group_count);
    return policy_forward<false>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, top_k, top_p, clip_lo,
                                 clip_hi, entropy_coef, row_loss, logprob, entropy, cut, summary, nullptr, 0.f, nullptr, stream, given, norm,
                                 ratio_div, group_logratio, group_count);
}

extern "C" int mage_policy_loss_grouped_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                            const float* advantage, int64_t adv_div, const float* behaviour_logprob,
                                            const float* reference_logprob, const uint32_t* cut, float temperature, float clip_lo, float clip_hi,
                                            float entropy_coef, float kl_coef, const float* grad_out, const float* norm, void* dlogits,
                                            int32_t dl_dtype, const uint8_t* given, int64_t ratio_div, const float* group_logratio,
                                            void* stream) {
    const char* who = "mage_policy_loss_grouped_bwd";
    if (int rc = policy_grouped_check(who, behaviour_logprob, rows, adv_div, ratio_div, group_logratio, nullptr, false, norm,
                                      reference_logprob != nullptr, reference_logprob != nullptr, kl_coef))
        return rc;
    if (reference_logprob)
        return policy_backward<true>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, cut, temperature, clip_lo, clip_hi,
                                     entropy_coef, grad_out, dlogits, dl_dtype, reference_logprob, kl_coef, stream, given, norm, ratio_div,
                                     group_logratio);
    return policy_backward<false>(who, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, cut, temperature, clip_lo, clip_hi,
                                  entropy_coef, grad_out, dlogits, dl_dtype, nullptr, 0.f, stream, given, norm, ratio_div, group_logratio);
}
