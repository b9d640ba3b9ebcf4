// Policy-gradient loss over given tokens: the eight mage_policy_loss* entry points (include/mage_hip_ext.h states the rule).  The policy is
// the sampler's: s, N of steps 1-3 of the sampling rule by sample_filter itself, logprob and entropy by the functions mage_token_stats calls
// (token_row.h), so on the same inputs they carry its bits.  One wave per row, the row read once into registers, one instance per filter
// combination; the forward kernel leaves the filter's threshold in cut[i] and the backward kernel keeps j iff sample_key(s_j) >= cut[i]: no
// second bisection, and the same set bit for bit.
// A call is one PolicyCall.  Three things in it are optional, each a group of fields that is set together or not at all:
//   a reference (ref, kl_coef, kl)       the loss gains kl_coef times the k3 estimate of the KL against a reference policy;
//   a mask      (given, norm)            a given row is not read and gets zeros, the means are over the free rows, norm = 1 / their number;
//   a group     (ratio_div, glr, gcount) one importance ratio per ratio_div consecutive rows in place of a row's own.
// The entry points differ in which of the three they accept (PolicyForm); policy_call_check states every rule once, policy_forward and
// policy_backward decide the kernels' instances from the call.
#include "token_row.h"

namespace {

enum PolicyForm { FORM_PLAIN, FORM_ANCHORED, FORM_MASKED, FORM_GROUPED };     // the entry point pair: which options it accepts

// What a forward or a backward call is made of.  policy_group_kernel and policy_part_kernel take it by value (as gemm4.hip's Gemm4Args);
// the two row kernels take its fields one by one (see policy_loss_kernel).
struct PolicyCall {
    const float* logits;                // the row geometry
    long rows;
    int K;
    long ld;
    const int64_t* tokens;
    const float* adv;
    long adv_div;
    const float* blp;                   // null: the reward-weighted likelihood, no ratio
    const float* ref;                   // the reference: null without one
    float kl_coef;
    float* kl;
    const uint8_t* given;               // the mask: null without one
    float* norm;                        // written by the masked and grouped forward calls, read by their backward calls
    long ratio_div;                     // the group: rows per group, m_g and the counted rows per group
    float* glr;
    int* gcount;
    float inv_t;                        // the scalars, as the kernels use them (policy_call)
    int top_k;
    float top_p, cmin, cmax, ent_coef;
    float *row_loss, *logprob, *entropy;        // the forward call's outputs (cut: the backward call's input)
    unsigned* cut;
    float* summary;
    int* err;
    const float* gout;                  // the backward call's operands
    float inv_rows;
    void* dl;
    int form, dl_dtype;                 // read on the host only: the form, and the scalars as the caller gave them
    float temperature, clip_lo, clip_hi;
};

// One row's loss term and the factor g of its gradient from logprob lp, entropy H, advantage A and (clipped form) the importance ratio rho:
// the row's own expf(lp - b) against the behaviour log-probability b, or its group's expf(m_g).  rho is the one fp32 value both passes use
// to decide which branch of the surrogate is active; the products and the final sum are taken in fp64 and rounded once.  An outside row
// (lp = -inf: a token the filter cannot draw) gives 0, 0.  A group of one row has m_g = lp - b: the same rho, the same bits.
struct PolicyTerm { float loss, g; bool outside, off; double sum; };   // sum: the loss before its one rounding (the anchored form adds to it)
__device__ __forceinline__ PolicyTerm policy_term(float lp, float H, float A, bool clipped, float rho, float cmin, float cmax, float ent_coef) {
    PolicyTerm t{0.f, 0.f, lp == -INFINITY, false, 0.0};
    if (t.outside) return t;
    double surr;
    if (!clipped) {
        surr = (double)A * (double)lp;
        t.g = -A;
    } else {
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
// a row's own ratio against its behaviour log-probability b; the unclipped rule has none and evaluates no expf
__device__ __forceinline__ float policy_row_rho(bool clipped, float lp, float b) { return clipped ? expf(lp - b) : 0.f; }

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

// The two row kernels take their operands one by one, not as a PolicyCall: with the aggregate every instance measured slower than before
// (the forward calls by 1.5 - 3 us of 170 - 630, the NV = 64 backward by 8 us of 608; profiles/r21_policy_family.txt), the pointers losing
// their const __restrict__ and moving from scalar into vector registers.  POLICY_ROW_ARGS / POLICY_BWD_ARGS below are the one place that
// spells either list out of a call.
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
    if (row_given(given, i)) {                          // (wave-uniform) a given row: nothing of it is read
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
        const bool clipped = blp != nullptr;
        const float A = adv[i / adv_div], b = clipped ? blp[i] : 0.f;
        const PolicyTerm t = policy_term(lp, H, A, clipped, policy_row_rho(clipped, lp, b), cmin, cmax, ent_coef);
        if constexpr (ANCH) {
            const PolicyAnchor a = policy_anchor(lp, ref[i]);
            kl[i] = (float)a.kl;
            row_loss[i] = policy_term_anchored(t, a, kl_coef).loss;
        } else {
            row_loss[i] = t.loss;
        }
    }
}
#define POLICY_ROW_ARGS(c)                                                                                                                  \
    (c).logits, (c).rows, (c).K, (c).ld, (c).tokens, (c).adv, (c).adv_div, (c).blp, (c).inv_t, (c).top_k, (c).top_p, (c).cmin, (c).cmax,    \
        (c).ent_coef, (c).row_loss, (c).logprob, (c).entropy, (c).cut, (c).err, (c).ref, (c).kl_coef, (c).kl, (c).given

// The grouped call, between the row kernel and the summary: group g owns rows [g * ratio_div, (g + 1) * ratio_div).  Its T threads
// (T = 64: one wave per group, four groups per workgroup; T = 1024: one workgroup of sixteen waves per group) add d_i = logprob_i - b_i
// (one fp32 subtraction) of the counted rows (free, logprob != -inf) in fp64 -- a thread its rows in ascending order, the lanes in the
// xor butterfly, the waves in order -- and count them; m_g = (float)(sum / n_g), +0 for n_g = 0.  Every thread then holds
// rho_g = expf(m_g) and rewrites row_loss of its counted rows (the row kernel left the token rule's value there); a given row and an
// outside row keep the row kernel's +0.  A clip of 3840 rows on 256 threads measured 31 us over its price (15 dependent rows per thread,
// twice, with the anchor's fp64 expm1): hence 1024.
template <int T>
__global__ __launch_bounds__(T == 64 ? 256 : T) void policy_group_kernel(const PolicyCall c) {
    const long g = T == 64 ? (long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long)blockIdx.x;
    const int t = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const long r0 = g * c.ratio_div;
    if (r0 >= c.rows) return;                           // (T = 64 only, wave-uniform: that form has no barrier)
    double sum = 0.0;
    int n = 0;
    for (long j = t; j < c.ratio_div; j += T) {
        const long i = r0 + j;
        if (c.given && c.given[i]) continue;
        const float lp = c.logprob[i];
        if (lp == -INFINITY) continue;
        sum += (double)(lp - c.blp[i]);
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
        c.glr[g] = m;
        c.gcount[g] = n;
    }
    const float rho = expf(m), A = c.adv[r0 / c.adv_div];
    for (long j = t; j < c.ratio_div; j += T) {
        const long i = r0 + j;
        if (c.given && c.given[i]) continue;
        const float lp = c.logprob[i];
        if (lp == -INFINITY) continue;
        PolicyTerm tm = policy_term(lp, c.entropy[i], A, true, rho, c.cmin, c.cmax, c.ent_coef);
        if (c.ref) tm = policy_term_anchored(tm, policy_anchor(lp, c.ref[i]), c.kl_coef);
        c.row_loss[i] = tm.loss;
    }
}

// summary, stage 1 of 2: workgroup b owns rows [b * chunk, (b + 1) * chunk) and leaves W fp64 sums in part[b * W ..]: the loss terms, the
// entropies, b - logprob, the rows whose gradient the clip switched off, the outside rows (an outside row counts in the last one only) and,
// with a reference (W >= 7), the KL estimates and the unanchored rows (a reference log-probability that is not finite).
// A thread adds its rows in ascending order, the lanes meet in an xor butterfly, thread 0 adds the four waves in order: a fixed order.
// With a mask or a group (W = 8) the free rows only are added, in the same order, and the given ones counted in an eighth sum; the mask and
// the reference may each be null (no reference: sums 5 and 6 stay 0).  GRP: a row's gradient is switched off by its group's
// rho_g = expf(glr[i / ratio_div]).
enum { POLICY_PARTS = 256, POLICY_MEANS = 7, POLICY_MASKED = 8, POLICY_GROUP_WAVE = 1024 };   // GROUP_WAVE: the largest group one wave takes
__device__ double g_policy_part[POLICY_PARTS * POLICY_MASKED];     // stage 1 -> stage 2, within one mage_policy_loss* call (stream order)
template <int W, bool GRP = false>
__global__ __launch_bounds__(256) void policy_part_kernel(const PolicyCall c, long chunk) {
    __shared__ double red[4][W];
    const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < c.rows ? r0 + chunk : c.rows;
    double a[W] = {};
    for (long i = r0 + threadIdx.x; i < r1; i += 256) {
        if constexpr (W == POLICY_MASKED) {
            if (c.given && c.given[i]) {
                a[7] += 1.0;
                continue;
            }
        }
        const float lp = c.logprob[i];
        if (lp == -INFINITY) {
            a[4] += 1.0;
            continue;
        }
        a[0] += (double)c.row_loss[i];
        a[1] += (double)c.entropy[i];
        if (c.blp) {
            const float b = c.blp[i], rho = GRP ? expf(c.glr[i / c.ratio_div]) : expf(lp - b);
            a[2] += (double)b - (double)lp;
            a[3] += policy_term(lp, 0.f, c.adv[i / c.adv_div], true, rho, c.cmin, c.cmax, 0.f).off ? 1.0 : 0.0;
        }
        if constexpr (W >= POLICY_MEANS) {
            if (W == POLICY_MEANS || c.ref) {
                a[5] += (double)c.kl[i];
                a[6] += __builtin_isfinite(c.ref[i]) ? 0.0 : 1.0;
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

// stage 2: thread t holds workgroup t's sums; the same butterfly and wave order, one multiply by 1 / n, one rounding to fp32.  n = rows; at
// W = 8 the eighth sum is the number of given rows (exact in fp64) and n = n_free = rows - given: the means are over the free rows (0 when
// everything is given), summary[7] is the given share, and norm[0] = 1.0f / (float)n_free is left for the backward call: the value the
// unmasked one forms on the host for its `rows`.
template <int W>
__global__ __launch_bounds__(256) void policy_summary_kernel(float* __restrict__ summary, float* __restrict__ norm, long rows) {
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
        const auto total = [&](int k) { return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]; };
        const double ng = W == POLICY_MASKED ? total(POLICY_MASKED - 1) : 0.0;
        const long n = rows - (long)ng;
        if (q < POLICY_MEANS) {
            summary[q] = (float)(total(q) * (n > 0 ? 1.0 / (double)n : 0.0));
        } else {
            summary[7] = (float)(ng / (double)rows);
            norm[0] = n > 0 ? __fdiv_rn(1.0f, (float)n) : 0.f;
        }
    }
}

// dlogits_ij = scale * [ g_i (1[j = t] - p_j) + ent_coef p_j (log p_j + H_i) ] for j in N, 0 outside N and in outside rows; scale =
// grad_out[0] / rows * inv_t, p_j = w_j / Z, log p_j + H_i = (s_j - smax) - (sum_N w (s - smax)) / Z; a p_j = 0 term is 0.  Z, H, logprob are
// recomputed with the forward kernel's operations (row_keys, kept_sums, row_score), so g_i is decided by the forward pass's rho.
// A mask: a given row is a zero row, and 1 / rows is the forward call's norm[0].  GRP: one more wave-uniform load, the group's m_g, and
// rho_g = expf(m_g) in place of the row's own ratio.
template <int NV, typename OT, bool ANCH, bool GRP>
__global__ __launch_bounds__(256) void policy_loss_bwd_kernel(const float* __restrict__ logits, long rows, int K, long ld,
                                                              const int64_t* __restrict__ tokens, const float* __restrict__ adv, long adv_div,
                                                              const float* __restrict__ blp, const unsigned* __restrict__ cut, float inv_t,
                                                              float cmin, float cmax, float ent_coef, const float* __restrict__ gout,
                                                              float inv_rows, OT* __restrict__ dl, const float* __restrict__ ref,
                                                              float kl_coef, const uint8_t* __restrict__ given,
                                                              const float* __restrict__ norm, const float* __restrict__ glr, long ratio_div) {
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
    if (norm) inv_rows = norm[0];                                       // a mask or a group: 1 / n_free, left by the forward call
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
    const bool clipped = GRP || blp != nullptr;
    const float A = adv[i / adv_div], b = GRP ? glr[i / ratio_div] : clipped ? blp[i] : 0.f;      // (GRP: b is the group's m_g)
    PolicyTerm t = policy_term(lp, H, A, clipped, GRP ? expf(b) : policy_row_rho(clipped, lp, b), cmin, cmax, ent_coef);
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
#define POLICY_BWD_ARGS(c, OT)                                                                                                            \
    (c).logits, (c).rows, (c).K, (c).ld, (c).tokens, (c).adv, (c).adv_div, (c).blp, (c).cut, (c).inv_t, (c).cmin, (c).cmax, (c).ent_coef, \
        (c).gout, (c).inv_rows, (OT*)(c).dl, (c).ref, (c).kl_coef, (c).given, (c).norm, (c).glr, (c).ratio_div

}  // namespace

// The argument rules of the eight entry points, each stated once, in the order a call meets them: the group's, the mask's, what the masked
// and grouped forms share, then what every form asks (mage_token_stats' sizes and temperature, the clip, the entropy weight), the forward
// call's filter or the backward call's dlogits, and the reference's.  A masked or grouped call is anchored iff it has a reference.
static int policy_call_check(const char* who, const PolicyCall& c, bool fwd) {
    const bool has_ref = c.ref != nullptr, anch = c.form == FORM_ANCHORED || has_ref;
    if (c.form == FORM_GROUPED) {     // a behaviour policy to form the ratio against, groups that tile the rows inside one advantage each
        MAGE_CHECK_ARG(c.blp != nullptr, "%s: behaviour_logprob must not be null (there is no ratio to group)", who);
        MAGE_CHECK_ARG(c.ratio_div >= 1 && c.ratio_div <= 0x7fffffff, "%s: ratio_div=%ld must be in [1, 2^31)", who, c.ratio_div);
        MAGE_CHECK_ARG(c.rows > 0 && c.rows % c.ratio_div == 0, "%s: rows=%ld is not a multiple of ratio_div=%ld", who, c.rows, c.ratio_div);
        MAGE_CHECK_ARG(c.adv_div > 0 && c.adv_div % c.ratio_div == 0, "%s: adv_div=%ld is not a multiple of ratio_div=%ld (a group has one advantage)",
                       who, c.adv_div, c.ratio_div);
        MAGE_CHECK_ARG(c.glr && (((uintptr_t)c.glr) & 3) == 0, "%s: group_logratio must be a 4-byte aligned pointer", who);
        MAGE_CHECK_ARG(!fwd || (c.gcount && (((uintptr_t)c.gcount) & 3) == 0), "%s: group_count must be a 4-byte aligned pointer", who);
    }
    if (c.form == FORM_MASKED)
        MAGE_CHECK_ARG(c.given != nullptr, "%s: given must not be null (the unmasked entry points take no mask)", who);
    if (c.form == FORM_MASKED || c.form == FORM_GROUPED) {
        MAGE_CHECK_ARG(c.norm && (((uintptr_t)c.norm) & 3) == 0, "%s: norm must be a 4-byte aligned pointer", who);
        MAGE_CHECK_ARG(!fwd || has_ref == (c.kl != nullptr),
                       "%s: reference_logprob and kl are given together (the anchored rule) or both null (the plain rule)", who);
        MAGE_CHECK_ARG(has_ref || c.kl_coef == 0.f, "%s: kl_coef=%g needs reference_logprob", who, (double)c.kl_coef);
    }
    if (fwd) MAGE_CHECK_ARG(c.logits && c.tokens && c.adv && c.row_loss && c.logprob && c.entropy && c.cut && c.summary, "%s: null pointer", who);
    else MAGE_CHECK_ARG(c.logits && c.tokens && c.adv && c.cut && c.gout && c.dl, "%s: null pointer", who);
    if (int rc = token_rows_check(who, c.logits, c.rows, c.K, c.ld, true, "adv_div", c.adv_div)) return rc;
    MAGE_CHECK_ARG(__builtin_isfinite(c.temperature) && c.temperature > 0.f && __builtin_isfinite(c.inv_t),
                   "%s: temperature=%g must be finite and > 0", who, (double)c.temperature);
    MAGE_CHECK_ARG(c.clip_lo >= 0.f && c.clip_lo <= 1.f && c.clip_hi >= 0.f, "%s: clip_lo=%g outside [0, 1] or clip_hi=%g < 0", who,
                   (double)c.clip_lo, (double)c.clip_hi);
    MAGE_CHECK_ARG(__builtin_isfinite(c.ent_coef), "%s: entropy_coef=%g must be finite", who, (double)c.ent_coef);
    if (fwd) {
        MAGE_CHECK_ARG(c.top_k >= 0 && c.top_k <= c.K, "%s: top_k=%d outside [0, K=%d]", who, c.top_k, c.K);
        MAGE_CHECK_ARG(c.top_k != 1, "%s: top_k=1 is greedy decoding: its log-probability is 0 and has no gradient", who);
        MAGE_CHECK_ARG(c.top_p > 0.f && c.top_p <= 1.f, "%s: top_p=%g outside (0, 1]", who, (double)c.top_p);
    } else {
        MAGE_CHECK_ARG((c.dl_dtype == MAGE_F32 || c.dl_dtype == MAGE_BF16) && (((uintptr_t)c.dl) & 15) == 0,
                       "%s: dlogits must be 16-byte aligned fp32 or bf16 (dtype %d)", who, c.dl_dtype);
    }
    if (anch) {                         // a reference log-probability per row and a weight that is a number
        MAGE_CHECK_ARG(has_ref && (((uintptr_t)c.ref) & 3) == 0, "%s: reference_logprob must be a 4-byte aligned pointer", who);
        MAGE_CHECK_ARG(__builtin_isfinite(c.kl_coef) && c.kl_coef >= 0.f, "%s: kl_coef=%g must be finite and >= 0", who, (double)c.kl_coef);
        MAGE_CHECK_ARG(!fwd || (c.kl && (((uintptr_t)c.kl) & 3) == 0), "%s: kl must be a 4-byte aligned pointer", who);
    }
    return MAGE_OK;
}

// The forward call: the row kernel (its instance by K, the filter and whether there is a reference), for a group the group kernel, then the
// two summary kernels over W = 5 sums, 7 with a reference, 8 with a mask or a group.
static int policy_forward(const char* who, const PolicyCall& call, void* stream) {
    if (int rc = policy_call_check(who, call, true)) return rc;
    PolicyCall c = call;
    c.err = mage_error_word();
    MAGE_CHECK_ARG(c.err != nullptr, "%s: mage_init() has not been called", who);
    const bool anch = c.ref != nullptr, topk = c.top_k > 0 && c.top_k < c.K, topp = c.top_p < 1.f;
    const dim3 grid((unsigned)((c.rows + 3) / 4)), parts(POLICY_PARTS), wg(256);
    hipStream_t s = (hipStream_t)stream;
#define MAGE_POLICY(NV, TK, TP)                                                                       \
    do {                                                                                              \
        if (anch) hipLaunchKernelGGL((policy_loss_kernel<NV, TK, TP, true>), grid, wg, 0, s, POLICY_ROW_ARGS(c));      \
        else hipLaunchKernelGGL((policy_loss_kernel<NV, TK, TP, false>), grid, wg, 0, s, POLICY_ROW_ARGS(c));          \
    } while (0)
#define MAGE_POLICY_NV(NV)                                \
    do {                                                  \
        if (topk && topp) MAGE_POLICY(NV, true, true);    \
        else if (topk) MAGE_POLICY(NV, true, false);      \
        else if (topp) MAGE_POLICY(NV, false, true);      \
        else MAGE_POLICY(NV, false, false);               \
    } while (0)
    MAGE_ROW_LADDER(c.K, MAGE_POLICY_NV);
#undef MAGE_POLICY_NV
#undef MAGE_POLICY
    const long chunk = (c.rows + POLICY_PARTS - 1) / POLICY_PARTS;
    if (c.form == FORM_GROUPED) {
        const long groups = c.rows / c.ratio_div;
        if (c.ratio_div <= POLICY_GROUP_WAVE) hipLaunchKernelGGL(policy_group_kernel<64>, dim3((unsigned)((groups + 3) / 4)), wg, 0, s, c);
        else hipLaunchKernelGGL(policy_group_kernel<1024>, dim3((unsigned)groups), dim3(1024), 0, s, c);
        hipLaunchKernelGGL((policy_part_kernel<POLICY_MASKED, true>), parts, wg, 0, s, c, chunk);
    } else if (c.form == FORM_MASKED) {
        hipLaunchKernelGGL(policy_part_kernel<POLICY_MASKED>, parts, wg, 0, s, c, chunk);
    } else if (anch) {
        hipLaunchKernelGGL(policy_part_kernel<POLICY_MEANS>, parts, wg, 0, s, c, chunk);
    } else {
        hipLaunchKernelGGL(policy_part_kernel<5>, parts, wg, 0, s, c, chunk);
    }
    if (c.form == FORM_MASKED || c.form == FORM_GROUPED)
        hipLaunchKernelGGL(policy_summary_kernel<POLICY_MASKED>, dim3(1), parts, 0, s, c.summary, c.norm, c.rows);
    else if (anch) hipLaunchKernelGGL(policy_summary_kernel<POLICY_MEANS>, dim3(1), parts, 0, s, c.summary, c.norm, c.rows);
    else hipLaunchKernelGGL(policy_summary_kernel<5>, dim3(1), parts, 0, s, c.summary, c.norm, c.rows);
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

static int policy_backward(const char* who, const PolicyCall& call, void* stream) {
    if (int rc = policy_call_check(who, call, false)) return rc;
    PolicyCall c = call;
    c.inv_rows = 1.0f / (float)c.rows;
    const bool anch = c.ref != nullptr, grp = c.form == FORM_GROUPED;
    const dim3 grid((unsigned)((c.rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_POLICY_BWD(NV, OT)                                                                                             \
    do {                                                                                                                    \
        if (anch && grp) hipLaunchKernelGGL((policy_loss_bwd_kernel<NV, OT, true, true>), grid, dim3(256), 0, s, POLICY_BWD_ARGS(c, OT));        \
        else if (anch) hipLaunchKernelGGL((policy_loss_bwd_kernel<NV, OT, true, false>), grid, dim3(256), 0, s, POLICY_BWD_ARGS(c, OT));         \
        else if (grp) hipLaunchKernelGGL((policy_loss_bwd_kernel<NV, OT, false, true>), grid, dim3(256), 0, s, POLICY_BWD_ARGS(c, OT));          \
        else hipLaunchKernelGGL((policy_loss_bwd_kernel<NV, OT, false, false>), grid, dim3(256), 0, s, POLICY_BWD_ARGS(c, OT));                  \
    } while (0)
#define MAGE_POLICY_BWD_NV(NV)                                          \
    do {                                                                \
        if (c.dl_dtype == MAGE_F32) MAGE_POLICY_BWD(NV, float);         \
        else MAGE_POLICY_BWD(NV, unsigned short);                       \
    } while (0)
    MAGE_ROW_LADDER(c.K, MAGE_POLICY_BWD_NV);
#undef MAGE_POLICY_BWD_NV
#undef MAGE_POLICY_BWD
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

// The twelve fields every entry point takes, and the scalars the kernels use in place of the caller's.  Everything else starts out absent.
static PolicyCall policy_call(int form, const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                              int64_t adv_div, const float* behaviour_logprob, float temperature, float clip_lo, float clip_hi,
                              float entropy_coef) {
    PolicyCall c{};
    c.form = form;
    c.logits = logits, c.rows = (long)rows, c.K = K, c.ld = (long)ld, c.tokens = tokens;
    c.adv = advantage, c.adv_div = (long)adv_div, c.blp = behaviour_logprob;
    c.temperature = temperature, c.clip_lo = clip_lo, c.clip_hi = clip_hi, c.ent_coef = entropy_coef;
    c.inv_t = (float)(1.0 / (double)temperature);
    c.cmin = (float)(1.0 - (double)clip_lo), c.cmax = (float)(1.0 + (double)clip_hi);
    return c;
}
// ... what the four forward entry points add to them, and the four backward ones (cut is theirs to read only)
static void policy_forward_fields(PolicyCall& c, int32_t top_k, float top_p, float* row_loss, float* logprob, float* entropy, uint32_t* cut,
                                  float* summary) {
    c.top_k = top_k, c.top_p = top_p, c.row_loss = row_loss, c.logprob = logprob, c.entropy = entropy, c.cut = cut, c.summary = summary;
}
static void policy_backward_fields(PolicyCall& c, const uint32_t* cut, const float* grad_out, void* dlogits, int32_t dl_dtype) {
    c.cut = const_cast<uint32_t*>(cut), c.gout = grad_out, c.dl = dlogits, c.dl_dtype = dl_dtype;
}

extern "C" int mage_policy_loss(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                int64_t adv_div, const float* behaviour_logprob, float temperature, int32_t top_k, float top_p, float clip_lo,
                                float clip_hi, float entropy_coef, float* row_loss, float* logprob, float* entropy, uint32_t* cut,
                                float* summary, void* stream) {
    PolicyCall c = policy_call(FORM_PLAIN, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_forward_fields(c, top_k, top_p, row_loss, logprob, entropy, cut, summary);
    return policy_forward("mage_policy_loss", c, stream);
}

extern "C" int mage_policy_loss_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                    int64_t adv_div, const float* behaviour_logprob, const uint32_t* cut, float temperature, float clip_lo,
                                    float clip_hi, float entropy_coef, const float* grad_out, void* dlogits, int32_t dl_dtype, void* stream) {
    PolicyCall c = policy_call(FORM_PLAIN, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_backward_fields(c, cut, grad_out, dlogits, dl_dtype);
    return policy_backward("mage_policy_loss_bwd", c, stream);
}

extern "C" int mage_policy_loss_anchored(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                         int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                                         int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef,
                                         float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary,
                                         void* stream) {
    PolicyCall c = policy_call(FORM_ANCHORED, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_forward_fields(c, top_k, top_p, row_loss, logprob, entropy, cut, summary);
    c.ref = reference_logprob, c.kl_coef = kl_coef, c.kl = kl;
    return policy_forward("mage_policy_loss_anchored", c, stream);
}

extern "C" int mage_policy_loss_anchored_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                             const float* advantage, int64_t adv_div, const float* behaviour_logprob,
                                             const float* reference_logprob, const uint32_t* cut, float temperature, float clip_lo,
                                             float clip_hi, float entropy_coef, float kl_coef, const float* grad_out, void* dlogits,
                                             int32_t dl_dtype, void* stream) {
    PolicyCall c = policy_call(FORM_ANCHORED, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_backward_fields(c, cut, grad_out, dlogits, dl_dtype);
    c.ref = reference_logprob, c.kl_coef = kl_coef;
    return policy_backward("mage_policy_loss_anchored_bwd", c, stream);
}

extern "C" int mage_policy_loss_masked(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                       int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                                       int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef,
                                       float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary, float* norm,
                                       const uint8_t* given, void* stream) {
    PolicyCall c = policy_call(FORM_MASKED, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_forward_fields(c, top_k, top_p, row_loss, logprob, entropy, cut, summary);
    c.ref = reference_logprob, c.kl_coef = kl_coef, c.kl = kl, c.given = given, c.norm = norm;
    return policy_forward("mage_policy_loss_masked", c, stream);
}

extern "C" int mage_policy_loss_masked_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                           const float* advantage, int64_t adv_div, const float* behaviour_logprob,
                                           const float* reference_logprob, const uint32_t* cut, float temperature, float clip_lo, float clip_hi,
                                           float entropy_coef, float kl_coef, const float* grad_out, const float* norm, void* dlogits,
                                           int32_t dl_dtype, const uint8_t* given, void* stream) {
    PolicyCall c = policy_call(FORM_MASKED, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_backward_fields(c, cut, grad_out, dlogits, dl_dtype);
    c.ref = reference_logprob, c.kl_coef = kl_coef, c.given = given, c.norm = const_cast<float*>(norm);
    return policy_backward("mage_policy_loss_masked_bwd", c, stream);
}

extern "C" int mage_policy_loss_grouped(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* advantage,
                                        int64_t adv_div, const float* behaviour_logprob, const float* reference_logprob, float temperature,
                                        int32_t top_k, float top_p, float clip_lo, float clip_hi, float entropy_coef, float kl_coef,
                                        float* row_loss, float* logprob, float* entropy, uint32_t* cut, float* kl, float* summary, float* norm,
                                        const uint8_t* given, int64_t ratio_div, float* group_logratio, int32_t* group_count, void* stream) {
    PolicyCall c = policy_call(FORM_GROUPED, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_forward_fields(c, top_k, top_p, row_loss, logprob, entropy, cut, summary);
    c.ref = reference_logprob, c.kl_coef = kl_coef, c.kl = kl, c.given = given, c.norm = norm;
    c.ratio_div = (long)ratio_div, c.glr = group_logratio, c.gcount = group_count;
    return policy_forward("mage_policy_loss_grouped", c, stream);
}

extern "C" int mage_policy_loss_grouped_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                            const float* advantage, int64_t adv_div, const float* behaviour_logprob,
                                            const float* reference_logprob, const uint32_t* cut, float temperature, float clip_lo, float clip_hi,
                                            float entropy_coef, float kl_coef, const float* grad_out, const float* norm, void* dlogits,
                                            int32_t dl_dtype, const uint8_t* given, int64_t ratio_div, const float* group_logratio,
                                            void* stream) {
    PolicyCall c = policy_call(FORM_GROUPED, logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob, temperature, clip_lo, clip_hi,
                               entropy_coef);
    policy_backward_fields(c, cut, grad_out, dlogits, dl_dtype);
    c.ref = reference_logprob, c.kl_coef = kl_coef, c.given = given, c.norm = const_cast<float*>(norm);
    c.ratio_div = (long)ratio_div, c.glr = const_cast<float*>(group_logratio);
    return policy_backward("mage_policy_loss_grouped_bwd", c, stream);
}
