// Supervised cross entropy over one row of logits per wave (mage_token_xent / mage_token_xent_bwd; include/mage_hip_ext.h states the rule):
// class weights, label smoothing, a z-loss, a per-row mask, and what the row predicts (the rank of the target).  The row lies in registers in
// token_row.h's layout; the log-sum-exp is row_logsumexp, so row_nll carries -mage_token_logprob's bits; the summary is mage_distill_loss's
// two-launch fixed-order fp64 reduction.
// The terms are written out operation by operation (the header gives them as formulas and the test's restatement counts the roundings), so
// the file is compiled with floating-point contraction off: a fused multiply-add is written __fmaf_rn.
#include "token_row.h"

#pragma clang fp contract(off)

namespace {

// stage 1 -> stage 2 of the summary, within one mage_token_xent call (stream order): a workgroup's six fp64 sums
enum { XENT_PARTS = 16384, XENT_SUMS = 6 };
enum { XS_LOSS = 0, XS_NLL = 1, XS_HIT = 2, XS_LSE2 = 3, XS_GIVEN = 4, XS_WY = 5 };
__device__ double g_xent_part[XENT_PARTS * XENT_SUMS];

// chunk c of the class weights, 0 past K (never used there: every user guards k < K); null: all ones
__device__ __forceinline__ f32x4 xent_weight_chunk(const float* __restrict__ cw, int lane, int K, int c) {
    const int k = c * 256 + lane * 4;
    if (!cw) return f32x4{1.f, 1.f, 1.f, 1.f};
    return k < K ? *(const f32x4*)(cw + k) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// The scalars of one call, formed once on the host: c1 = (float)(1 - eps), c2 = (float)(eps / K), both from fp64.
struct XentCoef { float c1, c2, zeta; };

// Workgroup b takes the row quads b, b + gridDim.x, ...; wave w of it the row 4 quad + w (distill_kernel's geometry).  A wave adds its rows'
// six terms in fp64 in ascending row order; thread q < 6 adds the four waves in order.
template <int NV, bool SMOOTH>
__global__ __launch_bounds__(256) void xent_kernel(const float* __restrict__ logits, long ld, long rows, int K, const int64_t* __restrict__ target,
                                                   const float* __restrict__ cw, XentCoef cf, const uint8_t* __restrict__ given,
                                                   float* __restrict__ row_loss, float* __restrict__ row_nll, float* __restrict__ row_lse,
                                                   int32_t* __restrict__ rank, long quads, int* __restrict__ err) {
    __shared__ double red[4][XENT_SUMS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc[XENT_SUMS] = {};
    for (long qd = blockIdx.x; qd < quads; qd += gridDim.x) {
        const long i = qd * 4 + wv;
        if (i >= rows) break;                               // (wave-uniform: the last quad's missing rows)
        if (row_given(given, i)) {                          // (wave-uniform) the row is not read, its target not looked at
            if (lane == 0) {
                row_loss[i] = 0.f;
                row_nll[i] = 0.f;
                row_lse[i] = 0.f;
                if (rank) rank[i] = 0;
            }
            acc[XS_GIVEN] += 1.0;
            continue;
        }
        const float* p = logits + i * ld;
        f32x4 zc[NV / 4];
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) zc[c] = row_chunk_inf(p, lane, K, c);
        float lse;
        {
            float w[NV];
            const RowLse l = row_logsumexp<NV>([&](int c) { return zc[c]; }, w);
            lse = l.mx + logf(l.zs);
        }
        const int y = (int)row_token<true>(target, i, K, lane == 0 ? err : nullptr);
        const float zy = p[y];
        const float nll = -(zy - lse);                      // mage_token_logprob's difference, negated: its bits with the sign turned
        const float wy = cw ? cw[y] : 1.f;
        // rank by ballots on the sampler's keys (exact); a code past K has key 0 and is never above a number
        const unsigned ky = sample_key(zy);
        int rk = 0;
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = c * 256 + lane * 4 + e;
                const unsigned key = k < K ? sample_key(zc[c][e]) : 0u;
                rk += __popcll(__ballot(key > ky || (key == ky && k < y)));
            }
        }
        if (zy != zy) rk = K;
        float loss = __fmul_rn(__fmul_rn(cf.c1, wy), nll);
        if constexpr (SMOOTH) {                             // sum_k w_k (lse - z_k), k < K: lane register order, then the butterfly
            // (the weights do not depend on the row: the compiler loads a lane's NV of them once, before the loop over the quads)
            float sm = 0.f;
#pragma unroll
            for (int c = 0; c < NV / 4; ++c) {
                const f32x4 wc = xent_weight_chunk(cw, lane, K, c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c * 256 + lane * 4 + e < K) sm = __fmaf_rn(wc[e], lse - zc[c][e], sm);
            }
            sm = wave_sum(sm);
            loss = __fmaf_rn(cf.c2, sm, loss);
        }
        if (lane == 0) {
            row_loss[i] = loss;
            row_nll[i] = nll;
            row_lse[i] = lse;
            if (rank) rank[i] = rk;
        }
        acc[XS_LOSS] += (double)loss;
        acc[XS_NLL] += (double)nll;
        acc[XS_HIT] += rk == 0 ? 1.0 : 0.0;
        acc[XS_LSE2] += (double)lse * (double)lse;
        acc[XS_WY] += (double)wy;
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < XENT_SUMS; ++s) red[wv][s] = acc[s];
    }
    __syncthreads();
    if (threadIdx.x < XENT_SUMS) {
        const int s = threadIdx.x;
        g_xent_part[(long)blockIdx.x * XENT_SUMS + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
    }
}

// stage 2 (distill_summary_kernel's shape): thread t adds the sums of workgroups t, t + 256, ... in ascending order, the lanes meet in an xor
// butterfly, the four waves in order.  The given count and, without class weights, sum w_y are sums of ones: exact.
__global__ __launch_bounds__(256) void xent_summary_kernel(float* __restrict__ summary, float* __restrict__ norm, long rows, int parts, double zeta) {
    constexpr int W = XENT_SUMS;
    __shared__ double red[4][W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        double v = 0.0;
        for (int b = threadIdx.x; b < parts; b += 256) v += g_xent_part[(long)b * W + s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[W];
#pragma unroll
        for (int s = 0; s < W; ++s) t[s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
        const long n_free = rows - (long)t[XS_GIVEN];
        const double sw = t[XS_WY], n = (double)n_free;
        const double lse2 = n_free > 0 ? t[XS_LSE2] / n : 0.0;
        const double wloss = sw > 0.0 ? t[XS_LOSS] / sw : 0.0;
        summary[0] = (float)(zeta > 0.0 ? wloss + zeta * lse2 : wloss);
        summary[1] = (float)(n_free > 0 ? t[XS_NLL] / n : 0.0);
        summary[2] = (float)(n_free > 0 ? t[XS_HIT] / n : 0.0);
        summary[3] = (float)lse2;
        summary[4] = (float)(t[XS_GIVEN] / (double)rows);
        norm[0] = (float)(sw > 0.0 ? 1.0 / sw : 0.0);
        norm[1] = (float)(n_free > 0 ? 1.0 / n : 0.0);
    }
}

// d_k = A p_k - B 1[k = y] - C w_k with, g = grad_out[0],
//   B = (g norm[0]) (c1 w_y),   C = (g norm[0]) c2,   A = fma(C, W, B) + ((g norm[1]) (2 zeta)) lse,
// p = expf(z - mx) * (1 / Z) from row_logsumexp, W = sum_k w_k in the smooth term's order ((float)K without class weights: the same bits).
// Without smoothing C = 0 and neither W nor the weights are formed.  A given row is +0 throughout and is not read.
template <int NV, typename OT, bool SMOOTH>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const float* __restrict__ logits, long ld, long rows, int K,
                                                       const int64_t* __restrict__ target, const float* __restrict__ cw, XentCoef cf,
                                                       const uint8_t* __restrict__ given, const float* __restrict__ gout,
                                                       const float* __restrict__ norm, OT* __restrict__ dl) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    OT* o = dl + i * (long)K;
    if (row_given(given, i)) {                              // (wave-uniform)
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
            const int k = c * 256 + lane * 4;
            if (k < K) store4(o + k, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    const float* p = logits + i * ld;
    float w[NV];
    const RowLse l = row_logsumexp<NV>([=](int c) { return row_chunk_inf(p, lane, K, c); }, w);
    const float inv = 1.0f / l.zs, lse = l.mx + logf(l.zs);
    const int y = (int)row_token<true>(target, i, K, nullptr);          // (a bad target: the forward call reported it; clamped as there)
    const float wy = cw ? cw[y] : 1.f;
    const float g0 = __fmul_rn(gout[0], norm[0]), g1 = __fmul_rn(gout[0], norm[1]);
    const float B = __fmul_rn(g0, __fmul_rn(cf.c1, wy));
    float A = B, C = 0.f;
    if constexpr (SMOOTH) {
        C = __fmul_rn(g0, cf.c2);
        float W = (float)K;
        if (cw) {
            W = 0.f;
#pragma unroll
            for (int c = 0; c < NV / 4; ++c) {
                const f32x4 wc = xent_weight_chunk(cw, lane, K, c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c * 256 + lane * 4 + e < K) W = __fadd_rn(W, wc[e]);
            }
            W = wave_sum(W);
        }
        A = __fmaf_rn(C, W, B);
    }
    if (cf.zeta > 0.f) A = __fmaf_rn(__fmul_rn(g1, __fmul_rn(2.f, cf.zeta)), lse, A);
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const int k = c * 256 + lane * 4;
        if (k >= K) break;
        f32x4 wc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (SMOOTH) wc = xent_weight_chunk(cw, lane, K, c);
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pk = __fmul_rn(w[c * 4 + e], inv);
            float v = __fmaf_rn(A, pk, k + e == y ? -B : -0.f);
            if constexpr (SMOOTH) v = __fmaf_rn(-C, wc[e], v);
            d[e] = v;
        }
        store4(o + k, d);
    }
}

}  // namespace

// the argument rules of the pair
static int xent_check(const char* who, const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* target,
                      const float* class_weight, float label_smoothing, float z_loss, XentCoef& cf) {
    if (int rc = token_rows_check(who, logits, rows, K, ld, true)) return rc;
    MAGE_CHECK_ARG((((uintptr_t)target) & 7) == 0 && (((uintptr_t)class_weight) & 15) == 0,
                   "%s: target must be 8-byte and class_weight 16-byte aligned", who);
    MAGE_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 1.f, "%s: label_smoothing=%g outside [0, 1)", who, (double)label_smoothing);
    MAGE_CHECK_ARG(__builtin_isfinite(z_loss) && z_loss >= 0.f, "%s: z_loss=%g must be finite and >= 0", who, (double)z_loss);
    cf.c1 = (float)(1.0 - (double)label_smoothing);
    cf.c2 = (float)((double)label_smoothing / (double)K);
    cf.zeta = z_loss;
    return MAGE_OK;
}

extern "C" int mage_token_xent(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* target, const float* class_weight,
                               float label_smoothing, float z_loss, const uint8_t* given, float* row_loss, float* row_nll, float* row_lse,
                               int32_t* rank, float* summary, float* norm, void* stream) {
    const char* who = "mage_token_xent";
    MAGE_CHECK_ARG(logits && target && row_loss && row_nll && row_lse && summary && norm, "%s: null pointer", who);
    XentCoef cf;
    if (int rc = xent_check(who, logits, rows, K, ld, target, class_weight, label_smoothing, z_loss, cf)) return rc;
    MAGE_CHECK_ARG(((((uintptr_t)row_loss) | ((uintptr_t)row_nll) | ((uintptr_t)row_lse) | ((uintptr_t)rank) | ((uintptr_t)summary) |
                     ((uintptr_t)norm)) & 3) == 0,
                   "%s: row_loss, row_nll, row_lse, rank, summary and norm must be 4-byte aligned", who);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "%s: mage_init() has not been called", who);
    const long quads = (long)((rows + 3) / 4);
    const int parts = (int)(quads < XENT_PARTS ? quads : XENT_PARTS);
    hipStream_t s = (hipStream_t)stream;
#define MAGE_XENT(NV, SM)                                                                                                                   \
    hipLaunchKernelGGL((xent_kernel<NV, SM>), dim3((unsigned)parts), dim3(256), 0, s, logits, (long)ld, (long)rows, K, target, class_weight, cf, \
                       given, row_loss, row_nll, row_lse, rank, quads, err)
#define MAGE_XENT_NV(NV)                                  \
    do {                                                  \
        if (label_smoothing > 0.f) MAGE_XENT(NV, true);   \
        else MAGE_XENT(NV, false);                        \
    } while (0)
    MAGE_ROW_LADDER(K, MAGE_XENT_NV);
#undef MAGE_XENT_NV
#undef MAGE_XENT
    hipLaunchKernelGGL(xent_summary_kernel, dim3(1), dim3(256), 0, s, summary, norm, (long)rows, parts, (double)z_loss);
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

extern "C" int mage_token_xent_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* target, const float* class_weight,
                                   float label_smoothing, float z_loss, const uint8_t* given, const float* grad_out, const float* norm,
                                   void* dlogits, int32_t dl_dtype, void* stream) {
    const char* who = "mage_token_xent_bwd";
    MAGE_CHECK_ARG(logits && target && grad_out && norm && dlogits, "%s: null pointer", who);
    XentCoef cf;
    if (int rc = xent_check(who, logits, rows, K, ld, target, class_weight, label_smoothing, z_loss, cf)) return rc;
    MAGE_CHECK_ARG(((((uintptr_t)grad_out) | ((uintptr_t)norm)) & 3) == 0, "%s: grad_out and norm must be 4-byte aligned", who);
    MAGE_CHECK_ARG((dl_dtype == MAGE_F32 || dl_dtype == MAGE_BF16) && (((uintptr_t)dlogits) & 15) == 0,
                   "%s: dlogits must be 16-byte aligned fp32 or bf16 (dtype %d)", who, dl_dtype);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_XENT_BWD(NV, OT, SM)                                                                                                          \
    hipLaunchKernelGGL((xent_bwd_kernel<NV, OT, SM>), grid, dim3(256), 0, s, logits, (long)ld, (long)rows, K, target, class_weight, cf, given, \
                       grad_out, norm, (OT*)dlogits)
#define MAGE_XENT_BWD_NV(NV)                                                        \
    do {                                                                            \
        const bool sm = label_smoothing > 0.f;                                      \
        if (dl_dtype == MAGE_F32 && sm) MAGE_XENT_BWD(NV, float, true);             \
        else if (dl_dtype == MAGE_F32) MAGE_XENT_BWD(NV, float, false);             \
        else if (sm) MAGE_XENT_BWD(NV, unsigned short, true);                       \
        else MAGE_XENT_BWD(NV, unsigned short, false);                              \
    } while (0)
    MAGE_ROW_LADDER(K, MAGE_XENT_BWD_NV);
#undef MAGE_XENT_BWD_NV
#undef MAGE_XENT_BWD
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}
