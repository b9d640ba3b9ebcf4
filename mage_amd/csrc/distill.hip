// Distillation loss: the full-distribution KL between a student's and a teacher's row of logits (mage_distill_loss / mage_distill_loss_bwd;
// include/mage_hip_ext.h states the rule).  One wave per row pair, both rows read once into registers in token_row.h's layout (a lane
// holds 2 NV raw logits; the forward kernel's NV = 64 instance keeps one row and reads the other twice), the sums in row_logsumexp's
// order.  The forward kernel computes KL(P || Q) for a pair of pointers: mode 0 hands it (teacher, student), mode 1 (student, teacher),
// so the two modes are one instruction stream.
// Equal rows must cancel exactly (p_S - p_T = 0 needs both products rounded before the subtraction), so this file is compiled with
// floating-point contraction off: an a * b + c below is two roundings, and a fused multiply-add is written __fmaf_rn.  (The __fmul_rn /
// __fsub_rn wrappers would not do: they are plain operators in a header compiled with contraction on, and the compiler did fuse them.)
#include "token_row.h"

#pragma clang fp contract(off)

namespace {

// a row's raw logits, -inf past K (row_logsumexp's padding: one more impossible code)
template <int NV>
__device__ __forceinline__ void pair_load(const float* __restrict__ p, int lane, int K, float (&z)[NV]) {
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const f32x4 v = row_chunk_inf(p, lane, K, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) z[c * 4 + e] = v[e];
    }
}
// max_j z_j, a NaN skipped (row_logsumexp's maximum).  The maximum of the scaled row is this value times inv_t: rounding is monotone and
// inv_t > 0, so max_j fl(z_j inv_t) = fl((max_j z_j) inv_t) -- the bits row_logsumexp would find on the scaled row.
template <int NV>
__device__ __forceinline__ float pair_max(const float (&z)[NV]) {
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < NV; ++e) m = fmaxf(m, z[e]);
    return wave_max(m);
}
// the first code that holds the maximum (mage_argmax's rule: NaNs skipped, -0 == +0, the lowest index wins; a row of NaNs: 0x7fffffff)
template <int NV>
__device__ __forceinline__ int pair_first(const float (&z)[NV], float m, int lane) {
    int bj = 0x7fffffff;
#pragma unroll
    for (int e = NV - 1; e >= 0; --e)
        if (z[e] == m) bj = (e >> 2) * 256 + lane * 4 + (e & 3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bj = min(bj, __shfl_xor(bj, o, 64));
    return bj;
}

// stage 1 -> stage 2 of the summary, within one mage_distill_loss call (stream order): a workgroup's five fp64 sums
enum { DISTILL_PARTS = 16384, DISTILL_SUMS = 5 };
__device__ double g_distill_part[DISTILL_PARTS * DISTILL_SUMS];

// the same two values of a row that is not kept: a lane's running maximum and the first code that holds it, in ascending code order
template <int NV>
__device__ __forceinline__ float pair_scan(const float* __restrict__ p, int lane, int K, int& first) {
    float m = -INFINITY;
    int idx = -1;
#pragma unroll
    for (int c = 0; c < NV / 4; ++c) {
        const f32x4 v = row_chunk_inf(p, lane, K, c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] > m || (idx < 0 && v[e] == m)) {
                m = v[e];
                idx = c * 256 + lane * 4 + e;
            }
    }
    const float r = wave_max(m);
    int bj = idx >= 0 && m == r ? idx : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bj = min(bj, __shfl_xor(bj, o, 64));
    first = bj;
    return r;
}

// KL(P || Q) of row i of p against row i of q, both at temperature 1 / inv_t, for every free row; swap: the student is P (mode 1).
// Workgroup b takes the row quads b, b + gridDim.x, ...; wave w of it the row 4 quad + w.  A wave adds its rows' kl, teacher entropy, student
// entropy and argmax agreement in fp64 in ascending row order and counts its given rows; thread q < 5 adds the four waves in order.
// REREAD (NV = 64: two rows of 64 values per lane leave one wave per SIMD): only P stays in registers; Q is read once for its maximum and
// once more, mostly from L2, for the sums.  The operations and their order are the same, so are the bits.
template <int NV, bool REREAD = (NV == 64)>
__global__ __launch_bounds__(256) void distill_kernel(const float* __restrict__ p, long ld_p, const float* __restrict__ q, long ld_q, long rows,
                                                      int K, float inv_t, bool swap, const uint8_t* __restrict__ given,
                                                      float* __restrict__ row_kl, long quads) {
    __shared__ double red[4][DISTILL_SUMS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc[DISTILL_SUMS] = {};
    for (long qd = blockIdx.x; qd < quads; qd += gridDim.x) {
        const long i = qd * 4 + wv;
        if (i >= rows) break;                               // (wave-uniform: the last quad's missing rows)
        if (row_given(given, i)) {                          // (wave-uniform) neither row is read
            if (lane == 0) row_kl[i] = 0.f;
            acc[4] += 1.0;
            continue;
        }
        const float* qrow = q + i * ld_q;
        float zp[NV], zq[REREAD ? 4 : NV];
        pair_load<NV>(p + i * ld_p, lane, K, zp);
        const float rp = pair_max<NV>(zp);
        float rq;
        int fq;
        if constexpr (REREAD) {
            rq = pair_scan<NV>(qrow, lane, K, fq);
        } else {
            pair_load<NV>(qrow, lane, K, zq);
            rq = pair_max<NV>(zq);
            fq = pair_first<NV>(zq, rq, lane);
        }
        const bool agree = pair_first<NV>(zp, rp, lane) == fq;
        const float mp = rp * inv_t, mq = rq * inv_t;
        // row_logsumexp's sums on both scaled rows, and A = sum_j w_P,j (d_P,j - d_Q,j) beside them (a zero weight adds nothing)
        float zsp = 0.f, zsq = 0.f, tsp = 0.f, tsq = 0.f, a = 0.f;
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
            f32x4 vq;
            if constexpr (REREAD) vq = row_chunk_inf(qrow, lane, K, c);
            else vq = f32x4{zq[c * 4], zq[c * 4 + 1], zq[c * 4 + 2], zq[c * 4 + 3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dp = zp[c * 4 + e] * inv_t - mp, dq = vq[e] * inv_t - mq;
                const float wp = expf(dp), wq = expf(dq);
                zsp = zsp + wp;
                zsq = zsq + wq;
                tsp = wp == 0.f ? tsp : __fmaf_rn(wp, dp, tsp);
                tsq = wq == 0.f ? tsq : __fmaf_rn(wq, dq, tsq);
                a = wp == 0.f ? a : __fmaf_rn(wp, dp - dq, a);
            }
        }
        zsp = wave_sum(zsp);
        zsq = wave_sum(zsq);
        tsp = wave_sum(tsp);
        tsq = wave_sum(tsq);
        a = wave_sum(a);
        const float lzp = logf(zsp), lzq = logf(zsq);
        const float kl = a / zsp + (lzq - lzp);
        const float hp = lzp - tsp / zsp, hq = lzq - tsq / zsq;
        if (lane == 0) row_kl[i] = kl;
        acc[0] += (double)kl;
        acc[1] += (double)(swap ? hq : hp);                 // the teacher's entropy
        acc[2] += (double)(swap ? hp : hq);                 // the student's
        acc[3] += agree ? 1.0 : 0.0;
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < DISTILL_SUMS; ++s) red[wv][s] = acc[s];
    }
    __syncthreads();
    if (threadIdx.x < DISTILL_SUMS) {
        const int s = threadIdx.x;
        g_distill_part[(long)blockIdx.x * DISTILL_SUMS + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
    }
}

// stage 2: thread t adds the sums of workgroups t, t + 256, ... in ascending order, the lanes meet in an xor butterfly, the four waves in
// order (policy_summary_masked_kernel's shape).  The fifth sum is the number of given rows, exact in fp64: n_free = rows - given.
__global__ __launch_bounds__(256) void distill_summary_kernel(float* __restrict__ summary, float* __restrict__ norm, long rows, int parts) {
    constexpr int W = DISTILL_SUMS;
    __shared__ double red[4][W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        double v = 0.0;
        for (int b = threadIdx.x; b < parts; b += 256) v += g_distill_part[(long)b * W + s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int s = threadIdx.x;
        const double ng = ((red[0][4] + red[1][4]) + red[2][4]) + red[3][4];
        const long n_free = rows - (long)ng;
        if (s < 4) {
            const double inv = n_free > 0 ? 1.0 / (double)n_free : 0.0;
            summary[s] = (float)((((red[0][s] + red[1][s]) + red[2][s]) + red[3][s]) * inv);
        } else {
            summary[4] = (float)(ng / (double)rows);
            norm[0] = n_free > 0 ? 1.0f / (float)n_free : 0.f;
        }
    }
}

// dlogits of the mean of row_kl over the free rows, c = grad_out[0] * norm[0] * inv_t:
//   MODE 0   c (p_S,j - p_T,j);      MODE 1   c p_S,j ((log p_S,j - log p_T,j) - row_kl_i), 0 where p_S,j == 0,
// p = w * (1 / Z) and log p_S - log p_T = (d_S - d_T) - (log Z_S - log Z_T) from the forward kernel's w, d and Z.  The raw logits in the
// registers give way to (w_S, w_T) or (w_S, d_S - d_T).  A given row, and a row whose row_kl is not finite, is +0 throughout.
template <int NV, typename OT, int MODE>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ teacher, long ld_t,
                                                          long rows, int K, float inv_t, const uint8_t* __restrict__ given,
                                                          const float* __restrict__ row_kl, const float* __restrict__ gout,
                                                          const float* __restrict__ norm, OT* __restrict__ dl) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    OT* o = dl + i * (long)K;
    bool zero = row_given(given, i);
    float kl = 0.f;
    if (!zero) {
        kl = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, row_kl[i])));
        zero = !__builtin_isfinite(kl);
    }
    if (zero) {                                             // (wave-uniform) nothing of either row is read
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
            const int k = c * 256 + lane * 4;
            if (k < K) store4(o + k, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    float zs[NV], zt[NV];
    pair_load<NV>(logits + i * ld, lane, K, zs);
    pair_load<NV>(teacher + i * ld_t, lane, K, zt);
    const float ms = pair_max<NV>(zs) * inv_t, mt = pair_max<NV>(zt) * inv_t;
    float sum_s = 0.f, sum_t = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const float ds = zs[e] * inv_t - ms, dt = zt[e] * inv_t - mt;
        const float ws = expf(ds), wt = expf(dt);
        sum_s = sum_s + ws;
        sum_t = sum_t + wt;
        zs[e] = ws;
        zt[e] = MODE == 0 ? wt : ds - dt;
    }
    sum_s = wave_sum(sum_s);
    sum_t = wave_sum(sum_t);
    const float c = gout[0] * norm[0] * inv_t, inv_s = 1.0f / sum_s, inv_tz = 1.0f / sum_t;
    const float lzd = logf(sum_s) - logf(sum_t);
#pragma unroll
    for (int ch = 0; ch < NV / 4; ++ch) {
        const int k = ch * 256 + lane * 4;
        if (k >= K) break;
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = ch * 4 + e;
            const float ps = zs[j] * inv_s;
            if constexpr (MODE == 0)
                d[e] = c * (ps - zt[j] * inv_tz);
            else
                d[e] = ps == 0.f ? 0.f : (c * ps) * ((zt[j] - lzd) - kl);
        }
        store4(o + k, d);
    }
}

}  // namespace

// the argument rules of the pair: token_rows_check's sizes on both buffers, the temperature, the mode
static int distill_check(const char* who, const float* logits, int64_t rows, int32_t K, int64_t ld, const float* teacher, int64_t ld_t,
                         float temperature, float inv_t, int32_t mode) {
    if (int rc = token_rows_check(who, logits, rows, K, ld, true)) return rc;
    if (int rc = token_rows_check(who, teacher, rows, K, ld_t, true, "ld_t", ld_t)) return rc;
    MAGE_CHECK_ARG(__builtin_isfinite(temperature) && temperature > 0.f && __builtin_isfinite(inv_t),
                   "%s: temperature=%g must be finite and > 0", who, (double)temperature);
    MAGE_CHECK_ARG(mode == 0 || mode == 1, "%s: mode=%d must be 0 (forward KL, teacher || student) or 1 (reverse KL)", who, mode);
    return MAGE_OK;
}

extern "C" int mage_distill_loss(const float* logits, int64_t rows, int32_t K, int64_t ld, const float* teacher, int64_t ld_t, float temperature,
                                 int32_t mode, const uint8_t* given, float* row_kl, float* summary, float* norm, void* stream) {
    const char* who = "mage_distill_loss";
    MAGE_CHECK_ARG(logits && teacher && row_kl && summary && norm, "%s: null pointer", who);
    const float inv_t = (float)(1.0 / (double)temperature);
    if (int rc = distill_check(who, logits, rows, K, ld, teacher, ld_t, temperature, inv_t, mode)) return rc;
    MAGE_CHECK_ARG(((((uintptr_t)row_kl) | ((uintptr_t)summary) | ((uintptr_t)norm)) & 3) == 0,
                   "%s: row_kl, summary and norm must be 4-byte aligned", who);
    const long quads = (long)((rows + 3) / 4);
    const int parts = (int)(quads < DISTILL_PARTS ? quads : DISTILL_PARTS);
    hipStream_t s = (hipStream_t)stream;
    const bool swap = mode == 1;
    const float *p = swap ? logits : teacher, *q = swap ? teacher : logits;
    const long ld_p = (long)(swap ? ld : ld_t), ld_q = (long)(swap ? ld_t : ld);
#define MAGE_DISTILL(NV) \
    hipLaunchKernelGGL(distill_kernel<NV>, dim3((unsigned)parts), dim3(256), 0, s, p, ld_p, q, ld_q, (long)rows, K, inv_t, swap, given, row_kl, quads)
    MAGE_ROW_LADDER(K, MAGE_DISTILL);
#undef MAGE_DISTILL
    hipLaunchKernelGGL(distill_summary_kernel, dim3(1), dim3(256), 0, s, summary, norm, (long)rows, parts);
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

extern "C" int mage_distill_loss_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const float* teacher, int64_t ld_t,
                                     float temperature, int32_t mode, const uint8_t* given, const float* row_kl, const float* grad_out,
                                     const float* norm, void* dlogits, int32_t dl_dtype, void* stream) {
    const char* who = "mage_distill_loss_bwd";
    MAGE_CHECK_ARG(logits && teacher && row_kl && grad_out && norm && dlogits, "%s: null pointer", who);
    const float inv_t = (float)(1.0 / (double)temperature);
    if (int rc = distill_check(who, logits, rows, K, ld, teacher, ld_t, temperature, inv_t, mode)) return rc;
    MAGE_CHECK_ARG(((((uintptr_t)row_kl) | ((uintptr_t)grad_out) | ((uintptr_t)norm)) & 3) == 0,
                   "%s: row_kl, grad_out and norm must be 4-byte aligned", who);
    MAGE_CHECK_ARG((dl_dtype == MAGE_F32 || dl_dtype == MAGE_BF16) && (((uintptr_t)dlogits) & 15) == 0,
                   "%s: dlogits must be 16-byte aligned fp32 or bf16 (dtype %d)", who, dl_dtype);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define MAGE_DISTILL_BWD(NV, OT, MODE)                                                                                                        \
    hipLaunchKernelGGL((distill_bwd_kernel<NV, OT, MODE>), grid, dim3(256), 0, s, logits, (long)ld, teacher, (long)ld_t, (long)rows, K, inv_t, \
                       given, row_kl, grad_out, norm, (OT*)dlogits)
#define MAGE_DISTILL_BWD_NV(NV)                                             \
    do {                                                                    \
        if (dl_dtype == MAGE_F32 && mode == 0) MAGE_DISTILL_BWD(NV, float, 0);       \
        else if (dl_dtype == MAGE_F32) MAGE_DISTILL_BWD(NV, float, 1);               \
        else if (mode == 0) MAGE_DISTILL_BWD(NV, unsigned short, 0);                 \
        else MAGE_DISTILL_BWD(NV, unsigned short, 1);                                \
    } while (0)
    MAGE_ROW_LADDER(K, MAGE_DISTILL_BWD_NV);
#undef MAGE_DISTILL_BWD_NV
#undef MAGE_DISTILL_BWD
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}
