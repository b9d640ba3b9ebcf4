// Preference fine-tuning on ranked pairs of clips (DPO / IPO): the pair stage (mage_preference_loss) and the gradient of weighted token
// log-probabilities with respect to the logits (mage_token_logprob_bwd).  include/mage_hip_ext.h states the rules; no site in the reference
// (it trains on cross-entropy only).
#include "token_row.h"
#include <math.h>

// The fp64 terms are written out operation by operation: the header gives them as formulas, and the test's restatement follows the same ones.
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------ the pair stage
enum { PREF_MAX = 65536, PREF_TILE = 256, PREF_MEANS = 5 };
struct __attribute__((aligned(16))) PrefPair { int w, l; double g; };   // 16 bytes: one LDS read per lane
__device__ PrefPair g_pref_pair[PREF_MAX];                              // launch 1 -> launch 2, within one mage_preference_loss call (stream order)
__device__ double g_pref_part[(PREF_MAX / PREF_TILE) * PREF_MEANS];     // a workgroup's five partial sums

struct PrefTerm { double l, g, a, b, u, h; };
__device__ __forceinline__ PrefTerm pref_term(float sw, float rw, float sl, float rl, double beta, double eps, int mode) {
    PrefTerm t;
    t.a = (double)sw - (double)rw;
    t.b = (double)sl - (double)rl;
    t.u = t.a - t.b;
    t.h = beta * t.u;
    if (mode == 1) {                                    // IPO
        const double d = t.u - 1.0 / (2.0 * beta);
        t.l = d * d;
        t.g = 2.0 * d;
        return t;
    }
    const double ah = fabs(t.h), e = exp(-ah), lg = log1p(e);
    const double ls_p = fmin(t.h, 0.0) - lg, ls_n = fmin(-t.h, 0.0) - lg;          // logsig(h), logsig(-h)
    const double sig_big = 1.0 / (1.0 + e), sig_small = e / (1.0 + e);              // sig(|h|), sig(-|h|)
    const double sp = t.h >= 0.0 ? sig_big : sig_small, sn = t.h >= 0.0 ? sig_small : sig_big;   // sig(h), sig(-h)  (a NaN h is NaN in e already)
    if (eps == 0.0) {                                   // the eps term is never formed: no 0 * inf on a saturated pair
        t.l = lg - fmin(t.h, 0.0);                      // -logsig(h), written so that a saturated pair is +0
        t.g = -beta * sn;
    } else {
        t.l = -(1.0 - eps) * ls_p - eps * ls_n;
        t.g = -beta * ((1.0 - eps) * sn - eps * sp);
    }
    return t;
}

__device__ __forceinline__ int pref_index(const int64_t* __restrict__ pairs, long e, long clips, int* err) {
    long c = pairs[e];
    if (c < 0 || c >= clips) {
        mage_raise(err, MAGE_DEVERR_PAIR_ID, c, (int)clips);
        c = c < 0 ? 0 : clips - 1;
    }
    return (int)c;
}

// five fp64 sums of a workgroup in a fixed order: the lanes of a wave meet in an xor butterfly, thread q (< 5) adds the four waves' q-th sums in
// order and returns the total (other threads: 0)
__device__ __forceinline__ double pref_block_sums(double (&t)[PREF_MEANS], double (&red)[4][PREF_MEANS]) {
#pragma unroll
    for (int q = 0; q < PREF_MEANS; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[q] += __shfl_xor(t[q], o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = t[q];
    }
    __syncthreads();
    if (threadIdx.x >= PREF_MEANS) return 0.0;
    const int q = threadIdx.x;
    return ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

// launch 1: one thread per pair
__global__ __launch_bounds__(256) void pref_pair_kernel(const float* __restrict__ s, const float* __restrict__ r, long clips,
                                                        const int64_t* __restrict__ pairs, int P, double beta, double eps, int mode,
                                                        float* __restrict__ pair_loss, float* __restrict__ pair_margin, int* __restrict__ err) {
    __shared__ double red[4][PREF_MEANS];
    const int p = blockIdx.x * PREF_TILE + threadIdx.x;
    double t[PREF_MEANS] = {};
    if (p < P) {
        const int w = pref_index(pairs, 2L * p, clips, err), l = pref_index(pairs, 2L * p + 1, clips, err);
        const PrefTerm v = pref_term(s[w], r[w], s[l], r[l], beta, eps, mode);
        pair_loss[p] = (float)v.l;
        pair_margin[p] = (float)v.h;
        g_pref_pair[p] = PrefPair{w, l, v.g};
        t[0] = v.l;
        t[1] = v.u > 0.0 ? 1.0 : 0.0;
        t[2] = beta * v.a;
        t[3] = beta * v.b;
        t[4] = v.h;
    }
    const double sum = pref_block_sums(t, red);
    if (threadIdx.x < PREF_MEANS) g_pref_part[blockIdx.x * PREF_MEANS + threadIdx.x] = sum;
}

// launch 2: workgroups 0 .. ceil(clips / 256) - 1 own 256 clips each, one per thread; the last workgroup adds launch 1's partial sums.
__global__ __launch_bounds__(256) void pref_coef_kernel(int clips, int P, float* __restrict__ clip_coef, float* __restrict__ summary) {
    __shared__ double red[4][PREF_MEANS];
    __shared__ PrefPair tile[PREF_TILE];
    if (blockIdx.x == gridDim.x - 1) {
        const int nb = (P + PREF_TILE - 1) / PREF_TILE;                 // <= 256: thread t holds workgroup t's sums
        double t[PREF_MEANS];
#pragma unroll
        for (int q = 0; q < PREF_MEANS; ++q) t[q] = (int)threadIdx.x < nb ? g_pref_part[threadIdx.x * PREF_MEANS + q] : 0.0;
        const double sum = pref_block_sums(t, red);
        if (threadIdx.x < PREF_MEANS) summary[threadIdx.x] = (float)(sum / (double)P);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int c0 = __builtin_amdgcn_readfirstlane(c - lane);            // the wave's first clip
    double acc = 0.0;
    for (int p0 = 0; p0 < P; p0 += PREF_TILE) {
        __syncthreads();                                                // the tile before has been read by every wave
        tile[threadIdx.x] = p0 + (int)threadIdx.x < P ? g_pref_pair[p0 + threadIdx.x] : PrefPair{-1, -1, 0.0};
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < PREF_TILE / 64; ++sub) {
            const PrefPair e = tile[sub * 64 + lane];                   // lane j looks at pair p0 + sub*64 + j
            const bool hit = e.w != e.l && ((unsigned)(e.w - c0) < 64u || (unsigned)(e.l - c0) < 64u);
            unsigned long long m = __ballot(hit);                       // the pairs that name one of this wave's clips, in increasing p
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int w = __builtin_amdgcn_readlane(e.w, j), l = __builtin_amdgcn_readlane(e.l, j);
                const double g = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(e.g), j),
                                                  __builtin_amdgcn_readlane(__double2loint(e.g), j));
                if (c == w) acc += g;
                else if (c == l) acc -= g;
            }
        }
    }
    if (c < clips) clip_coef[c] = (float)(acc / (double)P);
}

// ------------------------------------------------------------------------------------------------ weighted log-softmax backward
// The row's NV values of one lane -> dl, chunk by chunk (code k = chunk*256 + lane*4 + e).  fp32: one 16-byte store per quad.  bf16, wide
// (K % 8 == 0: every 8th code is 16-byte aligned): lanes 2m and 2m + 1 hold codes 8m .. 8m + 7 of a chunk between them; of two chunks the
// even lane takes the first (its own quad, then its neighbour's) and the odd lane the second, so each stores 16 bytes per pair of chunks.
// Every lane takes part in the exchange, past K too (what it sends from there is never stored).
template <int NV, typename OT>
__device__ __forceinline__ void logprob_bwd_store(OT* __restrict__ o, int lane, int K, const float (&d)[NV], bool wide) {
    if constexpr (sizeof(OT) == 4) {
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) {
            const int k = c * 256 + lane * 4;
            if (k < K) store4(o + k, f32x4{d[c * 4], d[c * 4 + 1], d[c * 4 + 2], d[c * 4 + 3]});
        }
    } else {
        if (!wide) {
#pragma unroll
            for (int c = 0; c < NV / 4; ++c) {
                const int k = c * 256 + lane * 4;
                if (k < K) store4(o + k, f32x4{d[c * 4], d[c * 4 + 1], d[c * 4 + 2], d[c * 4 + 3]});
            }
            return;
        }
        const bool odd = lane & 1;
        uint2 q[NV / 4];
#pragma unroll
        for (int c = 0; c < NV / 4; ++c) q[c] = uint2{pack_bf16x2(d[c * 4], d[c * 4 + 1]), pack_bf16x2(d[c * 4 + 2], d[c * 4 + 3])};
#pragma unroll
        for (int c = 0; c + 1 < NV / 4; c += 2) {
            const uint2 send = odd ? q[c] : q[c + 1];
            const uint2 recv = uint2{(unsigned)__shfl_xor((int)send.x, 1, 64), (unsigned)__shfl_xor((int)send.y, 1, 64)};
            const int k = (odd ? c + 1 : c) * 256 + (lane & ~1) * 4;     // eight codes from k: k % 8 == 0, so k < K means k + 8 <= K
            const uint4 v = odd ? uint4{recv.x, recv.y, q[c + 1].x, q[c + 1].y} : uint4{q[c].x, q[c].y, recv.x, recv.y};
            if (k < K) *(uint4*)(o + k) = v;
        }
        if constexpr ((NV / 4) % 2 == 1) {                               // NV = 4: one chunk, the even lanes store it
            constexpr int c = NV / 4 - 1;
            const uint2 recv = uint2{(unsigned)__shfl_xor((int)q[c].x, 1, 64), (unsigned)__shfl_xor((int)q[c].y, 1, 64)};
            const int k = c * 256 + lane * 4;
            if (!odd && k < K) *(uint4*)(o + k) = uint4{q[c].x, q[c].y, recv.x, recv.y};
        }
    }
}

// dlogits_ij = c_i (1[j = t] - p_ij): token_logprob_kernel's maximum and sum (row_logsumexp, token_row.h), ce_bwd_kernel's
// p = expf(z - max) * (1 / sum) (train.hip).  c_i == 0: the row is zeros and its logits are not read.
template <int NV, typename OT>
__global__ __launch_bounds__(256) void token_logprob_bwd_kernel(const float* __restrict__ logits, long rows, int K, long ld,
                                                                const int64_t* __restrict__ tokens, const float* __restrict__ weight,
                                                                long weight_div, const float* __restrict__ gout, OT* __restrict__ dl, bool wide,
                                                                const uint8_t* __restrict__ given) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    OT* o = dl + i * (long)K;
    // (mage_token_logprob_bwd_masked: a given row is a row of c_i == 0; a null mask, the unmasked entry point, has none)
    const float ci = row_given(given, i) ? 0.f : __fmul_rn(gout[0], weight[i / weight_div]);
    float d[NV];
    if (ci == 0.f) {                                    // (wave-uniform)
#pragma unroll
        for (int e = 0; e < NV; ++e) d[e] = 0.f;
        logprob_bwd_store<NV, OT>(o, lane, K, d, wide);
        return;
    }
    const float* p = logits + i * ld;
    const float inv = 1.0f / row_logsumexp<NV>([=](int c) { return row_chunk_inf(p, lane, K, c); }, d).zs;
    const long tg = row_token<false>(tokens, i, K, nullptr);            // (a bad token: no one-hot; mage_token_logprob, which ran before, reported it)
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int k = (e >> 2) * 256 + lane * 4 + (e & 3);
        d[e] = __fmul_rn(ci, (k == tg ? 1.f : 0.f) - __fmul_rn(d[e], inv));
    }
    logprob_bwd_store<NV, OT>(o, lane, K, d, wide);
}

}  // namespace

extern "C" int mage_preference_loss(const float* clip_logprob, const float* reference_logprob, int64_t clips, const int64_t* pairs,
                                    int64_t n_pairs, float beta, float label_smoothing, int32_t mode, float* pair_loss, float* pair_margin,
                                    float* clip_coef, float* summary, void* stream) {
    MAGE_CHECK_ARG(clip_logprob && reference_logprob && pairs && pair_loss && pair_margin && clip_coef && summary,
                   "mage_preference_loss: null pointer");
    MAGE_CHECK_ARG(((((uintptr_t)clip_logprob) | ((uintptr_t)reference_logprob) | ((uintptr_t)pair_loss) | ((uintptr_t)pair_margin) |
                     ((uintptr_t)clip_coef) | ((uintptr_t)summary)) & 3) == 0 && (((uintptr_t)pairs) & 7) == 0,
                   "mage_preference_loss: a pointer is not aligned to its element size (fp32: 4 bytes, pairs: 8)");
    MAGE_CHECK_ARG(clips >= 1 && clips <= PREF_MAX && n_pairs >= 1 && n_pairs <= PREF_MAX,
                   "mage_preference_loss: clips=%ld and n_pairs=%ld must lie in [1, %d]", (long)clips, (long)n_pairs, (int)PREF_MAX);
    MAGE_CHECK_ARG(mode == 0 || mode == 1, "mage_preference_loss: mode=%d must be 0 (DPO) or 1 (IPO)", mode);
    MAGE_CHECK_ARG(__builtin_isfinite(beta) && beta > 0.f && __builtin_isfinite(1.0 / (2.0 * (double)beta)),
                   "mage_preference_loss: beta=%g must be finite and > 0", (double)beta);
    MAGE_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 0.5f, "mage_preference_loss: label_smoothing=%g outside [0, 0.5)",
                   (double)label_smoothing);
    MAGE_CHECK_ARG(mode == 0 || label_smoothing == 0.f, "mage_preference_loss: label_smoothing=%g must be 0 in mode 1 (IPO)",
                   (double)label_smoothing);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_preference_loss: mage_init() has not been called");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pref_pair_kernel, dim3((unsigned)((n_pairs + PREF_TILE - 1) / PREF_TILE)), dim3(256), 0, s, clip_logprob,
                       reference_logprob, (long)clips, pairs, (int)n_pairs, (double)beta, (double)label_smoothing, mode, pair_loss, pair_margin,
                       err);
    hipLaunchKernelGGL(pref_coef_kernel, dim3((unsigned)((clips + 255) / 256) + 1), dim3(256), 0, s, (int)clips, (int)n_pairs, clip_coef,
                       summary);
    MAGE_CHECK_LAUNCH("mage_preference_loss");
    return MAGE_OK;
}

// mage_token_logprob_bwd (given null) and mage_token_logprob_bwd_masked behind one set of argument rules
static int token_logprob_backward(const char* who, const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens,
                                  const float* weight, int64_t weight_div, const float* grad_out, void* dlogits, int32_t dl_dtype,
                                  const uint8_t* given, void* stream) {
    MAGE_CHECK_ARG(logits && tokens && weight && grad_out && dlogits, "%s: null pointer", who);
    if (int rc = token_rows_check(who, logits, rows, K, ld, (((uintptr_t)dlogits) & 15) == 0, "weight_div", weight_div)) return rc;
    MAGE_CHECK_ARG((((uintptr_t)tokens) & 7) == 0 && ((((uintptr_t)weight) | ((uintptr_t)grad_out)) & 3) == 0,
                   "%s: tokens must be 8-byte, weight and grad_out 4-byte aligned", who);
    MAGE_CHECK_ARG(dl_dtype == MAGE_F32 || dl_dtype == MAGE_BF16, "%s: bad dtype %d", who, dl_dtype);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const bool wide = K % 8 == 0;
#define MAGE_LPB(NV, OT)                                                                                                                \
    hipLaunchKernelGGL((token_logprob_bwd_kernel<NV, OT>), grid, dim3(256), 0, s, logits, (long)rows, K, (long)ld, tokens, weight,   \
                       (long)weight_div, grad_out, (OT*)dlogits, wide, given)
#define MAGE_LPB_NV(NV)                                  \
    do {                                                 \
        if (dl_dtype == MAGE_F32) MAGE_LPB(NV, float);   \
        else MAGE_LPB(NV, unsigned short);               \
    } while (0)
    MAGE_ROW_LADDER(K, MAGE_LPB_NV);
#undef MAGE_LPB_NV
#undef MAGE_LPB
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

extern "C" int mage_token_logprob_bwd(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* weight,
                                      int64_t weight_div, const float* grad_out, void* dlogits, int32_t dl_dtype, void* stream) {
    return token_logprob_backward("mage_token_logprob_bwd", logits, rows, K, ld, tokens, weight, weight_div, grad_out, dlogits, dl_dtype, nullptr,
                                  stream);
}

extern "C" int mage_token_logprob_bwd_masked(const float* logits, int64_t rows, int32_t K, int64_t ld, const int64_t* tokens, const float* weight,
                                             int64_t weight_div, const float* grad_out, void* dlogits, int32_t dl_dtype, const uint8_t* given,
                                             void* stream) {
    MAGE_CHECK_ARG(given != nullptr, "mage_token_logprob_bwd_masked: given must not be null (mage_token_logprob_bwd takes no mask)");
    return token_logprob_backward("mage_token_logprob_bwd_masked", logits, rows, K, ld, tokens, weight, weight_div, grad_out, dlogits, dl_dtype,
                                  given, stream);
}
