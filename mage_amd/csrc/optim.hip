// FlatAdam's kernels: the Adam update of a flat arena (mage_adam; clipped by the global gradient norm; guarded: non-finite steps skipped,
// decoupled weight decay, EMA weights) and the two-stage sum of squares the norm comes from (mage_sumsq).  Fixed summation orders:
// deterministic.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ Adam
// torch.optim.Adam semantics (main_mage.py:121: betas (0.9, 0.98), eps 1e-6, no weight decay, no amsgrad):
//   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// One element: the one statement of the update, shared by adam_kernel, adam_clipped_kernel and adam_guarded_kernel so that equal scales
// give equal bits.  A macro, not a function: which of the two products of `a * x + b * y` the compiler fuses into the addition is its
// choice per use site (the vector path, the two-wide loop it makes of the tail and that loop's remainder choose differently), and it
// follows the shape of the code around the statement -- an inlined function taking references moved it in the tail.  The expansion is the
// text the kernels have always had; P, M, V are lvalues, and lr, b1, b2, eps, bc1, bc2_sqrt are taken from the scope.
#define ADAM_ELEMENT(P, G, M, V, SCALE)                                   \
    const float ge = (G) * (SCALE);                                       \
    (M) = b1 * (M) + (1.f - b1) * ge;                                     \
    (V) = b2 * (V) + (1.f - b2) * ge * ge;                                \
    (P) -= (lr / bc1) * ((M) / (sqrtf(V) / bc2_sqrt + eps));

// the four (or fewer, at the arena's tail) elements from index i on
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            long n, long i, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                            float grad_scale) {
    if (i + 4 <= n) {
        f32x4 pp = *(f32x4*)(p + i), gg = *(const f32x4*)(g + i), mm = *(f32x4*)(m + i), vv = *(f32x4*)(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ADAM_ELEMENT(pp[e], gg[e], mm[e], vv[e], grad_scale)
        }
        *(f32x4*)(p + i) = pp;
        *(f32x4*)(m + i) = mm;
        *(f32x4*)(v + i) = vv;
    } else {
        for (long j = i; j < n; ++j) {
            ADAM_ELEMENT(p[j], g[j], m[j], v[j], grad_scale)
        }
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                   float bc1, float bc2_sqrt, float grad_scale) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    adam_update(p, g, m, v, n, i, lr, b1, b2, eps, bc1, bc2_sqrt, grad_scale);
}

// mage_adam_clipped (include/mage_hip_ext.h): every thread derives the one scale from the one device value *sumsq -- the
// clip_grad_norm_ rule on the averaged gradient -- and where the norm is within the limit the scale IS grad_scale, so the update is
// adam_kernel's bit for bit.  A NaN norm fails the >= test and becomes the scale: it reaches every parameter, as clip_grad_norm_'s does.
__global__ __launch_bounds__(256) void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                           float bc1, float bc2_sqrt, float grad_scale, const double* __restrict__ sumsq,
                                                           float max_norm, float* __restrict__ norm_out) {
    const double norm = sqrt(sumsq[0]) * (double)grad_scale;
    const double coef = (double)max_norm / (norm + 1e-6);
    const float scale = coef >= 1.0 ? grad_scale : (float)((double)grad_scale * coef);
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = (float)norm;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    adam_update(p, g, m, v, n, i, lr, b1, b2, eps, bc1, bc2_sqrt, scale);
}

// mage_adam_guarded (include/mage_hip_ext.h): adam_clipped_kernel's scale from the one device value *sumsq, and around the shared update
// statement a skip of the whole step when *sumsq is not finite (every thread returns before it loads anything; one thread counts the skip),
// AdamW's decoupled decay of the elements below n_decay (p * decay_mul, rounded on its own, before the update) and an exponential moving
// average of the updated parameter, taken from the register on the vector path.  One instance per (EMA, DECAY): the plain form loads and
// tests nothing extra.
template <bool EMA, bool DECAY>
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ ema, long n, long n_decay, float lr,
                                                           float b1, float b2, float eps, float bc1, float bc2_sqrt, float grad_scale,
                                                           float decay_mul, float ema_decay, const double* __restrict__ sumsq, float max_norm,
                                                           int skip_nonfinite, float* __restrict__ norm_out, long long* __restrict__ skipped) {
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    float scale = grad_scale;
    if (sumsq) {
        const double ss = sumsq[0];
        const double norm = sqrt(ss) * (double)grad_scale;
        if (norm_out && first) norm_out[0] = (float)norm;
        if (skip_nonfinite && !__builtin_isfinite(ss)) {
            if (skipped && first) skipped[0] += 1;
            return;
        }
        if (max_norm > 0.f) {
            const double coef = (double)max_norm / (norm + 1e-6);
            scale = coef >= 1.0 ? grad_scale : (float)((double)grad_scale * coef);
        }
    }
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float ema_in = __fsub_rn(1.f, ema_decay);
    if (i + 4 <= n) {
        f32x4 pp = *(f32x4*)(p + i), gg = *(const f32x4*)(g + i), mm = *(f32x4*)(m + i), vv = *(f32x4*)(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (DECAY && i + e < n_decay) pp[e] = __fmul_rn(pp[e], decay_mul);
            ADAM_ELEMENT(pp[e], gg[e], mm[e], vv[e], scale)
        }
        *(f32x4*)(p + i) = pp;
        *(f32x4*)(m + i) = mm;
        *(f32x4*)(v + i) = vv;
        if (EMA) {
            f32x4 aa = *(f32x4*)(ema + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) aa[e] = __fmaf_rn(ema_decay, aa[e], __fmul_rn(ema_in, pp[e]));
            *(f32x4*)(ema + i) = aa;
        }
    } else {
        // the arena's last one to three elements, once per launch: the decay and the EMA in loops of their own around adam_update's own tail
        // loop, so that the update between them is compiled as it is in the other two kernels (here p passes through the thread's own store)
        if (DECAY)
            for (long j = i; j < n && j < n_decay; ++j) p[j] = __fmul_rn(p[j], decay_mul);
        adam_update(p, g, m, v, n, i, lr, b1, b2, eps, bc1, bc2_sqrt, scale);
        if (EMA)
            for (long j = i; j < n; ++j) ema[j] = __fmaf_rn(ema_decay, ema[j], __fmul_rn(ema_in, p[j]));
    }
}

// mage_sumsq, stage 1 of 2: workgroup b owns elements [b * chunk, (b + 1) * chunk) and leaves their sum of squares in g_sumsq_part[b].
// Scalar loads only, indexed from g: nothing depends on the pointer's alignment.  A thread squares in fp64 (exact for fp32 values) and adds
// its elements r0 + t, r0 + t + 256, ... into four accumulators in turn (they meet as ((a0 + a1) + a2) + a3), the lanes meet in an xor
// butterfly, thread 0 adds the four waves in order: a fixed order.
enum { SUMSQ_PARTS = 2048 };
__device__ double g_sumsq_part[SUMSQ_PARTS];            // stage 1 -> stage 2, within one mage_sumsq call (stream order)
__global__ __launch_bounds__(256) void sumsq_part_kernel(const float* __restrict__ g, long n, long chunk) {
    __shared__ double red[4];
    const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    long i = r0 + threadIdx.x;
    for (; i + 768 < r1; i += 1024) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double x = (double)g[i + e * 256];
            a[e] += x * x;
        }
    }
    for (int e = 0; i < r1; i += 256, ++e) {
        const double x = (double)g[i];
        a[e] += x * x;
    }
    double t = ((a[0] + a[1]) + a[2]) + a[3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) g_sumsq_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// stage 2: thread t adds partials t * 8 .. t * 8 + 7 in order; the same butterfly and wave order
__global__ __launch_bounds__(256) void sumsq_final_kernel(double* __restrict__ out) {
    __shared__ double red[4];
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < SUMSQ_PARTS / 256; ++e) t += g_sumsq_part[threadIdx.x * (SUMSQ_PARTS / 256) + e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

extern "C" int mage_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         int32_t step, float grad_scale, void* stream) {
    MAGE_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "mage_adam: bad arguments");
    MAGE_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "mage_adam: arenas must be 16-byte aligned");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr, beta1,
                       beta2, eps, bc1, bc2_sqrt, grad_scale);
    MAGE_CHECK_LAUNCH("mage_adam");
    return MAGE_OK;
}

extern "C" int mage_sumsq(const float* g, int64_t n, double* out, void* stream) {
    MAGE_CHECK_ARG(g && out && n > 0, "mage_sumsq: null pointer or n=%ld <= 0", (long)n);
    MAGE_CHECK_ARG((((uintptr_t)g) & 3) == 0 && (((uintptr_t)out) & 7) == 0, "mage_sumsq: g must be 4-byte and out 8-byte aligned");
    hipLaunchKernelGGL(sumsq_part_kernel, dim3(SUMSQ_PARTS), dim3(256), 0, (hipStream_t)stream, g, (long)n,
                       (long)((n + SUMSQ_PARTS - 1) / SUMSQ_PARTS));
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out);
    MAGE_CHECK_LAUNCH("mage_sumsq");
    return MAGE_OK;
}

extern "C" int mage_adam_clipped(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                 int32_t step, float grad_scale, const double* sumsq, float max_norm, float* norm_out, void* stream) {
    MAGE_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "mage_adam_clipped: bad arguments");
    MAGE_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "mage_adam_clipped: arenas must be 16-byte aligned");
    MAGE_CHECK_ARG(sumsq && (((uintptr_t)sumsq) & 7) == 0 && (((uintptr_t)norm_out) & 3) == 0,
                   "mage_adam_clipped: sumsq must be an 8-byte aligned pointer, norm_out null or 4-byte aligned");
    MAGE_CHECK_ARG(__builtin_isfinite(max_norm) && max_norm > 0.f, "mage_adam_clipped: max_norm=%g must be finite and > 0", (double)max_norm);
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adam_clipped_kernel, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr,
                       beta1, beta2, eps, bc1, bc2_sqrt, grad_scale, sumsq, max_norm, norm_out);
    MAGE_CHECK_LAUNCH("mage_adam_clipped");
    return MAGE_OK;
}

extern "C" int mage_adam_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t n, int64_t n_decay, float lr, float beta1,
                                 float beta2, float eps, int32_t step, float grad_scale, float decay_mul, float ema_decay, const double* sumsq,
                                 float max_norm, int32_t skip_nonfinite, float* norm_out, int64_t* skipped, void* stream) {
    MAGE_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "mage_adam_guarded: bad arguments");
    MAGE_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
                   "mage_adam_guarded: arenas (and ema, when given) must be 16-byte aligned");
    MAGE_CHECK_ARG(n_decay >= 0 && n_decay <= n, "mage_adam_guarded: n_decay=%ld outside [0, n=%ld]", (long)n_decay, (long)n);
    MAGE_CHECK_ARG(__builtin_isfinite(decay_mul) && decay_mul > 0.f && decay_mul <= 1.f, "mage_adam_guarded: decay_mul=%g must lie in (0, 1]",
                   (double)decay_mul);
    MAGE_CHECK_ARG(!ema || (ema_decay > 0.f && ema_decay < 1.f), "mage_adam_guarded: ema_decay=%g must lie in (0, 1)", (double)ema_decay);
    MAGE_CHECK_ARG(__builtin_isfinite(max_norm) && max_norm >= 0.f, "mage_adam_guarded: max_norm=%g must be finite and >= 0", (double)max_norm);
    MAGE_CHECK_ARG(sumsq || !(max_norm > 0.f || skip_nonfinite), "mage_adam_guarded: max_norm > 0 and skip_nonfinite need sumsq");
    MAGE_CHECK_ARG((((uintptr_t)sumsq) & 7) == 0 && (((uintptr_t)skipped) & 7) == 0 && (((uintptr_t)norm_out) & 3) == 0,
                   "mage_adam_guarded: sumsq and skipped must be 8-byte aligned (or null), norm_out null or 4-byte aligned");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    const dim3 grid((unsigned)((n / 4 + 256) / 256)), blk(256);
#define GUARDED(E, D)                                                                                                                       \
    hipLaunchKernelGGL((adam_guarded_kernel<E, D>), grid, blk, 0, (hipStream_t)stream, p, g, m, v, ema, (long)n, (long)n_decay, lr, beta1,  \
                       beta2, eps, bc1, bc2_sqrt, grad_scale, decay_mul, ema_decay, sumsq, max_norm, (int)skip_nonfinite, norm_out,         \
                       (long long*)skipped)
    if (ema && n_decay > 0) GUARDED(true, true);
    else if (ema) GUARDED(true, false);
    else if (n_decay > 0) GUARDED(false, true);
    else GUARDED(false, false);
#undef GUARDED
    MAGE_CHECK_LAUNCH("mage_adam_guarded");
    return MAGE_OK;
}
