// Row-wise glue, HBM-bound: fp32 rows to split-precision rows, the speed-embedding add and the row affine, the caption mask, the strided
// block copy; and the two small losses (reparameterisation + KL of the randomness branch, the mean squared error of the MAGE+ latent), each
// beside its backward.
#include "common.h"

// ------------------------------------------------------------------------------------ fp32 rows -> split-precision rows
namespace {
template <typename OT>
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ x, long ldx, OT* __restrict__ y, long ldy, long rows, int C) {
    const int vpr = C >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * vpr) return;
    const long r = i / vpr;
    const int c = (int)(i - r * vpr) << 2;
    store4(y + r * ldy + c, *(const f32x4*)(x + r * ldx + c));
}
}  // namespace

namespace {
template <typename OT>
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ x, long ldx, OT* __restrict__ y, long rows, int C, int relu,
                                                         long group, long group_stride, long off, long inner, long inner_stride,
                                                         float* __restrict__ x_relu) {
    const int vpr = C >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * vpr) return;
    const long r = i / vpr;
    const int c = (int)(i - r * vpr) << 2;
    f32x4 v = *(const f32x4*)(x + r * ldx + c);
    if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    if (x_relu) *(f32x4*)(x_relu + r * ldx + c) = v;
    const long ig = r % group;
    const long orow = (r / group) * group_stride + (ig / inner) * inner_stride + (ig % inner) + off;
    store4(y + orow * C + c, v);
}
}  // namespace

extern "C" int mage_split_rows(const float* x, int64_t ldx, void* y, int64_t rows, int32_t C, int32_t kind, int32_t relu, int64_t group,
                               int64_t group_stride, int64_t off, int64_t inner, int64_t inner_stride, float* x_relu, void* stream) {
    MAGE_CHECK_ARG(x && y && rows > 0 && C > 0 && C % 64 == 0 && ldx % 4 == 0 && group > 0, "mage_split_rows: C=%d must be a multiple of 64", C);
    MAGE_CHECK_ARG(((((uintptr_t)y) & 255) | (((uintptr_t)x) & 15)) == 0, "mage_split_rows: y must be 256-byte aligned, x 16-byte aligned");
    MAGE_CHECK_ARG(kind == MAGE_BF16X3 || kind == MAGE_F16X3, "mage_split_rows: kind %d is not a split kind", kind);
    if (inner <= 0) {
        inner = group;
        inner_stride = group;
    }
    const dim3 grid((unsigned)((rows * (C >> 2) + 255) / 256));
    if (kind == MAGE_BF16X3)
        hipLaunchKernelGGL((split_rows_kernel<split_bf16>), grid, dim3(256), 0, (hipStream_t)stream, x, (long)ldx, (split_bf16*)y, (long)rows, C, relu,
                           (long)group, (long)group_stride, (long)off, (long)inner, (long)inner_stride, x_relu);
    else
        hipLaunchKernelGGL((split_rows_kernel<split_f16>), grid, dim3(256), 0, (hipStream_t)stream, x, (long)ldx, (split_f16*)y, (long)rows, C, relu,
                           (long)group, (long)group_stride, (long)off, (long)inner, (long)inner_stride, x_relu);
    MAGE_CHECK_LAUNCH("mage_split_rows");
    return MAGE_OK;
}

extern "C" int mage_split(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t C, int32_t kind, void* stream) {
    MAGE_CHECK_ARG(x && y && rows > 0 && C > 0 && C % 64 == 0 && ldx % 4 == 0 && ldy % 128 == 0 && ldy >= 2 * (int64_t)C,
                   "mage_split: C=%d must be a multiple of 64, ldy a multiple of 128 16-bit elements (>= 2C)", C);
    MAGE_CHECK_ARG(((((uintptr_t)y) & 255) | (((uintptr_t)x) & 15)) == 0, "mage_split: y must be 256-byte aligned, x 16-byte aligned");
    MAGE_CHECK_ARG(kind == MAGE_BF16X3 || kind == MAGE_F16X3, "mage_split: kind %d is not a split kind", kind);
    const dim3 grid((unsigned)((rows * (C >> 2) + 255) / 256));
    if (kind == MAGE_BF16X3)
        hipLaunchKernelGGL((split_kernel<split_bf16>), grid, dim3(256), 0, (hipStream_t)stream, x, (long)ldx, (split_bf16*)y, (long)(ldy >> 1), (long)rows, C);
    else
        hipLaunchKernelGGL((split_kernel<split_f16>), grid, dim3(256), 0, (hipStream_t)stream, x, (long)ldx, (split_f16*)y, (long)(ldy >> 1), (long)rows, C);
    MAGE_CHECK_LAUNCH("mage_split");
    return MAGE_OK;
}

namespace {
__global__ void add_scaled_rowvec_kernel(float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ vec,
                                         long per_b, int C, long total) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
    const long b = i / per_b;
    const int c = (int)(i % C);
    f32x4 v = *(f32x4*)(x + i);
    v += s[b] * *(const f32x4*)(vec + c);
    *(f32x4*)(x + i) = v;
}

__global__ void row_affine_kernel(float* __restrict__ x, const float* __restrict__ rs, const float* __restrict__ table,
                                  long rows, int C, int div, int mod) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= rows * C) return;
    const long r = i / C;
    const int c = (int)(i - r * C);
    f32x4 v = *(f32x4*)(x + i);
    if (rs) v *= rs[r];
    if (table) v += *(const f32x4*)(table + ((r / div) % mod) * (long)C + c);
    *(f32x4*)(x + i) = v;
}
}  // namespace

extern "C" int mage_add_scaled_rowvec(float* x, const float* s, const float* vec, int32_t B, int32_t P, int32_t C,
                                      void* stream) {
    MAGE_CHECK_ARG(x && s && vec, "mage_add_scaled_rowvec: null pointer");
    MAGE_CHECK_ARG(B > 0 && P > 0 && C > 0 && C % 4 == 0, "mage_add_scaled_rowvec: C=%d must be a multiple of 4", C);
    const long total = (long)B * P * C;
    hipLaunchKernelGGL(add_scaled_rowvec_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, x, s, vec, (long)P * C, C, total);
    MAGE_CHECK_LAUNCH("mage_add_scaled_rowvec");
    return MAGE_OK;
}

extern "C" int mage_row_affine(float* x, const float* rs, const float* table, int64_t rows, int32_t C, int32_t div, int32_t mod,
                               void* stream) {
    MAGE_CHECK_ARG(x && rows > 0 && C > 0 && C % 4 == 0, "mage_row_affine: bad arguments");
    MAGE_CHECK_ARG(!table || (div >= 1 && mod >= 1), "mage_row_affine: bad div/mod");
    const long total = (long)rows * C;
    hipLaunchKernelGGL(row_affine_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, rs,
                       table, (long)rows, C, div, mod);
    MAGE_CHECK_LAUNCH("mage_row_affine");
    return MAGE_OK;
}

// Caption bookkeeping of the text encoder in one launch (mage_model.py:233-239: `text != padding_idx`, its row sums): keep[b*S + s] = 1.0 where
// ids[b][s] != padding_idx else 0.0 (the row scale that zeroes padded rows), kv_len[b] = number of kept tokens (the key-padding length).
namespace {
__global__ __launch_bounds__(64) void caption_mask_kernel(const int64_t* __restrict__ ids, int S, long padding_idx, int* __restrict__ kv_len,
                                                          float* __restrict__ keep) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int cnt = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool k = s < S && ids[(long)b * S + s] != padding_idx;
        if (s < S && keep) keep[(long)b * S + s] = k ? 1.0f : 0.0f;
        cnt += __popcll(__ballot(k));
    }
    if (lane == 0 && kv_len) kv_len[b] = cnt;
}
}  // namespace

extern "C" int mage_caption_mask(const int64_t* ids, int32_t B, int32_t S, int64_t padding_idx, int32_t* kv_len, float* keep, void* stream) {
    MAGE_CHECK_ARG(ids && B > 0 && S > 0 && (kv_len || keep), "mage_caption_mask: bad arguments");
    hipLaunchKernelGGL(caption_mask_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, ids, S, (long)padding_idx, kv_len, keep);
    MAGE_CHECK_LAUNCH("mage_caption_mask");
    return MAGE_OK;
}

// Strided block copy on the stream (hipMemcpy2DAsync, device to device): `height` rows of `width_bytes`, row pitches in bytes.  Output
// assembly without a compute kernel: the passed-through first frame and the decoded frames into the [B, L, C, H, W] result (mage_model.py:691).
extern "C" int mage_copy2d(void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width_bytes, int64_t height, void* stream) {
    MAGE_CHECK_ARG(dst && src && width_bytes > 0 && height > 0 && dst_pitch >= width_bytes && src_pitch >= width_bytes, "mage_copy2d: bad arguments");
    const hipError_t e = hipMemcpy2DAsync(dst, (size_t)dst_pitch, src, (size_t)src_pitch, (size_t)width_bytes, (size_t)height, hipMemcpyDeviceToDevice,
                                          (hipStream_t)stream);
    if (e != hipSuccess) {
        mage_set_error("mage_copy2d: %s", hipGetErrorString(e));
        return MAGE_EHIP;
    }
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------ reparameterisation + KL summand
namespace {
__global__ __launch_bounds__(256) void reparam_kl_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                         const float* __restrict__ eps, float* __restrict__ out,
                                                         float* __restrict__ kl_sum, long n) {
    __shared__ double red[4];
    const long base = (long)blockIdx.x * n;
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float m = mu[base + i], lv = logvar[base + i];
        out[base + i] = eps[base + i] * expf(0.5f * lv) + m;
        acc += (double)(1.0f + lv - m * m - expf(lv));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) kl_sum[blockIdx.x] = (float)(red[0] + red[1] + red[2] + red[3]);
}
}  // namespace

extern "C" int mage_reparam_kl(const float* mu, const float* logvar, const float* eps, float* out, float* kl_sum, int32_t B,
                               int64_t n, void* stream) {
    MAGE_CHECK_ARG(mu && logvar && eps && out && kl_sum && B > 0 && n > 0, "mage_reparam_kl: bad arguments");
    hipLaunchKernelGGL(reparam_kl_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mu, logvar, eps, out, kl_sum, (long)n);
    MAGE_CHECK_LAUNCH("mage_reparam_kl");
    return MAGE_OK;
}

namespace {
// z = eps exp(logvar / 2) + mu; kl = -1/2 mean_b sum(1 + logvar - mu^2 - exp(logvar)).  With dz and c = dL/dkl / B:
//   dmu = dz + c mu,  dlogvar = dz eps exp(logvar / 2) / 2 - c (1 - exp(logvar)) / 2
__global__ void reparam_kl_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ logvar, const float* __restrict__ eps,
                                      const float* __restrict__ dz, const float* __restrict__ coef, float* __restrict__ dmu,
                                      float* __restrict__ dlogvar, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float c = coef[0], lv = logvar[i];
    dmu[i] = dz[i] + c * mu[i];
    dlogvar[i] = 0.5f * dz[i] * eps[i] * expf(0.5f * lv) - 0.5f * c * (1.0f - expf(lv));
}
}  // namespace

extern "C" int mage_reparam_kl_bwd(const float* mu, const float* logvar, const float* eps, const float* dz, const float* coef, float* dmu,
                                   float* dlogvar, int64_t n, void* stream) {
    MAGE_CHECK_ARG(mu && logvar && eps && dz && coef && dmu && dlogvar && n > 0, "mage_reparam_kl_bwd: bad arguments");
    hipLaunchKernelGGL(reparam_kl_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mu, logvar, eps, dz, coef, dmu,
                       dlogvar, (long)n);
    MAGE_CHECK_LAUNCH("mage_reparam_kl_bwd");
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------ mean squared error (MAGE+ latent loss)
namespace {
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb,
                                                          long rows, int cols, double* __restrict__ partial) {
    __shared__ double red[4];
    double acc = 0.0;
    const long total = rows * cols;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / cols;
        const int c = (int)(i - r * cols);
        const float dlt = a[r * lda + c] - b[r * ldb + c];
        acc += (double)(dlt * dlt);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void mse_final_kernel(const double* __restrict__ partial, int n, double inv_count, float* __restrict__ out) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += partial[i];          // fixed order: deterministic
    out[0] = (float)(s * inv_count);
}
}  // namespace

extern "C" int mage_mse(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t cols, double* workspace,
                        float* out, void* stream) {
    MAGE_CHECK_ARG(a && b && workspace && out && rows > 0 && cols > 0, "mage_mse: bad arguments");
    MAGE_CHECK_ARG(lda >= cols && ldb >= cols, "mage_mse: lda=%ld ldb=%ld must be at least cols=%d", (long)lda, (long)ldb, cols);
    const int nblk = (int)((rows * cols + 255) / 256 < 256 ? (rows * cols + 255) / 256 : 256);
    hipLaunchKernelGGL(mse_partial_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, a, (long)lda, b, (long)ldb, (long)rows, cols,
                       workspace);
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, workspace, nblk, 1.0 / ((double)rows * cols), out);
    MAGE_CHECK_LAUNCH("mage_mse");
    return MAGE_OK;
}

// d mean((a - b)^2) / da = 2 (a - b) / (rows * cols) * gout for the first `cols` columns of each row of a (row stride lda), zero for the
// padding columns up to ld_da (F.mse_loss of the MAGE+ latent prediction, mage_model.py:620).
namespace {
__global__ void mse_bwd_kernel(const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb, long rows, int cols,
                               const float* __restrict__ gout, float* __restrict__ da, long ld_da, float inv_n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ld_da) return;
    const long r = i / ld_da;
    const int c = (int)(i - r * ld_da);
    da[i] = c < cols ? 2.0f * (a[r * lda + c] - b[r * ldb + c]) * inv_n * gout[0] : 0.f;
}
}  // namespace

extern "C" int mage_mse_bwd(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t cols, const float* gout, float* da,
                            int64_t ld_da, void* stream) {
    MAGE_CHECK_ARG(a && b && gout && da && rows > 0 && cols > 0 && ld_da >= cols, "mage_mse_bwd: bad arguments");
    MAGE_CHECK_ARG(lda >= cols && ldb >= cols, "mage_mse_bwd: lda=%ld ldb=%ld must be at least cols=%d", (long)lda, (long)ldb, cols);
    const long n = rows * ld_da;
    hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, (long)lda, b, (long)ldb, (long)rows,
                       cols, gout, da, (long)ld_da, (float)(1.0 / ((double)rows * cols)));
    MAGE_CHECK_LAUNCH("mage_mse_bwd");
    return MAGE_OK;
}
