// The normalisations, each forward beside its backward: LayerNorm (with the dropout + residual + LayerNorm pass of a transformer block and
// the statistics passes that feed the Linear prologues), GroupNorm, ADAIN, BatchNorm on batch statistics.
// All HBM-bound; LayerNorm: one pass over the data, 16-byte vector accesses, fp32 arithmetic.  The backward kernels' per-workgroup partial
// sums are added in a fixed order by mage_sum_partials (train.hip): deterministic.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------ LayerNorm
// One wave per row; two-pass (mean, then centred variance) entirely in registers.
template <typename OT, int VPL>   // VPL = float4 vectors per lane (C <= 256*VPL)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, OT* __restrict__ y, long rows,
                                                        int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        v[j] = (c < C) ? *(const f32x4*)(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        if (c < C) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dlt = v[j][e] - mean;
                q += dlt * dlt;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    OT* yr = y + row * C;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        if (c < C) {
            const f32x4 gm = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[j][e] - mean) * rstd * gm[e] + bt[e];
            store4(yr + c, o);
        }
    }
}

template <typename OT>
int ln_launch(const float* x, const float* g, const float* b, void* y, int64_t rows, int C, float eps, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    ln_vpl(C, [&](auto V) {
        hipLaunchKernelGGL((layernorm_kernel<OT, decltype(V)::value>), grid, blk, 0, s, x, g, b, (OT*)y, (long)rows, C, eps);
    });
    MAGE_CHECK_LAUNCH("mage_layernorm");
    return MAGE_OK;
}

}  // namespace

extern "C" int mage_layernorm(const float* x, const float* gamma, const float* beta, void* y, int32_t y_dtype,
                              int64_t rows, int32_t C, float eps, void* stream) {
    MAGE_CHECK_ARG(x && gamma && beta && y, "mage_layernorm: null pointer");
    MAGE_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0 && C <= 2048, "mage_layernorm: rows=%ld C=%d unsupported", (long)rows, C);
    if (y_dtype == MAGE_F32) return ln_launch<float>(x, gamma, beta, y, rows, C, eps, (hipStream_t)stream);
    if (y_dtype == MAGE_BF16) return ln_launch<unsigned short>(x, gamma, beta, y, rows, C, eps, (hipStream_t)stream);
    if (y_dtype == MAGE_F16) return ln_launch<f16_t>(x, gamma, beta, y, rows, C, eps, (hipStream_t)stream);
    if (y_dtype == MAGE_BF16X3 || y_dtype == MAGE_F16X3) {
        MAGE_CHECK_ARG(C % 64 == 0 && (((uintptr_t)y) & 255) == 0, "mage_layernorm: split output needs C %% 64 == 0 and y 256-byte aligned");
        if (y_dtype == MAGE_BF16X3) return ln_launch<split_bf16>(x, gamma, beta, y, rows, C, eps, (hipStream_t)stream);
        return ln_launch<split_f16>(x, gamma, beta, y, rows, C, eps, (hipStream_t)stream);
    }
    mage_set_error("mage_layernorm: bad y_dtype %d", y_dtype);
    return MAGE_EINVAL;
}

namespace {

// ------------------------------------------------------------------------------------------------ LayerNorm backward
// One wave per row (statistics recomputed from the saved LN input, two-pass as in the forward kernel):
//   xhat = (x - mean) rstd;  g = dy * gamma;  dx = rstd (g - mean_c(g) - xhat mean_c(g xhat))       [+= if accumulate]
// and per-workgroup partial sums of dgamma = sum_rows dy xhat, dbeta = sum_rows dy (part [gridDim.x][2][C], reduced by
// mage_sum_partials: fixed order, deterministic).
// dxb (optional): the updated dx row once more as bf16 through the dropout mask of the branch it enters next, keep(i) / (1 - p) of
// mage_dropout on the flat index i = row * C + c (thresh 0: a plain cast) -- the operand of that branch's data- and weight-gradient
// GEMMs, which a separate mage_dropout pass (read 4 B + write 2 B per element) produced before.
template <typename DT, int VPL>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const DT* __restrict__ dy, float* __restrict__ dx, float* __restrict__ part,
                                                            long rows, int C, float eps, int accumulate, unsigned short* __restrict__ dxb,
                                                            unsigned thresh, float inv_keep, unsigned long long seedmul) {
    __shared__ float red[4][2][VPL * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 dg[VPL], db[VPL], gm[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        dg[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int c = j * 256 + lane * 4;
        gm[j] = c < C ? *(const f32x4*)(gamma + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
        const float* xr = x + row * C;
        const DT* dr = dy + row * C;
        f32x4 v[VPL], d[VPL];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * 256 + lane * 4;
            v[j] = c < C ? *(const f32x4*)(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            d[j] = c < C ? load4(dr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * 256 + lane * 4;
            if (c < C) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = v[j][e] - mean;
                    q += t * t;
                }
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
        float sg = 0.f, sgx = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * 256 + lane * 4;
            if (c < C) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (v[j][e] - mean) * rstd;
                    const float g = d[j][e] * gm[j][e];
                    sg += g;
                    sgx += g * xh;
                    dg[j][e] += d[j][e] * xh;
                    db[j][e] += d[j][e];
                    v[j][e] = xh;
                    d[j][e] = g;
                }
            }
        }
        const float mg = wave_sum(sg) / (float)C, mgx = wave_sum(sgx) / (float)C;
        float* dxr = dx + row * C;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * 256 + lane * 4;
            if (c < C) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rstd * (d[j][e] - mg - v[j][e] * mgx);
                if (accumulate) o += *(const f32x4*)(dxr + c);
                *(f32x4*)(dxr + c) = o;
                if (dxb) {
                    const unsigned long long i = (unsigned long long)(row * C + c);
                    if (thresh) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = drop_keep(seedmul, i + e, thresh) ? o[e] * inv_keep : 0.f;
                    }
                    store4(dxb + i, o);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[wave][0][j * 256 + lane * 4 + e] = dg[j][e];
            red[wave][1][j * 256 + lane * 4 + e] = db[j][e];
        }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        part[((long)blockIdx.x * 2 + 0) * C + c] = (red[0][0][c] + red[1][0][c]) + (red[2][0][c] + red[3][0][c]);
        part[((long)blockIdx.x * 2 + 1) * C + c] = (red[0][1][c] + red[1][1][c]) + (red[2][1][c] + red[3][1][c]);
    }
}

template <typename DT>
int ln_bwd_launch(const float* x, const float* gamma, const void* dy, float* dx, float* part, int32_t n_part, int64_t rows, int32_t C,
                  float eps, int32_t accumulate, void* dxb, float p, uint64_t seed, hipStream_t s) {
    const dim3 grid(n_part), blk(256);
    const DropMask m(p, seed);
    ln_vpl(C, [&](auto V) {
        hipLaunchKernelGGL((layernorm_bwd_kernel<DT, decltype(V)::value>), grid, blk, 0, s, x, gamma, (const DT*)dy, dx, part, (long)rows, C, eps,
                           accumulate, (unsigned short*)dxb, m.thresh, m.inv_keep, m.seedmul);
    });
    MAGE_CHECK_LAUNCH("mage_layernorm_bwd");
    return MAGE_OK;
}

}  // namespace

extern "C" int mage_layernorm_bwd(const float* x, const float* gamma, const void* dy, int32_t dy_dtype, float* dx, float* partials,
                                  int32_t n_part, int64_t rows, int32_t C, float eps, int32_t accumulate, void* dx_bf16, float p, uint64_t seed,
                                  void* stream) {
    MAGE_CHECK_ARG(x && gamma && dy && dx && partials, "mage_layernorm_bwd: null pointer");
    MAGE_CHECK_ARG(p >= 0.f && p < 1.f && (!dx_bf16 || ((uintptr_t)dx_bf16 & 7) == 0), "mage_layernorm_bwd: bad dx_bf16 / p");
    MAGE_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0 && C <= 2048 && n_part >= 1, "mage_layernorm_bwd: rows=%ld C=%d unsupported", (long)rows, C);
    hipStream_t s = (hipStream_t)stream;
    DT_DISPATCH(dy_dtype, (ln_bwd_launch<float>(x, gamma, dy, dx, partials, n_part, rows, C, eps, accumulate, dx_bf16, p, seed, s)),
                (ln_bwd_launch<unsigned short>(x, gamma, dy, dx, partials, n_part, rows, C, eps, accumulate, dx_bf16, p, seed, s)),
                "mage_layernorm_bwd");
}

// y = r + dropout(x) and yn = LayerNorm(y) in one pass (one wave per row, the arithmetic of layernorm_kernel on the registers that hold
// the new row): the residual add of a transformer block followed by the norm that opens the next branch (mage_model.py:48-52).
namespace {
template <typename T, typename OT, int VPL>
__global__ __launch_bounds__(256) void dropout_add_ln_kernel(const T* __restrict__ x, const float* __restrict__ r, float* __restrict__ y,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             OT* __restrict__ yn, long rows, int C, float eps, unsigned thresh,
                                                             float inv_keep, unsigned long long seedmul) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            const long i = row * C + c;
            const f32x4 b = load4(x + i);
            v[j] = *(const f32x4*)(r + i);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (drop_keep(seedmul, (unsigned long long)(i + e), thresh)) v[j][e] += b[e] * inv_keep;
            *(f32x4*)(y + i) = v[j];
        }
        s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        if (c < C) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dlt = v[j][e] - mean;
                q += dlt * dlt;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    OT* yr = yn + row * C;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = j * 256 + lane * 4;
        if (c < C) {
            const f32x4 gm = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[j][e] - mean) * rstd * gm[e] + bt[e];
            store4(yr + c, o);
        }
    }
}

template <typename T, typename OT>
int dropout_add_ln_launch(const void* x, const float* r, float* y, const float* gamma, const float* beta, void* yn, int64_t rows, int32_t C,
                          float eps, float p, uint64_t seed, hipStream_t s) {
    const DropMask m(p, seed);
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    ln_vpl(C, [&](auto V) {
        hipLaunchKernelGGL((dropout_add_ln_kernel<T, OT, decltype(V)::value>), grid, blk, 0, s, (const T*)x, r, y, gamma, beta, (OT*)yn, (long)rows,
                           C, eps, m.thresh, m.inv_keep, m.seedmul);
    });
    MAGE_CHECK_LAUNCH("mage_dropout_add_layernorm");
    return MAGE_OK;
}
}  // namespace

extern "C" int mage_dropout_add_layernorm(const void* x, int32_t x_dtype, const float* r, float* y, const float* gamma, const float* beta,
                                          void* yn, int32_t yn_dtype, int64_t rows, int32_t C, float eps, float p, uint64_t seed,
                                          void* stream) {
    MAGE_CHECK_ARG(x && r && y && gamma && beta && yn && rows > 0 && C > 0 && C % 4 == 0 && C <= 2048 && p >= 0.f && p < 1.f,
                   "mage_dropout_add_layernorm: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == MAGE_F32 && yn_dtype == MAGE_F32) return dropout_add_ln_launch<float, float>(x, r, y, gamma, beta, yn, rows, C, eps, p, seed, s);
    if (x_dtype == MAGE_F32 && yn_dtype == MAGE_BF16) return dropout_add_ln_launch<float, unsigned short>(x, r, y, gamma, beta, yn, rows, C, eps, p, seed, s);
    if (x_dtype == MAGE_BF16 && yn_dtype == MAGE_BF16) return dropout_add_ln_launch<unsigned short, unsigned short>(x, r, y, gamma, beta, yn, rows, C, eps, p, seed, s);
    mage_set_error("mage_dropout_add_layernorm: bad dtypes %d %d", x_dtype, yn_dtype);
    return MAGE_EINVAL;
}

// ------------------------------------------------------------------------------------ LayerNorm statistics from GEMM partial sums
namespace {
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ part, long rows, int n_slices, float inv_c, float eps,
                                                       float* __restrict__ stats) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float mean, rstd;
    mage_ln_stats_row((const float2*)part + r, rows, n_slices, inv_c, eps, mean, rstd);          // slice-major: each slice's loads are coalesced
    *(float2*)(stats + 2 * r) = float2{mean, rstd};
}
}  // namespace

// (mean, rstd) of bf16 rows, one wave per row: the first LayerNorm of a decoder pass when the residual stream starts in bf16 (the frame
// fill and context_linear write bf16 rows; the Linear that follows takes (rows, stats) like every later one).  Sums in fp32 in a fixed
// order (lane: its 8-column groups left to right; then the xor tree), the closing formula is mage_ln_stats'.
namespace {
template <typename HT>                                  // unsigned short = bf16 rows, f16_t = f16 rows
__global__ __launch_bounds__(256) void row_stats_kernel(const unsigned short* __restrict__ x, long rows, int C, long ldx, float inv_c, float eps,
                                                        float* __restrict__ stats) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const unsigned short* p = x + r * ldx;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        const uint4 v = *(const uint4*)(p + c);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 ab = unpack16x2<HT>(w[j]);
            const float a = ab.x, b = ab.y;
            s1 = __fadd_rn(s1, __fadd_rn(a, b));
            s2 = __fadd_rn(s2, __fmaf_rn(a, a, __fmul_rn(b, b)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 = __fadd_rn(s1, __shfl_xor(s1, o));
        s2 = __fadd_rn(s2, __shfl_xor(s2, o));
    }
    if (lane == 0) {
        const float mean = __fmul_rn(s1, inv_c);
        const float var = fmaxf(__fmaf_rn(-mean, mean, __fmul_rn(s2, inv_c)), 0.f);
        *(float2*)(stats + 2 * r) = float2{mean, __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, eps)))};
    }
}
}  // namespace

extern "C" int mage_row_stats(const void* x, int32_t dtype, int64_t rows, int32_t C, int64_t ldx, float eps, float* stats, void* stream) {
    MAGE_CHECK_ARG(x && stats && rows > 0 && C > 0 && C % 8 == 0 && ldx >= C && ldx % 8 == 0 && (((uintptr_t)x) & 15) == 0 &&
                       (dtype == MAGE_BF16 || dtype == MAGE_F16),
                   "mage_row_stats: bf16 or f16 rows, C and ldx multiples of 8, x 16-byte aligned");
    if (dtype == MAGE_F16)
        hipLaunchKernelGGL(row_stats_kernel<f16_t>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x,
                           (long)rows, C, (long)ldx, 1.0f / (float)C, eps, stats);
    else
        hipLaunchKernelGGL(row_stats_kernel<unsigned short>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned short*)x, (long)rows, C, (long)ldx, 1.0f / (float)C, eps, stats);
    MAGE_CHECK_LAUNCH("mage_row_stats");
    return MAGE_OK;
}

extern "C" int mage_ln_stats(const float* part, int64_t rows, int32_t n_slices, int32_t C, float eps, float* stats, void* stream) {
    MAGE_CHECK_ARG(part && stats && rows > 0 && n_slices > 0 && C > 0, "mage_ln_stats: bad arguments");
    hipLaunchKernelGGL(ln_stats_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, (long)rows, n_slices,
                       1.0f / (float)C, eps, stats);
    MAGE_CHECK_LAUNCH("mage_ln_stats");
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------ GroupNorm + SiLU (MAGE+ head)
namespace {

// stats[b][g] = {mean, rstd} over rows_per_sample rows x (C/groups) channels; one workgroup per (b, g), two passes,
// fixed-order reductions (deterministic).
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, long sample_stride_rows, long row_off,
                                                       int rows_per_sample, int C, int groups, float eps,
                                                       float* __restrict__ stats) {
    __shared__ double red[4];
    const int b = blockIdx.x, g = blockIdx.y, cpg = C / groups;
    const float* base = x + ((long)b * sample_stride_rows + row_off) * C + g * cpg;
    const long n = (long)rows_per_sample * cpg;
    auto block_sum = [&](double v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        return red[0] + red[1] + red[2] + red[3];
    };
    double s = 0.0;
    for (int r = threadIdx.x; r < rows_per_sample; r += 256)
        for (int c = 0; c < cpg; ++c) s += (double)base[(long)r * C + c];
    const double mean = block_sum(s) / (double)n;
    double q = 0.0;
    for (int r = threadIdx.x; r < rows_per_sample; r += 256)
        for (int c = 0; c < cpg; ++c) {
            const double dlt = (double)base[(long)r * C + c] - mean;
            q += dlt * dlt;
        }
    const double var = block_sum(q) / (double)n;
    if (threadIdx.x == 0) {
        stats[((long)b * groups + g) * 2] = (float)mean;
        stats[((long)b * groups + g) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// act: 0 none, 1 ReLU, 2 SiLU.  residual (optional, fp32, packed like the logical output) is added after the affine, before act.
// Output row of (sample b, row r): b*y_sample_stride_rows + y_row_off + r.
template <typename OT>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, long sample_stride_rows, long row_off,
                                                       int rows_per_sample, int C, int groups, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ residual, int act, OT* __restrict__ y,
                                                       long y_sample_stride_rows, long y_row_off, long total) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    const long orow = i / C;
    const int c = (int)(i - orow * C);
    const long b = orow / rows_per_sample, r = orow - b * rows_per_sample;
    const int cpg = C / groups;
    const f32x4 v = *(const f32x4*)(x + ((b * sample_stride_rows + row_off + r) * C + c));
    const f32x4 gm = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
    f32x4 res = f32x4{0.f, 0.f, 0.f, 0.f};
    if (residual) res = *(const f32x4*)(residual + i);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = (c + e) / cpg;                                  // a vector may straddle groups when C/groups < 4
        const float mean = stats[(b * groups + g) * 2], rstd = stats[(b * groups + g) * 2 + 1];
        const float t = (v[e] - mean) * rstd * gm[e] + bt[e] + res[e];
        o[e] = act == 2 ? t / (1.0f + expf(-t)) : act == 1 ? fmaxf(t, 0.f) : t;
    }
    store4(y + ((b * y_sample_stride_rows + y_row_off + r) * C + c), o);
}

int gn_launch(const char* who, const float* x, int64_t sample_stride_rows, int64_t row_off, int32_t n_samples, int32_t rows_per_sample,
              int32_t C, int32_t groups, const float* gamma, const float* beta, float eps, float* stats, const float* residual,
              int32_t act, void* y, int32_t y_dtype, int64_t y_sample_stride_rows, int64_t y_row_off, hipStream_t s) {
    if (y_dtype != MAGE_F32 && y_dtype != MAGE_BF16 && y_dtype != MAGE_F16) {      // refuse before the statistics kernel writes stats
        mage_set_error("%s: bad y_dtype %d", who, y_dtype);
        return MAGE_EINVAL;
    }
    hipLaunchKernelGGL(gn_stats_kernel, dim3(n_samples, groups), dim3(256), 0, s, x, (long)sample_stride_rows, (long)row_off,
                       rows_per_sample, C, groups, eps, stats);
    const long total = (long)n_samples * rows_per_sample * C;
    const dim3 grid((unsigned)((total / 4 + 255) / 256));
    if (y_dtype == MAGE_F32)
        hipLaunchKernelGGL((gn_apply_kernel<float>), grid, dim3(256), 0, s, x, (long)sample_stride_rows, (long)row_off, rows_per_sample,
                           C, groups, stats, gamma, beta, residual, act, (float*)y, (long)y_sample_stride_rows, (long)y_row_off, total);
    else if (y_dtype == MAGE_BF16)
        hipLaunchKernelGGL((gn_apply_kernel<unsigned short>), grid, dim3(256), 0, s, x, (long)sample_stride_rows, (long)row_off,
                           rows_per_sample, C, groups, stats, gamma, beta, residual, act, (unsigned short*)y,
                           (long)y_sample_stride_rows, (long)y_row_off, total);
    else                                               // the f16 mode on the latent (MAGE+) path: the GroupNorm + SiLU head's rows (round 6)
        hipLaunchKernelGGL((gn_apply_kernel<f16_t>), grid, dim3(256), 0, s, x, (long)sample_stride_rows, (long)row_off,
                           rows_per_sample, C, groups, stats, gamma, beta, residual, act, (f16_t*)y,
                           (long)y_sample_stride_rows, (long)y_row_off, total);
    MAGE_CHECK_LAUNCH(who);
    return MAGE_OK;
}

}  // namespace

extern "C" int mage_groupnorm_silu(const float* x, int64_t sample_stride_rows, int64_t row_off, int32_t n_samples,
                                   int32_t rows_per_sample, int32_t C, int32_t groups, const float* gamma, const float* beta,
                                   float eps, float* stats, void* y, int32_t y_dtype, void* stream) {
    MAGE_CHECK_ARG(x && gamma && beta && stats && y, "mage_groupnorm_silu: null pointer");
    MAGE_CHECK_ARG(n_samples > 0 && rows_per_sample > 0 && groups > 0 && C % groups == 0 && C % 4 == 0,
                   "mage_groupnorm_silu: C=%d groups=%d unsupported", C, groups);
    return gn_launch("mage_groupnorm_silu", x, sample_stride_rows, row_off, n_samples, rows_per_sample, C, groups, gamma, beta, eps,
                     stats, nullptr, 2, y, y_dtype, rows_per_sample, 0, (hipStream_t)stream);
}

extern "C" int mage_groupnorm_act(const float* x, int64_t sample_stride_rows, int64_t row_off, int32_t n_samples,
                                  int32_t rows_per_sample, int32_t C, int32_t groups, const float* gamma, const float* beta,
                                  float eps, float* stats, const float* residual, int32_t act, void* y, int32_t y_dtype,
                                  int64_t y_sample_stride_rows, int64_t y_row_off, void* stream) {
    MAGE_CHECK_ARG(x && gamma && beta && stats && y, "mage_groupnorm_act: null pointer");
    MAGE_CHECK_ARG(n_samples > 0 && rows_per_sample > 0 && groups > 0 && C % groups == 0 && C % 4 == 0,
                   "mage_groupnorm_act: C=%d groups=%d unsupported", C, groups);
    MAGE_CHECK_ARG(act >= 0 && act <= 2, "mage_groupnorm_act: act=%d (0 none, 1 relu, 2 silu)", act);
    return gn_launch("mage_groupnorm_act", x, sample_stride_rows, row_off, n_samples, rows_per_sample, C, groups, gamma, beta, eps,
                     stats, residual, act, y, y_dtype, y_sample_stride_rows, y_row_off, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ GroupNorm backward
// Backward of the randomness branch of MAGE.forward (mage_model.py:601-609): GroupNorm of the Conv3d video prior (:264-297), the
// instance norm of ADAIN2D (:299-314; adain_bwd_kernel below).
namespace {

// d act(t) / dt * dy;  act: 0 none, 1 ReLU, 2 SiLU
__device__ __forceinline__ float gn_dact(int act, float t, float dy) {
    if (act == 1) return t > 0.f ? dy : 0.f;
    if (act == 2) {
        const float sg = 1.0f / (1.0f + expf(-t));
        return dy * sg * (1.0f + t * (1.0f - sg));
    }
    return dy;
}

// y = act(xhat * gamma + beta + residual), xhat = (x - mean_{b,g}) * rstd_{b,g}.  With g = dy * act'(.):
//   dgamma_c = sum_{b,r} g xhat,  dbeta_c = sum_{b,r} g,  dx = rstd (gamma g - m1 - xhat m2),  m1 = mean_{(b,g)}(gamma g), m2 = mean(gamma g xhat).
// Pass 1: one workgroup per (sample, group); thread = (channel of the group, row phase); writes the per-(sample, channel) sums
// (fixed order) and red[b][g] = (m1, m2).  Row maps: x rows b*xs + xo + r, dy rows b*ds + dof + r, residual packed b*rows + r.
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const float* __restrict__ x, long xs, long xo, int rows_per_sample, int C, int groups,
                                                            const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ residual, int act,
                                                            const float* __restrict__ dy, long ds, long dof, float* __restrict__ red,
                                                            float* __restrict__ dgam_part, float* __restrict__ dbet_part) {
    __shared__ double sm[2][256];
    const int b = blockIdx.x, g = blockIdx.y, cpg = C / groups;
    const int cl = threadIdx.x % cpg, ph = threadIdx.x / cpg, nph = 256 / cpg;
    const int c = g * cpg + cl;
    const float mean = stats[((long)b * groups + g) * 2], rstd = stats[((long)b * groups + g) * 2 + 1];
    const float gm = gamma[c], bt = beta[c];
    double sg = 0.0, sgx = 0.0;
    for (int r = ph; r < rows_per_sample; r += nph) {
        const float xh = (x[((long)b * xs + xo + r) * C + c] - mean) * rstd;
        float t = xh * gm + bt;
        if (residual) t += residual[((long)b * rows_per_sample + r) * C + c];
        const float ge = gn_dact(act, t, dy[((long)b * ds + dof + r) * C + c]);
        sg += (double)ge;
        sgx += (double)ge * (double)xh;
    }
    sm[0][threadIdx.x] = sg;
    sm[1][threadIdx.x] = sgx;
    __syncthreads();
    if (threadIdx.x < cpg) {
        double a = 0.0, q = 0.0;
        for (int p = 0; p < nph; ++p) {
            a += sm[0][p * cpg + threadIdx.x];
            q += sm[1][p * cpg + threadIdx.x];
        }
        dbet_part[(long)b * C + c] = (float)a;
        dgam_part[(long)b * C + c] = (float)q;
        sm[0][threadIdx.x] = a * (double)gm;
        sm[1][threadIdx.x] = q * (double)gm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, q = 0.0;
        for (int i = 0; i < cpg; ++i) {
            a += sm[0][i];
            q += sm[1][i];
        }
        const double n = (double)rows_per_sample * cpg;
        red[((long)b * groups + g) * 2] = (float)(a / n);
        red[((long)b * groups + g) * 2 + 1] = (float)(q / n);
    }
}

// Pass 2 (elementwise): dx rows in x's row map; dres (optional, packed) = g.
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, long xs, long xo, int rows_per_sample, int C, int groups,
                                                           const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ residual, int act,
                                                           const float* __restrict__ dy, long ds, long dof, const float* __restrict__ red,
                                                           float* __restrict__ dx, float* __restrict__ dres, long total) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    const long orow = i / C;
    const int c = (int)(i - orow * C);
    const long b = orow / rows_per_sample, r = orow - b * rows_per_sample;
    const int cpg = C / groups;
    const f32x4 v = *(const f32x4*)(x + ((b * xs + xo + r) * C + c));
    const f32x4 gy = *(const f32x4*)(dy + ((b * ds + dof + r) * C + c));
    const f32x4 gm = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
    f32x4 res = f32x4{0.f, 0.f, 0.f, 0.f};
    if (residual) res = *(const f32x4*)(residual + i);
    f32x4 o, ge4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long sg = (b * groups + (c + e) / cpg) * 2;
        const float mean = stats[sg], rstd = stats[sg + 1];
        const float xh = (v[e] - mean) * rstd;
        const float ge = gn_dact(act, xh * gm[e] + bt[e] + res[e], gy[e]);
        ge4[e] = ge;
        o[e] = rstd * (gm[e] * ge - red[sg] - xh * red[sg + 1]);
    }
    *(f32x4*)(dx + ((b * xs + xo + r) * C + c)) = o;
    if (dres) *(f32x4*)(dres + i) = ge4;
}

}  // namespace

extern "C" int mage_groupnorm_bwd(const float* x, int64_t sample_stride_rows, int64_t row_off, int32_t n_samples, int32_t rows_per_sample,
                                  int32_t C, int32_t groups, const float* stats, const float* gamma, const float* beta, const float* residual,
                                  int32_t act, const float* dy, int64_t dy_sample_stride_rows, int64_t dy_row_off, float* red, float* dx,
                                  float* dres, float* dgamma_part, float* dbeta_part, void* stream) {
    MAGE_CHECK_ARG(x && stats && gamma && beta && dy && red && dx && dgamma_part && dbeta_part, "mage_groupnorm_bwd: null pointer");
    MAGE_CHECK_ARG(n_samples > 0 && rows_per_sample > 0 && groups > 0 && C % groups == 0 && C % 4 == 0 && (C / groups) <= 256 &&
                       256 % (C / groups) == 0 && act >= 0 && act <= 2,
                   "mage_groupnorm_bwd: C=%d groups=%d act=%d unsupported (channels per group must divide 256)", C, groups, act);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_bwd_reduce_kernel, dim3(n_samples, groups), dim3(256), 0, s, x, (long)sample_stride_rows, (long)row_off, rows_per_sample,
                       C, groups, stats, gamma, beta, residual, act, dy, (long)dy_sample_stride_rows, (long)dy_row_off, red, dgamma_part,
                       dbeta_part);
    const long total = (long)n_samples * rows_per_sample * C;
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, x, (long)sample_stride_rows,
                       (long)row_off, rows_per_sample, C, groups, stats, gamma, beta, residual, act, dy, (long)dy_sample_stride_rows,
                       (long)dy_row_off, red, dx, dres, total);
    MAGE_CHECK_LAUNCH("mage_groupnorm_bwd");
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------ ADAIN
namespace {
// grid = (B, C/64); block 256 = 64 channels x 4 position phases.
__global__ __launch_bounds__(256) void adain_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ out, int P,
                                                    int C, float eps) {
    __shared__ float red[2][4][64];
    const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    const long base = (long)b * P * C + c;
    float s = 0.f;
    for (int p = ph; p < P; p += 4) s += x[base + (long)p * C];
    red[0][ph][threadIdx.x & 63] = s;
    __syncthreads();
    const float mean = (red[0][0][threadIdx.x & 63] + red[0][1][threadIdx.x & 63] + red[0][2][threadIdx.x & 63] +
                        red[0][3][threadIdx.x & 63]) / (float)P;
    float q = 0.f;
    for (int p = ph; p < P; p += 4) {
        const float dlt = x[base + (long)p * C] - mean;
        q += dlt * dlt;
    }
    red[1][ph][threadIdx.x & 63] = q;
    __syncthreads();
    const float var = (red[1][0][threadIdx.x & 63] + red[1][1][threadIdx.x & 63] + red[1][2][threadIdx.x & 63] +
                       red[1][3][threadIdx.x & 63]) / (float)P;
    const float rstd = 1.0f / sqrtf(var + eps);
    for (int p = ph; p < P; p += 4) {
        const long i = base + (long)p * C;
        out[i] = gamma[i] * ((x[i] - mean) * rstd) + beta[i];
    }
}
}  // namespace

extern "C" int mage_adain(const float* x, const float* gamma, const float* beta, float* out, int32_t B, int32_t P,
                          int32_t C, float eps, void* stream) {
    MAGE_CHECK_ARG(x && gamma && beta && out, "mage_adain: null pointer");
    MAGE_CHECK_ARG(B > 0 && P > 0 && C > 0 && C % 64 == 0, "mage_adain: C=%d must be a multiple of 64", C);
    hipLaunchKernelGGL(adain_kernel, dim3(B, C / 64), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, out, P, C, eps);
    MAGE_CHECK_LAUNCH("mage_adain");
    return MAGE_OK;
}

namespace {
// out = gamma_map * IN(x) + beta_map over the P positions of (b, c) (adain_kernel above).  Given dout:
//   dgamma_map = dout * xhat, dbeta_map = dout (no kernel), dx = rstd (g - mean_p(g) - xhat mean_p(g xhat)), g = dout * gamma_map.
// grid = (B, C/64); block 256 = 64 channels x 4 position phases.
__global__ __launch_bounds__(256) void adain_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gmap, const float* __restrict__ dout,
                                                        float* __restrict__ dx, float* __restrict__ dgmap, int P, int C, float eps) {
    __shared__ float red[4][4][64];
    const int b = blockIdx.x, cl = threadIdx.x & 63, c = blockIdx.y * 64 + cl, ph = threadIdx.x >> 6;
    const long base = (long)b * P * C + c;
    float s = 0.f;
    for (int p = ph; p < P; p += 4) s += x[base + (long)p * C];
    red[0][ph][cl] = s;
    __syncthreads();
    const float mean = (red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl]) / (float)P;
    float q = 0.f;
    for (int p = ph; p < P; p += 4) {
        const float dlt = x[base + (long)p * C] - mean;
        q += dlt * dlt;
    }
    red[1][ph][cl] = q;
    __syncthreads();
    const float var = (red[1][0][cl] + red[1][1][cl] + red[1][2][cl] + red[1][3][cl]) / (float)P;
    const float rstd = 1.0f / sqrtf(var + eps);
    float s1 = 0.f, s2 = 0.f;
    for (int p = ph; p < P; p += 4) {
        const long i = base + (long)p * C;
        const float xh = (x[i] - mean) * rstd, g = dout[i] * gmap[i];
        s1 += g;
        s2 += g * xh;
    }
    red[2][ph][cl] = s1;
    red[3][ph][cl] = s2;
    __syncthreads();
    const float m1 = (red[2][0][cl] + red[2][1][cl] + red[2][2][cl] + red[2][3][cl]) / (float)P;
    const float m2 = (red[3][0][cl] + red[3][1][cl] + red[3][2][cl] + red[3][3][cl]) / (float)P;
    for (int p = ph; p < P; p += 4) {
        const long i = base + (long)p * C;
        const float xh = (x[i] - mean) * rstd, go = dout[i];
        dgmap[i] = go * xh;
        dx[i] = rstd * (go * gmap[i] - m1 - xh * m2);
    }
}
}  // namespace

extern "C" int mage_adain_bwd(const float* x, const float* gamma_map, const float* dout, float* dx, float* dgamma_map, int32_t B, int32_t P,
                              int32_t C, float eps, void* stream) {
    MAGE_CHECK_ARG(x && gamma_map && dout && dx && dgamma_map && B > 0 && P > 0 && C > 0 && C % 64 == 0, "mage_adain_bwd: bad arguments");
    hipLaunchKernelGGL(adain_bwd_kernel, dim3(B, C / 64), dim3(256), 0, (hipStream_t)stream, x, gamma_map, dout, dx, dgamma_map, P, C, eps);
    MAGE_CHECK_LAUNCH("mage_adain_bwd");
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------------------ BatchNorm (training mode)
namespace {
// Stage-1 VQ-VAE training (train_vqvae.py:13-35) runs its BatchNorm2d layers on BATCH statistics.  Channels-last rows [rows, C]:
// the statistics are column reductions.  One workgroup owns a slab of rows, thread = channel (coalesced rows), partial sums per
// workgroup [gridDim.x][NOUT][C] are added in a fixed order by mage_sum_partials.
//   MODE 0: sum x                      MODE 1: sum (x - mean)^2                (two-pass variance)
//   MODE 2: sum g, sum g * xhat        g = dy * (mask ? mask > 0 : 1),  xhat = (x - mean) * rstd      (backward)
template <int MODE>
__global__ __launch_bounds__(256) void bn_colreduce_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ mask, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, long rows, int C, long rows_per_blk,
                                                           float* __restrict__ part) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const long r0 = (long)blockIdx.x * rows_per_blk, r1 = min(rows, r0 + rows_per_blk);
    float a0 = 0.f, a1 = 0.f;
    const float m = MODE >= 1 ? mean[c] : 0.f, rs = MODE == 2 ? rstd[c] : 0.f;
    for (long r = r0; r < r1; ++r) {
        const float v = x[r * C + c];
        if (MODE == 0) a0 += v;
        if (MODE == 1) a0 += (v - m) * (v - m);
        if (MODE == 2) {
            float g = dy[r * C + c];
            if (mask && !(mask[r * C + c] > 0.f)) g = 0.f;
            a0 += g;
            a1 += g * ((v - m) * rs);
        }
    }
    constexpr int NOUT = MODE == 2 ? 2 : 1;
    part[((long)blockIdx.x * NOUT + 0) * C + c] = a0;
    if (MODE == 2) part[((long)blockIdx.x * NOUT + 1) * C + c] = a1;
}

// y = [relu]((x - mean) * rstd * gamma + beta [+ residual])
template <typename OT>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ residual, OT* __restrict__ y, long n, int C, int relu) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const int c = (int)(i % C);
    const f32x4 v = *(const f32x4*)(x + i), m = *(const f32x4*)(mean + c), rs = *(const f32x4*)(rstd + c), g = *(const f32x4*)(gamma + c),
                b = *(const f32x4*)(beta + c);
    f32x4 o = (v - m) * rs * g + b;
    if (residual) o += *(const f32x4*)(residual + i);
    if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
    }
    store4(y + i, o);
}

// dx = gamma * rstd * (g - s1 / rows - xhat * s2 / rows),  g = dy * (mask ? mask > 0 : 1), (s1, s2) = the MODE 2 column sums
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mask,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ sums, float inv_rows,
                                                           float* __restrict__ dx, long n, int C) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const int c = (int)(i % C);
    const f32x4 v = *(const f32x4*)(x + i), m = *(const f32x4*)(mean + c), rs = *(const f32x4*)(rstd + c), gm = *(const f32x4*)(gamma + c),
                s1 = *(const f32x4*)(sums + c), s2 = *(const f32x4*)(sums + C + c);
    f32x4 g = *(const f32x4*)(dy + i);
    if (mask) {
        const f32x4 mk = *(const f32x4*)(mask + i);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!(mk[e] > 0.f)) g[e] = 0.f;
    }
    const f32x4 xh = (v - m) * rs;
    *(f32x4*)(dx + i) = gm * rs * (g - s1 * inv_rows - xh * (s2 * inv_rows));
}
}  // namespace

extern "C" int mage_bn_colreduce(int32_t mode, const float* x, const float* dy, const float* mask, const float* mean, const float* rstd,
                                 int64_t rows, int32_t C, float* partials, int32_t n_part, void* stream) {
    MAGE_CHECK_ARG(x && partials && rows > 0 && C > 0 && n_part >= 1 && mode >= 0 && mode <= 2, "mage_bn_colreduce: bad arguments");
    MAGE_CHECK_ARG(mode == 0 || mean, "mage_bn_colreduce: mean missing");
    MAGE_CHECK_ARG(mode != 2 || (dy && rstd), "mage_bn_colreduce: dy / rstd missing");
    const long rpb = (rows + n_part - 1) / n_part;
    const dim3 grid(n_part, (C + 255) / 256), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (mode == 0) hipLaunchKernelGGL((bn_colreduce_kernel<0>), grid, blk, 0, s, x, dy, mask, mean, rstd, (long)rows, C, rpb, partials);
    else if (mode == 1) hipLaunchKernelGGL((bn_colreduce_kernel<1>), grid, blk, 0, s, x, dy, mask, mean, rstd, (long)rows, C, rpb, partials);
    else hipLaunchKernelGGL((bn_colreduce_kernel<2>), grid, blk, 0, s, x, dy, mask, mean, rstd, (long)rows, C, rpb, partials);
    MAGE_CHECK_LAUNCH("mage_bn_colreduce");
    return MAGE_OK;
}

extern "C" int mage_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const float* residual, void* y, int32_t y_dtype, int64_t rows, int32_t C, int32_t relu, void* stream) {
    MAGE_CHECK_ARG(x && mean && rstd && gamma && beta && y && rows > 0 && C > 0 && C % 4 == 0, "mage_bn_apply: bad arguments");
    const long n = (long)rows * C;
    const dim3 grid((unsigned)((n / 4 + 255) / 256)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (y_dtype == MAGE_F32) hipLaunchKernelGGL((bn_apply_kernel<float>), grid, blk, 0, s, x, mean, rstd, gamma, beta, residual, (float*)y, n, C, relu);
    else if (y_dtype == MAGE_BF16)
        hipLaunchKernelGGL((bn_apply_kernel<unsigned short>), grid, blk, 0, s, x, mean, rstd, gamma, beta, residual, (unsigned short*)y, n, C, relu);
    else { mage_set_error("mage_bn_apply: bad y_dtype %d", y_dtype); return MAGE_EINVAL; }
    MAGE_CHECK_LAUNCH("mage_bn_apply");
    return MAGE_OK;
}

extern "C" int mage_bn_bwd_apply(const float* x, const float* dy, const float* mask, const float* mean, const float* rstd, const float* gamma,
                                 const float* sums, float* dx, int64_t rows, int32_t C, void* stream) {
    MAGE_CHECK_ARG(x && dy && mean && rstd && gamma && sums && dx && rows > 0 && C > 0 && C % 4 == 0, "mage_bn_bwd_apply: bad arguments");
    const long n = (long)rows * C;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, mask, mean, rstd,
                       gamma, sums, 1.0f / (float)rows, dx, n, C);
    MAGE_CHECK_LAUNCH("mage_bn_bwd_apply");
    return MAGE_OK;
}
