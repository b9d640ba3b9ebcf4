// Training path: the kernels of MAGE.forward's backward pass that are not GEMMs and whose forward is not in a file by
// subject (the norms' backwards are in norm.hip, attention's in attention_bwd.hip, the small losses' in rows.hip, Adam in optim.hip).
//
// The dense gradients reuse mage_gemm: dX = dY W is the forward kernel on a transposed weight copy; dW = dY^T X contracts over
// ALL M tokens while its output is only [N, K], so both operands are first transposed (mage_transpose: HBM-bound, one pass) and
// the product runs as one split-K launch of the same MFMA kernel (mage_gemm_desc::n_split) whose partial outputs
// mage_sum_partials adds in a fixed order.  Everything here is deterministic except mage_embedding_bwd (fp32 atomics, like the
// reference's own nn.Embedding backward on a GPU).
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ transpose (+ conv tap gather)
// y[(c + y_row0) * ldy + m] = x[arow(m) * ldx + c]   for m < M,  0 for M <= m < Mp  (the split-K GEMM reads whole 64-column
// slabs, so the tail up to the padded width is zero-filled).  arow(m) is the implicit-GEMM row map of mage_gemm: m -> (img, oy,
// ox) over an out_h x out_w plane, row = img*img_stride + (oy+dy)*in_w + (ox+dx) + a_off, zero outside [0,in_h) x [0,in_w): a
// plain transpose is out_h = 1, out_w = M; the nine shifted copies of the activation that the conv3x3 weight gradient
// contracts with are nine calls with (dy, dx) = tap - 1 and y_row0 = tap * C.
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y, long ldy, long y_row0,
                                                        long M, long Mp, int C, int out_h, int out_w, int in_h, int in_w,
                                                        long img_stride, long a_off, int dy, int dx, int stride) {
    __shared__ T tile[64][65];
    const long m0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // 64 x 4
    const long plane = (long)out_h * out_w;
#pragma unroll 4
    for (int r = ty; r < 64; r += 4) {                           // r: m within the tile; tx: channel
        const long m = m0 + r;
        T v = (T)0;
        if (m < M && c0 + tx < C) {
            const long img = m / plane, rem = m - img * plane;
            const int oy = (int)(rem / out_w), ox = (int)(rem - (long)oy * out_w);
            const int iy = oy * stride + dy, ix = ox * stride + dx;
            if ((unsigned)iy < (unsigned)in_h && (unsigned)ix < (unsigned)in_w)
                v = x[(img * img_stride + (long)iy * in_w + ix + a_off) * ldx + c0 + tx];
        }
        tile[r][tx] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = ty; r < 64; r += 4) {                           // r: channel within the tile; tx: m
        const long m = m0 + tx;
        if (c0 + r < C && m < Mp) y[(y_row0 + c0 + r) * ldy + m] = tile[tx][r];
    }
}


// 16-byte variant for bf16 with C % 8 == 0: a thread loads 8 consecutive channels of one (gathered) row, the 64 x 64 tile sits in LDS
// row-major (pitch 132 B: the column reads below touch distinct banks), then every thread assembles 8 consecutive m of one channel
// and stores 16 bytes: both sides of the transposition move whole 128-byte segments (the 2-byte version ran at 1.1 TB/s).
__global__ __launch_bounds__(256) void transpose8_kernel(const unsigned short* __restrict__ x, long ldx, unsigned short* __restrict__ y,
                                                         long ldy, long y_row0, long M, long Mp, int C, int out_h, int out_w, int in_h,
                                                         int in_w, long img_stride, long a_off, int dy, int dx, int stride) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[64 * 66];
    const long m0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const long plane = (long)out_h * out_w;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = threadIdx.x + 256 * k;          // 512 (row, 8-channel chunk) pairs
        const int r = e >> 3, cc = (e & 7) * 8;
        const long m = m0 + r;
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (m < M && c0 + cc < C) {
            const long img = m / plane, rem = m - img * plane;
            const int oy = (int)(rem / out_w), ox = (int)(rem - (long)oy * out_w);
            const int iy = oy * stride + dy, ix = ox * stride + dx;
            if ((unsigned)iy < (unsigned)in_h && (unsigned)ix < (unsigned)in_w)
                v = *(const uint4*)(x + (img * img_stride + (long)iy * in_w + ix + a_off) * ldx + c0 + cc);
        }
        unsigned* t32 = (unsigned*)(tile + r * 66 + cc);      // 66-element pitch: 4-byte aligned
        t32[0] = v.x; t32[1] = v.y; t32[2] = v.z; t32[3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = threadIdx.x + 256 * k;          // 512 (channel, 8-row chunk) pairs
        const int c = e >> 3, mm = (e & 7) * 8;
        if (c0 + c < C && m0 + mm < Mp) {
            unsigned short h[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = tile[(mm + j) * 66 + c];
            uint4 o;
            o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
            o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
            *(uint4*)(y + (y_row0 + c0 + c) * ldy + m0 + mm) = o;
        }
    }
}

// The same transposition with the column sums of x folded in (the bias gradient db = sum_m dY[m, :] of a Linear, which used to be a
// second pass over the transposed copy: 7 ms of a 119 ms training step): a workgroup walks TPW consecutive 64-row tiles, every thread adds
// up the 8 rows it assembles per channel, the 8 threads of a channel combine by xor-shuffles, and the workgroup's sums land in
// colsum[blockIdx.x][c] (fixed order; mage_sum_partials adds the ceil(tiles / TPW) partial rows).
constexpr int TRANSPOSE_TPW = 16;
__global__ __launch_bounds__(256) void transpose8_colsum_kernel(const unsigned short* __restrict__ x, long ldx, unsigned short* __restrict__ y,
                                                                long ldy, long M, long Mp, int C, int out_h, int out_w, int in_h, int in_w,
                                                                long img_stride, long a_off, float* __restrict__ colsum) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[64 * 66];
    const int c0 = blockIdx.y * 64;
    const long plane = (long)out_h * out_w;
    float cs[2] = {0.f, 0.f};
    for (int t = 0; t < TRANSPOSE_TPW; ++t) {
        const long m0 = ((long)blockIdx.x * TRANSPOSE_TPW + t) * 64;
        if (m0 >= Mp) break;                                              // block-uniform
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = threadIdx.x + 256 * k;
            const int r = e >> 3, cc = (e & 7) * 8;
            const long m = m0 + r;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (m < M && c0 + cc < C) {
                const long img = m / plane, rem = m - img * plane;
                const int oy = (int)(rem / out_w), ox = (int)(rem - (long)oy * out_w);
                if ((unsigned)oy < (unsigned)in_h && (unsigned)ox < (unsigned)in_w)
                    v = *(const uint4*)(x + (img * img_stride + (long)oy * in_w + ox + a_off) * ldx + c0 + cc);
            }
            unsigned* t32 = (unsigned*)(tile + r * 66 + cc);
            t32[0] = v.x; t32[1] = v.y; t32[2] = v.z; t32[3] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = threadIdx.x + 256 * k;
            const int c = e >> 3, mm = (e & 7) * 8;
            if (c0 + c < C && m0 + mm < Mp) {
                unsigned short h[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    h[j] = tile[(mm + j) * 66 + c];
                    cs[k] += bf_bits2f(h[j]);
                }
                uint4 o;
                o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
                o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
                *(uint4*)(y + (long)(c0 + c) * ldy + m0 + mm) = o;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float v = cs[k];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        const int e = threadIdx.x + 256 * k;
        const int c = e >> 3;
        if ((e & 7) == 0 && c0 + c < C) colsum[(long)blockIdx.x * C + c0 + c] = v;
    }
}

// out[r] = sum_c x[r*ld + c], c < n (fp32 accumulation, fixed order): bias gradients from the transposed dY.
// blockIdx.y = column chunk (a row of 10^5 columns on ONE wave was 0.76 ms per call: 19 % of a training step): partial sums
// out[chunk][r] for mage_sum_partials.
template <typename T>
__global__ __launch_bounds__(256) void row_sum_kernel(const T* __restrict__ x, long ld, long n, int rows, float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const long per = ((n + gridDim.y - 1) / gridDim.y + 7) / 8 * 8;
    const long c0 = (long)blockIdx.y * per, c1 = min(n, c0 + per);
    const T* p = x + (long)r * ld;
    float s = 0.f;
    for (long c = c0 + lane; c < c1; c += 64) s += to_f32<T>(p[c]);
    s = wave_sum(s);
    if (lane == 0) out[(long)blockIdx.y * rows + r] = s;
}

// out[i] = (accumulate ? out[i] : 0) + sum_s part[s*stride + i]
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, long stride, int n_part, long n,
                                                           float* __restrict__ out, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = accumulate ? out[i] : 0.f;
    for (int p = 0; p < n_part; ++p) s += part[(long)p * stride + i];
    out[i] = s;
}

// The same sum for 16-byte aligned operands: a workgroup owns 64 float4 columns, its four waves take the partials p = w, w+4, w+8, ..
// (independent 16-byte loads, 4 in flight per lane) and their four sums are added in a fixed order through LDS:
//     out = ((s_0 + s_1) + (s_2 + s_3)) [+ out],  s_w = part[w] + part[w+4] + ...      -- deterministic, like the scalar kernel's order.
// The scalar kernel walked 64 dependent 4-byte loads per thread: 6.9 ms per training step at B = 64 for ~2.7 GB of split-K partials.
__global__ __launch_bounds__(256) void sum_partials4_kernel(const float* __restrict__ part, long stride, int n_part, long n4,
                                                            float* __restrict__ out, int accumulate) {
    __shared__ f32x4 red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long i4 = (long)blockIdx.x * 64 + lane;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i4 < n4) {
        const float* p0 = part + i4 * 4;
        int p = w;
        for (; p + 12 < n_part; p += 16) {
            const f32x4 a = *(const f32x4*)(p0 + (long)p * stride), b = *(const f32x4*)(p0 + (long)(p + 4) * stride);
            const f32x4 c = *(const f32x4*)(p0 + (long)(p + 8) * stride), e = *(const f32x4*)(p0 + (long)(p + 12) * stride);
            s += a;
            s += b;
            s += c;
            s += e;
        }
        for (; p < n_part; p += 4) s += *(const f32x4*)(p0 + (long)p * stride);
    }
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && i4 < n4) {
        f32x4 t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (accumulate) t += *(const f32x4*)(out + i4 * 4);
        *(f32x4*)(out + i4 * 4) = t;
    }
}

// ------------------------------------------------------------------------------------------------ activations
template <int ACT>
__device__ __forceinline__ float actf(float v) {
    if (ACT == MAGE_ACT_RELU) return fmaxf(v, 0.f);
    if (ACT == MAGE_ACT_QUICKGELU) return v / (1.f + expf(-1.702f * v));
    if (ACT == MAGE_ACT_GELU_ERF) return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
    return v;
}
template <int ACT>
__device__ __forceinline__ float actdf(float v) {
    if (ACT == MAGE_ACT_RELU) return v > 0.f ? 1.f : 0.f;
    if (ACT == MAGE_ACT_QUICKGELU) {
        const float s = 1.f / (1.f + expf(-1.702f * v));
        return s * (1.f + 1.702f * v * (1.f - s));
    }
    if (ACT == MAGE_ACT_GELU_ERF)
        return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
    if (ACT == MAGE_ACT_TANH) return 1.f - v * v;       // backward only, and v is the OUTPUT y = tanh(.)
    return 1.f;
}
// BWD = 0: y = act(x);  BWD = 1: y = dy * act'(x)   (x = the saved pre-activation)
template <typename T, int ACT, int BWD>
__global__ __launch_bounds__(256) void act_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ y, long n) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const f32x4 v = load4(x + i);
    f32x4 o;
    if (BWD) {
        const f32x4 g = load4(dy + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = g[e] * actdf<ACT>(v[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = actf<ACT>(v[e]);
    }
    store4(y + i, o);
}

// ------------------------------------------------------------------------------------------------ cross entropy backward
// dlogits[i][k] = (softmax(logits[i])[k] - [k == target[i]]) * scale   (scale = upstream gradient / rows), one wave per row
template <typename OT>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, long rows,
                                                     int K, const float* __restrict__ gout, float inv_rows, OT* __restrict__ dl) {
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
    const float scale = gout[0] * inv_rows, inv = 1.0f / s;
    long tg = target[i];
    if (tg < 0 || tg >= K) tg = -1;                  // reported by the forward kernel (mage_cross_entropy)
    OT* o = dl + i * K;
    for (int k = lane; k < K; k += 64) o[k] = from_f32<OT>((expf(p[k] - mx) * inv - (k == tg ? 1.f : 0.f)) * scale);
}

// ------------------------------------------------------------------------------------------------ embedding backward
// dtable[ids[i]][:] += dout[orow(i)][:]   (orow as in mage_embedding; rows with ids[i] == padding_idx are skipped)
template <typename T>
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const int64_t* __restrict__ ids, const T* __restrict__ dout,
                                                            float* __restrict__ dtable, long n, int C, int n_table, long padding_idx,
                                                            long group, long group_stride, long off) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const long id = ids[i];
    if (id < 0 || id >= n_table || id == padding_idx) return;
    const long orow = (i / group) * group_stride + (i % group) + off;
    const T* src = dout + orow * C;
    float* dst = dtable + id * C;
    for (int c = lane; c < C; c += 64) atomicAdd(dst + c, to_f32<T>(src[c]));
}

// The same scatter for small tables (n_table * 256 B of LDS: the 512-entry visual token table): a workgroup owns a 64-channel slice and
// a chunk of the rows, accumulates into its private LDS copy of the slice with LDS atomics, and flushes the non-zero entries with one
// global atomic each: 262144 x 512 global atomics on 512 hot rows (2.1 ms per call) become 64 x 512 x 512.
template <typename T>
__global__ __launch_bounds__(512) void embedding_bwd_lds_kernel(const int64_t* __restrict__ ids, const T* __restrict__ dout,
                                                                float* __restrict__ dtable, long n, int C, int n_table, long padding_idx,
                                                                long group, long group_stride, long off, long rows_per_chunk,
                                                                float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* tab = (float*)smem_raw;                                        // [n_table][64]
    const int c0 = blockIdx.y * 64, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int e = threadIdx.x; e < n_table * 64; e += 512) tab[e] = 0.f;
    __syncthreads();
    const long i0 = (long)blockIdx.x * rows_per_chunk, i1 = min(n, i0 + rows_per_chunk);
    // U rows per wave in flight (one row at a time the kernel ran at one global round trip per row: 1 ms per 250 k rows against ~0.1 ms of bytes)
    constexpr int U = 16;
    for (long ib = i0 + wave; ib < i1; ib += 8 * U) {
        long id[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = ib + 8 * u;
            const long ii = i < i1 ? i : i0;                                // the row's address does not wait for its id
            id[u] = ids[ii];
            const bool ok = i < i1 && id[u] >= 0 && id[u] < n_table && id[u] != padding_idx;
            if (!ok) id[u] = -1;
            // 32-bit quotient (n, group < 2^31: host check): the two 64-bit divisions per row were most of this kernel's time
            const unsigned q = (unsigned)ii / (unsigned)group;
            const long orow = (long)q * group_stride + (long)((unsigned)ii - q * (unsigned)group) + off;
            v[u] = to_f32<T>(dout[orow * C + c0 + lane]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (id[u] >= 0) atomicAdd(&tab[id[u] * 64 + lane], v[u]);
    }
    __syncthreads();
    if (part) {                                                           // this chunk's table slice, plain stores: summed in chunk order by
        float* pp = part + (long)blockIdx.x * n_table * C;                // embedding_bwd_reduce_kernel (no global atomics, deterministic)
        for (int e = threadIdx.x; e < n_table * 64; e += 512) pp[(long)(e >> 6) * C + c0 + (e & 63)] = tab[e];
        return;
    }
    for (int e = threadIdx.x; e < n_table * 64; e += 512) {
        const float v = tab[e];
        if (v != 0.f) atomicAdd(dtable + (long)(e >> 6) * C + c0 + (e & 63), v);
    }
}

// The DETERMINISTIC form of the same scatter (scratch given): the workgroup's geometry is unchanged -- a 64-channel slice, a chunk of the rows,
// an LDS table of the slice -- but the WAVES split the slice's channels instead of the chunk's rows: wave w owns channels 8w .. 8w + 7, a wave
// instruction covers 8 rows x 8 channels (32 bytes of bf16 / 64 of fp32 per row), and the 8 rows are added one after the other in ascending
// order (LDS adds of one wave execute in program order; no other wave touches these channels).  Every (code, channel) sum therefore runs
// over the chunk's rows in ascending row order, whatever the scheduling: with the chunk-order sum of embedding_bwd_reduce_kernel the whole
// gradient is a fixed-order fp32 sum, bit-identical from run to run.  (The row-split kernel above let 8 waves race their LDS atomics on the
// same entries: associativity differences of ~1 ulp per step, enough to move a trained model's near-tie token decisions between runs.)
template <typename T>
__global__ __launch_bounds__(512) void embedding_bwd_det_kernel(const int64_t* __restrict__ ids, const T* __restrict__ dout, long n, int C, int n_table,
                                                                long padding_idx, long group, long group_stride, long off, long rows_per_chunk,
                                                                float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* tab = (float*)smem_raw;                                        // [n_table][64]
    const int c0 = blockIdx.y * 64, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int e = threadIdx.x; e < n_table * 64; e += 512) tab[e] = 0.f;
    __syncthreads();
    const long i0 = (long)blockIdx.x * rows_per_chunk, i1 = min(n, i0 + rows_per_chunk);
    const int rs = lane >> 3, ch = wave * 8 + (lane & 7);                  // row slot of the instruction, channel inside the slice
    constexpr int U = 8;                                                   // 8-row groups in flight per wave
    for (long ib = i0; ib < i1; ib += 8 * U) {
        long id[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = ib + 8 * u + rs;
            const long ii = i < i1 ? i : i0;
            id[u] = ids[ii];
            const bool ok = i < i1 && id[u] >= 0 && id[u] < n_table && id[u] != padding_idx;
            if (!ok) id[u] = -1;
            const unsigned q = (unsigned)ii / (unsigned)group;
            const long orow = (long)q * group_stride + (long)((unsigned)ii - q * (unsigned)group) + off;
            v[u] = to_f32<T>(dout[orow * C + c0 + ch]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {                                  // the instruction's 8 rows, ascending: one exec-masked LDS add each
                MAGE_DASSERT(id[u] < n_table && ch < 64);
                if (rs == r && id[u] >= 0) atomicAdd(&tab[id[u] * 64 + ch], v[u]);
                __builtin_amdgcn_wave_barrier();                           // keeps the eight adds eight instructions, in this order
            }
        }
    }
    __syncthreads();
    float* pp = part + (long)blockIdx.x * n_table * C;
    for (int e = threadIdx.x; e < n_table * 64; e += 512) pp[(long)(e >> 6) * C + c0 + (e & 63)] = tab[e];
}

// dtable[e] += sum over chunks (ascending) of part[chunk][e]: the flush of embedding_bwd_lds_kernel without global atomics (the 64 chunks'
// atomics on the same 1 MB table were 0.8 of the kernel's 1.0 ms)
__global__ __launch_bounds__(256) void embedding_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ dtable, long n_elem, int n_chunk) {
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= n_elem) return;
    f32x4 a = *(const f32x4*)(dtable + e);
    for (int c = 0; c < n_chunk; ++c) a += *(const f32x4*)(part + (long)c * n_elem + e);
    *(f32x4*)(dtable + e) = a;
}

// ------------------------------------------------------------------------------------------------ grouped row sums
// out[g][c] = sum over rows r with (r / div) % mod == g of w(r) * x[r][c],  w(r) = rs ? rs[r / rs_div] : 1.
// Gradients of broadcast row tables (T / H / W positional embeddings, text positions) and of the speed embedding.
template <typename T>
__global__ __launch_bounds__(256) void group_rowsum_kernel(const T* __restrict__ x, long rows, int C, long div, long mod,
                                                           const float* __restrict__ rs, long rs_div, float* __restrict__ out) {
    const long g = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    const long period = div * mod, nper = (rows + period - 1) / period;
    // blockIdx.z = chunk of the (period, row-in-group) index space: partial sums out[chunk][g][c] for mage_sum_partials
    const long total = nper * div, per = (total + gridDim.z - 1) / gridDim.z;
    const long i0 = (long)blockIdx.z * per, i1 = min(total, i0 + per);
    for (long i = i0; i < i1; ++i) {
        const long q = i / div, j = i - q * div;
        const long r = q * period + g * div + j;
        if (r < rows) s += (rs ? rs[r / rs_div] : 1.f) * to_f32<T>(x[r * C + c]);
    }
    out[((long)blockIdx.z * mod + g) * C + c] = s;
}

// ------------------------------------------------------------------------------------------------ dropout
// Stateless mask: keep(i) = hash(seed, i) >= p * 2^32, recomputed identically in the backward pass (no mask tensor).
// y = (accumulate ? y : 0) + x * keep / (1 - p)      x: T, y: YT
template <typename T, typename YT>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, YT* __restrict__ y, long n, unsigned thresh, float inv_keep,
                                                      unsigned long long seed, int accumulate) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const f32x4 v = load4(x + i);
    f32x4 o = accumulate ? load4(y + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (drop_keep(seed * 0x9e3779b97f4a7c15ULL, (unsigned long long)(i + e), thresh)) o[e] += v[e] * inv_keep;
    store4(y + i, o);
}

// Backward of the decoder head's fold + tanh (mage_convt_fold_tanh): ds = g * (1 - y^2) per output pixel (NCHW), scattered back to
// the per-input-pixel tap products:  dtaps[(n, iy, ix), (ky*4 + kx)*cout + co] = ds[n, co, 2 iy - 1 + ky, 2 ix - 1 + kx]  (0 outside)
__global__ __launch_bounds__(256) void convt_unfold_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ dtaps,
                                                           int N, int IH, int IW, int cout) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int ld = 16 * cout;
    if (gid >= (long)N * IH * IW * ld) return;
    const int col = (int)(gid % ld), co = col % cout, tap = col / cout, ky = tap >> 2, kx = tap & 3;
    const long pix = gid / ld;
    const int ix = (int)(pix % IW), iy = (int)((pix / IW) % IH), n = (int)(pix / ((long)IW * IH));
    const int oy = 2 * iy - 1 + ky, ox = 2 * ix - 1 + kx, OH = 2 * IH, OW = 2 * IW;
    float v = 0.f;
    if ((unsigned)oy < (unsigned)OH && (unsigned)ox < (unsigned)OW) {
        const long o = (((long)n * cout + co) * OH + oy) * OW + ox;
        v = y ? g[o] * (1.f - y[o] * y[o]) : g[o];
    }
    dtaps[gid] = v;
}

template <typename T>
int transpose_launch(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t y_row0, int64_t M, int64_t Mp, int32_t C, int32_t out_h,
                     int32_t out_w, int32_t in_h, int32_t in_w, int64_t img_stride, int64_t a_off, int32_t dy, int32_t dx, int32_t stride,
                     hipStream_t s) {
    const dim3 grid((unsigned)((Mp + 63) / 64), (unsigned)((C + 63) / 64));
    if constexpr (sizeof(T) == 2) {
        if (C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && Mp % 8 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
            hipLaunchKernelGGL(transpose8_kernel, grid, dim3(256), 0, s, (const unsigned short*)x, (long)ldx, (unsigned short*)y, (long)ldy,
                               (long)y_row0, (long)M, (long)Mp, C, out_h, out_w, in_h, in_w, (long)img_stride, (long)a_off, dy, dx, stride);
            MAGE_CHECK_LAUNCH("mage_transpose");
            return MAGE_OK;
        }
    }
    hipLaunchKernelGGL((transpose_kernel<T>), grid, dim3(256), 0, s, (const T*)x, (long)ldx, (T*)y, (long)ldy, (long)y_row0, (long)M,
                       (long)Mp, C, out_h, out_w, in_h, in_w, (long)img_stride, (long)a_off, dy, dx, stride);
    MAGE_CHECK_LAUNCH("mage_transpose");
    return MAGE_OK;
}

template <typename T, int BWD>
int act_launch(const void* x, const void* dy, void* y, int64_t n, int32_t act, hipStream_t s) {
    const dim3 grid((unsigned)((n / 4 + 255) / 256)), blk(256);
    switch (act) {
        case MAGE_ACT_RELU: hipLaunchKernelGGL((act_kernel<T, MAGE_ACT_RELU, BWD>), grid, blk, 0, s, (const T*)x, (const T*)dy, (T*)y, (long)n); break;
        case MAGE_ACT_QUICKGELU: hipLaunchKernelGGL((act_kernel<T, MAGE_ACT_QUICKGELU, BWD>), grid, blk, 0, s, (const T*)x, (const T*)dy, (T*)y, (long)n); break;
        case MAGE_ACT_GELU_ERF: hipLaunchKernelGGL((act_kernel<T, MAGE_ACT_GELU_ERF, BWD>), grid, blk, 0, s, (const T*)x, (const T*)dy, (T*)y, (long)n); break;
        case MAGE_ACT_TANH:
            if (BWD) { hipLaunchKernelGGL((act_kernel<T, MAGE_ACT_TANH, BWD>), grid, blk, 0, s, (const T*)x, (const T*)dy, (T*)y, (long)n); break; }
            [[fallthrough]];
        default: mage_set_error("mage_act: activation %d unsupported", act); return MAGE_EINVAL;
    }
    MAGE_CHECK_LAUNCH("mage_act");
    return MAGE_OK;
}

}  // namespace

extern "C" int mage_transpose(const void* x, int32_t dtype, int64_t ldx, void* y, int64_t ldy, int64_t y_row0, int64_t M, int64_t Mp,
                              int32_t C, int32_t out_h, int32_t out_w, int32_t in_h, int32_t in_w, int64_t img_stride, int64_t a_off,
                              int32_t dy, int32_t dx, int32_t stride, void* stream) {
    MAGE_CHECK_ARG(x && y && M > 0 && Mp >= M && C > 0 && out_h >= 1 && out_w >= 1 && in_h >= 1 && in_w >= 1 && ldy >= Mp && stride >= 1,
                   "mage_transpose: bad arguments");
    MAGE_CHECK_ARG(ldx >= C, "mage_transpose: ldx=%ld < C=%d (rows would alias)", (long)ldx, C);
    hipStream_t s = (hipStream_t)stream;
    DT_DISPATCH(dtype, (transpose_launch<float>(x, ldx, y, ldy, y_row0, M, Mp, C, out_h, out_w, in_h, in_w, img_stride, a_off, dy, dx, stride, s)),
                (transpose_launch<unsigned short>(x, ldx, y, ldy, y_row0, M, Mp, C, out_h, out_w, in_h, in_w, img_stride, a_off, dy, dx, stride, s)),
                "mage_transpose");
}


extern "C" int mage_transpose_colsum(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int64_t Mp, int32_t C, int32_t out_w,
                                     int64_t img_stride, int64_t a_off, float* colsum, int32_t n_part, void* stream) {
    const long tiles = (Mp + 63) / 64;
    MAGE_CHECK_ARG(x && y && colsum && M > 0 && Mp >= M && C > 0 && out_w >= 1 && ldy >= Mp, "mage_transpose_colsum: bad arguments");
    MAGE_CHECK_ARG(ldx >= C, "mage_transpose_colsum: ldx=%ld < C=%d (rows would alias)", (long)ldx, C);
    MAGE_CHECK_ARG(C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && Mp % 8 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0,
                   "mage_transpose_colsum: bf16 operands with 16-byte rows");
    MAGE_CHECK_ARG(n_part == (int)((tiles + TRANSPOSE_TPW - 1) / TRANSPOSE_TPW), "mage_transpose_colsum: n_part must be ceil(ceil(Mp/64)/%d)",
                   TRANSPOSE_TPW);
    // rows regrouped like mage_transpose with out_h = 1 (row m -> (m / out_w) * img_stride + m % out_w + a_off), no tap shift
    hipLaunchKernelGGL(transpose8_colsum_kernel, dim3(n_part, (C + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x,
                       (long)ldx, (unsigned short*)y, (long)ldy, (long)M, (long)Mp, C, 1, out_w, 1, out_w, (long)img_stride, (long)a_off, colsum);
    MAGE_CHECK_LAUNCH("mage_transpose_colsum");
    return MAGE_OK;
}

extern "C" int mage_convt_unfold_tanh_bwd(const float* grad_y, const float* y, float* dtaps, int32_t N, int32_t IH, int32_t IW, int32_t cout,
                                          void* stream) {
    MAGE_CHECK_ARG(grad_y && dtaps && N > 0 && IH > 0 && IW > 0 && cout >= 1 && cout <= 4, "mage_convt_unfold_tanh_bwd: bad arguments");
    const long total = (long)N * IH * IW * 16 * cout;
    hipLaunchKernelGGL(convt_unfold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_y, y, dtaps, N, IH,
                       IW, cout);
    MAGE_CHECK_LAUNCH("mage_convt_unfold_tanh_bwd");
    return MAGE_OK;
}

extern "C" int mage_row_sum(const void* x, int32_t dtype, int64_t ld, int64_t n, int32_t rows, float* out, int32_t n_chunk, void* stream) {
    MAGE_CHECK_ARG(x && out && rows > 0 && n > 0 && n_chunk >= 1, "mage_row_sum: bad arguments");
    const dim3 grid((rows + 3) / 4, n_chunk), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MAGE_F32) hipLaunchKernelGGL((row_sum_kernel<float>), grid, blk, 0, s, (const float*)x, (long)ld, (long)n, rows, out);
    else if (dtype == MAGE_BF16) hipLaunchKernelGGL((row_sum_kernel<unsigned short>), grid, blk, 0, s, (const unsigned short*)x, (long)ld, (long)n, rows, out);
    else { mage_set_error("mage_row_sum: bad dtype %d", dtype); return MAGE_EINVAL; }
    MAGE_CHECK_LAUNCH("mage_row_sum");
    return MAGE_OK;
}

extern "C" int mage_sum_partials(const float* part, int64_t stride, int32_t n_part, int64_t n, float* out, int32_t accumulate, void* stream) {
    MAGE_CHECK_ARG(part && out && n_part > 0 && n > 0, "mage_sum_partials: bad arguments");
    if (n % 4 == 0 && stride % 4 == 0 && n_part >= 4 && ((((uintptr_t)part | (uintptr_t)out) & 15) == 0)) {
        hipLaunchKernelGGL(sum_partials4_kernel, dim3((unsigned)((n / 4 + 63) / 64)), dim3(256), 0, (hipStream_t)stream, part, (long)stride, n_part,
                           (long)(n / 4), out, accumulate);
        MAGE_CHECK_LAUNCH("mage_sum_partials");
        return MAGE_OK;
    }
    hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, (long)stride, n_part,
                       (long)n, out, accumulate);
    MAGE_CHECK_LAUNCH("mage_sum_partials");
    return MAGE_OK;
}

extern "C" int mage_act(const void* x, void* y, int32_t dtype, int64_t n, int32_t act, void* stream) {
    MAGE_CHECK_ARG(x && y && n > 0 && n % 4 == 0, "mage_act: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    DT_DISPATCH(dtype, (act_launch<float, 0>(x, nullptr, y, n, act, s)), (act_launch<unsigned short, 0>(x, nullptr, y, n, act, s)), "mage_act");
}

extern "C" int mage_act_bwd(const void* x, const void* dy, void* dx, int32_t dtype, int64_t n, int32_t act, void* stream) {
    MAGE_CHECK_ARG(x && dy && dx && n > 0 && n % 4 == 0, "mage_act_bwd: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    DT_DISPATCH(dtype, (act_launch<float, 1>(x, dy, dx, n, act, s)), (act_launch<unsigned short, 1>(x, dy, dx, n, act, s)), "mage_act_bwd");
}

extern "C" int mage_cross_entropy_bwd(const float* logits, const int64_t* target, int64_t rows, int32_t K, const float* grad_out,
                                      void* dlogits, int32_t dl_dtype, void* stream) {
    MAGE_CHECK_ARG(logits && target && grad_out && dlogits && rows > 0 && K > 0, "mage_cross_entropy_bwd: bad arguments");
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (dl_dtype == MAGE_F32)
        hipLaunchKernelGGL((ce_bwd_kernel<float>), grid, blk, 0, s, logits, target, (long)rows, K, grad_out, 1.0f / (float)rows, (float*)dlogits);
    else if (dl_dtype == MAGE_BF16)
        hipLaunchKernelGGL((ce_bwd_kernel<unsigned short>), grid, blk, 0, s, logits, target, (long)rows, K, grad_out, 1.0f / (float)rows,
                           (unsigned short*)dlogits);
    else { mage_set_error("mage_cross_entropy_bwd: bad dtype %d", dl_dtype); return MAGE_EINVAL; }
    MAGE_CHECK_LAUNCH("mage_cross_entropy_bwd");
    return MAGE_OK;
}

extern "C" int mage_embedding_bwd(const int64_t* ids, const void* dout, int32_t dout_dtype, float* dtable, int64_t n, int32_t C,
                                  int32_t n_table, int64_t padding_idx, int64_t group, int64_t group_stride, int64_t off, float* scratch,
                                  int64_t scratch_floats, void* stream) {
    MAGE_CHECK_ARG(ids && dout && dtable && n > 0 && C > 0 && n_table > 0 && group > 0, "mage_embedding_bwd: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const bool small_tab = n_table <= 512 && C % 64 == 0 && n < (1L << 31) && group < (1L << 31) && (dout_dtype == MAGE_F32 || dout_dtype == MAGE_BF16);
    if (small_tab && (n >= 8192 || scratch)) {
        const int n_chunk = (int)(n / 4096 < 64 ? (n + 4095) / 4096 : 64);
        const long rpc = (((n + n_chunk - 1) / n_chunk) + 7) & ~7L;       // whole 8-row groups per chunk (the deterministic kernel's unit)
        const dim3 grid(n_chunk, C / 64), blk(512);
        const size_t lds = (size_t)n_table * 64 * sizeof(float);
        float* part = (scratch && scratch_floats >= (int64_t)n_chunk * n_table * C && (((uintptr_t)scratch | (uintptr_t)dtable) & 15) == 0) ? scratch : nullptr;
        if (part) {                                                       // deterministic: channel-split waves, rows in ascending order, chunk-order sum
            static bool attr_det[MAGE_MAX_DEVICES][2] = {{false}};
            const int dev_ = mage_device_index();
            MAGE_CHECK_ARG(dev_ >= 0, "mage_embedding_bwd: no current device");
            const int ti = dout_dtype == MAGE_F32 ? 0 : 1;
            if (!attr_det[dev_][ti]) {
                if (ti == 0) (void)hipFuncSetAttribute((const void*)embedding_bwd_det_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
                else (void)hipFuncSetAttribute((const void*)embedding_bwd_det_kernel<unsigned short>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
                attr_det[dev_][ti] = true;
            }
            if (ti == 0)
                hipLaunchKernelGGL((embedding_bwd_det_kernel<float>), grid, blk, lds, s, ids, (const float*)dout, (long)n, C, n_table, (long)padding_idx,
                                   (long)group, (long)group_stride, (long)off, rpc, part);
            else
                hipLaunchKernelGGL((embedding_bwd_det_kernel<unsigned short>), grid, blk, lds, s, ids, (const unsigned short*)dout, (long)n, C, n_table,
                                   (long)padding_idx, (long)group, (long)group_stride, (long)off, rpc, part);
            const long n_elem = (long)n_table * C;
            hipLaunchKernelGGL(embedding_bwd_reduce_kernel, dim3((unsigned)((n_elem / 4 + 255) / 256)), dim3(256), 0, s, part, dtable, n_elem, n_chunk);
            MAGE_CHECK_LAUNCH("mage_embedding_bwd");
            return MAGE_OK;
        }
        static bool attr_set[MAGE_MAX_DEVICES][2] = {{false}};
        const int dev = mage_device_index();
        MAGE_CHECK_ARG(dev >= 0, "mage_embedding_bwd: no current device");
        if (dout_dtype == MAGE_F32) {
            if (!attr_set[dev][0]) {
                (void)hipFuncSetAttribute((const void*)embedding_bwd_lds_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
                attr_set[dev][0] = true;
            }
            hipLaunchKernelGGL((embedding_bwd_lds_kernel<float>), grid, blk, lds, s, ids, (const float*)dout, dtable, (long)n, C, n_table,
                               (long)padding_idx, (long)group, (long)group_stride, (long)off, rpc, part);
        } else {
            if (!attr_set[dev][1]) {
                (void)hipFuncSetAttribute((const void*)embedding_bwd_lds_kernel<unsigned short>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          128 * 1024);
                attr_set[dev][1] = true;
            }
            hipLaunchKernelGGL((embedding_bwd_lds_kernel<unsigned short>), grid, blk, lds, s, ids, (const unsigned short*)dout, dtable, (long)n, C,
                               n_table, (long)padding_idx, (long)group, (long)group_stride, (long)off, rpc, part);
        }
        if (part) {
            const long n_elem = (long)n_table * C;
            hipLaunchKernelGGL(embedding_bwd_reduce_kernel, dim3((unsigned)((n_elem / 4 + 255) / 256)), dim3(256), 0, s, part, dtable, n_elem, n_chunk);
        }
        MAGE_CHECK_LAUNCH("mage_embedding_bwd");
        return MAGE_OK;
    }
    const dim3 grid((unsigned)((n + 3) / 4)), blk(256);
    if (dout_dtype == MAGE_F32)
        hipLaunchKernelGGL((embedding_bwd_kernel<float>), grid, blk, 0, s, ids, (const float*)dout, dtable, (long)n, C, n_table, (long)padding_idx,
                           (long)group, (long)group_stride, (long)off);
    else if (dout_dtype == MAGE_BF16)
        hipLaunchKernelGGL((embedding_bwd_kernel<unsigned short>), grid, blk, 0, s, ids, (const unsigned short*)dout, dtable, (long)n, C, n_table,
                           (long)padding_idx, (long)group, (long)group_stride, (long)off);
    else { mage_set_error("mage_embedding_bwd: bad dtype %d", dout_dtype); return MAGE_EINVAL; }
    MAGE_CHECK_LAUNCH("mage_embedding_bwd");
    return MAGE_OK;
}

extern "C" int mage_group_rowsum(const void* x, int32_t dtype, int64_t rows, int32_t C, int64_t div, int64_t mod, const float* row_scale,
                                 int64_t row_scale_div, float* out, int32_t n_chunk, void* stream) {
    MAGE_CHECK_ARG(x && out && rows > 0 && C > 0 && div >= 1 && mod >= 1 && n_chunk >= 1 && n_chunk <= 65535 && (!row_scale || row_scale_div >= 1),
                   "mage_group_rowsum: bad arguments");
    const dim3 grid((unsigned)mod, (C + 255) / 256, n_chunk), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MAGE_F32)
        hipLaunchKernelGGL((group_rowsum_kernel<float>), grid, blk, 0, s, (const float*)x, (long)rows, C, (long)div, (long)mod, row_scale,
                           (long)row_scale_div, out);
    else if (dtype == MAGE_BF16)
        hipLaunchKernelGGL((group_rowsum_kernel<unsigned short>), grid, blk, 0, s, (const unsigned short*)x, (long)rows, C, (long)div, (long)mod,
                           row_scale, (long)row_scale_div, out);
    else { mage_set_error("mage_group_rowsum: bad dtype %d", dtype); return MAGE_EINVAL; }
    MAGE_CHECK_LAUNCH("mage_group_rowsum");
    return MAGE_OK;
}

extern "C" int mage_dropout(const void* x, int32_t x_dtype, void* y, int32_t y_dtype, int64_t n, float p, uint64_t seed, int32_t accumulate,
                            void* stream) {
    MAGE_CHECK_ARG(x && y && n > 0 && n % 4 == 0 && p >= 0.f && p < 1.f, "mage_dropout: bad arguments");
    const DropMask m(p, seed);
    const dim3 grid((unsigned)((n / 4 + 255) / 256)), blk(256);
    hipStream_t s = (hipStream_t)stream;
#define DROP(T, YT) hipLaunchKernelGGL((dropout_kernel<T, YT>), grid, blk, 0, s, (const T*)x, (YT*)y, (long)n, m.thresh, m.inv_keep, (unsigned long long)seed, accumulate)
    if (x_dtype == MAGE_F32 && y_dtype == MAGE_F32) DROP(float, float);
    else if (x_dtype == MAGE_BF16 && y_dtype == MAGE_BF16) DROP(unsigned short, unsigned short);
    else if (x_dtype == MAGE_BF16 && y_dtype == MAGE_F32) DROP(unsigned short, float);
    else if (x_dtype == MAGE_F32 && y_dtype == MAGE_BF16) DROP(float, unsigned short);
    else { mage_set_error("mage_dropout: bad dtypes %d %d", x_dtype, y_dtype); return MAGE_EINVAL; }
#undef DROP
    MAGE_CHECK_LAUNCH("mage_dropout");
    return MAGE_OK;
}

// Backward of MaxPool2d(2) and of Upsample(scale 2, nearest) of the f8 VQ-VAE (vqvae_model.py:194-210), channels-last fp32.
namespace {
// dx of the 2x2 window = dy at the FIRST maximum in scan order (PyTorch's tie rule), zero elsewhere; one thread per output pixel x 4 channels.
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int N,
                                                           int H, int W, int C) {
    const int cq = C / 4, OH = H / 2, OW = W / 2;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)N * OH * OW * cq) return;
    const int c = (int)(gid % cq) * 4;
    const long pix = gid / cq;
    const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), n = (int)(pix / ((long)OW * OH));
    const long base = (((long)n * H + oy * 2) * W + ox * 2) * C + c;
    const long off[4] = {0, (long)C, (long)W * C, (long)W * C + C};
    f32x4 v[4], o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = *(const f32x4*)(x + base + off[k]);
        o[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const f32x4 g = *(const f32x4*)(dy + pix * C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int best = 0;
        float m = v[0][e];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (v[k][e] > m) {
                m = v[k][e];
                best = k;
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == best) o[k][e] = g[e];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) *(f32x4*)(dx + base + off[k]) = o[k];
}

// dx[n, y, x] = sum of the 2x2 block of dy it was copied to.
__global__ __launch_bounds__(256) void upsample2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N, int H, int W, int C) {
    const int cq = C / 4;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)N * H * W * cq) return;
    const int c = (int)(gid % cq) * 4;
    const long pix = gid / cq;
    const int ix = (int)(pix % W), iy = (int)((pix / W) % H), n = (int)(pix / ((long)W * H));
    const long base = (((long)n * 2 * H + iy * 2) * 2 * W + ix * 2) * C + c;
    const f32x4 s = (*(const f32x4*)(dy + base) + *(const f32x4*)(dy + base + C)) +
                    (*(const f32x4*)(dy + base + (long)2 * W * C) + *(const f32x4*)(dy + base + (long)2 * W * C + C));
    *(f32x4*)(dx + pix * C + c) = s;
}
}  // namespace

extern "C" int mage_maxpool2_bwd(const float* x, const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    MAGE_CHECK_ARG(x && dy && dx && N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "mage_maxpool2_bwd: bad arguments");
    const long items = (long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, N, H, W, C);
    MAGE_CHECK_LAUNCH("mage_maxpool2_bwd");
    return MAGE_OK;
}

extern "C" int mage_upsample2_bwd(const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    MAGE_CHECK_ARG(dy && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "mage_upsample2_bwd: bad arguments");
    const long items = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(upsample2_bwd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, N, H, W, C);
    MAGE_CHECK_LAUNCH("mage_upsample2_bwd");
    return MAGE_OK;
}

// y = r + dropout(x): the residual add of x + dropout(Linear(.)) (mage_model.py:48,52) without first copying r into y.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void dropout_add_kernel(const T* __restrict__ x, const float* __restrict__ r, float* __restrict__ y, long n,
                                                          unsigned thresh, float inv_keep, unsigned long long seed,
                                                          unsigned short* __restrict__ yb) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const f32x4 v = load4(x + i);
    f32x4 o = *(const f32x4*)(r + i);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (drop_keep(seed * 0x9e3779b97f4a7c15ULL, (unsigned long long)(i + e), thresh)) o[e] += v[e] * inv_keep;
    *(f32x4*)(y + i) = o;
    if (yb) store4(yb + i, o);
}
}  // namespace

extern "C" int mage_dropout_add(const void* x, int32_t x_dtype, const float* r, float* y, void* y_bf16, int64_t n, float p, uint64_t seed,
                                void* stream) {
    MAGE_CHECK_ARG(x && r && y && n > 0 && n % 4 == 0 && p >= 0.f && p < 1.f && ((uintptr_t)y_bf16 & 7) == 0, "mage_dropout_add: bad arguments");
    const DropMask m(p, seed);
    const dim3 grid((unsigned)((n / 4 + 255) / 256)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == MAGE_F32) hipLaunchKernelGGL((dropout_add_kernel<float>), grid, blk, 0, s, (const float*)x, r, y, (long)n, m.thresh, m.inv_keep, (unsigned long long)seed, (unsigned short*)y_bf16);
    else if (x_dtype == MAGE_BF16) hipLaunchKernelGGL((dropout_add_kernel<unsigned short>), grid, blk, 0, s, (const unsigned short*)x, r, y, (long)n, m.thresh, m.inv_keep, (unsigned long long)seed, (unsigned short*)y_bf16);
    else { mage_set_error("mage_dropout_add: bad dtype %d", x_dtype); return MAGE_EINVAL; }
    MAGE_CHECK_LAUNCH("mage_dropout_add");
    return MAGE_OK;
}
