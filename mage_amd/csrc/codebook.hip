// Codebook statistics and the EMA codebook update of stage-1 (VQ-VAE) training: mage_code_stats, mage_codebook_ema (include/mage_hip_ext.h
// states both rules).  No site in the reference: its codebook is moved by the gradient of mse(z_q_x, z_e_x.detach()) alone.
#include "common.h"
#include "../../include/mage_hip_ext.h"

// every fp64 operation of the update rule is rounded on its own, as the header states it: no a * b + c contraction in this file
#pragma clang fp contract(off)

#define MAGE_CODE_MAX_K 1024
#define MAGE_CODE_MAX_D 1024

// chunks of rows: a function of `rows` alone (the header states it; ops.code_stats sizes the scratch from the same formula)
static inline int code_chunks(int64_t rows) { return (int)(rows / 4096 < 64 ? (rows + 4095) / 4096 : 64); }

// ------------------------------------------------------------------------------------------------ per-code counts and row sums
// embedding_bwd_det_kernel's geometry (train.hip) over encoder rows: a workgroup owns a chunk of the rows and a slice of 8 * CW channels with
// an LDS table [K][8 * CW] of the slice; wave w owns channels CW w .. CW w + CW - 1 of the slice, one wave instruction covers 64 / CW rows
// x CW channels, and the rows of an instruction are added one after the other in ascending order (LDS adds of one wave execute in program
// order; no other wave touches these channels).  CW = 8 (a 64-channel slice) up to 512 codes, CW = 4 (32 channels) above: K x slice x 4 B
// stays within 128 KiB.  The workgroups of blockIdx.y == n_slices count: integer LDS adds, the chunk's counts as int32.
template <int CW>
__global__ __launch_bounds__(512) void code_stats_kernel(const int64_t* __restrict__ ids, const float* __restrict__ z, long rows, int D, long ldz,
                                                         int K, long rows_per_chunk, int n_slices, float* __restrict__ part,
                                                         int* __restrict__ cpart, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int CS = 8 * CW, RPI = 64 / CW, U = CW;                      // slice width, rows per instruction, instructions in flight (64 rows)
    const long i0 = min(rows, (long)blockIdx.x * rows_per_chunk), i1 = min(rows, i0 + rows_per_chunk);
    if ((int)blockIdx.y == n_slices) {
        int* cnt = (int*)smem_raw;                                          // [K]
        for (int k = threadIdx.x; k < K; k += 512) cnt[k] = 0;
        __syncthreads();
        for (long i = i0 + threadIdx.x; i < i1; i += 512) {
            const long id = ids[i];
            if (id < 0 || id >= K) mage_raise(err, MAGE_DEVERR_CODE_ID, id, K);      // reported by mage_check_device_errors; counted nowhere
            else atomicAdd(&cnt[id], 1);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += 512) cpart[(long)blockIdx.x * K + k] = cnt[k];
        return;
    }
    float* tab = (float*)smem_raw;                                          // [K][CS]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int e = threadIdx.x; e < K * CS; e += 512) tab[e] = 0.f;
    __syncthreads();
    const int c0 = blockIdx.y * CS, rs = lane / CW, ch = wave * CW + lane % CW;   // row slot of the instruction, channel inside the slice
    const bool cok = c0 + ch < D;                                           // the last slice of a D that is no multiple of the slice is ragged
    const long col = cok ? c0 + ch : 0;
    for (long ib = i0; ib < i1; ib += RPI * U) {
        long id[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = ib + RPI * u + rs;
            const long ii = i < i1 ? i : i0;                                // i0 < i1 <= rows here: a row of the chunk, its value unused
            id[u] = ids[ii];
            if (!(i < i1 && cok && id[u] >= 0 && id[u] < K)) id[u] = -1;
            v[u] = z[ii * ldz + col];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < RPI; ++r) {                                 // the instruction's rows, ascending: one exec-masked LDS add each
                MAGE_DASSERT(id[u] < K && ch < CS);
                if (rs == r && id[u] >= 0) atomicAdd(&tab[id[u] * CS + ch], v[u]);
                __builtin_amdgcn_wave_barrier();                            // keeps the adds separate instructions, in this order
            }
        }
    }
    __syncthreads();
    float* pp = part + (long)blockIdx.x * K * D;
    for (int e = threadIdx.x; e < K * CS; e += 512)
        if (c0 + e % CS < D) pp[(long)(e / CS) * D + c0 + e % CS] = tab[e];
}

// sums[e] = +0 + part[0][e] + part[1][e] + ... (chunks ascending); counts[k] = the int64 sum of the chunks' int32 counts
__global__ __launch_bounds__(256) void code_stats_reduce_kernel(const float* __restrict__ part, const int* __restrict__ cpart, float* __restrict__ sums,
                                                                int64_t* __restrict__ counts, long n_elem, int K, int n_chunk) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x, nq = n_elem / 4;
    if (t < nq) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < n_chunk; ++c) a += *(const f32x4*)(part + (long)c * n_elem + t * 4);
        *(f32x4*)(sums + t * 4) = a;
    } else if (t - nq < K) {
        const long k = t - nq;
        int64_t s = 0;
        for (int c = 0; c < n_chunk; ++c) s += cpart[(long)c * K + k];
        counts[k] = s;
    }
}

extern "C" int mage_code_stats(const int64_t* ids, const float* z, int64_t rows, int32_t D, int64_t ldz, int32_t K, int64_t* counts, float* sums,
                               void* scratch, int64_t scratch_bytes, void* stream) {
    MAGE_CHECK_ARG(ids && counts && scratch, "mage_code_stats: null ids, counts or scratch");
    MAGE_CHECK_ARG((z != nullptr) == (sums != nullptr), "mage_code_stats: z and sums are given together or not at all");
    MAGE_CHECK_ARG(rows > 0 && rows < (1LL << 31), "mage_code_stats: rows=%ld outside [1, 2^31)", (long)rows);
    MAGE_CHECK_ARG(K >= 1 && K <= MAGE_CODE_MAX_K, "mage_code_stats: K=%d outside [1, %d]", K, MAGE_CODE_MAX_K);
    if (sums) {
        MAGE_CHECK_ARG(D > 0 && D % 4 == 0 && D <= MAGE_CODE_MAX_D, "mage_code_stats: D=%d must be a multiple of 4 in [4, %d]", D, MAGE_CODE_MAX_D);
        MAGE_CHECK_ARG(ldz >= D && ldz < (1LL << 31), "mage_code_stats: ldz=%ld below D=%d (or 2^31 and above)", (long)ldz, D);
    }
    MAGE_CHECK_ARG((((uintptr_t)ids | (uintptr_t)counts) & 7) == 0 && ((uintptr_t)z & 3) == 0 && (((uintptr_t)sums | (uintptr_t)scratch) & 15) == 0,
                   "mage_code_stats: misaligned pointer (ids, counts: 8 bytes; z: 4; sums, scratch: 16)");
    const int n_chunk = code_chunks(rows);
    const long n_elem = sums ? (long)K * D : 0;
    const int64_t need = (int64_t)n_chunk * (n_elem + K) * 4;
    MAGE_CHECK_ARG(scratch_bytes >= need, "mage_code_stats: scratch of %ld bytes, %ld needed (%d chunks)", (long)scratch_bytes, (long)need, n_chunk);
    int* err = mage_error_word();
    MAGE_CHECK_ARG(err != nullptr, "mage_code_stats: mage_init() has not been called");
    const long rpc = (((rows + n_chunk - 1) / n_chunk) + 7) & ~7L;
    float* part = (float*)scratch;
    int* cpart = (int*)(part + (long)n_chunk * n_elem);
    hipStream_t s = (hipStream_t)stream;
    const bool wide = K <= 512;                                            // 64-channel slices
    const int cs = wide ? 64 : 32, n_slices = sums ? (D + cs - 1) / cs : 0;
    const size_t lds = sums ? (size_t)K * cs * sizeof(float) : (size_t)K * sizeof(int);
    static bool attr[MAGE_MAX_DEVICES] = {false};
    const int dev = mage_device_index();
    MAGE_CHECK_ARG(dev >= 0, "mage_code_stats: no current device");
    if (!attr[dev]) {
        (void)hipFuncSetAttribute((const void*)code_stats_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)code_stats_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        attr[dev] = true;
    }
    const dim3 grid(n_chunk, n_slices + 1), blk(512);
    if (wide)
        hipLaunchKernelGGL((code_stats_kernel<8>), grid, blk, lds, s, ids, z, (long)rows, D, (long)ldz, K, rpc, n_slices, part, cpart, err);
    else
        hipLaunchKernelGGL((code_stats_kernel<4>), grid, blk, lds, s, ids, z, (long)rows, D, (long)ldz, K, rpc, n_slices, part, cpart, err);
    hipLaunchKernelGGL(code_stats_reduce_kernel, dim3((unsigned)((n_elem / 4 + K + 255) / 256)), dim3(256), 0, s, part, cpart, sums, counts, n_elem, K,
                       n_chunk);
    MAGE_CHECK_LAUNCH("mage_code_stats");
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------------------ EMA update, restart, usage statistics
// Arrival counter of the update's workgroups, 0 between launches.  Every workgroup needs the K cluster sizes from BEFORE the update (for the
// sum n), so none of them may be overwritten while another workgroup has yet to read them: each workgroup reads all K at its start and takes
// a ticket at its end, and the one that takes the last ticket -- every other workgroup has read by then -- writes the K new sizes, which it
// holds itself.  No value passes between workgroups (the counter orders a write after reads, nothing more), so the result has no order in it.
__device__ unsigned g_ema_ticket;

// one fp32 value of the rule: g a + (1 - g) b in fp64 from fp32 operands, each operation rounded on its own (no contraction), rounded once
__device__ __forceinline__ float ema_mix(double g, double omg, float a, double b) {
    return (float)__dadd_rn(__dmul_rn(g, (double)a), __dmul_rn(omg, b));
}

__global__ __launch_bounds__(256) void codebook_ema_kernel(float* __restrict__ cb, float* __restrict__ csize, float* __restrict__ esum,
                                                           const int64_t* __restrict__ counts, const float* __restrict__ sums,
                                                           const float* __restrict__ z, long rows, long ldz, int K, int D, double g, double eps,
                                                           float restart_below, float restart_size, unsigned long long ctr0,
                                                           double* __restrict__ stats) {
    __shared__ float Np[MAGE_CODE_MAX_K];                                   // N_k'
    __shared__ long cnt[MAGE_CODE_MAX_K];
    __shared__ double term[MAGE_CODE_MAX_K];                                // p_k ln p_k (workgroup 0)
    __shared__ double s_n;
    __shared__ long s_total;
    __shared__ int s_last;
    const double omg = __dsub_rn(1.0, g);
    for (int k = threadIdx.x; k < K; k += 256) {
        cnt[k] = counts[k];
        Np[k] = ema_mix(g, omg, csize[k], (double)cnt[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                 // k ascending, fp64: the same bits in every workgroup
        double n = 0.0;
        long total = 0;
        for (int k = 0; k < K; ++k) {
            n = __dadd_rn(n, (double)Np[k]);
            total += cnt[k];
        }
        s_n = n;
        s_total = total;
    }
    __syncthreads();
    if (blockIdx.x == 0) {                                                  // the statistics: every code's term by its own thread (a log each), then
        const long total = s_total;                                         // one thread adds the terms k ascending -- the order of a serial loop
        for (int k = threadIdx.x; k < K; k += 256) {
            double t = 0.0;                                                 // a zero count adds 0, never 0 * inf
            if (cnt[k] > 0) {
                const double p = __ddiv_rn((double)cnt[k], (double)total);
                t = __dmul_rn(p, log(p));
            }
            term[k] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double h = 0.0;
            long active = 0, restarted = 0;
            for (int k = 0; k < K; ++k) {
                if (cnt[k] > 0) {
                    h = __dsub_rn(h, term[k]);
                    ++active;
                }
                if (total > 0 && restart_below > 0.f && Np[k] < restart_below) ++restarted;
            }
            stats[0] = total > 0 ? exp(h) : __longlong_as_double(0x7ff8000000000000LL);
            stats[1] = (double)active;
            stats[2] = (double)restarted;
            stats[3] = (double)total;
        }
    }
    if (s_total == 0) return;                                               // every id was invalid: the state is left as it is
    const double n = s_n, den = __dadd_rn(n, __dmul_rn((double)K, eps));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int k = blockIdx.x * 4 + wave; k < K; k += gridDim.x * 4) {        // one wave per code
        const float npk = Np[k];
        float* e_row = cb + (long)k * D;
        float* m_row = esum + (long)k * D;
        if (restart_below > 0.f && npk < restart_below) {                   // dead: an encoder row, copied bit for bit
            const long r = (long)(((unsigned long long)hash32(ctr0 + (unsigned long long)k) * (unsigned long long)rows) >> 32);
            MAGE_DASSERT(r >= 0 && r < rows);
            const float* zr = z + r * ldz;
            for (int d = lane; d < D; d += 64) {
                const float e = zr[d];
                e_row[d] = e;
                m_row[d] = (float)__dmul_rn((double)restart_size, (double)e);
            }
            continue;
        }
        const double nhat = __dmul_rn(__ddiv_rn(__dadd_rn((double)npk, eps), den), n);
        const float* s_row = sums + (long)k * D;
        for (int q = lane; q < D / 4; q += 64) {
            const f32x4 m = *(const f32x4*)(m_row + q * 4), sv = *(const f32x4*)(s_row + q * 4);
            f32x4 mo, eo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mo[j] = ema_mix(g, omg, m[j], (double)sv[j]);
                eo[j] = (float)__ddiv_rn((double)mo[j], nhat);
            }
            *(f32x4*)(m_row + q * 4) = mo;
            *(f32x4*)(e_row + q * 4) = eo;
        }
    }
    __syncthreads();                                                        // this workgroup's reads of csize were consumed long before
    if (threadIdx.x == 0) s_last = atomicAdd(&g_ema_ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    for (int k = threadIdx.x; k < K; k += 256) csize[k] = (restart_below > 0.f && Np[k] < restart_below) ? restart_size : Np[k];
    if (threadIdx.x == 0) atomicExch(&g_ema_ticket, 0u);
}

extern "C" int mage_codebook_ema(float* codebook, float* cluster_size, float* embed_sum, const int64_t* counts, const float* sums, const float* z,
                                 int64_t rows, int64_t ldz, int32_t K, int32_t D, float decay, float eps, float restart_below, float restart_size,
                                 uint64_t seed, uint64_t step, double* stats, void* stream) {
    MAGE_CHECK_ARG(codebook && cluster_size && embed_sum && counts && sums && stats, "mage_codebook_ema: null pointer");
    MAGE_CHECK_ARG(K >= 1 && K <= MAGE_CODE_MAX_K, "mage_codebook_ema: K=%d outside [1, %d]", K, MAGE_CODE_MAX_K);
    MAGE_CHECK_ARG(D > 0 && D % 4 == 0 && D <= MAGE_CODE_MAX_D, "mage_codebook_ema: D=%d must be a multiple of 4 in [4, %d]", D, MAGE_CODE_MAX_D);
    MAGE_CHECK_ARG(__builtin_isfinite(decay) && decay >= 0.f && decay < 1.f, "mage_codebook_ema: decay=%g outside [0, 1)", (double)decay);
    MAGE_CHECK_ARG(__builtin_isfinite(eps) && eps > 0.f, "mage_codebook_ema: eps=%g must be finite and > 0", (double)eps);
    MAGE_CHECK_ARG(__builtin_isfinite(restart_below) && restart_below >= 0.f, "mage_codebook_ema: restart_below=%g must be finite and >= 0",
                   (double)restart_below);
    MAGE_CHECK_ARG(__builtin_isfinite(restart_size) && restart_size > 0.f, "mage_codebook_ema: restart_size=%g must be finite and > 0",
                   (double)restart_size);
    if (restart_below > 0.f) {
        MAGE_CHECK_ARG(z != nullptr, "mage_codebook_ema: restart_below > 0 needs the encoder rows z");
        MAGE_CHECK_ARG(rows > 0 && rows < (1LL << 31), "mage_codebook_ema: rows=%ld outside [1, 2^31)", (long)rows);
        MAGE_CHECK_ARG(ldz >= D && ldz < (1LL << 31), "mage_codebook_ema: ldz=%ld below D=%d (or 2^31 and above)", (long)ldz, D);
    }
    MAGE_CHECK_ARG((((uintptr_t)codebook | (uintptr_t)embed_sum | (uintptr_t)sums) & 15) == 0 && (((uintptr_t)counts | (uintptr_t)stats) & 7) == 0 &&
                       (((uintptr_t)cluster_size | (uintptr_t)z) & 3) == 0,
                   "mage_codebook_ema: misaligned pointer (codebook, embed_sum, sums: 16 bytes; counts, stats: 8; cluster_size, z: 4)");
    MAGE_CHECK_ARG(mage_error_word() != nullptr, "mage_codebook_ema: mage_init() has not been called");
    const unsigned long long ctr0 = (unsigned long long)seed * 0x9e3779b97f4a7c15ULL + (unsigned long long)step * (unsigned long long)K;
    hipLaunchKernelGGL(codebook_ema_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, codebook, cluster_size, embed_sum, counts,
                       sums, z, (long)rows, (long)ldz, K, D, (double)decay, (double)eps, restart_below, restart_size, ctr0, stats);
    MAGE_CHECK_LAUNCH("mage_codebook_ema");
    return MAGE_OK;
}
