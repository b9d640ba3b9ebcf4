// gemm4_kernel: the bf16 256x256 plain GEMM with ONE wave per SIMD (4 waves of 128x128 outputs each, 256 accumulator registers per
// lane, launch_bounds(256): the 512-register budget) -- the decoder's Linear layers at M >= 2 tiles per CU (see include/mage_hip.h,
// mage_gemm; dispatch in gemm.hip).
//
// Why another tile shape.  The 8-wave kernels (gemm.hip) give each wave 128x64 outputs: per 64-wide K slab a wave reads 28 (8-phase)
// operand fragments of 1 KiB for 64 MFMAs, 224 KiB of LDS reads per slab per CU beside the slab's own 64 KiB of LDS-DMA writes, and the
// 8-phase schedule pays two barriers per 16-MFMA section: 3.1-3.2 k cycles per slab against 2.05 k of matrix-pipe time
// (profiles/r03_gemm_tile_phases.txt).  With 128x128 per wave a slab is 32 fragment reads for 128 MFMAs per wave -- 128 KiB per CU, half
// the fragment traffic per MAC -- there is no partner wave to hand the SIMD to, so no intra-slab barrier at all: ONE barrier per slab,
// and the wave's own instruction stream interleaves its ds_reads and LDS-DMA issues between its MFMAs (MI355X_MICROARCH.md: one wave
// per SIMD hides <= 5 single-issue instructions per 32-cycle MFMA gap; this loop needs < 1 per 16-cycle gap).
//
// The accumulators are the WHOLE accumulator file (a0..a255).  hipcc's register allocator cannot hold a 256-register value set in a
// 256-register class: given the MFMAs as builtins it split the accumulators between AGPRs and VGPRs and copied them back and forth
// inside the K loop (3800 v_accvgpr_write, 100 spilled VGPRs).  So the MFMAs are inline asm on LITERAL accumulator registers
// (cdna_hip_programming.md 5.7): the compiler never sees an accumulator value; it allocates only the operand fragments, the loader's
// offsets and the epilogue's temporaries (< 256 VGPRs, no spill: `make check4` audits the .s for spills and for compiler-made
// v_accvgpr_* outside the asm blocks).  The first k-step of a tile multiplies into C = 0 (no zeroing pass); the epilogue reads the
// accumulators back 64 registers at a time (v_accvgpr_read) into the array epilogue_lean takes.
//
// LDS: 2 stages x (256 A rows + 256 W rows) x 128 B = 128 KiB, the lane-linear XOR-swizzled image of gemm.hip (physical 16-byte chunk p
// of row r holds logical chunk p ^ ((r >> 1) & 7); applied on the DMA source address and on the ds_read_b128), + 4 KiB of epilogue
// staging per wave: 144 KiB.
//
// Schedule of slab j (stage s = j & 1), four QUARTERS of 32 MFMAs = (k-half t, row half mh), loads placed BETWEEN the MFMAs in source
// order and pinned there (sched_barrier):
//     Q0 (t0, rows 0-63)    reads: A(t0, rows 64-127)                                   DMA: W pieces of slab j+1 -> stage s^1
//     Q1 (t0, rows 64-127)  reads: W(t1) x 8, A(t1, rows 0-63)
//     Q2 (t1, rows 0-63)    reads: A(t1, rows 64-127);  then  s_waitcnt vmcnt(0) lgkmcnt(0);  s_barrier
//     Q3 (t1, rows 64-127)  reads from stage s^1: W'(t0) x 8, A'(t0, rows 0-63)          DMA: A pieces of slab j+2 -> stage s
// The barrier sits at the 3/4 point: by then this wave has issued (and waited for) its last read of stage s, and its share of slab
// j+1 has landed; past it stage s is free for slab j+2 and slab j+1 is visible, while the wave still holds the operands of 32 MFMAs
// in registers -- the matrix pipe restarts without an LDS round trip.  A pieces (streamed from HBM) are requested 1.75 slabs ahead
// of their first read, W pieces (L2-resident) 0.75.  The slab sequence runs across tile boundaries: Q3 of a tile's last slab already
// fetches the next tile's first fragments, the epilogue runs, the next tile's Q0 starts from registers.
//
// Arithmetic: v_mfma_f32_16x16x32_bf16, operands swapped (A-operand = W rows) and k ascending in steps of 32 exactly as in gemm.hip's
// three kernels, the SAME epilogue_lean on the same accumulator layout: every output element gets the same bits from all four kernels
// (incremental == full loop, B = 1 == row of a batch stay exact).
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "gemm_shared.h"
#include "gemm4_regs.h"
#include "attn_mfma.h"

namespace {

struct Gemm4Args {
    const void* A;
    const void* W;
    void* Y;
    const float* bias;
    const float* ln_stats;
    const float* ln_colsum;
    const void* residual;
    float* ln_part;
    void* y2;
    int M, N, K, lda, ldw, ldy, ldr, ldy2, y_dtype, a_off, y_off;
    int ntiles_n, ntiles;
    int stagger_groups, stagger_sleeps;
    // the fused H / W axial attention entry (QF, see gemm4_body): 1 = H axis | 2 = W axis, softmax scale, the regrouping of the output rows
    // (out_w rows at a time, y_img_stride apart).  On a 16-byte boundary: the fused kernel fetches the four with one s_load_dwordx4 of their
    // own.  Packed directly behind stagger_sleeps, hipcc merges the argument loads differently and the hand-scheduled kernel's scalar
    // registers fall differently from there on (profiles/r19_retire_two_launch_pair.txt).  The temporal form (TX, gemm4_tattn_kernel) regroups no
    // rows and carries its own two numbers in the last two: out_w = hw, the rows between two slots of a clip; y_img_stride = hw / 16, tiles per clip
    alignas(16) int attn_axis;
    float attn_scale;
    int out_w, y_img_stride;
};

#ifndef MAGE4_ABL
#define MAGE4_ABL 0      // tuning builds, bit flags: 1 = no epilogue (K loop only), 2 = no LDS-DMA in the loop, 4 = no fragment reads in the loop,
                         // 8 = LDS-DMA always from the first slab of the first tile (cache-resident source), 16 = no vmcnt wait at the barrier,
                         // 32 = every tile's output goes to one fixed window per workgroup (cache-resident stores), 64 = epilogue without stores
#endif

#ifdef MAGE4_STAMP
// tuning build: shader-clock stamps of every wave per (workgroup, tile < 32): [0] tile start, [1] K loop done, [2] epilogue done, [3] 100 MHz wall clock
// at [1], [4] 100 MHz wall clock at [0] (shader cycles per wall microsecond over the K loop = the clock the chip actually holds)
__device__ unsigned long long g4_stamps[256 * 32 * 4 * 8];
#define G4_STAMP(it, p)                                                                                                   \
    do {                                                                                                                  \
        if (lane == 0 && (it) < 32 && blockIdx.x < 256) {                                                                 \
            g4_stamps[((blockIdx.x * 32 + (it)) * 4 + wave) * 8 + (p)] = __builtin_readcyclecounter();                    \
            if ((p) == 1) g4_stamps[((blockIdx.x * 32 + (it)) * 4 + wave) * 8 + 3] = __builtin_amdgcn_s_memrealtime();    \
            if ((p) == 0) g4_stamps[((blockIdx.x * 32 + (it)) * 4 + wave) * 8 + 4] = __builtin_amdgcn_s_memrealtime();    \
        }                                                                                                                 \
    } while (0)
#else
#define G4_STAMP(it, p)
#endif

constexpr int G4_STAGE = 65536, G4_WOFF = 32768, G4_RING = 2 * G4_STAGE, G4_LDS = G4_RING + 4 * 4096;      // 144 KiB

#ifdef MAGE4_MFMA32
// Tuning build (tools/probes/gemm4_probe.hip -DMAGE4_MFMA32 -DMAGE4_ABL=1): the K loop on v_mfma_f32_32x32x16_bf16 -- 16 blocks of 32 x 32 outputs
// (16 accumulator registers each) instead of 64 of 16 x 16: half the MFMA issues and half the operand-register reads per FLOP.  K loop only:
// the epilogue is written for the 16 x 16 accumulator layout, so this build answers one question -- does the same slab of work draw less
// power (hold a higher clock) in the other MFMA shape -- and nothing else.
template <int B, bool ZERO, bool CLOB>
__device__ __forceinline__ void g4_mfma32(const u32x4& w, const u32x4& x) {
    if constexpr (ZERO && CLOB) asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, 0" ::"v"(w), "v"(x), "i"(16 * B), "i"(16 * B + 15) : G4_ALL_ACC);
    else if constexpr (ZERO) asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, 0" ::"v"(w), "v"(x), "i"(16 * B), "i"(16 * B + 15));
    else if constexpr (CLOB) asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(w), "v"(x), "i"(16 * B), "i"(16 * B + 15) : G4_ALL_ACC);
    else asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(w), "v"(x), "i"(16 * B), "i"(16 * B + 15));
}
#endif
// QF (the fused H / W axial attention of the decoder, 16 x 16 frames, head width 32, LayerNorm-consuming in_proj; mage_gemm_attn_fused_qkv): the pair
// QKV GEMM -> attention_mfma_kernel as ONE launch of gemm4_attn_kernel; q, k, v and the softmax numerators never reach memory.  A 256-row tile is
// one frame; the loader fetches its rows so that every 16-row m-fragment is one axial sequence (W axis: rows as they lie; H axis: tile row
// R = w*16 + h reads frame row h*16 + w), the LayerNorm statistics and the output rows follow the same map.  N = 3C, the in_proj rows packed per
// group of 4 heads as 384 rows [256 q k rows | 128 v rows]; one entry of the tile list per (frame, group), run as two tiles over the same rows:
//   the Q K part, the group's 256 rows: per head 64 columns [q_h | k_h], the 32 columns of each in the order that makes a lane's two packed
//     accumulator blocks the 8 consecutive head dims the S MFMA wants (column nt*16 + g*4 + e = dim g*8 + nt*4 + e).  The epilogue finishes the
//     LayerNorm, adds the bias and rounds as epilogue_lean does (the values qkv held), then per m-fragment and head S^T = K Q^T by ONE 16x16x32
//     MFMA on those registers, scale and softmax in attention_mfma_kernel's order; the numerators p = exp(s - max) stay, as fp32, in the wave's
//     accumulator registers.
//   the V part, half width, the group's 128 v rows over the frame's panel again (replayed from L2), MFMA roles swapped (A operand = the
//     activation rows, as gemm4h_kernel: the same products in the same k order): an accumulator block then holds V^T the way the P V MFMA takes it
//     (lane = head dim, register = key).  Same epilogue arithmetic per element, then den, P = hi + lo, O^T = V^T P_hi^T + V^T P_lo^T, the lane
//     swap, 1 / den and the 16-byte row stores of attention_mfma_kernel.  The lane that computed a numerator is the lane that multiplies it.
// The row statistics are fetched once per entry.  Every element takes the unfused pair's operations in the pair's order: the same bits in `ao`.
// TX (the temporal blocks of a full pass over clips of 16 slots, gemm4_tattn_kernel): the same entry with another row map and a mask.  A tile is 16
// adjacent positions of one clip x its 16 slots -- tile row R = slot * 16 + position reads row (R & 15) * hw + (R >> 4) behind the tile's first row
// (clip * 16 hw + position block * 16), so that an m-fragment is again one sequence, lane l15 = its slot; every row is still one contiguous piece
// for the loader.  The scores pass attention_mfma_kernel's causal select (key slot 4 grp + e <= query slot l15, else -inf; a masked numerator is
// +0) before and after the maximum; the slab schedule, the panel replay, the staging window and the stores are the H / W form's.
// The epilogue MFMAs of the fused attention entry (QF): attention_mfma_kernel's instructions (attn_mfma_qk / attn_mfma_pv in attn_mfma.h) on the
// same operands, but as inline asm on VGPRs: given the builtins, hipcc puts their results into the accumulator registers it believes free
// (a[0:3] -- live accumulators of the tile).  Wait states inside the strings: a just-written operand (1), the result before any reader (16);
// an accumulate chain needs none.
typedef unsigned g4_u32x2 __attribute__((ext_vector_type(2)));
template <bool HF>
__device__ __forceinline__ f32x4 g4_epi_qk(const u32x4& k, const u32x4& q) {
    f32x4 d;
    if constexpr (HF) asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, 0\n\ts_nop 15" : "=&v"(d) : "v"(k), "v"(q));
    else asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, 0\n\ts_nop 15" : "=&v"(d) : "v"(k), "v"(q));
    return d;
}
// o0 = vt0 x p_hi + vt0 x p_lo, o1 = vt1 x p_hi + vt1 x p_lo (each: the hi product into C = 0, then the lo product accumulated)
#define G4_EPI_PV(OP)                                                                                                                               \
    asm volatile("s_nop 1\n\t" OP " %0, %2, %4, 0\n\t" OP " %1, %3, %4, 0\n\t" OP " %0, %2, %5, %0\n\t" OP " %1, %3, %5, %1\n\ts_nop 15"           \
                 : "=&v"(o0), "=&v"(o1)                                                                                                             \
                 : "v"(__builtin_bit_cast(g4_u32x2, vt0)), "v"(__builtin_bit_cast(g4_u32x2, vt1)), "v"(__builtin_bit_cast(g4_u32x2, phi)),          \
                   "v"(__builtin_bit_cast(g4_u32x2, plo)))
template <bool HF>
__device__ __forceinline__ void g4_epi_pv(const ashort4& vt0, const ashort4& vt1, const ashort4& phi, const ashort4& plo, f32x4& o0, f32x4& o1) {
    if constexpr (HF) G4_EPI_PV("v_mfma_f32_16x16x16_f16");
    else G4_EPI_PV("v_mfma_f32_16x16x16_bf16");
}

// one MFMA of the K loop: A operand = the W fragment, B operand = the activation fragment; SWAP (the V part of the fused entry): the roles swapped (transposed block)
template <bool SWAP, int I, bool ZERO, bool CLOB, bool HF>
__device__ __forceinline__ void g4_mm(const u32x4& w, const u32x4& x) {
    if constexpr (SWAP) g4_mfma<I, ZERO, CLOB, HF>(x, w);
    else g4_mfma<I, ZERO, CLOB, HF>(w, x);
}
// (the body of both kernels below: gemm4_kernel = plain GEMM, gemm4_attn_kernel = QF, the fused attention entry)
template <int ACT, int EK, int LN, bool RB, bool HF, bool QF, bool TX = false>
__device__ __forceinline__ void gemm4_body(const Gemm4Args& g) {
    static_assert(EK != EK_GENERAL, "lean epilogue kinds");
    static_assert(!TX || QF, "the temporal row map belongs to the fused attention entry");
    static_assert(!QF || (LN == LN_CONSUME && ACT == MAGE_ACT_NONE), "fused attention: the LayerNorm-consuming in_proj");
    static_assert(!HF || (LN != LN_DUAL && LN != LN_GELUBWD), "f16 form: the generation path's epilogues");
    typedef std::conditional_t<HF, f16_t, unsigned short> H16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    g4_claim_accumulators();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // persistent tile schedule of gemm.hip: workgroup b runs on XCD b % 8 (speed only); each XCD owns a contiguous chunk of the tile list
    const int nwg8 = gridDim.x >> 3;
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const int q8 = g.ntiles >> 3, r8 = g.ntiles & 7;
    const int chunk0 = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    const int chunk1 = chunk0 + q8 + (xcd < r8 ? 1 : 0);
    const int nk = g.K >> 6;                           // K % 128 == 0, K >= 256 (host): FIRST and LAST slabs are peeled, the rest runs in pairs
    int c_tile = chunk0 + li;
    if (c_tile >= chunk1) return;
    const int last_tile = c_tile + ((chunk1 - 1 - c_tile) / nwg8) * nwg8;      // this workgroup's last tile (the cursors stop there)

    // ---- loader: per slab this wave moves 8 A units and 8 W units (unit = 8 rows x 128 B = one wave-wide LDS-DMA) of its 64-row strips.
    // global_load_lds_dwordx4 with an SGPR base and a 32-bit lane offset (no vector instruction per piece).  Inline asm, because the builtin
    // takes one 64-bit pointer per lane and an M0 write per piece: here M0 (the LDS destination base) is written ONCE per group of 8
    // units and the instruction's immediate offset (u - 4) KiB, which the hardware adds to the LDS address AND to the global address,
    // selects the unit; the lane offsets carry the opposite shift (and + 4 KiB, taken off the base pointers, to stay non-negative).
    // Nothing else in this kernel reads M0 (audited in the .s); the statements have no VGPR result, their completion is the explicit
    // vmcnt wait in front of each slab's barrier.
    const int lr = lane >> 3, lp = lane & 7;
    unsigned voffA[8], voffW[8];
    // QF: tile row R (0..255) -> row of the frame (H axis: sequences run down the columns of the 16 x 16 frame)
    // TX: tile row R = slot * 16 + position -> row of the tile's 16 positions x 16 slots (slots g.out_w = hw rows apart)
    [[maybe_unused]] auto frame_row = [&](int R) {
        if constexpr (TX) return (R & 15) * g.out_w + (R >> 4);
        else return g.attn_axis == 1 ? ((R & 15) << 4) + (R >> 4) : R;
    };
    // TX: first row of row tile tm = position block tm % tpc of clip tm / tpc (tpc = g.y_img_stride = hw / 16 tiles per clip of 16 * hw rows)
    [[maybe_unused]] auto tile_row0 = [&](int tm_) {
        const int clip = tm_ / g.y_img_stride;
        return (long)clip * 16 * g.out_w + (tm_ - clip * g.y_img_stride) * 16;
    };
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int r = u * 8 + lr;
        const int ch = lp ^ ((r >> 1) & 7);
        if constexpr (TX) voffA[u] = (unsigned)frame_row(wave * 64 + r) * (unsigned)(g.lda * 2) + (unsigned)(ch * 16 + 8192 - u * 1024);     // < 2^32 (host)
        else voffA[u] = (unsigned)((QF ? frame_row(wave * 64 + r) : r) * g.lda * 2 + ch * 16 + 8192 - u * 1024);
        voffW[u] = (unsigned)(r * g.ldw * 2 + ch * 16 + 8192 - u * 1024);
    }
    auto a_base = [&](int tile) {
        if constexpr (TX) return (const char*)g.A + (tile_row0(tile / g.ntiles_n) + g.a_off) * g.lda * 2 - 4096;
        else return (const char*)g.A + ((long)((tile / g.ntiles_n) * 256 + (QF ? 0 : wave * 64)) + g.a_off) * g.lda * 2 - 4096;
    };
    auto w_base = [&](int tile) { return (const char*)g.W + (long)((tile % g.ntiles_n) * (QF ? 384 : 256) + wave * 64) * g.ldw * 2 - 4096; };
    // QF: the 128 v rows behind a group's 256 [q | k] rows -- 4 units (32 rows) per wave, LDS rows wave*32 .. +31 of the W half of a stage
    [[maybe_unused]] auto w_base_v = [&](int tile) { return (const char*)g.W + (long)((tile % g.ntiles_n) * 384 + 256 + wave * 32) * g.ldw * 2 - 4096; };
    // two cursors: A pieces run 2 slabs ahead of the compute cursor, W pieces 1; at a tile's end they jump to the next tile's bases
    const char* a_src = a_base(c_tile);
    const char* w_src = w_base(c_tile);
    const char* a_next = a_src;
    const char* w_next = w_src;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * 8192 + 4096;     // (8 units of 1 KiB per wave and operand)
    auto dma_m0 = [&](unsigned lds_group) __attribute__((always_inline)) {       // lds_group: stage * G4_STAGE (+ G4_WOFF)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(lds0 + lds_group) : "memory");      // (m0 cannot be named as a clobber: the compiler treats it as reserved and warns; check4 audits its writers)
    };
    // the W half of a stage: all 8 units of the wave's 64 rows, or (half: the V part of QF) 4 units at rows wave*32
    auto dma_m0w = [&](unsigned stage_off, bool half) __attribute__((always_inline)) { dma_m0(stage_off + G4_WOFF - (half ? wave * 4096 : 0)); };

    // ---- compute state: wave (wm, wn) owns rows [wm*128, +128) x columns [wn*128, +128) of the tile
    const int wm = wave >> 1, wn = wave & 1;
    const int l15 = lane & 15, grp = lane >> 4;
    const int rsw = (l15 >> 1) & 7;
    const int pc[2] = {((grp + 0) ^ rsw) * 16, ((grp + 4) ^ rsw) * 16};
    const int x_off = (wm * 128 + l15) * 128;
    const int w_off = G4_WOFF + (wn * 128 + l15) * 128;
    [[maybe_unused]] const int w_off_v = G4_WOFF + (wn * 64 + l15) * 128;      // QF, V part: the wave's 64 of the 128 v rows
    u32x4 wf[2][8], xf[2][4];
    // accumulator block of (column half h, 16-row tile mt, 16-column block j): columns h*64 + j*16 + grp*4 + {0..3} of row mt*16 + l15
    // index = (h*8 + mt)*4 + j
    auto rd_w1 = [&](int buf, int stage, int t, int nt) __attribute__((always_inline)) {
        wf[buf][nt] = *(const u32x4*)(smem + stage * G4_STAGE + w_off + nt * 2048 + pc[t]);
    };
    [[maybe_unused]] auto rd_wv = [&](int buf, int stage, int t, int nt) __attribute__((always_inline)) {
        wf[buf][nt] = *(const u32x4*)(smem + stage * G4_STAGE + w_off_v + nt * 2048 + pc[t]);
    };
    auto rd_x1 = [&](int buf, int stage, int t, int mt) __attribute__((always_inline)) {
        xf[buf][mt & 3] = *(const u32x4*)(smem + stage * G4_STAGE + x_off + mt * 2048 + pc[t]);
    };

#ifdef MAGE4_MFMA32
    // 32 x 32 x 16: lane (l31 = lane & 31, hi = lane >> 5) holds 8 consecutive k (16 bytes) of fragment row l31: k-step s of a slab is logical
    // chunks 2s + hi of the 128-byte row
    const int l31 = lane & 31, hi5 = lane >> 5;
    const int rsw32 = (l31 >> 1) & 7;
    const int x32_off = (wm * 128 + l31) * 128, w32_off = G4_WOFF + (wn * 128 + l31) * 128;
    u32x4 wq[2][4], xq[2][4];
    auto rd_w32 = [&](int buf, int stage, int ks, int nb) __attribute__((always_inline)) {
        wq[buf][nb] = *(const u32x4*)(smem + stage * G4_STAGE + w32_off + nb * 4096 + (((2 * ks + hi5) ^ rsw32) << 4));
    };
    auto rd_x32 = [&](int buf, int stage, int ks, int mb) __attribute__((always_inline)) {
        xq[buf][mb] = *(const u32x4*)(smem + stage * G4_STAGE + x32_off + mb * 4096 + (((2 * ks + hi5) ^ rsw32) << 4));
    };
#endif
    if (g.stagger_groups > 1) {
        for (int w = (li % g.stagger_groups) * g.stagger_sleeps; w > 0; --w) __builtin_amdgcn_s_sleep(16);
    }
    // prologue: slab 0 complete in stage 0, slab 1 on its way to stage 1, slab 0's first fragments in registers
    dma_m0(0);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffA[decltype(u_)::value], a_src); });
    dma_m0(G4_WOFF);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffW[decltype(u_)::value], w_src); });
    a_src += 128;
    w_src += 128;
    dma_m0(G4_STAGE);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffA[decltype(u_)::value], a_src); });
    dma_m0(G4_STAGE + G4_WOFF);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffW[decltype(u_)::value], w_src); });
    a_src += 128;
    w_src += 128;
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): slabs 0 AND 1 (a tile's first slab waits with a count that assumes the previous
                                                       // tile's epilogue traffic behind slab 1's pieces; there is none in front of the first tile)
    ring_barrier();
#ifdef MAGE4_MFMA32
#pragma unroll
    for (int b = 0; b < 4; ++b) { rd_w32(0, 0, 0, b); rd_x32(0, 0, 0, b); }
#else
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) rd_w1(0, 0, 0, nt);
#pragma unroll
    for (int m = 0; m < 4; ++m) rd_x1(0, 0, 0, m);
#endif

    [[maybe_unused]] int it = 0;
    for (; c_tile < chunk1; c_tile += nwg8, ++it) {
        G4_STAMP(it, 0);
        const int tm = c_tile / g.ntiles_n, tn = c_tile - tm * g.ntiles_n;
        MAGE_DASSERT(c_tile >= 0 && c_tile < g.ntiles && tm * 256 < g.M && tn * (QF ? 384 : 256) < g.N);
        [[maybe_unused]] float ln_mean[8], ln_rstd[8];
        [[maybe_unused]] long row0 = 0;                    // TX: the entry's first row, once per entry (statistics rows, output rows, the panel replay)
        if constexpr (TX) row0 = tile_row0(tm);
        // One tile of kind PH.  Plain GEMM: the entry is this one tile, PH = 0.  QF: the entry (frame, group of 4 heads) is a PH = 1 tile (the
        // 256 packed [q | k] columns of the group; KEEP: the softmax numerators stay in this wave's registers) followed by a PH = 2 tile of HALF width
        // over the same rows (the group's 128 v columns; wave (wm, wn) takes the 64 columns of the two heads whose q and k it has just multiplied).
        // The HALF tile accumulates in a128..a255 (the blocks of column half 1); the numerators wait in a0..a63, which the Q K part's first
        // epilogue chunk has read out before the first of them is written: block c*4 + mt = chunk c (head c >> 1 of the wave, row half c & 1), sequence mt.
        auto tile = [&](auto PH_) __attribute__((always_inline)) {
            constexpr int PH = decltype(PH_)::value;
            constexpr bool HALF = PH == 2, KEEP = PH == 1;
            constexpr int NW = HALF ? 4 : 8;               // W fragments per k-half = 16-column blocks of the wave
            const int m0 = ((MAGE4_ABL & 32) ? (int)blockIdx.x : tm) * 256 + wm * 128;
            // n0: the wave's first column -- of W, bias and ln_colsum; ny0: of the output rows
            const int n0 = QF ? tn * 384 + (HALF ? 256 + wn * 64 : wn * 128) : ((MAGE4_ABL & 32) ? 0 : tn) * 256 + wn * 128;
            [[maybe_unused]] const int ny0 = HALF ? tn * 128 + wn * 64 : n0;
            if constexpr (KEEP) {                          // the V part replays the frame's panel (from L2: the frame's groups stream it together)
                if constexpr (TX) a_next = (const char*)g.A + (row0 + g.a_off) * g.lda * 2 - 4096;
                else a_next = a_base(c_tile);
                w_next = w_base_v(c_tile);
            } else {
                const int nt_tile = c_tile + nwg8 > last_tile ? last_tile : c_tile + nwg8;     // past the end: re-fetch the last tile (never read)
                a_next = a_base(nt_tile);
                w_next = w_base(nt_tile);
            }
            auto rd_w = [&](int buf, int stage, int t, int nt) __attribute__((always_inline)) {
                if constexpr (HALF) rd_wv(buf, stage, t, nt);
                else rd_w1(buf, stage, t, nt);
            };
            f32x4 biasm[2][4];
            [[maybe_unused]] f32x4 lns[2][4];
            // QF: the softmax numerators of one epilogue step (row half mh = 4 sequences mt; KEEP: one head, [mt][0]; HALF: the wave's two heads hd):
            // lane (l15, grp) holds p of query l15, keys 4 grp .. 4 grp + 3
            [[maybe_unused]] f32x4 pl[4][2];
            // (the lane's coordinates, opaque once per tile: the per-lane 64-bit addresses of the output rows built from them are then
            // recomputed where they are used instead of living in registers across the K loop, which this instantiation does not have)
            [[maybe_unused]] int ql15 = l15, qgrp = grp;
            if constexpr (QF) asm volatile("" : "+v"(ql15), "+v"(qgrp));
            // One slab.  j = its index in the tile (runtime; only the cursors' tile jumps depend on it), S = its stage.
            // LDS-DMA issue points: W(j+1) in Q0 and A(j+2) in Q3, one instruction per four MFMAs.  A tile's FIRST slab issues no W: the
            // previous tile's LAST slab sent W of this tile's slab 1 together with its A in Q3, BEFORE the epilogue's stores -- memory
            // operations retire in order, so a wait for pieces issued after the stores would also wait for every store acknowledgement
            // (the 8-wave kernels' "first-slab wait", 3.3 k cycles per tile); with both operands of slab 1 older than the stores the FIRST
            // slab waits with a count that leaves the stores in flight.
            auto slab = [&](auto S_, auto FIRST_, auto LAST_, int j) __attribute__((always_inline)) {
                constexpr int S = decltype(S_)::value;
                constexpr bool FIRST = decltype(FIRST_)::value, LAST = decltype(LAST_)::value;
                // HALF (the V part of QF): a quarter is 16 MFMAs on the 4 W fragments of column half 0 -- per slab 16 + 8 fragment reads, 8 A units
                // and 4 W units per wave.  ACC0: the first accumulator block.  The W pieces this slab sends belong to the next slab of this tile, or
                // (LAST) to the next tile: WH_ = that tile is a HALF one (4 units at their own LDS rows, dma_m0w).
                constexpr int ACC0 = HALF ? 32 : 0;
                constexpr bool WH_ = LAST ? KEEP : HALF;
                constexpr int WU = WH_ ? 4 : 8;
                // ---- Q0: (t0, rows 0-63) from wf[0], xf[0]
                g4_for<4 * NW>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, m = i / NW, nt = i % NW;
                    g4_mm<PH == 2, ACC0 + ((nt >> 2) * 8 + m) * 4 + (nt & 3), FIRST, i == 0, HF>(wf[0][nt], xf[0][m]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!(MAGE4_ABL & 4) && i < 4) {
                        rd_x1(1, S, 0, 4 + i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (!(MAGE4_ABL & 2) && !FIRST && i == 4) {
                        dma_m0w((S ^ 1) * G4_STAGE, WH_);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (!HALF) {                 // one piece per four MFMAs
                        if constexpr (!(MAGE4_ABL & 2) && !FIRST && (i & 3) == 1 && i > 4 && (i >> 2) - 1 < WU) {
                            g4_dma<(i >> 2) - 1>(voffW[(i >> 2) - 1], w_src);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {                               // 16 MFMAs: one piece per MFMA behind the fragment reads
                        if constexpr (!FIRST && i > 4 && i - 5 < WU) {
                            g4_dma<i - 5>(voffW[i - 5], w_src);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                });
                if constexpr (!(MAGE4_ABL & 2) && !FIRST && !HALF && WU == 8) {
                    g4_dma<7>(voffW[7], w_src);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (!(MAGE4_ABL & 8) && !FIRST) w_src = (j == nk - 2) ? w_next : w_src + 128;
                // ---- Q1: (t0, rows 64-127) from wf[0], xf[1]
                g4_for<4 * NW>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, m = i / NW, nt = i % NW;
                    g4_mm<PH == 2, ACC0 + ((nt >> 2) * 8 + 4 + m) * 4 + (nt & 3), FIRST, i == 0, HF>(wf[0][nt], xf[1][m]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!(MAGE4_ABL & 4) && i < 4 + NW) {
                        if constexpr (i < 4) rd_x1(0, S, 1, i);
                        else rd_w(1, S, 1, i - 4);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
                // ---- Q2: (t1, rows 0-63) from wf[1], xf[0]
                if constexpr (LAST) {                      // the epilogue's vectors, late: their registers are free during the K loop
#pragma unroll
                    for (int b = 0; b < 4; ++b) {          // column half 0 (half 1: requested in the epilogue, under half 0's arithmetic)
                        if constexpr (PH == 2) {           // transposed blocks: this lane's column of block b is b*16 + l15
                            biasm[0][0][b] = g.bias[n0 + b * 16 + l15];
                            lns[0][0][b] = g.ln_colsum[n0 + b * 16 + l15];
                            continue;
                        }
                        const int n = n0 + b * 16 + grp * 4;
                        biasm[0][b] = *(const f32x4*)(g.bias + n);                         // bias != null (host)
                        if constexpr (LN == LN_CONSUME) lns[0][b] = *(const f32x4*)(g.ln_colsum + n);
                    }
                    if constexpr (LN == LN_CONSUME && !HALF) {      // (HALF: the Q K part's are kept)
#pragma unroll
                        for (int a = 0; a < 8; ++a) {
                            long row;
                            if constexpr (TX) row = row0 + frame_row(wm * 128 + a * 16 + ql15);
                            else row = QF ? (long)tm * 256 + frame_row(wm * 128 + a * 16 + ql15) : (long)(m0 + a * 16 + l15);
                            const float2 st = *(const float2*)(g.ln_stats + 2 * row);
                            ln_mean[a] = st.x;
                            ln_rstd[a] = st.y;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                g4_for<4 * NW>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, m = i / NW, nt = i % NW;
                    g4_mm<PH == 2, ACC0 + ((nt >> 2) * 8 + m) * 4 + (nt & 3), false, i == 0, HF>(wf[1][nt], xf[0][m]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!(MAGE4_ABL & 4) && i < 4) {
                        rd_x1(1, S, 1, 4 + i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
                // my reads of this stage are done and my share of the next slab has landed.  FIRST: the next slab's 16 pieces are older than
                // the previous tile's epilogue traffic (4 or 8 vector loads and >= 32 stores per wave), which may stay in flight (the count waited
                // for is four below that traffic: a margin against any reordering of the epilogue's last stores)
                if constexpr (MAGE4_ABL & 16) __builtin_amdgcn_s_waitcnt(0xC07F);
                // QF: only the instructions whose place behind the pieces the source fixes are counted -- the stores, which follow the accumulator
                // reads (asm statements), not the epilogue's loads, which hipcc is free to issue earlier.  The Q K part follows a V part's 16 row
                // stores, four below = vmcnt(12); the V part follows a Q K part that stores nothing = vmcnt(0).  A too-low count only waits for
                // some store acknowledgements; tightening them is unmeasured.
                else if constexpr (FIRST && QF) __builtin_amdgcn_s_waitcnt(PH == 1 ? 0x007C : 0x0070);
                else if constexpr (FIRST) __builtin_amdgcn_s_waitcnt(LN == LN_CONSUME ? 0x8074 : 0x8070);       // vmcnt(36 | 32) lgkmcnt(0): four below the count
                else __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0)
                ring_barrier();
                __builtin_amdgcn_sched_barrier(0);
                // ---- Q3: (t1, rows 64-127) from wf[1], xf[1]; next slab's first fragments into wf[0], xf[0]
                g4_for<4 * NW>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, m = i / NW, nt = i % NW;
                    g4_mm<PH == 2, ACC0 + ((nt >> 2) * 8 + 4 + m) * 4 + (nt & 3), false, i == 0, HF>(wf[1][nt], xf[1][m]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!(MAGE4_ABL & 4) && i < 4 + NW && !LAST) {     // (a tile's last slab: after the epilogue, whose registers these would occupy)
                        if constexpr (i < 4) rd_x1(0, S ^ 1, 0, i);
                        else rd_w(0, S ^ 1, 0, i - 4);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (!(MAGE4_ABL & 2) && !LAST && !HALF) {      // A(j+2): 8 pieces
                        if constexpr (i == 2) dma_m0(S * G4_STAGE);
                        if constexpr ((i & 3) == 3) g4_dma<(i >> 2)>(voffA[i >> 2], a_src);
                        if constexpr (i == 2 || (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (!(MAGE4_ABL & 2) && LAST && !HALF) {       // A and W of the next tile's slab 1: 16 pieces (KEEP: 8 + the V part's 4)
                        if constexpr (i == 0) dma_m0(S * G4_STAGE);
                        if constexpr (i == 16) dma_m0w(S * G4_STAGE, WH_);
                        if constexpr ((i & 1) == 1 && i < 16) g4_dma<(i >> 1)>(voffA[i >> 1], a_src);
                        if constexpr ((i & 1) == 1 && i > 16 && ((i - 16) >> 1) < WU) g4_dma<((i - 16) >> 1)>(voffW[(i - 16) >> 1], w_src);
                        if constexpr (i == 0 || i == 16 || (i & 1) == 1) __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (HALF && !LAST) {                           // A(j+2): 8 pieces, one per two MFMAs
                        if constexpr (i == 0) dma_m0(S * G4_STAGE);
                        if constexpr ((i & 1) == 1) g4_dma<(i >> 1)>(voffA[i >> 1], a_src);
                        if constexpr (i == 0 || (i & 1) == 1) __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (HALF && LAST) {                            // A and W of the next entry's slab 1: 16 pieces, one per MFMA
                        if constexpr (i == 0) dma_m0(S * G4_STAGE);
                        if constexpr (i == 8) dma_m0w(S * G4_STAGE, false);
                        if constexpr (i < 8) g4_dma<i>(voffA[i], a_src);
                        else g4_dma<i - 8>(voffW[i - 8], w_src);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
                if constexpr (!(MAGE4_ABL & 8)) a_src = (j == nk - 3) ? a_next : a_src + 128;
                if constexpr (!(MAGE4_ABL & 8) && LAST) w_src += 128;
            };
#ifdef MAGE4_MFMA32
            // the same slab on 32 x 32 x 16 MFMAs: quarter q = k-step q (16 of the slab's 64 k), 16 MFMAs over the 4 x 4 blocks; the next k-step's 8
            // fragments are read during the quarter, the DMA issue points, the barrier and the waits are the 16 x 16 schedule's
            auto slab32 = [&](auto S_, auto FIRST_, auto LAST_, int j) __attribute__((always_inline)) {
                constexpr int S = decltype(S_)::value;
                constexpr bool FIRST = decltype(FIRST_)::value, LAST = decltype(LAST_)::value;
                auto quarter = [&](auto Q_) __attribute__((always_inline)) {
                    constexpr int Q = decltype(Q_)::value, buf = Q & 1;
                    g4_for<16>([&](auto i_) {
                        constexpr int i = decltype(i_)::value, mb = i >> 2, nb = i & 3;
                        g4_mfma32<mb * 4 + nb, FIRST && Q == 0, i == 0>(wq[buf][nb], xq[buf][mb]);
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (!(MAGE4_ABL & 4) && i < 8 && !(Q == 3 && LAST)) {        // next k-step's fragments (Q3: the next slab's first, other stage)
                            constexpr int st = Q == 3 ? (S ^ 1) : S, ks = (Q + 1) & 3;
                            if constexpr (i < 4) rd_x32(buf ^ 1, st, ks, i);
                            else rd_w32(buf ^ 1, st, ks, i - 4);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if constexpr (Q == 0 && !(MAGE4_ABL & 2) && !FIRST) {                  // W(j+1): 8 pieces
                            if constexpr (i == 4) dma_m0((S ^ 1) * G4_STAGE + G4_WOFF);
                            if constexpr (i >= 5 && i < 13) g4_dma<i - 5>(voffW[i - 5], w_src);
                            if constexpr (i >= 4 && i < 13) __builtin_amdgcn_sched_barrier(0);
                        }
                        if constexpr (Q == 3 && !(MAGE4_ABL & 2) && !LAST) {                   // A(j+2): 8 pieces
                            if constexpr (i == 1) dma_m0(S * G4_STAGE);
                            if constexpr (i >= 2 && i < 10) g4_dma<i - 2>(voffA[i - 2], a_src);
                            if constexpr (i >= 1 && i < 10) __builtin_amdgcn_sched_barrier(0);
                        }
                    });
                };
                quarter(std::integral_constant<int, 0>{});
                if constexpr (!(MAGE4_ABL & 8) && !FIRST) w_src = (j == nk - 2) ? w_next : w_src + 128;
                quarter(std::integral_constant<int, 1>{});
                quarter(std::integral_constant<int, 2>{});
                if constexpr (FIRST) __builtin_amdgcn_s_waitcnt(0x8070);
                else __builtin_amdgcn_s_waitcnt(0x0070);
                ring_barrier();
                __builtin_amdgcn_sched_barrier(0);
                quarter(std::integral_constant<int, 3>{});
                if constexpr (LAST && !(MAGE4_ABL & 2)) {                                       // the next tile's slab 1 (A and W), as the 16 x 16 schedule sends it
                    dma_m0(S * G4_STAGE);
                    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffA[decltype(u_)::value], a_src); });
                    dma_m0(S * G4_STAGE + G4_WOFF);
                    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffW[decltype(u_)::value], w_src); });
                }
                if constexpr (!(MAGE4_ABL & 8)) a_src = (j == nk - 3) ? a_next : a_src + 128;
                if constexpr (!(MAGE4_ABL & 8) && LAST) w_src += 128;
            };
#define slab slab32
#endif
            typedef std::integral_constant<int, 0> S0;
            typedef std::integral_constant<int, 1> S1;
            slab(S0{}, std::true_type{}, std::false_type{}, 0);
            slab(S1{}, std::false_type{}, std::false_type{}, 1);
            for (int j = 2; j < nk - 2; j += 2) {
                slab(S0{}, std::false_type{}, std::false_type{}, j);
                slab(S1{}, std::false_type{}, std::false_type{}, j + 1);
            }
            slab(S0{}, std::false_type{}, std::false_type{}, nk - 2);
            slab(S1{}, std::false_type{}, std::true_type{}, nk - 1);
#ifdef MAGE4_MFMA32
#undef slab
#endif
            // the last MFMAs' results must have left the matrix pipe before an accumulator is read (an asm statement gets no hazard padding)
            asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
            G4_STAMP(it, 1);
#if MAGE4_ABL & 1
            {
                f32x4 t = g4_acc_read<0>() + g4_acc_read<17>() + g4_acc_read<63>();
                if (t[0] + t[1] + t[2] + t[3] == 123456.789f) ((float*)g.Y)[0] = t[0] + biasm[0][0][0];
            }
#else
            char* win = smem + G4_RING + wave * 4096;
#pragma unroll
            for (int b = 0; b < (HALF ? 0 : 4); ++b) {
                if constexpr (PH == 2) {
                    biasm[1][0][b] = g.bias[n0 + 64 + b * 16 + l15];
                    lns[1][0][b] = g.ln_colsum[n0 + 64 + b * 16 + l15];
                    continue;
                }
                const int n = n0 + 64 + b * 16 + grp * 4;
                biasm[1][b] = *(const f32x4*)(g.bias + n);
                if constexpr (LN == LN_CONSUME) lns[1][b] = *(const f32x4*)(g.ln_colsum + n);
            }
            // gemm.hip's epilogue_lean, 64 x 64 outputs = 64 accumulator registers at a time.  (A software-pipelined rewrite -- 64 rows of staging
            // writes, then their reads under the next 64 rows' arithmetic -- was built and measured 5 % SLOWER per launch: the epilogue is not
            // waiting for its LDS round trips, it is issue-bound on the vector ALU at the clock the K loop's power draw leaves: 1.5 GHz.)
            if constexpr (QF) {
                g4_for<(HALF ? 2 : 4)>([&](auto c_) {
                    // h: the column half's index into biasm / lns, ha: into the accumulator blocks (HALF: the one half, kept in a128..a255)
                    constexpr int c = decltype(c_)::value, h = HALF ? 0 : c >> 1, mh = c & 1, ha = HALF ? 1 : h;
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 t[4][4];
                    g4_for<16>([&](auto q_) {
                        constexpr int q = decltype(q_)::value;
                        t[q >> 2][q & 3] = g4_acc_read<(ha * 8 + mh * 4 + (q >> 2)) * 4 + (q & 3), q == 0>();
                    });
                    if constexpr (PH == 1) {
                        // 64 packed columns [q_h | k_h] per head: this chunk is head h of the wave, sequences mh*4 .. mh*4 + 3
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) {
                            uint2 pk[4];
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                const f32x4 v = (t[mt][nt] - lns[h][nt] * ln_mean[mh * 4 + mt]) * ln_rstd[mh * 4 + mt] + biasm[h][nt];      // epilogue_lean's LN_CONSUME
                                pk[nt] = uint2{pack16x2<H16>(v[0], v[1]), pack16x2<H16>(v[2], v[3])};
                            }
                            // attention_mfma_kernel, one key block, every key visible: S^T = K Q^T, scale, max, exp
                            f32x4 st = g4_epi_qk<HF>(u32x4{pk[2].x, pk[2].y, pk[3].x, pk[3].y}, u32x4{pk[0].x, pk[0].y, pk[1].x, pk[1].y});
                            // (no contraction: there the scaled scores pass a select before the maximum is taken off, so the product is rounded --
                            // s * scale - max as ONE fma would give exp(> 0) at the maximum itself)
                            f32x4 p;
                            {
#pragma clang fp contract(off)
                                float mx = -INFINITY;
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    // TX: attention_mfma_kernel's causal select -- slot l15 sees the slots 4 grp + e <= l15
                                    if constexpr (TX) st[e] = (4 * qgrp + e <= ql15) ? st[e] * g.attn_scale : -INFINITY;
                                    else st[e] = st[e] * g.attn_scale;
                                    mx = fmaxf(mx, st[e]);
                                }
                                mx = fmaxf(mx, __shfl_xor(mx, 16));
                                mx = fmaxf(mx, __shfl_xor(mx, 32));
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    if constexpr (TX) p[e] = (4 * qgrp + e <= ql15) ? expf(st[e] - mx) : 0.f;
                                    else p[e] = expf(st[e] - mx);
                                }
                            }
                            pl[mt][0] = p;
                        }
                        g4_for<4>([&](auto mt_) { g4_acc_write<c * 4 + decltype(mt_)::value>(pl[decltype(mt_)::value][0]); });
                    } else {
                        long shift;
                        if constexpr (TX) shift = g.y_off;                                                         // (rows not regrouped: host)
                        else shift = (long)(tm * 256 / g.out_w) * (g.y_img_stride - g.out_w) + g.y_off;       // out_w % 256 == 0 (host): one group per tile
                        // the two heads' 16 rows x 64 B through the wave's staging window (epilogue_lean's swizzle; a wave's DS operations execute in order):
                        // stored as 2 x (8 rows x 128 B) instead of 2 x (16 rows x 64 B)
                        const int srow = (qgrp * 16 + ql15) >> 3, scc = ql15 & 7;
                        H16* op = (H16*)g.Y + ny0 + h * 64 + scc * 8;
                        const int wchunk = (qgrp & 1) * 2 + (qgrp >> 1);
                        g4_for<8>([&](auto q_) {           // the kept numerators of this row half
                            constexpr int q = decltype(q_)::value, hd = q >> 2, mt = q & 3;
                            pl[mt][hd] = g4_acc_read<(hd * 2 + mh) * 4 + mt>();
                        });
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) {
                            f32x4 mean4, rstd4;            // the statistics of this lane's four rows of the transposed blocks: 4 grp + e
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                mean4[e] = __shfl(ln_mean[mh * 4 + mt], 4 * grp + e);
                                rstd4[e] = __shfl(ln_rstd[mh * 4 + mt], 4 * grp + e);
                            }
#pragma unroll
                            for (int hd = 0; hd < 2; ++hd) {
                                const f32x4 p = pl[mt][hd];
                                float den = 0.f;
                                ashort4 phi, plo;
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    den += p[e];
                                    short ph, pw;
                                    attn_p_split<H16>(p[e], ph, pw);
                                    phi[e] = ph;
                                    plo[e] = pw;
                                }
                                den += __shfl_xor(den, 16);
                                den += __shfl_xor(den, 32);
                                f32x4 o[2];
                                ashort4 vt[2];
#pragma unroll
                                for (int b = 0; b < 2; ++b) {
                                    const int nt = hd * 2 + b;
                                    const f32x4 v = (t[mt][nt] - mean4 * lns[h][0][nt]) * rstd4 + biasm[h][0][nt];
                                    vt[b] = __builtin_bit_cast(ashort4, uint2{pack16x2<H16>(v[0], v[1]), pack16x2<H16>(v[2], v[3])});
                                }
                                g4_epi_pv<HF>(vt[0], vt[1], phi, plo, o[0], o[1]);
                                const float inv = 1.0f / den;
                                f32x4 v0, v1;
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[0][e]), __float_as_uint(o[1][e]), false, false);
                                    v0[e] = __uint_as_float(sw[0]) * inv;
                                    v1[e] = __uint_as_float(sw[1]) * inv;
                                }
                                *(u32x4*)(win + ql15 * 128 + (((hd * 4 + wchunk) ^ ((ql15 >> 1) & 7)) << 4)) =
                                    u32x4{pack16x2<H16>(v0[0], v0[1]), pack16x2<H16>(v0[2], v0[3]), pack16x2<H16>(v1[0], v1[1]), pack16x2<H16>(v1[2], v1[3])};
                            }
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                const int r = srow + 8 * i;
                                long yrow;
                                if constexpr (TX) yrow = row0 + frame_row(wm * 128 + mh * 64 + mt * 16 + r) + shift;
                                else yrow = (long)tm * 256 + frame_row(wm * 128 + mh * 64 + mt * 16 + r) + shift;
                                *(u32x4*)(op + yrow * g.ldy) = *(const u32x4*)(win + r * 128 + ((scc ^ ((r >> 1) & 7)) << 4));
                            }
                        }
                    }
                });
            } else {
            mage_gemm_desc e = {};
            e.M = 0x7fffffff;
            e.N = LN == LN_PRODUCE ? g.N : 0x7fffffff;
            e.K = g.K;
            e.Y = g.Y;
            e.ldy = g.ldy;
            e.y_dtype = g.y_dtype;
            e.out_h = 1;
            e.out_w = 0x7fffffff;
            e.y_mul_x = 1;
            e.y_off = g.y_off;
            e.y2 = g.y2;
            e.ldy2 = g.ldy2;
            e.ln_part = g.ln_part;
            g4_for<4>([&](auto c_) {
                constexpr int c = decltype(c_)::value, h = c >> 1, mh = c & 1;
                __builtin_amdgcn_sched_barrier(0);
                f32x4 t[4][4];
                g4_for<16>([&](auto q_) {
                    constexpr int q = decltype(q_)::value;
                    t[q >> 2][q & 3] = g4_acc_read<(h * 8 + mh * 4 + (q >> 2)) * 4 + (q & 3), q == 0>();
                });
                [[maybe_unused]] LnConsume lnc;
                if constexpr (LN == LN_CONSUME) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        lnc.mean[a] = ln_mean[mh * 4 + a];
                        lnc.rstd[a] = ln_rstd[mh * 4 + a];
                    }
#pragma unroll
                    for (int b = 0; b < 4; ++b) lnc.s[b] = lns[h][b];
                    if (g.y_dtype == MAGE_F32) epilogue_lean<ACT, float, 4, false, LN>(e, biasm[h], t, m0 + mh * 64, n0 + h * 64, lane, 1, win, 0, &lnc);
                    else epilogue_lean<ACT, H16, 4, false, LN>(e, biasm[h], t, m0 + mh * 64, n0 + h * 64, lane, 1, win, 0, &lnc);
                } else if constexpr (LN == LN_DUAL || LN == LN_GELUBWD) {
                    epilogue_lean<ACT, unsigned short, 4, false, LN>(e, biasm[h], t, m0 + mh * 64, n0 + h * 64, lane, 1, win, 0);       // bf16 rows (host check)
                } else {
                    if (g.y_dtype == MAGE_F32) epilogue_lean<ACT, float, 4, false, LN>(e, biasm[h], t, m0 + mh * 64, n0 + h * 64, lane, 1, win, 0);
                    else epilogue_lean<ACT, H16, 4, false, LN>(e, biasm[h], t, m0 + mh * 64, n0 + h * 64, lane, 1, win, 0);
                }
            });
            }
#endif
            G4_STAMP(it, 2);
            // the next tile's first fragments (its slab 0 has been in stage 0 since the last slab's barrier)
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (KEEP) {                          // the entry's V part
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) rd_wv(0, 0, 0, nt);
#pragma unroll
                for (int m = 0; m < 4; ++m) rd_x1(0, 0, 0, m);
            } else if (c_tile + nwg8 < chunk1) {
#ifdef MAGE4_MFMA32
#pragma unroll
                for (int b = 0; b < 4; ++b) { rd_w32(0, 0, 0, b); rd_x32(0, 0, 0, b); }
#else
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) rd_w1(0, 0, 0, nt);
#pragma unroll
                for (int m = 0; m < 4; ++m) rd_x1(0, 0, 0, m);
#endif
            }
        };
        if constexpr (QF) {
            tile(std::integral_constant<int, 1>{});
            tile(std::integral_constant<int, 2>{});
        } else {
            tile(std::integral_constant<int, 0>{});
        }
    }
}

template <int ACT, int EK, int LN, bool RB, bool HF = false>
__global__ __launch_bounds__(256) void gemm4_kernel(const Gemm4Args g) {
    gemm4_body<ACT, EK, LN, RB, HF, false>(g);
}
// the fused H / W axial attention entry: in_proj and the attention in one launch (QF, see gemm4_body)
template <bool HF>
__global__ __launch_bounds__(256) void gemm4_attn_kernel(const Gemm4Args g) {
    gemm4_body<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, HF, true>(g);
}
// the same entry for the temporal blocks (TX): a tile is 16 adjacent positions x the 16 slots of one clip, causal along the slots
template <bool HF>
__global__ __launch_bounds__(256) void gemm4_tattn_kernel(const Gemm4Args g) {
    gemm4_body<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, HF, true, true>(g);
}

template <int ACT, int EK, int LN, bool RB, bool HF = false, bool QF = false, bool TX = false>
int launch4(const mage_gemm_desc* d, hipStream_t s, int n_cu, int attn_axis = 0, float attn_scale = 0.f) {
    Gemm4Args a;
    a.attn_axis = attn_axis;
    a.attn_scale = attn_scale;
    a.out_w = d->out_w;
    a.y_img_stride = d->y_img_stride;
    if constexpr (TX) a.y_img_stride = d->out_w / 16;  // (out_w = hw, the slot stride; nothing is regrouped, so the second field carries the tiles per clip)
    a.A = d->A;
    a.W = d->W;
    a.Y = d->Y;
    a.bias = d->bias ? d->bias : (const float*)mage_zero_page();      // no bias (the data-gradient GEMMs of training): 16 KiB of zeros, N <= 4096
    a.ln_stats = d->ln_stats;
    a.ln_colsum = d->ln_colsum;
    a.residual = d->residual;
    a.ln_part = d->ln_part;
    a.y2 = d->y2;
    a.M = d->M;
    a.N = d->N;
    a.K = d->K;
    a.lda = d->lda;
    a.ldw = d->ldw ? d->ldw : d->K;
    a.ldy = d->ldy;
    a.ldr = d->ldr;
    a.ldy2 = d->ldy2;
    a.y_dtype = d->y_dtype;
    a.a_off = d->a_off;
    a.y_off = d->y_off;
    a.ntiles_n = d->N / (QF ? 384 : 256);              // (QF: an entry = 256 [q | k] + 128 v rows of the packed weight)
    a.ntiles = (d->M / 256) * a.ntiles_n;
    // staggered start (gemm.hip, launch_tile): the workgroups of an XCD start in G groups spread over a fraction of one tile period, so that
    // the tiles' output bursts (128-256 KiB per CU at once: HBM-bound when all 256 CUs store together) fall under other groups' K loops
    const int st_groups = mage_options().gemm4_stagger_groups, st_percent = mage_options().gemm4_stagger_percent;
    a.stagger_groups = 0;
    a.stagger_sleeps = 0;
    const int grid = a.ntiles >= n_cu ? n_cu : ((a.ntiles + 7) & ~7);
    if (st_groups > 1 && a.ntiles / grid >= 6) {
        const long period = (long)(d->K / 64) * 3100 + 9000;
        a.stagger_groups = st_groups;
        a.stagger_sleeps = (int)(period * st_percent / 100 / st_groups / 1024);
    }
    int r;
    if constexpr (TX) r = mage_gemm_launch<gemm4_tattn_kernel<HF>>(grid, 256, G4_LDS, s, a);
    else if constexpr (QF) r = mage_gemm_launch<gemm4_attn_kernel<HF>>(grid, 256, G4_LDS, s, a);
    else r = mage_gemm_launch<gemm4_kernel<ACT, EK, LN, RB, HF>>(grid, 256, G4_LDS, s, a);
    return r < 0 ? r : 1;
}

}  // namespace

namespace {

// ======================================================================================================================================
// gemm_tn4_kernel: the weight-gradient GEMM  P[s][n][k] = sum over the tokens t of slice s of dY[t][n] X[t][k]  (gemm_tn.hip, mage_gemm_tn) on the
// one-wave-per-SIMD schedule: 4 waves x 128 (dY columns) x 128 (X columns), the accumulator file behind inline-asm MFMAs, ONE barrier per
// 64-token slab at the 3/4 point, the loads placed between the MFMAs.  LDS image, transposing fragment reads (ds_read_b64_tr_b16), operand
// roles and the order of the MFMAs per accumulator are gemm_tn_kernel's: the same bits in every partial sum (and in the bias-gradient column
// sums, which the first column of waves of the first X tile takes from the dY fragments with v_dot2_f32_bf16 as before).
struct Tn4Args {
    const unsigned short* A;   // dY [T, lda]
    const unsigned short* B;   // X  [T, ldb]
    float* P;                  // [n_split][N][K]
    float* DB;                 // [n_split][N] or null
    long lda, ldb, T, tps;
    int N, K, n_split, ntk;
};
typedef short g4_tr4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ g4_tr4 g4_lds_tr(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) g4_tr4*)p); }

template <bool DB>
__global__ __launch_bounds__(256) void gemm_tn4_kernel(const Tn4Args g) {
    constexpr int PART = 32768, STAGE = 2 * PART;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    g4_claim_accumulators();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x / g.n_split, s = blockIdx.x - tile * g.n_split;
    const int tm = tile / g.ntk, tk = tile - tm * g.ntk;
    const long t_begin = (long)s * g.tps;
    const long t_end = t_begin + g.tps < g.T ? t_begin + g.tps : g.T;
    const int nslab = (int)((t_end - t_begin) >> 6);                 // whole slabs only (host: T % 64 == 0), >= 2 (host)
    // ---- loader: wave w moves the 8 token blocks of column strip w (64 columns) of each operand per slab: units w*8 + u
    const int rr = lane >> 3, pc = lane & 7;
    unsigned voffA[8], voffB[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int col_in_strip = (((pc >> 1) ^ (rr & 3) ^ (u & 1)) << 4) + ((pc & 1) << 3);
        voffA[u] = (unsigned)(((long)(u * 8 + rr) * g.lda + wave * 64 + col_in_strip) * 2 + 8192 - u * 1024);
        voffB[u] = (unsigned)(((long)(u * 8 + rr) * g.ldb + wave * 64 + col_in_strip) * 2 + 8192 - u * 1024);
    }
    const char* a_src = (const char*)(g.A + t_begin * g.lda + (long)tm * 256) - 4096;
    const char* b_src = (const char*)(g.B + t_begin * g.ldb + (long)tk * 256) - 4096;
    const long da = 64 * g.lda * 2, db_ = 64 * g.ldb * 2;
    int a_slab = 0, b_slab = 0;                                       // slab index the cursors point at (they stop at the last slab)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * 8192 + 4096;
    auto dma_m0 = [&](unsigned lds_group) __attribute__((always_inline)) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(lds0 + lds_group) : "memory");
    };
    auto a_advance = [&]() __attribute__((always_inline)) {
        const bool more = a_slab + 1 < nslab;
        a_src = more ? a_src + da : a_src;
        a_slab = more ? a_slab + 1 : a_slab;
    };
    auto b_advance = [&]() __attribute__((always_inline)) {
        const bool more = b_slab + 1 < nslab;
        b_src = more ? b_src + db_ : b_src;
        b_slab = more ? b_slab + 1 : b_slab;
    };
    // ---- compute state
    const int wm = wave >> 1, wn = wave & 1;
    const int i15 = lane & 15, grp = lane >> 4;
    const int lane_off = grp * 1024 + (i15 >> 2) * 128 + (i15 & 3) * 8;
    const int sw = (i15 >> 2) ^ (grp & 1);
    g4_tr4 bfh[2][8][2], afh[2][4][2];                 // fragment halves: [buffer][16-column block][tokens 0-3 | 4-7 of the lane group's 8]
    auto rd_b = [&](int buf, int stage, int t, int nt, int h) __attribute__((always_inline)) {       // X columns wn*128 + nt*16
        bfh[buf][nt][h] = g4_lds_tr(smem + stage * STAGE + PART + ((wn * 2 + (nt >> 2)) * 8 + t * 4) * 1024 + lane_off + (((nt & 3) ^ sw) << 5) + h * 512);
    };
    auto rd_a = [&](int buf, int stage, int t, int mt, int h) __attribute__((always_inline)) {       // dY columns wm*128 + mt*16
        afh[buf][mt & 3][h] = g4_lds_tr(smem + stage * STAGE + ((wm * 2 + (mt >> 2)) * 8 + t * 4) * 1024 + lane_off + (((mt & 3) ^ sw) << 5) + h * 512);
    };
    auto frag = [](const g4_tr4 (&h)[2]) __attribute__((always_inline)) {
        return __builtin_bit_cast(u32x4, __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7));
    };
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;
    const bf16x2v ones2 = {(__bf16)1.0f, (__bf16)1.0f};
    [[maybe_unused]] float dbs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] auto db_acc = [&](int mt, const g4_tr4 (&h)[2]) __attribute__((always_inline)) {       // column sums of dY from its fragments (gemm_tn_kernel's order)
        const uint2 w0 = __builtin_bit_cast(uint2, h[0]), w1 = __builtin_bit_cast(uint2, h[1]);
        float d = dbs[mt];
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2v, w0.x), ones2, d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2v, w0.y), ones2, d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2v, w1.x), ones2, d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2v, w1.y), ones2, d, false);
        dbs[mt] = d;
    };

    // prologue: slabs 0 and 1 complete, slab 0's first fragments in registers
    dma_m0(0);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffA[decltype(u_)::value], a_src); });
    dma_m0(PART);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffB[decltype(u_)::value], b_src); });
    a_advance();
    b_advance();
    dma_m0(STAGE);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffA[decltype(u_)::value], a_src); });
    dma_m0(STAGE + PART);
    g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffB[decltype(u_)::value], b_src); });
    a_advance();
    b_advance();
    __builtin_amdgcn_s_waitcnt(0x0F70);
    ring_barrier();
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) { rd_b(0, 0, 0, nt, 0); rd_b(0, 0, 0, nt, 1); }
#pragma unroll
    for (int m = 0; m < 4; ++m) { rd_a(0, 0, 0, m, 0); rd_a(0, 0, 0, m, 1); }

    // one slab (stage S); accumulator block of (mt, nt) = mt*8 + nt.  Quarters as in gemm4_kernel: (t0, mt 0-3) (t0, mt 4-7) (t1, mt 0-3) | barrier |
    // (t1, mt 4-7); 8 / 24 / 8 / 24 transposing 8-byte fragment reads and the 16 LDS-DMA pieces between the MFMAs
    auto slab = [&](auto S_, auto FIRST_) __attribute__((always_inline)) {
        constexpr int S = decltype(S_)::value;
        constexpr bool FIRST = decltype(FIRST_)::value;
        // ---- Q0: (t0, mt 0-3) from bfh[0], afh[0]; reads dY(t0, mt 4-7) -> afh[1]; X pieces of slab j+1... (sent one slab ahead: see below)
        g4_for<32>([&](auto i_) {
            constexpr int i = decltype(i_)::value, m = i >> 3, nt = i & 7;
            g4_mfma<m * 8 + nt, FIRST, i == 0>(frag(bfh[0][nt]), frag(afh[0][m]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i < 8) {
                rd_a(1, S, 0, 4 + (i >> 1), i & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (DB && nt == 7) {
                db_acc(m, afh[0][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (!FIRST && i == 8) {
                dma_m0((S ^ 1) * STAGE + PART);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (!FIRST && i > 8 && (i & 1) == 1 && i < 25) {
                g4_dma<((i - 9) >> 1)>(voffB[(i - 9) >> 1], b_src);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        if constexpr (!FIRST) b_advance();
        // ---- Q1: (t0, mt 4-7) from bfh[0], afh[1]; reads dY(t1, mt 0-3) -> afh[0], X(t1) -> bfh[1]
        g4_for<32>([&](auto i_) {
            constexpr int i = decltype(i_)::value, m = i >> 3, nt = i & 7;
            g4_mfma<(4 + m) * 8 + nt, FIRST, i == 0>(frag(bfh[0][nt]), frag(afh[1][m]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i < 24) {
                if constexpr (i < 8) rd_a(0, S, 1, i >> 1, i & 1);
                else rd_b(1, S, 1, (i - 8) >> 1, i & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (DB && nt == 7) {
                db_acc(4 + m, afh[1][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        // ---- Q2: (t1, mt 0-3) from bfh[1], afh[0]; reads dY(t1, mt 4-7) -> afh[1]
        g4_for<32>([&](auto i_) {
            constexpr int i = decltype(i_)::value, m = i >> 3, nt = i & 7;
            g4_mfma<m * 8 + nt, false, i == 0>(frag(bfh[1][nt]), frag(afh[0][m]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i < 8) {
                rd_a(1, S, 1, 4 + (i >> 1), i & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (DB && nt == 7) {
                db_acc(m, afh[0][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        __builtin_amdgcn_s_waitcnt(0x0070);            // vmcnt(0) lgkmcnt(0)
        ring_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- Q3: (t1, mt 4-7) from bfh[1], afh[1]; next slab's first fragments from the other stage; dY pieces of slab j+2 -> this stage
        g4_for<32>([&](auto i_) {
            constexpr int i = decltype(i_)::value, m = i >> 3, nt = i & 7;
            g4_mfma<(4 + m) * 8 + nt, false, i == 0>(frag(bfh[1][nt]), frag(afh[1][m]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i < 24) {
                if constexpr (i < 8) rd_a(0, S ^ 1, 0, i >> 1, i & 1);
                else rd_b(0, S ^ 1, 0, (i - 8) >> 1, i & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (DB && nt == 7) {
                db_acc(4 + m, afh[1][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (i == 24) {
                dma_m0(S * STAGE);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        g4_for<8>([&](auto u_) { g4_dma<decltype(u_)::value>(voffA[decltype(u_)::value], a_src); });
        __builtin_amdgcn_sched_barrier(0);
        a_advance();
    };
    typedef std::integral_constant<int, 0> S0;
    typedef std::integral_constant<int, 1> S1;
    slab(S0{}, std::true_type{});
    int j = 1;
    for (; j + 1 < nslab; j += 2) {
        slab(S1{}, std::false_type{});
        slab(S0{}, std::false_type{});
    }
    if (j < nslab) slab(S1{}, std::false_type{});
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    // ---- epilogue: lane (i, grp) of block (mt, nt) holds row (dY column) mt*16 + i, columns (X columns) nt*16 + grp*4 + {0..3}
    float* out = g.P + ((long)s * g.N + (long)tm * 256 + wm * 128) * g.K + (long)tk * 256 + wn * 128;
    g4_for<64>([&](auto q_) {
        constexpr int q = decltype(q_)::value, mt = q >> 3, nt = q & 7;
        *(f32x4*)(out + (long)(mt * 16 + i15) * g.K + nt * 16 + grp * 4) = g4_acc_read<q, (q & 15) == 0>();
    });
    if constexpr (DB) {
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            float v = dbs[mt];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (grp == 0) g.DB[(long)s * g.N + (long)tm * 256 + wm * 128 + mt * 16 + i15] = v;
        }
    }
}

}  // namespace

int mage_gemm4h_try(const mage_gemm_desc* d, hipStream_t s, int n_cu);      // gemm4h.hip (applies its own tile-count rule)

// 1 = launched, 0 = not eligible (the caller falls through to the 8-wave kernels), < 0 = error.
// Eligible: bf16 plain GEMMs (no gather, rows not regrouped) with the epilogues y = act(acc + b) (b optional), its LayerNorm-consuming form, or
// training's two c_fc forms (pre-activation + activated rows; data gradient times QuickGELU' of the saved rows),
// act = none | QuickGELU, M and N multiples of 256, K a multiple of 128 in [256, 1024], at least four tiles per CU: the decoder's QKV and c_fc
// at full-loop sizes (12 of the 24 GEMM launches of a decoder pass, 100 of 187 ms of a cfg2 call).  Measured against the 8-phase kernel
// (tools/probes/gemm4_probe.hip, same box, interleaved): QKV +11-12 %, c_fc +7-9 %, N = 512 / K = 512 +4 %; K = 2048 with N = 512 is 9 %
// SLOWER (its A panel is shared by two column tiles only: the loader's HBM latency shows) -- hence the K bound.  The x + Linear(.) kinds
// stay on the 8-wave kernels: their tiles are bounded by the residual / output bursts, not by the K loop.
int mage_gemm4_try(const mage_gemm_desc* d, hipStream_t s) {
    const bool hf = d->dtype == MAGE_F16;              // f16 operands: the bias and LayerNorm-consuming forms of the generation path
    if ((d->dtype != MAGE_BF16 && !hf) || d->n_split > 1) return 0;
    if (mage_options().gemm_no_4w) return 0;           // (mage_set_option: tests run the same product on both kernels in one process)
    if (d->M % 256 || d->N % 256 || d->K % 128 || d->K < 256 || d->K > 1024) return 0;
    if (d->taps_h * d->taps_w != 1 || d->stride != 1 || d->dy0 || d->dx0 || d->in_h != d->out_h || d->in_w != d->out_w || d->a_half) return 0;
    if (d->out_h != 1 || d->out_w < d->M || d->y_mul_x != 1) return 0;                     // plain rows in, plain rows out
    if (d->scale || d->rowadd || d->post_relu || d->res_half) return 0;
    if (d->residual || d->ln_part || d->rowadd) return 0;
    if (!d->bias && (d->N > 4096 || d->ln_stats || mage_zero_page() == nullptr)) return 0;
    if ((d->ln_colsum != nullptr) != (d->ln_stats != nullptr)) return 0;
    // training's two c_fc forms: y2 with QuickGELU = pre-activation rows AND activated rows (LN_DUAL); MAGE_ACT_QUICKGELU_GRAD = the data gradient
    // times QuickGELU'(saved pre-activation rows y2) (LN_GELUBWD); both bf16 rows, no LayerNorm fold
    const bool dual = d->y2 && d->act == MAGE_ACT_QUICKGELU && !d->ln_stats;
    const bool gbwd = d->y2 && d->act == MAGE_ACT_QUICKGELU_GRAD && !d->ln_stats;
    if (d->y2 && !dual && !gbwd) return 0;
    // measured in the training step (rocprofv3, same box): the data-gradient form 736 us per launch on the 8-phase kernel, 840 here (its saved
    // rows are requested inside the epilogue: two waves per SIMD hide that round trip, one does not); the two-output form 787 vs 794.  Both
    // stay on the 8-phase kernel unless the option gemm4_train_forms asks for them here (the instantiations are kept: tests compare the bits)
    if ((dual || gbwd) && !mage_options().gemm4_train_forms) return 0;
    if ((dual || gbwd) && (d->y_dtype != MAGE_BF16 || d->ldy2 % 8 || (((uintptr_t)d->y2) & 15))) return 0;
    if (!dual && !gbwd && d->act != MAGE_ACT_NONE && d->act != MAGE_ACT_QUICKGELU) return 0;
    if (d->y_dtype != MAGE_F32 && d->y_dtype != d->dtype) return 0;
    if (hf && (dual || gbwd)) return 0;
    if (d->ldy % 8 || d->lda % 8 || (((uintptr_t)d->bias | (uintptr_t)d->ln_colsum) & 15) || (((uintptr_t)d->ln_stats) & 7)) return 0;
    const int n_cu = mage_gemm_cu_count();
    // at least four tiles per CU: with two (the incremental loop's c_fc at 16 k rows) the prologue's un-overlapped slab pair and the single
    // tile boundary cost more than the K loop gains (47.5 vs 41 us per launch there): those sizes stay on the lockstep kernel
    const long ntiles = (long)(d->M / 256) * (d->N / 256);
    const bool few_tiles = ntiles < 4L * n_cu;          // gemm4_kernel itself stays above it; its split-half form also runs below (see mage_gemm4h_try)
    const int ldw = d->ldw ? d->ldw : d->K;
    if (((long)d->M + d->a_off) * d->lda * 2 + 16384 >= (1L << 32) || (long)d->N * ldw * 2 + 16384 >= (1L << 32)) return 0;     // 32-bit lane offsets
    if (!dual && !gbwd)
        if (const int r = mage_gemm4h_try(d, s, n_cu)) return r;         // K = 512, 16-bit rows out: the split-half form (gemm4h.hip)
    if (few_tiles) return 0;
    if (dual) return launch4<MAGE_ACT_QUICKGELU, EK_BIAS, LN_DUAL, false>(d, s, n_cu);
    if (gbwd) return launch4<MAGE_ACT_NONE, EK_BIAS, LN_GELUBWD, false>(d, s, n_cu);
    if (hf) {
        if (d->ln_stats) {
            if (d->act == MAGE_ACT_NONE) return launch4<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, true>(d, s, n_cu);
            return launch4<MAGE_ACT_QUICKGELU, EK_BIAS, LN_CONSUME, false, true>(d, s, n_cu);
        }
        if (d->act == MAGE_ACT_NONE) return launch4<MAGE_ACT_NONE, EK_BIAS, LN_NONE, false, true>(d, s, n_cu);
        return launch4<MAGE_ACT_QUICKGELU, EK_BIAS, LN_NONE, false, true>(d, s, n_cu);
    }
    if (d->ln_stats) {
        if (d->act == MAGE_ACT_NONE) return launch4<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false>(d, s, n_cu);
        return launch4<MAGE_ACT_QUICKGELU, EK_BIAS, LN_CONSUME, false>(d, s, n_cu);
    }
    if (d->act == MAGE_ACT_NONE) return launch4<MAGE_ACT_NONE, EK_BIAS, LN_NONE, false>(d, s, n_cu);
    return launch4<MAGE_ACT_QUICKGELU, EK_BIAS, LN_NONE, false>(d, s, n_cu);
}

// The fused H / W axial attention (include/mage_hip_ext.h): N = 3C, W / bias / ln_colsum packed per group of 4 heads, ao out
extern "C" int mage_gemm_attn_fused_qkv(const mage_gemm_desc* d, int32_t axis, float scale, void* stream) {
    MAGE_CHECK_ARG(d != nullptr, "mage_gemm_attn_fused_qkv: null descriptor");
    MAGE_CHECK_ARG(axis >= 0 && axis <= 2, "mage_gemm_attn_fused_qkv: axis %d (0 = T of clips of 16 slots, 1 = H, 2 = W of 16 x 16 frames)", (int)axis);
    if (axis == 0) {
        // T: the rows come as slots of out_w = hw rows (in_w, a_img_stride and y_img_stride say the same: nothing is regrouped), 16 slots per clip.
        // A tile is 16 adjacent positions x the 16 slots of one clip; a lane's offset inside a tile reaches row 15 hw + 15
        const long hw = d->out_w;
        MAGE_CHECK_ARG(hw >= 16 && hw % 16 == 0 && d->M > 0 && d->M % (16 * hw) == 0,
                       "mage_gemm_attn_fused_qkv: axis 0: out_w=%d (the rows of one slot) a multiple of 16, M=%d whole clips of 16 slots", d->out_w, d->M);
        MAGE_CHECK_ARG(d->y_img_stride == d->out_w && d->a_img_stride == d->out_w,
                       "mage_gemm_attn_fused_qkv: axis 0: rows are not regrouped (y_img_stride=%d, a_img_stride=%d must equal out_w=%d)", d->y_img_stride,
                       d->a_img_stride, d->out_w);
        MAGE_CHECK_ARG(d->a_off % (16 * hw) == 0 && d->y_off % (16 * hw) == 0, "mage_gemm_attn_fused_qkv: axis 0: a_off=%d and y_off=%d must be whole clips", d->a_off,
                       d->y_off);
        MAGE_CHECK_ARG(d->lda > 0 && (15 * hw + 16) * d->lda * 2 + 16384 < (1L << 32),
                       "mage_gemm_attn_fused_qkv: axis 0: a clip's rows beyond the kernel's 32-bit lane offsets");
    }
    MAGE_CHECK_ARG(d->dtype == MAGE_BF16 || d->dtype == MAGE_F16, "mage_gemm_attn_fused_qkv: bf16 or f16 operands");
    MAGE_CHECK_ARG(d->A && d->W && d->Y && d->bias && d->ln_stats && d->ln_colsum, "mage_gemm_attn_fused_qkv: A, W, Y, bias, ln_stats, ln_colsum must be given");
    MAGE_CHECK_ARG(d->M > 0 && d->M % 256 == 0 && d->N > 0 && d->N % 384 == 0 && d->K % 128 == 0 && d->K >= 256 && d->K <= 1024,
                   "mage_gemm_attn_fused_qkv: M=%d a multiple of 256 (whole 16 x 16 frames), N=%d = 3C a multiple of 384 (groups of 4 heads of width 32), K=%d a "
                   "multiple of 128 in [256, 1024]", d->M, d->N, d->K);
    MAGE_CHECK_ARG(d->taps_h * d->taps_w == 1 && d->stride == 1 && !d->dy0 && !d->dx0 && d->in_h == 1 && d->out_h == 1 && d->in_w == d->out_w && !d->a_half &&
                       d->y_mul_x == 1 && (axis == 0 || d->out_w >= d->M || (d->out_w % 256 == 0 && d->a_img_stride == d->out_w)) && d->a_off % 256 == 0 && d->a_off >= 0,
                   "mage_gemm_attn_fused_qkv: plain rows in (a_off a multiple of 256), output rows regrouped whole frames at a time");
    MAGE_CHECK_ARG(!d->scale && !d->shift && !d->rowadd && !d->residual && !d->post_relu && !d->res_half && !d->y2 && !d->ln_part && !d->head_w && !d->a_relu &&
                       d->n_split <= 1 && d->act == MAGE_ACT_NONE,
                   "mage_gemm_attn_fused_qkv: the LayerNorm-consuming bias epilogue only");
    MAGE_CHECK_ARG(d->y_dtype == d->dtype && d->ldy % 8 == 0 && d->ldy >= d->N / 3 && (((uintptr_t)d->Y) & 15) == 0 && d->y_off >= 0,
                   "mage_gemm_attn_fused_qkv: 16-bit output rows of the operands' type, ldy a multiple of 8 and >= C, Y 16-byte aligned");
    const int ldw = d->ldw ? d->ldw : d->K;
    MAGE_CHECK_ARG(ldw == d->K && d->lda % 8 == 0 && d->lda >= d->K, "mage_gemm_attn_fused_qkv: W packed [N][K], lda a multiple of 8");
    MAGE_CHECK_ARG((((uintptr_t)d->A | (uintptr_t)d->W | (uintptr_t)d->bias | (uintptr_t)d->ln_colsum) & 15) == 0 && (((uintptr_t)d->ln_stats) & 7) == 0,
                   "mage_gemm_attn_fused_qkv: operands must be 16-byte aligned");
    MAGE_CHECK_ARG(((long)d->M + d->a_off) * d->lda * 2 + 16384 < (1L << 32) && (long)d->N * ldw * 2 + 16384 < (1L << 32),
                   "mage_gemm_attn_fused_qkv: operands beyond the kernel's 32-bit lane offsets");
    hipStream_t s = (hipStream_t)stream;
    const int n_cu = mage_gemm_cu_count();
    int r;
    if (axis == 0)
        r = d->dtype == MAGE_F16 ? launch4<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, true, true, true>(d, s, n_cu, axis, scale)
                                 : launch4<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, false, true, true>(d, s, n_cu, axis, scale);
    else
        r = d->dtype == MAGE_F16 ? launch4<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, true, true>(d, s, n_cu, axis, scale)
                                 : launch4<MAGE_ACT_NONE, EK_BIAS, LN_CONSUME, false, false, true>(d, s, n_cu, axis, scale);
    return r < 0 ? r : MAGE_OK;
}

extern "C" int mage_gemm_attn_fused_qkv_kernel_name(const mage_gemm_desc* d, int32_t axis, char* buf, int32_t len) {
    MAGE_CHECK_ARG(buf != nullptr && len > 0, "mage_gemm_attn_fused_qkv_kernel_name: no buffer");
    const void* kernel = nullptr;
    mage_gemm_plan = &kernel;
    const int r = mage_gemm_attn_fused_qkv(d, axis, 1.f, nullptr);
    mage_gemm_plan = nullptr;
    if (r != MAGE_OK) return r;
    return mage_kernel_symbol_name(kernel, buf, len, "mage_gemm_attn_fused_qkv_kernel_name");
}

// mage_gemm_tn on the one-wave-per-SIMD schedule: 1 = launched, 0 = not eligible (gemm_tn.hip then runs its 8-wave kernel)
int mage_gemm_tn4_try(const void* dY, int64_t lda, const void* X, int64_t ldb, int64_t T, int32_t N, int32_t K, int32_t n_split, int64_t tps,
                      float* partials, float* db_partials, hipStream_t stream) {
    if (mage_options().gemm_no_4w) return 0;
    if (T % 64 || tps % 64 || tps < 128 || (T - (int64_t)(n_split - 1) * tps) < 128) return 0;          // whole slabs, at least two per slice
    if (lda * 2 * 64 + 16384 >= (1L << 31) || ldb * 2 * 64 + 16384 >= (1L << 31)) return 0;              // 32-bit lane offsets inside a slab
    const int dev = mage_device_index();
    if (dev < 0) return 0;
    static bool attr[MAGE_MAX_DEVICES] = {false};
    if (!attr[dev]) {
        (void)hipFuncSetAttribute((const void*)gemm_tn4_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)gemm_tn4_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        attr[dev] = true;
    }
    Tn4Args a;
    a.A = (const unsigned short*)dY;
    a.B = (const unsigned short*)X;
    a.P = partials;
    a.DB = db_partials;
    a.lda = lda;
    a.ldb = ldb;
    a.T = T;
    a.tps = tps;
    a.N = N;
    a.K = K;
    a.n_split = n_split;
    a.ntk = K / 256;
    const long grid = (long)(N / 256) * (K / 256) * n_split;
    if (db_partials) hipLaunchKernelGGL(gemm_tn4_kernel<true>, dim3((unsigned)grid), dim3(256), 128 * 1024, stream, a);
    else hipLaunchKernelGGL(gemm_tn4_kernel<false>, dim3((unsigned)grid), dim3(256), 128 * 1024, stream, a);
    MAGE_CHECK_LAUNCH("mage_gemm_tn");
    return 1;
}
