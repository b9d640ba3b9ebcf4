// gemm4m_kernel: the decoder MLP x + c_proj(QuickGELU(c_fc(LN(x)))) of one block in ONE launch (C = 512, hidden = 2048; mage_mlp_fused).
//
// The pair it replaces writes the hidden rows (M x 2048, 16 bit) to memory and reads them straight back.  Here a workgroup owns a 128-row tile
// of the residual stream for both GEMMs and walks the hidden dimension in CHUNKS of 32 units; a chunk of h lives in registers only:
//     GEMM 1 (chunk c): hacc[32 rows x 32 hidden units per wave] = x W1'^T over K = 512 (16 k-steps into one accumulator, k ascending)
//     chunk epilogue  : h = QuickGELU(rstd (hacc - mean s) + c1), rounded to the 16-bit type: gemm4h's operations in gemm4h's order
//     GEMM 2 (chunk c): out[32 rows x 512 columns per wave] += h W2^T -- ONE k-step (k = 32 c .. 32 c + 31) into each of the 64 accumulator blocks
// so every output element sees c_proj's k-steps in ascending order into one accumulator, and every h element c_fc's: with the same MFMA and the
// same epilogue operations (the closing epilogue is epilogue_lean's two-tile form, residual in the epilogue + LN_PRODUCE, operation for operation)
// the bits are the pair's.
//
// Wave = 32 rows (two 16-row tiles mt) x all 512 output columns: 64 accumulator blocks = 256 literal AGPRs (gemm4_regs.h); its x rows are the
// B-operand fragments of GEMM 1 for the whole tile (128 VGPRs, loaded once per tile).  The closing epilogue takes the residual from those same
// registers (the rows are not read a second time) and hands each 64-column slice's registers to the next tile's rows as soon as the slice is
// staged, so the next tile's rows arrive under the epilogue with nothing waiting for them; the first tile's are loaded in the prologue.
// Operand roles: GEMM 1 takes the W1 fragment as A-operand, so an accumulator block holds (lane = row l15, register e of lane group g = hidden unit
// 4 g + e of the block's 16); W1's rows are gathered into LDS in the order  slot (t, r) <- hidden unit 8 (r / 4) + 4 t + r % 4  (t = block 0 | 1 of the
// chunk), so that a lane's two packed blocks are the 8 CONSECUTIVE k = 8 g .. 8 g + 7 of GEMM 2's B-operand, in natural order (nothing is permuted
// inside an MFMA).  GEMM 2 takes the W2 fragment as A-operand: the output accumulators have the layout of every other GEMM kernel (lane = row,
// registers = 4 consecutive columns), which is what epilogue_lean expects.
//
// Schedule of chunk c (two phases of 64 MFMAs, one barrier in the middle of each; rings of two stages for W1 and for W2, 32 KB per stage):
//     Pa(c): GEMM 1 (c)      || activation of chunk c-1, block t = 1, and its pack   second half: LDS-DMA of W2(c),   first fragments of GEMM 2 (c-1)
//     Pb(c): GEMM 2 (c-1)    || activation of chunk c, block t = 0 (in place)         second half: LDS-DMA of W1(c+2), first fragments of GEMM 1 (c+1)
// A stage is requested one whole chunk before the barrier that publishes it (s_waitcnt vmcnt(8): the 8 pieces of the other ring are younger).
// The epilogue arithmetic is single-instruction asm statements between the MFMA statements (gemm4h's way), ONE per MFMA slot: what a wave issues
// for free beside a 16-cycle MFMA is 8 cycles, one transcendental or convert or two plain operations (profiles/r06_mfma_valu_coissue.txt), and
// the chunk's 120 operations fit the 128 slots of Pb(c) and Pa(c + 1) one by one (m_act_pos below).
// LDS: 128 KB of rings, 16 KB of c_fc's epilogue constants (colsum, bias: loaded once per workgroup), 4 x 4 KB staging for the closing epilogue
// (per wave: 2 KB for the transposed output rows, 2 KB for the residual fragments on their way into the accumulator layout) = 160 KB.
#include "gemm_shared.h"
#include "gemm4_regs.h"

namespace {

struct Gemm4mArgs {
    const void* X;
    void* Y;
    const void* W1;
    const void* W2;
    const float* c1;
    const float* s1;
    const float* stats;
    const float* b2;
    float* ln_part;
    long ln_part_rows;
    int M, ldx, ldy, ldw1, ldw2, a_off, y_off, ntiles;
};

constexpr int M_C = 512, M_HID = 2048, M_NCH = M_HID / 32;
constexpr int M_STG = 32768, M_W2OFF = 2 * M_STG, M_COFF = 4 * M_STG, M_SOFF = M_COFF + M_HID * 4, M_STGOFF = M_SOFF + M_HID * 4;
constexpr int M_LDS = M_STGOFF + 4 * 4096;              // 160 KB

#ifdef MAGE4M_STAMP
// tuning build (tools/probes/gemm4m_probe.hip): wave 0 of each workgroup takes five 100 MHz wall-clock stamps per tile -- 0 tile start, 1 chunk loop done
// (before the last chunk's block 1 and pack), 2 last GEMM 2 done, 3 closing epilogue done, 4 tile end (where the kernel used to request the rest of the next tile's rows
// after the epilogue; nothing lies between 3 and 4 now) -- into scalar registers and writes them at the tile's end: the stores are older than every
// LDS-DMA piece of the next tile, so no counted wait of the chunk loop sees them.  [workgroup][tile of the workgroup][5]
// Stamps 0 and 1 take the shader clock (s_memtime) beside the wall clock: the clock under the chunk loop.  Inside the chunk loop the chunk pairs
// (8, 9) and (32, 33) of every tile are stamped with the shader clock: per phase k = 3 ph + {0 phase start, 1 in front of the mid-phase s_waitcnt,
// 2 behind the s_barrier}, ph = 0 Pa(c), 1 Pb(c), 2 Pa(c + 1), 3 Pb(c + 1); k = 12 is the start of the next chunk's Pa.  The two pairs are copies
// of the loop body of their own (template parameter ST = 0 | 1; ST = -1: no stamps), so the other chunks run the release code: a scalar branch on
// c at every stamp point cost a quarter of the loop's time.  A stamp is requested at its point and stays in a scalar register until the next
// point, where it moves into a lane of ONE vector register (v_writelane: the kernel's scalar registers already spill into such lanes, 30 more
// would go to scratch), so nothing waits for the clock's answer where it is taken.  The low 32 bits are kept (a segment is a few thousand cycles,
// the chunk loop some 250 000): lane 13 ST + k, lanes 26 and 27 for stamps 0 and 1.  [workgroup][tile of the workgroup][32]
constexpr int M_STAMP_WG = 256, M_STAMP_TILES = 16, M_CSTAMP_N = 13, M_CSTAMP_LANES = 32, M_CSTAMP_C0 = 8, M_CSTAMP_C1 = 32;
__device__ unsigned long long m_stamps[M_STAMP_WG * M_STAMP_TILES * 5];
__device__ unsigned m_cstamps[M_STAMP_WG * M_STAMP_TILES * M_CSTAMP_LANES];
#define M_CSTAMP_PUT(lane_) asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(cstamp) : "s"(cpend), "i"(lane_))
#define M_STAMP(k)                                                        \
    do {                                                                  \
        fence();                                                          \
        stamp[k] = __builtin_amdgcn_s_memrealtime();                      \
        if constexpr ((k) < 2) {                                          \
            cpend = (unsigned)__builtin_amdgcn_s_memtime();               \
            M_CSTAMP_PUT(2 * M_CSTAMP_N + (k));                           \
        }                                                                 \
        fence();                                                          \
    } while (0)
#define M_CSTAMP(ST_, k)                                                                      \
    do {                                                                                      \
        if constexpr (decltype(ST_)::value >= 0) {                                            \
            fence();                                                                          \
            if constexpr ((k) > 0) M_CSTAMP_PUT(M_CSTAMP_N * decltype(ST_)::value + (k) - 1); \
            cpend = (unsigned)__builtin_amdgcn_s_memtime();                                   \
            if constexpr ((k) == M_CSTAMP_N - 1) M_CSTAMP_PUT(M_CSTAMP_N * decltype(ST_)::value + (k)); \
            fence();                                                                          \
        }                                                                                     \
    } while (0)
#else
#define M_STAMP(k) \
    do {           \
    } while (0)
#define M_CSTAMP(ST_, k) \
    do {                 \
    } while (0)
#endif

// ---- The chunk epilogue's schedule.  A chunk has 112 activation ops o = 28 G + K -- group G = accumulator block (block t = G >> 1 of the chunk,
// 16-row tile mt = G & 1), K = 4 a + j: row a of the 7 operations (0, 1 the LayerNorm fold, 2 the scaling, 3 exp, 4 (+ 1), 5 rcp, 6 the product) on
// value j of the block's 4 -- and 8 packs I (tile I >> 2, word I & 3).  They are issued one per MFMA slot at POSITIONS 0 .. 127: 0 .. 63 the slots of
// Pb(c), 64 .. 127 the slots of Pa(c + 1).  A row takes one UNIT of 4 slots; odd units are the slots k = 4 .. 7 of an 8-MFMA batch, which hold no
// fragment read, and every exp / rcp row and every pack sits on an odd unit (the plain rows share their slots with the ds_read_b128s):
//     Pb(c)    :  -  a0  a1  b0  a2 [a3] a4 [a5] a6  b1  b2 [b3] b4 [b5] b6  -          a = group 0, b = group 1 (block 0; tiles 0, 1)
//     Pa(c + 1):  c0 c1  c2 [c3] c4 [c5] c6 [P0] d0  d1  d2 [d3] d4 [d5] d6 [P1]        c = group 2, d = group 3 (block 1); P = the 4 packs of a tile
// Tile 0's words are packed as soon as group 2 is through; group 0 starts at slot 4 of Pb(c), 8 MFMAs behind the MFMA that wrote it, as it always has.
constexpr int M_NACT = 112, M_NPACK = 8, M_NPOS = 128;
constexpr int M_ROW_UNIT[4][7] = {{1, 2, 4, 5, 6, 7, 8}, {3, 9, 10, 11, 12, 13, 14}, {16, 17, 18, 19, 20, 21, 22}, {24, 25, 26, 27, 28, 29, 30}};
constexpr int M_PACK_UNIT[2] = {23, 31};
constexpr int M_CRD_SLOT[2] = {45, 47};          // the slots of Pb(c) that read block 1's (column sums, bias) and of Pa(c + 1) that read block 0's of chunk c + 1
constexpr int m_act_pos(int o) { return 4 * M_ROW_UNIT[o / 28][(o % 28) >> 2] + (o & 3); }
constexpr int m_pack_pos(int I) { return 4 * M_PACK_UNIT[I >> 2] + (I & 3); }
constexpr int m_act_at(int p) {                  // the activation op at position p, or -1
    for (int o = 0; o < M_NACT; ++o)
        if (m_act_pos(o) == p) return o;
    return -1;
}
constexpr int m_pack_at(int p) {
    for (int I = 0; I < M_NPACK; ++I)
        if (m_pack_pos(I) == p) return I;
    return -1;
}
constexpr bool m_heavy(int o) { return ((o % 28) >> 2) == 3 || ((o % 28) >> 2) == 5; }          // v_exp_f32, v_rcp_f32: 8 issue cycles; plain VALU 4; v_cvt_pk 8
constexpr int m_slot_cycles(int p) { return (m_act_at(p) >= 0 ? (m_heavy(m_act_at(p)) ? 8 : 4) : 0) + (m_pack_at(p) >= 0 ? 8 : 0); }
constexpr bool m_sched_once() {                  // every op at a position of its own, every position at most 8 issue cycles of vector work
    int n = 0;
    for (int p = 0; p < M_NPOS; ++p) {
        if (m_slot_cycles(p) > 8) return false;
        n += (m_act_at(p) >= 0) + (m_pack_at(p) >= 0);
    }
    for (int o = 0; o < M_NACT; ++o)
        if (m_act_pos(o) < 0 || m_act_pos(o) >= M_NPOS || m_act_at(m_act_pos(o)) != o) return false;
    for (int I = 0; I < M_NPACK; ++I)
        if (m_pack_pos(I) < 0 || m_pack_pos(I) >= M_NPOS || m_pack_at(m_pack_pos(I)) != I) return false;
    return n == M_NACT + M_NPACK;
}
constexpr bool m_sched_order() {                 // producer -> consumer
    for (int G = 0; G < 4; ++G)
        for (int K = 0; K < 28; ++K) {
            const int p = m_act_pos(28 * G + K);
            // GEMM 1's last MFMA into group G is slot 60 + G of Pa(c) = position G - 4: its result is read no sooner than 8 MFMAs later
            if (p - (G - 4) < 8) return false;
            // a value's operations in order; a transcendental's result is read no sooner than 4 instructions later
            if (K >= 4 && p - m_act_pos(28 * G + K - 4) < (m_heavy(28 * G + K - 4) ? 4 : 1)) return false;
            // eu[] is one set of 4 registers (written by row 2, last read by row 6): the groups take it one after the other
            if (G > 0 && K >= 8 && p < m_act_pos(28 * (G - 1) + 27)) return false;
            // sv / cv hold block 0's constants from Pa(c)'s M_CRD_SLOT to Pb(c)'s, where block 1's replace them until Pa(c + 1)'s M_CRD_SLOT
            if (K < 8 && G < 2 && p >= M_CRD_SLOT[0]) return false;
            if (K < 8 && G >= 2 && (p <= M_CRD_SLOT[1] || p >= 64 + M_CRD_SLOT[0])) return false;
        }
    for (int I = 0; I < M_NPACK; ++I) {
        const int mt = I >> 2, w = I & 3, G = 2 * (w >> 1) + mt, p = m_pack_pos(I);
        // a pack reads two finished values of group G; hpk[mt] is GEMM 2's operand from slot mt of Pb(c + 1) = position 128 + mt (an MFMA in
        // between covers the VALU -> MFMA operand wait states) and was Pb(c)'s operand until position 63
        if (p <= m_act_pos(28 * G + 24 + 2 * (w & 1)) || p <= m_act_pos(28 * G + 25 + 2 * (w & 1))) return false;
        if (p < 64 || M_NPOS + mt - p < 2) return false;
    }
    return true;
}
static_assert(m_sched_once(), "gemm4m: every activation op and every pack exactly once per chunk, at most 8 issue cycles of vector work per MFMA slot");
static_assert(m_sched_order(), "gemm4m: a producer -> consumer distance of the chunk epilogue's schedule is broken");

// one LDS-DMA piece: 64 lanes x 16 B from (scalar base + per-lane offset) to LDS lds .. lds + 1023
__device__ __forceinline__ void m_dma(unsigned lds, unsigned voff, const char* base) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(voff), "s"(base) : "memory");
}
// GEMM 1's MFMA: accumulator block in VGPRs (the chunk's 16 registers), W fragment = A-operand, x fragment = B-operand
template <bool ZERO, bool CLOB, bool HF>
__device__ __forceinline__ void m_mfma1(f32x4& acc, const u32x4& w, const u32x4& x) {
#define M_MFMA1(OP)                                                                                              \
    do {                                                                                                         \
        if constexpr (ZERO && CLOB) asm volatile(OP " %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(x) : G4_ALL_ACC); \
        else if constexpr (ZERO) asm volatile(OP " %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(x));                 \
        else if constexpr (CLOB) asm volatile(OP " %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(x) : G4_ALL_ACC);    \
        else asm volatile(OP " %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(x));                                     \
    } while (0)
    if constexpr (HF) M_MFMA1("v_mfma_f32_16x16x32_f16");
    else M_MFMA1("v_mfma_f32_16x16x32_bf16");
#undef M_MFMA1
}
constexpr int m_wait_imm(int vm) { return (((vm >> 4) & 3) << 14) | (vm & 15) | 0x70; }      // vmcnt(vm) lgkmcnt(0)

template <bool HF, bool LNP>
__global__ __launch_bounds__(256) void gemm4m_kernel(const Gemm4mArgs g) {
    typedef std::conditional_t<HF, f16_t, unsigned short> HT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    g4_claim_accumulators();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, grp = lane >> 4;
    const unsigned smem_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

    // ---- loader.  W1 chunk (32 hidden units x 512 k) in LDS: 8 slabs of 64 k, a slab = 32 row slots x 128 B, 16-byte chunk p of slot r at
    // p ^ ((r >> 1) & 7).  A piece = 8 slots of one slab; this wave moves slabs 2 wave, 2 wave + 1.  Slot r = 16 t + rr holds hidden unit
    // 8 (rr / 4) + 4 t + rr % 4 of the chunk.  W2 chunk (512 columns x 32 k): column block nb = 16 rows x 64 B = one piece, 16-byte chunk q of
    // row r at q ^ ((4 - r / 4) & 3): a ds_read_b128's 16-lane groups then touch 16 distinct slots.  This wave moves blocks 8 wave .. 8 wave + 7.
    const int lr = lane >> 3, lp = lane & 7;
    unsigned voffW1[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
        voffW1[h] = (unsigned)((8 * (lr >> 2) + (lr & 3)) * g.ldw1 * 2 + ((lp ^ ((h * 4 + (lr >> 1)) & 7)) << 4));
    const unsigned voffW2 = (unsigned)((lane >> 2) * g.ldw2 * 2 + (((lane & 3) ^ ((4 - (lane >> 4)) & 3)) << 4));
    auto dma_w1 = [&](int stage, int c, int u) __attribute__((always_inline)) {        // piece u (0..7) of chunk c -> stage
        const int sl = 2 * wave + (u >> 2), u4 = u & 3;
        const char* base = (const char*)g.W1 + (long)(32 * c + 16 * (u4 & 1) + 4 * (u4 >> 1)) * g.ldw1 * 2 + sl * 128;
        m_dma(smem_addr + stage * M_STG + sl * 4096 + u4 * 1024, voffW1[u4 & 1], base);
    };
    auto dma_w2 = [&](int stage, int c, int u) __attribute__((always_inline)) {
        const int nb = 8 * wave + u;
        const char* base = (const char*)g.W2 + (long)(nb * 16) * g.ldw2 * 2 + c * 64;
        m_dma(smem_addr + M_W2OFF + stage * M_STG + nb * 1024, voffW2, base);
    };

    // ---- fragment reads
    const int rsw = (l15 >> 1) & 7;
    const int w1_off = l15 * 128, w1_pc[2] = {((grp + 0) ^ rsw) * 16, ((grp + 4) ^ rsw) * 16};
    const int w2_off = M_W2OFF + l15 * 64 + ((grp ^ ((4 - (l15 >> 2)) & 3)) << 4);
    u32x4 wf[2][4];
    auto rd_w1 = [&](int buf, int stage, int b, int j) __attribute__((always_inline)) {      // fragment j of batch b: k-step 2 b + (j >> 1), block t = j & 1
        const int ks = 2 * b + (j >> 1), t = j & 1;
        wf[buf][j] = *(const u32x4*)(smem + stage * M_STG + (ks >> 1) * 4096 + t * 2048 + w1_off + w1_pc[ks & 1]);
    };
    auto rd_w2 = [&](int buf, int stage, int b, int j) __attribute__((always_inline)) {      // column block 4 b + j
        wf[buf][j] = *(const u32x4*)(smem + stage * M_STG + (4 * b + j) * 1024 + w2_off);
    };

    // ---- state
    u32x4 xf[2][16];                   // the wave's 32 x rows as B-operand fragments: [16-row tile][k-step]
    f32x4 hacc[2][2][2];               // [chunk parity][16-row tile][block t]
    u32x4 hpk[2];                      // the packed chunk: GEMM 2's B-operand of each 16-row tile
    f32x4 sv, cv;                      // c_fc's column sums and bias of 4 of the lane's 8 hidden units: block t = 0, then t = 1 of the chunk
    float mean[2], rstd[2];
    const unsigned xoff = (unsigned)((l15 * g.ldx + 8 * grp) * 2);      // per-lane byte offset inside a 16-row tile; the tile's position is scalar
    auto load_x = [&](int tile, int mt0, int mt1) __attribute__((always_inline)) {
#pragma unroll
        for (int mt = mt0; mt < mt1; ++mt) {
            const char* xp = (const char*)g.X + ((long)tile * 128 + wave * 32 + mt * 16 + g.a_off) * g.ldx * 2;
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) xf[mt][ks] = *(const u32x4*)(xp + ks * 64 + xoff);
        }
    };
    auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };
    auto wait_barrier = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_s_waitcnt(m_wait_imm(8));
        ring_barrier();
        fence();
    };
    // The chunk epilogue as single-instruction asm statements (hipcc keeps those where they are written; plain arithmetic sinks to its consumer):
    // gemm4h's operations in gemm4h's order.  Group G (block t = G >> 1, tile mt = G & 1: one accumulator block, 4 values j) has 28 ops K = 4 a + j:
    // a = 0, 1 the LayerNorm fold, 2 the scaling, 3 exp, 4 (+ 1), 5 rcp, 6 the product -- a transcendental's result is read 4 instructions later.
    float eu[4];
#ifdef MAGE4M_STAMP
    unsigned long long stamp[5];
    int cstamp = 0;
    unsigned cpend = 0;
    int stamp_tile = 0;
#endif
    auto act_op = [&](auto PAR_, auto G_, auto K_) __attribute__((always_inline)) {
        constexpr int PAR = decltype(PAR_)::value, G = decltype(G_)::value, K = decltype(K_)::value;
        constexpr int t = G >> 1, mt = G & 1, a = K >> 2, j = K & 3;
        float v = hacc[PAR][mt][t][j];
        if constexpr (a == 0) asm volatile("v_fma_f32 %0, -%1, %2, %0" : "+v"(v) : "v"(mean[mt]), "v"(sv[j]));
        else if constexpr (a == 1) asm volatile("v_fma_f32 %0, %1, %0, %2" : "+v"(v) : "v"(rstd[mt]), "v"(cv[j]));
        else if constexpr (a == 2) asm volatile("v_mul_f32 %0, 0xc01d265f, %1" : "=v"(eu[j]) : "v"(v));        // -1.702 log2(e) x
        else if constexpr (a == 3) asm volatile("v_exp_f32 %0, %0" : "+v"(eu[j]));
        else if constexpr (a == 4) asm volatile("v_add_f32 %0, 1.0, %0" : "+v"(eu[j]));
        else if constexpr (a == 5) asm volatile("v_rcp_f32 %0, %0" : "+v"(eu[j]));
        else asm volatile("v_mul_f32 %0, %0, %1" : "+v"(v) : "v"(eu[j]));
        if constexpr (a < 2 || a == 6) hacc[PAR][mt][t][j] = v;
    };
    auto pack_op = [&](auto PAR_, auto I_) __attribute__((always_inline)) {              // I = 0..7: tile I >> 2, word I & 3
        constexpr int PAR = decltype(PAR_)::value, I = decltype(I_)::value, mt = I >> 2, w = I & 3;
        const float a0 = hacc[PAR][mt][w >> 1][(w & 1) * 2], a1 = hacc[PAR][mt][w >> 1][(w & 1) * 2 + 1];
        unsigned r;
        if constexpr (HF) asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a0), "v"(a1));
        else asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a0), "v"(a1));
        hpk[mt][w] = r;
    };
    auto consts_rd = [&](int c, int t, int i) __attribute__((always_inline)) {           // i = 0: column sums, 1: bias, of block t of chunk c
        const char* p = smem + (i ? M_COFF : M_SOFF) + (32 * c + 8 * grp + 4 * t) * 4;
        if (i) cv = *(const f32x4*)p;
        else sv = *(const f32x4*)p;
    };

    auto sched_ops = [&](auto PAR_, auto P_) __attribute__((always_inline)) {          // the op of position P, on the chunk of parity PAR
        constexpr int o = m_act_at(decltype(P_)::value), I = m_pack_at(decltype(P_)::value);
        if constexpr (o >= 0 || I >= 0) fence();
        if constexpr (o >= 0) act_op(PAR_, std::integral_constant<int, o / 28>{}, std::integral_constant<int, o % 28>{});
        if constexpr (I >= 0) pack_op(PAR_, std::integral_constant<int, I>{});
    };
    // Pa(c): GEMM 1 of chunk c (parity PAR) || positions 64 .. 127 of chunk c - 1: its block 1 and its pack.  ACT = false: the tile's first chunk.
    auto phase_a = [&](auto PAR_, auto ACT_, auto ST_, int c) __attribute__((always_inline)) {
        constexpr int PAR = decltype(PAR_)::value;
        constexpr bool ACT = decltype(ACT_)::value;
        g4_for<64>([&](auto i_) {
            constexpr int i = decltype(i_)::value, b = i >> 3, k = i & 7, j = k >> 1, mt = k & 1, ks = 2 * b + (j >> 1), t = j & 1;
            if constexpr (i == 0) M_CSTAMP(ST_, 6 * PAR);
            m_mfma1<ks == 0, k == 0, HF>(hacc[PAR][mt][t], wf[b & 1][j], xf[mt][ks]);
            fence();
            if constexpr (ACT && (i == M_CRD_SLOT[0] || i == M_CRD_SLOT[1])) consts_rd(c, 0, i == M_CRD_SLOT[1]);      // this chunk's block 0, for Pb(c)
            if constexpr (k < 4 && b < 7) rd_w1((b + 1) & 1, PAR, b + 1, k);
            if constexpr (k < 4 && b == 7 && ACT) rd_w2(0, PAR ^ 1, 0, k);           // GEMM 2 (c - 1): W2 stage of parity PAR ^ 1
            if constexpr (ACT) sched_ops(std::integral_constant<int, PAR ^ 1>{}, std::integral_constant<int, 64 + i>{});
            if constexpr (b >= 4 && (k == 4 || k == 6)) dma_w2(PAR, c, (b - 4) * 2 + (k == 6));
            fence();
            if constexpr (i == 31) {
                M_CSTAMP(ST_, 6 * PAR + 1);
                wait_barrier();
                M_CSTAMP(ST_, 6 * PAR + 2);
            }
        });
    };
    // Pb(c): GEMM 2 of chunk c - 1 (ZERO: the tile's first k-step) || positions 0 .. 63 of chunk c (parity PAR): its block 0
    auto phase_b = [&](auto PAR_, auto ZERO_, auto ST_, int c) __attribute__((always_inline)) {
        constexpr int PAR = decltype(PAR_)::value;
        constexpr bool ZERO = decltype(ZERO_)::value;
        g4_for<64>([&](auto i_) {
            constexpr int i = decltype(i_)::value, b = i >> 3, k = i & 7, j = k >> 1, mt = k & 1, nb = 4 * b + j;
            if constexpr (i == 0) M_CSTAMP(ST_, 6 * PAR + 3);
            g4_mfma<mt * 32 + nb, ZERO, k == 0, HF>(wf[b & 1][j], hpk[mt]);
            fence();
            if constexpr (i == M_CRD_SLOT[0] || i == M_CRD_SLOT[1]) consts_rd(c, 1, i == M_CRD_SLOT[1]);               // block 1's constants, for Pa(c + 1)
            if constexpr (k < 4 && b < 7) rd_w2((b + 1) & 1, PAR ^ 1, b + 1, k);
            if constexpr (k < 4 && b == 7) rd_w1(0, PAR ^ 1, 0, k);                  // GEMM 1 (c + 1)
            sched_ops(PAR_, i_);
            if constexpr (b >= 4 && (k == 4 || k == 6)) dma_w1(PAR, (c + 2) & (M_NCH - 1), (b - 4) * 2 + (k == 6));
            fence();
            if constexpr (i == 31) {
                M_CSTAMP(ST_, 6 * PAR + 4);
                wait_barrier();
                M_CSTAMP(ST_, 6 * PAR + 5);
            }
        });
    };
    auto act_block = [&](auto PAR_, auto T_) __attribute__((always_inline)) {          // block T's two groups with no MFMA beside them (the tile's first and last chunk)
        g4_for<56>([&](auto k_) {
            act_op(PAR_, std::integral_constant<int, 2 * decltype(T_)::value + decltype(k_)::value / 28>{}, std::integral_constant<int, decltype(k_)::value % 28>{});
        });
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, -1> NST;              // a chunk without stamps

    // ---- prologue: c_fc's epilogue constants, W1(0), W1(1); the first tile's rows
    for (int i = tid; i < M_HID / 4; i += 256) {
        ((f32x4*)(smem + M_COFF))[i] = ((const f32x4*)g.c1)[i];
        ((f32x4*)(smem + M_SOFF))[i] = ((const f32x4*)g.s1)[i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) dma_w1(0, 0, u);
#pragma unroll
    for (int u = 0; u < 8; ++u) dma_w1(1, 1, u);
    load_x(blockIdx.x, 0, 2);
    __builtin_amdgcn_s_waitcnt(0x0070);                // vmcnt(0) lgkmcnt(0)
    ring_barrier();
    fence();

    for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        MAGE_DASSERT(tile >= 0 && tile < g.ntiles);
        M_STAMP(0);
        const int m0 = tile * 128 + wave * 32;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float2 st = *(const float2*)((const char*)(g.stats + 2 * (long)(m0 + mt * 16)) + (unsigned)(l15 * 8));
            mean[mt] = st.x;
            rstd[mt] = st.y;
        }
        // ---- chunk 0: GEMM 1 alone, then its block 0 alone; its block 1 runs under GEMM 1 (1) like every other chunk's
        g4_for<4>([&](auto j_) { rd_w1(0, 0, 0, decltype(j_)::value); });
        fence();
        phase_a(I0{}, std::false_type{}, NST{}, 0);
        consts_rd(0, 0, 0);
        consts_rd(0, 0, 1);
        asm volatile("s_nop 15" ::: "memory");         // the last MFMA's result -> VALU
        fence();
        act_block(I0{}, I0{});
        fence();
        consts_rd(0, 1, 0);
        consts_rd(0, 1, 1);
        fence();
        wait_barrier();
#pragma unroll
        for (int u = 0; u < 8; ++u) dma_w1(0, 2, u);
        g4_for<4>([&](auto j_) { rd_w1(0, 1, 0, decltype(j_)::value); });
        fence();
        // ---- chunk 1: its GEMM 2 is the tile's first k-step
        phase_a(I1{}, std::true_type{}, NST{}, 1);
        phase_b(I1{}, std::true_type{}, NST{}, 1);
#ifdef MAGE4M_STAMP
        auto chunk_pair = [&](auto ST_, int c) __attribute__((always_inline)) {
            phase_a(I0{}, std::true_type{}, ST_, c);
            phase_b(I0{}, std::false_type{}, ST_, c);
            phase_a(I1{}, std::true_type{}, ST_, c + 1);
            phase_b(I1{}, std::false_type{}, ST_, c + 1);
            M_CSTAMP(ST_, 12);
        };
        for (int c = 2; c < M_CSTAMP_C0; c += 2) chunk_pair(NST{}, c);
        chunk_pair(I0{}, M_CSTAMP_C0);
        for (int c = M_CSTAMP_C0 + 2; c < M_CSTAMP_C1; c += 2) chunk_pair(NST{}, c);
        chunk_pair(I1{}, M_CSTAMP_C1);
        for (int c = M_CSTAMP_C1 + 2; c < M_NCH; c += 2) chunk_pair(NST{}, c);
#else
        for (int c = 2; c < M_NCH; c += 2) {
            phase_a(I0{}, std::true_type{}, NST{}, c);
            phase_b(I0{}, std::false_type{}, NST{}, c);
            phase_a(I1{}, std::true_type{}, NST{}, c + 1);
            phase_b(I1{}, std::false_type{}, NST{}, c + 1);
        }
#endif
        M_STAMP(1);
        // ---- the last chunk's block 1 (its constants were read in Pb(63)), pack and GEMM 2 (W2 stage 1); the closing epilogue's first bias values
        // are requested under it
        asm volatile("s_nop 15" ::: "memory");
        fence();
        act_block(I1{}, I1{});
        fence();
        g4_for<8>([&](auto i_) { pack_op(I1{}, i_); });
        fence();
        wait_barrier();
        g4_for<4>([&](auto j_) { rd_w2(0, 1, 0, decltype(j_)::value); });
        fence();
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));               // keep the epilogue's lane-derived constants out of the chunk loop's registers
        const int l15_e = lane_e & 15, grp_e = lane_e >> 4;
        f32x4 bnext[4];                                // c_proj's bias of the NEXT slice of the closing epilogue: slice 0's lands under this GEMM 2
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bnext[nt] = *(const f32x4*)(g.b2 + nt * 16 + grp_e * 4);
        fence();
        asm volatile("s_nop 1" ::: "memory");
        g4_for<64>([&](auto i_) {
            constexpr int i = decltype(i_)::value, b = i >> 3, k = i & 7, j = k >> 1, mt = k & 1, nb = 4 * b + j;
            g4_mfma<mt * 32 + nb, false, k == 0, HF>(wf[b & 1][j], hpk[mt]);
            fence();
            if constexpr (k < 4 && b < 7) rd_w2((b + 1) & 1, 1, b + 1, k);
            fence();
        });
        asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
        fence();
        M_STAMP(2);
        // ---- closing epilogue: (acc + b2) + x, the LayerNorm partial sums, whole-row stores, 64-column slice by slice: epilogue_lean's two-tile
        // form (16-bit rows, residual in the epilogue, LN_PRODUCE) operation for operation, except where the residual comes from: the slice's
        // x values are the wave's own fragments xf[mt][2 sl], xf[mt][2 sl + 1] (lane (l15, grp): row l15, columns 32 ks + 8 grp .. + 7), written
        // to the upper half of the staging window where epilogue_lean lands the rows it loads (row r, 16-byte chunk c at c ^ ((r >> 1) & 7)) and
        // read back in the accumulator layout.  Nothing in a slice waits for memory that was requested in it: once a slice's fragments are
        // staged their registers take the NEXT tile's (GEMM 1 walks k upward, so the youngest are needed last), and the next slice's bias is
        // requested before this slice's rows are stored, so the counted wait at its use leaves the stores in flight.  NEXT = false (the
        // workgroup's last tile): no rows are requested.  A template parameter, not a branch around the loads: the compiler's wait counts stay exact.
        auto close_tile = [&](auto NEXT_) __attribute__((always_inline)) {
            constexpr bool NEXT = decltype(NEXT_)::value;
            char* stg = smem + M_STGOFF + wave * 4096;
            const int rr = lane_e >> 3, cc = lane_e & 7, rsw_e = (l15_e >> 1) & 7;
            int woff[4], roff[2], xwoff[2];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) woff[nt] = l15_e * 128 + (((nt * 2 + (grp_e >> 1)) ^ rsw_e) << 4) + (grp_e & 1) * 8;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = rr + 8 * i;
                roff[i] = r * 128 + ((cc ^ ((r >> 1) & 7)) << 4);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) xwoff[h] = 2048 + l15_e * 128 + (((4 * h + grp_e) ^ rsw_e) << 4);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) MAGE_DASSERT(woff[nt] >= 0 && woff[nt] + 8 <= 2048);
#pragma unroll
            for (int i = 0; i < 2; ++i) MAGE_DASSERT(roff[i] >= 0 && roff[i] + 16 <= 2048 && xwoff[i] >= 2048 && xwoff[i] + 16 <= 4096);
            HT* const yrow = (HT*)g.Y + ((long)(m0 + rr) + g.y_off) * g.ldy + cc * 8;           // row m0 + rr of the tile, the lane's 8 columns of slice 0
            const long step = 8L * g.ldy;
            [[maybe_unused]] float* const prow = g.ln_part + ((long)(m0 + l15_e) + g.y_off) * 2;
            [[maybe_unused]] const char* xnext[2];
            if constexpr (NEXT) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    xnext[mt] = (const char*)g.X + ((long)(tile + (int)gridDim.x) * 128 + wave * 32 + mt * 16 + g.a_off) * g.ldx * 2;
            }
            g4_for<8>([&](auto sl_) {
                constexpr int sl = decltype(sl_)::value;
                f32x4 biasm[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) biasm[nt] = bnext[nt];
                auto stage = [&](auto mt_, u32x4(&o)[2]) __attribute__((always_inline)) {      // math + transpose of 16-row tile mt: results land in o[] (row-contiguous)
                    constexpr int mt = decltype(mt_)::value;
                    [[maybe_unused]] float s1 = 0.f, s2 = 0.f;
                    uint2 auxb[4];
                    f32x4 acc[4];                          // the tile's 16 accumulator registers of this slice, read when it is staged (16 VGPRs, not 32)
                    g4_for<4>([&](auto nt_) {
                        constexpr int nt = decltype(nt_)::value;
                        acc[nt] = g4_acc_read<mt * 32 + 4 * sl + nt, mt == 0 && nt == 0>();
                    });
#pragma unroll
                    for (int h = 0; h < 2; ++h) *(u32x4*)(stg + xwoff[h]) = xf[mt][2 * sl + h];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) auxb[nt] = *(const uint2*)(stg + 2048 + woff[nt]);
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        f32x4 v;
                        v = acc[nt] + biasm[nt];
                        v = v + widen4<HT>(auxb[nt]);
                        if constexpr (LNP) {
                            s1 += (v[0] + v[1]) + (v[2] + v[3]);
                            s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                        }
                        *(uint2*)(stg + woff[nt]) = uint2{pack16x2<HT>(v[0], v[1]), pack16x2<HT>(v[2], v[3])};
                    }
                    if constexpr (LNP) {
                        // the four lane groups hold four 16-column pieces of row l15: fixed-order sum, written by group 0
                        s1 += __shfl_xor(s1, 16);
                        s2 += __shfl_xor(s2, 16);
                        s1 += __shfl_xor(s1, 32);
                        s2 += __shfl_xor(s2, 32);
                        if (grp_e == 0) *(float2*)(prow + ((long)sl * g.ln_part_rows + mt * 16) * 2) = float2{s1, s2};      // slice-major
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) o[i] = *(const u32x4*)(stg + roff[i]);
                };
                u32x4 o[2][2];
                stage(I0{}, o[0]);
                stage(I1{}, o[1]);
                fence();
                if constexpr (sl < 7) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bnext[nt] = *(const f32x4*)(g.b2 + (sl + 1) * 64 + nt * 16 + grp_e * 4);
                }
                if constexpr (NEXT) {
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int h = 0; h < 2; ++h) xf[mt][2 * sl + h] = *(const u32x4*)(xnext[mt] + (2 * sl + h) * 64 + xoff);
                }
                fence();
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int i = 0; i < 2; ++i)      // streaming stores, as epilogue_lean's: the rows are not read again by this launch
                        __builtin_nontemporal_store(o[mt][i], (u32x4*)(yrow + sl * 64 + (2 * mt + i) * step));
                fence();
            });
        };
        if (tile + (int)gridDim.x < g.ntiles) close_tile(std::true_type{});
        else close_tile(std::false_type{});
        fence();
        M_STAMP(3);
        M_STAMP(4);
#ifdef MAGE4M_STAMP
        if (tid == 0 && blockIdx.x < M_STAMP_WG && stamp_tile < M_STAMP_TILES) {
#pragma unroll
            for (int k = 0; k < 5; ++k) m_stamps[((int)blockIdx.x * M_STAMP_TILES + stamp_tile) * 5 + k] = stamp[k];
        }
        if (tid < M_CSTAMP_LANES && blockIdx.x < M_STAMP_WG && stamp_tile < M_STAMP_TILES) {
            MAGE_DASSERT(((int)blockIdx.x * M_STAMP_TILES + stamp_tile) * M_CSTAMP_LANES + tid < M_STAMP_WG * M_STAMP_TILES * M_CSTAMP_LANES);
            m_cstamps[((int)blockIdx.x * M_STAMP_TILES + stamp_tile) * M_CSTAMP_LANES + tid] = (unsigned)cstamp;
        }
        ++stamp_tile;
        fence();
#endif
    }
    __builtin_amdgcn_s_waitcnt(0x0070);                // the W1 pieces requested past the last tile land before the LDS is released
}

template <bool HF, bool LNP>
int launch4m(const Gemm4mArgs& a, hipStream_t s, int n_cu) {
    const int grid = a.ntiles >= n_cu ? n_cu : a.ntiles;
    return mage_gemm_launch<gemm4m_kernel<HF, LNP>>(grid, 256, M_LDS, s, a);
}

}  // namespace

extern "C" int mage_mlp_fused(int32_t dtype, int32_t w_dtype, int32_t y_dtype, int64_t M, int32_t C, const void* x, int64_t ldx, int64_t a_off, void* y, int64_t ldy, int64_t y_off,
                              const void* w1, int64_t ldw1, const float* c1, const float* s1, const float* ln_stats, const void* w2, int64_t ldw2,
                              const float* b2, float* ln_part, int64_t ln_part_rows, void* stream) {
    MAGE_CHECK_ARG(dtype == MAGE_BF16 || dtype == MAGE_F16, "mage_mlp_fused: bf16 or f16 rows and weights (dtype %d)", (int)dtype);
    MAGE_CHECK_ARG(w_dtype == dtype && y_dtype == dtype, "mage_mlp_fused: weights (dtype %d) and output rows (dtype %d) must have the type of x (%d)",
                   (int)w_dtype, (int)y_dtype, (int)dtype);
    MAGE_CHECK_ARG(C == M_C, "mage_mlp_fused: C=%d: the kernel is built for C = 512 (hidden = 2048)", (int)C);
    MAGE_CHECK_ARG(M > 0 && M % 128 == 0, "mage_mlp_fused: M=%ld must be a positive multiple of 128 (whole row tiles)", (long)M);
    MAGE_CHECK_ARG(x && y && w1 && c1 && s1 && ln_stats && w2 && b2, "mage_mlp_fused: x, y, w1, c1, s1, ln_stats, w2, b2 must be given");
    MAGE_CHECK_ARG(ldx >= C && ldy >= C && ldx % 8 == 0 && ldy % 8 == 0, "mage_mlp_fused: ldx=%ld, ldy=%ld must be multiples of 8 and >= C", (long)ldx,
                   (long)ldy);
    MAGE_CHECK_ARG(ldw1 >= C && ldw2 >= 4 * C && ldw1 % 8 == 0 && ldw2 % 8 == 0, "mage_mlp_fused: ldw1=%ld >= C, ldw2=%ld >= 4C, multiples of 8",
                   (long)ldw1, (long)ldw2);
    MAGE_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)c1 | (uintptr_t)s1 | (uintptr_t)b2) & 15) == 0 &&
                       (((uintptr_t)ln_stats | (uintptr_t)ln_part) & 7) == 0,
                   "mage_mlp_fused: rows, weights and vectors must be 16-byte aligned, ln_stats and ln_part 8-byte aligned");
    MAGE_CHECK_ARG(a_off >= 0 && y_off >= 0 && (x != y || a_off == y_off), "mage_mlp_fused: row offsets a_off=%ld, y_off=%ld (equal when in place)",
                   (long)a_off, (long)y_off);
    MAGE_CHECK_ARG(!ln_part || ln_part_rows >= M + y_off, "mage_mlp_fused: ln_part_rows=%ld must cover the output rows", (long)ln_part_rows);
    MAGE_CHECK_ARG((M + a_off) * ldx < (1L << 31) && (M + y_off) * ldy < (1L << 31) && 2048 * ldw1 * 2 < (1L << 31) && 512 * ldw2 * 2 < (1L << 31),
                   "mage_mlp_fused: operands beyond the kernel's 32-bit row arithmetic");
    Gemm4mArgs a;
    a.X = x;
    a.Y = y;
    a.W1 = w1;
    a.W2 = w2;
    a.c1 = c1;
    a.s1 = s1;
    a.stats = ln_stats;
    a.b2 = b2;
    a.ln_part = ln_part;
    a.ln_part_rows = ln_part_rows;
    a.M = (int)M;
    a.ldx = (int)ldx;
    a.ldy = (int)ldy;
    a.ldw1 = (int)ldw1;
    a.ldw2 = (int)ldw2;
    a.a_off = (int)a_off;
    a.y_off = (int)y_off;
    a.ntiles = (int)(M / 128);
    hipStream_t s = (hipStream_t)stream;
    const int n_cu = mage_gemm_cu_count();
    const bool hf = dtype == MAGE_F16;
    if (ln_part) return hf ? launch4m<true, true>(a, s, n_cu) : launch4m<false, true>(a, s, n_cu);
    return hf ? launch4m<true, false>(a, s, n_cu) : launch4m<false, false>(a, s, n_cu);
}

extern "C" int mage_mlp_fused_kernel_name(int32_t dtype, int32_t w_dtype, int32_t y_dtype, int64_t M, int32_t C, const void* x, int64_t ldx, int64_t a_off, void* y, int64_t ldy,
                                          int64_t y_off, const void* w1, int64_t ldw1, const float* c1, const float* s1, const float* ln_stats,
                                          const void* w2, int64_t ldw2, const float* b2, float* ln_part, int64_t ln_part_rows, char* buf, int32_t len) {
    MAGE_CHECK_ARG(buf != nullptr && len > 0, "mage_mlp_fused_kernel_name: no buffer");
    const void* kernel = nullptr;
    mage_gemm_plan = &kernel;
    const int r = mage_mlp_fused(dtype, w_dtype, y_dtype, M, C, x, ldx, a_off, y, ldy, y_off, w1, ldw1, c1, s1, ln_stats, w2, ldw2, b2, ln_part, ln_part_rows, nullptr);
    mage_gemm_plan = nullptr;
    if (r != MAGE_OK) return r;
    return mage_kernel_symbol_name(kernel, buf, len, "mage_mlp_fused_kernel_name");
}
