// Stamp probe of the fused decoder MLP launch (mage_amd/csrc/gemm4m.hip; this file compiles its own copy, so -DMAGE4M_STAMP and other tuning flags
// work) against the library's mage_mlp_fused: bitwise comparison of the output rows and of ln_part, HIP-event times of both, and -- with
// -DMAGE4M_STAMP -- where a tile's time goes: wave 0 of every workgroup stamps the 100 MHz wall clock at five points of each tile, and the shader
// clock at the phase starts, in front of the mid-phase waits and behind the barriers of the chunk pairs (8, 9) and (32, 33): per phase kind
// (Pa / Pb) the first half, the wait + barrier and the second half in shader cycles, and the clock under the chunk loop (shader / wall clock).
// build (from the repo root; the library must be built first):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DMAGE4M_STAMP tools/probes/gemm4m_probe.hip -Lmage_amd/lib -lmage_hip -Wl,-rpath,'$ORIGIN/../../mage_amd/lib' -o tools/probes/gemm4m_probe.bin
// run:  timeout -k 10 300 tools/probes/gemm4m_probe.bin [rounds = 5] [M = 262144]
#define mage_mlp_fused mage_mlp_fused_probe      // this file's own copy of the kernel, beside the library's
#define mage_mlp_fused_kernel_name mage_mlp_fused_kernel_name_probe
#include "../../mage_amd/csrc/gemm4m.hip"
#undef mage_mlp_fused
#undef mage_mlp_fused_kernel_name
#include <algorithm>
#include <cstring>
#include <vector>

extern "C" int mage_mlp_fused(int32_t dtype, int32_t w_dtype, int32_t y_dtype, int64_t M, int32_t C, const void* x, int64_t ldx, int64_t a_off, void* y, int64_t ldy, int64_t y_off,
                              const void* w1, int64_t ldw1, const float* c1, const float* s1, const float* ln_stats, const void* w2, int64_t ldw2,
                              const float* b2, float* ln_part, int64_t ln_part_rows, void* stream);

typedef int (*mlp_fn)(int32_t, int32_t, int32_t, int64_t, int32_t, const void*, int64_t, int64_t, void*, int64_t, int64_t, const void*, int64_t, const float*, const float*,
                      const float*, const void*, int64_t, const float*, float*, int64_t, void*);

static unsigned short f2bf(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static float bf2f(unsigned short b) {
    const unsigned u = (unsigned)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static float frand(unsigned& s) {
    s = s * 1664525u + 1013904223u;
    return ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
}
#define HIP_OK(call)                                                                         \
    do {                                                                                     \
        const hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                              \
            printf("%s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);            \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

static size_t count_diffs(const void* d0, const void* d1, size_t bytes, const char* what, int row_bytes) {
    std::vector<unsigned char> h0(bytes), h1(bytes);
    if (hipMemcpy(h0.data(), d0, bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h1.data(), d1, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        printf("%s: copy back failed\n", what);
        return (size_t)-1;
    }
    size_t nd = 0, first = 0;
    for (size_t i = 0; i < bytes; i += 2)
        if (h0[i] != h1[i] || h0[i + 1] != h1[i + 1]) {
            if (!nd) first = i;
            ++nd;
        }
    printf("    %-8s bitwise diffs vs the library's launch: %zu of %zu 16-bit words", what, nd, bytes / 2);
    if (nd) printf(" (first at row %zu, byte %zu of the row)", first / row_bytes, first % row_bytes);
    printf("\n");
    return nd;
}

#ifdef MAGE4M_STAMP
struct Dist { double med, p10, p90, lo, hi; };
static Dist dist(std::vector<double>& v) {
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return Dist{v[n / 2], v[n / 10], v[n * 9 / 10], v[0], v[n - 1]};
}
static int stamp_table(int grid, int tiles_per_wg_max, int ntiles) {
    std::vector<unsigned long long> st((size_t)M_STAMP_WG * M_STAMP_TILES * 5);
    std::vector<unsigned> cs((size_t)M_STAMP_WG * M_STAMP_TILES * M_CSTAMP_LANES);
    if (hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(m_stamps), st.size() * 8) != hipSuccess ||
        hipMemcpyFromSymbol(cs.data(), HIP_SYMBOL(m_cstamps), cs.size() * 4) != hipSuccess) {
        printf("stamps: copy back failed\n");
        return 1;
    }
    const char* names[6] = {"chunk loop (64 chunks)", "last pack + GEMM 2", "closing epilogue", "trailing row loads issued", "hand-over to next tile", "whole tile (start to start)"};
    std::vector<double> seg[6], share, ghz, ph[2][3], chunk;          // ph[0 Pa | 1 Pb][0 first half | 1 wait + barrier | 2 second half], shader cycles
    for (int wg = 0; wg < grid && wg < M_STAMP_WG; ++wg) {
        const int n_my = (ntiles - wg + grid - 1) / grid;
        for (int t = 0; t < n_my && t < M_STAMP_TILES; ++t) {
            const unsigned long long* s = &st[((size_t)wg * M_STAMP_TILES + t) * 5];
            const unsigned* cl = &cs[((size_t)wg * M_STAMP_TILES + t) * M_CSTAMP_LANES];
            for (int k = 0; k < 4; ++k) seg[k].push_back((double)(s[k + 1] - s[k]) * 10.0);
            ghz.push_back((double)(unsigned)(cl[2 * M_CSTAMP_N + 1] - cl[2 * M_CSTAMP_N]) / ((double)(s[1] - s[0]) * 10.0));
            for (int p = 0; p < 2; ++p) {
                const unsigned* c = cl + p * M_CSTAMP_N;
                for (int q = 0; q < 4; ++q)                      // phases Pa(c), Pb(c), Pa(c + 1), Pb(c + 1); unsigned differences survive a wrap of the low word
                    for (int h = 0; h < 3; ++h) ph[q & 1][h].push_back((double)(unsigned)(c[3 * q + h + 1] - c[3 * q + h]));
                for (int q = 0; q < 2; ++q) chunk.push_back((double)(unsigned)(c[6 * q + 6] - c[6 * q]));
            }
            if (t + 1 < n_my && t + 1 < M_STAMP_TILES) {
                seg[4].push_back((double)(s[5] - s[4]) * 10.0);
                seg[5].push_back((double)(s[5] - s[0]) * 10.0);
                share.push_back((double)(s[3] - s[2]) / (double)(s[5] - s[0]));
            }
        }
    }
    if (seg[5].empty()) {
        printf("    stamps: no workgroup ran two tiles\n");
        return 0;
    }
    const double tile = dist(seg[5]).med;
    printf("    stamps of wave 0, %zu tiles of %d workgroups (up to %d tiles each), ns (100 MHz clock: 10 ns steps)\n", seg[0].size(), grid, tiles_per_wg_max);
    printf("    %-30s %9s %9s %9s %9s %9s %8s\n", "segment", "median", "p10", "p90", "min", "max", "of tile");
    for (int k = 0; k < 6; ++k) {
        const Dist d = dist(seg[k]);
        printf("    %-30s %9.0f %9.0f %9.0f %9.0f %9.0f %7.2f%%\n", names[k], d.med, d.p10, d.p90, d.lo, d.hi, 100.0 * d.med / tile);
    }
    const Dist ds = dist(share);
    printf("    closing epilogue / whole tile, per tile: median %.2f%% (p10 %.2f%%, p90 %.2f%%)\n", 100 * ds.med, 100 * ds.p10, 100 * ds.p90);
    const Dist dg = dist(ghz);
    printf("    clock under the chunk loop (shader clock / wall clock, per tile): median %.3f GHz (p10 %.3f, p90 %.3f)\n", dg.med, dg.p10, dg.p90);
    printf("    chunks %d, %d, %d, %d of every tile, shader cycles (a phase = 64 MFMAs; 64 x 16.63 = 1064)\n", M_CSTAMP_C0, M_CSTAMP_C0 + 1, M_CSTAMP_C1, M_CSTAMP_C1 + 1);
    printf("    %-30s %9s %9s %9s\n", "segment", "median", "p10", "p90");
    const char* pn[2] = {"Pa", "Pb"};
    const char* hn[3] = {"first half (32 MFMAs)", "wait + barrier", "second half (32 MFMAs)"};
    double med[2][3];
    for (int q = 0; q < 2; ++q)
        for (int h = 0; h < 3; ++h) {
            const Dist d = dist(ph[q][h]);
            med[q][h] = d.med;
            char nm[64];
            snprintf(nm, sizeof nm, "%s %s", pn[q], hn[h]);
            printf("    %-30s %9.0f %9.0f %9.0f\n", nm, d.med, d.p10, d.p90);
        }
    const Dist dc = dist(chunk);
    printf("    %-30s %9.0f %9.0f %9.0f   = %.2f cycles per MFMA\n", "chunk (Pa + Pb)", dc.med, dc.p10, dc.p90, dc.med / 128);
    const double ideal = 128 * 16.63, over = med[0][0] + med[0][1] + med[0][2] + med[1][0] + med[1][1] + med[1][2] - ideal;
    printf("    overhead above 128 x 16.63 = %.0f cycles (sum of the medians): %.0f -- Pa halves %.0f (%.0f%%), Pb halves %.0f (%.0f%%), waits + barriers %.0f (%.0f%%)\n", ideal,
           over, med[0][0] + med[0][2] - ideal / 2, 100 * (med[0][0] + med[0][2] - ideal / 2) / over, med[1][0] + med[1][2] - ideal / 2,
           100 * (med[1][0] + med[1][2] - ideal / 2) / over, med[0][1] + med[1][1], 100 * (med[0][1] + med[1][1]) / over);
    return 0;
}
#endif

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 5;
    const int M = argc > 2 ? atoi(argv[2]) : 262144;
    if (M <= 0 || M % 128 != 0) { printf("M must be a positive multiple of 128\n"); return 1; }
    if (mage_init(0) != MAGE_OK) { printf("mage_init: %s\n", mage_last_error()); return 1; }
    const int C = M_C, H = M_HID;
    std::vector<unsigned short> hx((size_t)M * C), hw1((size_t)H * C), hw2((size_t)C * H);
    std::vector<float> hc1(H), hs1(H), hb2(C), hst((size_t)M * 2);
    unsigned seed = 20231u + M;
    for (auto& v : hx) v = f2bf(frand(seed));
    for (auto& v : hw1) v = f2bf(frand(seed) * 1.7f / sqrtf((float)C));
    for (auto& v : hw2) v = f2bf(frand(seed) * 1.7f / sqrtf((float)H));
    for (auto& v : hc1) v = frand(seed) * 0.1f;
    for (auto& v : hb2) v = frand(seed) * 0.1f;
    for (int n = 0; n < H; ++n) {
        double s = 0;
        for (int k = 0; k < C; ++k) s += bf2f(hw1[(size_t)n * C + k]);
        hs1[n] = (float)s;
    }
    for (int m = 0; m < M; ++m) {
        double s = 0, q = 0;
        for (int k = 0; k < C; ++k) {
            const double v = bf2f(hx[(size_t)m * C + k]);
            s += v;
            q += v * v;
        }
        const double mean = s / C, var = q / C - mean * mean;
        hst[2 * (size_t)m] = (float)mean;
        hst[2 * (size_t)m + 1] = (float)(1.0 / sqrt(var + 1e-5));
    }
    const size_t xb = (size_t)M * C * 2, pb = (size_t)(C / 64) * M * 8;
    void *Xm, *X0, *X1, *W1, *W2;
    float *c1, *s1, *b2, *stt, *P0, *P1;
    HIP_OK(hipMalloc(&Xm, xb)); HIP_OK(hipMalloc(&X0, xb)); HIP_OK(hipMalloc(&X1, xb));
    HIP_OK(hipMalloc(&W1, hw1.size() * 2)); HIP_OK(hipMalloc(&W2, hw2.size() * 2));
    HIP_OK(hipMalloc((void**)&c1, H * 4)); HIP_OK(hipMalloc((void**)&s1, H * 4)); HIP_OK(hipMalloc((void**)&b2, C * 4));
    HIP_OK(hipMalloc((void**)&stt, (size_t)M * 8)); HIP_OK(hipMalloc((void**)&P0, pb)); HIP_OK(hipMalloc((void**)&P1, pb));
    HIP_OK(hipMemcpy(Xm, hx.data(), xb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(W1, hw1.data(), hw1.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(W2, hw2.data(), hw2.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(c1, hc1.data(), H * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(s1, hs1.data(), H * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b2, hb2.data(), C * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(stt, hst.data(), (size_t)M * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    const int n_cu = mage_gemm_cu_count(), ntiles = M / 128, grid = ntiles >= n_cu ? n_cu : ntiles;
    printf("gemm4m probe: M = %d (%d tiles of 128 rows, %d workgroups), bf16, %d timing rounds\n", M, ntiles, grid, rounds);
    int bad = 0;
    // form 0: in place with ln_part (a block's MLP; kernel <false, true>); form 1: separate output without ln_part (the last block's; <false, false>)
    for (int form = 0; form < 2; ++form) {
        const bool lnp = form == 0;
        printf("%s\n", lnp ? "LNP = true: in place, ln_part written" : "LNP = false: separate output rows, no ln_part");
        auto run = [&](mlp_fn f, void* xin, void* yout, float* part) {
            return f(MAGE_BF16, MAGE_BF16, MAGE_BF16, M, C, xin, C, 0, yout, C, 0, W1, C, c1, s1, stt, W2, H, b2, lnp ? part : nullptr, lnp ? M : 0, nullptr);
        };
        // in place: each launch starts from a fresh copy of the rows; separate output: x = the master rows, y = X0 / X1
        auto launch = [&](mlp_fn f, void* buf, float* part) {
            if (lnp) {
                if (hipMemcpyAsync(buf, Xm, xb, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) return -100;
                return run(f, buf, buf, part);
            }
            return run(f, Xm, buf, part);
        };
        HIP_OK(hipMemset(X0, 0xff, xb)); HIP_OK(hipMemset(X1, 0xee, xb)); HIP_OK(hipMemset(P0, 0xff, pb)); HIP_OK(hipMemset(P1, 0xee, pb));
        if (launch(mage_mlp_fused, X0, P0) != MAGE_OK) { printf("mage_mlp_fused: %s\n", mage_last_error()); return 1; }
        if (launch(mage_mlp_fused_probe, X1, P1) != MAGE_OK) { printf("probe copy: %s\n", mage_last_error()); return 1; }
        HIP_OK(hipDeviceSynchronize());
        size_t nd = count_diffs(X0, X1, xb, "rows", C * 2);
        if (lnp) nd += count_diffs(P0, P1, pb, "ln_part", M * 8);
        if (nd) ++bad;
        double tl = 0, tp = 0, tlmin = 1e30, tpmin = 1e30, tlmax = 0, tpmax = 0;
        for (int rd = 0; rd < rounds; ++rd) {
            for (int which = 0; which < 2; ++which) {
                void* buf = which ? X1 : X0;
                if (lnp) HIP_OK(hipMemcpyAsync(buf, Xm, xb, hipMemcpyDeviceToDevice, nullptr));
                HIP_OK(hipEventRecord(e0));
                const int r = lnp ? run(which ? mage_mlp_fused_probe : mage_mlp_fused, buf, buf, which ? P1 : P0)
                                  : run(which ? mage_mlp_fused_probe : mage_mlp_fused, Xm, buf, nullptr);
                if (r != MAGE_OK) { printf("launch: %s\n", mage_last_error()); return 1; }
                HIP_OK(hipEventRecord(e1));
                HIP_OK(hipEventSynchronize(e1));
                float ms;
                HIP_OK(hipEventElapsedTime(&ms, e0, e1));
                double &t = which ? tp : tl, &mn = which ? tpmin : tlmin, &mx = which ? tpmax : tlmax;
                t += ms;
                mn = std::min(mn, (double)ms);
                mx = std::max(mx, (double)ms);
            }
        }
        printf("    HIP events, us per launch: library %.1f (min %.1f, max %.1f) | this file's copy%s %.1f (min %.1f, max %.1f)\n", tl / rounds * 1e3, tlmin * 1e3,
               tlmax * 1e3,
#ifdef MAGE4M_STAMP
               " (stamped)",
#else
               "",
#endif
               tp / rounds * 1e3, tpmin * 1e3, tpmax * 1e3);
#ifdef MAGE4M_STAMP
        if (stamp_table(grid, (ntiles + grid - 1) / grid, ntiles)) return 1;     // the stamps of the last timed launch
#endif
    }
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 2 : 0;
}
