// Per-frame video metrics (mage_video_metrics: MSE, PSNR, SSIM) and group-relative advantages (mage_group_advantages, per frame:
// mage_frame_advantages): the reward side of MAGE.rollout.  include/mage_hip_ext.h states the rules; no site in the reference (it reports no metric and trains on cross-entropy only).
#include "common.h"
#include "../../include/mage_hip_ext.h"
#include <math.h>

// Every product and sum below is written out: a contracted a*a + b*b would round one square and not the other, and metrics(x, y) would leave
// metrics(y, x).  The window sums call fma() themselves.
#pragma clang fp contract(off)

namespace {

// One workgroup per frame; it walks the frame's channels and tiles in a fixed order, so a frame's bits depend on its own pixels only.
// A tile is up to TH x TW window positions ("valid" region) and the (TH + 10) x (TW + 10) pixels under them:
//   A  both sides' pixels come from HBM once, into registers while the tile before is still being computed, then into LDS (fp32); the
//      thread that holds a pixel its tile owns adds (x - y)^2 to its fp64 sum;
//   B  row pass: a thread takes one row and 6 adjacent window columns, slides 16 pixels through registers and leaves the five horizontal
//      moments (x, y, x^2, y^2, xy; fp64: a product of two fp32 values is exact) in LDS, column-major;
//   C  column pass: a thread takes one column and 4 adjacent window rows, reads 14 row sums per moment and adds the 4 SSIM values.
// Lanes run along rows in B (pitch 41 floats) and along columns in C (pitch 39 doubles): both odd, no bank conflicts.
constexpr int SS_WIN = 11, SS_HALO = SS_WIN - 1, SS_TW = 30, SS_TH = 28;
constexpr int SS_XP = SS_TW + SS_HALO + 1;          // 41: floats per pixel row in LDS
constexpr int SS_IH = SS_TH + SS_HALO;              // 38: pixel rows per tile
constexpr int SS_RP = SS_IH + 1;                    // 39: doubles per column of row sums
constexpr int SS_GB = 6, SS_GC = 4;                 // window positions per thread in B / in C
constexpr int SS_LD = (SS_IH * (SS_TW + SS_HALO) + 255) / 256;      // 6: pixels of a tile per thread and side
static_assert(SS_TW % SS_GB == 0 && SS_TH % SS_GC == 0 && SS_IH * (SS_TW / SS_GB) <= 256 && 32 * (SS_TH / SS_GC) <= 256 && SS_TW <= 32, "thread maps");

// the window is symmetric: its first six weights, w(t) for tap t (half the scalar registers of all eleven)
struct SsimWindow {
    double g[SS_WIN / 2 + 1];
    __host__ __device__ double w(int t) const { return g[t <= SS_HALO / 2 ? t : SS_HALO - t]; }
};

struct SsimTile {
    int in_h, in_w, own_h, own_w, oh, ow;
    long base;                                      // of the tile's first pixel in the frame
};

__global__ __launch_bounds__(256) void video_metrics_kernel(const float* __restrict__ video, long v_stride, const float* __restrict__ target,
                                                            long t_stride, int T, int C, int H, int W, long tgt_div, int tiles_y, int tiles_x,
                                                            int th, int tw, SsimWindow win, double c1, double c2, double range2,
                                                            float* __restrict__ mse, float* __restrict__ psnr, float* __restrict__ ssim) {
    __shared__ float xs[SS_IH * SS_XP], ys[SS_IH * SS_XP];
    __shared__ double rows[5][SS_TW][SS_RP];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long frame = blockIdx.x, clip = frame / T, chw = (long)C * H * W;
    const int t = (int)(frame - clip * T);
    const float* x = video + clip * v_stride + t * chw;
    const float* y = target + (clip / tgt_div) * t_stride + t * chw;
    const int Ho = H - SS_HALO, Wo = W - SS_HALO, n_tiles = C * tiles_y * tiles_x;
    const bool want_ssim = ssim != nullptr;
    auto tile = [&](int q) {
        const int c = q / (tiles_y * tiles_x), ty = (q - c * tiles_y * tiles_x) / tiles_x, tx = q - (c * tiles_y + ty) * tiles_x;
        const int y0 = ty * th, x0 = tx * tw;
        SsimTile g;
        g.in_h = min(H - y0, th + SS_HALO);
        g.in_w = min(W - x0, tw + SS_HALO);
        g.own_h = ty == tiles_y - 1 ? g.in_h : th;                                  // the last tile of an axis owns its halo
        g.own_w = tx == tiles_x - 1 ? g.in_w : tw;
        g.oh = min(th, Ho - y0);
        g.ow = min(tw, Wo - x0);
        g.base = ((long)c * H + y0) * W + x0;
        return g;
    };
    // pixel u of this thread in a tile: number tid + 256 u of its in_h x in_w pixels, row-major (walked without a division per pixel)
    float pa[SS_LD], pb[SS_LD];
    auto fetch = [&](const SsimTile& g) {
        int r = tid / g.in_w, cc = tid - r * g.in_w;
        const int dr = 256 / g.in_w, dc = 256 - dr * g.in_w;
#pragma unroll
        for (int u = 0; u < SS_LD; ++u) {
            const long at = g.base + (long)min(r, g.in_h - 1) * W + cc;     // (past the tile: a pixel of its last row again, unused -- every
            pa[u] = x[at];                                                  // load unconditional, so all of them are in flight together)
            pb[u] = y[at];
            r += dr;
            cc += dc;
            if (cc >= g.in_w) {
                cc -= g.in_w;
                ++r;
            }
        }
    };
    double sse = 0.0, ssum = 0.0;
    fetch(tile(0));
    for (int q = 0; q < n_tiles; ++q) {
        const SsimTile g = tile(q);
        {                                                                                                    // A
            int r = tid / g.in_w, cc = tid - r * g.in_w;
            const int dr = 256 / g.in_w, dc = 256 - dr * g.in_w;
#pragma unroll
            for (int u = 0; u < SS_LD; ++u) {
                if (r < g.in_h) {
                    if (want_ssim) {
                        xs[r * SS_XP + cc] = pa[u];
                        ys[r * SS_XP + cc] = pb[u];
                    }
                    if (r < g.own_h && cc < g.own_w) {
                        const double d = (double)pa[u] - (double)pb[u];
                        sse += d * d;
                    }
                }
                r += dr;
                cc += dc;
                if (cc >= g.in_w) {
                    cc -= g.in_w;
                    ++r;
                }
            }
        }
        if (q + 1 < n_tiles) fetch(tile(q + 1));                                    // in flight under B and C
        if (!want_ssim) continue;                                                   // (workgroup-uniform)
        __syncthreads();
        if (tid < g.in_h * (SS_TW / SS_GB)) {                                                                // B
            const int r = tid % g.in_h, g0 = (tid / g.in_h) * SS_GB;
            if (g0 < g.ow) {
                double acc[5][SS_GB];
#pragma unroll
                for (int m = 0; m < 5; ++m)
#pragma unroll
                    for (int j = 0; j < SS_GB; ++j) acc[m][j] = 0.0;
#pragma unroll
                for (int k = 0; k < SS_GB + SS_HALO; ++k) {                         // (columns past in_w hold stale values: only positions >= ow see them)
                    const double a = (double)xs[r * SS_XP + g0 + k], b = (double)ys[r * SS_XP + g0 + k];
                    const double v[5] = {a, b, a * a, b * b, a * b};
#pragma unroll
                    for (int j = 0; j < SS_GB; ++j)
                        if (k - j >= 0 && k - j < SS_WIN) {
#pragma unroll
                            for (int m = 0; m < 5; ++m) acc[m][j] = fma(win.w(k - j), v[m], acc[m][j]);
                        }
                }
#pragma unroll
                for (int j = 0; j < SS_GB; ++j)
                    if (g0 + j < g.ow) {
#pragma unroll
                        for (int m = 0; m < 5; ++m) rows[m][g0 + j][r] = acc[m][j];
                    }
            }
        }
        __syncthreads();
        {                                                                                                    // C
            const int col = tid & 31, r0 = (tid >> 5) * SS_GC;
            if (col < g.ow && r0 < g.oh) {
                double acc[5][SS_GC];
#pragma unroll
                for (int m = 0; m < 5; ++m) {
#pragma unroll
                    for (int j = 0; j < SS_GC; ++j) acc[m][j] = 0.0;
#pragma unroll
                    for (int k = 0; k < SS_GC + SS_HALO; ++k) {                     // (rows past in_h are stale: only positions >= oh see them)
                        const double v = rows[m][col][r0 + k];
#pragma unroll
                        for (int j = 0; j < SS_GC; ++j)
                            if (k - j >= 0 && k - j < SS_WIN) acc[m][j] = fma(win.w(k - j), v, acc[m][j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < SS_GC; ++j)
                    if (r0 + j < g.oh) {
                        const double mx = acc[0][j], my = acc[1][j];
                        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
                        const double sxx = acc[2][j] - mxx, syy = acc[3][j] - myy, sxy = acc[4][j] - mxy;
                        const double num = (2.0 * mxy + c1) * (2.0 * sxy + c2);
                        const double den = ((mxx + myy) + c1) * ((sxx + syy) + c2);
                        ssum += num / den;
                    }
            }
        }
        __syncthreads();                                                            // the next tile's A writes what B read
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sse += __shfl_xor(sse, o, 64);
        ssum += __shfl_xor(ssum, o, 64);
    }
    if (lane == 0) {
        red[0][wave] = sse;
        red[1][wave] = ssum;
    }
    __syncthreads();
    if (tid == 0) {
        const double e = (((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / (double)chw;
        if (mse) mse[frame] = (float)e;
        if (psnr) psnr[frame] = (float)(10.0 * log10(range2 / e));
        if (ssim) ssim[frame] = (float)((((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) / ((double)C * Ho * Wo));
    }
}

// One wave per group of N candidates: lane l takes candidates l, l + 64, ...; a candidate's T frame rewards are added in fp64 in order and
// rounded once (`reward`), the group's sums meet in an xor butterfly.
__global__ __launch_bounds__(64) void group_advantages_kernel(const float* __restrict__ frame_reward, int N, int T, int mode, double eps,
                                                              float* __restrict__ reward, float* __restrict__ advantage) {
    const long g = blockIdx.x;
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int c = lane; c < N; c += 64) {
        const float* v = frame_reward + (g * N + c) * T;
        double a = 0.0;
        for (int j = 0; j < T; ++j) a += (double)v[j];
        const float r = (float)(a / (double)T);
        reward[g * N + c] = r;
        s += (double)r;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const double mean = s / (double)N;
    double q = 0.0;
    for (int c = lane; c < N; c += 64) {
        const double d = (double)reward[g * N + c] - mean;       // (this lane's own store)
        q += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const double sd = sqrt(q / (double)N);
    const bool bad = !(fabs(s) <= 1.79769313486231570815e308);   // a NaN or an infinite reward somewhere in the group
    for (int c = lane; c < N; c += 64) {
        const double d = (double)reward[g * N + c] - mean;
        double a = mode == 0 || d == 0.0 ? d : d / (sd + eps);
        if (bad) a = __builtin_nan("");
        advantage[g * N + c] = (float)a;
    }
}

// One wave per group.  Lane l first takes candidates l, l + 64, ...: a candidate's discounted sums run from its last frame down in fp64 (the
// product and the sum rounded separately -- this file contracts nothing -- so numpy restates them bit for bit) and every return is rounded
// once and stored.
// Behind the barrier lane l takes slots l, l + 64, ... of the group's advantage rows: a slot inside the window reads its frame's N returns
// back as stored (this workgroup's own stores; the barrier orders them) and adds them in candidate order, a slot outside it is zeros.
__global__ __launch_bounds__(64) void frame_advantages_kernel(const float* __restrict__ frame_reward, int N, int T, double gamma, int mode,
                                                              double eps, int slots, int slot_off, float* returns,
                                                              float* __restrict__ advantage) {
    const long g = blockIdx.x;
    const int lane = threadIdx.x;
    for (int c = lane; c < N; c += 64) {
        const long row = (g * N + c) * T;
        double s = (double)frame_reward[row + T - 1];
        returns[row + T - 1] = (float)(s / (double)T);
#pragma unroll 4
        for (int t = T - 2; t >= 0; --t) {
            const double r = (double)frame_reward[row + t];
            s = gamma == 0.0 ? r : r + gamma * s;                // (gamma 0 forms no product: a later inf must not arrive as 0 * inf)
            returns[row + t] = (float)(s / (double)T);
        }
    }
    __syncthreads();
    for (int j = lane; j < slots; j += 64) {
        float* out = advantage + g * N * slots + j;
        const int t = j - slot_off;
        if (t < 0 || t >= T) {
            for (int c = 0; c < N; ++c) out[(long)c * slots] = 0.f;
            continue;
        }
        const float* v = returns + g * N * T + t;
        double s = 0.0;
#pragma unroll 4
        for (int c = 0; c < N; ++c) s += (double)v[(long)c * T];
        const double mean = s / (double)N;
        double q = 0.0;
#pragma unroll 4
        for (int c = 0; c < N; ++c) {
            const double d = (double)v[(long)c * T] - mean;
            q += d * d;
        }
        const double sd = sqrt(q / (double)N);
        const bool bad = !(fabs(s) <= 1.79769313486231570815e308);   // a NaN or an infinite return somewhere in this (group, frame)
#pragma unroll 4
        for (int c = 0; c < N; ++c) {
            const double d = (double)v[(long)c * T] - mean;
            double a = d == 0.0 ? 0.0 : mode == 0 ? d : d / (sd + eps);
            if (bad) a = __builtin_nan("");
            out[(long)c * slots] = (float)a;
        }
    }
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int mage_video_metrics(const float* video, int64_t video_clip_stride, const float* target, int64_t target_clip_stride, int64_t clips,
                                  int32_t T, int32_t C, int32_t H, int32_t W, int64_t tgt_div, float data_range, float* mse, float* psnr,
                                  float* ssim, void* stream) {
    MAGE_CHECK_ARG(video && target && (mse || psnr || ssim), "mage_video_metrics: null video or target, or no output asked for");
    MAGE_CHECK_ARG(aligned4(video) && aligned4(target) && aligned4(mse) && aligned4(psnr) && aligned4(ssim),
                   "mage_video_metrics: pointers must be 4-byte aligned");
    MAGE_CHECK_ARG(clips > 0 && T > 0 && C > 0 && H > 0 && W > 0 && clips * (int64_t)T <= 0x7fffffffL && (int64_t)C * H * W <= 0x7fffffffL,
                   "mage_video_metrics: bad sizes clips=%ld T=%d C=%d H=%d W=%d", (long)clips, T, C, H, W);
    MAGE_CHECK_ARG(!ssim || (H >= SS_WIN && W >= SS_WIN), "mage_video_metrics: ssim needs H=%d and W=%d >= %d (the window)", H, W, SS_WIN);
    MAGE_CHECK_ARG(tgt_div >= 1, "mage_video_metrics: tgt_div=%ld must be >= 1", (long)tgt_div);
    MAGE_CHECK_ARG(data_range > 0.f && data_range <= 3.4028234e38f, "mage_video_metrics: data_range=%g must be finite and > 0", (double)data_range);
    const int64_t per_clip = (int64_t)T * C * H * W;
    MAGE_CHECK_ARG(video_clip_stride >= per_clip && target_clip_stride >= per_clip,
                   "mage_video_metrics: clip strides %ld / %ld are smaller than a clip (%ld elements)", (long)video_clip_stride,
                   (long)target_clip_stride, (long)per_clip);
    // balanced tiles: the window positions of an axis are shared out evenly over the fewest tiles that fit (an axis shorter than the window,
    // legal without ssim, is one tile)
    auto share = [](int n, int cap, int& tiles, int& size) {
        n = n < 1 ? 1 : n;
        size = (n + (n + cap - 1) / cap - 1) / ((n + cap - 1) / cap);
        tiles = (n + size - 1) / size;
    };
    int tiles_y, tiles_x, th, tw;
    share(H - SS_HALO, SS_TH, tiles_y, th);
    share(W - SS_HALO, SS_TW, tiles_x, tw);
    SsimWindow win;
    double sum = 0.0;
    for (int k = 0; k <= SS_HALO / 2; ++k) {
        const double d = (double)(k - SS_HALO / 2);
        win.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    }
    for (int k = 0; k < SS_WIN; ++k) sum += win.w(k);
    for (int k = 0; k <= SS_HALO / 2; ++k) win.g[k] /= sum;
    const double dr = (double)data_range, k1 = 0.01 * dr, k2 = 0.03 * dr;
    hipLaunchKernelGGL(video_metrics_kernel, dim3((unsigned)(clips * T)), dim3(256), 0, (hipStream_t)stream, video, (long)video_clip_stride, target,
                       (long)target_clip_stride, T, C, H, W, (long)tgt_div, tiles_y, tiles_x, th, tw, win, k1 * k1, k2 * k2, dr * dr, mse, psnr, ssim);
    MAGE_CHECK_LAUNCH("mage_video_metrics");
    return MAGE_OK;
}

extern "C" int mage_group_advantages(const float* frame_reward, int64_t groups, int32_t N, int32_t T, int32_t mode, float eps, float* reward,
                                     float* advantage, void* stream) {
    MAGE_CHECK_ARG(frame_reward && reward && advantage, "mage_group_advantages: null pointer");
    MAGE_CHECK_ARG(aligned4(frame_reward) && aligned4(reward) && aligned4(advantage), "mage_group_advantages: pointers must be 4-byte aligned");
    MAGE_CHECK_ARG(groups > 0 && groups <= 0x7fffffffL && N >= 2 && T >= 1, "mage_group_advantages: bad sizes groups=%ld N=%d (>= 2) T=%d (>= 1)",
                   (long)groups, N, T);
    MAGE_CHECK_ARG(mode == 0 || mode == 1, "mage_group_advantages: mode=%d is neither 0 (mean) nor 1 (mean and std)", mode);
    MAGE_CHECK_ARG(eps >= 0.f && eps <= 3.4028234e38f, "mage_group_advantages: eps=%g must be finite and >= 0", (double)eps);
    hipLaunchKernelGGL(group_advantages_kernel, dim3((unsigned)groups), dim3(64), 0, (hipStream_t)stream, frame_reward, N, T, mode, (double)eps,
                       reward, advantage);
    MAGE_CHECK_LAUNCH("mage_group_advantages");
    return MAGE_OK;
}

extern "C" int mage_frame_advantages(const float* frame_reward, int64_t groups, int32_t N, int32_t T, float gamma, int32_t mode, float eps,
                                     int32_t slots, int32_t slot_off, float* returns, float* advantage, void* stream) {
    MAGE_CHECK_ARG(frame_reward && returns && advantage, "mage_frame_advantages: null pointer");
    MAGE_CHECK_ARG(aligned4(frame_reward) && aligned4(returns) && aligned4(advantage), "mage_frame_advantages: pointers must be 4-byte aligned");
    MAGE_CHECK_ARG(groups > 0 && groups <= 0x7fffffffL && N >= 2 && T >= 1, "mage_frame_advantages: bad sizes groups=%ld N=%d (>= 2) T=%d (>= 1)",
                   (long)groups, N, T);
    MAGE_CHECK_ARG(slot_off >= 0 && (int64_t)slots >= (int64_t)slot_off + T,
                   "mage_frame_advantages: slot_off=%d must be >= 0 and slots=%d >= slot_off + T (T=%d)", slot_off, slots, T);
    MAGE_CHECK_ARG((int64_t)N * slots <= 0x7fffffffL / groups, "mage_frame_advantages: groups=%ld * N=%d * slots=%d must stay below 2^31",
                   (long)groups, N, slots);                      // (slots >= T: groups * N * T stays below it too)
    MAGE_CHECK_ARG(gamma >= 0.f && gamma <= 1.f, "mage_frame_advantages: gamma=%g must lie in [0, 1]", (double)gamma);
    MAGE_CHECK_ARG(mode == 0 || mode == 1, "mage_frame_advantages: mode=%d is neither 0 (mean) nor 1 (mean and std)", mode);
    MAGE_CHECK_ARG(eps >= 0.f && eps <= 3.4028234e38f, "mage_frame_advantages: eps=%g must be finite and >= 0", (double)eps);
    hipLaunchKernelGGL(frame_advantages_kernel, dim3((unsigned)groups), dim3(64), 0, (hipStream_t)stream, frame_reward, N, T, (double)gamma, mode,
                       (double)eps, slots, slot_off, returns, advantage);
    MAGE_CHECK_LAUNCH("mage_frame_advantages");
    return MAGE_OK;
}
