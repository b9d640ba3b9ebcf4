"""The rules of mage_video_metrics and mage_group_advantages (include/mage_hip_ext.h) restated in numpy.  `dtype` is the type every value is
held and every operation is done in: np.float64 is the reference, np.float32 the same formula evaluated naively -- its error against fp64
is what sets the SSIM bounds of tests/test_gpu_video_metrics.py."""
import numpy as np

WIN, SIGMA = 11, 1.5


def window(dtype=np.float64):
    """The 11-tap Gaussian, sigma 1.5, normalised to sum 1 (the 2-D window is its outer product with itself)."""
    d = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).astype(dtype)


def blur_valid(a, dtype=np.float64):
    """The windowed mean of a [..., H, W] at the (H-10) x (W-10) positions where the window lies inside: rows first, then columns."""
    g = window(dtype)
    a = a.astype(dtype)
    H, W = a.shape[-2:]
    rows = np.zeros(a.shape[:-1] + (W - WIN + 1,), dtype)
    for k in range(WIN):
        rows = rows + g[k] * a[..., k:k + W - WIN + 1]
    out = np.zeros(a.shape[:-2] + (H - WIN + 1, W - WIN + 1), dtype)
    for k in range(WIN):
        out = out + g[k] * rows[..., k:k + H - WIN + 1, :]
    return out


def ssim_map(x, y, data_range=2.0, dtype=np.float64):
    """SSIM at every valid position of x, y [..., H, W]."""
    x, y = x.astype(dtype), y.astype(dtype)
    c1, c2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    mx, my = blur_valid(x, dtype), blur_valid(y, dtype)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = blur_valid(x * x, dtype) - mxx, blur_valid(y * y, dtype) - myy, blur_valid(x * y, dtype) - mxy
    two = dtype(2)
    return ((two * mxy + c1) * (two * sxy + c2)) / ((mxx + myy + c1) * (sxx + syy + c2))


def ssim(x, y, data_range=2.0, dtype=np.float64):
    """x, y [..., C, H, W] -> [...]: the mean over channels and valid positions."""
    return ssim_map(x, y, data_range, dtype).mean(axis=(-3, -2, -1), dtype=dtype)


def mse(x, y, dtype=np.float64):
    d = x.astype(dtype) - y.astype(dtype)
    return (d * d).mean(axis=(-3, -2, -1), dtype=dtype)


def psnr(x, y, data_range=2.0, dtype=np.float64):
    with np.errstate(divide="ignore"):
        return dtype(10) * np.log10(dtype(data_range) ** 2 / mse(x, y, dtype))


def metrics(video, target, tgt_div=1, data_range=2.0, dtype=np.float64):
    """video [clips, T, C, H, W] against target clip r // tgt_div: {'mse', 'psnr', 'ssim'}, [clips, T] each, in `dtype`."""
    tgt = target[np.arange(video.shape[0]) // tgt_div]
    out = {"mse": mse(video, tgt, dtype), "psnr": psnr(video, tgt, data_range, dtype)}
    if video.shape[-1] >= WIN and video.shape[-2] >= WIN:
        out["ssim"] = ssim(video, tgt, data_range, dtype)
    return out


def group_advantages(frame_reward, groups, N, mode, eps):
    """frame_reward [groups*N, T] fp32 -> (reward fp32 [groups, N], advantage fp64 [groups*N]): the reward is rounded to fp32 before the group
    statistics, as the kernel stores it; a group holding a non-finite reward is NaN throughout; r == mean gives exactly 0."""
    fr = np.asarray(frame_reward, np.float32).reshape(groups, N, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        reward = fr.astype(np.float64).mean(-1).astype(np.float32)
        r = reward.astype(np.float64)
        mean = r.mean(1, keepdims=True)
        d = r - mean
        if mode == 1:
            sd = np.sqrt((d * d).mean(1, keepdims=True))
            d = np.where(d == 0.0, 0.0, d / (sd + float(np.float32(eps))))
        d = np.where(np.isfinite(r).all(1, keepdims=True), d, np.nan)
    return reward, d.reshape(-1)


def ulps(got, want):
    """|got - want| in units of fp32 ulps of want (want fp32 finite)."""
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
