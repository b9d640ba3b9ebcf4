"""GPU: mage_video_metrics and mage_group_advantages against their fp64 restatement (tests/video_metrics_ref.py) at every tile-dispatch edge,
and the bitwise properties include/mage_hip_ext.h promises.

Bounds.  mse and psnr: 2 fp32 ulp of the restatement rounded to fp32 (+inf exactly where the frames are equal).  ssim: one absolute bound per
input family, 4 x the largest error the restatement evaluated naively in fp32 makes against fp64 on that family's frames here (4: the
kernel's summation order is not numpy's); the kernel never sets it.  Measured on these frames on the CPU (the test prints them): noise
2.5e-7 (the single-position 11 x 11 frames, where a denominator can be small; 8.9e-10 per 64 x 64 frame), noisy copies 1.9e-7 (9.4e-8 per
64 x 64 frame), flat -1 background 1.1e-5 (4.1e-7 per 64 x 64 frame), noise around one NaN frame 7.0e-8, identical 0 (so the kernel must
give exactly 1.0 there)."""
import functools
import zlib

import numpy as np
import pytest
import torch

from mage_amd import ops
from tests import video_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (C, H, W): one window position; a few; no tile multiple (2 x 2 tiles of 18 x 30); the 64 x 64 x 1 frame of cfg2 (2 x 2 tiles of 27 x 27);
# the 128 x 128 x 3 frame of cfg4 (5 x 4 tiles of 24 x 30); exactly one full 28 x 30 tile; one position more than that on both axes (tiles
# of 15 x 16 and 14 x 15)
SHAPES = [(1, 11, 11), (1, 12, 17), (3, 45, 70), (1, 64, 64), (3, 128, 128), (1, 38, 40), (1, 39, 41)]
CLIPS_T = [(1, 1), (3, 5), (37, 2)]
FAMILIES = ("noise", "copy", "flat", "identical", "nan")


def _blobs(rng, n, H, W, shift=0):
    """Moving-MNIST-like frames: -1 background, two bright blobs, noise of 1e-3."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.full((n, H, W), -1.0)
    for i in range(n):
        for _ in range(2):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), max(1.0, min(H, W) / 8)
            out[i] = np.maximum(out[i], -1 + 2 * np.exp(-((yy - cy - shift) ** 2 + (xx - cx) ** 2) / (2 * s * s)))
    return out + 1e-3 * rng.standard_normal(out.shape)


@functools.lru_cache(maxsize=None)
def case(family, shape, clips_t, div, skip0):
    """(video [clips, T, C, H, W], target [tclips, T (+1 with skip0), C, H, W]) fp32 numpy and the fp64 / fp32 restatements."""
    (C, H, W), (clips, T) = shape, clips_t
    rng = np.random.default_rng(zlib.crc32(repr((family, shape, clips_t, div)).encode()))
    tclips = -(-clips // div)
    idx = np.arange(clips) // div
    if family == "flat":
        tgt = _blobs(rng, tclips * T * C, H, W).reshape(tclips, T, C, H, W)
        vid = tgt[idx] + 0.02 * rng.standard_normal((clips, T, C, H, W)) * (tgt[idx] > -0.9)
    else:
        tgt = rng.uniform(-1, 1, (tclips, T, C, H, W))
        vid = rng.uniform(-1, 1, (clips, T, C, H, W))
        if family == "copy":
            vid = np.clip(tgt[idx] + 0.05 * rng.standard_normal(vid.shape), -1, 1)
        if family == "identical":
            vid = tgt[idx].copy()
    vid, tgt = vid.astype(np.float32), tgt.astype(np.float32)
    nan_at = None
    if family == "nan":
        nan_at = (clips - 1, T // 2)
        vid[nan_at][C - 1, H // 2, W - 1] = np.nan
    ssim_ok = H >= 11 and W >= 11
    with np.errstate(invalid="ignore"):
        ref = R.metrics(vid, tgt, div)
        err32 = np.abs(R.metrics(vid, tgt, div, dtype=np.float32)["ssim"].astype(np.float64) - ref["ssim"]) if ssim_ok else None
    if skip0:
        tgt = np.concatenate([rng.uniform(-1, 1, (tclips, 1, C, H, W)).astype(np.float32), tgt], 1)
    return dict(video=vid, target=tgt, ref=ref, err32=err32, nan_at=nan_at, div=div, skip0=skip0)


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        for ci, ct in enumerate(CLIPS_T):
            for div in (1, 3):
                out.append(("noise", shape, ct, div, (si + ci + div) % 2 == 0))
        for fi, fam in enumerate(FAMILIES[1:]):
            out.append((fam, shape, (3, 5), 1 + 2 * ((si + fi) % 2), (si + fi) % 3 == 0))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def ssim_bound(family):
    """4 x the naive fp32 evaluation's largest error over every frame of the family in this file."""
    worst = max(np.nanmax(case(*c)["err32"]) for c in CASES if c[0] == family)
    print(f"naive fp32 ssim error, family {family}: {worst:.3e}")
    return 4.0 * float(worst)


def run(c, **kw):
    v, t = torch.from_numpy(c["video"]).to(DEV), torch.from_numpy(c["target"]).to(DEV)
    out = ops.video_metrics(v, t[:, 1:] if c["skip0"] else t, tgt_div=c["div"], **kw)
    torch.cuda.synchronize()
    return {k: o.cpu().numpy() for k, o in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(got, c, family):
    ref = c["ref"]
    nan = np.zeros(ref["mse"].shape, bool)
    if c["nan_at"] is not None:
        nan[c["nan_at"]] = True
        assert all(np.isnan(g[nan]).all() for g in got.values())                 # the NaN frame: every output NaN
    ok = ~nan
    assert all(g.dtype == np.float32 and g.shape == ref["mse"].shape and not np.isnan(g[ok]).any() for g in got.values())
    want = ref["mse"][ok].astype(np.float32)
    u = R.ulps(got["mse"][ok], want)
    u[want == 0] = np.where(got["mse"][ok][want == 0] == 0, 0.0, np.inf)
    zero = ref["mse"][ok] == 0
    pu = R.ulps(got["psnr"][ok][~zero], ref["psnr"][ok][~zero].astype(np.float32)) if (~zero).any() else np.zeros(1)
    assert np.all(got["psnr"][ok][zero] == np.inf)
    line = f"{family}: mse {u.max():.2f} ulp, psnr {pu.max():.2f} ulp"
    if "ssim" in got:
        e = np.abs(got["ssim"][ok].astype(np.float64) - ref["ssim"][ok]).max()
        line += f", ssim error {e:.3e} (bound {ssim_bound(family):.3e}, naive fp32 on this case {np.nanmax(c['err32']):.3e})"
    print(line)
    assert u.max() <= 2 and pu.max() <= 2
    if "ssim" in got:
        assert e <= ssim_bound(family)
    if family == "identical":
        assert np.all(got["mse"] == 0) and np.all(got["ssim"] == 1.0)


@pytest.mark.parametrize("family,shape,clips_t,div,skip0", CASES)
def test_every_frame_matches_the_restatement(family, shape, clips_t, div, skip0):
    c = case(family, shape, clips_t, div, skip0)
    got = run(c)
    check(got, c, family)
    again = run(c)
    assert all(np.array_equal(bits(got[k]), bits(again[k])) for k in got)        # two launches, the same bits


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 10, 40), (1, 64, 9)])
def test_mse_and_psnr_alone_below_the_window(shape):
    """Without ssim a frame may be smaller than the window (one tile on that axis)."""
    c = case("noise", shape, (3, 5), 1, False)
    got = run(c, ssim=False)
    assert set(got) == {"mse", "psnr"}
    check(got, c, "noise")
    only = run(c, ssim=False, mse=False)
    assert set(only) == {"psnr"} and np.array_equal(bits(only["psnr"]), bits(got["psnr"]))


@pytest.mark.parametrize("family,shape", [("noise", (3, 45, 70)), ("flat", (1, 64, 64)), ("copy", (3, 128, 128)), ("noise", (1, 11, 11))])
def test_symmetric_bit_for_bit(family, shape):
    c = case(family, shape, (3, 5), 1, False)
    v, t = torch.from_numpy(c["video"]).to(DEV), torch.from_numpy(c["target"]).to(DEV)
    a, b = ops.video_metrics(v, t), ops.video_metrics(t, v)
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
    same = ops.video_metrics(v, v.clone())
    assert torch.all(same["mse"] == 0) and torch.all(same["psnr"] == float("inf")) and torch.all(same["ssim"] == 1.0)


@pytest.mark.parametrize("shape", [(1, 12, 17), (3, 45, 70), (1, 64, 64)])
def test_a_nan_pixel_stays_in_its_frame(shape):
    c = case("nan", shape, (3, 5), 1, False)
    clean = c["video"].copy()
    clean[np.isnan(clean)] = 0.25
    got, ref = run(c), run({**c, "video": clean})
    for k in got:
        nan = np.isnan(got[k])
        assert nan.sum() == 1 and nan[c["nan_at"]] and np.array_equal(bits(got[k][~nan]), bits(ref[k][~nan]))
    t = c["target"].copy()                                                       # ... and on the target's side
    t[0, 1, 0, 3, 3] = np.nan
    got = run({**c, "video": clean, "target": t})
    for k in got:
        nan = np.isnan(got[k])
        assert nan.sum() == 1 and nan[0, 1] and np.array_equal(bits(got[k][~nan]), bits(ref[k][~nan]))


@pytest.mark.parametrize("shape", [(3, 45, 70), (1, 64, 64), (3, 128, 128)])
def test_a_frame_does_not_know_its_launch(shape):
    """A frame alone against the same frame inside a larger launch; tgt_div 3 against tgt_div 1 on an expanded target; clips far apart."""
    c = case("copy", shape, (37, 2), 3, False)
    v, t = torch.from_numpy(c["video"]).to(DEV), torch.from_numpy(c["target"]).to(DEV)
    whole = ops.video_metrics(v, t, tgt_div=3)
    expanded = ops.video_metrics(v, t.repeat_interleave(3, 0)[:37].contiguous(), tgt_div=1)
    assert all(torch.equal(whole[k].view(torch.int32), expanded[k].view(torch.int32)) for k in whole)
    for r, f in ((0, 0), (17, 1), (36, 1)):
        alone = ops.video_metrics(v[r:r + 1, f:f + 1].contiguous(), t[r // 3:r // 3 + 1, f:f + 1].contiguous())
        assert all(torch.equal(alone[k].view(torch.int32), whole[k][r:r + 1, f:f + 1].view(torch.int32)) for k in whole)
    wide = torch.full((37, 3, *v.shape[2:]), float("nan"), device=DEV)           # a view whose clips lie further apart
    wide[:, :2] = v
    strided = ops.video_metrics(wide[:, :2], t, tgt_div=3)
    assert all(torch.equal(whole[k].view(torch.int32), strided[k].view(torch.int32)) for k in whole)


# ---------------------------------------------------------------- mage_group_advantages
def _adv_case(seed, groups, N, T):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.2, 0.9, (groups, N, 1)) + 0.05 * rng.standard_normal((groups, N, T))).astype(np.float32).reshape(groups * N, T)


@pytest.mark.parametrize("groups,N,T", [(1, 2, 1), (3, 3, 4), (5, 8, 15), (2, 130, 3), (700, 4, 2)])
@pytest.mark.parametrize("mode,eps", [(0, 0.0), (1, 1e-6), (1, 0.0), (1, 0.5)])
def test_group_advantages_match_the_restatement(groups, N, T, mode, eps):
    fr = _adv_case(groups * 1000 + N, groups, N, T)
    rew, adv = ops.group_advantages(torch.from_numpy(fr).to(DEV), groups=groups, n_cand=N, mode=mode, eps=eps)
    rew2, adv2 = ops.group_advantages(torch.from_numpy(fr).to(DEV), groups=groups, n_cand=N, mode=mode, eps=eps)
    assert torch.equal(rew, rew2) and torch.equal(adv, adv2) and rew.shape == (groups, N) and adv.shape == (groups * N,)
    want_r, want_a = R.group_advantages(fr, groups, N, mode, eps)
    ur = R.ulps(rew.cpu().numpy(), want_r).max()
    # the advantage is a difference of rewards: 2 ulp of its own fp32 value, plus the fp64 rounding of the operands it was formed from
    got = adv.cpu().numpy().astype(np.float64)
    tol = 2 * np.spacing(np.abs(want_a).astype(np.float32)).astype(np.float64) + 1e-14
    print(f"reward {ur:.2f} ulp, advantage worst error / tolerance {np.max(np.abs(got - want_a) / tol):.3f}")
    assert ur <= 2 and np.all(np.abs(got - want_a) <= tol)


@pytest.mark.parametrize("mode,eps", [(0, 0.0), (1, 0.0), (1, 1e-6)])
def test_equal_rewards_give_zero_and_a_non_finite_reward_stays_in_its_group(mode, eps):
    groups, N, T = 4, 5, 3
    fr = _adv_case(7, groups, N, T).reshape(groups, N, T)
    fr[1] = np.float32(0.3)                                                      # 0.3 is not a binary fraction: the mean must still be exact
    fr[2, 3, 1] = np.inf
    fr[3, 0, 0] = np.nan
    fr = fr.reshape(groups * N, T)
    rew, adv = ops.group_advantages(torch.from_numpy(fr).to(DEV), groups=groups, n_cand=N, mode=mode, eps=eps)
    adv = adv.cpu().numpy().reshape(groups, N)
    assert np.array_equal(bits(adv[1]), np.zeros(N, np.int32))                   # exactly +0
    assert np.isnan(adv[2]).all() and np.isnan(adv[3]).all() and np.isfinite(adv[0]).all() and np.abs(adv[0]).max() > 0
    want = R.group_advantages(fr, groups, N, mode, eps)[1].reshape(groups, N)
    assert np.allclose(adv[0], want[0], rtol=1e-6, atol=0)
    assert rew[2, 3].item() == float("inf") and np.isnan(rew[3, 0].item())
