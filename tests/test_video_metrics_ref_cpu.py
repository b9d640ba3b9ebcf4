"""CPU: the numpy restatement of mage_video_metrics / mage_group_advantages (tests/video_metrics_ref.py) against independent facts, the
extension table against its header, the argument rules of both entry points through the loaded library, and the Python refusals of
MAGE.video_metrics / MAGE.rollout on a CPU model (nothing is launched)."""
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from mage_amd import _lib
from mage_amd.utils import synth
from tests import video_metrics_ref as R
from tests.helpers import build_mage, count_lib_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- the restatement
def test_window_is_the_normalised_gaussian():
    g = R.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1 / 4.5)) < 1e-15 and abs(g[0] / g[5] - np.exp(-25 / 4.5)) < 1e-15


def test_moments_match_scipy_correlate1d():
    rng = np.random.default_rng(0)
    x, y = rng.uniform(-1, 1, (2, 3, 23, 31)), rng.uniform(-1, 1, (2, 3, 23, 31))
    g = R.window()
    for a in (x, y, x * x, y * y, x * y):
        full = ndimage.correlate1d(ndimage.correlate1d(a, g, axis=-1, mode="constant"), g, axis=-2, mode="constant")
        assert np.abs(R.blur_valid(a) - full[..., 5:-5, 5:-5]).max() < 1e-15


def test_constant_images_give_the_closed_form():
    for a, b, dr in ((0.3, -0.7, 2.0), (0.9, 0.9, 2.0), (10.0, 200.0, 255.0), (-1.0, 1.0, 2.0)):
        x, y = np.full((1, 14, 19), a), np.full((1, 14, 19), b)
        c1 = (0.01 * dr) ** 2
        assert abs(R.ssim(x, y, dr) - (2 * a * b + c1) / (a * a + b * b + c1)) < 1e-12
        assert abs(R.mse(x, y) - (a - b) ** 2) < 1e-12 * max(1.0, (a - b) ** 2)


def test_identity_and_symmetry():
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1, 1, (4, 2, 20, 17)), rng.uniform(-1, 1, (4, 2, 20, 17))
    for dt in (np.float64, np.float32):
        assert np.array_equal(R.ssim(x, x, dtype=dt), np.ones(4, dt)) and np.array_equal(R.mse(x, x, dtype=dt), np.zeros(4, dt))
        assert np.all(R.psnr(x, x, dtype=dt) == np.inf)
        assert np.array_equal(R.ssim(x, y, dtype=dt), R.ssim(y, x, dtype=dt)) and np.array_equal(R.mse(x, y, dtype=dt), R.mse(y, x, dtype=dt))
    s = R.ssim(x, y)
    assert np.all(np.abs(s) < 0.5) and np.all(R.ssim(x, x + 0.01 * y) > 0.9)


def test_single_position_by_hand():
    """11 x 11: one valid position, its moments straight from the 2-D window (no separable passes)."""
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-1, 1, (11, 11)), rng.uniform(-1, 1, (11, 11))
    w = np.outer(R.window(), R.window())
    mx, my = (w * x).sum(), (w * y).sum()
    sxx, syy, sxy = (w * x * x).sum() - mx * mx, (w * y * y).sum() - my * my, (w * x * y).sum() - mx * my
    c1, c2 = 0.02 ** 2, 0.06 ** 2
    want = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    m = R.metrics(x[None, None, None], y[None, None, None])
    assert m["ssim"].shape == (1, 1) and abs(m["ssim"][0, 0] - want) < 1e-14
    assert abs(m["mse"][0, 0] - ((x - y) ** 2).mean()) < 1e-15
    assert abs(m["psnr"][0, 0] - 10 * np.log10(4.0 / ((x - y) ** 2).mean())) < 1e-12


def test_tgt_div_shares_targets():
    rng = np.random.default_rng(3)
    v, t = rng.uniform(-1, 1, (5, 2, 1, 12, 12)), rng.uniform(-1, 1, (2, 2, 1, 12, 12))
    a, b = R.metrics(v, t, tgt_div=3), R.metrics(v, t[[0, 0, 0, 1, 1]])
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_group_advantages_restatement():
    fr = np.array([[1, 2], [3, 4], [5, 9], [2, 2], [2, 2], [2, 2]], np.float32)
    rew, adv = R.group_advantages(fr, 2, 3, 0, 0.0)
    assert np.array_equal(rew, np.array([[1.5, 3.5, 7.0], [2, 2, 2]], np.float32)) and np.allclose(adv, [-2.5, -0.5, 3.0, 0, 0, 0])
    _, adv1 = R.group_advantages(fr, 2, 3, 1, 0.0)
    assert np.allclose(adv1[:3], np.array([-2.5, -0.5, 3.0]) / np.std([1.5, 3.5, 7.0])) and np.array_equal(adv1[3:], np.zeros(3))
    fr[1, 0] = INF
    _, adv2 = R.group_advantages(fr, 2, 3, 1, 1e-6)
    assert np.isnan(adv2[:3]).all() and np.array_equal(adv2[3:], np.zeros(3))


# ---------------------------------------------------------------- the extension table
def test_extension_table_matches_its_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.EXT_SIGNATURES) and {"mage_video_metrics", "mage_group_advantages"} <= declared
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.mage_abi_version() == 10
    for name in ("mage_video_metrics", "mage_group_advantages"):
        fn = getattr(lib, name)
        assert fn.restype is _lib.EXT_SIGNATURES[name][0] and list(fn.argtypes) == _lib.EXT_SIGNATURES[name][1]
        # the header's argument list has as many entries as the table's
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1])


# ---------------------------------------------------------------- argument rules (refused before anything is launched)
P = 4096                    # a fake, aligned device address
VM_ORDER = ("video", "video_clip_stride", "target", "target_clip_stride", "clips", "T", "C", "H", "W", "tgt_div", "data_range", "mse", "psnr",
            "ssim")
VM_GOOD = dict(video=P, video_clip_stride=4 * 3 * 16 * 16, target=P, target_clip_stride=5 * 3 * 16 * 16, clips=6, T=4, C=3, H=16, W=16, tgt_div=3,
               data_range=2.0, mse=P, psnr=P, ssim=P)


@pytest.mark.parametrize("bad", [
    dict(video=None), dict(target=None), dict(mse=None, psnr=None, ssim=None), dict(H=10), dict(W=10), dict(H=10, W=10), dict(clips=0),
    dict(clips=-1), dict(T=0), dict(C=0), dict(H=0), dict(W=-3), dict(tgt_div=0), dict(tgt_div=-2), dict(data_range=0.0), dict(data_range=-1.0),
    dict(data_range=INF), dict(data_range=NAN), dict(video=P + 2), dict(target=P + 1), dict(mse=P + 2), dict(psnr=P + 3), dict(ssim=P + 1),
    dict(video_clip_stride=4 * 3 * 16 * 16 - 1), dict(target_clip_stride=16), dict(video_clip_stride=-1), dict(clips=2 ** 31),
    dict(H=50000, W=50000, video_clip_stride=2 ** 40, target_clip_stride=2 ** 40),
])
def test_video_metrics_refuses_bad_arguments(bad):
    a = {**VM_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_video_metrics(*[a[k] for k in VM_ORDER], None)
    assert rc == -1 and "mage_video_metrics" in lib.mage_last_error().decode(), (bad, rc)


GA_ORDER = ("frame_reward", "groups", "N", "T", "mode", "eps", "reward", "advantage")
GA_GOOD = dict(frame_reward=P, groups=4, N=3, T=5, mode=1, eps=1e-6, reward=P, advantage=P)


@pytest.mark.parametrize("bad", [
    dict(frame_reward=None), dict(reward=None), dict(advantage=None), dict(groups=0), dict(groups=-1), dict(N=1), dict(N=0), dict(T=0),
    dict(mode=2), dict(mode=-1), dict(eps=-1e-6), dict(eps=INF), dict(eps=NAN), dict(frame_reward=P + 2), dict(reward=P + 1),
    dict(advantage=P + 3), dict(groups=2 ** 31),
])
def test_group_advantages_refuses_bad_arguments(bad):
    a = {**GA_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_group_advantages(*[a[k] for k in GA_ORDER], None)
    assert rc == -1 and "mage_group_advantages" in lib.mage_last_error().decode(), (bad, rc)


# ---------------------------------------------------------------- Python refusals on a CPU model
@pytest.fixture()
def counted(monkeypatch):
    return count_lib_calls(monkeypatch, _lib.load())


def test_rollout_and_video_metrics_refuse_on_a_cpu_model(counted):
    L = 4
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=16), 0)
    batch = synth.synth_batch_mnist(2, L, seed=0)
    state = lambda: (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.precision)      # noqa: E731

    def refused(match, *a, **kw):
        before = state()
        with pytest.raises(ValueError, match=match):
            m.rollout(*a, **kw)
        assert counted == [] and state() == before
    refused("set_sampling", batch, 3)
    m.set_sampling(0.9, top_k=8)
    m.use_cids = False
    refused("use_cids=False", batch, 3)
    m.use_cids = True
    for n in (1, 0, -2, 2.0, True, None):
        refused("candidates", batch, n)
    refused("reward", batch, 3, reward="lpips")
    refused("normalize", batch, 3, normalize="rank")
    for e in (-1.0, NAN, INF, "x"):
        refused("eps", batch, 3, eps=e)
    refused("images", {**batch, "images": batch["images"][:, 0]}, 3)
    refused("ground truth", {**batch, "images": batch["images"][:, :2]}, 3)
    refused("ground truth", {**batch, "images": batch["images"].double()}, 3, reward="psnr")
    refused("ground truth", {**batch, "images": batch["images"][..., :10]}, 3, reward="neg_mse")
    refused("GPU", batch, 3)
    refused("GPU", {**batch, "images": batch["images"][:, :1]}, 3, reward=lambda v, b: None)     # (a callable needs no ground truth)
    assert all(getattr(m, a) is None for a in m._LOGPROB_RESULTS) and m.last_tokens is None and m.last_sample_seeds is None

    x = batch["images"]

    def vm_refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            m.video_metrics(*a, **kw)
        assert counted == []
    vm_refused("GPU", x, x)
    vm_refused("fp32", x.double(), x.double())
    vm_refused("fp32", x[0], x[0])
    vm_refused("fp32", x.numpy(), x)
    vm_refused("same shape", x, x[:, 1:])
    vm_refused("11", x[..., :10], x[..., :10])
    for dr in (0.0, -1.0, NAN, INF):
        vm_refused("data_range", x, x, data_range=dr)
    plus = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)             # use_cids=False: frames only
    with pytest.raises(ValueError, match="GPU"):
        plus.video_metrics(x, x)
    with pytest.raises(ValueError, match="use_cids=False"):
        plus.rollout(batch, 3)
    assert counted == []
