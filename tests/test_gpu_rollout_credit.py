"""GPU: MAGE.rollout(credit='frame', gamma=) and MAGE.policy_loss with one advantage per frame, on tests/test_gpu_rollout.py's small model
(L = 5, 3 clips, 3 candidates; built the same way here).

Bounds.  returns against the restatement (tests/frame_advantages_ref.py) applied to the call's own frame_metrics: equal bits; advantages:
2 fp32 spacings of the expected value + 1e-14 (tests/test_gpu_frame_advantages.py's), and equal bits against the restatement applied to
the call's own returns.  Everything credit= must not touch -- tokens, video, seeds, rewards, frame_metrics, pairs, given -- and
policy_loss against the same advantages expanded to one per token: equal bits."""
import copy

import numpy as np
import pytest
import torch

from mage_amd.utils import synth
from tests import frame_advantages_ref as F
from tests.helpers import build_mage, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, N, TEMP, CTX, GAMMA = 5, 3, 3, 0.9, 3, 0.9
SEEDS = [11, 12, 13]


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), 41, DEV)
    batch = dev_batch({**synth.synth_batch_mnist(B, L, seed=41, text_len=9, ragged_text=True), "sample_seed": torch.tensor(SEEDS, dtype=torch.int64)})
    return m, batch


def _reset(m, ar_mode="full"):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32").set_context(1)
    m.ar_mode = ar_mode
    m.eval()
    m.zero_grad(set_to_none=True)


@pytest.fixture(scope="module")
def rolled(small):
    """The same rollout under both credits, plain and continued (context=3); shared and left unchanged by the tests below."""
    m, batch = small
    _reset(m)
    m.set_sampling(TEMP)
    out = {"clip": m.rollout(batch, N, pairs="best_worst"),
           "frame": m.rollout(batch, N, pairs="best_worst", credit="frame", gamma=GAMMA),
           "clip_ctx": m.rollout(batch, N, context=CTX),
           "frame_ctx": m.rollout(batch, N, context=CTX, credit="frame", gamma=GAMMA)}
    _reset(m)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        f32 = a.dtype == torch.float32
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a) if f32 else a, _bits(b) if f32 else b)
    return a is b or a == b


def _check_against_the_restatement(out, T, slot_off, gamma, mode, eps=1e-6, reward="ssim"):
    fr = out["frame_metrics"][reward].cpu().numpy()
    assert fr.shape == (B * N, T)
    want_r, want_a = F.frame_advantages(fr, B, N, gamma, mode, eps, L - 1, slot_off)
    ret, adv = out["returns"], out["advantages"]
    assert ret.shape == (B * N, T) and ret.dtype == torch.float32 and adv.shape == (B * N, L - 1) and adv.dtype == torch.float32
    ret, adv = ret.cpu().numpy(), adv.cpu().numpy()
    assert np.array_equal(F.bits(ret), F.bits(want_r))
    tol = 2 * np.spacing(np.abs(want_a).astype(np.float32)).astype(np.float64) + 1e-14
    assert np.all(np.abs(adv.astype(np.float64) - want_a) <= tol) and np.abs(adv).max() > 0
    assert np.array_equal(F.bits(adv), F.bits(F.advantages(ret, B, N, mode, eps, L - 1, slot_off).astype(np.float32)))
    assert np.array_equal(F.bits(adv[:, :slot_off]), np.zeros((B * N, slot_off), np.int32))


UNTOUCHED = ("tokens", "video", "seeds", "rewards", "frame_metrics", "behaviour_logprobs", "token_logprobs", "given", "batch")


def test_frame_credit_changes_the_advantages_alone(rolled):
    clip, frame = rolled["clip"], rolled["frame"]
    assert all(_same(clip[k], frame[k]) for k in UNTOUCHED + ("pairs",))
    assert set(frame) == set(clip) | {"returns"} and clip["advantages"].shape == (B * N,) and frame["rewards"].shape == (B, N)
    _check_against_the_restatement(frame, L - 1, 0, GAMMA, 1)
    adv = frame["advantages"].view(B, N, L - 1)
    assert float(adv.sum(1).abs().max()) < 1e-5                                        # centred per (clip, frame)
    assert not torch.equal(adv[..., 0], adv[..., L - 2])                               # (one advantage per frame, not one per clip)


def test_context_pads_the_given_frames_with_zeros(rolled):
    clip, frame = rolled["clip_ctx"], rolled["frame_ctx"]
    assert all(_same(clip[k], frame[k]) for k in UNTOUCHED) and frame["given"] is not None and bool(frame["given"][:, :CTX - 1].all())
    assert all(v.shape == (B * N, L - CTX) for v in frame["frame_metrics"].values())
    _check_against_the_restatement(frame, L - CTX, CTX - 1, GAMMA, 1)
    assert torch.equal(_bits(frame["advantages"][:, :CTX - 1]), torch.zeros(B * N, CTX - 1, dtype=torch.int32, device=DEV))      # +0 bits


@pytest.mark.parametrize("reward,normalize,gamma", [("psnr", "mean", 1.0), ("neg_mse", None, 0.0)])
def test_normalize_and_gamma_reach_the_kernel(small, rolled, reward, normalize, gamma):
    m, batch = small
    _reset(m)
    m.set_sampling(TEMP)
    out = m.rollout(batch, N, reward=reward, normalize=normalize, credit="frame", gamma=gamma)
    _reset(m)
    assert _same(out["tokens"], rolled["clip"]["tokens"]) and _same(out["frame_metrics"], rolled["clip"]["frame_metrics"])
    if normalize is None:                                                              # the returns themselves, in the slots
        assert torch.equal(_bits(out["advantages"]), _bits(out["returns"]))
        want = F.returns(-out["frame_metrics"]["mse"].cpu().numpy(), B, N, gamma)
        assert np.array_equal(F.bits(out["returns"].cpu().numpy()), F.bits(want))
        assert np.array_equal(F.bits(want), F.bits((-out["frame_metrics"]["mse"].cpu().numpy().astype(np.float64) / (L - 1)).astype(np.float32)))
    else:
        _check_against_the_restatement(out, L - 1, 0, gamma, 0, reward=reward)
        # gamma = 1: frame 0's return is the candidate's mean reward up to the order of the sum
        assert float((out["returns"][:, 0] - out["rewards"].reshape(-1)).abs().max()) <= 2 * float(np.spacing(np.float32(out["rewards"].abs().max().item())))


def test_a_callable_reward_gives_one_reward_per_frame(small, rolled):
    m, batch = small
    _reset(m)
    m.set_sampling(TEMP)
    per_frame = lambda video, b: video[:, 1:].mean(dim=(2, 3, 4))                      # noqa: E731   [B*N, L-1]
    per_clip = lambda video, b: video[:, 1:].mean(dim=(1, 2, 3, 4))                    # noqa: E731   [B*N]
    out = m.rollout(batch, N, reward=per_frame, credit="frame", gamma=GAMMA, normalize="mean")
    fr = out["video"][:, 1:].mean(dim=(2, 3, 4))
    assert out["frame_metrics"] is None and _same(out["tokens"], rolled["clip"]["tokens"])
    want_r, want_a = F.frame_advantages(fr.cpu().numpy(), B, N, GAMMA, 0, 1e-6)
    assert np.array_equal(F.bits(out["returns"].cpu().numpy()), F.bits(want_r))
    tol = 2 * np.spacing(np.abs(want_a).astype(np.float32)).astype(np.float64) + 1e-14
    assert np.all(np.abs(out["advantages"].cpu().numpy().astype(np.float64) - want_a) <= tol)
    assert float((out["rewards"].reshape(-1) - fr.mean(1)).abs().max()) < 1e-6        # still the per-candidate mean
    before = (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.context_frames)
    with pytest.raises(ValueError, match=r"reward callable.*\[9, 4\]"):
        m.rollout(batch, N, reward=per_clip, credit="frame")
    with pytest.raises(ValueError, match=r"reward callable.*\[9, 2\]"):
        m.rollout(batch, N, reward=per_frame, credit="frame", context=CTX)            # (L-1 frames where L-k were generated)
    assert before == (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.context_frames)
    assert m.rollout(batch, N, reward=per_clip)["advantages"].shape == (B * N,)
    with pytest.raises(ValueError, match=r"reward callable.*\[9\]"):
        m.rollout(batch, N, reward=per_frame)
    _reset(m)


def test_refusals_launch_nothing_and_clip_credit_calls_nothing_new(small, monkeypatch):
    m, batch = small
    _reset(m)
    m.set_sampling(TEMP)
    calls = count_lib_calls(monkeypatch)
    settings = lambda: (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.precision, m.ar_mode, m.context_frames)  # noqa: E731

    def refused(match, **kw):
        before = settings()
        with pytest.raises(ValueError, match=match):
            m.rollout(batch, N, **kw)
        assert calls == [] and settings() == before
    for c in ("token", "Frame", None, 1):
        refused("credit", credit=c)
    for g in (-0.1, 1.5, float("nan"), float("inf"), "1", None, True):
        refused("gamma", credit="frame", gamma=g)
    for g in (0.0, 0.9):
        refused("gamma", gamma=g)
        refused("gamma", credit="clip", gamma=g)
    m.rollout(batch, N, credit="clip", gamma=1.0)
    clip = list(calls)
    del calls[:]
    m.rollout(batch, N, credit="frame")
    frame = list(calls)
    monkeypatch.undo()
    _reset(m)
    assert "mage_frame_advantages" not in clip and "mage_group_advantages" in clip
    assert frame.count("mage_frame_advantages") == 1 and [c for c in frame if c != "mage_frame_advantages"] == clip


def test_the_documented_loop_runs_as_written(small):
    m, batch = small
    _reset(m)
    ref = copy.deepcopy(m).eval()
    m.set_sampling(TEMP)
    try:
        out = m.rollout(batch, 8, credit='frame', gamma=1.0, reference=ref)
        loss, info = m.policy_loss(out['batch'], out['tokens'], out['advantages'], out['behaviour_logprobs'],
                                   reference_logprobs=out['reference_logprobs'], kl_coef=0.1, given=out['given'])
        loss.backward()
        assert out["advantages"].shape == (B * 8, L - 1) and np.isfinite(info["loss"]) and abs(info["kl"]) < 1e-3      # the reference is a copy
        assert sum(p.grad is not None for p in m.parameters()) >= 90
    finally:
        _reset(m)


@pytest.mark.parametrize("way", ["plain", "anchored", "given"])
def test_policy_loss_takes_one_advantage_per_frame(small, rolled, way):
    m, _ = small
    out = rolled["frame_ctx"] if way == "given" else rolled["frame"]
    R_ = m.image_resolution
    adv = out["advantages"]
    per_token = adv[:, :, None, None].expand(B * N, L - 1, R_, R_).contiguous()
    kw = {"plain": {},
          "anchored": dict(behaviour_logprobs=out["behaviour_logprobs"], reference_logprobs=(out["behaviour_logprobs"] - 0.05).contiguous(), kl_coef=0.1),
          "given": dict(behaviour_logprobs=out["behaviour_logprobs"], given=out["given"])}[way]
    _reset(m)
    m.set_sampling(TEMP)
    try:
        res = []
        for a in (adv, per_token):
            loss, info = m.policy_loss(out["batch"], out["tokens"], a, **kw)
            loss.backward()
            res.append((loss.detach(), info, m.last_policy_token_logprobs, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
            m.zero_grad(set_to_none=True)
        (l0, i0, t0, g0), (l1, i1, t1, g1) = res
        assert torch.equal(_bits(l0), _bits(l1)) and i0 == i1 and torch.equal(_bits(t0), _bits(t1)) and np.isfinite(i0["loss"])
        assert g0.keys() == g1.keys() and len(g0) >= 90 and all(torch.equal(_bits(g0[n]), _bits(g1[n])) for n in g0)
        assert any(bool(g.abs().max() > 0) for g in g0.values())
        with pytest.raises(ValueError, match=r"advantages must be fp32 \[9\], \[9, 4\] or \[9, 4, "):
            m.policy_loss(out["batch"], out["tokens"], adv[:, :3].contiguous(), **kw)
    finally:
        _reset(m)
