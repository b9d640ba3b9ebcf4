"""GPU: MAGE.rollout -- its candidates against set_sampling(candidates=N)'s (the same B * N rows through the same code), its rewards and
advantages against their restatement (tests/video_metrics_ref.py), its output consumed by MAGE.policy_loss, the settings it must leave
alone, a callable reward, the refusals and a bf16 run.  The model is tests/test_gpu_policy_train.py's small one."""
import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.utils import synth
from tests import video_metrics_ref as R
from tests.helpers import build_mage, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, N, TEMP = 5, 3, 3, 0.9
SEEDS = [11, 12, 13]


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), 41, DEV)
    batch = dev_batch({**synth.synth_batch_mnist(B, L, seed=41, text_len=9, ragged_text=True), "sample_seed": torch.tensor(SEEDS, dtype=torch.int64)})
    return m, batch


def _reset(m, ar_mode="full"):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32")
    m.ar_mode = ar_mode
    m.eval()
    m.zero_grad(set_to_none=True)


@pytest.fixture(scope="module")
def rolled(small):
    """One rollout per ar_mode, shared (and left unchanged) by the tests below."""
    m, batch = small
    out = {}
    for mode in ("full", "incremental"):
        _reset(m, mode)
        m.set_sampling(TEMP)
        out[mode] = m.rollout(batch, N)
    _reset(m)
    return out


@pytest.mark.parametrize("ar_mode", ["full", "incremental"])
def test_candidates_are_best_of_n_s(small, rolled, ar_mode):
    m, batch = small
    out = rolled[ar_mode]
    R_ = m.image_resolution
    assert out["video"].shape == (B * N, L, *batch["images"].shape[2:]) and out["video"].dtype == torch.float32
    assert out["tokens"].shape == (B * N, L - 1, R_, R_) and out["tokens"].dtype == torch.int64
    assert out["behaviour_logprobs"].shape == out["tokens"].shape == out["token_logprobs"].shape
    assert out["rewards"].shape == (B, N) and out["advantages"].shape == (B * N,) and out["seeds"].shape == (B * N,)
    assert out["seeds"].tolist() == [s + c for s in SEEDS for c in range(N)]
    assert torch.equal(out["batch"]["text"], batch["text"].repeat_interleave(N, 0)) and out["batch"]["images"].shape[:2] == (B * N, 1)
    assert torch.equal(out["batch"]["images"][:, 0], batch["images"][:, 0].repeat_interleave(N, 0))
    assert torch.equal(out["video"][:, 0], out["batch"]["images"][:, 0])
    _reset(m, ar_mode)
    m.set_sampling(TEMP, candidates=N).set_logprobs(True, policy=True)
    video = m.autoregressive_generate(batch)
    best = m.last_candidate_index
    rows = torch.arange(B, device=DEV) * N + best
    assert torch.equal(m.last_tokens, out["tokens"][rows])
    assert torch.equal(m.last_token_logprobs, out["token_logprobs"][rows])
    assert torch.equal(m.last_token_policy_logprobs, out["behaviour_logprobs"][rows])
    scores, pick = ops.clip_scores(out["token_logprobs"].contiguous(), n_clips=B, n_cand=N)
    pscores, _ = ops.clip_scores(out["behaviour_logprobs"].contiguous(), n_clips=B, n_cand=N)
    assert torch.equal(scores.view(torch.int32), m.last_candidate_scores.view(torch.int32)) and torch.equal(pick, best)
    assert torch.equal(pscores.view(torch.int32), m.last_candidate_policy_scores.view(torch.int32))
    assert torch.equal(video, out["video"][rows])
    assert len({tuple(t.flatten().tolist()) for t in out["tokens"][:N]}) > 1            # the candidates of a clip differ
    _reset(m)


@pytest.mark.parametrize("ar_mode", ["full", "incremental"])
@pytest.mark.parametrize("reward,normalize", [("ssim", "std"), ("psnr", "mean"), ("neg_mse", None)])
def test_rewards_and_advantages(small, rolled, ar_mode, reward, normalize):
    m, batch = small
    _reset(m, ar_mode)
    m.set_sampling(TEMP)
    out = rolled[ar_mode] if (reward, normalize) == ("ssim", "std") else m.rollout(batch, N, reward=reward, normalize=normalize, eps=1e-6)
    _reset(m)
    base = rolled[ar_mode]
    assert torch.equal(out["tokens"], base["tokens"]) and torch.equal(out["video"], base["video"])
    fm = out["frame_metrics"]
    truth = batch["images"].repeat_interleave(N, 0)
    direct = m.video_metrics(out["video"][:, 1:], truth[:, 1:])
    assert set(fm) == set(direct) == {"mse", "psnr", "ssim"}
    assert all(fm[k].shape == (B * N, L - 1) and torch.equal(fm[k].view(torch.int32), direct[k].view(torch.int32)) for k in fm)
    v, t = out["video"][:, 1:].cpu().numpy(), batch["images"][:, 1:].cpu().numpy()
    ref = R.metrics(v, t, tgt_div=N)
    naive = np.abs(R.metrics(v, t, tgt_div=N, dtype=np.float32)["ssim"].astype(np.float64) - ref["ssim"]).max()
    e = np.abs(fm["ssim"].cpu().numpy().astype(np.float64) - ref["ssim"]).max()
    um = R.ulps(fm["mse"].cpu().numpy(), ref["mse"].astype(np.float32)).max()
    up = R.ulps(fm["psnr"].cpu().numpy(), ref["psnr"].astype(np.float32)).max()
    print(f"{ar_mode}: ssim error {e:.3e} (naive fp32 on these frames {naive:.3e}), mse {um:.2f} ulp, psnr {up:.2f} ulp; "
          f"rewards {out['rewards'].cpu().numpy().round(4).tolist()}")
    assert e <= 4 * naive and um <= 2 and up <= 2                                     # tests/test_gpu_video_metrics.py's bounds
    fr = {"ssim": fm["ssim"], "psnr": fm["psnr"], "neg_mse": -fm["mse"]}[reward].cpu().numpy()
    mode = 1 if normalize == "std" else 0
    want_r, want_a = R.group_advantages(fr, B, N, mode, 1e-6)
    assert R.ulps(out["rewards"].cpu().numpy(), want_r).max() <= 2
    got_a = out["advantages"].cpu().numpy().astype(np.float64)
    if normalize is None:
        assert torch.equal(out["advantages"], out["rewards"].reshape(-1))
    else:
        assert np.all(np.abs(got_a - want_a) <= 2 * np.spacing(np.abs(want_a).astype(np.float32)) + 1e-14)
        assert np.abs(got_a).max() > 0


@pytest.mark.parametrize("ar_mode", ["full", "incremental"])
def test_policy_loss_consumes_it(small, rolled, ar_mode):
    """The bound and the reasoning of test_on_policy_ratios_are_one (tests/test_gpu_policy_train.py): both passes are held to 1e-4 logits
    against the oracle, two paths x (logit + log-sum-exp) = 4e-4, with 2.5x margin: 1e-3."""
    m, _ = small
    out = rolled[ar_mode]
    _reset(m, ar_mode)
    m.set_sampling(TEMP)
    with torch.no_grad():
        loss, info = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"])
    d = (m.last_policy_token_logprobs - out["behaviour_logprobs"]).abs().max().item()
    print(f"{ar_mode}: max |teacher-forced - rollout| policy log-probability {d:.3e}; info {info}")
    assert not loss.requires_grad and d < 1e-3 and info["clip_fraction"] == 0.0 and info["outside_fraction"] == 0.0
    loss, _ = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"])
    loss.backward()
    n = 0
    for name, p in m.named_parameters():
        if name.startswith("first_stage_model."):
            assert p.grad is None
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            n += 1
    assert n >= 90
    _reset(m)


def _settings(m):
    return (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.precision, m.ar_mode, m.use_graph, m.streams)


def test_settings_and_results_are_left_alone(small, rolled):
    m, batch = small
    _reset(m)
    m.autoregressive_generate(batch)
    greedy = m.last_tokens.clone()
    m.set_sampling(TEMP, top_k=20, candidates=2).set_logprobs(True, entropy=True)
    m.autoregressive_generate(batch)
    before = _settings(m)
    last = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    out = m.rollout(batch, N)
    assert _settings(m) == before
    now = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    assert now.keys() == last.keys() and all(now[a] is last[a] for a in last)
    assert not torch.equal(out["tokens"], rolled["full"]["tokens"])                     # (top_k = 20 was honoured)
    with pytest.raises(ValueError, match="reward callable"):                           # a failure after the generation restores them too
        m.rollout(batch, N, reward=lambda v, b: torch.zeros(B, device=DEV))
    assert _settings(m) == before and all(getattr(m, a) is last[a] for a in last)
    _reset(m)
    m.autoregressive_generate(batch)
    assert torch.equal(m.last_tokens, greedy)


def test_a_callable_reward_reaches_the_advantages(small, rolled):
    m, batch = small
    _reset(m)
    m.set_sampling(TEMP)
    seen = {}

    def brightness(video, b):
        seen["video"], seen["batch"] = video, b
        return video[:, 1:].mean(dim=(1, 2, 3, 4))
    out = m.rollout(batch, N, reward=brightness, normalize="mean")
    _reset(m)
    assert seen["video"] is out["video"] and seen["batch"] is out["batch"] and out["frame_metrics"] is None
    assert torch.equal(out["tokens"], rolled["full"]["tokens"])
    r = out["video"][:, 1:].mean(dim=(1, 2, 3, 4))
    assert torch.equal(out["rewards"], r.view(B, N))                                   # T = 1: the mean of one value
    want = R.group_advantages(r.cpu().numpy().reshape(B * N, 1), B, N, 0, 0.0)[1]
    got = out["advantages"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want).astype(np.float32)) + 1e-14) and np.abs(got).max() > 0


def test_refusals_launch_nothing(small, monkeypatch):
    m, batch = small
    _reset(m)
    calls = count_lib_calls(monkeypatch)

    def refused(match, *a, **kw):
        before = _settings(m)
        with pytest.raises(ValueError, match=match):
            m.rollout(*a, **kw)
        assert calls == [] and _settings(m) == before
    refused("set_sampling", batch, N)
    m.set_sampling(TEMP)
    m.use_cids = False
    refused("use_cids=False", batch, N)
    m.use_cids = True
    for n in (1, 0, 2.5, True):
        refused("candidates", batch, n)
    refused("reward", batch, N, reward="fvd")
    refused("normalize", batch, N, normalize="rank")
    refused("eps", batch, N, eps=-1.0)
    refused("eps", batch, N, eps=float("nan"))
    refused("ground truth", {**batch, "images": batch["images"][:, :1]}, N)
    refused("ground truth", {**batch, "images": batch["images"][:, :L - 1]}, N, reward="psnr")
    refused("GPU", {**batch, "images": batch["images"].cpu()}, N)
    refused("GPU", {**batch, "text": batch["text"].cpu()}, N)
    x = batch["images"]
    for match, a, kw in (("GPU", (x.cpu(), x.cpu()), {}), ("GPU", (x, x.cpu()), {}), ("same shape", (x, x[:, 1:]), {}), ("fp32", (x.double(), x.double()), {}),
                         ("11", (x[..., :10, :], x[..., :10, :]), {}), ("data_range", (x, x), dict(data_range=0.0))):
        with pytest.raises(ValueError, match=match):
            m.video_metrics(*a, **kw)
        assert calls == []
    monkeypatch.undo()
    _reset(m)


def test_bf16_rollout_runs(small):
    m, batch = small
    _reset(m)
    m.set_precision("bf16").set_sampling(TEMP)
    out = m.rollout(batch, N)
    _reset(m)
    assert out["video"].shape[:2] == (B * N, L) and out["tokens"].shape[0] == B * N and out["rewards"].shape == (B, N)
    for k in ("video", "behaviour_logprobs", "token_logprobs", "rewards", "advantages"):
        assert torch.isfinite(out[k].float()).all(), k
    assert out["rewards"].min().item() >= -1.0 and out["rewards"].max().item() <= 1.0
    assert all(torch.isfinite(v).all() for v in out["frame_metrics"].values())
