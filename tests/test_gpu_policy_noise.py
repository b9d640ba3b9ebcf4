"""GPU: policy-gradient fine-tuning on randomness=True models -- the seeded, recorded generation-time noise (batch['noise_seed'],
last_video_noise), MAGE.policy_loss conditioned on it (gradients against autograd through the oracle's motion_anchor with the same noise),
rollout(noise='clip' | 'candidate') and a short optimisation loop.  The model is tests/test_gpu_train.py's small CATER one (R = 16,
128 x 128 f8 frames) at L = 4; fp32 mode and eval() throughout."""
import copy

import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from oracle import mage_oracle as O
from tests.helpers import build_mage, cpu_sd
from tests.test_gpu_policy_train import GRAD_TOL, dev_batch, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, N, TEMP = 4, 2, 3, 0.9
SMALL = dict(width=64, layers=3, vq_dim=32, K=64)
SEEDS, NOISE_SEEDS = [21, 40], [7, -3]
KL_BOUND = 1e-3             # test_on_policy_ratios_are_one's (tests/test_gpu_policy_train.py): both passes are held to 1e-4 logits against the
                            # oracle, two paths x (logit + log-sum-exp) = 4e-4, with 2.5x margin


def i64(v):
    return torch.tensor(v, dtype=torch.int64)


@pytest.fixture(scope="module")
def cater():
    m = build_mage(synth.cater_model_config(frames_length=L, **SMALL), 61, DEV)
    m.use_graph = False
    return m, dev_batch(synth.synth_batch_cater(B, L, seed=61, text_len=9))


def _reset(m):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32")
    m.use_graph, m.streams, m.ar_mode = False, 1, "full"
    m.eval()
    m.zero_grad(set_to_none=True)


def _generate(m, batch, **keys):
    """One sampled generation with policy log-probabilities: (video, tokens, behaviour log-probabilities, the noise it used)."""
    m.set_sampling(TEMP).set_logprobs(True, policy=True)
    video = m.autoregressive_generate({**batch, **{k: (i64(v) if isinstance(v, list) else v) for k, v in keys.items()}})
    return video, m.last_tokens.clone(), m.last_token_policy_logprobs.clone(), m.last_video_noise


# ---------------------------------------------------------------------------------------------------------------- gradients
def oracle_policy(sd, batch, tokens, adv_rows, noise, T, clip, c, seed, kl_coef):
    """tests/test_gpu_policy_train.py's oracle_policy with the motion anchor modulated by `noise` (O.motion_anchor(..., noise)) and,
    with kl_coef > 0, the k3 penalty against reference log-probabilities r = the oracle's own + noise of +-0.3."""
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.startswith("first_stage_model.") else v) for k, v in sd.items()}
    tok0 = O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, 0])
    tok = torch.cat([tok0[:, None], tokens], 1)
    ma = O.motion_anchor(sd, tok0, batch["text"], batch.get("speed"), noise)
    logits = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, tok[:, :L - 1]))
    K = logits.shape[-1]
    s = logits.reshape(-1, K) * float(np.float32(1.0 / float(np.float32(T))))
    logp = torch.log_softmax(s, -1)
    lp = logp.gather(1, tokens.reshape(-1, 1))[:, 0]
    ent = -(logp.exp() * logp).sum(-1)
    lo, hi = 1.0 - clip, 1.0 + clip
    g = torch.Generator().manual_seed(seed)
    jit = (torch.rand(lp.shape, generator=g) * 2 - 1) * 0.4
    for _ in range(8):
        rho = (-jit).exp()
        near = ((rho / lo - 1).abs() < 1e-2) | ((rho / hi - 1).abs() < 1e-2)
        jit[near] = ((torch.rand(lp.shape, generator=g) * 2 - 1) * 0.4)[near]
    assert not near.any()
    b = (lp.detach() + jit).float()
    rho = (lp - b).exp()
    loss = (-torch.minimum(rho * adv_rows, rho.clamp(lo, hi) * adv_rows) - c * ent).mean()
    r = None
    if kl_coef:
        r = (lp.detach() + (torch.rand(lp.shape, generator=g) * 2 - 1) * 0.3).float()
        d = r - lp
        loss = loss + kl_coef * (d.exp() - d - 1).mean()
    names = [k for k, v in sd.items() if v.requires_grad]
    gs = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)
    return loss.item(), dict(zip(names, gs)), b, r


@pytest.mark.parametrize("kl_coef", [0.0, 0.1])
def test_policy_gradients_match_oracle_autograd_under_the_recorded_noise(kl_coef):
    """Temperature 1.3, no filter, per-clip advantages of mixed sign; every trainable tensor within GRAD_TOL of its reference tensor's
    largest entry.  The Conv3d video prior and its two heads are not part of this policy (generation never runs them): exact zeros."""
    T, clip, c, seed = 1.3, 0.2, 0.01, 71
    m = build_mage(synth.cater_model_config(frames_length=L, **SMALL), seed, DEV)
    batch = synth.synth_batch_cater(B, L, seed=seed, text_len=9)
    R, K = m.image_resolution, m.codebook_size
    g = torch.Generator().manual_seed(seed + 1)
    tokens = torch.randint(0, K, (B, L - 1, R, R), generator=g)
    noise = torch.randn(B, 64, R, R, generator=g)
    adv = torch.tensor([0.8, -1.1])
    want_loss, want, b, r = oracle_policy(cpu_sd(m), batch, tokens, adv.repeat_interleave((L - 1) * R * R), noise, T, clip, c, seed + 2, kl_coef)
    m.set_sampling(T)
    db = {**dev_batch(batch), "video_noise": noise.to(DEV)}
    kw = dict(reference_logprobs=r.view(B, L - 1, R, R).to(DEV), kl_coef=kl_coef) if kl_coef else {}
    loss, info = m.policy_loss(db, tokens.to(DEV), adv.to(DEV), b.view(B, L - 1, R, R).to(DEV), clip=clip, entropy_coef=c, **kw)
    m.set_sampling(None)
    print(f"kl_coef {kl_coef}: loss {loss.item():.6f} want {want_loss:.6f}; info {info}")
    assert abs(loss.item() - want_loss) < 1e-4 and loss.requires_grad
    loss.backward()
    gmax = max(v.abs().max().item() for v in want.values() if v is not None)
    worst, checked = ("", 0.0), set()
    for name, p in m.named_parameters():
        if name.startswith("first_stage_model."):
            assert p.grad is None
            continue
        g_ref = want.get(name)
        assert p.grad is not None, name
        if name.startswith(("conv3d.", "conv_mu2.", "conv_var2.")):
            assert g_ref is None and p.grad.abs().max().item() == 0.0, name
            continue
        if g_ref is None or g_ref.abs().max().item() == 0.0:
            assert p.grad.abs().max().item() == 0.0, name
            continue
        if name == "ma_encoder.blocks.0.mlp.c_proj.bias":
            # a per-channel constant in front of ADAIN's instance norm: the exact gradient is zero, the reference's is rounding noise
            # (tests/test_gpu_train.py bounds it the same way)
            assert g_ref.abs().max().item() < 1e-6 * gmax and p.grad.abs().max().item() < 1e-6 * gmax, name
            continue
        e = rel(p.grad, g_ref)
        checked.add(name)
        if e > worst[1]:
            worst = (name, e)
    print(f"{len(checked)} gradients checked, worst relative error {worst[1]:.2e} at {worst[0]}")
    assert worst[1] < GRAD_TOL, worst
    branch = {n for n in checked if n.startswith("adain.")} | ({"conv_d2.weight"} & checked)
    assert len(branch) == 9 and len(checked) >= 60, sorted(branch)


# ---------------------------------------------------------------------------------------------------------------- on-policy ratio
def test_on_policy_ratio_is_one_only_under_the_recorded_noise(cater):
    m, batch = cater
    _reset(m)
    _, tokens, blp, vn = _generate(m, batch, sample_seed=SEEDS, noise_seed=NOISE_SEEDS)
    assert vn.shape == (B, 64, 16, 16) and vn.dtype == torch.float32
    adv = torch.tensor([1.0, -0.5], device=DEV)
    with torch.no_grad():
        loss, info = m.policy_loss({**batch, "video_noise": vn}, tokens, adv, blp)
        other, _ = ops.video_noise(i64([n + 1000 for n in NOISE_SEEDS]).to(DEV), C=64, h=16, w=16, rows=False)
        _, off = m.policy_loss({**batch, "video_noise": other}, tokens, adv, blp)
    _reset(m)
    print(f"approx_kl under the recorded noise {info['approx_kl']:.3e}, under another draw {off['approx_kl']:.3e}")
    assert not loss.requires_grad and abs(info["approx_kl"]) < KL_BOUND and info["outside_fraction"] == 0.0
    assert abs(off["approx_kl"]) > 10 * abs(info["approx_kl"])                          # the noise reaches the pass


def test_policy_loss_needs_the_noise(cater):
    m, batch = cater
    _reset(m)
    tokens = torch.zeros(B, L - 1, 16, 16, dtype=torch.int64, device=DEV)
    adv = torch.ones(B, device=DEV)
    good = torch.zeros(B, 64, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="randomness=True.*last_video_noise"):
        m.policy_loss(batch, tokens, adv)
    with pytest.raises(ValueError, match="randomness=True"):
        m.token_policy_logprobs(batch, tokens)
    for bad in (good[:1], good[:, :32], good.double(), good.cpu(), good.permute(0, 2, 3, 1)):
        with pytest.raises(ValueError, match="video_noise"):
            m.policy_loss({**batch, "video_noise": bad}, tokens, adv)


# ---------------------------------------------------------------------------------------------------------------- generation
def test_noise_seed_makes_generation_repeatable_and_recorded(cater):
    m, batch = cater
    _reset(m)
    video, tokens, _, vn = _generate(m, batch, sample_seed=SEEDS, noise_seed=NOISE_SEEDS)
    video2, tokens2, _, vn2 = _generate(m, batch, sample_seed=SEEDS, noise_seed=NOISE_SEEDS)
    assert torch.equal(video, video2) and torch.equal(tokens, tokens2) and torch.equal(vn, vn2)
    want, _ = ops.video_noise(i64(NOISE_SEEDS).to(DEV), C=64, h=16, w=16, rows=False)
    assert torch.equal(vn, want)
    flipped = {k: v.flip(0) for k, v in batch.items()}                                  # the same clips at other batch positions
    video3, tokens3, _, vn3 = _generate(m, flipped, sample_seed=SEEDS[::-1], noise_seed=NOISE_SEEDS[::-1])
    assert torch.equal(video3.flip(0), video) and torch.equal(tokens3.flip(0), tokens) and torch.equal(vn3.flip(0), vn)
    # the recorded noise, injected, reproduces the call; an injected tensor wins over a seed
    video4, tokens4, _, vn4 = _generate(m, batch, sample_seed=SEEDS, video_noise=vn.clone(), noise_seed=[99, 98])
    assert torch.equal(video4, video) and torch.equal(tokens4, tokens) and torch.equal(vn4, vn)
    _, tokens5, _, _ = _generate(m, batch, sample_seed=SEEDS, noise_seed=[99, 98])
    assert not torch.equal(tokens5, tokens)
    # the other call paths: two streams (noise_seed sliced per group as sample_seed is), the incremental loop
    four = {k: torch.cat([v, v], 0) for k, v in batch.items()}
    m.streams = 2
    video6, tokens6, _, vn6 = _generate(m, four, sample_seed=SEEDS + SEEDS, noise_seed=NOISE_SEEDS + NOISE_SEEDS)
    m.streams, m._side_streams = 1, None                                                # (the side streams: not kept for the other tests)
    assert torch.equal(tokens6, torch.cat([tokens, tokens], 0)) and torch.equal(vn6, torch.cat([vn, vn], 0))
    m.ar_mode = "incremental"
    _, tokens7, _, vn7 = _generate(m, batch, sample_seed=SEEDS, noise_seed=NOISE_SEEDS)
    assert torch.equal(tokens7, tokens) and torch.equal(vn7, vn)
    _reset(m)


def test_unseeded_noise_is_recorded_too(cater):
    m, batch = cater
    _reset(m)
    video, tokens, _, vn = _generate(m, batch, sample_seed=SEEDS)                      # neither key: torch.randn, as before
    assert vn is not None and vn.shape == (B, 64, 16, 16) and vn.dtype == torch.float32 and 0.9 < vn.std().item() < 1.1
    vn = vn.clone()
    video2, tokens2, _, _ = _generate(m, batch, sample_seed=SEEDS, video_noise=vn)
    assert torch.equal(video2, video) and torch.equal(tokens2, tokens)
    _reset(m)


def test_graph_replay_equals_eager_bit_for_bit(cater):
    m, batch = cater
    _reset(m)
    one = {k: v[:1].contiguous() for k, v in batch.items()}
    keys = dict(sample_seed=SEEDS[:1], noise_seed=NOISE_SEEDS[:1])
    video, tokens, blp, vn = _generate(m, one, **keys)
    assert m.last_call_mode == "eager"
    m.use_graph = True
    for _ in range(3):                                                                  # eager (warm), capture + replay, replay
        got = _generate(m, one, **keys)
    mode = m.last_call_mode
    m._graphs.clear()                                                                   # (the captured graph and its arena: not kept for the other tests)
    _reset(m)
    assert mode == "graph"
    assert torch.equal(got[0], video) and torch.equal(got[1], tokens) and torch.equal(got[2], blp) and torch.equal(got[3], vn)


def test_noise_seed_is_ignored_without_the_branch():
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 41, DEV)
    m.use_graph = False
    batch = dev_batch(synth.synth_batch_mnist(B, L, seed=41, text_len=9))
    m.set_sampling(TEMP)
    a = m.autoregressive_generate({**batch, "sample_seed": i64(SEEDS)})
    ta = m.last_tokens.clone()
    b = m.autoregressive_generate({**batch, "sample_seed": i64(SEEDS), "noise_seed": i64(NOISE_SEEDS)})
    assert torch.equal(a, b) and torch.equal(ta, m.last_tokens) and m.last_video_noise is None
    with pytest.raises(ValueError, match="randomness=False"):
        m.rollout({**batch, "sample_seed": i64(SEEDS)}, N, noise="candidate")


def test_the_latent_path_takes_noise_seed_too():
    """use_cids=False (MAGE+): the noise is read in the same place; seeded it equals the same tensor injected."""
    m = build_mage(synth.magep_model_config(frames_length=L, width=64, layers=3), 77, DEV)
    batch = dev_batch(synth.synth_batch_cater(B, L, seed=77, text_len=9, vocab=50))
    a = m.autoregressive_generate({**batch, "noise_seed": i64(NOISE_SEEDS)})
    vn, pred = m.last_video_noise, m.last_logits.clone()
    want, _ = ops.video_noise(i64(NOISE_SEEDS).to(DEV), C=64, h=m.image_resolution, w=m.image_resolution, rows=False)
    assert torch.equal(vn, want)
    b = m.autoregressive_generate({**batch, "video_noise": vn.clone()})
    assert torch.equal(a, b) and torch.equal(pred, m.last_logits) and torch.equal(m.last_video_noise, vn)
    c = m.autoregressive_generate({**batch, "noise_seed": i64([5, 6])})
    assert not torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------- rollout
@pytest.fixture(scope="module")
def rolled(cater):
    m, batch = cater
    _reset(m)
    m.set_sampling(TEMP)
    out = m.rollout({**batch, "sample_seed": i64(SEEDS)}, N, noise="candidate")
    _reset(m)
    return out


def test_candidate_rows_are_single_generations_with_their_own_noise(cater, rolled):
    m, batch = cater
    out = rolled
    assert out["video_noise"].shape == (B * N, 64, 16, 16) and out["video_noise"].dtype == torch.float32
    assert out["batch"]["video_noise"] is out["video_noise"] and "noise_seed" not in out["batch"]
    assert out["seeds"].tolist() == [s + c for s in SEEDS for c in range(N)]
    _reset(m)
    for c in range(N):
        seeds = [s + c for s in SEEDS]
        video, tokens, blp, vn = _generate(m, batch, sample_seed=seeds, noise_seed=seeds)
        rows = torch.arange(B, device=DEV) * N + c
        assert torch.equal(out["tokens"][rows], tokens), c
        assert torch.equal(out["video_noise"][rows], vn) and torch.equal(out["video"][rows], video), c
        assert torch.equal(out["behaviour_logprobs"][rows], blp), c
    _reset(m)
    for b in range(B):
        for i in range(N):
            for j in range(i + 1, N):
                assert not torch.equal(out["video_noise"][b * N + i], out["video_noise"][b * N + j])


def test_clip_mode_is_the_shared_noise_rollout_plus_the_noise(cater):
    m, batch = cater
    _reset(m)
    m.set_sampling(TEMP)
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(B, 64, 16, 16, generator=g).to(DEV)
    full = {**batch, "sample_seed": i64(SEEDS), "video_noise": noise}
    out = m.rollout(full, N)
    explicit = m.rollout(full, N, noise="clip")
    assert all(torch.equal(out[k], explicit[k]) for k in ("video", "tokens", "behaviour_logprobs", "token_logprobs", "rewards", "advantages"))
    assert torch.equal(out["video_noise"], noise.repeat_interleave(N, 0)) and torch.equal(out["batch"]["video_noise"], out["video_noise"])
    # its rows are the shared-noise candidates: candidate c of every clip under the injected noise and seed + c
    for c in range(N):
        video, tokens, blp, _ = _generate(m, batch, sample_seed=[s + c for s in SEEDS], video_noise=noise)
        rows = torch.arange(B, device=DEV) * N + c
        assert torch.equal(out["tokens"][rows], tokens) and torch.equal(out["video"][rows], video), c
        assert torch.equal(out["behaviour_logprobs"][rows], blp), c
    m.set_sampling(TEMP).set_logprobs(False)
    seeded = m.rollout({**batch, "sample_seed": i64(SEEDS), "noise_seed": i64(NOISE_SEEDS)}, N)
    want, _ = ops.video_noise(i64(NOISE_SEEDS).to(DEV), C=64, h=16, w=16, rows=False)
    assert torch.equal(seeded["video_noise"], want.repeat_interleave(N, 0))
    _reset(m)


def test_policy_loss_consumes_the_rollout(cater, rolled):
    m, _ = cater
    out = rolled
    _reset(m)
    m.set_sampling(TEMP)
    loss, info = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"])
    print(f"policy_loss on a candidate-noise rollout: {info}")
    assert abs(info["approx_kl"]) < KL_BOUND and info["outside_fraction"] == 0.0
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if not n.startswith("first_stage_model.")}
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert grads["conv_d2.weight"].abs().max().item() > 0 and grads["adain.conv_mu.0.weight"].abs().max().item() > 0
    assert grads["conv_mu2.weight"].abs().max().item() == 0.0
    _reset(m)


def test_the_reference_scores_under_the_same_noise(cater):
    m, batch = cater
    _reset(m)
    m.set_sampling(TEMP)
    out = m.rollout({**batch, "sample_seed": i64(SEEDS)}, N, noise="candidate", reference=copy.deepcopy(m))
    _reset(m)
    d = (out["reference_logprobs"] - out["behaviour_logprobs"]).abs().max().item()
    print(f"max |reference - behaviour| log-probability {d:.3e}")
    assert d < KL_BOUND


def test_rollout_refusals(cater):
    m, batch = cater
    _reset(m)
    m.set_sampling(TEMP)
    full = {**batch, "sample_seed": i64(SEEDS)}
    before = m.last_video_noise
    with pytest.raises(ValueError, match="video_noise"):
        m.rollout({**full, "video_noise": torch.zeros(B, 64, 16, 16, device=DEV)}, N, noise="candidate")
    for bad in ("frame", None, True):
        with pytest.raises(ValueError, match="noise must be"):
            m.rollout(full, N, noise=bad)
    assert m.last_video_noise is before
    _reset(m)


# ---------------------------------------------------------------------------------------------------------------- loop
def _loop(seed):
    m = build_mage(synth.cater_model_config(frames_length=L, **SMALL), seed, DEV)
    m.use_graph = False
    batch = dev_batch(synth.synth_batch_cater(B, L, seed=seed, text_len=9))
    m.set_sampling(1.0)
    opt = FlatAdam(m.parameters(), lr=1e-4, max_grad_norm=1.0)
    losses, norms = [], []
    for step in range(20):
        out = m.rollout({**batch, "sample_seed": i64([100 * step + 1, 100 * step + 50])}, N, noise="candidate")
        opt.zero_grad()
        loss, _ = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"])
        loss.backward()
        opt.step()
        losses.append(loss.item())
        norms.append(opt.last_grad_norm.item())
    return losses, norms


def test_twenty_rollout_steps_are_finite_and_repeat_bit_for_bit():
    losses, norms = _loop(83)
    print(f"losses first {losses[0]:.6e} last {losses[-1]:.6e}; gradient norms min {min(norms):.3e} max {max(norms):.3e}")
    assert all(np.isfinite(v) for v in losses) and all(np.isfinite(v) and v > 0 for v in norms)
    assert _loop(83)[0][-1] == losses[-1]
