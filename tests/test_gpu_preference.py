"""GPU: MAGE.preference_loss end to end on tests/test_gpu_policy_train.py's small model (L = 5, 4 clips, pairs (0, 1), (2, 3), (0, 3), fp32 mode,
eval()).  The loss is split so that every tolerance is one the project already holds:
  clip log-likelihoods   against the oracle's sums, within (L - 1) hw 2e-4: the 1e-4 logit gate on the logit and on the log-sum-exp of every
                         one of a clip's (L - 1) hw tokens, summed;
  the pair stage         against tests/preference_ref.py evaluated at the GPU's OWN clip log-likelihoods, within the kernel bounds;
  parameter gradients    against autograd through the oracle of sum_c coef_c S_c(theta), coef the GPU's coefficients and S_c the oracle's clip
                         log-likelihood: the reward-weighted-likelihood class tests/test_gpu_policy_train.py holds to GRAD_TOL = 1e-4.
Then: a neutral reference, grad mode against no-grad, clip_logprobs, the sampler's settings (no effect), ten optimisation steps, a
randomness=True model, bf16 mode, rollout(pairs='best_worst') and the refusals."""
import collections

import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from oracle import mage_oracle as O
from tests import preference_ref as R
from tests.helpers import build_mage, count_lib_calls, cpu_sd, within
from tests.test_gpu_policy_train import GRAD_TOL, SMALL, dev_batch, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B = 5, 4
PAIRS = [[0, 1], [2, 3], [0, 3]]
LOG2 = float(np.float32(np.log(2.0)))
LAST = ("last_preference_clip_logprobs", "last_preference_clip_coef", "last_preference_pair_loss", "last_preference_pair_margin",
        "last_preference_token_logprobs")


def oracle_clip_logprobs(sd, batch, tokens, noise=None, frames=L):
    """S_c: the sum over a clip's generated tokens of the log-softmax of the oracle's teacher-forced logits (temperature 1, no filter)."""
    tok0 = O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, 0])
    tok = torch.cat([tok0[:, None], tokens], 1)
    extra = () if noise is None else (noise,)
    ma = O.motion_anchor(sd, tok0, batch["text"], batch.get("speed"), *extra)
    logits = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, tok[:, :frames - 1]))
    logp = torch.log_softmax(logits.reshape(-1, logits.shape[-1]), -1)
    return logp.gather(1, tokens.reshape(-1, 1))[:, 0].view(tokens.shape[0], -1).sum(1)


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 41, DEV)
    ref = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 42, DEV)          # a "frozen reference": other weights, so u != 0
    batch = synth.synth_batch_mnist(B, L, seed=41, text_len=9, ragged_text=True)
    R_, K = m.image_resolution, m.codebook_size
    tokens = torch.randint(0, K, (B, L - 1, R_, R_), generator=torch.Generator().manual_seed(43))
    b, tok, pairs = dev_batch(batch), tokens.to(DEV), torch.tensor(PAIRS, device=DEV)
    ref_lp = ref.clip_logprobs(b, tok)
    return dict(m=m, ref=ref, batch=batch, b=b, tokens=tokens, tok=tok, pairs=pairs, ref_lp=ref_lp)


def _reset(m):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32")
    m.eval()
    m.zero_grad(set_to_none=True)


def _kept(m):
    return {a: getattr(m, a).clone() for a in LAST}


def test_values_and_gradients_against_the_oracle(small):
    m, b, tok, pairs, ref_lp = small["m"], small["b"], small["tok"], small["pairs"], small["ref_lp"]
    _reset(m)
    loss, info = m.preference_loss(b, tok, pairs, ref_lp, beta=0.1)
    assert loss.requires_grad and info["loss"] == loss.item()
    assert set(info) == {"loss", "accuracy", "chosen_reward", "rejected_reward", "margin"} and all(isinstance(v, float) for v in info.values())
    hw = m.image_resolution ** 2
    s_gpu = m.last_preference_clip_logprobs
    assert s_gpu.shape == (B,) and m.last_preference_clip_coef.shape == (B,) and m.last_preference_pair_loss.shape == (len(PAIRS),)
    assert m.last_preference_pair_margin.shape == (len(PAIRS),) and m.last_preference_token_logprobs.shape == tok.shape
    # clip log-likelihoods
    sd = cpu_sd(m)
    with torch.no_grad():
        s_ref = oracle_clip_logprobs(sd, small["batch"], small["tokens"])
    d = (s_gpu.cpu().double() - s_ref.double()).abs().max().item()
    print(f"clip log-likelihoods {s_gpu.tolist()}: max |GPU - oracle| {d:.3e} (bound {(L - 1) * hw * 2e-4:.3e})")
    assert d < (L - 1) * hw * 2e-4
    assert (m.last_preference_token_logprobs.flatten(1).double().sum(1) - s_gpu.double()).abs().max().item() < 1e-3      # (one fp32 rounding)
    # the pair stage at the GPU's own log-likelihoods
    want = R.pair_stage(s_gpu.cpu().numpy(), ref_lp.cpu().numpy(), PAIRS, 0.1)
    for k, got in (("clip_coef", m.last_preference_clip_coef), ("pair_loss", m.last_preference_pair_loss),
                   ("pair_margin", m.last_preference_pair_margin),
                   ("summary", torch.tensor([info[q] for q in ("loss", "accuracy", "chosen_reward", "rejected_reward", "margin")]))):
        within("MAGE.preference_loss", k, got.float(), torch.from_numpy(want[k]), torch.from_numpy(want[k + "_bound"]))
    assert np.abs(want["u"]).min() > 1e-3                                        # the two models do disagree
    # parameter gradients
    coef = m.last_preference_clip_coef.cpu().double()
    loss.backward()
    sdg = {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.startswith("first_stage_model.") else v) for k, v in sd.items()}
    names = [k for k, v in sdg.items() if v.requires_grad]
    total = (coef * oracle_clip_logprobs(sdg, small["batch"], small["tokens"]).double()).sum()
    gref = dict(zip(names, torch.autograd.grad(total, [sdg[k] for k in names], allow_unused=True)))
    worst, n_checked = ("", 0.0), 0
    for name, p in m.named_parameters():
        if name.startswith("first_stage_model."):
            assert p.grad is None, name
            continue
        g_ref = gref.get(name)
        assert p.grad is not None, name
        if g_ref is None or g_ref.abs().max().item() == 0.0:
            assert p.grad.abs().max().item() == 0.0, name
            continue
        e = rel(p.grad, g_ref)
        n_checked += 1
        if e > worst[1]:
            worst = (name, e)
    print(f"{n_checked} gradients checked, worst relative error {worst[1]:.2e} at {worst[0]}")
    _reset(m)
    assert worst[1] < GRAD_TOL, worst
    assert n_checked >= 90


def test_neutral_reference_is_log_two(small):
    m, b, tok, pairs = small["m"], small["b"], small["tok"], small["pairs"]
    _reset(m)
    own = m.clip_logprobs(b, tok)
    with torch.no_grad():
        loss, info = m.preference_loss(b, tok, pairs, own)
    assert torch.equal(own, m.last_preference_clip_logprobs)
    assert loss.item() == LOG2 and info["loss"] == LOG2 and info["accuracy"] == 0.0 and info["margin"] == 0.0
    assert (m.last_preference_pair_margin == 0).all() and (m.last_preference_pair_loss == LOG2).all()


@pytest.mark.parametrize("kw", [dict(beta=0.1), dict(beta=0.5, label_smoothing=0.1), dict(beta=0.2, loss="ipo")])
def test_grad_mode_no_grad_and_the_sampler_agree_bit_for_bit(small, kw):
    m, b, tok, pairs, ref_lp = small["m"], small["b"], small["tok"], small["pairs"], small["ref_lp"]
    _reset(m)
    loss, info = m.preference_loss(b, tok, pairs, ref_lp, **kw)
    kept = _kept(m)
    held = {a: getattr(m, a) for a in LAST}
    clp = m.clip_logprobs(b, tok)
    assert all(getattr(m, a) is held[a] for a in LAST), "clip_logprobs must leave every last_* as found"
    assert torch.equal(clp, kept["last_preference_clip_logprobs"]) and not clp.requires_grad
    with torch.no_grad():
        loss2, info2 = m.preference_loss(b, tok, pairs, ref_lp, **kw)
    assert loss.requires_grad and not loss2.requires_grad and loss.item() == loss2.item() and info == info2
    assert all(torch.equal(kept[a], getattr(m, a)) for a in LAST)
    m.set_sampling(1.3, top_k=5)                                                 # a preference is about the model: the sampler has no say
    with torch.no_grad():
        loss3, info3 = m.preference_loss(b, tok, pairs, ref_lp, **kw)
    assert loss3.item() == loss.item() and info3 == info and all(torch.equal(kept[a], getattr(m, a)) for a in LAST)
    assert torch.equal(m.clip_logprobs(b, tok), clp)
    _reset(m)
    want = R.pair_stage(kept["last_preference_clip_logprobs"].cpu().numpy(), ref_lp.cpu().numpy(), PAIRS, kw["beta"],
                        kw.get("label_smoothing", 0.0), 1 if kw.get("loss") == "ipo" else 0)
    within("MAGE.preference_loss", f"{kw} clip_coef", kept["last_preference_clip_coef"], torch.from_numpy(want["clip_coef"]),
           torch.from_numpy(want["clip_coef_bound"]))


def test_ten_steps_lower_the_loss_and_raise_the_margin(small):
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 44, DEV)
    b, tok, pairs = small["b"], small["tok"], small["pairs"]
    ref_lp = m.clip_logprobs(b, tok).clone()                                     # the model before fine-tuning: the usual reference
    opt = FlatAdam(m.parameters(), lr=1e-3)                                      # tests/test_gpu_policy_train.py's loop
    hist = []
    for _ in range(10):
        opt.zero_grad()
        loss, info = m.preference_loss(b, tok, pairs, ref_lp, beta=0.1)
        loss.backward()
        opt.step()
        hist.append((loss.item(), info["margin"]))
    with torch.no_grad():
        loss, info = m.preference_loss(b, tok, pairs, ref_lp, beta=0.1)
    print(f"preference loss over 10 FlatAdam steps: {hist[0][0]:.6f} -> {loss.item():.6f}; margin {hist[0][1]:.4f} -> {info['margin']:.4f}")
    assert hist[0] == (LOG2, 0.0)
    assert loss.item() < hist[0][0] and info["margin"] > hist[0][1]


def test_randomness_model_conditions_on_the_recorded_noise():
    Lc, Bc = 4, 2
    m = build_mage(synth.cater_model_config(frames_length=Lc, **SMALL), 61, DEV)
    b = dev_batch(synth.synth_batch_cater(Bc, Lc, seed=61, text_len=9))
    R_, K = m.image_resolution, m.codebook_size
    g = torch.Generator().manual_seed(62)
    tok = torch.randint(0, K, (Bc, Lc - 1, R_, R_), generator=g).to(DEV)
    noise = torch.randn(Bc, 64, R_, R_, generator=g).to(DEV)
    pairs, ref_lp = torch.tensor([[0, 1]], device=DEV), torch.tensor([-3000.0, -2990.0], device=DEV)
    with pytest.raises(ValueError, match="preference_loss: randomness=True.*last_video_noise"):
        m.preference_loss(b, tok, pairs, ref_lp)
    with pytest.raises(ValueError, match="clip_logprobs: randomness=True"):
        m.clip_logprobs(b, tok)
    bn = {**b, "video_noise": noise}
    loss, info = m.preference_loss(bn, tok, pairs, ref_lp)
    assert np.isfinite(loss.item()) and torch.equal(m.clip_logprobs(bn, tok), m.last_preference_clip_logprobs)
    with torch.no_grad():
        other = m.clip_logprobs({**b, "video_noise": noise.flip(0).contiguous()}, tok)
    assert not torch.equal(other, m.last_preference_clip_logprobs)               # the noise is part of the condition
    loss.backward()
    prior = [n for n, p in m.named_parameters() if n.startswith(("conv3d.", "conv_mu2.", "conv_var2."))]
    named = dict(m.named_parameters())
    assert len(prior) >= 3 and all(named[n].grad is not None and named[n].grad.abs().max().item() == 0.0 for n in prior)
    assert named["conv_d2.weight"].grad.abs().max().item() > 0


def test_bf16_mode_reaches_the_bf16_instance(small, monkeypatch):
    m, b, tok, pairs, ref_lp = small["m"], small["b"], small["tok"], small["pairs"], small["ref_lp"]
    _reset(m)
    m.set_precision("bf16")
    lib = _lib.lib(0)
    seen = []
    real = lib.mage_token_logprob_bwd
    monkeypatch.setattr(lib, "mage_token_logprob_bwd", lambda *a: (seen.append(a[9]), real(*a))[1])
    loss, info = m.preference_loss(b, tok, pairs, ref_lp)
    loss.backward()
    monkeypatch.undo()
    grads = [p.grad for n, p in m.named_parameters() if p.grad is not None]
    _reset(m)
    assert seen == [ops.BF16]
    assert all(np.isfinite(v) for v in info.values()) and np.isfinite(loss.item())
    assert len(grads) >= 90 and all(bool(torch.isfinite(g).all()) for g in grads) and any(g.abs().max().item() > 0 for g in grads)


def test_rollout_hands_over_pairs(small, monkeypatch):
    m, ref = small["m"], small["ref"]
    N = 3
    batch = {**small["b"], "sample_seed": torch.tensor([11, 12, 13, 14], dtype=torch.int64)}
    _reset(m)
    m.set_sampling(0.9)
    out = m.rollout(batch, N, reference=ref, pairs='best_worst')
    loss, info = m.preference_loss(out['batch'], out['tokens'], out['pairs'], out['reference_clip_logprobs'])
    assert np.isfinite(loss.item()) and loss.requires_grad
    p, rw = out["pairs"], out["rewards"].reshape(-1)
    assert p.shape == (B, 2) and p.dtype == torch.int64 and p.device == rw.device
    assert out["reference_clip_logprobs"].shape == (B * N,) and out["reference_clip_logprobs"].dtype == torch.float32
    assert (p // N == torch.arange(B, device=DEV)[:, None]).all() and (rw[p[:, 0]] >= rw[p[:, 1]]).all()
    assert torch.equal(rw[p[:, 0]], out["rewards"].amax(1)) and torch.equal(rw[p[:, 1]], out["rewards"].amin(1))
    assert torch.equal(out["reference_clip_logprobs"], ref.clip_logprobs(out["batch"], out["tokens"]))
    # a constant reward: no preference anywhere
    flat = m.rollout(batch, N, reward=lambda video, bb: torch.zeros(video.shape[0], device=video.device), reference=ref, pairs="best_worst")
    assert flat["pairs"].tolist() == [[i * N, i * N] for i in range(B)]
    m.zero_grad(set_to_none=True)
    loss, info = m.preference_loss(flat["batch"], flat["tokens"], flat["pairs"], flat["reference_clip_logprobs"])
    loss.backward()
    assert loss.item() == LOG2 and info["accuracy"] == 0.0
    grads = [p_.grad for p_ in m.parameters() if p_.grad is not None]
    assert len(grads) >= 90 and all(g.abs().max().item() == 0.0 for g in grads)
    m.zero_grad(set_to_none=True)
    # pairs add no launch, and without pairs no new entry point is reached
    calls = count_lib_calls(monkeypatch)
    plain = m.rollout(batch, N)
    n_plain = collections.Counter(calls)
    calls.clear()
    paired = m.rollout(batch, N, pairs="best_worst")
    monkeypatch.undo()
    assert collections.Counter(calls) == n_plain and "pairs" not in plain and "reference_clip_logprobs" not in paired
    assert not {"mage_preference_loss", "mage_token_logprob_bwd"} & set(n_plain)
    assert torch.equal(plain["tokens"], paired["tokens"]) and torch.equal(plain["rewards"], paired["rewards"])
    _reset(m)


def test_preference_loss_runs_policy_loss_pass(small, monkeypatch):
    """'preference_loss runs policy_loss' pass', by the call counter: for the same batch and tokens the ordered C-ABI entry points policy_loss
    reaches before its first mage_policy_loss* call are the ones preference_loss reaches before its first mage_token_logprob call, in grad
    mode and under no_grad; and in backward the entry points after the head's own *_bwd kernel are the same list too."""
    m, b, tok, pairs, ref_lp = small["m"], small["b"], small["tok"], small["pairs"], small["ref_lp"]
    _reset(m)
    adv = torch.ones(B, device=DEV)
    runs = {"policy_loss": (lambda: m.policy_loss(b, tok, adv)[0], "mage_policy_loss", "mage_policy_loss_bwd"),
            "preference_loss": (lambda: m.preference_loss(b, tok, pairs, ref_lp)[0], "mage_token_logprob", "mage_token_logprob_bwd")}
    for run, _, _ in runs.values():
        run().backward()                                                         # derived caches built
    calls = count_lib_calls(monkeypatch)

    def before(prefix):
        return calls[:next(i for i, c in enumerate(calls) if c.startswith(prefix))]
    seen = {}
    for name, (run, head, head_bwd) in runs.items():
        del calls[:]
        with torch.no_grad():
            run()
        no_grad = before(head)
        del calls[:]
        loss = run()
        grad = before(head)
        del calls[:]
        loss.backward()
        first = next(i for i, c in enumerate(calls) if c.endswith("_bwd"))
        assert calls[first] == head_bwd, calls[:first + 1]
        seen[name] = (no_grad, grad, calls[first + 1:])
        print(f"{name}: {len(no_grad)} entry points before the head under no_grad, {len(grad)} in grad mode, {len(seen[name][2])} after {head_bwd}")
    monkeypatch.undo()
    _reset(m)
    pol, pref = seen["policy_loss"], seen["preference_loss"]
    assert min(map(len, pol)) >= 20 and "mage_attention" in pol[0] and "mage_attention_bwd" in pol[2]
    for what, x, y in zip(("no_grad forward", "grad-mode forward", "backward"), pol, pref):
        assert x == y, (what, [(i, p, q) for i, (p, q) in enumerate(zip(x, y)) if p != q][:5], len(x), len(y))


def test_refusals_launch_nothing(small, monkeypatch):
    m, b, tok, pairs, ref_lp = small["m"], small["b"], small["tok"], small["pairs"], small["ref_lp"]
    _reset(m)
    calls = count_lib_calls(monkeypatch)

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            m.preference_loss(*a, **kw)
        assert calls == []
    m.use_cids = False
    refused("use_cids=False", b, tok, pairs, ref_lp)
    m.use_cids = True
    m.set_guidance(2.0)
    refused("guidance", b, tok, pairs, ref_lp)
    m.set_guidance(None)
    m.randomness = True
    refused("randomness=True", b, tok, pairs, ref_lp)
    m.randomness = False
    m.set_precision("f16")
    refused("f16", b, tok, pairs, ref_lp)
    m.set_precision("fp32")
    refused("tokens", b, tok[:, 1:], pairs, ref_lp)
    refused("tokens", b, tok.int(), pairs, ref_lp)
    refused("pairs", b, tok, pairs.int(), ref_lp)
    refused("pairs", b, tok, pairs[:0], ref_lp)
    refused("pairs", b, tok, pairs.reshape(-1), ref_lp)
    refused("reference_logprobs", b, tok, pairs, ref_lp[:2])
    refused("reference_logprobs", b, tok, pairs, ref_lp.double())
    refused("beta", b, tok, pairs, ref_lp, beta=0.0)
    refused("beta", b, tok, pairs, ref_lp, beta=float("nan"))
    refused("label_smoothing", b, tok, pairs, ref_lp, label_smoothing=0.5)
    refused("label_smoothing", b, tok, pairs, ref_lp, label_smoothing=0.1, loss="ipo")
    refused("loss", b, tok, pairs, ref_lp, loss="hinge")
    refused("GPU", b, tok.cpu(), pairs, ref_lp)
    refused("GPU", b, tok, pairs.cpu(), ref_lp)
    refused("GPU", b, tok, pairs, ref_lp.cpu())
    refused("GPU", {k: v.cpu() for k, v in b.items()}, tok, pairs, ref_lp)
    with pytest.raises(ValueError, match="clip_logprobs: tokens"):
        m.clip_logprobs(b, tok[:, 1:])
    m.set_sampling(0.9)
    with pytest.raises(ValueError, match="rollout: pairs"):
        m.rollout(b, 3, pairs="worst_best")
    assert calls == []
    monkeypatch.undo()
    _reset(m)
    with pytest.raises(ValueError, match="pair index out of range"):             # an index the host does not read: reported by the device
        m.preference_loss(b, tok, torch.tensor([[0, B]], device=DEV), ref_lp)
