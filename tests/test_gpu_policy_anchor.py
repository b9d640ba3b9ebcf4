"""GPU: the reference-policy anchor at model level -- MAGE.token_policy_logprobs, MAGE.policy_loss(reference_logprobs=, kl_coef=),
MAGE.rollout(reference=) and the whole step with FlatAdam(max_grad_norm=): against the plain call bit for bit where the reference is the
model itself, against autograd through the oracle (tests/test_gpu_policy_train.py's oracle side and tolerance, the KL term in torch fp64)
where it is a perturbed copy, and ten steps of the documented loop.  The model is tests/test_gpu_policy_train.py's small one."""
import copy
import math

import numpy as np
import pytest
import torch

from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from oracle import mage_oracle as O
from tests.helpers import build_mage, count_lib_calls, cpu_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_TOL = 1e-4             # tests/test_gpu_policy_train.py's: relative to the largest entry of the reference gradient tensor
SMALL = dict(width=64, layers=3, vq_dim=32, K=64)
L, B = 4, 2


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _last(m):
    return {a: v for a, v in vars(m).items() if a.startswith("last_")}


def _same_last(before, m):
    after = _last(m)
    return before.keys() == after.keys() and all(after[a] is v for a, v in before.items())


def _perturbed_copy(frames_length, model_seed, seed, amount=0.05):
    """The model build_mage makes from model_seed, its trainable weights scaled by 1 + amount * N(0, 1): a reference policy near it, not on it."""
    ref = build_mage(synth.mnist_model_config(frames_length=frames_length, **SMALL), model_seed, DEV).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if not n.startswith("first_stage_model."):
                p.mul_(1 + amount * torch.randn(p.shape, generator=g).to(DEV))
    return ref


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 41, DEV).eval()
    batch = dev_batch(synth.synth_batch_mnist(B, L, seed=41, text_len=9, ragged_text=True))
    R = m.image_resolution
    g = torch.Generator().manual_seed(42)
    tokens = torch.randint(0, m.codebook_size, (B, L - 1, R, R), generator=g).to(DEV)
    return m, batch, tokens


def _reset(m):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32")
    m.eval()
    m.zero_grad(set_to_none=True)


def test_token_policy_logprobs_is_the_no_grad_policy_loss_pass(small):
    m, batch, tokens = small
    _reset(m)
    m.set_sampling(0.9, top_k=16, top_p=0.95)
    with torch.no_grad():
        m.policy_loss(batch, tokens, torch.ones(B, device=DEV))
    want = m.last_policy_token_logprobs
    before, settings = _last(m), (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy)
    got = m.token_policy_logprobs(batch, tokens)
    assert got.shape == tokens.shape and got.dtype == torch.float32 and not got.requires_grad
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.isneginf(got).any()    # (the filter cannot draw every token)
    assert _same_last(before, m) and settings == (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy)
    assert all(p.grad is None for p in m.parameters())
    _reset(m)


def test_the_model_as_its_own_reference_changes_nothing(small):
    m, batch, tokens = small
    _reset(m)
    m.set_sampling(0.9, top_k=16)
    adv = torch.tensor([1.0, -0.5], device=DEV)
    blp = m.token_policy_logprobs(batch, tokens)
    ref = blp.clone()
    blp = torch.where(torch.isfinite(blp), blp + 0.3, torch.zeros_like(blp))       # some rows clip
    plain, info0 = m.policy_loss(batch, tokens, adv, blp, entropy_coef=0.01)
    plain.backward()
    g0 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert m.last_policy_token_kl is None and "kl" not in info0
    m.zero_grad(set_to_none=True)
    loss, info = m.policy_loss(batch, tokens, adv, blp, entropy_coef=0.01, reference_logprobs=ref, kl_coef=0.5)
    loss.backward()
    assert info["kl"] == 0.0 and (m.last_policy_token_kl == 0).all() and m.last_policy_token_kl.shape == tokens.shape
    assert set(info) == set(info0) | {"kl", "unanchored_fraction"} and all(info[k] == info0[k] for k in info0)
    assert info["unanchored_fraction"] == 0.0 and info["outside_fraction"] > 0          # (the reference's -inf rows are this policy's outside rows)
    assert torch.equal(loss.detach().view(torch.int32), plain.detach().view(torch.int32))
    g1 = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert g0.keys() == g1.keys() and all(torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)) for n in g0)
    _reset(m)


def test_anchored_gradients_match_oracle_autograd():
    """tests/test_gpu_policy_train.py's first configuration (fp32, eval(), temperature 1.3, no filter) with the KL term against a perturbed
    copy's log-probabilities added on both sides; on the oracle's side in torch fp64 from its own log-probabilities."""
    from tests.test_gpu_policy_train import rel
    Lo, Bo, seed, T, clip, c, kc = 5, 3, 31, 1.3, 0.2, 0.01, 0.3
    m = build_mage(synth.mnist_model_config(frames_length=Lo, **SMALL), seed, DEV)
    batch = synth.synth_batch_mnist(Bo, Lo, seed=seed, text_len=9, ragged_text=True)
    R, K = m.image_resolution, m.codebook_size
    g = torch.Generator().manual_seed(seed + 1)
    tokens = torch.randint(0, K, (Bo, Lo - 1, R, R), generator=g)
    adv = torch.randn((Bo,), generator=g)
    adv[0], adv[1] = adv[0].abs() + 0.1, -adv[1].abs() - 0.1
    adv_rows = adv.repeat_interleave((Lo - 1) * R * R)
    ref_model = _perturbed_copy(Lo, seed, seed + 5)
    ref_model.set_sampling(T)
    r = ref_model.token_policy_logprobs(dev_batch(batch), tokens.to(DEV))
    assert torch.isfinite(r).all()
    # the oracle's side: test_gpu_policy_train.oracle_policy's pass, the clipped surrogate plus kc * k3
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.startswith("first_stage_model.") else v) for k, v in cpu_sd(m).items()}
    tok0 = O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, 0])
    tok = torch.cat([tok0[:, None], tokens], 1)
    ma = O.motion_anchor(sd, tok0, batch["text"], batch.get("speed"))
    logits = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, tok[:, :Lo - 1]))
    logp = torch.log_softmax(logits.reshape(-1, K) * float(np.float32(1.0 / float(np.float32(T)))), -1)
    lp = logp.gather(1, tokens.reshape(-1, 1))[:, 0]
    ent = -(logp.exp() * logp).sum(-1)
    gen = torch.Generator().manual_seed(seed + 2)
    noise = (torch.rand(lp.shape, generator=gen) * 2 - 1) * 0.4
    lo, hi = 1.0 - clip, 1.0 + clip
    for _ in range(8):
        rho = (-noise).exp()
        near = ((rho / lo - 1).abs() < 1e-2) | ((rho / hi - 1).abs() < 1e-2)
        noise[near] = ((torch.rand(lp.shape, generator=gen) * 2 - 1) * 0.4)[near]
    assert not near.any()
    b = (lp.detach() + noise).float()
    rho = (lp - b).exp()
    d = r.cpu().reshape(-1).double() - lp.double()
    kl = d.exp() - d - 1
    want_loss = ((-torch.minimum(rho * adv_rows, rho.clamp(lo, hi) * adv_rows) - c * ent).double() + kc * kl).mean()
    names = [k for k, v in sd.items() if v.requires_grad]
    want = dict(zip(names, torch.autograd.grad(want_loss, [sd[k] for k in names], allow_unused=True)))
    m.set_sampling(T)
    loss, info = m.policy_loss(dev_batch(batch), tokens.to(DEV), adv.to(DEV), b.view(tokens.shape).to(DEV), clip=clip, entropy_coef=c,
                               reference_logprobs=r, kl_coef=kc)
    print(f"loss {loss.item():.6f} want {want_loss.item():.6f}; info {info}; oracle kl {kl.mean().item():.6f}")
    assert abs(loss.item() - want_loss.item()) < 1e-4 and abs(info["kl"] - kl.mean().item()) < 1e-4 and info["kl"] > 0
    assert info["unanchored_fraction"] == 0.0 and info["outside_fraction"] == 0.0
    loss.backward()
    worst, n_checked = ("", 0.0), 0
    for name, p in m.named_parameters():
        if name.startswith("first_stage_model."):
            assert p.grad is None
            continue
        g_ref = want.get(name)
        if g_ref is None or g_ref.abs().max().item() == 0.0:
            assert p.grad.abs().max().item() == 0.0, name
            continue
        e = rel(p.grad, g_ref.float())
        n_checked += 1
        if e > worst[1]:
            worst = (name, e)
    print(f"{n_checked} gradients checked, worst relative error {worst[1]:.2e} at {worst[0]}")
    assert worst[1] < GRAD_TOL and n_checked >= 90, worst


def _rollout_batch(seed=41):
    return dev_batch({**synth.synth_batch_mnist(B, L, seed=seed, text_len=9, ragged_text=True), "sample_seed": torch.tensor([11, 12], dtype=torch.int64)})


def test_rollout_scores_its_tokens_under_the_reference(small):
    m, _, _ = small
    _reset(m)
    batch = _rollout_batch()
    ref = _perturbed_copy(L, 41, 7)
    ref.set_sampling(1.7, top_k=5).set_logprobs(True)
    before, settings = _last(ref), (ref.sampling, ref.candidates, ref.logprobs, ref.logprob_policy, ref.logprob_entropy)
    m.set_sampling(0.9, top_k=32)
    out = m.rollout(batch, 3, reference=ref)
    assert _same_last(before, ref) and settings == (ref.sampling, ref.candidates, ref.logprobs, ref.logprob_policy, ref.logprob_entropy)
    assert out["reference_logprobs"].shape == out["tokens"].shape and out["reference_logprobs"].dtype == torch.float32
    ref.set_sampling(0.9, top_k=32)
    want = ref.token_policy_logprobs(out["batch"], out["tokens"])
    assert torch.equal(out["reference_logprobs"].view(torch.int32), want.view(torch.int32))
    assert "reference_logprobs" not in m.rollout(batch, 3)
    # the documented loop, as written
    loss, info = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"],
                               reference_logprobs=out["reference_logprobs"], kl_coef=0.1)
    loss.backward()
    assert math.isfinite(loss.item()) and info["kl"] > 0 and 0 <= info["unanchored_fraction"] < 1
    assert sum(p.grad is not None for p in m.parameters()) >= 90
    _reset(m)


def _ten_steps(seed):
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), seed, DEV).eval()
    ref = copy.deepcopy(m).eval()                                    # the frozen reference, as documented: the model before fine-tuning
    assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), m.state_dict().values()))
    for p in ref.parameters():
        p.requires_grad_(False)
    batch = _rollout_batch(seed)
    m.set_sampling(1.0, top_k=32)
    opt = FlatAdam(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    kls, norms, losses = [], [], []
    for _ in range(10):
        out = m.rollout(batch, 3, reference=ref)
        opt.zero_grad()
        loss, info = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"],
                                   reference_logprobs=out["reference_logprobs"], kl_coef=0.1)
        loss.backward()
        opt.step()
        kls.append(info["kl"])
        norms.append(opt.last_grad_norm.item())
        losses.append(loss.item())
    return kls, norms, losses, opt.flat_p.clone()


def test_ten_steps_of_the_documented_loop_repeat_bit_for_bit():
    kls, norms, losses, p = _ten_steps(43)
    print(f"kl {kls[0]:.3e} -> {kls[-1]:.3e}; gradient norms {min(norms):.3e} .. {max(norms):.3e}; loss {losses[0]:.4e} -> {losses[-1]:.4e}")
    assert all(math.isfinite(x) for x in norms + losses + kls)
    assert kls[0] == 0.0 and kls[9] > 0.0
    kls2, norms2, losses2, p2 = _ten_steps(43)
    assert kls2 == kls and norms2 == norms and losses2 == losses and torch.equal(p.view(torch.int32), p2.view(torch.int32))


def test_refusals_launch_nothing(small, monkeypatch):
    m, batch, tokens = small
    _reset(m)
    adv = torch.ones(B, device=DEV)
    ref = torch.zeros(tokens.shape, device=DEV)
    other = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=32), 5, DEV)
    longer = build_mage(synth.mnist_model_config(frames_length=L + 1, **SMALL), 5, DEV)
    on_cpu = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 5)
    m.set_sampling(0.9)
    calls = count_lib_calls(monkeypatch)

    def refused(match, fn, *a, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*a, **kw)
        assert calls == []
    refused("kl_coef", m.policy_loss, batch, tokens, adv, kl_coef=0.1)
    refused("kl_coef", m.policy_loss, batch, tokens, adv, reference_logprobs=ref, kl_coef=-0.1)
    refused("kl_coef", m.policy_loss, batch, tokens, adv, reference_logprobs=ref, kl_coef=float("nan"))
    refused("kl_coef", m.policy_loss, batch, tokens, adv, reference_logprobs=ref, kl_coef=float("inf"))
    refused("reference_logprobs", m.policy_loss, batch, tokens, adv, reference_logprobs=ref[:, 1:], kl_coef=0.1)
    refused("reference_logprobs", m.policy_loss, batch, tokens, adv, reference_logprobs=ref.double(), kl_coef=0.1)
    refused("GPU", m.policy_loss, batch, tokens, adv, reference_logprobs=ref.cpu(), kl_coef=0.1)
    refused("tokens", m.token_policy_logprobs, batch, tokens[:, 1:])
    rb = _rollout_batch()
    refused("codebook_size", m.rollout, rb, 3, reference=other)
    refused("frames_length", m.rollout, rb, 3, reference=longer)
    refused("same GPU", m.rollout, rb, 3, reference=on_cpu)
    refused("reference must be", m.rollout, rb, 3, reference="ref")
    other.use_cids = False
    refused("use_cids", m.rollout, rb, 3, reference=other)
    monkeypatch.undo()
    _reset(m)
