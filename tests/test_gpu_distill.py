"""GPU: MAGE.distill_targets and MAGE.distill_loss -- a model against its own logits (exactly 0), the gradients of both modes against
autograd through the oracle (the student's logits from oracle/mage_oracle.py on the CPU, the KL written in torch against fixed teacher
logits: tests/test_gpu_policy_train.py's oracle_policy with another loss), bf16 against fp32, a guided teacher, the mask, a short
optimisation loop and the refusals."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mage_amd import ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from mage_amd.utils.glue import null_caption
from oracle import mage_oracle as O
from tests import distill_ref as D
from tests.helpers import build_mage, count_lib_calls, cpu_sd
from tests.test_gpu_policy_train import GRAD_TOL, SMALL, dev_batch, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 5


def _model(seed, B=3):
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), seed, DEV)
    batch = dev_batch(synth.synth_batch_mnist(B, L, seed=seed, text_len=9, ragged_text=True))
    R, K = m.image_resolution, m.codebook_size
    tok = torch.randint(0, K, (B, L - 1, R, R), generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return m, batch, tok


@pytest.fixture(scope="module")
def small():
    return _model(41)


def _reset(m):
    m.set_guidance(None).set_sampling(None).set_precision("fp32").set_context(1)
    m.eval()
    m.zero_grad(set_to_none=True)


def _teacher_logits(m, seed, scale=1.5):
    """Fixed teacher logits near the model's own: its distill_targets plus seeded noise."""
    def f(batch, tok):
        own = m.distill_targets(batch, tok)
        return own + scale * torch.randn(own.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return f


def test_a_model_is_its_own_exact_teacher(small):
    m, batch, tok = small
    _reset(m)
    last = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    tl = m.distill_targets(batch, tok)
    now = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    assert last.keys() == now.keys() and all(now[a] is last[a] for a in last)           # every last_* attribute is left as found
    assert tl.shape == (tok.numel(), m.codebook_size) and tl.dtype == torch.float32 and not tl.requires_grad
    assert torch.equal(tl, m.distill_targets(batch, tok))
    for mode in ("forward", "reverse"):
        for T in (1.0, 2.0):
            m.zero_grad(set_to_none=True)
            loss, info = m.distill_loss(batch, tok, tl, temperature=T, mode=mode)
            assert loss.item() == 0.0 and loss.requires_grad and info["loss"] == 0.0 and info["agreement"] == 1.0
            assert info["entropy"] == info["teacher_entropy"] > 0 and info["given_fraction"] == 0.0
            assert set(info) == {"loss", "teacher_entropy", "entropy", "agreement", "given_fraction"}
            assert m.last_distill_token_kl.shape == tok.shape and (m.last_distill_token_kl.view(torch.int32) == 0).all()
            loss.backward()
            grads = [p.grad for n, p in m.named_parameters() if not n.startswith("first_stage_model.")]
            assert len(grads) > 90 and all(g is not None and (g == 0).all() for g in grads)
    _reset(m)


def oracle_distill(sd, batch, tokens, teacher, T, mode, given=None):
    """The mean KL through the oracle on the CPU in fp32, the loss in torch: (loss, gradients by name)."""
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.startswith("first_stage_model.") else v) for k, v in sd.items()}
    tok0 = O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, 0])
    tok = torch.cat([tok0[:, None], tokens], 1)
    ma = O.motion_anchor(sd, tok0, batch["text"], batch.get("speed"))
    logits = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, tok[:, :L - 1]))
    loss = D.torch_kl(logits.reshape(-1, logits.shape[-1]), teacher, T, mode, given)
    names = [k for k, v in sd.items() if v.requires_grad]
    return loss.item(), dict(zip(names, torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)))


@pytest.mark.parametrize("mode,T,masked", [("forward", 1.3, False), ("reverse", 0.8, False), ("forward", 2.0, True)])
def test_gradients_match_oracle_autograd(small, mode, T, masked):
    m, batch, tok = small
    _reset(m)
    B = tok.shape[0]
    teacher = _teacher_logits(m, 7)(batch, tok)
    given = None
    if masked:
        given = torch.zeros(tok.shape, dtype=torch.bool, device=DEV)
        given[:, 0], given[1, 2, :3] = True, True                                        # frame 1 everywhere, three rows of one more frame
    cpu = {k: v.cpu() for k, v in batch.items()}
    want_loss, want = oracle_distill(cpu_sd(m), cpu, tok.cpu(), teacher.cpu(), T, 0 if mode == "forward" else 1,
                                     None if given is None else given.reshape(-1).cpu())
    loss, info = m.distill_loss(batch, tok, teacher, temperature=T, mode=mode, given=given)
    print(f"{mode} T={T}: loss {loss.item():.6f} want {want_loss:.6f}; info {info}")
    assert abs(loss.item() - want_loss) < 1e-4 * max(1.0, want_loss) and info["loss"] == loss.item() and loss.item() > 0.05
    if masked:
        assert info["given_fraction"] == np.float32(given.sum().item() / given.numel()) and (m.last_distill_token_kl[given] == 0).all()
        assert (m.last_distill_token_kl[~given] > 0).all()
    (loss * T * T).backward()                                                            # the usual rescaling goes through grad_out
    worst, n_checked = ("", 0.0), 0
    for name, p in m.named_parameters():
        if name.startswith("first_stage_model."):
            assert p.grad is None
            continue
        g_ref = want.get(name)
        assert p.grad is not None, name
        if g_ref is None or g_ref.abs().max().item() == 0.0:
            assert p.grad.abs().max().item() == 0.0, name
            continue
        r = rel(p.grad, g_ref * T * T)
        n_checked += 1
        if r > worst[1]:
            worst = (name, r)
    print(f"{n_checked} gradients checked, worst relative error {worst[1]:.2e} at {worst[0]}")
    assert worst[1] < GRAD_TOL, worst
    assert n_checked >= 90
    _reset(m)


def test_bf16_gradients_track_fp32(small):
    m, batch, tok = small
    _reset(m)
    teacher = _teacher_logits(m, 8)(batch, tok)
    m.distill_loss(batch, tok, teacher)[0].backward()
    g32 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    m.set_precision("bf16")
    m.distill_loss(batch, tok, teacher)[0].backward()
    cos = [F.cosine_similarity(p.grad.flatten(), g32[n].flatten(), dim=0).item() for n, p in m.named_parameters()
           if p.grad is not None and g32[n].abs().max() > 0]
    _reset(m)
    print(f"bf16 vs fp32 distillation gradients: min cosine {min(cos):.4f}, mean {np.mean(cos):.4f}")
    assert len(cos) >= 90 and min(cos) > 0.98


def test_guided_teacher(small):
    m, batch, tok = small
    _reset(m)
    B, rows, K = tok.shape[0], tok.numel(), m.codebook_size
    pad = int(getattr(m.text_encoder, "padding_idx", 0))
    cond = m.distill_targets(batch, tok)
    neg = null_caption(batch["text"].to(torch.int64), pad)
    uncond = m.distill_targets({**batch, "text": neg}, tok)
    assert not torch.equal(cond, uncond)
    combine = lambda c, u, s: ops.guide_logits(c.clone(), u, s, rows=rows, K=K, scale_div=rows // B)      # noqa: E731
    m.set_guidance(3.0)
    last = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    got = m.distill_targets(batch, tok)
    now = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    assert last.keys() == now.keys() and all(now[a] is last[a] for a in last)
    assert torch.equal(got, combine(cond, uncond, torch.full((B,), 3.0, device=DEV))) and not torch.equal(got, cond)
    # an explicit negative caption, and one scale per clip
    other = batch["text"].roll(1, 0).contiguous()
    u2 = m.set_guidance(None).distill_targets({**batch, "text": other}, tok)
    scales = torch.tensor([1.0, 2.5, -0.5], device=DEV)
    got2 = m.set_guidance(3.0).distill_targets({**batch, "negative_text": other, "guidance_scale": scales}, tok)
    assert torch.equal(got2, combine(cond, u2, scales))
    per = rows // B
    assert torch.equal(got2[:per], cond[:per]) and not torch.equal(got2[per:2 * per], cond[per:2 * per])       # scale 1: the unguided rows
    assert torch.equal(m.set_guidance(1.0).distill_targets(batch, tok), cond)            # scale 1 is the unguided call bit for bit
    # the student side stays refused under guidance, in its pinned words
    with pytest.raises(ValueError, match="classifier-free guidance is on"):
        m.distill_loss(batch, tok, got)
    m.set_guidance(None)
    loss, info = m.distill_loss(batch, tok, got)
    assert loss.item() > 0 and 0 < info["agreement"] < 1
    _reset(m)


def test_given_mask(small):
    m, batch, tok = small
    _reset(m)
    teacher = _teacher_logits(m, 9)(batch, tok)
    with torch.no_grad():
        l0, i0 = m.distill_loss(batch, tok, teacher, mode="reverse")
        kl0 = m.last_distill_token_kl.clone()
        l1, i1 = m.distill_loss(batch, tok, teacher, mode="reverse", given=torch.zeros(tok.shape, dtype=torch.bool, device=DEV))
        assert not l0.requires_grad and torch.equal(l0, l1) and i0 == i1 and torch.equal(kl0, m.last_distill_token_kl)
        given = torch.zeros(tok.shape, dtype=torch.bool, device=DEV)
        given[:, :2] = True                                                              # two of four generated frames were given
        poisoned = teacher.clone()
        poisoned[given.reshape(-1)] = float("nan")                                       # the given rows are not read
        l2, i2 = m.distill_loss(batch, tok, poisoned, mode="reverse", given=given)
    assert i2["given_fraction"] == 0.5 and (m.last_distill_token_kl[given] == 0).all()
    assert torch.equal(m.last_distill_token_kl[~given], kl0[~given])
    assert abs(l2.item() - kl0[~given].double().mean().item()) <= 2.0 ** -23 * l2.item()
    _reset(m)


def _loop(seed):
    m, batch, tok = _model(seed)
    teacher = copy.deepcopy(m).eval().set_guidance(2.0)
    targets = teacher.distill_targets(batch, tok)
    del teacher
    g = torch.Generator().manual_seed(seed)
    # A perturbed student: every matrix moves by 0.3 of its own spread, far more than the optimiser can undo or overshoot in 20 steps (Adam
    # moves a parameter by about lr per step: 20 * 2e-4 in all), so every step is a descent step on a loss well away from 0.
    with torch.no_grad():
        for n, p in m.named_parameters():
            if not n.startswith("first_stage_model.") and p.dim() >= 2:
                p.add_((0.3 * p.std().item() * torch.randn(p.shape, generator=g)).to(DEV))
    opt = FlatAdam(m.parameters(), lr=2e-4)
    hist = []
    for _ in range(20):
        opt.zero_grad()
        loss, info = m.distill_loss(batch, tok, targets)
        loss.backward()
        opt.step()
        hist.append((info["loss"], info["agreement"]))
    with torch.no_grad():
        info = m.distill_loss(batch, tok, targets)[1]
    return hist + [(info["loss"], info["agreement"])]


def test_twenty_steps_lower_the_loss_and_repeat_bit_for_bit():
    a = _loop(43)
    print(f"distillation against a guided teacher over 20 FlatAdam steps: loss {a[0][0]:.6e} -> {a[-1][0]:.6e}, "
          f"agreement {a[0][1]:.4f} -> {a[-1][1]:.4f}")
    assert a[-1][0] < a[0][0] and a[-1][1] > a[0][1]
    assert _loop(43)[-1] == a[-1]


def test_refusals_launch_nothing_and_leave_forward_alone(small, monkeypatch):
    m, batch, tok = small
    _reset(m)
    teacher = _teacher_logits(m, 10)(batch, tok)

    def forward_bits():
        m.zero_grad(set_to_none=True)
        loss, _ = m(batch)
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    loss0, g0 = forward_bits()
    m.distill_loss(batch, tok, teacher, temperature=2.0, mode="reverse")[0].backward()
    m.set_guidance(2.0).distill_targets(batch, tok)
    m.set_guidance(None)
    loss1, g1 = forward_bits()
    assert torch.equal(loss0, loss1) and g0.keys() == g1.keys() and all(torch.equal(g0[n], g1[n]) for n in g0)       # no state leaks
    m.zero_grad(set_to_none=True)
    m.last_distill_token_kl = None
    calls = count_lib_calls(monkeypatch)

    def refused(match, *a, fn=None, **kw):
        with pytest.raises(ValueError, match=match):
            (fn or m.distill_loss)(*a, **kw)
        assert calls == [] and m.last_distill_token_kl is None
    m.use_cids = False
    refused("use_cids=False", batch, tok, teacher)
    refused("use_cids=False", batch, tok, fn=m.distill_targets)
    m.use_cids = True
    m.randomness = True
    refused("randomness=True", batch, tok, teacher)
    m.randomness = False
    m.set_precision("f16")
    refused("f16", batch, tok, teacher)
    m.set_precision("fp32")
    m.set_guidance(2.0)
    refused("classifier-free guidance is on", batch, tok, teacher)
    m.set_guidance(None)
    m.set_context(2)
    refused("set_context", batch, tok, teacher)
    refused("set_context", batch, tok, fn=m.distill_targets)
    m.set_context(1)
    refused("known_tokens", {**batch, "known_tokens": tok}, tok, teacher)
    refused("known_tokens", {**batch, "known_tokens": tok}, tok, fn=m.distill_targets)
    refused("tokens", batch, tok[:, 1:], teacher)
    refused("tokens", batch, tok.int(), fn=m.distill_targets)
    refused("teacher_logits", batch, tok, teacher[:-1])
    refused("teacher_logits", batch, tok, teacher.double())
    refused("teacher_logits", batch, tok, teacher.view(tok.shape + (-1,)))
    refused("temperature", batch, tok, teacher, temperature=0.0)
    refused("temperature", batch, tok, teacher, temperature=float("nan"))
    refused("mode", batch, tok, teacher, mode="kl")
    refused("given must be bool", batch, tok, teacher, given=torch.zeros(tok.shape, device=DEV))
    refused("GPU", batch, tok, teacher.cpu())
    refused("GPU", batch, tok.cpu(), teacher)
    refused("GPU", batch, tok, teacher, given=torch.zeros(tok.shape, dtype=torch.bool))
    refused("GPU", {k: v.cpu() for k, v in batch.items()}, tok, fn=m.distill_targets)
    refused("batch must be a dict", [batch], tok, teacher)
    monkeypatch.undo()
    _reset(m)
