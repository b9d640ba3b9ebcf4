"""GPU, end to end: MAGE.set_loss, batch['given'] and MAGE.evaluate on tests/test_gpu_policy_train.py's SMALL model (width 64, 3 layers,
K 64), B = 3.  forward's loss and gradients against autograd through the CPU oracle (F.cross_entropy with weight, label_smoothing and
ignore_index plus zeta * mean(logsumexp^2) on the oracle's logits); the defaults against a model that never heard of set_loss, by bits and by
launch names; the identities the README states; evaluate against score and mage_argmax; a short training loop."""
import copy

import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from mage_amd.utils.glue import balanced_class_weights
from oracle import mage_oracle as O
from tests import xent_ref as X
from tests.helpers import build_mage, count_lib_calls, cpu_sd
from tests.test_gpu_policy_loss import _ulp
from tests.test_gpu_policy_train import GRAD_TOL, SMALL, dev_batch, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, L, SEED = 3, 5, 41
LOSS_TOL = 1e-4             # tests/test_gpu_train.py's tolerance for forward's loss against the oracle


@pytest.fixture(scope="module")
def small():
    """The model, its batch (CPU), the first stage's tokens [B, L, h, w] (CPU), the oracle's logits' inputs and balanced class weights."""
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), SEED, DEV)
    batch = synth.synth_batch_mnist(B, L, seed=SEED, text_len=9, ragged_text=True)
    assert m.image_resolution == R
    tok = m.first_stage_encode(batch["images"].to(DEV)).cpu()
    counts = m.first_stage_model.code_usage(tok.to(DEV))["counts"]  # the weights' natural source
    assert torch.equal(counts.cpu(), torch.bincount(tok.reshape(-1), minlength=m.codebook_size))
    return m, batch, tok, balanced_class_weights(counts).cpu()


R = 16                      # the SMALL model's token grid (64 x 64 frames, down ratio 4)


def _mask(k=2):
    """The first k frames' slots given: a continuation's context."""
    g = torch.zeros(B, L - 1, R, R, dtype=torch.bool)
    g[:, :k] = True
    return g


def _oracle(sd, batch, tok, w, eps, zeta, given):
    """(loss, gradients by name) of the supervised objective on the oracle's CPU logits."""
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.startswith("first_stage_model.") else v) for k, v in sd.items()}
    ma = O.motion_anchor(sd, tok[:, 0], batch["text"], batch.get("speed"))
    logits = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, tok[:, :L - 1]))
    K = logits.shape[-1]
    loss = X.torch_loss(logits.reshape(-1, K), tok[:, 1:L].reshape(-1), w, eps, zeta, None if given is None else given.reshape(-1))
    names = [k for k, v in sd.items() if v.requires_grad]
    return loss.item(), dict(zip(names, torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)))


def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _reset(m):
    m.set_precision("fp32").set_sampling(None).set_guidance(None).set_logprobs(False).set_context(1).set_loss()
    m.eval()
    m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("eps,zeta,weighted,masked", [(0.1, 0.0, False, False), (0.0, 1e-3, False, False), (0.0, 0.0, True, False),
                                                      (0.1, 1e-3, True, True)])
def test_forward_matches_oracle_autograd(small, eps, zeta, weighted, masked):
    m, batch, tok, w = small
    _reset(m)
    w = w if weighted else None
    given = _mask() if masked else None
    want_loss, want = _oracle(cpu_sd(m), batch, tok, w, eps, zeta, given)
    m.set_loss(eps, zeta, w)
    db = dev_batch(batch)
    if masked:
        db["given"] = given.to(DEV)
    loss, ld = m(db)
    print(f"loss {loss.item():.6f} want {want_loss:.6f}; {ld}")
    assert abs(loss.item() - want_loss) < LOSS_TOL and loss.requires_grad and ld["val/prediction"] == loss.item()
    assert {"val/nll", "val/accuracy", "val/final_loss"} <= set(ld) and ("val/given_fraction" in ld) == masked
    if masked:
        assert ld["val/given_fraction"] == 0.5
    with torch.no_grad():                                            # the values-only path ends in the same head
        l0, ld0 = m(db)
    assert abs(l0.item() - loss.item()) <= 1e-5 and not l0.requires_grad and set(ld0) == set(ld)
    loss.backward()
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
        r = rel(p.grad, g_ref)
        n_checked += 1
        if r > worst[1]:
            worst = (name, r)
    print(f"{n_checked} gradients checked, worst relative error {worst[1]:.2e} at {worst[0]}")
    assert worst[1] < GRAD_TOL, worst
    assert n_checked >= 90
    _reset(m)


def test_defaults_are_the_plain_call_by_bits_and_launches(small, monkeypatch):
    m, batch, _, w = small
    _reset(m)
    db = dev_batch(batch)
    fresh = copy.deepcopy(m)                                          # never heard of set_loss
    lf, _ = fresh(db)
    lf.backward()
    want = _grads(fresh)
    m.set_loss(0.1, 1e-3, w).set_loss()                               # ... set and restored
    calls = count_lib_calls(monkeypatch)
    loss, ld = m(db)
    loss.backward()
    names = list(calls)
    monkeypatch.undo()
    assert "mage_token_xent" not in names and "mage_token_xent_bwd" not in names
    assert names.count("mage_cross_entropy") == 1 and names.count("mage_cross_entropy_bwd") == 1
    assert loss.view(torch.int32).item() == lf.view(torch.int32).item() and set(ld) == {"val/prediction", "val/final_loss"}
    got = _grads(m)
    assert got.keys() == want.keys() and all(torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)) for n in want)
    calls = count_lib_calls(monkeypatch)
    with torch.no_grad():
        m(db)
    assert "mage_token_xent" not in calls and calls.count("mage_cross_entropy") == 1
    monkeypatch.undo()
    calls = count_lib_calls(monkeypatch)                              # and with an option the new pair runs in its place
    m.set_loss(z_loss=1e-3)
    m(db)[0].backward()
    assert calls.count("mage_token_xent") == 1 and calls.count("mage_token_xent_bwd") == 1 and "mage_cross_entropy" not in calls
    monkeypatch.undo()
    _reset(m)


def _two_ulp(a, b, m, db, what, given=None):
    """|a - b| within the kernel test's allowance (tests/test_gpu_xent_kernels.py: two kernels that form nll from an fp32 log Z and maximum in
    a different order agree per row to 2 ulp at the larger of |nll| and |lse|): the mean of the rows' allowances over the free tokens, plus
    one rounding of each mean.  nll and lse come from torch's fp64 log-softmax of the model's own logits."""
    with torch.no_grad():
        tok, logits = m.teacher_forced_logits(db)
    K = logits.shape[-1]
    z = logits.reshape(-1, K).double()
    lse = torch.logsumexp(z, -1)
    nll = lse - z.gather(1, tok[:, 1:].reshape(-1, 1))[:, 0]
    free = torch.ones_like(nll, dtype=torch.bool) if given is None else ~given.reshape(-1)
    per = 2 * _ulp(torch.maximum(nll.abs(), lse.abs())[free].cpu().numpy())
    allow = per.mean() + 2 * 2.0 ** -24 * abs(b)
    print(f"{what}: {a!r} against {b!r}, allowance {float(allow):.3e}")
    assert abs(a - b) <= allow, what


def test_all_free_mask_trains_the_same_tokens(small):
    m, batch, _, _ = small
    _reset(m)
    db = dev_batch(batch)
    plain, _ = m(db)
    plain.backward()
    want = _grads(m)
    m.zero_grad(set_to_none=True)
    loss, ld = m({**db, "given": torch.zeros(B, L - 1, R, R, dtype=torch.bool, device=DEV)})
    assert ld["val/given_fraction"] == 0.0
    _two_ulp(loss.item(), plain.item(), m, db, "an all-False given against the plain loss")
    loss.backward()
    got = _grads(m)
    assert max(rel(got[n], want[n]) for n in want if want[n].abs().max() > 0) < GRAD_TOL
    _reset(m)


def test_masked_loss_is_policy_loss_with_unit_advantages(small):
    """README's identity: cross entropy over the free tokens == policy_loss(given=) with advantages 1, sampling off, entropy_coef 0."""
    m, batch, tok, _ = small
    _reset(m)
    db = dev_batch(batch)
    given = _mask(2).to(DEV)
    with torch.no_grad():
        loss, _ = m({**db, "given": given})
        pl, info = m.policy_loss(db, tok[:, 1:].contiguous().to(DEV), torch.ones(B, device=DEV), given=given, entropy_coef=0.0)
    assert info["given_fraction"] == 0.5
    _two_ulp(loss.item(), pl.item(), m, db, "forward(given) against policy_loss(given)", given)
    _reset(m)


def test_evaluate(small):
    m, batch, tok, w = small
    _reset(m)
    db = dev_batch(batch)
    K = m.codebook_size
    m.set_loss(0.1, 1e-3, w)                                          # ignored: evaluate measures the model
    ev = m.evaluate(db, topk=(1, 5, K))
    m.set_loss()
    m.set_logprobs(True)
    m.score(db)
    lp = m.last_token_logprobs
    m.set_logprobs(False)
    assert torch.equal(ev["token_nll"].view(torch.int32), (-lp).view(torch.int32)), "token_nll == -score's last_token_logprobs by bits"
    tgt = tok[:, 1:].to(DEV)
    _, logits = m.teacher_forced_logits(db)
    am = ops.argmax(logits.reshape(-1, K), torch.empty(tgt.numel(), dtype=torch.int64, device=DEV), rows=tgt.numel(), K=K).view(tgt.shape)
    hit = am == tgt
    assert ev["token_nll"].shape == tgt.shape and ev["token_rank"].dtype == torch.int32 and ev["token_nll"].dtype == torch.float32
    assert torch.equal(ev["token_rank"] == 0, hit)
    assert abs(ev["accuracy"].item() - hit.float().mean().item()) <= 2.0 ** -23
    assert ev["topk_accuracy"][1].item() == ev["accuracy"].item() and ev["topk_accuracy"][K].item() == 1.0
    assert ev["accuracy"].item() <= ev["topk_accuracy"][5].item() <= 1.0
    assert abs(ev["nll"].item() - ev["token_nll"].double().mean().item()) <= 2.0 ** -23 * ev["nll"].item()
    assert ev["perplexity"].item() == ev["nll"].exp().item()
    assert abs(ev["mean_rank"].item() - ev["token_rank"].double().mean().item()) <= 1e-5 * K
    assert ev["frame_nll"].shape == (L - 1,) and ev["frame_nll"].dtype == torch.float32
    assert torch.allclose(ev["frame_nll"].double(), ev["token_nll"].double().mean((0, 2, 3)), rtol=1e-6, atol=0)
    assert torch.allclose(ev["frame_accuracy"].double(), hit.double().mean((0, 2, 3)), rtol=1e-6, atol=0)
    # a given slot is excluded
    given = _mask(1).to(DEV)
    given[0, 2, 3, 4] = True
    ex = m.evaluate(db, given=given)
    free = ~given
    assert (ex["token_nll"][given] == 0).all() and (ex["token_rank"][given] == 0).all()
    assert torch.equal(ex["token_nll"][free].view(torch.int32), ev["token_nll"][free].view(torch.int32))
    assert abs(ex["nll"].item() - ev["token_nll"][free].double().mean().item()) <= 2.0 ** -23 * ex["nll"].item()
    assert abs(ex["accuracy"].item() - hit[free].float().mean().item()) <= 2.0 ** -23
    assert ex["frame_nll"][0].item() == 0.0 and ex["frame_accuracy"][0].item() == 0.0       # frame 1 is given throughout
    n2 = free[:, 2].sum().item()
    assert abs(ex["frame_nll"][2].item() - (ev["token_nll"][:, 2] * free[:, 2]).double().sum().item() / n2) <= 1e-6 * ex["frame_nll"][2].item()
    # refusals
    m.set_guidance(2.0)
    with pytest.raises(ValueError, match="guidance is on"):
        m.evaluate(db)
    m.set_guidance(None)
    plus = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)
    for fn in (lambda: plus.evaluate(db), lambda: plus.set_loss(label_smoothing=0.1)):
        with pytest.raises(ValueError, match="use_cids=False"):
            fn()
    _reset(m)


def _loop(seed):
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), seed, DEV)
    m.eval()
    batch = dev_batch(synth.synth_batch_mnist(B, L, seed=seed, text_len=9, ragged_text=True))
    tok = m.first_stage_encode(batch["images"])
    m.set_loss(0.1, 1e-3, balanced_class_weights(m.first_stage_model.code_usage(tok)["counts"]))
    opt = FlatAdam(m.parameters(), lr=2e-4)
    hist = [m.evaluate(batch)["nll"].item()]
    for _ in range(20):
        opt.zero_grad()
        loss, _ = m(batch)
        loss.backward()
        opt.step()
    ev = m.evaluate(batch)
    return hist + [ev["nll"].item(), ev["accuracy"].item(), loss.item()]


def test_twenty_steps_lower_the_nll_and_repeat_bit_for_bit():
    a = _loop(43)
    print(f"20 FlatAdam steps with (0.1, 1e-3, balanced): evaluate()['nll'] {a[0]:.6f} -> {a[1]:.6f}, accuracy {a[2]:.4f}")
    assert a[1] < a[0]
    assert _loop(43) == a
