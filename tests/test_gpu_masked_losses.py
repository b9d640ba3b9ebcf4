"""GPU: given= on the loss methods (score, policy_loss, token_policy_logprobs, preference_loss, clip_logprobs) and MAGE.rollout(context=,
known_tokens=), on tests/test_gpu_rollout.py's small model (L = 5, 3 clips, 2 candidates).

Bounds.
  given all-False: bit identity with the call without given -- values, info and every parameter gradient, in fp32 and bf16 (the masked kernels
    run the unmasked kernels' operations on a free row, and 1.0f / (float)n_free is 1.0f / (float)rows).
  teacher-forced against rollout log-probabilities at the free slots: 1e-3, the bound and the reasoning of
    tests/test_gpu_rollout.py::test_policy_loss_consumes_it (both passes are held to 1e-4 logits against the oracle, two paths x (logit +
    log-sum-exp) = 4e-4, with 2.5x margin); given slots: exactly 0.
  clip totals: the fp64 sum of the call's own per-token values over the free slots, rounded once: 2 ulp (mage_clip_scores adds in fp64).
  masking == zero advantage: loss_masked * n_free against loss_unmasked * rows and every gradient tensor after the same rescale, within
    2 * 1e-5 * max|grad| per tensor (token_stats_ref.TOL, the project's allowance for fixed-order fp32 sums; the two runs differ in the one
    normaliser, 1 / n_free against 1 / rows, rounded at different places)."""
import numpy as np
import pytest
import torch

from mage_amd.utils import synth
from tests import token_stats_ref as TS
from tests.helpers import build_mage, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, N, TEMP, CTX = 5, 3, 2, 0.9, 3
SEEDS = [11, 12, 13]


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _reset(m, ar_mode="full"):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32").set_context(1)
    m.ar_mode = ar_mode
    m.eval()
    m.zero_grad(set_to_none=True)


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), 41, DEV)
    batch = dev_batch({**synth.synth_batch_mnist(B, L, seed=41, text_len=9, ragged_text=True), "sample_seed": torch.tensor(SEEDS, dtype=torch.int64)})
    return m, batch


def _region(m, batch):
    """known_tokens with one fixed region: rows 4 .. 7, columns 2 .. 9 of every frame hold the ground truth's VQ tokens, the rest is free."""
    R_ = m.image_resolution
    truth = m.first_stage_encode(batch["images"][:, 1:L]).reshape(B, L - 1, R_, R_)
    known = torch.full_like(truth, -1)
    known[:, :, 4:8, 2:10] = truth[:, :, 4:8, 2:10]
    return known


@pytest.fixture(scope="module")
def rolled(small):
    """One plain rollout, one continued (context=3) per ar_mode and one around a fixed region, shared and left unchanged by the tests."""
    m, batch = small
    out = {}
    _reset(m)
    m.set_sampling(TEMP)
    out["plain"] = m.rollout(batch, N)
    out["known_tokens"] = _region(m, batch)
    out["region"] = m.rollout(batch, N, known_tokens=out["known_tokens"])
    for mode in ("full", "incremental"):
        _reset(m, mode)
        m.set_sampling(TEMP)
        out[mode] = m.rollout(batch, N, context=CTX)
    _reset(m)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _grads(m):
    g = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


def _pairs_and_ref(m, out):
    with torch.no_grad():
        ref = m.clip_logprobs(out["batch"], out["tokens"])
    ref = ref + torch.linspace(-0.5, 0.5, B * N, device=DEV)
    return torch.tensor([[0, 1], [3, 2], [4, 4]], dtype=torch.int64, device=DEV), ref.contiguous()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_all_false_is_the_unmasked_call(small, rolled, precision):
    m, batch = small
    out = rolled["plain"]
    assert out["given"] is None
    _reset(m)
    m.set_precision(precision).set_sampling(TEMP, top_k=20).set_logprobs(True, policy=True, entropy=True)
    free = torch.zeros(B, L - 1, m.image_resolution, m.image_resolution, dtype=torch.bool, device=DEV)
    freeN = free.repeat_interleave(N, 0)
    try:
        res = []
        for kw in ({}, {"given": free}):
            s = m.score(batch, **kw)
            res.append([s] + [getattr(m, a) for a in ("last_token_logprobs", "last_token_policy_logprobs", "last_token_kept", "last_token_entropy",
                                                      "last_token_policy_entropy", "last_clip_policy_logprob")])
        assert all(torch.equal(a, b) for a, b in zip(*res))
        b_, t_ = out["batch"], out["tokens"]
        assert torch.equal(_bits(m.clip_logprobs(b_, t_)), _bits(m.clip_logprobs(b_, t_, given=freeN)))
        assert torch.equal(_bits(m.token_policy_logprobs(b_, t_)), _bits(m.token_policy_logprobs(b_, t_, given=freeN)))
        pairs, ref = _pairs_and_ref(m, out)
        refp = (out["behaviour_logprobs"] - 0.05).contiguous()
        calls = [lambda kw: m.policy_loss(b_, t_, out["advantages"], out["behaviour_logprobs"], entropy_coef=0.01, **kw),
                 lambda kw: m.policy_loss(b_, t_, out["advantages"], **kw),
                 lambda kw: m.policy_loss(b_, t_, out["advantages"], out["behaviour_logprobs"], reference_logprobs=refp, kl_coef=0.1, **kw),
                 lambda kw: m.preference_loss(b_, t_, pairs, ref, **kw)]
        for call in calls:
            loss0, info0 = call({})
            loss0.backward()
            g0 = _grads(m)
            loss1, info1 = call({"given": freeN})
            loss1.backward()
            g1 = _grads(m)
            assert torch.equal(_bits(loss0.detach()), _bits(loss1.detach()))
            assert info1.pop("given_fraction") == 0.0 and info1 == info0
            assert g0.keys() == g1.keys() and len(g0) >= 90 and all(torch.equal(_bits(g0[n]), _bits(g1[n])) for n in g0)
    finally:
        _reset(m)


def _settings(m):
    return (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.precision, m.ar_mode, m.context_frames)


@pytest.mark.parametrize("ar_mode", ["full", "incremental"])
def test_rollout_continues_given_frames(small, rolled, ar_mode):
    m, batch = small
    out = rolled[ar_mode]
    R_ = m.image_resolution
    truth = m.first_stage_encode(batch["images"][:, 1:CTX]).reshape(B, CTX - 1, R_, R_).repeat_interleave(N, 0)
    assert out["tokens"].shape == (B * N, L - 1, R_, R_) and torch.equal(out["tokens"][:, :CTX - 1], truth)
    g = out["given"]
    assert g.dtype == torch.bool and g.shape == out["tokens"].shape and bool(g[:, :CTX - 1].all()) and not bool(g[:, CTX - 1:].any())
    assert bool((out["behaviour_logprobs"][g] == 0).all()) and bool((out["token_logprobs"][g] == 0).all())
    assert bool((out["behaviour_logprobs"][~g] < 0).any())
    fm = out["frame_metrics"]
    assert all(v.shape == (B * N, L - CTX) for v in fm.values())
    direct = m.video_metrics(out["video"][:, CTX:], batch["images"].repeat_interleave(N, 0)[:, CTX:])
    assert all(torch.equal(_bits(fm[k]), _bits(direct[k])) for k in fm)                 # the generated frames alone are rewarded
    assert torch.equal(out["video"][:, :CTX], batch["images"][:, :CTX].repeat_interleave(N, 0))      # the given frames, verbatim
    assert "known_tokens" not in out["batch"] and "context_tokens" not in out["batch"] and out["batch"]["images"].shape[:2] == (B * N, 1)
    assert len({tuple(t.flatten().tolist()) for t in out["tokens"][:N, CTX - 1:]}) > 1  # the candidates' continuations differ
    # the settings and the results are as found
    _reset(m, ar_mode)
    m.set_sampling(TEMP, top_k=20).set_logprobs(True)
    m.autoregressive_generate(batch)
    before, last = _settings(m), {a: v for a, v in vars(m).items() if a.startswith("last_")}
    m.rollout(batch, N, context=CTX)
    now = {a: v for a, v in vars(m).items() if a.startswith("last_")}
    assert _settings(m) == before and m.context_frames == 1 and now.keys() == last.keys() and all(now[a] is last[a] for a in last)
    with pytest.raises(ValueError, match="reward callable"):        # a failure after the generation restores them too
        m.rollout(batch, N, context=CTX, reward=lambda v, b: torch.zeros(B, device=DEV))
    assert _settings(m) == before and all(getattr(m, a) is last[a] for a in last)
    _reset(m)


def test_rollout_around_known_tokens(small, rolled):
    m, batch = small
    out, known = rolled["region"], rolled["known_tokens"]
    kN = known.repeat_interleave(N, 0)
    g = out["given"]
    assert torch.equal(g, kN >= 0) and torch.equal(out["tokens"][g], kN[g]) and 0 < int(g.sum()) < g.numel()
    assert bool((out["behaviour_logprobs"][g] == 0).all()) and bool((out["token_logprobs"][g] == 0).all())
    assert all(v.shape == (B * N, L - 1) for v in out["frame_metrics"].values())     # every frame holds free slots: all L-1 are rewarded
    direct = m.video_metrics(out["video"][:, 1:], batch["images"].repeat_interleave(N, 0)[:, 1:])
    assert all(torch.equal(_bits(out["frame_metrics"][k]), _bits(direct[k])) for k in direct)
    assert "known_tokens" not in out["batch"] and "context_tokens" not in out["batch"]
    assert not torch.equal(out["tokens"], rolled["plain"]["tokens"])
    _reset(m)
    m.set_sampling(TEMP)
    with torch.no_grad():
        loss, info = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"], given=g)
    assert info["given_fraction"] == float(np.float32(int(g.sum()) / g.numel())) and info["clip_fraction"] == 0.0
    assert bool((m.last_policy_token_logprobs[g] == 0).all())
    _reset(m)


@pytest.mark.parametrize("ar_mode", ["full", "incremental"])
def test_policy_loss_over_the_free_tokens(small, rolled, ar_mode):
    m, _ = small
    out = rolled[ar_mode]
    g = out["given"]
    _reset(m, ar_mode)
    m.set_sampling(TEMP)
    ref = (out["behaviour_logprobs"] - 0.02 * (~g)).contiguous()
    with torch.no_grad():
        loss, info = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"], reference_logprobs=ref, kl_coef=0.1,
                                   given=g)
    lp = m.last_policy_token_logprobs
    d = (lp - out["behaviour_logprobs"])[~g].abs().max().item()
    print(f"{ar_mode}: max |teacher-forced - rollout| policy log-probability over the free slots {d:.3e}; info {info}")
    assert not loss.requires_grad and bool((lp[g] == 0).all()) and bool((m.last_policy_token_kl[g] == 0).all())
    assert d < 1e-3 and info["clip_fraction"] == 0.0 and info["outside_fraction"] == 0.0
    assert info["given_fraction"] == (CTX - 1) / (L - 1) and info["kl"] > 0
    loss, _ = m.policy_loss(out["batch"], out["tokens"], out["advantages"], out["behaviour_logprobs"], given=g)
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


def test_clip_totals_are_over_the_free_slots(small, rolled):
    m, _ = small
    out = rolled["full"]
    g = out["given"]
    _reset(m)
    pairs, ref = torch.tensor([[0, 1]], dtype=torch.int64, device=DEV), torch.zeros(B * N, device=DEV)
    with torch.no_grad():
        m.preference_loss(out["batch"], out["tokens"], pairs, ref, given=g)
        tok_lp, clip_lp = m.last_preference_token_logprobs, m.last_preference_clip_logprobs
        got = m.clip_logprobs(out["batch"], out["tokens"], given=g)
    assert torch.equal(_bits(got), _bits(clip_lp)) and bool((tok_lp[g] == 0).all())
    want = torch.where(g, 0.0, tok_lp.double()).flatten(1).sum(1).cpu().numpy()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32))
    # against the generation's own report: one 1e-3 (test_policy_loss_consumes_it's per-token bound) per free token
    gen = torch.where(g, 0.0, out["token_logprobs"].double()).flatten(1).sum(1).cpu().numpy()
    n_free = int((~g[0]).sum())
    print(f"clip totals: {err.max():.2f} ulp against the fp64 sum of the free tokens; |teacher-forced - generation| {np.abs(want - gen).max():.3e} "
          f"(bound {1e-3 * n_free:.3e})")
    assert err.max() <= 2 and np.abs(want - gen).max() <= 1e-3 * n_free
    # score(given=) of the batch's own video: the same mechanism -- 0 at the given slots, totals over the free tokens
    m, batch = small
    g1 = g[::N].contiguous()
    m.set_sampling(TEMP).set_logprobs(True, policy=True, entropy=True)
    scored = m.score(batch, given=g1)
    for a, v in (("last_token_logprobs", 0), ("last_token_policy_logprobs", 0), ("last_token_entropy", 0), ("last_token_policy_entropy", 0),
                 ("last_token_kept", 1)):
        assert bool((getattr(m, a)[g1] == v).all()), a
    for tot, per in ((scored, m.last_token_logprobs), (m.last_clip_policy_logprob, m.last_token_policy_logprobs)):
        want = torch.where(g1, 0.0, per.double()).flatten(1).sum(1).cpu().numpy()
        assert (np.abs(tot.cpu().numpy().astype(np.float64) - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all()
    _reset(m)


def test_masking_equals_zero_advantage(small, rolled):
    m, _ = small
    out = rolled["full"]
    _reset(m)
    g = out["given"].clone()
    g[:, CTX - 1:, ::3, 1::2] = True                                # some slots of the generated frames too
    rows, n_free = g.numel(), int((~g).sum())
    A = (torch.rand(g.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) + 0.5) * torch.where(
        torch.arange(g.numel(), device=DEV).view(g.shape) % 3 == 0, -1.0, 1.0)
    loss_m, info = m.policy_loss(out["batch"], out["tokens"], A, given=g)
    loss_m.backward()
    gm = _grads(m)
    loss_u, _ = m.policy_loss(out["batch"], out["tokens"], (A * ~g).contiguous())
    loss_u.backward()
    gu = _grads(m)
    assert info["given_fraction"] == float(np.float32((rows - n_free) / rows))
    a, b = loss_m.item() * n_free, loss_u.item() * rows
    worst = abs(a - b) / (2 * TS.TOL * abs(b))
    assert gm.keys() == gu.keys() and len(gm) >= 90
    for n in gm:
        x, y = gm[n].double() * n_free, gu[n].double() * rows
        bound = 2 * TS.TOL * y.abs().max().item()
        worst = max(worst, ((x - y).abs().max().item() / bound) if bound else float((x - y).abs().max().item() > 0))
    print(f"masking against zero advantages: largest error / bound {worst:.3e} (loss {a:.6f} against {b:.6f})")
    assert worst <= 1.0
    _reset(m)


def test_preference_loss_leaves_the_given_slots_out(small, rolled):
    m, _ = small
    out = rolled["full"]
    _reset(m)
    pairs, ref = _pairs_and_ref(m, out)                              # clips 0 .. 4 are in pairs; clip 5 is in none
    g = torch.zeros_like(out["given"])
    g[5] = True
    loss0, info0 = m.preference_loss(out["batch"], out["tokens"], pairs, ref)
    loss0.backward()
    g0 = _grads(m)
    loss1, info1 = m.preference_loss(out["batch"], out["tokens"], pairs, ref, given=g)
    loss1.backward()
    g1 = _grads(m)
    assert m.last_preference_clip_logprobs[5].item() == 0.0 and bool((m.last_preference_token_logprobs[5] == 0).all())
    assert info1.pop("given_fraction") == 1 / (B * N) and info1 == info0 and torch.equal(_bits(loss0.detach()), _bits(loss1.detach()))
    assert g0.keys() == g1.keys() and all(torch.equal(_bits(g0[n]), _bits(g1[n])) for n in g0)
    # a mask inside the pairs' clips changes the loss: the given frames drop out of the log-likelihoods
    with torch.no_grad():
        _, info2 = m.preference_loss(out["batch"], out["tokens"], pairs, ref, given=out["given"])
    assert info2["given_fraction"] == (CTX - 1) / (L - 1) and info2["margin"] != info0["margin"]
    _reset(m)


def test_refusals_launch_nothing(small, rolled, monkeypatch):
    m, batch = small
    out = rolled["full"]
    _reset(m)
    m.set_sampling(TEMP)
    g, b_, t_ = out["given"], out["batch"], out["tokens"]
    pairs, ref = torch.tensor([[0, 1]], dtype=torch.int64, device=DEV), torch.zeros(B * N, device=DEV)
    video = {**b_, "images": out["video"]}
    calls = count_lib_calls(monkeypatch)
    bad = [g.to(torch.uint8), g.float(), g[:, 1:], g[:B], g.cpu(), g.tolist()]
    methods = [lambda x: m.score(video, given=x), lambda x: m.policy_loss(b_, t_, out["advantages"], given=x),
               lambda x: m.token_policy_logprobs(b_, t_, given=x), lambda x: m.preference_loss(b_, t_, pairs, ref, given=x),
               lambda x: m.clip_logprobs(b_, t_, given=x)]
    for call in methods:
        for x in bad:
            with pytest.raises(ValueError, match="given"):
                call(x)
            assert calls == []
    m.use_cids = False
    try:
        for call in methods:
            with pytest.raises(ValueError, match="use_cids=False"):
                call(g)
            assert calls == []
    finally:
        m.use_cids = True
    before = _settings(m)
    R_ = m.image_resolution
    for kw, match in ((dict(context=L), "context"), (dict(context=0), "context"), (dict(context=True), "context"), (dict(context=2.0), "context"),
                      (dict(known_tokens=torch.zeros(B, L, R_, R_, dtype=torch.int64, device=DEV)), "known_tokens"),
                      (dict(known_tokens=torch.zeros(B, L - 1, R_, R_, dtype=torch.int32, device=DEV)), "known_tokens"),
                      (dict(known_tokens=torch.zeros(B, L - 1, R_, R_, dtype=torch.int64)), "known_tokens")):
        with pytest.raises(ValueError, match=match):
            m.rollout(batch, N, **kw)
        assert calls == [] and _settings(m) == before
    # the setting and the batch keys are still refused, with the words the earlier tests match
    m.set_context(2)
    with pytest.raises(ValueError, match="policy_loss: given frames or tokens"):
        m.policy_loss(b_, t_, out["advantages"], given=g)
    m.set_context(1)
    with pytest.raises(ValueError, match="rollout: given frames or tokens"):
        m.rollout({**batch, "known_tokens": rolled["known_tokens"]}, N)
    assert calls == []
    monkeypatch.undo()
    _reset(m)
