"""GPU: classifier-free guidance of token generation (MAGE.set_guidance, batch['guidance_scale'] / ['negative_text']) and caption dropout
(MAGE.caption_dropout, batch['caption_drop']).

Against the CPU oracle: the small fp32 model of tests/test_gpu_sampling.py.  The GPU's own tokens are teacher-forced through the oracle
under the caption and under the null caption, the two logit tensors are combined in fp64, g = c + (s - 1)(c - u) = s c + (1 - s) u, and
every generated token must be the guided argmax (or the restated sampler's draw) wherever the decision is not inside the noise.  The noise:
the project's gate is 1e-4 per logit against the oracle; a guided logit carries |s| + |s - 1| of that, a top-2 margin is a difference of two
such values: tol = 2e-4 (|s| + |s - 1|).  Positions at or under tol may differ; they must be at most 1 % of the tokens (on the oracle's
own trajectory 23 of 5 120 are, at scale 3, for exactly this model and batch; at scale 7.5 it is 60, past the cap: hence scale 3).

Bitwise invariants: BASELINE cfg2 in bf16 with 8 clips (sixteen decoder clips), sampling 1.0 / 50 / 0.95 with given seeds."""
import numpy as np
import pytest
import torch

from mage_amd.utils import synth
from mage_amd.utils.glue import null_caption
from oracle import mage_oracle as O
from tests import sampling_ref as R
from tests.helpers import build_mage, cpu_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 3.0
TOL = 2e-4 * (abs(SCALE) + abs(SCALE - 1.0))


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.fixture(scope="module")
def small():
    L, B, seed = 6, 4, 13
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), seed, DEV)
    return m, cpu_sd(m), synth.synth_batch_mnist(B, L, seed=seed)


def _oracle_guided(m, sd, batch, gen):
    """fp64 guided logits [B, L-1, h, w, K] of the oracle, teacher-forced on the GPU's own tokens `gen` under the default null caption."""
    Lm1 = m.frames_length - 1
    tok0 = O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, 0])
    assert torch.equal(tok0, m.first_stage_encode(batch["images"][:, 0:1].to(DEV))[:, 0].cpu())
    with torch.no_grad():
        feats = O._frame_features(sd, torch.cat([tok0[:, None], gen[:, :Lm1 - 1]], 1))
        c = O.flat_axial_decoder(sd, "generate_model.", O.motion_anchor(sd, tok0, batch["text"], batch.get("speed")), feats).double()
        u = O.flat_axial_decoder(sd, "generate_model.", O.motion_anchor(sd, tok0, null_caption(batch["text"], 0), batch.get("speed")),
                                 feats).double()
    return (c + (SCALE - 1.0) * (c - u)).numpy()


def _frames_ok(m, sd, batch, video, gen):
    B, Lm1, R_ = gen.shape[0], gen.shape[1], m.image_resolution
    with torch.no_grad():
        want = O.vqvae_decode(sd, "first_stage_model.", gen.view(B * Lm1, R_, R_)).view(B, Lm1, *video.shape[2:])
    assert (video[:, 1:] - want).abs().max().item() <= 1e-4
    assert torch.equal(video[:, 0], batch["images"][:, 0])


@pytest.mark.parametrize("mode", ["full", "incremental"])
def test_greedy_guided_generation_matches_oracle(small, mode):
    m, sd, batch = small
    m.set_precision("fp32").set_sampling(None).set_guidance(SCALE)
    m.use_graph, m.ar_mode = False, mode
    try:
        video = m.autoregressive_generate(dev_batch(batch)).cpu()
        gen = m.last_tokens.cpu()
        logits = None if m.last_logits is None else m.last_logits.cpu()
        assert torch.equal(m.last_guidance_scale.cpu(), torch.full((4,), SCALE))
    finally:
        m.set_guidance(None)
        m.ar_mode = "full"
    g = _oracle_guided(m, sd, batch, gen)
    top2 = np.sort(g, axis=-1)[..., -2:]
    margin = top2[..., 1] - top2[..., 0]
    want = g.argmax(-1)
    bad = gen.numpy() != want
    n, under = bad.size, int((margin <= TOL).sum())
    print(f"{mode}: {n} tokens, {int(bad.sum())} differ from the oracle's guided argmax, {under} positions with a top-2 margin <= tol {TOL:.1e}")
    assert not (bad & (margin > TOL)).any(), f"{int((bad & (margin > TOL)).sum())} tokens differ where the guided margin exceeds {TOL}"
    assert under <= n // 100
    if logits is not None:                                         # the full loop keeps the guided logits of every frame
        err = np.abs(logits.double().numpy() - g).max()
        print(f"{mode}: max |last_logits - fp64 guided logits| {err:.3e} (bound {TOL / 2:.1e})")
        assert err <= TOL / 2
    else:
        assert mode == "incremental"
    _frames_ok(m, sd, batch, video, gen)


@pytest.mark.parametrize("mode", ["full", "incremental"])
def test_sampled_guided_generation_matches_oracle(small, mode):
    m, sd, batch = small
    T, k, p = 0.9, 20, 0.9
    seeds = torch.tensor([1, -2, 3 ** 30, 99], dtype=torch.int64)
    m.set_precision("fp32").set_sampling(T, top_k=k, top_p=p).set_guidance(SCALE)
    m.use_graph, m.ar_mode = False, mode
    try:
        video = m.autoregressive_generate(dev_batch({**batch, "sample_seed": seeds})).cpu()
        gen = m.last_tokens.cpu()
    finally:
        m.set_guidance(None).set_sampling(None)
        m.ar_mode = "full"
    g = _oracle_guided(m, sd, batch, gen)
    B, Lm1, R_ = gen.shape[0], gen.shape[1], m.image_resolution
    hw = R_ * R_
    tol = TOL * float(R.inv_temperature(T))
    hard = soft = 0
    for b in range(B):
        for i in range(Lm1):
            for px in range(hw):
                want, near = R.sample_row(g[b, i, px // R_, px % R_], T, k, p, int(seeds[b]), i * hw + px, tol)
                if int(gen[b, i, px // R_, px % R_]) != want:
                    soft, hard = soft + near, hard + (not near)
    print(f"{mode} T={T} top_k={k} top_p={p}: {B * Lm1 * hw} tokens, hard mismatches {hard}, soft {soft}")
    assert hard == 0 and soft <= max(5, B * Lm1 * hw // 1000)
    _frames_ok(m, sd, batch, video, gen)


# ---------------------------------------------------------------------------------------------------- bitwise invariants, cfg2 bf16
@pytest.fixture(scope="module")
def cfg2():
    m = build_mage(synth.mnist_model_config(frames_length=16), 0, DEV).set_precision("bf16")
    batch = dev_batch(synth.synth_batch_mnist(8, 16, seed=3))
    seeds = torch.arange(8, dtype=torch.int64, device=DEV) * 7919 - 12345
    return m, batch, seeds


def _reset(m):
    m.set_guidance(None).set_sampling(None).set_logprobs(False)
    m.use_graph, m.streams, m.ar_mode = False, 1, "incremental"


def _run(m, batch, seeds=None, **extra):
    b = {**batch, **extra}
    if seeds is not None:
        b["sample_seed"] = seeds
    v = m.autoregressive_generate(b)
    return v, m.last_tokens.clone()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cfg2_scale_one_and_equal_captions_are_the_unguided_call(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    m.ar_mode = "full"
    g0 = _run(m, batch)                                                               # greedy, before guidance was ever switched on
    m.set_sampling(1.0, top_k=50, top_p=0.95)
    s0 = _run(m, batch, seeds)
    l0 = m.last_logits.clone()
    assert m.last_guidance_scale is None
    m.set_guidance(1.0)
    s1 = _run(m, batch, seeds)
    assert _same(s1, s0) and torch.equal(m.last_logits.view(torch.int32), l0.view(torch.int32))     # scale 1: bit for bit
    assert m.last_logits.shape == l0.shape and torch.equal(m.last_guidance_scale, torch.ones(8, device=DEV))
    m.set_guidance(7.5)
    s2 = _run(m, batch, seeds, negative_text=batch["text"])
    assert _same(s2, s0) and torch.equal(m.last_logits.view(torch.int32), l0.view(torch.int32))     # uncond == cond: bit for bit
    m.ar_mode = "incremental"
    assert _same(_run(m, batch, seeds, negative_text=batch["text"]), s0)
    # ... and switching it off restores the greedy and the sampled call
    m.set_guidance(None)
    m.ar_mode = "full"
    assert _same(_run(m, batch, seeds), s0) and m.last_guidance_scale is None
    m.set_sampling(None)
    assert _same(_run(m, batch), g0)
    m.ar_mode = "incremental"
    assert _same(_run(m, batch, guidance_scale=torch.full((8,), 9.0, device=DEV)), g0)                  # the keys are ignored while it is off
    _reset(m)


def test_cfg2_guided_invariants(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    m.set_sampling(1.0, top_k=50, top_p=0.95)
    base = _run(m, batch, seeds)                                                      # unguided
    m.set_guidance(3.0)
    gi = _run(m, batch, seeds)
    changed = (gi[1] != base[1]).flatten(1).any(1).float().mean().item()
    print(f"cfg2 bf16: clips changed by scale 3 against the null caption {changed:.3f}")
    assert changed > 0.5                                                              # scale 3 changes most clips
    m.ar_mode = "full"
    assert _same(_run(m, batch, seeds), gi)                                           # full loop == incremental loop
    m.ar_mode = "incremental"
    sl = {k_: v[2:6] for k_, v in batch.items()}
    part = _run(m, sl, seeds[2:6])
    assert torch.equal(part[0], gi[0][2:6]) and torch.equal(part[1], gi[1][2:6])      # a slice of clips alone == the same slice
    m.streams = 2
    assert _same(_run(m, batch, seeds), gi)                                           # two streams == one
    m.streams = 1
    # the per-clip tensor: filled with 3 it is set_guidance(3.0); mixed, every clip gets what it gets alone
    m.set_guidance(1.0)
    assert _same(_run(m, batch, seeds, guidance_scale=torch.full((8,), 3.0, device=DEV)), gi)
    mixed = torch.tensor([3.0, 1.0, 7.5, 3.0, -0.5, 1.0, 3.0, 0.0], device=DEV)
    mx = _run(m, batch, seeds, guidance_scale=mixed)
    assert torch.equal(m.last_guidance_scale, mixed)
    for b in (0, 3, 6):
        assert torch.equal(mx[1][b], gi[1][b]) and torch.equal(mx[0][b], gi[0][b])
    for b in (1, 5):
        assert torch.equal(mx[1][b], base[1][b])
    for b in (2, 4):
        one = _run(m, {k_: v[b:b + 1] for k_, v in batch.items()}, seeds[b:b + 1], guidance_scale=mixed[b:b + 1])
        assert torch.equal(one[1][0], mx[1][b]) and torch.equal(one[0][0], mx[0][b])
    # an explicit negative caption that differs from the null caption changes the result
    m.set_guidance(3.0)
    neg = batch["text"].roll(1, 0)
    assert not torch.equal(neg, null_caption(batch["text"], 0))
    assert not torch.equal(_run(m, batch, seeds, negative_text=neg)[1], gi[1])
    _reset(m)


def test_cfg2_guided_candidates_and_logprobs(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    m.set_guidance(3.0).set_sampling(1.0, top_k=50, top_p=0.95).set_logprobs(True, policy=True, entropy=True)
    plain = []
    for c in range(3):
        v, t = _run(m, batch, seeds + c)
        plain.append((v, t, m.last_clip_logprob.clone()))
    _run(m, batch, seeds)
    lp, plp, kept = m.last_token_logprobs, m.last_token_policy_logprobs, m.last_token_kept
    assert lp.shape == plp.shape == kept.shape == plain[0][1].shape and m.last_token_entropy.shape == lp.shape
    assert bool(torch.isfinite(plp).all()) and bool((kept >= 1).all())               # every kept token: finite, never -inf
    assert bool(torch.isfinite(lp).all()) and bool((m.last_token_policy_entropy >= 0).all())
    m.set_sampling(1.0, top_k=50, top_p=0.95, candidates=3)
    v, t = _run(m, batch, seeds)
    scores, idx = m.last_candidate_scores, m.last_candidate_index
    assert scores.shape == (8, 3) and t.shape == plain[0][1].shape and m.last_token_logprobs.shape == t.shape
    for c in range(3):                                                                # candidate c is the candidates = 1 call under seed + c
        assert torch.equal(scores[:, c].view(torch.int32), plain[c][2].view(torch.int32))
    for b in range(8):
        w = plain[int(idx[b])]
        assert torch.equal(t[b], w[1][b]) and torch.equal(v[b], w[0][b])
    m.ar_mode = "full"
    assert _same(_run(m, batch, seeds), (v, t)) and torch.equal(m.last_candidate_scores, scores)
    _reset(m)


def test_cfg2_guided_graph_replay_equals_eager(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    two = {k_: v[:2] for k_, v in batch.items()}
    m.set_guidance(3.0).set_sampling(1.0, top_k=50, top_p=0.95)
    eager = _run(m, two, seeds[:2])
    gs2 = torch.tensor([7.5, 0.5], device=DEV)
    neg2 = batch["text"][2:4].clone()
    eager2 = _run(m, two, seeds[:2], guidance_scale=gs2, negative_text=neg2)
    assert not torch.equal(eager2[1], eager[1])
    m.use_graph = True
    ones = torch.full((2,), 3.0, device=DEV)
    null2 = null_caption(two["text"], 0)
    for rep in range(3):                                                              # warm-up (eager), capture + replay, replay
        assert _same(_run(m, two, seeds[:2], guidance_scale=ones, negative_text=null2), eager), (rep, m.last_call_mode)
    assert m.last_call_mode == "graph"
    assert _same(_run(m, two, seeds[:2], guidance_scale=gs2, negative_text=neg2), eager2)     # new scales, new caption: the same graph
    assert m.last_call_mode == "graph" and torch.equal(m.last_guidance_scale, gs2)
    m.use_graph = None                                                                # auto: 2 x 2 clips x 256 positions is still launch-bound
    assert m._graph_auto({**two, "sample_seed": seeds[:2]}) and not m._graph_auto({k_: v[:3] for k_, v in batch.items()})
    _reset(m)
    m.use_graph = None


def test_cater_randomness_guided():
    L, B = 6, 2
    m = build_mage(synth.cater_model_config(frames_length=L), 0, DEV).set_precision("bf16")
    cb = synth.synth_batch_cater(B, L, seed=2)
    cb["video_noise"] = torch.randn(B, 64, 16, 16, generator=torch.Generator().manual_seed(5))
    cb["sample_seed"] = torch.tensor([17, -4], dtype=torch.int64)
    batch = dev_batch(cb)
    m.set_sampling(0.9, top_k=40, top_p=0.95)
    m.use_graph = False
    v0 = m.autoregressive_generate(batch)
    t0 = m.last_tokens.clone()
    m.set_guidance(3.0)
    v = m.autoregressive_generate(batch)
    tk = m.last_tokens.clone()
    assert m.last_video_noise.shape == (B, 64, 16, 16) and torch.equal(m.last_video_noise, batch["video_noise"])
    m.ar_mode = "incremental"
    vi = m.autoregressive_generate(batch)
    assert torch.equal(m.last_tokens, tk) and torch.equal(vi, v) and bool(torch.isfinite(v).all())    # guided full == guided incremental
    assert not torch.equal(tk, t0)
    m.set_guidance(7.5)
    ve = m.autoregressive_generate({**batch, "negative_text": batch["text"]})
    assert torch.equal(m.last_tokens, t0) and torch.equal(ve, v0)                     # negative_text = text: the unguided call
    # seeded noise and torch.randn: the negative half shares the clip's draw (B clips of noise, not 2 B)
    nb = {k_: v_ for k_, v_ in batch.items() if k_ != "video_noise"}
    m.autoregressive_generate({**nb, "noise_seed": torch.tensor([5, 6], dtype=torch.int64), "negative_text": batch["text"]})
    tn = m.last_tokens.clone()
    assert m.last_video_noise.shape == (B, 64, 16, 16)
    m.set_guidance(None)
    m.autoregressive_generate({**nb, "noise_seed": torch.tensor([5, 6], dtype=torch.int64)})
    assert torch.equal(m.last_tokens, tn)
    m.set_guidance(2.0)
    m.autoregressive_generate(nb)
    assert m.last_video_noise.shape == (B, 64, 16, 16)


def test_refusals_leave_the_model_usable(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    two = {k_: v[:2] for k_, v in batch.items()}
    m.set_sampling(1.0, top_k=50, top_p=0.95)
    want = _run(m, two, seeds[:2])
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, "3", True):
        with pytest.raises(ValueError, match="set_guidance"):
            m.set_guidance(bad)
    assert m.guidance is None
    plus = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0, DEV)
    with pytest.raises(ValueError, match="use_cids=False"):
        plus.set_guidance(2.0)
    plus.set_guidance(None)
    m.set_guidance(3.0)
    ok = _run(m, two, seeds[:2])
    for key, val in (("negative_text", two["text"][:, :-1]), ("negative_text", two["text"][:1]), ("negative_text", two["text"].int()),
                     ("guidance_scale", torch.ones(3, device=DEV)), ("guidance_scale", torch.ones(2, 1, device=DEV)),
                     ("guidance_scale", torch.ones(2, device=DEV, dtype=torch.float64))):
        with pytest.raises(ValueError, match=key):
            m.autoregressive_generate({**two, "sample_seed": seeds[:2], key: val})
    R_, Lm1 = m.image_resolution, m.frames_length - 1
    tokens = torch.zeros(2, Lm1, R_, R_, dtype=torch.int64, device=DEV)
    for name, call in (("score", lambda: m.score(two)), ("policy_loss", lambda: m.policy_loss(two, tokens, torch.ones(2, device=DEV))),
                       ("token_policy_logprobs", lambda: m.token_policy_logprobs(two, tokens)), ("rollout", lambda: m.rollout(two, 2))):
        with pytest.raises(ValueError, match=f"{name}: classifier-free guidance"):
            call()
    assert _same(_run(m, two, seeds[:2]), ok)                                         # still usable, same result
    m.set_guidance(None)
    assert _same(_run(m, two, seeds[:2]), want)
    assert m.score(two).shape == (2,)                                                 # and the refused calls work again
    _reset(m)


# ---------------------------------------------------------------------------------------------------- caption dropout
def _loss_and_grads(m, b, seed=77):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)                                                           # the dropout seeds come from the CPU generator
    loss, _ = m(b)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _equal(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def test_caption_dropout(small):
    m, _, batch = small
    m.set_precision("fp32").set_sampling(None).set_guidance(None)
    b = dev_batch(batch)
    m.train()
    try:
        plain = _loss_and_grads(m, b)
        assert m.last_caption_drop is None and len(plain[1]) > 50
        none = _loss_and_grads(m, {**b, "caption_drop": torch.zeros(4, dtype=torch.bool)})
        assert _equal(none, plain) and torch.equal(m.last_caption_drop.cpu(), torch.zeros(4, dtype=torch.bool))
        mask = torch.tensor([True, False, True, False])
        got = _loss_and_grads(m, {**b, "caption_drop": mask})
        assert torch.equal(m.last_caption_drop.cpu(), mask) and m.last_caption_drop.device == b["text"].device
        by_hand = b["text"].clone()
        by_hand[mask.to(DEV)] = null_caption(b["text"], 0)[mask.to(DEV)]
        assert not torch.equal(by_hand, b["text"])
        want = _loss_and_grads(m, {**b, "text": by_hand})
        assert _equal(got, want) and not torch.equal(got[0], plain[0])
        # the draw: torch's CPU generator, reproduced by torch.manual_seed
        m.caption_dropout = 0.5
        torch.manual_seed(4242)
        drawn = torch.rand(4) < 0.5
        assert drawn.any() and not drawn.all()
        got = _loss_and_grads(m, b, seed=4242)
        assert torch.equal(m.last_caption_drop.cpu(), drawn)
        torch.manual_seed(4242)
        torch.rand(4)                                                                 # (the mask's draw comes before the dropout seeds)
        state = torch.get_rng_state()
        m.caption_dropout = 0.0
        m.zero_grad(set_to_none=True)
        torch.set_rng_state(state)
        loss, _ = m({**b, "caption_drop": drawn})
        loss.backward()
        assert torch.equal(loss.detach(), got[0]) and all(torch.equal(p.grad, got[1][n]) for n, p in m.named_parameters() if p.grad is not None)
        # eval(): the probability is ignored, a given mask still applies
        m.caption_dropout = 1.0
        m.eval()
        with torch.no_grad():
            e0, _ = m(b)
            assert m.last_caption_drop is None
            m.caption_dropout = 0.0
            e1, _ = m(b)
            e2, _ = m({**b, "caption_drop": mask})
            e3, _ = m({**b, "text": by_hand})
        assert torch.equal(e0, e1) and torch.equal(e2, e3) and not torch.equal(e2, e1)
        for bad in (1.5, -0.1, "0.5", True):
            m.caption_dropout = bad
            with pytest.raises(ValueError, match="caption_dropout"):
                m(b)
        m.caption_dropout = 0.0
        with pytest.raises(ValueError, match="caption_drop"):
            m({**b, "caption_drop": torch.zeros(3, dtype=torch.bool)})
        with pytest.raises(ValueError, match="caption_drop"):
            m({**b, "caption_drop": torch.zeros(4)})
    finally:
        m.caption_dropout = 0.0
        m.eval()
        m.zero_grad(set_to_none=True)
