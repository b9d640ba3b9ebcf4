"""GPU: generation conditioned on given frames (MAGE.set_context) and given tokens (batch['known_tokens']) against the CPU oracle.

The small fp32 model of tests/test_gpu_guidance.py.  The GPU's own tokens are teacher-forced through the oracle (tests/known_ref.py): forced
slots must hold the given tokens exactly, every free token must be the oracle's argmax wherever its top-2 margin exceeds tol = 2e-4 (a margin
is a difference of two logits, each under the project's 1e-4 gate), and the free positions at or under tol -- which may differ -- must be at
most 1 % of the free tokens.  On the oracle's own trajectories, for exactly this model and batch: context 3: 1 of 3 072 free positions at or
under tol, 2 871 free tokens differ from the unconstrained run; the mixed pattern: 1 of 3 980 free (1 140 forced), 1 836 differ; unconstrained:
1 of 5 120.  Decoded frames within 1e-4 of vqvae_decode of the tokens; given frames bit-equal to the input."""
import pytest
import torch

from mage_amd import ops
from mage_amd.utils import synth
from oracle import mage_oracle as O
from tests import known_ref as KR
from tests import sampling_ref as R
from tests.helpers import build_mage, cpu_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
L, B = 6, 4


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


@pytest.fixture(scope="module")
def small():
    seed = 13
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), seed, DEV)
    sd, batch = cpu_sd(m), synth.synth_batch_mnist(B, L, seed=seed)
    with torch.no_grad():                                          # the encoder's tokens of every frame, computed once
        ft = torch.stack([O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, j]) for j in range(L)], 1)
    assert torch.equal(ft, m.first_stage_encode(batch["images"].to(DEV)).cpu())
    return m, sd, batch, ft


def _reset(m):
    m.set_precision("fp32").set_sampling(None).set_guidance(None).set_logprobs(False).set_context(1)
    m.use_graph, m.streams, m.ar_mode = False, 1, "full"


def _frames_ok(sd, batch, video, gen, k):
    Lm1, R_ = gen.shape[1], gen.shape[2]
    n = Lm1 - (k - 1)
    with torch.no_grad():
        want = O.vqvae_decode(sd, "first_stage_model.", gen[:, k - 1:].reshape(B * n, R_, R_)).view(B, n, *video.shape[2:])
    assert video.shape == batch["images"].shape
    assert (video[:, k:] - want).abs().max().item() <= 1e-4
    assert torch.equal(video[:, :k], batch["images"][:, :k])       # the given frames, verbatim


@pytest.mark.parametrize("mode", ["full", "incremental"])
def test_context_frames_match_the_oracle(small, mode):
    m, sd, batch, ft = small
    _reset(m)
    k = 3
    m.set_context(k)
    m.ar_mode = mode
    try:
        video = m.autoregressive_generate(dev_batch(batch)).cpu()
        gen, mask = m.last_tokens.cpu(), m.last_known_mask.cpu()
        ctx_video = m.autoregressive_generate(dev_batch({**batch, "context_tokens": ft[:, :k]})).cpu()
        assert torch.equal(ctx_video, video) and torch.equal(m.last_tokens.cpu(), gen)     # the tokens in place of the encode
    finally:
        _reset(m)
    kn = KR.merged_known(ft[:, :k], None, k, L - 1)
    assert torch.equal(mask, kn >= 0) and torch.equal(gen[:, :k - 1], ft[:, 1:k])
    logits = KR.teacher_forced_logits(sd, ft[:, 0], batch["text"], batch.get("speed"), gen)
    KR.check_against_oracle(gen, kn, logits, TOL, f"context 3, {mode}")
    _frames_ok(sd, batch, video, gen, k)


def _mixed(ft):
    return KR.mixed_known(ft[:, 0], ft)


@pytest.mark.parametrize("mode", ["full", "incremental"])
def test_mixed_known_tokens_match_the_oracle(small, mode):
    m, sd, batch, ft = small
    _reset(m)
    known = _mixed(ft)
    m.ar_mode = mode
    try:
        plain = m.autoregressive_generate(dev_batch(batch)).cpu()
        plain_tok = m.last_tokens.cpu()
        assert m.last_known_mask is None
        video = m.autoregressive_generate(dev_batch({**batch, "known_tokens": known})).cpu()
        gen, mask = m.last_tokens.cpu(), m.last_known_mask.cpu()
    finally:
        _reset(m)
    assert torch.equal(mask, known >= 0)
    assert torch.equal(gen[0], plain_tok[0]) and torch.equal(video[0], plain[0])           # the free clip: its unconstrained self
    free = known < 0
    steered = int((gen[free] != plain_tok[free]).sum())
    print(f"mixed, {mode}: {steered} of {int(free.sum())} free tokens differ from the unconstrained run")
    assert steered > 0                                                                     # the given tokens steer the rest
    logits = KR.teacher_forced_logits(sd, ft[:, 0], batch["text"], batch.get("speed"), gen)
    KR.check_against_oracle(gen, known, logits, TOL, f"mixed, {mode}")
    _frames_ok(sd, batch, video, gen, 1)


@pytest.mark.parametrize("mode", ["full", "incremental"])
def test_sampled_mixed_known_tokens_and_their_results(small, mode):
    m, sd, batch, ft = small
    _reset(m)
    T, k, p = 0.9, 20, 0.9
    seeds = torch.tensor([1, -2, 3 ** 30, 99], dtype=torch.int64)
    known = _mixed(ft)
    b = dev_batch({**batch, "known_tokens": known, "sample_seed": seeds})
    m.set_sampling(T, top_k=k, top_p=p).set_logprobs(True, policy=True, entropy=True)
    try:
        m.ar_mode = "full"                                          # the full loop keeps the logits every token was picked from
        video = m.autoregressive_generate(b).cpu()
        gen, dev_logits = m.last_tokens.clone(), m.last_logits.clone()
        if mode == "incremental":
            m.ar_mode = mode
            video = m.autoregressive_generate(b).cpu()
            assert torch.equal(m.last_tokens, gen) and m.last_logits is None
        res = {a: getattr(m, a).clone() for a in ("last_token_logprobs", "last_token_policy_logprobs", "last_token_kept", "last_token_entropy",
                                                  "last_token_policy_entropy", "last_clip_logprob", "last_clip_policy_logprob")}
    finally:
        _reset(m)
    Lm1, R_, K = L - 1, 16, 64
    hw = R_ * R_
    # the results: forced slots exactly 0 / 0 / 1, free slots what a plain launch on the same logits gives
    f = (known >= 0).to(DEV)
    n = B * Lm1 * hw
    lp = ops.token_logprob(dev_logits, gen, torch.empty(gen.shape, device=DEV), rows=n, K=K)
    st = dict(policy_logprob=torch.empty(gen.shape, device=DEV), policy_entropy=torch.empty(gen.shape, device=DEV),
              kept=torch.empty(gen.shape, device=DEV, dtype=torch.int32), entropy=torch.empty(gen.shape, device=DEV))
    ops.token_stats(dev_logits, gen, rows=n, K=K, temperature=T, top_k=k, top_p=p, **st)
    for attr, plain, forced_val in (("last_token_logprobs", lp, 0.0), ("last_token_policy_logprobs", st["policy_logprob"], 0.0),
                                    ("last_token_entropy", st["entropy"], 0.0), ("last_token_policy_entropy", st["policy_entropy"], 0.0),
                                    ("last_token_kept", st["kept"], 1)):
        got = res[attr]
        assert got.shape == gen.shape and bool((got[f] == forced_val).all()), attr
        if got.dtype == torch.float32:
            assert not bool(torch.signbit(got[f]).any()), attr
            assert torch.equal(got[~f].view(torch.int32), plain[~f].view(torch.int32)), attr
        else:
            assert torch.equal(got[~f], plain[~f]), attr
    assert torch.equal(res["last_clip_logprob"], ops.clip_scores(res["last_token_logprobs"], n_clips=B)[0].view(B))
    assert torch.equal(res["last_clip_policy_logprob"], ops.clip_scores(res["last_token_policy_logprobs"], n_clips=B)[0].view(B))
    # the tokens: forced slots given, free ones the restated sampler's draw at position i * hw + px
    gen = gen.cpu()
    assert torch.equal(gen[known >= 0], known[known >= 0])
    lg = KR.teacher_forced_logits(sd, ft[:, 0], batch["text"], batch.get("speed"), gen).numpy()
    tol = 1e-4 * float(R.inv_temperature(T))
    hard = soft = free = 0
    for c in range(B):
        for i in range(Lm1):
            for px in range(hw):
                y, x = px // R_, px % R_
                if known[c, i, y, x] >= 0:
                    continue
                free += 1
                want, near = R.sample_row(lg[c, i, y, x], T, k, p, int(seeds[c]), i * hw + px, tol)
                if int(gen[c, i, y, x]) != want:
                    soft, hard = soft + near, hard + (not near)
    print(f"{mode} T={T} top_k={k} top_p={p}: {free} free tokens, hard mismatches {hard}, soft {soft}")
    assert free == int((known < 0).sum()) and hard == 0 and soft <= max(5, free // 1000)
    _frames_ok(sd, batch, video, gen, 1)
