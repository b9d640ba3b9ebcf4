"""GPU: MAGE.generate_long -- windows chained through batch['context_tokens'] on the device.  Bitwise against the same chain made by hand
from autoregressive_generate calls (the small fp32 model of tests/test_gpu_context.py and BASELINE cfg2 in bf16), truncation, window 1 against
the CPU oracle (tests/known_ref.py's check) under the batch's caption and under a second one, and the shapes and totals of the results."""
import pytest
import torch

from mage_amd import ops
from mage_amd.utils import synth
from tests import known_ref as KR
from tests.helpers import build_mage, cpu_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
STRIDE = 1_000_003


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


@pytest.fixture(scope="module")
def small():
    L, B, seed = 6, 4, 13
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), seed, DEV)
    return m, cpu_sd(m), synth.synth_batch_mnist(B, L, seed=seed)


@pytest.fixture(scope="module")
def cfg2():
    m = build_mage(synth.mnist_model_config(frames_length=16), 0, DEV).set_precision("bf16")
    return m, None, synth.synth_batch_mnist(4, 16, seed=3)


def _reset(m, precision):
    m.set_precision(precision).set_sampling(None).set_guidance(None).set_logprobs(False).set_context(1)
    m.use_graph, m.streams, m.ar_mode = False, 1, "incremental"


def _by_hand(m, b, o, seeds=None, text1=None):
    """Two autoregressive_generate calls chained through context_tokens: (video [B, 2L - o, ...], tokens [B, 2L - o - 1, h, w])."""
    L = m.frames_length
    b0 = dict(b) if seeds is None else {**b, "sample_seed": seeds}
    v0 = m.autoregressive_generate(b0)
    t0 = m.last_tokens.clone()
    b1 = {**b, "images": v0[:, L - o:], "context_tokens": t0[:, L - 1 - o:].contiguous()}
    if seeds is not None:
        b1["sample_seed"] = seeds + STRIDE
    if text1 is not None:
        b1["text"] = text1
    m.set_context(o)
    try:
        v1 = m.autoregressive_generate(b1)
        t1 = m.last_tokens.clone()
    finally:
        m.set_context(1)
    return torch.cat([v0, v1[:, o:]], 1), torch.cat([t0, t1[:, o - 1:]], 1), (t0, t1)


@pytest.mark.parametrize("which,precision", [("small", "fp32"), ("cfg2", "bf16")])
@pytest.mark.parametrize("o", [1, 3])
def test_chaining_equals_two_calls_chained_by_hand(request, which, precision, o):
    m, _, batch = request.getfixturevalue(which)
    _reset(m, precision)
    L, B = m.frames_length, batch["images"].shape[0]
    b = dev_batch(batch)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV) * 31 + 2 ** 62              # (the window stride wraps around in int64 for none of these)
    try:
        for s in (None, seeds):
            m.set_sampling(None) if s is None else m.set_sampling(1.0, top_k=50, top_p=0.95)
            want_v, want_t, _ = _by_hand(m, b, o, s)
            got = m.generate_long(b if s is None else {**b, "sample_seed": s}, frames=2 * L - o, overlap=o)
            assert got.shape == want_v.shape == (B, 2 * L - o, *b["images"].shape[2:])
            assert torch.equal(got, want_v) and torch.equal(m.last_tokens, want_t)
            assert m.context_frames == 1 and m.last_logits is None
            if s is not None:
                assert torch.equal(m.last_sample_seeds, s)
    finally:
        _reset(m, precision)


def test_truncation_and_the_plain_call(small):
    m, _, batch = small
    _reset(m, "fp32")
    L = m.frames_length
    b = dev_batch(batch)
    try:
        plain = m.autoregressive_generate(b)
        pt = m.last_tokens.clone()
        got = m.generate_long(b, frames=L)
        assert torch.equal(got, plain) and torch.equal(m.last_tokens, pt)                  # frames = L: the plain call
        want_v, want_t, _ = _by_hand(m, b, 2)
        got = m.generate_long(b, frames=L + 2, overlap=2)                                  # window 1's surplus frames are dropped
        assert got.shape[1] == L + 2 and torch.equal(got, want_v[:, :L + 2]) and torch.equal(m.last_tokens, want_t[:, :L + 1])
        # window 0 honours set_context
        m.set_context(3)
        got = m.generate_long(b, frames=L + 1, overlap=1)
        assert m.context_frames == 3 and torch.equal(got[:, :3], b["images"][:, :3])
        assert m.last_known_mask.shape == (4, L, 16, 16) and bool(m.last_known_mask[:, :2].all()) and not bool(m.last_known_mask[:, 2:].any())
        m.set_context(1)
        for kw in (dict(frames=L - 1), dict(frames=L, overlap=0), dict(frames=L, overlap=L), dict(frames=2 * L, texts=[b["text"]])):
            with pytest.raises(ValueError, match="generate_long"):
                m.generate_long(b, **kw)
        with pytest.raises(ValueError, match="known_tokens"):
            m.generate_long({**b, "known_tokens": torch.full((4, L - 1, 16, 16), -1, dtype=torch.int64, device=DEV)}, frames=L)
        m.set_sampling(1.0, candidates=2)
        with pytest.raises(ValueError, match="candidates"):
            m.generate_long(b, frames=L)
    finally:
        _reset(m, "fp32")


def test_window_one_matches_the_oracle_under_each_caption(small):
    m, sd, batch = small
    _reset(m, "fp32")
    L, o = m.frames_length, 2
    b = dev_batch(batch)
    text2 = batch["text"].roll(1, 0)
    assert not torch.equal(text2, batch["text"])
    try:
        wins = []
        for texts, text1 in ((None, batch["text"]), ([b["text"], text2.to(DEV)], text2)):
            m.generate_long(b, frames=2 * L - o, overlap=o, texts=texts)
            tok = m.last_tokens.cpu()
            w0, w1new = tok[:, :L - 1], tok[:, L - 1:]                                       # window 0's slots; window 1's new frames
            ctx = w0[:, L - 1 - o:]                                                        # the hand-over: window 0's last o frames
            w1 = torch.cat([ctx[:, 1:], w1new], 1)                                          # window 1's slots 0 .. L-2
            kn = KR.merged_known(ctx, None, o, L - 1)
            logits = KR.teacher_forced_logits(sd, ctx[:, 0], text1, batch.get("speed"), w1)  # the anchor from the hand-over frame
            KR.check_against_oracle(w1, kn, logits, TOL, f"window 1, caption {'of the batch' if texts is None else 'two'}")
            wins.append(w1new)
        assert not torch.equal(wins[0], wins[1])                                            # the second caption steers window 1
    finally:
        _reset(m, "fp32")


def test_shapes_and_totals(small):
    m, _, batch = small
    _reset(m, "fp32")
    L, B, frames = m.frames_length, 4, 13                                                  # three windows at overlap 2, the last one cut
    seeds = torch.tensor([5, -6, 7 ** 20, 2 ** 63 - 3], dtype=torch.int64, device=DEV)      # the last one wraps around
    m.set_sampling(0.9, top_k=20, top_p=0.9).set_logprobs(True, policy=True, entropy=True)
    try:
        v = m.generate_long({**dev_batch(batch), "sample_seed": seeds}, frames=frames, overlap=2)
        assert v.shape == (B, frames, *batch["images"].shape[2:]) and bool(torch.isfinite(v).all())
        shape = (B, frames - 1, 16, 16)
        for a in ("last_tokens", "last_token_logprobs", "last_token_policy_logprobs", "last_token_kept", "last_token_entropy",
                  "last_token_policy_entropy"):
            assert getattr(m, a).shape == shape and getattr(m, a).is_contiguous(), a
        assert bool((m.last_token_kept >= 1).all()) and bool(torch.isfinite(m.last_token_policy_logprobs).all())
        assert bool((m.last_token_logprobs < 0).all())                                      # every reported frame was generated, none handed over
        assert torch.equal(m.last_clip_logprob, ops.clip_scores(m.last_token_logprobs, n_clips=B)[0].view(B))
        assert torch.equal(m.last_clip_policy_logprob, ops.clip_scores(m.last_token_policy_logprobs, n_clips=B)[0].view(B))
        assert m.last_video_noise is None and torch.equal(m.last_sample_seeds, seeds)
    finally:
        _reset(m, "fp32")
