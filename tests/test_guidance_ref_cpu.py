"""CPU: the exact restatement of mage_guide_logits' rule (tests/guidance_ref.py) against hand-worked cases, and
mage_amd.utils.glue.null_caption.  No GPU, no library."""
import math

import numpy as np
import pytest
import torch

from mage_amd.utils import synth
from mage_amd.utils.glue import null_caption
from tests import guidance_ref as G
from tests.helpers import build_mage

f32 = np.float32


def test_round_f32_ties_subnormals_overflow():
    F = G.Fraction
    assert G.round_f32(F(1) + F(1, 2 ** 24)) == f32(1.0)                                   # a tie goes to the even neighbour
    assert G.round_f32(F(1) + F(3, 2 ** 24)) == f32(1.0 + 2.0 ** -22)                      # ... whichever side that is
    assert G.round_f32(F(1) + F(1, 2 ** 24) + F(1, 2 ** 90)) == f32(1.0 + 2.0 ** -23)      # a hair above the tie
    assert G.round_f32(-F(1, 2 ** 149)) == f32(-2.0 ** -149)                               # the smallest subnormal
    assert G.round_f32(F(1, 2 ** 150)) == f32(0.0)                                         # half of it: tie to even, 0
    assert G.round_f32(F(3, 2 ** 150)) == f32(2.0 ** -148)
    big = F((2 ** 24 - 1) * 2 ** 104)
    assert G.round_f32(big) == f32(3.4028234663852886e38)
    assert G.round_f32(big + F(2 ** 102)) == f32(3.4028234663852886e38)                    # below the rounding threshold of fp32's maximum
    assert math.isinf(float(G.round_f32(big + F(2 ** 103))))                               # the tie at the top rounds away: overflow


def test_hand_worked_cases():
    # w == 0: scale 1 returns c's bits whatever u is, NaN-free or not
    for c, u in ((1.5, -7.0), (-0.0, 3.0), (3.0e38, -3.0e38), (1e-40, 5.0)):
        assert G.f32_bits(G.guide_one(c, u, 1.0)) == G.f32_bits(f32(c))
    # d == 0 with c = -0.0: the fma would give 7.5 * 0 + (-0) = +0; the select keeps the sign
    z = G.guide_one(-0.0, -0.0, 8.5)
    assert z == 0 and math.copysign(1.0, float(z)) < 0
    z = G.guide_one(-0.0, 0.0, 8.5)                                                         # -0 - (+0) = -0: still d == 0
    assert z == 0 and math.copysign(1.0, float(z)) < 0
    assert G.f32_bits(G.guide_one(0.0, -0.0, -3.0)) == G.f32_bits(f32(0.0))
    # u == c returns c's bits at any finite scale
    for s in (7.5, -0.5, 0.0, 1e30):
        assert G.f32_bits(G.guide_one(0.1, 0.1, s)) == G.f32_bits(f32(0.1))
    # ordinary values: 2 + 2 * (2 - 0.5) = 5, scale 0 returns u when c - u is exact: c + (-1)(c - u)
    assert G.guide_one(2.0, 0.5, 3.0) == f32(5.0)
    assert G.guide_one(2.0, 0.5, 0.0) == f32(0.5)
    # NaN propagates from either input and from the scale; inf - inf is NaN
    for c, u, s in ((math.nan, 1.0, 3.0), (1.0, math.nan, 3.0), (1.0, 2.0, math.nan), (math.inf, math.inf, 3.0), (math.nan, 1.0, 1.0)):
        z = G.guide_one(c, u, s)
        assert np.isnan(z) or (s == 1.0 and np.isnan(f32(c)))                               # (scale 1 returns c: NaN here too)
    assert G.guide_one(math.inf, 1.0, 3.0) == f32(math.inf)
    assert G.guide_one(1.0, math.inf, 3.0) == f32(-math.inf)


def test_double_rounding_case_differs_from_fp64():
    # w * d = 13325 * 80581 * 2^-54 = (2^30 + 1) 2^-54 = 2^-24 + 2^-54, c = 1: the exact sum lies a hair ABOVE the fp32 tie 1 + 2^-24, so the
    # fma gives 1 + 2^-23; fp64 drops the 2^-54 (a quarter of its last place), lands ON the tie, and the second rounding goes to even: 1.0
    w, d, c = f32(13325 * 2.0 ** -10), f32(80581 * 2.0 ** -44), f32(1.0)
    assert float(w) * float(d) == 2.0 ** -24 + 2.0 ** -54                                    # the product is exact in fp64
    twice = f32(np.float64(c) + np.float64(w) * np.float64(d))
    assert twice == f32(1.0)
    assert G.fma_f32(w, d, c) == f32(1.0 + 2.0 ** -23)
    # the mirror image: with u = 2^-24, (1 + 4u) - (u + 2^-54) lies a hair BELOW the tie 1 + 3u between the fp32 neighbours 1 + 2u and
    # 1 + 4u, so the fma gives 1 + 2u; fp64 rounds up onto the tie and then to even, 1 + 4u
    c2 = f32(1.0 + 2.0 ** -22)
    assert f32(np.float64(c2) - np.float64(w) * np.float64(d)) == c2
    assert G.fma_f32(w, -d, c2) == f32(1.0 + 2.0 ** -23)


def test_vector_form_equals_scalar_form():
    g = np.random.default_rng(5)
    rows, K = 24, 128
    c = (3.0 * g.standard_normal((rows, K))).astype(f32)
    u = (c + g.standard_normal((rows, K)).astype(f32) * f32(0.5)).astype(f32)
    u[:, ::9] = c[:, ::9]                                                                   # d == 0 columns
    c[3, 5] = u[3, 5] = f32(-0.0)
    c[4, 1], u[5, 2] = f32(np.nan), f32(np.nan)
    c[6, 3] = u[6, 3] = f32(np.inf)
    c[7, :4] = f32(1.0)
    u[7, :4] = f32(1.0) - f32(2.0 ** -24) * np.arange(1, 5, dtype=f32)                      # tiny differences beside a large scale
    s = np.resize(np.array([1.0, 0.0, 3.0, 7.5, -0.5, 1.0 + 2.0 ** -23, 1e6, 1.0 / 3.0], f32), rows)
    z = G.guide_rows(c, u, s)
    want = np.array([[G.guide_one(c[r, k], u[r, k], s[r]) for k in range(K)] for r in range(rows)], f32)
    assert np.array_equal(G.f32_bits(z), G.f32_bits(want))
    assert np.array_equal(G.f32_bits(z[s == 1.0]), G.f32_bits(c[s == 1.0]))


PAD, CLS, SEP = 0, 1, 2


def test_null_caption():
    text = torch.tensor([[CLS, 13, 14, 5, SEP, PAD, PAD, PAD],      # ragged
                         [CLS, 13, SEP, PAD, PAD, PAD, PAD, PAD],
                         [CLS, 9, 8, 7, 6, 5, 4, SEP],              # full width
                         [CLS, SEP, PAD, PAD, PAD, PAD, PAD, PAD],  # already the null caption
                         [CLS, PAD, PAD, PAD, PAD, PAD, PAD, PAD],  # one token: returned as is
                         [PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD],  # all padding: returned as is
                         [CLS, 13, 14, 5, 7, PAD, PAD, PAD]])       # no [SEP]: the last non-padding token, whatever it is
    want = torch.tensor([[CLS, SEP] + [PAD] * 6, [CLS, SEP] + [PAD] * 6, [CLS, SEP] + [PAD] * 6, [CLS, SEP] + [PAD] * 6,
                         [CLS] + [PAD] * 7, [PAD] * 8, [CLS, 7] + [PAD] * 6])
    got = null_caption(text, PAD)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(null_caption(got, PAD), got)                                         # idempotent
    # another padding id, and a width of 1 and 2
    t9 = torch.tensor([[4, 6, 7, 9, 9], [4, 9, 9, 9, 9]])
    assert torch.equal(null_caption(t9, 9), torch.tensor([[4, 7, 9, 9, 9], [4, 9, 9, 9, 9]]))
    assert torch.equal(null_caption(torch.tensor([[CLS], [PAD]]), PAD), torch.tensor([[CLS], [PAD]]))
    assert torch.equal(null_caption(torch.tensor([[CLS, SEP], [CLS, PAD]]), PAD), torch.tensor([[CLS, SEP], [CLS, PAD]]))


def test_the_switch_and_the_batch_keys():
    """set_guidance's validation and what a guided call adds to its batch: host-side, before any kernel runs."""
    m = build_mage(synth.mnist_model_config(frames_length=4, width=64, layers=3, vq_dim=32, K=64), 0)
    batch = synth.synth_batch_mnist(3, 4, seed=1, text_len=9, ragged_text=True)
    assert m.guidance is None and m.caption_dropout == 0.0 and m._guidance_inputs(batch) is batch
    assert "guidance_scale" not in m._guidance_inputs({**batch, "guidance_scale": torch.ones(3)})    # ignored while guidance is off
    fp = m._graph_fingerprint()
    for bad in (float("nan"), float("inf"), 3.5e38, "2", True):
        with pytest.raises(ValueError, match="set_guidance"):
            m.set_guidance(bad)
    assert m.set_guidance(2) is m and m.guidance == 2.0 and m._graph_fingerprint() != fp
    b = m._guidance_inputs(batch)
    assert b["guidance_scale"].dtype == torch.float32 and torch.equal(b["guidance_scale"], torch.full((3,), 2.0))
    assert torch.equal(b["negative_text"], null_caption(batch["text"], 0)) and b["negative_text"] is not batch["text"]
    assert m.last_guidance_scale is b["guidance_scale"]
    gs, neg = torch.tensor([1.0, -2.0, 7.5]), batch["text"].flip(0)
    b = m._guidance_inputs({**batch, "guidance_scale": gs, "negative_text": neg})
    assert torch.equal(b["guidance_scale"], gs) and torch.equal(b["negative_text"], neg)
    for key, val in (("guidance_scale", torch.ones(2)), ("guidance_scale", torch.ones(3, dtype=torch.float64)),
                     ("negative_text", batch["text"][:, :-1]), ("negative_text", batch["text"].to(torch.int32))):
        with pytest.raises(ValueError, match=key):
            m._guidance_inputs({**batch, key: val})
    tokens = torch.zeros(3, 3, 16, 16, dtype=torch.int64)
    for name, call in (("score", lambda: m.score(batch)), ("policy_loss", lambda: m.policy_loss(batch, tokens, torch.ones(3))),
                       ("token_policy_logprobs", lambda: m.token_policy_logprobs(batch, tokens)), ("rollout", lambda: m.rollout(batch, 2))):
        with pytest.raises(ValueError, match=f"{name}: classifier-free guidance"):
            call()
    assert m.set_guidance(None).guidance is None and m._graph_fingerprint() == fp
    plus = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)
    with pytest.raises(ValueError, match="set_guidance: a use_cids=False"):
        plus.set_guidance(2.0)
    # caption dropout: the replacement at the top of forward, host-side
    m.train()
    torch.manual_seed(9)
    want = torch.rand(3) < 0.5
    m.caption_dropout = 0.5
    torch.manual_seed(9)
    out = m._drop_captions(batch)
    assert torch.equal(m.last_caption_drop, want) and "caption_drop" not in out
    assert torch.equal(out["text"], torch.where(want[:, None], null_caption(batch["text"], 0), batch["text"]))
    m.eval()
    assert m._drop_captions(batch) is batch and m.last_caption_drop is None
    mask = torch.tensor([False, True, False])
    assert torch.equal(m._drop_captions({**batch, "caption_drop": mask})["text"][1], null_caption(batch["text"], 0)[1])
    m.caption_dropout = 0.0
