"""CPU: mage_apply_known_tokens' declaration and binding, the properties of its numpy restatement (tests/known_ref.py), and the host-side
checks of MAGE.set_context / batch['known_tokens'] / batch['context_tokens'] that run before any kernel."""
import os
import re

import numpy as np
import pytest
import torch

from mage_amd import _lib
from mage_amd.utils import synth
from tests import known_ref as KR
from tests.helpers import ROOT, build_mage


def _declaration():
    src = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+mage_apply_known_tokens\s*\(([^)]*)\)\s*;", src)
    assert m, "include/mage_hip_ext.h does not declare mage_apply_known_tokens"
    return [a.strip() for a in m.group(1).split(",")]


def test_the_header_declares_the_entry_point_and_the_binding_agrees():
    args = _declaration()
    res, argtypes = _lib.EXT_SIGNATURES["mage_apply_known_tokens"]
    assert len(args) == len(argtypes) == 16
    for a, t in zip(args, argtypes):                               # pointers as void*, int64_t / int32_t by width
        want = _lib.vp if "*" in a else _lib.i64 if a.startswith("int64_t") else _lib.i32
        assert t is want, (a, t)
    assert "mage_apply_known_tokens" not in _lib.SIGNATURES and len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    from mage_amd import ops
    assert callable(ops.apply_known_tokens)


def _case(rows=37, group=5, K=64, seed=0, share=0.4):
    g = np.random.default_rng(seed)
    n = rows + 3
    tokens = g.integers(0, K, n)
    known = np.where(g.random(n) < share, g.integers(0, K, n), -1 - g.integers(0, 3, n))
    res = dict(logprob=g.standard_normal(n).astype(np.float32), policy_logprob=g.standard_normal(n).astype(np.float32),
               entropy=g.random(n).astype(np.float32), policy_entropy=g.random(n).astype(np.float32), kept=g.integers(2, K, n).astype(np.int32))
    return tokens, known, res, dict(rows=rows, group=group, K=K)


def test_all_free_is_the_identity():
    tokens, known, res, kw = _case()
    known = np.where(known >= 0, -1, known)                        # -1, -2, -3: any negative value is free
    assert (known < -1).any()
    got, out, bad = KR.apply_known(tokens, known, **kw, **res)
    assert bad == 0 and np.array_equal(got, tokens)
    for n, b in res.items():
        assert np.array_equal(out[n].view(np.uint32), b.view(np.uint32)), n


def test_forced_slots_are_constant_and_free_slots_untouched():
    tokens, known, res, kw = _case()
    got, out, bad = KR.apply_known(tokens, known, **kw, **res)
    f = np.zeros(tokens.shape, bool)
    f[:kw["rows"]] = known[:kw["rows"]] >= 0
    assert bad == 0 and f.any() and not f.all()
    assert np.array_equal(got[f], known[f]) and np.array_equal(got[~f], tokens[~f])
    for n, _, val in KR.RESULTS:
        assert (out[n][f] == val).all() and np.array_equal(out[n][~f], res[n][~f]), n
    assert not np.signbit(out["logprob"][f]).any()                 # +0, not -0
    # the result does not depend on what was there before, or on which results are asked for
    t2, known2, res2, _ = _case(seed=1)
    got2, out2, _ = KR.apply_known(t2, known, **kw, logprob=res2["logprob"], kept=None)
    assert np.array_equal(got2[f], got[f]) and (out2["logprob"][f] == 0).all() and out2["kept"] is None
    # the three entries past the last row stay as they were even where `known` is set there
    known3 = known.copy()
    known3[kw["rows"]:] = 7
    got3, _, _ = KR.apply_known(tokens, known3, **kw)
    assert np.array_equal(got3[kw["rows"]:], tokens[kw["rows"]:])


def test_addressing_candidates_share_a_row_and_bad_values_are_clamped():
    # full-loop addressing: frame i of [clips x N, T, hw] tokens against [clips, T, hw] known
    clips, N, T, hw, K, i = 2, 3, 5, 4, 16, 2
    g = np.random.default_rng(3)
    tokens = g.integers(0, K, clips * N * T * hw)
    known = np.where(g.random(clips * T * hw) < 0.5, g.integers(0, K, clips * T * hw), -1)
    known[1 * T * hw + i * hw + 1] = K + 5                         # one value >= K
    got, _, bad = KR.apply_known(tokens, known, rows=clips * N * hw, group=hw, K=K, tok_group_stride=T * hw, tok_off=i * hw,
                                 known_group_stride=T * hw, known_off=i * hw, known_clip_div=N)
    assert bad == N                                                # once per candidate of that clip
    want = tokens.reshape(clips, N, T, hw).copy()
    kf = known.reshape(clips, T, hw)[:, i]
    for c in range(clips):
        for n in range(N):
            want[c, n, i] = np.where(kf[c] >= 0, np.minimum(kf[c], K - 1), want[c, n, i])
    assert np.array_equal(got.reshape(clips, N, T, hw), want)
    t, kix = KR.indices(7, 3, 10, 4, 20, 2, 2)
    assert list(t) == [4, 5, 6, 14, 15, 16, 24] and list(kix) == [2, 3, 4, 2, 3, 4, 22]


def test_set_context_and_the_batch_keys():
    L = 4
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), 0)
    batch = synth.synth_batch_mnist(3, L, seed=1)
    assert m.context_frames == 1 and m.last_known_mask is None and m._known_inputs(batch) is batch
    fp = m._graph_fingerprint()
    for bad in (0, L, -1, 1.0, 2.5, "2", True, None):
        with pytest.raises(ValueError, match="set_context"):
            m.set_context(bad)
    assert m.context_frames == 1
    assert m.set_context(L - 1) is m and m.context_frames == L - 1 and m._graph_fingerprint() != fp
    b = m._known_inputs(batch)
    assert "known_tokens" not in b and m.last_known_mask.shape == (3, L - 1, 16, 16) and m.last_known_mask.dtype == torch.bool
    assert bool(m.last_known_mask[:, :L - 2].all()) and not bool(m.last_known_mask[:, L - 2:].any())
    tokens = torch.zeros(3, L - 1, 16, 16, dtype=torch.int64)
    for name, call in (("score", lambda: m.score(batch)), ("policy_loss", lambda: m.policy_loss(batch, tokens, torch.ones(3))),
                       ("token_policy_logprobs", lambda: m.token_policy_logprobs(batch, tokens)),
                       ("clip_logprobs", lambda: m.clip_logprobs(batch, tokens)),
                       ("preference_loss", lambda: m.preference_loss(batch, tokens, torch.tensor([[0, 1]]), torch.zeros(3))),
                       ("rollout", lambda: m.rollout(batch, 2))):
        with pytest.raises(ValueError, match=f"{name}: given frames or tokens"):
            call()
    assert m.set_context(1).context_frames == 1 and m._graph_fingerprint() == fp and m.set_context().context_frames == 1
    known = torch.full((3, L - 1, 16, 16), -1, dtype=torch.int64)
    known[1, 2, 3, 4] = 5
    assert m._graph_fingerprint({**batch, "known_tokens": known}) != fp
    b = m._known_inputs({**batch, "known_tokens": known})
    assert torch.equal(b["known_tokens"], known) and int(m.last_known_mask.sum()) == 1 and bool(m.last_known_mask[1, 2, 3, 4])
    for name, call in (("score", lambda: m.score({**batch, "known_tokens": known})), ("rollout", lambda: m.rollout({**batch, "known_tokens": known}, 2))):
        with pytest.raises(ValueError, match=f"{name}: given frames or tokens"):
            call()
    for key, val in (("known_tokens", known[:2]), ("known_tokens", known[:, :2]), ("known_tokens", known.int()), ("known_tokens", known.float()),
                     ("context_tokens", torch.zeros(3, 2, 16, 16, dtype=torch.int64)), ("context_tokens", torch.zeros(3, 1, 16, 16, dtype=torch.int32))):
        with pytest.raises(ValueError, match=key):
            m._known_inputs({**batch, key: val})
    for kw in (dict(frames=L - 1), dict(frames=L, overlap=0), dict(frames=L, overlap=L), dict(frames=L, texts=[batch["text"]] * 2),
               dict(frames=2 * L, overlap=1.0)):
        with pytest.raises(ValueError, match="generate_long"):
            m.generate_long(batch, **kw)
    with pytest.raises(ValueError, match="generate_long: batch\\['known_tokens'\\]"):
        m.generate_long({**batch, "known_tokens": known}, frames=L)
    m.set_sampling(1.0, candidates=2)
    with pytest.raises(ValueError, match="generate_long: candidates"):
        m.generate_long(batch, frames=L)
    m.set_sampling(None)
    plus = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)
    with pytest.raises(ValueError, match="set_context: a use_cids=False"):
        plus.set_context(2)
    assert plus.set_context(1).context_frames == 1
    with pytest.raises(ValueError, match="use_cids=False"):
        plus._known_inputs({**batch, "known_tokens": known})
    with pytest.raises(ValueError, match="use_cids=False"):
        plus._known_inputs({**batch, "context_tokens": known[:, :1]})
    with pytest.raises(ValueError, match="generate_long: a use_cids=False"):
        plus.generate_long(batch, frames=4)
