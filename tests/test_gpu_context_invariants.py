"""GPU, bitwise: what given frames (MAGE.set_context) and given tokens (batch['known_tokens']) must leave exactly as it was, and what must
agree with what.  BASELINE cfg2 in bf16 with 8 clips (the fixture of tests/test_gpu_guidance.py), sampling 1.0 / 50 / 0.95 with given seeds."""
import pytest
import torch

from mage_amd.utils import synth
from tests.helpers import build_mage, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAST = ("last_token_logprobs", "last_clip_logprob", "last_token_policy_logprobs", "last_clip_policy_logprob", "last_token_kept",
        "last_token_entropy", "last_token_policy_entropy", "last_candidate_scores", "last_candidate_index", "last_candidate_policy_scores")


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


@pytest.fixture(scope="module")
def cfg2():
    m = build_mage(synth.mnist_model_config(frames_length=16), 0, DEV).set_precision("bf16")
    batch = dev_batch(synth.synth_batch_mnist(8, 16, seed=3))
    seeds = torch.arange(8, dtype=torch.int64, device=DEV) * 7919 - 12345
    return m, batch, seeds


def _reset(m):
    m.set_precision("bf16").set_guidance(None).set_sampling(None).set_logprobs(False).set_context(1)
    m.use_graph, m.streams, m.ar_mode, m.context_prefill = False, 1, "incremental", True


def _run(m, batch, seeds=None, **extra):
    """(video, tokens, logits or None, every last_* result) of one call."""
    b = {**batch, **extra}
    if seeds is not None:
        b["sample_seed"] = seeds
    v = m.autoregressive_generate(b)
    return v, m.last_tokens.clone(), m.last_logits, {a: getattr(m, a) for a in LAST}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, rows=slice(None)):
    if not (torch.equal(a[0][rows], b[0][rows]) and torch.equal(a[1][rows], b[1][rows])):
        return False
    if (a[2] is None) != (b[2] is None) or (a[2] is not None and not torch.equal(_bits(a[2][rows]), _bits(b[2][rows]))):
        return False
    for n in LAST:
        x, y = a[3][n], b[3][n]
        if (x is None) != (y is None) or (x is not None and not torch.equal(_bits(x[rows]), _bits(y[rows]))):
            return False
    return True


def _nolog(r):
    """A call's results without last_logits (the incremental loop keeps none)."""
    return r[0], r[1], None, r[3]


def _take(r, idx):
    return r[0][idx], r[1][idx], None if r[2] is None else r[2][idx], {n: None if x is None else x[idx] for n, x in r[3].items()}


def _known(m, batch, clips=(1, 4, 6)):
    """A mixed batch: `clips` are given a block of every slot, a whole slot, and scattered tokens; the other clips are free."""
    R_, Lm1, K = m.image_resolution, m.frames_length - 1, m.codebook_size
    g = torch.Generator().manual_seed(11)
    known = torch.full((8, Lm1, R_, R_), -1, dtype=torch.int64)
    known[clips[0], :, 2:9, 5:12] = torch.randint(0, K, (Lm1, 7, 7), generator=g)
    known[clips[1], 3] = torch.randint(0, K, (R_, R_), generator=g)
    sc = torch.rand(Lm1, R_, R_, generator=g) < 0.2
    known[clips[2]][sc] = torch.randint(0, K, (Lm1, R_, R_), generator=g)[sc]
    return known.to(DEV)


@pytest.mark.parametrize("mode", ["full", "incremental"])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_all_free_is_the_call_without_the_key_and_free_clips_are_themselves(cfg2, mode, sampled):
    m, batch, seeds = cfg2
    _reset(m)
    m.ar_mode = mode
    if sampled:
        m.set_sampling(1.0, top_k=50, top_p=0.95).set_logprobs(True, policy=True, entropy=True)
    else:
        m.set_logprobs(True, entropy=True)
    s = seeds if sampled else None
    try:
        base = _run(m, batch, s)
        assert m.last_known_mask is None
        free = torch.full((8, 15, 16, 16), -1, dtype=torch.int64, device=DEV)
        free[3] = -7                                               # any negative value
        got = _run(m, batch, s, known_tokens=free)
        assert _same(got, base) and m.last_known_mask.shape == free.shape and not bool(m.last_known_mask.any())
        known = _known(m, batch)
        mixed = _run(m, batch, s, known_tokens=known)
        f = known >= 0
        assert torch.equal(m.last_known_mask, f) and torch.equal(mixed[1][f], known[f])
        idx = torch.tensor([0, 2, 3, 5, 7], device=DEV)
        assert _same(_take(mixed, idx), _take(base, idx))          # the free clips of a mixed batch: their unconstrained selves
        for c in (1, 4, 6):
            assert not torch.equal(mixed[1][c], base[1][c])
        lp = mixed[3]["last_token_logprobs"]
        assert bool((lp[f] == 0).all()) and bool((mixed[3]["last_token_entropy"][f] == 0).all())
    finally:
        _reset(m)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_prefilled_incremental_equals_the_full_loop(cfg2, precision, monkeypatch):
    m, batch, seeds = cfg2
    _reset(m)
    four = {k_: v[:2] for k_, v in batch.items()} if precision == "fp32" else batch      # (fp32: a fraction of the GEMM rate)
    s = seeds[:four["images"].shape[0]]
    m.set_precision(precision).set_sampling(1.0, top_k=50, top_p=0.95).set_logprobs(True, policy=True, entropy=True).set_context(8)
    try:
        m.ar_mode = "full"
        full = _run(m, four, s)
        m.ar_mode = "incremental"
        calls = count_lib_calls(monkeypatch)
        inc = _run(m, four, s)
        monkeypatch.undo()
        assert _same(_nolog(inc), _nolog(full))
        assert torch.equal(inc[0][:, :8], four["images"][:, :8])
        # 8 picks (frames 8 .. 15), none before frame 8; the first 7 slots come from the apply alone; and up to the first pick the call
        # launches as many attentions as the call without context does: the prologue's, and ONE decoder pass
        attn = lambda c: c[:c.index("mage_sample_tokens")].count("mage_attention")        # noqa: E731
        assert calls.count("mage_sample_tokens") == 8 and calls.count("mage_apply_known_tokens") == 7 + 8
        m.set_context(1)
        plain_calls = count_lib_calls(monkeypatch)
        _run(m, four, s)
        monkeypatch.undo()
        assert plain_calls.count("mage_sample_tokens") == 15 and plain_calls.count("mage_apply_known_tokens") == 0
        assert attn(calls) == attn(plain_calls) > 0
        # ... and it equals the one-position-at-a-time form, which runs eight passes
        m.set_context(8)
        m.context_prefill = False
        slow_calls = count_lib_calls(monkeypatch)
        slow = _run(m, four, s)
        monkeypatch.undo()
        per_pass = (plain_calls.count("mage_attention") - attn(plain_calls)) // 14
        assert _same(slow, inc) and attn(slow_calls) == attn(calls) + 7 * per_pass and per_pass > 0
        m.context_prefill = True
        # context_tokens set to the encoder's tokens: the pixel path
        ctx = m.first_stage_encode(four["images"][:, :8])
        assert _same(_run(m, four, s, context_tokens=ctx), inc)
    finally:
        _reset(m)


def test_candidates_guidance_streams_and_graph_replay(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    known = _known(m, batch)
    m.set_sampling(1.0, top_k=50, top_p=0.95).set_logprobs(True, policy=True, entropy=True).set_context(3)
    try:
        eager = _run(m, batch, seeds, known_tokens=known)
        f = m.last_known_mask.clone()
        want = known.clone()
        want[:, :2] = m.first_stage_encode(batch["images"][:, 1:3])                   # the given frames win over known_tokens in their slots
        assert bool(f[:, :2].all()) and torch.equal(f, want >= 0) and torch.equal(eager[1][f], want[f])
        m.streams = 2
        assert _same(_run(m, batch, seeds, known_tokens=known), eager)                # two streams == one
        m.streams = 1
        m.ar_mode = "full"
        assert _same(_nolog(_run(m, batch, seeds, known_tokens=known)), _nolog(eager))       # the full loop == the incremental one
        m.ar_mode = "incremental"
        # candidates = 4: candidate c is the plain call under seed + c, every candidate carries the forced slots
        plain = [_run(m, batch, seeds + c, known_tokens=known) for c in range(4)]
        m.set_sampling(1.0, top_k=50, top_p=0.95, candidates=4)
        best = _run(m, batch, seeds, known_tokens=known)
        idx = m.last_candidate_index
        for c in range(4):
            assert torch.equal(_bits(m.last_candidate_scores[:, c].contiguous()), _bits(plain[c][3]["last_clip_logprob"]))
        for b in range(8):
            w = plain[int(idx[b])]
            assert torch.equal(best[1][b], w[1][b]) and torch.equal(best[0][b], w[0][b])
        assert torch.equal(best[1][f], eager[1][f])
        m.set_sampling(1.0, top_k=50, top_p=0.95)
        # guidance on: scale 1 is the unguided call bit for bit, forced slots included; scale 3 keeps them and agrees across the AR modes
        m.set_guidance(1.0)
        g1 = _run(m, batch, seeds, known_tokens=known)
        assert _same(g1, eager)
        m.set_guidance(3.0)
        g3 = _run(m, batch, seeds, known_tokens=known)
        assert torch.equal(g3[1][f], eager[1][f]) and not torch.equal(g3[1], eager[1])
        m.ar_mode = "full"
        g3f = _run(m, batch, seeds, known_tokens=known)
        assert _same(_nolog(g3f), _nolog(g3))
        m.ar_mode = "incremental"
        m.set_guidance(None)
        # graph replay on the third call, at B = 1
        one = {k_: v[4:5] for k_, v in batch.items()}
        e1 = _run(m, one, seeds[4:5], known_tokens=known[4:5])
        m.use_graph = True
        for rep in range(3):
            assert _same(_run(m, one, seeds[4:5], known_tokens=known[4:5]), e1), (rep, m.last_call_mode)
        assert m.last_call_mode == "graph"
        other = _run(m, one, seeds[4:5], known_tokens=known[1:2])                     # new given tokens: the same graph
        k1 = known[1:2, 2:]
        assert m.last_call_mode == "graph" and torch.equal(other[1][:, 2:][k1 >= 0], k1[k1 >= 0])
        m.use_graph = False
        assert _same(_run(m, one, seeds[4:5], known_tokens=known[1:2]), other)
    finally:
        _reset(m)


def test_refused_entry_points(cfg2):
    m, batch, seeds = cfg2
    _reset(m)
    two = {k_: v[:2] for k_, v in batch.items()}
    R_, Lm1 = m.image_resolution, m.frames_length - 1
    tokens = torch.zeros(2, Lm1, R_, R_, dtype=torch.int64, device=DEV)
    known = torch.full((2, Lm1, R_, R_), -1, dtype=torch.int64, device=DEV)
    calls = lambda b: (("score", lambda: m.score(b)), ("policy_loss", lambda: m.policy_loss(b, tokens, torch.ones(2, device=DEV))),      # noqa: E731
                       ("token_policy_logprobs", lambda: m.token_policy_logprobs(b, tokens)), ("clip_logprobs", lambda: m.clip_logprobs(b, tokens)),
                       ("preference_loss", lambda: m.preference_loss(b, tokens, torch.tensor([[0, 1]], device=DEV), torch.zeros(2, device=DEV))),
                       ("rollout", lambda: m.rollout(b, 2)))
    try:
        want = _run(m, two)
        for name, call in calls({**two, "known_tokens": known}):
            with pytest.raises(ValueError, match=f"{name}: given frames or tokens"):
                call()
        m.set_context(4)
        for name, call in calls(two):
            with pytest.raises(ValueError, match=f"{name}: given frames or tokens"):
                call()
        for key, val in (("known_tokens", known[:1]), ("known_tokens", known.int()), ("context_tokens", tokens[:, :3]), ("context_tokens", tokens[:, :4].int())):
            with pytest.raises(ValueError, match=key):
                m.autoregressive_generate({**two, key: val})
        m.set_context(1)
        assert _same(_run(m, two), want) and m.score(two).shape == (2,)              # usable again, and the refused calls work
    finally:
        _reset(m)
