"""GPU: token log-probabilities and best-of-N (mage_token_logprob, mage_clip_scores, MAGE.set_logprobs / score / set_sampling(candidates=))
against the fp64 restatement (tests/logprob_ref.py) and the CPU oracle.

Kernel tolerance, per row: 1e-5 + 2^-23 |expected|.  z_t and the maximum are exact; the sum of K <= 4096 terms (accurate expf / logf, a few
ulp each; at most 64 sequential adds per lane + 6 butterfly stages) has a relative error of ~16 * 2^-24 = 1e-6, which log turns into the
same ABSOLUTE error; the last subtraction rounds once (2^-24 |lp|).  The kernel test prints the maximum it meets per K (DESIGN finding 95).
End to end: per token 2e-4 against the oracle (twice the 1e-4 logits gate: z_t and the logsumexp each move by at most the logit error), per
clip 2e-4 * (L - 1) * hw."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from mage_amd.utils import synth
from oracle import mage_oracle as O
from tests import logprob_ref as R
from tests.helpers import build_mage, cpu_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(frames_length=4, width=64, layers=1, vq_dim=32, K=16)
FOLD = dict(frames_length=4, width=256, layers=3, vq_dim=32, K=16)       # model_channels % 256 == 0: bf16 runs with the LayerNorm fold
SAMPLED = dict(temperature=0.9, top_k=8, top_p=0.9)


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _logits(rows, K, seed):
    """tests/test_gpu_sampling.py's recipe (ties on a 1/4 grid, a repeated boundary value) + the rows that stress a logsumexp."""
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((rows, K))).astype(np.float32)
    for r in range(0, rows, 7):
        z[r] = np.round(z[r] * 4) / 4
    for r in range(3, rows, 11):
        o = np.argsort(-z[r], kind="stable")
        if K > 22:
            z[r, o[20:23]] = z[r, o[19]]
    t = g.integers(0, K, rows)
    z[1] = z[1] / np.abs(z[1]).max() * 80.0                        # +-80: exp(80) = 5.5e34, no headroom left for a sum without the max subtraction
    z[12] = z[12] / np.abs(z[12]).max() * 100.0                    # +-100: exp(100) is past fp32 altogether
    z[2, g.integers(0, K, max(K // 3, 1))] = -np.inf               # -inf entries contribute nothing
    t[2] = int(np.argmax(z[2]))
    z[5, t[5]] = -np.inf                                           # the token's own logit is -inf
    z[5, (t[5] + 1) % K] = 1.0
    z[8, (t[8] + 1) % K] = np.nan                                  # one NaN
    z[9, :] = -np.inf                                              # no finite logit
    z[10, :] = 0.5                                                 # uniform: -log K
    return z, t.astype(np.int64)


def _assert_close(got, want, what):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN rows differ"
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinite rows differ"
    fin = ~nan & ~inf
    err = np.abs(got[fin] - want[fin])
    bound = 1e-5 + 2.0 ** -23 * np.abs(want[fin])
    print(f"{what}: {fin.sum()} finite rows, max |d| {err.max():.3e}, max |d| / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"{what}: max |d| {err.max():.3e}"


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
def test_kernel_matches_restatement(K):
    rows = 300                                                     # 75 workgroups of 4 waves; 301 below leaves a partial one
    z, t = _logits(rows + 1, K, seed=K)
    zd, td = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
    got = torch.full((rows + 1,), 7.0, device=DEV)
    ops.token_logprob(zd, td, got, rows=rows, K=K)
    ops.check_device_errors(DEV)
    assert got[rows].item() == 7.0                                 # the row past `rows` is not touched
    want = R.token_logprob(z[:rows], t[:rows])
    assert np.isnan(want[8]) and np.isnan(want[9]) and want[5] == -np.inf and abs(want[10] + np.log(K)) < 1e-12
    _assert_close(got[:rows].cpu().numpy(), want, f"K={K}")
    # a row's bits depend on the row alone: the same rows as the tail of a shorter, shifted launch (301 - 37 rows)
    got2 = torch.empty(rows + 1 - 37, device=DEV)
    ops.token_logprob(zd[37:], td[37:], got2, rows=rows + 1 - 37, K=K)
    assert torch.equal(got2[:rows - 37].view(torch.int32), got[37:rows].view(torch.int32))


def test_regrouped_addressing_writes_only_its_slots():
    K = 512
    z, _ = _logits(4 * 5 * 2, K, seed=52)
    z = z.reshape(4, 5, 2, K)
    tok = torch.from_numpy(np.random.default_rng(3).integers(0, K, (4, 5, 2)))
    out = torch.full((4, 5, 2), -77.0, device=DEV)
    # frame 2 of [B=4, T=5, hw=2, K] logits, tokens in slot 3 of a [4, 5, 2] buffer: the result lands in slot 3 of `out`
    ops.token_logprob(torch.from_numpy(z).to(DEV), tok.to(DEV), out, rows=8, K=K, group=2, in_group_stride=10, in_off=4, tok_group_stride=10,
                      tok_off=6)
    ops.check_device_errors(DEV)
    out = out.cpu()
    sent = torch.ones(4, 5, 2, dtype=torch.bool)
    sent[:, 3] = False
    assert (out[sent] == -77.0).all()
    want = R.token_logprob(z[:, 2].reshape(8, K), tok[:, 3].reshape(8).numpy())
    _assert_close(out[:, 3].reshape(8).numpy(), want, "regrouped")


def test_clip_scores_sums_ties_and_nan():
    g = np.random.default_rng(11)
    lp = (-3.0 * g.random((3, 4, 48))).astype(np.float32)
    lp[0, 2] = lp[0, 0]                                            # clip 0: candidates 0 and 2 tie ...
    lp[0, 1] -= 1.0
    lp[0, 3] -= 1.0                                                # ... above the other two
    lp[1, 0, 7] = np.nan                                           # clip 1: candidate 0 is NaN, 3 repeats the best of the rest
    lp[1, 3] = lp[1, 1]
    lp[1, 2] -= 1.0
    lp[2, :, 5] = np.nan                                           # clip 2: every candidate NaN
    exact, s32, best = R.clip_scores(lp.reshape(12, 48), 3, 4)
    assert best.tolist() == [0, 1, 0]
    d = torch.from_numpy(lp).to(DEV).view(12, 48)
    scores, pick = ops.clip_scores(d, n_clips=3, n_cand=4)
    scores, pick = scores.cpu().numpy(), pick.cpu().numpy()
    assert np.array_equal(np.isnan(scores), np.isnan(s32))
    fin = ~np.isnan(s32)
    ulp = np.spacing(np.abs(s32[fin]).astype(np.float32)).astype(np.float64)
    assert (np.abs(scores[fin].astype(np.float64) - exact[fin]) <= ulp).all()
    assert pick.dtype == np.int64 and pick.tolist() == best.tolist()
    one, none = ops.clip_scores(d[4:8], n_clips=1, n_cand=4)       # clip 1 alone: the same bits
    assert np.array_equal(one.cpu().numpy().view(np.int32), scores[1:2].view(np.int32))
    flat, none = ops.clip_scores(d, n_clips=12, n_cand=1)          # n_cand = 1: scores only
    assert none is None and np.array_equal(flat.cpu().numpy().reshape(3, 4).view(np.int32), scores.view(np.int32))


def test_token_out_of_range_surfaces_in_check_device_errors():
    """What MAGE.score would meet with a tampered token buffer: the id is reported, the read stays inside the row."""
    K = 16
    z = torch.zeros(8, K, device=DEV)
    for bad in (K, -1):
        tok = torch.arange(8, device=DEV, dtype=torch.int64)
        tok[3] = bad
        out = torch.empty(8, device=DEV)
        ops.token_logprob(z, tok, out, rows=8, K=K)
        with pytest.raises(ValueError, match="mage_token_logprob: token out of range"):
            ops.check_device_errors(DEV)
        assert torch.allclose(out, torch.full((8,), -float(np.log(K)), device=DEV))
    ops.check_device_errors(DEV)                                   # the word is cleared


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(**SMALL), 5, DEV)
    return m, synth.synth_batch_mnist(2, SMALL["frames_length"], seed=5)


@pytest.fixture(scope="module")
def fold():
    m = build_mage(synth.mnist_model_config(**FOLD), 6, DEV)
    return m, synth.synth_batch_mnist(2, FOLD["frames_length"], seed=6)


@pytest.fixture(scope="module")
def oracle_logprobs(small):
    """fp64 log_softmax + gather of the CPU oracle's teacher-forced logits on the batch's own tokens: [B, L-1, h, w], computed once."""
    m, batch = small
    sd, L = cpu_sd(m), SMALL["frames_length"]
    with torch.no_grad():
        tok = O.vqvae_encode(sd, "first_stage_model.", batch["images"].reshape(-1, *batch["images"].shape[2:]))
        tok = tok.view(2, L, *tok.shape[1:])                                                        # [B, L, h, w]
        ma = O.motion_anchor(sd, tok[:, 0], batch["text"], batch.get("speed"))
        lg = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, tok[:, :L - 1]))   # [B, L-1, h, w, K]
    lp = torch.log_softmax(lg.double(), -1).gather(-1, tok[:, 1:, :, :, None]).squeeze(-1)
    return tok, lp


def _reset(m):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32")
    m.use_graph, m.streams, m.ar_mode = None, 1, "full"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_score_matches_oracle(small, oracle_logprobs, precision):
    m, batch = small
    tok, want = oracle_logprobs
    _reset(m)
    m.set_precision(precision)
    got = m.score(dev_batch(batch)).cpu()
    lp = m.last_token_logprobs.cpu()
    _reset(m)
    assert torch.equal(m.first_stage_encode(batch["images"].to(DEV)).cpu().view(tok.shape), tok)
    assert got.shape == (2,) and got.dtype == torch.float32 and lp.shape == want.shape and lp.dtype == torch.float32
    d_tok = (lp.double() - want).abs().max().item()
    d_clip = (got.double() - want.flatten(1).sum(1)).abs().max().item()
    n = want[0].numel()
    print(f"score {precision}: per token max |d| {d_tok:.3e} (bound 2e-4), per clip {d_clip:.3e} (bound {2e-4 * n:.3e})")
    assert d_tok <= 2e-4 and d_clip <= 2e-4 * n


def test_greedy_full_loop_logprobs_match_its_logits(small):
    m, batch = small
    _reset(m)
    m.set_logprobs(True)
    m.use_graph = False
    m.autoregressive_generate(dev_batch(batch))
    lg, tk, lp, cl = m.last_logits.cpu().numpy(), m.last_tokens.cpu().numpy(), m.last_token_logprobs.cpu(), m.last_clip_logprob.cpu()
    _reset(m)
    K = lg.shape[-1]
    assert lp.shape == tk.shape and cl.shape == (2,) and m.last_candidate_scores is None and m.last_candidate_index is None
    want = R.token_logprob(lg.reshape(-1, K), tk.reshape(-1))
    _assert_close(lp.numpy(), want, "greedy full loop")
    _, s32, _ = R.clip_scores(lp.numpy().reshape(2, -1), 2, 1)
    assert np.abs(cl.numpy() - s32[:, 0]).max() <= np.spacing(np.abs(s32).max())
    assert (lp <= 0).all()                                          # the argmax token of a 16-way softmax ...
    assert (lp >= -float(np.log(K)) - 1e-5).all()                   # ... holds at least 1 / K of the mass


def _gen(m, batch, seeds=None):
    b = dev_batch(batch if seeds is None else {**batch, "sample_seed": seeds})
    v = m.autoregressive_generate(b)
    return v.cpu(), m.last_tokens.cpu(), m.last_token_logprobs.cpu(), m.last_clip_logprob.cpu()


@pytest.mark.parametrize("cfg,precision", [("small", "f16x3"), ("fold", "bf16")])
@pytest.mark.parametrize("sampled", [False, True])
def test_ar_modes_agree(request, cfg, precision, sampled):
    m, batch = request.getfixturevalue(cfg)
    _reset(m)
    m.set_precision(precision).set_logprobs(True)
    m.use_graph = False
    if precision == "bf16":
        assert m.generate_model._fold(torch.bfloat16, 2, m.image_resolution ** 2)
    seeds = None
    if sampled:
        m.set_sampling(**SAMPLED)
        seeds = torch.tensor([41, -9], dtype=torch.int64)
    m.ar_mode = "full"
    v_f, t_f, lp_f, c_f = _gen(m, batch, seeds)
    m.ar_mode = "incremental"
    v_i, t_i, lp_i, c_i = _gen(m, batch, seeds)
    m.streams = 2                                                   # (B = 2 < 2 * streams: one group; the results keep their shape)
    _, t_s, lp_s, c_s = _gen(m, batch, seeds)
    _reset(m)
    assert torch.equal(t_i, t_f) and torch.equal(v_i, v_f)
    assert torch.equal(lp_i, lp_f) and torch.equal(c_i, c_f), (lp_i - lp_f).abs().max().item()
    assert torch.equal(t_s, t_i) and torch.equal(lp_s, lp_i) and torch.equal(c_s, c_i)
    assert torch.isfinite(lp_f).all() and (lp_f <= 0).all()


def test_streams_concatenate_the_groups(small):
    m, _ = small
    batch = synth.synth_batch_mnist(4, SMALL["frames_length"], seed=8)
    seeds = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    _reset(m)
    m.set_sampling(candidates=2, **SAMPLED)
    m.use_graph, m.ar_mode = False, "incremental"
    v1, t1, lp1, c1 = _gen(m, batch, seeds)
    s1, i1 = m.last_candidate_scores.cpu(), m.last_candidate_index.cpu()
    m.streams = 2                                                   # two groups of two clips
    v2, t2, lp2, c2 = _gen(m, batch, seeds)
    s2, i2 = m.last_candidate_scores.cpu(), m.last_candidate_index.cpu()
    _reset(m)
    assert s1.shape == (4, 2) and i1.shape == (4,) and lp1.shape == t1.shape and c1.shape == (4,)
    for a, b in ((v1, v2), (t1, t2), (lp1, lp2), (c1, c2), (s1, s2), (i1, i2)):
        assert torch.equal(a, b)


@pytest.mark.timeout(120)
def test_graph_replay_equals_eager(small):
    m, batch = small
    one = {k: v[:1] for k, v in batch.items()}
    seeds = torch.tensor([77], dtype=torch.int64)
    _reset(m)
    m.set_logprobs(True).set_sampling(**SAMPLED)
    m.ar_mode, m.use_graph = "incremental", False
    v_e, t_e, lp_e, c_e = _gen(m, one, seeds)
    m.use_graph = True
    modes = []
    for rep in range(3):                                            # warm-up (eager), capture + replay, replay
        v_g, t_g, lp_g, c_g = _gen(m, one, seeds)
        modes.append(m.last_call_mode)
        assert torch.equal(t_g, t_e) and torch.equal(v_g, v_e) and torch.equal(lp_g, lp_e) and torch.equal(c_g, c_e), (rep, modes)
    keep = m.last_token_logprobs
    held = keep.clone()
    _, t_o, lp_o, _ = _gen(m, one, seeds + 1)                        # other seeds through the same graph: earlier results are not overwritten
    last = m.last_call_mode
    assert torch.equal(keep, held)
    _reset(m)
    assert modes[-1] == "graph" and last == "graph"
    assert not torch.equal(t_o, t_e) and not torch.equal(lp_o, lp_e)


def test_candidates_keep_the_most_likely(small):
    m, batch = small
    N, B = 3, 2
    seeds = torch.tensor([1234, -2 ** 63 + 1], dtype=torch.int64)   # (clip 1: seed + c stays in range; the wrap-around itself is below)
    _reset(m)
    m.use_graph, m.ar_mode = False, "incremental"
    m.set_sampling(**SAMPLED)
    v_today = m.autoregressive_generate(dev_batch({**batch, "sample_seed": seeds})).cpu()       # feature untouched: today's sampled output
    t_today = m.last_tokens.cpu()
    assert m.last_token_logprobs is None and m.last_clip_logprob is None
    m.set_logprobs(True)
    plain = [_gen(m, batch, seeds + c) for c in range(N)]          # N plain calls, candidates = 1
    assert torch.equal(plain[0][0], v_today) and torch.equal(plain[0][1], t_today)     # ... which set_logprobs does not change
    assert m.last_candidate_scores is None
    m.set_logprobs(False)                                           # candidates compute log-probabilities whatever set_logprobs says
    m.set_sampling(candidates=N, **SAMPLED)
    v, t, lp, cl = _gen(m, batch, seeds)
    scores, idx = m.last_candidate_scores.cpu(), m.last_candidate_index.cpu()
    m.set_sampling(candidates=1, **SAMPLED)
    v_1 = m.autoregressive_generate(dev_batch({**batch, "sample_seed": seeds})).cpu()
    assert torch.equal(v_1, v_today) and torch.equal(m.last_tokens.cpu(), t_today) and m.last_token_logprobs is None
    m.ar_mode = "full"
    m.set_sampling(candidates=N, **SAMPLED)
    v_f, t_f, lp_f, cl_f = _gen(m, batch, seeds)                     # the full loop picks the same winners
    scores_f = m.last_candidate_scores.cpu()
    _reset(m)
    want_scores = torch.stack([p[3] for p in plain], 1)             # [B, N]
    assert scores.shape == (B, N) and scores.dtype == torch.float32 and idx.shape == (B,) and idx.dtype == torch.int64
    assert torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
    want_idx = torch.tensor([R.pick(want_scores[b].numpy()) for b in range(B)])
    assert torch.equal(idx, want_idx)
    print(f"candidate scores {scores.tolist()}, kept {idx.tolist()}")
    for b in range(B):
        w = plain[int(idx[b])]
        assert torch.equal(v[b], w[0][b]) and torch.equal(t[b], w[1][b]) and torch.equal(lp[b], w[2][b])
        assert cl[b] == scores[b, idx[b]] and cl[b] >= scores[b, 0]
    assert len({tuple(p[1][0].flatten().tolist()) for p in plain}) >= 2            # the candidates do differ
    assert torch.equal(t_f, t) and torch.equal(v_f, v) and torch.equal(lp_f, lp) and torch.equal(cl_f, cl) and torch.equal(scores_f, scores)


def test_candidate_seeds_wrap_around(small):
    m, batch = small
    one = {k: v[:1] for k, v in batch.items()}
    _reset(m)
    m.use_graph, m.ar_mode = False, "incremental"
    m.set_sampling(**SAMPLED).set_logprobs(True)
    _, t_w, _, c_w = _gen(m, one, torch.tensor([-2 ** 63], dtype=torch.int64))                # 2^63 - 1 + 1 in int64
    m.set_sampling(candidates=2, **SAMPLED)
    _gen(m, one, torch.tensor([2 ** 63 - 1], dtype=torch.int64))
    s = m.last_candidate_scores.cpu()
    _reset(m)
    assert s[0, 1] == c_w[0]


def test_refusals(small):
    m, _ = small
    _reset(m)
    with pytest.raises(ValueError, match="candidates"):
        m.set_sampling(None, candidates=2)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="candidates"):
            m.set_sampling(1.0, candidates=bad)
    assert m.sampling is None and m.candidates == 1
    p = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0, DEV)
    with pytest.raises(ValueError, match="use_cids=False"):
        p.set_logprobs(True)
    with pytest.raises(ValueError, match="use_cids=False"):
        p.score({})


def test_off_is_off(small, monkeypatch):
    """The feature untouched: no results, and not one library call more than a call makes with the two new entry points removed."""
    m, batch = small
    lib = _lib.lib(0)
    calls = []

    def counted(name, fn):
        def f(*a):
            calls.append(name)
            return fn(*a)
        return f
    for name in _lib.SIGNATURES:
        if name not in ("mage_last_error", "mage_abi_version"):
            monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    _reset(m)
    m.use_graph = False
    b = dev_batch(batch)
    Lm1 = SMALL["frames_length"] - 1
    for mode in ("incremental", "full"):
        m.ar_mode = mode
        m.autoregressive_generate(b)                                # derived caches built
        del calls[:]
        m.autoregressive_generate(b)
        off = list(calls)
        assert m.last_token_logprobs is None and m.last_clip_logprob is None and m.last_candidate_scores is None
        assert "mage_token_logprob" not in off and "mage_clip_scores" not in off
        m.set_logprobs(True)
        del calls[:]
        m.autoregressive_generate(b)
        on = list(calls)
        m.set_logprobs(False)
        del calls[:]
        m.autoregressive_generate(b)
        assert calls == off and m.last_token_logprobs is None       # switched off again: the same sequence of launches
        extra = [c for c in on if c in ("mage_token_logprob", "mage_clip_scores")]
        assert extra == ["mage_token_logprob"] * (Lm1 if mode == "incremental" else 1) + ["mage_clip_scores"]
        assert [c for c in on if c not in ("mage_token_logprob", "mage_clip_scores")] == off
    _reset(m)
