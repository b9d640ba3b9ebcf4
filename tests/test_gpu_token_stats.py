"""GPU: per-token policy statistics (mage_token_stats, MAGE.set_logprobs(policy=, entropy=), score) against the fp64 restatement
(tests/token_stats_ref.py), against mage_token_logprob bit for bit, and the bitwise invariants of the model-side results.

Every row is compared.  `kept` is an exact count: it must be the size of the set one of the row's admissible top-p thresholds gives
(token_stats_ref.admissible_sets: one set unless the boundary mass is within 1e-5 W of top_p W), and the floating-point outputs must
match THAT set.  A token the sampler drew has a finite policy_logprob on every row, with no tolerance.

Tolerances, per row.  policy_logprob: the project's 1e-5 + 2^-23 |expected| (tests/test_gpu_logprobs.py: the same arithmetic as
mage_token_logprob).  The entropies H = log Z - T / Z, T = sum_j w_j d_j (d_j = s_j - s_max <= 0, every term of one sign), add one
fixed-order sum and one division.  log Z: no z_t - (s_max + log Z) cancellation stands behind it here, so it does not get the logprob bound's
1e-5 but its own worst case -- Z is a sum of positive terms, NV = max(4, K / 64) sequential adds per lane + 6 butterfly stages + expf's 3 ulp
(6 roundings): at most (NV + 12) * 2^-24 relative, which log turns into the same ABSOLUTE error (9.5e-7 at K <= 256, 1.2e-6 at K = 512,
4.5e-6 at K = 4096), the rounding of every d_j inside its w_j (2^-24 |d_j| relative: 2^-24 (H - log Z) over the sum) and logf's own
2 ulp, 2^-22 |log Z|.  T is at most 64 sequential fused multiply-adds per lane + 6 butterfly
stages (70 roundings), each term's w_j a few ulp (expf: 2, the rounding of d_j: |d_j| 2^-24 relative in w_j, which only matters where w_j
|d_j| is large, |d_j| ~ 1: 1 more), Z's own 16 * 2^-24 (the logprob bound's figure) and the division's rounding: (70 + 3 + 16 + 1) = 90
roundings of 2^-24 relative to |T / Z| = H - log Z, in the worst case of all of them adding up; the last subtraction rounds once.  So
    |dH| <= (NV + 12) * 2^-24 + 2^-22 |log Z| + 2^-23 |H| + (90 + 1) * 2^-24 (H - log Z),
which is below 1e-5 + 2^-23 |H| + 90 * 2^-24 (H - log Z) on every row (log Z <= H <= log K <= 8.4: the first two terms and the one more
rounding stay under 7e-6).
The kernel test prints the maxima it meets per K (DESIGN finding 96); they are measured against the fp64 restatement."""
import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.utils import synth
from tests import token_stats_ref as R
from tests.helpers import build_mage, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(frames_length=4, width=64, layers=1, vq_dim=32, K=16)          # tests/test_gpu_logprobs.py's models
FOLD = dict(frames_length=4, width=256, layers=3, vq_dim=32, K=16)
SAMPLED = dict(temperature=0.9, top_k=8, top_p=0.9)
FILTERS = [(0, 1.0), (20, 1.0), (0, 0.9), (20, 0.9), (1, 0.9)]              # tests/test_gpu_sampling.py's four + greedy by definition
TEMPS = (0.7, 1.0, 1.5)
NEW = ("last_token_policy_logprobs", "last_clip_policy_logprob", "last_token_kept", "last_token_entropy", "last_token_policy_entropy")
SPECIAL = dict(pm80=1, minus_inf=2, nan=8, all_minus_inf=9, uniform=10, pm100=12)


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _logits(rows, K, seed, every=None):
    """tests/test_gpu_sampling.py's recipe (ties on a 1/4 grid, a repeated top-20 boundary value) + the special rows, repeated from every
    `every`-th row on (one set per temperature)."""
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((rows, K))).astype(np.float32)
    for r in range(0, rows, 7):
        z[r] = np.round(z[r] * 4) / 4
    for r in range(3, rows, 11):
        o = np.argsort(-z[r], kind="stable")
        if K > 22:
            z[r, o[20:23]] = z[r, o[19]]
    for b in range(0, rows, every or rows):
        z[b + 1] = z[b + 1] / np.abs(z[b + 1]).max() * 80.0
        z[b + 12] = z[b + 12] / np.abs(z[b + 12]).max() * 100.0
        z[b + 2, g.integers(0, K, max(K // 3, 1))] = -np.inf
        z[b + 8, int(g.integers(0, K))] = np.nan
        z[b + 9, :] = -np.inf
        z[b + 10, :] = 0.5
    return z


def _bits(t):
    return t.contiguous().view(torch.int32)


def _close(got, want, bound, what):
    """NaN and infinite rows must agree exactly, the finite ones within `bound`; returns (max error, max error / bound)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN rows differ at {np.nonzero(np.isnan(got) != nan)[0][:8]}"
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinite rows differ"
    fin = ~nan & ~inf
    err = np.abs(got[fin] - want[fin])
    worst = int(np.argmax(err / bound[fin])) if fin.any() else 0
    assert (err <= bound[fin]).all(), f"{what}: |d| {err[worst]:.3e} > bound {bound[fin][worst]:.3e} at row {np.nonzero(fin)[0][worst]}"
    return (float(err.max()), float((err / bound[fin]).max())) if fin.any() else (0.0, 0.0)


def _entropy_bound(h, log_z, K):
    nv = max(4, -(-K // 64))                                        # values per lane (the kernel's instance holds at least as many adds)
    nv = 1 << (nv - 1).bit_length()
    with np.errstate(invalid="ignore"):
        return (nv + 12) * 2.0 ** -24 + 2.0 ** -22 * np.abs(log_z) + 2.0 ** -23 * np.abs(h) + 91 * 2.0 ** -24 * (h - log_z)


def _want_rows(z, tok, kept, T, k, p):
    """The restatement of every row, each under the admissible set whose size the kernel reported (none: an assertion)."""
    lp, ent, lz, n_multi = [], [], [], 0
    for r in range(z.shape[0]):
        sets = R.admissible_sets(z[r], T, k, p)
        n_multi += len(sets) > 1
        hit = [N for N in sets if int(N.sum()) == int(kept[r])]
        assert len(hit) == 1, f"row {r} (T={T} top_k={k} top_p={p}): kept {int(kept[r])}, admissible sizes {[int(N.sum()) for N in sets]}"
        st = R.stats_for_set(z[r], int(tok[r]), T, k, hit[0])
        lp.append(st["policy_logprob"])
        ent.append(st["policy_entropy"])
        lz.append(st["log_z"])
    return np.array(lp), np.array(ent), np.array(lz), n_multi


@pytest.mark.parametrize("K", [4, 512, 4096])
def test_kernel_matches_restatement(K):
    chunk, group, pos_off = 384, 64, 1000                           # 3 x 384 = 1152 rows, a third at each temperature
    rows = 3 * chunk
    z = _logits(rows, K, seed=K, every=chunk)
    zd = torch.from_numpy(z).to(DEV)
    g = np.random.default_rng(K + 1)
    sd_ = torch.from_numpy(g.integers(-2 ** 63, 2 ** 63 - 1, rows // group, dtype=np.int64)).to(DEV)
    rand = torch.from_numpy(g.integers(0, K, rows)).to(DEV)
    drawn = np.arange(rows) % 2 == 0                                # even rows keep the sampler's token, odd rows get a uniform one
    all_inf = np.isneginf(z).all(1)
    assert all_inf.sum() == 3 and not drawn[all_inf].any()          # (their every output is NaN by definition: inf - inf)
    h_lz = np.array([R._entropy(z[r].astype(np.float64)) for r in range(rows)])        # the plain entropy: one reference for every filter
    ent_first = None
    for k, p in FILTERS:
        k = min(k, K // 2) if k > 1 else k                          # K = 4: top_k = 2
        tok = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
        plp, pent, ent = (torch.full((rows + 1,), 7.0, device=DEV) for _ in range(3))
        kept = torch.full((rows + 1,), -7, dtype=torch.int32, device=DEV)
        for ti, T in enumerate(TEMPS):
            lo = ti * chunk
            ops.sample_tokens(zd[lo:], tok[lo:], sd_[lo // group:], rows=chunk, K=K, temperature=T, top_k=k, top_p=p, pos_off=pos_off, group=group)
        tok[1::2] = rand[1::2]
        for ti, T in enumerate(TEMPS):
            lo = ti * chunk
            ops.token_stats(zd[lo:], tok[lo:], rows=chunk, K=K, temperature=T, top_k=k, top_p=p, policy_logprob=plp[lo:], policy_entropy=pent[lo:],
                            kept=kept[lo:], entropy=ent[lo:])
        ops.check_device_errors(DEV)
        assert plp[rows].item() == 7.0 and pent[rows].item() == 7.0 and ent[rows].item() == 7.0 and kept[rows].item() == -7     # past `rows`
        if ent_first is None:
            ent_first = ent.clone()
            e_h = _close(ent[:rows].cpu().numpy(), h_lz[:, 1], _entropy_bound(h_lz[:, 1], h_lz[:, 0], K), f"K={K} entropy")
            assert np.isnan(h_lz[np.isnan(z).any(1), 1]).all()
        assert torch.equal(_bits(ent), _bits(ent_first))             # the plain entropy does not see the filter or the temperature
        tk, kp = tok.cpu().numpy(), kept[:rows].cpu().numpy()
        want_lp, want_ent, want_lz, multi = [], [], [], 0
        for ti, T in enumerate(TEMPS):
            sl = slice(ti * chunk, (ti + 1) * chunk)
            a, b, c, n = _want_rows(z[sl], tk[sl], kp[sl], T, k, p)
            want_lp, want_ent, want_lz, multi = want_lp + [a], want_ent + [b], want_lz + [c], multi + n
        want_lp, want_ent, want_lz = np.concatenate(want_lp), np.concatenate(want_ent), np.concatenate(want_lz)
        got_lp = plp[:rows].cpu().numpy()
        assert np.isfinite(got_lp[drawn]).all(), "a token the sampler drew is outside the reported set"
        assert (kp[~np.isnan(z).all(1)] >= 1).all() and (kp <= K).all()
        e_lp = _close(got_lp, want_lp, 1e-5 + 2.0 ** -23 * np.abs(want_lp), f"K={K} top_k={k} top_p={p} policy_logprob")
        e_pe = _close(pent[:rows].cpu().numpy(), want_ent, _entropy_bound(want_ent, want_lz, K), f"K={K} top_k={k} top_p={p} policy_entropy")
        print(f"K={K} top_k={k} top_p={p}: {rows} rows ({multi} with several admissible thresholds), policy_logprob max |d| {e_lp[0]:.3e} "
              f"({e_lp[1]:.3f} of its bound), policy_entropy {e_pe[0]:.3e} ({e_pe[1]:.3f}), entropy {e_h[0]:.3e} ({e_h[1]:.3f}), "
              f"-inf tokens {int(np.isneginf(got_lp).sum())}, kept {int(kp.min())}..{int(kp.max())}")
        if k == 1:
            assert set(np.unique(kp)) == {1} and set(np.unique(got_lp[~np.isnan(got_lp)])) <= {0.0, -np.inf}
            assert (pent[:rows] == 0).all()


@pytest.mark.parametrize("K", [4, 260, 512, 1024, 2048, 4096])
def test_unfiltered_policy_logprob_is_token_logprob_bit_for_bit(K):
    rows = 300
    z = _logits(rows, K, seed=K + 7)
    zd = torch.from_numpy(z).to(DEV)
    tok = torch.from_numpy(np.random.default_rng(K).integers(0, K, rows)).to(DEV)
    lp, plp = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    kept = torch.empty(rows, dtype=torch.int32, device=DEV)
    ops.token_logprob(zd, tok, lp, rows=rows, K=K)
    ops.token_stats(zd, tok, rows=rows, K=K, temperature=1.0, top_k=0, top_p=1.0, policy_logprob=plp, kept=kept)
    ops.check_device_errors(DEV)
    clean = torch.from_numpy(~np.isnan(z).any(1)).to(DEV)
    a, b = lp[clean], plp[clean]
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and int(torch.isnan(a).sum()) == 1       # (the row of -inf only)
    assert torch.equal(_bits(a[~torch.isnan(a)]), _bits(b[~torch.isnan(a)]))
    assert (kept[clean] == K).all() and kept[SPECIAL["nan"]].item() == K - 1
    ops.token_stats(zd, tok, rows=rows, K=K, temperature=1.0, top_k=K, top_p=1.0, policy_logprob=lp)            # top_k = K: off as well
    assert torch.equal(_bits(lp[clean][~torch.isnan(a)]), _bits(b[~torch.isnan(a)]))


def _stats(zd, tok, rows, K, T, k, p, **addr):
    out = dict(policy_logprob=torch.full((rows,), 7.0, device=DEV), policy_entropy=torch.full((rows,), 7.0, device=DEV),
               kept=torch.full((rows,), -7, dtype=torch.int32, device=DEV), entropy=torch.full((rows,), 7.0, device=DEV))
    ops.token_stats(zd, tok, rows=rows, K=K, temperature=T, top_k=k, top_p=p, **out, **addr)
    return out


@pytest.mark.parametrize("k,p", [(20, 0.9), (0, 1.0), (1, 1.0)])
def test_a_rows_bits_depend_on_the_row_alone(k, p):
    K, rows, T = 512, 301, 0.9                                      # 75 workgroups of 4 waves and a partial one
    z = _logits(rows, K, seed=31)
    zd = torch.from_numpy(z).to(DEV)
    tok = torch.from_numpy(np.random.default_rng(4).integers(0, K, rows)).to(DEV)
    base = _stats(zd, tok, rows, K, T, k, p)
    shifted = _stats(zd[37:], tok[37:], rows - 37, K, T, k, p)      # the same rows at another row index
    for r in (2, 9, 40):                                            # ... and launched alone
        alone = _stats(zd[r:], tok[r:], 1, K, T, k, p)
        for n in base:
            assert torch.equal(_bits(alone[n]), _bits(base[n][r:r + 1])), (n, r)
    for n in base:
        assert torch.equal(_bits(shifted[n]), _bits(base[n][37:])), n
    # only some outputs asked for: the same bits in those, nothing else written
    part = dict(policy_entropy=torch.full((rows,), 7.0, device=DEV))
    ops.token_stats(zd, None, rows=rows, K=K, temperature=T, top_k=k, top_p=p, **part)
    assert torch.equal(_bits(part["policy_entropy"]), _bits(base["policy_entropy"]))
    ops.check_device_errors(DEV)


def test_regrouped_addressing_writes_only_its_slots():
    K, T, k, p = 512, 0.9, 20, 0.9
    z = _logits(4 * 5 * 2, K, seed=52)
    zd = torch.from_numpy(z).to(DEV)
    tok = torch.from_numpy(np.random.default_rng(3).integers(0, K, (4, 5, 2))).to(DEV)
    # frame 2 of [B=4, T=5, hw=2, K] logits, tokens in slot 3 of a [4, 5, 2] buffer: the results land in slot 3 of the outputs
    out = dict(policy_logprob=torch.full((4, 5, 2), -77.0, device=DEV), policy_entropy=torch.full((4, 5, 2), -77.0, device=DEV),
               kept=torch.full((4, 5, 2), -77, dtype=torch.int32, device=DEV), entropy=torch.full((4, 5, 2), -77.0, device=DEV))
    ops.token_stats(zd, tok, rows=8, K=K, temperature=T, top_k=k, top_p=p, group=2, in_group_stride=10, in_off=4, tok_group_stride=10, tok_off=6,
                    **out)
    ops.check_device_errors(DEV)
    flat = _stats(zd.view(4, 5, 2, K)[:, 2].reshape(8, K).contiguous(), tok[:, 3].reshape(8).contiguous(), 8, K, T, k, p)
    sent = torch.ones(4, 5, 2, dtype=torch.bool, device=DEV)
    sent[:, 3] = False
    for n in out:
        assert (out[n][sent] == -77).all(), n
        assert torch.equal(_bits(out[n][:, 3].reshape(8)), _bits(flat[n])), n


def test_token_out_of_range_surfaces_in_check_device_errors():
    K = 16
    z = torch.zeros(8, K, device=DEV)
    for bad in (K, -1):
        tok = torch.arange(8, device=DEV, dtype=torch.int64)
        tok[3] = bad
        out = torch.empty(8, device=DEV)
        ops.token_stats(z, tok, rows=8, K=K, policy_logprob=out)
        with pytest.raises(ValueError, match="token out of range"):
            ops.check_device_errors(DEV)
        assert torch.allclose(out, torch.full((8,), -float(np.log(K)), device=DEV))
    ops.check_device_errors(DEV)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(**SMALL), 5, DEV)
    return m, synth.synth_batch_mnist(2, SMALL["frames_length"], seed=5)


@pytest.fixture(scope="module")
def fold():
    m = build_mage(synth.mnist_model_config(**FOLD), 6, DEV)
    return m, synth.synth_batch_mnist(2, FOLD["frames_length"], seed=6)


def _reset(m):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32")
    m.use_graph, m.streams, m.ar_mode = None, 1, "full"


def _gen(m, batch, seeds=None):
    """One generation: every result on the CPU, by attribute name (None: not left)."""
    b = dev_batch(batch if seeds is None else {**batch, "sample_seed": seeds})
    v = m.autoregressive_generate(b)
    res = {a: getattr(m, a) for a in m._LOGPROB_RESULTS + ("last_tokens",)}
    return {"video": v.cpu(), **{a: None if t is None else t.cpu() for a, t in res.items()}}


def _same(a, b, names):
    for n in names:
        assert a[n] is not None and a[n].shape == b[n].shape and a[n].dtype == b[n].dtype, n
        assert torch.equal(_bits(a[n]) if a[n].dtype == torch.float32 else a[n], _bits(b[n]) if b[n].dtype == torch.float32 else b[n]), n


@pytest.mark.parametrize("cfg,precision", [("small", "fp32"), ("small", "f16x3"), ("fold", "bf16")])
def test_sampled_results_agree_across_modes(request, cfg, precision):
    m, batch = request.getfixturevalue(cfg)
    K, L = m.codebook_size, m.frames_length
    seeds = torch.tensor([41, -9], dtype=torch.int64)
    names = NEW + ("last_tokens", "last_token_logprobs", "last_clip_logprob", "video")
    _reset(m)
    m.set_precision(precision).set_sampling(**SAMPLED).set_logprobs(True, policy=True, entropy=True)
    m.use_graph = False
    full = _gen(m, batch, seeds)
    m.ar_mode = "incremental"
    inc = _gen(m, batch, seeds)
    m.streams = 2                                                   # (B = 2 < 2 * streams: still ONE group -- two real groups: the next test)
    st2 = _gen(m, batch, seeds)
    m.streams = 1
    one = _gen(m, {k_: v[:1] for k_, v in batch.items()}, seeds[:1])
    m.set_logprobs(True)
    plain = _gen(m, batch, seeds)                                   # the new flags off again: nothing of theirs is left
    _reset(m)
    _same(inc, full, names)
    _same(st2, inc, names)
    _same(one, {n: inc[n][:1] for n in names}, names)
    assert all(plain[a] is None for a in NEW) and torch.equal(plain["last_tokens"], inc["last_tokens"])
    assert torch.equal(_bits(plain["last_token_logprobs"]), _bits(inc["last_token_logprobs"]))
    plp, kept = full["last_token_policy_logprobs"], full["last_token_kept"]
    assert plp.shape == full["last_tokens"].shape == kept.shape and plp.dtype == torch.float32 and kept.dtype == torch.int32
    assert full["last_clip_policy_logprob"].shape == (2,) and full["last_candidate_policy_scores"] is None
    assert torch.isfinite(plp).all() and (plp <= 0).all()           # every token was drawn by this sampler
    assert (kept >= 1).all() and (kept <= K).all()
    for a in ("last_token_entropy", "last_token_policy_entropy"):
        assert (full[a] >= 0).all() and (full[a] <= np.log(K) + 1e-5).all()
    assert (full["last_token_policy_entropy"] <= torch.log(kept.double()) + 1e-5).all()
    want_clip = plp.double().flatten(1).sum(1)
    assert (full["last_clip_policy_logprob"].double() - want_clip).abs().max() <= 1e-4


@pytest.mark.parametrize("cand", [1, 2])
def test_streams_concatenate_the_groups(small, monkeypatch, cand):
    """B = 4 with streams = 2 is two groups of two clips on two HIP streams (_generate_multistream: every result is the groups' torch.cat):
    every new result, the int32 kept sizes and the [B, N] candidate policy scores included, has streams = 1's bits, in both AR modes."""
    m, _ = small
    batch = synth.synth_batch_mnist(4, SMALL["frames_length"], seed=8)
    seeds = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    names = NEW + ("last_tokens", "last_token_logprobs", "last_clip_logprob", "video")
    if cand > 1:
        names += ("last_candidate_policy_scores", "last_candidate_scores", "last_candidate_index")
    groups = []
    inner = m._generate_multistream
    monkeypatch.setattr(m, "_generate_multistream", lambda b, n: (groups.append(n), inner(b, n))[1])
    _reset(m)
    m.set_sampling(candidates=cand, **SAMPLED).set_logprobs(True, policy=True, entropy=True)
    m.use_graph = False
    res = {}
    for mode in ("incremental", "full"):
        m.ar_mode = mode
        for n in (1, 2):
            m.streams = n
            res[mode, n] = _gen(m, batch, seeds)
    _reset(m)
    assert groups == [2, 2]                                         # the two streams = 2 calls did split, the streams = 1 ones did not
    for mode in ("incremental", "full"):
        _same(res[mode, 2], res[mode, 1], names)
    _same(res["full", 2], res["incremental", 2], names)
    r = res["incremental", 2]
    assert r["last_token_kept"].shape == r["last_tokens"].shape and r["last_tokens"].shape[0] == 4 and r["last_token_kept"].dtype == torch.int32
    assert r["last_clip_policy_logprob"].shape == (4,) and torch.isfinite(r["last_token_policy_logprobs"]).all()
    if cand > 1:
        assert r["last_candidate_policy_scores"].shape == (4, cand)
    else:
        assert r["last_candidate_policy_scores"] is None


def test_renormalising_over_a_subset_raises_a_logprob(small):
    m, batch = small
    _reset(m)
    m.set_sampling(1.0, top_k=8, top_p=0.9).set_logprobs(True, policy=True)
    m.use_graph, m.ar_mode = False, "incremental"
    r = _gen(m, batch, torch.tensor([3, 4], dtype=torch.int64))
    _reset(m)
    assert r["last_token_entropy"] is None and r["last_token_policy_entropy"] is None          # entropy was not asked for
    assert (r["last_token_policy_logprobs"] >= r["last_token_logprobs"] - 2e-5).all()
    assert (r["last_token_policy_logprobs"] > r["last_token_logprobs"] + 1e-3).any()           # ... and does raise it where something was cut


@pytest.mark.timeout(120)
def test_graph_replay_equals_eager(small):
    m, batch = small
    one = {k: v[:1] for k, v in batch.items()}
    seeds = torch.tensor([77], dtype=torch.int64)
    names = NEW + ("last_tokens", "last_token_logprobs", "video")
    _reset(m)
    m.set_sampling(**SAMPLED).set_logprobs(True, policy=True, entropy=True)
    m.ar_mode, m.use_graph = "incremental", False
    eager = _gen(m, one, seeds)
    m.use_graph = True
    modes = []
    for rep in range(3):                                            # warm-up (eager), capture + replay, replay
        g = _gen(m, one, seeds)
        modes.append(m.last_call_mode)
        _same(g, eager, names)
    keep = m.last_token_policy_logprobs
    held = keep.clone()
    other = _gen(m, one, seeds + 1)                                  # other seeds through the same graph: earlier results are not overwritten
    last = m.last_call_mode
    assert torch.equal(keep, held)
    _reset(m)
    assert modes[-1] == "graph" and last == "graph"
    assert not torch.equal(other["last_token_policy_logprobs"], eager["last_token_policy_logprobs"])


def test_candidates_report_every_policy_score(small):
    m, batch = small
    N, seeds = 2, torch.tensor([1234, -77], dtype=torch.int64)
    _reset(m)
    m.use_graph, m.ar_mode = False, "incremental"
    m.set_sampling(**SAMPLED).set_logprobs(True, policy=True, entropy=True)
    plain = [_gen(m, batch, seeds + c) for c in range(N)]
    m.set_sampling(candidates=N, **SAMPLED)
    best = _gen(m, batch, seeds)
    m.set_logprobs(False)                                           # the winner is picked by the model log-probability, flags or not
    ref = _gen(m, batch, seeds)
    m.ar_mode = "full"
    m.set_logprobs(True, policy=True, entropy=True)
    best_f = _gen(m, batch, seeds)
    m.score(dev_batch(batch))                                       # score has no candidates: it leaves no stale [B, N] scores behind
    after_score = m.last_candidate_policy_scores
    _reset(m)
    assert after_score is None
    ps = best["last_candidate_policy_scores"]
    assert ps.shape == (2, N) and ps.dtype == torch.float32
    assert torch.equal(_bits(ps), _bits(torch.stack([p["last_clip_policy_logprob"] for p in plain], 1)))
    idx = best["last_candidate_index"]
    assert torch.equal(idx, ref["last_candidate_index"]) and torch.equal(best["last_tokens"], ref["last_tokens"]) and ref["last_token_kept"] is None
    for b in range(2):
        w = plain[int(idx[b])]
        for a in NEW:
            assert torch.equal(_bits(best[a][b]) if best[a].dtype == torch.float32 else best[a][b],
                               _bits(w[a][b]) if w[a].dtype == torch.float32 else w[a][b]), (a, b)
        assert best["last_clip_policy_logprob"][b] == ps[b, idx[b]]
    _same(best_f, best, NEW + ("last_candidate_policy_scores", "last_tokens"))


def _check_against_own_logits(m, res, sampling):
    """Check 1's rule and bounds on the call's own last_logits / last_tokens."""
    K = m.codebook_size
    lg = res["last_logits"].reshape(-1, K).numpy()
    tk = res["last_tokens"].reshape(-1).numpy()
    h_lz = np.array([R._entropy(lg[r].astype(np.float64)) for r in range(lg.shape[0])])
    e = _close(res["last_token_entropy"].reshape(-1).numpy(), h_lz[:, 1], _entropy_bound(h_lz[:, 1], h_lz[:, 0], K), "entropy")
    print(f"own logits, entropy: {lg.shape[0]} rows, max |d| {e[0]:.3e} ({e[1]:.3f} of its bound)")
    if sampling is None:
        return
    T, k, p = sampling
    lp, ent, lz, multi = _want_rows(lg, tk, res["last_token_kept"].reshape(-1).numpy(), T, k, p)
    assert np.isfinite(lp).all()
    e1 = _close(res["last_token_policy_logprobs"].reshape(-1).numpy(), lp, 1e-5 + 2.0 ** -23 * np.abs(lp), "policy_logprob")
    e2 = _close(res["last_token_policy_entropy"].reshape(-1).numpy(), ent, _entropy_bound(ent, lz, K), "policy_entropy")
    print(f"own logits, sampled: {multi} rows with several admissible thresholds, policy_logprob max |d| {e1[0]:.3e} ({e1[1]:.3f}), "
          f"policy_entropy {e2[0]:.3e} ({e2[1]:.3f})")


def test_full_loop_results_match_the_restatement_on_its_own_logits(small):
    m, batch = small
    _reset(m)
    m.use_graph = False
    m.set_logprobs(True, entropy=True)                              # greedy: the plain entropy alone
    m.autoregressive_generate(dev_batch(batch))
    res = {a: None if getattr(m, a) is None else getattr(m, a).cpu() for a in NEW + ("last_logits", "last_tokens")}
    assert res["last_token_policy_entropy"] is None and res["last_token_policy_logprobs"] is None and res["last_token_kept"] is None
    _check_against_own_logits(m, res, None)
    m.set_sampling(**SAMPLED).set_logprobs(True, policy=True, entropy=True)
    m.autoregressive_generate(dev_batch({**batch, "sample_seed": torch.tensor([5, 6], dtype=torch.int64)}))
    res = {a: getattr(m, a).cpu() for a in NEW + ("last_logits", "last_tokens")}
    sampling = m.sampling
    _reset(m)
    _check_against_own_logits(m, res, sampling)


def test_score_honours_the_flags(small):
    m, batch = small
    K, T, k, p = m.codebook_size, 0.8, 2, 1.0
    _reset(m)
    b = dev_batch(batch)
    tok, logits = m.teacher_forced_logits(b)
    lg, tk = logits.reshape(-1, K).cpu().numpy(), tok[:, 1:].reshape(-1).cpu().numpy()
    want = [R.row_stats(lg[r], int(tk[r]), T, k, p) for r in range(lg.shape[0])]
    want_lp = np.array([w["policy_logprob"] for w in want]).reshape(2, -1)
    assert np.isneginf(want_lp).any(1).all() and np.isfinite(want_lp).any()      # the reference alone: every clip holds a token outside the top 2
    plain = m.score(b).cpu()
    assert all(getattr(m, a) is None for a in NEW)
    m.set_sampling(T, top_k=k, top_p=p).set_logprobs(True, policy=True, entropy=True)
    got = m.score(b).cpu()
    res = {a: getattr(m, a).cpu() for a in NEW + ("last_token_logprobs",)}
    _reset(m)
    assert torch.equal(_bits(got), _bits(plain)) and torch.isfinite(got).all()   # the model log-likelihood itself does not change
    plp = res["last_token_policy_logprobs"]
    assert plp.shape == res["last_token_logprobs"].shape
    _close(plp.reshape(-1).numpy(), want_lp.reshape(-1), 1e-5 + 2.0 ** -23 * np.abs(want_lp.reshape(-1)), "score policy_logprob")
    assert np.array_equal(res["last_token_kept"].reshape(-1).numpy(), np.array([w["kept"] for w in want]))
    ent, lz = np.array([w["policy_entropy"] for w in want]), np.array([w["log_z"] for w in want])
    _close(res["last_token_policy_entropy"].reshape(-1).numpy(), ent, _entropy_bound(ent, lz, K), "score policy_entropy")
    h_lz = np.array([R._entropy(lg[r].astype(np.float64)) for r in range(lg.shape[0])])
    _close(res["last_token_entropy"].reshape(-1).numpy(), h_lz[:, 1], _entropy_bound(h_lz[:, 1], h_lz[:, 0], K), "score entropy")
    assert torch.isneginf(res["last_clip_policy_logprob"]).all()     # a token the sampler could never draw: so is the clip's total


def test_off_is_off_and_on_is_counted(small, monkeypatch):
    """Flags off: not one call to mage_token_stats, and the launch sequence with set_logprobs(True) is the plain one plus
    mage_token_logprob / mage_clip_scores.  Flags on: exactly one mage_token_stats behind every mage_token_logprob, one more
    mage_clip_scores for policy."""
    m, batch = small
    calls = count_lib_calls(monkeypatch)
    ours = ("mage_token_logprob", "mage_clip_scores", "mage_token_stats")
    Lm1 = SMALL["frames_length"] - 1

    def run(b):
        del calls[:]
        m.autoregressive_generate(b)
        return list(calls)
    _reset(m)
    m.use_graph = False
    for sampled in (False, True):
        b = dev_batch({**batch, "sample_seed": torch.tensor([8, 9], dtype=torch.int64)} if sampled else batch)
        for mode in ("incremental", "full"):
            m.ar_mode = mode
            m.set_sampling(**SAMPLED) if sampled else m.set_sampling(None)
            m.set_logprobs(False)
            run(b)                                                  # derived caches built
            off = run(b)
            assert not [c for c in off if c in ours] and all(getattr(m, a) is None for a in m._LOGPROB_RESULTS)
            m.set_logprobs(True)
            on = run(b)
            sites = Lm1 if mode == "incremental" or sampled else 1
            assert [c for c in on if c in ours] == ["mage_token_logprob"] * sites + ["mage_clip_scores"]
            assert [c for c in on if c not in ours] == off and all(getattr(m, a) is None for a in NEW)
            m.set_logprobs(True, policy=sampled, entropy=True)
            both = run(b)
            assert [c for c in both if c in ours] == ["mage_token_logprob", "mage_token_stats"] * sites + ["mage_clip_scores"] * (1 + sampled)
            assert [c for c in both if c not in ours] == off
            m.set_logprobs(True)
            assert run(b) == on
            m.set_logprobs(False)
            assert run(b) == off and m.last_token_entropy is None
    _reset(m)


def test_refusals(small):
    m, batch = small
    _reset(m)
    for kw in (dict(policy=True), dict(entropy=True)):
        with pytest.raises(ValueError, match="on=True"):
            m.set_logprobs(False, **kw)
    m.set_logprobs(True, policy=True)                               # accepted: sampling may still be switched on before the call
    b = dev_batch(batch)
    with pytest.raises(ValueError, match="set_sampling"):
        m.autoregressive_generate(b)
    with pytest.raises(ValueError, match="set_sampling"):
        m.score(b)
    m.set_logprobs(True, entropy=True)                              # entropy alone works with greedy decoding
    m.autoregressive_generate(b)
    assert m.last_token_entropy is not None and m.last_token_policy_entropy is None and m.last_token_kept is None
    _reset(m)
    p = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0, DEV)
    for kw in (dict(policy=True), dict(entropy=True)):
        with pytest.raises(ValueError, match="use_cids=False"):
            p.set_logprobs(True, **kw)
