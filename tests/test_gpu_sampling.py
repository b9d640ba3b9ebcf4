"""GPU: seeded token sampling (mage_sample_tokens, MAGE.set_sampling) against the fp64 restatement of its rule (tests/sampling_ref.py):
exact draws at kernel level, the argmax row addressing, top_k = 1 == greedy, the law of the draws (chi-square), sampled generation
against the CPU oracle's teacher-forced logits, and the bitwise invariants a seeded stream promises at BASELINE cfg2 size (batch size,
clip slice, AR mode, streams, graph replay)."""
import math

import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.utils import synth
from oracle import mage_oracle as O
from tests import sampling_ref as R
from tests.helpers import build_mage, cpu_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILTERS = [(0, 1.0), (20, 1.0), (0, 0.9), (20, 0.9)]            # (top_k, top_p): none, top-k, top-p, both


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _logits(rows, K, seed):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((rows, K))).astype(np.float32)
    for r in range(0, rows, 7):                                    # constructed ties everywhere (both boundaries): values on a 1/4 grid
        z[r] = np.round(z[r] * 4) / 4
    for r in range(3, rows, 11):                                   # the top-20 boundary value repeated
        o = np.argsort(-z[r], kind="stable")
        if K > 22:
            z[r, o[20:23]] = z[r, o[19]]
    return z


def _check_rows(z, got, T, k, p, seeds, group, pos_off, tol=1e-5):
    hard = soft = 0
    for r in range(z.shape[0]):
        want, near = R.sample_row(z[r], T, k, p, int(seeds[r // group]), pos_off + r % group, tol)
        if int(got[r]) != want:
            if near:
                soft += 1
            else:
                hard += 1
    return hard, soft


@pytest.mark.parametrize("K", [4, 512, 4096])
def test_kernel_draws_match_restatement(K):
    chunk, group, pos_off = 1408, 64, 1000                          # 3 x 1408 = 4224 rows, a third at each temperature
    rows = 3 * chunk
    z = _logits(rows, K, seed=K)
    zd = torch.from_numpy(z).to(DEV)
    seeds = torch.from_numpy(np.random.default_rng(K + 1).integers(-2 ** 63, 2 ** 63 - 1, rows // group, dtype=np.int64))
    sd_ = seeds.to(DEV)
    for k, p in FILTERS:
        k = min(k, K // 2)                                          # K = 4: top_k = 2
        got = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
        for ti, T in enumerate((0.7, 1.0, 1.5)):
            lo = ti * chunk
            ops.sample_tokens(zd[lo:], got[lo:], sd_[lo // group:], rows=chunk, K=K, temperature=T, top_k=k, top_p=p, pos_off=pos_off,
                              group=group)
        g = got.cpu().numpy()
        hard = soft = 0
        for ti, T in enumerate((0.7, 1.0, 1.5)):
            lo = ti * chunk
            h, s = _check_rows(z[lo:lo + chunk], g[lo:lo + chunk], T, k, p, seeds[lo // group:].numpy(), group, pos_off)
            hard, soft = hard + h, soft + s
        print(f"K={K} top_k={k} top_p={p}: {rows} rows, hard mismatches {hard}, soft {soft}")
        assert hard == 0
        assert soft <= rows // 1000


def test_regrouped_addressing_writes_only_its_slots():
    K = 512
    lg = torch.from_numpy(_logits(4 * 5 * 2, K, seed=52))
    seeds = torch.tensor([3, -7, 11, 2 ** 62], dtype=torch.int64)
    buf = torch.full((4, 5, 2), -1, device=DEV, dtype=torch.int64)
    # frame 2 of [B=4, T=5, hw=2, K] -> slot 3 of a [B, 5, hw] token buffer, positions 2*hw + pixel
    ops.sample_tokens(lg.to(DEV), buf, seeds.to(DEV), rows=8, K=K, temperature=1.0, top_k=20, top_p=0.9, pos_off=4, group=2,
                      in_group_stride=10, in_off=4, out_group_stride=10, out_off=6)
    want = torch.full((4, 5, 2), -1, dtype=torch.int64)
    for b in range(4):
        for px in range(2):
            want[b, 3, px] = R.sample_row(lg.view(4, 5, 2, K)[b, 2, px].numpy(), 1.0, 20, 0.9, int(seeds[b]), 4 + px)[0]
    assert torch.equal(buf.cpu(), want)


def test_top_k_1_is_argmax():
    K, rows = 512, 2048
    z = torch.from_numpy(_logits(rows, K, seed=9)).to(DEV)
    want = torch.empty(rows, dtype=torch.int64, device=DEV)
    ops.argmax(z, want, rows=rows, K=K)
    seeds = torch.tensor([5], dtype=torch.int64, device=DEV)
    for T, p in ((1.0, 1.0), (0.3, 0.5), (2.0, 0.9)):
        got = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
        ops.sample_tokens(z, got, seeds, rows=rows, K=K, temperature=T, top_k=1, top_p=p)
        assert torch.equal(got, want)


def _chi2_z(counts, p):
    """Wilson-Hilferty normal score of Pearson's statistic (bins with expected count < 5 pooled)."""
    n = counts.sum()
    e = n * p
    small = e < 5
    obs = np.append(counts[~small], counts[small].sum()) if small.any() else counts
    exp = np.append(e[~small], e[small].sum()) if small.any() else e
    keep = exp > 0
    x2 = float((((obs - exp) ** 2)[keep] / exp[keep]).sum())
    df = int(keep.sum()) - 1
    return ((x2 / df) ** (1 / 3) - (1 - 2 / (9 * df))) / math.sqrt(2 / (9 * df)), x2, df


@pytest.mark.parametrize("k,p", FILTERS)
def test_draws_follow_the_target_distribution(k, p):
    K, n, T = 64, 1 << 16, 1.0
    z = (1.5 * np.random.default_rng(77).standard_normal(K)).astype(np.float32)
    zd = torch.from_numpy(z).to(DEV).repeat(n, 1).contiguous()
    got = torch.empty(n, dtype=torch.int64, device=DEV)
    ops.sample_tokens(zd, got, torch.tensor([123456789], dtype=torch.int64, device=DEV), rows=n, K=K, temperature=T, top_k=k, top_p=p)
    counts = np.bincount(got.cpu().numpy(), minlength=K).astype(np.float64)
    want = R.target_distribution(z, T, k, p)
    assert counts[want == 0].sum() == 0, "a code outside the candidate set was drawn"
    zs, x2, df = _chi2_z(counts, want)
    print(f"top_k={k} top_p={p}: {int((want > 0).sum())} candidates, chi2 {x2:.1f} on {df} dof (normal score {zs:.2f})")
    assert zs < 4.5


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.8, 32, 0.9)])
def test_sampled_generation_matches_oracle_teacher_forced(T, k, p):
    """fp32: every sampled token == the restatement applied to the oracle's logits on the GPU's own prefix (so one soft flip cannot
    cascade); frames == the oracle's decode of those tokens."""
    L, B, seed = 6, 4, 13
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=3, vq_dim=32, K=64), seed, DEV)
    sd = cpu_sd(m)
    batch = synth.synth_batch_mnist(B, L, seed=seed)
    seeds = torch.tensor([1, -2, 3 ** 30, 99], dtype=torch.int64)
    m.set_sampling(T, top_k=k, top_p=p)
    video = m.autoregressive_generate(dev_batch({**batch, "sample_seed": seeds})).cpu()
    gen = m.last_tokens.cpu()
    R_, Lm1, K = m.image_resolution, L - 1, m.codebook_size
    hw = R_ * R_
    tok0 = O.vqvae_encode(sd, "first_stage_model.", batch["images"][:, 0])
    assert torch.equal(tok0, m.first_stage_encode(batch["images"][:, 0:1].to(DEV))[:, 0].cpu())
    with torch.no_grad():
        ma = O.motion_anchor(sd, tok0, batch["text"], batch.get("speed"))
        cur = torch.cat([tok0[:, None], gen[:, :Lm1 - 1]], 1)
        lg = O.flat_axial_decoder(sd, "generate_model.", ma, O._frame_features(sd, cur)).numpy()
    tol = 1e-4 * float(R.inv_temperature(T))
    hard = soft = 0
    for b in range(B):
        for i in range(Lm1):
            for px in range(hw):
                want, near = R.sample_row(lg[b, i, px // R_, px % R_], T, k, p, int(seeds[b]), i * hw + px, tol)
                if int(gen[b, i, px // R_, px % R_]) != want:
                    soft, hard = soft + near, hard + (not near)
    print(f"T={T} top_k={k} top_p={p}: {B * Lm1 * hw} tokens, hard mismatches {hard}, soft {soft}")
    assert hard == 0 and soft <= max(5, B * Lm1 * hw // 1000)
    with torch.no_grad():
        want_frames = O.vqvae_decode(sd, "first_stage_model.", gen.view(B * Lm1, R_, R_)).view(B, Lm1, *video.shape[2:])
    assert (video[:, 1:] - want_frames).abs().max().item() <= 1e-4
    assert torch.equal(video[:, 0], batch["images"][:, 0])


@pytest.fixture(scope="module")
def cfg2():
    m = build_mage(synth.mnist_model_config(frames_length=16), 0, DEV).set_precision("bf16")
    batch = dev_batch(synth.synth_batch_mnist(64, 16, seed=3))
    seeds = torch.arange(64, dtype=torch.int64, device=DEV) * 7919 - 12345
    return m, batch, seeds


def _run(m, batch, seeds=None, **state):
    for a, v in state.items():
        setattr(m, a, v)
    b = batch if seeds is None else {**batch, "sample_seed": seeds}
    v = m.autoregressive_generate(b)
    return v, m.last_tokens.clone()


def test_cfg2_bf16_sampled_invariants(cfg2):
    m, batch, seeds = cfg2
    m.use_graph, m.streams = False, 1
    m.set_sampling(None)
    v_g, t_g = _run(m, batch, ar_mode="incremental")                                 # greedy, before any sampled call
    m.set_sampling(1.0, top_k=50, top_p=0.95)
    v_f, t_f = _run(m, batch, seeds, ar_mode="full")
    v_f2, t_f2 = _run(m, batch, seeds)
    assert torch.equal(t_f, t_f2) and torch.equal(v_f, v_f2)                         # same seeds: same result
    assert (t_f != t_g).flatten(1).any(1).float().mean().item() > 0.9                # sampling does change the tokens
    v_i, t_i = _run(m, batch, seeds, ar_mode="incremental")
    assert torch.equal(t_i, t_f) and torch.equal(v_i, v_f)                           # full loop == incremental loop
    v_s, t_s = _run(m, {k_: v[16:32] for k_, v in batch.items()}, seeds[16:32])
    assert torch.equal(t_s, t_i[16:32]) and torch.equal(v_s, v_i[16:32])             # a slice of clips alone == the same slice
    v_1, t_1 = _run(m, {k_: v[:1] for k_, v in batch.items()}, seeds[:1])
    assert torch.equal(t_1, t_i[:1]) and torch.equal(v_1, v_i[:1])                   # B = 1 == row 0
    v_2, t_2 = _run(m, batch, seeds, streams=2)
    assert torch.equal(t_2, t_i) and torch.equal(v_2, v_i)                           # two streams == one
    m.streams = 1
    v_o, t_o = _run(m, batch, seeds + 1)
    changed = (t_o != t_i).flatten(1).any(1).float().mean().item()
    print(f"cfg2 bf16 sampled: clips changed by other seeds {changed:.3f}, by greedy {(t_i != t_g).flatten(1).any(1).float().mean().item():.3f}")
    assert changed > 0.9                                                             # other seeds change most clips
    torch.manual_seed(321)
    v_n, t_n = _run(m, batch)                                                        # no seeds: drawn from the CPU generator
    used = m.last_sample_seeds.clone()
    assert used.shape == (64,) and used.dtype == torch.int64
    v_r, t_r = _run(m, batch, used)
    assert torch.equal(t_r, t_n) and torch.equal(v_r, v_n)
    torch.manual_seed(321)
    _, t_n2 = _run(m, batch)
    assert torch.equal(t_n2, t_n)                                                    # torch.manual_seed reproduces a call
    m.set_sampling(None)
    v_g2, t_g2 = _run(m, batch, seeds)                                               # greedy after sampled calls (seeds ignored)
    assert torch.equal(t_g2, t_g) and torch.equal(v_g2, v_g) and m.last_sample_seeds is None
    m.set_sampling(0.5, top_k=1, top_p=0.8)
    v_k1, t_k1 = _run(m, batch, seeds)
    assert torch.equal(t_k1, t_g) and torch.equal(v_k1, v_g)                         # top_k = 1 == greedy
    m.set_sampling(None)


def test_cfg2_bf16_graph_replay_equals_eager(cfg2):
    m, batch, seeds = cfg2
    small = {k_: v[:4] for k_, v in batch.items()}
    m.streams, m.ar_mode = 1, "incremental"
    for T in (1.0, 0.7, 1.0):
        m.set_sampling(T, top_k=50, top_p=0.95)
        m.use_graph = False
        v_e, t_e = _run(m, small, seeds[:4])
        m.use_graph = True
        for rep in range(3):                                    # warm-up (eager), capture + replay, replay
            v_g, t_g = _run(m, small, seeds[:4])
            assert torch.equal(t_g, t_e) and torch.equal(v_g, v_e), (T, rep, m.last_call_mode)
        assert m.last_call_mode == "graph"
        v_o, t_o = _run(m, small, seeds[:4] + 5)                 # new seeds through the same graph
        m.use_graph = False
        v_oe, t_oe = _run(m, small, seeds[:4] + 5)
        assert torch.equal(t_o, t_oe) and torch.equal(v_o, v_oe) and not torch.equal(t_o, t_e)
    m.use_graph = None
    m.set_sampling(None)


def test_cater_randomness_sampled_full_equals_incremental():
    L, B = 6, 2
    m = build_mage(synth.cater_model_config(frames_length=L), 0, DEV).set_precision("bf16")
    cb = synth.synth_batch_cater(B, L, seed=2)
    cb["video_noise"] = torch.randn(B, 64, 16, 16, generator=torch.Generator().manual_seed(5))
    cb["sample_seed"] = torch.tensor([17, -4], dtype=torch.int64)
    batch = dev_batch(cb)
    m.set_sampling(0.9, top_k=40, top_p=0.95)
    v = m.autoregressive_generate(batch)
    tk = m.last_tokens.clone()
    m.ar_mode = "incremental"
    vi = m.autoregressive_generate(batch)
    assert torch.equal(m.last_tokens, tk) and torch.equal(vi, v) and torch.isfinite(v).all()
