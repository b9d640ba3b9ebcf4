"""GPU: VectorQuantizedVAE.set_codebook_update on the small f4 and f8 stage-1 models: 'grad' after a round trip is the untouched model, one
EMA step is the rule (tests/codebook_ema_ref.py) on that step's ids and encoder rows, the derived caches follow the new codebook, runs
repeat and resume bit for bit, restarts undo a collapsed codebook where the gradient rule cannot, code_usage, and the refusals."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mage_amd import ops
from mage_amd.modules.vqvae_model import weights_frozen
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from tests import codebook_ema_ref as R
from tests.helpers import build_vqvae, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMA_KEYS = ["codebook.ema_cluster_size", "codebook.ema_embed_sum", "codebook.ema_step"]


def model(down_ratio, seed=13, dim=32, K=64):
    return build_vqvae(1 if down_ratio == 4 else 3, down_ratio, dim, K, seed, DEV).train()


def frames(down_ratio, n, seed):
    if down_ratio == 4:
        return synth.synth_batch_mnist(n, 1, seed=seed)["images"][:, 0].contiguous().to(DEV)               # [n, 1, 64, 64]
    return synth.synth_batch_cater(n, 1, seed=seed, res=64)["images"][:, 0].contiguous().to(DEV)          # [n, 3, 64, 64]


def loss_of(out, x, beta=0.25):
    x_tilde, z_e, z_q = out
    return F.mse_loss(x_tilde, x) + F.mse_loss(z_q, z_e.detach()) + beta * F.mse_loss(z_e, z_q.detach())   # the reference's three terms, as written


def rows_of(t):
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ---------------------------------------------------------------- 1. 'grad' after a round trip
@pytest.mark.parametrize("down_ratio", [4, 8])
def test_grad_mode_after_a_round_trip_is_the_untouched_model(down_ratio, monkeypatch):
    """Outputs, every gradient, the state_dict and the list of library calls of one training step.  (dim 64 on the f4 stack: at D = 32 the
    codebook's gradient comes from mage_embedding_bwd's floating-point atomics, which repeat no bits from run to run in either model.)"""
    dim = 64 if down_ratio == 4 else 32
    a, b = model(down_ratio, dim=dim), model(down_ratio, dim=dim)
    keys = list(a.state_dict())
    b.set_codebook_update("ema", restart_below=1.0)
    assert [k for k in b.state_dict() if k not in keys] == EMA_KEYS
    b.set_codebook_update("grad")
    assert list(b.state_dict()) == keys and b.codebook.embedding.weight.requires_grad
    x = frames(down_ratio, 2, 3)
    calls = count_lib_calls(monkeypatch)
    res = []
    for m in (a, b):
        del calls[:]
        out = m(x)
        loss_of(out, x).backward()
        res.append((out, {n: p.grad for n, p in m.named_parameters()}, list(calls)))
    monkeypatch.undo()
    (oa, ga, ca), (ob, gb, cb) = res
    assert ca == cb and "mage_embedding_bwd" in ca and "mage_code_stats" not in ca and "mage_codebook_ema" not in ca
    assert all(same_bits(u, v) for u, v in zip(oa, ob))
    assert set(ga) == set(gb) and all(g is not None for g in ga.values())
    for n in ga:
        assert same_bits(ga[n], gb[n]), n
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(same_bits(sa[k], sb[k]) for k in sa)
    assert b.last_codebook_stats is None


# ---------------------------------------------------------------- 2. one EMA step is the rule
@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("down_ratio", [4, 8])
def test_one_ema_step_is_the_rule(down_ratio, grad):
    m = model(down_ratio)
    kw = dict(decay=0.9, eps=1e-5, restart_below=1.0, restart_size=1.5, seed=5)
    m.set_codebook_update("ema", **kw)
    m.codebook.ema_cluster_size[::4] = 0.5                           # unused ones of these fall below restart_below, used ones do not
    old = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("codebook.")}
    x = frames(down_ratio, 2, 4)
    with torch.set_grad_enabled(grad):
        x_tilde, z_e, z_q = m(x)
    assert x_tilde.requires_grad == grad
    cb_old = old["codebook.embedding.weight"]
    ze = rows_of(z_e)
    ids = ops.vq_nearest(ze, *ops.vq_prepare(cb_old)).reshape(-1)    # the step's ids: the same kernel on the same operands
    assert same_bits(rows_of(z_q), cb_old[ids])                      # this call's z_q_x was gathered from the codebook BEFORE the update
    counts, sums = ops.code_stats(ids, ze, K=m.K)                    # fixed-order sums: the bits the step itself was fed
    stats = m.last_codebook_stats
    assert torch.equal(stats["counts"], counts) and int(counts.sum()) == ids.numel() and int(m.codebook.ema_step) == 1
    want = R.ema_update(cb_old.cpu().numpy(), old["codebook.ema_cluster_size"].cpu().numpy(), old["codebook.ema_embed_sum"].cpu().numpy(),
                        counts.cpu().numpy(), sums.cpu().numpy(), ze.cpu().numpy(), step=0, **kw)
    assert want["restarted"].any() and not want["restarted"].all()
    got = {"codebook": m.codebook.embedding.weight, "cluster_size": m.codebook.ema_cluster_size, "embed_sum": m.codebook.ema_embed_sum}
    for name, t in got.items():
        d = R.ulps(t.detach().cpu().numpy(), want[name])
        assert d.max() <= 1, (name, int(d.max()))
    for k in np.flatnonzero(want["restarted"]):
        assert same_bits(m.codebook.embedding.weight[k].detach(), ze[want["rows"][k]])
    ppl, active, restarted, total = want["stats"]
    assert abs(float(stats["perplexity"]) - ppl) <= 1e-12 * ppl and int(stats["active"]) == active and int(stats["restarted"]) == restarted
    assert all(v.is_cuda for v in stats.values())
    if grad:                                                         # the three-term loss runs as written; the codebook takes no gradient
        loss_of((x_tilde, z_e, z_q), x).backward()
        assert m.codebook.embedding.weight.grad is None and m.encoder[0].weight.grad is not None
    w_after = m.codebook.embedding.weight.detach().clone()
    m.eval()
    with torch.no_grad():
        m(x)
        m.encode(x)
    assert torch.equal(m.codebook.embedding.weight, w_after) and int(m.codebook.ema_step) == 1      # eval forward, encode: no update


# ---------------------------------------------------------------- 3. the derived caches follow the update
@pytest.mark.parametrize("down_ratio", [4, 8])
def test_eval_after_a_step_uses_the_new_codebook(down_ratio):
    m = model(down_ratio).set_codebook_update("ema", decay=0.5, restart_below=1.0)
    x = frames(down_ratio, 2, 6)
    m.eval()
    ids0 = m.encode(x)                                               # fills every cache derived from the codebook: cb, cbt, c2, the decode tables
    m.decode(ids0)
    w0 = m.codebook.embedding.weight.detach().clone()
    m.train()
    with torch.no_grad():                                            # f8: no BatchNorm buffer moves, nothing but the kernel's own write changes
        m(x)
    m.eval()
    w1 = m.codebook.embedding.weight.detach()
    assert not torch.equal(w0, w1)
    z = m._encode_features(x)
    want_ids = ops.vq_nearest(z, *ops.vq_prepare(w1.clone())).view(ids0.shape)
    got_ids = m.encode(x)
    assert torch.equal(got_ids, want_ids)
    assert not torch.equal(want_ids, ops.vq_nearest(z, *ops.vq_prepare(w0)).view(ids0.shape))       # the old codebook would answer otherwise
    fresh = build_vqvae(1 if down_ratio == 4 else 3, down_ratio, 32, 64, 99, DEV).set_codebook_update("ema")
    fresh.load_state_dict(m.state_dict())
    fresh.eval()
    assert same_bits(m.decode(got_ids), fresh.decode(got_ids))       # decode's tables were rebuilt from the new codebook
    with torch.no_grad():
        _, _, z_q = m(x)
    assert same_bits(rows_of(z_q), w1[got_ids.reshape(-1)])


# ---------------------------------------------------------------- 4. repeatable, resumable
def _run(m, down_ratio, steps, first=0):
    for i in range(first, first + steps):
        x = frames(down_ratio, 2, 20 + i)
        loss_of(m(x), x).backward()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("down_ratio", [4, 8])
def test_runs_repeat_and_resume_bit_for_bit(down_ratio):
    kw = dict(decay=0.8, restart_below=1.0, seed=9)
    a = _run(model(down_ratio).set_codebook_update("ema", **kw), down_ratio, 3)
    b = _run(model(down_ratio).set_codebook_update("ema", **kw), down_ratio, 3)
    assert int(a["codebook.ema_step"]) == 3
    for k in ["codebook.embedding.weight"] + EMA_KEYS:
        assert same_bits(a[k], b[k]), k
    half = _run(model(down_ratio).set_codebook_update("ema", **kw), down_ratio, 2)
    resumed = model(down_ratio, seed=77).set_codebook_update("ema", **kw)
    resumed.load_state_dict({k: v.cpu() for k, v in half.items()})                      # through the host, as a checkpoint file goes
    c = _run(resumed, down_ratio, 1, first=2)
    for k in ["codebook.embedding.weight"] + EMA_KEYS:
        assert same_bits(a[k], c[k]), k
    other = _run(model(down_ratio).set_codebook_update("ema", **{**kw, "seed": 10}), down_ratio, 3)
    assert not torch.equal(other["codebook.embedding.weight"], a["codebook.embedding.weight"])        # the seed chooses the restart rows


# ---------------------------------------------------------------- 5. collapse
def test_restarts_undo_a_collapse_the_gradient_rule_keeps():
    """All but 8 codes start far from anything the encoder puts out.  Under the gradient rule they never win an argmin and never move; EMA
    with restarts hands them encoder rows.  The comparison is against the gradient rule in the same test, not a fixed number."""
    held_out = frames(4, 8, 500)
    active, restarted = {}, 0
    for mode in ("grad", "ema"):
        m = model(4, seed=15)
        with torch.no_grad():
            m.codebook.embedding.weight[8:] *= 100.0
        if mode == "ema":
            m.set_codebook_update("ema", restart_below=1.0, seed=1)
        opt = FlatAdam(m.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        for step in range(20):
            x = frames(4, 8, 100 + step)
            opt.zero_grad()
            loss_of(m(x), x).backward()
            opt.step()
            if mode == "ema":
                restarted += int(m.last_codebook_stats["restarted"])
        m.eval()
        use = m.code_usage(m.encode(held_out))
        active[mode] = int(use["active"])
        print(f"collapse, {mode}: {active[mode]} of {m.K} codes active on the held-out batch (perplexity {float(use['perplexity']):.2f})")
    print(f"collapse: {restarted} restarts in 20 EMA steps")
    assert restarted > 0 and active["ema"] > active["grad"]


# ---------------------------------------------------------------- 6. code_usage and the refusals
def test_code_usage_is_bincount():
    m = model(4).eval()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 40, (3, 16, 16), generator=g).to(DEV)     # codes 40 .. 63 unused
    use = m.code_usage(ids)
    counts = torch.bincount(ids.reshape(-1), minlength=64)
    p = counts.double() / counts.sum()
    ppl = torch.exp(-(p[p > 0] * p[p > 0].log()).sum())
    assert torch.equal(use["counts"], counts) and int(use["active"]) == int((counts > 0).sum()) == 40
    assert abs(float(use["perplexity"]) - float(ppl)) <= 1e-12 * float(ppl)
    assert torch.equal(m.code_usage(m.encode(frames(4, 2, 1)))["counts"].sum(), torch.tensor(2 * 256, device=DEV))
    assert m.set_codebook_update("ema").code_usage(ids)["counts"].equal(counts)                      # in any mode
    with pytest.raises(TypeError, match="int64"):
        m.code_usage(ids.int())


def test_refusals(monkeypatch):
    import torch.distributed as dist
    m = model(4).set_codebook_update("ema")
    x = frames(4, 2, 1)
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("codebook.")}
    with weights_frozen():
        with pytest.raises(RuntimeError, match="weights_frozen"):
            m(x)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="all-reduced form is out of scope"):
        m(x)
    with pytest.raises(RuntimeError, match="all-reduced form is out of scope"):
        model(4).set_codebook_update("ema")
    monkeypatch.undo()
    torch.cuda.synchronize()
    after = m.state_dict()
    assert all(same_bits(before[k], after[k]) for k in before)       # a refused update changed nothing
    with pytest.raises(RuntimeError, match=r"set_codebook_update\('ema'"):
        model(4).load_state_dict(copy.deepcopy(m.state_dict()))
    m(x)                                                             # and the model still trains
    assert int(m.codebook.ema_step) == 1
