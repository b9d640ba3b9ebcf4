"""CPU side of mage_adam_guarded and FlatAdam(weight_decay=, no_decay=, ema_decay=, skip_nonfinite=): the fp64 restatement of the rule
(tests/adam_guarded_ref.py) against torch.optim.AdamW; FlatAdam's bookkeeping (which launches run, the arena's layout, the skip, the
sharded step over gloo, checkpoints, refusals) with the HIP launches replaced by stand-ins that state their rule, as
tests/test_flat_adam_clip_cpu.py replaces the clipped pair; the extension table against the header; and the argument rules of the entry
point through the loaded library (nothing is launched)."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mage_amd import _lib, ops
from tests import adam_guarded_ref as R
from tests.test_flat_adam_clip_cpu import _adam_clipped_double, _sumsq_double
from tests.test_train_cpu import _adam_double, _free_port, _net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
# The two-rank test steps at FlatAdam's default lr: a step's size, and with it whatever the summation order of two half-batch gradients
# against one whole-batch gradient is magnified to where an element's second moment is tiny, scales with lr, and at 1e-2 that alone comes
# to 2.8e-6 on one element -- at the 2e-6 allowance with nothing of the optimizer in it.  Three steps of decay at 0.1 still move a decayed
# weight by 3e-4 of its size, far above the allowance.
SHARD_HYPER = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-6)
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- a. the reference against torch.optim.AdamW
def _batch(i):
    return torch.randn(6, 7, generator=torch.Generator().manual_seed(i))


def test_reference_is_torch_adamw_with_a_decayed_and_an_undecayed_group():
    wd, d = 0.1, 0.9
    net = _net(1)
    params = list(net.parameters())
    decayed = [p for p in params if p.ndim >= 2]
    rest = [p for p in params if p.ndim < 2]
    assert decayed and rest
    opt = torch.optim.AdamW([dict(params=decayed, weight_decay=wd), dict(params=rest, weight_decay=0.0)], **HYPER)
    state = [dict(p=p.detach().numpy().copy().reshape(-1), m=np.zeros(p.numel(), np.float32), v=np.zeros(p.numel(), np.float32),
                  ema=p.detach().numpy().copy().reshape(-1)) for p in params]
    ema_torch = [p.detach().double().clone() for p in params]
    mul = float(np.float32(1.0 - HYPER["lr"] * wd))
    for step in range(1, 5):
        opt.zero_grad()
        net(_batch(step)).pow(2).mean().backward()
        grads = [p.grad.detach().numpy().copy().reshape(-1) for p in params]
        opt.step()
        for s, g, p in zip(state, grads, params):
            pn, mn, vn, en, norm, skipped = R.adam_guarded(s["p"], g, s["m"], s["v"], s["ema"], n_decay=p.numel() if p.ndim >= 2 else 0,
                                                           lr=HYPER["lr"], beta1=0.9, beta2=0.98, eps=1e-6, step=step, decay_mul=mul, ema_decay=d)
            assert not skipped and norm is None
            s.update(p=pn.astype(np.float32), m=mn.astype(np.float32), v=vn.astype(np.float32), ema=en.astype(np.float32))
        for e, p in zip(ema_torch, params):
            e.mul_(d).add_(p.detach().double(), alpha=1 - d)
    for s, p, e in zip(state, params, ema_torch):
        assert np.allclose(s["p"], p.detach().numpy().reshape(-1), rtol=0, atol=1e-6)
        assert np.allclose(s["ema"], e.numpy().reshape(-1), rtol=0, atol=1e-6)
    st = opt.state_dict()["state"]
    assert np.allclose(state[0]["m"], st[0]["exp_avg"].numpy().reshape(-1), rtol=0, atol=1e-6)


def test_reference_skips_on_a_sum_of_squares_that_is_not_finite_and_clips_like_the_clipped_rule():
    g = np.array([3.0, -4.0, 0.5], np.float32)
    p, z = np.array([1.0, 2.0, 3.0], np.float32), np.zeros(3, np.float32)
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, step=1)
    for bad in (INF, NAN):
        pn, mn, vn, en, norm, skipped = R.adam_guarded(p, g, z, z, p, sumsq=bad, skip_nonfinite=True, max_norm=1.0, ema_decay=0.5, **kw)
        assert skipped and not np.isfinite(norm) and np.array_equal(pn, p) and np.array_equal(en, p) and not mn.any() and not vn.any()
    ss = float((g.astype(np.float64) ** 2).sum())
    scale, norm = R.scale_and_norm(ss, 0.5, 1.0)
    assert abs(norm - 0.5 * ss ** 0.5) < 1e-12 and abs(scale - 0.5 / (norm + 1e-6)) < 1e-7
    assert R.scale_and_norm(ss, 0.5, 1e6) == (0.5, norm) and R.scale_and_norm(ss, 0.5, 0.0) == (0.5, norm) and R.scale_and_norm(None, 0.5, 0.0) == (0.5, None)
    _, m1, _, _, _, skipped = R.adam_guarded(p, g, z, z, sumsq=ss, skip_nonfinite=True, max_norm=1.0, grad_scale=0.5, **kw)
    assert not skipped and np.allclose(m1, float(np.float32(1) - np.float32(0.9)) * scale * g.astype(np.float64), rtol=1e-14, atol=0)


# ---------------------------------------------------------------- b. FlatAdam on stand-ins
def _adam_guarded_double(self, p, g, m, v, ema, n_decay, lr, b1, b2, eps, step, grad_scale, decay_mul, ema_decay, sumsq, max_norm, skip,
                         norm_out, skipped):
    """The launch's rule in torch arithmetic on the fp32 tensors, built on the stand-ins of tests/test_train_cpu.py and
    tests/test_flat_adam_clip_cpu.py (torch.optim's own operation order: the comparisons with torch.optim.AdamW below run through a
    feedback loop -- parameters, then gradients -- that magnifies any other rounding pattern)."""
    scale = grad_scale
    if sumsq is not None:
        norm = sumsq.sqrt() * grad_scale
        if norm_out is not None:
            norm_out.copy_(norm.float())
        if skip and not torch.isfinite(sumsq).all():
            if skipped is not None:
                skipped += 1
            return                                                          # nothing is written
        if max_norm > 0:
            scale = float(grad_scale * (max_norm / (norm + 1e-6)).clamp(max=1.0))
    else:
        assert not skip and not max_norm > 0 and norm_out is None
    p[:n_decay].mul_(decay_mul)
    _adam_double(self, p, g, m, v, lr, b1, b2, eps, step, scale)
    if ema is not None:
        ema.mul_(ema_decay).add_(p, alpha=1 - ema_decay)


def test_the_stand_in_states_the_reference_rule():
    n, n_decay = 11, 5
    gen = torch.Generator().manual_seed(0)
    p, g, m, v, ema = (torch.randn(n, generator=gen) for _ in range(5))
    v = v.abs()
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.98, eps=1e-6, step=3, grad_scale=0.5, decay_mul=float(np.float32(0.999)), ema_decay=0.9)
    for max_norm in (0.0, 0.3, 1e6):
        ss = g.double().pow(2).sum().reshape(1)
        want = R.adam_guarded(p.numpy(), g.numpy(), m.numpy(), v.numpy(), ema.numpy(), n_decay=n_decay, sumsq=ss.item(), max_norm=max_norm,
                              skip_nonfinite=True, **kw)
        got = [t.clone() for t in (p, m, v, ema)]
        norm, skipped = torch.zeros(1), torch.zeros(1, dtype=torch.int64)
        _adam_guarded_double(None, got[0], g, got[1], got[2], got[3], n_decay, 1e-2, 0.9, 0.98, 1e-6, 3, 0.5, kw["decay_mul"], 0.9, ss, max_norm,
                             True, norm, skipped)
        assert skipped.item() == 0 and not want[5] and abs(norm.item() - want[4]) <= 1e-6 * want[4]
        for t, w in zip(got, want[:4]):
            assert np.allclose(t.numpy(), w, rtol=0, atol=1e-6)
        assert not torch.equal(got[0][:n_decay], p[:n_decay])
    bad = torch.tensor([NAN], dtype=torch.float64)
    got = [t.clone() for t in (p, m, v, ema)]
    _adam_guarded_double(None, got[0], g, got[1], got[2], got[3], n_decay, 1e-2, 0.9, 0.98, 1e-6, 3, 0.5, kw["decay_mul"], 0.9, bad, 1.0, True, norm, skipped)
    assert skipped.item() == 1 and torch.isnan(norm).all() and all(torch.equal(a_, b_) for a_, b_ in zip(got, (p, m, v, ema)))


_PATCHED = ("_adam", "_sumsq", "_adam_clipped", "_adam_guarded")


def _patch(cls, calls=None):
    def count(name, fn):
        def wrapped(self, *a):
            if calls is not None:
                calls.append(name)
            return fn(self, *a)
        return wrapped
    cls._adam, cls._sumsq, cls._adam_clipped = count("adam", _adam_double), count("sumsq", _sumsq_double), count("clipped", _adam_clipped_double)
    cls._adam_guarded = count("guarded", _adam_guarded_double)


@pytest.fixture
def flat_adam():
    from mage_amd.optim import FlatAdam
    saved = [getattr(FlatAdam, k) for k in _PATCHED]
    yield FlatAdam
    for k, fn in zip(_PATCHED, saved):
        setattr(FlatAdam, k, fn)


def _one_step(net, opt, i=0, poison=None):
    opt.zero_grad()
    net(_batch(i)).pow(2).mean().backward()
    if poison is not None:
        list(net.parameters())[-1].grad.view(-1)[0] = poison
    opt.step()


@pytest.mark.parametrize("kw,want", [
    (dict(), ["adam"]),
    (dict(max_grad_norm=1.0), ["sumsq", "clipped"]),
    (dict(weight_decay=0.1), ["guarded"]),
    (dict(weight_decay=0.0), ["guarded"]),                                   # 0.0 counts as a number
    (dict(ema_decay=0.9), ["guarded"]),
    (dict(skip_nonfinite=True), ["sumsq", "guarded"]),
    (dict(weight_decay=0.1, max_grad_norm=1.0), ["sumsq", "guarded"]),
    (dict(ema_decay=0.9, max_grad_norm=1.0), ["sumsq", "guarded"]),
    (dict(weight_decay=0.1, ema_decay=0.9, skip_nonfinite=True, max_grad_norm=1.0), ["sumsq", "guarded"]),
])
def test_which_launches_a_step_makes(flat_adam, kw, want):
    calls = []
    _patch(flat_adam, calls)
    net = _net(4)
    opt = flat_adam(net.parameters(), **HYPER, **kw)
    g0 = opt.param_groups[0]
    assert g0["weight_decay"] == kw.get("weight_decay") and g0["ema_decay"] == kw.get("ema_decay") and g0["skip_nonfinite"] is bool(kw.get("skip_nonfinite"))
    for i in range(2):
        _one_step(net, opt, i)
    assert calls == want * 2
    assert (opt.ema is not None) == ("ema_decay" in kw) and (opt.skipped_steps is not None) == ("skip_nonfinite" in kw)
    assert (opt.last_grad_norm is not None) == ("sumsq" in want)


def test_defaults_keep_the_callers_order_and_weight_decay_puts_the_decayed_parameters_first(flat_adam):
    _patch(flat_adam)
    net = _net(4)
    plain = flat_adam(net.parameters(), **HYPER)
    sizes = [p.numel() for p in plain.params]
    assert plain.offsets == [sum(sizes[:j]) for j in range(len(sizes))] and plain.n_decay == 0
    net = _net(4)
    before = [p.detach().clone() for p in net.parameters()]
    params = list(net.parameters())
    opt = flat_adam(net.parameters(), weight_decay=0.1, no_decay=[params[2]], **HYPER)     # the second Linear's weight is exempt
    decayed = [j for j, p in enumerate(params) if p.ndim >= 2 and j != 2]
    rest = [j for j in range(len(params)) if j not in decayed]
    assert decayed == [0] and opt.n_decay == params[0].numel()
    assert [opt.params[j] is params[j] for j in range(len(params))] == [True] * len(params)                     # caller order kept
    assert sorted(opt.offsets[j] for j in decayed) == [0] and all(opt.offsets[j] >= opt.n_decay for j in rest)
    spans = sorted((opt.offsets[j], opt.offsets[j] + params[j].numel()) for j in range(len(params)))
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == opt.n
    for j, (p, b) in enumerate(zip(params, before)):                                                           # offsets still address each parameter
        assert torch.equal(p, b) and p.data_ptr() == opt.flat_p.data_ptr() + 4 * opt.offsets[j]
        assert torch.equal(opt.flat_p[opt.offsets[j]:opt.offsets[j] + p.numel()].view(p.shape), b)
    full = flat_adam(_net(4).parameters(), weight_decay=0.1, **HYPER)
    assert full.n_decay == sizes[0] + sizes[2] and full.offsets[0] == 0 and full.offsets[2] == sizes[0] and full.offsets[1] == sizes[0] + sizes[2]


def test_flat_adam_with_weight_decay_and_ema_is_torch_adamw(flat_adam):
    _patch(flat_adam)
    wd, d = 0.1, 0.9
    a, b = _net(1), _net(1)
    pa = list(a.parameters())
    ref = torch.optim.AdamW([dict(params=[pa[0]], weight_decay=wd), dict(params=[pa[2]] + [p for p in pa if p.ndim < 2], weight_decay=0.0)], **HYPER)
    opt = flat_adam(b.parameters(), weight_decay=wd, no_decay=[list(b.parameters())[2]], ema_decay=d, **HYPER)
    ema = [p.detach().double().clone() for p in pa]
    for i in range(3):
        ref.zero_grad()
        a(_batch(i)).pow(2).mean().backward()
        ref.step()
        _one_step(b, opt, i)
        for e, p in zip(ema, pa):
            e.mul_(d).add_(p.detach().double(), alpha=1 - d)
    for x, y, e, t in zip(pa, b.parameters(), ema, opt.ema_tensors()):
        assert torch.allclose(x, y, atol=1e-6) and torch.allclose(t.double(), e, atol=1e-6) and t.shape == x.shape
    sd = opt.state_dict()
    assert torch.allclose(sd["state"][0]["exp_avg"], ref.state_dict()["state"][0]["exp_avg"], atol=1e-6)
    assert all(torch.equal(sd["state"][j]["ema"], t) for j, t in enumerate(opt.ema_tensors()))


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_a_step_with_a_gradient_that_is_not_finite_is_skipped_and_the_next_proceeds(flat_adam, bad):
    _patch(flat_adam)
    net = _net(4)
    opt = flat_adam(net.parameters(), weight_decay=0.1, ema_decay=0.9, skip_nonfinite=True, max_grad_norm=1.0, **HYPER)
    _one_step(net, opt, 0)
    assert opt.skipped_steps.item() == 0 and np.isfinite(opt.last_grad_norm.item())
    kept = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.ema)]
    _one_step(net, opt, 1, poison=bad)
    assert opt.skipped_steps.item() == 1 and not np.isfinite(opt.last_grad_norm.item()) and opt.steps == 2      # the call counts as a step
    for t, k in zip((opt.flat_p, opt.m, opt.v, opt.ema), kept):
        assert torch.equal(t, k)
    _one_step(net, opt, 2)
    assert opt.skipped_steps.item() == 1 and opt.steps == 3 and np.isfinite(opt.last_grad_norm.item())
    for t, k in zip((opt.flat_p, opt.m, opt.v, opt.ema), kept):
        assert not torch.equal(t, k) and torch.isfinite(t).all()


def test_swap_ema_runs_the_model_on_the_average_and_restores_the_raw_weights(flat_adam):
    from mage_amd.modules import vqvae_model as _vq
    _patch(flat_adam)
    net = _net(4)
    opt = flat_adam(net.parameters(), ema_decay=0.5, **HYPER)
    for i in range(2):
        _one_step(net, opt, i)
    raw = [p.detach().clone() for p in net.parameters()]
    x = _batch(9)
    y_raw = net(x).detach().clone()
    epoch = _vq._WEIGHTS_EPOCH
    with opt.swap_ema() as o:
        assert o is opt
        for p, e, r in zip(net.parameters(), opt.ema_tensors(), raw):
            assert torch.equal(p, e) and not torch.equal(p, r)
        assert not torch.equal(net(x), y_raw)
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step()
        with pytest.raises(RuntimeError, match="swap_ema"):
            with opt.swap_ema():
                pass
    for p, r in zip(net.parameters(), raw):
        assert torch.equal(p, r)
    assert torch.equal(net(x), y_raw)
    assert _vq._WEIGHTS_EPOCH == epoch + 2                                  # bumped on entry and on exit
    _one_step(net, opt, 3)                                                  # and training goes on


# ---------------------------------------------------------------- c. world 2 over gloo
def _worker(rank, world, port, q, exempt_second_weight):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from mage_amd.optim import FlatAdam
    from mage_amd.utils import dist as D
    _patch(FlatAdam)
    D.init_from_env("gloo")
    net = _net(2 + 10 * rank)
    params = list(net.parameters())
    opt = FlatAdam(params, weight_decay=0.1, no_decay=[params[2]] if exempt_second_weight else None, ema_decay=0.9, skip_nonfinite=True,
                   max_grad_norm=0.05, **SHARD_HYPER)
    assert opt.sharded and opt.ema.numel() == opt.shard_n
    lo, hi = opt.shard_n * (0 if exempt_second_weight else 1), opt.shard_n * (1 if exempt_second_weight else 2)
    assert lo < opt.n_decay < hi                                            # the boundary lies strictly inside one rank's shard
    data = torch.randn(8, 7, generator=torch.Generator().manual_seed(5))
    mine = data[rank * 4:(rank + 1) * 4]
    for _ in range(3):
        opt.zero_grad()
        net(mine).pow(2).mean().backward()
        opt.step()
    flat = torch.cat([p.detach().reshape(-1) for p in params])
    opt.consolidate_state_dict(to=0)
    ema = []
    if rank == 0:
        sd = opt.state_dict()
        ema = torch.cat([sd["state"][i]["ema"].reshape(-1) for i in range(len(params))]).tolist()
    with opt.swap_ema():                                                    # collective: the gathered average in every replica
        swapped = torch.cat([p.detach().reshape(-1) for p in params]).tolist()
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in params]), flat)
    # a NaN in rank 1's gradient only, at an element of rank 1's own shard: rank 0 learns of it through the all-reduced sum of squares alone
    kept = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.ema)]
    opt.zero_grad()
    net(mine).pow(2).mean().backward()
    if rank == 1:
        assert opt.offsets[-1] >= opt.shard_n
        params[-1].grad.view(-1)[0] = NAN
    opt.step()
    untouched = all(torch.equal(t, k) for t, k in zip((opt.flat_p, opt.m, opt.v, opt.ema), kept))
    q.put((rank, flat.tolist(), ema, swapped, untouched, int(opt.skipped_steps.item()), opt.n_decay))
    D.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("exempt_second_weight", [False, True])            # n_decay inside rank 1's shard, inside rank 0's
def test_sharded_guarded_step_over_two_ranks_is_single_process_adamw(exempt_second_weight):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, exempt_second_weight)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1] and res[0][3] == res[1][3]               # identical replicas, raw and inside swap_ema
    assert res[0][4] and res[1][4] and res[0][5] == res[1][5] == 1          # both ranks skipped the step poisoned on rank 1
    net = _net(2)
    params = list(net.parameters())
    exempt = [params[2]] if exempt_second_weight else []
    decayed = [p for p in params if p.ndim >= 2 and not any(p is e for e in exempt)]
    assert res[0][6] == sum(p.numel() for p in decayed)
    ref = torch.optim.AdamW([dict(params=decayed, weight_decay=0.1), dict(params=[p for p in params if not any(p is e for e in decayed)],
                                                                            weight_decay=0.0)], **SHARD_HYPER)
    data = torch.randn(8, 7, generator=torch.Generator().manual_seed(5))
    ema = [p.detach().double().clone() for p in params]
    for _ in range(3):
        ref.zero_grad()
        (0.5 * (net(data[:4]).pow(2).mean() + net(data[4:]).pow(2).mean())).backward()
        assert torch.nn.utils.clip_grad_norm_(params, 0.05).item() > 0.05
        ref.step()
        for e, p in zip(ema, params):
            e.mul_(0.9).add_(p.detach().double(), alpha=1 - 0.9)
    want = torch.cat([p.detach().reshape(-1) for p in params])
    assert torch.allclose(torch.tensor(res[0][1]), want, atol=2e-6)         # the sharded clip test's allowance
    want_ema = torch.cat([e.reshape(-1) for e in ema])
    # a convex combination of parameters that are each within 2e-6 stays within 2e-6
    assert res[1][2] == [] and torch.allclose(torch.tensor(res[0][2], dtype=torch.float64), want_ema, atol=2e-6)
    assert torch.allclose(torch.tensor(res[0][3], dtype=torch.float64), want_ema, atol=2e-6)


# ---------------------------------------------------------------- d. checkpoints
def test_checkpoints_round_trip_the_ema_the_moments_and_the_group_keys(flat_adam):
    _patch(flat_adam)
    kw = dict(weight_decay=0.1, ema_decay=0.9, skip_nonfinite=True)
    net = _net(1)
    opt = flat_adam(net.parameters(), **HYPER, **kw)
    for i in range(2):
        _one_step(net, opt, i)
    sd = opt.state_dict()
    g0 = sd["param_groups"][0]
    assert g0["weight_decay"] == 0.1 and g0["ema_decay"] == 0.9 and g0["skip_nonfinite"] is True
    assert not torch.equal(sd["state"][0]["ema"], list(net.parameters())[0])
    opt2 = flat_adam(_net(7).parameters(), lr=1e-2, weight_decay=0.0, ema_decay=0.5)        # other values, a differently initialised net
    opt2.load_state_dict(sd)
    assert opt2.steps == 2 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and torch.equal(opt2.ema, opt.ema)
    assert {k: opt2.param_groups[0][k] for k in kw} == kw
    # torch.optim.Adam loads the same dict and carries the 'ema' entries along
    t = torch.optim.Adam(_net(1).parameters(), lr=1e-2)
    t.load_state_dict(sd)
    assert torch.equal(t.state_dict()["state"][0]["ema"], sd["state"][0]["ema"])
    # a checkpoint without the keys and without 'ema' (torch.optim.Adam's own: its weight_decay is the L2 term): the constructor's values
    # stay and the EMA starts again from the current parameters
    a = _net(1)
    ref = torch.optim.Adam(a.parameters(), **HYPER)
    for i in range(2):
        ref.zero_grad()
        a(_batch(i)).pow(2).mean().backward()
        ref.step()
    rsd = ref.state_dict()
    assert rsd["param_groups"][0]["weight_decay"] == 0 and "ema_decay" not in rsd["param_groups"][0]
    net3 = _net(7)
    opt3 = flat_adam(net3.parameters(), lr=1e-2, ema_decay=0.5, skip_nonfinite=True)
    opt3.ema.zero_()
    opt3.load_state_dict(rsd)
    g3 = opt3.param_groups[0]
    assert opt3.steps == 2 and g3["weight_decay"] is None and g3["ema_decay"] == 0.5 and g3["skip_nonfinite"] is True
    assert torch.equal(opt3.ema, opt3.flat_p) and all(torch.equal(e, p) for e, p in zip(opt3.ema_tensors(), net3.parameters()))
    _one_step(net3, opt3, 0)                                                # weight_decay None survived the load: the step is not refused
    # an optimizer without an EMA ignores the entries; one built without the decay layout refuses a checkpoint that decays
    opt4 = flat_adam(_net(1).parameters(), lr=1e-2, weight_decay=0.3)
    opt4.load_state_dict(sd)
    assert opt4.ema is None and opt4.param_groups[0]["ema_decay"] is None and opt4.param_groups[0]["weight_decay"] == 0.1
    with pytest.raises(ValueError, match="weight_decay"):
        flat_adam(_net(1).parameters(), lr=1e-2).load_state_dict(sd)


# ---------------------------------------------------------------- e. refusals
def test_constructor_and_group_refusals(flat_adam):
    _patch(flat_adam)
    for bad in (-0.1, NAN, INF, "0.1", True, 100.0):                        # 100.0: lr * weight_decay = 1
        with pytest.raises(ValueError, match="weight_decay"):
            flat_adam(_net(4).parameters(), lr=1e-2, weight_decay=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, NAN, "0.9", True):
        with pytest.raises(ValueError, match="ema_decay"):
            flat_adam(_net(4).parameters(), lr=1e-2, ema_decay=bad)
    net = _net(4)
    with pytest.raises(ValueError, match="no_decay"):
        flat_adam(net.parameters(), lr=1e-2, no_decay=[list(net.parameters())[0]])                   # without weight_decay
    with pytest.raises(ValueError, match="no_decay"):
        flat_adam(net.parameters(), lr=1e-2, weight_decay=0.1, no_decay=[torch.nn.Parameter(torch.zeros(2, 2))])
    frozen = _net(4)
    list(frozen.parameters())[0].requires_grad_(False)
    with pytest.raises(ValueError, match="no_decay"):
        flat_adam(frozen.parameters(), lr=1e-2, weight_decay=0.1, no_decay=[list(frozen.parameters())[0]])
    opt = flat_adam(net.parameters(), lr=1e-2)
    with pytest.raises(RuntimeError, match="EMA"):
        with opt.swap_ema():
            pass
    with pytest.raises(RuntimeError, match="EMA"):
        opt.ema_tensors()
    _one_step(net, opt, 0)
    opt.param_groups[0]["weight_decay"] = 0.1                               # the layout was fixed at construction
    with pytest.raises(ValueError, match="weight_decay"):
        _one_step(net, opt, 1)
    opt.param_groups[0]["weight_decay"] = None
    opt.param_groups[0]["ema_decay"] = 0.9                                  # and so was the buffer
    with pytest.raises(ValueError, match="ema_decay"):
        _one_step(net, opt, 1)
    net = _net(4)
    opt = flat_adam(net.parameters(), lr=1e-2, weight_decay=0.0)
    opt.param_groups[0]["weight_decay"] = 0.2                               # a schedule changes the value
    _one_step(net, opt, 0)
    opt.param_groups[0]["weight_decay"] = 200.0
    with pytest.raises(ValueError, match="weight_decay"):
        _one_step(net, opt, 1)


@pytest.mark.parametrize("kw,entry", [(dict(ema_decay=0.9), "mage_adam_guarded"), (dict(weight_decay=0.1), "mage_adam_guarded"),
                                      (dict(skip_nonfinite=True), "mage_sumsq")])
def test_guarded_step_refuses_cpu_tensors(kw, entry):
    from mage_amd.optim import FlatAdam
    net = _net(0)
    opt = FlatAdam(net.parameters(), lr=1e-2, **kw)
    net(torch.randn(3, 7)).sum().backward()
    with pytest.raises(RuntimeError, match=entry):
        opt.step()                                                          # no CPU path
    with pytest.raises(RuntimeError, match="mage_adam_guarded"):
        opt._adam_guarded(opt.flat_p, opt.flat_g, opt.m, opt.v, None, 0, 1e-2, 0.9, 0.98, 1e-6, 1, 1.0, 1.0, 0.0, None, 0.0, False, None, None)


# ---------------------------------------------------------------- f. the extension table and the argument rules
ORDER = ["p", "g", "m", "v", "ema", "n", "n_decay", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "decay_mul", "ema_decay", "sumsq",
         "max_norm", "skip_nonfinite", "norm_out", "skipped", "stream"]


def test_the_header_declares_what_the_table_binds():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    name = "mage_adam_guarded"
    assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES and len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M | re.S).group(1)
    C = {"const float*": _lib.C.c_void_p, "float*": _lib.C.c_void_p, "const double*": _lib.C.c_void_p, "int64_t*": _lib.C.c_void_p,
         "void*": _lib.C.c_void_p, "int64_t": _lib.C.c_int64, "int32_t": _lib.C.c_int32, "float": _lib.C.c_float}
    declared = [C[a.strip().rsplit(" ", 1)[0]] for a in decl.split(",")]
    assert [a.strip().rsplit(" ", 1)[1] for a in decl.split(",")] == ORDER
    res, args = _lib.EXT_SIGNATURES[name]
    assert res is _lib.C.c_int and args == declared
    fn = getattr(_lib.load(), name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert "adam_guarded" in ops.__all__ and callable(ops.adam_guarded)
    assert "there is no skip-step guard" not in header and "mage_adam_guarded" in header.split("int mage_sumsq")[0]


P = 0x7F0000001000                                                          # a fake, 16-byte aligned address: every call below is refused
GOOD = dict(p=P, g=P + 0x1000, m=P + 0x2000, v=P + 0x3000, ema=P + 0x4000, n=100, n_decay=50, lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, step=1,
            grad_scale=1.0, decay_mul=0.999, ema_decay=0.9, sumsq=P + 0x5000, max_norm=1.0, skip_nonfinite=1, norm_out=P + 0x5008,
            skipped=P + 0x5010, stream=None)


@pytest.mark.parametrize("bad", [
    dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-4), dict(step=0), dict(step=-1),
    dict(p=P + 4), dict(g=P + 8), dict(m=P + 0x2004), dict(v=P + 0x300c), dict(ema=P + 0x4004), dict(ema=P + 0x4008),
    dict(n_decay=-1), dict(n_decay=101), dict(n_decay=2 ** 40),
    dict(decay_mul=0.0), dict(decay_mul=-0.5), dict(decay_mul=1.0000001), dict(decay_mul=NAN), dict(decay_mul=INF), dict(decay_mul=-INF),
    dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=1.5), dict(ema_decay=NAN), dict(ema_decay=INF),
    dict(max_norm=-1.0), dict(max_norm=NAN), dict(max_norm=INF), dict(max_norm=-INF),
    dict(sumsq=None), dict(sumsq=None, max_norm=0.0), dict(sumsq=None, skip_nonfinite=0), dict(sumsq=P + 0x5004),
    dict(sumsq=P + 0x5004, max_norm=0.0, skip_nonfinite=0),
    dict(skipped=P + 0x5014), dict(norm_out=P + 0x500a), dict(norm_out=P + 0x5009),
])
def test_adam_guarded_refuses_bad_arguments(bad):
    a = {**GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_adam_guarded(*[a[k] for k in ORDER])
    assert rc == -1 and "mage_adam_guarded" in lib.mage_last_error().decode(), (bad, rc)
