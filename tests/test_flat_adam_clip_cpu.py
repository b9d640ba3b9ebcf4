"""CPU side of FlatAdam(max_grad_norm=): the order of operations of the clipped step (gradients into the arena, the reduce-scatter, the sum
of squares of the shard, its all-reduce, the clipped Adam launch), single process and world size 2 over gloo.  The two HIP launches
(mage_sumsq, mage_adam_clipped) are replaced by torch-double stand-ins stating their rule, as tests/test_train_cpu.py replaces mage_adam."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_train_cpu import _adam_double, _free_port, _net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sumsq_double(self, g):
    return g.double().pow(2).sum().reshape(1)


def _adam_clipped_double(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale, sumsq, max_norm, norm_out):
    norm = sumsq.sqrt() * grad_scale                                        # fp64: the norm of the averaged gradient
    coef = (max_norm / (norm + 1e-6)).clamp(max=1.0)
    norm_out.copy_(norm.float())
    _adam_double(self, p, g, m, v, lr, b1, b2, eps, step, float(grad_scale * coef))


def _patch(cls, calls=None):
    def count(name, fn):
        def wrapped(self, *a):
            if calls is not None:
                calls.append(name)
            return fn(self, *a)
        return wrapped
    cls._adam, cls._sumsq, cls._adam_clipped = count("adam", _adam_double), count("sumsq", _sumsq_double), count("clipped", _adam_clipped_double)


@pytest.fixture
def flat_adam():
    from mage_amd.optim import FlatAdam
    saved = FlatAdam._adam, FlatAdam._sumsq, FlatAdam._adam_clipped
    yield FlatAdam
    FlatAdam._adam, FlatAdam._sumsq, FlatAdam._adam_clipped = saved


@pytest.mark.parametrize("c", [0.05, 1e3])                                   # one limit that clips at every step, one that never does
def test_clipped_step_is_clip_grad_norm_then_torch_adam(flat_adam, c):
    calls = []
    _patch(flat_adam, calls)
    a, b = _net(1), _net(1)
    ref = torch.optim.Adam(a.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
    opt = flat_adam(b.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, max_grad_norm=c)
    assert opt.param_groups[0]["max_grad_norm"] == c and opt.last_grad_norm is None
    clipped = []
    for i in range(3):
        x = torch.randn(6, 7, generator=torch.Generator().manual_seed(i))
        ref.zero_grad()
        a(x).pow(2).mean().backward()
        want_norm = torch.nn.utils.clip_grad_norm_(a.parameters(), c)
        ref.step()
        opt.zero_grad()
        b(x).pow(2).mean().backward()
        opt.step()
        assert opt.last_grad_norm.dtype == torch.float32 and opt.last_grad_norm.shape == (1,)
        assert abs(opt.last_grad_norm.item() - want_norm.item()) <= 2.0 ** -22 * want_norm.item()      # fp32 sum against fp64 sum, both rounded to fp32
        clipped.append(want_norm.item() > c)
    assert all(clipped) if c < 1 else not any(clipped)
    assert calls == ["sumsq", "clipped"] * 3
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6)


def test_without_a_limit_only_the_plain_launch_runs_and_the_limit_is_a_group_entry(flat_adam):
    calls = []
    _patch(flat_adam, calls)
    net = _net(4)
    opt = flat_adam(net.parameters(), lr=1e-2)
    assert opt.param_groups[0]["max_grad_norm"] is None
    x = torch.randn(6, 7, generator=torch.Generator().manual_seed(0))
    for _ in range(2):
        opt.zero_grad()
        net(x).pow(2).mean().backward()
        opt.step()
    assert calls == ["adam", "adam"] and opt.last_grad_norm is None
    opt.param_groups[0]["max_grad_norm"] = 0.5                              # a schedule switches it on like lr
    opt.zero_grad()
    net(x).pow(2).mean().backward()
    opt.step()
    assert calls == ["adam", "adam", "sumsq", "clipped"] and torch.isfinite(opt.last_grad_norm).all()
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            flat_adam(_net(4).parameters(), max_grad_norm=bad)


def test_clipped_step_refuses_cpu_tensors():
    from mage_amd.optim import FlatAdam
    net = _net(0)
    opt = FlatAdam(net.parameters(), lr=1e-2, max_grad_norm=1.0)
    net(torch.randn(3, 7)).sum().backward()
    with pytest.raises(RuntimeError, match="mage_sumsq"):
        opt.step()                                                          # no CPU path


def test_checkpoints_round_trip_with_torch_adam_with_and_without_the_key(flat_adam):
    _patch(flat_adam)
    a, b = _net(1), _net(1)
    ref = torch.optim.Adam(a.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
    opt = flat_adam(b.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, max_grad_norm=1e3)
    for i in range(2):
        x = torch.randn(6, 7, generator=torch.Generator().manual_seed(i))
        for net, o in ((a, ref), (b, opt)):
            o.zero_grad()
            net(x).pow(2).mean().backward()
            o.step()
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 1e3 and "max_grad_norm" not in rsd["param_groups"][0]
    opt2 = flat_adam(_net(1).parameters(), lr=1e-2)                         # the key present: it is restored ...
    opt2.load_state_dict(sd)
    assert opt2.steps == 2 and torch.equal(opt2.m, opt.m) and opt2.param_groups[0]["max_grad_norm"] == 1e3
    opt3 = flat_adam(_net(1).parameters(), lr=1e-2, max_grad_norm=0.5)      # ... absent (torch.optim.Adam's checkpoint): None
    opt3.load_state_dict(rsd)
    assert opt3.steps == 2 and torch.allclose(opt3.m, opt.m, atol=1e-7) and opt3.param_groups[0]["max_grad_norm"] is None
    t = torch.optim.Adam(_net(1).parameters(), lr=1e-2)                     # and torch.optim.Adam carries the extra key along
    t.load_state_dict(sd)
    assert torch.allclose(t.state_dict()["state"][0]["exp_avg"], rsd["state"][0]["exp_avg"], atol=1e-7)


def _worker(rank, world, port, q, c):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from mage_amd.optim import FlatAdam
    from mage_amd.utils import dist as D
    _patch(FlatAdam)
    D.init_from_env("gloo")
    net = _net(2 + 10 * rank)
    opt = FlatAdam(net.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, max_grad_norm=c)
    assert opt.sharded
    data = torch.randn(8, 7, generator=torch.Generator().manual_seed(5))
    mine = data[rank * 4:(rank + 1) * 4]
    norms = []
    for _ in range(3):
        opt.zero_grad()
        net(mine).pow(2).mean().backward()
        opt.step()
        norms.append(opt.last_grad_norm.item())
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    q.put((rank, flat.tolist(), norms))
    D.barrier()
    dist.destroy_process_group()


def test_sharded_clipped_step_over_two_ranks_clips_the_global_batch_gradient():
    c = 0.05
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, c)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]                # identical replicas, and both ranks report the same norm
    net = _net(2)
    ref = torch.optim.Adam(net.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
    data = torch.randn(8, 7, generator=torch.Generator().manual_seed(5))
    for i in range(3):
        ref.zero_grad()
        (0.5 * (net(data[:4]).pow(2).mean() + net(data[4:]).pow(2).mean())).backward()
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), c)
        assert norm.item() > c and abs(res[0][2][i] - norm.item()) <= 2.0 ** -21 * norm.item()
        ref.step()
    want = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    assert torch.allclose(torch.tensor(res[0][1]), want, atol=2e-6)
