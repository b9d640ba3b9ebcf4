"""GPU: mage_sumsq and mage_adam_clipped (include/mage_hip_ext.h) and FlatAdam(max_grad_norm=) on top of them.

Bounds.
  sumsq against math.fsum of the exact squares (fp64 products of fp32 values are exact): every term is positive, so n fp64 additions in any
    order stay within n 2^-53 of the sum, relative.
  norm_out against the fp64 norm: one fp32 rounding (the kernel's sqrt and multiply are fp64), 1 ulp.
  a clipped step against clip_grad_norm_ + torch.optim.Adam on the same fp32 tensors: tests/test_gpu_train.py's test_fused_adam_matches_torch
    allowance, 2e-6 absolute on the parameters.
  FlatAdam's first clipped step, m = (1 - b1) scale g from m = 0: the rule's scale = max_norm / (norm + 1e-6) (fp64, from the device's own
    sum of squares) is rounded once to fp32, then two fp32 products, and (1 - b1) is the kernel's fp32 difference 1 - 0.9f: 2 fp32 ulp."""
import math
import os

import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from tests.helpers import build_mage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(width=64, layers=3, vq_dim=32, K=64)                   # tests/test_gpu_policy_train.py's small model
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6)


def _offset_view(x):
    """x's values in a view one element into a 16-byte aligned buffer: a pointer that is 4-byte but not 16-byte aligned."""
    buf = torch.zeros(x.numel() + 5, device=DEV)
    v = buf[1:1 + x.numel()]
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


def _exact(x):
    return math.fsum(float(a) * float(a) for a in x.tolist())


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4097, 1048579])
def test_sumsq_is_the_exact_sum_to_fp64_rounding(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.exp(2 * torch.randn(n, generator=g))
    xd = x.to(DEV)
    want = _exact(x)
    a, b, c = ops.sumsq(xd), ops.sumsq(_offset_view(xd)), ops.sumsq(xd)
    assert a.dtype == torch.float64 and a.shape == (1,)
    assert a.view(torch.int64).item() == c.view(torch.int64).item() == b.view(torch.int64).item()      # two launches; any 4-byte alignment
    err = abs(a.item() - want) / want
    print(f"n={n}: relative error {err:.2e}, bound {n * 2.0 ** -53:.2e}")
    assert err <= n * 2.0 ** -53


@pytest.mark.parametrize("what", ["large", "subnormal"])
def test_sumsq_of_large_and_subnormal_values(what):
    n = 4097
    g = torch.Generator().manual_seed(3)
    if what == "large":
        x = (1 + torch.rand(n, generator=g)) * 1e18                # squares of 1e36: past fp32's reach of a sum of 4097, inside fp64's
    else:
        x = torch.randint(1, 2 ** 22, (n,), generator=g).to(torch.int32).view(torch.float32)          # subnormal fp32 bit patterns
        assert (x > 0).all() and (x < 1.1754944e-38).all()
    want = _exact(x)
    got = ops.sumsq(_offset_view(x.to(DEV))).item()
    assert want > 0 and math.isfinite(got) and abs(got - want) / want <= n * 2.0 ** -53


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [0.1 * torch.randn(n, generator=g) for _ in range(3)]


@pytest.mark.parametrize("n", [3, 4, 4099])
def test_adam_clipped_within_the_limit_is_adam_bit_for_bit(n):
    p0, gs = _state(n, seed=n)
    pa, ma, va = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb, mb, vb = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    norm = torch.full((1,), float("nan"), device=DEV)
    for i, g in enumerate(gs):
        gd = g.to(DEV)
        ops.adam(pa, gd, ma, va, step=i + 1, grad_scale=0.5, **ADAM)
        ss = ops.sumsq(gd)
        ops.adam_clipped(pb, gd, mb, vb, step=i + 1, grad_scale=0.5, sumsq=ss, max_norm=1e6, norm_out=norm, **ADAM)
        want = math.sqrt(_exact(g)) * 0.5
        assert abs(norm.item() - want) <= float(np.spacing(np.float32(want)))
    for a, b in ((pa, pb), (ma, mb), (va, vb)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ops.adam_clipped(pb, gs[0].to(DEV), mb, vb, step=4, sumsq=ops.sumsq(gs[0].to(DEV)), max_norm=1e6, **ADAM)       # norm_out may be null
    assert torch.isfinite(pb).all()


@pytest.mark.parametrize("n", [3, 4, 4099])
def test_adam_clipped_beyond_the_limit_is_clip_grad_norm_then_adam(n):
    p0, gs = _state(n, seed=n + 1)
    ref = torch.nn.Parameter(p0.to(DEV).clone())
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(0.9, 0.98), eps=1e-6)
    p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    norm = torch.zeros(1, device=DEV)
    for i, g in enumerate(gs):
        c = 0.5 * math.sqrt(_exact(g))                              # half this step's norm: it clips
        ref.grad = g.to(DEV).clone()
        torch.nn.utils.clip_grad_norm_([ref], c)
        opt.step()
        ops.adam_clipped(p, g.to(DEV), m, v, step=i + 1, sumsq=ops.sumsq(g.to(DEV)), max_norm=c, norm_out=norm, **ADAM)
        want = math.sqrt(_exact(g))
        assert abs(norm.item() - want) <= float(np.spacing(np.float32(want)))
    assert (p - ref.detach()).abs().max().item() < 2e-6
    assert (m - opt.state[ref]["exp_avg"]).abs().max().item() < 2e-6


def _two_models_one_gradient(seed):
    """Two identical small models and one set of policy gradients (computed once, so that both optimizers see the same bits)."""
    L = 4
    cfg = synth.mnist_model_config(frames_length=L, **SMALL)
    a, b = build_mage(cfg, seed, DEV), build_mage(cfg, seed, DEV)
    batch = {k: v.to(DEV) for k, v in synth.synth_batch_mnist(2, L, seed=seed).items()}
    R = a.image_resolution
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, a.codebook_size, (2, L - 1, R, R), generator=g).to(DEV)
    adv = torch.tensor([1.0, -0.5], device=DEV)
    a.eval()
    a.policy_loss(batch, tokens, adv)[0].backward()
    grads = [None if p.grad is None else p.grad.clone() for p in a.parameters()]
    a.zero_grad(set_to_none=True)
    return a, b, grads


def _give(model, grads):
    for p, g in zip(model.parameters(), grads):
        p.grad = None if g is None else g.clone()


def _flat_adam_checks(**kw):
    a, b, grads = _two_models_one_gradient(47)
    plain, wide = FlatAdam(a.parameters(), lr=1e-3, **kw), FlatAdam(b.parameters(), lr=1e-3, max_grad_norm=1e9, **kw)
    _give(a, grads)
    _give(b, grads)
    plain.step()
    wide.step()
    assert torch.equal(plain.flat_p.view(torch.int32), wide.flat_p.view(torch.int32))                  # far above the norm: the plain step's bits
    assert torch.equal(plain.m.view(torch.int32), wide.m.view(torch.int32)) and torch.equal(plain.v.view(torch.int32), wide.v.view(torch.int32))
    assert wide.last_grad_norm.dtype == torch.float32 and wide.last_grad_norm.shape == (1,) and plain.last_grad_norm is None
    g_flat = wide.flat_g.clone()
    ss = ops.sumsq(g_flat).item()
    norm = math.sqrt(ss)
    assert norm > 0 and abs(wide.last_grad_norm.item() - norm) <= float(np.spacing(np.float32(norm)))
    # half the measured norm: m = (1 - b1) * scale * g from m = 0
    c = build_mage(synth.mnist_model_config(frames_length=4, **SMALL), 47, DEV)
    half = FlatAdam(c.parameters(), lr=1e-3, max_grad_norm=0.5 * norm, **kw)
    _give(c, grads)
    half.step()
    assert torch.equal(half.flat_g.view(torch.int32), g_flat.view(torch.int32))
    coef = float(np.float32(0.5 * norm)) / (norm + 1e-6)            # the rule's own value: half, up to the 1e-6 in the denominator
    want = float(np.float32(1.0) - np.float32(0.9)) * coef * g_flat.double()
    ulp = torch.from_numpy(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(DEV)
    err = (half.m.double() - want).abs()
    print(f"norm {norm:.6e}; m against (1 - b1) * coef * g: worst {float((err / ulp).max()):.2f} ulp")
    assert (err <= 2 * ulp).all()
    assert abs(half.last_grad_norm.item() - norm) <= float(np.spacing(np.float32(norm)))


def test_flat_adam_clips_on_the_small_model():
    _flat_adam_checks()


def test_flat_adam_clips_through_the_collective_path():
    """One rank, backend nccl (= RCCL), shard=True: the reduce-scatter, the all-reduce of the sum of squares and the all-gather run."""
    import torch.distributed as dist
    from mage_amd.utils.dist import free_port
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        _flat_adam_checks(shard=True)
    finally:
        dist.destroy_process_group()
