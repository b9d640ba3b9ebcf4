"""GPU: mage_adam_guarded (include/mage_hip_ext.h) and FlatAdam(skip_nonfinite=, ema_decay=) on top of it.

Bounds.
  p, m, v with ema null and n_decay 0 against mage_adam / mage_adam_clipped on twin buffers: bit equality (the update is the same device
    function and the scale the same operations).
  The decay against the fp64 rule (tests/adam_guarded_ref.py): tests/test_gpu_train.py's test_fused_adam_matches_torch allowance, 2e-6
    absolute on the parameters.  The parameters are at least 0.5 in magnitude and decay_mul is 0.9, so a decayed and an undecayed element
    differ by at least 0.05: the allowance separates the two sides of the boundary by four orders of magnitude.
  The EMA against the fp64 rule d * ema_old + (1 - d) * p_new, with d and 1 - d the kernel's fp32 values and p_new the kernel's own stored
    fp32 value (so nothing of the Adam update enters): the kernel rounds twice, t = fl((1 - d) * p_new) and ema = fl(d * ema_old + t), the
    second a fused multiply-add.  With M = max(|ema_old|, |p_new|): |t| <= M, so the first rounding is at most 1/2 ulp(M); the result is at
    most (d + (1 - d)) M <= (1 + 2^-24) M in magnitude, so the second is at most 1/2 ulp of a value that is M up to one rounding, i.e. at
    most 1 ulp(M) where the result crosses into the next binade.  Together below 2 fp32 ulp of M, the bound used."""
import math

import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from tests import adam_guarded_ref as R
from tests.helpers import bits, build_mage, refused, sent
from tests.test_gpu_policy_train import SMALL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6)
SIZES = [3, 4, 4099]                                                # the tail only; one full vector; several workgroups and a 3-element tail


def _state(n, seed):
    """p (|p| >= 0.5), three gradients, m, v (> 0) and an EMA: finite, on the device."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    p = torch.where(p < 0, p - 0.5, p + 0.5)
    gs = [(0.1 * torch.randn(n, generator=g)).to(DEV) for _ in range(3)]
    m, v, ema = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g) + 1e-4, torch.randn(n, generator=g)
    return p.to(DEV), gs, m.to(DEV), v.to(DEV), ema.to(DEV)


def _same_bits(*pairs):
    return all(torch.equal(bits(a), bits(b)) for a, b in pairs)


# ---------------------------------------------------------------- 1. the existing kernels' bits
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("mode", ["inside", "above", "noclip"])
@pytest.mark.parametrize("n", SIZES)
def test_without_ema_and_decay_the_bits_are_the_existing_kernels(n, mode, skip):
    p0, gs, m0, v0, _ = _state(n, seed=n)
    pa, ma, va, pb, mb, vb = (t.clone() for t in (p0, m0, v0, p0, m0, v0))
    norm_a, norm_b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
    for i, g in enumerate(gs):
        ss = ops.sumsq(g)
        c = {"inside": 1e6, "above": 0.25 * math.sqrt(ss.item()), "noclip": 0.0}[mode]       # grad_scale 0.5: the norm is twice the limit
        if mode == "noclip":
            ops.adam(pa, g, ma, va, step=i + 1, grad_scale=0.5, **ADAM)
        else:
            ops.adam_clipped(pa, g, ma, va, step=i + 1, grad_scale=0.5, sumsq=ss, max_norm=c, norm_out=norm_a, **ADAM)
        give = mode != "noclip" or skip                             # max_norm == 0 and no guard: the call mage_adam's arguments describe
        ops.adam_guarded(pb, g, mb, vb, step=i + 1, grad_scale=0.5, sumsq=ss if give else None, max_norm=c, skip_nonfinite=skip,
                         norm_out=norm_b if give else None, skipped=skipped if skip else None, **ADAM)
        assert _same_bits((pa, pb), (ma, mb), (va, vb)), (n, mode, skip, i)
        if mode != "noclip":
            assert _same_bits((norm_a, norm_b))
    assert skipped.item() == 0 and torch.isfinite(pb).all() and not torch.equal(pb, p0)


# ---------------------------------------------------------------- 2. the decay boundary
@pytest.mark.parametrize("n", SIZES)
def test_decay_reaches_exactly_the_elements_below_the_boundary(n):
    mul = float(np.float32(0.9))
    p0, gs, m0, v0, _ = _state(n, seed=n + 10)
    g = gs[0]
    kw = dict(step=2, grad_scale=0.5, **ADAM)
    host = [t.cpu().numpy() for t in (p0, g, m0, v0)]
    with_decay = R.adam_guarded(*host, n_decay=n, decay_mul=mul, **kw)[0]
    without = R.adam_guarded(*host, n_decay=0, **kw)[0]
    assert np.abs(with_decay - without).min() > 0.04                # the two rules are far apart at every element
    plain = [t.clone() for t in (p0, m0, v0)]
    ops.adam_guarded(plain[0], g, plain[1], plain[2], n_decay=0, **kw)
    assert np.abs(plain[0].double().cpu().numpy() - without).max() < 2e-6
    for n_decay in sorted({min(max(k, 0), n) for k in (0, 1, 2, 5, n - 1, n)}):
        p, m, v = (t.clone() for t in (p0, m0, v0))
        ops.adam_guarded(p, g, m, v, n_decay=n_decay, decay_mul=mul, **kw)
        got = p.double().cpu().numpy()
        want = np.where(np.arange(n) < n_decay, with_decay, without)
        err = np.abs(got - want).max()
        print(f"n={n} n_decay={n_decay}: worst |p - fp64 rule| {err:.2e} (allowed 2e-6)")
        assert err < 2e-6, (n, n_decay)
        assert _same_bits((p[n_decay:], plain[0][n_decay:]), (m, plain[1]), (v, plain[2])), (n, n_decay)      # at and above: the undecayed run's bits
    p, m, v = (t.clone() for t in (p0, m0, v0))                     # decay_mul 1: the decay instance with nothing to do
    ops.adam_guarded(p, g, m, v, n_decay=n, decay_mul=1.0, **kw)
    assert _same_bits((p, plain[0]))


# ---------------------------------------------------------------- 3. the EMA
@pytest.mark.parametrize("n_decay_on", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_ema_follows_the_kernels_own_parameters_within_two_ulp(n, n_decay_on):
    d = 0.9
    p, gs, m, v, ema = _state(n, seed=n + 20)
    twin = [t.clone() for t in (p, m, v)]
    worst = 0.0
    for i, g in enumerate(gs):
        old = ema.double().cpu().numpy()
        ops.adam_guarded(p, g, m, v, ema=ema, ema_decay=d, n_decay=n // 2 if n_decay_on else 0, decay_mul=0.99, step=i + 1, **ADAM)
        ops.adam_guarded(twin[0], g, twin[1], twin[2], n_decay=n // 2 if n_decay_on else 0, decay_mul=0.99, step=i + 1, **ADAM)
        assert _same_bits((p, twin[0]), (m, twin[1]), (v, twin[2]))          # the EMA changes nothing else
        new = p.double().cpu().numpy()
        want = R.ema_rule(old, new, d)
        ulp = np.spacing(np.maximum(np.abs(old), np.abs(new)).astype(np.float32)).astype(np.float64)
        ratio = np.abs(ema.double().cpu().numpy() - want) / ulp
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 2).all(), (n, i, float(ratio.max()))
    print(f"n={n}: EMA against the fp64 rule, worst {worst:.3f} ulp of max(|ema_old|, |p_new|) (allowed 2)")
    assert not torch.equal(ema, p)


# ---------------------------------------------------------------- 4. the skip
def _random_bits(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("n", SIZES)
def test_a_gradient_that_is_not_finite_skips_the_step_and_touches_nothing(n, bad):
    _, gs, _, _, _ = _state(n, seed=n + 30)
    for at in sorted({0, n - 1} | ({2048} if n > 2048 else set())):
        g = gs[0].clone()
        g[at] = bad
        ss = ops.sumsq(g)
        assert not math.isfinite(ss.item())
        bufs = [_random_bits(n, seed=100 * n + 4 * at + k) for k in range(4)]                 # p, m, v, ema: any rewrite would show
        p, m, v, ema = (t.clone() for t in bufs)
        skipped, norm = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, device=DEV)
        ops.adam_guarded(p, g, m, v, ema=ema, ema_decay=0.9, n_decay=n, decay_mul=0.99, step=1, sumsq=ss, max_norm=1.0, skip_nonfinite=True,
                         norm_out=norm, skipped=skipped, **ADAM)
        assert _same_bits(*zip((p, m, v, ema), bufs)), (n, bad, at)
        assert skipped.item() == 1 and not math.isfinite(norm.item())
        # the contrast, today's behaviour: without the guard the same gradient poisons the parameters
        q, gs_, qm, qv, _ = _state(n, seed=n + 31)
        ops.adam_guarded(q, g, qm, qv, step=1, sumsq=ss, max_norm=1.0, skip_nonfinite=False, **ADAM)
        assert not torch.isfinite(q).all(), (n, bad, at)
        # the next, finite step: a twin that never saw the skipped call, at the same step number
        twin = [t.clone() for t in bufs]
        ss2 = ops.sumsq(gs[1])
        for b_, sk in ((p, m, v, ema), skipped), (twin, None):
            ops.adam_guarded(b_[0], gs[1], b_[1], b_[2], ema=b_[3], ema_decay=0.9, n_decay=n, decay_mul=0.99, step=2, sumsq=ss2, max_norm=1.0,
                             skip_nonfinite=True, norm_out=norm, skipped=sk, **ADAM)
        assert _same_bits(*zip((p, m, v, ema), twin)) and not _same_bits((p, bufs[0])) and skipped.item() == 1
        assert math.isfinite(norm.item())


def test_the_skip_on_finite_buffers_is_followed_by_the_same_step_as_a_twins():
    """As above with ordinary values, where the follow-up step's result is finite and can be compared with the fp64 rule too."""
    n = 4099
    p0, gs, m0, v0, e0 = _state(n, seed=77)
    a, b = [t.clone() for t in (p0, m0, v0, e0)], [t.clone() for t in (p0, m0, v0, e0)]
    g = gs[0].clone()
    g[2048] = float("nan")
    skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(ema_decay=0.9, n_decay=1000, decay_mul=float(np.float32(0.99)), max_norm=0.0, skip_nonfinite=True, **ADAM)
    ops.adam_guarded(a[0], g, a[1], a[2], ema=a[3], step=1, sumsq=ops.sumsq(g), skipped=skipped, **kw)
    assert _same_bits(*zip(a, (p0, m0, v0, e0))) and skipped.item() == 1
    ss = ops.sumsq(gs[1])
    for t in (a, b):
        ops.adam_guarded(t[0], gs[1], t[1], t[2], ema=t[3], step=2, sumsq=ss, skipped=skipped, **kw)
    assert _same_bits(*zip(a, b)) and skipped.item() == 1 and all(torch.isfinite(t).all() for t in a)
    want = R.adam_guarded(*(t.cpu().numpy() for t in (p0, gs[1], m0, v0, e0)), n_decay=1000, decay_mul=kw["decay_mul"], ema_decay=0.9, step=2,
                          sumsq=ss.item(), skip_nonfinite=True, **ADAM)
    assert np.abs(a[0].double().cpu().numpy() - want[0]).max() < 2e-6 and np.abs(a[3].double().cpu().numpy() - want[3]).max() < 2e-6


# ---------------------------------------------------------------- 5. refusals
def test_refused_calls_write_nothing():
    n = 4099
    g = torch.zeros(n, device=DEV)
    ss = torch.ones(1, dtype=torch.float64, device=DEV)
    p, m, v, ema = (sent(n, torch.float32) for _ in range(4))
    norm = sent(1, torch.float32)
    skipped = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    good = dict(ema=ema, ema_decay=0.9, n_decay=100, decay_mul=0.99, step=1, sumsq=ss, max_norm=1.0, skip_nonfinite=True, norm_out=norm,
                skipped=skipped, **ADAM)
    for bad in (dict(n_decay=-1), dict(n_decay=n + 1), dict(decay_mul=0.0), dict(decay_mul=1.5), dict(decay_mul=float("nan")),
                dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=float("nan")), dict(max_norm=-1.0), dict(max_norm=float("inf")),
                dict(max_norm=float("nan")), dict(sumsq=None), dict(sumsq=None, max_norm=0.0), dict(sumsq=None, skip_nonfinite=False),
                dict(step=0)):
        refused(lambda: ops.adam_guarded(p, g, m, v, **{**good, **bad}), p, m, v, ema, norm)
        assert skipped.item() == -7, bad
    big = [sent(n + 4, torch.float32) for _ in range(4)]                    # arenas one element off a 16-byte boundary
    for k in range(4):
        args = [b_[1:n + 1] if j == k else b_[:n] for j, b_ in enumerate(big)]
        assert args[k].data_ptr() % 16 == 4
        refused(lambda: ops.adam_guarded(args[0], g, args[1], args[2], **{**good, "ema": args[3]}), *big, norm)
    refused(lambda: ops.adam_guarded(p, torch.zeros(n + 4, device=DEV)[1:n + 1], m, v, **good), p, m, v, ema, norm)
    assert skipped.item() == -7


# ---------------------------------------------------------------- 6. end to end on the small model
def _tokens(model, batch):
    model.autoregressive_generate(batch)
    return model.last_tokens.clone()


def test_flat_adam_skips_a_poisoned_step_and_swaps_in_the_averaged_weights():
    L, seed = 4, 53
    cfg = synth.mnist_model_config(frames_length=L, **SMALL)
    m = build_mage(cfg, seed, DEV)
    batch = {k: v.to(DEV) for k, v in synth.synth_batch_mnist(2, L, seed=seed).items()}
    R_ = m.image_resolution
    tokens = torch.randint(0, m.codebook_size, (2, L - 1, R_, R_), generator=torch.Generator().manual_seed(seed)).to(DEV)
    opt = FlatAdam(m.parameters(), lr=1e-2, skip_nonfinite=True, max_grad_norm=1.0, ema_decay=0.9)
    assert opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.shape == (1,) and opt.ema.shape == (opt.shard_n,)
    before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.ema)]
    assert torch.equal(opt.ema, opt.flat_p)
    # one advantage is inf: the gradient is not finite and the step is skipped
    opt.zero_grad()
    m.policy_loss(batch, tokens, torch.tensor([float("inf"), -0.5], device=DEV))[0].backward()
    opt.step()
    assert not torch.isfinite(opt.flat_g).all()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((opt.flat_p, opt.m, opt.v, opt.ema), before))
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert opt.skipped_steps.item() == 1 and not math.isfinite(opt.last_grad_norm.item()) and opt.steps == 1
    # a clean step moves the parameters and the EMA
    opt.zero_grad()
    m.policy_loss(batch, tokens, torch.tensor([1.0, -0.5], device=DEV))[0].backward()
    opt.step()
    assert opt.skipped_steps.item() == 1 and math.isfinite(opt.last_grad_norm.item()) and opt.steps == 2
    assert not torch.equal(opt.flat_p, before[0]) and not torch.equal(opt.ema, before[3]) and not torch.equal(opt.ema, opt.flat_p)
    assert torch.isfinite(opt.flat_p).all() and torch.isfinite(opt.ema).all()
    # the averaged weights: inside swap_ema() the model IS a fresh model loaded from ema_tensors()
    raw = [p.detach().clone() for p in opt.params]
    raw_tokens = _tokens(m, batch)
    fresh = build_mage(cfg, seed, DEV)
    with torch.no_grad():
        for p, e in zip([p for p in fresh.parameters() if p.requires_grad], opt.ema_tensors()):
            assert p.shape == e.shape
            p.copy_(e)
    want = _tokens(fresh, batch)
    with opt.swap_ema():
        assert all(torch.equal(p, e) for p, e in zip(opt.params, opt.ema_tensors()))
        got = _tokens(m, batch)
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step()
    assert torch.equal(got, want)
    assert all(torch.equal(bits(p), bits(r)) for p, r in zip(opt.params, raw))
    assert torch.equal(_tokens(m, batch), raw_tokens)
