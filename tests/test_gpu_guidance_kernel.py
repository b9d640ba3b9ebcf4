"""GPU: mage_guide_logits (include/mage_hip_ext.h) against the exact restatement of its rule (tests/guidance_ref.py), bit for bit, and the
properties the header promises: nothing written outside the addressed rows' first K columns, in place == out of place, the exact cases
(scale 1, uncond == cond, the sign of a zero), NaN propagation, row independence, and the refusals."""
import numpy as np
import pytest
import torch

from mage_amd import _lib
from tests import guidance_ref as G
from tests.helpers import refused, sent, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                                                           # floats of sentinel padding either side of `out` (16-byte aligned)
SCALES = np.array([1.0, 0.0, 3.0, 7.5, -0.5, 1.0 + 2.0 ** -23], np.float32)

# name -> (rows of the launch, K, ld, group, in_group_stride, in_off, rows of the buffers, the scale_div between 1 and rows)
CASES = {
    "smallest": (6, 4, 4, 6, 6, 0, 6, 2),
    "ld>K odd rows": (37, 64, 72, 37, 37, 0, 37, 5),
    # frame 2 of [B=3, T=5, hw=2, K]: the addressing of test_regrouped_addressing_writes_only_its_slots (tests/test_gpu_sampling.py)
    "regrouped": (6, 512, 512, 2, 10, 4, 30, 2),
    "largest K": (5, 4096, 4096, 5, 5, 0, 5, 2),
    "three workgroups": (19, 512, 516, 19, 19, 0, 19, 4),          # 8 rows per workgroup at K = 512: the last one holds 3
}


def addr(i, group, stride, off):
    return (i // group) * stride + i % group + off


def data(name):
    """cond, uncond fp32 [buffer rows, ld] (host): logit-like values, some columns equal, a few signed zeros."""
    rows, K, ld, group, stride, off, nbuf, _ = CASES[name]
    g = np.random.default_rng(sum(map(ord, name)))
    c = (3.0 * g.standard_normal((nbuf, ld))).astype(np.float32)
    u = (c + 0.7 * g.standard_normal((nbuf, ld)).astype(np.float32)).astype(np.float32)
    u[:, 1::7] = c[:, 1::7]                                         # d == 0
    c[:, 2::13] = np.float32(-0.0)
    u[:, 2::26] = np.float32(-0.0)                                  # every other one of those: -0 against -0
    return c, u


def call(cond, uncond, out, rows, K, ld, group, stride, off, scale, scale_div):
    """The raw entry point; every pointer argument is a tensor, an address, or None."""
    lib = _lib.lib(0)
    p = lambda t: t.data_ptr() if torch.is_tensor(t) else t        # noqa: E731
    with torch.cuda.device(0):
        _lib.check(lib.mage_guide_logits(p(cond), p(uncond), p(out), rows, K, ld, group, stride, off, p(scale), scale_div,
                                         torch.cuda.current_stream().cuda_stream), lib)


def scales_for(rows, scale_div):
    n = (rows - 1) // scale_div + 1
    return np.resize(SCALES, n) if n > 1 else np.array([7.5], np.float32)


def reference(name, scale_div):
    rows, K, ld, group, stride, off, nbuf, _ = CASES[name]
    c, u = data(name)
    idx = np.array([addr(i, group, stride, off) for i in range(rows)])
    s = scales_for(rows, scale_div)
    z = G.guide_rows(c[idx, :K], u[idx, :K], s[np.arange(rows) // scale_div])
    return c, u, idx, s, z


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_rule_bit_for_bit_and_writes_only_its_elements(name):
    rows, K, ld, group, stride, off, nbuf, mid = CASES[name]
    for scale_div in (1, mid, rows):
        c, u, idx, s, want = reference(name, scale_div)
        cd, ud, sd = torch.from_numpy(c).to(DEV), torch.from_numpy(u).to(DEV), torch.from_numpy(s).to(DEV)
        flat = sent(nbuf * ld + 2 * PAD, torch.float32)
        out = flat[PAD:PAD + nbuf * ld].view(nbuf, ld)
        call(cd, ud, out, rows, K, ld, group, stride, off, sd, scale_div)
        torch.cuda.synchronize()
        got = out[torch.from_numpy(idx).to(DEV), :K].cpu().numpy()
        bad = G.f32_bits(got) != G.f32_bits(want)
        assert not bad.any(), f"{name} scale_div={scale_div}: {int(bad.sum())} of {bad.size} elements differ from the rule, first at {np.argwhere(bad)[:3]}"
        mask = torch.ones(nbuf, ld, dtype=torch.bool, device=DEV)
        mask[torch.from_numpy(idx).to(DEV), :K] = False
        assert untouched(out[mask]) and untouched(flat[:PAD]) and untouched(flat[PAD + nbuf * ld:]), f"{name}: a store left its rows"
        # in place on cond: the same bits, and the rest of cond as it was
        ci = cd.clone()
        call(ci, ud, ci, rows, K, ld, group, stride, off, sd, scale_div)
        torch.cuda.synchronize()
        assert torch.equal(ci[torch.from_numpy(idx).to(DEV), :K].view(torch.int32), out[torch.from_numpy(idx).to(DEV), :K].view(torch.int32))
        assert torch.equal(ci[mask].view(torch.int32), cd[mask].view(torch.int32))
        assert torch.equal(ud.cpu().view(torch.int32), torch.from_numpy(u).view(torch.int32))          # the inputs are read only


def test_exact_cases():
    name = "ld>K odd rows"
    rows, K, ld, group, stride, off, nbuf, _ = CASES[name]
    c, u = data(name)
    cd, ud = torch.from_numpy(c).to(DEV), torch.from_numpy(u).to(DEV)
    cbits = torch.from_numpy(c[:, :K].copy()).view(torch.int32)
    one = torch.ones(rows, device=DEV)
    out = sent((nbuf, ld), torch.float32)
    call(cd, ud, out, rows, K, ld, group, stride, off, one, 1)                              # scale 1: cond's bits
    assert torch.equal(out[:, :K].cpu().view(torch.int32), cbits)
    out = sent((nbuf, ld), torch.float32)
    call(cd, cd.clone(), out, rows, K, ld, group, stride, off, torch.full((rows,), 7.5, device=DEV), 1)   # uncond a copy of cond
    got = out[:, :K].cpu()
    assert torch.equal(got.view(torch.int32), cbits)
    neg0 = torch.from_numpy(c[:, :K].copy()).view(torch.int32) == -2 ** 31
    assert neg0.any() and bool((got.view(torch.int32)[neg0] == -2 ** 31).all())             # a -0.0 keeps its sign
    # a -0.0 in cond against a +0.0 in uncond at scale 7.5: d = -0 - 0 = -0 == 0, still cond's bits (the fma would give +0)
    z = torch.zeros(4, 4, device=DEV)
    nz = -z
    out = sent((4, 4), torch.float32)
    call(nz, z, out, 4, 4, 4, 4, 4, 0, torch.full((4,), 7.5, device=DEV), 1)
    assert bool((out.cpu().view(torch.int32) == -2 ** 31).all())


def test_nan_reaches_only_its_own_element():
    name = "three workgroups"
    rows, K, ld, group, stride, off, nbuf, _ = CASES[name]
    c, u, idx, s, want = reference(name, 1)
    c, u = c.copy(), u.copy()
    c[4, 17] = np.nan
    u[11, 300] = np.nan
    c[13, 8] = u[13, 8] = np.inf                                                            # inf - inf
    assert all(s[r] != 1.0 for r in (4, 11, 13))
    out = sent((nbuf, ld), torch.float32)
    call(torch.from_numpy(c).to(DEV), torch.from_numpy(u).to(DEV), out, rows, K, ld, group, stride, off, torch.from_numpy(s).to(DEV), 1)
    got = out[:, :K].cpu().numpy()
    hit = np.zeros((rows, K), bool)
    hit[4, 17] = hit[11, 300] = hit[13, 8] = True
    assert np.isnan(got[hit]).all()
    assert np.array_equal(G.f32_bits(got[~hit]), G.f32_bits(want[~hit]))


def test_a_row_alone_equals_the_row_in_a_larger_launch():
    name = "ld>K odd rows"
    rows, K, ld, group, stride, off, nbuf, _ = CASES[name]
    c, u, idx, s, want = reference(name, 1)
    cd, ud, sd = torch.from_numpy(c).to(DEV), torch.from_numpy(u).to(DEV), torch.from_numpy(s).to(DEV)
    for r in (0, 20, 36):
        out = sent((1, ld), torch.float32)
        call(cd[r:], ud[r:], out, 1, K, ld, 1, 1, 0, sd[r:], 1)
        assert np.array_equal(G.f32_bits(out[0, :K].cpu().numpy()), G.f32_bits(want[r]))
        assert untouched(out[0, K:])


def test_refusals_launch_nothing():
    rows, K, ld = 8, 64, 72
    cd, ud = torch.randn(rows, ld, device=DEV), torch.randn(rows, ld, device=DEV)
    sd = torch.full((rows + 1,), 3.0, device=DEV)
    out = sent((rows, ld), torch.float32)
    ok = dict(cond=cd, uncond=ud, out=out, rows=rows, K=K, ld=ld, group=rows, stride=rows, off=0, scale=sd, scale_div=1)
    bad = [dict(K=6, ld=8), dict(K=62), dict(K=0), dict(K=-4), dict(K=4100, ld=4100), dict(ld=70), dict(ld=60), dict(ld=0), dict(rows=0),
           dict(rows=-1), dict(group=0), dict(group=-2), dict(scale_div=0), dict(scale_div=-1), dict(stride=-1), dict(off=-1),
           dict(cond=None), dict(uncond=None), dict(scale=None), dict(cond=cd.data_ptr() + 4), dict(uncond=ud.data_ptr() + 8),
           dict(out=out.data_ptr() + 4), dict(scale=sd.data_ptr() + 2), dict(scale=sd.data_ptr() + 1)]
    for b in bad:
        refused(lambda b=b: call(**{**ok, **b}), out)
    with pytest.raises(ValueError):
        call(**{**ok, "out": None})
    call(**ok)                                                                              # the same arguments unbroken: accepted
    torch.cuda.synchronize()
    assert not untouched(out[:, :K])
