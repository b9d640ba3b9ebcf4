"""CPU: the fp64 restatements and bounds of tests/norm_ref.py.  The backward references against fp64 autograd of the forward ones, the forward
ones against torch's own norms; float32 NumPy emulations of the kernels in the kernels' own summation order (position and row phases, the
butterfly and the four wave sums of the double accumulators, per-workgroup slabs, the order of the partials) must meet every bound on every
case of tests/test_gpu_norm_kernels.py; nine subtly wrong kernels ("mutants"), and a one-pass BatchNorm variance, must each leave a bound on the
case named in their test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import norm_ref as R
from tests.helpers import within

F = np.float32
F64 = np.float64
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def n32(t):
    return None if t is None else t.numpy().astype(F)


def d64(t):
    return None if t is None else t.double()


def ok(name, got, ref, bound):
    within("emulation", name, torch.from_numpy(np.asarray(got, dtype=F64)), ref, bound)


def leaves(got, ref, bound):
    """The worst |err| / bound of a mutant."""
    err = (torch.from_numpy(np.asarray(got, dtype=F64)) - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic
def block_sum(v):
    """[..., 256] doubles -> the workgroup sum: xor butterfly inside each wave (32 first), then red[0] + red[1] + red[2] + red[3]."""
    w = v.reshape(v.shape[:-1] + (4, 64))
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., idx ^ o]
    r = w[..., 0]
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def thread_rows(xg):
    """[B, R, G, cpg] -> per-thread slices [B, k, 256, G, cpg] (thread tid owns rows tid, tid + 256, ..) and their validity [k, 256]."""
    B, R, G, cpg = xg.shape
    k = -(-R // 256)
    buf = np.zeros((B, k * 256, G, cpg), xg.dtype)
    buf[:, :R] = xg
    return buf.reshape(B, k, 256, G, cpg), (np.arange(k * 256) < R).reshape(k, 256)


def silu32(t):
    with np.errstate(over="ignore"):
        return (t / (F(1) + np.exp(-t).astype(F))).astype(F)


def dact32(act, t, dy):
    if act == 1:
        return np.where(t > 0, dy, F(0)).astype(F)
    if act == 2:
        with np.errstate(over="ignore"):
            sg = (F(1) / (F(1) + np.exp(-t).astype(F))).astype(F)
        return (dy * sg * (F(1) + t * (F(1) - sg))).astype(F)
    return dy


def gn_stats_emu(x, groups, eps, count_rows=None):
    """gn_stats_kernel: (mean, rstd) float32 [B, G].  count_rows: the mutant's row count."""
    B, R, C = x.shape
    cpg = C // groups
    xt, valid = thread_rows(x.reshape(B, R, groups, cpg).astype(F64))
    n = F64((count_rows or R) * cpg)
    s = np.zeros((B, 256, groups), F64)
    for j in range(xt.shape[1]):
        for c in range(cpg):
            s = s + xt[:, j, :, :, c]
    mean = block_sum(np.moveaxis(s, 1, -1)) / n
    q = np.zeros((B, 256, groups), F64)
    for j in range(xt.shape[1]):
        for c in range(cpg):
            dlt = (xt[:, j, :, :, c] - mean[:, None, :]) * valid[j][None, :, None]
            q = q + dlt * dlt
    var = block_sum(np.moveaxis(q, 1, -1)) / n
    return mean.astype(F), (1.0 / np.sqrt(var + F64(F(eps)))).astype(F)


def gn_apply_emu(x, mean, rstd, gamma, beta, res, act, groups, first_group=False):
    B, R, C = x.shape
    cpg = C // groups
    c = np.arange(C)
    gi = ((c - c % 4) if first_group else c) // cpg
    t = (x - mean[:, None, gi]) * rstd[:, None, gi] * gamma + beta
    if res is not None:
        t = t + res
    t = t.astype(F)
    return silu32(t) if act == 2 else np.maximum(t, F(0)) if act == 1 else t


def gn_bwd_emu(x, mean, rstd, gamma, beta, res, act, dy, groups, no_m2=False, no_res_in_act=False):
    """gn_bwd_reduce_kernel + gn_bwd_apply_kernel: (dx, dres, red [B, G, 2], dgamma_part, dbeta_part)."""
    B, R, C = x.shape
    cpg = C // groups
    nph = 256 // cpg
    gi = np.arange(C) // cpg
    xh = ((x - mean[:, None, gi]) * rstd[:, None, gi]).astype(F)
    t = (xh * gamma + beta).astype(F)
    if res is not None and not no_res_in_act:
        t = (t + res).astype(F)
    ge = dact32(act, t, dy)
    k = -(-R // nph)
    buf = np.zeros((2, B, k * nph, C), F64)
    buf[0, :, :R], buf[1, :, :R] = ge, ge.astype(F64) * xh.astype(F64)
    ph = buf.reshape(2, B, k, nph, C)
    acc = np.zeros((2, B, nph, C), F64)
    for j in range(k):                                                       # a phase adds its rows in order
        acc = acc + ph[:, :, j]
    a = np.zeros((2, B, C), F64)
    for p in range(nph):                                                     # thread cl adds the phases in order
        a = a + acc[:, :, p]
    dbet, dgam = a[0].astype(F), a[1].astype(F)
    ag = (a * gamma.astype(F64)).reshape(2, B, groups, cpg)
    tot = np.zeros((2, B, groups), F64)
    for i in range(cpg):
        tot = tot + ag[..., i]
    red = (tot / F64(R * cpg)).astype(F)                                     # [2, B, G]
    m1, m2 = red[0][:, None, gi], red[1][:, None, gi]
    dx = (rstd[:, None, gi] * (gamma * ge - m1 - (F(0) if no_m2 else xh * m2))).astype(F)
    return dx, ge, np.stack([red[0], red[1]], -1), dgam, dbet


def adain_stats_emu(x, eps, onepass=False):
    B, P, C = x.shape
    Pf = F(P)

    def phases(v):
        s = np.zeros((4, B, C), F)
        for p in range(P):
            s[p % 4] = s[p % 4] + v[:, p]
        return ((s[0] + s[1]) + s[2]) + s[3]
    mean = (phases(x) / Pf)[:, None]
    if onepass:
        var = phases((x * x).astype(F)) / Pf - mean[:, 0] * mean[:, 0]
    else:
        dlt = (x - mean).astype(F)
        var = phases((dlt * dlt).astype(F)) / Pf
    return mean.astype(F), (F(1) / np.sqrt((var + F(eps)).astype(F))).astype(F)[:, None], phases


def adain_emu(x, gamma, beta, eps, onepass=False):
    mean, rstd, _ = adain_stats_emu(x, eps, onepass)
    return (gamma * ((x - mean) * rstd) + beta).astype(F)


def adain_bwd_emu(x, gamma, dout, eps):
    mean, rstd, phases = adain_stats_emu(x, eps)
    Pf = F(x.shape[1])
    xh = ((x - mean) * rstd).astype(F)
    g = (dout * gamma).astype(F)
    m1, m2 = (phases(g) / Pf)[:, None], (phases((g * xh).astype(F)) / Pf)[:, None]
    return (rstd * (g - m1 - xh * m2)).astype(F), (dout * xh).astype(F)


def bn_colreduce_emu(mode, xbuf, dybuf, maskbuf, mean, rstd, rows, n_part, overread=False, ignore_mask=False):
    """The buffers carry rows past `rows` (tests/norm_ref.py bn_tail); overread: the last workgroup does not stop at `rows`."""
    C = xbuf.shape[1]
    rpb = -(-rows // n_part)
    part = np.zeros((n_part, 2 if mode == 2 else 1, C), F)
    for p in range(n_part):
        r0 = p * rpb
        r1 = r0 + rpb if overread and r0 < rows else min(rows, r0 + rpb)
        for r in range(r0, r1):
            v = xbuf[r]
            if mode == 0:
                part[p, 0] += v
            elif mode == 1:
                part[p, 0] += (v - mean) * (v - mean)
            else:
                g = dybuf[r]
                if maskbuf is not None and not ignore_mask:
                    g = np.where(maskbuf[r] > 0, g, F(0))
                part[p, 0] += g
                part[p, 1] += g * ((v - mean) * rstd)
    return part


def sum_partials_emu(part):
    n_part = part.shape[0]
    if n_part >= 4:                                                          # sum_partials4_kernel: wave w takes w, w + 4, ..
        sw = [sum((part[p] for p in range(w + 4, n_part, 4)), part[w]) for w in range(4)]
        return (sw[0] + sw[1]) + (sw[2] + sw[3])
    tot = np.zeros_like(part[0])
    for p in range(n_part):
        tot = tot + part[p]
    return tot


def bn_apply_emu(x, mean, rstd, gamma, beta, res, relu):
    o = ((x - mean) * rstd * gamma + beta).astype(F)
    if res is not None:
        o = o + res
    return np.maximum(o, F(0)) if relu else o


def bn_bwd_apply_emu(x, dy, mask, mean, rstd, gamma, sums):
    inv = F(1) / F(x.shape[0])
    g = dy if mask is None else np.where(mask > 0, dy, F(0))
    xh = (x - mean) * rstd
    return (gamma * rstd * (g - sums[0] * inv - xh * (sums[1] * inv))).astype(F)


def kl_emu(mu, lv, eps):
    B, n = mu.shape
    out = (eps * np.exp(F(0.5) * lv).astype(F) + mu).astype(F)
    term = (F(1) + lv - mu * mu - np.exp(lv).astype(F)).astype(F)
    k = -(-n // 256)
    buf = np.zeros((B, k * 256), F64)
    buf[:, :n] = term
    acc = np.zeros((B, 256), F64)
    for j in range(k):
        acc = acc + buf[:, j * 256:(j + 1) * 256]
    return out, block_sum(acc).astype(F)


def kl_bwd_emu(mu, lv, eps, dz, coef, no_half=False):
    c = F(coef)
    h = F(1.0 if no_half else 0.5)
    dmu = (dz + c * mu).astype(F)
    return dmu, (F(0.5) * dz * eps * np.exp(F(0.5) * lv).astype(F) - h * c * (F(1) - np.exp(lv).astype(F))).astype(F)


def mse_emu(a, lda, b, ldb, rows, cols, cols_stride=False):
    """a, b flat float32; mse_partial_kernel's grid-stride loop into doubles, the block sums, mse_final_kernel."""
    total = rows * cols
    nblk = min(256, -(-total // 256))
    i = np.arange(total)
    r, c = i // cols, i % cols
    sa, sb = (cols, cols) if cols_stride else (lda, ldb)
    dlt = (a[r * sa + c] - b[r * sb + c]).astype(F)
    term = (dlt * dlt).astype(F).astype(F64)
    sweep = nblk * 256
    k = -(-total // sweep)
    buf = np.zeros(k * sweep, F64)
    buf[:total] = term
    acc = np.zeros(sweep, F64)
    for j in range(k):
        acc = acc + buf[j * sweep:(j + 1) * sweep]
    s = F64(0)
    for p in block_sum(acc.reshape(nblk, 256)):
        s = s + p
    return F(s * (1.0 / (F64(rows) * cols)))


def mse_bwd_emu(a, lda, b, ldb, rows, cols, gout, ld_da, cols_stride=False):
    inv = F(1.0 / (F64(rows) * cols))
    r, c = np.arange(rows)[:, None], np.arange(cols)[None]
    sa, sb = (cols, cols) if cols_stride else (lda, ldb)
    da = np.zeros((rows, ld_da), F)
    da[:, :cols] = F(2) * (a[r * sa + c] - b[r * sb + c]) * inv * F(gout)
    return da


# ------------------------------------------------------------------------------------------------ the references are right
def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("res", [False, True])
def test_groupnorm_reference(act, res):
    """Forward against F.group_norm, backward against fp64 autograd of the forward reference (stats handed over = the fp64 ones)."""
    for C, groups, rows, B in ((8, 4, 5, 3), (64, 16, 7, 2), (8, 8, 3, 1)):
        i = R.gn_inputs(C, groups, rows, B, act, res)
        x, gm, bt, dy = (d64(v).requires_grad_(v is not i.dy) for v in (i.x, i.gamma, i.beta, i.dy))
        r = d64(i.res).requires_grad_() if res else None
        f = R.groupnorm_act(x, gm, bt, groups, r, act)
        t = Fn.group_norm(x.transpose(1, 2), groups, gm, bt, R.f32(R.GN_EPS)).transpose(1, 2) + (r if res else 0)
        want = t if act == 0 else torch.relu(t) if act == 1 else Fn.silu(t)
        assert rel(f.y, want) < 1e-12
        grads = torch.autograd.grad(f.y, [x, gm, bt] + ([r] if res else []), dy)
        s = R.gn_stats(x.detach(), groups)
        b = R.groupnorm_bwd(x.detach(), s.mean, s.rstd, gm.detach(), bt.detach(), groups, None if r is None else r.detach(), act, dy)
        assert rel(b.dx, grads[0]) < 1e-12 and rel(b.dg.sum(0), grads[1]) < 1e-12 and rel(b.db.sum(0), grads[2]) < 1e-12
        if res:
            assert rel(b.dres, grads[3]) < 1e-12
        gg = (b.dres * gm.detach()).reshape(B, rows, groups, -1)
        xh = ((x.detach().reshape(B, rows, groups, -1) - s.mean[:, None, :, None]) * s.rstd[:, None, :, None])
        assert rel(b.red[..., 0], gg.mean((1, 3))) < 1e-12 and rel(b.red[..., 1], (gg * xh).mean((1, 3))) < 1e-12


def test_adain_reference():
    for B, P, C in ((3, 5, 64), (2, 257, 64), (1, 1, 64), (3, 1, 64)):
        i = R.adain_inputs(B, P, C)
        x, gm, bt, do = d64(i.x).requires_grad_(), d64(i.gamma).requires_grad_(), d64(i.beta), d64(i.dout)
        out, _ = R.adain(x, gm, bt)
        if B > 1 and P > 1:
            want = gm * Fn.instance_norm(x.transpose(1, 2), eps=R.f32(R.ADAIN_EPS)).transpose(1, 2) + bt
        else:                                                                # the written-out formula
            m = x.mean(1, keepdim=True)
            want = gm * (x - m) / torch.sqrt(((x - m) ** 2).mean(1, keepdim=True) + R.f32(R.ADAIN_EPS)) + bt
        assert rel(out, want) < 1e-12
        gx, gg = torch.autograd.grad(out, [x, gm], do)
        dx, _, dgm, _ = R.adain_bwd(x.detach(), gm.detach(), do)
        assert float((dx - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max())) and float((dgm - gg).abs().max()) <= 1e-12 * max(1.0, float(gg.abs().max()))
        if P == 1:
            assert not dx.any() and not gx.any() and torch.equal(out.detach(), bt)


@pytest.mark.parametrize("masked", [False, True])
def test_batchnorm_reference(masked):
    for rows, C in ((130, 8), (1, 4)):
        i = R.bn_inputs(rows, C, relu=masked)
        x, gm, bt, dy = d64(i.x).requires_grad_(), d64(i.gamma).requires_grad_(), d64(i.beta).requires_grad_(), d64(i.dy)
        mean = x.mean(0)
        rstd = (((x - mean) ** 2).mean(0) + R.f32(R.BN_EPS)).rsqrt()
        y, _, _, _ = R.bn_apply(x, mean, rstd, gm, bt, None, masked)
        if rows > 1:
            want = Fn.batch_norm(x, None, None, gm, bt, True, 0.0, R.f32(R.BN_EPS))
            assert rel(y, torch.relu(want) if masked else want) < 1e-12
        gx, gg, gb = torch.autograd.grad(y, [x, gm, bt], dy)
        mask = y.detach() if masked else None
        xd, md, rd = x.detach(), mean.detach(), rstd.detach()
        sums, _ = R.bn_sums(2, xd, dy, mask, md, rd, 2 if rows > 1 else 1)
        dx, _ = R.bn_bwd_apply(xd, dy, mask, md, rd, gm.detach(), sums)
        assert float((dx - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
        assert rel(sums[1], gg) < 1e-12 and rel(sums[0], gb) < 1e-12
        s0, _ = R.bn_sums(0, xd, None, None, None, None, 3 if rows > 1 else 1)
        s1, _ = R.bn_sums(1, xd, None, None, md, None, 3 if rows > 1 else 1)
        assert rel(s0[0] / rows, md) < 1e-12 and float((s1[0] / rows - ((xd - md) ** 2).mean(0)).abs().max()) < 1e-12


def test_kl_and_mse_reference():
    i = R.kl_inputs(3, 257)
    mu, lv, eps, dz = d64(i.mu).requires_grad_(), d64(i.lv).requires_grad_(), d64(i.eps), d64(i.dz)
    out, _, kl, _ = R.reparam_kl(mu, lv, eps)
    c = R.f32(R.KL_COEF / 3)
    loss = (out * dz).sum() + c * (-0.5 * kl.sum())                          # coef = dL/dkl / B of kl = -1/2 mean_b kl_sum
    gmu, glv = torch.autograd.grad(loss, [mu, lv])
    dmu, _, dlv, _ = R.reparam_kl_bwd(mu.detach(), lv.detach(), eps, dz, c)
    assert rel(dmu, gmu) < 1e-12 and rel(dlv, glv) < 1e-12
    a, b = R.mse_inputs(7, 5, 8, 5)
    a = d64(a).requires_grad_()
    v, _ = R.mse(a, d64(b), 5)
    assert rel(v, Fn.mse_loss(a[:, :5], d64(b)[:, :5])) < 1e-12
    (ga,) = torch.autograd.grad(v * R.f32(R.MSE_GOUT), [a])
    da, _ = R.mse_bwd(a.detach(), d64(b), 5, R.MSE_GOUT, 8)
    assert rel(da, ga) < 1e-12 and not da[:, 5:].any()


# ------------------------------------------------------------------------------------------------ the emulations meet the bounds
def _gn_fwd(c, cold=False, **mut):
    i = R.gn_inputs(c["C"], c["groups"], c["rows"], c["B"], c["act"], c["res"], cold=cold)
    f = R.groupnorm_act(d64(i.x), d64(i.gamma), d64(i.beta), c["groups"], d64(i.res), c["act"], c["kind"])
    count = mut.pop("count_rows", None)
    mean, rstd = gn_stats_emu(n32(i.x), c["groups"], R.GN_EPS, count)
    y = gn_apply_emu(n32(i.x), mean, rstd, n32(i.gamma), n32(i.beta), n32(i.res), c["act"], c["groups"], **mut)
    y = torch.from_numpy(y).to(DT[c["kind"]]).float().numpy()                # the store rounds to nearest even
    return i, f, mean, rstd, y


@pytest.mark.parametrize("c", R.gn_fwd_cases() + list(R.GN_SILU_CASES), ids=R.case_id)
def test_groupnorm_forward_emulation(c):
    i, f, mean, rstd, y = _gn_fwd(c, cold=c["act"] == 2)
    if c["act"] == 1:
        assert R.sign_margin(f.t, f.et) > 4
    ok("mean", mean, f.mean, f.b_mean)
    ok("rstd", rstd, f.rstd, f.b_rstd)
    ok("y", y, f.y, f.b_y)
    if c["act"] == 2 and c["C"] > 1:
        assert bool((f.t[..., 1] < -95).all()) and not y[..., 1].any(), "t ~ -100 under SiLU: exactly 0"
    if c["B"] == 3:                                                          # the constant sample
        t = n32(i.beta) + (n32(i.res)[2] if c["res"] else F(0))
        assert rstd[2].tolist() == [float(F(1.0 / np.sqrt(F64(F(R.GN_EPS)))))] * c["groups"] and not (mean[2] != F(0.5)).any()
        if c["act"] < 2:
            want = torch.from_numpy(np.maximum(t, 0) if c["act"] else t).to(DT[c["kind"]]).float().numpy()
            assert np.array_equal(y[2], np.broadcast_to(want, y[2].shape))


def _gn_bwd(c, chained, **mut):
    i = R.gn_inputs(c["C"], c["groups"], c["rows"], c["B"], c["act"], c["res"], seed=1)
    if chained:
        mean, rstd = gn_stats_emu(n32(i.x), c["groups"], R.GN_EPS)
    else:
        s = R.gn_stats(d64(i.x), c["groups"])
        mean, rstd = n32(s.mean), n32(s.rstd)
    r = R.groupnorm_bwd(d64(i.x), torch.from_numpy(mean).double(), torch.from_numpy(rstd).double(), d64(i.gamma), d64(i.beta), c["groups"],
                        d64(i.res), c["act"], d64(i.dy))
    e = gn_bwd_emu(n32(i.x), mean, rstd, n32(i.gamma), n32(i.beta), n32(i.res), c["act"], n32(i.dy), c["groups"], **mut)
    return r, e


@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("c", R.gn_bwd_cases(), ids=R.case_id)
def test_groupnorm_backward_emulation(c, chained):
    r, (dx, dres, red, dg, db) = _gn_bwd(c, chained)
    if c["act"] == 1:
        assert R.sign_margin(r.t, r.et) > 4
    ok("dx", dx, r.dx, r.b_dx)
    ok("dres", dres, r.dres, r.b_dres)
    ok("red", red, r.red, r.b_red)
    ok("dgamma_part", dg, r.dg, r.b_dg)
    ok("dbeta_part", db, r.db, r.b_db)


@pytest.mark.parametrize("B,P,C", R.ADAIN_CASES)
def test_adain_emulation(B, P, C):
    i = R.adain_inputs(B, P, C)
    out, b = R.adain(d64(i.x), d64(i.gamma), d64(i.beta))
    got = adain_emu(n32(i.x), n32(i.gamma), n32(i.beta), R.ADAIN_EPS)
    ok("adain", got, out, b)
    dx, b_dx, dgm, b_dgm = R.adain_bwd(d64(i.x), d64(i.gamma), d64(i.dout))
    gdx, gdgm = adain_bwd_emu(n32(i.x), n32(i.gamma), n32(i.dout), R.ADAIN_EPS)
    ok("adain_bwd dx", gdx, dx, b_dx)
    ok("adain_bwd dgamma_map", gdgm, dgm, b_dgm)
    if P == 1:
        assert np.array_equal(got, n32(i.beta)) and not gdx.any()


@pytest.mark.parametrize("B,P,C", R.ROWVEC_CASES)
def test_rowvec_emulation(B, P, C):
    g = R._g(B, P, C)
    x, s, v = torch.randn(B, P, C, generator=g), torch.randn(B, generator=g), torch.randn(C, generator=g)
    ref, b = R.add_scaled_rowvec(d64(x), d64(s), d64(v))
    ok("rowvec", n32(x) + n32(s)[:, None, None] * n32(v), ref, b)


@pytest.mark.parametrize("C", R.BN_RED_C)
@pytest.mark.parametrize("rows,n_part", R.BN_RED_SHAPES)
def test_bn_colreduce_emulation(rows, n_part, C):
    i = R.bn_inputs(rows, C)
    xb, dyb, mb = (n32(R.bn_tail(v)) for v in (i.x, i.dy, i.mask))
    for mode, mask in ((0, None), (1, None), (2, None), (2, i.mask)):
        ref, b = R.bn_colreduce(mode, d64(i.x), d64(i.dy), d64(mask), d64(i.mean), d64(i.rstd), n_part)
        got = bn_colreduce_emu(mode, xb, dyb, None if mask is None else mb, n32(i.mean), n32(i.rstd), rows, n_part)
        ok(f"mode {mode}", got, ref, b)
        sums, bs = R.bn_sums(mode, d64(i.x), d64(i.dy), d64(mask), d64(i.mean), d64(i.rstd), n_part)
        ok(f"mode {mode} summed", sum_partials_emu(got), sums, bs)
    if rows * C >= 4:
        g = torch.where(i.mask > 0, i.dy, torch.zeros_like(i.dy)).view(-1)
        assert not g[:3].any() and g[3] == i.dy.view(-1)[3], "0.0, -0.0 and a negative mask drop the gradient, 2^-126 keeps it"


@pytest.mark.parametrize("C", R.BN_APPLY_C)
@pytest.mark.parametrize("rows", R.BN_APPLY_ROWS)
def test_bn_apply_emulation(rows, C):
    for relu in (False, True):
        for res in (False, True):
            i = R.bn_inputs(rows, C, relu=relu, res=res)
            y, b, t, et = R.bn_apply(d64(i.x), d64(i.mean), d64(i.rstd), d64(i.gamma), d64(i.beta), d64(i.res), relu)
            if relu:
                assert R.sign_margin(t, et) > 4
            got = bn_apply_emu(n32(i.x), n32(i.mean), n32(i.rstd), n32(i.gamma), n32(i.beta), n32(i.res), relu)
            ok("bn_apply", got, y, b)
            yb, bb, _, _ = R.bn_apply(d64(i.x), d64(i.mean), d64(i.rstd), d64(i.gamma), d64(i.beta), d64(i.res), relu, "bf16")
            ok("bn_apply bf16", torch.from_numpy(got).bfloat16().float().numpy(), yb, bb)
    i = R.bn_inputs(rows, C)
    for mask in (None, i.mask):
        sums = sum_partials_emu(bn_colreduce_emu(2, n32(i.x), n32(i.dy), n32(mask), n32(i.mean), n32(i.rstd), rows, 1))
        dx, b = R.bn_bwd_apply(d64(i.x), d64(i.dy), d64(mask), d64(i.mean), d64(i.rstd), d64(i.gamma), torch.from_numpy(sums).double())
        ok("bn_bwd_apply", bn_bwd_apply_emu(n32(i.x), n32(i.dy), n32(mask), n32(i.mean), n32(i.rstd), n32(i.gamma), sums), dx, b)


def bn_stats_emu(x, n_part, onepass=False):
    """ops.bn_train_stats: (mean, var, rstd) float32 from two reductions; onepass: the mutant's E[x^2] - mean^2."""
    rows = F(x.shape[0])
    mean = sum_partials_emu(bn_colreduce_emu(0, x, None, None, None, None, x.shape[0], n_part))[0] / rows
    if onepass:
        var = sum_partials_emu(bn_colreduce_emu(0, (x * x).astype(F), None, None, None, None, x.shape[0], n_part))[0] / rows - mean * mean
    else:
        var = sum_partials_emu(bn_colreduce_emu(1, x, None, None, mean, None, x.shape[0], n_part))[0] / rows
    return mean, var, (F(1) / np.sqrt(var + F(R.BN_EPS))).astype(F)


@pytest.mark.parametrize("big", [False, True])
def test_bn_composition_emulation(big):
    """rows 130, n_part 2, as ops.bn_train_stats / ops.bn_backward run it; a one-pass variance leaves the bound on rows ~ N(64, 1)."""
    i = R.bn_inputs(130, 260, big=big)
    x = d64(i.x)
    mean, var, rstd = bn_stats_emu(n32(i.x), 2)
    rm, bm = R.bn_mean(x, 2)
    ok("mean", mean, rm, bm)
    rv, bv, rr, br = R.bn_var_rstd(x, torch.from_numpy(mean).double(), 2)
    ok("var", var, rv, bv)
    ok("rstd", rstd, rr, br)
    for mask in (None, i.mask):
        sums = sum_partials_emu(bn_colreduce_emu(2, n32(i.x), n32(i.dy), n32(mask), mean, rstd, 130, 2))
        ref, b = R.bn_sums(2, x, d64(i.dy), d64(mask), torch.from_numpy(mean).double(), torch.from_numpy(rstd).double(), 2)
        ok("sums", sums, ref, b)
    if big:
        _, v1, r1 = bn_stats_emu(n32(i.x), 2, onepass=True)
        assert leaves(v1, rv, bv) > 1 and leaves(r1, rr, br) > 1


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", R.KL_N)
def test_kl_emulation(n, B):
    i = R.kl_inputs(B, n)
    out, b_out, kl, b_kl = R.reparam_kl(d64(i.mu), d64(i.lv), d64(i.eps))
    go, gk = kl_emu(n32(i.mu), n32(i.lv), n32(i.eps))
    ok("out", go, out, b_out)
    ok("kl_sum", gk, kl, b_kl)
    for coef in (0.0, R.KL_COEF / B):
        dmu, b_dmu, dlv, b_dlv = R.reparam_kl_bwd(d64(i.mu), d64(i.lv), d64(i.eps), d64(i.dz), coef)
        gm, gl = kl_bwd_emu(n32(i.mu), n32(i.lv), n32(i.eps), n32(i.dz), coef)
        ok("dmu", gm, dmu, b_dmu)
        ok("dlogvar", gl, dlv, b_dlv)


@pytest.mark.parametrize("rows,cols,lda,ldb", R.MSE_CASES)
def test_mse_emulation(rows, cols, lda, ldb):
    a, b = R.mse_inputs(rows, cols, lda, ldb)
    v, bv = R.mse(d64(a), d64(b), cols)
    ok("mse", mse_emu(n32(a).reshape(-1), lda, n32(b).reshape(-1), ldb, rows, cols), v.reshape(1), bv.reshape(1))
    for ld_da in (cols, cols + 3):
        da, bd = R.mse_bwd(d64(a), d64(b), cols, R.MSE_GOUT, ld_da)
        ok("mse_bwd", mse_bwd_emu(n32(a).reshape(-1), lda, n32(b).reshape(-1), ldb, rows, cols, R.MSE_GOUT, ld_da), da, bd)


# ------------------------------------------------------------------------------------------------ the bounds bite: mutants
def _case(cases, **want):
    (c,) = [c for c in cases if all(c[k] == v for k, v in want.items())]
    return c


def test_mutant_float4_takes_the_group_of_its_first_channel():
    """(C, groups) = (8, 4), rows 257: channels 1 and 3 of every float4 get the neighbouring group's statistics."""
    _, f, _, _, y = _gn_fwd(_case(R.gn_fwd_cases(), C=8, groups=4, rows=257), first_group=True)
    assert leaves(y, f.y, f.b_y) > 1


def test_mutant_groupnorm_divides_by_the_padded_count():
    """(C, groups) = (64, 16), rows 300: n = (rows + 40) cpg."""
    c = _case(R.gn_fwd_cases(), C=64, groups=16, rows=300)
    _, f, mean, rstd, y = _gn_fwd(c, count_rows=c["rows"] + R.GN_PAD)
    assert leaves(mean, f.mean, f.b_mean) > 1 and leaves(rstd, f.rstd, f.b_rstd) > 1 and leaves(y, f.y, f.b_y) > 1


def test_mutant_one_pass_variance_in_adain():
    """(B, P, C) = (3, 257, 64): sample 1 ~ N(64, 1)."""
    i = R.adain_inputs(3, 257, 64)
    out, b = R.adain(d64(i.x), d64(i.gamma), d64(i.beta))
    got = adain_emu(n32(i.x), n32(i.gamma), n32(i.beta), R.ADAIN_EPS, onepass=True)
    assert leaves(got[1], out[1], b[1]) > 1


def test_mutant_gn_bwd_drops_the_xhat_m2_term():
    r, e = _gn_bwd(_case(R.gn_bwd_cases(), C=64, groups=16, rows=257), False, no_m2=True)
    assert leaves(e[0], r.dx, r.b_dx) > 1


def test_mutant_gn_bwd_ignores_the_residual_in_the_activation_derivative():
    for act in (1, 2):
        (c,) = [c for c in R.gn_bwd_cases() if c["res"] and c["act"] == act][:1]
        r, e = _gn_bwd(c, False, no_res_in_act=True)
        assert leaves(e[1], r.dres, torch.maximum(r.b_dres, torch.tensor(R.TINY, dtype=torch.float64))) > 1 and leaves(e[0], r.dx, r.b_dx) > 1


def test_mutant_bn_backward_counts_masked_elements_in_the_sums():
    """(rows, n_part, C) = (7, 3, 4) with the planted mask: the sums ignore the mask, dx applies it."""
    i = R.bn_inputs(7, 4)
    ref, b = R.bn_colreduce(2, d64(i.x), d64(i.dy), d64(i.mask), d64(i.mean), d64(i.rstd), 3)
    got = bn_colreduce_emu(2, n32(i.x), n32(i.dy), n32(i.mask), n32(i.mean), n32(i.rstd), 7, 3, ignore_mask=True)
    assert leaves(got, ref, b) > 1


def test_mutant_bn_reduction_reads_past_rows():
    """(rows, n_part) = (7, 3): the last workgroup reads rows 7 and 8."""
    i = R.bn_inputs(7, 260)
    ref, b = R.bn_colreduce(0, d64(i.x), None, None, None, None, 3)
    got = bn_colreduce_emu(0, n32(R.bn_tail(i.x)), None, None, None, None, 7, 3, overread=True)
    assert leaves(got, ref, b) > 1


def test_mutant_mse_indexes_with_cols():
    """(rows, cols, lda, ldb) = (7, 5, 8, 5): the row stride of a is 8, not 5."""
    a, b = R.mse_inputs(7, 5, 8, 5)
    v, bv = R.mse(d64(a), d64(b), 5)
    assert leaves(mse_emu(n32(a).reshape(-1), 8, n32(b).reshape(-1), 5, 7, 5, cols_stride=True), v.reshape(1), bv.reshape(1)) > 1
    da, bd = R.mse_bwd(d64(a), d64(b), 5, R.MSE_GOUT, 8)
    assert leaves(mse_bwd_emu(n32(a).reshape(-1), 8, n32(b).reshape(-1), 5, 7, 5, R.MSE_GOUT, 8, cols_stride=True), da, bd) > 1


def test_mutant_kl_bwd_omits_the_half():
    """n = 63, coef 0.37 / 3."""
    i = R.kl_inputs(3, 63)
    _, _, dlv, b = R.reparam_kl_bwd(d64(i.mu), d64(i.lv), d64(i.eps), d64(i.dz), R.KL_COEF / 3)
    assert leaves(kl_bwd_emu(n32(i.mu), n32(i.lv), n32(i.eps), n32(i.dz), R.KL_COEF / 3, no_half=True)[1], dlv, b) > 1
