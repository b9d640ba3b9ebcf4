"""GPU: the GroupNorm, BatchNorm, ADAIN, KL and MSE kernels of the randomness branch, the MAGE+ head and the stage-1 VQ-VAE
(mage_amd/csrc/norm.hip, rows.hip) against the fp64 restatements of tests/norm_ref.py (formulas and the derivation of every per-element
bound are in that module's docstring), at the edges of their dispatch.  The C entry points are called through mage_amd._lib where mage_amd.ops
hides a parameter (n_part, stats, red, the partial buffers).

Which kernel a call reaches, and the cases that reach it:
  gn_stats_kernel + gn_apply_kernel<float | bf16 | f16>   test_groupnorm_forward[case]: (C, groups) (8, 8), (8, 4), (12, 4), (64, 16), (512, 32),
                                                  (256, 1): cpg 1, 2, 3 (a float4 straddles groups), 4, 16, 256; rows_per_sample 1, 5, 255, 257
                                                  (a thread with two rows), 300; 1 and 3 samples (sample 1 ~ N(64, 1), sample 2 constant);
                                                  act 0, 1, 2; residual; x and y in different padded row maps; t ~ -100 under SiLU;
                                                  test_groupnorm_silu: the packed-output entry point, the three dtypes
  gn_bwd_reduce_kernel + gn_bwd_apply_kernel      test_groupnorm_backward[case-chained]: the ladder without cpg 3; cpg 256 is one row phase, rows 3
                                                  fewer rows than the 16 to 256 phases of the others; rows 257; stats from fp64 or from the
                                                  forward kernel; residual and dres each present or null
  adain_kernel, adain_bwd_kernel                  test_adain[B-P-C]: C 64 and 128 (two column blocks); P 1, 2, 3 (phases that own nothing), 4, 5, 257
  add_scaled_rowvec_kernel                        test_add_scaled_rowvec: (3, 5, 4), (2, 65, 260)
  bn_colreduce_kernel<0 | 1 | 2>                  test_bn_colreduce[shape-C]: C 4, 256, 260 (a second column block of 4 live threads);
                                                  (rows, n_part) (1, 1), (7, 3), (5, 8) (three workgroups own nothing), (1000, 4); the mask
  bn_apply_kernel<float | bf16>, bn_bwd_apply_kernel  test_bn_apply[rows-C]: rows 1, 5, 257, C 4 and 260, relu, residual, mask
  the three through mage_amd.ops + sum_partials   test_bn_composition: rows 130 (n_part 2), rows ~ N(64, 1)
  reparam_kl_kernel, reparam_kl_bwd_kernel        test_reparam_kl[n-B]: n 1, 63, 255, 256, 257, 1000; logvar over [-20, 10]; coef 0 and 0.37 / B
  mse_partial_kernel + mse_final_kernel,          test_mse[case]: (1, 1, 1, 1), (7, 5, 8, 5), (33, 300, 304, 512), (300, 257, 260, 257): 77100
    mse_bwd_kernel                                elements, a second sweep of the 65536-thread grid; ld_da = cols and cols + 3

Every case: each output starts filled with the NaN sentinel of its dtype (tests/helpers.py SENTINEL) with rows or elements past its end;
everything outside the written region must still hold the sentinel, everything inside must have been written and lie within its bound; no
element is exempt.  The constant sample of a GroupNorm case (variance exactly 0) must give act(beta + residual) bit for bit for act 0 and 1; under
SiLU, where expf has no bit-exact restatement, it must meet the bound of the activation alone (et = 0).  Refused calls return MAGE_EINVAL and
leave the outputs untouched."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import norm_ref as R
from tests.helpers import DEV, bits, lib, ptr, refused, sent, untouched, within, written

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": ops.F32, "bf16": ops.BF16, "f16": ops.F16}
TAIL = 64


def d64(t):
    return None if t is None else t.double()


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ GroupNorm forward
def _gn_forward(c, silu_entry=False):
    C, groups, rows, B, act, kind = c["C"], c["groups"], c["rows"], c["B"], c["act"], c["kind"]
    i = R.gn_inputs(C, groups, rows, B, act, c["res"], cold=act == 2)
    xbuf, _, _ = R.padded(i.x, R.GN_PAD, R.GN_OFF)                         # NaN in the rows between the samples: reading one is loud
    ypad, yoff = (0, 0) if silu_entry else (R.GN_YPAD, R.GN_YOFF)
    _, ymask, yrows = R.padded(i.x, ypad, yoff)
    y = sent((ymask.numel(), C), DT[kind])
    stats = sent(B * groups * 2 + TAIL, torch.float32)
    l, s = lib()
    xd, gd, bd, rd = dev(xbuf), dev(i.gamma), dev(i.beta), dev(None if i.res is None else i.res.reshape(B * rows, C))
    if silu_entry:
        _lib.check(l.mage_groupnorm_silu(xd.data_ptr(), rows + R.GN_PAD, R.GN_OFF, B, rows, C, groups, gd.data_ptr(), bd.data_ptr(), R.GN_EPS,
                                         stats.data_ptr(), y.data_ptr(), CODE[kind], s), l)
    else:
        _lib.check(l.mage_groupnorm_act(xd.data_ptr(), rows + R.GN_PAD, R.GN_OFF, B, rows, C, groups, gd.data_ptr(), bd.data_ptr(), R.GN_EPS,
                                        stats.data_ptr(), ptr(rd), act, y.data_ptr(), CODE[kind], rows + ypad, yoff, s), l)
    sync()
    entry = "mage_groupnorm_silu" if silu_entry else "mage_groupnorm_act"
    name = R.case_id(c)
    yc, st = y.cpu(), stats.cpu()
    assert untouched(yc[~ymask]) and written(yc[ymask]) and untouched(st[B * groups * 2:]) and written(st[:B * groups * 2]), f"{name}: footprint"
    f = R.groupnorm_act(d64(i.x), d64(i.gamma), d64(i.beta), groups, d64(i.res), act, kind)
    st = st[:B * groups * 2].reshape(B, groups, 2)
    within(entry, name + " mean", st[..., 0], f.mean, f.b_mean)
    within(entry, name + " rstd", st[..., 1], f.rstd, f.b_rstd)
    got = yc[yrows].reshape(B, rows, C)
    within(entry, name + " y", got, f.y, f.b_y)
    if act == 2:
        assert bool((f.t[..., 1] < -95).all()) and not got[..., 1].any(), "t ~ -100 under SiLU: exactly 0, not NaN"
    if B == 3:                                                               # the constant sample: variance exactly 0
        t = i.beta + (i.res[2] if c["res"] else 0.0)
        assert bool((st[2, :, 0] == 0.5).all()) and bool((st[2, :, 1] == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(R.GN_EPS)))))).all())
        if act < 2:
            want = (torch.relu(t) if act else t).expand(rows, C).to(DT[kind])
            assert torch.equal(bits(got[2].contiguous()), bits(want.contiguous())), f"{name}: the constant sample is act(beta + residual), bit for bit"
        else:                                                                # SiLU of the exact t: only the activation's own error
            y2, b2 = R.act_fwd(d64(t).expand(rows, C), torch.zeros(rows, C, dtype=torch.float64), 2)
            within(entry, name + " y of the constant sample", got[2], y2, b2 + R.store_err(y2, kind))
    return st


@pytest.mark.parametrize("c", R.gn_fwd_cases(), ids=R.case_id)
def test_groupnorm_forward(c):
    _gn_forward(c)


@pytest.mark.parametrize("c", R.GN_SILU_CASES, ids=R.case_id)
def test_groupnorm_silu(c):
    _gn_forward(c, silu_entry=True)


# ------------------------------------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("chained", [False, True], ids=["fp64stats", "chained"])
@pytest.mark.parametrize("c", R.gn_bwd_cases(), ids=R.case_id)
def test_groupnorm_backward(c, chained):
    C, groups, rows, B, act = c["C"], c["groups"], c["rows"], c["B"], c["act"]
    i = R.gn_inputs(C, groups, rows, B, act, c["res"], seed=1)
    xbuf, xmask, xrows = R.padded(i.x, R.GN_PAD, R.GN_OFF)
    dybuf, _, _ = R.padded(i.dy, R.GN_YPAD, R.GN_YOFF)
    l, s = lib()
    xd, gd, bd, dyd = dev(xbuf), dev(i.gamma), dev(i.beta), dev(dybuf)
    rd = dev(None if i.res is None else i.res.reshape(B * rows, C))
    if chained:                                                              # the forward kernel's own stats
        stats = torch.empty(B, groups, 2, device=DEV)
        y = torch.empty(B * rows, C, device=DEV)
        _lib.check(l.mage_groupnorm_act(xd.data_ptr(), rows + R.GN_PAD, R.GN_OFF, B, rows, C, groups, gd.data_ptr(), bd.data_ptr(), R.GN_EPS,
                                        stats.data_ptr(), ptr(rd), act, y.data_ptr(), ops.F32, rows, 0, s), l)
    else:
        st = R.gn_stats(d64(i.x), groups)
        stats = dev(torch.stack([st.mean, st.rstd], -1).float())
    dx = sent(tuple(xbuf.shape), torch.float32)
    dres = sent((B * rows + 3, C), torch.float32) if c["res"] != chained else None   # all four of residual x dres over the two variants
    red = sent(B * groups * 2 + TAIL, torch.float32)
    dgp, dbp = sent(B * C + TAIL, torch.float32), sent(B * C + TAIL, torch.float32)
    _lib.check(l.mage_groupnorm_bwd(xd.data_ptr(), rows + R.GN_PAD, R.GN_OFF, B, rows, C, groups, stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), ptr(rd),
                                    act, dyd.data_ptr(), rows + R.GN_YPAD, R.GN_YOFF, red.data_ptr(), dx.data_ptr(), ptr(dres), dgp.data_ptr(), dbp.data_ptr(), s), l)
    sync()
    name = R.case_id(c) + (" chained" if chained else "")
    dxc, redc, dgc, dbc, stc = dx.cpu(), red.cpu(), dgp.cpu(), dbp.cpu(), stats.cpu()
    assert untouched(dxc[~xmask]) and written(dxc[xmask]), f"{name}: dx is written with x's row map and nowhere else"
    assert untouched(redc[B * groups * 2:]) and written(redc[:B * groups * 2]) and untouched(dgc[B * C:]) and written(dgc[:B * C]) and \
        untouched(dbc[B * C:]) and written(dbc[:B * C]), f"{name}: footprint"
    r = R.groupnorm_bwd(d64(i.x), stc[..., 0].double(), stc[..., 1].double(), d64(i.gamma), d64(i.beta), groups, d64(i.res), act, d64(i.dy))
    if act == 1:
        assert R.sign_margin(r.t, r.et) > 4
    e = "mage_groupnorm_bwd"
    within(e, name + " dx", dxc[xrows].reshape(B, rows, C), r.dx, r.b_dx)
    within(e, name + " red", redc[:B * groups * 2].reshape(B, groups, 2), r.red, r.b_red)
    within(e, name + " dgamma_part", dgc[:B * C].reshape(B, C), r.dg, r.b_dg)
    within(e, name + " dbeta_part", dbc[:B * C].reshape(B, C), r.db, r.b_db)
    if dres is not None:
        drc = dres.cpu()
        assert untouched(drc[B * rows:]) and written(drc[:B * rows])
        within(e, name + " dres", drc[:B * rows].reshape(B, rows, C), r.dres, r.b_dres)


def test_groupnorm_refusals():
    l, s = lib()
    x, g = torch.randn(64, 12, device=DEV), torch.randn(12, device=DEV)
    stats_in = torch.randn(2, 4, 2, device=DEV)
    y, stats = sent((64, 12), torch.float32), sent(64, torch.float32)
    dx, red, dgp, dbp = sent((64, 12), torch.float32), sent(64, torch.float32), sent(64, torch.float32), sent(64, torch.float32)

    def fwd(C=8, groups=4, rows=5, B=2, act=1, code=ops.F32, xx=x, yy=y, st=stats):
        return lambda: _lib.check(l.mage_groupnorm_act(ptr(xx), 16, 2, B, rows, C, groups, g.data_ptr(), g.data_ptr(), 1e-5, ptr(st), None, act, ptr(yy), code,
                                                       rows, 0, s), l)

    def silu(C=8, groups=4, code=ops.F32, yy=y):
        return lambda: _lib.check(l.mage_groupnorm_silu(x.data_ptr(), 16, 2, 2, 5, C, groups, g.data_ptr(), g.data_ptr(), 1e-5, stats.data_ptr(), ptr(yy), code, s), l)

    def bwd(C=8, groups=4, rows=5, B=2, act=1, xx=x, dd=dx):
        return lambda: _lib.check(l.mage_groupnorm_bwd(ptr(xx), 16, 2, B, rows, C, groups, stats_in.data_ptr(), g.data_ptr(), g.data_ptr(), None, act, x.data_ptr(),
                                                       16, 2, red.data_ptr(), ptr(dd), None, dgp.data_ptr(), dbp.data_ptr(), s), l)
    for call in (fwd(xx=None), fwd(yy=None), fwd(st=None), fwd(rows=0), fwd(B=0), fwd(groups=0), fwd(C=6, groups=3), fwd(C=8, groups=3), fwd(act=3), fwd(act=-1),
                 fwd(code=9), fwd(code=ops.BF16X3), silu(yy=None), silu(C=6, groups=3), silu(code=9)):
        refused(call, y, stats)
    for call in (bwd(C=12, groups=4), bwd(xx=None), bwd(dd=None), bwd(rows=0), bwd(B=0), bwd(groups=0), bwd(C=8, groups=3), bwd(act=3), bwd(act=-1)):
        refused(call, dx, red, dgp, dbp)                                     # the first: 3 channels per group do not divide 256


# ------------------------------------------------------------------------------------------------ ADAIN, row vector
@pytest.mark.parametrize("B,P,C", R.ADAIN_CASES)
def test_adain(B, P, C):
    i = R.adain_inputs(B, P, C)
    n = B * P * C
    l, s = lib()
    xd, gd, bd, dd = dev(i.x), dev(i.gamma), dev(i.beta), dev(i.dout)
    out = sent(n + TAIL, torch.float32)
    _lib.check(l.mage_adain(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, P, C, R.ADAIN_EPS, s), l)
    dx, dgm = sent(n + TAIL, torch.float32), sent(n + TAIL, torch.float32)
    _lib.check(l.mage_adain_bwd(xd.data_ptr(), gd.data_ptr(), dd.data_ptr(), dx.data_ptr(), dgm.data_ptr(), B, P, C, R.ADAIN_EPS, s), l)
    sync()
    for t in (out, dx, dgm):
        assert untouched(t[n:]) and written(t[:n])
    name = f"B={B} P={P} C={C}"
    ref, b = R.adain(d64(i.x), d64(i.gamma), d64(i.beta))
    got = out[:n].cpu().reshape(B, P, C)
    within("mage_adain", name, got, ref, b)
    rdx, b_dx, rdg, b_dg = R.adain_bwd(d64(i.x), d64(i.gamma), d64(i.dout))
    gdx = dx[:n].cpu().reshape(B, P, C)
    within("mage_adain_bwd", name + " dx", gdx, rdx, b_dx)
    within("mage_adain_bwd", name + " dgamma_map", dgm[:n].cpu().reshape(B, P, C), rdg, b_dg)
    if P == 1:
        assert torch.equal(got, i.beta), "one position: xhat = 0, out = beta exactly"
        assert not gdx.any(), "one position: dx = 0 exactly"


@pytest.mark.parametrize("B,P,C", R.ROWVEC_CASES)
def test_add_scaled_rowvec(B, P, C):
    g = R._g(B, P, C)
    x, sv, v = torch.randn(B, P, C, generator=g), torch.randn(B, generator=g), torch.randn(C, generator=g)
    n = B * P * C
    buf = sent(n + TAIL, torch.float32)
    buf[:n] = x.reshape(-1).to(DEV)
    l, s = lib()
    sd, vd = dev(sv), dev(v)
    _lib.check(l.mage_add_scaled_rowvec(buf.data_ptr(), sd.data_ptr(), vd.data_ptr(), B, P, C, s), l)
    sync()
    assert untouched(buf[n:]) and written(buf[:n])
    ref, b = R.add_scaled_rowvec(d64(x), d64(sv), d64(v))
    within("mage_add_scaled_rowvec", f"B={B} P={P} C={C}", buf[:n].cpu().reshape(B, P, C), ref, b)


def test_adain_refusals():
    l, s = lib()
    x = torch.randn(2 * 5 * 72, device=DEV)
    out, dx, dgm = sent(2 * 5 * 72, torch.float32), sent(2 * 5 * 72, torch.float32), sent(2 * 5 * 72, torch.float32)

    def fwd(B=2, P=5, C=64, xx=x, oo=out):
        return lambda: _lib.check(l.mage_adain(ptr(xx), x.data_ptr(), x.data_ptr(), ptr(oo), B, P, C, 1e-5, s), l)

    def bwd(B=2, P=5, C=64, xx=x, oo=dx):
        return lambda: _lib.check(l.mage_adain_bwd(ptr(xx), x.data_ptr(), x.data_ptr(), ptr(oo), dgm.data_ptr(), B, P, C, 1e-5, s), l)

    def vec(B=2, P=5, C=64, xx=out, vv=x):
        return lambda: _lib.check(l.mage_add_scaled_rowvec(ptr(xx), x.data_ptr(), ptr(vv), B, P, C, s), l)
    for call in (fwd(C=72), fwd(C=32), fwd(C=0), fwd(P=0), fwd(B=0), fwd(xx=None), fwd(oo=None)):
        refused(call, out)
    for call in (bwd(C=72), bwd(C=32), bwd(P=0), bwd(B=0), bwd(xx=None), bwd(oo=None)):
        refused(call, dx, dgm)
    for call in (vec(C=6), vec(C=0), vec(P=0), vec(B=0), vec(xx=None), vec(vv=None)):
        refused(call, out)


# ------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("C", R.BN_RED_C)
@pytest.mark.parametrize("rows,n_part", R.BN_RED_SHAPES)
def test_bn_colreduce(rows, n_part, C):
    i = R.bn_inputs(rows, C)
    xd, dyd, md = (dev(R.bn_tail(v)) for v in (i.x, i.dy, i.mask))           # rows of 1e6 past `rows`
    mean, rstd = dev(i.mean), dev(i.rstd)
    l, s = lib()
    rpb = -(-rows // n_part)
    for mode, mask in ((0, None), (1, None), (2, None), (2, i.mask)):
        nout = 2 if mode == 2 else 1
        part = sent(n_part * nout * C + TAIL, torch.float32)
        _lib.check(l.mage_bn_colreduce(mode, xd.data_ptr(), dyd.data_ptr() if mode == 2 else None, None if mask is None else md.data_ptr(),
                                       mean.data_ptr() if mode else None, rstd.data_ptr() if mode == 2 else None, rows, C, part.data_ptr(), n_part, s), l)
        sync()
        pc = part.cpu()
        assert untouched(pc[n_part * nout * C:]) and written(pc[:n_part * nout * C])
        got = pc[:n_part * nout * C].reshape(n_part, nout, C)
        for p in range(n_part):
            if p * rpb >= rows:
                assert not got[p].any(), f"workgroup {p} owns no row: its partials must be exactly 0"
        ref, b = R.bn_colreduce(mode, d64(i.x), d64(i.dy), d64(mask), d64(i.mean), d64(i.rstd), n_part)
        within("mage_bn_colreduce", f"mode={mode} rows={rows} n_part={n_part} C={C} mask={mask is not None}", got, ref, b)


@pytest.mark.parametrize("C", R.BN_APPLY_C)
@pytest.mark.parametrize("rows", R.BN_APPLY_ROWS)
def test_bn_apply(rows, C):
    l, s = lib()
    for relu in (False, True):
        for res in (False, True):
            i = R.bn_inputs(rows, C, relu=relu, res=res)
            xd, md, rsd, gd, bd, rd = dev(i.x), dev(i.mean), dev(i.rstd), dev(i.gamma), dev(i.beta), dev(i.res)
            for kind in ("f32", "bf16"):
                y = sent((rows + 3, C), DT[kind])
                _lib.check(l.mage_bn_apply(xd.data_ptr(), md.data_ptr(), rsd.data_ptr(), gd.data_ptr(), bd.data_ptr(), ptr(rd), y.data_ptr(), CODE[kind], rows, C,
                                           int(relu), s), l)
                sync()
                assert untouched(y[rows:]) and written(y[:rows])
                ref, b, t, et = R.bn_apply(d64(i.x), d64(i.mean), d64(i.rstd), d64(i.gamma), d64(i.beta), d64(i.res), relu, kind)
                if relu:
                    assert R.sign_margin(t, et) > 4
                within("mage_bn_apply", f"rows={rows} C={C} relu={relu} res={res} {kind}", y[:rows].cpu(), ref, b)
    i = R.bn_inputs(rows, C)
    xd, dyd, mkd, md, rsd, gd = dev(i.x), dev(i.dy), dev(i.mask), dev(i.mean), dev(i.rstd), dev(i.gamma)
    sums = torch.randn(2, C, generator=R._g(rows, C, 3)) * rows ** 0.5
    sd = dev(sums)
    for mask in (None, i.mask):
        dx = sent((rows + 3, C), torch.float32)
        _lib.check(l.mage_bn_bwd_apply(xd.data_ptr(), dyd.data_ptr(), None if mask is None else mkd.data_ptr(), md.data_ptr(), rsd.data_ptr(), gd.data_ptr(),
                                       sd.data_ptr(), dx.data_ptr(), rows, C, s), l)
        sync()
        assert untouched(dx[rows:]) and written(dx[:rows])
        ref, b = R.bn_bwd_apply(d64(i.x), d64(i.dy), d64(mask), d64(i.mean), d64(i.rstd), d64(i.gamma), d64(sums))
        within("mage_bn_bwd_apply", f"rows={rows} C={C} mask={mask is not None}", dx[:rows].cpu(), ref, b)


@pytest.mark.parametrize("big", [False, True], ids=["plain", "mean64"])
def test_bn_composition(big):
    """ops.bn_train_stats / ops.bn_backward (n_part = rows / 64 = 2) against fp64: the statistics, then dx, dgamma, dbeta from them."""
    rows, C = 130, 260
    i = R.bn_inputs(rows, C, big=big)
    xd, dyd, mkd, gd = dev(i.x), dev(i.dy), dev(i.mask), dev(i.gamma)
    mean, var, rstd = ops.bn_train_stats(xd, R.BN_EPS)
    x = d64(i.x)
    rm, bm = R.bn_mean(x, 2)
    within("ops.bn_train_stats", f"big={big} mean", mean.cpu(), rm, bm)
    mc = mean.cpu().double()
    rv, bv, rr, br = R.bn_var_rstd(x, mc, 2)                                 # the variance about the mean the kernel was handed
    within("ops.bn_train_stats", f"big={big} var", var.cpu(), rv, bv)
    within("ops.bn_train_stats", f"big={big} rstd", rstd.cpu(), rr, br)
    for mask in (None, i.mask):
        dx = sent((rows + 3, C), torch.float32)
        dgamma, dbeta = ops.bn_backward(xd, dyd, mean, rstd, gd, dx[:rows], mask=None if mask is None else mkd)
        sync()
        assert untouched(dx[rows:]) and written(dx[:rows])
        rc = rstd.cpu().double()
        sums, bs = R.bn_sums(2, x, d64(i.dy), d64(mask), mc, rc, 2)
        within("ops.bn_backward", f"big={big} mask={mask is not None} dbeta", dbeta.cpu(), sums[0], bs[0])
        within("ops.bn_backward", f"big={big} mask={mask is not None} dgamma", dgamma.cpu(), sums[1], bs[1])
        got = torch.stack([dbeta, dgamma]).cpu().double()
        ref, b = R.bn_bwd_apply(x, d64(i.dy), d64(mask), mc, rc, d64(i.gamma), got)
        within("ops.bn_backward", f"big={big} mask={mask is not None} dx", dx[:rows].cpu(), ref, b)


def test_bn_refusals():
    l, s = lib()
    x = torch.randn(8, 8, device=DEV)
    v = torch.randn(16, device=DEV)
    part, y, dx = sent(64, torch.float32), sent((8, 8), torch.float32), sent((8, 8), torch.float32)

    def red(mode=0, xx=x, pp=part, rows=8, C=8, n_part=2, dy=x, mean=v, rstd=v):
        return lambda: _lib.check(l.mage_bn_colreduce(mode, ptr(xx), ptr(dy), None, ptr(mean), ptr(rstd), rows, C, ptr(pp), n_part, s), l)

    def app(xx=x, yy=y, rows=8, C=8, code=ops.F32, mean=v):
        return lambda: _lib.check(l.mage_bn_apply(ptr(xx), ptr(mean), v.data_ptr(), v.data_ptr(), v.data_ptr(), None, ptr(yy), code, rows, C, 1, s), l)

    def bwd(xx=x, dd=dx, rows=8, C=8, sums=v):
        return lambda: _lib.check(l.mage_bn_bwd_apply(ptr(xx), x.data_ptr(), None, v.data_ptr(), v.data_ptr(), v.data_ptr(), ptr(sums), ptr(dd), rows, C, s), l)
    for call in (red(mode=3), red(mode=-1), red(xx=None), red(pp=None), red(rows=0), red(C=0), red(n_part=0), red(mode=1, mean=None), red(mode=2, mean=None),
                 red(mode=2, dy=None), red(mode=2, rstd=None)):
        refused(call, part)
    for call in (app(xx=None), app(yy=None), app(mean=None), app(rows=0), app(C=0), app(C=6), app(code=ops.F16), app(code=9)):
        refused(call, y)
    for call in (bwd(xx=None), bwd(dd=None), bwd(sums=None), bwd(rows=0), bwd(C=0), bwd(C=6)):
        refused(call, dx)


# ------------------------------------------------------------------------------------------------ reparameterisation + KL
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", R.KL_N)
def test_reparam_kl(n, B):
    i = R.kl_inputs(B, n)
    l, s = lib()
    mu, lv, eps, dz = dev(i.mu), dev(i.lv), dev(i.eps), dev(i.dz)
    out, kl = sent(B * n + TAIL, torch.float32), sent(B + TAIL, torch.float32)
    _lib.check(l.mage_reparam_kl(mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), out.data_ptr(), kl.data_ptr(), B, n, s), l)
    sync()
    assert untouched(out[B * n:]) and written(out[:B * n]) and untouched(kl[B:]) and written(kl[:B])
    ro, bo, rk, bk = R.reparam_kl(d64(i.mu), d64(i.lv), d64(i.eps))
    within("mage_reparam_kl", f"n={n} B={B} out", out[:B * n].cpu().reshape(B, n), ro, bo)
    within("mage_reparam_kl", f"n={n} B={B} kl_sum", kl[:B].cpu(), rk, bk)
    for coef in (0.0, R.KL_COEF / B):
        cd = torch.tensor([coef], device=DEV)
        dmu, dlv = sent(B * n + TAIL, torch.float32), sent(B * n + TAIL, torch.float32)
        _lib.check(l.mage_reparam_kl_bwd(mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), dz.data_ptr(), cd.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), B * n, s), l)
        sync()
        assert untouched(dmu[B * n:]) and written(dmu[:B * n]) and untouched(dlv[B * n:]) and written(dlv[:B * n])
        rm, bm, rl, bl = R.reparam_kl_bwd(d64(i.mu), d64(i.lv), d64(i.eps), d64(i.dz), float(cd.cpu()[0]))
        within("mage_reparam_kl_bwd", f"n={n} B={B} coef={coef:.3g} dmu", dmu[:B * n].cpu().reshape(B, n), rm, bm)
        within("mage_reparam_kl_bwd", f"n={n} B={B} coef={coef:.3g} dlogvar", dlv[:B * n].cpu().reshape(B, n), rl, bl)
        if coef == 0.0:
            assert torch.equal(dmu[:B * n].cpu().reshape(B, n), i.dz), "coef 0: dmu = dz exactly"


def test_reparam_kl_refusals():
    l, s = lib()
    x = torch.randn(64, device=DEV)
    out, kl, dmu, dlv = (sent(64, torch.float32) for _ in range(4))

    def fwd(mu=x, oo=out, kk=kl, B=2, n=32):
        return lambda: _lib.check(l.mage_reparam_kl(ptr(mu), x.data_ptr(), x.data_ptr(), ptr(oo), ptr(kk), B, n, s), l)

    def bwd(mu=x, coef=x, dm=dmu, dl=dlv, n=64):
        return lambda: _lib.check(l.mage_reparam_kl_bwd(ptr(mu), x.data_ptr(), x.data_ptr(), x.data_ptr(), ptr(coef), ptr(dm), ptr(dl), n, s), l)
    for call in (fwd(mu=None), fwd(oo=None), fwd(kk=None), fwd(B=0), fwd(n=0), fwd(n=-1)):
        refused(call, out, kl)
    for call in (bwd(mu=None), bwd(coef=None), bwd(dm=None), bwd(dl=None), bwd(n=0)):
        refused(call, dmu, dlv)


# ------------------------------------------------------------------------------------------------ MSE
@pytest.mark.parametrize("rows,cols,lda,ldb", R.MSE_CASES)
def test_mse(rows, cols, lda, ldb):
    a, b = R.mse_inputs(rows, cols, lda, ldb)
    ad, bd = dev(a), dev(b)
    l, s = lib()
    ws = torch.full((256 + 8,), -1.0e300, dtype=torch.float64, device=DEV)
    out = sent(1 + TAIL, torch.float32)
    _lib.check(l.mage_mse(ad.data_ptr(), lda, bd.data_ptr(), ldb, rows, cols, ws.data_ptr(), out.data_ptr(), s), l)
    sync()
    assert untouched(out[1:]) and written(out[:1]) and bool((ws[256:] == -1.0e300).all()), "one float of output, 256 doubles of workspace"
    ref, bnd = R.mse(d64(a), d64(b), cols)
    name = f"rows={rows} cols={cols} lda={lda} ldb={ldb}"
    within("mage_mse", name, out[:1].cpu(), ref.reshape(1), bnd.reshape(1))
    go = torch.tensor([R.MSE_GOUT], device=DEV)
    for ld_da in (cols, cols + 3):
        da = sent((rows + 1, ld_da), torch.float32)
        _lib.check(l.mage_mse_bwd(ad.data_ptr(), lda, bd.data_ptr(), ldb, rows, cols, go.data_ptr(), da.data_ptr(), ld_da, s), l)
        sync()
        assert untouched(da[rows:]) and written(da[:rows])
        rda, bda = R.mse_bwd(d64(a), d64(b), cols, float(go.cpu()[0]), ld_da)
        got = da[:rows].cpu()
        within("mage_mse_bwd", f"{name} ld_da={ld_da}", got, rda, bda)
        assert not got[:, cols:].any(), "padding columns are exactly 0"


def test_mse_refusals():
    l, s = lib()
    a = torch.randn(8, 8, device=DEV)
    ws = torch.zeros(256, dtype=torch.float64, device=DEV)
    out, da = sent(4, torch.float32), sent((8, 8), torch.float32)

    def fwd(aa=a, bb=a, lda=8, ldb=8, rows=8, cols=5, ww=ws, oo=out):
        return lambda: _lib.check(l.mage_mse(ptr(aa), lda, ptr(bb), ldb, rows, cols, ptr(ww), ptr(oo), s), l)

    def bwd(aa=a, lda=8, ldb=8, rows=8, cols=5, gg=a, dd=da, ld_da=8):
        return lambda: _lib.check(l.mage_mse_bwd(ptr(aa), lda, a.data_ptr(), ldb, rows, cols, ptr(gg), ptr(dd), ld_da, s), l)
    for call in (fwd(lda=4), fwd(ldb=4), fwd(lda=0), fwd(ldb=-8), fwd(aa=None), fwd(bb=None), fwd(ww=None), fwd(oo=None), fwd(rows=0), fwd(cols=0)):
        refused(call, out)                                                   # the first four: a row stride below cols
    for call in (bwd(lda=4), bwd(ldb=4), bwd(ld_da=4), bwd(aa=None), bwd(gg=None), bwd(dd=None), bwd(rows=0), bwd(cols=0)):
        refused(call, da)
