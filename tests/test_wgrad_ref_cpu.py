"""CPU: the fp64 restatements and bounds of tests/wgrad_ref.py.  Each reference is pinned against torch (autograd of F.gelu, x * sigmoid(1.702 x),
relu and tanh; torch.optim.Adam in float64; dy.double().t() @ x.double(); F.unfold and plain indexing for the gathers).  Float32 emulations of
the kernels in the summation order their comments in train.hip / optim.hip / gemm_tn.hip state must meet every bound on every case of
tests/test_gpu_wgrad_kernels.py, and eleven subtly wrong kernels ("mutants") must each leave a bound, or break a bit-exact check, on the case
named in their test."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import train_ref as TR
from tests import wgrad_ref as R

F = np.float32
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
def transpose_emu(xb, M, Mp, C, out_h=1, out_w=None, in_h=None, in_w=None, img_stride=None, a_off=0, dy=0, dx=0, stride=1, mutant=None):
    """transpose_kernel's index arithmetic, one output column at a time.  mutants: 'swap_hw' (out_h and out_w exchanged in the decomposition of
    m), 'stride_on_tap' (the stride multiplies the tap shift instead of the output pixel)."""
    out_w = M if out_w is None else out_w
    in_h = out_h if in_h is None else in_h
    in_w = out_w if in_w is None else in_w
    img_stride = in_h * in_w if img_stride is None else img_stride
    x = xb.numpy()
    y = np.zeros((C, Mp), x.dtype)
    ow = out_h if mutant == "swap_hw" else out_w
    for m in range(M):
        img, rem = divmod(m, out_h * out_w)
        oy, ox = divmod(rem, ow)
        iy, ix = (oy + dy * stride, ox + dx * stride) if mutant == "stride_on_tap" else (oy * stride + dy, ox * stride + dx)
        if 0 <= iy < in_h and 0 <= ix < in_w:
            y[:, m] = x[img * img_stride + iy * in_w + ix + a_off, :C]
    return torch.from_numpy(y)


def tc_emu(x, M, Mp, C, geo, mutant=None):
    """transpose8_colsum_kernel's sums: a thread owns the 8 rows mm .. mm + 7 of every tile of its part and adds them in order; the 8 threads of
    a channel meet by xor-shuffles 1, 2, 4.  mutant 'drop_partial_tile': a tile that is not full (m0 + 64 > Mp) is left out of the sum."""
    g = R.transpose(x, M, Mp, C, **geo).t().numpy().astype(F)               # [Mp, C]
    n_part = R.tc_n_part(Mp)
    out = np.zeros((n_part, C), F)
    for p in range(n_part):
        cs = np.zeros((8, C), F)
        for t in range(16):
            m0 = (p * 16 + t) * 64
            if m0 >= Mp or (mutant == "drop_partial_tile" and m0 + 64 > Mp):
                break
            for k in range(8):
                for j in range(8):
                    if m0 + k * 8 < Mp:
                        cs[k] = cs[k] + g[m0 + k * 8 + j]
        for o in (1, 2, 4):
            cs = cs + cs[np.arange(8) ^ o]
        out[p] = cs[0]
    return torch.from_numpy(out)


def gemm_emu(dy, x, T, tps, n_split, mutant=None):
    """gemm_tn_kernel: 64-token slabs, two 32-token MFMA steps each, rows from t_end on read as zeros; an accumulator takes its 32 products in
    token order (one rounding each: the 16-bit MFMA's inner order is not stated).  db: a lane group adds tokens 8 g .. 8 g + 7 of every step,
    two per v_dot2 (rounded once), the four groups meet as (g0 + g1) + (g2 + g3).  dy, x: float32 arrays WITH their guard rows.
    mutants: 'past_T' (the rows of the last slab are read up to the slab's end), 'empty_unwritten' (a slice without tokens stores nothing)."""
    N, K = dy.shape[1], x.shape[1]
    P, db = np.full((n_split, N, K), NAN, F), np.full((n_split, N), NAN, F)
    for s in range(n_split):
        t0, t1 = s * tps, min(T, (s + 1) * tps)
        nslab = R.cdiv(t1 - t0, 64) if t1 > t0 else 0
        if nslab == 0 and mutant == "empty_unwritten":
            continue
        acc, d = np.zeros((N, K), F), np.zeros((4, N), F)
        lim = t0 + nslab * 64 if mutant == "past_T" else t1
        for step in range(2 * nslab):
            for i in range(32):
                t = t0 + step * 32 + i
                a, b = (dy[t], x[t]) if t < lim else (np.zeros(N, F), np.zeros(K, F))
                acc = acc + a[:, None] * b[None, :]
                if i % 2 == 1:
                    a0 = dy[t - 1] if t - 1 < lim else np.zeros(N, F)
                    d[i // 8] = (d[i // 8].astype(np.float64) + a0.astype(np.float64) + a.astype(np.float64)).astype(F)
        P[s], db[s] = acc, (d[0] + d[1]) + (d[2] + d[3])
    return torch.from_numpy(P), torch.from_numpy(db)


def colsum_emu(x, T, n_part):
    """colsum_kernel: wave w adds the rows t0 + w, t0 + w + 4, ... of its chunk in order; (w0 + w1) + (w2 + w3)."""
    C, per = x.shape[1], R.cdiv(T, n_part)
    out = np.zeros((n_part, C), F)
    for p in range(n_part):
        sw = np.zeros((4, C), F)
        for w in range(4):
            for t in range(p * per + w, min(T, (p + 1) * per), 4):
                sw[w] = sw[w] + x[t]
        out[p] = (sw[0] + sw[1]) + (sw[2] + sw[3])
    return torch.from_numpy(out)


def act_emu(x, kind, dy=None, mutant=None):
    """act_kernel in float32 (torch's float32 exp, erf): y = act(x), or dx = dy act'(x).  mutants: 'qg_no_term' (the QuickGELU derivative
    without 1.702 v (1 - s)), 'tanh_pre' (tanh backward reads x as the pre-activation)."""
    v = x.float()
    one, c = torch.tensor(1.0), torch.tensor(1.702)
    if dy is None:
        y = {"relu": lambda: v.clamp(min=0), "quickgelu": lambda: v / (one + torch.exp(-c * v)),
             "gelu_erf": lambda: 0.5 * v * (one + torch.erf(v * 0.70710678118654752))}[kind]()
    else:
        if kind == "relu":
            D = (v > 0).float()
        elif kind == "tanh":
            t = torch.tanh(v) if mutant == "tanh_pre" else v
            D = one - t * t
        elif kind == "quickgelu":
            s = one / (one + torch.exp(-c * v))
            D = s if mutant == "qg_no_term" else s * (one + c * v * (one - s))
        else:
            D = 0.5 * (one + torch.erf(v * 0.70710678118654752)) + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)
        y = dy.float() * D
    return y.to(x.dtype)


def dropout_emu(x, r, n, p, seed, mutant=None):
    """dropout_add_kernel: y = r + x / (1 - p) where hash32(seed * golden + i) >= p 2^32.  mutant 'mask_per_vector': the mask is taken at i / 4."""
    keep = TR.keep_mask(1, n, p, seed)[0]
    if mutant == "mask_per_vector":
        keep = TR.keep_mask(1, n, p, seed)[0][torch.arange(n) // 4]
    xn, rn = x.numpy().astype(F), r.numpy().astype(F)
    return torch.from_numpy(np.where(keep.numpy(), rn + xn * TR.inv_keep(p), rn).astype(F)), keep


def adam_emu(p, g, m, v, lr, b1, b2, eps, step, gs, mutant=None):
    """adam_update in float32, the bias corrections as mage_adam's host code takes them.  mutants: 'step_minus_1' (the corrections of the step
    before), 'tail_no_v' (the scalar tail from 4 (n / 4) on updates m and p but leaves v)."""
    lr, b1, b2, eps, gs = F(lr), F(b1), F(b2), F(eps), F(gs)
    t = step - 1 if mutant == "step_minus_1" else step
    with np.errstate(all="ignore"):
        bc1 = F(1) - F(math.pow(float(b1), t))
        bc2s = np.sqrt(F(1) - F(math.pow(float(b2), t)))
        p, g, m, v = (a.numpy().astype(F) for a in (p, g, m, v))
        ge = g * gs
        m1 = b1 * m + (F(1) - b1) * ge
        v1 = b2 * v + (F(1) - b2) * ge * ge
        p1 = p - (lr / bc1) * (m1 / (np.sqrt(v1) / bc2s + eps))
        if mutant == "tail_no_v":
            n4 = p.size // 4 * 4
            v1[n4:] = v[n4:]
    return torch.from_numpy(p1), torch.from_numpy(m1), torch.from_numpy(v1)


# ------------------------------------------------------------------------------------------------ mage_transpose
def case(name):
    return next(c for c in R.TRANSPOSE_CASES if c.name == name)


def test_transpose_reference_against_indexing_and_unfold():
    C = 8
    x = torch.randn(2 * 15, C, dtype=torch.float64)
    assert torch.equal(R.transpose(x, 30, 32, C)[:, :30], x.t()) and not R.transpose(x, 30, 32, C)[:, 30:].any()
    xs = torch.randn(2 * 3 * 5, C, dtype=torch.float64)                      # [B 2, L 3, hw 5]
    assert torch.equal(R.transpose(xs, 20, 24, C, **R.REGROUP)[:, :20], xs.view(2, 3, 5, C)[:, 1:].reshape(20, C).t())
    img = x.view(2, 3, 5, C).permute(0, 3, 1, 2)
    cols = Fn.unfold(img, 3, padding=1).view(2, C, 9, 15)                     # [img, c, tap, pixel]
    for t, geo in R.TAPS3:
        assert torch.equal(R.transpose(x, 30, 30, C, **geo), cols[:, :, t].permute(1, 0, 2).reshape(C, 30)), f"3x3 tap {t}"
    x4 = torch.randn(2 * 60, C, dtype=torch.float64)
    cols = Fn.unfold(x4.view(2, 6, 10, C).permute(0, 3, 1, 2), 4, padding=1, stride=2).view(2, C, 16, 15)
    for t, geo in R.TAPS4:
        assert torch.equal(R.transpose(x4, 30, 30, C, **geo), cols[:, :, t].permute(1, 0, 2).reshape(C, 30)), f"4x4 / stride 2 tap {t}"


def test_transpose_emulation_matches_bits_on_every_case():
    for c in R.TRANSPOSE_CASES:
        xb = R.transpose_inputs(c)
        for _, geo in c.calls:
            assert torch.equal(transpose_emu(xb, c.M, c.Mp, c.C, **geo), R.transpose(xb, c.M, c.Mp, c.C, **geo)), c.name
    names = {c.kernel for c in R.TRANSPOSE_CASES}
    assert names == {"transpose_kernel<float>", "transpose_kernel<bf16>", "transpose8_kernel"}
    for n in ("ldx", "ldy", "Mp", "x_off", "y_off"):
        assert case("bf16_fallback_" + n).kernel == "transpose_kernel<bf16>"


def test_mutant_transpose_swaps_out_h_and_out_w():
    c = case("f32_taps3x3")                                                  # the 3 x 5 plane: a square one hides the swap
    xb = R.transpose_inputs(c)
    geo = c.calls[4][1]                                                      # the centre tap: no shift
    assert not torch.equal(transpose_emu(xb, c.M, c.Mp, c.C, mutant="swap_hw", **geo), R.transpose(xb, c.M, c.Mp, c.C, **geo))


def test_mutant_transpose_applies_the_stride_to_the_tap():
    c = case("bf16_taps4x4_s2")
    xb = R.transpose_inputs(c)
    geo = c.calls[0][1]                                                      # dy = dx = -1
    assert not torch.equal(transpose_emu(xb, c.M, c.Mp, c.C, mutant="stride_on_tap", **geo), R.transpose(xb, c.M, c.Mp, c.C, **geo))
    geo = dict(geo, stride=1, in_h=3, in_w=5, img_stride=15)                 # with stride 1 the two readings agree: the stride-1 tests cannot see it
    assert torch.equal(transpose_emu(xb, c.M, c.Mp, c.C, mutant="stride_on_tap", **geo), R.transpose(xb, c.M, c.Mp, c.C, **geo))


# ------------------------------------------------------------------------------------------------ mage_transpose_colsum
def tc_values(c):
    return R.tc_inputs(c).view(torch.bfloat16)


def test_transpose_colsum_emulation_within_bound():
    for c in R.TC_CASES:
        x = tc_values(c)
        ref, b = R.transpose_colsum(x.double(), c.M, c.Mp, c.C, **c.geo)
        assert ref.shape[0] == R.tc_n_part(c.Mp) == (2 if c.Mp == 1032 else 1)
        assert torch.allclose(ref.sum(0), R.transpose(x.double(), c.M, c.Mp, c.C, **c.geo).sum(1), rtol=1e-12, atol=1e-12)
        assert R.ratio(tc_emu(x.float(), c.M, c.Mp, c.C, c.geo), ref, b) <= 1.0, c.name


def test_mutant_transpose_colsum_drops_the_partial_last_tile():
    c = next(c for c in R.TC_CASES if c.name == "C8_Mp1032_M1032")          # tile 16 holds 8 columns: the second part's only tile
    x = tc_values(c)
    ref, b = R.transpose_colsum(x.double(), c.M, c.Mp, c.C, **c.geo)
    got = tc_emu(x.float(), c.M, c.Mp, c.C, c.geo, mutant="drop_partial_tile")
    assert R.ratio(got[:1], ref[:1], b[:1]) <= 1.0 and R.ratio(got[1:], ref[1:], b[1:]) > 1.0


# ------------------------------------------------------------------------------------------------ mage_gemm_tn
def test_gemm_tn_reference_and_emulation():
    for N, K in R.GEMM_NK:
        for T, tps, n_split in R.GEMM_8W + R.GEMM_4W:
            assert R.gemm_4w(T, tps, n_split) == ((T, tps, n_split) in R.GEMM_4W)
            dy, x = R.gemm_inputs(T, N, K)
            r = R.gemm_tn(dy[:T].double(), x[:T].double(), T, tps, n_split)
            assert torch.allclose(r.P.sum(0), dy[:T].double().t() @ x[:T].double(), rtol=1e-12, atol=1e-12)
            assert torch.allclose(r.db.sum(0), dy[:T].double().sum(0), rtol=1e-12, atol=1e-12)
            P, db = gemm_emu(dy.float().numpy(), x.float().numpy(), T, tps, n_split)
            assert R.ratio(P, r.P, r.bP) <= 1.0 and R.ratio(db, r.db, r.bdb) <= 1.0, (N, K, T, tps, n_split)
            for s in range(n_split):
                if s * tps >= T:
                    assert not P[s].any() and not db[s].any() and not r.P[s].any()


def test_mutant_gemm_tn_reads_the_last_slab_past_T():
    T, tps, n_split = 65, 64, 2                                              # the second slice holds one token: 63 guard rows follow it
    dy, x = R.gemm_inputs(T, 256, 256)
    r = R.gemm_tn(dy[:T].double(), x[:T].double(), T, tps, n_split)
    P, db = gemm_emu(dy.float().numpy(), x.float().numpy(), T, tps, n_split, mutant="past_T")
    assert R.ratio(P[:1], r.P[:1], r.bP[:1]) <= 1.0 and R.ratio(P[1:], r.P[1:], r.bP[1:]) > 1.0 and R.ratio(db[1:], r.db[1:], r.bdb[1:]) > 1.0


def test_mutant_gemm_tn_leaves_an_empty_slice_unwritten():
    T, tps, n_split = 64, 64, 3
    dy, x = R.gemm_inputs(T, 256, 256)
    r = R.gemm_tn(dy[:T].double(), x[:T].double(), T, tps, n_split)
    P, db = gemm_emu(dy.float().numpy(), x.float().numpy(), T, tps, n_split, mutant="empty_unwritten")
    assert R.ratio(P[:1], r.P[:1], r.bP[:1]) <= 1.0 and R.ratio(P[1:], r.P[1:], r.bP[1:]) > 1.0 and R.ratio(db[1:], r.db[1:], r.bdb[1:]) > 1.0


# ------------------------------------------------------------------------------------------------ mage_colsum, mage_sum_partials
def test_colsum_emulation_within_bound():
    for C, T, n_part in R.COLSUM_CASES:
        x = R.colsum_inputs(C, T)[:T, :C]
        ref, b = R.colsum(x.double(), T, n_part)
        assert torch.allclose(ref.sum(0), x.double().sum(0), rtol=1e-12, atol=1e-12)
        got = colsum_emu(x.float().numpy(), T, n_part)
        assert R.ratio(got, ref, b) <= 1.0, (C, T, n_part)
        if (T, n_part) == (3, 5):
            assert not ref[3:].any() and not got[3:].any()


def sp_cases():
    for n_part in R.SP_NPART:
        for n in R.SP_N:
            yield n, n, n_part, 0
        for e in R.SP_EXTRA:
            yield e["n"], e["stride"], n_part, e["out_off"]


def test_sum_partials_fixed_order_sum_within_bound():
    kinds = set()
    for n, stride, n_part, off in sp_cases():
        part, start = R.sp_inputs(n, stride, n_part)
        vec = R.sp_vector(n, stride, n_part, off)
        kinds.add(vec)
        for st in (None, start):
            ref, b = R.sum_partials(part.double(), n, None if st is None else st.double())
            assert torch.allclose(ref, part[:, :n].double().sum(0) + (0 if st is None else st.double()), rtol=1e-12, atol=1e-12)
            assert R.ratio(R.sum_partials_f32(part, n, st, vec), ref, b) <= 1.0, (n, stride, n_part, off)
    assert kinds == {True, False}
    assert not R.sp_vector(250, 250, 16, 0) and not R.sp_vector(252, 252, 3, 0) and not R.sp_vector(252, 254, 16, 0) and not R.sp_vector(252, 252, 16, 1)


def test_mutant_sum_partials4_skips_partials_from_16_on():
    n, n_part = 252, 17
    part, start = R.sp_inputs(n, n, n_part)
    part[16] = 3.0                                                           # a last partial that cannot hide
    ref, b = R.sum_partials(part.double(), n)
    good, bad = R.sum_partials_f32(part, n, None, True), R.sum_partials_f32(part, n, None, True, skip_from=16)
    assert R.ratio(good, ref, b) <= 1.0 and R.ratio(bad, ref, b) > 1.0 and not torch.equal(good, bad)


# ------------------------------------------------------------------------------------------------ mage_act, mage_act_bwd
def test_act_references_against_autograd():
    z = torch.linspace(-12, 12, 481, dtype=torch.float64).requires_grad_()
    dy = torch.randn(481, dtype=torch.float64)
    for kind, fn in (("relu", torch.relu), ("gelu_erf", Fn.gelu), ("quickgelu", lambda t: t * torch.sigmoid(R.C_QG * t))):      # x * sigmoid(1.702 x), 1.702 as the fp32 literal
        y = fn(z)
        (gz,) = torch.autograd.grad(y, z, dy)
        assert torch.allclose(R.act(z.detach(), kind)[0], y.detach(), rtol=1e-12, atol=1e-14), kind
        assert torch.allclose(R.act_bwd(z.detach(), dy, kind)[0], gz, rtol=1e-12, atol=1e-14), kind
    y = torch.tanh(z)
    (gz,) = torch.autograd.grad(y, z, dy)
    assert torch.allclose(R.act_bwd(y.detach(), dy, "tanh")[0], gz, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_act_emulation_within_bound(dt):
    for n in R.ACT_N:
        for x, dy in R.act_inputs(n, dt):
            assert x.numel() == n
            for kind in R.ACTS_BWD:
                if kind != "tanh":
                    ref, e = R.act(x.double(), kind)
                    got = act_emu(x, kind)
                    assert R.ratio(got, ref, e if dt == "f32" else R.bf16_bound(ref, e)) <= 1.0, (n, kind, "forward")
                ref, e = R.act_bwd(x.double(), dy.double(), kind)
                got = act_emu(x, kind, dy)
                assert R.ratio(got, ref, e if dt == "f32" else R.bf16_bound(ref, e)) <= 1.0, (n, kind, "backward")
    allx = torch.cat([x for n in R.ACT_N for x, _ in R.act_inputs(n, "f32")])
    for v in R.ACT_SPECIAL:
        assert bool(((allx == v) & (torch.signbit(allx) == (math.copysign(1, v) < 0))).any())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mutant_quickgelu_derivative_loses_its_second_term(dt):
    (x, dy), = R.act_inputs(1024, dt)
    ref, e = R.act_bwd(x.double(), dy.double(), "quickgelu")
    assert R.ratio(act_emu(x, "quickgelu", dy, mutant="qg_no_term"), ref, e if dt == "f32" else R.bf16_bound(ref, e)) > 1.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mutant_tanh_backward_takes_x_as_the_pre_activation(dt):
    (x, dy), = R.act_inputs(1024, dt)
    ref, e = R.act_bwd(x.double(), dy.double(), "tanh")
    assert R.ratio(act_emu(x, "tanh", dy, mutant="tanh_pre"), ref, e if dt == "f32" else R.bf16_bound(ref, e)) > 1.0


# ------------------------------------------------------------------------------------------------ mage_dropout, mage_dropout_add
def test_dropout_emulation_is_exact_and_the_per_vector_mask_is_not():
    for n in R.DROP_N:
        for p in R.DROP_P:
            for seed in R.DROP_SEEDS:
                x, r = R.drop_inputs(n, seed)
                keep = TR.keep_mask(1, n, p, seed)[0]
                unf, fus = TR.dropout_add_exact(x, r, keep, TR.inv_keep(p))
                y, k = dropout_emu(x, r, n, p, seed)
                assert torch.equal(y.view(torch.int32), unf.view(torch.int32)) and torch.equal(k, keep)
                assert bool(keep.all()) == (p == 0.0)
    n, p, seed = 1028, 0.5, R.GOLD                                           # the named case of the mutant
    x, r = R.drop_inputs(n, seed)
    keep = TR.keep_mask(1, n, p, seed)[0]
    unf, fus = TR.dropout_add_exact(x, r, keep, TR.inv_keep(p))
    y, k = dropout_emu(x, r, n, p, seed, mutant="mask_per_vector")
    assert not torch.equal(k, keep) and not torch.equal(y.view(torch.int32), unf.view(torch.int32)) and not torch.equal(y.view(torch.int32), fus.view(torch.int32))


# ------------------------------------------------------------------------------------------------ mage_adam
def adam_cases():
    for n in R.ADAM_N:
        for step in R.ADAM_STEPS:
            for gs in R.ADAM_SCALES:
                for hyper in R.ADAM_HYPER:
                    yield n, step, gs, hyper


def test_adam_reference_against_torch_optim():
    for b1, b2, eps in R.ADAM_HYPER:
        p0 = torch.randn(37, dtype=torch.float64)
        w = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([w], lr=TR.f32(R.ADAM_LR), betas=(TR.f32(b1), TR.f32(b2)), eps=TR.f32(eps))
        p, m, v = p0.clone(), torch.zeros(37, dtype=torch.float64), torch.zeros(37, dtype=torch.float64)
        for step in (1, 2, 3):
            g = torch.randn(37, dtype=torch.float64)
            w.grad = g * 0.125
            opt.step()
            r = R.adam(p, g, m, v, R.ADAM_LR, b1, b2, eps, step, 0.125)
            p, m, v = r.p, r.m, r.v
            assert torch.allclose(p, w.detach(), rtol=1e-12, atol=1e-14), (b1, b2, eps, step)


def adam_check(n, step, gs, hyper, mutant=None):
    """The largest ratio of four consecutive steps of the emulation, each against the reference fed the emulation's previous state."""
    b1, b2, eps = hyper
    p, g, m, v, idx = R.adam_inputs(n, step, b1, b2)
    worst = 0.0
    for k in range(4):
        r = R.adam(p.double(), g.double(), m.double(), v.double(), R.ADAM_LR, b1, b2, eps, step + k, gs)
        p1, m1, v1 = adam_emu(p, g, m, v, R.ADAM_LR, b1, b2, eps, step + k, gs, mutant)
        worst = max(worst, R.ratio(p1, r.p, r.bp), R.ratio(m1, r.m, r.bm), R.ratio(v1, r.v, r.bv))
        if mutant is None and idx.zero is not None:
            assert p1[idx.zero].view(torch.int32) == p[idx.zero].view(torch.int32), "g = m = v = 0 must leave p bit-identical"
        p, m, v = p1, m1, v1
    return worst


def test_adam_emulation_within_bound():
    for n, step, gs, hyper in adam_cases():
        assert adam_check(n, step, gs, hyper) <= 1.0, (n, step, gs, hyper)


def test_mutant_adam_bias_correction_of_the_step_before():
    assert adam_check(1024, 2, 1.0, R.ADAM_HYPER[0], mutant="step_minus_1") > 1.0
    assert adam_check(1024, 1, 1.0, R.ADAM_HYPER[0], mutant="step_minus_1") > 1.0      # 1 - beta^0 = 0: a division by zero


def test_mutant_adam_tail_leaves_v():
    assert adam_check(1027, 2, 1.0, R.ADAM_HYPER[0], mutant="tail_no_v") > 1.0         # n = 1027: three tail elements, two of them with g != 0
    assert adam_check(3, 2, 1.0, R.ADAM_HYPER[0], mutant="tail_no_v") > 1.0            # n = 3: nothing but the tail
    assert adam_check(1024, 2, 1.0, R.ADAM_HYPER[0], mutant="tail_no_v") <= 1.0        # no tail: the mutant is the kernel
