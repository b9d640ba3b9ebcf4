"""CPU: the fp64 restatements and bounds of tests/train_ref.py against float32 NumPy emulations of the kernels in the kernels' own summation
order (lane layout, butterfly, per-wave accumulators, chunk order).  The emulation must meet every bound on every case of
tests/test_gpu_train_kernels.py; eight subtly wrong kernels ("mutants") must each leave a bound on a case named in their test."""
import numpy as np
import pytest
import torch

from tests import train_ref as R

F = np.float32
LN_ROWS = {4: 5, 252: 4, 256: 5, 260: 5, 512: 4, 516: 5, 1024: 4, 1028: 5, 2044: 4, 2048: 5}
LN_EPS = {516: 1e-8}


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
def lanes(a, C):
    """[rows, C] -> [rows, VPL, 64 lanes, 4]: element c sits in vector c / 256 of lane (c % 256) / 4; zero beyond C."""
    buf = np.zeros((a.shape[0], R.vpl(C) * 256), F)
    buf[:, :C] = a
    return buf.reshape(a.shape[0], -1, 64, 4)


def unlanes(a4, C):
    return a4.reshape(a4.shape[0], -1)[:, :C]


def wave_sum(v):
    """common.h wave_sum on the last axis (64 lanes): the xor butterfly, 32 first."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def ln_stats_emu(x4, m4, C, eps, div=None, onepass=False):
    div = F(div or C)
    s = np.zeros(x4.shape[:1] + (64,), F)
    for j in range(x4.shape[1]):
        s = s + ((x4[:, j, :, 0] + x4[:, j, :, 1]) + (x4[:, j, :, 2] + x4[:, j, :, 3]))
    mean = (wave_sum(s) / div)[:, None, None, None]
    t = ((x4 - mean) * m4).astype(F)
    sq = x4 if onepass else t
    q = np.zeros_like(s)
    for j in range(x4.shape[1]):
        for e in range(4):
            q = q + sq[:, j, :, e] * sq[:, j, :, e]
    var = wave_sum(q) / div
    if onepass:
        var = var - mean[:, 0, 0, 0] * mean[:, 0, 0, 0]
    rstd = (F(1) / np.sqrt(var + F(eps)))[:, None, None, None]
    return t, rstd.astype(F)


def ln_emu(x, gamma, beta, eps, **kw):
    C = x.shape[1]
    x4, m4 = lanes(x, C), lanes(np.ones_like(x), C)
    t, rstd = ln_stats_emu(x4, m4, C, eps, **kw)
    return unlanes(t * rstd * lanes(gamma[None], C) + lanes(beta[None], C), C)


def ln_bwd_emu(x, gamma, dy, eps, n_part, start=None, div=None, no_xhat_term=False):
    """layernorm_bwd_kernel with n_part workgroups + mage_sum_partials: (dx, dgamma, dbeta)."""
    rows, C = x.shape
    dv = F(div or C)
    g4, m4 = lanes(gamma[None], C), lanes(np.ones((1, C), F), C)
    dx = np.zeros_like(x) if start is None else start.copy()
    part = np.zeros((n_part, 2) + g4.shape, F)
    for b in range(n_part):
        acc = np.zeros((4, 2) + g4.shape, F)
        for w in range(4):
            for row in range(b * 4 + w, rows, 4 * n_part):
                x4, d4 = lanes(x[row:row + 1], C), lanes(dy[row:row + 1], C)
                t, rstd = ln_stats_emu(x4, m4, C, eps, div=div)
                xh, g = (t * rstd).astype(F), d4 * g4
                sg, sgx = np.zeros((1, 64), F), np.zeros((1, 64), F)
                for j in range(x4.shape[1]):
                    for e in range(4):
                        sg = sg + g[:, j, :, e]
                        sgx = sgx + g[:, j, :, e] * xh[:, j, :, e]
                mg, mgx = wave_sum(sg) / dv, wave_sum(sgx) / dv
                acc[w, 0] += d4 * xh
                acc[w, 1] += d4
                o = rstd * (g - mg - (F(0) if no_xhat_term else xh * mgx))
                dx[row] = unlanes(o, C)[0] + (dx[row] if start is not None else F(0))
        part[b] = (acc[0] + acc[1]) + (acc[2] + acc[3])
    if n_part >= 4:                                                          # sum_partials4_kernel: wave w takes w, w + 4, ..
        sw = [sum((part[p] for p in range(w + 4, n_part, 4)), part[w]) for w in range(4)]
        tot = (sw[0] + sw[1]) + (sw[2] + sw[3])
    else:
        tot = np.zeros_like(part[0])
        for p in range(n_part):
            tot = tot + part[p]
    return dx, unlanes(tot[0], C)[0], unlanes(tot[1], C)[0]


def ce_emu(z, tg, grad_out, no_inv_rows=False, clamp_target=False):
    rows, K = z.shape
    n = -(-K // 64)
    zp = np.full((rows, n * 64), -np.inf, F)
    zp[:, :K] = z
    zl = zp.reshape(rows, n, 64)
    mx = zl.max(1).max(1)[:, None]
    with np.errstate(invalid="ignore"):
        w = np.exp(zp - mx).astype(F)
    s = np.zeros((rows, 64), F)
    for j in range(n):
        s = s + w.reshape(rows, n, 64)[:, j]
    inv = F(1) / wave_sum(s)
    scale = F(grad_out) * (F(1) if no_inv_rows else F(1) / F(rows))
    tgn = np.clip(tg, 0, K - 1) if clamp_target else np.where((tg < 0) | (tg >= K), -1, tg)
    hot = (np.arange(K)[None] == tgn[:, None]).astype(F)
    return ((w[:, :K] * inv[:, None] - hot) * scale).astype(F)


def emb_emu(ids, dout, start, n_table, pad, group, stride, off, count_padding=False):
    i = torch.arange(ids.numel())
    orow = (i // group) * stride + i % group + off
    return R.embedding_det_f32(ids, dout.double()[orow], start, n_table, -1 if count_padding else pad)


def group_emu(x, rows, C, div, mod, rs, rs_div, n_chunk, guard=True):
    out = np.zeros((n_chunk, mod, C), F)
    period = div * mod
    total = -(-rows // period) * div
    per = -(-total // n_chunk)
    for z in range(n_chunk):
        for g in range(mod):
            for i in range(z * per, min(total, (z + 1) * per)):
                r = (i // div) * period + g * div + i % div
                if r < rows or not guard:
                    out[z, g] = out[z, g] + (F(rs[r // rs_div]) if rs is not None else F(1)) * x[r, :C]
    return out


def row_sum_emu(x, n, n_chunk):
    rows = x.shape[0]
    per = R.row_chunk(n, n_chunk)
    out = np.zeros((n_chunk, rows), F)
    for z in range(n_chunk):
        seg = x[:, z * per:min(n, (z + 1) * per)]
        m = -(-max(seg.shape[1], 1) // 64) * 64
        buf = np.zeros((rows, m), F)
        buf[:, :seg.shape[1]] = seg
        s = np.zeros((rows, 64), F)
        for j in range(m // 64):
            s = s + buf[:, j * 64:(j + 1) * 64]
        out[z] = wave_sum(s)
    return out


def stored(y, kind):
    """The fp64 value a store of `kind` leaves of the float32 array y (torch's round-to-nearest-even casts; split pieces hi + lo)."""
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=F))
    if kind == "f32":
        return t.double()
    if kind in ("bf16", "f16"):
        return t.to(torch.bfloat16 if kind == "bf16" else torch.float16).double()
    if kind == "bf16x3":
        hi = t.to(torch.bfloat16).float()
        return hi.double() + (t - hi).to(torch.bfloat16).double()
    hi = t.to(torch.float16).float()
    return hi.double() + ((t - hi) * 2048.0).to(torch.float16).double() / 2048.0


def worst(got, ref, bound):
    err = (torch.as_tensor(got).double() - ref).abs()
    assert bool(torch.isfinite(err).all())
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ------------------------------------------------------------------------------------------------ the references themselves
def test_keep_mask_is_the_attention_masks_hash():
    """The same construction as attention_bwd_ref.keep_scale on a flat index, and the fraction kept is about 1 - p."""
    from tests.attention_bwd_ref import keep_scale
    for p, seed in ((0.1, 0), (0.5, 0x9E3779B97F4A7C15), (R.P_MAX, 3)):
        k = R.keep_mask(6, 516, p, seed)
        ks = keep_scale(dict(n_seq=1, nq=6, nk=516, H=1), p, seed)[0, 0]
        assert torch.equal(k, ks > 0)
        assert abs(float(k.double().mean()) - (1 - p)) < 0.05
    assert bool(R.keep_mask(3, 8, 0.0, 9).all())
    assert float(R.inv_keep(0.5)) == 2.0 and float(R.inv_keep(R.P_MAX)) == 2.0 ** 24


def test_references_agree_with_autograd():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 260, generator=g, dtype=torch.float64).requires_grad_()
    gamma = torch.randn(260, generator=g, dtype=torch.float64).requires_grad_()
    beta = torch.randn(260, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(6, 260, generator=g, dtype=torch.float64)
    y = torch.nn.functional.layer_norm(x, (260,), gamma, beta, 1e-5)
    y.backward(dy)
    yr, _ = R.layernorm(x.detach(), gamma.detach(), beta.detach(), 1e-5)
    r = R.layernorm_bwd(x.detach(), gamma.detach(), dy, 1e-5, 2)
    for a, b in ((yr, y.detach()), (r.dx, x.grad), (r.dg, gamma.grad), (r.db, beta.grad)):
        assert float((a - b).abs().max()) < 1e-9 * max(1.0, float(b.abs().max()))
    z = torch.randn(5, 63, generator=g, dtype=torch.float64).requires_grad_()
    tg = torch.randint(0, 63, (5,), generator=g)
    (torch.nn.functional.cross_entropy(z, tg) * R.f32(0.7)).backward()
    out, _ = R.cross_entropy_bwd(z.detach(), tg, 0.7)
    assert float((out - z.grad).abs().max()) < 1e-15
    tab = torch.randn(30, 8, generator=g, dtype=torch.float64).requires_grad_()
    ids = torch.randint(0, 30, (50,), generator=g)
    do = torch.randn(50, 8, generator=g, dtype=torch.float64)
    torch.nn.functional.embedding(ids, tab, padding_idx=3).backward(do)
    got, _ = R.embedding_bwd(ids, do, torch.zeros(30, 8, dtype=torch.float64), 30, 3)
    assert float((got - tab.grad).abs().max()) < 1e-12


def test_dropout_add_exact_fused_and_unfused():
    """The fused candidate is the correctly rounded r + x * ik (checked in exact rational arithmetic); both candidates occur."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(2)
    x, r = torch.randn(4000, generator=g), torch.randn(4000, generator=g)
    ik = R.inv_keep(0.1)
    unf, fus = R.dropout_add_exact(x, r, torch.ones(4000, dtype=torch.bool), ik)
    assert int((unf != fus).sum()) > 0
    for i in range(0, 4000, 7):
        exact = Fraction(float(x[i])) * Fraction(float(ik)) + Fraction(float(r[i]))
        f = float(fus[i])
        lo, hi = float(np.nextafter(F(f), F(-np.inf))), float(np.nextafter(F(f), F(np.inf)))
        assert abs(exact - Fraction(f)) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi)))


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def _ln(C, special=None, rows=None):
    rows = rows or LN_ROWS[C]
    x, gamma, beta = R.ln_inputs(C, rows, 1, special)
    return x, gamma, beta, LN_EPS.get(C, 1e-5)


@pytest.mark.parametrize("C", R.LN_C + (64,))
def test_layernorm_emulation_meets_the_bound(C):
    kinds = ("f32", "bf16", "f16") + (("bf16x3", "f16x3") if C % 64 == 0 else ())
    for special, rows in ((None, LN_ROWS.get(C, 4)), ("const", 1), ("mean", 1)):
        x, gamma, beta, eps = _ln(C, special, rows)
        y = ln_emu(x.numpy(), gamma.numpy(), beta.numpy(), eps)
        if special != "mean":
            assert np.array_equal(y[0], beta.numpy()), "the constant row must give beta exactly"
        for kind in kinds:
            ref, b = R.layernorm(x.double(), gamma.double(), beta.double(), eps, kind)
            assert worst(stored(y, kind), ref, b) <= 1.0, (C, kind)


@pytest.mark.parametrize("C", [252, 260, 516, 1028, 2044])
def test_mutant_1_layernorm_divides_by_the_padded_width(C):
    x, gamma, beta, eps = _ln(C)
    ref, b = R.layernorm(x.double(), gamma.double(), beta.double(), eps)
    assert worst(ln_emu(x.numpy(), gamma.numpy(), beta.numpy(), eps, div=256 * R.vpl(C)), ref, b) > 1.0
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(C))
    r = R.layernorm_bwd(x.double(), gamma.double(), dy.double(), eps, 2)
    dx, dg, db = ln_bwd_emu(x.numpy(), gamma.numpy(), dy.numpy(), eps, 2, div=256 * R.vpl(C))
    assert worst(dx, r.dx, r.b_dx) > 1.0 and worst(dg, r.dg, r.b_dg) > 1.0


@pytest.mark.parametrize("C", [260, 2048])
def test_mutant_2_one_pass_variance_on_the_large_mean_row(C):
    """Rows ~ N(64, 1): E[x^2] - mean^2 in fp32 leaves the bound by a wide margin, the two-pass emulation stays inside."""
    x, gamma, beta, eps = _ln(C)
    ref, b = R.layernorm(x.double(), gamma.double(), beta.double(), eps)
    big = slice(x.shape[0] - 1, x.shape[0])
    two = worst(ln_emu(x.numpy(), gamma.numpy(), beta.numpy(), eps)[big], ref[big], b[big])
    one = worst(ln_emu(x.numpy(), gamma.numpy(), beta.numpy(), eps, onepass=True)[big], ref[big], b[big])
    assert two <= 1.0 < one, (two, one)
    assert one > 4 * two


# ------------------------------------------------------------------------------------------------ dropout + add + LayerNorm
def _dal(C, p, seed, bf16_x, idx_mutant=False):
    rows = LN_ROWS[C]
    r, gamma, beta = R.ln_inputs(C, rows, 2)
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(C + 1))
    x[0] = 0.0                                                               # with r[0] = 0.5: y[0] constant whatever the mask
    if bf16_x:
        x = x.to(torch.bfloat16).float()
    keep = R.keep_mask(rows, C, p, seed)
    if idx_mutant:
        keep = keep.reshape(rows, C // 4, 4)[:, :, :1].expand(-1, -1, 4).reshape(rows, C)
    y = np.where(keep.numpy(), r.numpy() + x.numpy() * R.inv_keep(p), r.numpy()).astype(F)
    return x, r, gamma, beta, y


@pytest.mark.parametrize("C", R.LN_C)
def test_dropout_add_layernorm_emulation(C):
    eps = LN_EPS.get(C, 1e-5)
    for p, seed in ((0.0, 0), (0.1, 0x9E3779B97F4A7C15), (0.5, 0), (R.P_MAX, 0x9E3779B97F4A7C15)):
        for bf16_x, kind in ((False, "f32"), (False, "bf16"), (True, "bf16")):
            x, r, gamma, beta, y = _dal(C, p, seed, bf16_x)
            unf, _ = R.dropout_add_exact(x, r, R.keep_mask(*x.shape, p, seed), R.inv_keep(p))
            assert np.array_equal(y, unf.numpy())
            yn = ln_emu(y, gamma.numpy(), beta.numpy(), eps)
            ref, b = R.layernorm(torch.from_numpy(y).double(), gamma.double(), beta.double(), eps, kind)
            assert worst(stored(yn, kind), ref, b) <= 1.0, (C, p, kind)


@pytest.mark.parametrize("C,p", [(260, 0.5), (4, 0.5), (2048, 0.1)])
def test_mutant_3_dropout_index_of_the_vector_not_the_element(C, p):
    x, r, gamma, beta, y = _dal(C, p, 0, False, idx_mutant=True)
    unf, fus = R.dropout_add_exact(x, r, R.keep_mask(*x.shape, p, 0), R.inv_keep(p))
    assert not np.array_equal(y, unf.numpy()) and not np.array_equal(y, fus.numpy())


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _lnb(C, rows, bf16_dy):
    x, gamma, _ = R.ln_inputs(C, rows, 3)
    g = torch.Generator().manual_seed(C * 3 + rows)
    dy = torch.randn(rows, C, generator=g)
    if bf16_dy:
        dy = dy.to(torch.bfloat16).float()
    return x, gamma, dy, torch.randn(rows, C, generator=g)


@pytest.mark.parametrize("C", R.LN_C)
def test_layernorm_bwd_emulation_meets_the_bound(C):
    eps = LN_EPS.get(C, 1e-5)
    for rows, n_part, bf16_dy, acc in ((LN_ROWS[C], -(-LN_ROWS[C] // 4), False, False), (LN_ROWS[C], -(-LN_ROWS[C] // 4), True, True),
                                       (11, 1, False, True), (11, 2, True, False), (5, 5, False, False), (1, 1, True, False)):
        x, gamma, dy, start = _lnb(C, rows, bf16_dy)
        st = start if acc else None
        r = R.layernorm_bwd(x.double(), gamma.double(), dy.double(), eps, n_part, None if st is None else st.double())
        dx, dg, db = ln_bwd_emu(x.numpy(), gamma.numpy(), dy.numpy(), eps, n_part, None if st is None else st.numpy())
        assert worst(dx, r.dx, r.b_dx) <= 1.0 and worst(dg, r.dg, r.b_dg) <= 1.0 and worst(db, r.db, r.b_db) <= 1.0, (C, rows, n_part)


@pytest.mark.parametrize("C", [4, 260, 2048])
def test_mutant_4_layernorm_bwd_drops_the_xhat_term(C):
    x, gamma, dy, _ = _lnb(C, 5, False)
    r = R.layernorm_bwd(x.double(), gamma.double(), dy.double(), 1e-5, 2)
    dx, _, _ = ln_bwd_emu(x.numpy(), gamma.numpy(), dy.numpy(), 1e-5, 2, no_xhat_term=True)
    assert worst(dx, r.dx, r.b_dx) > 1.0


# ------------------------------------------------------------------------------------------------ cross entropy backward
@pytest.mark.parametrize("rows,K", R.CE_SHAPES)
def test_cross_entropy_bwd_emulation_meets_the_bound(rows, K):
    z, tg = R.ce_inputs(rows, K)
    out = ce_emu(z.numpy(), tg.numpy(), R.CE_GRAD_OUT)
    for kind in ("f32", "bf16"):
        ref, b = R.cross_entropy_bwd(z.double(), tg, R.CE_GRAD_OUT, kind)
        assert worst(stored(out, kind), ref, b) <= 1.0
    assert bool((torch.from_numpy(out)[torch.isinf(z)] == 0).all())


@pytest.mark.parametrize("rows,K", [(5, 63), (7, 65), (6, 1000)])
def test_mutant_7_cross_entropy_scale_and_out_of_range_targets(rows, K):
    z, tg = R.ce_inputs(rows, K)
    ref, b = R.cross_entropy_bwd(z.double(), tg, R.CE_GRAD_OUT)
    assert worst(ce_emu(z.numpy(), tg.numpy(), R.CE_GRAD_OUT, no_inv_rows=True), ref, b) > 1.0
    assert worst(ce_emu(z.numpy(), tg.numpy(), R.CE_GRAD_OUT, clamp_target=True), ref, b) > 1.0


# ------------------------------------------------------------------------------------------------ embedding backward
EMB = [(1, 1, 64, False), (7, 30, 64, True), (8, 30, 192, False), (9, 512, 64, True), (4096, 30, 64, False), (4097, 30, 64, True),
       (8200, 30, 192, True), (8200, 1, 64, True), (500, 30, 72, True), (500, 513, 64, True), (8191, 512, 64, False), (1, 1, 4, False),
       (8192, 512, 64, True), (8197, 30, 128, True), (300, 512, 64, True), (9000, 64, 64, True)]


@pytest.mark.parametrize("n,n_table,C,grouped", EMB)
def test_embedding_bwd_emulation_meets_the_bound(n, n_table, C, grouped):
    for dt in (torch.float32, torch.bfloat16):
        ids, dout, start, orow, (group, stride, off), pad = R.emb_inputs(n, n_table, C, dt, grouped)
        ref, b = R.embedding_bwd(ids, dout.double()[orow], start.double(), n_table, pad)
        assert worst(emb_emu(ids, dout, start, n_table, pad, group, stride, off), ref, b) <= 1.0


def test_embedding_bwd_emulation_meets_the_bound_at_64_chunks():
    n = 64 * 4096 + 1
    ids, dout, start, orow, (group, stride, off), pad = R.emb_inputs(n, 30, 64, torch.bfloat16, False)
    ref, b = R.embedding_bwd(ids, dout.double()[orow], start.double(), 30, pad)
    assert worst(emb_emu(ids, dout, start, 30, pad, group, stride, off), ref, b) <= 1.0


def test_embedding_chunks_are_the_headers():
    assert R.emb_chunks(4096) == (1, 4096) and R.emb_chunks(4097) == (2, 2056) and R.emb_chunks(8200) == (3, 2736)
    assert R.emb_chunks(64 * 4096 + 1) == (64, 4104) and R.emb_chunks(7) == (1, 8)


@pytest.mark.parametrize("n,n_table,C", [(9, 512, 64), (4097, 30, 64)])
def test_mutant_5_embedding_ignores_off_or_confuses_the_group_stride(n, n_table, C):
    ids, dout, start, orow, (group, stride, off), pad = R.emb_inputs(n, n_table, C, torch.float32, True)
    ref, b = R.embedding_bwd(ids, dout.double()[orow], start.double(), n_table, pad)
    assert worst(emb_emu(ids, dout, start, n_table, pad, group, stride, 0), ref, b) > 1.0
    assert worst(emb_emu(ids, dout, start, n_table, pad, group, group, off), ref, b) > 1.0


@pytest.mark.parametrize("n,n_table,C,grouped", [(7, 30, 64, True), (4096, 30, 64, False)])
def test_mutant_6_embedding_counts_padding_rows(n, n_table, C, grouped):
    ids, dout, start, orow, (group, stride, off), pad = R.emb_inputs(n, n_table, C, torch.float32, grouped)
    assert int((ids == pad).sum()) > 0
    ref, b = R.embedding_bwd(ids, dout.double()[orow], start.double(), n_table, pad)
    assert worst(emb_emu(ids, dout, start, n_table, pad, group, stride, off, count_padding=True), ref, b) > 1.0


# ------------------------------------------------------------------------------------------------ grouped row sums, row sums
@pytest.mark.parametrize("rows,C,div,mod,scaled", R.GROUP_CASES)
def test_group_rowsum_emulation_meets_the_bound(rows, C, div, mod, scaled):
    for dt in (torch.float32, torch.bfloat16):
        x, rs = R.group_inputs(rows, C, div, mod, scaled, dt)
        for n_chunk in (1, 3, 50):
            ref, b = R.group_rowsum(x.double(), rows, div, mod, None if rs is None else rs.double(), 4, n_chunk)
            out = group_emu(x.float().numpy(), rows, C, div, mod, None if rs is None else rs.numpy(), 4, n_chunk)
            assert worst(out.astype(np.float64).sum(0), ref, b) <= 1.0


def test_mutant_8_group_rowsum_reads_past_the_last_row():
    """(3 * 5 * 16 - 7, 72, 16, 5): the last period is ragged; without the r < rows guard the 7 rows behind the tensor are added."""
    rows, C, div, mod, _ = R.GROUP_CASES[1]
    x, _ = R.group_inputs(rows, C, div, mod, False, torch.float32)
    ref, b = R.group_rowsum(x.double(), rows, div, mod, None, 1, 3)
    padded = torch.cat([x, torch.full((7, C), 3.0)]).numpy()
    assert worst(group_emu(padded, rows, C, div, mod, None, 1, 3).astype(np.float64).sum(0), ref, b) <= 1.0
    assert worst(group_emu(padded, rows, C, div, mod, None, 1, 3, guard=False).astype(np.float64).sum(0), ref, b) > 1.0


@pytest.mark.parametrize("n", [1, 10, 63, 64, 65, 1000])
def test_row_sum_emulation_meets_the_bound(n):
    for rows in (1, 4, 5):
        x = torch.randn(rows, n + 8, generator=torch.Generator().manual_seed(n + rows))
        x[:, n:] = 1.0e6
        for n_chunk in (1, 3):
            ref, b = R.row_sum(x.double(), n, n_chunk)
            out = row_sum_emu(x.numpy(), n, n_chunk)
            assert worst(out.astype(np.float64).sum(0), ref, b) <= 1.0
            if n == 10 and n_chunk == 3:
                assert not out[2].any()                                       # 8-column rounding: chunks of 8, 2, 0 columns
