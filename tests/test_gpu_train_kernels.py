"""GPU: the norm, loss, scatter and row-sum kernels of the decoder's backward pass (mage_amd/csrc/train.hip, norm.hip) against the fp64
restatements of tests/train_ref.py (formulas and the derivation of every per-element bound are in that module's docstring), at the edges of
their dispatch.  The C entry points are called through mage_amd._lib where mage_amd.ops hides a parameter (n_part, n_chunk, scratch).

Which kernel a call reaches, and the cases that reach it (C ladder: VPL 1: C 4, 252, 256 | 2: 260, 512 | 4: 516, 1024 | 8: 1028, 2044, 2048;
every C but 256, 512, 1024, 2048 leaves the last vector column partly filled):
  layernorm_kernel<float | bf16 | f16, VPL>       test_layernorm[C-kind]: every C, rows 4 or 5 (a ragged last workgroup) and two one-row
                                                  launches (the constant row, the N(64, 1) row); eps 1e-8 at C = 516
  layernorm_kernel<split_bf16 | split_f16, VPL>   test_layernorm_split[C-kind]: C 64, 256, 512, 1024, 2048
  dropout_add_ln_kernel<float, float, VPL>,       test_dropout_add_layernorm[C-pair]: every C, p 0, 0.1, 0.5, 1 - 2^-24, seeds 0 and
    <float, bf16, VPL>, <bf16, bf16, VPL>         0x9E3779B97F4A7C15
  layernorm_bwd_kernel<float | bf16, VPL>         test_layernorm_bwd[C-dy]: every C, accumulate 0 and 1; n_part 1 with 11 rows (three grid-stride
                                                  steps, a wave that runs out of rows), n_part 2 with 11 rows, n_part 5 with 5 rows (three
                                                  workgroups own no row: zero partials); test_layernorm_bwd_dx_bf16[C-p]: C 4, 260, 1028, 2048
  sum_partials_kernel / sum_partials4_kernel      behind dgamma, dbeta: n_part < 4 / n_part 5
  ce_bwd_kernel<float | bf16>                     test_cross_entropy_bwd[shape-kind]: (1, 1), (5, 63), (4, 64), (7, 65), (3, 512), (6, 1000)
  embedding_bwd_kernel<float | bf16>              test_embedding_bwd_atomic: n_table 513; C 72; n 8191 without scratch; (1, 1, 4)
  embedding_bwd_lds_kernel<float | bf16>          test_embedding_bwd_racing_lds: n 8192 and 8197 without scratch; a scratch one float short;
                                                  a scratch 4 bytes off 16-byte alignment
  embedding_bwd_det_kernel<float | bf16> +        test_embedding_bwd_deterministic: n 1, 7, 8, 9, 4096, 4097 (two chunks of 2056 rows), 8200,
    embedding_bwd_reduce_kernel                   64 * 4096 + 1 (64 chunks of 4104 rows); n_table 1, 30, 512; C 64, 192
  group_rowsum_kernel<float | bf16>               test_group_rowsum[case-dt]: a ragged last period, C 72 and 260 (two column blocks), row_scale,
                                                  n_chunk 1, 3, 50 (chunks that own nothing)
  row_sum_kernel<float | bf16>                    test_row_sum[n-dt]: n 1, 63, 64, 65, 1000 and (n 10, n_chunk 3: an empty last chunk), ld = n + 8
The dispatch has no kernel-name query; the embedding cases state the host conditions (n_table <= 512, C % 64 == 0, n >= 8192 or scratch, a
usable scratch) that select each kernel, and the deterministic form is told from the racing one by its bit-exact fixed-order sum.

Every case: each output starts filled with the NaN sentinel of its dtype (tests/helpers.py SENTINEL) with rows or elements past its end;
everything outside the written region must still hold the sentinel, everything inside must have been written and lie within its bound; no
element is exempt.  Refused calls return MAGE_EINVAL and leave the outputs untouched."""
import pytest
import torch

from mage_amd import _lib, ops
from tests import train_ref as R
from tests.helpers import DEV, bits, lib, ptr, refused, sent, untouched, unsplit, within, written

pytestmark = pytest.mark.gpu

GOLD = 0x9E3779B97F4A7C15
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": ops.F32, "bf16": ops.BF16, "f16": ops.F16, "bf16x3": ops.BF16X3, "f16x3": ops.F16X3}
LN_ROWS = {4: 5, 252: 4, 256: 5, 260: 5, 512: 4, 516: 5, 1024: 4, 1028: 5, 2044: 4, 2048: 5, 64: 5}
LN_EPS = {516: 1e-8}


# ------------------------------------------------------------------------------------------------ mage_layernorm
def _layernorm(C, kind, rows, special=None):
    x, gamma, beta = R.ln_inputs(C, rows, 1, special)
    eps = LN_EPS.get(C, 1e-5)
    split = kind.endswith("x3")
    dt = (torch.bfloat16 if kind == "bf16x3" else torch.float16) if split else DT[kind]
    y = sent((rows + 3, 2 * C if split else C), dt)
    l, s = lib()
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    _lib.check(l.mage_layernorm(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), CODE[kind], rows, C, eps, s), l)
    torch.cuda.synchronize()
    assert untouched(y[rows:]) and written(y[:rows]), f"C={C} {kind}: footprint"
    got = unsplit(y[:rows].cpu(), CODE[kind]) if split else y[:rows].cpu()
    ref, b = R.layernorm(x.double(), gamma.double(), beta.double(), eps, kind)
    within("mage_layernorm", f"C={C} rows={rows} {kind} {special or ''}", got, ref, b)
    if kind == "f32" and special != "mean":
        assert torch.equal(got[0], beta), "a constant row has variance 0 exactly: y == beta"


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", R.LN_C)
def test_layernorm(C, kind):
    _layernorm(C, kind, LN_ROWS[C])
    _layernorm(C, kind, 1, "const")
    _layernorm(C, kind, 1, "mean")


@pytest.mark.parametrize("kind", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("C", [64, 256, 512, 1024, 2048])
def test_layernorm_split(C, kind):
    _layernorm(C, kind, LN_ROWS[C])
    _layernorm(C, kind, 1, "mean")


def test_layernorm_refusals():
    l, s = lib()
    x, g = torch.randn(8, 2052, device=DEV), torch.randn(2052, device=DEV)
    y = sent((8, 2 * 2052), torch.float32)
    yh = sent((8, 4 * 2052), torch.bfloat16)

    def call(out, code, rows, C):
        return lambda: _lib.check(l.mage_layernorm(x.data_ptr(), g.data_ptr(), g.data_ptr(), out.data_ptr(), code, rows, C, 1e-5, s), l)
    refused(call(y, ops.F32, 4, 6), y)                                       # C % 4 != 0
    refused(call(y, ops.F32, 4, 2052), y)
    refused(call(y, ops.F32, 0, 256), y)
    refused(call(y, 9, 4, 256), y)                                           # an unknown dtype
    refused(call(yh, ops.BF16X3, 4, 260), yh)                                # split needs C % 64 == 0
    refused(call(yh, ops.F16X3, 4, 260), yh)
    assert yh.data_ptr() % 256 == 0
    refused(call(yh.view(-1)[64:], ops.BF16X3, 4, 256), yh)                  # 128 bytes off a 256-byte boundary
    refused(call(yh.view(-1)[64:], ops.F16X3, 4, 256), yh)


# ------------------------------------------------------------------------------------------------ mage_dropout_add_layernorm
PAIRS = {"f32_f32": ("f32", "f32"), "f32_bf16": ("f32", "bf16"), "bf16_bf16": ("bf16", "bf16")}


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("C", R.LN_C)
def test_dropout_add_layernorm(C, pair):
    xk, yk = PAIRS[pair]
    rows, eps = LN_ROWS[C], LN_EPS.get(C, 1e-5)
    r, gamma, beta = R.ln_inputs(C, rows, 2)
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(C + 1))
    x[0] = 0.0                                                               # r[0] = 0.5: y[0] is constant whatever the mask
    x = x.to(DT[xk])
    l, s = lib()
    xd, rd, gd, bd = x.to(DEV), r.to(DEV), gamma.to(DEV), beta.to(DEV)
    for p in (0.0, 0.1, 0.5, R.P_MAX):
        for seed in (0, GOLD):
            y, yn = sent((rows + 3, C), torch.float32), sent((rows + 3, C), DT[yk])
            _lib.check(l.mage_dropout_add_layernorm(xd.data_ptr(), CODE[xk], rd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), yn.data_ptr(),
                                                    CODE[yk], rows, C, eps, p, seed, s), l)
            torch.cuda.synchronize()
            name = f"C={C} {pair} p={p:.3g} seed={seed:#x}"
            assert untouched(y[rows:]) and untouched(yn[rows:]) and written(y[:rows]) and written(yn[:rows]), f"{name}: footprint"
            keep = R.keep_mask(rows, C, p, seed)
            unf, fus = R.dropout_add_exact(x.float(), r, keep, R.inv_keep(p))
            yc = y[:rows].cpu()
            assert torch.equal(bits(yc), bits(unf)) or torch.equal(bits(yc), bits(fus)), \
                f"{name}: y is neither the rounded-product nor the fused r + x / (1 - p) under the reference mask " \
                f"({int((bits(yc) != bits(unf)).sum())} / {int((bits(yc) != bits(fus)).sum())} elements differ)"
            ref, b = R.layernorm(yc.double(), gamma.double(), beta.double(), eps, yk)
            within("mage_dropout_add_layernorm", name, yn[:rows].cpu(), ref, b)
            if yk == "f32":
                assert torch.equal(yn[0].cpu(), beta)


def test_dropout_add_layernorm_refusals():
    l, s = lib()
    x, xb = torch.randn(4, 256, device=DEV), torch.randn(4, 256, device=DEV).bfloat16()
    g = torch.randn(256, device=DEV)
    y, yn, ynb = sent((4, 256), torch.float32), sent((4, 512), torch.float32), sent((4, 512), torch.bfloat16)

    def call(xx, xc, out, oc, p):
        return lambda: _lib.check(l.mage_dropout_add_layernorm(xx.data_ptr(), xc, x.data_ptr(), y.data_ptr(), g.data_ptr(), g.data_ptr(), out.data_ptr(), oc,
                                                               4, 256, 1e-5, p, 1, s), l)
    refused(call(xb, ops.BF16, yn, ops.F32, 0.1), y, yn)                     # bf16 x with fp32 yn
    refused(call(x, ops.F32, ynb, ops.BF16X3, 0.1), y, ynb)                  # a split yn
    refused(call(x, ops.F32, ynb, ops.F16X3, 0.1), y, ynb)
    refused(call(x, ops.F32, yn, ops.F32, 1.0), y, yn)
    refused(call(x, ops.F32, yn, ops.F32, -0.1), y, yn)


# ------------------------------------------------------------------------------------------------ mage_layernorm_bwd
def _ln_bwd(C, rows, n_part, dyk, acc, p=0.0, seed=0, with_bf16=False, eps=None):
    """One launch + mage_sum_partials; returns the CPU copies (dx buffer, partials buffer, gb buffer, dx_bf16 buffer) and the inputs."""
    eps = LN_EPS.get(C, 1e-5) if eps is None else eps
    x, gamma, _ = R.ln_inputs(C, rows, 3)
    g = torch.Generator().manual_seed(C * 3 + rows)
    dy = torch.randn(rows, C, generator=g).to(DT[dyk])
    start = torch.randn(rows, C, generator=g)
    dx = sent((rows + 3, C), torch.float32)
    if acc:
        dx[:rows] = start.to(DEV)
    part = sent((n_part + 1, 2, C), torch.float32)
    gb = sent(2 * C + 8, torch.float32)
    dxb = sent((rows + 3, C), torch.bfloat16) if with_bf16 else None
    l, s = lib()
    xd, gd, dyd = x.to(DEV), gamma.to(DEV), dy.to(DEV)
    _lib.check(l.mage_layernorm_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), CODE[dyk], dx.data_ptr(), part.data_ptr(), n_part, rows, C, eps,
                                    int(acc), ptr(dxb), p, seed, s), l)
    _lib.check(l.mage_sum_partials(part.data_ptr(), 2 * C, n_part, 2 * C, gb.data_ptr(), 0, s), l)
    torch.cuda.synchronize()
    return (dx.cpu(), part.cpu(), gb.cpu(), None if dxb is None else dxb.cpu()), (x, gamma, dy, start if acc else None, eps)


def _check_ln_bwd(C, rows, n_part, dyk, acc):
    (dx, part, gb, _), (x, gamma, dy, start, eps) = _ln_bwd(C, rows, n_part, dyk, acc)
    name = f"C={C} rows={rows} n_part={n_part} dy={dyk} acc={int(acc)}"
    assert untouched(dx[rows:]) and written(dx[:rows]) and untouched(part[n_part:]) and written(part[:n_part]) and untouched(gb[2 * C:]), f"{name}: footprint"
    for b in range(-(-rows // 4), n_part):
        assert not part[b].any(), f"{name}: workgroup {b} owns no row, its partials must be exactly 0"
    r = R.layernorm_bwd(x.double(), gamma.double(), dy.double(), eps, n_part, None if start is None else start.double())
    within("mage_layernorm_bwd", name + " dx", dx[:rows], r.dx, r.b_dx)
    within("mage_layernorm_bwd", name + " dgamma", gb[:C], r.dg, r.b_dg)
    within("mage_layernorm_bwd", name + " dbeta", gb[C:2 * C], r.db, r.b_db)
    (dx2, part2, gb2, _), _ = _ln_bwd(C, rows, n_part, dyk, acc)
    assert torch.equal(bits(dx), bits(dx2)) and torch.equal(bits(part), bits(part2)) and torch.equal(bits(gb), bits(gb2)), f"{name}: two launches differ"


@pytest.mark.parametrize("dyk", ["f32", "bf16"])
@pytest.mark.parametrize("C", R.LN_C)
def test_layernorm_bwd(C, dyk):
    rows = LN_ROWS[C]
    _check_ln_bwd(C, rows, -(-rows // 4), dyk, False)
    _check_ln_bwd(C, rows, -(-rows // 4), dyk, True)
    _check_ln_bwd(C, 1, 1, dyk, False)
    _check_ln_bwd(C, 11, 1, dyk, dyk == "f32")
    _check_ln_bwd(C, 11, 2, dyk, dyk == "bf16")
    _check_ln_bwd(C, 5, 5, dyk, False)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("C", [4, 260, 1028, 2048])
def test_layernorm_bwd_dx_bf16(C, p):
    """dx_bf16 is the bf16 rounding of the dx the kernel wrote, through the reference mask; dx, dgamma, dbeta do not depend on it."""
    rows = 5
    for acc in (False, True):
        (dx, part, gb, dxb), _ = _ln_bwd(C, rows, 2, "bf16", acc, p=p, seed=GOLD, with_bf16=True)
        (dx0, part0, gb0, _), _ = _ln_bwd(C, rows, 2, "bf16", acc)
        assert untouched(dxb[rows:]) and written(dxb[:rows])
        assert torch.equal(bits(dx), bits(dx0)) and torch.equal(bits(part), bits(part0)) and torch.equal(bits(gb), bits(gb0))
        want = dx[:rows]
        if p > 0:
            want = torch.where(R.keep_mask(rows, C, p, GOLD), want * float(R.inv_keep(p)), torch.zeros_like(want))
        assert torch.equal(bits(dxb[:rows]), bits(want.to(torch.bfloat16))), f"C={C} p={p} acc={acc}: dx_bf16"


def test_layernorm_bwd_refusals():
    l, s = lib()
    x, g = torch.randn(8, 2052, device=DEV), torch.randn(2052, device=DEV)
    dx, part, dxb = sent((8, 2052), torch.float32), sent((3, 2, 2052), torch.float32), sent(8 * 2052 + 8, torch.bfloat16)

    def call(C, n_part, p, b16=None):
        return lambda: _lib.check(l.mage_layernorm_bwd(x.data_ptr(), g.data_ptr(), x.data_ptr(), ops.F32, dx.data_ptr(), part.data_ptr(), n_part, 4, C, 1e-5, 0,
                                                       ptr(b16), p, 1, s), l)
    refused(call(6, 1, 0.0), dx, part)
    refused(call(2052, 1, 0.0), dx, part)
    refused(call(256, 0, 0.0), dx, part)
    refused(call(256, 1, 1.0, dxb), dx, part, dxb)
    refused(call(256, 1, 0.1, dxb[1:]), dx, part, dxb)                       # 2 bytes off 8-byte alignment


# ------------------------------------------------------------------------------------------------ mage_cross_entropy_bwd
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("rows,K", R.CE_SHAPES)
def test_cross_entropy_bwd(rows, K, kind):
    z, tg = R.ce_inputs(rows, K)
    out = sent((rows + 3, K), DT[kind])
    go = torch.tensor([R.CE_GRAD_OUT], device=DEV)
    l, s = lib()
    zd, td = z.to(DEV), tg.to(DEV)
    _lib.check(l.mage_cross_entropy_bwd(zd.data_ptr(), td.data_ptr(), rows, K, go.data_ptr(), out.data_ptr(), CODE[kind], s), l)
    torch.cuda.synchronize()
    assert untouched(out[rows:]) and written(out[:rows])
    got = out[:rows].cpu()
    ref, b = R.cross_entropy_bwd(z.double(), tg, R.CE_GRAD_OUT, kind)
    within("mage_cross_entropy_bwd", f"rows={rows} K={K} {kind}", got, ref, b)
    assert bool((got[torch.isinf(z)] == 0).all()), "a -inf logit has probability 0 and gradient 0 exactly"


def test_cross_entropy_bwd_refusals():
    l, s = lib()
    z, tg, go = torch.randn(4, 64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), torch.ones(1, device=DEV)
    out = sent((4, 64), torch.float32)
    refused(lambda: _lib.check(l.mage_cross_entropy_bwd(z.data_ptr(), tg.data_ptr(), 4, 64, go.data_ptr(), out.data_ptr(), ops.F16, s), l), out)
    refused(lambda: _lib.check(l.mage_cross_entropy_bwd(z.data_ptr(), tg.data_ptr(), 4, 64, go.data_ptr(), out.data_ptr(), 9, s), l), out)
    refused(lambda: _lib.check(l.mage_cross_entropy_bwd(z.data_ptr(), tg.data_ptr(), 0, 64, go.data_ptr(), out.data_ptr(), ops.F32, s), l), out)


# ------------------------------------------------------------------------------------------------ mage_embedding_bwd
TAIL = 64


def _embedding(n, n_table, C, dk, grouped, scratch="none", launches=1):
    """scratch: 'none' | 'exact' (sentinel tail) | 'short' (one float short) | 'misaligned' (the right size, 4 bytes off 16).  Returns the
    dtable results of `launches` launches (CPU, [n_table, C]) and the inputs."""
    ids, dout, start, orow, (group, stride, off), pad = R.emb_inputs(n, n_table, C, DT[dk], grouped)
    n_chunk, _ = R.emb_chunks(n)
    need = n_chunk * n_table * C
    idd, dd = ids.to(DEV), dout.to(DEV)
    l, s = lib()
    res = []
    for _ in range(launches):
        tab = sent(n_table * C + TAIL, torch.float32)
        tab[:n_table * C] = start.reshape(-1).to(DEV)
        sc, sf = None, 0
        if scratch == "exact":
            buf = sent(need + TAIL, torch.float32)
            sc, sf = buf, need
        elif scratch == "short":
            buf = sent(need + TAIL, torch.float32)
            sc, sf = buf, need - 1
        elif scratch == "misaligned":
            buf = sent(need + TAIL, torch.float32)
            sc, sf = buf[1:], need
            assert sc.data_ptr() % 16 == 4
        _lib.check(l.mage_embedding_bwd(idd.data_ptr(), dd.data_ptr(), CODE[dk], tab.data_ptr(), n, C, n_table, pad, group, stride, off, ptr(sc), sf, s), l)
        torch.cuda.synchronize()
        assert untouched(tab[n_table * C:]) and written(tab[:n_table * C]), "dtable footprint"
        if scratch == "exact":
            assert untouched(buf[need:]), "the deterministic form wrote past n_chunk * n_table * C floats of scratch"
        elif scratch != "none":
            assert untouched(buf), "an unusable scratch was written"
        res.append(tab[:n_table * C].cpu().reshape(n_table, C))
    return res, (ids, dout.double()[orow], start, n_table, pad)


def _emb_bound(entry_case, got, ids, rows_read, start, n_table, pad):
    ref, b = R.embedding_bwd(ids, rows_read, start.double(), n_table, pad)
    within("mage_embedding_bwd", entry_case, got, ref, b)


@pytest.mark.parametrize("n,n_table,C,dk,grouped", [(500, 513, 64, "f32", True), (500, 30, 72, "bf16", True), (8191, 512, 64, "bf16", False),
                                                    (8191, 512, 64, "f32", True), (1, 1, 4, "f32", False), (500, 513, 64, "bf16", False)])
def test_embedding_bwd_atomic(n, n_table, C, dk, grouped):
    """embedding_bwd_kernel: a table over 512 rows, C % 64 != 0, or n < 8192 without scratch."""
    assert n_table > 512 or C % 64 or n < 8192
    (got,), inp = _embedding(n, n_table, C, dk, grouped)
    _emb_bound(f"atomic n={n} n_table={n_table} C={C} {dk} grouped={grouped}", got, *inp)


@pytest.mark.parametrize("n,n_table,C,dk,grouped,scratch", [(8192, 512, 64, "f32", True, "none"), (8192, 512, 64, "bf16", False, "none"),
                                                            (8197, 30, 128, "bf16", True, "none"), (8197, 30, 128, "f32", False, "none"),
                                                            (300, 512, 64, "f32", True, "short"), (9000, 64, 64, "bf16", True, "misaligned")])
def test_embedding_bwd_racing_lds(n, n_table, C, dk, grouped, scratch):
    """embedding_bwd_lds_kernel: a small table with n >= 8192 and no scratch, or a scratch too short or misaligned to be used."""
    assert n_table <= 512 and C % 64 == 0 and (n >= 8192 or scratch != "none")
    (got,), inp = _embedding(n, n_table, C, dk, grouped, scratch)
    _emb_bound(f"racing n={n} n_table={n_table} C={C} {dk} grouped={grouped} scratch={scratch}", got, *inp)


@pytest.mark.parametrize("n,n_table,C,dk,grouped", [(1, 1, 64, "f32", False), (7, 30, 64, "bf16", True), (8, 30, 192, "f32", False), (9, 512, 64, "f32", True),
                                                    (4096, 30, 64, "bf16", False), (4097, 30, 64, "f32", True), (8200, 512, 192, "bf16", True),
                                                    (8200, 1, 64, "f32", True), (64 * 4096 + 1, 30, 64, "bf16", False)])
def test_embedding_bwd_deterministic(n, n_table, C, dk, grouped):
    """embedding_bwd_det_kernel + embedding_bwd_reduce_kernel (an exact scratch): every (code, channel) equals the float32 sum in the order
    the header states, bit for bit; three launches agree; the fp64 bound holds."""
    res, inp = _embedding(n, n_table, C, dk, grouped, "exact", launches=3)
    want = R.embedding_det_f32(*inp)
    diff = bits(res[0]) != bits(want)
    assert not bool(diff.any()), f"{int(diff.sum())} entries differ from the fixed-order float32 sum (first at {diff.nonzero()[:4].tolist()})"
    assert torch.equal(bits(res[0]), bits(res[1])) and torch.equal(bits(res[0]), bits(res[2])), "launches differ"
    _emb_bound(f"deterministic n={n} n_table={n_table} C={C} {dk} grouped={grouped}", res[0], *inp)


def test_embedding_bwd_refusals():
    l, s = lib()
    ids = torch.zeros(16, dtype=torch.int64, device=DEV)
    dout = torch.randn(64, 64, device=DEV)
    tab = sent(513 * 64, torch.float32)

    def call(n, group, code, n_table):
        return lambda: _lib.check(l.mage_embedding_bwd(ids.data_ptr(), dout.data_ptr(), code, tab.data_ptr(), n, 64, n_table, -1, group, group, 0, None, 0, s), l)
    refused(call(0, 16, ops.F32, 30), tab)
    refused(call(16, 0, ops.F32, 30), tab)
    refused(call(16, 16, ops.F16, 513), tab)
    refused(call(16, 16, 9, 513), tab)


# ------------------------------------------------------------------------------------------------ mage_group_rowsum
@pytest.mark.parametrize("dk", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C,div,mod,scaled", R.GROUP_CASES)
def test_group_rowsum(rows, C, div, mod, scaled, dk):
    x, rs = R.group_inputs(rows, C, div, mod, scaled, DT[dk])
    xd = torch.cat([x, torch.full((16, C), 1.0e6, dtype=x.dtype)]).to(DEV)  # rows behind the tensor that would show if they were summed
    rsd = None if rs is None else rs.to(DEV)
    l, s = lib()
    total = -(-rows // (div * mod)) * div
    for n_chunk in (1, 3, 50):
        outs = []
        for _ in range(2):
            out = sent(n_chunk * mod * C + TAIL, torch.float32)
            _lib.check(l.mage_group_rowsum(xd.data_ptr(), CODE[dk], rows, C, div, mod, ptr(rsd), 4 if scaled else 1, out.data_ptr(), n_chunk, s), l)
            torch.cuda.synchronize()
            assert untouched(out[n_chunk * mod * C:]) and written(out[:n_chunk * mod * C])
            outs.append(out[:n_chunk * mod * C].cpu().reshape(n_chunk, mod, C))
        assert torch.equal(bits(outs[0]), bits(outs[1])), "launches differ"
        per = -(-total // n_chunk)
        for z in range(n_chunk):
            if z * per >= total:
                assert not outs[0][z].any(), f"chunk {z} of {n_chunk} owns nothing: its slice must be exactly 0"
        ref, b = R.group_rowsum(x.double(), rows, div, mod, None if rs is None else rs.double(), 4, n_chunk)
        within("mage_group_rowsum", f"rows={rows} C={C} div={div} mod={mod} {dk} n_chunk={n_chunk}", outs[0].double().sum(0), ref, b)


def test_group_rowsum_refusals():
    l, s = lib()
    x, rs = torch.randn(32, 64, device=DEV), torch.randn(32, device=DEV)
    out = sent(4 * 64, torch.float32)

    def call(n_chunk, scale, rs_div):
        return lambda: _lib.check(l.mage_group_rowsum(x.data_ptr(), ops.F32, 32, 64, 2, 4, ptr(scale), rs_div, out.data_ptr(), n_chunk, s), l)
    refused(call(0, None, 1), out)
    refused(call(65536, None, 1), out)
    refused(call(1, rs, 0), out)


# ------------------------------------------------------------------------------------------------ mage_row_sum
@pytest.mark.parametrize("dk", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 10, 63, 64, 65, 1000])
def test_row_sum(n, dk):
    l, s = lib()
    for rows in (1, 4, 5):
        x = torch.randn(rows, n + 8, generator=torch.Generator().manual_seed(n + rows))
        x[:, n:] = 1.0e6                                                     # the gap columns up to ld
        x = x.to(DT[dk])
        xd = x.to(DEV)
        for n_chunk in (1, 3):
            outs = []
            for _ in range(2):
                out = sent(n_chunk * rows + TAIL, torch.float32)
                _lib.check(l.mage_row_sum(xd.data_ptr(), CODE[dk], n + 8, n, rows, out.data_ptr(), n_chunk, s), l)
                torch.cuda.synchronize()
                assert untouched(out[n_chunk * rows:]) and written(out[:n_chunk * rows])
                outs.append(out[:n_chunk * rows].cpu().reshape(n_chunk, rows))
            assert torch.equal(bits(outs[0]), bits(outs[1])), "launches differ"
            per = R.row_chunk(n, n_chunk)
            for z in range(n_chunk):
                if z * per >= n:
                    assert not outs[0][z].any(), f"n={n}: chunk {z} of {n_chunk} is empty, it must be exactly 0"
            if n == 10 and n_chunk == 3:
                assert per == 8 and not outs[0][2].any()
            ref, b = R.row_sum(x.double(), n, n_chunk)
            within("mage_row_sum", f"n={n} rows={rows} {dk} n_chunk={n_chunk}", outs[0].double().sum(0), ref, b)
