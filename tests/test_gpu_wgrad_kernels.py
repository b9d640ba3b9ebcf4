"""GPU: the weight-gradient, activation, dropout and Adam kernels of the training path (mage_amd/csrc/train.hip, optim.hip, gemm_tn.hip, gemm4.hip) against
the fp64 restatements of tests/wgrad_ref.py (formulas and the derivation of every per-element bound are in that module's docstring), at the
edges of their dispatch.  The C entry points are called through mage_amd._lib, which shows every parameter (n_split, tokens_per_split, n_part).

Which kernel a call reaches, the host condition that selects it, and the cases that reach it:
  transpose_kernel<float>            mage_transpose, MAGE_F32: test_transpose[f32_*]: C 8, 12, 64, 72 (a ragged second column block) x (M, Mp)
                                     (1, 8), (63, 64), (64, 64), (65, 72), (65, 128); (1, 1); y_row0 5 with ldy 80 > Mp; regrouped rows; the nine
                                     3x3 taps on a 3 x 5 plane of 2 images; the sixteen 4x4 taps with stride 2 from 6 x 10 onto 3 x 5
  transpose8_kernel                  MAGE_BF16 with C % 8 == 0, ldx % 8 == 0, ldy % 8 == 0, Mp % 8 == 0, x and y 16-byte aligned:
                                     test_transpose[bf16_*] at C 8, 64, 72 and Mp 8, 64, 72, 128, row0_ldy, regroup, taps3x3, taps4x4_s2
  transpose_kernel<bf16>             MAGE_BF16 otherwise: C 12 (every (M, Mp); the 4x4 taps), Mp 1, and one case per condition:
                                     bf16_fallback_ldx (ldx 68), _ldy (ldy 76), _Mp (Mp 68), _x_off, _y_off (2 bytes off)
  transpose8_colsum_kernel           mage_transpose_colsum: test_transpose_colsum: Mp 64, 1024 (one part of 16 tiles), 1032 (a second part of one
                                     8-column tile), M = Mp and Mp - 7, C 8 and 72, regrouped rows; every colsum row against its own group
  gemm_tn_kernel (8 waves)           mage_gemm_tn with T % 64 != 0, tokens_per_split < 128 or a last slice under 128 tokens:
                                     test_gemm_tn[8w-*]: (T, tps, n_split) (1, 64, 1), (63, 64, 1), (64, 64, 1), (65, 64, 2) (a slice of one
                                     token), (64, 64, 3) (two empty slices: exact zeros), (192, 128, 2) (a last slice of 64); and every 4w case once
                                     more under the library option gemm_no_4w
  gemm_tn4_kernel<true | false>      otherwise (whole slabs, two or more per slice): test_gemm_tn[4w-*]: (128, 128, 1), (256, 128, 2),
                                     (320, 192, 2) (3 slabs, then 2); <false> is db_partials null (test_gemm_tn_operands)
                                     each x (N, K) (256, 256), (512, 256), (256, 512); test_gemm_tn_operands: lda = N + 8, ldb = K + 8, bases 16
                                     bytes into their buffers; db_partials null -- on both kernels
  colsum_kernel                      mage_colsum: test_colsum: C 8, 512, 520 (a second column block of one lane) x T 1, 3, 4, 5, 16, 17, 67
                                     (n_part 1: both sides of the unrolled loop's t + 12 < t1), (T 10, n_part 3), (T 3, n_part 5: empty chunks)
  sum_partials_kernel                mage_sum_partials with n % 4 != 0, stride % 4 != 0, n_part < 4 or part / out off 16-byte alignment:
                                     test_sum_partials: n 250; n_part 1, 3; stride 254; out 4 bytes off
  sum_partials4_kernel               otherwise: n 4, 252, 260 x n_part 4, 5, 13, 16, 17, 20 (from 13 on the unrolled loop runs for some waves
                                     only), stride 260 > n 252; accumulate 0 and 1 everywhere
  act_kernel<float | bf16, ACT, 0>   mage_act: test_act[dt]: ReLU, QuickGELU, erf-GELU x n 4, 1020, 1024 (a full workgroup), 1028
  act_kernel<float | bf16, ACT, 1>   mage_act_bwd: the same and tanh
  dropout_kernel<T, YT>              mage_dropout: test_dropout[pair-n]: the four dtype pairs x n 4, 1020, 1028 x p 0, 0.1, 0.5, 1 - 2^-24 x seeds
                                     0, 0x9E3779B97F4A7C15 x accumulate 0, 1
  dropout_add_kernel<float | bf16>   mage_dropout_add: test_dropout_add[x-n]: the same p, seeds and n, with and without y_bf16
  adam_kernel                        mage_adam: test_adam[n-step]: n 1, 3, 4, 5, 1023, 1024, 1027 (tails of 1, 2, 3 elements; both sides of the
                                     grid step at 1024) x steps 1, 2, 1000, 100000 (four consecutive steps each) x grad_scale 1, 0.125, 1 / 3 x
                                     (0.9, 0.98, 1e-6), (0.9, 0.999, 1e-8)
The dispatch has no kernel-name query for these entry points: the cases state the host conditions, asserted from wgrad_ref's restatement of
them (tcase's kernel, gemm_4w, sp_vector); the two GEMM kernels are told apart by the gemm_no_4w option, under which they must give equal bits.

Every case: each output starts filled with the NaN sentinel of its dtype (tests/helpers.py SENTINEL) with rows or elements past its end;
everything outside the written region must still hold the sentinel, everything inside must have been written and lie within its bound (or
equal the reference's bits, for the transposes, the fixed-order sums and dropout); no element is exempt.  Refused calls return MAGE_EINVAL
and leave the outputs untouched; only arguments that the host code checks are used."""
import pytest
import torch

from mage_amd import _lib, config, ops
from tests import train_ref as TR
from tests import wgrad_ref as R
from tests.helpers import DEV, SENTINEL, bits, lib, ptr, refused, sent, untouched, within, written

pytestmark = pytest.mark.gpu

DT = R.TDT
CODE = {"f32": ops.F32, "bf16": ops.BF16}
ACT_CODE = {"relu": 1, "quickgelu": 2, "gelu_erf": 3, "tanh": 4}              # MAGE_ACT_* of include/mage_hip.h
TAIL = 8


def sync():
    torch.cuda.synchronize()


def geo_args(M, out_h=1, out_w=None, in_h=None, in_w=None, img_stride=None, a_off=0, dy=0, dx=0, stride=1):
    """The header's defaults: a plain transpose is out_h = 1, out_w = M, no shift, stride 1, the input plane the output plane."""
    out_w = M if out_w is None else out_w
    in_h = out_h if in_h is None else in_h
    in_w = out_w if in_w is None else in_w
    return out_h, out_w, in_h, in_w, in_h * in_w if img_stride is None else img_stride, a_off, dy, dx, stride


# ------------------------------------------------------------------------------------------------ mage_transpose
@pytest.mark.parametrize("c", R.TRANSPOSE_CASES, ids=lambda c: c.name)
def test_transpose(c):
    """Bits of y against the indexed gather, -0.0, a NaN payload, +-inf and a subnormal among them; the whole buffer around y keeps the sentinel."""
    dt = DT[c.dt]
    xb = R.transpose_inputs(c)
    want = R.transpose_expected(c, xb, SENTINEL[dt][1])
    xflat = torch.zeros(c.x_rows * c.ldx + c.x_off + 8, dtype=xb.dtype)
    xflat[c.x_off:c.x_off + xb.numel()] = xb.reshape(-1)
    xd = xflat.to(DEV).view(dt)
    yflat = sent(want.numel() + c.y_off + 16, dt)
    x_ptr, y_ptr = xd[c.x_off:].data_ptr(), yflat[c.y_off:].data_ptr()
    aligned = x_ptr % 16 == 0 and y_ptr % 16 == 0
    t8 = c.dt == "bf16" and c.C % 8 == 0 and c.ldx % 8 == 0 and c.ldy % 8 == 0 and c.Mp % 8 == 0 and aligned
    assert c.kernel == ("transpose8_kernel" if t8 else "transpose_kernel<%s>" % ("bf16" if c.dt == "bf16" else "float")), "the case's host condition"
    l, s = lib()
    for r0, geo in c.calls:
        _lib.check(l.mage_transpose(x_ptr, CODE[c.dt], c.ldx, y_ptr, c.ldy, r0, c.M, c.Mp, c.C, *geo_args(c.M, **geo), s), l)
    sync()
    full = torch.full((yflat.numel(),), SENTINEL[dt][1], dtype=xb.dtype)
    full[c.y_off:c.y_off + want.numel()] = want.reshape(-1)
    diff = bits(yflat.cpu()) != full
    assert not bool(diff.any()), f"{c.name} ({c.kernel}): {int(diff.sum())} elements differ from the gather (first flat indices {diff.nonzero()[:6].flatten().tolist()})"


def test_transpose_refusals():
    l, s = lib()
    x = torch.randn(64, 64, device=DEV)
    y = sent((64, 64), torch.float32)
    yh = sent((64, 64), torch.float16)

    def call(out=y, code=ops.F32, ldx=64, ldy=64, M=32, Mp=32, C=64, stride=1):
        return lambda: _lib.check(l.mage_transpose(x.data_ptr(), code, ldx, out.data_ptr(), ldy, 0, M, Mp, C, 1, M if M > 0 else 1, 1, M if M > 0 else 1,
                                                   M, 0, 0, 0, stride, s), l)
    refused(call(Mp=31), y)                                                  # Mp < M
    refused(call(ldy=24), y)                                                 # ldy < Mp
    refused(call(stride=0), y)
    refused(call(M=0), y)
    refused(call(code=9), y)                                                 # an unknown dtype
    refused(call(out=yh, code=ops.F16), yh)
    refused(call(ldx=56), y)                                                 # ldx < C: rows would alias
    yb = sent((64, 64), torch.bfloat16)
    refused(call(out=yb, code=ops.BF16, ldx=56), yb)


# ------------------------------------------------------------------------------------------------ mage_transpose_colsum
def _transpose_colsum(c):
    xb = R.tc_inputs(c)
    n_part = R.tc_n_part(c.Mp)
    xd = xb.to(DEV).view(torch.bfloat16)
    y, cs = sent((c.C + 3, c.Mp), torch.bfloat16), sent((n_part + 1, c.C), torch.float32)
    out_h, out_w, _, _, img_stride, a_off, _, _, _ = geo_args(c.M, **c.geo)
    l, s = lib()
    _lib.check(l.mage_transpose_colsum(xd.data_ptr(), c.C, y.data_ptr(), c.Mp, c.M, c.Mp, c.C, out_w, img_stride, a_off, cs.data_ptr(),
                                       n_part, s), l)
    sync()
    return xb, y.cpu(), cs.cpu(), n_part


@pytest.mark.parametrize("c", R.TC_CASES, ids=lambda c: c.name)
def test_transpose_colsum(c):
    xb, y, cs, n_part = _transpose_colsum(c)
    want = torch.full((c.C + 3, c.Mp), SENTINEL[torch.bfloat16][1], dtype=torch.int16)
    want[:c.C] = R.transpose(xb, c.M, c.Mp, c.C, **c.geo)
    assert torch.equal(bits(y), want), f"{c.name}: y differs from the gather, or rows past C were written"
    assert untouched(cs[n_part:]) and written(cs[:n_part]), f"{c.name}: colsum footprint"
    ref, b = R.transpose_colsum(xb.view(torch.bfloat16).double(), c.M, c.Mp, c.C, **c.geo)
    for p in range(n_part):
        within("mage_transpose_colsum", f"{c.name} part {p}", cs[p], ref[p], b[p])
    _, y2, cs2, _ = _transpose_colsum(c)
    assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(cs), bits(cs2)), f"{c.name}: two launches differ"


def test_transpose_colsum_refusals():
    l, s = lib()
    xf = torch.randn(64 * 72 + 16, device=DEV).bfloat16()
    yf, cs = sent(64 * 72 + 16, torch.bfloat16), sent((2, 64), torch.float32)

    def call(x=xf, y=yf, ldx=64, ldy=64, Mp=64, C=64, n_part=1):
        return lambda: _lib.check(l.mage_transpose_colsum(x.data_ptr(), ldx, y.data_ptr(), ldy, 60, Mp, C, 60, 60, 0, cs.data_ptr(), n_part, s), l)
    refused(call(n_part=2), yf, cs)                                          # n_part must be ceil(ceil(Mp / 64) / 16)
    refused(call(n_part=0), yf, cs)
    refused(call(C=60, ldx=64), yf, cs)                                      # C % 8
    refused(call(ldx=68), yf, cs)                                            # ldx % 8
    refused(call(ldy=68), yf, cs)                                            # ldy % 8
    refused(call(Mp=68, ldy=72), yf, cs)                                     # Mp % 8
    refused(call(x=xf[1:]), yf, cs)                                          # x 2 bytes off
    refused(call(y=yf[1:]), yf, cs)                                          # y 2 bytes off
    refused(call(ldy=56), yf, cs)                                            # ldy < Mp
    refused(call(ldx=56), yf, cs)                                            # ldx < C: rows would alias


# ------------------------------------------------------------------------------------------------ mage_gemm_tn
def _gemm_tn(T, N, K, tps, n_split, pad=0, off=0, with_db=True):
    """One launch; returns the CPU copies of the partials [n_split + 1, N, K] and db [n_split + 1, N] buffers (one sentinel slice each) and
    the operands as stored.  pad: lda = N + pad, ldb = K + pad; off: elements by which both bases sit inside their buffers."""
    dy, x = R.gemm_inputs(T, N, K, pad)
    dyf, xf = torch.zeros(dy.numel() + off, dtype=torch.bfloat16), torch.zeros(x.numel() + off, dtype=torch.bfloat16)
    dyf[off:], xf[off:] = dy.reshape(-1), x.reshape(-1)
    dyd, xd = dyf.to(DEV), xf.to(DEV)
    P = sent((n_split + 1, N, K), torch.float32)
    db = sent((n_split + 1, N), torch.float32)
    l, s = lib()
    _lib.check(l.mage_gemm_tn(dyd[off:].data_ptr(), N + pad, xd[off:].data_ptr(), K + pad, T, N, K, n_split, tps, P.data_ptr(), ptr(db if with_db else None), s), l)
    sync()
    return P.cpu(), db.cpu(), dy, x


def _check_gemm_tn(T, N, K, tps, n_split, **kw):
    P, db, dy, x = _gemm_tn(T, N, K, tps, n_split, **kw)
    name = f"T={T} N={N} K={K} tps={tps} n_split={n_split} {kw or ''}"
    with_db = kw.get("with_db", True)
    assert untouched(P[n_split:]) and written(P[:n_split]), f"{name}: partials footprint"
    assert untouched(db[n_split:]) and (written(db[:n_split]) if with_db else untouched(db)), f"{name}: db footprint"
    r = R.gemm_tn(dy[:T, :N].double(), x[:T, :K].double(), T, tps, n_split)
    for s_ in range(n_split):
        within("mage_gemm_tn", f"{name} slice {s_} dW", P[s_], r.P[s_], r.bP[s_])
        if with_db:
            within("mage_gemm_tn", f"{name} slice {s_} db", db[s_], r.db[s_], r.bdb[s_])
        if s_ * tps >= T:
            assert not P[s_].any() and (not with_db or not db[s_].any()), f"{name}: slice {s_} holds no token, its partials and db row must be exactly 0"
    return P, db


@pytest.mark.parametrize("T,tps,n_split", R.GEMM_8W + R.GEMM_4W, ids=[("4w-" if R.gemm_4w(*c) else "8w-") + "-".join(map(str, c)) for c in R.GEMM_8W + R.GEMM_4W])
@pytest.mark.parametrize("N,K", R.GEMM_NK)
def test_gemm_tn(N, K, T, tps, n_split):
    assert R.gemm_4w(T, tps, n_split) == ((T, tps, n_split) in R.GEMM_4W), "the case's host condition"
    P, db = _check_gemm_tn(T, N, K, tps, n_split)
    if R.gemm_4w(T, tps, n_split):
        with config.lib_option("gemm_no_4w", 1):
            P8, db8 = _check_gemm_tn(T, N, K, tps, n_split)
        assert torch.equal(bits(P), bits(P8)) and torch.equal(bits(db), bits(db8)), "the 8-wave and the one-wave-per-SIMD kernel differ"


@pytest.mark.parametrize("T,tps,n_split", [(65, 64, 2), (320, 192, 2)])
def test_gemm_tn_operands(T, tps, n_split):
    _check_gemm_tn(T, 512, 256, tps, n_split, pad=8, off=8)                  # lda = N + 8, ldb = K + 8, both bases 16 bytes into their buffers
    P, _ = _check_gemm_tn(T, 256, 512, tps, n_split, with_db=False)
    P1, _ = _check_gemm_tn(T, 256, 512, tps, n_split)
    assert torch.equal(bits(P), bits(P1)), "the partials depend on db_partials"


def test_gemm_tn_refusals():
    l, s = lib()
    a = torch.randn(256 * 520 + 16, device=DEV).bfloat16()
    P, db = sent((2, 256, 256), torch.float32), sent((2, 256), torch.float32)

    def call(dy=a, x=a, out=None, lda=256, ldb=256, T=128, N=256, K=256, n_split=2, tps=64):
        out = P.view(-1) if out is None else out
        return lambda: _lib.check(l.mage_gemm_tn(dy.data_ptr(), lda, x.data_ptr(), ldb, T, N, K, n_split, tps, out.data_ptr(), db.data_ptr(), s), l)
    refused(call(N=128), P, db)                                              # N % 256
    refused(call(K=384), P, db)                                              # K % 256
    refused(call(lda=260), P, db)                                            # lda % 8
    refused(call(ldb=260), P, db)
    refused(call(lda=248), P, db)                                            # lda < N
    refused(call(ldb=248), P, db)
    refused(call(tps=96, n_split=2), P, db)                                  # tokens_per_split % 64
    refused(call(T=129), P, db)                                              # n_split * tokens_per_split < T
    refused(call(dy=a[4:]), P, db)                                           # dY 8 bytes off
    refused(call(x=a[4:]), P, db)                                            # X 8 bytes off
    refused(call(out=P.view(-1)[2:]), P, db)                                 # partials 8 bytes off
    refused(call(T=0), P, db)
    refused(call(n_split=0), P, db)


# ------------------------------------------------------------------------------------------------ mage_colsum
@pytest.mark.parametrize("C,T,n_part", R.COLSUM_CASES)
def test_colsum(C, T, n_part):
    x = R.colsum_inputs(C, T)
    xd = x.to(DEV)
    l, s = lib()
    outs = []
    for _ in range(2):
        part = sent((n_part + 1, C), torch.float32)
        _lib.check(l.mage_colsum(xd.data_ptr(), C + 8, T, C, part.data_ptr(), n_part, s), l)
        sync()
        assert untouched(part[n_part:]) and written(part[:n_part]), "partials footprint"
        outs.append(part[:n_part].cpu())
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two launches differ"
    ref, b = R.colsum(x[:T, :C].double(), T, n_part)
    per = R.cdiv(T, n_part)
    for p in range(n_part):
        within("mage_colsum", f"C={C} T={T} n_part={n_part} chunk {p}", outs[0][p], ref[p], b[p])
        if p * per >= T:
            assert not outs[0][p].any(), f"chunk {p} of {n_part} owns no row: exact zeros"
    if (T, n_part) == (3, 5):
        assert not outs[0][3:].any()


def test_colsum_refusals():
    l, s = lib()
    x = torch.randn(16 * 72 + 16, device=DEV).bfloat16()
    part = sent((2, 64), torch.float32)

    def call(xx=x, out=None, ld=72, C=64, n_part=1, T=16):
        out = part.view(-1) if out is None else out
        return lambda: _lib.check(l.mage_colsum(xx.data_ptr(), ld, T, C, out.data_ptr(), n_part, s), l)
    refused(call(C=60), part)                                                # C % 8
    refused(call(ld=68), part)                                               # ld % 8
    refused(call(n_part=0), part)
    refused(call(xx=x[1:]), part)                                            # x 2 bytes off
    refused(call(out=part.view(-1)[1:]), part)                               # partials 4 bytes off
    refused(call(T=0), part)
    refused(call(ld=56), part)                                               # ld < C: rows would alias


# ------------------------------------------------------------------------------------------------ mage_sum_partials
def _sum_partials(n, stride, n_part, out_off):
    part, start = R.sp_inputs(n, stride, n_part)
    pd = part.to(DEV)
    vec = R.sp_vector(n, stride, n_part, out_off)
    l, s = lib()
    for acc in (0, 1):
        flat = sent(n + out_off + TAIL, torch.float32)
        out = flat[out_off:out_off + n]
        assert (pd.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0) == (out_off % 4 == 0)
        if acc:
            out.copy_(start.to(DEV))
        _lib.check(l.mage_sum_partials(pd.data_ptr(), stride, n_part, n, out.data_ptr(), acc, s), l)
        sync()
        name = f"n={n} stride={stride} n_part={n_part} out_off={out_off} acc={acc} ({'sum_partials4_kernel' if vec else 'sum_partials_kernel'})"
        assert untouched(flat[:out_off]) and untouched(flat[out_off + n:]) and written(out), f"{name}: footprint"
        st = start if acc else None
        ref, b = R.sum_partials(part.double(), n, None if st is None else st.double())
        got = out.cpu()
        within("mage_sum_partials", name, got, ref, b)
        want = R.sum_partials_f32(part, n, st, vec)
        diff = bits(got) != bits(want)
        assert not bool(diff.any()), f"{name}: {int(diff.sum())} elements differ from the float32 sum in the stated order (first at {diff.nonzero()[:4].flatten().tolist()})"


@pytest.mark.parametrize("n_part", R.SP_NPART)
def test_sum_partials(n_part):
    for n in R.SP_N:
        _sum_partials(n, n, n_part, 0)
    for e in R.SP_EXTRA:
        _sum_partials(e["n"], e["stride"], n_part, e["out_off"])


def test_sum_partials_refusals():
    l, s = lib()
    part, out = torch.randn(4, 64, device=DEV), sent(64, torch.float32)
    refused(lambda: _lib.check(l.mage_sum_partials(part.data_ptr(), 64, 0, 64, out.data_ptr(), 0, s), l), out)
    refused(lambda: _lib.check(l.mage_sum_partials(part.data_ptr(), 64, 4, 0, out.data_ptr(), 0, s), l), out)


# ------------------------------------------------------------------------------------------------ mage_act, mage_act_bwd
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_act(dt):
    l, s = lib()
    for n in R.ACT_N:
        for x, dy in R.act_inputs(n, dt):
            xd, dyd = x.to(DEV), dy.to(DEV)
            for kind in R.ACTS_BWD:
                for bwd in ((0, 1) if kind != "tanh" else (1,)):
                    y = sent(n + TAIL, DT[dt])
                    if bwd:
                        _lib.check(l.mage_act_bwd(xd.data_ptr(), dyd.data_ptr(), y.data_ptr(), CODE[dt], n, ACT_CODE[kind], s), l)
                        ref, e = R.act_bwd(x.double(), dy.double(), kind)
                    else:
                        _lib.check(l.mage_act(xd.data_ptr(), y.data_ptr(), CODE[dt], n, ACT_CODE[kind], s), l)
                        ref, e = R.act(x.double(), kind)
                    sync()
                    assert untouched(y[n:]) and written(y[:n]), f"{kind} n={n} {dt} bwd={bwd}: footprint"
                    within("mage_act_bwd" if bwd else "mage_act", f"{kind} n={n} {dt} x[1]={float(x[1]):g}", y[:n].cpu(), ref, e if dt == "f32" else R.bf16_bound(ref, e))


def test_act_refusals():
    l, s = lib()
    x = torch.randn(64, device=DEV)
    y, yh = sent(64, torch.float32), sent(64, torch.float16)
    for bwd in (0, 1):
        def call(out=y, code=ops.F32, n=64, act=1):
            if bwd:
                return lambda: _lib.check(l.mage_act_bwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), code, n, act, s), l)
            return lambda: _lib.check(l.mage_act(x.data_ptr(), out.data_ptr(), code, n, act, s), l)
        refused(call(n=62), y)                                               # n % 4
        refused(call(n=0), y)
        refused(call(act=9), y)                                              # an unknown activation
        refused(call(act=0), y)
        refused(call(out=yh, code=ops.F16), yh)
        refused(call(code=9), y)
    refused(lambda: _lib.check(l.mage_act(x.data_ptr(), y.data_ptr(), ops.F32, 64, ACT_CODE["tanh"], s), l), y)      # tanh forward is not here


# ------------------------------------------------------------------------------------------------ mage_dropout, mage_dropout_add
def _exact(got, unf, fus, name):
    """got equals the rounded-product or the fused value everywhere (both already in got's dtype)."""
    a, b = bits(got) != bits(unf), bits(got) != bits(fus)
    assert not bool(a.any()) or not bool(b.any()), f"{name}: neither the rounded-product nor the fused r + x / (1 - p) under the reference mask " \
                                                   f"({int(a.sum())} / {int(b.sum())} elements differ, first at {a.nonzero()[:4].flatten().tolist()})"


@pytest.mark.parametrize("n", R.DROP_N)
@pytest.mark.parametrize("xk,yk", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16")])
def test_dropout(xk, yk, n):
    l, s = lib()
    for p in R.DROP_P:
        for seed in R.DROP_SEEDS:
            x, r = R.drop_inputs(n, seed)
            x, r = x.to(DT[xk]), r.to(DT[yk])
            xd = x.to(DEV)
            keep = TR.keep_mask(1, n, p, seed)[0]
            for acc in (0, 1):
                y = sent(n + TAIL, DT[yk])
                if acc:
                    y[:n] = r.to(DEV)
                _lib.check(l.mage_dropout(xd.data_ptr(), CODE[xk], y.data_ptr(), CODE[yk], n, p, seed, acc, s), l)
                sync()
                name = f"{xk}->{yk} n={n} p={p:.3g} seed={seed:#x} acc={acc}"
                assert untouched(y[n:]) and written(y[:n]), f"{name}: footprint"
                got = y[:n].cpu()
                prev = r.float() if acc else torch.zeros(n)
                unf, fus = TR.dropout_add_exact(x.float(), prev, keep, TR.inv_keep(p))
                _exact(got, unf.to(DT[yk]), fus.to(DT[yk]), name)
                if not acc:
                    nz = x.float() != 0
                    wrong = ((got.float() == 0) != ~keep) & nz
                    assert not bool(wrong.any()), f"{name}: the dropped set differs from keep_mask at {wrong.nonzero()[:6].flatten().tolist()}"


@pytest.mark.parametrize("n", R.DROP_N)
@pytest.mark.parametrize("xk", ["f32", "bf16"])
def test_dropout_add(xk, n):
    l, s = lib()
    for p in R.DROP_P:
        for seed in R.DROP_SEEDS:
            x, r = R.drop_inputs(n, seed)
            x = x.to(DT[xk])
            xd, rd = x.to(DEV), r.to(DEV)
            keep = TR.keep_mask(1, n, p, seed)[0]
            unf, fus = TR.dropout_add_exact(x.float(), r, keep, TR.inv_keep(p))
            for with_b in (False, True):
                y, yb = sent(n + TAIL, torch.float32), sent(n + TAIL, torch.bfloat16)
                _lib.check(l.mage_dropout_add(xd.data_ptr(), CODE[xk], rd.data_ptr(), y.data_ptr(), ptr(yb if with_b else None), n, p, seed, s), l)
                sync()
                name = f"{xk} n={n} p={p:.3g} seed={seed:#x} y_bf16={with_b}"
                assert untouched(y[n:]) and written(y[:n]) and untouched(yb[n:]) and (written(yb[:n]) if with_b else untouched(yb)), f"{name}: footprint"
                got = y[:n].cpu()
                _exact(got, unf, fus, name)
                dropped = bits(got) == bits(r)
                assert bool(dropped[~keep].all()), f"{name}: a dropped element is not the residual's bits"
                if with_b:
                    assert torch.equal(bits(yb[:n].cpu()), bits(got.to(torch.bfloat16))), f"{name}: y_bf16 is not the bf16 rounding of y"


def test_dropout_refusals():
    l, s = lib()
    x, xh = torch.randn(64, device=DEV), torch.randn(64, device=DEV).half()
    y, yb = sent(64, torch.float32), sent(72, torch.bfloat16)

    def drop(xx=x, xc=ops.F32, n=64, p=0.1):
        return lambda: _lib.check(l.mage_dropout(xx.data_ptr(), xc, y.data_ptr(), ops.F32, n, p, 1, 0, s), l)

    def add(xx=x, xc=ops.F32, n=64, p=0.1, b16=None):
        return lambda: _lib.check(l.mage_dropout_add(xx.data_ptr(), xc, x.data_ptr(), y.data_ptr(), ptr(b16), n, p, 1, s), l)
    for call in (drop, add):
        refused(call(n=62), y, yb)                                           # n % 4
        refused(call(n=0), y, yb)
        refused(call(p=-0.1), y, yb)
        refused(call(p=1.0), y, yb)
        refused(call(p=float("nan")), y, yb)
        refused(call(xx=xh, xc=ops.F16), y, yb)                              # the (f16, f32) pair
        refused(call(xc=9), y, yb)
    refused(add(b16=yb[1:]), y, yb)                                          # y_bf16 2 bytes off 8-byte alignment


# ------------------------------------------------------------------------------------------------ mage_adam
def _arena(t, n):
    a = sent(n + TAIL, torch.float32)
    a[:n] = t.to(DEV)
    return a


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam(n, step):
    """Four consecutive steps per (grad_scale, hyperparameters); each step against the reference fed the state the kernel read."""
    l, s = lib()
    for gs in R.ADAM_SCALES:
        for b1, b2, eps in R.ADAM_HYPER:
            p, g, m, v, idx = R.adam_inputs(n, step, b1, b2)
            pa, ma, va, gd = _arena(p, n), _arena(m, n), _arena(v, n), g.to(DEV)
            for k in range(4):
                _lib.check(l.mage_adam(pa.data_ptr(), gd.data_ptr(), ma.data_ptr(), va.data_ptr(), n, R.ADAM_LR, b1, b2, eps, step + k, gs, s), l)
                sync()
                name = f"n={n} step={step + k} grad_scale={gs:.3g} betas=({b1}, {b2}) eps={eps:g}"
                for a in (pa, ma, va):
                    assert untouched(a[n:]) and written(a[:n]), f"{name}: footprint"
                r = R.adam(p.double(), g.double(), m.double(), v.double(), R.ADAM_LR, b1, b2, eps, step + k, gs)
                p1, m1, v1 = pa[:n].cpu(), ma[:n].cpu(), va[:n].cpu()
                within("mage_adam", name + " p", p1, r.p, r.bp)
                within("mage_adam", name + " m", m1, r.m, r.bm)
                within("mage_adam", name + " v", v1, r.v, r.bv)
                if idx.zero is not None:
                    assert int(bits(p1)[idx.zero]) == int(bits(p)[idx.zero]) and float(m1[idx.zero]) == 0 and float(v1[idx.zero]) == 0, \
                        f"{name}: g = m = v = 0 must leave p bit-identical"
                p, m, v = p1, m1, v1


def test_adam_refusals():
    l, s = lib()
    g = torch.randn(72, device=DEV)
    p, m, v = sent(72, torch.float32), sent(72, torch.float32), sent(72, torch.float32)

    def call(pp=p, gg=g, mm=m, vv=v, n=64, step=1):
        return lambda: _lib.check(l.mage_adam(pp.data_ptr(), gg.data_ptr(), mm.data_ptr(), vv.data_ptr(), n, 1e-3, 0.9, 0.98, 1e-6, step, 1.0, s), l)
    refused(call(step=0), p, m, v)
    refused(call(n=0), p, m, v)
    refused(call(pp=p[1:]), p, m, v)                                         # each arena 4 bytes off 16-byte alignment
    refused(call(gg=g[1:]), p, m, v)
    refused(call(mm=m[1:]), p, m, v)
    refused(call(vv=v[1:]), p, m, v)
