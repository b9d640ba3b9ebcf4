"""GPU: the small-channel ends of the VQ-VAE (mage_amd/csrc/conv_direct.hip), their backward twins (train.hip) and the gather kernels of the decoder's
input rows (vq.hip) against the fp64 restatements of tests/conv_ref.py (formulas, case tables and the derivation of every per-element bound are in
that module's docstring), at the edges of their dispatch.  The C entry points are called through mage_amd._lib: mage_amd.ops hides ldy, the two
tap counts, the row maps and the relu flags.

Which kernel a call reaches, the host predicate that sends it there, and the cases that reach it:
  conv_in_kernel<float | bf16 | split_bf16 | split_f16>   test_conv_in[case], CONV_IN_GENERIC: everything the image predicate below rejects; the f4 stem
                                                  (1, c, 4, 2, 1) on 6x8 and 7x5, the f8 stem (3, c, 7, 1, 3) on 5x9 (smaller than the filter), cin 4 / 3x3;
                                                  cout 4, 8, 64; bias, scale/shift and ReLU each on and off; the four output kinds; s2d rows on 4x4 and 4x8
                                                  planes in fp32 and split; and the out_* cases of CONV_IN_IMAGE, one outside every term of the predicate
                                                  (N 63, H 5, W 6, W 84, plane 148x80, cout 12, cout 512, bf16 output)
  conv_in_4x4s2_kernel<float | split_bf16 | split_f16>    cin 1, 4x4 / 2 / 1, N >= 64, H even, W % 4 == 0, W <= 80, (H + 2)(W + 2) 4 <= 48 KiB, cout / 4 divides 64,
                                                  fp32 or split output: the img_* cases: N 64 and 65, planes (4,4), (2,4), (6,80), (146,80), cout 4, 64, 256,
                                                  fp32, s2d fp32 and split s2d; each also equal, as values, to the generic kernel run on the same images
                                                  in batches below 64
  conv_out_1x1_c4_kernel                          test_conv_out[1x1_f32_cin4_*]: not transposed, fp32, cin == 4, 16-byte aligned x and weights
  conv_out_1x1_kernel<float>                      test_conv_out[1x1_f32_cin8 | 64 | 68_*]: not transposed, fp32, cin % 4 == 0; 68: a second sweep of one lane
  conv_out_1x1_kernel<bf16>                       test_conv_out[1x1_bf16_cin8 | 128 | 136_*]: bf16, cin % 8 == 0; 136: a second sweep of one lane
  conv_out_kernel<bf16, false>                    test_conv_out[1x1_bf16_cin12_*]: bf16 with cin % 8 != 0 falls through to the wave per pixel
  conv_out_kernel<float | bf16, true>             test_conv_out[t_*]: transposed; cin 4, 64, 256, 260 (a second sweep of one lane), planes (1,1), (2,3), (5,4),
                                                  cout 1 to 4, two images
      (conv_out_kernel<float, false> serves only x or weights that are not 16-byte aligned: no such operand is built here)
      every 1x1 case: 15 or 17 pixels, either side of a 16-pixel workgroup; cout 1 to 4; bias null and given
  convt_fold_tanh_kernel                          test_fold[px_* | fallback_*]: N 1 and 63, cout 1 to 4, planes (1,1), (3,5); at N 64 a 33x32 plane or cout 2
  convt_fold_tanh_img_kernel                      test_fold[img_*]: cout 1, IH IW <= 1024, N >= 64: planes (1,1), (3,5), (32,32), (16,64); bit-identical to the
                                                  per-pixel kernel run on the same images in two batches of 32
  maxpool2_kernel<float | bf16>, upsample2_kernel<float | bf16>   test_pool_upsample[case]: C 4, 8, 260, planes (2,2), (4,6), N 1 and 3, the relu flag
  map_kernel<float | bf16, ., true>               test_relu[kind-n]: n 4, 1020, 1028
  map_kernel<., ., false>                         test_cast[src-dst]: the five pairs, n 4, 1020, 1028 and the edge values of conv_ref.cast_edges
  maxpool2_bwd_kernel, upsample2_bwd_kernel       test_pool_bwd[case]: ties on every pair of window positions, an all-equal window, zeros in dy
  convt_unfold_kernel                             test_unfold[case]: y given and null, cout 1 and 3, planes (1,1) and (3,5)
  table_conv_kernel<TT, OT, VPL>                  test_table_conv[case]: VPL = ceil(C / 256) -> 1 (C 4, 64), 2 (260, 512), 8 (1028, 2048); the seven type pairs and
                                                  the two split outputs; tap windows 1x1, 3x3, 5x5, 1x3, 3x1; planes (1,1), (1,7), (5,3); n_codes 1 and 7;
                                                  pos, bias, rowadd and ReLU each on and off; a group / stride / offset map with ldy = C + 8; rowadd_div 2, mod 3
  table_conv512_kernel<bf16 | f16>                test_table_conv[C512_*_fast]: C == 512, 16-bit table of y's type, ldy % 8 == 0; the *_ldy516 twin (ldy % 8 != 0)
                                                  runs the generic kernel on the same data: test_table_twins holds them bit-identical
  embedding_kernel<float | bf16 | f16 | split_bf16 | split_f16>   test_embedding[case]: C 4, 260, 64; ReLU; one- and two-level row maps with gaps

Every case: each output starts filled with the NaN sentinel of its dtype (tests/helpers.py SENTINEL) with slack past its end and in every gap of its
row map; everything outside the written region must still hold the sentinel, everything inside must have been written and lie within its bound; no
element is exempt.  The exact kernels (pool, upsample, relu, cast, the pool's backward) are compared bit for bit.  Refused calls return MAGE_EINVAL
and leave the outputs untouched."""
import pytest
import torch

from mage_amd import _lib, ops
from tests import conv_ref as R
from tests.helpers import DEV, bits, lib, ptr, refused, sent, unsplit, untouched, within, written

pytestmark = pytest.mark.gpu

CODE = {"f32": ops.F32, "bf16": ops.BF16, "f16": ops.F16, "bf16x3": ops.BF16X3, "f16x3": ops.F16X3}
ESIZE = {"f32": 4, "bf16": 2, "f16": 2, "bf16x3": 4, "f16x3": 4}             # bytes per logical element


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def sync():
    torch.cuda.synchronize()


def out_buf(size, kind):
    return sent(size * (2 if kind in R.SPLIT else 1), R.TORCH_DT[kind])


def logical(raw, kind):
    """The fp64 logical elements of an output buffer brought to the host."""
    if kind in R.SPLIT:
        return unsplit(raw.reshape(-1, 128), CODE[kind]).reshape(-1)
    return raw.double()


def check(entry, name, buf, r, kind):
    raw = buf.cpu()
    m = R.raw_mask(R.footprint(r.size, r.idx), kind)
    assert untouched(raw[~m]), f"{name}: wrote outside its footprint"
    assert written(raw[m]), f"{name}: left part of its footprint unwritten"
    within(entry, name, logical(raw, kind)[r.idx], r.y, r.b)
    return raw


def same_values(raw_a, ra, raw_b, rb, kind, exact):
    """The written elements of two runs agree: bit for bit, or as values (a -0 for a +0 allowed)."""
    ma, mb = R.raw_mask(R.footprint(ra.size, ra.idx), kind), R.raw_mask(R.footprint(rb.size, rb.idx), kind)
    a, b = raw_a[ma], raw_b[mb]
    return torch.equal(bits(a), bits(b)) if exact else torch.equal(a.float(), b.float())


# ------------------------------------------------------------------------------------------------ mage_conv_in
def run_conv_in(c, d, y, n0, n):
    l, s = lib()
    OH, OW = R.conv_in_shape(c)
    per_img = ((OH // 2 + 1) * (OW // 2 + 1) * 4 if c["s2d"] else OH * OW) * c["cout"]
    _lib.check(l.mage_conv_in(d.x[n0:n0 + n].data_ptr(), d.wt.data_ptr(), ptr(d.bias), ptr(d.scale), ptr(d.shift), y.data_ptr() + n0 * per_img * ESIZE[c["kind"]],
                              CODE[c["kind"]], n, c["cin"], c["H"], c["W"], c["cout"], c["k"], c["k"], c["stride"], c["pad"], c["act"], int(c["s2d"]), s), l)


@pytest.mark.parametrize("c", R.CONV_IN_GENERIC + R.CONV_IN_IMAGE, ids=R.case_id)
def test_conv_in(c):
    i = R.with_margin(R.conv_in_inputs, R.conv_in, c)
    r = R.conv_in(c, i)
    d = type(i)(**{k: dev(v) for k, v in vars(i).items()})
    y = out_buf(r.size, c["kind"])
    run_conv_in(c, d, y, 0, c["N"])
    sync()
    raw = check("mage_conv_in", c["name"], y, r, c["kind"])
    if c["path"] == "image":                                                # the same images in batches below 64: the generic kernel
        y2 = out_buf(r.size, c["kind"])
        for n0 in range(0, c["N"], 24):
            run_conv_in(c, d, y2, n0, min(24, c["N"] - n0))
        sync()
        raw2 = check("mage_conv_in", c["name"] + " in batches", y2, r, c["kind"])
        assert same_values(raw, r, raw2, r, c["kind"], exact=False), f"{c['name']}: the image kernel and the generic kernel differ"


# ------------------------------------------------------------------------------------------------ mage_conv_out, mage_convt_fold_tanh
@pytest.mark.parametrize("c", R.CONV_OUT_1X1 + R.CONV_OUT_T, ids=R.case_id)
def test_conv_out(c):
    i = R.conv_out_inputs(c)
    r = R.conv_out(c, i)
    l, s = lib()
    x, wt, bias = dev(i.x), dev(i.wt), dev(i.bias)
    y = out_buf(r.size, "f32")
    _lib.check(l.mage_conv_out(x.data_ptr(), CODE[c["kind"]], wt.data_ptr(), ptr(bias), y.data_ptr(), c["N"], c["IH"], c["IW"], c["cin"], c["cout"],
                               int(c["transposed"]), s), l)
    sync()
    check("mage_conv_out", c["name"], y, r, "f32")


def run_fold(c, taps, bias, y, n0, n):
    l, s = lib()
    per_img = c["cout"] * 4 * c["IH"] * c["IW"]
    _lib.check(l.mage_convt_fold_tanh(taps[n0:n0 + n].data_ptr(), ptr(bias), y.data_ptr() + n0 * per_img * 4, n, c["IH"], c["IW"], c["cout"], s), l)


@pytest.mark.parametrize("c", R.FOLD_CASES, ids=R.case_id)
def test_fold(c):
    i = R.fold_inputs(c)
    r = R.fold(c, i)
    taps, bias = dev(i.taps), dev(i.bias)
    y = out_buf(r.size, "f32")
    run_fold(c, taps, bias, y, 0, c["N"])
    sync()
    raw = check("mage_convt_fold_tanh", c["name"], y, r, "f32")
    if c["path"] == "image":                                                # two batches of 32: the per-pixel kernel
        y2 = out_buf(r.size, "f32")
        run_fold(c, taps, bias, y2, 0, 32)
        run_fold(c, taps, bias, y2, 32, 32)
        sync()
        raw2 = check("mage_convt_fold_tanh", c["name"] + " in batches", y2, r, "f32")
        assert same_values(raw, r, raw2, r, "f32", exact=True), f"{c['name']}: the image kernel and the per-pixel kernel differ"


# ------------------------------------------------------------------------------------------------ the exact kernels
def exact(name, y, want):
    raw = y.cpu()
    n = want.numel()
    assert untouched(raw[n:]), f"{name}: wrote past its end"
    assert written(raw[:n]) and torch.equal(bits(raw[:n]), bits(want.reshape(-1).contiguous())), f"{name}: not bit for bit"


@pytest.mark.parametrize("c", R.POOL_CASES, ids=R.case_id)
def test_pool_upsample(c):
    x = R.pool_inputs(c)
    l, s = lib()
    xd = dev(x)
    N, H, W, C = x.shape
    y = sent(N * (H // 2) * (W // 2) * C + R.TAIL, x.dtype)
    _lib.check(l.mage_maxpool2(xd.data_ptr(), y.data_ptr(), CODE[c["kind"]], N, H, W, C, c["relu"], s), l)
    up = sent(N * 4 * H * W * C + R.TAIL, x.dtype)
    _lib.check(l.mage_upsample2(xd.data_ptr(), up.data_ptr(), CODE[c["kind"]], N, H, W, C, s), l)
    sync()
    exact(c["name"] + " maxpool2", y, R.maxpool2(x, c["relu"]))
    exact(c["name"] + " upsample2", up, R.upsample2(x))


@pytest.mark.parametrize("n", R.MAP_N)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_relu(kind, n):
    x = R.map_inputs(n, kind)
    l, s = lib()
    y, xd = sent(n + R.TAIL, x.dtype), dev(x)
    _lib.check(l.mage_relu(xd.data_ptr(), y.data_ptr(), CODE[kind], n, s), l)
    sync()
    exact(f"relu {kind} {n}", y, x.clamp(min=0))


@pytest.mark.parametrize("src,dst", R.CAST_PAIRS, ids=[f"{a}-{b}" for a, b in R.CAST_PAIRS])
def test_cast(src, dst):
    l, s = lib()
    for x in [R.map_inputs(n, src) for n in R.MAP_N] + [R.cast_edges(src)]:
        y, xd = sent(x.numel() + R.TAIL, R.TORCH_DT[dst]), dev(x)
        _lib.check(l.mage_cast(xd.data_ptr(), CODE[src], y.data_ptr(), CODE[dst], x.numel(), s), l)
        sync()
        exact(f"cast {src} -> {dst} n {x.numel()}", y, x.to(R.TORCH_DT[dst]))


# ------------------------------------------------------------------------------------------------ the backward twins
@pytest.mark.parametrize("c", R.POOL_BWD_CASES, ids=R.case_id)
def test_pool_bwd(c):
    i = R.pool_bwd_inputs(c)
    l, s = lib()
    N, H, W, C = i.x.shape
    dx = sent(i.x.numel() + R.TAIL, torch.float32)
    xd, dyd = dev(i.x), dev(i.dy)
    _lib.check(l.mage_maxpool2_bwd(xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), N, H, W, C, s), l)
    dy = torch.randn(N, H, W, C, generator=R._g("up_bwd", c["name"]))
    du, dud = sent(N * (H // 2) * (W // 2) * C + R.TAIL, torch.float32), dev(dy)
    _lib.check(l.mage_upsample2_bwd(dud.data_ptr(), du.data_ptr(), N, H // 2, W // 2, C, s), l)
    sync()
    exact(c["name"] + " maxpool2_bwd", dx, R.maxpool2_bwd(i.x, i.dy))      # every element written, the zeros included
    ref, b = R.upsample2_bwd(dy.double())
    raw = du.cpu()
    assert untouched(raw[ref.numel():]) and written(raw[:ref.numel()])
    within("mage_upsample2_bwd", c["name"], raw[:ref.numel()].reshape(ref.shape), ref, b)


@pytest.mark.parametrize("c", R.UNFOLD_CASES, ids=R.case_id)
def test_unfold(c):
    i = R.unfold_inputs(c)
    r = R.unfold(c, i)
    l, s = lib()
    dt = out_buf(r.size, "f32")
    gd, yd = dev(i.g), dev(i.y)
    _lib.check(l.mage_convt_unfold_tanh_bwd(gd.data_ptr(), ptr(yd), dt.data_ptr(), c["N"], c["IH"], c["IW"], c["cout"], s), l)
    sync()
    raw = check("mage_convt_unfold_tanh_bwd", c["name"], dt, r, "f32")
    assert not raw[:r.y.numel()].reshape(r.y.shape)[~r.inside].any(), f"{c['name']}: the out-of-image taps are exactly 0"


# ------------------------------------------------------------------------------------------------ mage_table_conv, mage_embedding
_TABLE_RAW = {}


def run_table(c):
    i = R.with_margin(R.table_inputs, R.table_conv, c)
    r = R.table_conv(c, i)
    l, s = lib()
    group, stride, off, ldy = R.table_map(c)
    ids, table, pos, bias, rowadd = dev(i.ids), dev(i.table), dev(i.pos), dev(i.bias), dev(i.rowadd)
    y = out_buf(r.size, c["yk"])
    _lib.check(l.mage_table_conv(ids.data_ptr(), c["n_img"], c["H"], c["W"], c["th"], c["tw"], table.data_ptr(), CODE[c["tk"]], c["n_codes"], c["C"], ptr(pos),
                                 ptr(bias), c["act"], ptr(rowadd), R.ROWADD_DIV, R.ROWADD_MOD, y.data_ptr(), CODE[c["yk"]], ldy, group, stride, off, s), l)
    sync()
    ops.check_device_errors(DEV)
    return check("mage_table_conv", c["name"], y, r, c["yk"]), r


@pytest.mark.parametrize("c", R.TABLE_CASES, ids=R.case_id)
def test_table_conv(c):
    _TABLE_RAW[c["name"]] = run_table(c)


@pytest.mark.parametrize("fast,slow", R.TABLE_TWINS, ids=[a for a, _ in R.TABLE_TWINS])
def test_table_twins(fast, slow):
    by = {c["name"]: c for c in R.TABLE_CASES}
    (ra, a), (rb, b) = (_TABLE_RAW.get(n) or run_table(by[n]) for n in (fast, slow))
    assert same_values(ra, a, rb, b, by[fast]["yk"], exact=True), f"{fast}: the 512-channel kernel and the generic kernel differ"


@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.case_id)
def test_embedding(c):
    i = R.emb_inputs(c)
    r = R.embedding(c, i)
    l, s = lib()
    out = out_buf(r.size, c["kind"])
    ids, table = dev(i.ids), dev(i.table)
    _lib.check(l.mage_embedding(ids.data_ptr(), table.data_ptr(), out.data_ptr(), CODE[c["kind"]], c["n"], c["C"], R.EMB_TABLE, c["relu"], c["group"],
                                c["group_stride"], c["off"], c["inner"], c["inner_stride"], s), l)
    sync()
    ops.check_device_errors(DEV)
    raw = check("mage_embedding", c["name"], out, r, c["kind"])
    if c["kind"] == "f32":
        want = i.table[i.ids].clamp(min=0) if c["relu"] else i.table[i.ids]
        assert torch.equal(bits(raw[r.idx.reshape(-1)]), bits(want.reshape(-1).contiguous())), f"{c['name']}: an fp32 copy is bit for bit"


# ------------------------------------------------------------------------------------------------ refusals
def test_conv_in_refusals():
    l, s = lib()
    x, w, v = torch.randn(4, 4, 8, 8, device=DEV), torch.randn(4 * 49, 64, device=DEV), torch.randn(64, device=DEV)
    y = sent(1 << 16, torch.float32)
    yh = sent(1 << 16, torch.bfloat16)

    def call(N=2, cin=1, H=8, W=8, cout=8, kh=4, kw=4, stride=2, pad=1, act=0, s2d=0, code=ops.F32, scale=None, shift=None, yy=y):
        return lambda: _lib.check(l.mage_conv_in(x.data_ptr(), w.data_ptr(), v.data_ptr(), ptr(scale), ptr(shift), yy.data_ptr(), code, N, cin, H, W, cout, kh, kw,
                                                 stride, pad, act, s2d, s), l)

    call()()                                                                # the baseline itself runs
    sync()
    assert not untouched(y)
    y = sent(1 << 16, torch.float32)
    for kw in (dict(H=0), dict(W=0), dict(H=-8), dict(kh=0), dict(kw=0), dict(kh=-1), dict(pad=-1), dict(cout=0), dict(N=0), dict(stride=0),
               dict(H=2, W=2, kh=7, kw=7, stride=1), dict(H=8, W=2, kh=4, kw=7, stride=1), dict(cin=5), dict(cin=0), dict(cout=6), dict(scale=v), dict(shift=v),
               dict(act=2), dict(H=6, W=8, s2d=1), dict(H=8, W=6, s2d=1), dict(code=ops.F16), dict(code=99)):
        refused(call(yy=y, **kw), y)
    for code in (ops.BF16X3, ops.F16X3):
        refused(call(cout=32, code=code, yy=yh), yh)


def test_conv_out_and_fold_refusals():
    l, s = lib()
    x, w, b = torch.randn(2, 4, 4, 8, device=DEV), torch.randn(64, 8, device=DEV), torch.randn(4, device=DEV)
    y = sent(4096, torch.float32)

    def out(code=ops.F32, N=2, IH=4, IW=4, cin=8, cout=3, tr=0):
        return lambda: _lib.check(l.mage_conv_out(x.data_ptr(), code, w.data_ptr(), b.data_ptr(), y.data_ptr(), N, IH, IW, cin, cout, tr, s), l)

    def fold(N=2, IH=2, IW=2, cout=2):
        return lambda: _lib.check(l.mage_convt_fold_tanh(x.data_ptr(), b.data_ptr(), y.data_ptr(), N, IH, IW, cout, s), l)

    def unfold(N=2, IH=2, IW=2, cout=2):
        return lambda: _lib.check(l.mage_convt_unfold_tanh_bwd(x.data_ptr(), None, y.data_ptr(), N, IH, IW, cout, s), l)

    for tr in (0, 1):
        for kw in (dict(IH=0), dict(IW=0), dict(IH=-4), dict(N=0), dict(cin=6), dict(cin=0), dict(cout=5), dict(cout=0), dict(code=ops.F16)):
            refused(out(tr=tr, **kw), y)
    for f in (fold, unfold):
        for kw in (dict(cout=5), dict(cout=0), dict(IH=0), dict(IW=0), dict(N=0)):
            refused(f(**kw), y)


def test_pool_map_refusals():
    l, s = lib()
    x = torch.randn(4096, device=DEV)
    y, yh = sent(8192, torch.float32), sent(8192, torch.bfloat16)

    def pool(code=ops.F32, N=2, H=4, W=4, C=8):
        return lambda: _lib.check(l.mage_maxpool2(x.data_ptr(), y.data_ptr(), code, N, H, W, C, 0, s), l)

    def up(code=ops.F32, N=2, H=4, W=4, C=8):
        return lambda: _lib.check(l.mage_upsample2(x.data_ptr(), y.data_ptr(), code, N, H, W, C, s), l)

    def pool_bwd(N=2, H=4, W=4, C=8):
        return lambda: _lib.check(l.mage_maxpool2_bwd(x.data_ptr(), x.data_ptr(), y.data_ptr(), N, H, W, C, s), l)

    def up_bwd(N=2, H=4, W=4, C=8):
        return lambda: _lib.check(l.mage_upsample2_bwd(x.data_ptr(), y.data_ptr(), N, H, W, C, s), l)

    for kw in (dict(H=0), dict(W=0), dict(C=0), dict(H=-4), dict(C=-4), dict(N=0), dict(C=6)):
        for f in (pool, up, pool_bwd, up_bwd):
            refused(f(**kw), y)
    for kw in (dict(H=3), dict(W=5)):
        refused(pool(**kw), y)
        refused(pool_bwd(**kw), y)
    for f in (pool, up):
        refused(f(code=ops.F16), y)
    for n in (0, 6, -4):
        refused(lambda: _lib.check(l.mage_relu(x.data_ptr(), y.data_ptr(), ops.F32, n, s), l), y)
        refused(lambda: _lib.check(l.mage_cast(x.data_ptr(), ops.F32, yh.data_ptr(), ops.BF16, n, s), l), yh)
    refused(lambda: _lib.check(l.mage_relu(x.data_ptr(), y.data_ptr(), ops.F16, 64, s), l), y)
    for a, b in ((ops.BF16, ops.BF16), (ops.F16, ops.BF16), (ops.BF16, ops.F16), (ops.F16, ops.F16), (ops.BF16X3, ops.F32), (ops.F32, ops.BF16X3)):
        refused(lambda: _lib.check(l.mage_cast(x.data_ptr(), a, yh.data_ptr(), b, 64, s), l), yh)


def test_table_and_embedding_refusals():
    l, s = lib()
    ids = torch.zeros(64, dtype=torch.int64, device=DEV)
    tab, v = torch.randn(25 * 2 * 64, device=DEV), torch.randn(256, device=DEV)
    y, yh = sent(1 << 14, torch.float32), sent(1 << 14, torch.bfloat16)

    def table(th=3, tw=3, C=64, ldy=64, tk=ops.F32, yk=ops.F32, n_codes=2, n_img=2, H=2, W=2, rowadd=None, div=1, mod=1, group=8, yy=y):
        return lambda: _lib.check(l.mage_table_conv(ids.data_ptr(), n_img, H, W, th, tw, tab.data_ptr(), tk, n_codes, C, None, None, 0, ptr(rowadd), div, mod, yy.data_ptr(),
                                                    yk, ldy, group, group, 0, s), l)

    def emb(C=64, n=8, code=ops.F32, n_table=2, group=8, yy=y):
        return lambda: _lib.check(l.mage_embedding(ids.data_ptr(), tab.data_ptr(), yy.data_ptr(), code, n, C, n_table, 0, group, group, 0, 0, 0, s), l)

    for kw in (dict(th=2), dict(tw=2), dict(th=0), dict(th=4, tw=4), dict(C=6, ldy=8), dict(C=0, ldy=0), dict(C=2052, ldy=2052), dict(ldy=60), dict(ldy=66),
               dict(n_codes=0), dict(n_img=0), dict(H=0), dict(W=0), dict(group=0), dict(rowadd=v, div=0), dict(rowadd=v, mod=0), dict(tk=99), dict(yk=99)):
        refused(table(**kw), y)
    for kw in (dict(tk=ops.BF16, yk=ops.F16), dict(tk=ops.F16, yk=ops.BF16), dict(tk=ops.BF16, yk=ops.BF16X3), dict(tk=ops.F16, yk=ops.F16X3),
               dict(C=32, ldy=32, yk=ops.BF16X3), dict(ldy=128, yk=ops.F16X3)):
        refused(table(yy=yh, **kw), yh)
    for kw in (dict(C=6), dict(C=0), dict(n=0), dict(n_table=0), dict(group=0), dict(code=99)):
        refused(emb(**kw), y)
    for code in (ops.BF16X3, ops.F16X3):
        refused(emb(C=32, code=code, yy=yh), yh)
