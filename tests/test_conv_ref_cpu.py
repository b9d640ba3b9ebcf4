"""CPU: the fp64 restatements and bounds of tests/conv_ref.py, without a GPU.  For every case table: the kernel's arithmetic emulated in torch
fp32 in the kernel's summation order (separately rounded products: a correct implementation with or without contraction) sits inside the
bound and has the reference's footprint, and every ReLU case keeps its sign margin; every reference agrees with torch's own fp64 conv2d,
conv_transpose2d, max_pool2d, interpolate and embedding, and with autograd through them; and a list of plausible indexing mistakes (MUTANTS)
falls outside the bound or the footprint on a named case each."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

F32, F64 = torch.float32, torch.float64


def stored(x, kind):
    """The fp64 value an fp32 x has after a store of `kind` (split pieces as mage_amd/csrc/common.h builds them)."""
    if kind == "f32":
        return x.double()
    if kind in ("bf16", "f16"):
        return x.to(R.TORCH_DT[kind]).double()
    if kind == "bf16x3":
        hi = x.to(torch.bfloat16).float()
        return hi.double() + (x - hi).to(torch.bfloat16).double()
    x = x.clamp(-65504.0, 65504.0)
    hi = x.to(torch.float16).float()
    return hi.double() + ((x - hi) * 2048.0).to(torch.float16).double() / 2048.0


def scatter(r_size, idx, vals):
    buf = torch.full((r_size,), float("nan"), dtype=F64)
    buf[idx.reshape(-1)] = vals.reshape(-1)
    return buf


def inside(c, buf, r, what=""):
    ok, worst = R.verdict(buf, r)
    assert ok, f"{c['name']}{what}: footprint"
    assert worst <= 1.0, f"{c['name']}{what}: the fp32 emulation is {worst:.3f} of the bound"
    return worst


def outside(c, buf, r):
    ok, worst = R.verdict(buf, r)
    return (not ok) or worst > 1.0


# ------------------------------------------------------------------------------------------------ emulations
def emu_conv_in(c, i, mutant=None):
    P = R.patches(i.x, c["k"], c["stride"], c["pad"])
    wt, T = i.wt, i.wt.shape[0]
    if mutant == "kykx":
        wt = wt.reshape(c["cin"], c["k"], c["k"], c["cout"]).transpose(1, 2).reshape(T, c["cout"])
    acc = (i.bias if i.bias is not None else torch.zeros(c["cout"])).expand(P.shape[0], P.shape[1], c["cout"])
    for t in range(T):
        acc = acc + P[..., t:t + 1] * wt[t]
    if i.scale is not None:
        acc = acc * i.scale + i.shift
    if c["act"]:
        acc = acc.clamp(min=0)
    idx, size = R.conv_in_layout(c, swap=mutant == "quadrant")
    return scatter(size, idx, stored(acc, c["kind"]))


def lane_sums(p, nl, cpl, acc=None, skip_last=False):
    """p [..., cin] fp32 products -> the per-lane sums [..., nl]: lane l takes the chunks of cpl channels at l cpl + nl cpl j, and adds every
    float4 of a chunk left to right onto its sum."""
    cin, per = p.shape[-1], nl * cpl
    J = -(-cin // per)
    p = F.pad(p, (0, J * per - cin)).reshape(*p.shape[:-1], J, nl, cpl // 4, 4)
    if acc is None:
        acc = torch.zeros(*p.shape[:-4], nl)
    for j in range(J):
        if skip_last and j == J - 1 and cin % per:
            continue
        for q in range(cpl // 4):
            v = p[..., j, :, q, :]
            acc = acc + (((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])
    return acc


def butterfly(v, offs):
    lanes = torch.arange(v.shape[-1])
    for o in offs:
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def emu_conv_out(c, i, mutant=None):
    x, w, cout, cin = i.x.float(), i.wt, c["cout"], c["cin"]
    N, IH, IW = c["N"], c["IH"], c["IW"]
    bias = i.bias if i.bias is not None else torch.zeros(cout)
    if c["transposed"]:
        w = w.reshape(16, cout, cin)
        acc = None
        for iy, ix, tap, v in R.fold_index(IH, IW):
            xg = x[:, iy, ix] * v[None, :, :, None].float()                 # [N, OH, OW, cin]
            p = xg[:, :, :, None, :] * w[tap][None]                         # [N, OH, OW, cout, cin]
            acc = lane_sums(p, 64, 4, acc)
        s = butterfly(acc, (32, 16, 8, 4, 2, 1))
    else:
        p = x[:, :, :, None, :] * w[None, None, None]                       # [N, IH, IW, cout, cin]
        cpl = 8 if c["kind"] == "bf16" else 4
        if cin % cpl == 0:                                                  # 16 lanes per pixel (one of them at cin = 4: the thread-per-pixel kernel)
            acc = bias[:, None].expand(N, IH, IW, cout, 16) if mutant == "bias_first" else None
            s = butterfly(lane_sums(p, 16, cpl, acc, skip_last=mutant == "skip_sweep"), (1, 2, 4, 8))
            if mutant == "bias_first":
                bias = torch.zeros(cout)
        else:
            s = butterfly(lane_sums(p, 64, 4), (32, 16, 8, 4, 2, 1))
    y = torch.tanh(s + bias).permute(0, 3, 1, 2)
    r = R.conv_out(c, i)
    return scatter(r.size, r.idx, y.double())


def emu_fold(c, i, mutant=None):
    tp = i.taps.reshape(c["N"], c["IH"], c["IW"], 16, c["cout"])
    s = (i.bias if i.bias is not None else torch.zeros(c["cout"]))[None, :, None, None]
    for t in R.fold_terms(tp, parity=mutant == "parity"):
        s = s + t
    r = R.fold(c, i)
    return scatter(r.size, r.idx, torch.tanh(s).double())


def emu_table(c, i, **mutant):
    acc = None
    for t in R.table_terms(c, i, dt=F32, **mutant):
        acc = t if acc is None else acc + t
    if c["act"]:
        acc = acc.clamp(min=0)
    idx, size = R.table_layout(c)
    return scatter(size, idx, stored(acc, c["yk"]))


# ------------------------------------------------------------------------------------------------ the emulation inside every bound
@pytest.mark.parametrize("c", R.CONV_IN_GENERIC + R.CONV_IN_IMAGE, ids=R.case_id)
def test_conv_in(c):
    i = R.with_margin(R.conv_in_inputs, R.conv_in, c)
    r = R.conv_in(c, i)
    if c["act"]:
        assert R.margin(r) > 4
    inside(c, emu_conv_in(c, i), r)
    OH, OW = R.conv_in_shape(c)
    w = i.wt.double().T.reshape(c["cout"], c["cin"], c["k"], c["k"])
    t = F.conv2d(i.x.double(), w, None if i.bias is None else i.bias.double(), stride=c["stride"], padding=c["pad"])
    assert tuple(t.shape[2:]) == (OH, OW)
    if i.scale is not None:
        t = t * i.scale.double()[None, :, None, None] + i.shift.double()[None, :, None, None]
    torch.testing.assert_close(r.t, t.permute(0, 2, 3, 1).reshape(r.t.shape), rtol=1e-12, atol=1e-12)
    if c["s2d"]:                                                            # the rows are what a 2x2 / stride-1 window over blocks reads
        BH, BW = OH // 2 + 1, OW // 2 + 1
        buf = torch.zeros(r.size, dtype=F64)
        buf[r.idx.reshape(-1)] = r.y.reshape(-1)
        blocks = buf[:c["N"] * BH * BW * 4 * c["cout"]].reshape(c["N"], BH, BW, 2, 2, c["cout"])
        full = blocks.permute(0, 1, 3, 2, 4, 5).reshape(c["N"], 2 * BH, 2 * BW, c["cout"])               # the plane with a one-pixel zero border
        torch.testing.assert_close(full[:, 1:OH + 1, 1:OW + 1], r.y.reshape(c["N"], OH, OW, c["cout"]), rtol=0, atol=0)
        assert not full[:, 0].any() and not full[:, :, 0].any() and not full[:, OH + 1:].any() and not full[:, :, OW + 1:].any()


@pytest.mark.parametrize("c", R.CONV_OUT_1X1 + R.CONV_OUT_T, ids=R.case_id)
def test_conv_out(c):
    i = R.conv_out_inputs(c)
    r = R.conv_out(c, i)
    inside(c, emu_conv_out(c, i), r)
    x = i.x.double().permute(0, 3, 1, 2)
    b = None if i.bias is None else i.bias.double()
    if c["transposed"]:
        w = i.wt.double().reshape(4, 4, c["cout"], c["cin"]).permute(3, 2, 0, 1)
        pre = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    else:
        pre = F.conv2d(x, i.wt.double()[:, :, None, None], b)
    torch.testing.assert_close(r.pre, pre, rtol=1e-12, atol=1e-12)


def selection(cout):
    """conv_transpose2d weights [16 cout, cout, 4, 4] under which the taps themselves are the input channels."""
    w = torch.zeros(16, cout, cout, 4, 4, dtype=F64)
    for t in range(16):
        for co in range(cout):
            w[t, co, co, t >> 2, t & 3] = 1
    return w.reshape(16 * cout, cout, 4, 4)


@pytest.mark.parametrize("c", R.FOLD_CASES, ids=R.case_id)
def test_fold(c):
    i = R.fold_inputs(c)
    r = R.fold(c, i)
    inside(c, emu_fold(c, i), r)
    pre = F.conv_transpose2d(i.taps.double().permute(0, 3, 1, 2), selection(c["cout"]), None if i.bias is None else i.bias.double(), stride=2, padding=1)
    torch.testing.assert_close(r.pre, pre, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", R.POOL_CASES, ids=R.case_id)
def test_pool_upsample(c):
    x = R.pool_inputs(c)
    nchw = x.float().permute(0, 3, 1, 2)
    want = F.max_pool2d(nchw, 2)
    want = (want.clamp(min=0) if c["relu"] else want).permute(0, 2, 3, 1)
    assert torch.equal(R.maxpool2(x, c["relu"]).float(), want)
    assert torch.equal(R.upsample2(x).float(), F.interpolate(nchw, scale_factor=2, mode="nearest").permute(0, 2, 3, 1))


def test_cast_edges():
    for src, dst in R.CAST_PAIRS:
        x = R.cast_edges(src)
        assert x.numel() % 4 == 0 and not torch.isnan(x.float()).any()
        y = x.to(R.TORCH_DT[dst])
        assert not torch.isnan(y.float()).any()
    x = R.cast_edges("f32")
    h, b = x.to(torch.float16), x.to(torch.bfloat16)
    assert float(h[x == 65519.0]) == 65504.0 and bool(torch.isinf(h[x == 65520.0]).all()) and float(h[x == 2.0 ** -25]) == 0.0
    assert float(h[x == 3 * 2.0 ** -25]) == 2.0 ** -23 and float(b[x == 1 + 2.0 ** -8]) == 1.0 and float(b[x == 1 + 3 * 2.0 ** -8]) == 1 + 2.0 ** -6
    assert float(b[x == 3 * 2.0 ** -134]) == 2.0 ** -132 and bool(torch.isinf(b[x == 3.4e38]).all())


@pytest.mark.parametrize("c", R.POOL_BWD_CASES, ids=R.case_id)
def test_pool_bwd(c):
    i = R.pool_bwd_inputs(c)
    win = i.x.reshape(c["N"], c["H"] // 2, 2, c["W"] // 2, 2, c["C"])
    ties = (win == win.amax((2, 4), keepdim=True)).sum((2, 4))
    assert bool((ties == 2).any()) and bool((ties == 4).any())
    first = win.permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    tied = first[(first == first.amax(1, keepdim=True)).sum(1) == 2]
    for k in range(4):                                                      # a tie placed at each of the four window positions
        assert bool((tied[:, k] == tied.amax(1)).any())
    x = i.x.double().permute(0, 3, 1, 2).requires_grad_()
    F.max_pool2d(x, 2).backward(i.dy.double().permute(0, 3, 1, 2))
    dx = R.maxpool2_bwd(i.x, i.dy)
    assert torch.equal(dx.double(), x.grad.permute(0, 2, 3, 1)) and bool((dx == 0).any())
    dy = torch.randn(c["N"], c["H"], c["W"], c["C"], generator=R._g("up_bwd", c["name"]))
    ref, b = R.upsample2_bwd(dy.double())
    w = dy.reshape(c["N"], c["H"] // 2, 2, c["W"] // 2, 2, c["C"])
    emu = (w[:, :, 0, :, 0] + w[:, :, 0, :, 1]) + (w[:, :, 1, :, 0] + w[:, :, 1, :, 1])
    assert bool(((emu.double() - ref).abs() <= b).all())
    xs = torch.zeros(c["N"], c["C"], c["H"] // 2, c["W"] // 2, dtype=F64, requires_grad=True)
    F.interpolate(xs, scale_factor=2, mode="nearest").backward(dy.double().permute(0, 3, 1, 2))
    torch.testing.assert_close(ref, xs.grad.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("c", R.UNFOLD_CASES, ids=R.case_id)
def test_unfold(c):
    i = R.unfold_inputs(c)
    r = R.unfold(c, i)
    emu = R.unfold(c, i, dt=F32).y.double()
    inside(c, scatter(r.size, r.idx, emu), r)
    assert not emu[~r.inside].any() and not r.b[~r.inside].any() and bool((~r.inside).any())
    v = i.g.double() * (1 - i.y.double() ** 2) if i.y is not None else i.g.double()
    taps = torch.zeros(c["N"], 16 * c["cout"], c["IH"], c["IW"], dtype=F64, requires_grad=True)
    F.conv_transpose2d(taps, selection(c["cout"]), stride=2, padding=1).backward(v)
    torch.testing.assert_close(r.y, taps.grad.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("c", R.TABLE_CASES, ids=R.case_id)
def test_table_conv(c):
    i = R.with_margin(R.table_inputs, R.table_conv, c)
    r = R.table_conv(c, i)
    if c["act"]:
        assert R.margin(r) > 4
    inside(c, emu_table(c, i), r)
    assert (c["C"] + 255) // 256 in (1, 2, 5, 8)


@pytest.mark.parametrize("th,tw", [(1, 1), (3, 3), (5, 5), (1, 3), (3, 1)])
def test_table_conv_is_a_convolution_of_embeddings(th, tw):
    c = R._tc("conv", 8, th, tw, 5, 3, 7, "f32", "f32", n_img=2)
    g = R._g("emb_conv", th, tw)
    emb, w = torch.randn(7, 3, generator=g, dtype=F64), torch.randn(8, 3, th, tw, generator=g, dtype=F64)
    i = R.table_inputs(c)
    i.table = torch.einsum("oiyx,ki->yxko", w, emb).reshape(th * tw, 7, 8)
    want = F.conv2d(emb[i.ids].permute(0, 3, 1, 2), w, padding=(th // 2, tw // 2)).permute(0, 2, 3, 1).reshape(-1, 8)
    torch.testing.assert_close(sum(R.table_terms(c, i)), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.case_id)
def test_embedding(c):
    i = R.emb_inputs(c)
    r = R.embedding(c, i)
    v = F.embedding(i.ids, i.table)
    inside(c, scatter(r.size, r.idx, stored(v.clamp(min=0) if c["relu"] else v, c["kind"])), r)
    rows = R.emb_rows(c)
    assert rows.unique().numel() == c["n"]


# ------------------------------------------------------------------------------------------------ mutants
def _case(table, name):
    return next(c for c in table if c["name"] == name)


def m_fold_parity():
    c = _case(R.FOLD_CASES, "px_n1_c2_3x5")
    i = R.fold_inputs(c)
    return outside(c, emu_fold(c, i, "parity"), R.fold(c, i))


def m_kykx():
    c = _case(R.CONV_IN_GENERIC, "cin4_3x3_c8")
    i = R.conv_in_inputs(c)
    return outside(c, emu_conv_in(c, i, "kykx"), R.conv_in(c, i))


def m_skip_sweep():
    out = []
    for kind, cin in (("f32", 68), ("bf16", 136)):                          # a second sweep with one live lane
        c = next(c for c in R.CONV_OUT_1X1 if c["kind"] == kind and c["cin"] == cin)
        i = R.conv_out_inputs(c)
        out.append(outside(c, emu_conv_out(c, i, "skip_sweep"), R.conv_out(c, i)))
    c = _case(R.TABLE_CASES, "C260_3x3_f32_bf16")                           # the table sum's second chunk of 256 channels: 4 live channels
    i = R.table_inputs(c)
    buf = emu_table(c, i)
    idx, _ = R.table_layout(c)
    buf[idx[:, 256:].reshape(-1)] = float("nan")
    out.append(outside(c, buf, R.table_conv(c, i)))
    return all(out)


def m_quadrant():
    c = _case(R.CONV_IN_GENERIC, "s2d_4x8_c8")
    i = R.conv_in_inputs(c)
    return outside(c, emu_conv_in(c, i, "quadrant"), R.conv_in(c, i))


def m_rowadd_input_row():
    c = _case(R.TABLE_CASES, "C260_3x3_grouped_ldy")
    i = R.table_inputs(c)
    return outside(c, emu_table(c, i, rowadd_by_input=True), R.table_conv(c, i))


def m_pos_per_image():
    c = _case(R.TABLE_CASES, "C260_3x3_grouped_ldy")
    i = R.table_inputs(c)
    return outside(c, emu_table(c, i, pos_per_image=True), R.table_conv(c, i))


def m_pool_last_max():
    c = R.POOL_BWD_CASES[0]
    i = R.pool_bwd_inputs(c)
    return not torch.equal(R.maxpool2_bwd(i.x, i.dy, last=True), R.maxpool2_bwd(i.x, i.dy))


def m_bias_first():
    c = next(c for c in R.CONV_OUT_1X1 if c["cin"] == 8 and c["bias"])
    i = R.conv_out_inputs(c)
    return outside(c, emu_conv_out(c, i, "bias_first"), R.conv_out(c, i))


def m_even_centre():
    c = _case(R.TABLE_CASES, "C260_3x3_f32_bf16")
    i = R.table_inputs(c)
    return outside(c, emu_table(c, i, centre=1), R.table_conv(c, i))


MUTANTS = {"the transposed fold's tap parity off by one at the border": m_fold_parity, "ky / kx swapped": m_kykx,
           "the last partial channel sweep skipped": m_skip_sweep, "an s2d quadrant swapped": m_quadrant,
           "rowadd indexed by the input row": m_rowadd_input_row, "pos applied per image": m_pos_per_image,
           "the pool gradient sent to the last maximum": m_pool_last_max, "the 1x1 head's bias added before the reduction": m_bias_first,
           "the tap window centred as an even-sized window would be": m_even_centre}


@pytest.mark.parametrize("name", list(MUTANTS), ids=[k.replace(" ", "_") for k in MUTANTS])
def test_mutant_is_caught(name):
    assert MUTANTS[name](), f"{name}: inside the bound and the footprint"
