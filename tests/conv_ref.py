"""fp64 restatements of the small-channel ends of the VQ-VAE (mage_amd/csrc/conv_direct.hip), of their three backward twins (train.hip) and of
the gather kernels that produce the decoder's input rows (vq.hip), as closed formulas on their logical tensors, with a per-element error
bound for every output:
    mage_conv_in, mage_conv_out (1x1 and transposed), mage_convt_fold_tanh, mage_maxpool2, mage_upsample2, mage_relu, mage_cast,
    mage_maxpool2_bwd, mage_upsample2_bwd, mage_convt_unfold_tanh_bwd, mage_table_conv, mage_embedding.
The references take the exact values the kernels read (16-bit inputs converted from their stored bits) and return, beside the values and the
bounds, the flat index of every output element in the buffer the kernel writes (`idx`, in logical elements: a split element counts once) and
that buffer's size, slack included: the footprint.  The case tables live here so the CPU and the GPU tests share them.

Bounds.  u = 2^-24, first order in u, the accounting of tests/train_ref.py and tests/norm_ref.py: an fp32 add, multiply or fused multiply-add:
relative u (a bound that counts the product's rounding AND the add's holds with or without contraction); a fixed-order fp32 sum whose every
term passes through at most n additions: n u sum|terms|; a 16-bit or split store: tests/train_ref.py store_err at |ref|.

mage_conv_in (conv_in_kernel, conv_in_4x4s2_kernel): acc = bias, then T = cin kh kw fused multiply-adds in (ci, ky, kx) order; a tap outside the
  image is skipped (or, in the image kernel, adds 0 w: the same value).  The bias and the first product pass through T additions, a product rounds
  once more without contraction:                 |err s| <= es = (T + 1) u (|bias| + sum |x w|).
  t = s scale + shift (one product, one add):    |err t| <= et = |scale| es + u |s scale| + u |t|;      without scale t = s, et = es.
  ReLU is exact once the sign is right: the inputs are built so that every |t| > 16 et; then err y <= et where t > 0 and y = 0 exactly elsewhere.
mage_conv_out: s = sum_c x_c w_c (+ the four taps of the transposed form), y = tanhf(s + bias).  Every kernel adds a float4's four products
  left to right (3 additions, 1 product rounding) onto the lane's sum, then reduces the lanes with xor shuffles, then adds the bias:
    16 lanes per pixel (conv_out_1x1_kernel; CPL = 4 fp32 | 8 bf16 channels per 16-byte chunk): ceil(cin / (16 CPL)) CPL / 4 additions onto
        the lane's sum, 4 shuffles;              n = 4 + ceil(cin / (16 CPL)) CPL / 4 + 4 + 1
    a thread per pixel (conv_out_1x1_c4_kernel, cin = 4): n = 4 + 1, covered by the figure above;
    a wave per pixel (conv_out_kernel): taps ceil(cin / 256) additions onto the lane's sum (taps = 4 transposed, 1 otherwise), 6 shuffles:
                                                 n = 4 + taps ceil(cin / 256) + 6 + 1.
  The 1x1 bound takes the larger n of the two kernels that can serve a 1x1 call, so it covers both twins whatever the predicate picks:
                                                 |err pre| <= es = n u (|bias| + sum |x w|).
mage_convt_fold_tanh: s = bias + at most four taps in (a, b) order: 4 additions: es = 4 u (|bias| + sum |taps|); y = tanhf(s).
tanhf: nothing in the project or in the ROCm tree on the build machine states the device library's accuracy, so it gets what its
  specification promises: 5 ulp of the fp32 result (the OpenCL full-profile figure the device math library is written to meet), on top of the
  propagated pre-activation error (1 - y^2) es, plus the second-order term es^2 (|tanh''| < 0.77: half of it rounds up to es^2):
                                                 |err y| <= (1 - y^2) es + es^2 + 5 ulp32(y).
mage_convt_unfold_tanh_bwd: dtaps = g (1 - y y) where the tap lands inside the image, exactly 0 elsewhere, g itself when y is null.  y y: u y^2;
  1 - .: u |1 - y^2|; the product: u |v|:       |err| <= |g| u (y^2 + |1 - y^2|) + u |v|   (3 u |g| at most).
mage_upsample2_bwd: (d0 + d1) + (d2 + d3): 2 additions above every term:  2 u sum |d|.
mage_maxpool2, mage_upsample2, mage_relu, mage_cast, mage_maxpool2_bwd: exact; their references are typed tensors compared bit for bit (the pool
  gradient goes to the FIRST maximum in scan order; no NaN and no window holding both +0 and -0 is built).
mage_table_conv (table_conv_kernel, table_conv512_kernel: the same order): acc = pos (+ bias: 1 addition), the taps in (ky, kx) order (at most
  th tw additions), + rowadd (1):               |err t| <= et = (th tw + 2) u (|pos| + |bias| + sum |table rows| + |rowadd|); ReLU as above.
mage_embedding: a copy (+ ReLU): exact in fp32, one store_err otherwise.
No constant here is fitted to a kernel's output."""
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests.train_ref import U, store_err

TAIL = 192                                  # slack elements (a multiple of 64: three split slabs) past every output's last mapped element
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "bf16x3": torch.bfloat16, "f16x3": torch.float16}
SPLIT = ("bf16x3", "f16x3")
TANH_ULPS = 5.0


def _g(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def case_id(c):
    return c["name"]


def ulp32(y):
    """The spacing of fp32 values at |y|."""
    _, e = torch.frexp(y.abs())
    e = torch.where(y == 0, -1000.0, e.to(torch.float64) - 1)
    return torch.exp2(e.clamp(min=-126) - 23)


def tanh_bound(y, es):
    return (1 - y * y) * es + es * es + TANH_ULPS * ulp32(y)


def relu_out(t, et, act, kind):
    """(y, bound) of act(t) stored as `kind`; under ReLU the bound is 0 where t < 0 (the caller's inputs keep |t| > 16 et)."""
    if act:
        y = t.clamp(min=0)
        b = torch.where(t > 0, et, torch.zeros_like(et))
    else:
        y, b = t, et
    return y, b + store_err(y, kind)


def with_margin(build, ref, c):
    """The first of the seeds 0, 1, ... whose inputs keep every pre-activation of a ReLU case at |t| > 16 et."""
    for seed in range(60):
        i = build(c, seed)
        if not c.get("act"):
            return i
        r = ref(c, i)
        if bool((r.t.abs() > 16 * r.et).all()):
            return i
    raise AssertionError(f"{c['name']}: no seed gives the ReLU margin")


def margin(r):
    return float((r.t.abs() / r.et).min())


def raw_mask(mask, kind):
    """The written-element mask of a logical buffer -> of its stored 16-bit / fp32 elements (a split slab of 64 is [hi(64) | lo(64)])."""
    if kind not in SPLIT:
        return mask
    return mask.reshape(-1, 1, 64).expand(-1, 2, 64).reshape(-1)


def footprint(size, idx):
    m = torch.zeros(size, dtype=torch.bool)
    m[idx.reshape(-1)] = True
    assert int(m.sum()) == idx.numel(), "two outputs share an element"
    return m


def verdict(buf, r):
    """buf: the fp64 logical buffer, NaN where nothing was written.  (footprint right, worst |err| / bound)."""
    m = footprint(r.size, r.idx)
    ok = bool((~torch.isnan(buf) == m).all())
    got = buf[r.idx]
    err = (got - r.y).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / r.b)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return ok, float(ratio.max())


def qz(x, kind):
    """x rounded to the values a tensor of `kind` holds, as that typed tensor."""
    return x.to(TORCH_DT[kind])


# ------------------------------------------------------------------------------------------------ mage_conv_in
def _ci(name, N, cin, H, W, cout, k, stride, pad, bias=True, scale=False, act=0, kind="f32", s2d=False, path="generic"):
    return dict(name=name, N=N, cin=cin, H=H, W=W, cout=cout, k=k, stride=stride, pad=pad, bias=bias, scale=scale, act=act, kind=kind, s2d=s2d,
                path=path)


CONV_IN_GENERIC = (
    _ci("f4_6x8_c4", 3, 1, 6, 8, 4, 4, 2, 1),                                                       # 36 items: one partial workgroup
    _ci("f4_7x5_c8_scale_relu", 5, 1, 7, 5, 8, 4, 2, 1, bias=False, scale=True, act=1),             # odd plane: OH = 3, OW = 2 by the floor
    _ci("f4_7x5_c64_bf16", 2, 1, 7, 5, 64, 4, 2, 1, bias=False, kind="bf16"),
    _ci("f8_5x9_c64_bf16_relu", 2, 3, 5, 9, 64, 7, 1, 3, scale=True, act=1, kind="bf16"),           # a plane smaller than the filter; 1440 items
    _ci("f8_5x9_c64_f16x3", 1, 3, 5, 9, 64, 7, 1, 3, bias=False, kind="f16x3"),
    _ci("cin4_3x3_c8", 2, 4, 5, 4, 8, 3, 1, 1),
    _ci("f4_6x8_c64_bf16x3_relu", 3, 1, 6, 8, 64, 4, 2, 1, scale=True, act=1, kind="bf16x3"),
    _ci("s2d_4x4_c4_relu", 2, 1, 8, 8, 4, 4, 2, 1, act=1, s2d=True),
    _ci("s2d_4x8_c8", 3, 1, 8, 16, 8, 4, 2, 1, s2d=True),
    _ci("s2d_4x4_c64_f16x3", 2, 1, 8, 8, 64, 4, 2, 1, bias=False, kind="f16x3", s2d=True),
    _ci("s2d_4x8_c64_bf16x3", 3, 1, 8, 16, 64, 4, 2, 1, scale=True, kind="bf16x3", s2d=True),
    _ci("s2d_f8_4x8_c64_f16x3", 2, 3, 4, 8, 64, 7, 1, 3, kind="f16x3", s2d=True),
)
CONV_IN_IMAGE = (
    _ci("img_n64_4x4_c4_relu", 64, 1, 4, 4, 4, 4, 2, 1, act=1, path="image"),                       # one lane per pixel: 64 pixels per wave on 4
    _ci("img_n65_2x4_c64_scale", 65, 1, 2, 4, 64, 4, 2, 1, bias=False, scale=True, path="image"),
    _ci("img_n64_6x80_c256", 64, 1, 6, 80, 256, 4, 2, 1, scale=True, path="image"),
    _ci("img_n64_146x80_c4", 64, 1, 146, 80, 4, 4, 2, 1, path="image"),                             # the last plane inside 48 KiB of LDS
    _ci("img_n65_4x4_c64_s2d_relu", 65, 1, 4, 4, 64, 4, 2, 1, act=1, s2d=True, path="image"),
    _ci("img_n64_4x4_c64_s2d_bf16x3", 64, 1, 4, 4, 64, 4, 2, 1, kind="bf16x3", s2d=True, path="image"),
    _ci("img_n64_4x4_c256_s2d_f16x3", 64, 1, 4, 4, 256, 4, 2, 1, scale=True, kind="f16x3", s2d=True, path="image"),
    _ci("img_n64_2x4_c64_f16x3", 64, 1, 2, 4, 64, 4, 2, 1, kind="f16x3", path="image"),
    # one case just outside every term of the predicate
    _ci("out_n63", 63, 1, 4, 4, 64, 4, 2, 1),
    _ci("out_h5", 64, 1, 5, 4, 4, 4, 2, 1),
    _ci("out_w6", 64, 1, 4, 6, 4, 4, 2, 1),
    _ci("out_w84", 64, 1, 4, 84, 4, 4, 2, 1),
    _ci("out_148x80", 64, 1, 148, 80, 4, 4, 2, 1),
    _ci("out_c12", 64, 1, 4, 4, 12, 4, 2, 1),
    _ci("out_c512", 64, 1, 4, 4, 512, 4, 2, 1),
    _ci("out_bf16", 64, 1, 4, 4, 64, 4, 2, 1, kind="bf16"),
)


def conv_in_shape(c):
    OH = (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
    OW = (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
    return OH, OW


def conv_in_inputs(c, seed=0):
    g = _g("conv_in", c["name"], seed)
    T = c["cin"] * c["k"] * c["k"]
    x = torch.randn(c["N"], c["cin"], c["H"], c["W"], generator=g)
    wt = torch.randn(T, c["cout"], generator=g) * (2.0 / T ** 0.5)
    bias = torch.randn(c["cout"], generator=g) if c["bias"] else None
    scale = shift = None
    if c["scale"]:
        scale = 0.5 + torch.rand(c["cout"], generator=g)
        scale[0] = -0.75
        shift = torch.randn(c["cout"], generator=g)
    return SimpleNamespace(x=x, wt=wt, bias=bias, scale=scale, shift=shift)


def patches(x, k, stride, pad):
    """x [N, cin, H, W] -> [N, OH * OW, cin k k], taps in (ci, ky, kx) order, zeros outside the image."""
    return F.unfold(x, (k, k), padding=pad, stride=stride).transpose(1, 2)


def s2d_index(N, OH, OW, cout, swap=False):
    """Flat logical index [N, OH * OW, cout] of the offset space-to-depth rows: block (R, C) = ((oy + 1) / 2, (ox + 1) / 2) of a
    (OH / 2 + 1) x (OW / 2 + 1) grid, quadrant q = ((oy + 1) & 1) 2 + ((ox + 1) & 1), 4 cout channels per row."""
    BH, BW = OH // 2 + 1, OW // 2 + 1
    oy, ox = torch.arange(OH)[:, None], torch.arange(OW)[None, :]
    row = ((oy + 1) >> 1) * BW + ((ox + 1) >> 1)
    q = ((ox + 1) & 1) * 2 + ((oy + 1) & 1) if swap else ((oy + 1) & 1) * 2 + ((ox + 1) & 1)
    row = torch.arange(N)[:, None, None] * (BH * BW) + row[None]
    base = (row * (4 * cout) + q[None] * cout).reshape(N, OH * OW, 1)
    return base + torch.arange(cout), N * BH * BW * 4 * cout


def conv_in_layout(c, swap=False):
    OH, OW = conv_in_shape(c)
    if c["s2d"]:
        idx, n = s2d_index(c["N"], OH, OW, c["cout"], swap)
    else:
        n = c["N"] * OH * OW * c["cout"]
        idx = torch.arange(n).reshape(c["N"], OH * OW, c["cout"])
    return idx, n + TAIL


def conv_in(c, i):
    P = patches(i.x.double(), c["k"], c["stride"], c["pad"])
    w = i.wt.double()
    T = w.shape[0]
    s, A = P @ w, P.abs() @ w.abs()
    if i.bias is not None:
        s, A = s + i.bias.double(), A + i.bias.double().abs()
    es = (T + 1) * U * A
    if i.scale is not None:
        sc, sh = i.scale.double(), i.shift.double()
        t = s * sc + sh
        et = sc.abs() * es + U * (s * sc).abs() + U * t.abs()
    else:
        t, et = s, es
    y, b = relu_out(t, et, c["act"], c["kind"])
    idx, size = conv_in_layout(c)
    return SimpleNamespace(y=y, b=b, t=t, et=et, idx=idx, size=size)


# ------------------------------------------------------------------------------------------------ mage_conv_out, mage_convt_fold_tanh
def _co(name, kind, cin, cout, N, IH, IW, bias=True, transposed=False):
    return dict(name=name, kind=kind, cin=cin, cout=cout, N=N, IH=IH, IW=IW, bias=bias, transposed=transposed)


def _conv_out_1x1_cases():
    out, k = [], 0
    for kind, cins in (("f32", (4, 8, 64, 68)), ("bf16", (8, 128, 136, 12))):
        for cin in cins:
            for N, IH, IW in ((3, 1, 5), (1, 17, 1)):                        # 15 and 17 pixels: either side of a 16-pixel workgroup
                cout, bias = 1 + k % 4, bool((k // 2) % 2)
                out.append(_co(f"1x1_{kind}_cin{cin}_cout{cout}_px{N * IH * IW}_b{int(bias)}", kind, cin, cout, N, IH, IW, bias))
                k += 1
    return tuple(out)


def _conv_out_t_cases():
    out, k = [], 0
    for kind in ("f32", "bf16"):
        for cin in (4, 64, 256, 260):
            IH, IW = ((1, 1), (2, 3), (5, 4))[k % 3]
            cout, bias = 1 + (k + k // 4) % 4, bool(k % 2)
            out.append(_co(f"t_{kind}_cin{cin}_cout{cout}_{IH}x{IW}_b{int(bias)}", kind, cin, cout, 2, IH, IW, bias, True))
            k += 1
    out.append(_co("t_f32_cin64_cout4_1x1_b1", "f32", 64, 4, 2, 1, 1, True, True))
    out.append(_co("t_bf16_cin260_cout3_5x4_b0", "bf16", 260, 3, 2, 5, 4, False, True))
    return tuple(out)


CONV_OUT_1X1 = _conv_out_1x1_cases()
CONV_OUT_T = _conv_out_t_cases()


def conv_out_inputs(c, seed=0):
    g = _g("conv_out", c["name"], seed)
    x = qz(torch.randn(c["N"], c["IH"], c["IW"], c["cin"], generator=g), c["kind"])
    rows = (16 if c["transposed"] else 1) * c["cout"]
    wt = torch.randn(rows, c["cin"], generator=g) * (1.0 / c["cin"] ** 0.5)
    bias = torch.randn(c["cout"], generator=g) * 0.5 if c["bias"] else None
    return SimpleNamespace(x=x, wt=wt, bias=bias)


def conv_out_n(c):
    cin = c["cin"]
    if c["transposed"]:
        return 4 + 4 * -(-cin // 256) + 6 + 1
    cpl = 8 if c["kind"] == "bf16" else 4
    return max(4 + -(-cin // (16 * cpl)) * (cpl // 4) + 4 + 1, 4 + -(-cin // 256) + 6 + 1)


def fold_index(IH, IW, parity=False):
    """The four taps of every output pixel of the 4x4 / stride 2 / pad 1 transposed fold in the kernels' (a, b) order, as (iy [OH, 1], ix [1, OW],
    tap [OH, OW], valid [OH, OW]) with the input pixel clamped into the image: oy = 2 iy - 1 + ky, so the rows are iy0 = (oy + 1) >> 1 with
    ky0 = oy + 1 - 2 iy0, and iy0 - 1 with ky0 + 2.  parity: the mutant that flips ky0 on the two border rows."""
    oy, ox = torch.arange(2 * IH), torch.arange(2 * IW)
    iy0, ix0 = (oy + 1) >> 1, (ox + 1) >> 1
    ky0, kx0 = oy + 1 - 2 * iy0, ox + 1 - 2 * ix0
    if parity:
        ky0 = torch.where((oy == 0) | (oy == 2 * IH - 1), 1 - ky0, ky0)
    out = []
    for a in range(2):
        iy, ky = iy0 - a, ky0 + 2 * a
        vy = (iy >= 0) & (iy < IH)
        for b in range(2):
            ix, kx = ix0 - b, kx0 + 2 * b
            vx = (ix >= 0) & (ix < IW)
            out.append((iy.clamp(0, IH - 1)[:, None], ix.clamp(0, IW - 1)[None, :], ky[:, None] * 4 + kx[None, :], vy[:, None] & vx[None, :]))
    return out


def fold_terms(tp, parity=False):
    """tp [N, IH, IW, 16, cout] -> the four terms [N, cout, 2 IH, 2 IW] of the fold in the order of fold_index, 0 where the tap is outside."""
    out = []
    for iy, ix, tap, v in fold_index(tp.shape[1], tp.shape[2], parity):
        t = tp[:, iy, ix, tap] * v[None, :, :, None].to(tp.dtype)
        out.append(t.permute(0, 3, 1, 2))
    return out


def _flat(shape):
    n = 1
    for s in shape:
        n *= s
    return torch.arange(n).reshape(shape), n + TAIL


def conv_out(c, i):
    x, w = i.x.double(), i.wt.double()
    if c["transposed"]:
        w = w.reshape(16, c["cout"], c["cin"])
        s = sum(fold_terms(torch.einsum("nyxc,tkc->nyxtk", x, w)))
        A = sum(fold_terms(torch.einsum("nyxc,tkc->nyxtk", x.abs(), w.abs())))
    else:
        s, A = (x @ w.T).permute(0, 3, 1, 2), (x.abs() @ w.abs().T).permute(0, 3, 1, 2)
    if i.bias is not None:
        bb = i.bias.double()[None, :, None, None]
        s, A = s + bb, A + bb.abs()
    es = conv_out_n(c) * U * A
    y = torch.tanh(s)
    idx, size = _flat(tuple(y.shape))
    return SimpleNamespace(y=y, b=tanh_bound(y, es), pre=s, es=es, idx=idx, size=size)


def _fd(name, N, cout, IH, IW, bias=True, path="pixel"):
    return dict(name=name, N=N, cout=cout, IH=IH, IW=IW, bias=bias, path=path)


FOLD_CASES = (
    _fd("px_n1_c1_1x1", 1, 1, 1, 1), _fd("px_n1_c2_3x5", 1, 2, 3, 5, bias=False), _fd("px_n63_c3_1x1", 63, 3, 1, 1, bias=False),
    _fd("px_n63_c4_3x5", 63, 4, 3, 5), _fd("px_n63_c1_3x5", 63, 1, 3, 5),
    _fd("img_1x1", 64, 1, 1, 1, path="image"), _fd("img_3x5", 64, 1, 3, 5, bias=False, path="image"),
    _fd("img_32x32", 64, 1, 32, 32, path="image"), _fd("img_16x64", 64, 1, 16, 64, path="image"),       # exactly 1024 pixels
    _fd("fallback_33x32", 64, 1, 33, 32), _fd("fallback_c2", 64, 2, 3, 5),
)


def fold_inputs(c, seed=0):
    g = _g("fold", c["name"], seed)
    taps = torch.randn(c["N"], c["IH"], c["IW"], 16 * c["cout"], generator=g) * 0.5
    bias = torch.randn(c["cout"], generator=g) * 0.5 if c["bias"] else None
    return SimpleNamespace(taps=taps, bias=bias)


def fold(c, i):
    tp = i.taps.double().reshape(c["N"], c["IH"], c["IW"], 16, c["cout"])
    s, A = sum(fold_terms(tp)), sum(fold_terms(tp.abs()))
    if i.bias is not None:
        bb = i.bias.double()[None, :, None, None]
        s, A = s + bb, A + bb.abs()
    es = 4 * U * A
    y = torch.tanh(s)
    idx, size = _flat(tuple(y.shape))
    return SimpleNamespace(y=y, b=tanh_bound(y, es), pre=s, es=es, idx=idx, size=size)


# ------------------------------------------------------------------------------------------------ pool, upsample, relu, cast (exact)
def _pool_cases():
    out, k = [], 0
    for kind in ("f32", "bf16"):
        for C in (4, 8, 260):
            for H, W in ((2, 2), (4, 6)):
                N, relu = (1, 3)[(k + k // 2) % 2], (k // 2 + k // 6) % 2
                out.append(dict(name=f"{kind}_C{C}_{H}x{W}_n{N}_relu{relu}", kind=kind, C=C, H=H, W=W, N=N, relu=relu))
                k += 1
    return tuple(out)


POOL_CASES = _pool_cases()
MAP_N = (4, 1020, 1028)
CAST_PAIRS = (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("f32", "f16"), ("f16", "f32"))


def pool_inputs(c):
    g = _g("pool", c["name"])
    return qz(torch.randn(c["N"], c["H"], c["W"], c["C"], generator=g) - 0.3, c["kind"])


def maxpool2(x, relu):
    """x [N, H, W, C] typed -> the typed maximum of every 2x2 window (max(., 0) with the relu flag)."""
    N, H, W, C = x.shape
    y = x.reshape(N, H // 2, 2, W // 2, 2, C).amax((2, 4))
    return y.clamp(min=0) if relu else y


def upsample2(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def map_inputs(n, kind):
    return qz(torch.randn(n, generator=_g("map", n, kind)) * 3, kind)


def cast_edges(src):
    """Edge values of the source type, a multiple of 4 of them: subnormals of either side, round-to-even halfway cases, +-inf, the f16 overflow."""
    if src == "f32":
        v = [0.0, 2.0 ** -149, -2.0 ** -127, 2.0 ** -126, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25 * 1.0000001, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -133,
             3 * 2.0 ** -134, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65504.0, 65519.0,
             65520.0, 70000.0, -70000.0, 1e38, 3.4e38, -3.4e38, float("inf"), float("-inf"), -0.0]
        return torch.tensor(v + [1.0] * (-len(v) % 4), dtype=torch.float32)
    it = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)     # every bit pattern that is not a NaN
    x = it.view(TORCH_DT[src])
    x = x[~torch.isnan(x)]
    return x[:x.numel() // 4 * 4].clone()


# ------------------------------------------------------------------------------------------------ the backward twins
POOL_BWD_CASES = tuple(dict(name=f"C{C}_{H}x{W}_n{N}", C=C, H=H, W=W, N=N) for C, H, W, N in ((4, 2, 2, 1), (8, 4, 6, 3), (260, 4, 6, 1), (260, 2, 2, 3)))
UNFOLD_CASES = tuple(dict(name=f"y{int(y)}_c{cout}_{IH}x{IW}_n{N}", y=y, cout=cout, IH=IH, IW=IW, N=N)
                     for y, cout, IH, IW, N in ((True, 1, 1, 1, 1), (True, 3, 3, 5, 2), (False, 1, 3, 5, 3), (False, 3, 1, 1, 2), (True, 1, 3, 5, 1)))


def pool_bwd_inputs(c):
    """x [N, H, W, C] with, in the first windows of channel 0, the maximum tied on each pair of window positions and an all-equal window (at
    least the pairs (0, 1) and (2, 3): a tie at each of the four positions); dy [N, H / 2, W / 2, C] with exact zeros."""
    g = _g("pool_bwd", c["name"])
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    x = torch.randn(N, H, W, C, generator=g)
    win = x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, C, 4).clone()      # [windows, C, 4 (scan order)]
    pats = [(0, 1), (2, 3), None, (1, 2), (0, 3), (0, 2), (1, 3)]            # None: the all-equal window; the first three hold every position
    for j in range(min(win.shape[0] * C, 14)):
        w_, ch = j % win.shape[0], j // win.shape[0]
        if pats[j % 7] is None:
            win[w_, ch, :] = 0.5
        else:
            win[w_, ch, :] = torch.tensor([-1.0, -2.0, -3.0, -4.0])
            win[w_, ch, list(pats[j % 7])] = 1.25
    x = win.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C).contiguous()
    dy = torch.randn(N, H // 2, W // 2, C, generator=g)
    dy[..., 0::3] = torch.where(torch.rand(dy[..., 0::3].shape, generator=g) < 0.3, torch.zeros(()), dy[..., 0::3])
    return SimpleNamespace(x=x, dy=dy)


def maxpool2_bwd(x, dy, last=False):
    """dx (typed like dy): dy at the first maximum of the window in scan order, 0 elsewhere.  last: the mutant that takes the last."""
    N, H, W, C = x.shape
    win = x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
    best = torch.zeros(win.shape[:-1], dtype=torch.long)
    m = win[..., 0]
    for k in range(1, 4):
        better = win[..., k] >= m if last else win[..., k] > m
        m = torch.where(better, win[..., k], m)
        best = torch.where(better, torch.full_like(best, k), best)
    o = torch.zeros(win.shape, dtype=dy.dtype).scatter_(-1, best[..., None], dy[..., None])
    return o.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C).contiguous()


def upsample2_bwd(dy):
    """dy [N, 2H, 2W, C] fp64 -> (dx, bound)."""
    N, H2, W2, C = dy.shape
    w = dy.reshape(N, H2 // 2, 2, W2 // 2, 2, C)
    return w.sum((2, 4)), 2 * U * w.abs().sum((2, 4))


def unfold_inputs(c):
    g = _g("unfold", c["name"])
    shape = (c["N"], c["cout"], 2 * c["IH"], 2 * c["IW"])
    gy = torch.randn(shape, generator=g)
    y = torch.tanh(torch.randn(shape, generator=g) * 1.5) if c["y"] else None
    return SimpleNamespace(g=gy, y=y)


def unfold(c, i, dt=torch.float64):
    """dtaps [N, IH, IW, 16 cout] in dt (fp64: the reference and its bound; fp32: the kernel's arithmetic) and the out-of-image mask."""
    N, cout, IH, IW = c["N"], c["cout"], c["IH"], c["IW"]
    gy = i.g.to(dt)
    if i.y is not None:
        yy = i.y.to(dt)
        v = gy * (1 - yy * yy)
        b = gy.abs() * U * (yy * yy + (1 - yy * yy).abs()) + U * v.abs()
    else:
        v, b = gy, torch.zeros_like(gy)
    iy, ix, tap = torch.arange(IH)[:, None, None], torch.arange(IW)[None, :, None], torch.arange(16)[None, None, :]
    oy, ox = 2 * iy - 1 + (tap >> 2), 2 * ix - 1 + (tap & 3)
    inside = ((oy >= 0) & (oy < 2 * IH) & (ox >= 0) & (ox < 2 * IW)).expand(IH, IW, 16)
    oyc, oxc = oy.clamp(0, 2 * IH - 1).expand(IH, IW, 16), ox.clamp(0, 2 * IW - 1).expand(IH, IW, 16)

    def take(a):
        t = a[:, :, oyc, oxc].permute(0, 2, 3, 4, 1)                        # [N, IH, IW, 16, cout]
        return (t * inside[None, :, :, :, None].to(dt)).reshape(N, IH, IW, 16 * cout)
    y = take(v)
    idx, size = _flat(tuple(y.shape))
    return SimpleNamespace(y=y, b=take(b), inside=inside[None, :, :, :, None].expand(N, IH, IW, 16, cout).reshape(y.shape), idx=idx, size=size)


# ------------------------------------------------------------------------------------------------ mage_table_conv
def _tc(name, C, th, tw, H, W, n_codes, tk, yk, n_img=2, pos=False, bias=False, rowadd=False, act=0, grouped=False, ldy_pad=0, path="generic"):
    return dict(name=name, C=C, th=th, tw=tw, H=H, W=W, n_codes=n_codes, tk=tk, yk=yk, n_img=n_img, pos=pos, bias=bias, rowadd=rowadd, act=act,
                grouped=grouped, ldy_pad=ldy_pad, path=path)


TABLE_CASES = (
    _tc("C4_1x1_f32_f32", 4, 1, 1, 1, 1, 1, "f32", "f32", n_img=3),
    _tc("C260_3x3_f32_bf16", 260, 3, 3, 1, 7, 7, "f32", "bf16", pos=True, bias=True),
    _tc("C512_5x5_f32_f16_relu", 512, 5, 5, 5, 3, 7, "f32", "f16", rowadd=True, act=1),
    _tc("C1028_3x3_bf16_f32", 1028, 3, 3, 5, 3, 7, "bf16", "f32", pos=True, rowadd=True),
    _tc("C2048_3x3_f16_f32_relu", 2048, 3, 3, 1, 7, 7, "f16", "f32", bias=True, act=1),
    _tc("C260_1x3_bf16_bf16", 260, 1, 3, 5, 3, 7, "bf16", "bf16", pos=True),
    _tc("C1028_3x1_f16_f16_relu", 1028, 3, 1, 1, 7, 7, "f16", "f16", bias=True, act=1),
    _tc("C2048_5x5_f32_f32", 2048, 5, 5, 1, 1, 1, "f32", "f32", bias=True),
    _tc("C64_3x3_bf16x3", 64, 3, 3, 5, 3, 7, "f32", "bf16x3", pos=True, bias=True, rowadd=True),
    _tc("C64_3x3_f16x3_relu", 64, 3, 3, 1, 7, 7, "f32", "f16x3", pos=True, act=1),
    _tc("C260_3x3_grouped_ldy", 260, 3, 3, 5, 3, 7, "f32", "f32", n_img=3, pos=True, rowadd=True, grouped=True, ldy_pad=8),
    _tc("C4_5x5_grouped_f16", 4, 5, 5, 5, 3, 7, "f16", "f16", n_img=3, rowadd=True, grouped=True, ldy_pad=8),
    # 16-bit table and rows of 512 channels: the eight-channels-per-lane kernel; ldy = 516 sends the same call back to the generic kernel
    _tc("C512_bf16_fast", 512, 3, 3, 5, 3, 7, "bf16", "bf16", n_img=3, pos=True, bias=True, rowadd=True, act=1, grouped=True, ldy_pad=8, path="512"),
    _tc("C512_bf16_ldy516", 512, 3, 3, 5, 3, 7, "bf16", "bf16", n_img=3, pos=True, bias=True, rowadd=True, act=1, grouped=True, ldy_pad=4),
    _tc("C512_f16_fast", 512, 5, 5, 1, 7, 7, "f16", "f16", pos=True, rowadd=True, path="512"),
    _tc("C512_f16_ldy516", 512, 5, 5, 1, 7, 7, "f16", "f16", pos=True, rowadd=True, ldy_pad=4),
)
TABLE_TWINS = (("C512_bf16_fast", "C512_bf16_ldy516"), ("C512_f16_fast", "C512_f16_ldy516"))
ROWADD_DIV, ROWADD_MOD = 2, 3


def table_map(c):
    """(group, y_group_stride, y_off, ldy): grouped cases write a group of 5 pixels every 8 rows from row 3 (gaps between the groups)."""
    n_pix = c["n_img"] * c["H"] * c["W"]
    group, stride, off = (5, 8, 3) if c["grouped"] else (n_pix, n_pix, 0)
    return group, stride, off, c["C"] + c["ldy_pad"]


def table_inputs(c, seed=0):
    if c["name"].endswith("_ldy516"):                                       # the twin reads the same data
        return table_inputs(dict(c, name=c["name"].replace("_ldy516", "_fast")), seed)
    g = _g("table", c["name"], seed)
    C, T, plane = c["C"], c["th"] * c["tw"], c["H"] * c["W"]
    ids = torch.randint(0, c["n_codes"], (c["n_img"], c["H"], c["W"]), generator=g)
    table = qz(torch.randn(T, c["n_codes"], C, generator=g), c["tk"])
    pos = torch.randn(plane, C, generator=g) if c["pos"] else None
    bias = torch.randn(C, generator=g) if c["bias"] else None
    rowadd = torch.randn(ROWADD_MOD, C, generator=g) if c["rowadd"] else None
    return SimpleNamespace(ids=ids, table=table, pos=pos, bias=bias, rowadd=rowadd)


def table_rows(c):
    group, stride, off, _ = table_map(c)
    m = torch.arange(c["n_img"] * c["H"] * c["W"])
    return m // group * stride + m % group + off


def table_terms(c, i, dt=torch.float64, centre=0, pos_per_image=False, rowadd_by_input=False):
    """The terms of every output row [n_pix, C] in the kernel's order of addition (pos, bias, the taps in (ky, kx) order, rowadd), in dt.  The
    three flags are the mutants of tests/test_conv_ref_cpu.py."""
    n_img, H, W, th, tw, C = c["n_img"], c["H"], c["W"], c["th"], c["tw"], c["C"]
    plane = H * W
    out = []
    m = torch.arange(n_img * plane)
    if i.pos is not None:
        out.append(i.pos.to(dt)[(m // plane) % plane if pos_per_image else m % plane])
    if i.bias is not None:
        out.append(i.bias.to(dt)[None].expand(n_img * plane, C))
    py, px = torch.arange(H)[:, None], torch.arange(W)[None, :]
    tab = i.table.to(dt)
    for ky in range(th):
        iy = py + ky - (th >> 1) - centre
        for kx in range(tw):
            ix = px + kx - (tw >> 1) - centre
            ok = ((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).expand(H, W)
            code = i.ids[:, iy.clamp(0, H - 1).expand(H, W), ix.clamp(0, W - 1).expand(H, W)]          # [n_img, H, W]
            out.append((tab[ky * tw + kx][code] * ok[None, :, :, None].to(dt)).reshape(n_img * plane, C))
    if i.rowadd is not None:
        r = m if rowadd_by_input else table_rows(c)
        out.append(i.rowadd.to(dt)[(r // ROWADD_DIV) % ROWADD_MOD])
    return out


def table_layout(c):
    *_, ldy = table_map(c)
    rows = table_rows(c)
    n_rows = int(rows.max()) + 1 + 2                                        # two slack rows
    size = -(-n_rows * ldy // 64) * 64 + TAIL
    return rows[:, None] * ldy + torch.arange(c["C"])[None], size


def table_conv(c, i):
    terms = table_terms(c, i)
    t = sum(terms)
    et = (c["th"] * c["tw"] + 2) * U * sum(x.abs() for x in terms)
    y, b = relu_out(t, et, c["act"], c["yk"])
    idx, size = table_layout(c)
    return SimpleNamespace(y=y, b=b, t=t, et=et, idx=idx, size=size)


# ------------------------------------------------------------------------------------------------ mage_embedding
def _em(name, C, kind, n, relu, group, group_stride, off, inner=0, inner_stride=0):
    return dict(name=name, C=C, kind=kind, n=n, relu=relu, group=group, group_stride=group_stride, off=off, inner=inner, inner_stride=inner_stride)


EMB_CASES = (
    _em("C4_f32_one_level", 4, "f32", 7, 0, 3, 5, 2),
    _em("C4_f32_relu_two_level", 4, "f32", 15, 1, 6, 20, 1, 2, 5),
    _em("C260_bf16_relu_two_level", 260, "bf16", 15, 1, 6, 20, 1, 2, 5),
    _em("C260_f16_one_level", 260, "f16", 7, 0, 3, 5, 2),
    _em("C260_f32_packed", 260, "f32", 9, 0, 9, 9, 0),
    _em("C64_bf16x3_two_level", 64, "bf16x3", 15, 0, 6, 20, 0, 2, 5),
    _em("C64_f16x3_relu_one_level", 64, "f16x3", 7, 1, 3, 5, 2),
)
EMB_TABLE = 11


def emb_inputs(c):
    g = _g("emb", c["name"])
    ids = torch.randint(0, EMB_TABLE, (c["n"],), generator=g)
    ids[0], ids[-1] = 0, EMB_TABLE - 1
    return SimpleNamespace(ids=ids, table=torch.randn(EMB_TABLE, c["C"], generator=g))


def emb_rows(c):
    i = torch.arange(c["n"])
    inner, inner_stride = (c["inner"], c["inner_stride"]) if c["inner"] > 0 else (c["group"], c["group"])
    ig = i % c["group"]
    return i // c["group"] * c["group_stride"] + ig // inner * inner_stride + ig % inner + c["off"]


def embedding(c, i):
    t = i.table.double()[i.ids]
    y = t.clamp(min=0) if c["relu"] else t
    rows = emb_rows(c)
    size = -(-(int(rows.max()) + 3) * c["C"] // 64) * 64 + TAIL
    return SimpleNamespace(y=y, b=store_err(y, c["kind"]), idx=rows[:, None] * c["C"] + torch.arange(c["C"])[None], size=size)
