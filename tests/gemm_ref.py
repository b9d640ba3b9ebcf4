"""A plain fp64 restatement of the mage_gemm_desc contract (include/mage_hip.h, "Fused GEMM / implicit-GEMM convolution"), written from the
header's words: no tiles, no kernel structure, nothing shared with mage_amd.ops.  tests/test_gemm_ref_cpu.py pins it against torch
(F.conv2d, F.conv_transpose2d, nn.Upsample, F.layer_norm); tests/test_gpu_gemm.py compares every kernel family with it.

The caller hands over the VALUES the kernel reads, as fp64 tensors: 16-bit operands after their rounding, split-precision operands through
tests.helpers.unsplit (lda / ldw then count logical elements, i.e. half the descriptor's).  A and W are addressed flat, as the library
addresses them: element (row, c) of A is A.reshape(-1)[row * lda + c].

desc(**fields) fills the descriptor's defaults the way the header states them (a plain Linear: out_h = in_h = 1, out_w = in_w = M, ...).
gemm_ref(...) returns a Result:
  yrow [M]        the output row of GEMM row m
  y    [M, N]     the value of the epilogue BEFORE the store rounds it to y_dtype (head_w: [M, 16] / head_phases: see gemm_head_ref)
  S    [M, N]     sum_k |a| |w| of the element: what an accumulation bound scales with
  mag             the magnitude of each epilogue term, [M, N] each (or broadcastable): 'bias', 'pre_act' (|v| entering the activation),
                  'scale', 'shift', 'rowadd', 'residual', 'ln_mean_colsum', 'rstd'
  y2, ln_part     the extra outputs of the LayerNorm-folded forms (ln_part slice-major [N / 64, rows, 2], rows indexed by yrow)
store(v, kind) rounds fp64 values the way a store of that type does."""
import math
from types import SimpleNamespace

import torch

F32, BF16, BF16X3, F16X3, F16 = 0, 1, 2, 3, 4                                # the header's dtype tags
ACT_NONE, ACT_RELU, ACT_QUICKGELU, ACT_GELU_ERF, ACT_QUICKGELU_GRAD = 0, 1, 2, 3, 5

_DEFAULTS = dict(lda=None, ldw=0, out_h=1, out_w=None, in_h=None, in_w=None, a_img_stride=None, a_off=0, taps_h=1, taps_w=1, cin=None,
                 stride=1, dy0=0, dx0=0, dys=1, dxs=1, y_img_stride=None, y_mul_y=None, y_mul_x=1, y_off=0, act=ACT_NONE, rowadd_div=1,
                 rowadd_mod=1, ldr=None, post_relu=0, n_split=1, a_split_stride=0, w_split_stride=0, res_half=0, a_half=0, a_relu=0,
                 ln_eps=0.0, head_phases=0)


def desc(M, N, K, **kw):
    unknown = set(kw) - set(_DEFAULTS)
    assert not unknown, unknown
    d = SimpleNamespace(M=M, N=N, K=K, **{**_DEFAULTS, **kw})
    d.out_w = M if d.out_w is None else d.out_w
    d.in_h = d.out_h if d.in_h is None else d.in_h
    d.in_w = d.out_w if d.in_w is None else d.in_w
    d.cin = K // (d.taps_h * d.taps_w) if d.cin is None else d.cin
    d.lda = d.cin if d.lda is None else d.lda
    d.ldw = d.ldw or K                                                       # "0 = K (W packed [N][K])"
    d.a_img_stride = d.in_h * d.in_w if d.a_img_stride is None else d.a_img_stride
    d.y_img_stride = d.out_h * d.out_w if d.y_img_stride is None else d.y_img_stride
    d.y_mul_y = d.out_w if d.y_mul_y is None else d.y_mul_y
    d.ldr = N if d.ldr is None else d.ldr
    d.n_split = max(d.n_split, 1)
    assert K == d.taps_h * d.taps_w * d.cin
    return d


def row_geometry(d, device="cpu"):
    """m -> (img, oy, ox, yrow): "img = m / (out_h*out_w), oy = (m / out_w) % out_h, ox = m % out_w"."""
    m = torch.arange(d.M, device=device)
    img, oy, ox = m // (d.out_h * d.out_w), (m // d.out_w) % d.out_h, m % d.out_w
    return img, oy, ox, img * d.y_img_stride + oy * d.y_mul_y + ox * d.y_mul_x + d.y_off


def tap_rows(d, ky, kx, device="cpu"):
    """(arow [M], inside [M]) of tap (ky, kx): "iy = oy*stride + dy0 + ky*dys, ix likewise (zero outside [0,in_h)x[0,in_w));
    arow = img*a_img_stride + iy*in_w + ix + a_off"; a_half: "tap pixel (iy, ix) reads row (iy/2)*(in_w/2) + ix/2"."""
    img, oy, ox, _ = row_geometry(d, device)
    iy = oy * d.stride + d.dy0 + ky * d.dys
    ix = ox * d.stride + d.dx0 + kx * d.dxs
    inside = (iy >= 0) & (iy < d.in_h) & (ix >= 0) & (ix < d.in_w)
    pix = (iy // 2) * (d.in_w // 2) + ix // 2 if d.a_half else iy * d.in_w + ix
    return torch.where(inside, img * d.a_img_stride + pix + d.a_off, torch.zeros_like(pix)), inside


def product(A, W, d, split=0):
    """(sum_k A[arow(m, k), ci] W[n, k], sum_k |.||.|) for k = (ky, kx, ci), ci fastest; slice `split` of a split-K descriptor."""
    A, W = A.reshape(-1), W.reshape(-1)
    dev = A.device
    ci = torch.arange(d.cin, device=dev)
    n = torch.arange(d.N, device=dev)
    acc = torch.zeros(d.M, d.N, dtype=torch.float64, device=dev)
    S = torch.zeros_like(acc)
    for ky in range(d.taps_h):
        for kx in range(d.taps_w):
            arow, inside = tap_rows(d, ky, kx, dev)
            a = A[split * d.a_split_stride + arow[:, None] * d.lda + ci[None]] * inside[:, None]
            if d.a_relu:
                a = a.clamp(min=0)
            w = W[split * d.w_split_stride + n[:, None] * d.ldw + (ky * d.taps_w + kx) * d.cin + ci[None]]
            acc += a @ w.t()
            S += a.abs() @ w.abs().t()
    return acc, S


def act_ref(v, act):
    if act == ACT_RELU:
        return v.clamp(min=0)
    if act == ACT_QUICKGELU:
        return v * torch.sigmoid(1.702 * v)
    if act == ACT_GELU_ERF:
        return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    assert act == ACT_NONE, act
    return v


def quickgelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


def ln_stats_from_part(part, C, eps):
    """mage_ln_stats' words: mean = sum_s part[s][row][0] / C, var = sum_s part[s][row][1] / C - mean^2, rstd = 1 / sqrt(max(var, 0) + eps)."""
    mean = part[:, :, 0].sum(0) / C
    var = part[:, :, 1].sum(0) / C - mean * mean
    return mean, 1.0 / torch.sqrt(var.clamp(min=0) + eps)


def store(v, kind):
    """fp64 values as a store of type `kind` leaves them (round to nearest even; split kinds: hi + lo of the header's definition)."""
    if kind == F32:
        return v.float().double()
    if kind == BF16:
        return v.float().bfloat16().double()
    if kind == F16:
        return v.float().half().double()
    x = v.float()
    if kind == BF16X3:
        hi = x.bfloat16().float()
        return hi.double() + (x - hi).bfloat16().double()
    assert kind == F16X3
    x = x.clamp(-65504.0, 65504.0)
    hi = x.half().float()
    return hi.double() + ((x - hi) * 2048.0).half().double() / 2048.0


def gemm_ref(A, W, d, *, bias=None, scale=None, shift=None, rowadd=None, residual=None, ln_stats=None, ln_part_in=None, ln_colsum=None,
             y2_in=None, want_ln_part=False, split=0):
    """The header's epilogue order: v = acc + bias; v = v*scale + shift; v = act(v); v += rowadd[(yrow / div) % mod]; v += residual[yrow]
    (res_half: the pixel (oy/2, ox/2) of the half-resolution tensor); v = relu(v) if post_relu.
    Consumer (ln_colsum set): "rstd_m (acc - mean_m ln_colsum[n]) + bias[n] before the activation", (mean, rstd) = ln_stats rows, or
    mage_ln_stats' arithmetic on ln_part_in with ln_eps (C = K).  ACT_QUICKGELU_GRAD: y = (acc + bias) * QuickGELU'(y2_in).
    want_ln_part: the producer's partial sums of the values it stores, per 64-column slice; y2 is then the same rows (a 16-bit copy).
    residual / rowadd / y2_in are fp64 [rows, >= N] tensors (leading dimension = their row length)."""
    dev = A.device
    img, oy, ox, yrow = row_geometry(d, dev)
    acc, S = product(A, W, d, split)
    mag = {}
    v = acc
    if ln_colsum is not None:
        if ln_stats is not None:
            mean, rstd = ln_stats[:d.M, 0], ln_stats[:d.M, 1]
        else:
            mean, rstd = ln_stats_from_part(ln_part_in[:, :d.M], d.K, d.ln_eps)
        mag["ln_mean_colsum"] = (mean[:, None] * ln_colsum[None]).abs()
        mag["rstd"] = rstd[:, None].abs()
        v = rstd[:, None] * (acc - mean[:, None] * ln_colsum[None])
    if bias is not None:
        mag["bias"] = bias[None].abs().expand_as(v)
        v = v + bias[None]
    if scale is not None:
        mag["scale"], mag["shift"] = scale[None].abs().expand_as(v), shift[None].abs().expand_as(v)
        v = v * scale[None] + shift[None]
    mag["pre_act"] = v.abs()
    pre = v
    if d.act == ACT_QUICKGELU_GRAD:
        v = v * quickgelu_grad(y2_in[yrow, :d.N])
    else:
        v = act_ref(v, d.act)
    if rowadd is not None:
        t = rowadd[(yrow // d.rowadd_div) % d.rowadd_mod, :d.N]
        mag["rowadd"] = t.abs()
        v = v + t
    if residual is not None:
        rrow = img * (d.out_h * d.out_w // 4) + (oy // 2) * (d.out_w // 2) + ox // 2 if d.res_half else yrow
        r = residual[rrow, :d.N]
        mag["residual"] = r.abs()
        v = v + r
    if d.post_relu:
        v = v.clamp(min=0)
    out = SimpleNamespace(yrow=yrow, y=v, S=S, mag=mag, pre=pre, y2=None, ln_part=None)
    if want_ln_part:
        sl = v.reshape(d.M, d.N // 64, 64)
        out.ln_part = torch.stack([sl.sum(-1), (sl * sl).sum(-1)], -1).permute(1, 0, 2)      # [N / 64, M, 2]: row m is output row yrow[m]
        out.y2 = v
    return out


def gemm_head_ref(A, W, d, head_w, *, bias, residual=None):
    """head_w: "the rows y = relu(acc + bias) [with residual: relu((acc + bias) + residual)], rounded to bf16 as a store would round them,
    are NOT written; Y[yrow][t] = sum_n y[n] * head_w[t][n], t = 0..15".  head_phases = 4: N = 4 * 256, column block p = (py, px) "reads its
    2 x 2 window at a_off + py*in_w + px and writes the rows y_off + py*(y_mul_y/2) + px*(y_mul_x/2)".
    Returns one Result per phase: yrow [M], y [M, 16], rows [M, 256] (the rows before their bf16 rounding), S and mag [M, 256] of the rows."""
    outs = []
    for p in range(max(d.head_phases, 1)):
        dp = SimpleNamespace(**vars(d))
        nb = 256
        Wp, bp = W, bias
        if d.head_phases:
            py, px = p // 2, p % 2
            dp.N, dp.a_off, dp.y_off = nb, d.a_off + py * d.in_w + px, d.y_off + py * (d.y_mul_y // 2) + px * (d.y_mul_x // 2)
            Wp, bp = W.reshape(-1)[p * nb * d.ldw:], bias[p * nb:(p + 1) * nb]
        dp.act = ACT_NONE
        r = gemm_ref(A, Wp, dp, bias=bp, residual=residual)
        rows = r.y.clamp(min=0)
        outs.append(SimpleNamespace(yrow=r.yrow, y=store(rows, BF16) @ head_w.t(), rows=rows, S=r.S, mag=r.mag))
    return outs
