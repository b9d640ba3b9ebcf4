"""CPU: tests/gemm_ref.py -- the fp64 restatement of the mage_gemm_desc contract that tests/test_gpu_gemm.py measures every GEMM kernel
against -- pinned against torch's own operators in fp64 on small shapes.  Channels-last throughout: an [n, C, H, W] tensor is the row
matrix [n*H*W, C]; a Conv2d weight [cout, cin, kh, kw] is the GEMM's W [cout, (ky, kx, ci)]."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R

TOL = 1e-12


def _rows(x):
    """[n, C, H, W] -> [n*H*W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _wrows(w):
    """Conv2d weight [cout, cin, kh, kw] -> [cout, kh*kw*cin], ci fastest"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= TOL * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


@pytest.mark.parametrize("k,stride,pad,dil,H,W", [(3, 1, 1, 1, 5, 7), (4, 2, 1, 1, 8, 6), (1, 1, 0, 1, 3, 4), (3, 2, 2, 2, 9, 7), (3, 1, 0, 1, 6, 5),
                                                  (2, 1, 1, 3, 7, 4)])
def test_gather_is_conv2d(k, stride, pad, dil, H, W):
    n, cin, cout = 3, 8, 16
    x, w, b = _rand(n, cin, H, W, seed=1), _rand(cout, cin, k, k, seed=2), _rand(cout, seed=3)
    want = F.conv2d(x, w, b, stride=stride, padding=pad, dilation=dil)
    OH, OW = want.shape[2:]
    d = R.desc(n * OH * OW, cout, k * k * cin, out_h=OH, out_w=OW, in_h=H, in_w=W, taps_h=k, taps_w=k, cin=cin, stride=stride, dy0=-pad, dx0=-pad,
               dys=dil, dxs=dil)
    r = R.gemm_ref(_rows(x), _wrows(w), d, bias=b)
    _close(r.y, _rows(want))
    assert torch.equal(r.yrow, torch.arange(d.M))
    # S: the same convolution of the magnitudes
    _close(r.S, _rows(F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=pad, dilation=dil)))


def test_leading_dimensions_offsets_and_an_incomplete_last_image():
    """lda > cin, ldw > K, a_off, a_img_stride wider than the plane, M that ends inside an image, the output row map with y_off, y_mul_x = 2
    and y_img_stride wider than the plane."""
    n, cin, cout, H, W, lda, a_off, plane_pitch = 3, 8, 16, 4, 5, 24, 7, 4 * 5 + 3
    x, w = _rand(n, cin, H, W, seed=4), _rand(cout, cin, 3, 3, seed=5)
    want = _rows(F.conv2d(x, w, None, padding=1))
    buf = _rand(a_off + n * plane_pitch, lda, seed=6)
    for i in range(n):
        buf[a_off + i * plane_pitch: a_off + i * plane_pitch + H * W, :cin] = _rows(x[i:i + 1])
    K = 9 * cin
    wbuf = _rand(cout, K + 8, seed=7)
    wbuf[:, :K] = _wrows(w)
    M = 2 * H * W + 7
    d = R.desc(M, cout, K, lda=lda, ldw=K + 8, out_h=H, out_w=W, taps_h=3, taps_w=3, cin=cin, dy0=-1, dx0=-1, a_img_stride=plane_pitch, a_off=a_off,
               y_img_stride=2 * H * W + 11, y_mul_y=2 * W, y_mul_x=2, y_off=3)
    r = R.gemm_ref(buf, wbuf, d)
    _close(r.y, want[:M])
    m = torch.arange(M)
    assert torch.equal(r.yrow, (m // (H * W)) * (2 * H * W + 11) + ((m // W) % H) * 2 * W + (m % W) * 2 + 3)


def test_four_subpixel_phases_are_conv_transpose2d():
    """ConvTranspose2d(cin, cout, 4, 2, 1) as the four 2 x 2 sub-pixel GEMMs with dys = dxs = -1 and dy0 = py, dx0 = px, each writing its
    pixels of the 2h x 2w output through y_mul_x = 2 (the way the VQ-VAE decoder issues it)."""
    n, cin, cout, h, wd = 2, 8, 16, 3, 5
    x, wt, b = _rand(n, cin, h, wd, seed=8), _rand(cin, cout, 4, 4, seed=9), _rand(cout, seed=10)
    want = _rows(F.conv_transpose2d(x, wt, b, stride=2, padding=1))
    got = torch.full_like(want, float("nan"))
    for py in range(2):
        for px in range(2):
            kys = [py + 1 - 2 * (py - k2) for k2 in range(2)]
            kxs = [px + 1 - 2 * (px - k2) for k2 in range(2)]
            sub = wt[:, :, kys][:, :, :, kxs].permute(1, 2, 3, 0).reshape(cout, -1)
            d = R.desc(n * h * wd, cout, 4 * cin, out_h=h, out_w=wd, taps_h=2, taps_w=2, cin=cin, dy0=py, dx0=px, dys=-1, dxs=-1,
                       y_img_stride=4 * h * wd, y_mul_y=4 * wd, y_mul_x=2, y_off=py * 2 * wd + px)
            r = R.gemm_ref(_rows(x), sub, d, bias=b)
            assert bool(torch.isnan(got[r.yrow]).all())                      # every output pixel belongs to exactly one phase
            got[r.yrow] = r.y
    _close(got, want)


def test_stride_2_with_dys_2_and_negative_dy0_is_the_transposed_convolutions_data_gradient():
    """The gradient of ConvTranspose2d(4, 2, 1) with respect to its input, phase by phase, as vqvae_train issues it: stride = 2, dys = dxs = 2,
    dy0 = -py over the 2h x 2w gradient; the four phases add up through the residual."""
    n, cin, cout, h, wd = 2, 8, 16, 3, 4
    x = _rand(n, cin, h, wd, seed=11).requires_grad_()
    wt, g = _rand(cin, cout, 4, 4, seed=12), _rand(n, cout, 2 * h, 2 * wd, seed=13)
    (F.conv_transpose2d(x, wt, None, stride=2, padding=1) * g).sum().backward()
    # input pixel (iy, ix) reaches output (2 iy - 1 + ky, 2 ix - 1 + kx): tap (k2y, k2x) of phase (py, px) is ky = 1 - py + 2 k2y
    du = None
    for py in range(2):
        for px in range(2):
            sub = wt[:, :, [1 - py, 3 - py]][:, :, :, [1 - px, 3 - px]].permute(0, 2, 3, 1).reshape(cin, -1)      # [ci, (k2y, k2x, co)]
            d = R.desc(n * h * wd, cin, 4 * cout, out_h=h, out_w=wd, in_h=2 * h, in_w=2 * wd, taps_h=2, taps_w=2, cin=cout, stride=2,
                       dy0=-py, dx0=-px, dys=2, dxs=2)
            du = R.gemm_ref(_rows(g), sub, d, residual=du).y
    _close(du, _rows(x.grad))


def test_a_half_is_upsample_in_front_of_a_convolution_and_res_half_on_the_skip_path():
    n, cin, cout, h, wd = 2, 8, 16, 3, 4
    x, w, b, skip = _rand(n, cin, h, wd, seed=14), _rand(cout, cin, 3, 3, seed=15), _rand(cout, seed=16), _rand(n, cout, h, wd, seed=17)
    up = torch.nn.Upsample(scale_factor=2)
    want = F.conv2d(up(x), w, b, padding=1) + up(skip)
    d = R.desc(n * 4 * h * wd, cout, 9 * cin, out_h=2 * h, out_w=2 * wd, in_h=2 * h, in_w=2 * wd, taps_h=3, taps_w=3, cin=cin, dy0=-1, dx0=-1,
               a_img_stride=h * wd, a_half=1, res_half=1)
    _close(R.gemm_ref(_rows(x), _wrows(w), d, bias=b, residual=_rows(skip)).y, _rows(want))


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_QUICKGELU, R.ACT_GELU_ERF])
def test_epilogue_order(act):
    """bias, BatchNorm(eval) as scale / shift, the activation, the row table indexed with (yrow / div) % mod, the residual at yrow, post_relu."""
    M, N, K, div, mod, y_off = 24, 16, 8, 2, 5, 3
    a, w, b, sc, sh = _rand(M, K, seed=18), _rand(N, K, seed=19), _rand(N, seed=20), _rand(N, seed=21), _rand(N, seed=22)
    tab, res = _rand(mod, N, seed=23), _rand(M + y_off, N + 8, seed=24)
    d = R.desc(M, N, K, act=act, rowadd_div=div, rowadd_mod=mod, y_off=y_off, post_relu=1)
    r = R.gemm_ref(a, w, d, bias=b, scale=sc, shift=sh, rowadd=tab, residual=res)
    v = (a @ w.t() + b) * sc + sh
    v = {R.ACT_NONE: v, R.ACT_RELU: F.relu(v), R.ACT_QUICKGELU: v * torch.sigmoid(1.702 * v), R.ACT_GELU_ERF: F.gelu(v)}[act]
    yrow = torch.arange(M) + y_off
    want = F.relu(v + tab[(yrow // div) % mod] + res[yrow, :N])
    _close(r.y, want)
    for name in ("bias", "scale", "shift", "pre_act", "rowadd", "residual"):
        assert r.mag[name].shape == (M, N) and bool((r.mag[name] >= 0).all())
    _close(r.mag["pre_act"], ((a @ w.t() + b) * sc + sh).abs())


def test_a_relu_and_the_quickgelu_gradient_epilogue():
    M, N, K = 16, 64, 16
    a, w, b = _rand(M, K, seed=25), _rand(N, K, seed=26), _rand(N, seed=27)
    _close(R.gemm_ref(a, w, R.desc(M, N, K, a_relu=1), bias=b).y, F.relu(a) @ w.t() + b)
    x = _rand(M, N, seed=28).requires_grad_()
    (x * torch.sigmoid(1.702 * x)).sum().backward()
    r = R.gemm_ref(a, w, R.desc(M, N, K, act=R.ACT_QUICKGELU_GRAD), y2_in=x.detach())
    _close(r.y, (a @ w.t()) * x.grad)


def test_layernorm_folded_around_a_linear():
    """Producer x = r + Linear(.) with its per-slice partial sums, mage_ln_stats' arithmetic, and the consumer
    rstd (x W'^T - mean colsum) + bias' = Linear(LayerNorm(x)) with W' = gamma W, bias' = W beta + b."""
    M, C, N, eps = 12, 128, 64, 1e-5
    a0, w0, b0, res = _rand(M, 32, seed=29), _rand(C, 32, seed=30), _rand(C, seed=31), _rand(M, C, seed=32)
    p = R.gemm_ref(a0, w0, R.desc(M, C, 32), bias=b0, residual=res, want_ln_part=True)
    x = res + a0 @ w0.t() + b0
    _close(p.y, x)
    _close(p.y2, x)
    assert p.ln_part.shape == (C // 64, M, 2)
    _close(p.ln_part[1, :, 0], x[:, 64:].sum(1))
    _close(p.ln_part[0, :, 1], (x[:, :64] ** 2).sum(1))
    gamma, beta, w, b = _rand(C, seed=33), _rand(C, seed=34), _rand(N, C, seed=35), _rand(N, seed=36)
    want = F.linear(F.layer_norm(x, (C,), gamma, beta, eps), w, b)
    wp, bp = w * gamma[None], w @ beta + b
    mean, rstd = R.ln_stats_from_part(p.ln_part, C, eps)
    _close(mean, x.mean(1))
    _close(rstd, 1 / torch.sqrt(x.var(1, unbiased=False) + eps))
    stats = torch.stack([mean, rstd], 1)
    for kw in (dict(ln_stats=stats), dict(ln_part_in=p.ln_part)):
        r = R.gemm_ref(x, wp, R.desc(M, N, C, ln_eps=eps, act=R.ACT_QUICKGELU), bias=bp, ln_colsum=wp.sum(1), **kw)
        assert (r.y - want * torch.sigmoid(1.702 * want)).abs().max().item() < 1e-10
        assert set(r.mag) >= {"ln_mean_colsum", "rstd", "bias", "pre_act"}


def test_split_k_slices_add_up_to_the_product():
    N_out, K_out, S, Mc = 16, 24, 3, 8
    dyT, xT = _rand(N_out, S * Mc, seed=37), _rand(K_out, S * Mc, seed=38)
    d = R.desc(N_out, K_out, Mc, lda=S * Mc, ldw=S * Mc, n_split=S, a_split_stride=Mc, w_split_stride=Mc)
    parts = [R.gemm_ref(dyT, xT, d, split=s).y for s in range(S)]
    _close(parts[1], dyT[:, Mc:2 * Mc] @ xT[:, Mc:2 * Mc].t())
    _close(sum(parts), dyT @ xT.t())


@pytest.mark.parametrize("phases", [0, 4])
def test_head_w_is_a_narrow_linear_on_the_bf16_rounded_rows(phases):
    n, cin, h, wd, N = 1, 8, 4, 4, 256
    taps = 2 if phases else 3
    ph, pw = h + taps - 1 + (1 if phases else 0), wd + taps - 1 + (1 if phases else 0)                   # the zero-padded input
    x, hw = _rand(n * ph * pw, cin, seed=39), _rand(16, N, seed=40)
    w, b = _rand(max(phases, 1) * N, taps * taps * cin, seed=41) / 8, _rand(max(phases, 1) * N, seed=42)
    kw = dict(out_h=h, out_w=wd, in_h=ph, in_w=pw, taps_h=taps, taps_w=taps, cin=cin)
    if not phases:
        res = _rand(n * h * wd, N, seed=43)
        o, = R.gemm_head_ref(x, w, R.desc(n * h * wd, N, 9 * cin, **kw), hw, bias=b, residual=res)
        full = R.gemm_ref(x, w, R.desc(n * h * wd, N, 9 * cin, **kw), bias=b, residual=res).y
        _close(o.rows, F.relu(full))
        _close(o.y, F.relu(full).float().bfloat16().double() @ hw.t())
        assert set(o.mag) >= {"bias", "residual"} and o.S.shape == (n * h * wd, N)
        return
    d = R.desc(n * h * wd, 4 * N, 4 * cin, head_phases=4, y_img_stride=4 * h * wd, y_mul_y=4 * wd, y_mul_x=2, **kw)
    outs = R.gemm_head_ref(x, w, d, hw, bias=b)
    seen = torch.cat([o.yrow for o in outs])
    assert sorted(seen.tolist()) == list(range(4 * h * wd))                # the four phases tile the 2h x 2w output
    for p, o in enumerate(outs):
        py, px, yrow, y = p // 2, p % 2, o.yrow, o.y
        one = R.desc(n * h * wd, N, 4 * cin, a_off=py * pw + px, y_img_stride=4 * h * wd, y_mul_y=4 * wd, y_mul_x=2, y_off=py * 2 * wd + px, **kw)
        r = R.gemm_ref(x, w[p * N:(p + 1) * N], one, bias=b[p * N:(p + 1) * N])
        assert torch.equal(yrow, r.yrow)
        _close(y, F.relu(r.y).float().bfloat16().double() @ hw.t())


def test_store_rounds_like_the_output_types():
    v = _rand(64, 64, seed=44) * 3
    v[0, :4] = torch.tensor([0.0, 1e-6, 70000.0, -70000.0], dtype=torch.float64)
    assert torch.equal(R.store(v, R.F32), v.float().double())
    assert torch.equal(R.store(v, R.BF16), v.float().bfloat16().double()) and torch.equal(R.store(v, R.F16), v.float().half().double())
    x = v.float().double()
    assert bool(((R.store(v, R.BF16X3) - x).abs() <= 2.0 ** -17 * x.abs()).all())
    xc = x.clamp(-65504, 65504)                                           # "|x| clamped to 65504"
    assert bool(((R.store(v, R.F16X3) - xc).abs() <= 2.0 ** -21 * xc.abs() + 2.0 ** -35).all())
    assert R.store(v, R.F16X3)[0, 2].item() == 65504.0 and R.store(v, R.F16X3)[0, 3].item() == -65504.0
