"""GPU: every kernel family behind mage_gemm (csrc/gemm_impl.h, gemm4.hip, gemm4h.hip, gemm_f16.hip, conv_tile.hip) against the fp64
restatement of the descriptor contract in tests/gemm_ref.py, at the edges of its dispatch.  One case table (cases), one launch, one check.
Every case names the kernel it means to reach; launch() asks the library (mage_gemm_kernel_name) and refuses to launch anything else, so
this map cannot drift.  Sizes follow from the CU count n the way the dispatch computes them (written here for n = 256).

Which kernel a descriptor reaches, and the cases that reach it (template parameters in the kernel's own order):
  gemm_kernel<DT, GATHER, ACT, MT, EK, SPLIT, LN, NW, SPL, RB>   the lockstep kernel
    DT fp32 (0) / bf16 (1) / f16 (4), plain rows, MT 4: lock_f32_*, lock_bf16_k8, lock_bf16_k72_qgelu, lock_f16_k64, lock_bf16_k2112,
      lock_bf16_below_mt8; MT 8 (256-row tiles >= 2 n, not the 8-phase kernel's: K % 64 != 0, general epilogue, gemm_no_8phase): lock_bf16_mt8_k72,
      lock_bf16_mt8_general, stagger_lock_rb, and the other side of test_8phase_bit_identical_to_the_lockstep_kernel
    EK 0 bias / 1 residual seeded into the accumulators (fp32 residual) or added in the epilogue (RB: the 16-bit stream) / 2 general:
      lock_f32_res*, lock_bf16_rb, lock_*_general*, lock_f32_only_*
    NW 1 (the 256 x 64 tile): narrow_f32_on (N <= 128 at >= one tile per CU; narrow_f32_off one tile below), narrow_arelu*, narrow_gather,
      few-rows x + Linear(.): nfew_*
    GATHER: gather_* (3x3 / pad 1, 4x4 / stride 2, 1x1 / stride 2, dys = dxs = -1, dys = 2 with stride 2, cin 8 / 40 / 64, a_half, res_half)
    SPL 1 / 2 (split precision): spl_*_mt4, spl_*_mt8_lock;  LN 1 / 2: ln_prod_nfew*, ln_prod_mt4, ln_cons_mt4*
  gemm8_kernel<ACT, EK, SPLIT, TAPS, LN, SPL, RB, HF>             the 8-phase kernel
    plain: g8_* (1, 5, 32 slabs; bias, QuickGELU, fp32 residual, 16-bit residual, f16; an edge tile in M and in N), ln_prod_g8*, ln_cons_g8,
      spl_*_mt8, stagger_*
    TAPS (padded taps): taps_table*, taps_conv_*, taps_res*, taps_head* (LN 5), taps_f16_table, taps_bf16x3_table, taps_f16x3_*; next to
      each a descriptor that is not eligible and runs on the generic kernel: taps_off_* (head_w and the split kinds have no generic form:
      their neighbours are the refusals in test_gemm_refuses_a_relu_off_its_tile_and_head_w_off_its_form and
      test_split_precision_refuses_a_geometry_that_is_not_padded_taps).  Same bits as the generic gather where a K slab is one tap (cin = 64:
      test_padded_taps_bit_identical_to_the_generic_gather); cin > 64 and the row-table form are not claimed equal and only meet the bound
  gemm_small_kernel<ACT, EK, LN, RB, RW, SPL, HF>                 few rows: small_* (RW 1, 2, 4), just off each clause of small_shape: small_off_*
  gemm4_kernel<ACT, EK, LN, ., HF> / gemm4h_kernel<ACT, LN, HF>   one wave per SIMD and its split-half form: g4_*, g4h_*
  conv3x3_c64_kernel                                              conv64_*
  SPLIT = true (split-K, lda and ldw > K) on gemm_kernel at MT 4 and 8 and on gemm8_kernel: splitk_*
Not covered here (training-only forms): LN_DUAL (LN 3), LN_GELUBWD (LN 4), option gemm4_train_forms.  tests/gemm_ref.py restates the
QuickGELU-gradient epilogue already (tests/test_gemm_ref_cpu.py); tests/test_gpu_train.py holds what exists for these forms.

Footprint.  Y, y2 and ln_part start as a NaN sentinel of a bit pattern no kernel produces, with ldy > N, rows past the last mapped one and (y_mul_x
= 2, y_img_stride wider than the plane, y_off) gaps between mapped rows: outside the mapped rows and columns every element still holds the
sentinel, inside every element was written.  Cases with Y aliasing the residual (*_alias) compare the outside with a copy of the buffer.

Bounds, per output element, u = 2^-24, S = sum_k |a||w| of the element, from gemm_ref's magnitudes; nothing is excluded, nothing fitted.
  accumulation   fp32 operands: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain (MI355X guide), one rounding per product: gamma_K S, taken as
                 (K + 2) u S.  16-bit operands: the products are exact in fp32; how the 16-bit MFMAs round their internal sums is not stated in
                 the guides and has not been measured here, so 2 u per accumulated term is ALLOWED: 2 K u S (the printed ratios show the slack).
                 Split kinds: three passes, 2 * 3 K u S, plus the dropped lo * lo products at the header's figure (2^-18 S bf16x3, 2^-22 S f16x3);
                 the inputs of the reference are the represented values hi + lo, so no representation term; the f16 form's 2^-11 is exact.
                 The kernels of EK 1 without RB (x + Linear(.) on an fp32 residual, the padded-taps table form) load the residual / the row
                 table INTO the accumulators before the K loop: for the cases whose asserted kernel is one of them, and only for them,
                 S + |residual| + |rowadd| takes the place of S.
  epilogue       one rounding per stage on the running magnitude T (the sum of the magnitudes added so far, so the order of the additions does
                 not matter): bias u T; scale / shift 2 u (T |scale| + |shift|) on top of |scale| times the incoming error; rowadd, residual u T.
                 ReLU and post_relu add nothing (slope <= 1).  QuickGELU as act_apply executes it, v * rcp(1 + exp2(c v)), c = fl(-2.4554669596):
                 |slope| <= 1.1; the scaled argument carries 2 u |c v| (c's own rounding and the product's), which exp2 turns into 1.39 u |c v|
                 = 3.41 u |v| relative; v_exp_f32 and v_rcp_f32 1 ulp = 2 u each (ISA manual), 1 + e one u, the last product one u: |v| u (3.41 |v| + 6).
                 erf-GELU, 0.5 v (1 + erff(0.7071 v)): |slope| <= 1.13; erff is the device libm's, ASSUMED within 4 ulp (8 u absolute, |erf| <= 1), its
                 argument's rounding moves it by < u, three more roundings: 10 u |v|.
  LayerNorm      consumer rstd (acc - mean s_n) + bias: (e_acc + u (S + 2 |mean s_n|)) rstd + u rstd (S + |mean s_n|).  With ln_part + ln_eps the
                 statistics are mage_ln_stats_row's correctly rounded chain over ns = K / 64 slices: d_mean <= (ns + 1) u sum|p0| / K, d_var <=
                 (ns + 1) u E2 + 2 |mean| d_mean + u (E2 + mean^2), d_rstd / rstd <= d_var / (2 (var + eps)) + 3 u.
                 producer: the 64-column partial sums are a tree of depth 8 over the fp32 values v: sum e_v + 8.1 u sum |v|, and for the squares
                 sum (2 |v| e_v + u v^2) + 8.1 u sum v^2.
  store          fp32: nothing more (the last rounding is counted above); bf16 / f16: one ulp of the type at |ref|; split rows as
                 tests/test_gpu_split.py: 2^-17 |ref| (bf16x3), 2^-21 |ref| + 2^-35 (f16x3).  y2 of the producer: the fp32 row's bound + one bf16 ulp.
  head_w         per row value y_n: its fp32 bound e_n, and a bf16 rounding that may fall the other way, ulp_bf16(|y_n| + e_n); the narrow product is
                 256 exact bf16 products summed in fp32 by an MFMA and across four wave columns: sum_n |h_tn| (e_n + ulp_n) + 2 u 260 sum_n |h_tn y_n|."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

from mage_amd import config, ops
from tests import gemm_ref as R
from tests.helpers import unsplit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = {torch.float32: (torch.int32, 0xFFC0DEAD - 2 ** 32), torch.bfloat16: (torch.int16, 0xFFDE - 2 ** 16),
            torch.float16: (torch.int16, 0xFE5A - 2 ** 16)}
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTC = {"f32": 0, "bf16": 1, "f16": 4}
SPLK = {"bf16x3": ops.BF16X3, "f16x3": ops.F16X3}
NONE, RELU, QGELU, ERF = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_QUICKGELU, ops.ACT_GELU_ERF
WORST = {}                                                                  # family -> worst |err| / bound seen in this process


def _b(x):
    return "true" if x else "false"


def gk(dt, gather, act, mt, ek, ln=0, nw=4, spl=0, rb=False, split=False):
    return f"gemm_kernel<{DTC[dt]}, {_b(gather)}, {act}, {mt}, {ek}, {_b(split)}, {ln}, {nw}, {spl}, {_b(rb)}>"


def g8(act, ek, taps=False, ln=0, spl=0, rb=False, hf=False, split=False):
    return f"gemm8_kernel<{act}, {ek}, {_b(split)}, {_b(taps)}, {ln}, {spl}, {_b(rb)}, {_b(hf)}>"


def gs(act, ek, ln=0, rb=False, rw=1, spl=0, hf=False):
    return f"gemm_small_kernel<{act}, {ek}, {ln}, {_b(rb)}, {rw}, {spl}, {_b(hf)}>"


def g4(act, ln=0, hf=False):
    return f"gemm4_kernel<{act}, 0, {ln}, false, {_b(hf)}>"


def g4h(act, ln=0, hf=False):
    return f"gemm4h_kernel<{act}, {ln}, {_b(hf)}>"


def _seeds(kernel):
    """Does this kernel load the residual / the row table INTO its accumulators before the K loop?  EK = 1 without RB (gemm_shared.h)."""
    name, _, args = kernel.partition("<")
    a = [x.strip() for x in args.rstrip(">").split(",")]
    ek, rb = {"gemm_kernel": (4, 9), "gemm8_kernel": (1, 6), "gemm_small_kernel": (1, 3)}.get(name, (None, None))
    return ek is not None and a[ek] == "1" and a[rb] == "false"


def conv_geo(n_img, H, W, cin, k, stride=1, pad=None, dil=1, OH=None, OW=None, **kw):
    """Conv2d(cin, ., k, stride, pad, dilation) on channels-last [n_img, H, W, cin] rows: the fields of the implicit GEMM"""
    pad = k // 2 if pad is None else pad
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1 if OH is None else OH
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1 if OW is None else OW
    return dict(M=n_img * OH * OW, K=k * k * cin, geo=dict(out_h=OH, out_w=OW, in_h=H, in_w=W, taps_h=k, taps_w=k, cin=cin, stride=stride, dy0=-pad,
                                                           dx0=-pad, dys=dil, dxs=dil, **kw))


def padded_geo(n_img, h, w, cin, k, extra_pitch=0, img_extra=0, **kw):
    """k x k / stride 1 over a zero-padded (h + k - 1) x (w + k - 1 + extra_pitch) input: the padded-taps form"""
    ph, pw = h + k - 1, w + k - 1 + extra_pitch
    return dict(M=n_img * h * w, K=k * k * cin, geo=dict(out_h=h, out_w=w, in_h=ph, in_w=pw, taps_h=k, taps_w=k, cin=cin, a_img_stride=ph * pw + img_extra, **kw))


def cases(n):
    """name -> case, for a device of n compute units (n = 256: the sizes in the comments)."""
    big = 256 * n                                                           # rows of 2 n tiles of 256 x 256 at N = 512: the MT = 8 / 8-phase edge
    t = {}

    def add(name, fam, dt, M, N, K, kernel, y=None, **kw):
        assert name not in t, name
        defaults = dict(geo={}, bias=True, scale=False, act=NONE, rowadd=None, res=None, res_half=False, post_relu=False, ln=None, head=0,
                        head_phases=0, a_relu=False, a_half=False, n_split=1, lda_pad=0, ldw_pad=0, ldy_pad=8, ldr_pad=16, alias=False, opts={},
                        tab_off=0)
        t[name] = SimpleNamespace(name=name, fam=fam, dt=dt, y=y or ("f32" if dt in SPLK else dt), M=M, N=N, K=K, kernel=kernel,
                                  seeds=_seeds(kernel), **{**defaults, **kw})

    # ---- lockstep, plain rows, fp32 (MT = 4 always) and 16-bit below 2 n tiles of 256 rows
    add("lock_f32_k4", "lockstep", "f32", 255, 72, 4, gk("f32", 0, NONE, 4, 0))                     # one partial slab, M one row short of 2 tiles, N % 64 != 0
    add("lock_f32_k36_relu", "lockstep", "f32", 257, 264, 36, gk("f32", 0, RELU, 4, 0), act=RELU)   # K % 32 != 0, one row past a tile, 2 column tiles
    add("lock_f32_k32_qgelu", "lockstep", "f32", 128, 256, 32, gk("f32", 0, QGELU, 4, 0), act=QGELU, geo=dict(y_mul_x=2, y_off=3))   # one whole slab
    add("lock_f32_k100_erf", "lockstep", "f32", 129, 64, 100, gk("f32", 0, ERF, 4, 0), act=ERF, lda_pad=12)
    add("lock_f32_nobias_bf16out", "lockstep", "f32", 130, 136, 68, gk("f32", 0, NONE, 4, 0), y="bf16", bias=False)
    add("lock_f32_res", "lockstep", "f32", 300, 136, 68, gk("f32", 0, NONE, 4, 1), res="f32", geo=dict(y_off=2))
    add("lock_f32_res_alias", "lockstep", "f32", 300, 136, 68, gk("f32", 0, NONE, 4, 1), res="f32", alias=True)
    add("lock_f32_general_all", "lockstep", "f32", 301, 72, 44, gk("f32", 0, RELU, 4, 2), act=RELU, scale=True, rowadd=(3, 5), res="f32", post_relu=True,
        geo=dict(y_mul_x=2, y_off=5))
    add("lock_f32_general_qgelu", "lockstep", "f32", 301, 72, 44, gk("f32", 0, QGELU, 4, 2), act=QGELU, scale=True, res="f32")      # the twin of the next
    add("lock_f32_general_alias", "lockstep", "f32", 301, 72, 44, gk("f32", 0, QGELU, 4, 2), act=QGELU, scale=True, res="f32", alias=True)
    add("lock_f32_only_scale", "lockstep", "f32", 64, 64, 40, gk("f32", 0, NONE, 4, 2), scale=True, bias=False)
    add("lock_f32_only_rowadd", "lockstep", "f32", 64, 64, 40, gk("f32", 0, NONE, 4, 2), rowadd=(2, 7), bias=False, geo=dict(y_off=9))
    add("lock_f32_only_res16", "lockstep", "f32", 64, 64, 40, gk("f32", 0, NONE, 4, 2), res="16", bias=False)
    add("lock_f32_only_postrelu", "lockstep", "f32", 64, 64, 40, gk("f32", 0, NONE, 4, 2), post_relu=True, bias=False)
    add("lock_bf16_k8", "lockstep", "bf16", 255, 72, 8, gk("bf16", 0, NONE, 4, 0))
    add("lock_bf16_k72_qgelu", "lockstep", "bf16", 257, 264, 72, gk("bf16", 0, QGELU, 4, 0), act=QGELU, y="f32", lda_pad=8)
    add("lock_f16_k64", "lockstep", "f16", 128, 256, 64, gk("f16", 0, NONE, 4, 0))
    add("lock_f16_k200_qgelu", "lockstep", "f16", 300, 72, 200, gk("f16", 0, QGELU, 4, 0), act=QGELU, y="f32")
    add("lock_bf16_k2112", "lockstep", "bf16", 384, 256, 2112, gk("bf16", 0, NONE, 4, 0), y="f32")   # 33 slabs
    add("lock_bf16_erf","lockstep", "bf16", 129, 72, 136, gk("bf16", 0, ERF, 4, 0), act=ERF)
    add("lock_bf16_rb", "lockstep", "bf16", 1000, 264, 192, gk("bf16", 0, NONE, 4, 1, rb=True), res="16")   # N % 64 != 0: not the narrow few-rows form
    add("lock_bf16_rb_alias", "lockstep", "bf16", 1000, 264, 192, gk("bf16", 0, NONE, 4, 1, rb=True), res="16", alias=True)
    add("lock_f16_rb", "lockstep", "f16", 515, 264, 72, gk("f16", 0, NONE, 4, 1, rb=True), res="16")
    add("lock_bf16_res32", "lockstep", "bf16", 1000, 264, 192, gk("bf16", 0, NONE, 4, 1), res="f32", y="f32")
    add("lock_bf16_general", "lockstep", "bf16", 300, 72, 72, gk("bf16", 0, RELU, 4, 2), act=RELU, scale=True, rowadd=(1, 4), res="16", post_relu=True)
    add("lock_bf16_below_mt8", "lockstep", "bf16", big - 256, 512, 64, gk("bf16", 0, NONE, 4, 0))    # 2 n - 2 tiles of 256 rows: the 128-row tile
    add("lock_bf16_mt8_k72", "lockstep", "bf16", big, 512, 72, gk("bf16", 0, NONE, 8, 0))            # 2 n tiles, K % 64 != 0: not the 8-phase kernel
    add("lock_bf16_mt8_general", "lockstep", "bf16", big + 1, 520, 64, gk("bf16", 0, RELU, 8, 2), act=RELU, scale=True)
    # ---- the 256 x 64 tile
    add("narrow_f32_on", "narrow", "f32", 256 * (n - 1) + 1, 64, 12, gk("f32", 0, RELU, 2, 0, nw=1), act=RELU)     # n tiles, the last of one row
    add("narrow_f32_off", "narrow", "f32", 256 * (n - 1), 64, 12, gk("f32", 0, RELU, 4, 0), act=RELU)              # n - 1 tiles: the 256-column tile
    add("narrow_bf16_n128", "narrow", "bf16", 128 * n, 128, 72, gk("bf16", 0, NONE, 2, 0, nw=1), y="f32")
    add("narrow_arelu", "narrow", "bf16", 256 * n, 64, 64, gk("bf16", 0, NONE, 2, 0, nw=1), a_relu=True)
    add("narrow_arelu_relu", "narrow", "bf16", 128 * n, 72, 200, gk("bf16", 0, RELU, 2, 0, nw=1), a_relu=True, act=RELU, y="f32")
    add("nfew_bf16_res32", "narrow_few", "bf16", 1000, 256, 192, gk("bf16", 0, NONE, 2, 1, nw=1), res="f32", y="f32")
    add("nfew_bf16_rb", "narrow_few", "bf16", 1000, 256, 192, gk("bf16", 0, NONE, 2, 1, nw=1, rb=True), res="16")
    add("nfew_f16_rb", "narrow_few", "f16", 777, 128, 72, gk("f16", 0, NONE, 2, 1, nw=1, rb=True), res="16")   # the twin of the next
    add("nfew_f16_rb_alias", "narrow_few", "f16", 777, 128, 72, gk("f16", 0, NONE, 2, 1, nw=1, rb=True), res="16", alias=True)
    add("nfew_off_bf16", "narrow_few", "bf16", 128 * n, 256, 192, gk("bf16", 0, NONE, 4, 1), res="f32", y="f32")     # tiles4 == n: the 128 x 256 tile stays
    # ---- gather geometry on the lockstep kernel
    add("gather_f32_3x3_c8", "gather", "f32", N=40, kernel=gk("f32", 1, RELU, 4, 0), act=RELU,
        **{**conv_geo(9, 5, 7, 8, 3, y_img_stride=40, y_off=3), "M": 8 * 35 + 11})                                   # M ends inside the last image
    add("gather_bf16_4x4s2_c40", "gather", "bf16", N=72, kernel=gk("bf16", 1, NONE, 4, 0), **conv_geo(7, 10, 6, 40, 4, stride=2, pad=1), lda_pad=8)
    add("gather_bf16_1x1s2_c64", "gather", "bf16", N=64, kernel=gk("bf16", 1, QGELU, 4, 0), act=QGELU, y="f32", **conv_geo(5, 9, 7, 64, 1, stride=2, pad=0))
    add("gather_f16_3x3_c64", "gather", "f16", N=136, kernel=gk("f16", 1, NONE, 4, 0), **conv_geo(3, 6, 5, 64, 3))
    for py, px in ((0, 0), (0, 1), (1, 0), (1, 1)):                         # a transposed convolution's sub-pixel phases, as vqvae_model issues them
        add(f"gather_bf16_phase{py}{px}", "gather", "bf16", 6 * 5 * 7, 72, 4 * 64, gk("bf16", 1, RELU, 4, 2), act=RELU, scale=True,
            geo=dict(out_h=5, out_w=7, taps_h=2, taps_w=2, cin=64, dy0=py, dx0=px, dys=-1, dxs=-1, y_img_stride=4 * 35, y_mul_y=4 * 7, y_mul_x=2,
                     y_off=py * 2 * 7 + px))
    add("gather_f32_s2_dys2", "gather", "f32", 4 * 3 * 5, 40, 4 * 8, gk("f32", 1, NONE, 4, 2), res="f32", bias=False,
        geo=dict(out_h=3, out_w=5, in_h=6, in_w=10, taps_h=2, taps_w=2, cin=8, stride=2, dy0=-1, dx0=-1, dys=2, dxs=2))
    add("gather_bf16_ahalf_reshalf", "gather", "bf16", N=72, kernel=gk("bf16", 1, NONE, 4, 2), res="16", res_half=True, post_relu=True, a_half=True,
        **conv_geo(5, 8, 12, 64, 3, a_img_stride=4 * 6))
    add("gather_f32_dil2_c40", "gather", "f32", N=64, kernel=gk("f32", 1, NONE, 4, 2), scale=True, y="bf16", **conv_geo(3, 9, 7, 40, 3, pad=2, dil=2))
    add("narrow_gather", "narrow", "bf16", N=64, kernel=gk("bf16", 1, RELU, 2, 0, nw=1), act=RELU, **conv_geo((256 * n) // 576 + 1, 24, 24, 64, 3))
    add("conv64_relu", "conv3x3_c64", "bf16", N=64, kernel="conv3x3_c64_kernel", act=RELU, **conv_geo(n // 16, 64, 64, 64, 3, y_img_stride=4096 + 64, y_off=8))
    add("conv64_ahalf", "conv3x3_c64", "bf16", N=64, kernel="conv3x3_c64_kernel", a_half=True, **conv_geo(n // 4, 32, 32, 64, 3, a_img_stride=256))
    add("conv64_off_tiles", "conv3x3_c64", "bf16", N=64, kernel=gk("bf16", 1, RELU, 4, 0), act=RELU, **conv_geo(n // 16 - 1, 64, 64, 64, 3))   # n - 16 tiles
    # ---- the 8-phase kernel, plain rows
    add("g8_bias_k64", "gemm8", "bf16", big, 512, 64, g8(NONE, 0))
    add("g8_qgelu_k320_edges", "gemm8", "bf16", big + 1, 520, 320, g8(QGELU, 0), act=QGELU, y="f32")    # a tile of one row, a column tile of 8 columns
    add("g8_res32_k2048", "gemm8", "bf16", big, 512, 2048, g8(NONE, 1), res="f32", y="f32")
    add("g8_res32_k64", "gemm8", "bf16", big, 512, 64, g8(NONE, 1), res="f32", y="f32")                 # the twin of the next
    add("g8_res32_alias", "gemm8", "bf16", big, 512, 64, g8(NONE, 1), res="f32", y="f32", alias=True)
    add("g8_rb_k64", "gemm8", "bf16", big, 512, 64, g8(NONE, 1, rb=True), res="16")
    add("g8_f16_rb_k320", "gemm8", "f16", big, 512, 320, g8(NONE, 1, rb=True, hf=True), res="16")
    add("g8_f16_qgelu", "gemm8", "f16", big, 512, 64, g8(QGELU, 0, hf=True), act=QGELU)
    add("stagger_g8_res32", "gemm8", "bf16", 256 * 3 * n, 512, 64, g8(NONE, 1), res="f32", y="f32")     # 6 tiles per workgroup, 1 slab: staggered start
    add("stagger_lock_rb", "lockstep", "bf16", 256 * 3 * n, 512, 72, gk("bf16", 0, NONE, 8, 1, rb=True), res="16")
    add("stagger_forced_bias", "gemm8", "bf16", 256 * 3 * n, 512, 64, g8(NONE, 0), opts=dict(gemm_stagger_forced=1))
    # ---- padded taps on the 8-phase kernel, and for each a neighbour that is not eligible
    tab = dict(geo=dict(out_h=1, out_w=256, y_img_stride=300, y_off=7), rowadd=(1, 16))               # rows regrouped 256 at a time + a row table
    add("taps_table_f32", "taps8", "bf16", 512, 256, 64, g8(NONE, 1, taps=True), y="f32", bias=False, **tab)
    add("taps_table_bias_bf16", "taps8", "bf16", 512, 512, 192, g8(NONE, 1, taps=True), **tab)
    add("taps_off_table_m", "taps8", "bf16", 520, 256, 64, gk("bf16", 0, NONE, 4, 2), y="f32", bias=False, **tab)          # M % 256 != 0
    add("taps_off_table_misaligned", "taps8", "bf16", 512, 256, 64, gk("bf16", 0, NONE, 4, 2), y="f32", bias=False, tab_off=2, **tab)
    add("taps_f16_table", "taps8", "f16", 512, 256, 64, g8(NONE, 1, taps=True, hf=True), **tab)
    add("taps_off_f16_table_m", "taps8", "f16", 520, 256, 64, gk("f16", 0, NONE, 4, 2), **tab)                             # M % 256 != 0
    add("taps_bf16x3_table", "taps8", "bf16x3", 512, 256, 64, g8(NONE, 1, taps=True, spl=1), bias=False, **tab)
    add("taps_f16x3_table_split", "taps8", "f16x3", 512, 256, 128, g8(NONE, 1, taps=True, spl=2), y="split", bias=False, **tab)
    add("taps_conv_none", "taps8", "bf16", N=256, kernel=g8(NONE, 0, taps=True), **padded_geo(2, 16, 16, 64, 3, img_extra=5))
    add("taps_conv_relu", "taps8", "bf16", N=256, kernel=g8(RELU, 0, taps=True), act=RELU, **padded_geo(2, 16, 16, 64, 3, extra_pitch=2))
    add("taps_conv_relu_2x2", "taps8", "bf16", N=512, kernel=g8(RELU, 0, taps=True), act=RELU, y="f32",
        **padded_geo(4, 8, 16, 128, 2, extra_pitch=1, a_off=19, y_img_stride=4 * 128, y_mul_y=64, y_mul_x=2, y_off=33))
    add("taps_off_conv_n", "taps8", "bf16", N=264, kernel=gk("bf16", 1, RELU, 4, 0), act=RELU, **padded_geo(2, 16, 16, 64, 3))        # N % 256 != 0
    add("taps_off_conv_imgstride", "taps8", "bf16", N=256, kernel=gk("bf16", 1, NONE, 4, 0), **padded_geo(2, 16, 16, 64, 3, img_extra=-4))   # images overlap
    add("taps_f16x3_conv_relu", "taps8", "f16x3", N=256, kernel=g8(RELU, 0, taps=True, spl=2), act=RELU, y="split", **padded_geo(1, 16, 16, 64, 3))
    add("taps_res", "taps8", "bf16", N=256, kernel=g8(NONE, 0, taps=True, rb=True), res="16", **padded_geo(2, 16, 16, 64, 3))
    add("taps_res_half", "taps8", "bf16", N=256, kernel=g8(NONE, 0, taps=True, rb=True), res="16", res_half=True,
        **padded_geo(2, 16, 16, 64, 3, y_img_stride=300, y_off=4))
    add("taps_off_res_n", "taps8", "bf16", N=264, kernel=gk("bf16", 1, NONE, 4, 2), res="16", res_half=True, **padded_geo(2, 16, 16, 64, 3))
    add("taps_head16", "taps8", "bf16", N=256, kernel=g8(RELU, 0, taps=True, ln=5), act=RELU, y="f32", head=16, ldy_pad=4, **padded_geo(2, 16, 16, 64, 3))
    add("taps_head4", "taps8", "bf16", N=256, kernel=g8(RELU, 0, taps=True, ln=5), act=RELU, y="f32", head=4, ldy_pad=0, **padded_geo(2, 16, 16, 64, 3))
    add("taps_head_res_half", "taps8", "bf16", N=256, kernel=g8(RELU, 0, taps=True, ln=5), act=RELU, y="f32", head=16, res="16", res_half=True,
        **padded_geo(2, 16, 16, 64, 3))
    add("taps_head_phases", "taps8", "bf16", N=1024, kernel=g8(RELU, 0, taps=True, ln=5), act=RELU, y="f32", head=16, head_phases=4,
        **padded_geo(2, 16, 16, 64, 2, extra_pitch=1, img_extra=18, y_img_stride=4 * 256, y_mul_y=64, y_mul_x=2))
    # ---- few rows
    add("small_bias", "small", "bf16", 256, 512, 512, gs(NONE, 0))
    add("small_qgelu_rw2", "small", "bf16", 512, 8 * n, 512, gs(QGELU, 0, rw=2), act=QGELU, y="f32")
    add("small_res32_rw4", "small", "bf16", 1024, 16 * n, 1024, gs(NONE, 1, rw=4), res="f32", y="f32")          # 2 tiles4 == n, M == gemm_small_m
    add("small_res32", "small", "bf16", 200, 512, 512, gs(NONE, 1), res="f32", y="f32")                        # the twin of the next
    add("small_res32_alias", "small", "bf16", 200, 512, 512, gs(NONE, 1), res="f32", y="f32", alias=True)
    add("small_rb", "small", "bf16", 200, 528, 512, gs(NONE, 1, rb=True), res="16")                              # rows and columns that end inside a piece
    add("small_f16_qgelu", "small", "f16", 256, 512, 1024, gs(QGELU, 0, hf=True), act=QGELU)
    add("small_f16x3_bias", "small", "f16x3", 256, 512, 512, gs(NONE, 0, spl=2), lda_pad=64, ldw_pad=64)
    add("small_f16x3_qgelu_split", "small", "f16x3", 200, 512, 512, gs(QGELU, 0, spl=2), act=QGELU, y="split")
    add("small_f16x3_res", "small", "f16x3", 256, 512, 1024, gs(NONE, 1, spl=2), res="f32")
    add("small_cons_stats", "small", "bf16", 256, 512, 512, gs(QGELU, 0, ln=2), act=QGELU, ln="stats")
    add("small_cons_part", "small", "bf16", 256, 768, 512, gs(NONE, 0, ln=2), ln="part", y="f32")
    add("small_f16_cons_part", "small", "f16", 512, 512, 1024, gs(QGELU, 0, ln=2, hf=True), act=QGELU, ln="part")
    add("small_off_k", "small", "bf16", 256, 512, 576, gk("bf16", 0, NONE, 4, 0))                               # K % 512 != 0
    add("small_off_n", "small", "bf16", 256, 520, 512, gk("bf16", 0, NONE, 4, 0))                               # N % 16 != 0
    add("small_off_m", "small", "bf16", 1025, 512, 512, gk("bf16", 0, NONE, 4, 0))                              # M > gemm_small_m
    add("small_off_tiles", "small", "bf16", 1024, 16 * n + 256, 512, gk("bf16", 0, NONE, 4, 0))                         # 2 tiles4 = n + 16
    # ---- LayerNorm folded around the tiled kernels
    add("ln_prod_nfew", "ln_fold", "bf16", 512, 512, 192, gk("bf16", 0, NONE, 2, 1, ln=1, nw=1), res="f32", y="f32", ln="produce")
    add("ln_prod_nfew_rb", "ln_fold", "bf16", 512, 512, 192, gk("bf16", 0, NONE, 2, 1, ln=1, nw=1, rb=True), res="16", ln="produce")
    add("ln_prod_mt4", "ln_fold", "bf16", 512, 512, 192, gk("bf16", 0, NONE, 4, 1, ln=1), res="f32", y="f32", ln="produce", opts=dict(gemm_no_narrow_few=1))
    add("ln_prod_g8", "ln_fold", "bf16", big, 512, 64, g8(NONE, 1, ln=1), res="f32", y="f32", ln="produce")
    add("ln_prod_g8_rb_f16", "ln_fold", "f16", big, 512, 128, g8(NONE, 1, ln=1, rb=True, hf=True), res="16", ln="produce")
    add("ln_cons_mt4", "ln_fold", "bf16", 512, 256, 192, gk("bf16", 0, NONE, 4, 0, ln=2), ln="stats", y="f32")
    add("ln_cons_mt4_qgelu", "ln_fold", "bf16", 512, 256, 192, gk("bf16", 0, QGELU, 4, 0, ln=2), ln="stats", act=QGELU)
    add("ln_cons_g8", "ln_fold", "bf16", big, 512, 64, g8(QGELU, 0, ln=2), ln="stats", act=QGELU)
    # ---- one wave per SIMD (>= 4 n tiles) and its split-half form (K = 512, 16-bit rows out, >= 3 n / 4 tiles)
    add("g4_bias_k256", "gemm4", "bf16", big, 1024, 256, g4(NONE))
    add("g4_f32out_k512", "gemm4", "bf16", big, 1024, 512, g4(NONE), y="f32", bias=False)
    add("g4_qgelu_k1024", "gemm4", "bf16", big, 1024, 1024, g4(QGELU), act=QGELU, y="f32")
    add("g4_f16_cons", "gemm4", "f16", big, 1024, 256, g4(QGELU, ln=2, hf=True), act=QGELU, ln="stats")
    add("g4_off_tiles", "gemm4", "bf16", big - 256, 1024, 256, g8(NONE, 0))                                    # 4 n - 4 tiles: the 8-phase kernel
    add("g4h_qgelu", "gemm4h", "bf16", big // 2, 2048, 512, g4h(QGELU), act=QGELU)
    add("g4h_f16_cons", "gemm4h", "f16", big // 2, 2048, 512, g4h(QGELU, ln=2, hf=True), act=QGELU, ln="stats")
    add("g4h_plain_below", "gemm4h", "bf16", big // 2 - 256, 2048, 512, g4h(NONE))                             # below 4 n tiles: every form
    add("g4h_plain_option", "gemm4h", "bf16", big // 2, 2048, 512, g4h(NONE, ln=2), ln="stats", opts=dict(gemm_4h_plain=1))
    add("g4h_off_plain", "gemm4h", "bf16", big // 2, 2048, 512, g4(NONE))                                       # >= 4 n tiles without QuickGELU: gemm4_kernel
    # ---- split precision on the tiled kernels
    add("spl_bf16x3_mt4", "split", "bf16x3", 1000, 256, 64, gk("bf16", 0, NONE, 4, 0, spl=1), lda_pad=64, ldw_pad=64)
    add("spl_f16x3_mt4_qgelu_split", "split", "f16x3", 1025, 256, 192, gk("bf16", 0, QGELU, 4, 0, spl=2), act=QGELU, y="split")
    add("spl_f16x3_mt4_res", "split", "f16x3", 1025, 264, 64, gk("bf16", 0, NONE, 4, 1, spl=2), res="f32")
    add("spl_bf16x3_mt4_res", "split", "bf16x3", 1000, 256, 128, gk("bf16", 0, NONE, 4, 1, spl=1), res="f32")      # the twin of the next
    add("spl_bf16x3_mt4_res_alias", "split", "bf16x3", 1000, 256, 128, gk("bf16", 0, NONE, 4, 1, spl=1), res="f32", alias=True)
    add("spl_f16x3_mt8", "split", "f16x3", big, 512, 64, g8(NONE, 0, spl=2))
    add("spl_bf16x3_mt8_qgelu_split", "split", "bf16x3", big, 512, 128, g8(QGELU, 0, spl=1), act=QGELU, y="split")
    add("spl_f16x3_mt8_lock_res", "split", "f16x3", big, 512, 64, gk("bf16", 0, NONE, 8, 1, spl=2), res="f32", opts=dict(gemm_no_8phase=1))
    # ---- split-K (the weight-gradient products): n_split slices of A and W side by side in rows of lda, ldw > K, one output block per slice
    add("splitk_f32_mt4", "split_k", "f32", 136, 72, 36, gk("f32", 0, NONE, 4, 0, split=True), bias=False, n_split=3, lda_pad=4, ldw_pad=8)
    add("splitk_bf16_mt4", "split_k", "bf16", 264, 520, 72, gk("bf16", 0, NONE, 4, 0, split=True), y="f32", bias=False, n_split=2, ldw_pad=8)
    add("splitk_bf16_mt8_lock", "split_k", "bf16", 2048, 8 * n, 72, gk("bf16", 0, NONE, 8, 0, split=True), y="f32", bias=False, n_split=8)   # 2 n tiles
    add("splitk_bf16_mt8_g8", "split_k", "bf16", 2048, 8 * n, 128, g8(NONE, 0, split=True), y="f32", bias=False, n_split=8, lda_pad=8)
    add("splitk_bf16_below_mt8", "split_k", "bf16", 2048, 8 * n - 256, 128, gk("bf16", 0, NONE, 4, 0, split=True), y="f32", bias=False, n_split=8)
    return t


NAMES = list(cases(256))


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7


@contextlib.contextmanager
def _options(opts):
    with contextlib.ExitStack() as es:
        for k, v in opts.items():
            es.enter_context(config.lib_option(k, v))
        yield


@contextlib.contextmanager
def _expect_kernel(name, want):
    """Asks mage_gemm_kernel_name for the descriptor ops.gemm built; launches only if it is the kernel the case means to reach."""
    from mage_amd import _lib
    l = _lib.lib(0)
    real = l.mage_gemm
    seen = []

    def spy(d, s):
        seen.append(ops._kernel_name(l, d._obj))
        assert seen[-1] == want, f"{name}: the dispatch picks {seen[-1]}, the case means {want}: nothing launched"
        return real(d, s)
    l.mage_gemm = spy
    try:
        yield seen
    finally:
        l.mage_gemm = real


def _sentinel(rows, cols, dt):
    it, val = SENTINEL[dt]
    return torch.full((rows, cols), val, dtype=it, device=DEV).view(dt)


def _ulp(x, dt):
    """The spacing of dt's values at |x| (bf16: 8 significand bits; f16: 11 bits, subnormals below 2^-14)."""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, -1000.0, e.to(torch.float64) - 1)
    if dt == torch.bfloat16:
        return torch.exp2(e.clamp(min=-126) - 7)
    return torch.exp2(e.clamp(min=-14) - 10)


def _operand(rows, cols, pad, dt, gen, scale=1.0):
    """A random [rows, cols (+ pad)] operand of kind dt on the device: (tensor handed to the library, its leading dimension in the
    descriptor's units, the fp64 values it holds, their leading dimension)."""
    x = (torch.randn(rows, cols + pad, generator=gen) * scale).to(DEV)
    if dt in SPLK:
        xs = ops.split(x, SPLK[dt])
        return xs, 2 * (cols + pad), unsplit(xs, SPLK[dt]), cols + pad
    xs = x.to(TDT[dt])
    return xs, cols + pad, xs.double(), cols + pad


def launch(c, seed=0, kernel="case"):
    """Builds the buffers of case c and runs mage_gemm once.  Returns what check needs: the output buffers, the fp64 values of every input,
    the reference descriptor."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * c.M + 3 * c.N + c.K)
    spl = SPLK.get(c.dt, 0)
    geo = dict(c.geo)
    cin = geo.get("cin", c.K)
    S = c.n_split
    rd = R.desc(c.M, c.N, c.K, lda=cin * S + c.lda_pad, ldw=c.K * S + c.ldw_pad, n_split=S, a_split_stride=c.K * (S > 1),
                w_split_stride=c.K * (S > 1), a_relu=int(c.a_relu), a_half=int(c.a_half), res_half=int(c.res_half), act=c.act,
                post_relu=int(c.post_relu), head_phases=c.head_phases, rowadd_div=c.rowadd[0] if c.rowadd else 1,
                rowadd_mod=c.rowadd[1] if c.rowadd else 1, **geo)
    # A: every row any tap of any GEMM row (of any phase) can address, and two more
    a_rows = max(int(R.tap_rows(rd, ky, kx)[0].max()) for ky in range(rd.taps_h) for kx in range(rd.taps_w)) + 1 + 2
    if c.head_phases:
        a_rows += rd.in_w + 1
    A, lda, Av, _ = _operand(a_rows, cin * S, c.lda_pad, c.dt, gen)
    W, ldw, Wv, _ = _operand(c.N, c.K * S, c.ldw_pad, c.dt, gen, scale=c.K ** -0.5)
    yrow = R.row_geometry(rd)[3]
    y_rows = int(yrow.max()) + 1 + 3 + (rd.y_mul_y // 2 + 1 if c.head_phases else 0)
    f32v = lambda *s, k=1.0: (torch.randn(*s, generator=gen) * k).to(DEV)                                   # noqa: E731
    inp = SimpleNamespace(A=Av, W=Wv, bias=None, scale=None, shift=None, rowadd=None, residual=None, ln_stats=None, ln_part_in=None, ln_colsum=None,
                          head_w=None)
    kw = dict(M=c.M, N=c.N, K=c.K, lda=lda, act=c.act, post_relu=c.post_relu, a_relu=c.a_relu, res_half=c.res_half, a_half=c.a_half, **geo)
    if ldw != (2 * c.K if spl else c.K):
        kw["ldw"] = ldw
    if c.bias:
        kw["bias"] = f32v(c.N)
        inp.bias = kw["bias"].double()
    if c.scale:
        kw["scale"], kw["shift"] = f32v(c.N) * 0.5 + 1.0, f32v(c.N)
        inp.scale, inp.shift = kw["scale"].double(), kw["shift"].double()
    if c.rowadd:
        tabbuf = f32v(c.rowadd[1] * c.N + 8)
        tab = tabbuf[c.tab_off:c.tab_off + c.rowadd[1] * c.N].view(c.rowadd[1], c.N)                        # tab_off 2: a table 8 bytes off a 16-byte boundary
        kw.update(rowadd=tab, rowadd_div=c.rowadd[0], rowadd_mod=c.rowadd[1])
        inp.rowadd = tab.double()
    # the output: N columns (head_w: 16 or 4; split rows: 2N 16-bit pieces) of ldy
    y_dt = ops.split_dtype(spl) if c.y == "split" else TDT[c.y]
    pcols = c.head if c.head else (2 * c.N if c.y == "split" else c.N)
    ldy = pcols + (128 if c.y == "split" else c.ldy_pad)
    res_dt = None if c.res is None else torch.float32 if c.res == "f32" else torch.float16 if c.dt == "f16" else torch.bfloat16
    Y0 = None
    if c.alias:                                                             # the documented in-place form: Y is the residual buffer
        assert res_dt == y_dt and not c.res_half and not c.head
        Y = torch.randn(y_rows, ldy, generator=gen).to(res_dt).to(DEV)
        Y0 = Y.clone()
        kw.update(residual=Y, ldr=ldy)
        inp.residual = Y0.double()
    else:
        Y = _sentinel(S * y_rows, ldy, y_dt)
        if S > 1:                                                           # slice s writes the block of y_rows rows at s * y_split_stride
            kw.update(n_split=S, a_split_stride=c.K, w_split_stride=c.K, y_split_stride=y_rows * ldy)
        if c.res:
            r_rows = (c.M // (rd.out_h * rd.out_w) + 1) * (rd.out_h * rd.out_w // 4) if c.res_half else y_rows
            res = torch.randn(r_rows, c.N + c.ldr_pad, generator=gen).to(res_dt).to(DEV)
            kw.update(residual=res, ldr=c.N + c.ldr_pad)
            inp.residual = res.double()
    kw["ldy"] = ldy
    out = SimpleNamespace(Y=Y, Y0=Y0, y2=None, ln_part=None, pcols=pcols, split_rows=y_rows)
    if c.ln == "produce":
        out.ln_part = _sentinel((c.N // 64 + 1) * (y_rows + 5), 2, torch.float32).view(c.N // 64 + 1, y_rows + 5, 2)
        kw["ln_part"] = out.ln_part
        if c.y == "f32":
            out.y2 = _sentinel(y_rows, c.N + 8, TDT[c.dt])
            kw.update(y2=out.y2, ldy2=c.N + 8)
    if c.ln in ("stats", "part"):
        eps = 1e-5
        x = Av.reshape(-1, lda)[:c.M, :c.K]
        kw["ln_colsum"] = Wv.reshape(c.N, -1)[:, :c.K].sum(1).float()
        inp.ln_colsum = kw["ln_colsum"].double()
        if c.ln == "stats":
            kw["ln_stats"] = torch.stack([x.mean(1), 1 / torch.sqrt(x.var(1, unbiased=False) + eps)], 1).float().contiguous()
            inp.ln_stats = kw["ln_stats"].double()
        else:
            sl = x.reshape(c.M, c.K // 64, 64)
            part = torch.zeros(c.K // 64, c.M + 3, 2, device=DEV)
            part[:, :c.M] = torch.stack([sl.sum(-1), (sl * sl).sum(-1)], -1).permute(1, 0, 2).float()
            kw.update(ln_part=part, ln_eps=eps)
            inp.ln_part_in = part.double()
            rd.ln_eps = eps
    if c.head:
        kw["head_w"] = (torch.randn(16, 256, generator=gen) / 16).to(torch.bfloat16).to(DEV)
        inp.head_w = kw["head_w"].double()
        kw["head_phases"] = c.head_phases
    if spl:
        kw.update(split_kind=spl, y_split=c.y == "split")
    want = c.kernel if kernel == "case" else kernel
    with _options(c.opts), _expect_kernel(c.name, want) as seen:
        ops.gemm(A, W, Y, **kw)
    torch.cuda.synchronize()
    out.kernel = seen[0]
    return out, inp, rd


def accumulation(c, K):
    if c.dt == "f32":
        return (K + 2) * U, 0.0
    if c.dt in SPLK:
        return 2 * U * 3 * K, (2.0 ** -18 if c.dt == "bf16x3" else 2.0 ** -22)
    return 2 * U * K, 0.0


def bound_fp32(c, r, inp, rd):
    """The bound on the epilogue's fp32 value (before the store), per element: the module header's derivation."""
    S, mag = r.S, r.mag
    zero = torch.zeros_like(S)
    bias, tab, res = mag.get("bias", zero), mag.get("rowadd", zero), mag.get("residual", zero)
    cacc, drop = accumulation(c, c.K)
    consumer = "ln_mean_colsum" in mag
    seeded = (res + tab) if c.seeds else zero                              # the asserted kernel's EK decides, not the descriptor
    e = (cacc + drop) * (S + seeded)
    T = S + seeded
    if consumer:
        sm, rstd = mag["ln_mean_colsum"], mag["rstd"]
        e = (e + U * (S + 2 * sm)) * rstd + U * rstd * (S + sm)
        T = rstd * (S + sm)
        if inp.ln_part_in is not None:
            p = inp.ln_part_in[:, :c.M]
            ns, Kf = p.shape[0], float(c.K)
            mean, E2 = p[:, :, 0].sum(0) / Kf, p[:, :, 1].sum(0) / Kf
            var = (E2 - mean * mean).clamp(min=0)
            d_mean = (ns + 1) * U * p[:, :, 0].abs().sum(0) / Kf
            d_var = (ns + 1) * U * E2 + 2 * mean.abs() * d_mean + U * (E2 + mean * mean)
            d_rel = d_var / (2 * (var + rd.ln_eps)) + 3 * U
            e = e + inp.ln_colsum.abs()[None] * rstd * d_mean[:, None] + d_rel[:, None] * T
    if inp.bias is not None:
        T = T + bias
        e = e + U * T
    if c.scale:
        e = e * mag["scale"] + 2 * U * (T * mag["scale"] + mag["shift"])
        T = T * mag["scale"] + mag["shift"]
    if c.act == QGELU:
        v = mag["pre_act"] + e
        e = 1.1 * e + U * v * (3.41 * v + 6)
    elif c.act == ERF:
        e = 1.13 * e + 10 * U * (mag["pre_act"] + e)
    if c.act != NONE:
        T = mag["pre_act"] + e
    if inp.rowadd is not None:
        T = T + tab
        e = e + U * T
    if inp.residual is not None:
        T = T + res
        e = e + U * T
    return e


def store_term(kind, ref):
    if kind == "bf16":
        return _ulp(ref, torch.bfloat16)
    if kind == "f16":
        return _ulp(ref, torch.float16)
    if kind == "bf16x3":
        return 2.0 ** -17 * ref.abs()
    if kind == "f16x3":
        return 2.0 ** -21 * ref.abs() + 2.0 ** -35
    return torch.zeros_like(ref)


def _footprint(name, what, buf, mapped, orig=None):
    """mapped: bool mask of buf's shape.  Outside it the buffer still holds the sentinel (orig given: its earlier bits); inside, no sentinel."""
    it, sval = SENTINEL[buf.dtype]
    bits = buf.view(it)
    if orig is not None:
        touched = (bits != orig.view(it)) & ~mapped
        assert not bool(touched.any()), f"{name}: {int(touched.sum())} elements of {what} changed outside the mapped rows / columns"
        return
    assert bool((bits[~mapped] == sval).all()), f"{name}: {int((bits[~mapped] != sval).sum())} elements of {what} written outside the mapped rows / columns"
    assert bool((bits[mapped] != sval).all()), f"{name}: {int((bits[mapped] == sval).sum())} mapped elements of {what} left unwritten"


def _ratio(name, what, got, ref, b):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in {what}"
    err = (got - ref).abs()
    q = err / b
    ratio = q.max().item()
    i = q.flatten().argmax().item()
    assert ratio <= 1.0, (f"{name}: {what}: |err| {err.flatten()[i].item():.3e} > bound {b.flatten()[i].item():.3e} at element {i} "
                          f"(ref {ref.flatten()[i].item():.9e}, got {got.flatten()[i].item():.9e})")
    return ratio


def check(c, out, inp, rd):
    """The footprint and the bound of every output; prints and returns the worst |err| / bound."""
    epi = dict(bias=inp.bias, scale=inp.scale, shift=inp.shift, rowadd=inp.rowadd, residual=inp.residual)
    Y = out.Y
    if c.head:
        worst, mapped = 0.0, torch.zeros(Y.shape, dtype=torch.bool, device=DEV)
        hc = SimpleNamespace(**{**vars(c), "act": NONE})                                             # the rows before their ReLU: bias (+ residual)
        for p, h in enumerate(R.gemm_head_ref(inp.A, inp.W, rd, inp.head_w, bias=inp.bias, residual=inp.residual)):
            e = bound_fp32(hc, h, inp, rd)
            en = e + _ulp(h.rows + e, torch.bfloat16)
            hw = inp.head_w.abs()
            b = en @ hw.t() + 2 * U * 260 * (h.rows @ hw.t())
            mapped[h.yrow, :c.head] = True
            worst = max(worst, _ratio(c.name, f"Y (phase {p})", Y[h.yrow, :c.head].double(), h.y[:, :c.head], b[:, :c.head]))
        _footprint(c.name, "Y", Y, mapped)
    elif c.n_split > 1:
        worst, mapped = 0.0, torch.zeros(Y.shape, dtype=torch.bool, device=DEV)
        for s in range(c.n_split):
            r = R.gemm_ref(inp.A, inp.W, rd, split=s)
            rows = r.yrow + s * out.split_rows
            mapped[rows, :c.N] = True
            worst = max(worst, _ratio(c.name, f"Y (slice {s})", Y[rows, :c.N].double(), r.y, bound_fp32(c, r, inp, rd) + store_term(c.y, r.y)))
        _footprint(c.name, "Y", Y, mapped)
    else:
        r = R.gemm_ref(inp.A, inp.W, rd, ln_stats=inp.ln_stats, ln_part_in=inp.ln_part_in, ln_colsum=inp.ln_colsum, want_ln_part=c.ln == "produce", **epi)
        e = bound_fp32(c, r, inp, rd)
        mapped = torch.zeros(Y.shape, dtype=torch.bool, device=DEV)
        mapped[r.yrow, :out.pcols] = True
        _footprint(c.name, "Y", Y, mapped, out.Y0)
        if c.y == "split":
            got = unsplit(Y[r.yrow, :out.pcols], SPLK[c.dt])
            kind = c.dt
        else:
            got, kind = Y[r.yrow, :c.N].double(), c.y
        worst = _ratio(c.name, "Y", got, r.y, e + store_term(kind, r.y))
        if out.y2 is not None:
            m2 = torch.zeros(out.y2.shape, dtype=torch.bool, device=DEV)
            m2[r.yrow, :c.N] = True
            _footprint(c.name, "y2", out.y2, m2)
            worst = max(worst, _ratio(c.name, "y2", out.y2[r.yrow, :c.N].double(), r.y, e + store_term(c.dt, r.y)))
        if out.ln_part is not None:
            mp = torch.zeros(out.ln_part.shape, dtype=torch.bool, device=DEV)
            mp[:c.N // 64, r.yrow] = True
            _footprint(c.name, "ln_part", out.ln_part.view(-1, 2), mp.view(-1, 2))
            v, ev = r.y.abs().reshape(c.M, c.N // 64, 64), e.reshape(c.M, c.N // 64, 64)
            b1 = ev.sum(-1) + 8.1 * U * v.sum(-1)
            b2 = (2 * v * ev + U * v * v).sum(-1) + 8.1 * U * (v * v).sum(-1)
            for s in range(c.N // 64):                                                               # slice by slice
                gp = out.ln_part[s, r.yrow].double()
                worst = max(worst, _ratio(c.name, f"ln_part[{s}] sums", gp[:, 0], r.ln_part[s, :, 0], b1[:, s]),
                            _ratio(c.name, f"ln_part[{s}] squares", gp[:, 1], r.ln_part[s, :, 1], b2[:, s]))
    WORST[c.fam] = max(WORST.get(c.fam, 0.0), worst)
    print(f"gemm {c.name} [{c.fam}: {out.kernel}]: worst |err| / bound {worst:.4f} (family so far {WORST[c.fam]:.4f})")
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_gemm_against_fp64(name):
    c = cases(_n_cu())[name]
    check(c, *launch(c))


def _bits(t):
    return None if t is None else t.view(SENTINEL[t.dtype][0])


def _same_bits(c, opts, other_kernel):
    """Case c on its own kernel and, with the library options opts, on other_kernel: the same bits in every output."""
    a = launch(c)[0]
    c2 = SimpleNamespace(**{**vars(c), "opts": {**c.opts, **opts}})
    b = launch(c2, kernel=other_kernel)[0]
    for what in ("Y", "y2", "ln_part"):
        x, y = _bits(getattr(a, what)), _bits(getattr(b, what))
        assert (x is None and y is None) or torch.equal(x, y), f"{c.name}: {what} of {a.kernel} and of {b.kernel} differ in {int((x != y).sum())} elements"


@pytest.mark.parametrize("name,lock", [
    ("g8_bias_k64", gk("bf16", 0, NONE, 8, 0)), ("g8_qgelu_k320_edges", gk("bf16", 0, QGELU, 8, 0)), ("g8_res32_k2048", gk("bf16", 0, NONE, 8, 1)),
    ("g8_rb_k64", gk("bf16", 0, NONE, 8, 1, rb=True)), ("g8_f16_rb_k320", gk("f16", 0, NONE, 8, 1, rb=True)), ("ln_prod_g8", gk("bf16", 0, NONE, 8, 1, ln=1)),
    ("ln_cons_g8", gk("bf16", 0, QGELU, 8, 0, ln=2)), ("spl_f16x3_mt8", gk("bf16", 0, NONE, 8, 0, spl=2))])
def test_8phase_bit_identical_to_the_lockstep_kernel(name, lock):
    """include/mage_hip.h: "same bits per output element from all of them" -- the 8-phase kernel against the lockstep one (gemm_no_8phase)."""
    _same_bits(cases(_n_cu())[name], dict(gemm_no_8phase=1), lock)


@pytest.mark.parametrize("name,opts,tiled", [
    ("small_bias", dict(gemm_no_small=1), gk("bf16", 0, NONE, 4, 0)), ("small_qgelu_rw2", dict(gemm_no_small=1), gk("bf16", 0, QGELU, 4, 0)),
    ("small_res32_rw4", dict(gemm_no_small=1, gemm_no_narrow_few=1), gk("bf16", 0, NONE, 4, 1)),
    ("small_rb", dict(gemm_no_small=1), gk("bf16", 0, NONE, 4, 1, rb=True)), ("small_f16_qgelu", dict(gemm_no_small=1), gk("f16", 0, QGELU, 4, 0)),
    ("small_cons_stats", dict(gemm_no_small=1), gk("bf16", 0, QGELU, 4, 0, ln=2)), ("small_f16x3_res", dict(gemm_no_small=1), gk("bf16", 0, NONE, 4, 1, spl=2)),
    ("nfew_bf16_res32", dict(gemm_no_narrow_few=1), gk("bf16", 0, NONE, 4, 1)), ("nfew_bf16_rb", dict(gemm_no_narrow_few=1), gk("bf16", 0, NONE, 4, 1, rb=True)),
    ("ln_prod_nfew_rb", dict(gemm_no_narrow_few=1), gk("bf16", 0, NONE, 4, 1, ln=1, rb=True))])
def test_few_rows_kernels_bit_identical_to_the_tiled_kernel(name, opts, tiled):
    """gemm_impl.h: gemm_small_kernel "the same bits from all three kernels"; the narrow few-rows tile "the tokens stay bit-identical to the
    full loop's" -- against the 128 x 256 tile of the lockstep kernel (gemm_no_small, gemm_no_narrow_few)."""
    _same_bits(cases(_n_cu())[name], opts, tiled)


@pytest.mark.parametrize("name,generic", [
    ("taps_conv_none", gk("bf16", 1, NONE, 4, 0)), ("taps_conv_relu", gk("bf16", 1, RELU, 4, 0)), ("taps_res", gk("bf16", 1, NONE, 4, 2)),
    ("taps_res_half", gk("bf16", 1, NONE, 4, 2))])
def test_padded_taps_bit_identical_to_the_generic_gather(name, generic):
    """include/mage_hip.h names the padded-taps forms among the kernels that give the same bits: the padded-taps convolutions with cin = 64 (a K
    slab is one tap, so both kernels sum in the same order; the residual is added after the bias in both), against the generic gather
    kernel on the SAME padded descriptor (gemm_no_taps8).  Not claimed and not tested equal: cin > 64 (taps_conv_relu_2x2: the slabs of a tap
    are summed in another order), the row-table form (taps_table*: the table seeds the accumulators, the generic kernel adds it after the
    product), head_w (it has no generic form: refused) and the split kinds (they run nowhere else).  Those meet the fp64 bound on both sides
    of their taps_* / taps_off_* pairs."""
    _same_bits(cases(_n_cu())[name], dict(gemm_no_taps8=1), generic)


@pytest.mark.parametrize("name", ["stagger_g8_res32", "stagger_lock_rb", "stagger_forced_bias"])
def test_staggered_start_changes_no_bit(name):
    c = cases(_n_cu())[name]
    _same_bits(c, dict(gemm_stagger_groups=0, gemm_stagger_forced=0), c.kernel)


def test_head_phases_equal_four_single_phase_launches():
    """include/mage_hip.h, head_phases: "four launches' tiles, bit for bit, from one tile list"."""
    c = cases(_n_cu())["taps_head_phases"]
    out, inp, rd = launch(c)
    for p in range(4):
        py, px = p // 2, p % 2
        # the same operands (bf16 values, so the way back from fp64 is exact): phase p's W rows and bias, its window and its rows
        geo = dict(c.geo, a_off=rd.a_off + py * rd.in_w + px, y_off=rd.y_off + py * (rd.y_mul_y // 2) + px * (rd.y_mul_x // 2))
        rows = R.row_geometry(R.desc(c.M, 256, c.K, **geo))[3].to(DEV)
        Y1 = _sentinel(out.Y.shape[0], out.Y.shape[1], torch.float32)
        with _expect_kernel(c.name, c.kernel):
            ops.gemm(inp.A.to(torch.bfloat16), inp.W.reshape(c.N, -1)[p * 256:(p + 1) * 256].to(torch.bfloat16).contiguous(), Y1, M=c.M, N=256, K=c.K,
                     lda=rd.lda, ldy=out.Y.shape[1], act=RELU, head_w=inp.head_w.to(torch.bfloat16), bias=inp.bias[p * 256:(p + 1) * 256].float().contiguous(),
                     **geo)
        torch.cuda.synchronize()
        assert torch.equal(_bits(Y1)[rows, :16], _bits(out.Y)[rows, :16]), f"phase {p} of the four-phase launch differs from its own launch"


def test_span_limit_of_the_8phase_kernel_by_name():
    """A spans 2^32 bytes or more: 32-bit offsets do not reach, the lockstep kernel runs.  Asked by name only: nothing that size is launched."""
    from mage_amd import _lib
    l = _lib.lib(0)
    n = _n_cu()
    M = 256 * n
    z = torch.zeros(8, device=DEV, dtype=torch.bfloat16)
    # the limit: (M + 1) * lda * 2 bytes against 2^32 -- the largest multiple of 8 below it and the smallest at or above it (n = 256: 32760, 32768)
    below, above = (2 ** 31 - 1) // (M + 1) // 8 * 8, (-(-2 ** 31 // (M + 1)) + 7) // 8 * 8
    assert (M + 1) * below * 2 < 2 ** 32 <= (M + 1) * above * 2 and below >= 64
    for lda, want in ((below, g8(NONE, 0)), (above, gk("bf16", 0, NONE, 8, 0))):
        d = _lib.GemmDesc(dtype=ops.BF16, M=M, N=512, K=64, A=z.data_ptr(), W=z.data_ptr(), Y=z.data_ptr(), lda=lda, ldy=512, y_dtype=ops.BF16, out_h=1,
                          out_w=M, in_h=1, in_w=M, a_img_stride=M, taps_h=1, taps_w=1, cin=64, stride=1, dys=1, dxs=1, y_img_stride=M, y_mul_y=M, y_mul_x=1)
        assert ops._kernel_name(l, d) == want, (lda, ops._kernel_name(l, d))


# ---- refusals: MAGE_EINVAL / MAGE_EUNSUPPORTED before anything is launched; Y keeps its sentinel
def _refused(match, exc=ValueError, **kw):
    Y = kw["y"]
    with pytest.raises(exc, match=match):
        ops.gemm(kw.pop("a"), kw.pop("w"), kw.pop("y"), **kw)
    torch.cuda.synchronize()
    it, sval = SENTINEL[Y.dtype]
    base = Y._base if Y._base is not None else Y
    assert bool((base.view(it) == sval).all()), "a refused call wrote to Y"


def _plain(dt, M=256, N=256, K=64, y_dt=None, **kw):
    t = TDT[dt]
    return dict(a=torch.zeros(M + 1, K, device=DEV, dtype=t), w=torch.zeros(N + 1, K, device=DEV, dtype=t), y=_sentinel(M + 1, N, y_dt or t),
                M=M, N=N, K=K, lda=K, ldy=N, **kw)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("which", ["a", "w", "y"])
def test_gemm_refuses_operands_8_bytes_off(dt, which):
    kw = _plain(dt)
    off = 8 // kw[which].element_size()
    kw[which] = kw[which].view(-1)[off:]
    _refused("16-byte aligned", **kw)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_gemm_refuses_a_w_row_stride_below_k_or_one_its_kernel_ignores(dt):
    _refused("ldw=56 < K=64", **_plain(dt, ldw=56))
    _refused("ldw=72 != K=64", **_plain(dt, ldw=72))
    n = _n_cu()
    _refused("ldw=520 != K=512", **_plain(dt, M=256 * n // 2, N=2048, K=512, ldw=520))                # a gemm4h / gemm4 shape: they would honour it, the rule is one


def test_gemm_refuses_a_relu_off_its_tile_and_head_w_off_its_form():
    _refused("a_relu", **_plain("bf16", a_relu=True))                                                # N = 256
    _refused("a_relu runs on the 256 x 64 tile", **_plain("bf16", N=64, a_relu=True))                # N <= 128 but below one tile per CU
    hw = torch.zeros(16, 256, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(256, device=DEV)
    _refused("head_w", **_plain("bf16", y_dt=torch.float32, head_w=hw, bias=b, act=RELU))           # plain rows: not the padded-taps form
    pad = dict(a=torch.zeros(18 * 18 + 1, 64, device=DEV, dtype=torch.bfloat16), w=torch.zeros(256, 576, device=DEV, dtype=torch.bfloat16), M=256, N=256,
               K=576, lda=64, ldy=256, out_h=16, out_w=16, in_h=18, in_w=18, taps_h=3, taps_w=3, bias=b, head_w=hw)
    _refused("head_w takes the bf16 padded-taps form", y=_sentinel(256, 256, torch.float32), **pad)   # act none


@pytest.mark.parametrize("kind", [ops.BF16X3, ops.F16X3])
def test_split_precision_refuses_a_geometry_that_is_not_padded_taps(kind):
    from mage_amd import _lib
    tab = torch.zeros(16, 256, device=DEV)
    kw = dict(a=ops.split_empty(521, 64, kind, DEV, zero=True), w=ops.split_empty(256, 64, kind, DEV, zero=True), y=_sentinel(521, 256, torch.float32),
              M=520, N=256, K=64, lda=128, ldy=256, out_h=1, out_w=260, rowadd=tab, rowadd_mod=16, split_kind=kind)   # M % 256 != 0
    _refused("not eligible for the padded-taps kernel", exc=_lib.MageHipError, **kw)
