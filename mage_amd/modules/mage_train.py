"""Training path of MAGE on the HIP kernels: ``loss, _ = model(batch); loss.backward()``.

The reference trains with ``loss.backward(); optimizer.step()`` (main_mage.py:150-153) through PyTorch autograd.  Here the
whole teacher-forced pass is ONE ``torch.autograd.Function``: ``forward`` runs the same libmage_hip.so kernels as inference
while keeping what the backward pass needs (the LayerNorm inputs, qkv, attention outputs, MLP pre-activations), ``backward``
walks the graph by hand and hands autograd one gradient per parameter -- so ``.grad`` fields, optimizers and
``DistributedDataParallel`` hooks see exactly what they see with the reference.

Dense gradients are MFMA GEMMs: dX = dY W runs the forward kernel on a transposed weight copy; dW = dY^T X contracts over all
tokens into a small [N, K] matrix, so both operands are transposed once (mage_transpose) and multiplied in ONE split-K launch
(mage_gemm n_split) whose partials are summed in a fixed order.  The activation and cross-entropy backward, the embedding scatter and
the positional-table reductions are the kernels of csrc/train.hip; the LayerNorm backward is in csrc/norm.hip, attention's in
csrc/attention_bwd.hip.

Built for every config family of the reference: the MNIST configs of BASELINE cfg1-3; with the randomness branch of
modules/mage_train_prior.py (Conv3d video prior, reparameterisation + KL, ADAIN) config/mage_caterv1.yaml / mage_caterv2.yaml; and
MAGE+ (config/mage+_*.yaml: use_cids=False -- Linear token embedding of the first stage's latents, GroupNorm + SiLU + Conv3d head,
MSE loss, the ln_q / ln_kv TransformerBlock variant, PID-controlled beta).  The first stage is frozen, as in the reference
(mage_model.py:516-521).  Dropout (training mode only) is a stateless mask recomputed in the
backward pass from a per-call seed.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import config, ops
from .vqvae_model import VectorQuantizedVAE

F32 = torch.float32
BF16 = torch.bfloat16

__all__ = ["MageLossFn", "train_forward", "train_backward", "trainable_names"]


def _sfx(dt):
    return ".f32" if dt == F32 else ".bf16"


def _wt(d: Dict[str, torch.Tensor], name: str, dt) -> torch.Tensor:
    """Transposed copy [K, N] of the Linear weight `name` ([N, K]) in dt: the W operand of dX = dY W (a derived cache like the
    bf16 copies; rebuilt with them when a parameter changes)."""
    key = name + ".T" + _sfx(dt)
    if key not in d:
        d[key] = d[name + _sfx(dt)].t().contiguous()
    return d[key]


class _Run:
    """Per-call state: compute dtype, dropout probability and seeds; sk / split_w: the split kind of the fp32 products (_gemm32; 0: exact fp32)
    and the split weight copies of this call."""

    def __init__(self, dt, p: float, training: bool):
        self.sk, self.split_w = 0, {}
        self.dt = dt
        self.p = float(p) if training else 0.0
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.p > 0 else 0
        if self.p > 0 and torch.distributed.is_available() and torch.distributed.is_initialized():
            self.seed += 1000003 * torch.distributed.get_rank()       # identically seeded data-parallel ranks draw different masks
        self.site = 0

    def next_seed(self) -> int:
        self.site += 1
        return self.seed + 7919 * self.site


# ----------------------------------------------------------------------------------------------------------------- GEMM helpers
# fp32 products of the text / motion-anchor encoders (activations, gradients and weights stay fp32 there in every mode).  In bf16 training
# mode they run on f16x3 split operands (three f16 MFMA products per K slab, fp32-class result: include/mage_hip.h) instead of the
# exact-fp32 MFMA chain, 3x its rate -- as in generation (mage_model._linear under split_kind); precision 'fp32' keeps the exact chain, which
# is what the 1e-4 gradient gates against the oracle are stated for.  train_forward sets run32.sk; the tape carries run32 to train_backward.
def _f32_branch() -> bool:
    """fp32 branch rows / LayerNorm-output gradients in bf16 mode too (the round-2 form; config.train_f32_branch)."""
    return config.get().train_f32_branch


def _gemm32(run: _Run, a, w, y, *, M, N, K, lda=None, **kw):
    """ops.gemm for fp32 operands; plain products (bias / fp32 residual / QuickGELU only) go through split copies when run.sk says so."""
    sk = run.sk
    lda = K if lda is None else lda
    ldy = kw.pop("ldy", N)
    if (sk and a.dtype == F32 and w.dtype == F32 and K % 64 == 0 and N % 8 == 0 and lda == K and ldy == N and a.dim() == 2 and a.stride(1) == 1
            and w.dim() == 2 and w.is_contiguous() and set(kw) <= {"bias", "residual", "ldr", "act"}
            and kw.get("act", ops.ACT_NONE) in (ops.ACT_NONE, ops.ACT_QUICKGELU) and (kw.get("residual") is None or kw.get("act", 0) == ops.ACT_NONE)):
        key = (w.data_ptr(), tuple(w.shape), w._version)
        ws = run.split_w.get(key)
        if ws is None:
            ws = run.split_w[key] = (ops.split(w, sk), w)          # keeps w alive: the key is its address
        return ops.gemm(ops.split(a[:M], sk), ws[0], y, M=M, N=N, K=K, lda=2 * K, ldy=N, split_kind=sk, **kw)
    return ops.gemm(a, w, y, M=M, N=N, K=K, lda=lda, ldy=ldy, **kw)


def _gemm_x(run: _Run, a, wT, y, *, M, N, K, lda=None, **kw):
    """y[M, N] = a[M, K] @ wT[N, K]^T (no bias): dX of a Linear, or any plain product."""
    return _gemm32(run, a, wT, y, M=M, N=N, K=K, lda=lda, **kw)


def _split_plan(M: int, N: int, K: int):
    tiles = ((N + 255) // 256) * ((K + 255) // 256)
    S = max(1, min(64, (512 + tiles - 1) // tiles, M // 512 if M >= 1024 else 1))
    Mc = ((M + S - 1) // S + 63) // 64 * 64
    return S, Mc


TAPS3 = tuple((ky - 1, kx - 1) for ky in range(3) for kx in range(3))       # a 3 x 3 convolution's (dy, dx)


def _wgrad_taps(dy, x, *, M: int, N: int, Cin: int, taps=((0, 0),), ld_dy: Optional[int] = None, ld_x: Optional[int] = None,
                dy_geo: Optional[dict] = None, x_geo: Optional[dict] = None, want_bias: bool = True, colsum: bool = False, dyT=None):
    """dW[N, len(taps) * Cin] (tap-major, ci fastest: the GEMM weight layout; fp32) = sum_m dy[row(m), :N]^T x[gather_tap(m), :Cin] and
    db[N] = sum_m dy[row(m), :]: dy transposed once, one gathered transpose of x per tap stacked below each other, ONE split-K GEMM whose
    partials are summed in a fixed order.  taps: the (dy, dx) shifts of x's gather; x_geo: the grid it runs over and where x's images lie, in
    ops.transpose's own keywords (out_h, out_w, in_h, in_w, stride, img_stride, a_off; None: plain rows); dy_geo: a row map for dy, likewise;
    ld_dy / ld_x: the operands' leading dimensions (N / Cin).  colsum: db may come from the pass that transposes dy (bf16; dy_geo then has
    out_w, img_stride, a_off at the most).  dyT: the transposed dy of an earlier call on the same dy.  Returns (dW, db or None, dyT)."""
    assert dy.dtype == x.dtype
    dev, dt, K = dy.device, dy.dtype, len(taps) * Cin
    ld_dy = N if ld_dy is None else ld_dy
    S, Mc = _split_plan(M, N, K)
    Mp = S * Mc
    db = None
    if dyT is None:
        dyT = torch.empty(N, Mp, device=dev, dtype=dt)
        if colsum and want_bias and dt == BF16 and N % 8 == 0 and ld_dy % 8 == 0 and Mp % 8 == 0:
            db = ops.transpose_colsum(dy, dyT, M=M, Mp=Mp, C=N, ldx=ld_dy, ldy=Mp, **(dy_geo or {}))
        else:
            ops.transpose(dy, dyT, M=M, Mp=Mp, C=N, ldx=ld_dy, ldy=Mp, **(dy_geo or {}))
    xT = torch.empty(K, Mp, device=dev, dtype=dt)
    for i, (sy, sx) in enumerate(taps):
        ops.transpose(x, xT, M=M, Mp=Mp, C=Cin, ldx=Cin if ld_x is None else ld_x, ldy=Mp, y_row0=i * Cin, dy=sy, dx=sx, **(x_geo or {}))
    part = torch.empty(S, N, K, device=dev, dtype=F32)
    ops.gemm(dyT, xT, part, M=N, N=K, K=Mc, lda=Mp, ldy=K, ldw=Mp, n_split=S, a_split_stride=Mc, w_split_stride=Mc, y_split_stride=N * K)
    dW = part[0] if S == 1 else ops.sum_partials(part, torch.empty(N, K, device=dev, dtype=F32), stride=N * K, n_part=S, n=N * K)
    if want_bias and db is None:
        db = ops.row_sum(dyT, torch.empty(N, device=dev, dtype=F32), ld=Mp, n=M, rows=N)
    return dW, db, dyT


def _wgrad(dy, x, *, M: int, N: int, K: int, ld_dy: int, ld_x: int, dy_geo: Optional[dict] = None, x_geo: Optional[dict] = None,
           want_bias: bool = True):
    """dW[N, K] = sum_m dy[m, :N]^T x[m, :K] (fp32) and db[N] = sum_m dy[m, :].  dy and x are row sets of the same M logical rows
    (optionally regrouped views: dict(out_w, img_stride, a_off), the [:, 1:] / [:, 0] slices of [B, L, hw, C] streams), same
    dtype (the compute dtype)."""
    assert dy.dtype == x.dtype
    if (dy.dtype == BF16 and dy_geo is None and x_geo is None and N % 256 == 0 and K % 256 == 0 and M >= 4096 and ld_dy % 8 == 0
            and ld_x % 8 == 0 and not config.get().train_wgrad_transpose):
        # the decoder stack's Linear layers: dW = dY^T X straight from the row-major operands (mage_gemm_tn: transposing LDS loads),
        # no dY^T / X^T copies (they were 11.8 ms of a 92 ms step at cfg2)
        return ops.gemm_tn(dy, x, T=M, N=N, K=K, ld_dy=ld_dy, ld_x=ld_x, want_bias=want_bias)
    return _wgrad_taps(dy, x, M=M, N=N, Cin=K, ld_dy=ld_dy, ld_x=ld_x, dy_geo=dy_geo, x_geo=x_geo, want_bias=want_bias, colsum=True)[:2]


def _flipped(w: torch.Tensor, cout: int, k: int, cin: int) -> torch.Tensor:
    """GEMM weight [cin, k*k*cout] of the input-gradient convolution of the k x k convolution with GEMM weight w ([cout, k, k, cin]
    flattened): Wf[ci, (ky, kx), co] = W[co, (k-1-ky, k-1-kx), ci]."""
    return w.reshape(cout, k, k, cin).flip(1, 2).permute(3, 1, 2, 0).reshape(cin, k * k * cout).contiguous()


def _linear_bwd(run: _Run, d, grads, name: str, key: str, dy, x, *, M: int, N: int, K: int, geo: Optional[dict] = None, out_dt=None, out=None,
                **gemm_kw):
    """Backward of the Linear y[M, N] = x[M, K] W^T + b (W: d[key + suffix]; dy and x in the compute dtype): the gradients into
    grads[name + 'weight'] / grads[name + 'bias'] (geo: _wgrad's dy_geo / x_geo), then dx = dy W, which is returned: a fresh [M, K] in out_dt,
    or `out` (gemm_kw: the product's epilogue or row maps).  Neither out_dt nor out: the weight gradient only."""
    grads[name + "weight"], grads[name + "bias"] = _wgrad(dy, x, M=M, N=N, K=K, ld_dy=N, ld_x=K, **(geo or {}))
    if out is None and out_dt is None:
        return None
    if out is None:
        out = torch.empty(M, K, device=dy.device, dtype=out_dt)
    return _gemm_x(run, dy, _wt(d, key, dy.dtype), out, M=M, N=K, K=N, **gemm_kw)


def _self_attn_bwd(run: _Run, d, grads, name: str, p: str, dbr, t, x_in, *, M: int, C: int, geo: dict, out_dt, **last_kw):
    """Backward of the self-attention branch out_proj(attention(in_proj(x_in))) with packed [q | k | v] rows (t['qkv'], t['ao'] of the
    forward pass): out_proj, attention_bwd on the three column views, in_proj.  dbr: the branch's output gradient as a GEMM operand;
    name: the nn.MultiheadAttention's state_dict prefix; geo: attention_bwd's keywords.  Returns the gradient of x_in in out_dt (last_kw:
    that product's residual)."""
    dt, qkv = dbr.dtype, t["qkv"]
    dao = _linear_bwd(run, d, grads, name + "out_proj.", p + ".out_proj", dbr, t["ao"], M=M, N=C, K=C, out_dt=dt)
    dqkv = torch.empty(M, 3 * C, device=dbr.device, dtype=dt)
    ops.attention_bwd(qkv, qkv[:, C:], qkv[:, 2 * C:], dao, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], ldq=3 * C, ldk=3 * C, ldv=3 * C, ldo=C,
                      ld_dq=3 * C, ld_dk=3 * C, ld_dv=3 * C, **geo)
    return _linear_bwd(run, d, grads, name + "in_proj_", p + ".in_proj", dqkv, x_in, M=M, N=3 * C, K=C, out_dt=out_dt, **last_kw)


def _to_dt(run: _Run, g32: torch.Tensor, seed: Optional[int] = None) -> torch.Tensor:
    """The fp32 gradient stream as a GEMM operand in the compute dtype, through the dropout mask of the branch it enters."""
    if seed is not None and run.p > 0:
        return ops.dropout(g32, torch.empty(g32.shape, device=g32.device, dtype=run.dt), run.p, seed)
    if run.dt == F32:
        return g32
    return ops.cast(g32, torch.empty(g32.shape, device=g32.device, dtype=run.dt))


def _res_linear(run: _Run, a, d, name, x_old, dt, *, M, N, K, seed, ln=None, cast_to=None):
    """x_new = x_old + dropout(a @ W^T + b): a fresh tensor (x_old is the saved LayerNorm input of the backward pass).
    ln = (gamma, beta, out dtype): also returns LayerNorm(x_new) -- the norm that opens the next branch -- as (x_new, xn); with dropout on,
    the mask-and-add pass and the norm are one launch (mage_dropout_add_layernorm)."""
    w, b = d[name + _sfx(dt)], d.get(name + ".b")
    if run.p == 0:
        x_new = _gemm32(run, a, w, torch.empty_like(x_old), M=M, N=N, K=K, lda=K, ldy=N, bias=b, residual=x_old, ldr=N)
        if ln is None:
            return x_new if cast_to is None else (x_new, ops.cast(x_new, torch.empty(M, N, device=a.device, dtype=cast_to)))
        return x_new, ops.layernorm(x_new, ln[0], ln[1], torch.empty(M, N, device=a.device, dtype=ln[2]), 1e-5)
    # the branch rows leave the GEMM in the compute dtype (bf16 mode: half the bytes written here and read by the mask-and-add pass;
    # the stream x itself stays fp32).  MAGE_TRAIN_F32_BRANCH=1 keeps fp32 branch rows.
    br = _gemm32(run, a, w, torch.empty(M, N, device=a.device, dtype=F32 if _f32_branch() else a.dtype), M=M, N=N, K=K, lda=K, ldy=N, bias=b)
    if ln is None:
        if cast_to is not None:                      # the last block: its rows also as the head GEMM's bf16 operand
            xb = torch.empty(M, N, device=a.device, dtype=cast_to)
            return ops.dropout_add(br, x_old, torch.empty_like(x_old), run.p, seed, y_bf16=xb), xb
        return ops.dropout_add(br, x_old, torch.empty_like(x_old), run.p, seed)
    if not config.get().train_emit:
        x_new = ops.dropout_add(br, x_old, torch.empty_like(x_old), run.p, seed)
        return x_new, ops.layernorm(x_new, ln[0], ln[1], torch.empty(M, N, device=a.device, dtype=ln[2]), 1e-5)
    return ops.dropout_add_layernorm(br, x_old, torch.empty_like(x_old), ln[0], ln[1], torch.empty(M, N, device=a.device, dtype=ln[2]), 1e-5,
                                     run.p, seed)


# ----------------------------------------------------------------------------------------------------------------- decoder stack
def _dec_forward(gm, run: _Run, motion, feats, B: int, hh: int, ww: int):
    d = gm._derived.get(gm._build)
    dt, Cc, L, dev = run.dt, gm.model_channels, gm.frames_length, motion.device
    hw = hh * ww
    M = B * L * hw
    x = torch.empty(M, Cc, device=dev, dtype=F32)
    ops.gemm(motion, d["context_linear" + _sfx(dt)], x, M=B * hw, N=Cc, K=gm.context_channels, lda=gm.context_channels, ldy=Cc,
             bias=d["context_linear.b"], out_w=hw, y_img_stride=L * hw, rowadd=d["tpos"], rowadd_div=hw, rowadd_mod=L)
    ops.gemm(feats, d["in_linear" + _sfx(dt)], x, M=B * (L - 1) * hw, N=Cc, K=gm.in_channels, lda=gm.in_channels, ldy=Cc,
             bias=d["in_linear.b"], out_w=(L - 1) * hw, y_img_stride=L * hw, y_off=hw, rowadd=d["tpos"], rowadd_div=hw, rowadd_mod=L)
    blocks = []
    xn1 = xa = None
    for i in range(gm.layers):
        p = f"b{i}"
        geo = gm._axial_geo(i % 3, B, hh, ww, L)
        if xn1 is None:                              # later blocks: written with the previous block's residual add
            xn1 = ops.layernorm(x, d[p + ".ln_1.w"], d[p + ".ln_1.b"], torch.empty(M, Cc, device=dev, dtype=dt), 1e-5)
        qkv = ops.gemm(xn1, d[p + ".in_proj" + _sfx(dt)], torch.empty(M, 3 * Cc, device=dev, dtype=dt), M=M, N=3 * Cc, K=Cc, lda=Cc,
                       ldy=3 * Cc, bias=d[p + ".in_proj.b"])
        ao = torch.empty(M, Cc, device=dev, dtype=dt)
        ops.attention(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], ao, ldq=3 * Cc, ldk=3 * Cc, ldv=3 * Cc, ldo=Cc, **geo)
        s_attn, s_mlp = run.next_seed(), run.next_seed()
        x1, xn2 = _res_linear(run, ao, d, p + ".out_proj", x, dt, M=M, N=Cc, K=Cc, seed=s_attn, ln=(d[p + ".ln_2.w"], d[p + ".ln_2.b"], dt))
        if dt != F32 and M % 256 == 0 and Cc % 64 == 0 and config.get().train_dual:
            # one launch writes the pre-activation rows (kept for the backward pass) and QuickGELU of them (the next Linear's operand)
            hdn = torch.empty(M, 4 * Cc, device=dev, dtype=dt)
            hpre = ops.gemm(xn2, d[p + ".c_fc" + _sfx(dt)], torch.empty(M, 4 * Cc, device=dev, dtype=dt), M=M, N=4 * Cc, K=Cc, lda=Cc,
                            ldy=4 * Cc, bias=d[p + ".c_fc.b"], act=ops.ACT_QUICKGELU, y2=hdn, ldy2=4 * Cc)
        else:
            hpre = ops.gemm(xn2, d[p + ".c_fc" + _sfx(dt)], torch.empty(M, 4 * Cc, device=dev, dtype=dt), M=M, N=4 * Cc, K=Cc, lda=Cc,
                            ldy=4 * Cc, bias=d[p + ".c_fc.b"])
            hdn = ops.act(hpre, torch.empty_like(hpre), ops.ACT_QUICKGELU)
        nxt = f"b{i + 1}" if i + 1 < gm.layers else None
        if nxt is not None:
            x2, xn_next = _res_linear(run, hdn, d, p + ".c_proj", x1, dt, M=M, N=Cc, K=4 * Cc, seed=s_mlp,
                                      ln=(d[nxt + ".ln_1.w"], d[nxt + ".ln_1.b"], dt))
        else:
            xa = None
            if gm.use_cids and dt == BF16:
                x2, xa = _res_linear(run, hdn, d, p + ".c_proj", x1, dt, M=M, N=Cc, K=4 * Cc, seed=s_mlp, cast_to=dt)
            else:
                x2 = _res_linear(run, hdn, d, p + ".c_proj", x1, dt, M=M, N=Cc, K=4 * Cc, seed=s_mlp)
            xn_next = None
        # hdn is kept for the c_proj weight gradient (recomputing it was one more pass over [M, 4C] per block; 288 GB of HBM)
        blocks.append(dict(x0=x, xn1=xn1, qkv=qkv, ao=ao, x1=x1, xn2=xn2, hpre=hpre, hdn=hdn, geo=geo, s_attn=s_attn, s_mlp=s_mlp))
        x, xn1 = x2, xn_next
    if not gm.use_cids:
        # MAGE+ head (mage_model.py:350-354,387-388): GroupNorm(32) over all L-1 predicted frames of a clip -> SiLU -> Conv3d 1x1x1
        M1 = B * (L - 1) * hw
        st = torch.empty(B, 32, 2, device=dev, dtype=F32)
        y = ops.groupnorm_act(x, d["gn.w"], d["gn.b"], torch.empty(M1, Cc, device=dev, dtype=dt), n_samples=B, rows_per_sample=(L - 1) * hw,
                              sample_stride_rows=L * hw, row_off=hw, groups=32, eps=gm.out[0].eps, act=2, stats=st)
        n8 = d["out.f32"].shape[0]
        pred = ops.gemm(y, d["out" + _sfx(dt)], torch.empty(M1, n8, device=dev, dtype=F32), M=M1, N=n8, K=Cc, lda=Cc, ldy=n8, bias=d["out.b"])
        return pred, dict(blocks=blocks, x_last=x, y=y, gn_stats=st, motion=motion, feats=feats, B=B, hh=hh, ww=ww)
    if dt == F32:
        xa = x
    elif xa is None:
        xa = ops.cast(x, torch.empty(M, Cc, device=dev, dtype=dt))
    Kc = gm.out_channels
    logits = torch.empty(B * (L - 1) * hw, Kc, device=dev, dtype=F32)
    ops.gemm(xa, d["out" + _sfx(dt)], logits, M=B * (L - 1) * hw, N=Kc, K=Cc, lda=Cc, ldy=Kc, bias=d["out.b"], out_w=(L - 1) * hw,
             a_img_stride=L * hw, a_off=hw)
    return logits, dict(blocks=blocks, xa=xa, motion=motion, feats=feats, B=B, hh=hh, ww=ww)


def _emit_next(run, dx, emit):
    """layernorm_bwd's extra output for `emit` = (seed of the branch the updated dx enters next, or None for a plain cast): bf16 mode
    only (the masked / cast copy _to_dt would make in a separate pass); None otherwise."""
    if emit is None or run.dt != BF16 or not config.get().train_emit:
        return None, {}
    seed = emit[0]
    dxb = torch.empty(dx.shape, device=dx.device, dtype=BF16)
    return dxb, dict(dx_bf16=dxb, p=run.p if seed is not None else 0.0, seed=seed or 0)


def _block_mlp_bwd(run, d, p, pre, grads, dx, x1, xn2, hpre, M, Cc, seed, hdn=None, dxb=None, emit=None):
    """Backward of x2 = x1 + drop(c_proj(QuickGELU(c_fc(ln_2(x1))))) given dx = d/dx2 (fp32, updated in place to d/dx1).  dxb: dx as this
    branch's GEMM operand if the caller already holds it; emit = (seed,): returns the updated dx as the NEXT branch's operand (see _emit_next)."""
    dt, dev = run.dt, dx.device
    if dxb is None:
        dxb = _to_dt(run, dx, seed)
    if hdn is None:
        hdn = ops.act(hpre, torch.empty_like(hpre), ops.ACT_QUICKGELU)
    _linear_bwd(run, d, grads, f"{pre}.mlp.c_proj.", f"{p}.c_proj", dxb, hdn, M=M, N=Cc, K=4 * Cc)      # hdn is released before dh exists
    del hdn
    # d/d(pre-activation) straight from the data-gradient GEMM where its epilogue can multiply the accumulators by QuickGELU'(hpre)
    dual = dt != F32 and M % 256 == 0 and Cc % 64 == 0 and config.get().train_dual
    dh = _gemm_x(run, dxb, _wt(d, f"{p}.c_proj", dt), torch.empty(M, 4 * Cc, device=dev, dtype=dt), M=M, N=4 * Cc, K=Cc,
                 **(dict(act=ops.ACT_QUICKGELU_GRAD, y2=hpre, ldy2=4 * Cc) if dual else {}))
    if not dual:
        ops.act_bwd(hpre, dh, dh, ops.ACT_QUICKGELU)
    # d/d(LayerNorm output) in the compute dtype: layernorm_bwd reads it once (its dx stream stays fp32)
    dxn = _linear_bwd(run, d, grads, f"{pre}.mlp.c_fc.", f"{p}.c_fc", dh, xn2, M=M, N=4 * Cc, K=Cc, out_dt=F32 if _f32_branch() else dt)
    del dh, dxb
    nxt, kw = _emit_next(run, dx, emit)
    grads[f"{pre}.ln_2.weight"], grads[f"{pre}.ln_2.bias"] = ops.layernorm_bwd(x1, d[f"{p}.ln_2.w"], dxn, dx, eps=1e-5, accumulate=True, **kw)
    return nxt


def _dec_backward(gm, run: _Run, tape, dlogits, grads: Dict[str, torch.Tensor], pre: str = "generate_model"):
    d = gm._derived.get(gm._build)
    dt, Cc, L, dev = run.dt, gm.model_channels, gm.frames_length, dlogits.device
    B, hh, ww = tape["B"], tape["hh"], tape["ww"]
    hw = hh * ww
    M, Kc, M1 = B * L * hw, gm.out_channels, B * (L - 1) * hw
    tail = dict(out_w=(L - 1) * hw, img_stride=L * hw, a_off=hw)            # the x[:, 1:] rows of a [B, L, hw, C] stream
    dx = torch.zeros(M, Cc, device=dev, dtype=F32)
    if gm.use_cids:
        _linear_bwd(run, d, grads, pre + ".out.", "out", dlogits, tape["xa"], M=M1, N=Kc, K=Cc, geo=dict(x_geo=tail), out=dx, out_w=(L - 1) * hw,
                    y_img_stride=L * hw, y_off=hw)
    else:                                                                    # dlogits = d loss / d pred [M1, n8] (padding columns zero)
        n8 = d["out.f32"].shape[0]
        dWo, dbo = _wgrad(dlogits, tape["y"], M=M1, N=n8, K=Cc, ld_dy=n8, ld_x=Cc)
        grads[pre + ".out.2.weight"], grads[pre + ".out.2.bias"] = dWo[:Kc].reshape(Kc, Cc, 1, 1, 1), dbo[:Kc]
        dy = _gemm_x(run, dlogits, _wt(d, "out", dt), torch.empty(M1, Cc, device=dev, dtype=F32), M=M1, N=Cc, K=n8)
        dg, db, _ = ops.groupnorm_bwd(tape["x_last"], d["gn.w"], d["gn.b"], tape["gn_stats"], dy, dx, n_samples=B, rows_per_sample=(L - 1) * hw,
                                      sample_stride_rows=L * hw, row_off=hw, groups=32, act=2)       # slot 0 rows stay zero
        grads[pre + ".out.0.weight"], grads[pre + ".out.0.bias"] = dg, db
        del dy
    dxb = None                                                               # dx as the next branch's operand, from layernorm_bwd
    for i in reversed(range(gm.layers)):
        p, bp, t = f"b{i}", f"{pre}.blocks.{i}", tape["blocks"][i]
        dxb = _block_mlp_bwd(run, d, p, bp, grads, dx, t["x1"], t["xn2"], t["hpre"], M, Cc, t["s_mlp"], hdn=t.pop("hdn"), dxb=dxb,
                             emit=(t["s_attn"],))
        if dxb is None:
            dxb = _to_dt(run, dx, t["s_attn"])
        dxn = _self_attn_bwd(run, d, grads, bp + ".attn.", p, dxb, t, t["xn1"], M=M, C=Cc, geo=t["geo"], out_dt=F32 if _f32_branch() else dt)
        del dxb
        dxb, kw = _emit_next(run, dx, (tape["blocks"][i - 1]["s_mlp"] if i > 0 else None,))
        grads[bp + ".ln_1.weight"], grads[bp + ".ln_1.bias"] = ops.layernorm_bwd(t["x0"], d[p + ".ln_1.w"], dxn, dx, eps=1e-5, accumulate=True, **kw)
        tape["blocks"][i] = None                                             # release the block's activations
    # x_init = [context_linear(motion) | in_linear(feats)] + T_positional_embedding
    tp = ops.group_rowsum(dx, torch.empty(L, Cc, device=dev, dtype=F32), rows=M, C=Cc, div=hw, mod=L)
    grads[pre + ".T_positional_embedding"] = tp.view(L, 1, 1, Cc)
    if dxb is None:
        dxb = _to_dt(run, dx)
    head = dict(out_w=hw, img_stride=L * hw, a_off=0)                        # the x[:, 0] rows
    Ki, Kx = gm.in_channels, gm.context_channels                             # both weight gradients first, then both input gradients
    _linear_bwd(run, d, grads, pre + ".in_linear.", "in_linear", dxb, tape["feats"], M=M1, N=Cc, K=Ki, geo=dict(dy_geo=tail))
    _linear_bwd(run, d, grads, pre + ".context_linear.", "context_linear", dxb, tape["motion"], M=B * hw, N=Cc, K=Kx, geo=dict(dy_geo=head))
    dfeats = _gemm_x(run, dxb, _wt(d, "in_linear", dt), torch.empty(M1, Ki, device=dev, dtype=F32), M=M1, N=Ki, K=Cc, out_w=(L - 1) * hw,
                     a_img_stride=L * hw, a_off=hw)
    dmotion = _gemm_x(run, dxb, _wt(d, "context_linear", dt), torch.empty(B * hw, Kx, device=dev, dtype=F32), M=B * hw, N=Kx, K=Cc, out_w=hw,
                      a_img_stride=L * hw, a_off=0)
    return dfeats, dmotion


# ----------------------------------------------------------------------------------------------------------------- frame features
def _conv_flip(model, d, dt):
    """Weight of the input-gradient convolution: Wf[ci, (ky, kx), co] = W[co, (2-ky, 2-kx), ci]."""
    key = "conv.flip" + _sfx(dt)
    if key not in d:
        d[key] = _flipped(d["conv" + _sfx(dt)], model.vision_width, 3, model.vision_width)
    return d[key]


def _frame_backward(model, run_dt, tok_rows, emb, dfeats, grads, acc, lat_rows=None):
    """feats = conv3x3(emb[tok]) + (H_pos + W_pos): gradients of the conv weight, the positional tables and the token table
    (accumulated into acc['conv'], acc['hwpos'], acc['emb']: the fp32 prologue pass and the decoder pass both land here).
    use_cids=False: emb = Linear(latents) (mage_model.py:583): lat_rows [rows, LD] fp32 instead of tok_rows, the Linear's gradients
    accumulate in acc['emb_lin.w'] [C, LD] / acc['emb_lin.b']."""
    d = model._derived.get(model._build)
    R, Cc, dev = model.image_resolution, model.vision_width, dfeats.device
    hw = R * R
    rows = dfeats.shape[0]
    n_img = rows // hw
    hp = ops.group_rowsum(dfeats, torch.empty(hw, Cc, device=dev, dtype=F32), rows=rows, C=Cc, div=1, mod=hw)
    acc["hwpos"] = hp if acc.get("hwpos") is None else acc["hwpos"] + hp
    P = R + 2
    taps = run_dt == BF16 and Cc % 256 == 0 and rows % 256 == 0 and config.get().train_taps
    if taps:
        # dfeats as bf16 rows in the interior of a zero-padded (R+2) x (R+2) frame buffer (border written once): its transposed
        # convolution below is then the padded-taps form of mage_gemm (8-phase kernel, 1.4 -> 0.9 ms at cfg2), as in _frame_features
        key = ("dfeats", n_img, str(dev))
        pad = model._pad_frames.get(key)
        if pad is None:
            pad = model._pad_frames[key] = torch.zeros((n_img * P * P + 1) * Cc, device=dev, dtype=run_dt).view(-1, Cc)
        pad[:n_img * P * P].view(n_img, P, P, Cc)[:, 1:R + 1, 1:R + 1].copy_(dfeats.view(n_img, R, R, Cc))       # cast + placement
        dfe, dfe_geo = pad, dict(out_h=R, out_w=R, in_h=P, in_w=P, img_stride=P * P, dy=1, dx=1)
    else:
        dfe = dfeats if run_dt == F32 else ops.cast(dfeats, torch.empty(rows, Cc, device=dev, dtype=run_dt))
        dfe_geo = {}
    # dW[co, tap, ci] = sum_p dfeats[p, co] * emb[shift_tap(p), ci]
    dW = _wgrad_taps(dfe, emb, M=rows, N=Cc, Cin=Cc, taps=TAPS3, dy_geo=dfe_geo, x_geo=dict(out_h=R, out_w=R, in_h=R, in_w=R, img_stride=hw),
                     want_bias=False)[0]
    acc["conv"] = dW if acc.get("conv") is None else acc["conv"] + dW
    # d emb = the transposed convolution of dfeats
    if taps:
        demb = ops.gemm(dfe, _conv_flip(model, d, run_dt), torch.empty(rows, Cc, device=dev, dtype=F32), M=rows, N=Cc, K=9 * Cc, lda=Cc, ldy=Cc,
                        out_h=R, out_w=R, in_h=P, in_w=P, a_img_stride=P * P, taps_h=3, taps_w=3, cin=Cc, stride=1, dy0=0, dx0=0)
    else:
        demb = VectorQuantizedVAE._conv(dfe, _conv_flip(model, d, run_dt), torch.empty(rows, Cc, device=dev, dtype=F32), n_img=n_img, H=R, W=R,
                                        cin=Cc, cout=Cc, k=3)
    if lat_rows is not None:
        LD = lat_rows.shape[1]
        dW, db = _wgrad(demb, lat_rows, M=rows, N=Cc, K=LD, ld_dy=Cc, ld_x=LD)
        acc["emb_lin.w"] = dW if acc.get("emb_lin.w") is None else acc["emb_lin.w"] + dW
        acc["emb_lin.b"] = db if acc.get("emb_lin.b") is None else acc["emb_lin.b"] + db
        return
    if acc.get("emb") is None:
        acc["emb"] = torch.zeros(model.codebook_size, Cc, device=dev, dtype=F32)
    ops.embedding_bwd(tok_rows, demb, acc["emb"])


# ----------------------------------------------------------------------------------------------------------------- MA encoder
def _ma_forward(ma, run: _Run, q, kv, B: int, nq: int, nk: int):
    """MAEncoder (one or more TransformerBlocks, the MAGE variant mage_model.py:92), batch-first rows, fp32."""
    d = ma._derived.get(ma._build)
    Cc, dev, H = ma.d_model, q.device, ma.d_model // 32
    x = q
    layers = []
    for i in range(ma.layers):
        p = f"b{i}"
        w, b = d[p + ".in_proj.f32"], d[p + ".in_proj.b"]
        qin, kvin = x, kv
        if ma.mage_plus:                                                     # the ln_q / ln_kv line of mage_model.py:93 (MAGE+)
            qin = ops.layernorm(x, d[p + ".ln_q.w"], d[p + ".ln_q.b"], torch.empty_like(x), 1e-5)
            kvin = ops.layernorm(kv, d[p + ".ln_kv.w"], d[p + ".ln_kv.b"], torch.empty_like(kv), 1e-5)
        qp = _gemm32(run, qin, w[:Cc], torch.empty(B * nq, Cc, device=dev, dtype=F32), M=B * nq, N=Cc, K=Cc, lda=Cc, ldy=Cc, bias=b[:Cc])
        kvp = _gemm32(run, kvin, w[Cc:], torch.empty(B * nk, 2 * Cc, device=dev, dtype=F32), M=B * nk, N=2 * Cc, K=Cc, lda=Cc, ldy=2 * Cc, bias=b[Cc:])
        geo = dict(n_seq=B, inner=1, nq=nq, nk=nk, n_head=H, q_outer_stride=nq, q_axis_stride=1, kv_outer_stride=nk, kv_axis_stride=1)
        ao = torch.empty(B * nq, Cc, device=dev, dtype=F32)
        ops.attention(qp, kvp, kvp[:, Cc:], ao, ldq=Cc, ldk=2 * Cc, ldv=2 * Cc, ldo=Cc, **geo)
        s_attn, s_mlp = run.next_seed(), run.next_seed()
        x1 = _res_linear(run, ao, d, p + ".out_proj", x, F32, M=B * nq, N=Cc, K=Cc, seed=s_attn)
        xn = ops.layernorm(x1, d[p + ".ln_2.w"], d[p + ".ln_2.b"], torch.empty_like(x1), 1e-5)
        hpre = _gemm32(run, xn, d[p + ".c_fc.f32"], torch.empty(B * nq, 4 * Cc, device=dev, dtype=F32), M=B * nq, N=4 * Cc, K=Cc, lda=Cc,
                       ldy=4 * Cc, bias=d[p + ".c_fc.b"])
        hdn = ops.act(hpre, torch.empty_like(hpre), ops.ACT_QUICKGELU)
        x2 = _res_linear(run, hdn, d, p + ".c_proj", x1, F32, M=B * nq, N=Cc, K=4 * Cc, seed=s_mlp)
        layers.append(dict(x0=x, qin=qin, kvin=kvin, qp=qp, kvp=kvp, ao=ao, x1=x1, xn=xn, hpre=hpre, geo=geo, s_attn=s_attn, s_mlp=s_mlp))
        x = x2
    return x, dict(layers=layers, kv=kv, B=B, nq=nq, nk=nk)


def _ma_backward(ma, run32: _Run, tape, dx, grads, pre: str = "ma_encoder"):
    d = ma._derived.get(ma._build)
    Cc, dev = ma.d_model, dx.device
    B, nq, nk, kv = tape["B"], tape["nq"], tape["nk"], tape["kv"]
    dkv_total = None
    dx = dx.clone()
    for i in reversed(range(ma.layers)):
        p, bp, t = f"b{i}", f"{pre}.blocks.{i}", tape["layers"][i]
        _block_mlp_bwd(run32, d, p, bp, grads, dx, t["x1"], t["xn"], t["hpre"], B * nq, Cc, t["s_mlp"])
        dbr = _to_dt(run32, dx, t["s_attn"])
        dao = _linear_bwd(run32, d, grads, bp + ".attn.out_proj.", p + ".out_proj", dbr, t["ao"], M=B * nq, N=Cc, K=Cc, out_dt=F32)
        dqp = torch.empty(B * nq, Cc, device=dev, dtype=F32)
        dkvp = torch.empty(B * nk, 2 * Cc, device=dev, dtype=F32)
        kvp = t["kvp"]
        ops.attention_bwd(t["qp"], kvp, kvp[:, Cc:], dao, dqp, dkvp, dkvp[:, Cc:], ldq=Cc, ldk=2 * Cc, ldv=2 * Cc, ldo=Cc, ld_dq=Cc,
                          ld_dk=2 * Cc, ld_dv=2 * Cc, **t["geo"])
        # in_proj is two Linears over the rows of one weight (q of x, k | v of the text): their gradients are assembled, their dx products
        # read column slices of the transposed copy
        dWq, dbq = _wgrad(dqp, t["qin"], M=B * nq, N=Cc, K=Cc, ld_dy=Cc, ld_x=Cc)
        dWkv, dbkv = _wgrad(dkvp, t["kvin"], M=B * nk, N=2 * Cc, K=Cc, ld_dy=2 * Cc, ld_x=Cc)
        grads[bp + ".attn.in_proj_weight"] = torch.cat([dWq, dWkv], 0)                      # [3C, C] assembly (layout plumbing)
        grads[bp + ".attn.in_proj_bias"] = torch.cat([dbq, dbkv], 0)
        wT = _wt(d, p + ".in_proj", F32)                                                    # [C, 3C]
        wqT, wkvT = wT[:, :Cc].contiguous(), wT[:, Cc:].contiguous()
        if ma.mage_plus:
            dqin = _gemm_x(run32, dqp, wqT, torch.empty(B * nq, Cc, device=dev, dtype=F32), M=B * nq, N=Cc, K=Cc)
            grads[bp + ".ln_q.weight"], grads[bp + ".ln_q.bias"] = ops.layernorm_bwd(t["x0"], d[p + ".ln_q.w"], dqin, dx, eps=1e-5, accumulate=True)
            dkvin = _gemm_x(run32, dkvp, wkvT, torch.empty(B * nk, Cc, device=dev, dtype=F32), M=B * nk, N=Cc, K=2 * Cc)
            dkv = torch.empty_like(dkvin)
            grads[bp + ".ln_kv.weight"], grads[bp + ".ln_kv.bias"] = ops.layernorm_bwd(kv, d[p + ".ln_kv.w"], dkvin, dkv, eps=1e-5,
                                                                                      accumulate=False)
        else:
            dx = _gemm_x(run32, dqp, wqT, torch.empty(B * nq, Cc, device=dev, dtype=F32), M=B * nq, N=Cc, K=Cc, residual=dx, ldr=Cc)
            dkv = _gemm_x(run32, dkvp, wkvT, torch.empty(B * nk, Cc, device=dev, dtype=F32), M=B * nk, N=Cc, K=2 * Cc)
            # ln_q / ln_kv exist in the checkpoint but are not applied by MAGE (mage_model.py:92): zero gradients
        dkv_total = dkv if dkv_total is None else dkv_total + dkv
    return dx, dkv_total


# ----------------------------------------------------------------------------------------------------------------- text encoder
def _text_forward(te, run: _Run, text):
    d = te._derived.get(te._build)
    B, S = text.shape
    Wd, dev, H = te.transformer_width, text.device, te.transformer_width // 32
    ids = text.to(torch.int64).contiguous()
    keep = ids != te.padding_idx
    kv_len = keep.sum(-1).to(torch.int32).contiguous()
    keepf = keep.reshape(-1).to(F32).contiguous()
    e = ops.embedding(ids, d["tok"], torch.empty(B * S, Wd, device=dev, dtype=F32))
    ops.row_affine(e, None, d["pos"], div=1, mod=S)
    x = ops.layernorm(e, d["layer_norm.w"], d["layer_norm.b"], torch.empty_like(e), te.layer_norm.eps)
    s_emb = run.next_seed()
    if run.p > 0:
        x = ops.dropout(x, torch.empty_like(x), run.p, s_emb)
    ops.row_affine(x, keepf, None)
    geo = dict(n_seq=B, inner=1, nq=S, nk=S, n_head=H, q_outer_stride=S, q_axis_stride=1, kv_outer_stride=S, kv_axis_stride=1,
               kv_len=kv_len, kv_len_div=1)
    layers = []
    for i in range(te.transformer_layers):
        p = f"l{i}"
        qkv = _gemm32(run, x, d[p + ".in_proj.f32"], torch.empty(B * S, 3 * Wd, device=dev, dtype=F32), M=B * S, N=3 * Wd, K=Wd, lda=Wd,
                      ldy=3 * Wd, bias=d[p + ".in_proj.b"])
        ao = torch.empty(B * S, Wd, device=dev, dtype=F32)
        # nn.TransformerEncoderLayer(dropout=p) also drops attention PROBABILITIES in train() (mage_model.py:193-199)
        sa_seed = run.next_seed()
        ops.attention(qkv, qkv[:, Wd:], qkv[:, 2 * Wd:], ao, ldq=3 * Wd, ldk=3 * Wd, ldv=3 * Wd, ldo=Wd, drop_p=run.p, drop_seed=sa_seed, **geo)
        s1_seed, sh_seed, s2_seed = run.next_seed(), run.next_seed(), run.next_seed()
        s1 = _res_linear(run, ao, d, p + ".out_proj", x, F32, M=B * S, N=Wd, K=Wd, seed=s1_seed)
        x1 = ops.layernorm(s1, d[p + ".norm1.w"], d[p + ".norm1.b"], torch.empty_like(s1), d[p + ".norm1.eps"])
        hpre = _gemm32(run, x1, d[p + ".fc1.f32"], torch.empty(B * S, 4 * Wd, device=dev, dtype=F32), M=B * S, N=4 * Wd, K=Wd, lda=Wd,
                       ldy=4 * Wd, bias=d[p + ".fc1.b"])
        hdn = ops.act(hpre, torch.empty_like(hpre), ops.ACT_GELU_ERF)
        if run.p > 0:
            hdn = ops.dropout(hdn, torch.empty_like(hdn), run.p, sh_seed)
        s2 = _res_linear(run, hdn, d, p + ".fc2", x1, F32, M=B * S, N=Wd, K=4 * Wd, seed=s2_seed)
        x2 = ops.layernorm(s2, d[p + ".norm2.w"], d[p + ".norm2.b"], torch.empty_like(s2), d[p + ".norm2.eps"])
        layers.append(dict(x_in=x, qkv=qkv, ao=ao, s1=s1, x1=x1, hpre=hpre, s2=s2, seeds=(s1_seed, sh_seed, s2_seed), sa_seed=sa_seed))
        x = x2
    xf = ops.layernorm(x, d["ln_text_final.w"], d["ln_text_final.b"], torch.empty_like(x), te.ln_text_final.eps)
    out = _gemm32(run, xf, d["proj.f32"], torch.empty(B * S, te.output_dim, device=dev, dtype=F32), M=B * S, N=te.output_dim, K=Wd, lda=Wd,
                   ldy=te.output_dim, bias=d["proj.b"])
    return out, dict(ids=ids, keepf=keepf, e=e, s_emb=s_emb, layers=layers, x_last=x, xf=xf, geo=geo, B=B, S=S)


def _text_backward(te, run32: _Run, tape, dout, grads, pre: str = "text_encoder"):
    d = te._derived.get(te._build)
    B, S = tape["B"], tape["S"]
    Wd, dev, R = te.transformer_width, dout.device, tape["B"] * tape["S"]
    dxf = _linear_bwd(run32, d, grads, pre + ".text_projection.", "proj", dout, tape["xf"], M=R, N=te.output_dim, K=Wd, out_dt=F32)
    dx = torch.empty(R, Wd, device=dev, dtype=F32)
    grads[pre + ".ln_text_final.weight"], grads[pre + ".ln_text_final.bias"] = ops.layernorm_bwd(tape["x_last"], d["ln_text_final.w"], dxf,
                                                                                                dx, eps=te.ln_text_final.eps,
                                                                                                accumulate=False)
    for i in reversed(range(te.transformer_layers)):
        p, lp, t = f"l{i}", f"{pre}.transformer.layers.{i}", tape["layers"][i]
        s1_seed, sh_seed, s2_seed = t["seeds"]
        ds2 = torch.empty(R, Wd, device=dev, dtype=F32)
        grads[lp + ".norm2.weight"], grads[lp + ".norm2.bias"] = ops.layernorm_bwd(t["s2"], d[p + ".norm2.w"], dx, ds2, eps=d[p + ".norm2.eps"],
                                                                                  accumulate=False)
        # the MLP half is written out: post-norm order, GELU(erf), and a dropout of the hidden rows in both directions
        dbr = _to_dt(run32, ds2, s2_seed)
        hdn = ops.act(t["hpre"], torch.empty_like(t["hpre"]), ops.ACT_GELU_ERF)
        if run32.p > 0:
            hdn = ops.dropout(hdn, torch.empty_like(hdn), run32.p, sh_seed)
        dh = _linear_bwd(run32, d, grads, lp + ".linear2.", p + ".fc2", dbr, hdn, M=R, N=Wd, K=4 * Wd, out_dt=F32)
        if run32.p > 0:
            dh = ops.dropout(dh, torch.empty_like(dh), run32.p, sh_seed)
        ops.act_bwd(t["hpre"], dh, dh, ops.ACT_GELU_ERF)
        dx1 = _linear_bwd(run32, d, grads, lp + ".linear1.", p + ".fc1", dh, t["x1"], M=R, N=4 * Wd, K=Wd, out_dt=F32, residual=ds2, ldr=Wd)
        ds1 = torch.empty(R, Wd, device=dev, dtype=F32)
        grads[lp + ".norm1.weight"], grads[lp + ".norm1.bias"] = ops.layernorm_bwd(t["s1"], d[p + ".norm1.w"], dx1, ds1, eps=d[p + ".norm1.eps"],
                                                                                  accumulate=False)
        dbr = _to_dt(run32, ds1, s1_seed)
        dx = _self_attn_bwd(run32, d, grads, lp + ".self_attn.", p, dbr, t, t["x_in"], M=R, C=Wd, out_dt=F32, residual=ds1, ldr=Wd,
                            geo=dict(tape["geo"], drop_p=run32.p, drop_seed=t["sa_seed"]))
    ops.row_affine(dx, tape["keepf"], None)                                   # x = dropout(LN(e)) * keep
    if run32.p > 0:
        dx = ops.dropout(dx, torch.empty_like(dx), run32.p, tape["s_emb"])
    de = torch.empty(R, Wd, device=dev, dtype=F32)
    grads[pre + ".layer_norm.weight"], grads[pre + ".layer_norm.bias"] = ops.layernorm_bwd(tape["e"], d["layer_norm.w"], dx, de,
                                                                                          eps=te.layer_norm.eps, accumulate=False)
    gt = torch.zeros(te.vocab_size, Wd, device=dev, dtype=F32)
    ops.embedding_bwd(tape["ids"].reshape(-1), de, gt, padding_idx=te.padding_idx if te.padding_idx is not None else -1)
    grads[pre + ".token_embedding.weight"] = gt
    gp = torch.zeros(te.context_length, Wd, device=dev, dtype=F32)
    ops.group_rowsum(de, gp, rows=R, C=Wd, div=1, mod=S)                      # rows 0..S-1 of the positions table
    grads[pre + ".positions.weight"] = gp


# ----------------------------------------------------------------------------------------------------------------- whole model
def _policy_scalars(policy: dict) -> dict:
    """The keyword arguments ops.policy_loss and ops.policy_loss_bwd share: the four scalars and the three options -- a reference (with its
    kl_coef), a mask, a group -- each None where the head has none; ops picks the entry points from that."""
    kw = {k: policy[k] for k in ("temperature", "clip_lo", "clip_hi", "entropy_coef")}
    kw.update(reference_logprob=policy.get("reference"), given=policy.get("given"), ratio_div=policy.get("ratio_div"))
    kw["kl_coef"] = 0.0 if kw["reference_logprob"] is None else policy["kl_coef"]
    return kw


# Loss heads: what train_forward ends in and train_backward starts from.  A head has `tokens` (None: the pass runs over the batch's own video;
# int64 [B, L-1, h, w]: over frame 0 plus these GIVEN tokens), forward(model, logits, target, B) -> (loss, parts, saved) and
# backward(logits, target, saved, gout, dt) -> d loss / d logits in dt.  parts is the loss dict the MAGE method reports, saved whatever backward
# and the method need besides; both travel back to the method as model._last_head_out = (parts, saved).
def _dlogits(logits, dt):
    return torch.empty(logits.shape, device=logits.device, dtype=dt)


class CrossEntropyHead:
    """forward on a use_cids model (mage_model.py:618)."""
    tokens = None

    def forward(self, model, logits, target, B):
        loss = ops.cross_entropy(logits, target)
        return loss, {"prediction": loss.item()}, None

    def backward(self, logits, target, saved, gout, dt):
        return ops.cross_entropy_bwd(logits, target, gout, _dlogits(logits, dt))


class SupervisedHead:
    """forward on a use_cids model after MAGE.set_loss, or with batch['given']: mage_token_xent (include/mage_hip_ext.h) -- the cross entropy
    of CrossEntropyHead with class_weights (fp32 [K] or None), label_smoothing, a z_loss and given (bool per token, or None: the token's row
    is left out, F.cross_entropy's ignore_index).  tokens None: the pass runs over the batch's own video and forward's randomness terms are
    added on top, as for CrossEntropyHead.  parts: 'prediction' (the objective), 'nll' (the plain mean negative log-likelihood of the free
    tokens), 'accuracy' (the share of them the argmax predicts) and, with a mask, 'given_fraction'.  saved: the kernel's results."""

    def __init__(self, tokens=None, *, label_smoothing=0.0, z_loss=0.0, class_weights=None, given=None):
        self.tokens, self.given = tokens, given
        self.opts = dict(label_smoothing=float(label_smoothing), z_loss=float(z_loss), class_weight=class_weights)

    def forward(self, model, logits, target, B):
        res = ops.token_xent(logits, target, given=self.given, rank=False, **self.opts)
        s = res["summary"].tolist()
        parts = {"prediction": s[0], "nll": s[1], "accuracy": s[2]}
        if self.given is not None:
            parts["given_fraction"] = s[4]
        return res["summary"][0], parts, res

    def backward(self, logits, target, saved, gout, dt):
        return ops.token_xent_bwd(logits, target, saved["norm"], gout, _dlogits(logits, dt), given=self.given, **self.opts)


class MseHead:
    """forward on a MAGE+ model (mage_model.py:620): `logits` are the predicted latents, kept as model.last_logits."""
    tokens = None

    def forward(self, model, logits, target, B):
        E = model.first_stage_model.embed_dim
        loss = ops.mse(logits, target, rows=logits.shape[0], cols=E, lda=logits.shape[1], ldb=8)
        model.last_logits = logits
        return loss, {"prediction": loss.item()}, E

    def backward(self, logits, target, saved, gout, dt):
        g = ops.mse_bwd(logits, target, gout, rows=logits.shape[0], cols=saved, lda=logits.shape[1], ldb=8)
        return g if dt == F32 else ops.cast(g, _dlogits(g, dt))


class PolicyHead:
    """MAGE.policy_loss: the mage_policy_loss* pair that ops.policy_loss picks over the given tokens.  args: advantage (fp32, one per clip, frame
    or token), behaviour (fp32 per token, or None), the scalars temperature, top_k, top_p, clip_lo, clip_hi, entropy_coef of
    include/mage_hip_ext.h, and three options, each absent or None when not wanted:
      reference (fp32 per token) with kl_coef   parts gains 'kl' and 'unanchored_fraction' (PARTS' last two), saved 'kl';
      given (bool per token: given, not drawn)  the means are over the free tokens, parts gains 'given_fraction', saved 'norm';
      ratio_div (rows per group)                one importance ratio per group: parts as without it, saved gains 'group_logratio',
                                                'group_count' and 'norm'.
    saved: the kernel's results (cut, logprob, summary and the options' own); backward hands back what policy_loss_bwd needs of them."""
    PARTS = ("loss", "entropy", "approx_kl", "clip_fraction", "outside_fraction", "kl", "unanchored_fraction")

    def __init__(self, tokens, **args):
        self.tokens, self.args = tokens, args

    def forward(self, model, logits, target, B):
        a = self.args
        res = ops.policy_loss(logits, target, a["advantage"], a["behaviour"], **_policy_scalars(a), top_k=a["top_k"], top_p=a["top_p"])
        summary = res["summary"].tolist()                # [5], [7] with a reference, [8] with a mask or a group: the first 5 or 7 are the parts
        parts = dict(zip(self.PARTS[:5 if a.get("reference") is None else 7], summary))
        if a.get("given") is not None:
            parts["given_fraction"] = summary[7]
        return res["summary"][0], parts, res

    def backward(self, logits, target, saved, gout, dt):
        a = self.args
        left = {k: saved[k] for k in ("norm", "group_logratio") if k in saved}        # what the forward call left for this one
        return ops.policy_loss_bwd(logits, target, a["advantage"], a["behaviour"], saved["cut"], gout, _dlogits(logits, dt), **_policy_scalars(a),
                                   **left)


class PreferenceHead:
    """MAGE.preference_loss: mage_token_logprob (temperature 1, no filter: the model's own distribution), mage_clip_scores (one log-likelihood
    per clip) and mage_preference_loss over args' pairs (int64 [P, 2]) and reference (fp32 [B]) with the scalars beta, label_smoothing and mode
    (include/mage_hip_ext.h); backward is mage_token_logprob_bwd with the pair stage's one coefficient per clip.  saved: the pair stage's
    results plus logprob and clip_logprob.  With a 'given' (bool per token) one mage_apply_known_tokens launch writes the given slots'
    log-probability 0 before the clip totals -- what generation reports there -- and backward is mage_token_logprob_bwd_masked."""
    PARTS = ("loss", "accuracy", "chosen_reward", "rejected_reward", "margin")

    def __init__(self, tokens, **args):
        self.tokens, self.args = tokens, args

    def forward(self, model, logits, target, B):
        a = self.args
        lp = ops.token_logprob(logits, target, torch.empty(target.shape, device=logits.device, dtype=F32), rows=target.numel(), K=logits.shape[1],
                               ld=logits.stride(0))
        if a.get("given") is not None:
            ops.apply_known_tokens(target, torch.where(a["given"].view(target.shape), target, -1), rows=target.numel(), K=logits.shape[1],
                                   logprob=lp)
        clip_lp = ops.clip_scores(lp, n_clips=B)[0].view(B)
        res = ops.preference_loss(clip_lp, a["reference"], a["pairs"], beta=a["beta"], label_smoothing=a["label_smoothing"], mode=a["mode"])
        return res["summary"][0], dict(zip(self.PARTS, res["summary"].tolist())), dict(res, logprob=lp, clip_logprob=clip_lp)

    def backward(self, logits, target, saved, gout, dt):
        return ops.token_logprob_bwd(logits, target, saved["clip_coef"], gout, _dlogits(logits, dt), given=self.args.get("given"))


class DistillHead:
    """MAGE.distill_loss: mage_distill_loss of the pass's logits against a teacher's (fp32 [rows, K], MAGE.distill_targets' result) at
    `temperature`; mode 0: KL(teacher || student), 1: KL(student || teacher) (include/mage_hip_ext.h).  given (bool per token, or None): the
    token's row is left out; the means are over the free tokens.  saved: the kernel's results (row_kl, summary, norm)."""
    PARTS = ("loss", "teacher_entropy", "entropy", "agreement", "given_fraction")

    def __init__(self, tokens, *, teacher, temperature=1.0, mode=0, given=None):
        self.tokens, self.teacher, self.temperature, self.mode, self.given = tokens, teacher, temperature, mode, given

    def forward(self, model, logits, target, B):
        res = ops.distill_loss(logits, self.teacher, temperature=self.temperature, mode=self.mode, given=self.given)
        return res["summary"][0], dict(zip(self.PARTS, res["summary"].tolist())), res

    def backward(self, logits, target, saved, gout, dt):
        return ops.distill_loss_bwd(logits, self.teacher, saved["row_kl"], saved["norm"], gout, _dlogits(logits, dt),
                                    temperature=self.temperature, mode=self.mode, given=self.given)


class LogitsHead:
    """MAGE.distill_targets: the pass's logits themselves, fp32 [rows, K], handed back as `saved`; no loss of its own (a zero) and no
    backward pass."""

    def __init__(self, tokens):
        self.tokens = tokens

    def forward(self, model, logits, target, B):
        return torch.zeros((), device=logits.device, dtype=F32), {}, logits


def train_forward(model, batch, head=None):
    """Teacher-forced pass of MAGE.forward (mage_model.py:575-639) with the activations the backward pass needs.
    Returns (loss 0-dim fp32 tensor, tape).
    head: the loss head the pass ends in (above); None: the model's own, CrossEntropyHead or MseHead.  With head.tokens None the pass runs over
    the batch's own video and the loss gains forward's randomness terms (the prior's KL under beta, the PID, the speed l2 under alpha).  With
    given tokens (use_cids models) frame 0 is still first_stage_encode(images[:, 0:1]) and frames 1 .. L-1 are head.tokens; the loss is the
    head's alone (beta = alpha = 0), and with the randomness branch batch['video_noise'] (fp32 [B, 64, h, w], the recorded generation-time
    noise) modulates the motion anchor in place of the reparameterised video prior."""
    if head is None:
        head = CrossEntropyHead() if model.use_cids else MseHead()
    given = head.tokens is not None
    images = batch["images"]
    B = images.shape[0]
    R, L, Cc = model.image_resolution, model.frames_length, model.vision_width
    hw = R * R
    dt = model._dt()
    if dt == torch.float16:
        raise ValueError("precision 'f16' is a generation mode (forward values, autoregressive_generate): the backward kernels are bf16 / fp32 -- "
                         "train with set_precision('bf16') or 'fp32'")
    run = _Run(dt, model.dropout, model.training)
    run32 = _Run(F32, model.dropout, model.training)
    run32.seed, run32.p = run.seed, run.p
    run32.site = 1 << 20            # its own stream of dropout sites: the decoder's and the encoders' layers never share a seed
    run32.sk = ops.F16X3 if (dt != F32 and config.get().train_enc_split) else 0
    d = model._derived.get(model._build)
    dev = images.device
    tok = tok_in = tok0 = lat_all = lat_in = lat0 = None
    if model.use_cids:
        if given:
            tok = torch.cat([model.first_stage_encode(images[:, 0:1]).reshape(B, 1, hw), head.tokens.reshape(B, L - 1, hw)], 1)
        else:
            tok = model.first_stage_encode(images).reshape(B, -1, hw)                 # frozen first stage: no gradient
        tok_in = tok[:, :L - 1].contiguous()
        tok0 = tok[:, 0].contiguous()
        # frame features for the decoder (compute dtype) and, as the inference prologue does, frame 0's in fp32 for the MA encoder
        emb = ops.embedding(tok_in.reshape(-1), d["emb"], torch.empty(B * (L - 1) * hw, Cc, device=dev, dtype=dt))
        emb0 = ops.embedding(tok0.reshape(-1), d["emb"], torch.empty(B * hw, Cc, device=dev, dtype=F32))
    else:
        # MAGE+ (mage_model.py:579,583): latents of ALL frames from the external first stage as zero-padded rows [., LD], token
        # embedding = Linear(embed_dim -> C)
        E, LD = model.first_stage_model.embed_dim, 8
        lat = model.first_stage_encode(images)                                        # [B, Lb, E, h, w]
        Lb = lat.shape[1]
        lat_all = torch.zeros(B, Lb, hw, LD, device=dev, dtype=F32)
        lat_all[..., :E] = lat.permute(0, 1, 3, 4, 2).reshape(B, Lb, hw, E).float()   # layout plumbing (channels last)
        lat_in = lat_all[:, :L - 1].contiguous().view(-1, LD)
        lat0 = lat_all[:, 0].contiguous().view(-1, LD)
        lin = dict(N=Cc, K=E, lda=LD, ldy=Cc, bias=d["emb_lin.b"])
        emb = ops.gemm(lat_in, d["emb_lin.w"], torch.empty(B * (L - 1) * hw, Cc, device=dev, dtype=dt), M=B * (L - 1) * hw, **lin)
        emb0 = ops.gemm(lat0, d["emb_lin.w"], torch.empty(B * hw, Cc, device=dev, dtype=F32), M=B * hw, **lin)
    if model.use_cids and dt == BF16 and Cc % 64 == 0 and config.get().train_taps:
        # the generation path's padded-taps convolution (embedding rows written into a zero-padded frame buffer: the 8-phase kernel
        # instead of the per-lane gather, 1.45 -> 0.9 ms at cfg2); emb (plain rows) stays the backward pass's operand
        feats = model._frame_features(tok_in, dt)
    else:
        feats = VectorQuantizedVAE._conv(emb, d["conv" + _sfx(dt)], torch.empty_like(emb), n_img=B * (L - 1), H=R, W=R, cin=Cc, cout=Cc, k=3,
                                         rowadd=d["hwpos"], rowadd_div=1, rowadd_mod=hw)
    first = VectorQuantizedVAE._conv(emb0, d["conv.f32"], torch.empty_like(emb0), n_img=B, H=R, W=R, cin=Cc, cout=Cc, k=3,
                                     rowadd=d["hwpos"], rowadd_div=1, rowadd_mod=hw)
    txt, t_text = _text_forward(model.text_encoder, run32, batch["text"])
    S = batch["text"].shape[1]
    ma, t_ma = _ma_forward(model.ma_encoder, run32, first, txt, B, hw, S)
    t_rand = None
    if model.randomness:                                                     # :601-609: ADAIN modulation by the reparameterised video prior
        from . import mage_train_prior
        if given:
            # the policy is conditioned on the noise its tokens were generated under (batch['video_noise'], recorded by the generation):
            # generation's modulation -- conv_d2, the ADAIN convolutions, ADAIN -- without the Conv3d prior, which generation never runs
            nz = batch["video_noise"].permute(0, 2, 3, 1).reshape(B * hw, 64).contiguous()
            ma, t_rand = mage_train_prior.modulate_forward(model, nz, ma, B)
        else:
            ma, t_rand = mage_train_prior.rand_forward(model, batch, tok, ma, B, lat_rows=None if model.use_cids else lat_all.view(-1, 8),
                                                       L=0 if model.use_cids else lat_all.shape[1])
    speed = None
    if "speed" in batch:
        speed = batch["speed"].float().contiguous()
        ma = ma.clone()
        ops.add_scaled_rowvec(ma, speed, d["speed"], B=B, P=hw, Cc=Cc)
    ma_dt = ma if dt == F32 else ma.to(dt)
    logits, t_dec = _dec_forward(model.generate_model, run, ma_dt, feats, B, R, R)
    if model.use_cids:
        target = tok[:, 1:L].reshape(-1).contiguous()
    else:
        target = lat_all[:, 1:L].contiguous().view(-1, 8)
    recon, parts, saved = head.forward(model, logits, target, B)
    loss, beta, alpha = recon, 0.0, 0.0
    if not given:                                                            # forward's own terms; a given-tokens head's loss is final
        if model.randomness:                                                 # :622-632 ([B]-element reductions and scalars)
            kl = -0.5 * t_rand["kl_sum"].mean()
            parts["kl_loss"] = kl.item()
            if model.auto_beta:
                model.beta, _ = model.PID.pid(model.KL_loss, parts["kl_loss"])
                parts["beta"] = model.beta
                beta = float(model.beta)
                loss = recon + beta * kl
            else:
                if speed is None:
                    raise KeyError("MAGE.forward with randomness=True and auto_beta=False needs batch['speed'] (mage_model.py:631)")
                beta, alpha = float(model.beta), float(model.alpha)
                l2 = (speed ** 2).mean() * (d["speed"] ** 2).sum()
                loss = recon + beta * kl + alpha * l2
        parts["final_loss"] = loss.item()
    tape = dict(run=run, run32=run32, tok_in=tok_in, tok0=tok0, lat_in=lat_in, lat0=lat0, emb=emb, emb0=emb0, text=t_text, ma=t_ma, dec=t_dec,
                logits=logits, target=target, speed=speed, B=B, rand=t_rand, beta=beta, alpha=alpha, parts=parts, head=head, saved=saved)
    return loss, tape


def train_backward(model, tape, grad_out: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Gradients of every trainable parameter, keyed by state_dict name (fp32, the parameter's shape)."""
    run, run32 = tape["run"], tape["run32"]
    dt = run.dt
    R, L, Cc, B = model.image_resolution, model.frames_length, model.vision_width, tape["B"]
    hw = R * R
    dev = tape["logits"].device
    grads: Dict[str, torch.Tensor] = {}
    gout = grad_out.detach().to(device=dev, dtype=F32).reshape(1).contiguous()
    head = tape["head"]
    dlogits = head.backward(tape["logits"], tape["target"], tape["saved"], gout, dt)
    tape["logits"] = None
    dfeats, dma = _dec_backward(model.generate_model, run, tape["dec"], dlogits, grads)
    del dlogits
    acc: Dict[str, Optional[torch.Tensor]] = {}
    _frame_backward(model, dt, None if tape["tok_in"] is None else tape["tok_in"].reshape(-1), tape["emb"], dfeats, grads, acc,
                    lat_rows=tape["lat_in"])
    del dfeats
    if tape["speed"] is not None:                                            # ma += speed_b * speed_embedding  (:666-668)
        gs = ops.group_rowsum(dma, torch.empty(1, Cc, device=dev, dtype=F32), rows=B * hw, C=Cc, div=1, mod=1, row_scale=tape["speed"],
                              row_scale_div=hw)
        if tape["alpha"] != 0.0:                                             # alpha * mean_b(speed_b^2) * |speed_embedding|^2  (:631)
            d = model._derived.get(model._build)
            gs = gs + (2.0 * tape["alpha"]) * gout * (tape["speed"] ** 2).mean() * d["speed"].view(1, Cc)
        grads["speed_embedding"] = gs
    if tape["rand"] is not None:
        from . import mage_train_prior
        if head.tokens is not None:                                          # given tokens: the noise is a recorded constant: the ADAIN half, no dz
            dma, _ = mage_train_prior.modulate_backward(model, tape["rand"], dma, grads, want_dz=False)
        else:
            kl_coef = (gout * (tape["beta"] / B)).contiguous()
            dma = mage_train_prior.rand_backward(model, tape["rand"], dma, kl_coef, grads, acc)
        tape["rand"] = None
    dfirst, dtxt = _ma_backward(model.ma_encoder, run32, tape["ma"], dma, grads)
    _text_backward(model.text_encoder, run32, tape["text"], dtxt, grads)
    _frame_backward(model, F32, None if tape["tok0"] is None else tape["tok0"].reshape(-1), tape["emb0"], dfirst, grads, acc,
                    lat_rows=tape["lat0"])
    if model.use_cids:
        grads["visual_token_embedding.weight"] = acc["emb"]
    else:
        E = model.first_stage_model.embed_dim
        grads["visual_token_embedding.weight"] = acc["emb_lin.w"][:, :E].contiguous()
        grads["visual_token_embedding.bias"] = acc["emb_lin.b"]
    grads["conv.0.weight"] = acc["conv"].view(Cc, 3, 3, Cc).permute(0, 3, 1, 2).contiguous()       # [Cout, Cin, kh, kw] layout
    hp = acc["hwpos"].contiguous()                                           # [R*R, C] -> H table (sum over w), W table (sum over h)
    grads["H_positional_embedding"] = ops.group_rowsum(hp, torch.empty(R, Cc, device=dev, dtype=F32), rows=hw, C=Cc, div=R,
                                                       mod=R).view(1, R, 1, Cc)
    grads["W_positional_embedding"] = ops.group_rowsum(hp, torch.empty(R, Cc, device=dev, dtype=F32), rows=hw, C=Cc, div=1,
                                                       mod=R).view(1, 1, R, Cc)
    return grads


def trainable_names(model):
    return [n for n, p in model.named_parameters() if p.requires_grad]


class MageLossFn(torch.autograd.Function):
    """loss = MageLossFn.apply(model, batch, head, names, *params): autograd sees one node whose inputs are the trainable parameters.
    head: train_forward's.  What the MAGE method reads back -- the loss dict (the reference's loss_dict values, without the prefix) and what the
    head saved -- is left in model._last_head_out for it to take and clear."""

    @staticmethod
    def forward(ctx, model, batch, head, names, *params):
        with torch.no_grad():
            loss, tape = train_forward(model, batch, head)
        model._last_head_out = (tape["parts"], tape["saved"])
        ctx.model, ctx.tape, ctx.names, ctx.shapes = model, tape, names, [p.shape for p in params]
        ctx.devices = [p.device for p in params]
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.tape is None:
            raise RuntimeError("MAGE training graph: backward through the same forward a second time (activations were released)")
        with torch.no_grad(), torch.cuda.device(ctx.devices[0]):
            grads = train_backward(ctx.model, ctx.tape, grad_out)
        ctx.tape = None
        out = []
        for n, shp, dev in zip(ctx.names, ctx.shapes, ctx.devices):
            g = grads.get(n)
            out.append(g.reshape(shp) if g is not None else torch.zeros(shp, device=dev, dtype=F32))     # ln_q / ln_kv: unused -> 0
        return (None, None, None, None, *out)
