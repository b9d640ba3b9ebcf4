"""MI355X-native MAGE (drop-in for the reference's modules/mage_model.py).

Same class names, constructor kwargs, ``forward`` / ``autoregressive_generate`` signatures and
state_dict layout as the reference (mage_model.py:15-693).  ``nn.Linear`` /
``nn.MultiheadAttention`` / ``nn.LayerNorm`` objects are parameter containers only; all arithmetic is
libmage_hip.so: channels-last activations ([B, L, H, W, C] is a row-major [tokens, C] matrix), axial
attention over strided row sets (no permute/contiguous copies -- the reference spends 19 % of its time
there), LayerNorm / bias / QuickGELU / residual / positional tables fused around MFMA GEMMs.

Precision: ``set_precision('fp32')`` (default; exact-fp32 MFMA, the parity mode), ``'bf16'``
(bf16 MFMA with fp32 accumulation for the decoder stack and VQ-VAE decode; the residual stream,
LayerNorm, softmax, logits, the once-per-clip prologue and the VQ-VAE encode + quantiser stay fp32), or the
FAST PARITY modes ``'f16x3'`` / ``'bf16x3'``: everything as in fp32 mode except that the decoder's Linear layers and
the frame convolution multiply split-precision operands (x ~ hi + lo in two 16-bit pieces; three f16 / bf16 MFMA
products per K slab, fp32 accumulation -- include/mage_hip.h): fp32-class logits at 3/16 of the exact-fp32 MFMA cost.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import math
from collections import OrderedDict
from math import exp
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from .. import config, ops
from ..utils.util import default, instantiate_from_config, zero_module
from .vqvae_model import VectorQuantizedVAE, _Derived, _conv_w, _no_torch_forward, weights_frozen

__all__ = ["QuickGELU", "AxialAttentionBlock", "TransformerBlock", "MAEncoder", "TransformerTextEncoder", "BasicBlock",
           "ADAIN2D", "FlatAxialDecoder", "PIDControl", "MAGE"]

F32 = torch.float32
BF16 = torch.bfloat16
F16 = torch.float16
HALF_TYPES = (BF16, F16)                      # the 16-bit compute dtypes: the same kernels on v_mfma_f32_16x16x32_bf16 / _f16


def _sfx(dt: torch.dtype) -> str:
    return ".f32" if dt == F32 else ".bf16" if dt == BF16 else ".f16"


def _wdt(d: Dict[str, torch.Tensor], name: str, dt: torch.dtype) -> torch.Tensor:
    """The copy of the fp32 weight d[name + '.f32'] in the compute dtype (the f16 copies are built on first use: most models never ask)."""
    w = d.get(name + _sfx(dt))
    if w is None:
        w = d[name + _sfx(dt)] = d[name + ".f32"].to(dt)
    return w


# name -> (compute dtype of the decoder stack, split kind).  'f16' = the bf16 mode's kernels, schedules and data flow with IEEE half operands
# (11 significand bits instead of 8, same MFMA rate): every rounding of 'bf16' mode is 8x smaller; values must stay inside +-65504.
PRECISIONS = {"fp32": (F32, 0), "bf16": (BF16, 0), "f16": (F16, 0), "bf16x3": (F32, ops.BF16X3), "f16x3": (F32, ops.F16X3)}


class FrameTokens:
    """Frames handed to the decoder as TOKEN IDS [n_img, hw] instead of features: conv3x3(embedding(ids)) + positions and the
    decoder's in_linear are one table sum straight into the residual stream (MAGE._frame_tables, mage_table_conv)."""

    def __init__(self, tokens: torch.Tensor, T2: torch.Tensor, P2: torch.Tensor, R: int):
        self.tokens, self.T2, self.P2, self.R = tokens.contiguous(), T2, P2, R

    def fill(self, x: torch.Tensor, *, n_img: int, per_clip: int, P: int, y_off: int, tp: torch.Tensor) -> None:
        """Rows (clip b, slot y_off/hw + l) of x [B*P*hw, C] (fp32, or the bf16 stream) <- in_linear(conv(emb(ids[b, l])) + H/W positions)
        + T positions."""
        hw = self.R * self.R
        ops.table_conv(self.tokens, self.T2, x, n_img=n_img, H=self.R, W=self.R, pos=self.P2, rowadd=tp, rowadd_div=hw, rowadd_mod=P,
                       ldy=x.shape[1], group=per_clip * hw, y_group_stride=P * hw, y_off=y_off)


def _wsplit(d: Dict[str, torch.Tensor], name: str, kind: int) -> torch.Tensor:
    """Split-precision copy of the fp32 weight d[name + '.f32'] ([N, K] -> [N, 2K] 16-bit pieces), built on first use."""
    key = f"{name}.s{kind}"
    w = d.get(key)
    if w is None:
        w = d[key] = ops.split(d[name + ".f32"].reshape(d[name + ".f32"].shape[0], -1), kind)
    return w


def _to_dt(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """fp32 rows in the decoder's compute dtype (mage_cast)."""
    return x if dt == x.dtype else ops.cast(x.contiguous(), torch.empty(x.shape, device=x.device, dtype=dt))


def _assemble(images: torch.Tensor, video: torch.Tensor) -> torch.Tensor:
    """The result of autoregressive_generate (mage_model.py:691): the input's first frame followed by the decoded frames."""
    if images.dtype == video.dtype and video.is_contiguous() and images[0, 0].is_contiguous():
        return ops.assemble_video(images, video)
    return torch.cat([images[:, 0:1].to(video.dtype), video], 1)


def _need_gpu(t: torch.Tensor, who: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on libmage_hip.so kernels: move the model and the batch to a ROCm GPU "
                           "(there is no CPU / PyTorch fallback)")


def _pack_linear(d: Dict[str, torch.Tensor], name: str, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> None:
    w = weight.float().contiguous()
    d[name + ".f32"] = w
    d[name + ".bf16"] = w.to(BF16)
    if bias is not None:
        d[name + ".b"] = bias.float().contiguous()


def _linear(a, d, name, y, dt, *, M, N, K, sk=0, lo=0, hi=None, **kw):
    """The Linear layer `name` of the derived weights d: y = a @ W[lo:hi]^T + b[lo:hi] (+ the epilogue that kw asks of ops.gemm).
    sk = 0: the weight copy in the compute dtype dt (fp32: the exact-fp32 MFMA chain).  sk = BF16X3 / F16X3 (the fast parity modes, and the
    once-per-clip encoders outside precision 'fp32'; dt is fp32 there): split-precision operands, three 16-bit MFMA products per K slab
    (mage_hip.h) -- 3x the fp32 chain's rate and a smaller error than its own accumulation (profiles/r03_split_probe.txt).  `a` is taken as
    is where its producer wrote split rows and split here (one small pass) otherwise; y receives split rows if that is its dtype.  A K that
    is no multiple of 64 and an epilogue the split GEMM does not have (the exact GELU) keep the dt chain."""
    b = d.get(name + ".b")
    if sk and K % 64 == 0 and kw.get("act", ops.ACT_NONE) in (ops.ACT_NONE, ops.ACT_QUICKGELU):
        sdt = ops.split_dtype(sk)
        assert dt == F32 and y.dtype in (F32, sdt)       # so the dtype alone tells split rows from plain ones
        if a.dtype != sdt:
            a = ops.split(a, sk)
        y_split = y.dtype == sdt
        w, lda, ldy = _wsplit(d, name, sk), 2 * K, 2 * N if y_split else N          # split rows: 2 16-bit elements per logical column
        kw.update(split_kind=sk, y_split=y_split)
    else:
        w, lda, ldy = _wdt(d, name, dt), K, N
    if lo or hi is not None:
        w, b = w[lo:hi], (None if b is None else b[lo:hi])
    return ops.gemm(a, w, y, M=M, N=N, K=K, lda=kw.pop("lda", lda), ldy=kw.pop("ldy", ldy), bias=b, **kw)


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x) (mage_model.py:11-13); fused into the c_fc GEMM epilogue on the GPU path."""

    forward = _no_torch_forward


def _mlp(d_model: int) -> nn.Sequential:
    return nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                      ("c_proj", nn.Linear(d_model * 4, d_model))]))


class AxialAttentionBlock(nn.Module):
    """Parameter container with the reference's keys (mage_model.py:15-29)."""

    def __init__(self, d_model: int, n_head: int, dropout: float = 0.1, axial_dim: int = 1):
        super().__init__()
        self.d_model, self.n_head, self.axial_dim = d_model, n_head, axial_dim
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = _mlp(d_model)
        self.ln_2 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)

    forward = _no_torch_forward


class TransformerBlock(nn.Module):
    """Parameter container (mage_model.py:72-85); ln_q / ln_kv exist in checkpoints but MAGE never applies them (:92)."""

    def __init__(self, d_model: int, n_head: int, dropout: float = 0.1):
        super().__init__()
        self.d_model, self.n_head = d_model, n_head
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_q = nn.LayerNorm(d_model)
        self.ln_kv = nn.LayerNorm(d_model)
        self.mlp = _mlp(d_model)
        self.ln_2 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)

    forward = _no_torch_forward


def _pack_block(d: Dict[str, torch.Tensor], p: str, blk) -> None:
    _pack_linear(d, p + ".in_proj", blk.attn.in_proj_weight, blk.attn.in_proj_bias)
    _pack_linear(d, p + ".out_proj", blk.attn.out_proj.weight, blk.attn.out_proj.bias)
    _pack_linear(d, p + ".c_fc", blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
    _pack_linear(d, p + ".c_proj", blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)
    for ln in ("ln_1", "ln_2", "ln_q", "ln_kv"):
        if hasattr(blk, ln):
            d[f"{p}.{ln}.w"] = getattr(blk, ln).weight.float().contiguous()
            d[f"{p}.{ln}.b"] = getattr(blk, ln).bias.float().contiguous()


class MAEncoder(nn.Module):
    """Motion-anchor cross-attention encoder (mage_model.py:104-117).  ``forward(x, kv)`` keeps the reference's
    sequence-first convention: x [Tq, B, C], kv [Tk, B, C] -> [Tq, B, C]; rows are addressed by stride, not permuted."""

    def __init__(self, layers: int, d_model: int, dropout: float = 0.1):
        super().__init__()
        self.d_model, self.layers = d_model, layers
        self.blocks = nn.ModuleList([TransformerBlock(d_model, d_model // 32, dropout) for _ in range(layers)])
        self.mage_plus = False          # True = the ln_q/ln_kv variant of mage_model.py:93 (MAGE+); MAGE(use_cids=False) sets it
        self.split_kind = 0             # ops.F16X3 outside precision 'fp32' (MAGE.set_precision): Linear layers on split operands (_linear)
        self._derived = _Derived(self)

    def _build(self):
        d: Dict[str, torch.Tensor] = {}
        for i, blk in enumerate(self.blocks):
            _pack_block(d, f"b{i}", blk)
        return d

    @torch.no_grad()
    def _run(self, q: torch.Tensor, kv: torch.Tensor, *, B: int, nq: int, nk: int, seq_first: bool) -> torch.Tensor:
        """q [B*nq, C] / kv [B*nk, C] fp32 rows (batch-first: row = b*n + i; seq-first: row = i*B + b)."""
        d = self._derived.get(self._build)
        Cc, dev, H = self.d_model, q.device, self.d_model // 32
        x = q.float().contiguous().clone()
        kv = kv.float().contiguous()
        inner, qo, qa, ko, ka = (B, 0, B, 0, B) if seq_first else (1, nq, 1, nk, 1)
        sk = self.split_kind if Cc % 64 == 0 else 0

        def rows(n):
            """The q rows of an operand of the next Linear (n columns): split rows straight from their producers -- the attention, LayerNorm,
            the c_fc epilogue (QuickGELU) -- where the Linear layers take those."""
            return ops.split_empty(B * nq, n, sk, dev) if sk else torch.empty(B * nq, n, device=dev, dtype=F32)

        for i in range(self.layers):
            p = f"b{i}"
            qin, kvin = x, kv
            if self.mage_plus:
                qin = ops.layernorm(x, d[p + ".ln_q.w"], d[p + ".ln_q.b"], torch.empty_like(x), 1e-5)
                kvin = ops.layernorm(kv, d[p + ".ln_kv.w"], d[p + ".ln_kv.b"], torch.empty_like(kv), 1e-5)
            qp = _linear(qin, d, p + ".in_proj", torch.empty(B * nq, Cc, device=dev, dtype=F32), F32, M=B * nq, N=Cc, K=Cc, sk=sk, lo=0, hi=Cc)
            kvp = _linear(kvin, d, p + ".in_proj", torch.empty(B * nk, 2 * Cc, device=dev, dtype=F32), F32, M=B * nk, N=2 * Cc, K=Cc, sk=sk,
                          lo=Cc, hi=3 * Cc)
            ao = rows(Cc)
            ops.attention(qp, kvp[:, :Cc], kvp[:, Cc:], ao, ldq=Cc, ldk=2 * Cc, ldv=2 * Cc, ldo=ao.shape[1], n_seq=B, inner=inner,
                          nq=nq, nk=nk, n_head=H, q_outer_stride=qo, q_axis_stride=qa, kv_outer_stride=ko, kv_axis_stride=ka, out_split=sk)
            _linear(ao, d, p + ".out_proj", x, F32, M=B * nq, N=Cc, K=Cc, sk=sk, residual=x, ldr=Cc)
            xn = ops.layernorm(x, d[p + ".ln_2.w"], d[p + ".ln_2.b"], rows(Cc), 1e-5, split_kind=sk)
            hdn = _linear(xn, d, p + ".c_fc", rows(4 * Cc), F32, M=B * nq, N=4 * Cc, K=Cc, sk=sk, act=ops.ACT_QUICKGELU)
            _linear(hdn, d, p + ".c_proj", x, F32, M=B * nq, N=Cc, K=4 * Cc, sk=sk, residual=x, ldr=Cc)
        return x

    def forward(self, x: torch.Tensor, kv: torch.Tensor, key_mask=None, need_weights=False):
        _need_gpu(x, "MAEncoder")
        if key_mask is not None:
            raise NotImplementedError("key_mask is never passed by MAGE (mage_model.py:596,657)")
        Tq, B, Cc = x.shape
        return self._run(x.reshape(Tq * B, Cc), kv.reshape(-1, Cc), B=B, nq=Tq, nk=kv.shape[0], seq_first=True).view(Tq, B, Cc)


class TransformerTextEncoder(nn.Module):
    """Text encoder (mage_model.py:180-250): token+position embedding -> LN(eps 1e-8) -> zero padded rows ->
    post-norm encoder layers (erf-GELU, key-padding mask) -> LN -> Linear.  forward(text int64 [B,S]) -> [B,S,out]."""

    def __init__(self, vocab_size: int, transformer_width: int, transformer_layers: int, output_dim: int,
                 context_length: int, padding_idx: int = 0, dropout: float = 0.1):
        super().__init__()
        self.vocab_size, self.padding_idx = vocab_size, padding_idx
        self.transformer_width, self.context_length = transformer_width, context_length
        self.transformer_layers, self.output_dim = transformer_layers, output_dim
        layer = nn.TransformerEncoderLayer(transformer_width, transformer_width // 32, dim_feedforward=transformer_width * 4,
                                           dropout=dropout, activation="gelu")
        self.transformer = nn.TransformerEncoder(layer, transformer_layers, enable_nested_tensor=False)
        self.token_embedding = nn.Embedding(vocab_size, transformer_width, padding_idx=padding_idx)
        self.positions = nn.Embedding(context_length, transformer_width)
        self.layer_norm = nn.LayerNorm(transformer_width, eps=1e-8, elementwise_affine=True)
        self.dropout = nn.Dropout(p=dropout)
        self.ln_text_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Linear(transformer_width, output_dim)
        self.apply(self._init_weights)
        self._derived = _Derived(self)

    @staticmethod
    def _init_weights(module):
        """mage_model.py:211-221."""
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=0.02)
        elif isinstance(module, nn.MultiheadAttention):
            module.in_proj_weight.data.normal_(mean=0.0, std=0.02)
            module.out_proj.weight.data.normal_(mean=0.0, std=0.02)
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()

    def _build(self):
        d: Dict[str, torch.Tensor] = {"tok": self.token_embedding.weight.float().contiguous(),
                                      "pos": self.positions.weight.float().contiguous()}
        for n in ("layer_norm", "ln_text_final"):
            d[n + ".w"], d[n + ".b"] = getattr(self, n).weight.float().contiguous(), getattr(self, n).bias.float().contiguous()
        _pack_linear(d, "proj", self.text_projection.weight, self.text_projection.bias)
        for i, l in enumerate(self.transformer.layers):
            _pack_linear(d, f"l{i}.in_proj", l.self_attn.in_proj_weight, l.self_attn.in_proj_bias)
            _pack_linear(d, f"l{i}.out_proj", l.self_attn.out_proj.weight, l.self_attn.out_proj.bias)
            _pack_linear(d, f"l{i}.fc1", l.linear1.weight, l.linear1.bias)
            _pack_linear(d, f"l{i}.fc2", l.linear2.weight, l.linear2.bias)
            for n in ("norm1", "norm2"):
                d[f"l{i}.{n}.w"], d[f"l{i}.{n}.b"] = getattr(l, n).weight.float().contiguous(), getattr(l, n).bias.float().contiguous()
                d[f"l{i}.{n}.eps"] = getattr(l, n).eps
        return d

    @torch.no_grad()
    def forward(self, text: torch.Tensor) -> torch.Tensor:
        _need_gpu(text, "TransformerTextEncoder")
        d = self._derived.get(self._build)
        B, S = text.shape
        if S > 64 or S > self.context_length:
            raise ValueError(f"caption length {S} exceeds context_length {self.context_length} (kernel limit 64)")
        Wd, dev, H = self.transformer_width, text.device, self.transformer_width // 32
        ids = text.to(torch.int64).contiguous()
        kv_len, keep = ops.caption_mask(ids, self.padding_idx)          # key-padding lengths, row scale of the padded rows (:233-239)
        x = ops.embedding(ids, d["tok"], torch.empty(B * S, Wd, device=dev, dtype=F32))
        ops.row_affine(x, None, d["pos"], div=1, mod=S)                  # + positions[0..S)       (:227-228)
        ops.layernorm(x, d["layer_norm.w"], d["layer_norm.b"], x, self.layer_norm.eps)
        ops.row_affine(x, keep, None)                                    # zero padded rows          (:233-235)
        sk = getattr(self, "split_kind", 0) if Wd % 64 == 0 else 0
        for i in range(self.transformer_layers):
            p = f"l{i}"
            qkv = _linear(x, d, p + ".in_proj", torch.empty(B * S, 3 * Wd, device=dev, dtype=F32), F32, M=B * S, N=3 * Wd, K=Wd, sk=sk)
            ao = ops.split_empty(B * S, Wd, sk, dev) if sk else torch.empty(B * S, Wd, device=dev, dtype=F32)
            ops.attention(qkv, qkv[:, Wd:], qkv[:, 2 * Wd:], ao, ldq=3 * Wd, ldk=3 * Wd, ldv=3 * Wd, ldo=ao.shape[1], n_seq=B, inner=1,
                          nq=S, nk=S, n_head=H, q_outer_stride=S, q_axis_stride=1, kv_outer_stride=S, kv_axis_stride=1,
                          kv_len=kv_len, kv_len_div=1, out_split=sk)
            _linear(ao, d, p + ".out_proj", x, F32, M=B * S, N=Wd, K=Wd, sk=sk, residual=x, ldr=Wd)
            ops.layernorm(x, d[p + ".norm1.w"], d[p + ".norm1.b"], x, d[p + ".norm1.eps"])
            # the exact GELU is not a split-GEMM epilogue: _linear keeps this Linear on the fp32 chain in every mode
            hdn = _linear(x, d, p + ".fc1", torch.empty(B * S, 4 * Wd, device=dev, dtype=F32), F32, M=B * S, N=4 * Wd, K=Wd, sk=sk,
                          act=ops.ACT_GELU_ERF)
            _linear(hdn, d, p + ".fc2", x, F32, M=B * S, N=Wd, K=4 * Wd, sk=sk, residual=x, ldr=Wd)
            ops.layernorm(x, d[p + ".norm2.w"], d[p + ".norm2.b"], x, d[p + ".norm2.eps"])
        ops.layernorm(x, d["ln_text_final.w"], d["ln_text_final.b"], x, self.ln_text_final.eps)
        out = _linear(x, d, "proj", torch.empty(B * S, self.output_dim, device=dev, dtype=F32), F32, M=B * S, N=self.output_dim, K=Wd, sk=sk)
        return out.view(B, S, self.output_dim)


class BasicBlock(nn.Module):
    """Conv3d + GroupNorm video-prior block (mage_model.py:264-297), used by MAGE.forward with randomness=True only.
    Parameter container with the reference's keys; MAGE._video_prior runs the four blocks on the GPU (three temporal-tap
    implicit GEMMs per Conv3d + mage_groupnorm_act)."""

    def __init__(self, in_planes, out_planes, stride=1, stride_t=1, downsample=False, spectral=False):
        super().__init__()
        st = [stride_t, stride, stride]
        self.conv1 = nn.Conv3d(in_planes, out_planes, kernel_size=(3, 3, 3), stride=st, padding=1, bias=False)
        self.bn1 = nn.GroupNorm(num_groups=16, num_channels=out_planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv3d(out_planes, out_planes, kernel_size=(3, 3, 3), stride=[1, 1, 1], padding=1, bias=False)
        self.bn2 = nn.GroupNorm(num_groups=16, num_channels=out_planes)
        self.downsample = nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=(3, 3, 3), stride=st, padding=[1, 1, 1],
                                                  bias=False),
                                        nn.GroupNorm(num_channels=out_planes, num_groups=16)) if downsample else None
        self.stride = stride
        if spectral:
            self.conv1 = torch.nn.utils.spectral_norm(self.conv1)
            self.conv2 = torch.nn.utils.spectral_norm(self.conv2)

    forward = _no_torch_forward


class ADAIN2D(nn.Module):
    """InstanceNorm2d(x) * conv_mu(y) + conv_var(y) (mage_model.py:299-314).  forward(x, y) takes the reference's
    NCHW tensors; the GPU path runs channels-last."""

    def __init__(self, num_features, z_dim):
        super().__init__()
        self.num_features = num_features
        self.norm = nn.InstanceNorm2d(num_features, affine=False, track_running_stats=False)
        self.conv_mu = nn.Sequential(nn.Conv2d(z_dim, num_features, 3, 1, 1), nn.Conv2d(num_features, num_features, 3, 1, 1))
        self.conv_var = nn.Sequential(nn.Conv2d(z_dim, num_features, 3, 1, 1), nn.Conv2d(num_features, num_features, 3, 1, 1))
        self._derived = _Derived(self)

    def _build(self):
        d: Dict[str, torch.Tensor] = {}
        for n, seq in (("mu", self.conv_mu), ("var", self.conv_var)):
            for j in range(2):
                d[f"{n}{j}.w"] = _conv_w(seq[j])
                d[f"{n}{j}.b"] = seq[j].bias.float().contiguous()
        return d

    @torch.no_grad()
    def _run(self, x_rows: torch.Tensor, y_rows: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """x_rows [B*H*W, C] fp32 (motion anchor), y_rows [B*H*W, z] fp32 -> [B*H*W, C]."""
        d = self._derived.get(self._build)
        Cc, z, dev = self.num_features, y_rows.shape[1], x_rows.device
        outs = []
        for n in ("mu", "var"):
            t = VectorQuantizedVAE._conv(y_rows, d[n + "0.w"], torch.empty(B * H * W, Cc, device=dev, dtype=F32), n_img=B, H=H,
                                         W=W, cin=z, cout=Cc, k=3, bias=d[n + "0.b"])
            outs.append(VectorQuantizedVAE._conv(t, d[n + "1.w"], torch.empty(B * H * W, Cc, device=dev, dtype=F32), n_img=B,
                                                 H=H, W=W, cin=Cc, cout=Cc, k=3, bias=d[n + "1.b"]))
        return ops.adain(x_rows, outs[0], outs[1], torch.empty_like(x_rows), B=B, P=H * W, Cc=Cc, eps=self.norm.eps)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _need_gpu(x, "ADAIN2D")
        B, Cc, H, W = x.shape
        xr = x.permute(0, 2, 3, 1).reshape(B * H * W, Cc).float().contiguous()
        yr = y.permute(0, 2, 3, 1).reshape(B * H * W, -1).float().contiguous()
        return self._run(xr, yr, B, H, W).view(B, H, W, Cc).permute(0, 3, 1, 2)


class FlatAxialDecoder(nn.Module):
    """Axial-attention AR decoder (mage_model.py:317-390): in/context Linear -> concat along L -> + T positions ->
    `layers` blocks attending along L (causal), H, W in turn -> Linear head on x[:, 1:]."""

    def __init__(self, in_channels, model_channels, out_channels, frames_length, layers, context_channels=None, use_cids=True,
                 dropout=0.1):
        super().__init__()
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.frames_length, self.layers = frames_length, layers
        self.in_linear = nn.Linear(in_channels, model_channels)
        context_channels = default(context_channels, in_channels)
        self.context_channels = context_channels
        self.context_linear = nn.Linear(context_channels, model_channels)
        scale = model_channels ** -0.5
        self.T_positional_embedding = nn.Parameter(scale * torch.randn(frames_length, 1, 1, model_channels))
        num_heads = model_channels // 32
        self.blocks = nn.ModuleList([AxialAttentionBlock(model_channels, num_heads, axial_dim=i % 3 + 1, dropout=dropout)
                                     for i in range(layers)])
        self.use_cids = use_cids
        if use_cids:
            self.out = nn.Linear(model_channels, out_channels)
        else:
            self.out = nn.Sequential(nn.GroupNorm(32, model_channels), nn.SiLU(),
                                     zero_module(nn.Conv3d(model_channels, out_channels, 1)))
        self.initialize_parameters()
        self.compute_dtype = F32
        self.split_kind = 0                    # ops.BF16X3 / ops.F16X3: the fast parity modes (compute_dtype stays fp32)
        self.stream_bf16 = True                # bf16 mode: x stays in bf16 between the blocks (_stream_bf16)
        self.qkv_fuse_tiles = 8                # H / W attention inside the in_proj GEMM from this many (frame, group of 4 heads) entries per CU on (_qkv_fuse)
        self.mlp_fuse_tiles = 8                # c_fc + QuickGELU + c_proj in one launch from this many 128-row tiles per CU on (_mlp_fuse)
        self._derived = _Derived(self)

    def initialize_parameters(self):
        """mage_model.py:357-365."""
        proj_std = (self.model_channels ** -0.5) * ((2 * self.layers) ** -0.5)
        attn_std = self.model_channels ** -0.5
        fc_std = (2 * self.model_channels) ** -0.5
        for block in self.blocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)

    def build_casual_attention_mask(self):
        """Kept for API parity (mage_model.py:367-372); the GPU attention kernel applies j <= i directly."""
        mask = torch.empty(self.frames_length, self.frames_length)
        mask.fill_(float("-inf"))
        mask.triu_(1)
        return mask

    def _build(self):
        d: Dict[str, torch.Tensor] = {}
        _pack_linear(d, "in_linear", self.in_linear.weight, self.in_linear.bias)
        _pack_linear(d, "context_linear", self.context_linear.weight, self.context_linear.bias)
        if self.use_cids:
            _pack_linear(d, "out", self.out.weight, self.out.bias)
        else:                                  # MAGE+ head: GroupNorm(32) + SiLU + Conv3d 1x1x1 (mage_model.py:350-354)
            d["gn.w"], d["gn.b"] = self.out[0].weight.float().contiguous(), self.out[0].bias.float().contiguous()
            w = self.out[2].weight.float().reshape(self.out_channels, self.model_channels)
            n8 = (self.out_channels + 7) // 8 * 8                        # GEMM wants N % 8 == 0: zero rows pad the 4 outputs
            wp = torch.zeros(n8, self.model_channels, device=w.device)
            wp[:self.out_channels] = w
            bp = torch.zeros(n8, device=w.device)
            bp[:self.out_channels] = self.out[2].bias.float()
            _pack_linear(d, "out", wp, bp)
        d["tpos"] = self.T_positional_embedding.float().reshape(self.frames_length, self.model_channels).contiguous()
        for i, blk in enumerate(self.blocks):
            _pack_block(d, f"b{i}", blk)
            # LayerNorm folded into the Linear that follows it (bf16 path, see _fold): W' = gamma * W per input channel,
            # s_n = sum_k W'[n, k] (of the ROUNDED weights: what the MFMA multiplies), c_n = W beta + b
            for ln, lin in (("ln_1", "in_proj"), ("ln_2", "c_fc")):
                w, g, bt = d[f"b{i}.{lin}.f32"], d[f"b{i}.{ln}.w"], d[f"b{i}.{ln}.b"]
                wq = (w * g[None, :]).to(BF16)
                d[f"b{i}.{lin}.lnw"] = wq                   # (f16 mode: `.lnw.f16` / `.lns.f16`, built on first use by _ln_fold_w)
                d[f"b{i}.{lin}.lns"] = wq.float().sum(dim=1).contiguous()
                # c_n = sum_k W_nk beta_k + b_n in fp64 (a row-wise reduction: derived-cache bookkeeping, no BLAS call)
                d[f"b{i}.{lin}.lnc"] = ((w.double() * bt.double()[None, :]).sum(1) + d[f"b{i}.{lin}.b"].double()).float().contiguous()
            if i % 3 and self.model_channels % 128 == 0:        # H / W blocks: in_proj as the fused attention launch takes it (_qkv_fuse)
                self._qkv_fuse_pack(d, f"b{i}", d[f"b{i}.in_proj.lnw"], d[f"b{i}.in_proj.lns"], "")
        return d

    def _fold(self, dt, B: int, hw: int) -> bool:
        """bf16 path: the standalone LayerNorm launches between the GEMMs are folded into them (csrc/gemm.hip, epilogue_lean):
        the x + Linear(.) GEMM also writes a bf16 copy of x and per-row partial (sum, sum of squares); the next Linear takes that
        copy with gamma folded into its weights and finishes the normalisation in its epilogue.  Needs whole 256-row tiles per
        frame slot (so that the full pass and the incremental loop take the same route: their tokens stay bit-identical)."""
        return (dt in HALF_TYPES and (B * hw) % 256 == 0 and self.model_channels % 256 == 0 and config.get().ln_fold)

    def _stream_bf16(self) -> bool:
        """bf16 mode with the LayerNorm fold: x itself stays in bf16 between the blocks -- every x + Linear(.) reads the bf16 rows as its
        residual and writes bf16 rows (+ the LayerNorm partial sums of the fp32 values before rounding); no fp32 stream, no second copy:
        -0.8 GB of HBM traffic per x + Linear(.) launch at cfg2.  Measured against the fp32-stream form (`stream_bf16 = False` or
        config stream_16bit = False (MAGE_STREAM_FP32=1)): first-generated-frame token agreement with the fp32-class modes 0.956 vs 0.958 (16 clips), i.e. inside the
        bf16 GEMM noise.  The incremental loop uses the same kernels on the same rows: still bit-identical to the full loop."""
        return getattr(self, "stream_bf16", True) and config.get().stream_16bit

    def _ln_linear(self, d, p, lin, xn, xb, ln, y, *, M, N, sk=0, **kw):
        """y = Linear(LN(x)) for block p's in_proj / c_fc.  ln None: from xn, the output of a standalone layernorm (sk: split rows).
        Otherwise from the 16-bit rows xb, gamma folded into the weights and the normalisation finished in the epilogue; ln names the row
        statistics (ln_stats) or the producer's partial sums that the few-rows kernel reduces in its prologue (ln_part; _stats_inline)."""
        Cc, name = self.model_channels, f"{p}.{lin}"
        if ln is None:
            return _linear(xn, d, name, y, self.compute_dtype, M=M, N=N, K=Cc, sk=sk, **kw)
        lnw, lns = self._ln_fold_w(d, p, lin, xb.dtype)
        return ops.gemm(xb, lnw, y, M=M, N=N, K=Cc, lda=Cc, ldy=N, bias=d[name + ".lnc"], ln_colsum=lns, **ln, **kw)

    @staticmethod
    def _ln_fold_w(d, p, lin, dt):
        """(W' = gamma * W rounded to dt, s_n = the row sums of the ROUNDED W') of the LayerNorm fold (see _build): bf16 from _build, f16 on
        first use."""
        if dt == BF16:
            return d[f"{p}.{lin}.lnw"], d[f"{p}.{lin}.lns"]
        kw_, ks_ = f"{p}.{lin}.lnw.f16", f"{p}.{lin}.lns.f16"
        if kw_ not in d:
            ln = "ln_1" if lin == "in_proj" else "ln_2"
            wq = (d[f"{p}.{lin}.f32"] * d[f"{p}.{ln}.w"][None, :]).to(F16)
            d[kw_], d[ks_] = wq, wq.float().sum(dim=1).contiguous()
        return d[kw_], d[ks_]

    def _qkv_fuse(self, xb, M: int, hh: int, ww: int, stats_rows: bool, cache) -> bool:
        """The H / W blocks of a pass run their attention inside the in_proj GEMM, one launch per block (ops.gemm_attn_fused_qkv; q, k, v and the
        softmax numerators never reach memory): the 16-bit LayerNorm-fold path with (mean, rstd) rows, 16 x 16 frames (a 256-row GEMM tile is one
        frame), head width 32.  Its tile list has one entry per (frame, group of 4 heads); from qkv_fuse_tiles = eight entries per CU on (the full
        loop; the incremental step and small batches keep the QKV GEMM + attention pair -- both write the same bits).  The threshold is inherited
        from the two-launch form this launch replaced (four 256-column tiles per CU in its V launch: the same inequality, C being a multiple of 256);
        it is not measured against a lower one, and the launch has only been timed at the cfg2 full loop, 15 entries per CU.  use_cids=False keeps
        the old pair.  config qk_fuse = False (MAGE_NO_QK_FUSE=1) turns it off."""
        Cc = self.model_channels
        if not (stats_rows and cache is None and hh == 16 and ww == 16 and self.use_cids and config.get().qk_fuse):
            return False
        if Cc % 256 or not 256 <= Cc <= 1024 or M % 256 or (M + 8) * Cc * 2 >= 2 ** 32:
            return False
        return (M // 256) * (Cc // 128) >= getattr(self, "qkv_fuse_tiles", 8) * torch.cuda.get_device_properties(xb.device).multi_processor_count

    def _tqkv_fuse(self, xb, M: int, hw: int, P: int, p0: int, stats_rows: bool, cache) -> bool:
        """The temporal blocks of a pass take the same launch (ops.gemm_attn_fused_qkv, axis 0: a tile is 16 adjacent positions x the 16 slots of a
        clip, attention_mfma_kernel's causal select in the epilogue): _qkv_fuse's conditions without the 16 x 16 frame shape -- the 16-bit
        LayerNorm-fold path with (mean, rstd) rows, no cache, use_cids, the same widths and the same size rule qkv_fuse_tiles (a tile list of the
        same length) -- for a full window of exactly 16 slots (P == 16, p0 == 0) of hw % 16 == 0 rows each.  Every other window (the incremental
        loop, set_context's prefill, frames_length != 16, generation past L) keeps the QKV GEMM + attention pair, which writes the same bits.
        Timed at the cfg2 full loop only.  config tqkv_fuse = False (MAGE_NO_TQKV_FUSE=1) turns it off alone, qk_fuse = False with the H / W blocks'."""
        Cc, cfg = self.model_channels, config.get()
        if not (stats_rows and cache is None and P == 16 and p0 == 0 and hw % 16 == 0 and self.use_cids and cfg.qk_fuse and cfg.tqkv_fuse):
            return False
        if Cc % 256 or not 256 <= Cc <= 1024 or M % (16 * hw) or (M + 8) * Cc * 2 >= 2 ** 32 or (15 * hw + 16) * Cc * 2 + 16384 >= 2 ** 32:
            return False
        return (M // 256) * (Cc // 128) >= getattr(self, "qkv_fuse_tiles", 8) * torch.cuda.get_device_properties(xb.device).multi_processor_count

    def _mlp_fuse(self, xb, M: int, stats_rows: bool, sb: bool) -> bool:
        """The blocks of a pass run c_fc, QuickGELU and c_proj in ONE launch (ops.mlp_fused, csrc/gemm4m.hip: the hidden rows never reach memory): the
        16-bit LayerNorm-fold path with (mean, rstd) rows and the 16-bit stream, C = 512 (the width the kernel is built for), whole 128-row tiles,
        from mlp_fuse_tiles = eight tiles per CU on: the cfg2 full loop (262 144 rows: exactly eight on 256 CUs) qualifies, the incremental step's
        16 k rows (half a tile per CU) and small batches keep the two GEMMs -- both write the same bits.  Only the cfg2 full loop was timed
        (profiles/r20_mlp_fused.txt); no lower threshold, no other width and no f16 timing was measured.  use_cids=False (its head reads fp32 rows)
        keeps the pair.  config mlp_fuse = False (MAGE_NO_MLP_FUSE=1) turns it off."""
        if not (stats_rows and sb and self.use_cids and self.model_channels == 512 and config.get().mlp_fuse):
            return False
        if M % 128 or M * 512 >= 2 ** 31:
            return False
        return M // 128 >= getattr(self, "mlp_fuse_tiles", 8) * torch.cuda.get_device_properties(xb.device).multi_processor_count

    def _qkv_fuse_w(self, d, p, dt):
        """Block p's LayerNorm-folded in_proj operands (_ln_fold_w) as the fused launch takes them: all 3C rows in ops.qkv_pack_rows' order, with their colsum
        and bias.  bf16: from _build; f16: on first use."""
        sfx = ".f16" if dt == F16 else ""
        if f"{p}.in_proj.qkv.w{sfx}" not in d:
            lnw, lns = self._ln_fold_w(d, p, "in_proj", dt)
            self._qkv_fuse_pack(d, p, lnw, lns, sfx)
        q = f"{p}.in_proj.qkv."
        return dict(w=d[q + "w" + sfx], s=d[q + "s" + sfx], c=d[q + "c"])

    def _qkv_fuse_pack(self, d, p, lnw, lns, sfx: str) -> None:
        idx = ops.qkv_pack_rows(self.model_channels, lnw.device)
        d[f"{p}.in_proj.qkv.w{sfx}"], d[f"{p}.in_proj.qkv.s{sfx}"] = lnw[idx].contiguous(), lns[idx].contiguous()
        d[f"{p}.in_proj.qkv.c"] = d[f"{p}.in_proj.lnc"][idx].contiguous()       # (fp32: one copy serves both types)

    def _stats_inline(self, xb, M: int) -> bool:
        """One clip per call: every Linear that follows a LayerNorm (N = C .. 4C) runs on the few-rows kernel, which reduces the
        producer's partial sums itself (same arithmetic as mage_ln_stats, mage_ln_stats_row in csrc/common.h).  (The tiled kernels doing the
        same at the incremental loop's 16 k rows was measured in round 5: slower than the 7 us launch it removes.)"""
        Cc = self.model_channels
        return all(ops.gemm_is_small(xb, M, n, Cc) for n in (Cc, 2 * Cc, 3 * Cc, 4 * Cc))

    # ------------------------------------------------------------------ the two loops: one pass serves both, in every precision
    # A pass computes positions p0 .. p0+P-1 of the L slots: the motion anchor goes to slot 0 when the window starts there, the nf new
    # frames to the last nf slots of the window.  The reference's full-recompute loop is p0 = 0, P = L, nf = L-1 (_run); the incremental
    # loop appends one frame per step (_inc_step).  Both loops run the same body on the same per-row arithmetic, so their tokens are
    # bit-identical by construction.
    @torch.no_grad()
    def _run(self, motion: torch.Tensor, imgs: torch.Tensor, *, B: int, hh: int, ww: int) -> torch.Tensor:
        """motion [B*hw, Cc], imgs [B*(L-1)*hw, Ci] in the compute dtype -> logits [B*(L-1)*hw, K] fp32
        (use_cids=False: predicted latents [B*(L-1)*hw, 8] fp32 whose first out_channels columns are valid)."""
        L = self.frames_length
        return self._pass(motion, imgs, B=B, hh=hh, ww=ww, p0=0, P=L, nf=L - 1, cache=None)

    # the decoder is causal along L (temporal blocks masked, spatial blocks per frame), so the logits of
    # frame k do not depend on later slots.  Instead of recomputing all L positions in each of the L-1 iterations
    # (mage_model.py:673-684) only the NEW position(s) run through the stack; the temporal blocks keep their K,V of
    # earlier positions in a cache.
    def _inc_begin(self, B: int, hh: int, ww: int) -> dict:
        """State of one incremental decode: the next position, and the temporal blocks' caches (laid out by the pass of the first step)."""
        return {"B": B, "hh": hh, "ww": ww, "kv": {}, "p": 0}

    @torch.no_grad()
    def _inc_step(self, st: dict, motion: Optional[torch.Tensor], imgs: torch.Tensor, nf: int = 1) -> torch.Tensor:
        """Append position(s): the first call takes the motion anchor (slot 0) and frame 0's features (slot 1); later calls
        take the features of the newest frame only.  nf > 1 (MAGE.set_context's prefill): imgs holds nf given frames per clip, appended as
        one window.  Returns the logits of the last appended slot, [B*hw, K] fp32: the head runs on that slot only."""
        p0 = st["p"]
        P = nf + 1 if motion is not None else nf                            # new positions p0 .. p0+P-1
        # (the MAGE+ head's GroupNorm spans all frames of a clip: only the full loop is valid there)
        assert self.use_cids and nf >= 1 and (p0 == 0) == (motion is not None) and p0 + P <= self.frames_length
        logits = self._pass(motion, imgs, B=st["B"], hh=st["hh"], ww=st["ww"], p0=p0, P=P, nf=nf, nh=1, cache=st["kv"])
        st["p"] = p0 + P
        return logits

    def _axial_geo(self, axis: int, B: int, hh: int, ww: int, P: int, p0: int = 0, *, cached: bool = False,
                   q_cached: bool = False) -> dict:
        """Row map of the axial attention of a block attending along `axis` (0: L, causal; 1: H; 2: W -- :344,382) at positions
        p0 .. p0+P-1 of B clips of hh x ww frames, as keyword arguments of ops.attention / ops.attention_bwd.  Temporal blocks: q, K, V
        are the window's own rows [B, P, hh, ww] unless `cached`: K, V of positions 0 .. p0+P-1 then come from the [B, L, hh, ww] cache,
        and so does q with `q_cached` (the output keeps the window's row map)."""
        hw, H = hh * ww, self.model_channels // 32
        if axis == 1:
            return dict(n_seq=B * P * ww, inner=ww, nq=hh, nk=hh, q_outer_stride=hw, q_axis_stride=ww, causal=False,
                        kv_outer_stride=hw, kv_axis_stride=ww, n_head=H)
        if axis == 2:
            return dict(n_seq=B * P * hh, inner=1, nq=ww, nk=ww, q_outer_stride=ww, q_axis_stride=1, causal=False,
                        kv_outer_stride=ww, kv_axis_stride=1, n_head=H)
        kvo = (self.frames_length if cached else P) * hw
        geo = dict(n_seq=B * hw, inner=hw, nq=P, nk=p0 + P, q_outer_stride=kvo if q_cached else P * hw, q_axis_stride=hw, causal=True,
                   kv_outer_stride=kvo, kv_axis_stride=hw, n_head=H)
        if q_cached:
            geo.update(o_outer_stride=P * hw, o_axis_stride=hw)
        return geo

    def _embed(self, d, x, motion, imgs, *, B: int, hw: int, P: int, nf: int, tp: torch.Tensor) -> None:
        """The window's input rows of x [B*P*hw, C] (:375-378, no concat copy): context_linear(motion) -> slot 0 (if motion), in_linear
        (frames) -> the last nf slots, + the window's T positions tp.  imgs: rows in the compute dtype, or FrameTokens.  Split modes: both
        products take split operands only as the padded-taps form of the split GEMM (_taps_ok), else the fp32 chain: motion is fp32 rows,
        split on the way in; imgs are split rows (_frame_features) where that form runs and fp32 rows where it does not."""
        dt, Cc, sk = self.compute_dtype, self.model_channels, self._sk()
        if motion is not None:
            _linear(motion, d, "context_linear", x, dt, M=B * hw, N=Cc, K=self.context_channels, sk=sk if sk and self._taps_ok(B * hw) else 0,
                    out_w=hw, y_img_stride=P * hw, rowadd=tp, rowadd_div=hw, rowadd_mod=P)
        off = (P - nf) * hw
        if isinstance(imgs, FrameTokens):
            imgs.fill(x, n_img=B * nf, per_clip=nf, P=P, y_off=off, tp=tp)
        else:
            _linear(imgs, d, "in_linear", x, dt, M=B * nf * hw, N=Cc, K=self.in_channels, sk=sk if imgs.dtype != dt else 0, out_w=nf * hw,
                    y_img_stride=P * hw, y_off=off, rowadd=tp, rowadd_div=hw, rowadd_mod=P)

    def _head(self, d, xa, *, B: int, hw: int, P: int, nf: int) -> torch.Tensor:
        """The head on the window's last nf slots (:385), reading the last block's output xa: logits [B*nf*hw, K] fp32 from rows in the
        compute dtype (split modes: split rows); use_cids=False: predicted latents [B*nf*hw, 8] fp32 (first out_channels columns valid) from
        fp32 rows, on the compute dtype's chain in every mode."""
        dt, Cc, rows = self.compute_dtype, self.model_channels, B * nf * hw
        if not self.use_cids:
            # MAGE+: GroupNorm + SiLU + Conv3d 1x1x1 (:350-354); the GroupNorm statistics span all frames of a clip (:387-388): NOT causal along L
            y = ops.groupnorm_silu(xa, d["gn.w"], d["gn.b"], torch.empty(rows, Cc, device=xa.device, dtype=dt), n_samples=B,
                                   rows_per_sample=nf * hw, sample_stride_rows=P * hw, row_off=(P - nf) * hw, groups=32, eps=self.out[0].eps)
            n8 = d["out.f32"].shape[0]
            return _linear(y, d, "out", torch.empty(rows, n8, device=xa.device, dtype=F32), dt, M=rows, N=n8, K=Cc)
        logits = torch.empty(rows, self.out_channels, device=xa.device, dtype=F32)
        return _linear(xa, d, "out", logits, dt, M=rows, N=self.out_channels, K=Cc, sk=self._sk(), out_w=nf * hw, a_img_stride=P * hw,
                       a_off=(P - nf) * hw)

    def _pass(self, motion, imgs, *, B: int, hh: int, ww: int, p0: int, P: int, nf: int, cache: Optional[dict],
              nh: Optional[int] = None) -> torch.Tensor:
        """One window (see above) through the stack, in every precision.  cache (incremental loop): block -> the temporal block's rows of
        all L slots, [B, L, hw, q|k|v] (split modes: [B, L, hw, K|V]).  nf frames are embedded into the window's last nf slots; the head
        runs on the last nh of them (None: all nf)."""
        d = self._derived.get(self._build)
        dt, Cc, L = self.compute_dtype, self.model_channels, self.frames_length
        dev = (imgs.tokens if isinstance(imgs, FrameTokens) else imgs).device
        hw = hh * ww
        M = B * P * hw
        # The form of the Linear layers' operand rows, decided once per pass; the block loop below is the same for all three.
        #   plain (fp32; 16-bit where the fold does not apply): rows in the compute dtype, written by a standalone layernorm of the fp32
        #     rows x into xn (ln None), by the attention and by the c_fc epilogue.
        #   split (sk: 'bf16x3' / 'f16x3'): plain with fp32 everywhere EXCEPT those rows, which their producers write as split-precision
        #     rows (two 16-bit pieces per element, ops.split_empty) and the Linear layers multiply as three 16-bit MFMA products per K slab
        #     (include/mage_hip.h).  qs (f16x3, _attn_split): q, k, v leave the QKV epilogue as split rows too, attention on the matrix cores.
        #   fold (16-bit, _fold): no standalone layernorm.  Every x + Linear(.) (res) also leaves per-row partial sums `part` and the 16-bit
        #     rows xb, and the Linear normalises xb itself (_ln_linear): from (mean, rstd) rows `stats` that an ln_stats launch reduces from
        #     `part`, or, on the few-rows kernel (inl), from `part` directly.  Block 0's in_proj (ln0) follows the fill: the statistics of
        #     one row_stats pass over the 16-bit stream (sb), else a layernorm of the fp32 rows.
        sk = self._sk()
        qs = bool(sk) and self._attn_split()
        cw = 2 * Cc if qs else Cc                       # elements per row of each of q, k, v (split rows: 2 per logical column)
        fold = not sk and self._fold(dt, B, hw)
        sb = fold and self._stream_bf16()
        xb = part = stats = None
        if fold:
            xb = torch.empty(M, Cc, device=dev, dtype=dt)                          # the 16-bit stream (or the 16-bit copy of the fp32 one)
            part = torch.empty(Cc // 64, M, 2, device=dev, dtype=F32)       # slice-major (mage_gemm_desc::ln_part_rows)
            stats = torch.empty(M, 2, device=dev, dtype=F32)
        inl = fold and self._stats_inline(xb, M)
        ln = None if not fold else dict(ln_part=part, ln_eps=1e-5) if inl else dict(ln_stats=stats)
        ln0 = dict(ln_stats=stats) if sb else None
        x = xb if sb else torch.empty(M, Cc, device=dev, dtype=F32)                # the residual stream
        res = dict(residual=x, ldr=Cc)                  # every x + Linear(.) but the last: in place on the stream
        if fold:                                        # ... leaving the partial sums (and, fp32 stream, the 16-bit copy xb)
            res["ln_part"] = part
            if not sb:
                res.update(y2=xb, ldy2=Cc)
        self._embed(d, x, motion, imgs, B=B, hw=hw, P=P, nf=nf, tp=d["tpos"][p0:])
        if sb:
            ops.row_stats(xb, 1e-5, stats)

        def rows(n, split=bool(sk), m=M):
            """m operand rows of n columns: split rows in the split modes (or where `split` says), else rows in the compute dtype."""
            return ops.split_empty(m, n, sk, dev) if split else torch.empty(m, n, device=dev, dtype=dt)

        geo = [self._axial_geo(a, B, hh, ww, P, p0, cached=cache is not None, q_cached=cache is not None and not sk) for a in range(3)]
        fuse = not sk and self._qkv_fuse(xb, M, hh, ww, fold and not inl, cache)
        tfuse = not sk and self._tqkv_fuse(xb, M, hw, P, p0, fold and not inl, cache)
        # per block: its attention runs inside its in_proj launch (a temporal block 0 needs the fill's statistics rows, ln0)
        fused = [(fuse if i % 3 else tfuse and (i > 0 or ln0 is not None)) for i in range(self.layers)]
        xn, ao = rows(Cc), rows(Cc)
        qkv = None if all(fused) else rows(3 * Cc, qs)      # (every block fused: q, k and v are stored nowhere)
        mfuse = not sk and self._mlp_fuse(xb, M, fold and not inl, sb)
        hdn = None if mfuse else rows(4 * Cc)
        for i in range(self.layers):
            p = f"b{i}"
            ln1 = ln if i else ln0
            if ln1 is None:
                ops.layernorm(x, d[p + ".ln_1.w"], d[p + ".ln_1.b"], xn, 1e-5, split_kind=sk)
            if fused[i]:
                # the attention inside the in_proj GEMM's epilogues (csrc/gemm4.hip, QF): per (row tile, group of 4 heads) a Q K tile that keeps
                # the softmax numerators in registers, then a V tile that finishes P V -- the same bits in ao as the QKV GEMM + ops.attention
                # below, q, k and v never stored.  H / W blocks: a tile is a frame; temporal blocks: 16 positions x the clip's 16 slots, causal
                f = self._qkv_fuse_w(d, p, dt)
                ops.gemm_attn_fused_qkv(xb, f["w"], ao, axis=i % 3, M=M, C_=Cc, K=Cc, lda=Cc, ldy=Cc, bias=f["c"], ln_stats=stats, ln_colsum=f["s"],
                                        out_w=None if i % 3 else hw)
            elif i % 3 == 0 and cache is not None and not sk:
                # one row [q | k | v] per (clip, slot, pixel): the new positions' QKV projection is ONE launch writing straight into their
                # slots, and the attention reads q back from there (1.5x the K,V bytes of a cache that is 0.8 GB at cfg2)
                if p0 == 0:
                    cache[i] = rows(3 * Cc, m=B * L * hw)
                kv = cache[i]
                self._ln_linear(d, p, "in_proj", xn, xb, ln1, kv, M=M, N=3 * Cc, out_w=P * hw, y_img_stride=L * hw, y_off=p0 * hw)
                q, k, v = kv[p0 * hw:], kv[:, cw:], kv[:, 2 * cw:]
            elif i % 3 == 0 and cache is not None:
                # the split modes' layout: one row [K | V] per (clip, slot, pixel), fp32 or (qs) split rows; q of the new positions stays
                # packed [M, C] in qkv; two launches
                if p0 == 0:
                    cache[i] = rows(2 * Cc, qs, B * L * hw)
                k = cache[i]
                q, v = qkv.view(-1)[:M * cw].view(M, cw), k[:, cw:]
                _linear(xn, d, p + ".in_proj", q, dt, M=M, N=Cc, K=Cc, sk=sk, lo=0, hi=Cc)
                _linear(xn, d, p + ".in_proj", k, dt, M=M, N=2 * Cc, K=Cc, sk=sk, lo=Cc, hi=3 * Cc, out_w=P * hw, y_img_stride=L * hw,
                        y_off=p0 * hw)
            else:
                q, k, v = qkv, qkv[:, cw:], qkv[:, 2 * cw:]
                self._ln_linear(d, p, "in_proj", xn, xb, ln1, qkv, M=M, N=3 * Cc, sk=sk)
            if not fused[i]:
                ops.attention(q, k, v, ao, ldq=q.stride(0), ldk=k.stride(0), ldv=v.stride(0), ldo=ao.stride(0), out_split=sk,
                              split_kind=sk if qs else 0, **geo[i % 3])
            _linear(ao, d, p + ".out_proj", x, dt, M=M, N=Cc, K=Cc, sk=sk, **res)
            if fold and not inl:
                ops.ln_stats(part, Cc, 1e-5, stats)
            if ln is None:
                ops.layernorm(x, d[p + ".ln_2.w"], d[p + ".ln_2.b"], xn, 1e-5, split_kind=sk)
            if mfuse:
                # c_fc, QuickGELU and c_proj in one launch: a 128-row tile keeps its hidden rows on the CU (csrc/gemm4m.hip) -- the same bits in x
                # and part as the two GEMMs below.  The last block writes the head's 16-bit rows xn, no partial sums.
                lnw, lns = self._ln_fold_w(d, p, "c_fc", dt)
                last = i == self.layers - 1
                ops.mlp_fused(xb, xn if last else xb, M=M, C_=Cc, w1=lnw, c1=d[p + ".c_fc.lnc"], s1=lns, ln_stats=stats,
                              w2=_wdt(d, p + ".c_proj", dt), b2=d[p + ".c_proj.b"], ln_part=None if last else part)
                if last:
                    xa = xn
                else:
                    ops.ln_stats(part, Cc, 1e-5, stats)
                continue
            self._ln_linear(d, p, "c_fc", xn, xb, ln, hdn, M=M, N=4 * Cc, sk=sk, act=ops.ACT_QUICKGELU)
            if i < self.layers - 1:
                _linear(hdn, d, p + ".c_proj", x, dt, M=M, N=Cc, K=4 * Cc, sk=sk, **res)
                if fold and not inl:
                    ops.ln_stats(part, Cc, 1e-5, stats)
            else:
                # the last x + c_proj(.) is only read by the head.  Logits head on 16-bit or split rows: the epilogue writes them as such
                # (16-bit: same fp32 sum, same round-to-nearest-even as a separate cast pass: bit-identical) instead of writing fp32 rows and
                # converting them in another launch.  MAGE+ head: its GroupNorm reads fp32 rows (fresh ones behind the 16-bit stream).
                if self.use_cids and (sk or dt != F32):
                    xa = xn
                else:
                    xa = torch.empty(M, Cc, device=dev, dtype=F32) if sb else x
                _linear(hdn, d, p + ".c_proj", xa, dt, M=M, N=Cc, K=4 * Cc, sk=sk, residual=x, ldr=Cc)
        return self._head(d, xa, B=B, hw=hw, P=P, nf=nf if nh is None else nh)

    # ------------------------------------------------------------------ the fast parity modes ('f16x3' / 'bf16x3'): what selects _pass's split form
    # Residual stream, q / k / v (bf16x3), softmax and logits are fp32 as in 'fp32' mode; only the operands of the Linear layers differ (_linear).
    def _split_on(self) -> bool:
        return bool(self.split_kind) and self.compute_dtype == F32 and self.model_channels % 64 == 0

    def _sk(self) -> int:
        """The split kind that the passes run on: split_kind in the fast parity modes, else 0."""
        return self.split_kind if self._split_on() else 0

    def _warm_split(self) -> None:
        """Build every split-precision weight copy now (MAGE._warm_derived: on the caller's stream, before side streams fork)."""
        if not self._split_on():
            return
        d = self._derived.get(self._build)
        names = ["in_linear", "context_linear"] + (["out"] if self.use_cids else [])
        for i in range(self.layers):
            names += [f"b{i}.in_proj", f"b{i}.out_proj", f"b{i}.c_fc", f"b{i}.c_proj"]
        for n in names:
            _wsplit(d, n, self.split_kind)

    def _attn_split(self) -> bool:
        """f16x3: the axial attentions read split q, k, v on the matrix cores (attention_mfma_kernel over the f16x3 operand policy); sequences up to 32."""
        return (self.split_kind == ops.F16X3 and self.frames_length <= 32 and (self.model_channels // 32) % 2 == 0
                and config.get().attn_split)

    def _taps_ok(self, rows: int) -> bool:
        """in_linear / context_linear (+ T positions) and the frame convolution run as the padded-taps form of the split GEMM."""
        return self.model_channels % 256 == 0 and rows % 256 == 0 and self.in_channels % 64 == 0 and self.context_channels % 64 == 0

    def forward(self, motion: torch.Tensor, imgs: torch.Tensor) -> torch.Tensor:
        """motion [B,H,W,Cc], imgs [B,L-1,H,W,Ci] -> logits [B,L-1,H,W,out] fp32."""
        _need_gpu(motion, "FlatAxialDecoder")
        B, hh, ww, _ = motion.shape
        dt = self.compute_dtype
        m = motion.reshape(B * hh * ww, -1).to(dt).contiguous()
        im = imgs.reshape(-1, imgs.shape[-1]).to(dt).contiguous()
        out = self._run(m, im, B=B, hh=hh, ww=ww)
        return out.view(B, self.frames_length - 1, hh, ww, -1)[..., :self.out_channels]


class PIDControl:
    """KL-weight PI controller (mage_model.py:394-434); host-side scalar bookkeeping, training only."""

    def __init__(self):
        self.I_k1 = 0.0
        self.W_k1 = 0.0
        self.e_k1 = 0.0

    def _Kp_fun(self, Err, scale=1):
        return 1.0 / (1.0 + float(scale) * exp(Err))

    def pid(self, exp_KL, KL_loss, Kp=0.01, Ki=-0.0001, Kd=0.0):
        error_k = exp_KL - KL_loss
        Pk = Kp * self._Kp_fun(error_k)
        Ik = self.I_k1 + Ki * error_k
        if self.W_k1 < 0 and self.W_k1 >= 1:      # (sic) never true in the reference either
            Ik = self.I_k1
        Wk = Pk + Ik
        self.W_k1, self.I_k1, self.e_k1 = Wk, Ik, error_k
        return min(max(Wk, 0.0), 1.0), error_k


def disabled_train(self, mode=True):
    return self


class _Generation:
    """What is fixed for one MAGE._generate_one call, and the per-frame step both AR loops share.  B = Bc * N: the clips (x candidates)
    whose tokens are picked; Bd: the decoder's batch -- under guidance 2 B, rows B .. 2 B the uncond half, fed the tokens of the cond half.
    Every pick / logprob / stats / known-token launch addresses the first B clips only, in the ops functions' own terms: a group is one
    clip's frame (hw rows), in_group_stride / in_off find its logits rows, tok_group_stride / tok_off its token slot, and `sel` takes the
    launch's view of a result buffer, indexed like the tokens."""

    def __init__(self, model: "MAGE", images, Bc: int, N: int, k: int, tok0, ctx, ma, seeds, gs, kn, lp, st):
        self.model, self.images, self.Bc, self.N, self.k = model, images, Bc, N, k            # k: the given frames (set_context)
        self.tok0, self.ctx, self.ma = tok0, ctx, ma     # int64 [Bd, hw] frame 0, [Bd, k, hw] the given frames; the anchor's rows [Bd * hw, C]
        self.seeds, self.gs, self.kn = seeds, gs, kn     # int64 [B] (None: greedy); fp32 [Bc] (None: no guidance); int64 [Bc, (L-1) * hw] (None)
        self.B = Bc * N
        self.Bd = self.B * (1 if gs is None else 2)
        self.hw, self.Lm1, self.K = model.image_resolution ** 2, model.frames_length - 1, model.codebook_size
        self.lp, self.st = lp, st                        # the result buffers (None: off): fp32 token log-probabilities, _stats_alloc's dict

    def guide(self, logits, frames: int = 1, **at) -> None:
        """Guidance on: `frames` frames of the first B clips, in place on the cond half's rows of the decoder's [cond | uncond] logits; one
        scale per clip covers its N candidates.  at: group / in_group_stride / in_off."""
        if self.gs is not None:
            ops.guide_logits(logits, logits[logits.shape[0] // 2:], self.gs, rows=self.B * frames * self.hw, K=self.K,
                             scale_div=self.N * frames * self.hw, **at)

    def pick(self, logits, tokens, sel, *, rows: int, pos_off: int = 0, scored: bool = True, tok_group_stride=None, tok_off: int = 0, **inp) -> None:
        """Tokens of `rows` logits rows (inp: group / in_group_stride / in_off) into their slots -- the sampler under the candidates' seeds,
        or argmax -- then (scored) the log-probabilities and statistics of the tokens just picked, under the logits they came from."""
        out = dict(rows=rows, K=self.K, out_group_stride=tok_group_stride, out_off=tok_off, **inp)
        if self.seeds is None:
            ops.argmax(logits, tokens, **out)
        else:
            t, k, p = self.model.sampling
            ops.sample_tokens(logits, tokens, self.seeds, temperature=t, top_k=k, top_p=p, pos_off=pos_off, **out)
        at = dict(rows=rows, K=self.K, tok_group_stride=tok_group_stride, tok_off=tok_off, **inp)
        if scored and self.lp is not None:
            ops.token_logprob(logits, tokens, sel(self.lp), **at)
        if scored and self.st is not None:
            self.model._stats(logits, tokens, self.st, sel, **at)

    def hold(self, tokens, sel, rows: int, **at) -> None:
        """Tokens given: one launch stores them over the picked ones, and the certain policy's 0 / 0 / 1 over their results (sel None: the
        tokens alone); a clip's N candidates share its row of kn.  at: group / tok_group_stride / tok_off / known_off."""
        if self.kn is not None:
            res = {} if sel is None else {n: sel(b) for n, b in (("logprob", self.lp), *(self.st or {}).items()) if b is not None}
            ops.apply_known_tokens(tokens, self.kn, rows=rows, K=self.K, known_group_stride=self.Lm1 * self.hw, known_clip_div=self.N, **res, **at)

    def frame(self, i: int, logits, tokens, sel, *, in_group_stride: int, in_off: int = 0, tok_group_stride: int, tok_off: int = 0,
              slot=None, scored: bool = True) -> None:
        """Frame i of every clip: guide its logits, pick its tokens (position i * hw + pixel of the clip's sampler stream), score them
        (scored False: the results are filled later), store the given tokens over them, and copy the slot ([Bd, hw]; None: nothing reads
        it) to the uncond half, which conditions on the same tokens (one small int64 copy per frame)."""
        hw, rows = self.hw, self.B * self.hw
        self.guide(logits, group=hw, in_group_stride=in_group_stride, in_off=in_off)
        self.pick(logits, tokens, sel, rows=rows, pos_off=i * hw, scored=scored, group=hw, in_group_stride=in_group_stride, in_off=in_off,
                  tok_group_stride=tok_group_stride, tok_off=tok_off)
        self.hold(tokens, sel if scored else None, rows, group=hw, tok_group_stride=tok_group_stride, tok_off=tok_off, known_off=i * hw)
        if self.gs is not None and slot is not None:
            slot[self.B:].copy_(slot[:self.B])


class MAGE(nn.Module):
    def __init__(self, first_stage_config, text_encoder_config, ma_config, generate_decoder_config, codebook_size: int,
                 frames_length: int, image_resolution: int, vision_width: int, dropout: float = 0.1, use_cids=False,
                 randomness=False, alpha=0., beta=1., v_kl=0., auto_beta=False):
        super().__init__()
        self.instantiate_first_stage(first_stage_config)
        self.frames_length, self.image_resolution, self.vision_width = frames_length, image_resolution, vision_width
        self.dropout, self.use_cids, self.auto_beta = dropout, use_cids, auto_beta
        self.text_encoder = instantiate_from_config(text_encoder_config)
        self.ma_encoder = instantiate_from_config(ma_config, {"dropout": dropout})
        # The reference ships ONE TransformerBlock.forward with two alternative first lines (mage_model.py:92-93) and tells the
        # user to swap them by hand for MAGE+.  MAGE+ is exactly the use_cids=False family (config/mage+_*.yaml), so the variant
        # follows that switch; `model.ma_encoder.mage_plus = False` restores the shipped line for a MAGE+ config.
        if hasattr(self.ma_encoder, "mage_plus"):
            self.ma_encoder.mage_plus = not use_cids
        self.generate_model = instantiate_from_config(
            generate_decoder_config, {"use_cids": use_cids, "dropout": dropout, "context_channels": ma_config["params"]["d_model"]})
        self.codebook_size = codebook_size
        if use_cids:
            self.visual_token_embedding = nn.Embedding(codebook_size, vision_width)
        else:
            self.visual_token_embedding = nn.Linear(self.first_stage_model.embed_dim, vision_width)
        self.conv = nn.Sequential(nn.Conv2d(vision_width, vision_width, kernel_size=3, stride=1, padding=1, bias=False))
        scale = vision_width ** -0.5
        self.speed_embedding = nn.Parameter(scale * torch.randn(1, vision_width))
        self.H_positional_embedding = nn.Parameter(scale * torch.randn(1, image_resolution, 1, vision_width))
        self.W_positional_embedding = nn.Parameter(scale * torch.randn(1, 1, image_resolution, vision_width))
        self.randomness = randomness
        if randomness:
            dm = ma_config["params"]["d_model"]
            self.conv3d = nn.Sequential(*[BasicBlock(vision_width, vision_width if i < 3 else dm, stride=1, stride_t=2,
                                                     downsample=True) for i in range(4)])
            self.conv_mu2 = nn.Conv2d(vision_width, 64, 3, 1, 1)
            self.conv_var2 = nn.Conv2d(vision_width, 64, 3, 1, 1)
            self.conv_d2 = nn.Conv2d(64, vision_width, kernel_size=3, stride=1, padding=1, bias=False)
            self.adain = ADAIN2D(vision_width, vision_width)
            if auto_beta:
                self.PID = PIDControl()
                self.KL_loss = v_kl
            else:
                self.alpha, self.beta = alpha, beta
        self.initialize_parameters()
        self.precision = "fp32"
        self.streams = 1               # >1: clip groups on concurrent HIP streams (see autoregressive_generate)
        self.ar_mode = "full"          # 'full' = the reference's per-iteration full recompute (mage_model.py:673-684);
                                       # 'incremental' = temporal KV cache, each position once
        self.last_call_mode = "eager"
        self._pad_frames: dict = {}    # zero-padded frame buffers of _frame_features (bf16 mode), by (images, device, stream)
        self.use_graph = None          # True: autoregressive_generate replays a captured HIP graph of the whole call (see _generate_graphed);
                                       # None (default): only where the call is launch-bound -- a few clips per call (_graph_auto); False: never
        self.frame_table = True        # conv3x3(token embedding) (+ in_linear) as a table sum (_frame_tables); False: the convolution GEMM
        self._graphs: dict = {}
        self._derived = _Derived(self)
        self.last_tokens: Optional[torch.Tensor] = None
        self.last_logits: Optional[torch.Tensor] = None           # full AR mode: fp32 [B, L-1, h, w, K], the last iteration's logits
        self.sampling: Optional[Tuple[float, int, float]] = None   # (temperature, top_k, top_p) of set_sampling; None: greedy (the reference)
        self.last_sample_seeds: Optional[torch.Tensor] = None     # the per-clip seeds of the last sampled call
        self.logprobs = False          # set_logprobs: autoregressive_generate also leaves the log-probabilities of the tokens it generated
        self.candidates = 1            # set_sampling(candidates=N): N sampled candidates per clip, the most likely one kept
        self.last_token_logprobs: Optional[torch.Tensor] = None   # fp32 [B, L-1, h, w] (set_logprobs, candidates > 1, score)
        self.last_clip_logprob: Optional[torch.Tensor] = None     # fp32 [B]: their per-clip totals
        self.last_candidate_scores: Optional[torch.Tensor] = None  # candidates > 1: fp32 [B, N], every candidate's total
        self.last_candidate_index: Optional[torch.Tensor] = None   # candidates > 1: int64 [B], the candidate kept
        self.logprob_policy = False    # set_logprobs(policy=True): the same under the sampler's own filtered distribution (mage_token_stats)
        self.logprob_entropy = False   # set_logprobs(entropy=True): per-token entropies
        self.last_token_policy_logprobs: Optional[torch.Tensor] = None   # policy: fp32 [B, L-1, h, w], -inf where the sampler could not draw the token
        self.last_clip_policy_logprob: Optional[torch.Tensor] = None     # policy: fp32 [B], their per-clip totals
        self.last_token_kept: Optional[torch.Tensor] = None              # policy: int32 [B, L-1, h, w], the size of the set the sampler drew from
        self.last_candidate_policy_scores: Optional[torch.Tensor] = None  # policy, candidates > 1: fp32 [B, N]
        self.last_token_entropy: Optional[torch.Tensor] = None           # entropy: fp32 [B, L-1, h, w], the full softmax at temperature 1 (nats)
        self.last_token_policy_entropy: Optional[torch.Tensor] = None    # entropy, sampling on: the filtered distribution's
        self.last_policy_token_logprobs: Optional[torch.Tensor] = None   # policy_loss: fp32 [B, L-1, h, w], the given tokens under the current policy
        self.last_policy_token_kl: Optional[torch.Tensor] = None         # policy_loss with a reference: fp32 [B, L-1, h, w], the k3 KL estimates
        self.last_policy_group_logratio: Optional[torch.Tensor] = None   # policy_loss(ratio='frame' | 'clip'): fp32 [B, L-1] | [B], the groups' mean log-ratios
        self.last_video_noise: Optional[torch.Tensor] = None             # randomness: fp32 [B, 64, h, w], the noise the last generation used
        self.last_preference_clip_logprobs: Optional[torch.Tensor] = None    # preference_loss: fp32 [B], the clips' log-likelihoods under the model
        self.last_preference_clip_coef: Optional[torch.Tensor] = None        # fp32 [B]: d(loss) / d(clip log-likelihood)
        self.last_preference_pair_loss: Optional[torch.Tensor] = None        # fp32 [P]
        self.last_preference_pair_margin: Optional[torch.Tensor] = None      # fp32 [P]: beta * ((s_w - r_w) - (s_l - r_l))
        self.last_preference_token_logprobs: Optional[torch.Tensor] = None   # fp32 [B, L-1, h, w]: the given tokens at temperature 1, no filter
        self.last_distill_token_kl: Optional[torch.Tensor] = None        # distill_loss: fp32 [B, L-1, h, w], every token's KL against the teacher
        self._last_head_out = None                                       # mage_train.MageLossFn -> _run_head: (loss dict, what the head saved)
        self.guidance: Optional[float] = None                            # set_guidance: the classifier-free guidance scale; None: off
        self.last_guidance_scale: Optional[torch.Tensor] = None          # guidance on: fp32 [B], the per-clip scales the last generation used
        self.context_frames = 1        # set_context: frames 0 .. k-1 of batch['images'] are given; 1: only frame 0 (off)
        self.context_prefill = True    # incremental mode: the given frames enter as ONE window; False: one position at a time, no pick
        self.last_known_mask: Optional[torch.Tensor] = None              # bool [B, L-1, h, w]: the slots the last generation was given
        self.loss_options: Optional[dict] = None                         # set_loss: forward's supervised-loss options; None: the plain cross entropy
        self.caption_dropout = 0.0     # forward in training mode: the probability that a clip's caption is replaced by the null caption
        self.last_caption_drop: Optional[torch.Tensor] = None            # bool [B]: the clips whose caption the last forward dropped

    # ------------------------------------------------------------------ construction helpers
    def instantiate_first_stage(self, config):
        """Frozen, eval, train() disabled (mage_model.py:516-521)."""
        model = instantiate_from_config(config)
        self.first_stage_model = model.eval()
        self.first_stage_model.train = disabled_train.__get__(self.first_stage_model)
        for p in self.first_stage_model.parameters():
            p.requires_grad = False

    def initialize_parameters(self):
        nn.init.normal_(self.visual_token_embedding.weight, std=0.02)            # mage_model.py:524

    def set_precision(self, precision: str) -> "MAGE":
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.precision = precision
        self.generate_model.compute_dtype, self.generate_model.split_kind = PRECISIONS[precision]
        # the once-per-clip prologue: exact-fp32 MFMA chains only in 'fp32' mode, f16x3 split operands otherwise (_linear)
        self.ma_encoder.split_kind = self.text_encoder.split_kind = 0 if precision == "fp32" else ops.F16X3
        if hasattr(self.first_stage_model, "set_precision"):     # an external latent first stage (MAGE+) has no such switch
            self.first_stage_model.set_precision(precision)
        return self

    def set_sampling(self, temperature: Optional[float] = 1.0, top_k: int = 0, top_p: float = 1.0, candidates: int = 1) -> "MAGE":
        """Seeded stochastic decoding of the VQ tokens in autoregressive_generate: temperature, top-k (0: off), top-p (1: off), one seed per
        clip (batch['sample_seed'], int64 [B]; drawn from torch's default CPU generator when absent).  The rule is mage_sample_tokens'
        (include/mage_hip.h); top_k = 1 is greedy.  set_sampling(None): greedy argmax, the reference's decoding (the default).
        candidates = N > 1: every clip is drawn N times behind ONE prologue (candidate c with seed sample_seed + c, int64 wrap-around; candidate
        0 is the candidates = 1 result) and only the candidate with the largest log-probability (unfiltered softmax, temperature 1) is decoded:
        last_tokens / last_token_logprobs / last_clip_logprob are the winner's, last_candidate_scores [B, N] and last_candidate_index [B]
        tell the rest."""
        if isinstance(candidates, bool) or int(candidates) != candidates or candidates < 1:
            raise ValueError(f"set_sampling: candidates must be an integer >= 1, got {candidates}")
        if temperature is None:
            if candidates > 1:
                raise ValueError("set_sampling: candidates > 1 needs sampling on (greedy candidates would all be the same clip)")
            self.sampling, self.candidates = None, 1
            return self
        if not self.use_cids:
            raise ValueError("set_sampling: a use_cids=False (MAGE+) model regresses continuous latents; it has no tokens to sample")
        t, k, p = float(temperature), int(top_k), float(top_p)
        t32 = ctypes.c_float(t).value if math.isfinite(t) and abs(t) < 3e38 else math.inf     # the library takes it as fp32
        if not (math.isfinite(t32) and t32 > 0 and 1.0 / t32 < 3.4e38):
            raise ValueError(f"set_sampling: temperature must be finite and > 0 (in fp32, and so must 1 / temperature), got {temperature}")
        if int(top_k) != top_k or not 0 <= k <= self.codebook_size:
            raise ValueError(f"set_sampling: top_k must be an integer in [0, {self.codebook_size}], got {top_k}")
        if not 0.0 < p <= 1.0:
            raise ValueError(f"set_sampling: top_p must be in (0, 1], got {top_p}")
        self.sampling, self.candidates = (t, k, p), int(candidates)
        return self

    def set_guidance(self, scale: Optional[float] = None) -> "MAGE":
        """Classifier-free guidance of autoregressive_generate: how strongly the caption steers the video.  scale None (the default): off,
        every call is the unguided one.  Otherwise a float that is finite in fp32; any finite value is legal -- 1 is "no guidance, at twice
        the cost", values above 1 push towards the caption, values below 1 (negative ones too) away from it.
        The caption reaches the decoder only through the motion anchor, so a guided call is the same decoder over 2 B clips -- the B clips
        under batch['text'], then the same clips under the negative caption, both halves fed the same tokens -- and every position's two
        logit rows are combined before its token is picked: z = c + (scale - 1)(c - u) (mage_guide_logits, include/mage_hip_ext.h: scale 1,
        and a negative caption equal to the caption, return the unguided logits bit for bit).  Everything downstream sees the guided logits:
        argmax or the sampler, best-of-N (set_sampling(candidates=N)), graph replay, both AR modes, last_logits, and set_logprobs'
        results -- last_token_logprobs is the softmax of the GUIDED logits at temperature 1, last_token_policy_logprobs the sampler's
        filtered view of the same guided logits.  Every result has B clips.
        batch['guidance_scale'] (fp32 [B], optional) overrides the float per clip: a tensor, so a captured graph replays under new scales;
        last_guidance_scale keeps what the call used.  batch['negative_text'] (int64, the shape of batch['text'], optional) is the caption
        steered away from; absent, it is mage_amd.utils.glue.null_caption(text, padding_idx) -- [CLS] [SEP] and padding -- which
        caption_dropout teaches a model fine-tuned here.  Both keys are ignored while guidance is off.  On a randomness=True model clip b's
        negative half uses clip b's noise and speed.
        While guidance is on, score, policy_loss, token_policy_logprobs and rollout are refused: a guided behaviour policy against an
        unguided learner is a different estimator.  distill_targets is the one pass over given tokens that runs guided: it returns the guided
        logits themselves, for a student's distill_loss."""
        if scale is None:
            self.guidance = None
            return self
        if not self.use_cids:
            raise ValueError("set_guidance: a use_cids=False (MAGE+) model regresses continuous latents; it has no tokens to sample")
        if isinstance(scale, bool) or not isinstance(scale, (int, float)):
            raise ValueError(f"set_guidance: scale must be a float or None, got {scale!r}")
        s = float(scale)
        if not (math.isfinite(s) and abs(s) < 3.4028236e38 and math.isfinite(ctypes.c_float(s).value)):
            raise ValueError(f"set_guidance: scale must be finite (in fp32), got {scale}")
        self.guidance = s
        return self

    def _guided(self) -> bool:
        return self.use_cids and self.guidance is not None

    def _refuse_guided(self, who: str) -> None:
        if self._guided():
            raise ValueError(f"{who}: classifier-free guidance is on (set_guidance): it shapes generation only -- a guided behaviour policy "
                             "against an unguided learner is a different estimator; switch it off with set_guidance(None) first")

    def _guidance_inputs(self, batch) -> dict:
        """Guidance on: the batch with 'guidance_scale' as fp32 [B] (the float of set_guidance where the batch gives none; kept as
        last_guidance_scale) and 'negative_text' as int64 in the shape of 'text' (the null caption when absent: index operations on the
        device, no host synchronisation) on the images' device.  Guidance off: the batch without the two keys."""
        if not self._guided():
            return {k: v for k, v in batch.items() if k not in ("guidance_scale", "negative_text")} if (
                "guidance_scale" in batch or "negative_text" in batch) else batch
        images, text = batch["images"], batch["text"]
        B = images.shape[0]
        gs = batch.get("guidance_scale")
        if gs is None:
            gs = torch.full((B,), self.guidance, dtype=F32)
        gs = torch.as_tensor(gs)
        if gs.dtype != F32 or tuple(gs.shape) != (B,):
            raise ValueError(f"batch['guidance_scale'] must be fp32 [{B}], got {gs.dtype} {tuple(gs.shape)}")
        gs = gs.to(images.device).contiguous()
        neg = batch.get("negative_text")
        if neg is None:
            from ..utils.glue import null_caption
            neg = null_caption(text.to(torch.int64), int(getattr(self.text_encoder, "padding_idx", 0)))
        neg = torch.as_tensor(neg)
        if neg.dtype != torch.int64 or tuple(neg.shape) != tuple(text.shape):
            raise ValueError(f"batch['negative_text'] must be int64 {list(text.shape)} (the shape of batch['text']: the motion-anchor "
                             f"cross-attention is unmasked, so the padded length is part of the result), got {neg.dtype} {list(neg.shape)}")
        self.last_guidance_scale = gs
        return {**batch, "guidance_scale": gs, "negative_text": neg.to(images.device).contiguous()}

    def set_context(self, frames: int = 1) -> "MAGE":
        """Continue a clip: frames 0 .. k-1 of batch['images'] are given (1 <= k <= frames_length - 1; 1, the default: only frame 0, off)
        and autoregressive_generate produces frames k .. L-1.  All B * k given frames go through the VQ encoder in one call (or come as
        batch['context_tokens'], int64 [B, k, h, w], which replaces the encode); the returned video holds images[:, :k] verbatim, as frame 0
        is held, and only the generated frames are decoded.
        Together with batch['known_tokens'] (int64 [B, L-1, h, w]: slot i is frame i + 1, any negative value means "free") this is one
        mechanism -- some token slots are given, the rest are picked, later frames condition on both: after every frame's pick one
        mage_apply_known_tokens launch (include/mage_hip_ext.h) stores the given tokens over the picked ones.  Given frames 1 .. k-1 are slots
        0 .. k-2 and win over known_tokens there.  A given slot reports log-probability 0, entropy 0 and a kept set of 1 in set_logprobs'
        results (a policy that takes the token with certainty), so clip totals and the best-of-N choice are over the free tokens; last_logits
        (full loop) still holds the model's own prediction everywhere.  last_known_mask (bool [B, L-1, h, w]) tells which slots were given.
        Free slots keep their sampler counters: a clip with nothing given is the unconstrained clip bit for bit.
        Incremental mode takes the anchor and the k given frames as one window (no decoder step and no pick before frame k).
        While k > 1, or for a batch that carries known_tokens, score, policy_loss, token_policy_logprobs, clip_logprobs, preference_loss and
        rollout are refused: the setting and the batch keys shape generation.  Fine-tuning on continued clips is explicit instead --
        rollout(context=, known_tokens=) draws them and the loss methods take the mask of the given slots as given=."""
        if isinstance(frames, bool) or not isinstance(frames, int):
            raise ValueError(f"set_context: frames must be an integer, got {frames!r}")
        if not 1 <= frames <= self.frames_length - 1:
            raise ValueError(f"set_context: frames must be in [1, {self.frames_length - 1}] (frames_length - 1), got {frames}")
        if frames > 1 and not self.use_cids:
            raise ValueError("set_context: a use_cids=False (MAGE+) model regresses continuous latents; it has no tokens to hold")
        self.context_frames = frames
        return self

    def _ctx(self) -> int:
        return int(self.context_frames) if self.use_cids else 1

    def _refuse_known(self, who: str, batch=None) -> None:
        if self._ctx() > 1 or (isinstance(batch, dict) and ("known_tokens" in batch or "context_tokens" in batch)):
            raise ValueError(f"{who}: given frames or tokens (set_context, batch['known_tokens'] / ['context_tokens']) shape generation only -- "
                             "call set_context(1) and drop the keys first; the loss methods take the given slots explicitly, as given= "
                             "(rollout: as context= and known_tokens=)")

    def _given_mask(self, who: str, given, tshape, device=None):
        """given= of the loss methods: None, or bool [B, L-1, h, w] on the model's GPU (slot i is frame i + 1: last_known_mask's layout,
        rollout's out['given']), contiguous.  Refused before any launch otherwise."""
        if given is None:
            return None
        if not self.use_cids:
            raise ValueError(f"{who}: a use_cids=False (MAGE+) model regresses continuous latents; it has no tokens to hold (given=)")
        if not (torch.is_tensor(given) and given.dtype == torch.bool and tuple(given.shape) == tuple(tshape)):
            raise ValueError(f"{who}: given must be bool {list(tshape)} (True: the slot's token was given, not drawn)")
        if not (given.is_cuda and (device is None or given.device == device)):
            raise ValueError(f"{who}: given must be on the model's ROCm GPU (there is no CPU / PyTorch fallback)")
        return given.contiguous()

    def _known_inputs(self, batch) -> dict:
        """The batch with its optional 'context_tokens' (int64 [B, k, h, w]) and 'known_tokens' (int64 [B, L-1, h, w]) checked and on the
        images' device; last_known_mask is set from them (None on a call with neither set_context(k > 1) nor known_tokens)."""
        self.last_known_mask = None
        ctx, known = batch.get("context_tokens"), batch.get("known_tokens")
        if not self.use_cids:
            if ctx is not None or known is not None:
                raise ValueError("batch['context_tokens'] / ['known_tokens']: a use_cids=False (MAGE+) model regresses continuous latents; "
                                 "it has no tokens to hold")
            return batch
        k = self._ctx()
        if ctx is None and known is None and k == 1:
            return batch
        images = batch["images"]
        B, R, Lm1 = images.shape[0], self.image_resolution, self.frames_length - 1
        if images.shape[1] < k:
            raise ValueError(f"set_context({k}): batch['images'] holds {images.shape[1]} frames")
        out = dict(batch)
        for key, t_, shape in (("context_tokens", ctx, (B, k, R, R)), ("known_tokens", known, (B, Lm1, R, R))):
            if t_ is None:
                continue
            t_ = torch.as_tensor(t_)
            if t_.dtype != torch.int64 or tuple(t_.shape) != shape:
                raise ValueError(f"batch['{key}'] must be int64 {list(shape)}, got {t_.dtype} {list(t_.shape)}")
            out[key] = t_.to(images.device).contiguous()
        if known is not None or k > 1:
            mask = out["known_tokens"] >= 0 if known is not None else torch.zeros(B, Lm1, R, R, device=images.device, dtype=torch.bool)
            mask[:, :k - 1] = True
            self.last_known_mask = mask
        return out

    def set_logprobs(self, on: bool = True, *, policy: bool = False, entropy: bool = False) -> "MAGE":
        """on: autoregressive_generate leaves last_token_logprobs (fp32 [B, L-1, h, w]: the log-probability of each generated token under the
        logits it was picked from -- the model's full softmax at temperature 1, not the filtered set of set_sampling) and last_clip_logprob
        (fp32 [B], their per-clip totals).  Off (the default): both are None and the call launches nothing more.
        policy (needs on, and set_sampling on when a generation or score starts): also the sampler's own view (mage_token_stats: the filter
        of mage_sample_tokens run again in the same arithmetic) -- last_token_policy_logprobs (fp32 [B, L-1, h, w]: the log-probability under
        the temperature-scaled softmax renormalised over the kept top-k / top-p set, -inf for a token outside it), last_clip_policy_logprob
        (fp32 [B]), last_token_kept (int32 [B, L-1, h, w]: the size of the kept set) and, with candidates = N > 1, last_candidate_policy_scores
        [B, N] (the winner is still picked by the model log-probability).
        entropy (needs on; works with greedy decoding): last_token_entropy (fp32 [B, L-1, h, w], nats: the full softmax at temperature 1) and,
        with sampling on, last_token_policy_entropy (the kept set's).  score honours both flags for the batch's own tokens.
        With set_guidance on, "the logits it was picked from" are the guided logits: last_token_logprobs is their softmax at temperature
        1, last_token_policy_logprobs the sampler's filtered view of the same guided logits, and the entropies are theirs too.
        set_logprobs(False) clears all three switches."""
        if (policy or entropy) and not on:
            raise ValueError("set_logprobs: policy / entropy need on=True")
        if on and not self.use_cids:
            raise ValueError("set_logprobs: a use_cids=False (MAGE+) model regresses continuous latents; it has no token probabilities")
        self.logprobs, self.logprob_policy, self.logprob_entropy = bool(on), bool(policy), bool(entropy)
        return self

    def _n_cand(self) -> int:
        return int(self.candidates) if self.sampling is not None and self.use_cids else 1

    def _want_logprobs(self) -> bool:
        return self.use_cids and (bool(self.logprobs) or self._n_cand() > 1)

    def _want_stats(self) -> Tuple[bool, bool]:
        """(policy, entropy) of set_logprobs; policy without a sampler to describe is refused here, where a generation or score starts."""
        if not (self.use_cids and self.logprobs):
            return False, False
        pol, ent = bool(self.logprob_policy), bool(self.logprob_entropy)
        if pol and self.sampling is None:
            raise ValueError("set_logprobs(policy=True) reports the sampler's distribution: switch sampling on with set_sampling first")
        return pol, ent

    def _stats_alloc(self, shape, device) -> Optional[dict]:
        """The output buffers of mage_token_stats the switches ask for (by its argument names), None when they ask for nothing."""
        pol, ent = self._want_stats()
        if not (pol or ent):
            return None
        sampled = self.sampling is not None
        mk = lambda want, dt: torch.empty(shape, device=device, dtype=dt) if want else None      # noqa: E731
        return {"policy_logprob": mk(pol, F32), "kept": mk(pol, torch.int32), "entropy": mk(ent, F32), "policy_entropy": mk(ent and sampled, F32)}

    def _stats(self, logits, tokens, bufs: dict, sel, **kw) -> None:
        """One mage_token_stats launch beside a mage_token_logprob one (same addressing kw), under the current sampler (greedy: the plain
        softmax); sel picks the launch's view of each buffer."""
        t, k, p = self.sampling or (1.0, 0, 1.0)
        ops.token_stats(logits, tokens, temperature=t, top_k=k, top_p=p, **{n: None if b is None else sel(b) for n, b in bufs.items()}, **kw)

    _STATS_RESULTS = (("policy_logprob", "last_token_policy_logprobs"), ("kept", "last_token_kept"), ("entropy", "last_token_entropy"),
                      ("policy_entropy", "last_token_policy_entropy"))

    @torch.no_grad()
    def score(self, batch, given=None) -> torch.Tensor:
        """Teacher-forced log-likelihood of the batch's own video under its caption: fp32 [B], the sum over frames 1 .. L-1 of the
        log-probabilities of the frames' VQ tokens given the frames before them (last_token_logprobs [B, L-1, h, w] keeps the terms).
        With set_logprobs(policy=, entropy=) it leaves their results for the batch's own tokens too; every result of theirs that this call
        does not compute is None afterwards, last_candidate_policy_scores included (score has no candidates).
        given (bool [B, L-1, h, w], slot i is frame i + 1): the slots whose tokens were given, not drawn -- one mage_apply_known_tokens launch
        writes what generation reports there (log-probabilities and entropies 0, kept 1) before the clip totals, so the score of a continued
        clip is the sum over its free tokens: the generation's last_clip_logprob, by the same mechanism on both sides."""
        if not self.use_cids:
            raise ValueError("score: a use_cids=False (MAGE+) model regresses continuous latents; it has no token probabilities")
        self._refuse_guided("score")
        self._refuse_known("score", batch)
        images = batch["images"]
        _need_gpu(images, "MAGE.score")
        given = self._given_mask("score", given, (images.shape[0], self.frames_length - 1, self.image_resolution, self.image_resolution),
                                 images.device)
        self._want_stats()                                # (refuses policy without sampling before anything runs)
        with torch.cuda.device(images.device), weights_frozen():
            tok, logits = self.teacher_forced_logits(batch)
            B, L, K = images.shape[0], self.frames_length, self.codebook_size
            tgt = tok[:, 1:L].contiguous()
            lp = torch.empty(tgt.shape, device=images.device, dtype=F32)
            ops.token_logprob(logits, tgt, lp, rows=tgt.numel(), K=K)
            if given is None:
                scores, _ = ops.clip_scores(lp, n_clips=B)
            self.last_token_logprobs = lp
            st = self._stats_alloc(tgt.shape, images.device)   # the batch's own tokens under the current sampler: -inf where it could never draw one
            for _, attr in self._STATS_RESULTS:
                setattr(self, attr, None)
            self.last_clip_policy_logprob = self.last_candidate_policy_scores = None
            if st is not None:
                self._stats(logits, tgt, st, lambda b: b, rows=tgt.numel(), K=K)
                for name, attr in self._STATS_RESULTS:
                    setattr(self, attr, st[name])
            if given is not None:                         # the given slots' results, then the totals over the free tokens
                ops.apply_known_tokens(tgt, torch.where(given, tgt, -1), rows=tgt.numel(), K=K, logprob=lp, **(st or {}))
                scores, _ = ops.clip_scores(lp, n_clips=B)
            if st is not None and st["policy_logprob"] is not None:
                self.last_clip_policy_logprob = ops.clip_scores(st["policy_logprob"], n_clips=B)[0].view(B)
            ops.check_device_errors(images.device)
        return scores.view(B)

    def _refuse_no_rows(self, who: str) -> None:
        """The supervised-loss kernel reads rows of codebook_size logits as 16-byte vectors: a token model whose codebook is a multiple of 4."""
        if not self.use_cids:
            raise ValueError(f"{who}: a use_cids=False (MAGE+) model regresses continuous latents; it has no token probabilities")
        if self.codebook_size % 4 != 0:
            raise ValueError(f"{who}: codebook_size={self.codebook_size} must be a multiple of 4 (mage_token_xent reads 16-byte vectors)")

    def set_loss(self, label_smoothing: float = 0.0, z_loss: float = 0.0, class_weights: Optional[torch.Tensor] = None) -> "MAGE":
        """The options of forward's supervised next-token loss (mage_token_xent, include/mage_hip_ext.h), F.cross_entropy's own:
        label_smoothing in [0, 1): every token's target is (1 - eps) one-hot + eps / K uniform;
        z_loss >= 0: the loss gains z_loss * mean(logsumexp(logits)^2), which keeps the logits' scale near log Z = 0;
        class_weights fp32 [codebook_size], finite, >= 0, at least one > 0 (mage_amd.utils.glue.balanced_class_weights): token k's term is
        weighted by class_weights[k] and the mean is a weighted mean (F.cross_entropy's weight=).  They are kept on the model's device.
        With any of them set, forward ends in the SupervisedHead (modules/mage_train.py) in both grad modes and its loss dict gains 'nll' (the
        plain mean negative log-likelihood, comparable across settings) and 'accuracy'.  set_loss() restores the defaults: forward is then
        the plain cross entropy again, launch for launch.  evaluate ignores these options: it measures the model, not the objective."""
        for name, v, hi in (("label_smoothing", label_smoothing, 1.0), ("z_loss", z_loss, 3.4e38)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and 0.0 <= v < hi):
                raise ValueError(f"set_loss: {name} must be a finite number in [0, {'1' if hi == 1.0 else 'inf'}), got {v!r}")
        w = class_weights
        if w is not None:
            K = self.codebook_size
            if not (torch.is_tensor(w) and w.dtype == F32 and tuple(w.shape) == (K,) and bool(torch.isfinite(w).all()) and bool((w >= 0).all())
                    and bool((w > 0).any())):
                raise ValueError(f"set_loss: class_weights must be fp32 [{K}], finite, >= 0 and somewhere > 0")
        if label_smoothing == 0 and z_loss == 0 and w is None:
            self.loss_options = None
            return self
        self._refuse_no_rows("set_loss")
        if w is not None:
            w = w.detach().to(next(self.parameters()).device).contiguous().clone()
        self.loss_options = dict(label_smoothing=float(label_smoothing), z_loss=float(z_loss), class_weights=w)
        return self

    def _supervised_head(self, batch):
        """forward's loss head: None (the model's own: the plain cross entropy or MSE) unless set_loss set an option or the batch carries
        'given' (bool [B, L-1, h, w], last_known_mask's layout: the slots left out of the loss); then the SupervisedHead.  Refusals before
        any launch."""
        given = batch.get("given")
        if self.loss_options is None and given is None:
            return None
        from . import mage_train
        self._refuse_no_rows("forward")
        images = batch["images"]
        given = self._given_mask("forward", given, (images.shape[0], self.frames_length - 1, self.image_resolution, self.image_resolution),
                                 images.device if images.is_cuda else None)
        o = dict(self.loss_options or {})
        w = o.get("class_weights")
        if w is not None and w.device != images.device:
            w = w.to(images.device)
            self.loss_options["class_weights"] = w       # (the model has moved since set_loss)
            o["class_weights"] = w
        return mage_train.SupervisedHead(None, given=None if given is None else given.reshape(-1), **o)

    @torch.no_grad()
    def evaluate(self, batch, topk=(1, 5), given=None) -> dict:
        """What the model predicts on the batch's own video, token by token: one teacher-forced pass (score's) ending in mage_token_xent with
        every option off, under no_grad.  Returns device tensors:
          'nll' (the mean negative log-likelihood of the free tokens, nats), 'perplexity' (exp nll), 'accuracy' (the share of free tokens the
          argmax predicts), 'mean_rank' (the mean rank of the true code among the K logits; 0: always first), all 0-dim fp32;
          'topk_accuracy': {k: 0-dim fp32, the share of free tokens whose true code is among the k largest logits} for k in topk;
          'frame_nll', 'frame_accuracy': fp32 [L-1], the same means per frame over the frame's free tokens (a frame without one: 0) -- how
          exposure bias shows along a clip;
          'token_nll' fp32 and 'token_rank' int32, [B, L-1, h, w]: -last_token_logprobs of score, bit for bit, and each true code's rank.
        given (bool [B, L-1, h, w], slot i is frame i + 1): slots to leave out, e.g. the context of a continuation; their token values are 0.
        set_loss is ignored (the model is measured, not the objective); guidance and given frames or tokens are refused as by score.  The
        per-frame and top-k reductions are torch ops on the per-token tensors."""
        self._refuse_no_rows("evaluate")
        self._refuse_guided("evaluate")
        self._refuse_known("evaluate", batch)
        K = self.codebook_size
        if not (isinstance(topk, (tuple, list)) and len(topk) > 0
                and all(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= K for k in topk)):
            raise ValueError(f"evaluate: topk must be a non-empty tuple of ints in [1, {K}], got {topk!r}")
        images = batch["images"]
        B, Lm1, R = images.shape[0], self.frames_length - 1, self.image_resolution
        given = self._given_mask("evaluate", given, (B, Lm1, R, R), images.device if images.is_cuda else None)
        if not images.is_cuda:
            raise ValueError("evaluate: batch['images'] must be on the model's ROCm GPU (there is no CPU / PyTorch fallback)")
        with torch.cuda.device(images.device), weights_frozen():
            tok, logits = self.teacher_forced_logits(batch)
            tgt = tok[:, 1:].reshape(-1).contiguous()
            res = ops.token_xent(logits.reshape(-1, K), tgt, given=None if given is None else given.reshape(-1))
            ops.check_device_errors(images.device)
            tshape = (B, Lm1, R, R)
            nll_t, rank_t = res["row_nll"].view(tshape), res["rank"].view(tshape)
            free = torch.ones(tshape, device=images.device, dtype=torch.bool) if given is None else ~given
            # (integer counts and fp64 sums of a few thousand values, rounded once to fp32)
            n_all, n_frame = free.sum().clamp(min=1).double(), free.sum((0, 2, 3)).clamp(min=1).double()
            hit = lambda k: free & (rank_t < k)      # noqa: E731
            nll = res["summary"][1].clone()
            return {"nll": nll, "perplexity": nll.exp(), "accuracy": res["summary"][2].clone(),
                    "mean_rank": ((rank_t * free).sum().double() / n_all).to(F32),
                    "topk_accuracy": {int(k): (hit(k).sum().double() / n_all).to(F32) for k in topk},
                    "frame_nll": ((nll_t.double() * free).sum((0, 2, 3)) / n_frame).to(F32),
                    "frame_accuracy": (hit(1).sum((0, 2, 3)).double() / n_frame).to(F32), "token_nll": nll_t, "token_rank": rank_t}

    def policy_loss(self, batch, tokens, advantages, behaviour_logprobs=None, *, clip=0.2, entropy_coef: float = 0.0, reference_logprobs=None,
                    kl_coef: float = 0.0, given=None, ratio: str = "token"):
        """Policy-gradient loss of given tokens under the policy set_sampling currently describes (sampling off: temperature 1, no filter):
        (loss, info) of one teacher-forced pass over frame 0 of batch['images'] (plus batch['text'] and the optional batch['speed'], as
        autoregressive_generate reads them) followed by `tokens` (int64 [B, L-1, h, w], e.g. last_tokens), ending in mage_policy_loss
        (include/mage_hip_ext.h states the rule).  advantages: fp32 [B] (one per clip), [B, L-1] (one per frame:
        rollout(credit='frame')'s) or [B, L-1, h, w] (one per token).
        behaviour_logprobs None: the reward-weighted likelihood, mean of -A logprob - entropy_coef entropy.  behaviour_logprobs fp32
        [B, L-1, h, w] (e.g. last_token_policy_logprobs of the call that drew the tokens): the clipped surrogate with the importance ratio
        rho = exp(logprob - behaviour), clipped to [1 - lo, 1 + hi]; clip is a float (lo = hi) or a (lo, hi) pair.  A token the current
        filter could never draw contributes 0 and no gradient and is counted in info['outside_fraction'].
        In grad mode (any parameter requiring grad) the loss carries one autograd node over the trainable parameters backed by the HIP
        backward kernels, as forward's does: loss.backward(); optimizer.step() works.  Under torch.no_grad(): values only.
        info = {'loss', 'entropy', 'approx_kl' (mean of behaviour - logprob), 'clip_fraction', 'outside_fraction'} as floats;
        last_policy_token_logprobs keeps the per-token log-probabilities (fp32 [B, L-1, h, w]).
        randomness=True: the policy is pi(tokens | frame 0, caption, speed, z) with z the generation-time noise, a latent drawn from a fixed
        N(0, 1) -- context, not a parameter: batch['video_noise'] (fp32 [B, 64, h, w]: last_video_noise of the generation that drew the
        tokens, or rollout's out['batch']) is required, and the pass modulates the motion anchor with it as generation did (conv_d2, the
        ADAIN convolutions, ADAIN; no Conv3d video prior, no reparameterisation, no KL of the prior: generation runs none of them, so their
        parameters get zero gradients).
        reference_logprobs fp32 [B, L-1, h, w] (the same tokens under a frozen reference policy: token_policy_logprobs of a copy of the
        model taken before fine-tuning, or rollout(reference=)'s 'reference_logprobs') with kl_coef >= 0: every token's loss gains kl_coef
        times the k3 estimate exp(d) - d - 1, d = reference - logprob, of its KL against the reference (mage_policy_loss_anchored); a token
        whose reference value is not finite (the reference's filter could not draw it) is unanchored: no penalty.  info gains 'kl' (the
        mean estimate) and 'unanchored_fraction', last_policy_token_kl keeps the per-token values.  Without a reference the call is the
        plain one in every bit, and last_policy_token_kl is None.
        given bool [B, L-1, h, w] (slot i is frame i + 1; rollout(context=, known_tokens=)'s out['given'], or last_known_mask of a
        generation): the slots whose tokens were given, not drawn (mage_policy_loss_masked).  A given slot is not scored -- no ratio, no KL
        term, no gradient, its logits are not even read -- every mean in info is over the free tokens, info gains 'given_fraction', and
        last_policy_token_logprobs / last_policy_token_kl hold 0 there.  With advantages 1, sampling off and entropy_coef 0 this is the
        cross-entropy over the free tokens only: the supervised loss for continuation fine-tuning.  Without given the call is the unmasked
        one in every launch.
        ratio 'token' (the default: the calls above, launch for launch), 'frame' or 'clip': the unit that gets ONE importance ratio
        (mage_policy_loss_grouped).  A frame's h*w tokens are drawn in one step, so a frame is one action: under 'frame' every token of a
        frame is clipped by the frame's ratio rho_g = exp(mean over its free, drawable tokens of logprob - behaviour), the geometric mean
        of their token ratios (GSPO's length-normalised sequence ratio); under 'clip' the group is all (L-1)*h*w tokens of a clip.
        behaviour_logprobs is required (without one there is no ratio to group) and the advantages may not be finer than the group: [B] or
        [B, L-1] under 'frame', [B] under 'clip'.  given, the reference KL, entropy_coef, the sampler's filter and randomness=True work as
        under 'token', and info has the same keys ('clip_fraction' stays a share of tokens: those of the groups the clip switched off).
        last_policy_group_logratio keeps the groups' mean log-ratios, fp32 [B, L-1] or [B] (0 for a group with nothing to count, e.g. a
        frame given by a context); it is None under 'token'.
            out = m.rollout(batch, 8, credit='frame', reference=ref)
            m.policy_loss(out['batch'], out['tokens'], out['advantages'], out['behaviour_logprobs'],
                          reference_logprobs=out['reference_logprobs'], kl_coef=0.1, given=out['given'], ratio='frame')
        Dropout follows self.training, as in forward: the ratios against a generation's log-probabilities are only meaningful in eval()."""
        from . import mage_train
        images, B, tshape, vn = self._given_tokens_inputs("policy_loss", batch, tokens)
        t, k, p = self.sampling or (1.0, 0, 1.0)
        if k == 1:
            raise ValueError("policy_loss: top_k=1 is greedy decoding: its log-probability is 0 and has no gradient")
        if not (torch.is_tensor(advantages) and advantages.dtype == F32 and tuple(advantages.shape) in ((B,), tshape[:2], tshape)):
            raise ValueError(f"policy_loss: advantages must be fp32 [{B}], {list(tshape[:2])} or {list(tshape)}")
        b = behaviour_logprobs
        if b is not None and not (torch.is_tensor(b) and b.dtype == F32 and tuple(b.shape) == tshape):
            raise ValueError(f"policy_loss: behaviour_logprobs must be fp32 {list(tshape)} or None")
        try:
            lo, hi = (float(clip), float(clip)) if not isinstance(clip, (tuple, list)) else (float(clip[0]), float(clip[1]))
            if isinstance(clip, (tuple, list)) and len(clip) != 2:
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"policy_loss: clip must be a float or a (lo, hi) pair, got {clip!r}") from None
        if not (0.0 <= lo <= 1.0 and hi >= 0.0):
            raise ValueError(f"policy_loss: clip lo={lo} must lie in [0, 1] and hi={hi} must be >= 0")
        if not math.isfinite(float(entropy_coef)):
            raise ValueError(f"policy_loss: entropy_coef must be finite, got {entropy_coef}")
        ref = reference_logprobs
        if ref is not None and not (torch.is_tensor(ref) and ref.dtype == F32 and tuple(ref.shape) == tshape):
            raise ValueError(f"policy_loss: reference_logprobs must be fp32 {list(tshape)} or None")
        if isinstance(kl_coef, bool) or not isinstance(kl_coef, (int, float)) or not (math.isfinite(kl_coef) and 0 <= kl_coef < 3.4e38):
            raise ValueError(f"policy_loss: kl_coef must be finite and >= 0, got {kl_coef!r}")
        if kl_coef > 0 and ref is None:
            raise ValueError("policy_loss: kl_coef > 0 needs reference_logprobs (the penalty is against a reference policy)")
        given = self._given_mask("policy_loss", given, tshape)
        if ratio not in ("token", "frame", "clip"):
            raise ValueError(f"policy_loss: ratio must be 'token', 'frame' or 'clip', got {ratio!r}")
        ratio_div = None
        if ratio != "token":
            if b is None:
                raise ValueError(f"policy_loss: ratio={ratio!r} needs behaviour_logprobs (without one there is no ratio to group)")
            coarse = ((B,), tshape[:2]) if ratio == "frame" else ((B,),)
            if tuple(advantages.shape) not in coarse:
                raise ValueError(f"policy_loss: ratio={ratio!r} takes one ratio per {ratio}: advantages must be fp32 "
                                 + " or ".join(str(list(c)) for c in coarse) + f", not finer than the group (got {list(advantages.shape)})")
            ratio_div = tshape[2] * tshape[3] * (1 if ratio == "frame" else tshape[1])
        self._refuse_off_gpu("policy_loss", batch, images, tokens, vn, (("advantages", advantages), ("behaviour_logprobs", b),
                                                                       ("reference_logprobs", ref), ("given", given)))
        args = dict(advantage=advantages.contiguous().reshape(-1), temperature=t, top_k=k, top_p=p, clip_lo=lo, clip_hi=hi,
                    entropy_coef=float(entropy_coef), behaviour=None if b is None else b.contiguous().reshape(-1),
                    reference=None if ref is None else ref.contiguous().reshape(-1), kl_coef=float(kl_coef),
                    given=None if given is None else given.reshape(-1), ratio_div=ratio_div)
        with torch.cuda.device(images.device):
            loss, (info, res) = self._run_head(batch, mage_train.PolicyHead(tokens.contiguous(), **args))
            self.last_policy_token_logprobs = res["logprob"].view(tshape)
            self.last_policy_token_kl = None if res.get("kl") is None else res["kl"].view(tshape)
            self.last_policy_group_logratio = None if ratio_div is None else res["group_logratio"].view(tshape[:2] if ratio == "frame" else (B,))
            ops.check_device_errors(images.device)
        return loss, info

    def _given_tokens_inputs(self, who, batch, tokens, guided_ok: bool = False):
        """The refusals every pass over given tokens shares (policy_loss and preference_loss, under the name `who`), all before the first
        launch.  Returns (images, B, the tokens' shape (B, L-1, h, w), batch['video_noise'] on a randomness=True model or None).
        guided_ok: distill_targets alone, whose result is the guided logits."""
        L, R = self.frames_length, self.image_resolution
        if not self.use_cids:
            raise ValueError(f"{who}: a use_cids=False (MAGE+) model regresses continuous latents; it has no token probabilities")
        if not guided_ok:
            self._refuse_guided(who)
        self._refuse_known(who, batch)
        if not isinstance(batch, dict):
            raise ValueError(f"{who}: batch must be a dict with 'images' and 'text'")
        vn = batch.get("video_noise") if self.randomness else None
        if self.randomness and vn is None:
            raise ValueError(f"{who}: randomness=True conditions the policy on the generation-time noise: batch['video_noise'] must hold "
                             "the noise the tokens were drawn under (last_video_noise of the generation, or rollout's out['batch'])")
        if self._dt() == torch.float16:
            raise ValueError(f"{who}: precision 'f16' is a generation mode: train with set_precision('bf16') or 'fp32'")
        images = batch.get("images")
        if not (torch.is_tensor(images) and images.dim() == 5 and images.shape[0] >= 1 and images.shape[1] >= 1):
            raise ValueError(f"{who}: batch['images'] must be [B, >= 1, C, H, W]")
        B = images.shape[0]
        tshape = (B, L - 1, R, R)
        if vn is not None and not (torch.is_tensor(vn) and vn.dtype == F32 and tuple(vn.shape) == (B, 64, R, R)):
            raise ValueError(f"{who}: batch['video_noise'] must be fp32 {[B, 64, R, R]} (randomness=True: the tokens' generation noise)")
        if not (torch.is_tensor(tokens) and tokens.dtype == torch.int64 and tuple(tokens.shape) == tshape):
            raise ValueError(f"{who}: tokens must be int64 {list(tshape)}")
        return images, B, tshape, vn

    @staticmethod
    def _refuse_off_gpu(who, batch, images, tokens, vn, own):
        """The last refusal of a pass over given tokens: the batch's tensors, the tokens and the method's `own` (name, tensor) arguments."""
        for name, x in (("batch['images']", images), ("batch['text']", batch["text"]), ("tokens", tokens), *own, ("batch['video_noise']", vn)):
            if x is not None and not (x.is_cuda and x.device == images.device):
                raise ValueError(f"{who}: {name} must be on the model's ROCm GPU (there is no CPU / PyTorch fallback)")

    def _run_head(self, batch, head):
        """One mage_train pass ending in `head` (None: forward's own): (loss, (loss dict, what the head saved)).  In grad mode (any parameter
        requiring grad) the loss carries the autograd node over the trainable parameters; under torch.no_grad(): values only."""
        from . import mage_train
        if torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters()):
            names = mage_train.trainable_names(self)
            byname = dict(self.named_parameters())
            loss = mage_train.MageLossFn.apply(self, batch, head, names, *[byname[n] for n in names])
            out, self._last_head_out = self._last_head_out, None
            return loss, out
        with torch.no_grad():
            loss, tape = mage_train.train_forward(self, batch, head)
        return loss.clone(), (tape["parts"], tape["saved"])

    @contextlib.contextmanager
    def _last_results_kept(self):
        """Every last_* result is left as found: what the block adds is removed, what it overwrites is put back."""
        last = lambda: {a: v for a, v in vars(self).items() if a.startswith("last_")}      # noqa: E731
        keep = last()
        try:
            yield
        finally:
            for a in last().keys() - keep.keys():
                delattr(self, a)
            for a, v in keep.items():
                setattr(self, a, v)

    @torch.no_grad()
    def token_policy_logprobs(self, batch, tokens, given=None) -> torch.Tensor:
        """fp32 [B, L-1, h, w]: the log-probabilities of given tokens (int64 [B, L-1, h, w]) under the policy set_sampling currently
        describes, by the teacher-forced pass policy_loss runs -- bit for bit last_policy_token_logprobs of a no-grad policy_loss on the
        same inputs (-inf where the filter could not draw the token).  How a frozen copy of the model gives policy_loss its
        reference_logprobs.  given: policy_loss' (0 at the given slots).  Values only; every last_* result is left as found."""
        self._refuse_guided("token_policy_logprobs")
        self._refuse_known("token_policy_logprobs", batch)
        images = batch["images"] if isinstance(batch, dict) else None
        if not (torch.is_tensor(images) and images.dim() == 5 and images.shape[0] >= 1):
            raise ValueError("token_policy_logprobs: batch['images'] must be [B, >= 1, C, H, W]")
        with self._last_results_kept():
            self.policy_loss(batch, tokens, torch.zeros(images.shape[0], device=images.device, dtype=F32), given=given)
            return self.last_policy_token_logprobs

    _PREFERENCE_LOSSES = {"sigmoid": 0, "ipo": 1}

    def preference_loss(self, batch, tokens, pairs, reference_logprobs, *, beta: float = 0.1, label_smoothing: float = 0.0,
                        loss: str = "sigmoid", given=None):
        """Preference loss (DPO; loss='ipo': IPO) over ranked pairs of clips: (loss, info) of policy_loss' teacher-forced pass over frame 0
        of batch['images'] (plus batch['text'], the optional batch['speed'], and batch['video_noise'] on a randomness=True model) followed
        by `tokens` (int64 [B, L-1, h, w]), ending in mage_token_logprob, mage_clip_scores and mage_preference_loss (include/mage_hip_ext.h
        states the rule).  pairs: int64 [P, 2] rows of the batch, (chosen, rejected) -- e.g. rollout(pairs='best_worst')'s, human labels
        or a stored dataset; a pair (i, i) is no preference and has no gradient.  reference_logprobs: fp32 [B], the same clips'
        log-likelihoods under a frozen reference model: ref.clip_logprobs(batch, tokens), or rollout(reference=, pairs=)'s
        'reference_clip_logprobs'.  With s the clips' log-likelihoods under this model, r the reference's and u = (s_w - r_w) - (s_l - r_l)
        for a pair (w, l), the loss is the mean over the pairs of -(1 - eps) logsig(beta u) - eps logsig(-beta u) (eps = label_smoothing in
        [0, 0.5)), or of (u - 1 / (2 beta))^2 with loss='ipo' (label_smoothing must be 0).
        The log-likelihoods are the model's own -- the full softmax at temperature 1 with no filter, what score reports -- whatever
        set_sampling says: a preference is about the model, and a filtered policy would turn one undrawable token into a -inf sequence.
        In grad mode the loss carries one autograd node over the trainable parameters, as policy_loss' does: its backward pass starts from
        mage_token_logprob_bwd with one coefficient per clip (clips in no pair cost a zero fill).  Under torch.no_grad(): values only.
        info = {'loss', 'accuracy' (the share of pairs with u > 0), 'chosen_reward' (mean beta (s_w - r_w)), 'rejected_reward', 'margin'
        (mean beta u)} as floats; last_preference_clip_logprobs (fp32 [B]), last_preference_clip_coef (fp32 [B]: d loss / d s),
        last_preference_pair_loss, last_preference_pair_margin (fp32 [P]) and last_preference_token_logprobs (fp32 [B, L-1, h, w]) keep the
        rest.  Dropout follows self.training, as in forward: compare with a reference in eval().
        given bool [B, L-1, h, w] (policy_loss'): the given slots count 0 in every clip's log-likelihood (one mage_apply_known_tokens launch
        before the totals: what generation and score(given=) report) and get no gradient (mage_token_logprob_bwd_masked); the reference's
        log-likelihoods should leave them out alike (clip_logprobs(given=)).  info gains 'given_fraction'."""
        return self._preference("preference_loss", batch, tokens, pairs, reference_logprobs, beta, label_smoothing, loss, given)

    def _preference(self, who, batch, tokens, pairs, reference_logprobs, beta, label_smoothing, loss, given=None):
        """preference_loss under the name `who` (clip_logprobs runs it too); every refusal comes before the first launch."""
        from . import mage_train
        images, B, tshape, vn = self._given_tokens_inputs(who, batch, tokens)
        if not (torch.is_tensor(pairs) and pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2
                and 1 <= pairs.shape[0] <= 65536):
            raise ValueError(f"{who}: pairs must be int64 [P, 2] (chosen row, rejected row) with 1 <= P <= 65536")
        if B > 65536:
            raise ValueError(f"{who}: at most 65536 clips per call, got {B}")
        ref = reference_logprobs
        if not (torch.is_tensor(ref) and ref.dtype == F32 and tuple(ref.shape) == (B,)):
            raise ValueError(f"{who}: reference_logprobs must be fp32 [{B}] (clip_logprobs of the reference model)")
        if loss not in self._PREFERENCE_LOSSES:
            raise ValueError(f"{who}: loss must be one of {list(self._PREFERENCE_LOSSES)}, got {loss!r}")
        ok_num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)      # noqa: E731
        if not (ok_num(beta) and 1e-45 <= beta < 3.4e38):              # (a positive fp32 value)
            raise ValueError(f"{who}: beta must be finite and > 0, got {beta!r}")
        if not (ok_num(label_smoothing) and 0 <= label_smoothing < 0.5):
            raise ValueError(f"{who}: label_smoothing must lie in [0, 0.5), got {label_smoothing!r}")
        if loss == "ipo" and label_smoothing != 0:
            raise ValueError(f"{who}: label_smoothing is the sigmoid loss's; loss='ipo' takes 0, got {label_smoothing!r}")
        given = self._given_mask(who, given, tshape)
        self._refuse_off_gpu(who, batch, images, tokens, vn, (("pairs", pairs), ("reference_logprobs", ref), ("given", given)))
        head = mage_train.PreferenceHead(tokens.contiguous(), pairs=pairs.contiguous(), reference=ref.contiguous(), beta=float(beta),
                                         label_smoothing=float(label_smoothing), mode=self._PREFERENCE_LOSSES[loss],
                                         **({} if given is None else {"given": given.reshape(-1)}))
        with torch.cuda.device(images.device):
            val, (info, res) = self._run_head(batch, head)
            if given is not None:
                info = dict(info, given_fraction=int(given.sum().item()) / given.numel())
            self.last_preference_clip_logprobs = res["clip_logprob"]
            self.last_preference_clip_coef = res["clip_coef"]
            self.last_preference_pair_loss = res["pair_loss"]
            self.last_preference_pair_margin = res["pair_margin"]
            self.last_preference_token_logprobs = res["logprob"].view(tshape)
            ops.check_device_errors(images.device)
        return val, info

    @torch.no_grad()
    def clip_logprobs(self, batch, tokens, given=None) -> torch.Tensor:
        """fp32 [B]: the teacher-forced log-likelihood of given tokens (int64 [B, L-1, h, w]) after frame 0 of batch['images'], under the
        model's own distribution -- the full softmax at temperature 1 with no filter, the one score reports, whatever set_sampling says --
        by the pass preference_loss runs: bit for bit its last_preference_clip_logprobs on the same inputs.  How a frozen copy of the model
        gives preference_loss its reference_logprobs.  given: preference_loss' (the totals are over the free slots).  Values only; every
        last_* result is left as found."""
        images = batch.get("images") if isinstance(batch, dict) else None
        if not (torch.is_tensor(images) and images.dim() == 5 and images.shape[0] >= 1):
            raise ValueError("clip_logprobs: batch['images'] must be [B, >= 1, C, H, W]")
        with self._last_results_kept():
            self._preference("clip_logprobs", batch, tokens, torch.zeros(1, 2, device=images.device, dtype=torch.int64),   # (0, 0): no preference
                             torch.zeros(images.shape[0], device=images.device, dtype=F32), 1.0, 0.0, "sigmoid", given)
            return self.last_preference_clip_logprobs

    @torch.no_grad()
    def distill_targets(self, batch, tokens) -> torch.Tensor:
        """fp32 [B*(L-1)*h*w, K]: this model's logits for given tokens (int64 [B, L-1, h, w]), by the teacher-forced pass policy_loss runs --
        frame 0 of batch['images'], batch['text'], the optional batch['speed'] and batch['video_noise'] on a randomness=True model, followed
        by `tokens`.  What a teacher hands a student's distill_loss; a model is its own exact teacher (the same pass, the same bits).
        Allowed while guidance is on, and that is the point: the pass then runs once under batch['text'] and once under
        batch['negative_text'] (the null caption when absent), and one mage_guide_logits launch combines the two in place with the per-clip
        scales of set_guidance / batch['guidance_scale'] -- the distribution a guided generation picks from, for a student that runs once.
        Scale 1 gives the unguided result bit for bit.  Values only; every last_* result is left as found.  Refused under
        set_context(k > 1) and the known-token batch keys, as policy_loss is."""
        from . import mage_train
        images, B, tshape, vn = self._given_tokens_inputs("distill_targets", batch, tokens, guided_ok=True)
        self._refuse_off_gpu("distill_targets", batch, images, tokens, vn, ())
        with self._last_results_kept(), torch.cuda.device(images.device):
            gb = self._guidance_inputs(batch)
            run = lambda b: self._run_head(b, mage_train.LogitsHead(tokens.contiguous()))[1][1]      # noqa: E731
            logits = run(gb)
            if self._guided():
                rows, K = logits.shape
                ops.guide_logits(logits, run({**gb, "text": gb["negative_text"]}), gb["guidance_scale"], rows=rows, K=K, scale_div=rows // B)
            ops.check_device_errors(images.device)
        return logits

    _DISTILL_MODES = {"forward": 0, "reverse": 1}

    def distill_loss(self, batch, tokens, teacher_logits, *, temperature: float = 1.0, mode: str = "forward", given=None):
        """Distillation loss against a teacher's whole distribution: (loss, info) of policy_loss' teacher-forced pass over frame 0 of
        batch['images'] (plus batch['text'], the optional batch['speed'], and batch['video_noise'] on a randomness=True model) followed by
        `tokens` (int64 [B, L-1, h, w]: what to distil on, e.g. the teacher's own generation), ending in mage_distill_loss
        (include/mage_hip_ext.h states the rule).  teacher_logits: fp32 [B*(L-1)*h*w, K] on the model's GPU, teacher.distill_targets(batch,
        tokens) -- a guided teacher's, a higher-precision copy's, the model's own starting point's.  The loss is the mean over the tokens
        of the KL between the two softmaxes at `temperature` (both rows divided by it): mode 'forward' KL(teacher || student), 'reverse'
        KL(student || teacher).  It is not multiplied by temperature^2: `loss * t * t` does that through the gradient.  Equal logits give
        exactly 0.0 and exactly zero gradients.
        In grad mode the loss carries one autograd node over the trainable parameters, as policy_loss' does; under torch.no_grad(): values
        only.  info = {'loss', 'teacher_entropy', 'entropy' (the student's), 'agreement' (the share of tokens where both argmax codes
        coincide), 'given_fraction'} as floats; last_distill_token_kl keeps the per-token KL (fp32 [B, L-1, h, w]).
        given bool [B, L-1, h, w] (policy_loss'): the given slots are not read, count 0 and get no gradient; the means are over the free
        tokens.  Refused while guidance is on in THIS model (the student runs unguided: that is what it is trained for), under
        set_context(k > 1) and the known-token batch keys."""
        from . import mage_train
        images, B, tshape, vn = self._given_tokens_inputs("distill_loss", batch, tokens)
        rows = B * tshape[1] * tshape[2] * tshape[3]
        tl = teacher_logits
        if not (torch.is_tensor(tl) and tl.dtype == F32 and tuple(tl.shape) == (rows, self.codebook_size)):
            raise ValueError(f"distill_loss: teacher_logits must be fp32 {[rows, self.codebook_size]} (distill_targets of the teacher)")
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (
                math.isfinite(temperature) and 1e-30 <= temperature < 3.4e38):
            raise ValueError(f"distill_loss: temperature must be finite and > 0, got {temperature!r}")
        if mode not in self._DISTILL_MODES:
            raise ValueError(f"distill_loss: mode must be one of {list(self._DISTILL_MODES)}, got {mode!r}")
        given = self._given_mask("distill_loss", given, tshape)
        self._refuse_off_gpu("distill_loss", batch, images, tokens, vn, (("teacher_logits", tl), ("given", given)))
        if tl.stride(1) != 1 or tl.stride(0) % 4 or tl.data_ptr() % 16:
            tl = tl.contiguous()
        head = mage_train.DistillHead(tokens.contiguous(), teacher=tl, temperature=float(temperature), mode=self._DISTILL_MODES[mode],
                                      given=None if given is None else given.reshape(-1))
        with torch.cuda.device(images.device):
            loss, (info, res) = self._run_head(batch, head)
            self.last_distill_token_kl = res["row_kl"].view(tshape)
            ops.check_device_errors(images.device)
        return loss, info

    @torch.no_grad()
    def video_metrics(self, video, target, data_range: float = 2.0) -> dict:
        """Per-frame quality of `video` against `target`, both fp32 [B, T, C, H, W] on the model's GPU: {'mse', 'psnr', 'ssim'}, fp32 [B, T]
        each (mage_video_metrics, include/mage_hip_ext.h: the standard 11 x 11 Gaussian-window SSIM over the valid region, PSNR = 10 log10(
        data_range^2 / mse), +inf for identical frames).  data_range is the span of the pixel values: the models' frames lie in (-1, 1), so
        2.0.  Works for any model (use_cids or not): it only looks at frames.  Either side may be a view along the frame axis, e.g.
        batch['images'][:, 1:]."""
        for name, x in (("video", video), ("target", target)):
            if not (torch.is_tensor(x) and x.dim() == 5 and x.dtype == F32 and x.numel() > 0):
                raise ValueError(f"video_metrics: {name} must be a non-empty fp32 [B, T, C, H, W] tensor")
        if tuple(video.shape) != tuple(target.shape):
            raise ValueError(f"video_metrics: video {list(video.shape)} and target {list(target.shape)} must have the same shape")
        if video.shape[-2] < 11 or video.shape[-1] < 11:
            raise ValueError(f"video_metrics: SSIM's 11 x 11 window needs H and W >= 11, got {video.shape[-2]} x {video.shape[-1]}")
        dr = float(data_range)
        if not (math.isfinite(dr) and dr > 0 and dr < 3.4e38):
            raise ValueError(f"video_metrics: data_range must be finite and > 0, got {data_range}")
        try:
            _need_gpu(video, "MAGE.video_metrics")
            _need_gpu(target, "MAGE.video_metrics")
        except RuntimeError as e:                        # (a refusal like the ones above: the same words, as a ValueError)
            raise ValueError(str(e)) from None
        if video.device != target.device:
            raise ValueError("video_metrics: video and target must be on the same GPU")
        with torch.cuda.device(video.device):
            video, target = (x if ops._frames_ok(x) else x.contiguous() for x in (video, target))
            return ops.video_metrics(video, target, data_range=dr)

    _ROLLOUT_REWARDS = ("ssim", "psnr", "neg_mse")

    @torch.no_grad()
    def rollout(self, batch, candidates: int, reward="ssim", normalize="std", eps: float = 1e-6, reference: Optional["MAGE"] = None,
                noise: str = "clip", pairs: Optional[str] = None, context: int = 1, known_tokens=None, credit: str = "clip",
                gamma: float = 1.0) -> dict:
        """What policy_loss consumes, from the model's own samples: `candidates` = N >= 2 sampled continuations of every clip of the batch
        under the sampler set_sampling describes, ALL of them kept and decoded (set_sampling(candidates=N) keeps only the likeliest), each
        rewarded on the device, and the rewards turned into group-relative advantages:
            out = m.rollout(batch, 8); loss, info = m.policy_loss(out['batch'], out['tokens'], out['advantages'], out['behaviour_logprobs'])
        batch is autoregressive_generate's ('sample_seed' int64 [B] optional: candidate c of a clip draws with seed + c, so candidate 0 is
        the candidates = 1 sample).  reward: 'ssim', 'psnr' or 'neg_mse' -- the mean over the L-1 generated frames of that metric against
        frames 1 .. L-1 of batch['images'], which must then hold all L frames (mage_video_metrics, data_range 2) -- or a callable
        (video [B*N, L, C, H, W], batch) -> fp32 [B*N] on the GPU, one reward per clip (batch: the returned one).  normalize: 'std'
        ((r - mean) / (std + eps) over a clip's N candidates), 'mean' (r - mean) or None (the rewards themselves) (mage_group_advantages; a
        group holding a non-finite reward -- a PSNR of identical frames -- gets NaN advantages, unchecked: a check would be a sync).
        Returns {'video' [B*N, L, C, H, W], 'tokens' int64 [B*N, L-1, h, w], 'behaviour_logprobs' fp32 like tokens (the policy
        log-probabilities: last_token_policy_logprobs of a generation), 'token_logprobs' (the model's, temperature 1, unfiltered), 'rewards'
        fp32 [B, N], 'advantages' fp32 [B*N], 'frame_metrics' {'mse', 'psnr', 'ssim'} fp32 [B*N, L-1] each (None for a callable reward),
        'seeds' int64 [B*N], 'batch': the input with every per-clip tensor repeated N times along dim 0, 'images' cut to frame 0 (all
        policy_loss reads)}; row b*N + c is candidate c of clip b throughout.
        reference (another MAGE of the same configuration on the same GPU, e.g. a frozen copy taken before fine-tuning): the result gains
        'reference_logprobs' = reference.token_policy_logprobs(out['batch'], out['tokens']) under THIS model's sampling settings (set on the
        reference for the call; its own settings and last_* results are restored) -- policy_loss' reference_logprobs.
        noise (randomness=True models; the generation-time noise z is part of what the policy is conditioned on): 'clip' (the default) --
        one draw per clip shared by its N candidates, from batch['video_noise'], batch['noise_seed'] or torch.randn as in
        autoregressive_generate; 'candidate' -- candidate c of clip b draws its own noise with mage_video_noise under the seed that drives
        its sampler, sample_seed[b] + c (the two streams of one seed are disjoint; the text and MA encoders still run once per clip, the
        noise convolution, ADAIN and the speed term on the B*N rows), refused together with batch['video_noise'] and on a model without
        the branch.  Either way the result carries 'video_noise' fp32 [B*N, 64, h, w], also as out['batch']['video_noise']: the
        policy_loss call above -- and the reference's scoring -- condition on the noise the tokens were drawn under.
        pairs='best_worst': the result gains 'pairs' int64 [B, 2], rows into the B*N candidates -- every clip's highest-reward candidate as
        the chosen one and its lowest-reward candidate as the rejected one, built on the device; a clip whose candidates all earned the
        same reward gives (i, i), which preference_loss treats as no preference (zero gradient).  With reference as well the result also
        gains 'reference_clip_logprobs' = reference.clip_logprobs(out['batch'], out['tokens']) (fp32 [B*N]), so that
            out = m.rollout(batch, 8, reference=ref, pairs='best_worst')
            loss, info = m.preference_loss(out['batch'], out['tokens'], out['pairs'], out['reference_clip_logprobs'])
        runs as written.  Without pairs the call is the one it was, launch for launch.
        context=k (set_context's range; 1: off) and known_tokens (int64 [B, L-1, h, w], negative: free; batch['known_tokens']' layout):
        every candidate continues frames 0 .. k-1 of batch['images'] and holds the given tokens, by generation's own mechanism (the model's
        set_context setting is put back afterwards, as the sampler settings are).  The result gains 'given' (bool [B*N, L-1, h, w]: the slots
        that were given, policy_loss' given=; None without either argument); 'tokens' hold the given tokens there and
        'behaviour_logprobs' / 'token_logprobs' 0; out['batch'] carries neither key, so that
            out = m.rollout(batch, 8, context=4, reference=ref)
            loss, info = m.policy_loss(out['batch'], out['tokens'], out['advantages'], out['behaviour_logprobs'],
                                       reference_logprobs=out['reference_logprobs'], kl_coef=0.1, given=out['given'])
        runs as written; the reference's scores leave the given slots out alike.  Under context=k the video holds the k given frames
        verbatim and the built-in rewards average over the generated frames k .. L-1 alone ('frame_metrics' is [B*N, L-k]: the given frames
        would add a constant); with known_tokens alone all L-1 frames count.
        credit='frame' (with gamma in [0, 1]; the default 'clip' is everything above, launch for launch, and takes no gamma but 1): a
        frame's tokens are drawn given the earlier frames only, so they are credited with their own frame's reward and the later ones',
        not with the clip's.  'returns' (fp32 [B*N, L-k]) holds every generated frame's discounted reward-to-go over L-k, G[t] = (r[t] +
        gamma r[t+1] + gamma^2 r[t+2] + ...) / (L-k), and 'advantages' becomes fp32 [B*N, L-1] in the layout of tokens and given (slot i is
        frame i+1; the slots of given frames hold +0): each return against the same frame of its clip's N candidates, as normalize says
        (mage_frame_advantages; None: the returns themselves) -- policy_loss takes that shape as it stands.  'rewards' stays the
        per-candidate mean and pairs= its best and worst.  A callable reward must then return fp32 [B*N, L-k], one reward per generated
        frame.  Generation does not depend on credit: the same seeds give the same tokens.
        One eager pass over B*N rows behind one prologue per clip, in either ar_mode: no graph replay and no multi-stream grouping
        (use_graph and streams are ignored).  The model's set_sampling / set_logprobs settings and every last_* result are left as found."""
        self._refuse_guided("rollout")
        self._refuse_known("rollout", batch)
        if noise not in ("clip", "candidate"):
            raise ValueError(f"rollout: noise must be 'clip' or 'candidate', got {noise!r}")
        if noise == "candidate":
            if not self.randomness:
                raise ValueError("rollout: noise='candidate' needs the randomness branch; this model has none (randomness=False): there is "
                                 "no generation-time noise to draw per candidate")
            if batch.get("video_noise") is not None:
                raise ValueError("rollout: noise='candidate' draws every candidate's noise from its seed; batch['video_noise'] holds one "
                                 "tensor per clip and cannot describe N candidates -- drop it, or use noise='clip'")
        if pairs not in (None, "best_worst"):
            raise ValueError(f"rollout: pairs must be 'best_worst' or None, got {pairs!r}")
        if credit not in ("clip", "frame"):
            raise ValueError(f"rollout: credit must be 'clip' or 'frame', got {credit!r}")
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not 0.0 <= gamma <= 1.0:
            raise ValueError(f"rollout: gamma must be a number in [0, 1], got {gamma!r}")
        if credit == "clip" and gamma != 1:
            raise ValueError(f"rollout: gamma={gamma!r} discounts per-frame returns: it needs credit='frame' (credit='clip' averages the frames)")
        if not self.use_cids:
            raise ValueError("rollout: a use_cids=False (MAGE+) model regresses continuous latents; it has no tokens to sample")
        if self.sampling is None:
            raise ValueError("rollout: candidates are drawn by the sampler: switch sampling on with set_sampling first")
        if isinstance(candidates, bool) or not isinstance(candidates, int) or candidates < 2:
            raise ValueError(f"rollout: candidates must be an integer >= 2 (a group of one has no relative advantage), got {candidates!r}")
        if not (callable(reward) or reward in self._ROLLOUT_REWARDS):
            raise ValueError(f"rollout: reward must be one of {list(self._ROLLOUT_REWARDS)} or a callable, got {reward!r}")
        if normalize not in ("std", "mean", None):
            raise ValueError(f"rollout: normalize must be 'std', 'mean' or None, got {normalize!r}")
        if not (isinstance(eps, (int, float)) and math.isfinite(eps) and 0 <= eps < 3.4e38):
            raise ValueError(f"rollout: eps must be finite and >= 0, got {eps!r}")
        N, L = int(candidates), self.frames_length
        images = batch["images"]
        if not (torch.is_tensor(images) and images.dim() == 5 and images.shape[0] >= 1 and images.shape[1] >= 1):
            raise ValueError("rollout: batch['images'] must be [B, >= 1, C, H, W]")
        if isinstance(context, bool) or not isinstance(context, int) or not 1 <= context <= L - 1:
            raise ValueError(f"rollout: context must be an integer in [1, {L - 1}] (frames_length - 1), got {context!r}")
        if images.shape[1] < context:
            raise ValueError(f"rollout: context={context} continues that many frames; batch['images'] holds {images.shape[1]}")
        if known_tokens is not None:
            kshape = (images.shape[0], L - 1, self.image_resolution, self.image_resolution)
            if not (torch.is_tensor(known_tokens) and known_tokens.dtype == torch.int64 and tuple(known_tokens.shape) == kshape):
                raise ValueError(f"rollout: known_tokens must be int64 {list(kshape)} (negative: free)")
            if not (known_tokens.is_cuda and known_tokens.device == images.device):
                raise ValueError("rollout: known_tokens must be on the model's ROCm GPU (there is no CPU / PyTorch fallback)")
        masked = context > 1 or known_tokens is not None
        builtin = not callable(reward)
        per_frame = credit == "frame"
        if builtin and not (images.shape[1] >= L and images.dtype == F32 and min(images.shape[-2:]) >= 11):
            raise ValueError(f"rollout: reward '{reward}' compares with the ground truth: batch['images'] must be fp32 [B, {L}, C, H, W] with "
                             "H, W >= 11")
        for name, x in batch.items():
            if torch.is_tensor(x) and name not in ("sample_seed", "noise_seed") and not (x.is_cuda and x.device == images.device):
                raise ValueError(f"rollout: batch['{name}'] must be on the model's ROCm GPU (there is no CPU / PyTorch fallback)")
        if reference is not None:
            if not (isinstance(reference, MAGE) and reference.use_cids):
                raise ValueError("rollout: reference must be a use_cids=True MAGE model (it scores tokens)")
            for a in ("codebook_size", "frames_length", "image_resolution"):
                if getattr(reference, a) != getattr(self, a):
                    raise ValueError(f"rollout: the reference model's {a}={getattr(reference, a)} differs from this model's {getattr(self, a)}")
            if next(reference.parameters()).device != images.device:
                raise ValueError("rollout: the reference model must be on the same GPU as the batch")
        Bc = images.shape[0]
        settings = (self.candidates, self.logprobs, self.logprob_policy, self.logprob_entropy, self.context_frames)
        with self._last_results_kept():
            try:
                self.candidates, self.logprobs, self.logprob_policy, self.logprob_entropy = N, True, True, False
                b = self._sample_seeds(self._noise_seeds(batch))
                if masked:                                # generation's own path: the setting and the batch key, for this call
                    self.context_frames = context
                    b = self._known_inputs(b if known_tokens is None else {**b, "known_tokens": known_tokens})
                with torch.cuda.device(images.device), weights_frozen():
                    self.last_video_noise = None
                    out = self._generate_one(b, keep_all=True, candidate_noise=noise == "candidate")
                    rep = {k: (v.repeat_interleave(N, 0) if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == Bc else v) for k, v in batch.items()
                           if k not in ("images", "sample_seed", "noise_seed")}
                    out["batch"] = {**rep, "images": out.pop("first"), "sample_seed": out["seeds"]}      # (the candidates' seeds: sample_seed[b] + c)
                    if self.randomness:                      # the noise every row was drawn under: what policy_loss conditions on
                        vn = self.last_video_noise
                        out["video_noise"] = out["batch"]["video_noise"] = vn if vn.shape[0] == Bc * N else vn.repeat_interleave(N, 0)
                    video = out["video"]
                    out["given"] = self.last_known_mask.repeat_interleave(N, 0) if masked else None
                    if builtin:                              # the generated frames: context .. L-1 (the given ones came back verbatim)
                        gen = video[:, context:] if video.dtype == F32 else video[:, context:].float()
                        fm = out["frame_metrics"] = ops.video_metrics(gen, images[:, context:L], tgt_div=N, data_range=2.0)
                        fr = fm[reward] if reward != "neg_mse" else -fm["mse"]
                    else:
                        out["frame_metrics"] = None
                        fr = reward(video, out["batch"])
                        want = (Bc * N, L - context) if per_frame else (Bc * N,)
                        if not (torch.is_tensor(fr) and fr.dtype == F32 and tuple(fr.shape) == want and fr.device == images.device):
                            raise ValueError(f"rollout: the reward callable must return fp32 {list(want)} on the model's GPU"
                                             + (" (credit='frame': one reward per generated frame)" if per_frame else ""))
                        fr = fr.contiguous()
                    out["rewards"], adv = ops.group_advantages(fr, groups=Bc, n_cand=N, mode=1 if normalize == "std" else 0, eps=float(eps))
                    if per_frame:                            # slot i is frame i + 1: the generated frames start at slot context - 1
                        out["returns"], adv = ops.frame_advantages(fr, groups=Bc, n_cand=N, gamma=float(gamma), mode=1 if normalize == "std" else 0,
                                                                   eps=float(eps), slots=L - 1, slot_off=context - 1)
                        if normalize is None:                # (the slots of the given frames stay the kernel's +0)
                            adv[:, context - 1:] = out["returns"]
                        out["advantages"] = adv
                    else:
                        out["advantages"] = adv if normalize is not None else out["rewards"].reshape(-1).clone()
                    giv = {"given": out["given"]} if masked else {}
                    if reference is not None:
                        theirs = (reference.sampling, reference.candidates)
                        try:
                            reference.sampling, reference.candidates = self.sampling, 1
                            out["reference_logprobs"] = reference.token_policy_logprobs(out["batch"], out["tokens"], **giv)
                        finally:
                            reference.sampling, reference.candidates = theirs
                    if pairs is not None:
                        rw = out["rewards"].view(Bc, N)
                        hi, lo = rw.argmax(1), rw.argmin(1)
                        lo = torch.where(rw.amax(1) == rw.amin(1), hi, lo)           # all rewards equal: (i, i), no preference
                        base = torch.arange(Bc, device=images.device, dtype=torch.int64) * N
                        out["pairs"] = torch.stack([base + hi, base + lo], 1).contiguous()
                        if reference is not None:
                            out["reference_clip_logprobs"] = reference.clip_logprobs(out["batch"], out["tokens"], **giv)
                    ops.check_device_errors(images.device)
            finally:
                self.candidates, self.logprobs, self.logprob_policy, self.logprob_entropy, self.context_frames = settings
        return out

    def _sample_seeds(self, batch) -> dict:
        """The batch with its 'sample_seed' entry as int64 [B] on the images' device (drawn here when absent); kept as last_sample_seeds."""
        images = batch["images"]
        B = images.shape[0]
        seeds = batch.get("sample_seed")
        if seeds is None:
            seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, (B,), dtype=torch.int64)
        seeds = torch.as_tensor(seeds)
        if seeds.dtype != torch.int64 or tuple(seeds.shape) != (B,):
            raise ValueError(f"batch['sample_seed'] must be int64 [{B}], got {seeds.dtype} {tuple(seeds.shape)}")
        seeds = seeds.to(images.device).contiguous()
        self.last_sample_seeds = seeds
        return {**batch, "sample_seed": seeds}

    def _noise_seeds(self, batch) -> dict:
        """The batch with its optional 'noise_seed' entry as int64 [B] on the images' device; without it on a model that has no randomness
        branch (there it is ignored: the call, its graph key included, is the one without the entry)."""
        if "noise_seed" not in batch:
            return batch
        if not self.randomness:
            return {k: v for k, v in batch.items() if k != "noise_seed"}
        images = batch["images"]
        B = images.shape[0]
        seeds = torch.as_tensor(batch["noise_seed"])
        if seeds.dtype != torch.int64 or tuple(seeds.shape) != (B,):
            raise ValueError(f"batch['noise_seed'] must be int64 [{B}], got {seeds.dtype} {tuple(seeds.shape)}")
        return {**batch, "noise_seed": seeds.to(images.device).contiguous()}

    def _dt(self) -> torch.dtype:
        return PRECISIONS[self.precision][0]

    def _sk(self) -> int:
        """Split kind of the fast parity modes (0 otherwise, and for a decoder width the split GEMM does not take)."""
        gm = self.generate_model
        return gm.split_kind if getattr(gm, "_split_on", None) and gm._split_on() else 0

    def _build(self):
        d: Dict[str, torch.Tensor] = {}
        if self.use_cids:
            d["emb"] = self.visual_token_embedding.weight.float().contiguous()
        else:
            d["emb_lin.w"] = self.visual_token_embedding.weight.float().contiguous()       # [C, embed_dim]
            d["emb_lin.b"] = self.visual_token_embedding.bias.float().contiguous()
        cw = _conv_w(self.conv[0])
        d["conv.f32"], d["conv.bf16"] = cw, cw.to(BF16)
        R, Cc = self.image_resolution, self.vision_width
        d["hwpos"] = (self.H_positional_embedding.float() + self.W_positional_embedding.float()).reshape(R * R, Cc).contiguous()
        d["speed"] = self.speed_embedding.float().reshape(-1).contiguous()
        if self.randomness:
            d["conv_d2"] = _conv_w(self.conv_d2)
            # MAGE.forward only: the Conv3d video prior, one [Cout, 3, 3, Cin] slice per temporal tap, and the two 3x3 heads
            for i, blk in enumerate(self.conv3d):
                for nm, conv in (("c1", blk.conv1), ("c2", blk.conv2), ("ds", blk.downsample[0])):
                    w = conv.weight.float()                                                # [Cout, Cin, kd, kh, kw]
                    for kd in range(3):
                        d[f"p{i}.{nm}.{kd}"] = w[:, :, kd].permute(0, 2, 3, 1).contiguous()
                for nm, gn in (("g1", blk.bn1), ("g2", blk.bn2), ("gd", blk.downsample[1])):
                    d[f"p{i}.{nm}.w"], d[f"p{i}.{nm}.b"] = gn.weight.float().contiguous(), gn.bias.float().contiguous()
            for nm, conv in (("mu2", self.conv_mu2), ("var2", self.conv_var2)):
                d[nm + ".w"], d[nm + ".b"] = _conv_w(conv), conv.bias.float().contiguous()
        return d

    # ------------------------------------------------------------------ first stage wrappers (mage_model.py:530-567)
    @torch.no_grad()
    def first_stage_encode(self, x):
        """[B, T, C, H, W] -> token ids int64 [B, T, h, w]."""
        out = self.get_first_stage_encoding(self.first_stage_model.encode(x.reshape(-1, *x.shape[-3:])))
        return out.view(*x.shape[:-3], *out.shape[1:]).contiguous()

    def get_first_stage_encoding(self, encoder_posterior):
        if isinstance(encoder_posterior, torch.Tensor):
            return encoder_posterior
        if hasattr(encoder_posterior, "sample"):          # ldm DiagonalGaussianDistribution (mage_model.py:543-544)
            return encoder_posterior.sample()
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    @torch.no_grad()
    def first_stage_decode(self, x):
        """[B, T, h, w] ids -> [B, T, C, H, W]."""
        dec = getattr(self.first_stage_model, "_decode_nocheck", self.first_stage_model.decode)   # one error check per public call
        out = dec(x.reshape(-1, *x.shape[-2:]) if self.use_cids else x.reshape(-1, *x.shape[-3:]))
        return out.view(*x.shape[:2], *out.shape[1:]).contiguous()

    # ------------------------------------------------------------------ shared pieces
    def _frame_tables(self):
        """conv3x3 over token EMBEDDINGS has only codebook_size distinct input vectors (mage_model.py:581,586-588): by linearity
            conv(emb(ids))[p] = sum_taps T[tap][ids[p + tap]],   T[tap][code] = W_tap emb[code]        [9, K, C] fp32
        and the decoder's in_linear applied to it (+ H/W positions, + bias) folds in as well:
            T2[tap][code] = W_in T[tap][code],   P2[p] = W_in (H_pos + W_pos)[p] + b_in               (mage_model.py:375-376)
        Built once per weights on the fp32 MFMA kernels (a derived cache like the folded BatchNorm vectors); 9.4 MB each at the MNIST
        config: resident in L2 / Infinity Cache.  The per-call work becomes a gather-sum (mage_table_conv): 0 matrix-core FLOPs for
        the 2*9*C^2 + 2*C^2 per pixel the reference spends (11 % of a decoder iteration), fp32-exact sums in every precision mode.
        Returns the cache dict with 'ft.T', 'ft.T2', 'ft.P2' (None when not applicable: use_cids=False, config frame_table = False); `self.frame_table = False`
        switches the callers back to the convolution GEMM + in_linear (the reference's operation order) at any time."""
        d = self._derived.get(self._build)
        if not config.get().frame_table:
            # switched off for this call only: the decision is NOT cached (a `config.override(frame_table=False)` block must not leave the tables
            # off behind it -- ADVICE r5), tables built earlier stay in the cache for when the switch is back on
            return {**d, "ft.T": None, "ft.T2": None, "ft.P2": None}
        if "ft.T" in d:
            return d
        R, Cc, Kc = self.image_resolution, self.vision_width, self.codebook_size
        gm = self.generate_model
        ok = (self.use_cids and Cc % 4 == 0
              and 9 * Kc * max(Cc, getattr(gm, "model_channels", Cc)) * 4 <= (256 << 20) and "emb" in d and d["emb"].is_cuda
              and getattr(gm, "in_channels", None) == Cc and hasattr(gm, "_build"))
        if not ok:                                  # structural: cached with the weights
            d["ft.T"] = d["ft.T2"] = d["ft.P2"] = None
            return d
        gd = gm._derived.get(gm._build)
        Cd = gm.model_channels
        emb, dev = d["emb"], d["emb"].device
        cw = d["conv.f32"].view(Cc, 9, Cc)
        T = torch.empty(9, Kc, Cc, device=dev, dtype=F32)
        T2 = torch.empty(9, Kc, Cd, device=dev, dtype=F32)
        w_in = gd["in_linear.f32"]
        for tap in range(9):
            ops.gemm(emb, cw[:, tap].contiguous(), T[tap], M=Kc, N=Cc, K=Cc, lda=Cc, ldy=Cc)
            ops.gemm(T[tap], w_in, T2[tap], M=Kc, N=Cd, K=Cc, lda=Cc, ldy=Cd)
        P2 = ops.gemm(d["hwpos"], w_in, torch.empty(R * R, Cd, device=dev, dtype=F32), M=R * R, N=Cd, K=Cc, lda=Cc, ldy=Cd, bias=gd.get("in_linear.b"))
        d["ft.T"], d["ft.T2"], d["ft.P2"] = T, T2, P2
        return d

    def _frame_source(self, tokens: torch.Tensor, dt: torch.dtype):
        """What the decoder gets for its frame slots: FrameTokens (table sum, in_linear folded) or the convolved features."""
        ft = self._frame_tables()
        if ft["ft.T2"] is not None and self.frame_table:
            T2 = ft["ft.T2"]
            if dt in HALF_TYPES and self._sk() == 0:
                # bf16 / f16 mode: the table itself in that type (half the L2 / Infinity-Cache bytes per gathered row; entries rounded once,
                # sums and positions stay fp32 -- the same class of error as the 16-bit operands of the convolution it replaces)
                if "ft.T2" + _sfx(dt) not in ft:
                    ft["ft.T2" + _sfx(dt)] = T2.to(dt)
                T2 = ft["ft.T2" + _sfx(dt)]
            return FrameTokens(tokens.reshape(-1, self.image_resolution ** 2), T2, ft["ft.P2"], self.image_resolution)
        return self._frame_features(tokens, dt, split=True)

    def _frame_features(self, tokens: torch.Tensor, dt: torch.dtype, split: bool = False) -> torch.Tensor:
        """ids [n, hw] -> conv3x3(embedding) + (H_pos + W_pos) as rows [n*hw, C] (mage_model.py:581,586-588,674-676).

        bf16 mode: the embedding rows are written into the interior of a zero-padded (R+2) x (R+2) frame buffer, so that the
        convolution is the padded-taps form of mage_gemm (every tap a valid row: the 8-phase ping-pong kernel with one scalar
        offset per K slab, the positional table loaded into the accumulators) instead of the generic per-lane gather.  The buffer
        is kept between calls: its border is written once (zeros), its interior on every call."""
        d = self._derived.get(self._build)
        R, Cc = self.image_resolution, self.vision_width
        n = tokens.numel() // (R * R)
        if dt == F32 and not split:
            ft = self._frame_tables()
            if ft["ft.T"] is not None and self.frame_table:                                                  # the once-per-clip prologue: fp32 features
                return ops.table_conv(tokens.reshape(-1).contiguous(), ft["ft.T"], torch.empty(n * R * R, Cc, device=tokens.device, dtype=F32),
                                      n_img=n, H=R, W=R, pos=d["hwpos"])
        sk = self._sk() if split else 0
        if sk and Cc % 256 == 0 and (n * R * R) % 256 == 0 and self.generate_model._taps_ok(n * R * R):
            # fast parity modes: the same padded-taps convolution on split-precision operands; the features leave as split rows
            # (in_linear's A operand)
            P = R + 2
            key = (n, str(tokens.device), torch.cuda.current_stream(tokens.device).cuda_stream, sk)
            pad = self._pad_frames.get(key)
            if pad is None:
                if len(self._pad_frames) > 8:
                    self._pad_frames.clear()
                pad = self._pad_frames[key] = ops.split_empty(n * P * P + 1, Cc, sk, tokens.device, zero=True)
            ops.embedding(tokens.reshape(-1), d["emb"], pad, group=R * R, group_stride=P * P, off=P + 1, inner=R, inner_stride=P, split_kind=sk)
            out = ops.split_empty(n * R * R, Cc, sk, tokens.device)
            return ops.gemm(pad, _wsplit(d, "conv", sk), out, M=n * R * R, N=Cc, K=9 * Cc, lda=2 * Cc, ldy=2 * Cc, out_h=R, out_w=R, in_h=P,
                            in_w=P, a_img_stride=P * P, taps_h=3, taps_w=3, cin=Cc, rowadd=d["hwpos"], rowadd_div=1, rowadd_mod=R * R,
                            split_kind=sk, y_split=True)
        if dt == F32 or Cc % 64:
            emb = ops.embedding(tokens.reshape(-1), d["emb"], torch.empty(n * R * R, Cc, device=tokens.device, dtype=dt))
            return VectorQuantizedVAE._conv(emb, _wdt(d, "conv", dt), torch.empty_like(emb), n_img=n, H=R, W=R, cin=Cc, cout=Cc,
                                            k=3, rowadd=d["hwpos"], rowadd_div=1, rowadd_mod=R * R)
        P = R + 2
        key = (n, str(tokens.device), torch.cuda.current_stream(tokens.device).cuda_stream if tokens.is_cuda else 0)
        pad = self._pad_frames.get(key)
        if pad is None:
            if len(self._pad_frames) > 8:
                self._pad_frames.clear()
            pad = self._pad_frames[key] = torch.zeros((n * P * P + 1) * Cc, device=tokens.device, dtype=dt).view(-1, Cc)
        ops.embedding(tokens.reshape(-1), d["emb"], pad, group=R * R, group_stride=P * P, off=P + 1, inner=R, inner_stride=P)
        out = torch.empty(n * R * R, Cc, device=tokens.device, dtype=dt)
        return ops.gemm(pad, _wdt(d, "conv", dt), out, M=n * R * R, N=Cc, K=9 * Cc, lda=Cc, ldy=Cc, out_h=R, out_w=R, in_h=P, in_w=P,
                        a_img_stride=P * P, taps_h=3, taps_w=3, cin=Cc, stride=1, dy0=0, dx0=0, rowadd=d["hwpos"], rowadd_div=1,
                        rowadd_mod=R * R)

    def _frame_features_latent(self, lat: torch.Tensor, ld: int, dt: torch.dtype) -> torch.Tensor:
        """use_cids=False: latents as fp32 rows [n*hw, ld] (first embed_dim columns valid) -> Linear(embed_dim -> C)
        (mage_model.py:483,583,646) -> conv3x3 + (H_pos + W_pos), rows [n*hw, C]."""
        d = self._derived.get(self._build)
        R, Cc = self.image_resolution, self.vision_width
        rows = lat.numel() // ld
        E = d["emb_lin.w"].shape[1]
        # K = 4: fp32 MFMA path; it writes fp32 or bf16 rows -- the f16 mode takes fp32 rows through one cast pass
        emb = ops.gemm(lat, d["emb_lin.w"], torch.empty(rows, Cc, device=lat.device, dtype=F32 if dt == F16 else dt), M=rows, N=Cc, K=E, lda=ld,
                       ldy=Cc, bias=d["emb_lin.b"])
        if dt == F16:
            emb = ops.cast(emb, torch.empty(rows, Cc, device=lat.device, dtype=F16))
        return VectorQuantizedVAE._conv(emb, _wdt(d, "conv", dt), torch.empty_like(emb), n_img=rows // (R * R), H=R, W=R, cin=Cc,
                                        cout=Cc, k=3, rowadd=d["hwpos"], rowadd_div=1, rowadd_mod=R * R)

    def _motion_anchor(self, tok0: torch.Tensor, batch, noise: Optional[torch.Tensor], first: Optional[torch.Tensor] = None,
                       video_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Once-per-clip prologue, fp32 (mage_model.py:648-668 / 586-613): rows [B*hw, C].  video_rows [B*hw, 64] (forward with
        randomness: the reparameterised video prior, before conv_d2) replaces the sampled noise."""
        return self._anchor_tail(self._anchor_head(tok0, batch, first), batch, noise, batch["text"].shape[0], video_rows=video_rows)

    def _anchor_head(self, tok0: torch.Tensor, batch, first: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The part of the prologue that does not see the noise: text encoder and MA encoder over frame 0, rows [B*hw, C]."""
        B = batch["text"].shape[0]
        R = self.image_resolution
        if first is None:
            first = self._frame_features(tok0, F32)                                           # [B*hw, C]
        txt = self.text_encoder(batch["text"])                                                # [B, S, C]
        S = txt.shape[1]
        return self.ma_encoder._run(first, txt.reshape(B * S, -1), B=B, nq=R * R, nk=S, seq_first=False)

    def _anchor_tail(self, ma: torch.Tensor, batch, noise: Optional[torch.Tensor], B: int, video_rows: Optional[torch.Tensor] = None,
                     noise_seed: Optional[torch.Tensor] = None, speed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rest of it over B clips' rows of ma (rollout(noise='candidate'): B is clips x candidates): conv_d2 of the noise, ADAIN, the
        speed term.  The noise is `noise` [B,64,h,w] when given, else mage_video_noise under noise_seed / batch['noise_seed'] (int64 [B]:
        the rows come straight from the kernel, no permute copy), else torch.randn (mage_model.py:661); last_video_noise keeps it."""
        d = self._derived.get(self._build)
        R, Cc = self.image_resolution, self.vision_width
        if self.randomness:
            if video_rows is not None:                                                        # forward(): reparameterised prior
                nz = video_rows
            else:
                if noise_seed is None:
                    noise_seed = batch.get("noise_seed")
                if noise is None and noise_seed is not None:
                    noise, nz = ops.video_noise(noise_seed, C=64, h=R, w=R)
                else:
                    if noise is None:
                        noise = torch.randn([B, 64, R, R], device=ma.device)                  # mage_model.py:661
                    noise = noise.float()
                    nz = noise.permute(0, 2, 3, 1).reshape(B * R * R, 64).contiguous()
                self.last_video_noise = noise
            y = VectorQuantizedVAE._conv(nz, d["conv_d2"], torch.empty(B * R * R, Cc, device=ma.device, dtype=F32), n_img=B,
                                         H=R, W=R, cin=64, cout=Cc, k=3)
            ma = self.adain._run(ma, y, B, R, R)
        if speed is None and "speed" in batch:
            speed = batch["speed"]
        if speed is not None:
            ops.add_scaled_rowvec(ma, speed.float().contiguous(), d["speed"], B=B, P=R * R, Cc=Cc)
        return ma

    # ------------------------------------------------------------------ sampling (mage_model.py:641-693)
    @torch.no_grad()
    def autoregressive_generate(self, batch):
        """batch {'images' [B,L,C,H,W] (only frame 0 is read), 'text' int64 [B,S], 'speed' [B] optional,
        'video_noise' [B,64,h,w] optional (injects the randomness-branch noise instead of torch.randn), 'sample_seed' int64 [B] optional
        (one seed per clip when set_sampling is on; drawn from torch's default CPU generator when absent, kept as last_sample_seeds)}
        -> [B,L,C,H,W].
        set_context(k): frames 0 .. k-1 of 'images' are read and given ('context_tokens' int64 [B,k,h,w] optional: their tokens, in place
        of the encode); 'known_tokens' int64 [B,L-1,h,w] optional: slot i is frame i+1, negative = free, anything else is held
        (set_context's docstring; last_known_mask tells which slots were given).

        With ``self.streams = n > 1`` the clips are processed as n independent groups on n HIP streams: clips never
        interact, so the results are bit-identical, and the HBM-bound kernels of one group (LayerNorm, attention, casts)
        run under the MFMA-bound GEMMs of the other instead of in front of them."""
        images = batch["images"]
        _need_gpu(images, "MAGE.autoregressive_generate")
        self.last_sample_seeds = None
        self._set_generation_results([None] * len(self._GENERATION_RESULTS))
        self._want_stats()                               # (refuses policy without sampling before anything runs)
        batch = self._noise_seeds(batch)
        if self.sampling is not None and self.use_cids:
            batch = self._sample_seeds(batch)            # before the graph path keys on the batch and copies it into its static inputs
        self.last_guidance_scale = None
        batch = self._guidance_inputs(batch)             # (likewise: the scales and the negative caption are inputs of a captured graph)
        batch = self._known_inputs(batch)                # (likewise the given tokens; refuses a wrong dtype or shape before anything runs)
        # (weights_frozen: no parameter changes during one inference call -- the derived caches validate once, not at each of their ~40 fetches)
        with torch.cuda.device(images.device), weights_frozen():
            ug = self._graph_auto(batch) if self.use_graph is None else bool(self.use_graph)
            # (clip groups on several streams are not captured: slower than one stream at every size, DESIGN finding 94)
            if ug and int(self.streams) == 1 and not torch.cuda.is_current_stream_capturing():
                out = self._generate_graphed(batch)
            else:
                self.last_call_mode = "eager"
                out = self._generate_eager(batch)
            ops.check_device_errors(images.device)        # e.g. a caption id >= vocab_size: the reference raises IndexError
        return out

    @torch.no_grad()
    def generate_long(self, batch, frames: int, overlap: int = 1, texts=None):
        """A video of `frames` >= frames_length frames as a chain of windows -> [B, frames, C, H, W].  Window 0 is
        autoregressive_generate(batch) as it stands (set_context included); window w >= 1 takes the tokens of the last `overlap` frames of
        window w-1 (1 <= overlap <= L-1) as its batch['context_tokens'] -- the hand-over stays on the device: no pixel decode or encode, no
        host decision -- so its frame 0, the motion anchor's input, is the oldest of them, and it adds L - overlap new frames.  The last
        window's surplus frames are dropped.
        texts: a sequence of one caption tensor [B, S] per window (default: batch['text'] for every window).  Window w samples with
        sample_seed + 1_000_003 * w (int64 wrap-around) and, where batch['noise_seed'] is given, draws its noise under noise_seed + w.
        Only new tokens are decoded.  last_tokens and every per-token last_* result are [B, frames-1, h, w], each frame's entry from the
        window that generated it; the per-clip totals are mage_clip_scores of those; last_video_noise is stacked per window
        [windows, B, 64, h, w]; last_logits is None.  candidates > 1, batch['known_tokens'] and a use_cids=False model are refused."""
        L = self.frames_length
        if not self.use_cids:
            raise ValueError("generate_long: a use_cids=False (MAGE+) model regresses continuous latents; it has no tokens to hand over")
        if self._n_cand() > 1:
            raise ValueError("generate_long: candidates > 1 is refused (a winner per window would be a host-side choice of what to hand over)")
        if "known_tokens" in batch:
            raise ValueError("generate_long: batch['known_tokens'] is refused (its slots are one window's)")
        for name, v, lo, hi in (("frames", frames, L, None), ("overlap", overlap, 1, L - 1)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
                raise ValueError(f"generate_long: {name} must be an integer in [{lo}, {'...' if hi is None else hi}], got {v!r}")
        step = L - overlap
        n_win = 1 + -(-(frames - L) // step)
        if texts is not None and len(texts) != n_win:
            raise ValueError(f"generate_long: texts must hold one caption tensor per window ({n_win}), got {len(texts)}")
        images = batch["images"]
        _need_gpu(images, "MAGE.generate_long")
        base = dict(batch)
        if self.sampling is not None:
            base = self._sample_seeds(base)              # drawn once when absent: every window derives its seeds from these
        seeds0, nseed0 = base.get("sample_seed"), base.get("noise_seed")
        k0 = self.context_frames
        videos, toks, masks, noises = [], [], [], []
        per_tok = {a: [] for a in ("last_token_logprobs",) + tuple(attr for _, attr in self._STATS_RESULTS)}
        try:
            for w in range(n_win):
                b = dict(base)
                if texts is not None:
                    b["text"] = texts[w]
                if w:
                    if seeds0 is not None:
                        b["sample_seed"] = seeds0 + 1_000_003 * w                              # (int64 tensors wrap around)
                    if nseed0 is not None:
                        b["noise_seed"] = torch.as_tensor(nseed0) + w
                    b["images"] = videos[-1][:, L - overlap:]                                # only its first `overlap` frames are read
                    b["context_tokens"] = self.last_tokens[:, L - 1 - overlap:].contiguous()  # slot i is frame i + 1
                    self.context_frames = overlap
                out = self.autoregressive_generate(b)
                new = slice(0, None) if w == 0 else slice(overlap - 1, None)                  # the slots this window generated
                videos.append(out)
                toks.append(self.last_tokens[:, new])
                masks.append(self.last_known_mask[:, new] if w == 0 and self.last_known_mask is not None else None)
                noises.append(self.last_video_noise)
                for a, col in per_tok.items():
                    t_ = getattr(self, a, None)
                    col.append(None if t_ is None else t_[:, new])
        finally:
            self.context_frames = k0
        B = images.shape[0]
        cat = lambda col: None if col[0] is None else torch.cat(col, 1)[:, :frames - 1].contiguous()      # noqa: E731
        self.last_tokens, self.last_logits = cat(toks), None
        for a, col in per_tok.items():
            setattr(self, a, cat(col))
        self.last_known_mask = None
        if masks[0] is not None:
            self.last_known_mask = torch.zeros(self.last_tokens.shape, device=images.device, dtype=torch.bool)
            self.last_known_mask[:, :L - 1] = masks[0]
        self.last_video_noise = None if noises[0] is None else torch.stack(noises, 0)
        self.last_sample_seeds = seeds0                   # window 0's: the seeds that reproduce the whole chain
        if self.last_token_logprobs is not None:
            self.last_clip_logprob = ops.clip_scores(self.last_token_logprobs, n_clips=B)[0].view(B)
        if self.last_token_policy_logprobs is not None:
            self.last_clip_policy_logprob = ops.clip_scores(self.last_token_policy_logprobs, n_clips=B)[0].view(B)
        return torch.cat([videos[0]] + [v[:, overlap:] for v in videos[1:]], 1)[:, :frames].contiguous()

    def _graph_auto(self, batch) -> bool:
        """use_graph = None: replay from a captured graph where the call is launch-bound -- up to 4 clips per call (the reference samples
        ONE, main_mage.py:205: ~870 launches of 3-15 µs; 13.7 ms eager vs 7.6 ms replayed per 16-frame clip), the VQ-token path only (an
        external latent first stage is not ours to capture), and not while per-launch profiling is on.  A guided call decodes 2 B clips."""
        images = batch["images"]
        clips = images.shape[0] * (2 if self._guided() else 1)
        return (self.use_cids and clips * self.image_resolution ** 2 <= 1024 and not ops.PROFILE.enabled
                and all(torch.is_tensor(v) for v in batch.values()) and config.get().auto_graph)

    def _graph_fingerprint(self, batch=None):
        """Everything besides shapes, precision, AR mode and weights that selects kernels: a captured graph replays only under the same."""
        fs = self.first_stage_model
        return (int(self.streams), bool(self.frame_table), self.generate_model._stream_bf16(), bool(getattr(self.ma_encoder, "mage_plus", False)),
                getattr(self.ma_encoder, "split_kind", 0), getattr(self.text_encoder, "split_kind", 0),
                tuple(str(getattr(fs, a, None)) for a in ("decode_dtype", "encode_split", "decode_split")),
                config.get(), tuple(sorted(config.lib_options().items())), self.sampling,
                self._want_logprobs(), self._n_cand(), bool(self.logprob_policy), bool(self.logprob_entropy),
                self._guided(),                          # (on / off selects the launches; the scales themselves are a batch tensor)
                self._ctx(), bool(self.context_prefill),                                     # (likewise: the given tokens are batch tensors)
                batch is not None and "known_tokens" in batch, batch is not None and "context_tokens" in batch)

    def _generate_eager(self, batch):
        if not self.use_cids:
            return self._generate_latent(batch)
        n = int(self.streams)
        if n > 1 and batch["images"].shape[0] >= 2 * n and batch["images"].shape[0] % n == 0:
            return self._generate_multistream(batch, n)
        return self._generate_one(batch)

    def _generate_graphed(self, batch):
        """HIP-graph replay of the whole call ("whole-loop residency").  The call is a fixed sequence of
        kernel launches on device-resident buffers -- no host decision depends on device data (the argmax of frame i is written
        into slot i+1 of the token buffer on the device) -- so one capture of the launch stream replays it with ONE host call
        instead of ~50 per AR iteration: the Python / ctypes launch loop (14 of 30 ms per call in incremental mode) disappears.
        First call with a given (shapes, precision, AR mode, weights): eager, which also builds every derived cache; second:
        captured on static copies of the inputs (all intermediates live in the graph's private pool: an arena that is never
        re-allocated); from then on: inputs are copied into the static buffers, the graph is replayed, the video and tokens are
        cloned out (last_logits too).  Same kernels, same order, same
        arithmetic: bit-identical to the eager call."""
        self._warm_derived()
        gens = tuple(getattr(m, "_derived").gen for m in (self, self.generate_model, self.ma_encoder, self.text_encoder,
                                                          getattr(self, "adain", None), self.first_stage_model)
                     if m is not None and hasattr(m, "_derived"))
        prof = ops.PROFILE.mode_key()
        self.last_call_mode = "eager"
        if prof != "off" and not ops.graph_events_supported(batch["images"].device):
            return self._generate_eager(batch)              # per-launch events wanted, but they cannot be captured here
        key = (tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(batch.items())), self.precision, self.ar_mode, gens, prof,
               str(batch["images"].device), self._graph_fingerprint(batch))
        ent = self._graphs.get(key)
        if ent is None:
            self._graphs = {k: v for k, v in self._graphs.items() if k[3] == gens}       # graphs of replaced weights are dead
            while len(self._graphs) >= 4:                                                # each graph owns an arena: keep the 4 newest shapes
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[key] = "warm" if self.use_graph else "warm2"
            return self._generate_eager(batch)
        if ent == "off":
            return self._generate_eager(batch)
        if ent == "warm2":                               # auto mode: a shape has to come back twice before it is worth a capture
            self._graphs[key] = "warm"
            return self._generate_eager(batch)
        if ent == "warm":
            static = {k: v.clone() for k, v in batch.items()}
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            saved = ops.PROFILE.capture_begin()
            # no cyclic garbage collection while the stream is capturing: a collection that frees device memory or another captured
            # graph in the middle of a capture (older models of the same process going away) aborts the process
            gc_was = gc.isenabled()
            gc.collect()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    out = self._generate_eager(static)
                    results = self._generation_results()
            except Exception:
                if self.use_graph:                       # asked for explicitly: loud
                    raise
                self._graphs[key] = "off"                # auto mode: this call shape cannot be captured here -- eager from now on
                torch.cuda.synchronize()
                return self._generate_eager(batch)
            finally:
                if gc_was:
                    gc.enable()
                recs = ops.PROFILE.capture_end(saved)
            ent = self._graphs[key] = {"g": g, "in": static, "out": out, "results": results, "recs": recs}
        else:
            for k, v in batch.items():
                ent["in"][k].copy_(v)
        ent["g"].replay()
        self.last_call_mode = "graph"
        if ent["recs"] and ops.PROFILE.enabled:
            torch.cuda.current_stream().synchronize()
            ops.PROFILE.absorb(ent["recs"])
        # every result is cloned like the output: graph replay is the DEFAULT for small calls (use_graph = None), and a caller that keeps
        # last_logits across two generations must not find the first one overwritten by the second (0.5 MB per clip at cfg2)
        self._set_generation_results([None if t_ is None else t_.clone() for t_ in ent["results"]])
        return ent["out"].clone()

    _LOGPROB_RESULTS = ("last_token_logprobs", "last_clip_logprob", "last_candidate_scores", "last_candidate_index",
                        "last_token_policy_logprobs", "last_clip_policy_logprob", "last_token_kept", "last_candidate_policy_scores",
                        "last_token_entropy", "last_token_policy_entropy")

    # what a generation leaves behind: reset when one starts, kept by a captured graph, cloned out of its replay, joined across streams
    _GENERATION_RESULTS = ("last_tokens", "last_logits", "last_video_noise") + _LOGPROB_RESULTS

    def _generation_results(self) -> list:
        return [getattr(self, a) for a in self._GENERATION_RESULTS]

    def _set_generation_results(self, vals) -> None:
        for a, v in zip(self._GENERATION_RESULTS, vals):
            setattr(self, a, v)

    def _warm_derived(self) -> None:
        """Build every derived weight cache (bf16 copies, transposed codebook, folded BatchNorm vectors, summed positional
        tables) on the CALLER's stream: a cache built lazily inside one side stream would be read by the others with no event
        in between."""
        self._derived.get(self._build)
        for mod in (self.generate_model, self.ma_encoder, self.text_encoder, getattr(self, "adain", None), self.first_stage_model):
            if mod is not None and hasattr(mod, "_derived") and hasattr(mod, "_build"):
                mod._derived.get(mod._build)
        self._frame_tables()
        for enc, names in ((self.ma_encoder, [f"b{i}.{n}" for i in range(self.ma_encoder.layers) for n in ("in_proj", "out_proj", "c_fc", "c_proj")]),
                           (self.text_encoder, [f"l{i}.{n}" for i in range(self.text_encoder.transformer_layers)
                                                for n in ("in_proj", "out_proj", "fc2")] + ["proj"])):
            if getattr(enc, "split_kind", 0):
                de = enc._derived.get(enc._build)
                for n in names:
                    if de[n + ".f32"].shape[1] % 64 == 0:
                        _wsplit(de, n, enc.split_kind)
        if hasattr(self.generate_model, "_warm_split"):
            self.generate_model._warm_split()
            if self._sk():
                _wsplit(self._derived.get(self._build), "conv", self._sk())

    def _generate_multistream(self, batch, n):
        B = batch["images"].shape[0]
        per = B // n
        self._warm_derived()                                          # before the fork: side streams only READ the caches
        main = torch.cuda.current_stream(batch["images"].device)
        if getattr(self, "_side_streams", None) is None or len(self._side_streams) != n:
            self._side_streams = [torch.cuda.Stream(device=batch["images"].device) for _ in range(n)]
        outs, results = [None] * n, [None] * n
        for g, st in enumerate(self._side_streams):
            st.wait_stream(main)                                      # inputs were produced on the caller's stream
            with torch.cuda.stream(st):
                sub = {k: v[g * per:(g + 1) * per] for k, v in batch.items()}
                outs[g] = self._generate_one(sub)
                self.last_logits = None                               # (not joined: last_logits is None after a multi-stream call)
                results[g] = self._generation_results()
        for st in self._side_streams:
            main.wait_stream(st)
        for t_ in outs + [t_ for r_ in results for t_ in r_ if t_ is not None]:
            t_.record_stream(main)                                    # allocator plumbing: consumed on the caller's stream
        self._set_generation_results([None if col[0] is None else torch.cat(col, 0) for col in zip(*results)])
        return torch.cat(outs, 0)

    @torch.no_grad()
    def _generate_latent(self, batch):
        """use_cids=False (MAGE+, mage_model.py:645-646,683-684,689): the first stage is an external latent autoencoder
        (ldm AutoencoderKL in config/mage+_*.yaml); its encode/decode are the boundary, everything between runs here.
        The GroupNorm head mixes all frames of a clip, so only the reference's full-recompute loop is valid."""
        images = batch["images"]
        B = images.shape[0]
        R, L = self.image_resolution, self.frames_length
        hw, Lm1 = R * R, L - 1
        dt = self._dt()
        E = self.first_stage_model.embed_dim
        lat0 = self.first_stage_encode(images[:, 0:1])[:, 0]                                   # [B, E, h, w]
        LD = 8                                                                                # row stride of the latent buffer
        cur = torch.zeros(B, Lm1, hw, LD, device=images.device, dtype=F32)
        cur[..., :E] = lat0.permute(0, 2, 3, 1).reshape(B, 1, hw, E).float()                  # :670 every slot holds frame 0
        first = self._frame_features_latent(cur[:, 0].contiguous(), LD, F32)
        ma = self._motion_anchor(None, batch, batch.get("video_noise"), first=first)
        ma_dt = _to_dt(ma, dt)
        pred = None
        for i in range(Lm1):                                                                  # :673-684
            feats = self._frame_features_latent(cur.view(-1, LD), LD, dt)
            pred = self.generate_model._run(ma_dt, feats, B=B, hh=R, ww=R).view(B, Lm1, hw, -1)
            if i != Lm1 - 1:
                cur[:, i + 1, :, :E] = pred[:, i, :, :E]                                      # :684 (index plumbing)
        self.last_tokens, self.last_logits = None, pred[..., :E].reshape(B, Lm1, R, R, E)
        gen = pred[..., :E].reshape(B * Lm1, R, R, E).permute(0, 3, 1, 2).contiguous()          # :689
        video = self.first_stage_model.decode(gen)
        video = video.view(B, Lm1, *video.shape[1:])
        return _assemble(images, video)

    @torch.no_grad()
    def _generate_one(self, batch, keep_all: bool = False, candidate_noise: bool = False):
        """One eager generation of the batch on the current stream: the once-per-clip prologue, the AR loop of self.ar_mode, _finish.
        keep_all / candidate_noise: MAGE.rollout's (every candidate kept; a noise draw per candidate); the dict then carries 'seeds'."""
        c = self._prologue(batch, candidate_noise)
        gen, logits = (self._ar_incremental if self.ar_mode == "incremental" else self._ar_full)(c)
        out = self._finish(c.images, gen, logits, c.lp, c.Bc, c.N, c.st, keep_all, c.k)
        if keep_all:
            out["seeds"] = c.seeds
        return out

    def _prologue(self, batch, candidate_noise: bool = False) -> "_Generation":
        """What is computed once per call: the tokens of the k given frames, the given token of every slot, the candidate seeds and the
        motion anchor -- plain, guided ([cond | uncond]: 2 Bc clips) or with a noise draw per candidate -- expanded to N candidates."""
        images = batch["images"]
        Bc, hw, Lm1 = images.shape[0], self.image_resolution ** 2, self.frames_length - 1
        # k given frames (set_context; 1: frame 0 alone): one encode of all Bc * k, or batch['context_tokens'] in its place
        k = self._ctx()
        ctx = batch.get("context_tokens")
        ctx = (self.first_stage_encode(images[:, 0:k]) if ctx is None else ctx).reshape(Bc, k, hw)      # :642
        tok0 = ctx[:, 0].contiguous()
        # kn [Bc, (L-1) * hw]: the given token of every slot, negative where the slot is free (None: nothing given) -- batch['known_tokens']
        # with the given frames 1 .. k-1 merged into slots 0 .. k-2 on the device
        kn = batch.get("known_tokens")
        if kn is not None or k > 1:
            kn = torch.full((Bc, Lm1, hw), -1, device=images.device, dtype=torch.int64) if kn is None else kn.reshape(Bc, Lm1, hw).clone()
            kn[:, :k - 1] = ctx[:, 1:]
        # best of N: from the anchor on every clip is N adjacent rows of a batch of Bc * N, candidate c drawing with seed + c (int64 wrap-around)
        N = self._n_cand()
        expand = lambda t_: t_ if N == 1 else t_[:, None].expand(t_.shape[0], N, *t_.shape[1:]).reshape(t_.shape[0] * N, *t_.shape[1:])   # noqa: E731
        seeds = batch.get("sample_seed") if self.sampling is not None else None               # None: greedy
        if N > 1:
            seeds = (seeds[:, None] + torch.arange(N, device=seeds.device, dtype=torch.int64)[None, :]).reshape(Bc * N)
        gs = batch.get("guidance_scale") if self._guided() else None                          # None: no guidance
        if gs is not None:
            # classifier-free guidance: the prologue runs once over 2 Bc captions -- [the clips under their caption | the same clips under
            # the negative caption], clip b's second copy with clip b's frame 0, noise and speed -- and from here the batch is [cond | uncond]
            assert not candidate_noise                                                        # (rollout is refused while guidance is on)
            two = lambda t_: torch.cat([t_, t_], 0)      # noqa: E731
            tok0, ctx = two(tok0), two(ctx)
            noise, nseed = batch.get("video_noise"), batch.get("noise_seed")
            if self.randomness and noise is None and nseed is None:
                noise = torch.randn([Bc, 64, self.image_resolution, self.image_resolution], device=images.device)   # mage_model.py:661, one draw per clip
            ma = self._anchor_head(tok0, {"text": torch.cat([batch["text"].to(torch.int64), batch["negative_text"]], 0)})
            ma = self._anchor_tail(ma, {}, None if noise is None else two(noise), 2 * Bc, noise_seed=None if nseed is None else two(nseed),
                                   speed=two(batch["speed"]) if "speed" in batch else None)
            if self.last_video_noise is not None:
                self.last_video_noise = self.last_video_noise[:Bc]
        elif candidate_noise:
            # rollout(noise='candidate'): the text and MA encoders run once per clip; every candidate then draws its own noise -- under the
            # seed that also drives its sampler -- and conv_d2, ADAIN and the speed term run on the Bc * N rows
            ma = expand(self._anchor_head(tok0, batch).view(Bc, hw, -1)).reshape(Bc * N * hw, -1)
            ma = self._anchor_tail(ma, {}, None, Bc * N, noise_seed=seeds, speed=expand(batch["speed"]) if "speed" in batch else None)
        else:
            ma = self._motion_anchor(tok0, batch, batch.get("video_noise"))
        if N > 1:
            tok0, ctx = expand(tok0), expand(ctx)                                             # (under guidance each half expands alike)
            if not candidate_noise:
                ma = expand(ma.view(-1, hw, ma.shape[-1])).reshape(-1, ma.shape[-1])
        shape = (Lm1, Bc * N, hw) if self.ar_mode == "incremental" else (Bc * N, Lm1, self.image_resolution, self.image_resolution)
        lp = torch.empty(shape, device=images.device, dtype=F32) if self._want_logprobs() else None
        return _Generation(self, images, Bc, N, k, tok0, ctx, _to_dt(ma, self._dt()), seeds, gs, kn, lp, self._stats_alloc(shape, images.device))

    def _ar_incremental(self, c: "_Generation"):
        """each position once, temporal K,V cached; bit-identical tokens to the reference loop (_ar_full).  Tokens and results
        are frame-major while the loop runs: a frame's tokens are contiguous, and the pick writes them where the next step reads them."""
        R, Lm1, B, hw, k = self.image_resolution, c.Lm1, c.B, c.hw, c.k
        dec, dt = self.generate_model, self._dt()
        st = dec._inc_begin(c.Bd, R, R)
        gen_t = torch.empty(Lm1, c.Bd, hw, device=c.images.device, dtype=torch.int64)
        prev = c.tok0.contiguous() if k == 1 else c.ctx.contiguous()                          # [Bd, k, hw]: the given frames
        for i in range(k - 1):                            # the given frames' own slots: nothing is decoded or picked for them
            c.hold(gen_t[i], lambda b: b[i], B * hw, group=hw, known_off=i * hw)
        for i in range(k - 1, Lm1):
            first = i == k - 1
            if not first or k == 1 or self.context_prefill:
                # newest frame only; the first step takes the anchor and all k given frames as one window, the head on its last slot
                logits = dec._inc_step(st, c.ma if first else None, self._frame_source(prev, dt), nf=k if first else 1)
            else:                                         # context_prefill off: the given frames one position at a time, no pick
                for j in range(k):
                    logits = dec._inc_step(st, c.ma if j == 0 else None, self._frame_source(prev[:, j].contiguous(), dt))
            prev = gen_t[i]                               # clip = row // hw; the last frame's tokens condition nothing
            c.frame(i, logits, prev, lambda b: b[i], in_group_stride=hw, tok_group_stride=hw, slot=None if i == Lm1 - 1 else prev)
        clip_major = lambda t_: t_.permute(1, 0, 2).contiguous().view(B, Lm1, R, R)          # noqa: E731  (index plumbing, once; no copy at B = 1)
        c.lp = None if c.lp is None else clip_major(c.lp)
        c.st = None if c.st is None else {n: None if b is None else clip_major(b) for n, b in c.st.items()}
        return clip_major(gen_t[:, :B]), None

    def _ar_full(self, c: "_Generation"):
        """The reference's loop (:670-687): every iteration recomputes all L-1 slots and takes frame i's tokens into slot i + 1.  What it
        keeps from the reference's shape: a greedy call scores all frames at once after the loop, a sampled one draws only the last frame
        there (the others are the tokens the loop conditioned on), and last_logits are the last iteration's."""
        R, Lm1, B, hw, k, K = self.image_resolution, c.Lm1, c.B, c.hw, c.k, self.codebook_size
        dt, clip = self._dt(), c.Lm1 * c.hw
        cur = c.tok0[:, None, :].repeat(1, Lm1, 1).contiguous()                               # :670 future slots hold frame 0
        if k > 1:
            cur[:, 1:k] = c.ctx[:, 1:]                                                        # slots 1 .. k-1: the given frames
        flat = lambda b: b.view(-1)      # noqa: E731
        nxt = cur.view(-1)[hw:]                           # frame i's tokens go to slot i + 1: index i * hw of the flat view one frame on
        for i in range(k - 1, Lm1):                                                           # :673-684
            feats = self._frame_source(cur, dt)
            ev = ops.PROFILE.begin() if ops.PROFILE.wants("decoder_step") else None          # bench.py: the transformer step on its own
            logits = self.generate_model._run(c.ma, feats, B=c.Bd, hh=R, ww=R)                # [Bd*(L-1)*hw, K]
            if ev is not None:
                ops.PROFILE.end("decoder_step", ev, 0.0)
            if i != Lm1 - 1:                              # frame i's rows of the logits are all its pick needs
                c.frame(i, logits, nxt, flat, in_group_stride=clip, in_off=i * hw, tok_group_stride=clip, tok_off=i * hw, slot=cur[:, i + 1],
                        scored=c.seeds is not None)
        c.guide(logits, frames=Lm1)                       # the last iteration's: every frame, for the final pick and last_logits
        gen = torch.empty(B, Lm1, R, R, device=c.images.device, dtype=torch.int64)
        if c.seeds is None:
            c.pick(logits, gen, flat, rows=B * clip)                                          # :687
        else:
            gen.view(B, Lm1, hw)[:, :Lm1 - 1].copy_(cur[:B, 1:])
            last = (Lm1 - 1) * hw
            c.pick(logits, gen, flat, rows=B * hw, pos_off=last, group=hw, in_group_stride=clip, in_off=last, tok_group_stride=clip, tok_off=last)
        c.hold(gen, flat, B * clip, group=clip)           # every slot at once: the final pick's tokens and results, the given frames' slots
        return gen, logits[:B * clip].view(B, Lm1, R, R, K)

    def _video(self, head: torch.Tensor, gen: torch.Tensor, k: int) -> torch.Tensor:
        """The first k frames of head [rows, >= k, C, H, W] verbatim, then the decode of the generated slots k-1 .. of gen (:690-691)."""
        if k == 1:
            return _assemble(head, self.first_stage_decode(gen))
        video = self.first_stage_decode(gen[:, k - 1:])
        return torch.cat([head[:, :k].to(video.dtype), video], 1)

    def _finish(self, images, gen, logits, lp, Bc: int, N: int, st: Optional[dict] = None, keep_all: bool = False, k: int = 1):
        """The end of _generate_one: the per-clip scores of the token log-probabilities lp (None: the feature is off), with N > 1 the winners
        of every clip's N adjacent candidates (a device-side gather: no host decision), the results, the decode (_video).  st: the
        mage_token_stats buffers of set_logprobs(policy=, entropy=), [B * N, L-1, h, w] each (None: off); the winner's rows are kept.
        keep_all (MAGE.rollout only): no winner is picked -- all B * N candidates are decoded, each behind its clip's given frames, and handed
        back with their tokens and log-probabilities as a dict, and no result attribute is written."""
        if keep_all:
            first = images[:, 0:1] if N == 1 else images[:, 0:1].repeat_interleave(N, 0)
            head = first if k == 1 else images[:, :k].repeat_interleave(N, 0)
            return {"video": self._video(head, gen, k), "tokens": gen, "token_logprobs": lp, "first": first,
                    "behaviour_logprobs": st["policy_logprob"]}
        if lp is not None:
            scores, best = ops.clip_scores(lp, n_clips=Bc, n_cand=N)
            pscores = None
            if st is not None and st["policy_logprob"] is not None:
                pscores = ops.clip_scores(st["policy_logprob"], n_clips=Bc, n_cand=N)[0]
            if N > 1:
                win = best + torch.arange(Bc, device=best.device, dtype=torch.int64) * N
                gen, lp = gen.index_select(0, win), lp.index_select(0, win)
                logits = None if logits is None else logits.index_select(0, win)
                self.last_candidate_scores, self.last_candidate_index = scores, best
                self.last_clip_logprob = scores.gather(1, best[:, None]).view(Bc)
                if st is not None:
                    st = {n: None if b is None else b.index_select(0, win) for n, b in st.items()}
                if pscores is not None:
                    self.last_candidate_policy_scores = pscores
                    self.last_clip_policy_logprob = pscores.gather(1, best[:, None]).view(Bc)
            else:
                self.last_clip_logprob = scores.view(Bc)
                if pscores is not None:
                    self.last_clip_policy_logprob = pscores.view(Bc)
            self.last_token_logprobs = lp
            if st is not None:
                for name, attr in self._STATS_RESULTS:
                    setattr(self, attr, st[name])
        self.last_tokens, self.last_logits = gen, logits
        return self._video(images, gen, k)

    # ------------------------------------------------------------------ teacher-forced pass (mage_model.py:575-639)
    @torch.no_grad()
    def _video_prior(self, tok: Optional[torch.Tensor], lat_rows: Optional[torch.Tensor] = None, B: int = 0, L: int = 0,
                     tape: Optional[list] = None, dt: torch.dtype = F32) -> torch.Tensor:
        """self.conv3d over the token embeddings of ALL frames (mage_model.py:496-501,602-603): tok int64 [B, L, hw] (or, for
        use_cids=False, lat_rows [B*L*hw, 8] fp32 latents whose Linear(E -> C) embedding is taken) -> rows [B*hw, d_model] fp32.  Each Conv3d(3x3x3, temporal stride s, pad 1) is three implicit-GEMM launches, one per temporal tap,
        accumulating in place: the block input lives in a zero-padded frame buffer in which clip b owns frames
        [b*Lp, (b+1)*Lp) (frame 0 = the leading zero pad) with Lp = s * (virtual output frames per clip), so that output image
        i' = b*Lv + t' gathers from frame s*i' + kd: one affine image stride for the whole batch, the clip boundaries and the
        temporal padding are zero frames.  The Lv - Lout virtual frames per clip are never normalised or read.
        `tape` (a list, training path): receives per block what the backward pass needs (modules/mage_train_prior.py).
        dt: storage / MFMA dtype of the activations and weights (bf16 in bf16 training: the convolution outputs, the GroupNorm
        statistics and the block's result stay fp32; the values path and fp32 mode run everything in fp32)."""
        d = self._derived.get(self._build)
        R, Cc = self.image_resolution, self.vision_width
        hw = R * R
        if tok is not None:
            B, L = tok.shape[0], tok.shape[1]
        dev = tok.device if tok is not None else lat_rows.device

        def wdt(key):
            if dt == F32:
                return d[key]
            if key + ".bf16" not in d:
                d[key + ".bf16"] = d[key].to(BF16)
            return d[key + ".bf16"]

        def conv3(xpad, key, Lv, s_t, cin, cout):
            out = torch.empty(B * Lv * hw, cout, device=dev, dtype=F32)
            for kd in range(3):
                ops.gemm(xpad, wdt(f"{key}.{kd}"), out, M=B * Lv * hw, N=cout, K=9 * cin, lda=cin, ldy=cout, out_h=R, out_w=R,
                         in_h=R, in_w=R, taps_h=3, taps_w=3, cin=cin, stride=1, dy0=-1, dx0=-1, a_img_stride=s_t * hw,
                         a_off=kd * hw, residual=out if kd else None, ldr=cout)
            return out

        Lin = L
        Lout = (Lin + 1) // 2
        Lp = 2 * (Lout + 1)
        xa = torch.zeros((B * Lp + 1) * hw, Cc, device=dev, dtype=dt)                         # block 0 input: the embeddings
        if tok is not None:
            ops.embedding(tok.reshape(-1).contiguous(), d["emb"], xa, group=L * hw, group_stride=Lp * hw, off=hw)
        else:                                                      # Linear(E -> C) straight into the padded frame buffer (:583)
            E = d["emb_lin.w"].shape[1]
            ops.gemm(lat_rows, d["emb_lin.w"], xa, M=B * L * hw, N=Cc, K=E, lda=lat_rows.shape[1], ldy=Cc, out_w=L * hw,
                     y_img_stride=Lp * hw, y_off=hw, bias=d["emb_lin.b"])
        cin = Cc
        for i, blk in enumerate(self.conv3d):
            cout = blk.conv1.out_channels
            Lout = (Lin + 1) // 2
            Lv = Lout + 1
            gn = dict(n_samples=B, rows_per_sample=Lout * hw, groups=16)
            st1, std, st2 = (torch.empty(B, 16, 2, device=dev, dtype=F32) for _ in range(3))
            c1 = conv3(xa, f"p{i}.c1", Lv, 2, cin, cout)
            cd = conv3(xa, f"p{i}.ds", Lv, 2, cin, cout)
            xb = torch.zeros((B * (Lout + 2) + 2) * hw, cout, device=dev, dtype=dt)            # conv2 input: stride-1 layout
            ops.groupnorm_act(c1, d[f"p{i}.g1.w"], d[f"p{i}.g1.b"], xb, sample_stride_rows=Lv * hw, row_off=0, eps=blk.bn1.eps,
                              act=1, y_sample_stride_rows=(Lout + 2) * hw, y_row_off=hw, stats=st1, **gn)
            res = ops.groupnorm_act(cd, d[f"p{i}.gd.w"], d[f"p{i}.gd.b"], torch.empty(B * Lout * hw, cout, device=dev, dtype=F32),
                                    sample_stride_rows=Lv * hw, row_off=0, eps=blk.downsample[1].eps, act=0, stats=std, **gn)
            c2 = conv3(xb, f"p{i}.c2", Lout + 2, 1, cout, cout)
            if i + 1 < len(self.conv3d):                                                       # next block's stride-2 input
                Lp2 = 2 * ((Lout + 1) // 2 + 1)
                nxt = torch.zeros((B * Lp2 + 1) * hw, cout, device=dev, dtype=dt)
                ops.groupnorm_act(c2, d[f"p{i}.g2.w"], d[f"p{i}.g2.b"], nxt, sample_stride_rows=(Lout + 2) * hw, row_off=0,
                                  eps=blk.bn2.eps, act=1, residual=res, y_sample_stride_rows=Lp2 * hw, y_row_off=hw, stats=st2, **gn)
                out_map = (Lp2 * hw, hw)
            else:
                if Lout != 1:
                    raise ValueError(f"the Conv3d video prior's four stride-2 blocks must collapse the clip to ONE frame "
                                     f"(frames_length <= 16); got {L} frames -> {Lout}")
                nxt = ops.groupnorm_act(c2, d[f"p{i}.g2.w"], d[f"p{i}.g2.b"], torch.empty(B * hw, cout, device=dev, dtype=F32),
                                        sample_stride_rows=(Lout + 2) * hw, row_off=0, eps=blk.bn2.eps, act=1, residual=res, stats=st2,
                                        **gn)
                out_map = (hw, 0)
            if tape is not None:
                tape.append(dict(xa=xa, c1=c1, cd=cd, xb=xb, c2=c2, res=res, st1=st1, std=std, st2=st2, Lin=Lin, Lout=Lout, Lv=Lv, cin=cin,
                                 cout=cout, out_map=out_map, dt=dt))
            xa, cin, Lin = nxt, cout, Lout
        return xa

    def teacher_forced_logits(self, batch, extras: Optional[dict] = None):
        """tokens [B, L, h, w] and logits [B, L-1, h, w, K] of one teacher-forced decoder pass.  With randomness=True the motion
        anchor is modulated by the reparameterised Conv3d video prior (mage_model.py:601-609); `extras` (a dict) then receives
        'kl_sum' [B] (sum of 1 + logvar - mu^2 - exp(logvar) per sample) and 'prior' rows [B*hw, C]."""
        images = batch["images"]
        _need_gpu(images, "MAGE.forward")
        if not self.use_cids:
            raise NotImplementedError("teacher_forced_logits is the use_cids=True path; MAGE.forward handles use_cids=False")
        B = images.shape[0]
        R, L = self.image_resolution, self.frames_length
        dt = self._dt()
        tok = self.first_stage_encode(images).reshape(B, -1, R * R)                          # :579
        video_rows = self._reparam_video_rows(batch, B, extras, tok=tok) if self.randomness else None
        ma = self._motion_anchor(tok[:, 0].contiguous(), batch, None, video_rows=video_rows)
        feats = self._frame_source(tok[:, :L - 1].contiguous(), dt)
        logits = self.generate_model._run(_to_dt(ma, dt), feats, B=B, hh=R, ww=R)
        return tok.view(B, -1, R, R), logits.view(B, L - 1, R, R, self.codebook_size)

    def _reparam_video_rows(self, batch, B: int, extras: Optional[dict], tok=None, lat_rows=None, L: int = 0) -> torch.Tensor:
        """Conv3d video prior -> conv_mu2 / conv_var2 -> reparameterisation (mage_model.py:601-604,569-573): rows [B*hw, 64]
        (before conv_d2); extras receives 'kl_sum' [B] and 'prior' rows."""
        R = self.image_resolution
        d = self._derived.get(self._build)
        prior = self._video_prior(tok, lat_rows, B, L)                                    # :602-603
        Cp, dev = prior.shape[1], prior.device
        mu = VectorQuantizedVAE._conv(prior, d["mu2.w"], torch.empty(B * R * R, 64, device=dev, dtype=F32), n_img=B, H=R, W=R,
                                      cin=Cp, cout=64, k=3, bias=d["mu2.b"])              # :570
        logvar = VectorQuantizedVAE._conv(prior, d["var2.w"], torch.empty_like(mu), n_img=B, H=R, W=R, cin=Cp, cout=64, k=3,
                                          bias=d["var2.b"])
        eps = batch.get("reparam_noise")                                                  # [B,64,h,w]; else torch.randn (:571)
        if eps is None:
            eps = torch.randn(B, 64, R, R, device=dev)
        eps = eps.to(dev).float().permute(0, 2, 3, 1).reshape(B * R * R, 64).contiguous()
        kl_sum = torch.empty(B, device=dev, dtype=F32)
        video_rows = ops.reparam_kl(mu.view(B, -1), logvar.view(B, -1), eps.view(B, -1), torch.empty_like(mu).view(B, -1), kl_sum)
        video_rows = video_rows.view(B * R * R, 64)
        if extras is not None:
            extras.update(kl_sum=kl_sum, prior=prior)
        if batch.get("_test_flag"):
            # forward(test_flag=True) (mage_model.py:604-605): mu / logvar still feed the KL term, the embedding itself is fresh noise
            # (batch['video_noise'] [B,64,h,w] injects it, as in autoregressive_generate)
            nz = batch.get("video_noise")
            if nz is None:
                nz = torch.randn(B, 64, R, R, device=dev)
            video_rows = nz.to(dev).float().permute(0, 2, 3, 1).reshape(B * R * R, 64).contiguous()
        return video_rows

    @torch.no_grad()
    def _forward_latent(self, batch, extras: dict):
        """use_cids=False (MAGE+, mage_model.py:579,583,620): latents of ALL frames from the external first stage, teacher-forced
        latent prediction, MSE.  Returns (mse 0-dim tensor, pred rows [B*(L-1)*hw, 8])."""
        images = batch["images"]
        B = images.shape[0]
        R, L = self.image_resolution, self.frames_length
        hw, dt = R * R, self._dt()
        E, LD = self.first_stage_model.embed_dim, 8
        lat = self.first_stage_encode(images)                                                 # [B, L, E, h, w]
        Lb = lat.shape[1]
        rows = torch.zeros(B, Lb, hw, LD, device=images.device, dtype=F32)
        rows[..., :E] = lat.permute(0, 1, 3, 4, 2).reshape(B, Lb, hw, E).float()              # layout plumbing (channels last)
        video_rows = None
        if self.randomness:
            video_rows = self._reparam_video_rows(batch, B, extras, lat_rows=rows.view(-1, LD), L=Lb)
        first = self._frame_features_latent(rows[:, 0].contiguous().view(-1, LD), LD, F32)
        ma = self._motion_anchor(None, batch, None, first=first, video_rows=video_rows)
        feats = self._frame_features_latent(rows[:, :L - 1].contiguous().view(-1, LD), LD, dt)
        pred = self.generate_model._run(_to_dt(ma, dt), feats, B=B, hh=R, ww=R)      # [B*(L-1)*hw, 8]
        tgt = rows[:, 1:L].contiguous().view(-1, LD)
        return ops.mse(pred, tgt, rows=B * (L - 1) * hw, cols=E, lda=pred.shape[1], ldb=LD), pred

    def _forward_with_graph(self, batch, head=None):
        """Grad mode (the training loop, main_mage.py:150-153): the same pass as one autograd node whose inputs are the trainable
        parameters (mage_train.MageLossFn, through _run_head), so that ``loss.backward()`` fills every ``.grad`` from the HIP backward kernels."""
        _need_gpu(batch["images"], "MAGE.forward")
        with torch.cuda.device(batch["images"].device):
            loss, (parts, _) = self._run_head(batch, head)
            prefix = "train" if self.training else "val"
            ops.check_device_errors(batch["images"].device)
        return loss, {f"{prefix}/{k}": v for k, v in parts.items()}

    def _drop_captions(self, batch) -> dict:
        """Caption dropout at the top of forward (see there): the batch with the dropped rows of 'text' replaced by their null caption (one
        torch.where on the text's device), and without its 'caption_drop' entry."""
        self.last_caption_drop = None
        p = getattr(self, "caption_dropout", 0.0)
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
            raise ValueError(f"caption_dropout must be a float in [0, 1], got {p!r}")
        drop = batch.get("caption_drop")
        if drop is None and not (self.training and p > 0):
            return batch
        text = batch["text"]
        B = text.shape[0]
        if drop is None:
            drop = torch.rand(B) < p                     # torch's default CPU generator, as the dropout seeds and the sample seeds
        drop = torch.as_tensor(drop)
        if drop.dtype != torch.bool or tuple(drop.shape) != (B,):
            raise ValueError(f"batch['caption_drop'] must be bool [{B}], got {drop.dtype} {tuple(drop.shape)}")
        from ..utils.glue import null_caption
        drop = drop.to(text.device)
        self.last_caption_drop = drop
        text = torch.where(drop[:, None], null_caption(text, int(getattr(self.text_encoder, "padding_idx", 0))), text)
        return {**{k: v for k, v in batch.items() if k != "caption_drop"}, "text": text}

    def forward(self, batch, test_flag=False):
        """(loss, loss_dict) of the teacher-forced pass (mage_model.py:575-639), incl. the randomness=True terms (KL of the
        reparameterised video prior, the PID-controlled or fixed beta, the speed-embedding l2).  batch['reparam_noise']
        [B,64,h,w] optionally injects the reparameterisation noise; ``test_flag=True`` (values only) replaces the video embedding by noise
        (batch['video_noise'] injects it) while the KL term still comes from mu / logvar (:604).  Under ``torch.no_grad()``: values only.  In grad mode (any
        parameter requiring grad): the returned loss carries an autograd node backed by the HIP backward kernels
        (modules/mage_train.py, mage_train_prior.py: every config family -- MNIST, CATER with the randomness branch, MAGE+), so
        ``loss.backward(); optimizer.step()`` works.
        Caption dropout (what teaches the model the null caption classifier-free guidance steers away from, set_guidance): with
        ``self.caption_dropout = p`` in (0, 1] and the model in training mode, each clip's caption is replaced, with probability p, by
        mage_amd.utils.glue.null_caption of itself before anything else runs -- the mask comes from torch's default CPU generator;
        batch['caption_drop'] (bool [B], optional) replaces the draw and applies in either mode.  last_caption_drop keeps the mask (None when
        nothing was dropped or drawn).  p = 0 (the default) and no mask: the call is the one it was."""
        batch = self._drop_captions(batch)
        head = self._supervised_head(batch)              # None: the plain loss; set_loss / batch['given']: mage_token_xent (see set_loss)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if test_flag and self.randomness:
                raise NotImplementedError("forward(test_flag=True) is an evaluation switch (mage_model.py:604): call it under torch.no_grad()")
            return self._forward_with_graph(batch, head)
        batch = dict(batch, _test_flag=bool(test_flag and self.randomness))      # :604: the video embedding is replaced by noise
        extras: dict = {}
        L = self.frames_length
        if self.use_cids:
            tok, logits = self.teacher_forced_logits(batch, extras)
            logits, tgt, more = logits.reshape(-1, self.codebook_size), tok[:, 1:L].reshape(-1).contiguous(), {}
            if head is None:
                recon = ops.cross_entropy(logits, tgt)                                                                # :618
            else:
                recon, more, _ = head.forward(self, logits, tgt, batch["images"].shape[0])
        else:
            _need_gpu(batch["images"], "MAGE.forward")
            recon, self.last_logits = self._forward_latent(batch, extras)                                            # :620
        prefix = "train" if self.training else "val"
        ld = {f"{prefix}/prediction": recon.item()}
        if self.use_cids:
            ld.update({f"{prefix}/{k}": v for k, v in more.items()})       # the SupervisedHead's parts ('prediction' again, 'nll', 'accuracy', ...)
        final = recon
        if self.randomness:
            kl = -0.5 * extras["kl_sum"].mean()                                               # :623 (a [B]-element reduction)
            ld[f"{prefix}/kl_loss"] = kl.item()
            if self.auto_beta:
                self.beta, _ = self.PID.pid(self.KL_loss, kl.item())                          # :627
                ld[f"{prefix}/beta"] = self.beta
                final = recon + self.beta * kl
            else:
                # mean_b || speed_b * speed_embedding ||^2 (:631); like the reference this branch needs batch['speed']
                l2 = (batch["speed"].float().to(recon.device) ** 2).mean() * (self.speed_embedding.float() ** 2).sum()
                final = recon + self.beta * kl + self.alpha * l2
        ld[f"{prefix}/final_loss"] = final.item()
        ops.check_device_errors(batch["images"].device)
        return final, ld
