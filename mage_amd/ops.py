"""Thin tensor-level wrappers over the C ABI (include/mage_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic
op below is one libmage_hip.so call on ``torch.cuda.current_stream()``.
All wrappers raise if a tensor is not on a CUDA (ROCm) device -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import ACT_GELU_ERF, ACT_NONE, ACT_QUICKGELU, ACT_QUICKGELU_GRAD, ACT_RELU, ACT_TANH, BF16, BF16X3, F16, F16X3, F32, AttnDesc, GemmDesc

__all__ = ["gemm", "layernorm", "attention", "embedding", "table_conv", "split_rows", "vq_prepare", "vq_nearest", "argmax", "cross_entropy",
           "conv_in", "conv_out", "convt_fold_tanh", "row_affine", "groupnorm_silu", "groupnorm_act", "reparam_kl", "mse", "check_device_errors", "graph_events_supported", "transpose", "row_sum", "sum_partials", "layernorm_bwd", "dropout_add_layernorm", "act", "act_bwd", "cross_entropy_bwd", "embedding_bwd", "code_stats", "code_stats_chunks", "codebook_ema", "group_rowsum", "attention_bwd", "dropout", "adam", "adam_clipped", "adam_guarded", "sumsq", "bn_train_stats", "bn_apply", "bn_backward", "convt_unfold_tanh_bwd", "maxpool2", "upsample2", "relu", "cast", "adain", "add_scaled_rowvec",
           "token_logprob", "clip_scores", "video_metrics", "group_advantages", "frame_advantages", "policy_loss", "policy_loss_bwd", "preference_loss", "token_logprob_bwd", "distill_loss", "distill_loss_bwd", "token_xent", "token_xent_bwd", "split", "split_empty", "split_dtype", "PROFILE", "F32", "BF16", "F16", "BF16X3", "F16X3", "ACT_NONE", "ACT_RELU", "ACT_QUICKGELU", "ACT_GELU_ERF", "ACT_TANH", "tdtype", "code"]


def code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"unsupported dtype {t.dtype}")


def tdtype(c: int) -> torch.dtype:
    return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[c]


# ---- split-precision tensors (MAGE_BF16X3 / MAGE_F16X3, include/mage_hip.h): a logical fp32 [rows, C] matrix kept as two 16-bit pieces
# per element, per row as 64-column slabs [hi(64) | lo(64)].  To torch it is a [rows, 2C] tensor of bfloat16 / float16 (plumbing:
# the pieces are only ever read by mage_gemm); the kind travels beside it.
def split_dtype(kind: int) -> torch.dtype:
    return torch.bfloat16 if kind == BF16X3 else torch.float16


def split_empty(rows: int, C_: int, kind: int, device, zero: bool = False) -> torch.Tensor:
    assert C_ % 64 == 0 and kind in (BF16X3, F16X3)
    f = torch.zeros if zero else torch.empty
    return f(rows, 2 * C_, device=device, dtype=split_dtype(kind))


def split(x: torch.Tensor, kind: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 rows [rows, C] (row stride x.stride(0)) -> split rows [rows, 2C] (mage_split)."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, C_ = x.shape
    if out is None:
        out = split_empty(rows, C_, kind, x.device)
    assert out.dtype == split_dtype(kind) and out.is_contiguous() and out.shape[-1] == 2 * C_
    _lib.check(l.mage_split(x.data_ptr(), x.stride(0), out.data_ptr(), 2 * C_, rows, C_, kind, s), l)
    return out


def _dev(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("mage_amd ops need tensors on a ROCm GPU (cuda device); there is no CPU fallback")
    idx = t.device.index or 0
    if idx != torch.cuda.current_device():
        # the C ABI launches on the CURRENT device (zero page, launch attributes, the kernels themselves): a tensor of another
        # device would be addressed from the wrong GPU
        raise RuntimeError(f"mage_amd ops: tensor on cuda:{idx} but the current device is cuda:{torch.cuda.current_device()}; "
                           f"wrap the call in torch.cuda.device({idx})")
    return _lib.lib(idx), torch.cuda.current_stream(t.device).cuda_stream


_GRAPH_EVENTS = {}


def graph_events_supported(device) -> bool:
    """Can timing events be captured into a HIP graph as event-record nodes (torch.cuda.Event(external=True)) and read back
    after a replay?  Probed once per device with a two-node graph."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _GRAPH_EVENTS:
        ok = False
        import warnings
        try:
            with torch.cuda.device(idx), warnings.catch_warnings():
                warnings.simplefilter("ignore")          # a runtime without event-record nodes leaves an empty graph behind: expected, not news
                x = torch.zeros(1 << 20, device=dev)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                a = torch.cuda.Event(enable_timing=True, external=True)
                b = torch.cuda.Event(enable_timing=True, external=True)
                with torch.cuda.graph(g):
                    a.record()
                    x.add_(1.0)
                    b.record()
                for _ in range(2):
                    g.replay()
                    torch.cuda.synchronize()
                    ms = a.elapsed_time(b)
                ok = 0.0 < ms < 100.0
        except Exception:
            ok = False
        _GRAPH_EVENTS[idx] = ok
    return _GRAPH_EVENTS[idx]


def check_device_errors(device) -> None:
    """Raise (ValueError) if a kernel met an out-of-range id / target since the last check; synchronises the current stream
    of `device` (include/mage_hip.h: mage_check_device_errors)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(idx):
        l = _lib.lib(idx)
        _lib.check(l.mage_check_device_errors(torch.cuda.current_stream(idx).cuda_stream), l)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _kernel_name(l, d) -> str:
    """The symbol of the kernel mage_gemm picks for descriptor d (mage_gemm_kernel_name: the library's own dispatch, nothing launched), as
    rocprofv3's per-symbol statistics name it: the profile keys line up with them."""
    buf = C.create_string_buffer(256)
    _lib.check(l.mage_gemm_kernel_name(C.byref(d), buf, len(buf)), l)
    return buf.value.decode()


class _Profile:
    """Optional per-launch timing with HIP events recorded on the launch stream (torch.cuda.Event on the
    current stream IS a hipEvent on the stream the kernels are enqueued on).  Used by bench.py for the
    roofline of the dominant kernel; off by default (zero overhead).

    Eager launches: begin()/end() record a pair of events per instrumented launch.  Graph replay (MAGE.use_graph): the pairs
    are recorded ONCE, while the graph is captured, as `external` events (event-record nodes of the graph); every replay
    re-records them, and absorb() adds their elapsed times after the replay has been synchronised."""

    def __init__(self):
        self.enabled = False
        self.records = []
        self.only = None             # None: every instrumented launch; else the set of keys to time (others run un-bracketed)
        self.external = False        # True while a HIP graph is being captured
        self.acc = {}

    def reset(self, enabled: bool = False, only=None):
        self.enabled, self.records, self.only = enabled, [], (set(only) if only is not None else None)
        self.acc = {}

    def clear(self):
        """Drop what was measured so far, keep the mode (so that graphs captured for this mode stay valid)."""
        self.records, self.acc = [], {}

    def mode_key(self):
        """What a captured graph has to match: off / every launch / a set of keys."""
        if not self.enabled:
            return "off"
        return "all" if self.only is None else tuple(sorted(self.only))

    def wants(self, key: str) -> bool:
        return self.enabled and (self.only is None or key in self.only)

    def begin(self):
        e = torch.cuda.Event(enable_timing=True, external=True) if self.external else torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, key: str, start, flops: float = 0.0, nbytes: float = 0.0):
        e = torch.cuda.Event(enable_timing=True, external=True) if self.external else torch.cuda.Event(enable_timing=True)
        e.record()
        self.records.append((key, start, e, flops, nbytes))

    def capture_begin(self):
        """Start collecting the event pairs of a graph capture; returns the state to hand back to capture_end."""
        saved = (self.records, self.external)
        self.records, self.external = [], True
        return saved

    def capture_end(self, saved):
        recs = self.records
        self.records, self.external = saved
        return recs

    def _add(self, out, recs):
        for key, s, e, fl, nb in recs:
            d = out.setdefault(key, {"ms": 0.0, "calls": 0, "flops": 0.0, "bytes": 0.0})
            d["ms"] += s.elapsed_time(e)
            d["calls"] += 1
            d["flops"] += fl
            d["bytes"] += nb

    def absorb(self, recs):
        """Add the elapsed times of a replayed graph's event pairs (the replay must have completed)."""
        if self.enabled and recs:
            self._add(self.acc, recs)

    def summary(self):
        torch.cuda.synchronize()
        out = {k: dict(v) for k, v in self.acc.items()}
        self._add(out, self.records)
        return out


PROFILE = _Profile()


def gemm(a: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, M: int, N: int, K: int, lda: int, ldy: int,
         out_h: int = 1, out_w: Optional[int] = None, in_h: Optional[int] = None, in_w: Optional[int] = None,
         a_img_stride: Optional[int] = None, a_off: int = 0, taps_h: int = 1, taps_w: int = 1, cin: Optional[int] = None,
         stride: int = 1, dy0: int = 0, dx0: int = 0, dys: int = 1, dxs: int = 1,
         y_img_stride: Optional[int] = None, y_mul_y: Optional[int] = None, y_mul_x: int = 1, y_off: int = 0,
         bias=None, scale=None, shift=None, act: int = ACT_NONE, rowadd=None, rowadd_div: int = 1, rowadd_mod: int = 1,
         residual=None, ldr: int = 0, post_relu: bool = False, ldw: int = 0, n_split: int = 1, a_split_stride: int = 0,
         w_split_stride: int = 0, y_split_stride: int = 0, y2=None, ldy2: int = 0, ln_part=None, ln_stats=None,
         ln_colsum=None, res_half: bool = False, a_half: bool = False, split_kind: int = 0, y_split: bool = False,
         ln_eps: float = 0.0, head_w=None, head_phases: int = 0, a_relu: bool = False) -> torch.Tensor:
    """Y = epilogue(A (*) W^T); see mage_gemm in include/mage_hip.h for the geometry fields.
    split_kind BF16X3 / F16X3: a and w are split-precision tensors (lda / ldw in 16-bit elements); y_split: so is y (ldy likewise).
    head_w (bf16 [16, N], padded-taps form with N == 256, bias, ReLU): y (fp32, ldy >= 16) receives the narrow Linear head_w on the
    bf16-rounded rows relu(acc + bias), which are not stored (mage_gemm_desc::head_w).
    a_relu (16-bit plain GEMM, N <= 128): the product over relu(a) (mage_gemm_desc::a_relu)."""
    l, s = _dev(a)
    if split_kind and a_relu:
        raise ValueError("ops.gemm: split-precision operands (split_kind) do not take a_relu")
    if split_kind:
        # the split-precision form takes a subset of the arguments (launch_spl / try_taps8 in csrc/gemm.hip): refuse the rest loudly
        # instead of dropping them
        unsupported = dict(scale=scale, shift=shift, y2=y2, ln_part=ln_part, ln_stats=ln_stats, ln_colsum=ln_colsum, head_w=head_w)
        bad = [k for k, v_ in unsupported.items() if v_ is not None]
        bad += [k for k, v_ in dict(post_relu=post_relu, res_half=res_half, a_half=a_half).items() if v_]
        bad += [k for k, v_ in dict(n_split=n_split).items() if v_ not in (0, 1)]
        bad += [k for k, v_ in dict(a_split_stride=a_split_stride, w_split_stride=w_split_stride, y_split_stride=y_split_stride, ldy2=ldy2,
                                    stride=stride - 1, dy0=dy0, dx0=dx0, dys=dys - 1, dxs=dxs - 1).items() if v_]
        if ln_eps:
            bad.append("ln_eps")
        if bad:
            raise ValueError(f"ops.gemm: split-precision operands (split_kind) do not take {', '.join(bad)}")
        if residual is not None and residual.dtype != torch.float32:
            raise ValueError(f"ops.gemm: the split-precision x + Linear(.) form adds an fp32 residual, got {residual.dtype}")
        return _gemm_split(l, s, a, w, y, M=M, N=N, K=K, lda=lda, ldy=ldy, out_h=out_h, out_w=out_w, in_h=in_h, in_w=in_w,
                           a_img_stride=a_img_stride, a_off=a_off, taps_h=taps_h, taps_w=taps_w, cin=cin, y_img_stride=y_img_stride,
                           y_mul_y=y_mul_y, y_mul_x=y_mul_x, y_off=y_off, bias=bias, act=act, rowadd=rowadd, rowadd_div=rowadd_div,
                           rowadd_mod=rowadd_mod, residual=residual, ldr=ldr, ldw=ldw, split_kind=split_kind, y_split=y_split)
    out_w = M if out_w is None else out_w
    in_h = out_h if in_h is None else in_h
    in_w = out_w if in_w is None else in_w
    d = GemmDesc()
    d.dtype, d.M, d.N, d.K = code(a), M, N, K
    assert w.dtype == a.dtype, (w.dtype, a.dtype)
    d.A, d.W, d.Y = a.data_ptr(), w.data_ptr(), y.data_ptr()
    d.lda, d.ldy, d.y_dtype = lda, ldy, code(y)
    d.out_h, d.out_w, d.in_h, d.in_w = out_h, out_w, in_h, in_w
    d.a_img_stride = in_h * in_w if a_img_stride is None else a_img_stride
    d.a_off = a_off
    d.taps_h, d.taps_w, d.cin, d.stride = taps_h, taps_w, (K // (taps_h * taps_w) if cin is None else cin), stride
    d.dy0, d.dx0, d.dys, d.dxs = dy0, dx0, dys, dxs
    d.y_img_stride = out_h * out_w if y_img_stride is None else y_img_stride
    d.y_mul_y = out_w if y_mul_y is None else y_mul_y
    d.y_mul_x, d.y_off = y_mul_x, y_off
    d.bias, d.scale, d.shift = _p(bias), _p(scale), _p(shift)
    d.act = act
    d.rowadd, d.rowadd_div, d.rowadd_mod = _p(rowadd), rowadd_div, rowadd_mod
    d.residual, d.ldr, d.res_dtype = _p(residual), ldr, (code(residual) if residual is not None else 0)
    d.post_relu = int(post_relu)
    d.ldw, d.n_split = ldw, n_split
    d.a_split_stride, d.w_split_stride, d.y_split_stride = a_split_stride, w_split_stride, y_split_stride
    d.y2, d.ldy2, d.ln_part, d.ln_stats, d.ln_colsum = _p(y2), ldy2, _p(ln_part), _p(ln_stats), _p(ln_colsum)
    d.ln_eps = float(ln_eps)
    if ln_part is not None:                                 # slice-major partial sums [n_slices, rows, 2] (mage_gemm_desc::ln_part_rows)
        assert ln_part.dtype == torch.float32 and ln_part.dim() == 3 and ln_part.shape[2] == 2 and ln_part.is_contiguous(), tuple(ln_part.shape)
        d.ln_part_rows = ln_part.shape[1]
    if head_w is not None:
        assert head_w.dtype == torch.bfloat16 and head_w.is_contiguous() and tuple(head_w.shape) == (16, N // (head_phases or 1)) \
            and y.dtype == torch.float32, (head_w.dtype, tuple(head_w.shape), y.dtype)
    d.head_w = _p(head_w)
    d.head_phases = head_phases if head_w is not None else 0
    d.res_half = int(res_half)
    d.a_half = int(a_half)
    d.a_relu = int(a_relu)
    if PROFILE.enabled:
        key = _kernel_name(l, d)
        if PROFILE.wants(key):
            ev = PROFILE.begin()
            _lib.check(l.mage_gemm(C.byref(d), s), l)
            # algorithmic HBM bytes of this launch (SURVEY 8d's convention: every operand once): A + W + Y (+ fp32 residual, + the bf16
            # copy and the LayerNorm partial sums of the producer form)
            es, ys = a.element_size(), y.element_size()
            nb = float(M) * K * es + float(N) * K * es + float(M) * N * ys
            if key == "conv3x3_c64_kernel":                  # the input once (a quarter of it with a_half), not once per tap
                nb = float(M) * 64 * es * (0.25 if a_half else 1.0) + float(N) * K * es + float(M) * N * ys
            if residual is not None:
                nb += float(M) * N * residual.element_size()
            if y2 is not None:
                nb += float(M) * N * 2
            if ln_part is not None:
                nb += float(M) * (N // 64) * 8
            fl = 2.0 * M * N * K
            if head_w is not None:                           # the rows stay on the CU; 16 fp32 values per row (and phase) leave it
                nb += float(M) * 16 * 4 * (head_phases or 1) - float(M) * N * ys
                fl += 2.0 * M * N * 16
            PROFILE.end(key, ev, fl, nb)
            return y
    _lib.check(l.mage_gemm(C.byref(d), s), l)
    return y


def qkv_pack_rows(C_: int, device=None) -> torch.Tensor:
    """Row order of the packed weight of gemm_attn_fused_qkv (mage_gemm_attn_fused_qkv, include/mage_hip_ext.h): packed row n of the 3C rows =
    row index[n] of in_proj's [q; k; v] rows.  Group g of 4 heads takes rows 384g .. 384g+383.  Its first 256 rows: head h of the group at rows
    64h .. 64h+63 as [q_h | k_h]; inside each 32 rows, row j is head dim (j % 16 // 4) * 8 + (j // 16) * 4 + j % 4 -- the order in which a
    lane's two packed accumulator blocks are 8 consecutive dims.  Then its 128 v rows in their natural order."""
    n = torch.arange(2 * C_, device=device)
    head, part, j = n // 64, (n % 64) // 32, n % 32
    dim = (j % 16 // 4) * 8 + (j // 16) * 4 + j % 4
    qk = (part * C_ + head * 32 + dim).view(C_ // 128, 256)
    v = (2 * C_ + torch.arange(C_, device=device)).view(C_ // 128, 128)
    return torch.cat([qk, v], dim=1).reshape(-1)


def gemm_attn_fused_qkv(a: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, axis: int, M: int, C_: int, K: int, lda: int, bias, ln_stats, ln_colsum,
                        ldy: int, scale: Optional[float] = None, a_off: int = 0, out_w: Optional[int] = None, y_img_stride: Optional[int] = None,
                        y_off: int = 0):
    """The axial attention inside the in_proj GEMM, one launch (mage_gemm_attn_fused_qkv): w, bias and ln_colsum are the 3 C_ rows of the
    LayerNorm-folded in_proj in qkv_pack_rows' order; writes the attention output rows y [.., C_] -- the bits of ops.gemm (QKV) followed by
    ops.attention.  axis 1 = H, 2 = W of 16 x 16 frames (out_w, y_img_stride, y_off regroup the output rows whole frames at a time); axis 0 = T,
    causal, over whole clips of 16 slots: rows [clip, slot, hw] with out_w = hw, the rows of one slot, a multiple of 16 (a_off and y_off whole
    clips; y_img_stride stays out_w: the rows are not regrouped); scale as ops.attention's."""
    l, s = _dev(a)
    assert w.dtype == a.dtype and y.dtype == a.dtype, (w.dtype, y.dtype)
    out_w = M if out_w is None else out_w
    d = GemmDesc()
    d.dtype, d.M, d.N, d.K = code(a), M, 3 * C_, K
    d.A, d.W, d.Y = a.data_ptr(), w.data_ptr(), _p(y)
    d.lda, d.ldy, d.y_dtype = lda, ldy, code(y)
    d.out_h, d.out_w, d.in_h, d.in_w = 1, out_w, 1, out_w
    d.a_img_stride, d.a_off = out_w, a_off
    d.taps_h, d.taps_w, d.cin, d.stride = 1, 1, K, 1
    d.dys, d.dxs = 1, 1
    d.y_img_stride = out_w if y_img_stride is None else y_img_stride
    d.y_mul_y, d.y_mul_x, d.y_off = out_w, 1, y_off
    d.bias, d.ln_stats, d.ln_colsum = _p(bias), _p(ln_stats), _p(ln_colsum)
    d.n_split = 1
    sc = float(32 ** -0.5 if scale is None else scale)
    ev = None
    if PROFILE.enabled:
        buf = C.create_string_buffer(256)
        _lib.check(l.mage_gemm_attn_fused_qkv_kernel_name(C.byref(d), axis, buf, len(buf)), l)
        key = buf.value.decode()
        if PROFILE.wants(key):
            ev = PROFILE.begin()
    _lib.check(l.mage_gemm_attn_fused_qkv(C.byref(d), axis, sc, s), l)
    if ev is not None:
        # algorithmic HBM bytes: the rows a read once (their second pass comes from L2), the weights, y written.  q, k, v and P never appear.
        es = a.element_size()
        nb = float(M) * K * es + 3.0 * C_ * K * es + float(M) * C_ * y.element_size()
        fl = 2.0 * M * 3 * C_ * K + 6.0 * M * 16 * C_
        PROFILE.end(key, ev, fl, nb)
    return y


def mlp_fused(x: torch.Tensor, y: torch.Tensor, *, M: int, C_: int, w1: torch.Tensor, c1, s1, ln_stats, w2: torch.Tensor, b2, ln_part=None,
              ldx: Optional[int] = None, ldy: Optional[int] = None, a_off: int = 0, y_off: int = 0, ldw1: Optional[int] = None,
              ldw2: Optional[int] = None):
    """A decoder block's MLP in one launch (mage_mlp_fused, csrc/gemm4m.hip): y = x + c_proj(QuickGELU(c_fc(LN(x)))) on the 16-bit rows x with the
    LayerNorm folded into c_fc (w1 = gamma * W_fc, c1 = W_fc beta + b, s1 = w1's row sums, ln_stats = (mean, rstd) rows), y is x (in place) or another
    buffer; ln_part (optional, [C_/64, rows, 2]) receives the LayerNorm partial sums of the new rows.  The bits of ops.gemm (c_fc, QuickGELU)
    followed by ops.gemm (c_proj with the 16-bit residual); the hidden rows are never stored.  C_ = 512, M % 128 == 0."""
    l, s = _dev(x)
    ldx, ldy = C_ if ldx is None else ldx, C_ if ldy is None else ldy
    ldw1, ldw2 = C_ if ldw1 is None else ldw1, 4 * C_ if ldw2 is None else ldw2
    lpr = 0
    if ln_part is not None:
        assert ln_part.dtype == torch.float32 and ln_part.dim() == 3 and ln_part.shape[2] == 2 and ln_part.is_contiguous(), tuple(ln_part.shape)
        lpr = ln_part.shape[1]
    args = (code(x), code(w1), code(y), M, C_, x.data_ptr(), ldx, a_off, y.data_ptr(), ldy, y_off, w1.data_ptr(), ldw1, _p(c1), _p(s1), _p(ln_stats),
            w2.data_ptr(), ldw2, _p(b2), _p(ln_part), lpr)
    ev = None
    if PROFILE.enabled:
        buf = C.create_string_buffer(256)
        _lib.check(l.mage_mlp_fused_kernel_name(*args, buf, len(buf)), l)
        key = buf.value.decode()
        if PROFILE.wants(key):
            ev = PROFILE.begin()
    _lib.check(l.mage_mlp_fused(*args, s), l)
    if ev is not None:
        # algorithmic HBM bytes: x in, y out, both weights, the partial sums; the hidden rows never appear
        es = x.element_size()
        nb = 2.0 * M * C_ * es + 8.0 * C_ * C_ * es + (float(M) * (C_ // 64) * 8 if ln_part is not None else 0.0)
        PROFILE.end(key, ev, 2.0 * M * C_ * 4 * C_ * 2, nb)
    return y


def gemm_is_small(a: torch.Tensor, M: int, N: int, K: int) -> bool:
    """True if a bf16 plain GEMM of this size runs on the few-rows kernel on a's device (mage_gemm_is_small): its LayerNorm-consuming form
    then takes (mean, rstd) straight from the producer's partial sums (ln_part + ln_eps) and the mage_ln_stats launch can be skipped."""
    l, _ = _dev(a)
    r = l.mage_gemm_is_small(M, N, K)
    if r < 0:
        _lib.check(r, l)
    return r == 1


def _gemm_split(l, s, a, w, y, *, M, N, K, lda, ldy, out_h, out_w, in_h, in_w, a_img_stride, a_off, taps_h, taps_w, cin, y_img_stride, y_mul_y,
                y_mul_x, y_off, bias, act, rowadd, rowadd_div, rowadd_mod, residual, ldr, ldw, split_kind, y_split):
    """The split-precision form of mage_gemm (3 MFMA products per K slab, fp32-class result): plain rows or the padded-taps form."""
    sd = split_dtype(split_kind)
    assert a.dtype == sd and w.dtype == sd and (y.dtype == sd if y_split else y.dtype == torch.float32), (a.dtype, w.dtype, y.dtype)
    out_w = M if out_w is None else out_w
    in_h = out_h if in_h is None else in_h
    in_w = out_w if in_w is None else in_w
    d = GemmDesc()
    d.dtype, d.M, d.N, d.K = split_kind, M, N, K
    d.A, d.W, d.Y = a.data_ptr(), w.data_ptr(), y.data_ptr()
    d.lda, d.ldy, d.y_dtype = lda, ldy, (split_kind if y_split else F32)
    d.out_h, d.out_w, d.in_h, d.in_w = out_h, out_w, in_h, in_w
    d.a_img_stride = in_h * in_w if a_img_stride is None else a_img_stride
    d.a_off = a_off
    d.taps_h, d.taps_w, d.cin, d.stride = taps_h, taps_w, (K // (taps_h * taps_w) if cin is None else cin), 1
    d.dy0, d.dx0, d.dys, d.dxs = 0, 0, 1, 1
    d.y_img_stride = out_h * out_w if y_img_stride is None else y_img_stride
    d.y_mul_y = out_w if y_mul_y is None else y_mul_y
    d.y_mul_x, d.y_off = y_mul_x, y_off
    d.bias, d.act = _p(bias), act
    d.rowadd, d.rowadd_div, d.rowadd_mod = _p(rowadd), rowadd_div, rowadd_mod
    d.residual, d.ldr, d.res_dtype = _p(residual), ldr, F32
    d.ldw, d.n_split = ldw, 1
    if PROFILE.enabled:
        key = _kernel_name(l, d)
        if PROFILE.wants(key):
            ev = PROFILE.begin()
            _lib.check(l.mage_gemm(C.byref(d), s), l)
            nb = 4.0 * M * K + 4.0 * N * K + float(M) * N * 4 * (2 if residual is not None else 1)
            PROFILE.end(key, ev, 2.0 * M * N * K, nb)
            return y
    _lib.check(l.mage_gemm(C.byref(d), s), l)
    return y


def row_stats(x: torch.Tensor, eps: float, stats: torch.Tensor) -> torch.Tensor:
    """(mean, rstd) per row of bf16 rows x [rows, C] (mage_row_stats)."""
    l, s = _dev(x)
    assert x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 2 and x.stride(1) == 1 and stats.is_contiguous() and stats.numel() >= 2 * x.shape[0]
    ev = PROFILE.begin() if PROFILE.wants("layernorm") else None
    _lib.check(l.mage_row_stats(x.data_ptr(), code(x), x.shape[0], x.shape[1], x.stride(0), float(eps), stats.data_ptr(), s), l)
    if ev is not None:
        PROFILE.end("layernorm", ev, 0.0, float(x.numel()) * 2)
    return stats


def ln_stats(part: torch.Tensor, C_: int, eps: float, stats: torch.Tensor) -> torch.Tensor:
    """(mean, rstd) per row from a producer GEMM's partial sums ``part[n_slices, rows, 2]`` (slice-major; mage_ln_stats)."""
    l, s = _dev(part)
    n_slices, rows = part.shape[0], part.shape[1]
    assert part.dtype == torch.float32 and part.is_contiguous() and stats.is_contiguous() and stats.numel() >= 2 * rows
    if PROFILE.wants("ln_stats_kernel"):
        ev = PROFILE.begin()
        _lib.check(l.mage_ln_stats(part.data_ptr(), rows, n_slices, C_, eps, stats.data_ptr(), s), l)
        PROFILE.end("ln_stats_kernel", ev, 0.0)
        return stats
    _lib.check(l.mage_ln_stats(part.data_ptr(), rows, n_slices, C_, eps, stats.data_ptr(), s), l)
    return stats


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y: torch.Tensor, eps: float, split_kind: int = 0) -> torch.Tensor:
    """y = LayerNorm(x); split_kind BF16X3 / F16X3: y is a split-precision tensor [rows, 2C]."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous()
    Cc = x.shape[-1]
    assert not split_kind or (y.dtype == split_dtype(split_kind) and y.numel() == 2 * x.numel())
    ev = PROFILE.begin() if PROFILE.wants("layernorm") else None
    _lib.check(l.mage_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), split_kind or code(y),
                                x.numel() // Cc, Cc, float(eps), s), l)
    if ev is not None:
        PROFILE.end("layernorm", ev, 0.0, float(x.numel()) * (4 + y.element_size()))
    return y


def attention(q, k, v, out, *, ldq, ldk, ldv, ldo, n_seq, inner, nq, nk, n_head, q_outer_stride, q_axis_stride,
              kv_outer_stride, kv_axis_stride, causal=False, kv_len=None, kv_len_div=1, scale=None, out_split: int = 0,
              drop_p: float = 0.0, drop_seed: int = 0, split_kind: int = 0, o_outer_stride: int = 0, o_axis_stride: int = 0):
    """out_split BF16X3 / F16X3 (fp32 q, k, v): out is a split-precision tensor, ldo in 16-bit elements (2 * logical width).
    split_kind F16X3: q, k, v are split-precision tensors too (ld* in 16-bit elements; views start at 2 * the logical column)."""
    l, s = _dev(q)
    d = AttnDesc()
    d.dtype = split_kind or code(q)
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldv, d.ldo = ldq, ldk, ldv, ldo
    d.n_seq, d.inner, d.nq, d.nk, d.n_head = n_seq, inner, nq, nk, n_head
    d.q_outer_stride, d.q_axis_stride = q_outer_stride, q_axis_stride
    d.kv_outer_stride, d.kv_axis_stride = kv_outer_stride, kv_axis_stride
    d.causal = int(causal)
    d.kv_len, d.kv_len_div = _p(kv_len), kv_len_div
    d.scale = float(32 ** -0.5 if scale is None else scale)
    d.out_split = out_split
    d.drop_p, d.drop_seed = float(drop_p), int(drop_seed) & (2 ** 64 - 1)       # dropout on the probabilities (fp32 kernels; mage_hip.h)
    d.o_outer_stride, d.o_axis_stride = o_outer_stride, o_axis_stride            # out's own row map (0, 0: q's)
    ev = PROFILE.begin() if PROFILE.wants("attention") else None
    _lib.check(l.mage_attention(C.byref(d), s), l)
    if ev is not None:
        es = q.element_size()
        PROFILE.end("attention", ev, 4.0 * n_seq * nq * nk * n_head * 32, float(n_seq) * n_head * 32 * es * (2 * nq + 2 * nk))
    return out


def embedding(ids: torch.Tensor, table: torch.Tensor, out: torch.Tensor, *, relu: bool = False, group: Optional[int] = None,
              group_stride: Optional[int] = None, off: int = 0, inner: int = 0, inner_stride: int = 0, split_kind: int = 0) -> torch.Tensor:
    l, s = _dev(table)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and table.dtype == torch.float32 and table.is_contiguous()
    n = ids.numel()
    group = n if group is None else group
    group_stride = group if group_stride is None else group_stride
    _lib.check(l.mage_embedding(ids.data_ptr(), table.data_ptr(), out.data_ptr(), split_kind or code(out), n, table.shape[1],
                                table.shape[0], int(relu), group, group_stride, off, inner, inner_stride, s), l)
    return out


def table_conv(ids: torch.Tensor, table: torch.Tensor, y: torch.Tensor, *, n_img: int, H: int, W: int, taps: int = 3, pos=None, bias=None,
               relu: bool = False, rowadd=None, split_kind: int = 0,
               rowadd_div: int = 1, rowadd_mod: int = 1, ldy: Optional[int] = None, group: Optional[int] = None,
               y_group_stride: Optional[int] = None, y_off: int = 0) -> torch.Tensor:
    """y rows = pos + sum of table[tap][ids[neighbour]] + rowadd: a k x k convolution of embedding rows as a table sum (mage_table_conv)."""
    l, s = _dev(table)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == n_img * H * W
    assert table.dim() == 3 and table.shape[0] == taps * taps and table.is_contiguous()
    Cc = table.shape[2]
    group = n_img * H * W if group is None else group
    y_group_stride = group if y_group_stride is None else y_group_stride
    ev = PROFILE.begin() if PROFILE.wants("table_conv") else None
    _lib.check(l.mage_table_conv(ids.data_ptr(), n_img, H, W, taps, taps, table.data_ptr(), code(table), table.shape[1], Cc, _p(pos), _p(bias),
                                 int(relu), _p(rowadd), rowadd_div, rowadd_mod, y.data_ptr(), split_kind or code(y), Cc if ldy is None else ldy, group,
                                 y_group_stride, y_off, s), l)
    if ev is not None:
        PROFILE.end("table_conv", ev, 0.0, float(n_img) * H * W * Cc * (taps * taps * table.element_size() + 4))
    return y


def resblock_table(ids: torch.Tensor, table: torch.Tensor, codebook: torch.Tensor, w1: torch.Tensor, y: torch.Tensor, *, n_img: int, H: int, W: int,
                   bias3: torch.Tensor, b1: torch.Tensor, scale1=None, shift1=None, post_relu: bool = False, ldy: int, y_img_stride: int,
                   y_row_pitch: int, y_off: int = 0) -> torch.Tensor:
    """The first ResBlock of the f4 VQ-VAE decoder on codebook rows in one launch (mage_resblock_table): y rows (bf16, the interior of a
    zero-padded frame buffer) = relu(x + BN(conv1x1(relu(table sum)))), x = relu(codebook[ids])."""
    l, s = _dev(table)
    Cc = table.shape[2]
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == n_img * H * W
    assert table.dtype == torch.bfloat16 and table.dim() == 3 and table.shape[0] == 9 and table.is_contiguous()
    assert codebook.dtype == torch.float32 and codebook.is_contiguous() and tuple(codebook.shape) == (table.shape[1], Cc)
    assert w1.dtype == torch.bfloat16 and w1.is_contiguous() and tuple(w1.shape) == (Cc, Cc) and y.dtype == torch.bfloat16
    ev = PROFILE.begin() if PROFILE.wants("resblock_table") else None
    _lib.check(l.mage_resblock_table(ids.data_ptr(), n_img, H, W, table.data_ptr(), table.shape[1], Cc, bias3.data_ptr(), codebook.data_ptr(),
                                     w1.data_ptr(), b1.data_ptr(), _p(scale1), _p(shift1), int(post_relu), y.data_ptr(), ldy, y_img_stride,
                                     y_row_pitch, y_off, s), l)
    if ev is not None:
        npix = float(n_img) * H * W
        PROFILE.end("resblock_table", ev, 2.0 * npix * Cc * Cc, npix * (8 + 2 * Cc))       # HBM: the ids in, the bf16 rows out
    return y


def resblock_rows(t: torch.Tensor, w1: torch.Tensor, residual: torch.Tensor, y: torch.Tensor, *, n_img: int, H: int, W: int, b1: torch.Tensor,
                  scale1=None, shift1=None, post_relu: bool = False, lda: int, ldr: int, ldy: int, img_stride: int, row_pitch: int,
                  off: int = 0) -> torch.Tensor:
    """y = relu(x + BN(conv1x1(t))) on bf16 rows, x and y in (padded) frame buffers (mage_resblock_rows): the tail of a ResBlock."""
    l, s = _dev(t)
    Cc = w1.shape[0]
    assert t.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
    assert w1.is_contiguous() and tuple(w1.shape) == (Cc, Cc)
    ev = PROFILE.begin() if PROFILE.wants("resblock_rows") else None
    _lib.check(l.mage_resblock_rows(t.data_ptr(), lda, w1.data_ptr(), b1.data_ptr(), _p(scale1), _p(shift1), residual.data_ptr(), ldr,
                                    int(post_relu), y.data_ptr(), ldy, n_img, H, W, Cc, img_stride, row_pitch, off, s), l)
    if ev is not None:
        npix = float(n_img) * H * W
        PROFILE.end("resblock_rows", ev, 2.0 * npix * Cc * Cc, npix * 3 * 2 * Cc)
    return y


def vq_prepare(codebook: torch.Tensor):
    l, s = _dev(codebook)
    K, D = codebook.shape
    cbt = torch.empty(D, K, device=codebook.device, dtype=torch.float32)
    c2 = torch.empty(K, device=codebook.device, dtype=torch.float32)
    _lib.check(l.mage_vq_prepare(codebook.contiguous().data_ptr(), K, D, cbt.data_ptr(), c2.data_ptr(), s), l)
    return cbt, c2


def vq_nearest(z: torch.Tensor, cbt: torch.Tensor, c2: torch.Tensor, want_margin: bool = False):
    l, s = _dev(z)
    assert z.dtype == torch.float32 and z.is_contiguous()
    D, K = cbt.shape
    M = z.numel() // D
    idx = torch.empty(M, device=z.device, dtype=torch.int64)
    margin = torch.empty(M, device=z.device, dtype=torch.float32) if want_margin else None
    _lib.check(l.mage_vq_nearest(z.data_ptr(), cbt.data_ptr(), c2.data_ptr(), M, D, K, idx.data_ptr(), _p(margin), s), l)
    return (idx, margin) if want_margin else idx


def argmax(logits: torch.Tensor, out: torch.Tensor, *, rows: int, K: int, ld: Optional[int] = None, group: Optional[int] = None,
           in_group_stride: Optional[int] = None, in_off: int = 0, out_group_stride: Optional[int] = None, out_off: int = 0,
           margin=None) -> torch.Tensor:
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and out.dtype == torch.int64
    group = rows if group is None else group
    in_group_stride = group if in_group_stride is None else in_group_stride
    out_group_stride = group if out_group_stride is None else out_group_stride
    _lib.check(l.mage_argmax(logits.data_ptr(), rows, K, K if ld is None else ld, group, in_group_stride, in_off,
                             out.data_ptr(), out_group_stride, out_off, _p(margin), s), l)
    return out


def sample_tokens(logits: torch.Tensor, out: torch.Tensor, seeds: torch.Tensor, *, rows: int, K: int, temperature: float = 1.0,
                  top_k: int = 0, top_p: float = 1.0, pos_off: int = 0, ld: Optional[int] = None, group: Optional[int] = None,
                  in_group_stride: Optional[int] = None, in_off: int = 0, out_group_stride: Optional[int] = None,
                  out_off: int = 0) -> torch.Tensor:
    """argmax's row addressing; row i draws with seeds[i // group] at position pos_off + i % group (mage_sample_tokens)."""
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and out.dtype == torch.int64 and seeds.dtype == torch.int64 and seeds.is_contiguous()
    group = rows if group is None else group
    in_group_stride = group if in_group_stride is None else in_group_stride
    out_group_stride = group if out_group_stride is None else out_group_stride
    assert seeds.device == logits.device and seeds.numel() >= (rows + group - 1) // group
    _lib.check(l.mage_sample_tokens(logits.data_ptr(), rows, K, K if ld is None else ld, group, in_group_stride, in_off,
                                    out.data_ptr(), out_group_stride, out_off, seeds.data_ptr(), pos_off, float(temperature),
                                    int(top_k), float(top_p), s), l)
    return out


def video_noise(seeds: torch.Tensor, *, C: int, h: int, w: int, nchw: bool = True, rows: bool = True):
    """(noise fp32 [B, C, h, w] or None, the same values as channel-last rows fp32 [B*h*w, C] or None) of int64 seeds [B] on the GPU: clip b's
    standard-normal noise under seeds[b] (mage_video_noise: one launch, both layouts bit-equal)."""
    l, s = _dev(seeds)
    assert seeds.dtype == torch.int64 and seeds.dim() == 1 and seeds.is_contiguous() and (nchw or rows)
    B = seeds.shape[0]
    a = torch.empty(B, C, h, w, device=seeds.device, dtype=torch.float32) if nchw else None
    r = torch.empty(B * h * w, C, device=seeds.device, dtype=torch.float32) if rows else None
    _lib.check(l.mage_video_noise(seeds.data_ptr(), B, C, h * w, _p(a), _p(r), s), l)
    return a, r


def token_logprob(logits: torch.Tensor, tokens: torch.Tensor, logprob: torch.Tensor, *, rows: int, K: int, ld: Optional[int] = None,
                  group: Optional[int] = None, in_group_stride: Optional[int] = None, in_off: int = 0,
                  tok_group_stride: Optional[int] = None, tok_off: int = 0) -> torch.Tensor:
    """argmax's input addressing; row i scores tokens[(i // group) * tok_group_stride + i % group + tok_off] and writes the same index of
    logprob (mage_token_logprob).  tokens / logprob are addressed from their first element: pass a flat slice to shift one against the other."""
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and tokens.dtype == torch.int64 and logprob.dtype == torch.float32
    assert tokens.device == logits.device and logprob.device == logits.device
    group = rows if group is None else group
    in_group_stride = group if in_group_stride is None else in_group_stride
    tok_group_stride = group if tok_group_stride is None else tok_group_stride
    last = ((rows - 1) // group) * tok_group_stride + (rows - 1) % group + tok_off          # the largest index addressed
    assert tok_off >= 0 and last < tokens.numel() and last < logprob.numel()
    _lib.check(l.mage_token_logprob(logits.data_ptr(), rows, K, K if ld is None else ld, group, in_group_stride, in_off, tokens.data_ptr(),
                                    logprob.data_ptr(), tok_group_stride, tok_off, s), l)
    return logprob


def token_stats(logits: torch.Tensor, tokens: Optional[torch.Tensor], *, rows: int, K: int, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 1.0, policy_logprob: Optional[torch.Tensor] = None, policy_entropy: Optional[torch.Tensor] = None,
                kept: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None, ld: Optional[int] = None,
                group: Optional[int] = None, in_group_stride: Optional[int] = None, in_off: int = 0,
                tok_group_stride: Optional[int] = None, tok_off: int = 0) -> None:
    """token_logprob's addressing and sample_tokens' parameters; row i writes index (i // group) * tok_group_stride + i % group + tok_off of
    every output given (mage_token_stats): policy_logprob fp32 (needs tokens), policy_entropy fp32, kept int32 -- under the set the sampler
    draws from -- and entropy fp32 (the whole row at temperature 1).  At least one output."""
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and (tokens is None or (tokens.dtype == torch.int64 and tokens.device == logits.device))
    group = rows if group is None else group
    in_group_stride = group if in_group_stride is None else in_group_stride
    tok_group_stride = group if tok_group_stride is None else tok_group_stride
    last = ((rows - 1) // group) * tok_group_stride + (rows - 1) % group + tok_off          # the largest index addressed
    assert tok_off >= 0 and (tokens is None or last < tokens.numel())
    for o, dt in ((policy_logprob, torch.float32), (policy_entropy, torch.float32), (kept, torch.int32), (entropy, torch.float32)):
        assert o is None or (o.dtype == dt and o.device == logits.device and last < o.numel())
    _lib.check(l.mage_token_stats(logits.data_ptr(), rows, K, K if ld is None else ld, group, in_group_stride, in_off, _p(tokens),
                                  tok_group_stride, tok_off, float(temperature), int(top_k), float(top_p), _p(policy_logprob),
                                  _p(policy_entropy), _p(kept), _p(entropy), s), l)


def guide_logits(cond: torch.Tensor, uncond: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None, *, rows: int, K: int,
                 scale_div: int, ld: Optional[int] = None, group: Optional[int] = None, in_group_stride: Optional[int] = None,
                 in_off: int = 0) -> torch.Tensor:
    """Classifier-free guidance, z = c + (scale - 1)(c - u) (mage_guide_logits): argmax's input addressing in all three buffers, each
    addressed from its first element; row i uses scale[i // scale_div].  out None: in place on cond."""
    l, s = _dev(cond)
    out = cond if out is None else out
    assert cond.dtype == uncond.dtype == out.dtype == scale.dtype == torch.float32 and scale.is_contiguous()
    assert uncond.device == cond.device and out.device == cond.device and scale.device == cond.device
    ld = K if ld is None else ld
    group = rows if group is None else group
    in_group_stride = group if in_group_stride is None else in_group_stride
    end = (((rows - 1) // group) * in_group_stride + (rows - 1) % group + in_off) * ld + K       # one past the last element addressed
    assert in_off >= 0 and end <= min(cond.numel(), uncond.numel(), out.numel()) and scale.numel() >= (rows - 1) // scale_div + 1
    _lib.check(l.mage_guide_logits(cond.data_ptr(), uncond.data_ptr(), out.data_ptr(), rows, K, ld, group, in_group_stride, in_off,
                                   scale.data_ptr(), scale_div, s), l)
    return out


def apply_known_tokens(tokens: torch.Tensor, known: torch.Tensor, *, rows: int, K: int, group: Optional[int] = None,
                       tok_group_stride: Optional[int] = None, tok_off: int = 0, known_group_stride: Optional[int] = None, known_off: int = 0,
                       known_clip_div: int = 1, logprob: Optional[torch.Tensor] = None, policy_logprob: Optional[torch.Tensor] = None,
                       entropy: Optional[torch.Tensor] = None, policy_entropy: Optional[torch.Tensor] = None,
                       kept: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Given tokens over picked ones (mage_apply_known_tokens): row i reads known[((i // group) // known_clip_div) * known_group_stride +
    i % group + known_off]; a value >= 0 is stored at token_logprob's index (i // group) * tok_group_stride + i % group + tok_off of tokens, and
    that index of every result given gets the certain policy's value (log-probabilities and entropies 0, kept 1).  A negative value leaves the
    slot as it is.  Every buffer is addressed from its first element."""
    l, s = _dev(tokens)
    assert tokens.dtype == torch.int64 and known.dtype == torch.int64 and known.device == tokens.device
    group = max(rows, 1) if group is None else group
    tok_group_stride = group if tok_group_stride is None else tok_group_stride
    known_group_stride = group if known_group_stride is None else known_group_stride
    if rows > 0:
        c, j = (rows - 1) // group, (rows - 1) % group
        full = group - 1 if c > 0 else j                                                      # a full group before a partial last one
        last = max(c * tok_group_stride + j, (c - 1) * tok_group_stride + full) + tok_off     # the largest index addressed
        assert tok_off >= 0 and known_off >= 0 and last < tokens.numel()
        kc, kp = c // known_clip_div, (c - 1) // known_clip_div
        assert max(kc * known_group_stride + j, kp * known_group_stride + full) + known_off < known.numel()
        for o, dt in ((logprob, torch.float32), (policy_logprob, torch.float32), (entropy, torch.float32), (policy_entropy, torch.float32),
                      (kept, torch.int32)):
            assert o is None or (o.dtype == dt and o.device == tokens.device and last < o.numel())
    _lib.check(l.mage_apply_known_tokens(tokens.data_ptr(), rows, group, tok_group_stride, tok_off, known.data_ptr(), known_group_stride,
                                         known_off, known_clip_div, K, _p(logprob), _p(policy_logprob), _p(entropy), _p(policy_entropy),
                                         _p(kept), s), l)
    return tokens


def _policy_args(logits, tokens, advantage, behaviour_logprob, adv_div):
    """The asserts policy_loss and policy_loss_bwd share; returns (rows, K, ld, adv_div).  adv_div None: advantage's entries share the rows
    out equally (one per row, or one per clip)."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, K = logits.shape
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() == rows and tokens.device == logits.device
    assert advantage.dtype == torch.float32 and advantage.is_contiguous() and advantage.device == logits.device
    if adv_div is None:
        assert advantage.numel() > 0 and rows % advantage.numel() == 0, "one advantage per row, or per equal group of consecutive rows"
        adv_div = rows // advantage.numel()
    assert adv_div > 0 and (rows - 1) // adv_div < advantage.numel()         # the largest index addressed
    if behaviour_logprob is not None:
        assert behaviour_logprob.dtype == torch.float32 and behaviour_logprob.is_contiguous() and behaviour_logprob.numel() == rows
        assert behaviour_logprob.device == logits.device
    return rows, K, logits.stride(0), adv_div


def _policy_ref(reference_logprob, kl_coef, logits):
    """The reference log-probabilities of the anchored pair: None (and then no kl_coef), or fp32 [rows] beside the logits."""
    if reference_logprob is None:
        if kl_coef != 0:
            raise ValueError("policy_loss: kl_coef needs reference_logprob (the penalty is against a reference policy)")
        return
    assert reference_logprob.dtype == torch.float32 and reference_logprob.is_contiguous() and reference_logprob.numel() == logits.shape[0]
    assert reference_logprob.device == logits.device


def _given_rows(given, logits):
    """The per-row mask of the masked entry points: None, or bool / uint8 [rows] (any shape, contiguous) beside the logits."""
    if given is not None:
        assert given.dtype in (torch.bool, torch.uint8) and given.is_contiguous() and given.numel() == logits.shape[0]
        assert given.device == logits.device


def _ratio_div(ratio_div, rows, adv_div, behaviour_logprob) -> int:
    """The grouped pair's own rules (the library states them again): a ratio to group, groups that tile the rows inside one advantage each."""
    if behaviour_logprob is None:
        raise ValueError("policy_loss: ratio_div needs behaviour_logprob (without one there is no ratio to group)")
    if isinstance(ratio_div, bool) or not isinstance(ratio_div, int) or ratio_div < 1:
        raise ValueError(f"policy_loss: ratio_div must be an int >= 1, got {ratio_div!r}")
    if rows % ratio_div or adv_div % ratio_div:
        raise ValueError(f"policy_loss: rows={rows} and adv_div={adv_div} must be multiples of ratio_div={ratio_div} (a group has one advantage)")
    return ratio_div


# The four pairs of entry points: form -> (forward symbol; the backward one is it + "_bwd", summary length, outputs besides 'kl').  A call
# has a reference, a mask and a group or not; the pair that takes the most of what is there serves it.
_POLICY_FORMS = {"plain": ("mage_policy_loss", 5, ()), "anchored": ("mage_policy_loss_anchored", 7, ()),
                 "masked": ("mage_policy_loss_masked", 8, ("norm",)),
                 "grouped": ("mage_policy_loss_grouped", 8, ("norm", "group_logratio", "group_count"))}


def _policy_form(reference_logprob, given, ratio_div) -> str:
    return "grouped" if ratio_div is not None else "masked" if given is not None else "anchored" if reference_logprob is not None else "plain"


def _policy_prefix(logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob) -> list:
    """The arguments all eight entry points begin with."""
    return [logits.data_ptr(), rows, K, ld, tokens.data_ptr(), advantage.data_ptr(), adv_div, _p(behaviour_logprob)]


def policy_loss(logits: torch.Tensor, tokens: torch.Tensor, advantage: torch.Tensor, behaviour_logprob: Optional[torch.Tensor] = None, *,
                temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, clip_lo: float = 0.2, clip_hi: float = 0.2,
                entropy_coef: float = 0.0, adv_div: Optional[int] = None, reference_logprob: Optional[torch.Tensor] = None,
                kl_coef: float = 0.0, given: Optional[torch.Tensor] = None, ratio_div: Optional[int] = None) -> dict:
    """mage_policy_loss over logits [rows, K] fp32 (row stride >= K) and tokens int64 [rows]; advantage fp32, row i using entry i // adv_div
    (default: rows / numel consecutive rows per entry); behaviour_logprob fp32 [rows] selects the clipped surrogate, None the reward-weighted likelihood.  Returns the per-row
    fp32 tensors 'row_loss', 'logprob', 'entropy', the uint32 thresholds 'cut' (kept as int32 storage: policy_loss_bwd's input) and
    'summary' fp32 [5]: the means of the loss, the entropy, b - logprob, the clipped share and the outside share.
    reference_logprob fp32 [rows] (with kl_coef >= 0): mage_policy_loss_anchored -- the loss gains kl_coef times the k3 estimate of the KL
    against the reference policy, the result the per-row 'kl', and 'summary' is fp32 [7]: the five, the mean KL and the unanchored share.
    given bool [rows] (True: the row's token was given, not drawn): mage_policy_loss_masked in either form -- a given row is not read and
    gets zeros, 'summary' is fp32 [8]: the seven means over the free rows (the last two 0 without a reference) and the given share, and the
    result gains 'norm' fp32 [1] = 1 / the number of free rows, policy_loss_bwd's input.
    ratio_div (None: the dispatch above, untouched): mage_policy_loss_grouped -- one importance ratio per group of ratio_div consecutive rows
    (behaviour_logprob required; rows and adv_div multiples of ratio_div), with or without given and a reference; the masked call's results
    plus 'group_logratio' fp32 and 'group_count' int32 [rows / ratio_div], policy_loss_bwd's input and the counted rows per group."""
    _policy_ref(reference_logprob, kl_coef, logits)
    _given_rows(given, logits)
    l, s = _dev(logits)
    rows, K, ld, adv_div = _policy_args(logits, tokens, advantage, behaviour_logprob, adv_div)
    form = _policy_form(reference_logprob, given, ratio_div)
    entry, n_summary, extra = _POLICY_FORMS[form]
    mk = lambda n, dt: torch.empty(n, device=logits.device, dtype=dt)      # noqa: E731
    out = dict(row_loss=mk(rows, torch.float32), logprob=mk(rows, torch.float32), entropy=mk(rows, torch.float32), cut=mk(rows, torch.int32),
               summary=mk(n_summary, torch.float32))
    groups = 0
    if form == "grouped":
        ratio_div = _ratio_div(ratio_div, rows, adv_div, behaviour_logprob)
        groups = rows // ratio_div
    sizes = dict(norm=(1, torch.float32), group_logratio=(groups, torch.float32), group_count=(groups, torch.int32))
    out.update({k: mk(*sizes[k]) for k in extra})
    if reference_logprob is not None:
        out["kl"] = mk(rows, torch.float32)
    plain = form == "plain"                                                 # the one entry point without the reference's three arguments
    args = _policy_prefix(logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob) + ([] if plain else [_p(reference_logprob)])
    args += [float(temperature), int(top_k), float(top_p), float(clip_lo), float(clip_hi), float(entropy_coef)]
    args += ([] if plain else [float(kl_coef)]) + [out[k].data_ptr() for k in ("row_loss", "logprob", "entropy", "cut")]
    args += ([] if plain else [_p(out.get("kl"))]) + [out["summary"].data_ptr()]
    if form in ("masked", "grouped"):
        args += [out["norm"].data_ptr(), _p(given)]
    if form == "grouped":
        args += [ratio_div, out["group_logratio"].data_ptr(), out["group_count"].data_ptr()]
    _lib.check(getattr(l, entry)(*args, s), l)
    return out


def policy_loss_bwd(logits: torch.Tensor, tokens: torch.Tensor, advantage: torch.Tensor, behaviour_logprob: Optional[torch.Tensor],
                    cut: torch.Tensor, grad_out: torch.Tensor, dlogits: torch.Tensor, *, temperature: float = 1.0, clip_lo: float = 0.2,
                    clip_hi: float = 0.2, entropy_coef: float = 0.0, adv_div: Optional[int] = None,
                    reference_logprob: Optional[torch.Tensor] = None, kl_coef: float = 0.0, given: Optional[torch.Tensor] = None,
                    norm: Optional[torch.Tensor] = None, ratio_div: Optional[int] = None,
                    group_logratio: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mage_policy_loss_bwd: dlogits [rows, K] contiguous fp32 or bf16 from policy_loss' inputs and its 'cut'; grad_out fp32 [1].  With
    reference_logprob: mage_policy_loss_anchored_bwd.  With given (and the masked policy_loss' 'norm'): mage_policy_loss_masked_bwd.  With
    ratio_div (and the grouped policy_loss' 'norm' and 'group_logratio'; given or not): mage_policy_loss_grouped_bwd."""
    _policy_ref(reference_logprob, kl_coef, logits)
    _given_rows(given, logits)
    assert (ratio_div is None) == (group_logratio is None), "ratio_div and group_logratio come together (the grouped forward call writes it)"
    assert (given is None and ratio_div is None) == (norm is None), "given / ratio_div and norm come together (the forward call writes norm)"
    l, s = _dev(logits)
    rows, K, ld, adv_div = _policy_args(logits, tokens, advantage, behaviour_logprob, adv_div)
    assert cut.dtype == torch.int32 and cut.is_contiguous() and cut.numel() == rows and cut.device == logits.device
    assert grad_out.dtype == torch.float32 and grad_out.numel() == 1 and grad_out.device == logits.device
    assert dlogits.dtype in (torch.float32, torch.bfloat16) and dlogits.is_contiguous() and dlogits.numel() == rows * K
    assert dlogits.device == logits.device
    form = _policy_form(reference_logprob, given, ratio_div)
    if form == "grouped":
        ratio_div = _ratio_div(ratio_div, rows, adv_div, behaviour_logprob)
    if norm is not None:
        assert norm.dtype == torch.float32 and norm.numel() == 1 and norm.device == logits.device
    if form == "grouped":
        assert group_logratio.dtype == torch.float32 and group_logratio.is_contiguous() and group_logratio.numel() == rows // ratio_div
        assert group_logratio.device == logits.device
    plain = form == "plain"
    args = _policy_prefix(logits, rows, K, ld, tokens, advantage, adv_div, behaviour_logprob) + ([] if plain else [_p(reference_logprob)])
    args += [cut.data_ptr(), float(temperature), float(clip_lo), float(clip_hi), float(entropy_coef)] + ([] if plain else [float(kl_coef)])
    args += [grad_out.data_ptr()] + ([norm.data_ptr()] if form in ("masked", "grouped") else []) + [dlogits.data_ptr(), code(dlogits)]
    if form in ("masked", "grouped"):
        args += [_p(given)]
    if form == "grouped":
        args += [ratio_div, group_logratio.data_ptr()]
    _lib.check(getattr(l, _POLICY_FORMS[form][0] + "_bwd")(*args, s), l)
    return dlogits


def preference_loss(clip_logprob: torch.Tensor, reference_logprob: torch.Tensor, pairs: torch.Tensor, *, beta: float = 0.1,
                    label_smoothing: float = 0.0, mode: int = 0) -> dict:
    """mage_preference_loss: the pair stage of DPO (mode 0) / IPO (mode 1) over clip_logprob and reference_logprob fp32 [clips] and pairs
    int64 [n_pairs, 2] (chosen row, rejected row).  Returns fp32 'pair_loss' and 'pair_margin' [n_pairs], 'clip_coef' [clips] (the derivative
    of the mean loss with respect to clip_logprob: token_logprob_bwd's weights) and 'summary' [5]: the means of the loss, the accuracy, the
    chosen reward, the rejected reward and the margin."""
    l, s = _dev(clip_logprob)
    clips = clip_logprob.numel()
    for x in (clip_logprob, reference_logprob):
        assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == clips and x.device == clip_logprob.device
    assert pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.is_contiguous()
    assert pairs.device == clip_logprob.device
    P = pairs.shape[0]
    mk = lambda n: torch.empty(n, device=clip_logprob.device, dtype=torch.float32)      # noqa: E731
    out = dict(pair_loss=mk(P), pair_margin=mk(P), clip_coef=mk(clips), summary=mk(5))
    _lib.check(l.mage_preference_loss(clip_logprob.data_ptr(), reference_logprob.data_ptr(), clips, pairs.data_ptr(), P, float(beta),
                                      float(label_smoothing), int(mode), out["pair_loss"].data_ptr(), out["pair_margin"].data_ptr(),
                                      out["clip_coef"].data_ptr(), out["summary"].data_ptr(), s), l)
    return out


def token_logprob_bwd(logits: torch.Tensor, tokens: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor, dlogits: torch.Tensor, *,
                      weight_div: Optional[int] = None, given: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mage_token_logprob_bwd: dlogits [rows, K] contiguous fp32 or bf16, the gradient of sum_i weight[i // weight_div] * token_logprob_i
    times grad_out (fp32 [1]) over logits [rows, K] fp32 (row stride >= K) and tokens int64 [rows].  weight_div None: weight's entries share
    the rows out equally (one per row, or one per clip).  Rows of weight 0 are written as zeros without being read.  given bool [rows]:
    mage_token_logprob_bwd_masked -- a given row is a row of weight 0."""
    _given_rows(given, logits)
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, K = logits.shape
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() == rows and tokens.device == logits.device
    assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.device == logits.device
    if weight_div is None:
        assert weight.numel() > 0 and rows % weight.numel() == 0, "one weight per row, or per equal group of consecutive rows"
        weight_div = rows // weight.numel()
    assert weight_div > 0 and (rows - 1) // weight_div < weight.numel()      # the largest index addressed
    assert grad_out.dtype == torch.float32 and grad_out.numel() == 1 and grad_out.device == logits.device
    assert dlogits.dtype in (torch.float32, torch.bfloat16) and dlogits.is_contiguous() and dlogits.numel() == rows * K
    assert dlogits.device == logits.device
    if given is not None:
        _lib.check(l.mage_token_logprob_bwd_masked(logits.data_ptr(), rows, K, logits.stride(0), tokens.data_ptr(), weight.data_ptr(), weight_div,
                                                   grad_out.data_ptr(), dlogits.data_ptr(), code(dlogits), given.data_ptr(), s), l)
        return dlogits
    _lib.check(l.mage_token_logprob_bwd(logits.data_ptr(), rows, K, logits.stride(0), tokens.data_ptr(), weight.data_ptr(), weight_div,
                                        grad_out.data_ptr(), dlogits.data_ptr(), code(dlogits), s), l)
    return dlogits


def _distill_args(logits, teacher, given):
    """The asserts distill_loss and distill_loss_bwd share; returns (rows, K)."""
    _given_rows(given, logits)
    for x in (logits, teacher):
        assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.device == logits.device
    assert teacher.shape == logits.shape, "one teacher row per student row"
    return logits.shape


def distill_loss(logits: torch.Tensor, teacher: torch.Tensor, *, temperature: float = 1.0, mode: int = 0,
                 given: Optional[torch.Tensor] = None) -> dict:
    """mage_distill_loss over student logits and teacher logits, both [rows, K] fp32 (row strides >= K, each its own): the per-row KL at
    `temperature`, mode 0 KL(teacher || student), mode 1 KL(student || teacher).  Returns fp32 'row_kl' [rows], 'summary' [5] (the means over
    the free rows of the KL, the teacher's entropy, the student's entropy and the argmax agreement; the given share) and 'norm' [1] = 1 / the
    number of free rows, distill_loss_bwd's input.  given bool [rows] (True: the row is left out, not read, and gets zeros); None: every row
    is free."""
    rows, K = _distill_args(logits, teacher, given)
    l, s = _dev(logits)
    mk = lambda n: torch.empty(n, device=logits.device, dtype=torch.float32)      # noqa: E731
    out = dict(row_kl=mk(rows), summary=mk(5), norm=mk(1))
    _lib.check(l.mage_distill_loss(logits.data_ptr(), rows, K, logits.stride(0), teacher.data_ptr(), teacher.stride(0), float(temperature),
                                   int(mode), _p(given), out["row_kl"].data_ptr(), out["summary"].data_ptr(), out["norm"].data_ptr(), s), l)
    return out


def distill_loss_bwd(logits: torch.Tensor, teacher: torch.Tensor, row_kl: torch.Tensor, norm: torch.Tensor, grad_out: torch.Tensor,
                     dlogits: torch.Tensor, *, temperature: float = 1.0, mode: int = 0, given: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mage_distill_loss_bwd: dlogits [rows, K] contiguous fp32 or bf16, the gradient of grad_out (fp32 [1]) times distill_loss' mean KL with
    respect to the student's logits, from distill_loss' inputs and its 'row_kl' and 'norm'."""
    rows, K = _distill_args(logits, teacher, given)
    l, s = _dev(logits)
    assert row_kl.dtype == torch.float32 and row_kl.is_contiguous() and row_kl.numel() == rows and row_kl.device == logits.device
    for x in (norm, grad_out):
        assert x.dtype == torch.float32 and x.numel() == 1 and x.device == logits.device
    assert dlogits.dtype in (torch.float32, torch.bfloat16) and dlogits.is_contiguous() and dlogits.numel() == rows * K
    assert dlogits.device == logits.device
    _lib.check(l.mage_distill_loss_bwd(logits.data_ptr(), rows, K, logits.stride(0), teacher.data_ptr(), teacher.stride(0), float(temperature),
                                       int(mode), _p(given), row_kl.data_ptr(), grad_out.data_ptr(), norm.data_ptr(), dlogits.data_ptr(),
                                       code(dlogits), s), l)
    return dlogits


def _xent_args(logits, target, class_weight, given):
    """The asserts token_xent and token_xent_bwd share; returns (rows, K)."""
    _given_rows(given, logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, K = logits.shape
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == rows and target.device == logits.device
    if class_weight is not None:
        assert class_weight.dtype == torch.float32 and class_weight.is_contiguous() and tuple(class_weight.shape) == (K,)
        assert class_weight.device == logits.device
    return rows, K


def token_xent(logits: torch.Tensor, target: torch.Tensor, *, class_weight: Optional[torch.Tensor] = None, label_smoothing: float = 0.0,
               z_loss: float = 0.0, given: Optional[torch.Tensor] = None, rank: bool = True) -> dict:
    """mage_token_xent over logits [rows, K] fp32 (row stride >= K) and target int64 [rows]: F.cross_entropy(weight=class_weight (fp32 [K]),
    label_smoothing=) per row with the rows of `given` (bool [rows]) left out as by ignore_index, plus z_loss * mean(logsumexp^2).  Returns
    fp32 'row_loss', 'row_nll' (= -token_logprob, bit for bit), 'row_lse' [rows], int32 'rank' [rows] (the target's rank among the row's
    logits, 0: the argmax; None with rank=False), 'summary' [5] (the objective, the mean nll, the accuracy, the mean lse^2, the given share)
    and 'norm' [2] (1 / the free rows' weight, 1 / their number), token_xent_bwd's input."""
    rows, K = _xent_args(logits, target, class_weight, given)
    l, s = _dev(logits)
    mk = lambda n: torch.empty(n, device=logits.device, dtype=torch.float32)      # noqa: E731
    out = dict(row_loss=mk(rows), row_nll=mk(rows), row_lse=mk(rows),
               rank=torch.empty(rows, device=logits.device, dtype=torch.int32) if rank else None, summary=mk(5), norm=mk(2))
    _lib.check(l.mage_token_xent(logits.data_ptr(), rows, K, logits.stride(0), target.data_ptr(), _p(class_weight), float(label_smoothing),
                                 float(z_loss), _p(given), out["row_loss"].data_ptr(), out["row_nll"].data_ptr(), out["row_lse"].data_ptr(),
                                 _p(out["rank"]), out["summary"].data_ptr(), out["norm"].data_ptr(), s), l)
    return out


def token_xent_bwd(logits: torch.Tensor, target: torch.Tensor, norm: torch.Tensor, grad_out: torch.Tensor, dlogits: torch.Tensor, *,
                   class_weight: Optional[torch.Tensor] = None, label_smoothing: float = 0.0, z_loss: float = 0.0,
                   given: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mage_token_xent_bwd: dlogits [rows, K] contiguous fp32 or bf16, the gradient of grad_out (fp32 [1]) times token_xent's summary[0] with
    respect to the logits, from token_xent's inputs and its 'norm'."""
    rows, K = _xent_args(logits, target, class_weight, given)
    l, s = _dev(logits)
    assert norm.dtype == torch.float32 and norm.numel() == 2 and norm.is_contiguous() and norm.device == logits.device
    assert grad_out.dtype == torch.float32 and grad_out.numel() == 1 and grad_out.device == logits.device
    assert dlogits.dtype in (torch.float32, torch.bfloat16) and dlogits.is_contiguous() and dlogits.numel() == rows * K
    assert dlogits.device == logits.device
    _lib.check(l.mage_token_xent_bwd(logits.data_ptr(), rows, K, logits.stride(0), target.data_ptr(), _p(class_weight), float(label_smoothing),
                                     float(z_loss), _p(given), grad_out.data_ptr(), norm.data_ptr(), dlogits.data_ptr(), code(dlogits), s), l)
    return dlogits


def clip_scores(logprob: torch.Tensor, *, n_clips: int, n_cand: int = 1):
    """(scores [n_clips, n_cand] fp32, best [n_clips] int64 or None when n_cand == 1) of logprob [n_clips * n_cand, ...] fp32
    (mage_clip_scores)."""
    l, s = _dev(logprob)
    assert logprob.dtype == torch.float32 and logprob.is_contiguous() and logprob.numel() % (n_clips * n_cand) == 0
    scores = torch.empty(n_clips, n_cand, device=logprob.device, dtype=torch.float32)
    best = torch.empty(n_clips, device=logprob.device, dtype=torch.int64) if n_cand > 1 else None
    _lib.check(l.mage_clip_scores(logprob.data_ptr(), n_clips, n_cand, logprob.numel() // (n_clips * n_cand), scores.data_ptr(), _p(best), s), l)
    return scores, best


def _frames_ok(x: torch.Tensor) -> bool:
    """[clips, T, C, H, W] fp32 with every clip's T*C*H*W values contiguous (the clips themselves may lie further apart)."""
    if not (x.dtype == torch.float32 and x.dim() == 5 and x.numel() > 0):
        return False
    want = 1
    for n, st in zip(reversed(x.shape[1:]), reversed(x.stride()[1:])):
        if n != 1 and st != want:
            return False
        want *= n
    return x.shape[0] == 1 or x.stride(0) >= want


def video_metrics(video: torch.Tensor, target: torch.Tensor, *, tgt_div: int = 1, data_range: float = 2.0, mse: bool = True, psnr: bool = True,
                  ssim: bool = True) -> dict:
    """Per-frame metrics of video [clips, T, C, H, W] fp32 against target [>= ceil(clips / tgt_div), T, C, H, W] fp32, video clip r against
    target clip r // tgt_div (mage_video_metrics).  Either side may be a view whose clips lie further apart than T*C*H*W (batch['images'][:, 1:]).
    Returns the outputs asked for, fp32 [clips, T] each, under 'mse', 'psnr', 'ssim'."""
    l, s = _dev(video)
    assert _frames_ok(video) and _frames_ok(target) and target.device == video.device and target.shape[1:] == video.shape[1:]
    clips, T, C, H, W = video.shape
    assert tgt_div >= 1 and (clips - 1) // tgt_div < target.shape[0]                           # the last target clip addressed
    out = {n: torch.empty(clips, T, device=video.device, dtype=torch.float32) for n, on in (("mse", mse), ("psnr", psnr), ("ssim", ssim)) if on}
    _lib.check(l.mage_video_metrics(video.data_ptr(), max(video.stride(0), video[0].numel()), target.data_ptr(),
                                    max(target.stride(0), target[0].numel()), clips, T, C, H, W, int(tgt_div), float(data_range),
                                    _p(out.get("mse")), _p(out.get("psnr")), _p(out.get("ssim")), s), l)
    return out


def group_advantages(frame_reward: torch.Tensor, *, groups: int, n_cand: int, mode: int = 1, eps: float = 1e-6):
    """(reward [groups, n_cand] fp32, advantage [groups * n_cand] fp32) of frame_reward [groups * n_cand, T] fp32: each candidate's mean over
    its T frames, and it against its group's mean (mode 0) or mean and standard deviation (mode 1) (mage_group_advantages)."""
    l, s = _dev(frame_reward)
    assert frame_reward.dtype == torch.float32 and frame_reward.is_contiguous() and groups > 0 and n_cand > 0
    assert frame_reward.numel() > 0 and frame_reward.numel() % (groups * n_cand) == 0
    reward = torch.empty(groups, n_cand, device=frame_reward.device, dtype=torch.float32)
    advantage = torch.empty(groups * n_cand, device=frame_reward.device, dtype=torch.float32)
    _lib.check(l.mage_group_advantages(frame_reward.data_ptr(), groups, n_cand, frame_reward.numel() // (groups * n_cand), int(mode), float(eps),
                                       reward.data_ptr(), advantage.data_ptr(), s), l)
    return reward, advantage


def frame_advantages(frame_reward: torch.Tensor, *, groups: int, n_cand: int, gamma: float = 1.0, mode: int = 1, eps: float = 1e-6,
                     slots: Optional[int] = None, slot_off: int = 0):
    """(returns [groups * n_cand, T] fp32, advantage [groups * n_cand, slots] fp32) of frame_reward [groups * n_cand, T] fp32: each frame's
    discounted reward-to-go over T, and it against the same frame of its group's candidates (mode 0: mean; mode 1: mean and standard
    deviation), frame t in slot slot_off + t and +0 elsewhere; slots None: slot_off + T (mage_frame_advantages)."""
    l, s = _dev(frame_reward)
    assert frame_reward.dtype == torch.float32 and frame_reward.is_contiguous() and groups > 0 and n_cand > 0
    assert frame_reward.numel() > 0 and frame_reward.numel() % (groups * n_cand) == 0
    T = frame_reward.numel() // (groups * n_cand)
    slots = int(slot_off) + T if slots is None else int(slots)
    returns = torch.empty(groups * n_cand, T, device=frame_reward.device, dtype=torch.float32)
    advantage = torch.empty(groups * n_cand, slots, device=frame_reward.device, dtype=torch.float32)
    _lib.check(l.mage_frame_advantages(frame_reward.data_ptr(), groups, n_cand, T, float(gamma), int(mode), float(eps), slots, int(slot_off),
                                       returns.data_ptr(), advantage.data_ptr(), s), l)
    return returns, advantage


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and target.dtype == torch.int64
    K = logits.shape[-1]
    rows = logits.numel() // K
    row_loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    _lib.check(l.mage_cross_entropy(logits.data_ptr(), target.contiguous().data_ptr(), rows, K, row_loss.data_ptr(),
                                    loss.data_ptr(), s), l)
    return loss[0]


def conv_in(x, weight_t, bias, scale, shift, y, *, cin, H, W, cout, kh, kw, stride, pad, act=ACT_NONE, split_kind: int = 0, s2d: bool = False):
    """split_kind: y is a split-precision tensor; s2d: offset space-to-depth rows [N, OH/2+1, OW/2+1, 4*cout] (mage_hip.h)."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    _lib.check(l.mage_conv_in(x.data_ptr(), weight_t.data_ptr(), _p(bias), _p(scale), _p(shift), y.data_ptr(), split_kind or code(y),
                              x.shape[0], cin, H, W, cout, kh, kw, stride, pad, act, int(s2d), s), l)
    return y


def split_rows(x: torch.Tensor, y: torch.Tensor, kind: int, *, relu: bool = False, group: Optional[int] = None,
               group_stride: Optional[int] = None, off: int = 0, inner: int = 0, inner_stride: int = 0, relu_writeback: bool = False):
    """fp32 rows x [rows, C] -> split rows of y under mage_embedding's row map (+ ReLU; relu_writeback: x itself becomes relu(x))."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and y.dtype == split_dtype(kind)
    rows, C_ = x.shape
    group = rows if group is None else group
    group_stride = group if group_stride is None else group_stride
    _lib.check(l.mage_split_rows(x.data_ptr(), x.stride(0), y.data_ptr(), rows, C_, kind, int(relu), group, group_stride, off, inner, inner_stride,
                                 x.data_ptr() if relu_writeback else None, s), l)
    return y


def conv_out(x, weight_t, bias, y, *, N, IH, IW, cin, cout, transposed: bool):
    l, s = _dev(x)
    _lib.check(l.mage_conv_out(x.data_ptr(), code(x), weight_t.data_ptr(), _p(bias), y.data_ptr(), N, IH, IW, cin, cout,
                               int(transposed), s), l)
    return y



def convt_fold_tanh(taps, bias, y, *, N, IH, IW, cout):
    """ConvTranspose2d(., cout, 4, 2, 1) + tanh from per-input-pixel tap products [N*IH*IW, 16*cout] (see mage_hip.h)."""
    l, s = _dev(taps)
    assert taps.dtype == torch.float32 and taps.is_contiguous() and taps.numel() == N * IH * IW * 16 * cout
    _lib.check(l.mage_convt_fold_tanh(taps.data_ptr(), _p(bias), y.data_ptr(), N, IH, IW, cout, s), l)
    return y

def maxpool2(x, y, *, N, H, W, Cc, relu=False):
    l, s = _dev(x)
    _lib.check(l.mage_maxpool2(x.data_ptr(), y.data_ptr(), code(x), N, H, W, Cc, int(relu), s), l)
    return y


def upsample2(x, y, *, N, H, W, Cc):
    l, s = _dev(x)
    _lib.check(l.mage_upsample2(x.data_ptr(), y.data_ptr(), code(x), N, H, W, Cc, s), l)
    return y


def relu(x, y):
    l, s = _dev(x)
    _lib.check(l.mage_relu(x.data_ptr(), y.data_ptr(), code(x), x.numel(), s), l)
    return y


def cast(x, y):
    l, s = _dev(x)
    _lib.check(l.mage_cast(x.data_ptr(), code(x), y.data_ptr(), code(y), x.numel(), s), l)
    return y


def adain(x, gamma, beta, out, *, B, P, Cc, eps=1e-5):
    l, s = _dev(x)
    _lib.check(l.mage_adain(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B, P, Cc, float(eps), s), l)
    return out


def add_scaled_rowvec(x, svec, vec, *, B, P, Cc):
    l, s = _dev(x)
    _lib.check(l.mage_add_scaled_rowvec(x.data_ptr(), svec.data_ptr(), vec.data_ptr(), B, P, Cc, s), l)
    return x


def row_affine(x, rs=None, table=None, *, div: int = 1, mod: int = 1):
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    Cc = x.shape[-1]
    _lib.check(l.mage_row_affine(x.data_ptr(), _p(rs), _p(table), x.numel() // Cc, Cc, div, mod, s), l)
    return x


def caption_mask(ids: torch.Tensor, padding_idx: int):
    """(kv_len int32 [B], keep fp32 [B*S]) of int64 captions [B, S] (mage_caption_mask)."""
    l, s = _dev(ids)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2
    B, S = ids.shape
    kv_len = torch.empty(B, device=ids.device, dtype=torch.int32)
    keep = torch.empty(B * S, device=ids.device, dtype=torch.float32)
    _lib.check(l.mage_caption_mask(ids.data_ptr(), B, S, int(padding_idx), kv_len.data_ptr(), keep.data_ptr(), s), l)
    return kv_len, keep


def assemble_video(first: torch.Tensor, video: torch.Tensor) -> torch.Tensor:
    """[B, L, C, H, W] = frame 0 of `first` ([B, >=1, C, H, W], any batch stride) followed by `video` [B, L-1, C, H, W] (mage_model.py:691),
    as two strided block copies on the stream (mage_copy2d)."""
    l, s = _dev(video)
    B, Lm1 = video.shape[0], video.shape[1]
    frame = video[0, 0].numel()
    assert first.dtype == video.dtype and video.is_contiguous() and first[0, 0].is_contiguous() and first[0, 0].numel() == frame
    out = torch.empty(B, Lm1 + 1, *video.shape[2:], device=video.device, dtype=video.dtype)
    es = video.element_size()
    pitch = (Lm1 + 1) * frame * es
    _lib.check(l.mage_copy2d(out.data_ptr(), pitch, first.data_ptr(), max(first.stride(0), frame) * es, frame * es, B, s), l)
    _lib.check(l.mage_copy2d(out.data_ptr() + frame * es, pitch, video.data_ptr(), Lm1 * frame * es, Lm1 * frame * es, B, s), l)
    return out


def groupnorm_silu(x, gamma, beta, y, *, n_samples, rows_per_sample, sample_stride_rows, row_off, groups, eps=1e-5):
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    Cc = x.shape[-1]
    stats = torch.empty(n_samples, groups, 2, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_groupnorm_silu(x.data_ptr(), sample_stride_rows, row_off, n_samples, rows_per_sample, Cc, groups,
                                     gamma.data_ptr(), beta.data_ptr(), float(eps), stats.data_ptr(), y.data_ptr(), code(y), s), l)
    return y


def groupnorm_act(x, gamma, beta, y, *, n_samples, rows_per_sample, sample_stride_rows, row_off, groups, eps=1e-5, act=0,
                  residual=None, y_sample_stride_rows=None, y_row_off=0, stats=None):
    """y rows (b*y_sample_stride_rows + y_row_off + r) = act(GroupNorm(x rows (b*sample_stride_rows + row_off + r)) + residual);
    act 0 none / 1 ReLU / 2 SiLU (see mage_hip.h)."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous()
    assert residual is None or (residual.dtype == torch.float32 and residual.is_contiguous())
    Cc = x.shape[-1]
    if stats is None:                                   # (mean, rstd) per (sample, group): kept by the training path for the backward
        stats = torch.empty(n_samples, groups, 2, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_groupnorm_act(x.data_ptr(), sample_stride_rows, row_off, n_samples, rows_per_sample, Cc, groups,
                                    gamma.data_ptr(), beta.data_ptr(), float(eps), stats.data_ptr(), _p(residual), act, y.data_ptr(),
                                    code(y), rows_per_sample if y_sample_stride_rows is None else y_sample_stride_rows, y_row_off, s), l)
    return y


def reparam_kl(mu, logvar, eps, out, kl_sum):
    """out = eps * exp(0.5 logvar) + mu; kl_sum[b] = sum(1 + logvar - mu^2 - exp(logvar)) over sample b.  All [B, n] fp32."""
    l, s = _dev(mu)
    B = mu.shape[0]
    n = mu.numel() // B
    for t_ in (mu, logvar, eps, out):
        assert t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == B * n
    _lib.check(l.mage_reparam_kl(mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), out.data_ptr(), kl_sum.data_ptr(), B, n, s), l)
    return out


def groupnorm_bwd(x, gamma, beta, stats, dy, dx, *, n_samples, rows_per_sample, sample_stride_rows, row_off, groups, act=0, residual=None,
                  dy_sample_stride_rows=None, dy_row_off=0, want_dres=False):
    """Backward of groupnorm_act (same row maps): writes dx (x's row map; other rows untouched), returns (dgamma [C], dbeta [C], dres|None)."""
    l, s = _dev(x)
    Cc = x.shape[-1]
    for t_ in (x, dy, dx, stats):
        assert t_.dtype == torch.float32 and t_.is_contiguous()
    dev = x.device
    red = torch.empty(n_samples, groups, 2, device=dev, dtype=torch.float32)
    dgp = torch.empty(n_samples, Cc, device=dev, dtype=torch.float32)
    dbp = torch.empty(n_samples, Cc, device=dev, dtype=torch.float32)
    dres = torch.empty(n_samples * rows_per_sample, Cc, device=dev, dtype=torch.float32) if want_dres else None
    _lib.check(l.mage_groupnorm_bwd(x.data_ptr(), sample_stride_rows, row_off, n_samples, rows_per_sample, Cc, groups, stats.data_ptr(),
                                    gamma.data_ptr(), beta.data_ptr(), _p(residual), act, dy.data_ptr(),
                                    rows_per_sample if dy_sample_stride_rows is None else dy_sample_stride_rows, dy_row_off,
                                    red.data_ptr(), dx.data_ptr(), _p(dres), dgp.data_ptr(), dbp.data_ptr(), s), l)
    if n_samples == 1:
        return dgp[0], dbp[0], dres
    dg = sum_partials(dgp, torch.empty(Cc, device=dev, dtype=torch.float32), stride=Cc, n_part=n_samples, n=Cc)
    db = sum_partials(dbp, torch.empty(Cc, device=dev, dtype=torch.float32), stride=Cc, n_part=n_samples, n=Cc)
    return dg, db, dres


def adain_bwd(x, gamma_map, dout, *, B, P, Cc, eps=1e-5):
    """Backward of adain: (dx, dgamma_map); dbeta_map is dout itself."""
    l, s = _dev(x)
    dx, dg = torch.empty_like(x), torch.empty_like(x)
    _lib.check(l.mage_adain_bwd(x.data_ptr(), gamma_map.data_ptr(), dout.data_ptr(), dx.data_ptr(), dg.data_ptr(), B, P, Cc, float(eps), s), l)
    return dx, dg


def reparam_kl_bwd(mu, logvar, eps, dz, coef):
    """(dmu, dlogvar) of z = eps exp(logvar/2) + mu and the KL term; coef = 1-element fp32 device tensor dL/dkl / B."""
    l, s = _dev(mu)
    dmu, dlv = torch.empty_like(mu), torch.empty_like(mu)
    _lib.check(l.mage_reparam_kl_bwd(mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), dz.data_ptr(), coef.data_ptr(), dmu.data_ptr(),
                                     dlv.data_ptr(), mu.numel(), s), l)
    return dmu, dlv


def transpose_colsum(x, y, *, M: int, Mp: int, C: int, ldx: int, ldy: int, out_w: Optional[int] = None, img_stride: Optional[int] = None,
                     a_off: int = 0):
    """y[c, m] = x[arow(m), c] (bf16, zero for M <= m < Mp) and the column sums of the gathered rows in the same pass: returns
    db [C] fp32 (mage_transpose_colsum + mage_sum_partials)."""
    l, s = _dev(x)
    assert x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
    out_w = M if out_w is None else out_w
    n_part = ((Mp + 63) // 64 + 15) // 16
    part = torch.empty(n_part, C, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_transpose_colsum(x.data_ptr(), ldx, y.data_ptr(), ldy, M, Mp, C, out_w, out_w if img_stride is None else img_stride,
                                       a_off, part.data_ptr(), n_part, s), l)
    if n_part == 1:
        return part[0]
    return sum_partials(part, torch.empty(C, device=x.device, dtype=torch.float32), stride=C, n_part=n_part, n=C)


def maxpool2_bwd(x, dy, *, N, H, W, Cc):
    """dx [N*H*W, C] of y = maxpool2(x): dy [N*(H/2)*(W/2), C] routed to the first maximum of each window."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x)
    _lib.check(l.mage_maxpool2_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), N, H, W, Cc, s), l)
    return dx


def upsample2_bwd(dy, *, N, H, W, Cc):
    """dx [N*H*W, C] of y = upsample2(x) (nearest): the sum of each 2x2 block of dy [N*2H*2W, C]."""
    l, s = _dev(dy)
    assert dy.dtype == torch.float32 and dy.is_contiguous()
    dx = torch.empty(N * H * W, Cc, device=dy.device, dtype=torch.float32)
    _lib.check(l.mage_upsample2_bwd(dy.data_ptr(), dx.data_ptr(), N, H, W, Cc, s), l)
    return dx


def mse_bwd(a, b, gout, *, rows, cols, lda, ldb):
    """d mse / da * gout as [rows, lda] fp32 (zeros in the padding columns)."""
    l, s = _dev(a)
    da = torch.empty(rows, lda, device=a.device, dtype=torch.float32)
    _lib.check(l.mage_mse_bwd(a.data_ptr(), lda, b.data_ptr(), ldb, rows, cols, gout.data_ptr(), da.data_ptr(), lda, s), l)
    return da


def mse(a, b, *, rows, cols, lda, ldb):
    """mean((a[:, :cols] - b[:, :cols])^2) over `rows` rows with row strides lda / ldb (fp32) -> 0-dim fp32 tensor."""
    l, s = _dev(a)
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    ws = torch.empty(256, device=a.device, dtype=torch.float64)
    _lib.check(l.mage_mse(a.data_ptr(), lda, b.data_ptr(), ldb, rows, cols, ws.data_ptr(), out.data_ptr(), s), l)
    return out[0]


# ----------------------------------------------------------------------------------------------------------------- training path
def transpose(x, y, *, M: int, Mp: int, C: int, ldx: int, ldy: int, y_row0: int = 0, out_h: int = 1, out_w: Optional[int] = None,
              in_h: Optional[int] = None, in_w: Optional[int] = None, img_stride: Optional[int] = None, a_off: int = 0, dy: int = 0,
              dx: int = 0, stride: int = 1):
    """y[(c + y_row0), m] = x[arow(m), c] (zero for M <= m < Mp and outside the plane); see mage_transpose in mage_hip.h."""
    l, s = _dev(x)
    assert x.dtype == y.dtype
    out_w = M if out_w is None else out_w
    in_h = out_h if in_h is None else in_h
    in_w = out_w if in_w is None else in_w
    img_stride = in_h * in_w if img_stride is None else img_stride
    _lib.check(l.mage_transpose(x.data_ptr(), code(x), ldx, y.data_ptr(), ldy, y_row0, M, Mp, C, out_h, out_w, in_h, in_w, img_stride,
                                a_off, dy, dx, stride, s), l)
    return y


def gemm_tn(dy, x, *, T: int, N: int, K: int, ld_dy: int, ld_x: int, want_bias: bool = True):
    """dW [N, K] = dy[:T, :N]^T x[:T, :K] (fp32) and db [N] = column sums of dy, from ROW-MAJOR bf16 dy / x (no transposed copies):
    mage_gemm_tn over token slices + mage_sum_partials (+ mage_colsum)."""
    l, s = _dev(dy)
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and N % 256 == 0 and K % 256 == 0
    n_cu = torch.cuda.get_device_properties(dy.device).multi_processor_count & ~7
    tiles = (N // 256) * (K // 256)
    # ONE workgroup per CU, never a partial second round (measured at cfg2, TFLOP/s for in_proj / out_proj / c_fc / c_proj: one round
    # 596 / 631 / 734 / 719, two 574 / 535 / 689 / 675, four 502 / 418 / 648 / 629: long K loops amortise the ring start-up and the 256 KB
    # of fp32 partials each workgroup writes); >= 512 tokens per slice
    S = int(max(1, min(256, n_cu // tiles, (T + 511) // 512)))
    tps = ((T + S - 1) // S + 63) // 64 * 64
    S = (T + tps - 1) // tps
    part = torch.empty(S, N, K, device=dy.device, dtype=torch.float32)
    dbp = torch.empty(S, N, device=dy.device, dtype=torch.float32) if want_bias else None
    ev = PROFILE.begin() if PROFILE.wants("gemm_tn") else None
    _lib.check(l.mage_gemm_tn(dy.data_ptr(), ld_dy, x.data_ptr(), ld_x, T, N, K, S, tps, part.data_ptr(), _p(dbp), s), l)
    if ev is not None:
        PROFILE.end("gemm_tn", ev, 2.0 * T * N * K)
    dW = part[0] if S == 1 else sum_partials(part, torch.empty(N, K, device=dy.device, dtype=torch.float32), stride=N * K, n_part=S, n=N * K)
    db = None
    if want_bias:           # the kernel's per-slice column sums of dy (from the fragments it holds anyway), added in a fixed order
        db = dbp[0] if S == 1 else sum_partials(dbp, torch.empty(N, device=dy.device, dtype=torch.float32), stride=N, n_part=S, n=N)
    return dW, db


def colsum(x: torch.Tensor, *, T: int, C_: int, ld: int) -> torch.Tensor:
    """Column sums (fp32 [C]) of bf16 rows x[:T, :C] (mage_colsum + mage_sum_partials): a bias gradient on its own."""
    l, s = _dev(x)
    n_part = int(max(1, min(1024, T // 128)))
    cp = torch.empty(n_part, C_, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_colsum(x.data_ptr(), ld, T, C_, cp.data_ptr(), n_part, s), l)
    return cp[0] if n_part == 1 else sum_partials(cp, torch.empty(C_, device=x.device, dtype=torch.float32), stride=C_, n_part=n_part, n=C_)


def row_sum(x, out, *, ld: int, n: int, rows: int):
    l, s = _dev(x)
    n_chunk = int(max(1, min(64, n // 2048, 16384 // max(rows, 1))))      # enough waves to fill the chip, >= 2048 columns each
    if n_chunk == 1:
        _lib.check(l.mage_row_sum(x.data_ptr(), code(x), ld, n, rows, out.data_ptr(), 1, s), l)
        return out
    part = torch.empty(n_chunk, rows, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_row_sum(x.data_ptr(), code(x), ld, n, rows, part.data_ptr(), n_chunk, s), l)
    return sum_partials(part, out, stride=rows, n_part=n_chunk, n=rows)


def sum_partials(part, out, *, stride: int, n_part: int, n: int, accumulate: bool = False):
    l, s = _dev(part)
    assert part.dtype == torch.float32 and out.dtype == torch.float32
    _lib.check(l.mage_sum_partials(part.data_ptr(), stride, n_part, n, out.data_ptr(), int(accumulate), s), l)
    return out


def layernorm_bwd(x, gamma, dy, dx, *, eps: float, accumulate: bool, dx_bf16=None, p: float = 0.0, seed: int = 0):
    """dx (+)= dLN/dx; returns (dgamma, dbeta) fp32 [C].  dx_bf16: the updated dx once more as bf16 through dropout(., p, seed)'s mask."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and dx.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous()
    assert dx_bf16 is None or (dx_bf16.dtype == torch.bfloat16 and dx_bf16.is_contiguous() and dx_bf16.numel() == dx.numel())
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    n_part = int(min(1024, (rows + 3) // 4))
    part = torch.empty(n_part, 2, Cc, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_layernorm_bwd(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), code(dy), dx.data_ptr(), part.data_ptr(), n_part, rows,
                                    Cc, float(eps), int(accumulate), dx_bf16.data_ptr() if dx_bf16 is not None else None, float(p),
                                    int(seed) & (2 ** 64 - 1), s), l)
    gb = torch.empty(2, Cc, device=x.device, dtype=torch.float32)
    sum_partials(part, gb, stride=2 * Cc, n_part=n_part, n=2 * Cc)
    return gb[0], gb[1]


def act(x, y, kind: int):
    l, s = _dev(x)
    assert x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous()
    _lib.check(l.mage_act(x.data_ptr(), y.data_ptr(), code(x), x.numel(), kind, s), l)
    return y


def act_bwd(x, dy, dx, kind: int):
    l, s = _dev(x)
    assert x.dtype == dy.dtype == dx.dtype and x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous()
    _lib.check(l.mage_act_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), code(x), x.numel(), kind, s), l)
    return dx


def cross_entropy_bwd(logits, target, grad_out, dlogits):
    l, s = _dev(logits)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and target.dtype == torch.int64 and grad_out.dtype == torch.float32
    K = logits.shape[-1]
    _lib.check(l.mage_cross_entropy_bwd(logits.data_ptr(), target.contiguous().data_ptr(), logits.numel() // K, K, grad_out.data_ptr(),
                                        dlogits.data_ptr(), code(dlogits), s), l)
    return dlogits


def embedding_bwd(ids, dout, dtable, *, padding_idx: int = -1, group: Optional[int] = None, group_stride: Optional[int] = None, off: int = 0):
    l, s = _dev(dout)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and dtable.dtype == torch.float32 and dtable.is_contiguous()
    n = ids.numel()
    group = n if group is None else group
    group_stride = group if group_stride is None else group_stride
    scratch = None
    if dtable.shape[0] <= 512 and dtable.shape[1] % 64 == 0:
        # small table (the visual token table, the codebook, the caption vocabulary): per-chunk partial tables summed in chunk order, rows added
        # in ascending order inside a chunk -- no atomics between waves, a fixed-order fp32 sum: bit-identical gradients from run to run
        n_chunk = min(64, (n + 4095) // 4096)
        scratch = torch.empty(n_chunk * dtable.numel(), device=dtable.device, dtype=torch.float32)
    _lib.check(l.mage_embedding_bwd(ids.data_ptr(), dout.data_ptr(), code(dout), dtable.data_ptr(), n, dtable.shape[1], dtable.shape[0],
                                    padding_idx, group, group_stride, off, _p(scratch), 0 if scratch is None else scratch.numel(), s), l)
    return dtable


def code_stats_chunks(rows: int) -> int:
    """The number of row chunks mage_code_stats cuts `rows` into (include/mage_hip_ext.h states the formula): its scratch is sized from it."""
    return min(64, (rows + 4095) // 4096)


def code_stats(ids: torch.Tensor, z: Optional[torch.Tensor] = None, *, K: int, D: Optional[int] = None, counts: Optional[torch.Tensor] = None,
               sums: Optional[torch.Tensor] = None):
    """mage_code_stats: (counts int64 [K], sums fp32 [K, D] or None) of ids (int64, any shape) and the encoder rows z [rows, >= D] fp32 (row
    stride z.stride(0)).  counts[k] = the number of rows with id k, sums[k] = the fixed-order fp32 sum of those rows of z.  z None: the
    counts-only form.  An id outside [0, K) is counted nowhere and reported by check_device_errors."""
    l, s = _dev(ids)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() > 0
    rows, dev = ids.numel(), ids.device
    if counts is None:
        counts = torch.empty(K, device=dev, dtype=torch.int64)
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == K and counts.device == dev
    ldz = 0
    if z is not None:
        assert z.dtype == torch.float32 and z.dim() == 2 and z.stride(1) == 1 and z.shape[0] == rows and z.device == dev
        D = z.shape[1] if D is None else D
        ldz = z.stride(0)
        assert 0 < D <= z.shape[1]
        if sums is None:
            sums = torch.empty(K, D, device=dev, dtype=torch.float32)
        assert sums.dtype == torch.float32 and sums.is_contiguous() and tuple(sums.shape) == (K, D) and sums.device == dev
    else:
        assert sums is None
        D = 0
    scratch = torch.empty(code_stats_chunks(rows) * K * (D + 1), device=dev, dtype=torch.float32)
    _lib.check(l.mage_code_stats(ids.data_ptr(), _p(z), rows, D, ldz, K, counts.data_ptr(), _p(sums), scratch.data_ptr(), scratch.numel() * 4, s), l)
    return counts, sums


def codebook_ema(codebook: torch.Tensor, cluster_size: torch.Tensor, embed_sum: torch.Tensor, counts: torch.Tensor, sums: torch.Tensor,
                 z: Optional[torch.Tensor] = None, *, decay: float = 0.99, eps: float = 1e-5, restart_below: float = 0.0,
                 restart_size: Optional[float] = None, seed: int = 0, step: int = 0, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mage_codebook_ema: one launch updates codebook [K, D], cluster_size [K] and embed_sum [K, D] (fp32, in place) from code_stats' counts
    and sums; with restart_below > 0 a code whose new size is below it takes a row of z (fp32 [rows, >= D], row stride z.stride(0)) chosen by
    (seed, step).  Returns stats, fp64 [4] on the device: perplexity, codes used, codes restarted, rows counted.  The writes go behind
    autograd's version counters: the caller invalidates what it derived from the codebook."""
    l, s = _dev(codebook)
    K, D = codebook.shape
    dev = codebook.device
    for t_, shape in ((codebook, (K, D)), (embed_sum, (K, D)), (sums, (K, D)), (cluster_size, (K,))):
        assert t_.dtype == torch.float32 and t_.is_contiguous() and tuple(t_.shape) == shape and t_.device == dev
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == K and counts.device == dev
    rows = ldz = 0
    if z is not None:
        assert z.dtype == torch.float32 and z.dim() == 2 and z.stride(1) == 1 and z.shape[1] >= D and z.device == dev
        rows, ldz = z.shape[0], z.stride(0)
    if stats is None:
        stats = torch.empty(4, device=dev, dtype=torch.float64)
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 4 and stats.device == dev
    restart_size = (restart_below if restart_below > 0 else 1.0) if restart_size is None else restart_size      # unused without a restart
    _lib.check(l.mage_codebook_ema(codebook.data_ptr(), cluster_size.data_ptr(), embed_sum.data_ptr(), counts.data_ptr(), sums.data_ptr(), _p(z),
                                   rows, ldz, K, D, float(decay), float(eps), float(restart_below), float(restart_size),
                                   int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), stats.data_ptr(), s), l)
    return stats


def group_rowsum(x, out, *, rows: int, C: int, div: int, mod: int, row_scale=None, row_scale_div: int = 1):
    l, s = _dev(x)
    assert out.dtype == torch.float32
    per_group = rows // max(mod, 1)
    n_chunk = int(max(1, min(256, per_group // 64, 2048 // max(mod, 1))))
    if n_chunk == 1:
        _lib.check(l.mage_group_rowsum(x.data_ptr(), code(x), rows, C, div, mod, _p(row_scale), row_scale_div, out.data_ptr(), 1, s), l)
        return out
    part = torch.empty(n_chunk, mod, C, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_group_rowsum(x.data_ptr(), code(x), rows, C, div, mod, _p(row_scale), row_scale_div, part.data_ptr(), n_chunk, s), l)
    return sum_partials(part, out, stride=mod * C, n_part=n_chunk, n=mod * C)


def attention_bwd(q, k, v, dout, dq, dk, dv, *, ldq, ldk, ldv, ldo, ld_dq, ld_dk, ld_dv, n_seq, inner, nq, nk, n_head, q_outer_stride,
                  q_axis_stride, kv_outer_stride, kv_axis_stride, causal=False, kv_len=None, kv_len_div=1, scale=None,
                  drop_p: float = 0.0, drop_seed: int = 0):
    l, s = _dev(q)
    d = AttnDesc()
    d.dtype = code(q)
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr()
    d.ldq, d.ldk, d.ldv, d.ldo = ldq, ldk, ldv, ldo
    d.n_seq, d.inner, d.nq, d.nk, d.n_head = n_seq, inner, nq, nk, n_head
    d.q_outer_stride, d.q_axis_stride = q_outer_stride, q_axis_stride
    d.kv_outer_stride, d.kv_axis_stride = kv_outer_stride, kv_axis_stride
    d.causal = int(causal)
    d.kv_len, d.kv_len_div = _p(kv_len), kv_len_div
    d.scale = float(32 ** -0.5 if scale is None else scale)
    d.drop_p, d.drop_seed = float(drop_p), int(drop_seed) & (2 ** 64 - 1)
    _lib.check(l.mage_attention_bwd(C.byref(d), dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ld_dq, ld_dk, ld_dv, s), l)


def dropout(x, y, p: float, seed: int, accumulate: bool = False):
    l, s = _dev(x)
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    _lib.check(l.mage_dropout(x.data_ptr(), code(x), y.data_ptr(), code(y), x.numel(), float(p), int(seed) & (2 ** 64 - 1), int(accumulate), s), l)
    return y


def dropout_add(x, r, y, p: float, seed: int, y_bf16=None):
    """y = r + dropout(x) (the mask of dropout(x, ., p, seed)); r, y fp32; y_bf16: the same rows once more as bf16."""
    l, s = _dev(x)
    assert x.is_contiguous() and r.is_contiguous() and y.is_contiguous() and r.dtype == y.dtype == torch.float32 and x.numel() == y.numel() == r.numel()
    assert y_bf16 is None or (y_bf16.dtype == torch.bfloat16 and y_bf16.is_contiguous() and y_bf16.numel() == y.numel())
    _lib.check(l.mage_dropout_add(x.data_ptr(), code(x), r.data_ptr(), y.data_ptr(), y_bf16.data_ptr() if y_bf16 is not None else None,
                                  x.numel(), float(p), int(seed) & (2 ** 64 - 1), s), l)
    return y


def dropout_add_layernorm(x, r, y, gamma, beta, yn, eps: float, p: float, seed: int):
    """y = r + dropout(x) (fp32) and yn = LayerNorm(y) in one pass; returns (y, yn)."""
    l, s = _dev(x)
    Cc = r.shape[-1]
    assert x.is_contiguous() and r.is_contiguous() and y.is_contiguous() and yn.is_contiguous() and r.dtype == y.dtype == torch.float32
    assert x.numel() == y.numel() == r.numel() == yn.numel() and gamma.numel() == beta.numel() == Cc
    _lib.check(l.mage_dropout_add_layernorm(x.data_ptr(), code(x), r.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), yn.data_ptr(),
                                            code(yn), r.numel() // Cc, Cc, float(eps), float(p), int(seed) & (2 ** 64 - 1), s), l)
    return y, yn


def adam(p, g, m, v, *, lr: float, beta1: float, beta2: float, eps: float, step: int, grad_scale: float = 1.0):
    l, s = _dev(p)
    for t_ in (p, g, m, v):
        assert t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == p.numel()
    _lib.check(l.mage_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(beta1), float(beta2),
                           float(eps), int(step), float(grad_scale), s), l)
    return p


def sumsq(g: torch.Tensor) -> torch.Tensor:
    """fp64 [1]: the sum of the squares of a flat fp32 tensor, exact squares added in a fixed order (mage_sumsq)."""
    l, s = _dev(g)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.numel() > 0
    out = torch.empty(1, device=g.device, dtype=torch.float64)
    _lib.check(l.mage_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), s), l)
    return out


def adam_clipped(p, g, m, v, *, lr: float, beta1: float, beta2: float, eps: float, step: int, grad_scale: float = 1.0, sumsq: torch.Tensor,
                 max_norm: float, norm_out: Optional[torch.Tensor] = None):
    """adam with the gradient scaled by clip_grad_norm_'s rule from the device value sumsq (fp64 [1]: the whole gradient's sum of squares);
    norm_out (fp32 [1], optional) receives the norm of the averaged gradient before the clip (mage_adam_clipped)."""
    l, s = _dev(p)
    for t_ in (p, g, m, v):
        assert t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == p.numel()
    assert sumsq.dtype == torch.float64 and sumsq.numel() == 1 and sumsq.device == p.device
    assert norm_out is None or (norm_out.dtype == torch.float32 and norm_out.numel() == 1 and norm_out.device == p.device)
    _lib.check(l.mage_adam_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(beta1), float(beta2),
                                   float(eps), int(step), float(grad_scale), sumsq.data_ptr(), float(max_norm), _p(norm_out), s), l)
    return p


def adam_guarded(p, g, m, v, *, lr: float, beta1: float, beta2: float, eps: float, step: int, grad_scale: float = 1.0,
                 ema: Optional[torch.Tensor] = None, ema_decay: float = 0.0, n_decay: int = 0, decay_mul: float = 1.0,
                 sumsq: Optional[torch.Tensor] = None, max_norm: float = 0.0, skip_nonfinite: bool = False,
                 norm_out: Optional[torch.Tensor] = None, skipped: Optional[torch.Tensor] = None):
    """adam / adam_clipped in one launch that can also skip a step whose gradient is not finite (skip_nonfinite, decided on the device from
    sumsq; skipped, int64 [1], counts the skips), decay the first n_decay elements by decay_mul before the update (AdamW's order) and keep an
    exponential moving average of the updated parameters in ema (fp32, p's size).  max_norm 0: no clip (mage_adam_guarded)."""
    l, s = _dev(p)
    for t_ in (p, g, m, v) + (() if ema is None else (ema,)):
        assert t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == p.numel() and t_.device == p.device
    assert sumsq is None or (sumsq.dtype == torch.float64 and sumsq.numel() == 1 and sumsq.device == p.device)
    assert norm_out is None or (norm_out.dtype == torch.float32 and norm_out.numel() == 1 and norm_out.device == p.device)
    assert skipped is None or (skipped.dtype == torch.int64 and skipped.numel() == 1 and skipped.device == p.device)
    _lib.check(l.mage_adam_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(ema), p.numel(), int(n_decay), float(lr),
                                   float(beta1), float(beta2), float(eps), int(step), float(grad_scale), float(decay_mul), float(ema_decay),
                                   _p(sumsq), float(max_norm), int(bool(skip_nonfinite)), _p(norm_out), _p(skipped), s), l)
    return p


def _bn_reduce(mode, x, dy, mask, mean, rstd, nout):
    l, s = _dev(x)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    n_part = int(min(1024, max(1, rows // 64)))
    part = torch.empty(n_part, nout, Cc, device=x.device, dtype=torch.float32)
    _lib.check(l.mage_bn_colreduce(mode, x.data_ptr(), _p(dy), _p(mask), _p(mean), _p(rstd), rows, Cc, part.data_ptr(), n_part, s), l)
    out = torch.empty(nout, Cc, device=x.device, dtype=torch.float32)
    return sum_partials(part, out, stride=nout * Cc, n_part=n_part, n=nout * Cc), rows


def bn_train_stats(x, eps: float):
    """Batch statistics of channels-last rows x [rows, C] fp32 (two passes): (mean [C], biased var [C], rstd [C])."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    s, rows = _bn_reduce(0, x, None, None, None, None, 1)
    mean = (s[0] / rows).contiguous()
    q, _ = _bn_reduce(1, x, None, None, mean, None, 1)
    var = (q[0] / rows).contiguous()
    return mean, var, torch.rsqrt(var + eps).contiguous()        # [C]-sized vector bookkeeping


def bn_apply(x, mean, rstd, gamma, beta, y, relu: bool, residual=None):
    l, s = _dev(x)
    Cc = x.shape[-1]
    _lib.check(l.mage_bn_apply(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _p(residual), y.data_ptr(),
                               code(y), x.numel() // Cc, Cc, int(relu), s), l)
    return y


def bn_backward(x, dy, mean, rstd, gamma, dx, mask=None):
    """dx (into `dx`), dgamma, dbeta of training-mode BatchNorm; mask = the post-ReLU output when a ReLU follows the norm."""
    l, s = _dev(x)
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous()
    Cc = x.shape[-1]
    sums, rows = _bn_reduce(2, x, dy, mask, mean, rstd, 2)
    _lib.check(l.mage_bn_bwd_apply(x.data_ptr(), dy.data_ptr(), _p(mask), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), sums.data_ptr(),
                                   dx.data_ptr(), rows, Cc, s), l)
    return sums[1], sums[0]                                       # dgamma = sum g xhat, dbeta = sum g


def convt_unfold_tanh_bwd(grad_y, y, dtaps, *, N, IH, IW, cout):
    l, s = _dev(grad_y)
    assert grad_y.dtype == torch.float32 and grad_y.is_contiguous() and (y is None or (y.dtype == torch.float32 and y.is_contiguous()))
    _lib.check(l.mage_convt_unfold_tanh_bwd(grad_y.data_ptr(), _p(y), dtaps.data_ptr(), N, IH, IW, cout, s), l)
    return dtaps
