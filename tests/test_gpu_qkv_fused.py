"""GPU: the H / W axial attention and the in_proj GEMM in ONE launch (mage_gemm_attn_fused_qkv, csrc/gemm4.hip QF: per (frame, group of 4
heads) a Q K tile that keeps the softmax numerators in registers, then a half-width V tile that finishes P V) against the pair it replaces --
ops.gemm (QKV, LayerNorm-consuming form) + ops.attention -- BITWISE on the attention output rows `ao`.

  * M = 256 and 512 rows (one and two 16 x 16 frames), C = 256 (2 groups; a K loop of 4 slabs: the peeled first / last pairs only) and 512,
    both axes, bf16 and f16;
  * 600 frames at C = 256: 4.7 entries per workgroup -- the panel replay and the slab hand-over across Q K -> V -> next entry -> last entry;
  * a non-zero row offset on the input and regrouped output rows (out_w, y_img_stride, y_off);
  * ao is pre-filled with a sentinel and carries guard rows: every row of the window is written, nothing outside it is;
  * the decoder itself: fused blocks == the QKV GEMM + attention pair bitwise, the off switch (config qk_fuse), the size rule
    (qkv_fuse_tiles entries per CU) and a geometry outside the fusion (hh = 8) launch no fused kernel.
"""
from fractions import Fraction

import pytest
import torch

from mage_amd import config, ops
from mage_amd.modules.mage_model import FlatAxialDecoder
from tests.helpers import count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                  # sentinel rows in front of and behind every output
FILL = 777.0


def _geo(axis, frames, heads):
    """ops.attention's row map of `frames` 16 x 16 frames along H (1) or W (2): FlatAxialDecoder._axial_geo."""
    if axis == 1:
        return dict(n_seq=frames * 16, inner=16, nq=16, nk=16, q_outer_stride=256, q_axis_stride=16, causal=False, kv_outer_stride=256,
                    kv_axis_stride=16, n_head=heads)
    return dict(n_seq=frames * 16, inner=1, nq=16, nk=16, q_outer_stride=16, q_axis_stride=1, causal=False, kv_outer_stride=16,
                kv_axis_stride=1, n_head=heads)


def _operands(M, C, dt, a_rows):
    g = torch.Generator(device="cpu").manual_seed(1000 * M + C)
    xb = torch.randn(a_rows, C, generator=g).to(DEV).to(dt)
    w = (torch.randn(3 * C, C, generator=g) * C ** -0.5).to(DEV).to(dt)           # gamma * W, rounded: what the MFMA multiplies
    lns = w.float().sum(dim=1).contiguous()
    lnc = (0.1 * torch.randn(3 * C, generator=g)).to(DEV)
    stats = torch.stack([0.05 * torch.randn(M, generator=g), 1.0 + 0.2 * torch.rand(M, generator=g)], 1).contiguous().to(DEV)
    return xb, w, lns, lnc, stats


def _pair(xb, w, lns, lnc, stats, M, C, axis, dt):
    """The replaced pair on plain rows: ao [M, C]."""
    qkv = torch.empty(M, 3 * C, device=DEV, dtype=dt)
    ops.gemm(xb, w, qkv, M=M, N=3 * C, K=C, lda=C, ldy=3 * C, bias=lnc, ln_colsum=lns, ln_stats=stats)
    ao = torch.empty(M, C, device=DEV, dtype=dt)
    ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], ao, ldq=3 * C, ldk=3 * C, ldv=3 * C, ldo=C, **_geo(axis, M // 256, C // 32))
    return ao


def _fused(xb, w, lns, lnc, stats, M, C, axis, dt, *, a_off=0, out_rows=None, **rows):
    """The single launch; returns ao with its guard rows."""
    idx = ops.qkv_pack_rows(C, DEV)
    out_rows = M if out_rows is None else out_rows
    ao = torch.full((out_rows + 2 * GUARD, C), FILL, device=DEV, dtype=dt)
    ops.gemm_attn_fused_qkv(xb, w[idx].contiguous(), ao[GUARD:], axis=axis, M=M, C_=C, K=C, lda=C, ldy=C, bias=lnc[idx].contiguous(),
                            ln_colsum=lns[idx].contiguous(), ln_stats=stats, a_off=a_off, **rows)
    torch.cuda.synchronize()
    return ao


def _bits(x):
    return x.contiguous().view(torch.int16)


def _fill_bits(dt):
    return _bits(torch.full((1,), FILL, dtype=dt))[0].item()


def test_pack_rows_is_a_permutation_in_group_order():
    C = 256
    idx = ops.qkv_pack_rows(C).view(C // 128, 384)
    assert torch.equal(idx.reshape(-1).sort().values, torch.arange(3 * C))
    # head h of group g (head 4g + h of the layer) at rows 64h .. 64h+63 as [q_h | k_h]; within each 32 rows, row j is head dim
    # (j % 16 // 4) * 8 + (j // 16) * 4 + j % 4
    want = [[part * C + (4 * g + h) * 32 + (j % 16 // 4) * 8 + (j // 16) * 4 + j % 4 for h in range(4) for part in (0, 1) for j in range(32)]
            for g in range(C // 128)]
    assert idx[:, :256].tolist() == want
    assert torch.equal(idx[:, 256:].reshape(-1), 2 * C + torch.arange(C))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("axis", [1, 2], ids=["H", "W"])
@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("M", [256, 512])
def test_single_launch_matches_gemm_plus_attention_bitwise(M, C, axis, dt):
    xb, w, lns, lnc, stats = _operands(M, C, dt, M)
    want = _pair(xb, w, lns, lnc, stats, M, C, axis, dt)
    ao = _fused(xb, w, lns, lnc, stats, M, C, axis, dt)
    fill = _fill_bits(dt)
    assert bool((_bits(ao[:GUARD]) == fill).all()) and bool((_bits(ao[GUARD + M:]) == fill).all()), "ao written outside its window"
    got = ao[GUARD:GUARD + M]
    ndiff = int((_bits(got) != _bits(want)).sum())
    print(f"M={M} C={C} axis={axis} {dt}: {ndiff} of {got.numel()} ao elements differ, max |d| {(got.float() - want.float()).abs().max().item():.3e}")
    assert ndiff == 0


def test_several_entries_per_workgroup():
    """600 frames at C = 256: 1200 entries on 256 workgroups -- a workgroup's next entry starts under the V part's row stores, the V part
    replays the panel, and the last entry's hand-over fetches nothing that is read."""
    M, C, dt = 600 * 256, 256, torch.bfloat16
    xb, w, lns, lnc, stats = _operands(M, C, dt, M)
    fill = _fill_bits(dt)
    for axis in (1, 2):
        want = _pair(xb, w, lns, lnc, stats, M, C, axis, dt)
        ao = _fused(xb, w, lns, lnc, stats, M, C, axis, dt)
        assert bool((_bits(ao[:GUARD]) == fill).all()) and bool((_bits(ao[GUARD + M:]) == fill).all()), "ao written outside its window"
        assert torch.equal(_bits(ao[GUARD:GUARD + M]), _bits(want)), f"axis {axis}"


@pytest.mark.parametrize("axis", [1, 2], ids=["H", "W"])
def test_row_offset_and_regrouped_output_rows(axis):
    """Two frames read behind a_off = 256 rows, written to slot 1 of two-slot windows (out_w = 256, y_img_stride = 512, y_off = 256)."""
    M, C, dt = 512, 256, torch.bfloat16
    xb, w, lns, lnc, stats = _operands(M, C, dt, M + 256)
    want = _pair(xb[256:], w, lns, lnc, stats, M, C, axis, dt)
    ao = _fused(xb, w, lns, lnc, stats, M, C, axis, dt, a_off=256, out_rows=1024, out_w=256, y_img_stride=512, y_off=256)
    fill = _fill_bits(dt)
    body = ao[GUARD:GUARD + 1024].view(2, 2, 256, C)
    assert bool((_bits(ao[:GUARD]) == fill).all()) and bool((_bits(ao[GUARD + 1024:]) == fill).all()) and bool((_bits(body[:, 0]) == fill).all()), \
        "ao written outside its window"
    assert torch.equal(_bits(body[:, 1]), _bits(want.view(2, 256, C)))


def _decoder(dt, tiles=0):
    torch.manual_seed(7)
    m = FlatAxialDecoder(64, 256, 64, frames_length=2, layers=3, context_channels=64).to(DEV).eval()
    m.compute_dtype = dt
    if tiles is not None:                       # (the size rule keeps calls this small on the QKV GEMM + attention)
        m.qkv_fuse_tiles = tiles
    return m


def _logits(m, B, hh, ww):
    g = torch.Generator(device="cpu").manual_seed(3)
    motion = torch.randn(B * hh * ww, 64, generator=g).to(DEV).to(m.compute_dtype)
    imgs = torch.randn(B * (m.frames_length - 1) * hh * ww, 64, generator=g).to(DEV).to(m.compute_dtype)
    out = m._run(motion, imgs, B=B, hh=hh, ww=ww)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_decoder_single_launch_blocks_and_the_off_switch(monkeypatch, dt):
    m = _decoder(dt)
    calls = count_lib_calls(monkeypatch)
    on = _logits(m, 4, 16, 16)
    n_on = calls.count("mage_gemm_attn_fused_qkv")
    del calls[:]
    with config.override(qk_fuse=False):
        off = _logits(m, 4, 16, 16)
    n_off = calls.count("mage_gemm_attn_fused_qkv")
    monkeypatch.undo()
    assert n_on == 2 and n_off == 0 and "mage_attention" in calls, (n_on, n_off)      # blocks 1 (H) and 2 (W): one launch each
    assert torch.equal(on, off)


def test_size_rule_counts_entries_per_cu(monkeypatch):
    """M = 2048 rows (8 frames) at C = 256 (2 groups of 4 heads) = 16 entries: fused from qkv_fuse_tiles * n_cu <= 16 on, and the default of
    eight entries per CU keeps a call this small on the QKV GEMM + attention."""
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    m = _decoder(torch.bfloat16, tiles=None)
    assert m.qkv_fuse_tiles == 8
    calls = count_lib_calls(monkeypatch)
    n = []
    for tiles in (None, Fraction(16, n_cu), Fraction(17, n_cu)):      # the default left in place, then exactly at and just above 16 entries
        if tiles is not None:
            m.qkv_fuse_tiles = tiles
        del calls[:]
        _logits(m, 4, 16, 16)
        n.append(calls.count("mage_gemm_attn_fused_qkv"))
    monkeypatch.undo()
    assert n == [0, 2, 0], n


def test_geometry_outside_the_fusion_takes_neither(monkeypatch):
    """hh = 8 (8 x 32 frames: still whole 256-row tiles for the LayerNorm fold, but a tile is no 16 x 16 frame)."""
    m = _decoder(torch.bfloat16)
    calls = count_lib_calls(monkeypatch)
    got = _logits(m, 4, 8, 32)
    n = calls.count("mage_gemm_attn_fused_qkv")
    with config.override(qk_fuse=False):
        want = _logits(m, 4, 8, 32)
    monkeypatch.undo()
    assert n == 0 and "mage_attention" in calls
    assert torch.equal(got, want)
