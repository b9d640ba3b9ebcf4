"""GPU: the temporal blocks' causal attention inside the fused in_proj launch (mage_gemm_attn_fused_qkv, axis 0; csrc/gemm4.hip TX: a tile is 16
adjacent positions x the 16 slots of one clip, attention_mfma_kernel's causal select in the Q K epilogue) against the pair it replaces -- ops.gemm
(QKV, LayerNorm-consuming form) + ops.attention with FlatAxialDecoder._axial_geo(0)'s causal row map -- BITWISE on the attention output rows `ao`.
No tolerance anywhere.

  * the smallest tile counts: one tile (hw = 16, one clip), two tiles of one clip (hw = 32), two clips of one tile; C = 256 (a K loop of 4 slabs:
    the peeled pairs only) and 512; bf16 and f16; ao pre-filled with a sentinel between guard rows: every row of the window written, nothing else;
  * hw = 48 (3 tiles per clip) x 199 clips = 597 tiles, 1194 entries on 256 workgroups: the clip / tile division, the panel replay, the hand-over
    across entries, uneven XCD chunks;
  * causality by itself: other values in the input rows (and statistics rows) of the slots >= s leave the outputs of the slots < s bit for bit;
  * refusals (hw = 24, M no whole number of clips, regrouped output rows): ValueError from MAGE_EINVAL, nothing written;
  * the decoder: a full pass over 16 slots with the temporal launch == the same pass with tqkv_fuse off == with qk_fuse off, the launches counted;
    frames_length = 8 keeps the pair on its temporal block; the incremental loop (the pair) ends on the full pass's last slot.
"""
import pytest
import torch

from mage_amd import config, ops
from mage_amd.modules.mage_model import FlatAxialDecoder
from tests.helpers import count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                  # sentinel rows in front of and behind every output
FILL = 777.0


def _geo(clips, hw, heads):
    """ops.attention's row map of `clips` clips of 16 slots of hw rows along T: FlatAxialDecoder._axial_geo(0, ...) at P = 16, p0 = 0."""
    return dict(n_seq=clips * hw, inner=hw, nq=16, nk=16, q_outer_stride=16 * hw, q_axis_stride=hw, causal=True, kv_outer_stride=16 * hw,
                kv_axis_stride=hw, n_head=heads)


def _operands(M, C, dt):
    g = torch.Generator(device="cpu").manual_seed(1000 * M + C)
    xb = torch.randn(M, C, generator=g).to(DEV).to(dt)
    w = (torch.randn(3 * C, C, generator=g) * C ** -0.5).to(DEV).to(dt)           # gamma * W, rounded: what the MFMA multiplies
    lns = w.float().sum(dim=1).contiguous()
    lnc = (0.1 * torch.randn(3 * C, generator=g)).to(DEV)
    stats = torch.stack([0.05 * torch.randn(M, generator=g), 1.0 + 0.2 * torch.rand(M, generator=g)], 1).contiguous().to(DEV)
    return xb, w, lns, lnc, stats


def _pair(xb, w, lns, lnc, stats, M, C, hw, dt):
    """The replaced pair: ao [M, C]."""
    qkv = torch.empty(M, 3 * C, device=DEV, dtype=dt)
    ops.gemm(xb, w, qkv, M=M, N=3 * C, K=C, lda=C, ldy=3 * C, bias=lnc, ln_colsum=lns, ln_stats=stats)
    ao = torch.empty(M, C, device=DEV, dtype=dt)
    ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], ao, ldq=3 * C, ldk=3 * C, ldv=3 * C, ldo=C, **_geo(M // (16 * hw), hw, C // 32))
    return ao


def _fused(xb, w, lns, lnc, stats, M, C, hw, dt, *, out_rows=None, **rows):
    """The single launch; returns ao with its guard rows."""
    idx = ops.qkv_pack_rows(C, DEV)
    out_rows = M if out_rows is None else out_rows
    ao = torch.full((out_rows + 2 * GUARD, C), FILL, device=DEV, dtype=dt)
    try:
        ops.gemm_attn_fused_qkv(xb, w[idx].contiguous(), ao[GUARD:], axis=0, out_w=hw, M=M, C_=C, K=C, lda=C, ldy=C, bias=lnc[idx].contiguous(),
                                ln_colsum=lns[idx].contiguous(), ln_stats=stats, **rows)
    finally:
        torch.cuda.synchronize()
    return ao


def _bits(x):
    return x.contiguous().view(torch.int16)


def _fill_bits(dt):
    return _bits(torch.full((1,), FILL, dtype=dt))[0].item()


def _check(ao, want, M, dt, what):
    fill = _fill_bits(dt)
    assert bool((_bits(ao[:GUARD]) == fill).all()) and bool((_bits(ao[GUARD + M:]) == fill).all()), f"{what}: ao written outside its window"
    got = ao[GUARD:GUARD + M]
    ndiff = int((_bits(got) != _bits(want)).sum())
    print(f"{what}: {ndiff} of {got.numel()} ao elements differ, max |d| {(got.float() - want.float()).abs().max().item():.3e}")
    assert ndiff == 0, what


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("hw,clips", [(16, 1), (32, 1), (16, 2)], ids=["one-tile", "two-tiles-one-clip", "two-clips"])
def test_temporal_launch_matches_gemm_plus_causal_attention_bitwise(hw, clips, C, dt):
    M = clips * 16 * hw
    xb, w, lns, lnc, stats = _operands(M, C, dt)
    want = _pair(xb, w, lns, lnc, stats, M, C, hw, dt)
    assert bool(torch.isfinite(want.float()).all())
    ao = _fused(xb, w, lns, lnc, stats, M, C, hw, dt)
    _check(ao, want, M, dt, f"hw={hw} clips={clips} C={C} {dt}")


def test_several_entries_per_workgroup_three_tiles_per_clip():
    """hw = 48: 3 tiles per clip; 199 clips = 597 tiles = 1194 entries (no multiple of 8: the XCD chunks are uneven) on 256 workgroups -- a
    workgroup's next entry starts under the V part's row stores, the V part replays the panel through the temporal row map, clips and tiles
    divide by a non-power-of-two."""
    hw, clips, C, dt = 48, 199, 256, torch.bfloat16
    M = clips * 16 * hw
    assert M // 256 == 597
    xb, w, lns, lnc, stats = _operands(M, C, dt)
    want = _pair(xb, w, lns, lnc, stats, M, C, hw, dt)
    ao = _fused(xb, w, lns, lnc, stats, M, C, hw, dt)
    _check(ao, want, M, dt, "597 tiles")


def test_causality_later_slots_do_not_reach_earlier_outputs():
    """Independent of the pair: with the rows of the slots >= s replaced (activations and their statistics), the outputs of the slots < s keep
    their bits, for s = 1, 8, 15; the replaced slots' own outputs do change (the test's inputs are not ignored)."""
    hw, clips, C, dt = 32, 2, 256, torch.bfloat16
    M = clips * 16 * hw
    xb, w, lns, lnc, stats = _operands(M, C, dt)
    base = _fused(xb, w, lns, lnc, stats, M, C, hw, dt)[GUARD:GUARD + M].view(clips, 16, hw, C)
    g = torch.Generator(device="cpu").manual_seed(5)
    for s in (1, 8, 15):
        xb2, st2 = xb.clone().view(clips, 16, hw, C), stats.clone().view(clips, 16, hw, 2)
        xb2[:, s:] = (3.0 * torch.randn(clips, 16 - s, hw, C, generator=g)).to(DEV).to(dt)
        st2[:, s:, :, 0] += 0.25
        st2[:, s:, :, 1] *= 1.5
        got = _fused(xb2.view(M, C), w, lns, lnc, st2.view(M, 2), M, C, hw, dt)[GUARD:GUARD + M].view(clips, 16, hw, C)
        assert torch.equal(_bits(got[:, :s]), _bits(base[:, :s])), f"slots < {s} changed with the slots >= {s}"
        assert not torch.equal(_bits(got[:, s:]), _bits(base[:, s:])), f"s = {s}: the replaced slots' outputs did not change"


def test_refusals_write_nothing():
    C, dt = 256, torch.bfloat16
    fill = _fill_bits(dt)
    cases = [
        ("hw = 24", dict(hw=24, M=2 * 16 * 24), {}),                                   # 768 rows: whole 256-row tiles, but hw % 16 != 0
        ("M no whole number of clips", dict(hw=32, M=768), {}),                        # a clip is 512 rows
        ("regrouped output rows", dict(hw=16, M=512), dict(out_rows=1024, y_img_stride=32, y_off=256)),   # (slots 32 rows apart in the output)
    ]
    for what, shape, rows in cases:
        hw, M = shape["hw"], shape["M"]
        xb, w, lns, lnc, stats = _operands(M, C, dt)
        ao = torch.full((rows.get("out_rows", M) + 2 * GUARD, C), FILL, device=DEV, dtype=dt)
        idx = ops.qkv_pack_rows(C, DEV)
        kw = {k: v for k, v in rows.items() if k != "out_rows"}
        with pytest.raises(ValueError):
            ops.gemm_attn_fused_qkv(xb, w[idx].contiguous(), ao[GUARD:], axis=0, out_w=hw, M=M, C_=C, K=C, lda=C, ldy=C, bias=lnc[idx].contiguous(),
                                    ln_colsum=lns[idx].contiguous(), ln_stats=stats, **kw)
        torch.cuda.synchronize()
        assert bool((_bits(ao) == fill).all()), f"{what}: a refused call wrote to ao"


# ------------------------------------------------------------------------------------------------------------------------ the decoder
def _decoder(dt, L=16):
    torch.manual_seed(7)
    m = FlatAxialDecoder(64, 256, 64, frames_length=L, layers=3, context_channels=64).to(DEV).eval()
    m.compute_dtype = dt
    m.qkv_fuse_tiles = 0                        # (the size rule keeps calls this small on the pair)
    return m


def _inputs(m, B, hh, ww):
    g = torch.Generator(device="cpu").manual_seed(3)
    motion = torch.randn(B * hh * ww, 64, generator=g).to(DEV).to(m.compute_dtype)
    imgs = torch.randn(B * (m.frames_length - 1) * hh * ww, 64, generator=g).to(DEV).to(m.compute_dtype)
    return motion, imgs


def _logits(m, B, hh, ww):
    motion, imgs = _inputs(m, B, hh, ww)
    out = m._run(motion, imgs, B=B, hh=hh, ww=ww)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_decoder_temporal_block_takes_the_launch_and_the_switches(monkeypatch, dt):
    """L = 16, B = 1, 16 x 16 frames (M = 4096), 3 blocks (T, H, W)."""
    m = _decoder(dt)
    calls = count_lib_calls(monkeypatch)
    on = _logits(m, 1, 16, 16)
    n_on, attn_on = calls.count("mage_gemm_attn_fused_qkv"), calls.count("mage_attention")
    del calls[:]
    with config.override(tqkv_fuse=False):
        t_off = _logits(m, 1, 16, 16)
    n_toff, attn_toff = calls.count("mage_gemm_attn_fused_qkv"), calls.count("mage_attention")
    del calls[:]
    with config.override(qk_fuse=False):
        off = _logits(m, 1, 16, 16)
    n_off, attn_off = calls.count("mage_gemm_attn_fused_qkv"), calls.count("mage_attention")
    monkeypatch.undo()
    assert (n_on, attn_on) == (3, 0) and (n_toff, attn_toff) == (2, 1) and (n_off, attn_off) == (0, 3), \
        ((n_on, attn_on), (n_toff, attn_toff), (n_off, attn_off))
    assert bool(torch.isfinite(on).all())
    assert torch.equal(on, t_off) and torch.equal(on, off)
    # the incremental loop (the pair on its temporal block, one frame per step) on the same inputs ends on the full pass's last slot
    hw = 256
    motion, imgs = _inputs(m, 1, 16, 16)
    st = m._inc_begin(1, 16, 16)
    inc = m._inc_step(st, motion, imgs[:hw])
    for k in range(1, m.frames_length - 1):
        inc = m._inc_step(st, None, imgs[k * hw:(k + 1) * hw])
    torch.cuda.synchronize()
    assert torch.equal(inc, on[(m.frames_length - 2) * hw:])


def test_eight_slots_keep_the_pair_on_the_temporal_block(monkeypatch):
    """frames_length = 8: P != 16, the temporal block runs QKV GEMM + attention whatever the switch says."""
    m = _decoder(torch.bfloat16, L=8)
    calls = count_lib_calls(monkeypatch)
    n, out = [], []
    for sw in (True, False):
        del calls[:]
        with config.override(tqkv_fuse=sw):
            out.append(_logits(m, 2, 16, 16))
        n.append((calls.count("mage_gemm_attn_fused_qkv"), calls.count("mage_attention")))
    monkeypatch.undo()
    assert n == [(2, 1), (2, 1)], n
    assert torch.equal(out[0], out[1])
