"""GPU: a decoder block's MLP in ONE launch (mage_mlp_fused, csrc/gemm4m.hip: c_fc with the LayerNorm fold, QuickGELU and c_proj with the 16-bit
residual; the hidden rows stay on the CU) against the pair it replaces -- ops.gemm (c_fc, LN-consume, QuickGELU) + ops.gemm (c_proj, 16-bit
residual, ln_part) -- BIT FOR BIT on the output rows and on the LayerNorm partial sums.  No tolerance anywhere.

  * M = 128 (one tile), 256, 128 (CUs + 1) (one workgroup runs a second tile), 128 (3 CUs + 5) (several tiles per workgroup: the weight rings and
    the prefetched rows carried across tiles; first and last tile of a workgroup checked on their own); bf16 and f16;
  * rows of standard-normal x scaled by 0.1, 1 and 30, one all-zero row and one constant row (rstd large), a few +-1e3 entries;
  * NaN-sentinel guard rows before and after x, ln_part and the output: the footprint is exactly the rows of the tiles;
  * both forms: in place with ln_part, and a separate output without ln_part (the last block's); row offsets a_off / y_off;
  * the decoder: logits and tokens with the route on == mlp_fuse=False, full loop == incremental loop, the size rule, what keeps the pair;
  * refusals (each MAGE_EINVAL with its own message), also through the *_kernel_name query, which launches nothing;
  * CPU: the two entry points' ctypes signatures against the header.
"""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import pytest
import torch

from mage_amd import _lib, config, ops
from mage_amd.modules.mage_model import FlatAxialDecoder
from tests.helpers import count_lib_calls

DEV = "cuda:0"
GUARD = 32                  # sentinel rows in front of and behind every buffer the launch writes or reads by rows
CC = 512
gpu = pytest.mark.gpu


def _ncu():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


_CACHE = {}


def _operands(M, dt):
    """x with guard rows (NaN), the folded c_fc and c_proj operands, (mean, rstd) rows; the pair's outputs, computed once per (M, dt)."""
    key = (M, dt)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator(device="cpu").manual_seed(M + (7 if dt == torch.float16 else 0))
    x = torch.randn(M, CC, generator=g)
    x *= torch.tensor([0.1, 1.0, 30.0])[torch.arange(M) % 3][:, None]
    x[5] = 0.0                                          # an all-zero row
    x[M - 3] = 2.5                                      # a constant row
    big = torch.randint(0, M * CC, (16,), generator=g)
    x.view(-1)[big] = torch.tensor([1e3, -1e3]).repeat(8)
    xg = torch.full((M + 2 * GUARD, CC), float("nan"), dtype=dt)
    xg[GUARD:GUARD + M] = x.to(dt)
    xg = xg.to(DEV)
    w1 = (torch.randn(4 * CC, CC, generator=g) * CC ** -0.5).to(DEV).to(dt)
    s1 = w1.float().sum(dim=1).contiguous()
    c1 = (0.1 * torch.randn(4 * CC, generator=g)).to(DEV)
    w2 = (torch.randn(CC, 4 * CC, generator=g) * (4 * CC) ** -0.5).to(DEV).to(dt)
    b2 = (0.1 * torch.randn(CC, generator=g)).to(DEV)
    stats = torch.empty(M, 2, device=DEV)
    ops.row_stats(xg[GUARD:GUARD + M], 1e-5, stats)     # the constant and the zero row: rstd = eps ** -0.5
    # ---- the pair.  Its LayerNorm-folded forms take whole 256-row tiles: an odd number of 128-row tiles is padded with zero rows (rows are
    # independent of each other in both GEMMs), and only the first M rows are compared.
    Mp = (M + 255) // 256 * 256
    xb = torch.zeros(Mp, CC, device=DEV, dtype=dt)
    xb[:M] = xg[GUARD:GUARD + M]
    stp = torch.zeros(Mp, 2, device=DEV)
    stp[:, 1] = 1.0
    stp[:M] = stats
    hdn = torch.empty(Mp, 4 * CC, device=DEV, dtype=dt)
    ops.gemm(xb, w1, hdn, M=Mp, N=4 * CC, K=CC, lda=CC, ldy=4 * CC, bias=c1, ln_colsum=s1, ln_stats=stp, act=ops.ACT_QUICKGELU)
    part = torch.empty(CC // 64, Mp, 2, device=DEV)
    y_ln = torch.empty(Mp, CC, device=DEV, dtype=dt)
    ops.gemm(hdn, w2, y_ln, M=Mp, N=CC, K=4 * CC, lda=4 * CC, ldy=CC, bias=b2, residual=xb, ldr=CC, ln_part=part)
    y_plain = torch.empty(Mp, CC, device=DEV, dtype=dt)
    ops.gemm(hdn, w2, y_plain, M=Mp, N=CC, K=4 * CC, lda=4 * CC, ldy=CC, bias=b2, residual=xb, ldr=CC)
    torch.cuda.synchronize()
    del hdn
    y_ln, y_plain, part = y_ln[:M], y_plain[:M], part[:, :M]
    _CACHE[key] = dict(xg=xg, w1=w1, s1=s1, c1=c1, w2=w2, b2=b2, stats=stats, y_ln=y_ln, y_plain=y_plain, part=part)
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _sizes():
    n = _ncu()
    return [128, 256, 128 * (n + 1), 128 * (3 * n + 5)]


def _check_rows(got, want, M, what):
    n = _ncu()
    ndiff = int((_bits(got) != _bits(want)).sum())
    print(f"{what}: M={M}: {ndiff} of {got.numel()} elements differ")
    assert ndiff == 0, what
    if M > 128 * n:                                     # workgroup 0's first and last tile, on their own
        last = ((M // 128 - 1) // n) * n
        for t in (0, last):
            assert torch.equal(_bits(got[128 * t:128 * t + 128]), _bits(want[128 * t:128 * t + 128])), (what, "tile", t)


@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mi", range(4), ids=["one_tile", "two_tiles", "cus_plus_1", "several_per_wg"])
def test_in_place_with_ln_part_matches_the_pair_bitwise(mi, dt):
    M = _sizes()[mi]
    o = _operands(M, dt)
    x = o["xg"].clone()
    part = torch.full((CC // 64, M + 2 * GUARD, 2), float("nan"), device=DEV)
    ops.mlp_fused(x, x, M=M, C_=CC, w1=o["w1"], c1=o["c1"], s1=o["s1"], ln_stats=o["stats"], w2=o["w2"], b2=o["b2"], ln_part=part, a_off=GUARD,
                  y_off=GUARD)
    torch.cuda.synchronize()
    assert _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "rows written outside the tiles"
    assert _all_nan(part[:, :GUARD]) and _all_nan(part[:, GUARD + M:]), "partial sums written outside the tiles"
    _check_rows(x[GUARD:GUARD + M], o["y_ln"], M, "rows")
    _check_rows(part[:, GUARD:GUARD + M].transpose(0, 1), o["part"].transpose(0, 1), M, "ln_part")


@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mi", range(4), ids=["one_tile", "two_tiles", "cus_plus_1", "several_per_wg"])
def test_separate_output_without_ln_part_matches_the_pair_bitwise(mi, dt):
    """The last block's form; the input at row offset GUARD, the output at another offset."""
    M = _sizes()[mi]
    o = _operands(M, dt)
    x = o["xg"].clone()
    y = torch.full((M + 3 * GUARD, CC), float("nan"), device=DEV, dtype=dt)
    ops.mlp_fused(x, y, M=M, C_=CC, w1=o["w1"], c1=o["c1"], s1=o["s1"], ln_stats=o["stats"], w2=o["w2"], b2=o["b2"], a_off=GUARD, y_off=2 * GUARD)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x[GUARD:GUARD + M]), _bits(o["xg"][GUARD:GUARD + M])) and _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "x changed"
    assert _all_nan(y[:2 * GUARD]) and _all_nan(y[2 * GUARD + M:]), "rows written outside the tiles"
    _check_rows(y[2 * GUARD:2 * GUARD + M], o["y_plain"], M, "rows")


# ---- the decoder
def _decoder(dt, Cc=512, tiles=0, **kw):
    torch.manual_seed(7)
    m = FlatAxialDecoder(64, Cc, 64, frames_length=2, layers=3, context_channels=64, **kw).to(DEV).eval()
    m.compute_dtype = dt
    if tiles is not None:
        m.mlp_fuse_tiles = tiles
    return m


def _inputs(m, B, hh, ww):
    g = torch.Generator(device="cpu").manual_seed(3)
    dt = m.compute_dtype
    motion = torch.randn(B * hh * ww, 64, generator=g).to(DEV).to(dt)
    imgs = torch.randn(B * (m.frames_length - 1) * hh * ww, 64, generator=g).to(DEV).to(dt)
    return motion, imgs


def _logits(m, B=4, hh=16, ww=16):
    motion, imgs = _inputs(m, B, hh, ww)
    out = m._run(motion, imgs, B=B, hh=hh, ww=ww)
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_decoder_route_on_equals_the_pair_and_the_incremental_loop(monkeypatch, dt):
    m = _decoder(dt)
    calls = count_lib_calls(monkeypatch)
    on = _logits(m)
    n_on = calls.count("mage_mlp_fused")
    del calls[:]
    with config.override(mlp_fuse=False):
        off = _logits(m)
    n_off = calls.count("mage_mlp_fused")
    monkeypatch.undo()
    assert n_on == m.layers and n_off == 0, (n_on, n_off)
    assert torch.equal(on, off) and torch.equal(on.argmax(-1), off.argmax(-1))
    # the incremental loop (one frame per step) on the same inputs: the last slot's logits
    motion, imgs = _inputs(m, 4, 16, 16)
    st = m._inc_begin(4, 16, 16)
    inc = m._inc_step(st, motion, imgs)
    torch.cuda.synchronize()
    assert torch.equal(inc, on)


@gpu
def test_size_rule_counts_tiles_per_cu(monkeypatch):
    """B = 4, L = 2, 16 x 16 frames: M = 2048 rows = 16 tiles of 128: fused from mlp_fuse_tiles * n_cu <= 16 on; the default (eight tiles per CU)
    keeps a call this small on the pair."""
    n_cu = _ncu()
    m = _decoder(torch.bfloat16, tiles=None)
    assert m.mlp_fuse_tiles == 8
    calls = count_lib_calls(monkeypatch)
    n = []
    for tiles in (None, Fraction(16, n_cu), Fraction(17, n_cu)):
        if tiles is not None:
            m.mlp_fuse_tiles = tiles
        del calls[:]
        _logits(m)
        n.append(calls.count("mage_mlp_fused"))
    monkeypatch.undo()
    assert n == [0, m.layers, 0], n


def _keys(m, **kw):
    ops.PROFILE.reset(enabled=True)
    try:
        _logits(m, **kw)
        return set(ops.PROFILE.summary())
    finally:
        ops.PROFILE.reset()


@gpu
def test_what_keeps_the_pair(monkeypatch):
    """Through the profile keys: the fused kernel's symbol appears on the route, and not for widths 256 / 768, use_cids=False, fp32 and a split mode."""
    on = _keys(_decoder(torch.bfloat16))
    assert any("gemm4m_kernel" in k for k in on), on
    for Cc in (256, 768):
        assert not any("gemm4m_kernel" in k for k in _keys(_decoder(torch.bfloat16, Cc=Cc)))
    assert not any("gemm4m_kernel" in k for k in _keys(_decoder(torch.bfloat16, use_cids=False)))
    assert not any("gemm4m_kernel" in k for k in _keys(_decoder(torch.float32)))
    ms = _decoder(torch.float32)
    ms.split_kind = ops.F16X3
    assert not any("gemm4m_kernel" in k for k in _keys(ms))


# ---- refusals
def _raw_args(o, M, *, dtype=None, w_dtype=None, y_dtype=None, C_=CC, ldx=CC, ldy=CC, ldw1=CC, ldw2=4 * CC, x_shift=0):
    x = o["xg"]
    dt = ops.code(x)
    return (dt if dtype is None else dtype, dt if w_dtype is None else w_dtype, dt if y_dtype is None else y_dtype, M, C_, x.data_ptr() + x_shift, ldx, GUARD,
            x.data_ptr() + x_shift, ldy, GUARD, o["w1"].data_ptr(), ldw1, o["c1"].data_ptr(), o["s1"].data_ptr(), o["stats"].data_ptr(), o["w2"].data_ptr(),
            ldw2, o["b2"].data_ptr(), None, 0)


@gpu
def test_refusals_each_with_its_own_message_and_nothing_launched():
    o = _operands(256, torch.bfloat16)
    l, s = ops._dev(o["xg"])
    before = o["xg"].clone()
    cases = {
        "multiple of 128": _raw_args(o, 200),
        "C = 512": _raw_args(o, 256, C_=256),
        "must have the type of x": _raw_args(o, 256, w_dtype=ops.F16),
        "ldx=": _raw_args(o, 256, ldx=504),
        "ldw1=": _raw_args(o, 256, ldw2=2040),
        "16-byte aligned": _raw_args(o, 256, x_shift=8),
    }
    seen = set()
    buf = C.create_string_buffer(256)
    for want, args in cases.items():
        for call in (lambda: l.mage_mlp_fused(*args, s), lambda: l.mage_mlp_fused_kernel_name(*args, buf, len(buf))):
            r = call()
            msg = l.mage_last_error().decode()
            assert r == -1 and want in msg, (want, r, msg)
            seen.add(msg)
    assert len(seen) == len(cases)
    # the query on valid arguments names the kernel and launches nothing
    assert l.mage_mlp_fused_kernel_name(*_raw_args(o, 256), buf, len(buf)) == 0 and b"gemm4m_kernel" in buf.value
    torch.cuda.synchronize()
    assert torch.equal(_bits(o["xg"][GUARD:GUARD + 256]), _bits(before[GUARD:GUARD + 256]))


# ---- CPU
def test_signatures_match_the_header():
    text = Path(__file__).resolve().parents[1].joinpath("include", "mage_hip_ext.h").read_text()
    for name in ("mage_mlp_fused", "mage_mlp_fused_kernel_name"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert decl, name
        res, args = _lib.EXT_SIGNATURES[name]
        assert res is C.c_int and len(decl.group(1).split(",")) == len(args), name
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    assert "mlp_fuse" in config.ENV and config.ENV["mlp_fuse"] == ("MAGE_NO_MLP_FUSE", False) and config.Config().mlp_fuse is True
