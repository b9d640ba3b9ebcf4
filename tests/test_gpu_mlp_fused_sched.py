"""GPU: the chunk epilogue of the fused decoder MLP (mage_mlp_fused, csrc/gemm4m.hip) is issued one operation per MFMA slot across two phases: a
chunk's block 0 under GEMM 2 of the chunk before (Pb), its block 1 and its pack under GEMM 1 of the chunk after (Pa), the first chunk's block 0
and the last chunk's block 1 with no MFMA beside them.  A slot that reads a value too early, a constant of the wrong block or chunk, or a pack
that runs ahead of its block changes bits; these operands make such a fault show WHERE it is.  Against the pair the launch replaces -- ops.gemm
(c_fc, LN-consume, QuickGELU) + ops.gemm (c_proj, 16-bit residual, with and without ln_part), built as tests/test_gpu_mlp_fused_close.py builds
it -- BIT FOR BIT on the output rows and on ln_part, bf16 and f16.  No tolerance anywhere.

  * sizes: M = 128 (one tile) and M = 128 (n_cu + 1): workgroup 0 runs a second tile, whose chunk 0 follows the first tile's chunk 63;
  * chunk-localised weights: w2 is non-zero only in the 16 hidden units of ONE (chunk, block t) pair -- hidden units 32 chunk + 8 q + 4 t + e,
    q, e = 0 .. 3, the kernel's block t -- so only that block's activation reaches the output; c1 and s1 are random (s1 is NOT w1's row sums:
    a column sum of another block or chunk gives another value).  chunk in {0, 1, 2, 62, 63} x t in {0, 1}: the peeled chunks, the loop's first
    and last iteration, the tail, each half of the split;
  * transcendental extremes: rows whose rstd is 200 times the true one, so that -1.702 log2(e) x passes +-128 on most hidden units (exp -> inf
    and -> 0, rcp of inf), an all-zero row and a constant row (both with rstd = eps ** -0.5), with the true column sums.
Every buffer the launch reads or writes by rows has NaN guard rows.
"""
import pytest
import torch

from mage_amd import ops

DEV = "cuda:0"
GUARD = 32
CC = 512
EPS = 1e-5
gpu = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


def _ncu():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _sizes():
    return (128, 128 * (_ncu() + 1))


_BASE = {}


def _base(M, dt, kind):
    """Rows, c_fc's operands, the (mean, rstd) rows and the pair's hidden rows (which do not depend on w2): once per (M, dt, kind)."""
    key = (M, dt, kind)
    if key in _BASE:
        return _BASE[key]
    g = torch.Generator(device="cpu").manual_seed(2900 + M % 9973 + (5 if dt == torch.float16 else 0) + (11 if kind == "extreme" else 0))
    x = torch.randn(M, CC, generator=g)
    x *= torch.tensor([0.1, 1.0, 30.0])[torch.arange(M) % 3][:, None]
    x[7] = 0.0                                          # an all-zero row: mean 0, rstd = eps ** -0.5
    x[M - 2] = -1.5                                     # a constant row: rstd = eps ** -0.5
    x = x.to(dt).to(DEV).contiguous()
    w1 = (torch.randn(4 * CC, CC, generator=g) * CC ** -0.5).to(DEV).to(dt)
    c1 = (0.1 * torch.randn(4 * CC, generator=g)).to(DEV)
    if kind == "extreme":
        s1 = w1.float().sum(dim=1).contiguous()
    else:
        s1 = torch.randn(4 * CC, generator=g).to(DEV)   # random, not the row sums: every hidden unit has a column sum of its own
    stats = torch.empty(M, 2, device=DEV)
    ops.row_stats(x, EPS, stats)
    if kind == "extreme":
        assert abs(stats[7, 1].item() - EPS ** -0.5) < 1e-2 * EPS ** -0.5 and abs(stats[M - 2, 1].item() - EPS ** -0.5) < 1e-2 * EPS ** -0.5
        stats[0::5, 1] *= 200.0
    Mp = (M + 255) // 256 * 256
    xb = torch.zeros(Mp, CC, device=DEV, dtype=dt)
    xb[:M] = x
    stp = torch.zeros(Mp, 2, device=DEV)
    stp[:, 1] = 1.0
    stp[:M] = stats
    hdn = torch.empty(Mp, 4 * CC, device=DEV, dtype=dt)
    ops.gemm(xb, w1, hdn, M=Mp, N=4 * CC, K=CC, lda=CC, ldy=4 * CC, bias=c1, ln_colsum=s1, ln_stats=stp, act=ops.ACT_QUICKGELU)
    torch.cuda.synchronize()
    b2 = (0.1 * torch.randn(CC, generator=g)).to(DEV)
    w2 = (torch.randn(CC, 4 * CC, generator=g) * (4 * CC) ** -0.5).to(DEV).to(dt)
    _BASE[key] = dict(x=x, xb=xb, w1=w1, c1=c1, s1=s1, stats=stats, hdn=hdn, b2=b2, w2=w2, Mp=Mp)
    return _BASE[key]


def _block_units(chunk, t):
    q, e = torch.arange(4)[:, None], torch.arange(4)[None, :]
    return (32 * chunk + 8 * q + 4 * t + e).reshape(-1).to(DEV)


def _pair(b, M, w2):
    """c_proj of the pair on the shared hidden rows: (rows with ln_part, ln_part, rows without)."""
    Mp = b["Mp"]
    part = torch.empty(CC // 64, Mp, 2, device=DEV)
    y_ln = torch.empty(Mp, CC, device=DEV, dtype=w2.dtype)
    ops.gemm(b["hdn"], w2, y_ln, M=Mp, N=CC, K=4 * CC, lda=4 * CC, ldy=CC, bias=b["b2"], residual=b["xb"], ldr=CC, ln_part=part)
    y_plain = torch.empty(Mp, CC, device=DEV, dtype=w2.dtype)
    ops.gemm(b["hdn"], w2, y_plain, M=Mp, N=CC, K=4 * CC, lda=4 * CC, ldy=CC, bias=b["b2"], residual=b["xb"], ldr=CC)
    torch.cuda.synchronize()
    return y_ln[:M], part[:, :M], y_plain[:M]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _check(got, want, what):
    bad = _bits(got) != _bits(want)
    ndiff = int(bad.sum())
    print(f"{what}: {ndiff} of {got.numel()} elements differ")
    if ndiff:
        r, c = bad.nonzero(as_tuple=True)
        print(f"{what}: rows % 32 with differences: {sorted(set((r % 32).tolist()))}")
        print(f"{what}: 128-row tiles with differences: {sorted(set((r // 128).tolist()))[:32]}")
    assert ndiff == 0, what


def _part_rows(part, off, M):
    return part[:, off:off + M].permute(1, 0, 2).reshape(M, -1)


def _fused_both_forms(b, M, w2, want, what):
    y_ln, part_w, y_plain = want
    kw = dict(C_=CC, w1=b["w1"], c1=b["c1"], s1=b["s1"], ln_stats=b["stats"], w2=w2, b2=b["b2"])
    dt = w2.dtype
    # in place, ln_part written
    x = torch.full((M + 2 * GUARD, CC), float("nan"), device=DEV, dtype=dt)
    x[GUARD:GUARD + M] = b["x"]
    part = torch.full((CC // 64, M + 2 * GUARD, 2), float("nan"), device=DEV)
    ops.mlp_fused(x, x, M=M, ln_part=part, a_off=GUARD, y_off=GUARD, **kw)
    torch.cuda.synchronize()
    assert _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "rows written outside the tiles"
    assert _all_nan(part[:, :GUARD]) and _all_nan(part[:, GUARD + M:]), "partial sums written outside the tiles"
    _check(x[GUARD:GUARD + M], y_ln, f"{what}, M = {M}, in place: rows")
    _check(_part_rows(part, GUARD, M), _part_rows(part_w, 0, M), f"{what}, M = {M}, in place: ln_part")
    # separate output, no ln_part
    x = torch.full((M + 2 * GUARD, CC), float("nan"), device=DEV, dtype=dt)
    x[GUARD:GUARD + M] = b["x"]
    y = torch.full((M + 3 * GUARD, CC), float("nan"), device=DEV, dtype=dt)
    ops.mlp_fused(x, y, M=M, a_off=GUARD, y_off=2 * GUARD, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x[GUARD:GUARD + M]), _bits(b["x"])) and _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "x changed"
    assert _all_nan(y[:2 * GUARD]) and _all_nan(y[2 * GUARD + M:]), "rows written outside the tiles"
    _check(y[2 * GUARD:2 * GUARD + M], y_plain, f"{what}, M = {M}, separate output: rows")


@gpu
@DTYPES
@pytest.mark.parametrize("t", [0, 1], ids=["block0", "block1"])
@pytest.mark.parametrize("chunk", [0, 1, 2, 62, 63])
def test_one_block_of_one_chunk_reaches_the_output(dt, chunk, t):
    for M in _sizes():
        b = _base(M, dt, "normal")
        units = _block_units(chunk, t)
        w2 = torch.zeros_like(b["w2"])
        w2[:, units] = b["w2"][:, units]
        want = _pair(b, M, w2)
        # the case is what it claims: the block's hidden values move the output away from x + b2 (so a wrong activation shows)
        moved = (want[2].float() - (b["x"].float() + b["b2"])).abs().max().item()
        print(f"chunk {chunk}, block {t}, M = {M}: max |y - (x + b2)| of the pair = {moved:.3e}")
        assert moved > 1e-2
        _fused_both_forms(b, M, w2, want, f"chunk {chunk} block {t}")


@gpu
@DTYPES
def test_transcendental_extremes(dt):
    for M in _sizes():
        b = _base(M, dt, "extreme")
        # the scaled rows drive the exponent past +-128 on most hidden units, in both directions
        pre = b["hdn"][0].float()
        big, zero = int((pre > 100).sum()), int((pre == 0).sum())
        print(f"M = {M}, row 0 (rstd x 200): {big} hidden values above 100 (sigmoid = 1), {zero} exactly 0 (exp -> inf, rcp -> 0) of {pre.numel()}")
        assert big > 100 and zero > 100
        want = _pair(b, M, b["w2"])
        assert bool(torch.isfinite(want[2].float()).all())
        _fused_both_forms(b, M, b["w2"], want, "extremes")
