"""GPU: the closing epilogue of the fused decoder MLP (mage_mlp_fused, csrc/gemm4m.hip) takes the residual from the wave's own x fragments, requests the
next tile's rows slice by slice while it runs and the bias one slice ahead.  The cases tests/test_gpu_mlp_fused.py does not have, against the pair
the launch replaces -- ops.gemm (c_fc, LN-consume, QuickGELU) + ops.gemm (c_proj, 16-bit residual, with and without ln_part), on 256-row-padded
copies, the first M rows compared -- BIT FOR BIT on the output rows and on ln_part.  No tolerance anywhere.  bf16 and f16.

  * strided rows: ldx = ldy = 576, in place, M = 256; the 64 gap columns of every row carry a sentinel and must keep it;
  * separate output at other offsets and strides: x != y, a_off = 32, y_off = 96, ldx = 512, ldy = 640, with and without ln_part; x unchanged;
  * residual-dominated rows: x[r, c] = +-2^((c // 8) % 12 - 6) (1 + (r % 32) / 64), w2 scaled by 2^-12, b2 = 0: every 8-column chunk and every row
    of a wave has its own magnitude and the output is the residual to within the last bits, so a misrouted fragment shows; M = 128 and 256;
  * tile hand-overs: M = 128 (2 n_cu + 1): workgroup 0 runs three tiles (the slice-by-slice prefetch carried over two hand-overs), the last
    workgroups two, ending without a next tile; workgroup 0's first, middle and last tile checked on their own;
  * one tile: M = 128, no next tile at all.
Every buffer the launch reads or writes by rows has NaN guard rows.  A mismatch prints which (row % 32, column // 8) positions differ: the wave's
row and the 8-column fragment chunk.
"""
import pytest
import torch

from mage_amd import ops

DEV = "cuda:0"
GUARD = 32
CC = 512
SENT = -1234.0              # the gap columns' sentinel (exact in bf16 and f16)
gpu = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


def _ncu():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


_CACHE = {}


def _rows(M, kind, g):
    if kind == "residual":
        r, c = torch.arange(M)[:, None], torch.arange(CC)[None, :]
        sign = 1.0 - 2.0 * ((r + c // 8 + c) % 2).float()
        return sign * torch.exp2(((c // 8) % 12 - 6).float()) * (1.0 + (r % 32).float() / 64.0)
    x = torch.randn(M, CC, generator=g)
    x *= torch.tensor([0.1, 1.0, 30.0])[torch.arange(M) % 3][:, None]
    x[7] = 0.0                                          # an all-zero row
    x[M - 2] = -1.5                                     # a constant row
    return x


def _operands(M, dt, kind="normal"):
    """The rows (contiguous, on the device), the folded c_fc and c_proj operands, (mean, rstd) rows and the pair's outputs: once per (M, dt, kind)."""
    key = (M, dt, kind)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator(device="cpu").manual_seed(1000 + M % 9973 + (5 if dt == torch.float16 else 0) + (11 if kind == "residual" else 0))
    x = _rows(M, kind, g).to(dt).to(DEV).contiguous()
    w1 = (torch.randn(4 * CC, CC, generator=g) * CC ** -0.5).to(DEV).to(dt)
    s1 = w1.float().sum(dim=1).contiguous()
    c1 = (0.1 * torch.randn(4 * CC, generator=g)).to(DEV)
    w2 = torch.randn(CC, 4 * CC, generator=g) * (4 * CC) ** -0.5
    b2 = 0.1 * torch.randn(CC, generator=g)
    if kind == "residual":
        w2, b2 = w2 * 2.0 ** -12, torch.zeros(CC)
    w2, b2 = w2.to(DEV).to(dt), b2.to(DEV)
    stats = torch.empty(M, 2, device=DEV)
    ops.row_stats(x, 1e-5, stats)
    # ---- the pair, on whole 256-row tiles (zero rows appended; rows are independent of each other in both GEMMs)
    Mp = (M + 255) // 256 * 256
    xb = torch.zeros(Mp, CC, device=DEV, dtype=dt)
    xb[:M] = x
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
    del hdn, xb
    _CACHE[key] = dict(x=x, w1=w1, s1=s1, c1=c1, w2=w2, b2=b2, stats=stats, y_ln=y_ln[:M], y_plain=y_plain[:M], part=part[:, :M])
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _check(got, want, what, tiles=()):
    """got, want: [M, columns] rows (16 columns of fp32 for ln_part: slice-major pairs).  Prints where they differ before it asserts."""
    bad = _bits(got) != _bits(want)
    ndiff = int(bad.sum())
    per_chunk = 8 if got.element_size() == 2 else 2     # rows: 8 columns per fragment chunk; ln_part: one (sum, sum of squares) pair per slice
    print(f"{what}: {ndiff} of {got.numel()} elements differ")
    if ndiff:
        r, c = bad.nonzero(as_tuple=True)
        where = sorted(set(zip((r % 32).tolist(), (c // per_chunk).tolist())))
        print(f"{what}: (row % 32, column // {per_chunk}) of the differing positions: {where[:64]}{' ...' if len(where) > 64 else ''}")
        print(f"{what}: 128-row tiles with differences: {sorted(set((r // 128).tolist()))[:32]}")
    assert ndiff == 0, what
    for t in tiles:
        assert torch.equal(_bits(got[128 * t:128 * t + 128]), _bits(want[128 * t:128 * t + 128])), (what, "tile", t)


def _part_rows(part, off, M):
    """ln_part [8, rows, 2] -> [M, 16]: row-major view of the M rows from `off` on."""
    return part[:, off:off + M].permute(1, 0, 2).reshape(M, -1)


def _kw(o):
    return dict(C_=CC, w1=o["w1"], c1=o["c1"], s1=o["s1"], ln_stats=o["stats"], w2=o["w2"], b2=o["b2"])


def _guarded(o, M, ld=CC, a_off=GUARD):
    """The rows at row offset a_off of a NaN buffer with row stride ld; gap columns (ld > 512) hold the sentinel."""
    dt = o["x"].dtype
    buf = torch.full((a_off + M + GUARD, ld), float("nan"), device=DEV, dtype=dt)
    buf[a_off:a_off + M, :CC] = o["x"]
    buf[a_off:a_off + M, CC:] = SENT
    return buf


def _run_in_place(o, M, tiles=()):
    x = _guarded(o, M)
    part = torch.full((CC // 64, M + 2 * GUARD, 2), float("nan"), device=DEV)
    ops.mlp_fused(x, x, M=M, ln_part=part, a_off=GUARD, y_off=GUARD, **_kw(o))
    torch.cuda.synchronize()
    assert _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "rows written outside the tiles"
    assert _all_nan(part[:, :GUARD]) and _all_nan(part[:, GUARD + M:]), "partial sums written outside the tiles"
    _check(x[GUARD:GUARD + M], o["y_ln"], "rows", tiles)
    _check(_part_rows(part, GUARD, M), _part_rows(o["part"], 0, M), "ln_part", tiles)


def _run_separate(o, M, tiles=()):
    x = _guarded(o, M)
    before = x.clone()
    y = torch.full((M + 3 * GUARD, CC), float("nan"), device=DEV, dtype=x.dtype)
    ops.mlp_fused(x, y, M=M, a_off=GUARD, y_off=2 * GUARD, **_kw(o))
    torch.cuda.synchronize()
    assert torch.equal(_bits(x[GUARD:GUARD + M]), _bits(before[GUARD:GUARD + M])) and _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "x changed"
    assert _all_nan(y[:2 * GUARD]) and _all_nan(y[2 * GUARD + M:]), "rows written outside the tiles"
    _check(y[2 * GUARD:2 * GUARD + M], o["y_plain"], "rows", tiles)


FORMS = pytest.mark.parametrize("form", ["in_place_ln_part", "separate_plain"])


@gpu
@DTYPES
def test_strided_rows_in_place_leave_the_gap_columns_alone(dt):
    M, LD = 256, 576
    o = _operands(M, dt)
    x = _guarded(o, M, ld=LD)
    part = torch.full((CC // 64, M + 2 * GUARD, 2), float("nan"), device=DEV)
    ops.mlp_fused(x, x, M=M, ln_part=part, ldx=LD, ldy=LD, a_off=GUARD, y_off=GUARD, **_kw(o))
    torch.cuda.synchronize()
    assert _all_nan(x[:GUARD]) and _all_nan(x[GUARD + M:]), "rows written outside the tiles"
    assert bool((x[GUARD:GUARD + M, CC:] == SENT).all()), "gap columns written"
    assert _all_nan(part[:, :GUARD]) and _all_nan(part[:, GUARD + M:]), "partial sums written outside the tiles"
    _check(x[GUARD:GUARD + M, :CC], o["y_ln"], "rows")
    _check(_part_rows(part, GUARD, M), _part_rows(o["part"], 0, M), "ln_part")


@gpu
@DTYPES
@pytest.mark.parametrize("with_part", [True, False], ids=["ln_part", "plain"])
def test_separate_output_at_other_offsets_and_strides(dt, with_part):
    M, A_OFF, Y_OFF, LDY = 256, 32, 96, 640
    o = _operands(M, dt)
    x = _guarded(o, M, a_off=A_OFF)
    before = x.clone()
    y = torch.full((Y_OFF + M + GUARD, LDY), float("nan"), device=DEV, dtype=dt)
    y[Y_OFF:Y_OFF + M, CC:] = SENT
    part = torch.full((CC // 64, Y_OFF + M + GUARD, 2), float("nan"), device=DEV) if with_part else None
    ops.mlp_fused(x, y, M=M, ln_part=part, ldx=CC, ldy=LDY, a_off=A_OFF, y_off=Y_OFF, **_kw(o))
    torch.cuda.synchronize()
    assert torch.equal(_bits(x[A_OFF:A_OFF + M]), _bits(before[A_OFF:A_OFF + M])) and _all_nan(x[:A_OFF]) and _all_nan(x[A_OFF + M:]), "x changed"
    assert _all_nan(y[:Y_OFF]) and _all_nan(y[Y_OFF + M:]), "rows written outside the tiles"
    assert bool((y[Y_OFF:Y_OFF + M, CC:] == SENT).all()), "gap columns written"
    _check(y[Y_OFF:Y_OFF + M, :CC], o["y_ln"] if with_part else o["y_plain"], "rows")
    if with_part:
        assert _all_nan(part[:, :Y_OFF]) and _all_nan(part[:, Y_OFF + M:]), "partial sums written outside the tiles"
        _check(_part_rows(part, Y_OFF, M), _part_rows(o["part"], 0, M), "ln_part")


@gpu
@DTYPES
@pytest.mark.parametrize("M", [128, 256])
def test_residual_dominated_rows(dt, M):
    o = _operands(M, dt, "residual")
    # the pattern is what it claims: the pair's output is the residual to within a few units in the last place
    rel = ((o["y_ln"].float() - o["x"].float()).abs() / o["x"].float().abs()).max().item()
    print(f"residual-dominated rows: max |y - x| / |x| of the pair = {rel:.3e}")
    _run_in_place(o, M)
    _run_separate(o, M)


@gpu
@DTYPES
@FORMS
def test_tile_hand_overs_three_tiles_on_workgroup_0(dt, form):
    n = _ncu()
    M = 128 * (2 * n + 1)
    o = _operands(M, dt)
    (_run_in_place if form == "in_place_ln_part" else _run_separate)(o, M, tiles=(0, n, 2 * n))


@gpu
@DTYPES
@FORMS
def test_one_tile_has_no_next_tile(dt, form):
    o = _operands(128, dt)
    (_run_in_place if form == "in_place_ln_part" else _run_separate)(o, 128)
