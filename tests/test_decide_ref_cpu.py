"""CPU: the references, case tables and checkers of tests/decide_ref.py, without a GPU.  The references agree with torch's own fp64 (torch.min over
the quantiser's formula, torch.max, F.cross_entropy); every quantiser case has zero soft rows and holds the rows it was built for (duplicates
hit exactly, the last code, K = 1); an fp32 emulation of the inexact kernels in their own order sits inside the bounds; the buffers a correct
kernel leaves pass the checkers, and wrong answers built from the reference (MUTANTS below) do not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import decide_ref as R

F32, F64 = np.float32, np.float64


def rejects(check, *a, **kw):
    with pytest.raises(AssertionError):
        check(*a, **kw)


# ------------------------------------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("c", R.VQ_CASES, ids=R.case_id)
def test_vq_case_has_no_soft_row_and_agrees_with_torch(c):
    i, r = R.vq_case(c)
    assert not r.soft.any() and not r.soft_codes.any(), "a committed case has a soft row"
    z, cb = torch.from_numpy(i.z).double(), torch.from_numpy(i.cb).double()
    x2, c2, dot = (z * z).sum(1).float(), (cb * cb).sum(1).float(), (z @ cb.T).float()         # fp64 sums in torch's order, rounded once
    dist = (c2[None, :] + x2[:, None]) - 2.0 * dot
    assert dist.dtype == torch.float32 and np.array_equal(R.bits(dist.numpy()), R.bits(r.dist)), "no soft pair: the distances are determined"
    val, idx = torch.min(dist, 1)
    assert np.array_equal(val.numpy(), r.dist[np.arange(r.M), r.idx])
    clear = r.margin > 0
    assert np.array_equal(idx.numpy()[clear], r.idx[clear])
    assert np.array_equal(r.cbt, i.cb.T) and np.array_equal(r.c2, c2.numpy())
    R.check_vq(c["name"], r, R.filled(r.M + R.TAIL, np.arange(r.M), r.idx), R.filled(r.M + R.TAIL, np.arange(r.M), r.margin))
    R.check_vq_prepare(c["name"], r, R.filled(r.D * r.K + R.TAIL, np.arange(r.D * r.K), r.cbt), R.filled(r.K + R.TAIL, np.arange(r.K), r.c2))


@pytest.mark.parametrize("c", R.VQ_CASES, ids=R.case_id)
def test_vq_case_holds_its_constructed_rows(c):
    i, r = R.vq_case(c)
    dups = {lo: hi for lo, hi in R.VQ_DUPS if hi < c["K"]}
    for row, k in R.vq_exact_rows(c):
        assert r.idx[row] == k and r.dist[row, k] == 0, "a row that is a code vector is at distance exactly 0 from it"
        if k in dups:
            assert r.margin[row] == 0 and r.dist[row, dups[k]] == 0 and np.array_equal(i.cb[k], i.cb[dups[k]])
        elif c["K"] > 1:
            assert r.margin[row] > 0
    if c["K"] == 1:
        assert np.isinf(r.margin).all() and not r.idx.any()
    if c["exact"]:
        assert r.idx[c["M"] - 1] == c["K"] - 1


def test_vq_tables_cover_the_issue():
    Ms, Ds, Ks = ({c[k] for c in R.VQ_CASES} for k in "MDK")
    assert Ms == {1, 31, 32, 33, 65} and Ds == {4, 8, 64, 260} and Ks == {1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024}
    ragged = {c["K"] for c in R.VQ_CASES if c["M"] % 32}
    assert {255, 256, 257, 511, 512, 513, 1023, 1024} <= ragged
    used = {lo for c in R.VQ_CASES for _, lo in R.vq_exact_rows(c)}
    assert {lo for lo, _ in R.VQ_DUPS} <= used, "a duplicate pair that no row hits"


def _vq_bufs(r, idx=None, margin=None):
    n = np.arange(r.M)
    return R.filled(r.M + R.TAIL, n, r.idx if idx is None else idx), R.filled(r.M + R.TAIL, n, r.margin if margin is None else margin)


def test_vq_mutants_are_rejected():
    by = {c["name"]: c for c in R.VQ_CASES}
    # the higher index at a tie
    c = by["k256_d64_m33"]
    i, r = R.vq_case(c)
    dups = dict(R.VQ_DUPS)
    idx = r.idx.copy()
    tied = [row for row, k in R.vq_exact_rows(c) if k in dups and dups[k] < c["K"]]
    assert len(tied) >= 5
    for row in tied:
        idx[row] = dups[int(r.idx[row])]
        rejects(R.check_vq, "tie", r, *_vq_bufs(r, idx=idx))
        idx[row] = r.idx[row]
    R.check_vq("tie", r, *_vq_bufs(r, idx=idx))
    # the last code ignored
    for name in ("k17_d260_m33", "k257_d64_m33", "k513_d8_m65", "k1023_d64_m32", "k511_d8_m1"):
        i, r = R.vq_case(by[name])
        cut = R.vq_reference(type(i)(z=i.z, cb=i.cb[:-1]))
        rejects(R.check_vq, name, r, *_vq_bufs(r, idx=cut.idx))
        rejects(R.check_vq, name, r, *_vq_bufs(r, margin=cut.margin))
    # the last ragged row block left unwritten
    for name in ("k1024_d8_m33", "k255_d8_m65", "k15_d4_m31"):
        i, r = R.vq_case(by[name])
        ib, mb = _vq_bufs(r)
        first = (r.M - 1) // 16 * 16
        ib2 = ib.copy()
        ib2[first:r.M] = R.I64_SENT
        rejects(R.check_vq, name, r, ib2, mb)
        mb2 = mb.copy()
        mb2[r.M - 1:r.M] = R.sent_buf(1, F32)
        rejects(R.check_vq, name, r, ib, mb2)
        ib3 = ib.copy()
        ib3[r.M] = 0                                                         # a row past M written
        rejects(R.check_vq, name, r, ib3, mb)
    # vq_prepare: the codebook copied, not transposed; c2 rounded from an fp32 sum
    i, r = R.vq_case(by["k17_d260_m33"])
    n = r.D * r.K
    rejects(R.check_vq_prepare, "copy", r, R.filled(n + R.TAIL, np.arange(n), i.cb), R.filled(r.K + R.TAIL, np.arange(r.K), r.c2))
    c2_32 = (i.cb * i.cb).sum(1, dtype=F32)
    assert (c2_32 != r.c2).any()
    rejects(R.check_vq_prepare, "c2", r, R.filled(n + R.TAIL, np.arange(n), r.cbt), R.filled(r.K + R.TAIL, np.arange(r.K), c2_32))


# ------------------------------------------------------------------------------------------------ mage_argmax
@pytest.mark.parametrize("c", R.ARGMAX_CASES, ids=R.case_id)
def test_argmax_reference_agrees_with_torch(c):
    z = R.argmax_inputs(c)
    r = R.argmax_reference(c, z)
    irow, _ = R.argmax_maps(c)
    rows = torch.from_numpy(z[irow][:, :c["K"]])
    some = ~torch.isnan(rows).all(1)
    val, idx = torch.max(torch.where(torch.isnan(rows), torch.tensor(-np.inf), rows).double(), 1)
    clear = some.numpy() & ~(r.margin == 0) & ~np.isnan(r.margin)
    assert np.array_equal(idx.numpy()[clear], r.idx[clear])
    got = rows.numpy()[np.arange(c["rows"]), np.minimum(r.idx, c["K"] - 1)]
    assert np.array_equal(got[some.numpy()].astype(F64), val.numpy()[some.numpy()])
    for j, pat in enumerate(c["pat"]):
        v = rows.numpy()[j]
        if pat == "all_nan":
            assert r.idx[j] == R.NO_CODE == 0x7fffffff and np.isnan(r.margin[j])
        elif pat in ("tie_lanes", "tie_sweeps", "tie_hi_lane", "zeros", "zeros_pm"):
            assert r.margin[j] == 0 and (v == v[r.idx[j]]).sum() >= 2 and r.idx[j] == np.flatnonzero(v == v[r.idx[j]])[0]
            assert bool(np.signbit(r.margin[j])) == (pat == "zeros"), "one IEEE subtraction: (-0) - (+0) = -0, every other tie +0"
        elif pat in ("one", "inf1"):
            assert np.isposinf(r.margin[j])
        elif pat in ("inf2", "ninf"):
            assert np.isnan(r.margin[j]) and r.idx[j] == (1 if pat == "inf2" else 0)
        elif pat == "last":
            assert r.idx[j] == c["K"] - 1
        elif pat == "nan_max":
            assert np.isnan(v[0]) and np.isnan(v).sum() == 2 and r.idx[j] > 0
    R.check_argmax(c["name"], r, R.filled(r.out_size, r.orow, r.idx), R.filled(r.margin_size, np.arange(c["rows"]), r.margin))


def test_argmax_tables_cover_the_issue():
    assert {c["K"] for c in R.ARGMAX_CASES} == {4, 8, 252, 256, 260, 512, 516, 4096, 8192}
    assert {c["rows"] for c in R.ARGMAX_CASES} == {1, 3, 4, 5}
    assert any(c["ld"] > c["K"] for c in R.ARGMAX_CASES) and any(c["ld"] == c["K"] for c in R.ARGMAX_CASES)
    assert any(c["group"] < c["rows"] and c["in_stride"] > c["group"] and c["out_stride"] > c["group"] for c in R.ARGMAX_CASES)
    assert {p for c in R.ARGMAX_CASES for p in c["pat"]} >= {"tie_lanes", "tie_sweeps", "tie_hi_lane", "zeros", "zeros_pm", "nan_max", "all_nan", "inf1",
                                                             "inf2", "ninf", "one", "last"}


def test_argmax_mutants_are_rejected():
    by = {c["name"]: c for c in R.ARGMAX_CASES}
    for name in ("k8_r3", "k512_r5_grouped", "k8192_r4"):                  # a NaN logit chosen
        c = by[name]
        z = R.argmax_inputs(c)
        r = R.argmax_reference(c, z)
        j = c["pat"].index("nan_max")
        irow, _ = R.argmax_maps(c)
        idx = r.idx.copy()
        idx[j] = int(np.flatnonzero(np.isnan(z[irow[j], :c["K"]]))[-1])
        rejects(R.check_argmax, name, r, R.filled(r.out_size, r.orow, idx))
    for name in ("k4_r5", "k252_r4_grouped", "k516_r4", "k4096_r3_grouped"):    # a gap column read as a code
        c = by[name]
        z = R.argmax_inputs(c)
        r = R.argmax_reference(c, z)
        wide = R.argmax_reference(c, z, K=c["K"] + 4)
        assert (wide.idx >= c["K"]).sum() >= c["rows"] - 1                  # (a row that holds +inf itself keeps its pick)
        rejects(R.check_argmax, name, r, R.filled(r.out_size, r.orow, wide.idx))
    c = by["k512_r5_grouped"]
    z = R.argmax_inputs(c)
    r = R.argmax_reference(c, z)
    m = R.filled(r.margin_size, np.arange(c["rows"]), r.margin)
    rejects(R.check_argmax, "packed", r, R.filled(r.out_size, np.arange(c["rows"]), r.idx), m)          # the output map ignored
    flat = dict(c, in_stride=c["group"], in_off=0)
    rejects(R.check_argmax, "in map", r, R.filled(r.out_size, r.orow, R.argmax_reference(flat, z).idx), m)   # the input map ignored
    for name, pat in (("k260_r3", "tie_sweeps"), ("k260_r3", "tie_hi_lane"), ("k4_r5", "zeros")):  # the later of two maxima
        c = by[name]
        z = R.argmax_inputs(c)
        r = R.argmax_reference(c, z)
        j = c["pat"].index(pat)
        v = z[R.argmax_maps(c)[0][j], :c["K"]]
        idx = r.idx.copy()
        idx[j] = int(np.flatnonzero(v == v[r.idx[j]])[-1])
        assert idx[j] != r.idx[j]
        rejects(R.check_argmax, name, r, R.filled(r.out_size, r.orow, idx))


# ------------------------------------------------------------------------------------------------ mage_cross_entropy
def ce_emulation(z, tg, skip_tail=False):
    """ce_rows_kernel in numpy fp32: lane l adds its terms 64 apart in order, an xor butterfly joins the lanes."""
    rows, K = z.shape
    out = np.empty(rows, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(rows):
            p = z[r]
            mx = p.max()
            lanes = np.zeros(64, F32)
            for k in range(K - (K % 64 if skip_tail else 0)):
                lanes[k % 64] = lanes[k % 64] + np.exp(F32(p[k] - mx), dtype=F32)
            for o in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[np.arange(64) ^ o]
            out[r] = F32(F32(np.log(lanes[0], dtype=F32) + mx) - p[tg[r]])
    return out


@pytest.mark.parametrize("c", R.CE_CASES, ids=R.case_id)
def test_cross_entropy_reference_agrees_with_torch_and_bounds_the_emulation(c):
    z, tg = R.ce_inputs(c)
    loss, bound = R.ce_reference(z, tg)
    fin = np.isfinite(z).any(1) & np.isfinite(z[np.arange(c["rows"]), tg])
    want = F.cross_entropy(torch.from_numpy(z[fin]).double(), torch.from_numpy(tg[fin]), reduction="none").numpy()
    assert np.allclose(loss[fin], want, rtol=1e-12, atol=1e-10)
    assert (bound[fin] > 0).all() and (bound[fin] < 64 * R.U * (np.abs(z[fin]).max() + 16)).all(), "the bound is a few fp32 roundings of the operands"
    if c["ninf"]:
        assert fin.tolist() == [True, False, False, True] + [True] * (c["rows"] - 4)
        assert np.isposinf(loss[1]) and np.isnan(loss[2]) and loss[3] == 0
    sub = np.arange(c["rows"]) if c["rows"] <= 8 else np.array([0, 1, c["rows"] - 1])
    emu = ce_emulation(z[sub], tg[sub])
    rows = R.filled(sub.size + R.TAIL, np.arange(sub.size), emu)
    m, b = R.ce_mean(emu, sub.size)
    R.check_ce(c["name"], z[sub], tg[sub], rows, R.filled(1 + R.TAIL, np.arange(1), np.array([m], F32)))
    if fin[sub].all():
        off = R.filled(1 + R.TAIL, np.arange(1), np.array([m + F32(3 * b)], F32))
        rejects(R.check_ce, "mean 3 ulp off", z[sub], tg[sub], rows, off)


def test_cross_entropy_tables_and_mutants():
    assert {c["K"] for c in R.CE_CASES} == {1, 3, 63, 64, 65, 512, 1000} and {c["rows"] for c in R.CE_CASES} == {1, 3, 4, 5, 1023, 1024, 1025}
    assert {c["offset"] for c in R.CE_CASES} == {0.0, 1e4, -1e4}
    by = {c["name"]: c for c in R.CE_CASES}
    for name in ("r4_k63", "r4_k1000_minus1e4"):                             # the ragged last sweep of a row dropped
        z, tg = R.ce_inputs(by[name])
        emu = ce_emulation(z, tg, skip_tail=True)
        m, _ = R.ce_mean(emu, emu.size)
        rejects(R.check_ce, name, z, tg, R.filled(emu.size + R.TAIL, np.arange(emu.size), emu), R.filled(1 + R.TAIL, np.arange(1), np.array([m], F32)))
    z, tg = R.ce_inputs(by["r1025_k64"])                                     # the mean over the first 1024 rows only
    loss, _ = R.ce_reference(z, tg)
    l32 = loss.astype(F32)
    short = F32(l32[:1024].astype(F64).sum() / 1025)
    rejects(R.check_ce, "short mean", z, tg, R.filled(1025 + R.TAIL, np.arange(1025), l32), R.filled(1 + R.TAIL, np.arange(1), np.array([short], F32)))
    z, tg = R.ce_inputs(by["r5_k65_ninf"])                                   # a NaN row reported as a number, an infinite one as a large number
    loss, _ = R.ce_reference(z, tg)
    for row, v in ((2, 0.0), (1, 3.0e38)):
        l32 = loss.astype(F32)
        l32[row] = v
        m, _ = R.ce_mean(l32, 5)
        rejects(R.check_ce, "non-finite", z, tg, R.filled(5 + R.TAIL, np.arange(5), l32), R.filled(1 + R.TAIL, np.arange(1), np.array([m], F32)))


# ------------------------------------------------------------------------------------------------ mage_caption_mask
@pytest.mark.parametrize("c", R.CAPTION_CASES, ids=R.case_id)
def test_caption_reference_and_prefix_mutant(c):
    ids = R.caption_inputs(c)
    keep, kv = R.caption_reference(ids, c["pad"])
    t = torch.from_numpy(ids) != c["pad"]
    assert np.array_equal(keep, t.float().reshape(-1).numpy()) and np.array_equal(kv, t.sum(1).to(torch.int32).numpy())
    kb, vb = R.filled(keep.size + R.TAIL, np.arange(keep.size), keep), R.filled(kv.size + R.TAIL, np.arange(kv.size), kv)
    R.check_caption(c["name"], c, ids, kb, vb)
    prefix = np.array([int(np.flatnonzero(row == c["pad"])[0]) if (row == c["pad"]).any() else c["S"] for row in ids], np.int32)
    if "middle" in c["pats"] and c["S"] > 1:                                 # kv_len counted as a prefix length
        assert (prefix != kv).any()
        rejects(R.check_caption, c["name"], c, ids, kb, R.filled(kv.size + R.TAIL, np.arange(kv.size), prefix))
    if c["pad"]:                                                             # the padding id taken for 0
        rejects(R.check_caption, c["name"], c, ids, R.filled(keep.size + R.TAIL, np.arange(keep.size), (ids != 0).astype(F32)), vb)


def test_caption_tables_cover_the_issue():
    assert {c["S"] for c in R.CAPTION_CASES} == {1, 63, 64, 65, 130} and {c["B"] for c in R.CAPTION_CASES} == {1, 3}
    assert {c["pad"] for c in R.CAPTION_CASES} == {0, 7} and {c["outs"] for c in R.CAPTION_CASES} == {"both", "kv_len", "keep"}
    assert {p for c in R.CAPTION_CASES for p in c["pats"]} == {"none", "tail", "middle", "all"}


# ------------------------------------------------------------------------------------------------ mage_row_affine
@pytest.mark.parametrize("c", R.ROW_AFFINE_CASES, ids=R.case_id)
def test_row_affine_bound_allows_fused_and_unfused(c):
    i = R.row_affine_inputs(c)
    y, b = R.row_affine_reference(c, i)
    x, rs, tab = torch.from_numpy(i.x), None if i.rs is None else torch.from_numpy(i.rs), None if i.table is None else torch.from_numpy(i.table)
    trow = (torch.arange(c["rows"]) // c["div"]) % c["mod"]
    want = x.double() * (rs.double()[:, None] if rs is not None else 1.0) + (tab.double()[trow] if tab is not None else 0.0)
    assert np.array_equal(y, want.numpy())
    unfused = x * rs[:, None] if rs is not None else x
    unfused = unfused + tab[trow] if tab is not None else unfused
    fused = want.float()                                                    # one rounding of the exact value
    n = y.size
    for got in (unfused, fused):
        assert R.check_out(c["name"], R.filled(n + R.TAIL, np.arange(n), got.numpy()), np.arange(n), y, b) <= 1.0
    if tab is not None and c["mod"] > 1 and c["rows"] > c["div"] * c["mod"]:    # the table row clamped instead of wrapped
        clamped = unfused - tab[trow] + tab[torch.clamp(torch.arange(c["rows"]) // c["div"], max=c["mod"] - 1)]
        rejects(R.check_out, c["name"], R.filled(n + R.TAIL, np.arange(n), clamped.numpy()), np.arange(n), y, b)
    if rs is not None:                                                      # a row's scale taken from its neighbour
        shifted = x * torch.roll(rs, 1)[:, None] + (tab[trow] if tab is not None else 0.0)
        rejects(R.check_out, c["name"], R.filled(n + R.TAIL, np.arange(n), shifted.numpy()), np.arange(n), y, b)


def test_row_affine_tables_cover_the_issue():
    assert {c["C"] for c in R.ROW_AFFINE_CASES} == {4, 260}
    assert {(c["rs"], c["table"]) for c in R.ROW_AFFINE_CASES} == {(True, True), (True, False), (False, True)}
    threads = {c["rows"] * c["C"] // 4 for c in R.ROW_AFFINE_CASES}
    assert {255, 256, 257} <= threads and any(t < 256 for t in threads) and any(t > 256 for t in threads)
    assert any(c["table"] and c["rows"] > c["div"] * c["mod"] > c["div"] for c in R.ROW_AFFINE_CASES)


# ------------------------------------------------------------------------------------------------ the checker itself
def test_check_out_sees_the_sentinels():
    want = np.array([1.0, np.inf, np.nan, -0.0], F32)
    idx = np.array([0, 2, 3, 5])
    good = R.filled(8, idx, want)
    assert R.check_out("ok", good, idx, want) == 0.0
    for pos, v in ((1, 0.0), (7, 1.0)):                                      # a gap, the slack
        bad = good.copy()
        bad[pos] = v
        rejects(R.check_out, "outside", bad, idx, want)
    bad = good.copy()
    bad[2:3] = R.sent_buf(1, F32)
    rejects(R.check_out, "unwritten", bad, idx, want)
    bad = good.copy()
    bad[5] = 0.0                                                             # +0 for -0
    rejects(R.check_out, "sign of zero", bad, idx, want)
    bad[5], bad[3] = -0.0, 1.0                                               # a number for a NaN
    rejects(R.check_out, "nan", bad, idx, want)
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.99999) == 2.0 ** -24 and R.ulp32(3e38) == 2.0 ** 104 and R.ulp32(0.0) == 2.0 ** -149
