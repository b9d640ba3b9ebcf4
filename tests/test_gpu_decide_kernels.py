"""GPU: the kernels that make or score the discrete decisions -- the codebook quantiser and its caches (mage_amd/csrc/vq.hip), the row argmax and the
forward cross entropy (token_heads.hip), the caption mask and the row affine (rows.hip) -- against the numpy / fp64 references of
tests/decide_ref.py (formulas, case tables and the derivation of every bound are in that module's docstring), at the edges of their dispatch.
The C entry points are called through mage_amd._lib: mage_amd.ops allocates the outputs itself and hides ld, the row maps and the null outputs.

Which kernel a call reaches, the host predicate that sends it there, and the cases that reach it:
  vq_nearest_mfma_kernel<4, 2, 4>     test_vq_nearest[case], default options, K <= 256: K 1, 15, 16, 17, 255, 256 (4 waves x 4 tiles of 16 codes)
  vq_nearest_mfma_kernel<4, 2, 8>     256 < K <= 512: K 257 (D 64 and 260), 511, 512 (8 waves x 4 tiles)
  vq_nearest_mfma_kernel<8, 2, 8>     512 < K <= 1024: K 513, 1000, 1023, 1024 (8 waves x 8 tiles)
  vq_nearest_kernel<1 | 2 | 4>        the same cases under config.lib_option("vq_no_mfma", 1): one, two, four codes per thread at the same K steps
      every case on both kernels: M 1, 31, 32, 33, 65 (32 rows per workgroup on the matrix cores, 16 in the fallback), D 4, 8, 64, 260; rows that
      are code vectors, the last code of a ragged K, duplicate code vectors hit exactly (decide_ref.VQ_DUPS: inside a tile, across tiles, across
      waves, the lower index in the later lane), K = 1.  No case has a soft row: ids and margins are compared bit for bit with the reference,
      and between the two kernels.  The quantiser is fed the REFERENCE's codebook_t and c2
  vq_prepare_kernel                   test_vq_nearest[case] (checked before the quantiser runs): K 1 .. 1024 on both sides of its 256-thread workgroup
  argmax_kernel                       test_argmax[case]: the one instance sweeps any K % 4 == 0: K 4, 8, 252, 256, 260, 512, 516, 4096, 8192; rows 1, 3, 4, 5
                                      (four rows per workgroup); ld == K and ld > K with NaN / +inf in the gap columns; grouped input and output maps
                                      with gaps; ties across lanes and sweeps, +0 against -0, NaN at the maximum, rows of NaN, +inf, rows of -inf;
                                      mage_sample_tokens(top_k = 1) returns the same tokens where K <= 4096
  ce_rows_kernel, sum_kernel          test_cross_entropy[case]: K 1, 3, 63, 64, 65, 512, 1000 (a lane's terms are 64 apart), rows 1 .. 5 and 1023, 1024, 1025
                                      (sum_kernel's 1024 threads); logits offset by +-1e4; -inf off the target, at the target, everywhere
  caption_mask_kernel                 test_caption_mask[case]: S 1, 63, 64, 65, 130 (sweeps of 64), B 1 and 3, padding id 0 and 7, padding inside a caption,
                                      only padding, none; each output null in turn
  row_affine_kernel                   test_row_affine[case]: C 4 and 260, rows C / 4 = 195 .. 520 threads around the 256-thread workgroup, rs / table / both,
                                      (r / div) % mod wrapping

Every case: each output starts filled with a sentinel (the NaN of tests/helpers.py SENTINEL for fp32, decide_ref.I64_SENT / I32_SENT for the
integers) with slack past its end and in every gap of its map; everything outside the footprint must still hold the sentinel, everything
inside must have been written and be right: bit for bit for the quantiser, its caches, the argmax and the caption mask, within the derived
bound for the cross entropy and the row affine.  Refused calls return MAGE_EINVAL and leave the outputs untouched."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, config, ops
from tests import decide_ref as R
from tests.helpers import DEV, WORST, lib, ptr, sent, untouched

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def isent(n, dt):
    return torch.full((n,), R.I64_SENT if dt == torch.int64 else R.I32_SENT, dtype=dt, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return None if t is None else t.cpu().numpy()


def report(entry, name, worst):
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print(f"{entry} {name}: worst |err| / bound {worst:.3f} (largest so far {WORST[entry]:.3f})")


def refused(call, *outs):
    with pytest.raises(ValueError):
        call()
    torch.cuda.synchronize()
    for o in outs:
        raw = o.cpu().numpy()
        assert np.array_equal(raw, R.sent_buf(raw.size, raw.dtype)) if raw.dtype != np.float32 else untouched(o), "a refused call wrote to an output"


# ------------------------------------------------------------------------------------------------ mage_vq_prepare, mage_vq_nearest
def run_vq(z, cbt, c2, r, want_margin=True):
    l, s = lib()
    idx, margin = isent(r.M + R.TAIL, torch.int64), sent(r.M + R.TAIL, torch.float32) if want_margin else None
    _lib.check(l.mage_vq_nearest(z.data_ptr(), cbt.data_ptr(), c2.data_ptr(), r.M, r.D, r.K, idx.data_ptr(), ptr(margin), s), l)
    return host(idx), host(margin)


@pytest.mark.parametrize("c", R.VQ_CASES, ids=R.case_id)
def test_vq_nearest(c):
    i, r = R.vq_case(c)
    assert not r.soft.any()
    l, s = lib()
    cb = dev(i.cb)
    cbt_k, c2_k = sent(r.D * r.K + R.TAIL, torch.float32), sent(r.K + R.TAIL, torch.float32)
    _lib.check(l.mage_vq_prepare(cb.data_ptr(), r.K, r.D, cbt_k.data_ptr(), c2_k.data_ptr(), s), l)
    R.check_vq_prepare(c["name"], r, host(cbt_k), host(c2_k))
    z, cbt, c2 = dev(i.z), dev(r.cbt), dev(r.c2)                           # the reference's caches, not the kernel's
    idx_m, margin_m = run_vq(z, cbt, c2, r)
    R.check_vq(c["name"] + " matrix cores", r, idx_m, margin_m)
    idx_n, _ = run_vq(z, cbt, c2, r, want_margin=False)                     # margin is optional
    R.check_vq(c["name"] + " matrix cores, no margin", r, idx_n, None)
    with config.lib_option("vq_no_mfma", 1):
        idx_f, margin_f = run_vq(z, cbt, c2, r)
        idx_g, _ = run_vq(z, cbt, c2, r, want_margin=False)
    R.check_vq(c["name"] + " fallback", r, idx_f, margin_f)
    R.check_vq(c["name"] + " fallback, no margin", r, idx_g, None)
    assert np.array_equal(idx_m, idx_f) and np.array_equal(R.bits(margin_m), R.bits(margin_f)), f"{c['name']}: the two kernels differ"


# ------------------------------------------------------------------------------------------------ mage_argmax
@pytest.mark.parametrize("c", R.ARGMAX_CASES, ids=R.case_id)
def test_argmax(c):
    z = R.argmax_inputs(c)
    r = R.argmax_reference(c, z)
    l, s = lib()
    zd = dev(z)
    a = (zd.data_ptr(), c["rows"], c["K"], c["ld"], c["group"], c["in_stride"], c["in_off"])
    out, margin = isent(r.out_size, torch.int64), sent(r.margin_size, torch.float32)
    _lib.check(l.mage_argmax(*a, out.data_ptr(), c["out_stride"], c["out_off"], margin.data_ptr(), s), l)
    R.check_argmax(c["name"], r, host(out), host(margin))
    out2 = isent(r.out_size, torch.int64)
    _lib.check(l.mage_argmax(*a, out2.data_ptr(), c["out_stride"], c["out_off"], None, s), l)
    R.check_argmax(c["name"] + ", no margin", r, host(out2))
    if c["K"] <= 4096:                                                      # the sampler's greedy path: the same kernel
        seeds = torch.arange(7, 7 + c["rows"], dtype=torch.int64, device=DEV)
        for T, p in ((1.0, 1.0), (0.3, 0.5)):
            out3 = isent(r.out_size, torch.int64)
            _lib.check(l.mage_sample_tokens(*a, out3.data_ptr(), c["out_stride"], c["out_off"], seeds.data_ptr(), 3, T, 1, p, s), l)
            R.check_argmax(c["name"] + f", mage_sample_tokens(top_k=1, T={T}, top_p={p})", r, host(out3))


# ------------------------------------------------------------------------------------------------ mage_cross_entropy
@pytest.mark.parametrize("c", R.CE_CASES, ids=R.case_id)
def test_cross_entropy(c):
    z, tg = R.ce_inputs(c)
    l, s = lib()
    zd, td = dev(z), dev(tg)
    row_loss, mean = sent(c["rows"] + R.TAIL, torch.float32), sent(1 + R.TAIL, torch.float32)
    _lib.check(l.mage_cross_entropy(zd.data_ptr(), td.data_ptr(), c["rows"], c["K"], row_loss.data_ptr(), mean.data_ptr(), s), l)
    ops.check_device_errors(DEV)
    w_rows, w_mean = R.check_ce(c["name"], z, tg, host(row_loss), host(mean))
    report("mage_cross_entropy row_loss", c["name"], w_rows)
    report("mage_cross_entropy loss_mean", c["name"], w_mean)


# ------------------------------------------------------------------------------------------------ mage_caption_mask
@pytest.mark.parametrize("c", R.CAPTION_CASES, ids=R.case_id)
def test_caption_mask(c):
    ids = R.caption_inputs(c)
    l, s = lib()
    d = dev(ids)
    keep = sent(c["B"] * c["S"] + R.TAIL, torch.float32) if c["outs"] in ("both", "keep") else None
    kv = isent(c["B"] + R.TAIL, torch.int32) if c["outs"] in ("both", "kv_len") else None
    _lib.check(l.mage_caption_mask(d.data_ptr(), c["B"], c["S"], c["pad"], ptr(kv), ptr(keep), s), l)
    R.check_caption(c["name"], c, ids, host(keep), host(kv))


# ------------------------------------------------------------------------------------------------ mage_row_affine
@pytest.mark.parametrize("c", R.ROW_AFFINE_CASES, ids=R.case_id)
def test_row_affine(c):
    i = R.row_affine_inputs(c)
    y, b = R.row_affine_reference(c, i)
    l, s = lib()
    n = y.size
    x = sent(n + R.TAIL, torch.float32)                                     # in place: the inputs, then slack
    x[:n] = dev(i.x).reshape(-1)
    rs, table = dev(i.rs), dev(i.table)
    _lib.check(l.mage_row_affine(x.data_ptr(), ptr(rs), ptr(table), c["rows"], c["C"], c["div"], c["mod"], s), l)
    report("mage_row_affine", c["name"], R.check_out(c["name"], host(x), np.arange(n), y, b))


# ------------------------------------------------------------------------------------------------ refusals
def test_vq_refusals():
    l, s = lib()
    z, cbt, c2 = torch.randn(16, 1280, device=DEV), torch.randn(1280, 1028, device=DEV), torch.randn(1028, device=DEV)
    idx, margin = isent(16 + R.TAIL, torch.int64), sent(16 + R.TAIL, torch.float32)
    cbt_o, c2_o = sent(1280 * 1028, torch.float32), sent(1028, torch.float32)

    def nearest(M=16, D=8, K=16, zz=z, tt=cbt, cc=c2, ii=idx, mm=margin):
        return lambda: _lib.check(l.mage_vq_nearest(ptr(zz), ptr(tt), ptr(cc), M, D, K, ptr(ii), ptr(mm), s), l)

    def prepare(K=16, D=8, cb=cbt, tt=cbt_o, cc=c2_o):
        return lambda: _lib.check(l.mage_vq_prepare(ptr(cb), K, D, ptr(tt), ptr(cc), s), l)

    bad = (dict(D=6), dict(D=2), dict(D=0), dict(K=1025), dict(K=1028), dict(K=0), dict(M=0), dict(M=-1), dict(zz=None), dict(tt=None), dict(cc=None),
           dict(ii=None))
    for kw in bad:
        refused(nearest(**kw), idx, margin)
    with config.lib_option("vq_no_mfma", 1):
        for kw in bad + (dict(D=1280, K=1024), dict(D=1284, K=1020)):      # 16 (D + 1 + K) 4 bytes of LDS > 144 KiB
            refused(nearest(**kw), idx, margin)
    for kw in (dict(K=0), dict(D=0), dict(K=-4), dict(cb=None), dict(tt=None), dict(cc=None)):
        refused(prepare(**kw), cbt_o, c2_o)


def test_argmax_refusals():
    l, s = lib()
    z = torch.randn(8, 16, device=DEV)
    out, margin = isent(8 + R.TAIL, torch.int64), sent(8 + R.TAIL, torch.float32)

    def call(rows=4, K=8, ld=16, group=4, zp=z.data_ptr(), op=out.data_ptr()):
        return lambda: _lib.check(l.mage_argmax(zp, rows, K, ld, group, group, 0, op, group, 0, margin.data_ptr(), s), l)

    call()()                                                                # the baseline itself runs
    torch.cuda.synchronize()
    assert not (out[:4] == R.I64_SENT).any()
    out.fill_(R.I64_SENT)
    margin.copy_(sent(8 + R.TAIL, torch.float32))
    for kw in (dict(K=6), dict(K=0), dict(K=-4), dict(ld=10), dict(ld=14), dict(group=0), dict(group=-1), dict(rows=0), dict(rows=-3), dict(zp=None),
               dict(op=None),
               dict(ld=4), dict(K=16, ld=12), dict(ld=0), dict(ld=-16),                             # ld < K
               dict(zp=z.data_ptr() + 4), dict(zp=z.data_ptr() + 8), dict(zp=z.data_ptr() + 12)):    # rows that are not 16-byte aligned
        refused(call(**kw), out, margin)
    with pytest.raises(ValueError, match="ld >= K, logits 16-byte aligned"):
        call(ld=4)()
    with pytest.raises(ValueError, match="ld >= K, logits 16-byte aligned"):
        call(zp=z.data_ptr() + 4)()


def test_small_entry_point_refusals():
    l, s = lib()
    ids = torch.ones(4, 8, dtype=torch.int64, device=DEV)
    keep, kv = sent(32 + R.TAIL, torch.float32), isent(4 + R.TAIL, torch.int32)
    for a in ((ids.data_ptr(), 4, 8, 0, None, None), (None, 4, 8, 0, kv.data_ptr(), keep.data_ptr()), (ids.data_ptr(), 0, 8, 0, kv.data_ptr(), keep.data_ptr()),
              (ids.data_ptr(), 4, 0, 0, kv.data_ptr(), keep.data_ptr()), (ids.data_ptr(), -4, 8, 0, kv.data_ptr(), keep.data_ptr())):
        refused(lambda: _lib.check(l.mage_caption_mask(*a, s), l), keep, kv)
    z, tg = torch.randn(4, 8, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    row_loss, mean = sent(4 + R.TAIL, torch.float32), sent(1 + R.TAIL, torch.float32)
    for a in ((None, tg.data_ptr(), 4, 8, row_loss.data_ptr(), mean.data_ptr()), (z.data_ptr(), None, 4, 8, row_loss.data_ptr(), mean.data_ptr()),
              (z.data_ptr(), tg.data_ptr(), 4, 8, None, mean.data_ptr()), (z.data_ptr(), tg.data_ptr(), 4, 8, row_loss.data_ptr(), None),
              (z.data_ptr(), tg.data_ptr(), 0, 8, row_loss.data_ptr(), mean.data_ptr()), (z.data_ptr(), tg.data_ptr(), 4, 0, row_loss.data_ptr(), mean.data_ptr())):
        refused(lambda: _lib.check(l.mage_cross_entropy(*a, s), l), row_loss, mean)
    x = sent(64 + R.TAIL, torch.float32)
    v = torch.randn(64, device=DEV)
    for a in ((None, v.data_ptr(), v.data_ptr(), 4, 8, 1, 1), (x.data_ptr(), v.data_ptr(), v.data_ptr(), 0, 8, 1, 1), (x.data_ptr(), v.data_ptr(), v.data_ptr(), 4, 6, 1, 1),
              (x.data_ptr(), v.data_ptr(), v.data_ptr(), 4, 0, 1, 1), (x.data_ptr(), v.data_ptr(), v.data_ptr(), 4, 8, 0, 1),
              (x.data_ptr(), v.data_ptr(), v.data_ptr(), 4, 8, 1, 0), (x.data_ptr(), None, v.data_ptr(), 4, 8, -1, 1)):
        refused(lambda: _lib.check(l.mage_row_affine(*a, s), l), x)
