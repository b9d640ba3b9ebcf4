"""GPU: every kernel behind mage_attention_bwd (csrc/attention_bwd.hip) against the fp64 restatement of tests/attention_bwd_ref.py (formulas
and the derivation of the per-element bounds are in that module's docstring), at the edges of its dispatch.

Which kernel a descriptor reaches, and the cases that reach it:
  attention_bwd_kernel<float>            fp32 (F32_CASES):
                                         f32_nk1 (nk = 1); f32_nk64_nq31 (nk = 64, the last nq under the LDS limit; causal nq < nk; kv_len
                                         'edge'; 5 heads); f32_nq100_nk30 (two query blocks, the last one ragged; the last nk under the LDS
                                         limit for nq >= 64; 9 heads; spread 2; kv_len 'edge0' / div 3); f32_nq256_nk12 (four query blocks;
                                         scale 1.0; 1 head); f32_axial_nk16 (axial buffers, inner 4, causal, kv_len 'edge0' / div 3, 5 heads);
                                         f32_nq8_nk20 (causal nq < nk, inner 2, kv_len 'edge' / div 1); f32_causal_nq20_nk15 (causal nq > nk:
                                         queries 0..4 see no key); f32_axial_edge_div3 (kv_len 'edge' / div 3, inner 3);
                                         f32_drop_kvlen, f32_drop_nq70 (drop_p > 0 with kv_len; one and two query blocks);
                                         f32_drop_edge0 (drop_p > 0, kv_len 'edge0' / div 1: dropout over a sequence with kv_len 0),
                                         f32_drop_causal_nq15_nk14 (drop_p > 0 with one query that sees no key)
  attention_bwd_kernel<unsigned short>   bf16 with nq or nk > 32 (TPQ_CASES): bf16_nk33 (axial, causal), bf16_nq40_nk20 (kv_len 'edge0'),
                                         bf16_nk64_nq8 (causal nq < nk); bf16 with nq, nk <= 32 and a misaligned operand: bf16_mis_ld (ldk 4
                                         elements off a multiple of 8), bf16_mis_base (q 8 bytes off); and every MFMA_CASES case once more
                                         under option attn_no_mfma
  attention_bwd_mfma_kernel<1>           bf16, nq <= 32, nk <= 16 (MFMA_CASES m1_*): nq 1, 2, 15, 16, 17, 31, 32; heads 1, 3, 4, 5, 16, 17;
                                         causal nq < nk (m1_nq1_nk16_h1), nq == nk (m1_nq15_nk15_h4, axial, inner 3), nq > nk
                                         (m1_nq17_nk16_h16: query 0 sees no key); kv_len 'edge0' / div 3 (m1_nq2_nk9_h3); spread 2
                                         (m1_nq31_nk7_h17); axial inner 4 (m1_nq16_nk16_h5); nk = 1 (m1_nq32_nk1_h1)
  attention_bwd_mfma_kernel<2>           bf16, nq <= 32, nk 17..32 (MFMA_CASES m2_*): nq 1, 2, 15, 16, 17, 31, 32; heads 1, 3, 4, 5, 16, 17;
                                         causal nq < nk (m2_nq2_nk32_h17; m2_nq15_nk31_h5 with kv_len 'edge0' / div 3), nq == nk
                                         (m2_nq17_nk17_h16, m2_nq32_nk32_h5: axial; scale 1.0), nq > nk (m2_nq32_nk20_h3); kv_len 'edge0' / div 3
                                         on axial buffers with inner 3 (m2_nq31_nk31_h1); spread 2 with inner 2 (m2_nq16_nk17_h4)
The dispatch has no kernel-name query: every MFMA_CASES case runs twice, once as dispatched and once under attn_no_mfma, and both runs must
meet the bound of their own family (the thread-per-query one has no hi + lo term).

Every case: dq, dk, dv start filled with the NaN sentinel of their dtype, in buffers wider than 32 n_head (separate buffers: ld_dq, ld_dk,
ld_dv all different; axial: one [rows, 3 C + 8] buffer, as the model packs them) with 3 rows past the last mapped one.  Every element
outside the mapped rows and columns must still hold the sentinel and every mapped element must have been written; every live element is
within its bound; dq of a query that sees no key and dk, dv of every key of its (sequence, head) are NaN (the contract of
include/mage_hip.h); keys no query sees have dk == 0 and dv == 0 exactly."""
import ctypes as C

import pytest
import torch

from mage_amd import _lib, config, ops
from tests import attention_bwd_ref as R
from tests.attention_bwd_ref import bwd_case as case
from tests.helpers import SENTINEL, attn_geometry, attn_lens, attn_row_maps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

F32_CASES = [
    case("f32_nk1", "f32", 3, 1, 1, 2),
    case("f32_nk64_nq31", "f32", 31, 64, 5, 6, causal=True, lens="edge"),               # 162 752 of 163 840 bytes of LDS
    case("f32_nq100_nk30", "f32", 100, 30, 9, 18, spread=2, lens="edge0", div=3),      # 161 792 bytes of LDS
    case("f32_nq256_nk12", "f32", 256, 12, 1, 3, scale=1.0),
    case("f32_axial_nk16", "f32", 16, 16, 5, 24, inner=4, causal=True, geo="axial", lens="edge0", div=3),
    case("f32_nq8_nk20", "f32", 8, 20, 2, 6, inner=2, causal=True, lens="edge"),
    case("f32_causal_nq20_nk15", "f32", 20, 15, 2, 3, causal=True),
    case("f32_axial_edge_div3", "f32", 12, 12, 3, 15, inner=3, geo="axial", lens="edge", div=3),
    case("f32_drop_kvlen", "f32", 12, 12, 2, 6, geo="axial", lens="edge", drop=0.1, seed=0x9E3779B97F4A7C15),
    case("f32_drop_nq70", "f32", 70, 12, 5, 7, lens="edge", drop=0.5, seed=3),
    # dropout over queries that see no key: a dropped (i, j) of such a query is NaN * 0, still NaN in dv
    case("f32_drop_edge0", "f32", 10, 14, 3, 8, lens="edge0", drop=0.3, seed=11),
    case("f32_drop_causal_nq15_nk14", "f32", 15, 14, 2, 4, causal=True, drop=0.5, seed=5),        # one dead query per sequence
]
TPQ_CASES = [
    case("bf16_nk33", "bf16", 33, 33, 5, 7, causal=True, geo="axial"),
    case("bf16_nq40_nk20", "bf16", 40, 20, 3, 7, lens="edge0"),
    case("bf16_nk64_nq8", "bf16", 8, 64, 4, 5, causal=True),
    case("bf16_mis_ld", "bf16", 16, 16, 3, 5, causal=True, mis="ld"),
    case("bf16_mis_base", "bf16", 17, 20, 2, 5, mis="base"),
]
MFMA_CASES = [
    case("m1_nq1_nk16_h1", "bf16", 1, 16, 1, 7, causal=True),
    case("m1_nq2_nk9_h3", "bf16", 2, 9, 3, 18, lens="edge0", div=3),
    case("m1_nq15_nk15_h4", "bf16", 15, 15, 4, 6, inner=3, causal=True, geo="axial"),
    case("m1_nq16_nk16_h5", "bf16", 16, 16, 5, 8, inner=4, geo="axial"),
    case("m1_nq17_nk16_h16", "bf16", 17, 16, 16, 3, causal=True),                       # causal nq > nk: query 0 sees no key
    case("m1_nq31_nk7_h17", "bf16", 31, 7, 17, 4, spread=2),
    case("m1_nq32_nk1_h1", "bf16", 32, 1, 1, 3),
    case("m2_nq1_nk17_h3", "bf16", 1, 17, 3, 7),
    case("m2_nq2_nk32_h17", "bf16", 2, 32, 17, 5, causal=True),
    case("m2_nq15_nk31_h5", "bf16", 15, 31, 5, 18, causal=True, lens="edge0", div=3),
    case("m2_nq16_nk17_h4", "bf16", 16, 17, 4, 6, inner=2, spread=2),
    case("m2_nq17_nk17_h16", "bf16", 17, 17, 16, 4, causal=True, geo="axial"),
    case("m2_nq31_nk31_h1", "bf16", 31, 31, 1, 18, inner=3, geo="axial", lens="edge0", div=3),
    case("m2_nq32_nk32_h5", "bf16", 32, 32, 5, 4, inner=2, causal=True, geo="axial", scale=1.0),
    case("m2_nq32_nk20_h3", "bf16", 32, 20, 3, 3, causal=True),                         # causal nq > nk: queries 0..11 see no key
]


def family(c, no_mfma=False):
    if c["kind"] == "f32":
        return "f32"
    return "bf16_mfma" if c["nq"] <= 32 and c["nk"] <= 32 and not c["mis"] and not no_mfma else "bf16_tpq"


def _sentinel_full(rows, cols, dt):
    it, val = SENTINEL[dt]
    return torch.full((rows, cols), val, dtype=it, device=DEV).view(dt)


def launch(c, seed=0):
    """Builds the buffers of case c and runs mage_attention_bwd once.  Returns the gradient buffers on the CPU as
    {name: (buffer index, column offset)} + the list of buffers, the fp64 values of the inputs, the geometry, lens and scale."""
    dt = DTYPES[c["kind"]]
    H, Cc = c["H"], 32 * c["H"]
    g, q_rows, kv_rows, _ = attn_geometry(c)
    gen = torch.Generator().manual_seed(1000 * seed + 31 * c["nq"] + 7 * c["nk"] + H)
    if c["geo"] == "axial":
        qkv = torch.randn(q_rows, 3 * Cc, generator=gen).to(dt).to(DEV)
        qd, kd, vd = qkv, qkv[:, Cc:], qkv[:, 2 * Cc:]
        ldq = ldk = ldv = 3 * Cc
        grads = [_sentinel_full(q_rows + 3, 3 * Cc + 8, dt)]
        where = {"dq": (0, 0), "dk": (0, Cc), "dv": (0, 2 * Cc)}
        lds = {n: 3 * Cc + 8 for n in where}
    else:
        ldq, ldk, ldv = Cc + 8, Cc + (28 if c["mis"] == "ld" else 24), Cc + 40
        qbuf = torch.randn(q_rows + 1, ldq, generator=gen).to(dt).to(DEV)
        qd = qbuf.view(-1)[4:4 + q_rows * ldq].view(q_rows, ldq) if c["mis"] == "base" else qbuf[:q_rows]
        kd = torch.randn(kv_rows, ldk, generator=gen).to(dt).to(DEV)
        vd = torch.randn(kv_rows, ldv, generator=gen).to(dt).to(DEV)
        lds = {"dq": Cc + 48, "dk": Cc + 56, "dv": Cc + 72}
        grads = [_sentinel_full(q_rows + 3, lds["dq"], dt), _sentinel_full(kv_rows + 3, lds["dk"], dt), _sentinel_full(kv_rows + 3, lds["dv"], dt)]
        where = {"dq": (0, 0), "dk": (1, 0), "dv": (2, 0)}
    ldo = Cc + 16
    do = torch.randn(q_rows, ldo, generator=gen).to(dt).to(DEV)
    lens = attn_lens(c) if c["lens"] else None
    scale = float(torch.tensor(32 ** -0.5 if c["scale"] is None else c["scale"], dtype=torch.float32))
    out = {n: grads[b][:, off:] for n, (b, off) in where.items()}
    ops.attention_bwd(qd, kd, vd, do, out["dq"], out["dk"], out["dv"], ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, ld_dq=lds["dq"], ld_dk=lds["dk"],
                      ld_dv=lds["dv"], n_seq=c["n_seq"], inner=c["inner"], nq=c["nq"], nk=c["nk"], n_head=H, causal=c["causal"],
                      kv_len=lens.to(DEV) if lens is not None else None, kv_len_div=c["div"], scale=scale, drop_p=c["drop"],
                      drop_seed=c["seed"], **g)
    torch.cuda.synchronize()
    inputs = tuple(t.cpu().double() for t in (qd, kd, vd, do))             # 16-bit: the rounded inputs
    return [b.cpu() for b in grads], where, inputs, g, lens, scale


def check(c, fam, grads, where, inputs, g, lens, scale):
    """The footprint, the NaN rows, the exact zeros and the bound; returns the worst |err| / bound over dq, dk, dv."""
    name, Cc = c["name"], 32 * c["H"]
    dt = DTYPES[c["kind"]]
    it, sval = SENTINEL[dt]
    qr, kr, _ = attn_row_maps(c, g)
    rows = {"dq": qr.reshape(-1), "dk": kr.reshape(-1), "dv": kr.reshape(-1)}
    inside = [torch.zeros(b.shape, dtype=torch.bool) for b in grads]
    for n, (b, off) in where.items():
        inside[b][rows[n], off:off + Cc] = True
    for b, m in zip(grads, inside):
        bits = b.view(it)
        assert bool((bits[~m] == sval).all()), f"{name}: {int((bits[~m] != sval).sum())} elements written outside the mapped rows / columns"
        assert bool((bits[m] != sval).all()), f"{name}: {int((bits[m] == sval).sum())} mapped elements left unwritten"
    r = R.reference(*inputs, c, g, lens, scale)
    bq, bk, bv = R.bounds(fam, r, c)
    worst = 0.0
    for n, ref, b, dead in (("dq", r.dq, bq, r.dead_q), ("dk", r.dk, bk, r.dead_k), ("dv", r.dv, bv, r.dead_k)):
        bi, off = where[n]
        got = grads[bi][rows[n], off:off + Cc].double()
        assert bool(torch.isnan(got[dead]).all()), f"{name} {n}: finite values where a query of the (sequence, head) sees no key"
        live = ~dead
        assert bool(torch.isfinite(got[live]).all()), f"{name} {n}: non-finite values in rows whose queries all see a key"
        if n != "dq":
            assert bool((got[r.zero_k] == 0).all()), f"{name} {n}: a key that no query sees has a nonzero gradient"
        err, bl = (got[live] - ref[live]).abs(), b[live]
        if err.numel() == 0:
            continue
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bl)      # a zero bound only with a zero reference (an unseen key)
        w = ratio.flatten().argmax().item()
        assert ratio.max().item() <= 1.0, (f"{name} {n} [{fam}]: |err| {err.flatten()[w].item():.3e} > bound {bl.flatten()[w].item():.3e} "
                                           f"(ref {ref[live].flatten()[w].item():.6e}, got {got[live].flatten()[w].item():.6e})")
        worst = max(worst, ratio.max().item())
    print(f"attention_bwd {name} [{fam}]: worst |err| / bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("c", F32_CASES + TPQ_CASES)
def test_attention_bwd_against_fp64(c):
    check(c, family(c), *launch(c))


@pytest.mark.parametrize("c", MFMA_CASES)
def test_attention_bwd_matrix_cores_and_thread_per_query_against_fp64(c):
    assert family(c) == "bf16_mfma"
    check(c, "bf16_mfma", *launch(c))
    with config.lib_option("attn_no_mfma", 1):
        check(c, "bf16_tpq", *launch(c))


# one per family (the thread-per-query bf16 kernel also through attn_no_mfma), by case id: (id, attn_no_mfma)
DETERMINISM = [("f32_nq100_nk30", False), ("f32_drop_nq70", False), ("bf16_nq40_nk20", False), ("m2_nq15_nk31_h5", True),
               ("m1_nq16_nk16_h5", False), ("m2_nq15_nk31_h5", False)]
BY_ID = {p.id: p.values[0] for p in F32_CASES + TPQ_CASES + MFMA_CASES}


@pytest.mark.parametrize("c,no_mfma", [pytest.param(BY_ID[i], n, id=i + ("_no_mfma" if n else "")) for i, n in DETERMINISM])
def test_attention_bwd_is_deterministic(c, no_mfma):
    """include/mage_hip.h: 'fixed-order sums (deterministic)': two runs on the same inputs agree bit for bit, NaN included."""
    with config.lib_option("attn_no_mfma", int(no_mfma)):
        a, b = launch(c)[0], launch(c)[0]
    it = SENTINEL[DTYPES[c["kind"]]][0]
    for x, y in zip(a, b):
        assert torch.equal(x.view(it), y.view(it)), f"{c['name']}: two runs differ"


# ------------------------------------------------------------------------------------------------ refusals
def _raw_bwd(dt, dtype_code, nq, nk, H=2, n_seq=3, inner=1, kv_outer_stride=None, drop_p=0.0, o_strides=(0, 0), refused=None):
    """mage_attention_bwd through a hand-filled descriptor, on buffers large enough for any row the call could touch.  Returns the three
    gradient buffers, sentinel-filled before the call.  refused: the call must raise ValueError matching it."""
    Cc = 32 * H
    ld = Cc + 8
    rows = n_seq * max(nq, nk) * 2 + 4
    q, k, v, do = (torch.randn(rows, ld).to(dt).to(DEV) for _ in range(4))
    grads = [_sentinel_full(rows, ld, dt) for _ in range(3)]
    l, s = ops._dev(q)
    d = _lib.AttnDesc()
    d.dtype = dtype_code
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr()
    d.ldq = d.ldk = d.ldv = d.ldo = ld
    d.n_seq, d.inner, d.nq, d.nk, d.n_head = n_seq, inner, nq, nk, H
    d.q_outer_stride, d.q_axis_stride = nq * inner, inner
    d.kv_outer_stride, d.kv_axis_stride = nk * inner if kv_outer_stride is None else kv_outer_stride, inner
    d.kv_len, d.kv_len_div, d.scale = None, 1, 32 ** -0.5
    d.drop_p, d.drop_seed = drop_p, 1
    d.o_outer_stride, d.o_axis_stride = o_strides

    def call():
        _lib.check(l.mage_attention_bwd(C.byref(d), do.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), ld, ld, ld, s), l)
    if refused is None:
        call()
    else:
        with pytest.raises(ValueError, match=refused):
            call()
    torch.cuda.synchronize()
    return [t.cpu() for t in grads]


def _refused(match, dt, *a, **kw):
    """The call is refused with MAGE_EINVAL (ValueError) and every gradient buffer still holds the sentinel."""
    it, sval = SENTINEL[dt]
    for t in _raw_bwd(dt, *a, refused=match, **kw):
        assert bool((t.view(it) == sval).all()), "a refused call wrote to a gradient buffer"


@pytest.mark.parametrize("dt,code", [(torch.float16, ops.F16), (torch.bfloat16, ops.BF16X3), (torch.float16, ops.F16X3)])
def test_attention_bwd_refuses_other_dtypes(dt, code):
    """fp32 and bf16 only: f16 and the split kinds are refused before anything launches."""
    _refused("bad dtype", dt, code, 8, 8)


def test_attention_bwd_refuses_dropout_on_bf16():
    _refused("drop_p", torch.bfloat16, ops.BF16, 8, 8, drop_p=0.1)
    _refused("drop_p", torch.bfloat16, ops.BF16, 40, 8, drop_p=0.1)


def test_attention_bwd_refuses_an_output_row_map():
    _refused("no separate output row map", torch.float32, ops.F32, 8, 8, o_strides=(16, 2))
    _refused("no separate output row map", torch.bfloat16, ops.BF16, 8, 8, o_strides=(0, 2))


@pytest.mark.parametrize("dt,code", [(torch.float32, ops.F32), (torch.bfloat16, ops.BF16)])
@pytest.mark.parametrize("nq,nk", [(32, 64), (64, 31), (100, 31), (61, 33)])
def test_attention_bwd_refuses_shapes_over_the_lds_limit(dt, code, nq, nk):
    """The thread-per-query kernel needs 16 (2 nk 32 + 2 qb 33 + 2 qb (nk + 1)) bytes of LDS, qb = min(nq, 64), of at most 163 840: the
    first refused shapes next to the last accepted ones of F32_CASES / TPQ_CASES (nq 31 at nk 64; nk 30 at nq >= 64) and of the
    accepted neighbours below."""
    qb = min(nq, 64)
    assert 16 * (2 * nk * 32 + 2 * qb * 33 + 2 * qb * (nk + 1)) > 163840
    _refused("LDS budget", dt, code, nq, nk)


@pytest.mark.parametrize("dt,code", [(torch.float32, ops.F32), (torch.bfloat16, ops.BF16)])
@pytest.mark.parametrize("nq,nk", [(31, 64), (64, 30), (60, 33)])
def test_attention_bwd_accepts_shapes_at_the_lds_limit(dt, code, nq, nk):
    """The last accepted shapes next to the refused ones above run, and write finite gradients."""
    qb = min(nq, 64)
    assert 16 * (2 * nk * 32 + 2 * qb * 33 + 2 * qb * (nk + 1)) <= 163840
    grads = _raw_bwd(dt, code, nq, nk)
    assert all(bool(torch.isfinite(t[:3 * n, :64].float()).all()) for t, n in zip(grads, (nq, nk, nk)))


@pytest.mark.parametrize("dt,code,nq,nk", [(torch.float32, ops.F32, 8, 8), (torch.bfloat16, ops.BF16, 8, 8), (torch.bfloat16, ops.BF16, 40, 8)])
def test_attention_bwd_refuses_shared_key_rows(dt, code, nq, nk):
    """kv_outer_stride 0 with n_seq > inner (the forward's kv_shared geometry): every sequence would STORE its own dk / dv to the same rows.
    Refused in front of all three kernels; n_seq <= inner (one outer block) shares nothing and runs."""
    _refused("share key rows", dt, code, nq, nk, n_seq=6, inner=2, kv_outer_stride=0)
    grads = _raw_bwd(dt, code, nq, nk, n_seq=2, inner=2, kv_outer_stride=0)
    assert bool(torch.isfinite(grads[1][:2 * nk, :64].float()).all())
