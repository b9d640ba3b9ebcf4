"""GPU: every kernel behind mage_attention (csrc/attention.hip) against an fp64 restatement of the descriptor contract
(include/mage_hip.h, mage_attn_desc), at the edges of its dispatch (attn_launch, attn_split_launch and attn_mfma_launch beneath both).

Which kernel a descriptor reaches, and the cases of CASES / test_fewq_bit_identical_to_the_workgroup_kernel that reach it:
  attention_kernel<float, 16 | 32 | 64>                fp32: f32_nk1, f32_nk15_nq16, f32_axial_nk16 | f32_axial_nk17, f32_nk31_hg3, f32_nk32 |
                                                       f32_axial_nk33_hg4, f32_nk64_hg4, f32_nk64_kvshared.  K,V head groups (hg < n_head,
                                                       grid.y > 1) once nk*hg*32*2*sizeof(T) > 64 KiB: halved while even
                                                       (f32_axial_nk33_hg4, f32_nk64_hg4), an odd count by its largest divisor that fits
                                                       (f32_nk31_hg3, f16_nk64_h9_hg3: 9 heads)
  attention_kernel<float, NK, split_bf16 | split_f16>  fp32 q/k/v, out_split: outsplit_* (NK 16, 32, 64 for each kind; hg < n_head in
                                                       outsplit_f16x3_nk31, outsplit_f16x3_nk33)
  attention_kernel<bf16 | f16, 16 | 32 | 64>           16-bit with nq or nk > 32 (or option attn_no_mfma): bf16_nq33_nk15 (16), f16_nq33_nk32
                                                       (32), bf16_axial_nk33, f16_nk64_hg8, f16_nk64_h9_hg3,
                                                       bf16_nk64 (64); through attn_no_mfma in
                                                       test_fewq_bit_identical_to_the_workgroup_kernel: bf16 16 and 32, f16 16 and 32
  attention_mfma_kernel<NKB, MAXH, Ops>                nq, nk, n_head <= 32: NKB = 1 for nk <= 16, else 2; MAXH = 2 for n_head <= 8, 4 for
                                                       9..16, 8 for 17..32.  Ops = the operand policy (csrc/attn_mfma.h):
    Ops = attn_ops_plain<bf16 | f16>                   16-bit q/k/v: mfma_<dtype>_nkb<NKB>_h<n_head>.  n_head = 32 with nk > 16
                                                       (mfma_*_nkb2_h32) stages 66 560 bytes of V in LDS, above 64 KiB: the launcher
                                                       raises the kernel's dynamic LDS limit for such a launch, in either policy
    Ops = attn_ops_f16x3                               f16x3 q/k/v: split_nkb<NKB>_h<n_head>
  attention_mfma_fewq_kernel<NKB, bf16 | f16>          16-bit as above with nq <= 2 and n_seq >= 1024 (the incremental step): fewq_*
  attention_mfma_split_fewq_kernel<NKB>                f16x3, nq <= 2, n_seq >= 1024: split_fewq_*

Rows that see no key (kv_len = 0, or a causal query i < nq - nk): every kernel computes NaN there (its probabilities are all 0, the
output is 0 * (1 / 0)), as torch's softmax over an all -inf row gives, and every fp32, bf16, f16 and bf16x3 output stores it.  f16x3
outputs (out_split F16X3 from fp32, and the split kernels) do not: their store clamps to the f16 range with v_med3_f32 (common.h
split_pack2), which turns NaN into -65504, so such a row reads -65504 (hi -65504, lo 0).  check() pins both (the cases with kv_len
pattern 'edge0' and the causal nq > nk ones reach every kernel family).

Bounds, per output element, u = 2^-24, W = sum_j p_j |v_j| (p the exact probabilities), Smax = max over visible keys of
|scale| * sum_d |q_d| |k_jd|, nk the key count:
  fp32 arithmetic:  |err| <= c u W,  c = 72 Smax + 3 nk + 6.
    A score s_j is a 32-term fp32 dot product scaled once: |ds_j| <= (32 + 2) u Smax.  exp(s_j - m) adds the rounding of the subtraction
    (<= u |s_j - m| <= 2 u Smax: m cancels in the ratio whatever its own error) and expf's own (<= 2 u): relative errors e_j <= 36 u Smax
    + 2 u in the weights p_j, which move o = sum p_j v_j / sum p_j by at most 2 max|e_j| W.  The numerator sums at most 2 nk terms (the
    matrix-core kernels accumulate P = hi + lo as two products), the denominator nk positive terms (nk u |o| <= nk u W), then one
    reciprocal and one multiply (2 u W): c = 2 (36 Smax + 2) + 2 nk + nk + 2.
  bf16 / f16 out:   the fp32 term, the P = hi + lo split of the matrix-core kernels (attn_p_split) -- bf16: two 8-bit truncations,
                    |dp| < 2^-15 p; f16: two roundings, |dp| <= 2^-22 p + 2^-25 (the subnormal grid; sum p >= 1, so <= 2^-25 sum_j |v_j|) --
                    and the rounding of the output: 1 ulp of the output type at |ref|.
  out_split:        the fp32 term and the split representation of the output (tests/test_gpu_split.py: 2^-17 |ref| for bf16x3, 2^-21 |ref|
                    + 2^-35 for f16x3).
  f16x3 q/k/v:      the fp32 term, the dropped lo * lo products of Q K^T (2^-22 |q||k|: 8 u Smax W more) and of V^T P^T (2^-22 W), the f16
                    P split with the lo piece scaled by 2^11 (2^-22 W + 2^-36 sum |v|), and the f16x3 output representation as above.

Every output buffer starts filled with a NaN sentinel of its own bit pattern, with ldo wider than the heads and gaps between the mapped rows:
every element outside the mapped rows and columns must still hold the sentinel; every element inside must have been written."""
import pytest
import torch

from mage_amd import config, ops
from tests.helpers import SENTINEL, unsplit
from tests.helpers import attn_case as case, attn_geometry as _geometry, attn_lens as _lens, attn_row_maps as _row_maps, ulp as _ulp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
# kind -> (input dtype on the device, output dtype, out_split kind, split q/k/v)
KINDS = {"f32": (torch.float32, torch.float32, 0, False), "bf16": (torch.bfloat16, torch.bfloat16, 0, False),
         "f16": (torch.float16, torch.float16, 0, False), "f32>bf16x3": (torch.float32, torch.bfloat16, ops.BF16X3, False),
         "f32>f16x3": (torch.float32, torch.float16, ops.F16X3, False), "f16x3": (torch.float32, torch.float16, ops.F16X3, True)}


CASES = [
    # attention_kernel<float, 16 | 32 | 64>
    case("f32_nk1", "f32", 1, 1, 1, 1),
    case("f32_nk15_nq16", "f32", 16, 15, 3, 7, causal=True),                          # causal nq > nk: query 0 sees no key
    case("f32_axial_nk16", "f32", 16, 16, 2, 24, inner=4, causal=True, geo="axial", lens="edge0", div=3),
    case("f32_axial_nk17", "f32", 17, 17, 5, 7, inner=3, geo="axial"),
    case("f32_nk31_hg3", "f32", 3, 31, 9, 7, causal=True, lens="edge", omap=True, spread=2),  # 9 heads: hg = 3, grid.y = 3
    case("f32_nk32", "f32", 32, 32, 8, 5, scale=1.0),                                  # K,V of all 8 heads: exactly 64 KiB
    case("f32_axial_nk33_hg4", "f32", 33, 33, 16, 3, geo="axial"),                     # hg = 4: grid.y = 4
    case("f32_nk64_hg4", "f32", 16, 64, 8, 7, causal=True, lens="edge0", div=3, omap=True),   # hg = 4: grid.y = 2
    case("f32_nk64_kvshared", "f32", 1, 64, 1, 1025, inner=5, kv_shared=True),
    # attention_kernel<float, NK, split_bf16 | split_f16>
    case("outsplit_bf16x3_nk16", "f32>bf16x3", 16, 16, 2, 7, causal=True, geo="axial"),
    case("outsplit_f16x3_nk1", "f32>f16x3", 2, 1, 4, 7, lens="edge0"),
    case("outsplit_bf16x3_nk32", "f32>bf16x3", 3, 32, 8, 7, causal=True, lens="edge0", omap=True),
    case("outsplit_f16x3_nk31", "f32>f16x3", 31, 31, 16, 4),                          # hg = 8: grid.y = 2
    case("outsplit_bf16x3_nk64", "f32>bf16x3", 64, 64, 2, 3, causal=True),
    case("outsplit_f16x3_nk33", "f32>f16x3", 2, 33, 24, 7, lens="edge", div=3),       # hg = 6: grid.y = 4
    # attention_kernel<bf16 | f16, 16 | 32 | 64>
    case("bf16_axial_nk33", "bf16", 33, 33, 5, 7, causal=True, geo="axial"),
    case("f16_nk64_hg8", "f16", 16, 64, 16, 5, lens="edge0", omap=True),               # hg = 8: grid.y = 2
    case("f16_nk64_h9_hg3", "f16", 2, 64, 9, 5, causal=True, lens="edge0"),          # hg = 3: grid.y = 3
    case("bf16_nk64", "bf16", 64, 64, 2, 3, causal=True, lens="edge0"),
    case("bf16_nq33_nk15", "bf16", 33, 15, 3, 7),
    case("f16_nq33_nk32", "f16", 33, 32, 1, 7, causal=True),                          # causal nq > nk: query 0 sees no key
    # attention_mfma_kernel<NKB, MAXH, attn_ops_plain<bf16 | f16>>
    case("mfma_bf16_nkb1_h1", "bf16", 16, 16, 1, 7, causal=True),
    case("mfma_f16_nkb1_h3", "f16", 1, 1, 3, 7),
    case("mfma_bf16_nkb2_h8", "bf16", 3, 17, 8, 9, causal=True, lens="edge0", div=3),
    case("mfma_f16_nkb2_h5", "f16", 32, 32, 5, 8, inner=4, causal=True, geo="axial"),
    case("mfma_bf16_nkb1_h9", "bf16", 2, 15, 9, 1023, inner=31, causal=True),          # nq <= 2 but n_seq 1023: not the fewq kernel
    case("mfma_f16_nkb1_h16", "f16", 16, 16, 16, 6, lens="edge", omap=True, spread=2),
    case("mfma_bf16_nkb2_h16", "bf16", 31, 31, 16, 5, lens="edge0", div=3, scale=1.0),
    case("mfma_f16_nkb2_h9", "f16", 1, 17, 9, 1023, causal=True),
    case("mfma_bf16_nkb1_h17", "bf16", 3, 16, 17, 7, causal=True),
    case("mfma_f16_nkb1_h32", "f16", 16, 15, 32, 5, causal=True),                      # causal nq > nk: query 0 sees no key
    case("mfma_bf16_nkb2_h32", "bf16", 32, 32, 32, 4, causal=True, geo="axial"),       # 66 560 bytes of dynamic LDS
    case("mfma_f16_nkb2_h32", "f16", 17, 17, 32, 4, lens="edge0"),                     # 66 560 bytes of dynamic LDS
    case("mfma_f16_nkb2_h24", "f16", 2, 31, 24, 7, causal=True, omap=True),
    # attention_mfma_fewq_kernel<NKB, bf16 | f16>: the (n_seq + 3) / 4 grid tail, odd head counts (the clamped last 4-head chunk)
    case("fewq_bf16_nkb1_h16", "bf16", 1, 16, 16, 1024, inner=16, lens="edge0"),
    case("fewq_f16_nkb1_h5", "f16", 2, 15, 5, 1025, inner=5, causal=True, omap=True),
    case("fewq_bf16_nkb2_h3", "bf16", 2, 32, 3, 4099, inner=7, causal=True, spread=2),
    case("fewq_f16_nkb2_h9", "f16", 1, 17, 9, 4099, lens="edge0", div=3),
    # attention_mfma_kernel<NKB, MAXH, attn_ops_f16x3>
    case("split_nkb1_h2", "f16x3", 16, 16, 2, 7, causal=True, geo="axial"),
    case("split_nkb1_h10", "f16x3", 3, 15, 10, 9, lens="edge0", div=3),
    case("split_nkb1_h18", "f16x3", 1, 16, 18, 7),
    case("split_nkb2_h8", "f16x3", 17, 17, 8, 6, inner=3, causal=True, geo="axial"),
    case("split_nkb2_h16", "f16x3", 32, 32, 16, 4, omap=True, scale=1.0),
    case("split_nkb2_h32", "f16x3", 2, 31, 32, 1023, causal=True),
    # attention_mfma_split_fewq_kernel<NKB>
    case("split_fewq_nkb1_h16", "f16x3", 1, 16, 16, 1024, lens="edge0"),
    case("split_fewq_nkb2_h6", "f16x3", 2, 32, 6, 4099, inner=3, causal=True, omap=True),
]


def reference(q, k, v, c, g, lens, scale):
    """fp64 softmax(q k^T scale + mask) v on the logical rows of q, k, v (fp64 [rows, >= 32 H] tensors of the values the kernel reads).
    Returns out, W = sum_j p_j |v_j|, Smax, sum over visible keys of |v_j| (each [n_seq * nq, 32 H]) and the rows that see no key."""
    n_seq, nq, nk, H = c["n_seq"], c["nq"], c["nk"], c["H"]
    Cc = 32 * H
    qr, kr, _ = _row_maps(c, g)
    Q = q[qr][..., :Cc].reshape(n_seq, nq, H, 32)
    K = k[kr][..., :Cc].reshape(n_seq, nk, H, 32)
    V = v[kr][..., :Cc].reshape(n_seq, nk, H, 32)
    i, j = torch.arange(nq)[:, None], torch.arange(nk)[None, :]
    vis = torch.ones(n_seq, nq, nk, dtype=torch.bool)
    if c["causal"]:
        vis &= (j <= i + nk - nq)[None]
    if lens is not None:
        vis &= j[None] < lens[torch.arange(n_seq) // c["div"]].long()[:, None, None]
    vis4 = vis[:, None]                                                     # [s, 1, i, j]
    S = torch.einsum("sihd,sjhd->shij", Q, K) * scale
    P = torch.softmax(S.masked_fill(~vis4, float("-inf")), -1)              # all -inf rows: NaN, like the kernels
    Smax = (torch.einsum("sihd,sjhd->shij", Q.abs(), K.abs()) * abs(scale)).masked_fill(~vis4, 0).amax(-1)
    out = torch.einsum("shij,sjhd->sihd", P, V)
    W = torch.einsum("shij,sjhd->sihd", P, V.abs())
    sumv = torch.einsum("shij,sjhd->sihd", vis4.double().expand(-1, H, -1, -1), V.abs())
    flat = lambda x: x.reshape(n_seq * nq, Cc)                              # noqa: E731
    return (flat(out), flat(W), flat(Smax.permute(0, 2, 1)[..., None].expand(-1, -1, -1, 32)), flat(sumv),
            ~vis.any(-1).reshape(n_seq * nq))


def bound(kind, ref, W, Smax, sumv, nk):
    b = U * (72 * Smax + 3 * nk + 6) * W
    if kind == "bf16":
        return b + 2.0 ** -15 * W + _ulp(ref, torch.bfloat16)
    if kind == "f16":
        return b + 2.0 ** -22 * W + 2.0 ** -25 * sumv + _ulp(ref, torch.float16)
    if kind == "f32>bf16x3":
        return b + 2.0 ** -17 * ref.abs()
    if kind == "f32>f16x3":
        return b + 2.0 ** -21 * ref.abs() + 2.0 ** -35
    if kind == "f16x3":
        return b + 8 * U * Smax * W + 2.0 ** -21 * W + 2.0 ** -36 * sumv + 2.0 ** -21 * ref.abs() + 2.0 ** -35
    return b


def _sentinel_empty(rows, cols, dt):
    it, val = SENTINEL[dt]
    return torch.full((rows, cols), val, dtype=it, device=DEV).view(dt)


def launch(c, seed=0):
    """Builds the buffers of case c, runs mage_attention once; returns (out buffer on the CPU, reference inputs, geometry, lens)."""
    in_dt, out_dt, out_split, split_in = KINDS[c["kind"]]
    H, Cc = c["H"], 32 * c["H"]
    g, q_rows, kv_rows, o_rows = _geometry(c)
    gen = torch.Generator().manual_seed(1000 * seed + 31 * c["nq"] + 7 * c["nk"] + H)
    if c["geo"] == "axial":
        w = [3 * Cc] * 3
        offs = (0, Cc, 2 * Cc)
        rows = (q_rows, q_rows, q_rows)
    else:
        w = [Cc + 64, Cc + 128, Cc + 192] if split_in else [Cc + 8, Cc + 24, Cc + 40]     # ldq, ldk, ldv all different
        offs = (0, 0, 0)
        rows = (q_rows, kv_rows, kv_rows)
    bufs = [torch.randn(rows[0], w[0], generator=gen)]
    if c["geo"] != "axial":
        bufs += [torch.randn(rows[1], w[1], generator=gen), torch.randn(rows[2], w[2], generator=gen)]
    if split_in:
        dev = [ops.split(b.to(DEV), ops.F16X3) for b in bufs]
        vals = [unsplit(d.cpu(), ops.F16X3) for d in dev]                   # the values the split rows represent
        lds = [2 * x for x in w]
        offs = tuple(2 * o for o in offs)
    else:
        dev = [b.to(in_dt).to(DEV) for b in bufs]
        vals = [d.cpu().double() for d in dev]                              # 16-bit: the rounded inputs
        lds = w
    if c["geo"] == "axial":
        dev, vals = dev * 3, vals * 3
    qv, kv, vv = (vals[t][:, offs[t] // (2 if split_in else 1):] for t in range(3))
    qd, kd, vd = (dev[t][:, offs[t]:] for t in range(3))
    ldo = 2 * Cc + 128 if out_split else Cc + 16
    out = _sentinel_empty(o_rows, ldo, out_dt)
    lens = _lens(c) if c["lens"] else None
    scale = float(torch.tensor(32 ** -0.5 if c["scale"] is None else c["scale"], dtype=torch.float32))
    ops.attention(qd, kd, vd, out, ldq=lds[0], ldk=lds[1], ldv=lds[2], ldo=ldo, n_seq=c["n_seq"], inner=c["inner"], nq=c["nq"], nk=c["nk"],
                  n_head=H, causal=c["causal"], kv_len=lens.to(DEV) if lens is not None else None, kv_len_div=c["div"], scale=scale,
                  out_split=out_split, split_kind=ops.F16X3 if split_in else 0, **g)
    torch.cuda.synchronize()
    return out.cpu(), (qv, kv, vv), g, lens, scale


def check(c, out, inputs, g, lens, scale):
    """The footprint, the NaN rows and the bound; returns the worst |err| / bound."""
    _, out_dt, out_split, _ = KINDS[c["kind"]]
    Cc = 32 * c["H"]
    ref, W, Smax, sumv, dead = reference(*inputs, c, g, lens, scale)
    _, _, orr = _row_maps(c, g)
    orr = orr.reshape(-1)
    pcols = 2 * Cc if out_split else Cc                                     # physical columns written per mapped row
    it, sval = SENTINEL[out_dt]
    bits = out.view(it)
    inside = torch.zeros_like(bits, dtype=torch.bool)
    inside[orr, :pcols] = True
    assert bool((bits[~inside] == sval).all()), f"{c['name']}: {int((bits[~inside] != sval).sum())} elements written outside the mapped rows / columns"
    assert bool((bits[orr, :pcols] != sval).all()), f"{c['name']}: mapped elements left unwritten"
    got = unsplit(out[orr, :pcols], out_split) if out_split else out[orr, :Cc].double()
    if bool(dead.any()):
        if out_dt == torch.float16 and out_split:                           # f16x3 store: NaN clamped to -65504 (see the header)
            assert bool((got[dead] == -65504.0).all()), f"{c['name']}: a row that sees no key is not -65504 in f16x3"
        else:
            assert bool(torch.isnan(got[dead]).all()), f"{c['name']}: a row that sees no key is not NaN"
    live = ~dead
    assert bool(torch.isfinite(got[live]).all()), f"{c['name']}: non-finite output in a row with visible keys"
    err = (got[live] - ref[live]).abs()
    b = bound(c["kind"], ref[live], W[live], Smax[live], sumv[live], c["nk"])
    ratio = (err / b).max().item() if err.numel() else 0.0
    worst = (err / b).flatten().argmax().item() if err.numel() else 0
    assert ratio <= 1.0, (f"{c['name']}: |err| {err.flatten()[worst].item():.3e} > bound {b.flatten()[worst].item():.3e} "
                          f"(ref {ref[live].flatten()[worst].item():.6e}, got {got[live].flatten()[worst].item():.6e})")
    print(f"attention {c['name']} [{c['kind']}]: worst |err| / bound {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("c", CASES)
def test_attention_against_fp64(c):
    check(c, *launch(c))


FEWQ_IDENTITY = [
    case("id_fewq_bf16_nkb1_h5", "bf16", 2, 16, 5, 1025, causal=True),                # no fewq: mfma<1, 2>; no mfma: attention_kernel<bf16, 16>
    case("id_fewq_f16_nkb2_h9", "f16", 1, 17, 9, 4099, lens="edge0"),                  # mfma<2, 4>; attention_kernel<f16, 32>
    case("id_fewq_bf16_nkb2_h3", "bf16", 1, 32, 3, 1024, inner=4, lens="edge", div=3, omap=True),   # mfma<2, 2>; attention_kernel<bf16, 32>
    case("id_fewq_f16_nkb1_h17", "f16", 2, 1, 17, 1024, inner=2),                      # mfma<1, 8>; attention_kernel<f16, 16>
    case("id_split_fewq_nkb1_h6", "f16x3", 2, 15, 6, 1025, causal=True),               # split<1, 2>
    case("id_split_fewq_nkb2_h10", "f16x3", 1, 32, 10, 4099, inner=3, lens="edge0"),   # split<2, 4>
]


@pytest.mark.parametrize("c", FEWQ_IDENTITY)
def test_fewq_bit_identical_to_the_workgroup_kernel(c):
    """attention.hip's claim under attention_mfma_fewq_kernel: per (sequence, head) the same operations on the same values as
    attention_mfma_kernel (and the split pair likewise), so the incremental loop's rows equal the full pass's bit for bit.  The
    thread-per-query kernel behind attn_no_mfma has its own arithmetic: it must meet the same fp64 bound."""
    out, inputs, g, lens, scale = launch(c)
    check(c, out, inputs, g, lens, scale)
    with config.lib_option("attn_no_fewq", 1):
        out2 = launch(c)[0]
    it = SENTINEL[out.dtype][0]
    assert torch.equal(out.view(it), out2.view(it)), f"{c['name']}: fewq kernel differs from the workgroup kernel"
    if c["kind"] in ("bf16", "f16"):
        with config.lib_option("attn_no_mfma", 1):
            check(c, *launch(c))


@pytest.mark.parametrize("dt,off", [(torch.bfloat16, 4), (torch.float16, 4), (torch.float32, 2), (torch.float32, 1)])
@pytest.mark.parametrize("which", ["q", "k", "v", "out"])
def test_attention_refuses_misaligned_operands(dt, off, which):
    """Every kernel moves q, k, v and out in 16-byte vectors: a base 8 (or 4) bytes off is refused before anything launches.
    (The buffers are large enough that even a launch would stay inside them.)"""
    H, nq, nk, n_seq = 2, 4, 4, 2
    Cc = 32 * H
    ld = Cc + 8
    base = {t: torch.randn(n_seq * 8 + 2, ld).to(dt).to(DEV) for t in ("q", "k", "v")}
    base["out"] = _sentinel_empty(n_seq * 8 + 2, ld, dt)
    views = {t: (b.view(-1)[off:] if t == which else b) for t, b in base.items()}
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.attention(views["q"], views["k"], views["v"], views["out"], ldq=ld, ldk=ld, ldv=ld, ldo=ld, n_seq=n_seq, inner=1, nq=nq, nk=nk,
                      n_head=H, q_outer_stride=nq, q_axis_stride=1, kv_outer_stride=nk, kv_axis_stride=1)
    torch.cuda.synchronize()
    it, sval = SENTINEL[dt]
    assert bool((base["out"].cpu().view(it) == sval).all())
