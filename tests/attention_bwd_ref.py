"""fp64 restatement of mage_attention_bwd (include/mage_hip.h; kernels in mage_amd/csrc/attention_bwd.hip) on the logical rows of a
mage_attn_desc, as closed formulas, with the per-element error bounds of the three kernel families.

For one (sequence s, head h), queries i, keys j, 32 columns c, mask as in the forward (causal aligned to the last key, then
kv_len[s / kv_len_div]), m_ij = keep(s, h, i, j) / (1 - p) (1 without dropout; keep = hash32(drop_seed * 0x9e3779b97f4a7c15 +
((s * n_head + h) * nq + i) * nk + j) >= p * 2^32 in uint64 wrap-around arithmetic):
    P = softmax(scale Q K^T + mask)      P' = P m              dV = P'^T dO
    dP = (dO V^T) m                      D_i = sum_j P_ij dP_ij dS = P (dP - D)
    dQ = scale dS K                      dK = scale dS^T Q
A query that sees no key has an all -inf row: P, hence dS, is NaN on every key of that row, so dq of the query and dk, dv of EVERY key
of its (sequence, head) are NaN (what torch.autograd gives through softmax(scores + mask); tests/test_attention_bwd_ref_cpu.py).

Bounds.  u = 2^-24, first order in u.  Per query i: Smax_i = max over visible j of |scale| sum_c |q_ic| |k_jc|; A_ij = m_ij sum_c
|dO_ic| |v_jc| (>= |dP_ij|); E_ij = |dP_ij| + sum_l P_il |dP_il|; F_ij = A_ij + sum_l P_il A_il.  Condition sums:
    Cq_ic = |scale| sum_j P_ij E_ij |k_jc|      CAq: the same with F for E
    Ck_jc = |scale| sum_i P_ij E_ij |q_ic|      CAk: the same with F for E
    Cv_jc = sum_i P'_ij |dO_ic|
(|dS_ij| <= P_ij E_ij, so Cq, Ck, Cv bound the absolute sums behind dq, dk, dv.)  kt and qt are the term counts of the sums over keys and
over queries: nk and nq in the thread-per-query kernel, 2 nk and 2 nq in the matrix-core kernel (P and dS enter as hi + lo: two
products per term).
  P:   as in the forward (tests/test_gpu_attention.py): a score is a 32-term fp32 dot product scaled once, (32 + 2) u Smax; the
       subtraction of the maximum 2 u Smax, expf 2 u: relative 36 u Smax + 2 u in the unnormalised weight; the nk-term denominator
       moves the ratio by as much again plus nk u, then one reciprocal and one multiply:  eP_i = (72 Smax_i + nk + 6) u, relative.
  dP:  a 32-term dot product, |d dP_ij| <= cd u A_ij, cd = 32; with dropout the fp32 1 / (1 - p) and its multiply: cd = 34.
  D:   nk products and additions of the computed P and dP:  |dD_i| <= (eP_i + (nk + 1) u) sum_l P_il |dP_il| + cd u sum_l P_il A_il.
  dS:  t_ij = P_ij (dP_ij - D_i): eP_i on P, the errors of dP and D, one subtraction and one multiply (2 u (|dP_ij| + |D_i|)):
       |dt_ij| <= P_ij ((2 eP_i + (nk + 3) u) E_ij + cd u F_ij).
  dq:  kt fused multiply-adds and the multiply by scale, (kt + 1) u sum_j |t_ij| |k_jc| |scale|:
       |err dq_ic| <= u sum_j |scale| P_ij |k_jc| ((144 Smax_i + 3 nk + kt + 16) E_ij + cd F_ij).
  dk:  the same t, qt terms accumulated over the queries in a fixed order, and the scale:
       |err dk_jc| <= u sum_i |scale| P_ij |q_ic| ((144 Smax_i + 3 nk + qt + 16) E_ij + cd F_ij).
  dv:  P' = P m (eP_i, and 2 u for 1 / (1 - p) and its multiply under dropout), qt terms:
       |err dv_jc| <= u sum_i P'_ij |dO_ic| (72 Smax_i + nk + 6 + cm + qt), cm = 2 with dropout, else 0.
  matrix cores (bf16):  P and dS go through split_hi_lo, two 8-bit truncations: relative 2^-15 on every term, + 2^-15 (Cq | Ck | Cv).
  bf16 output:          + 1 bf16 ulp at |ref| for the store (both bf16 kernels).
Keys no query of the sequence sees have P = 0 exactly: dk = dv = 0 exactly there (when every query of the sequence sees some key).
No constant here is fitted to a kernel's output."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers import attn_case, attn_row_maps, ulp
from tests.sampling_ref import GOLDEN_GAMMA, hash32

U = 2.0 ** -24
FAMILIES = ("f32", "bf16_tpq", "bf16_mfma")          # attention_bwd_kernel<float>, attention_bwd_kernel<unsigned short>, attention_bwd_mfma_kernel


def bwd_case(name, kind, nq, nk, H, n_seq, drop=0.0, seed=0, mis=None, **kw):
    """A forward case (tests/helpers.py attn_case) with the backward's extras: drop / seed: dropout on the probabilities; mis: 'ld' (ldk
    4 elements off a multiple of 8) or 'base' (q 8 bytes off a 16-byte boundary), which send bf16 to the thread-per-query kernel."""
    p = attn_case(name, kind, nq, nk, H, n_seq, **kw)
    p.values[0].update(drop=drop, seed=seed, mis=mis)
    return p


def keep_scale(c, drop, seed):
    """m[s, h, i, j] = keep / (1 - p) in fp64, p the fp32 value the descriptor carries; the threshold is (uint32)(p * 2^32)."""
    n_seq, nq, nk, H = c["n_seq"], c["nq"], c["nk"], c["H"]
    p = float(np.float32(drop))
    thresh = np.uint64(int(p * 4294967296.0))
    idx = np.arange(n_seq * H * nq * nk, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = np.uint64(seed & (2 ** 64 - 1)) * GOLDEN_GAMMA + idx
    keep = hash32(ctr) >= thresh
    return torch.from_numpy(keep.reshape(n_seq, H, nq, nk)).double() / (1.0 - p)


def visible(c, lens):
    """vis[s, i, j]: key j visible to query i of sequence s."""
    n_seq, nq, nk = c["n_seq"], c["nq"], c["nk"]
    i, j = torch.arange(nq)[:, None], torch.arange(nk)[None, :]
    vis = torch.ones(n_seq, nq, nk, dtype=torch.bool)
    if c["causal"]:
        vis &= (j <= i + nk - nq)[None]
    if lens is not None:
        vis &= j[None] < lens[torch.arange(n_seq) // c["div"]].long()[:, None, None]
    return vis


def gather(q, k, v, do, c, g):
    """The logical [n_seq, n, H, 32] operands behind the row maps (q, k, v, do: fp64 [rows, >= 32 H] of the values the kernel reads)."""
    n_seq, nq, nk, H = c["n_seq"], c["nq"], c["nk"], c["H"]
    Cc = 32 * H
    qr, kr, _ = attn_row_maps(dict(c, omap=False), g)
    return (q[qr][..., :Cc].reshape(n_seq, nq, H, 32), k[kr][..., :Cc].reshape(n_seq, nk, H, 32), v[kr][..., :Cc].reshape(n_seq, nk, H, 32),
            do[qr][..., :Cc].reshape(n_seq, nq, H, 32))


def reference(q, k, v, do, c, g, lens, scale):
    """dq [n_seq * nq, 32 H], dk, dv [n_seq * nk, 32 H] in fp64 with the condition sums of the module docstring (same shapes), and
    dead_q [n_seq * nq] (the query sees no key), dead_k [n_seq * nk] (a query of the key's sequence sees no key: dk, dv NaN),
    zero_k [n_seq * nk] (no query sees the key, none is dead: dk = dv = 0 exactly)."""
    n_seq, nq, nk, H = c["n_seq"], c["nq"], c["nk"], c["H"]
    Cc = 32 * H
    Q, K, V, G = gather(q, k, v, do, c, g)
    vis = visible(c, lens)
    vis4 = vis[:, None]                                                     # [s, 1, i, j]
    m = keep_scale(c, c["drop"], c["seed"]) if c["drop"] > 0 else torch.ones(n_seq, H, nq, nk, dtype=torch.float64)
    S = torch.einsum("sihd,sjhd->shij", Q, K) * scale
    P = torch.softmax(S.masked_fill(~vis4, float("-inf")), -1)              # all -inf rows: NaN
    Smax = (torch.einsum("sihd,sjhd->shij", Q.abs(), K.abs()) * abs(scale)).masked_fill(~vis4, 0).amax(-1, keepdim=True)
    Pm = P * m
    dP = torch.einsum("sihd,sjhd->shij", G, V) * m
    A = torch.einsum("sihd,sjhd->shij", G.abs(), V.abs()) * m
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    E = dP.abs() + (P * dP.abs()).sum(-1, keepdim=True)
    F = A + (P * A).sum(-1, keepdim=True)
    PE, PF = P * E, P * F
    onq = lambda w, x: torch.einsum("shij,sjhd->sihd", w, x).reshape(n_seq * nq, Cc)      # noqa: E731  sums over keys
    onk = lambda w, x: torch.einsum("shij,sihd->sjhd", w, x).reshape(n_seq * nk, Cc)      # noqa: E731  sums over queries
    a = abs(scale)
    dead_q = ~vis.any(-1)                                                   # [s, i]
    dead_s = dead_q.any(-1)                                                 # [s]
    return SimpleNamespace(
        dq=scale * onq(dS, K), dk=scale * onk(dS, Q), dv=onk(Pm, G),
        Cq=a * onq(PE, K.abs()), CqS=a * onq(PE * Smax, K.abs()), CAq=a * onq(PF, K.abs()),
        Ck=a * onk(PE, Q.abs()), CkS=a * onk(PE * Smax, Q.abs()), CAk=a * onk(PF, Q.abs()),
        Cv=onk(Pm, G.abs()), CvS=onk(Pm * Smax, G.abs()),
        dead_q=dead_q.reshape(-1), dead_k=dead_s[:, None].expand(-1, nk).reshape(-1),
        zero_k=(~vis.any(1) & ~dead_s[:, None]).reshape(-1))


def bounds(family, r, c):
    """(bound of dq, of dk, of dv) for a kernel family of FAMILIES; NaN where the reference is."""
    assert family in FAMILIES
    nq, nk = c["nq"], c["nk"]
    mfma = family == "bf16_mfma"
    kt, qt = (2 * nk, 2 * nq) if mfma else (nk, nq)
    cd, cm = (34, 2) if c["drop"] > 0 else (32, 0)
    bq = U * (144 * r.CqS + (3 * nk + kt + 16) * r.Cq + cd * r.CAq)
    bk = U * (144 * r.CkS + (3 * nk + qt + 16) * r.Ck + cd * r.CAk)
    bv = U * (72 * r.CvS + (nk + 6 + cm + qt) * r.Cv)
    if mfma:
        bq, bk, bv = bq + 2.0 ** -15 * r.Cq, bk + 2.0 ** -15 * r.Ck, bv + 2.0 ** -15 * r.Cv
    if family != "f32":
        bq, bk, bv = bq + ulp(r.dq, torch.bfloat16), bk + ulp(r.dk, torch.bfloat16), bv + ulp(r.dv, torch.bfloat16)
    return bq, bk, bv
