"""CPU: the fp64 restatement of mage_attention_bwd (tests/attention_bwd_ref.py) against torch.autograd in float64 through
softmax(scale q k^T + mask) with an additive -inf mask, the dropout mask applied as a constant.  Agreement to fp64 rounding: 1e-12 of the
condition sums.  A query that sees no key makes autograd return NaN in dq of that query and in dk, dv of every key of its (sequence,
head), and nowhere else: the restatement must place its NaN identically -- this is the contract the kernels are held to on the GPU."""
import pytest
import torch

from tests import attention_bwd_ref as R
from tests.helpers import attn_geometry, attn_lens, attn_row_maps

CASES = [
    R.bwd_case("axial_causal", "f64", 7, 7, 3, 10, inner=4, causal=True, geo="axial"),
    R.bwd_case("causal_nq_lt_nk", "f64", 5, 13, 2, 6, inner=2, causal=True),
    R.bwd_case("kv_len_div3", "f64", 6, 9, 2, 14, lens="edge", div=3),
    R.bwd_case("sep_row_gaps", "f64", 4, 10, 5, 6, inner=3, spread=2, scale=1.0),
    R.bwd_case("dropout", "f64", 9, 12, 2, 5, lens="edge", drop=0.25, seed=0x1234567890ABCDEF),
    # queries that see no key: kv_len 0 (sequences 0..2 of 'edge0' / div 3), and the first nq - nk queries of a causal nq > nk
    R.bwd_case("dead_kv_len0", "f64", 6, 9, 2, 14, lens="edge0", div=3),
    R.bwd_case("dead_causal_nq_gt_nk", "f64", 8, 5, 3, 4, causal=True),
    R.bwd_case("dead_causal_kv_len", "f64", 6, 6, 2, 7, causal=True, geo="axial", lens="edge0"),
    # dropout over dead queries: a dropped (i, j) is NaN * 0, so dv stays NaN on every key
    R.bwd_case("dead_dropout_kv_len0", "f64", 10, 14, 3, 8, lens="edge0", drop=0.3, seed=11),
    R.bwd_case("dead_dropout_causal_nq_gt_nk", "f64", 15, 14, 2, 4, causal=True, drop=0.5, seed=5),
]


def _buffers(c, g, q_rows, kv_rows):
    Cc = 32 * c["H"]
    gen = torch.Generator().manual_seed(17 * c["nq"] + c["nk"])
    if c["geo"] == "axial":
        qkv = torch.randn(q_rows, 3 * Cc, generator=gen, dtype=torch.float64)
        q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    else:
        q = torch.randn(q_rows, Cc + 8, generator=gen, dtype=torch.float64)
        k = torch.randn(kv_rows, Cc + 24, generator=gen, dtype=torch.float64)
        v = torch.randn(kv_rows, Cc + 40, generator=gen, dtype=torch.float64)
    do = torch.randn(q_rows, Cc + 16, generator=gen, dtype=torch.float64)
    return q, k, v, do


def _autograd(q, k, v, do, c, g, lens, scale):
    """Gradients with respect to the BUFFERS (rows outside the maps get 0), gathered back to the logical rows."""
    n_seq, nq, nk, H = c["n_seq"], c["nq"], c["nk"], c["H"]
    Cc = 32 * H
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    Q, K, V, G = R.gather(q, k, v, do, c, g)
    mask = torch.zeros(n_seq, 1, nq, nk, dtype=torch.float64).masked_fill(~R.visible(c, lens)[:, None], float("-inf"))
    P = torch.softmax(torch.einsum("sihd,sjhd->shij", Q, K) * scale + mask, -1)
    if c["drop"] > 0:
        P = P * R.keep_scale(c, c["drop"], c["seed"])
    out = torch.einsum("shij,sjhd->sihd", P, V)
    (out * G).sum().backward()
    qr, kr, _ = attn_row_maps(c, g)
    return q.grad[qr.reshape(-1), :Cc], k.grad[kr.reshape(-1), :Cc], v.grad[kr.reshape(-1), :Cc]


@pytest.mark.parametrize("c", CASES)
def test_restatement_matches_float64_autograd(c):
    g, q_rows, kv_rows, _ = attn_geometry(c)
    lens = attn_lens(c) if c["lens"] else None
    scale = 32 ** -0.5 if c["scale"] is None else c["scale"]
    q, k, v, do = _buffers(c, g, q_rows, kv_rows)
    r = R.reference(q, k, v, do, c, g, lens, scale)
    wq, wk, wv = _autograd(q, k, v, do, c, g, lens, scale)
    dead = c["name"].startswith("dead")
    assert bool(r.dead_q.any()) == dead, "the case does not have the dead queries its name promises"
    for name, got, want, cond in (("dq", r.dq, wq, r.Cq), ("dk", r.dk, wk, r.Ck), ("dv", r.dv, wv, r.Cv)):
        assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{c['name']} {name}: NaN placement differs from autograd's"
        live = ~torch.isnan(want)
        assert bool(torch.isfinite(got[live]).all())
        err = (got[live] - want[live]).abs()
        assert bool((err <= 1e-12 * cond[live]).all()), f"{c['name']} {name}: max err / cond {(err / cond[live]).max().item():.3e}"
    # the NaN placement, stated: dq rows of the dead queries; dk, dv rows of every key of a sequence that has one; all heads; nothing else
    assert torch.equal(torch.isnan(wq), r.dead_q[:, None].expand_as(wq))
    assert torch.equal(torch.isnan(wk), r.dead_k[:, None].expand_as(wk)) and torch.equal(torch.isnan(wv), r.dead_k[:, None].expand_as(wv))
    if dead and not (c["causal"] and c["nq"] > c["nk"]):          # causal nq > nk: every sequence has dead queries
        assert bool((~r.dead_k).any()), "no sequence without a dead query: 'other sequences are unaffected' is not exercised"
    # keys no query sees (no dead query in the sequence): exactly zero gradients
    assert bool((wk[r.zero_k] == 0).all()) and bool((wv[r.zero_k] == 0).all())
    assert bool((r.dk[r.zero_k] == 0).all()) and bool((r.dv[r.zero_k] == 0).all())


def test_dropout_mask_matches_the_header_formula():
    """keep_scale against a scalar evaluation of the header's formula (uint64 wrap-around), at a few indices."""
    c = dict(n_seq=3, nq=5, nk=7, H=2)
    seed, p = 0xFEDCBA9876543210, 0.3
    m = R.keep_scale(c, p, seed)
    p32 = float(torch.tensor(p, dtype=torch.float32))
    M64 = 2 ** 64

    def h32(x):
        x ^= x >> 33
        x = x * 0xFF51AFD7ED558CCD % M64
        x ^= x >> 33
        x = x * 0xC4CEB9FE1A85EC53 % M64
        x ^= x >> 33
        return x & 0xFFFFFFFF
    for s, h, i, j in ((0, 0, 0, 0), (2, 1, 4, 6), (1, 0, 3, 2), (2, 0, 0, 5)):
        idx = ((s * 2 + h) * 5 + i) * 7 + j
        keep = h32((seed * 0x9E3779B97F4A7C15 + idx) % M64) >= int(p32 * 2 ** 32)
        assert m[s, h, i, j].item() == (1.0 / (1.0 - p32) if keep else 0.0)
    assert 0.55 < (m > 0).double().mean().item() < 0.85
