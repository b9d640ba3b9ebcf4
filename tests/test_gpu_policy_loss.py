"""GPU: mage_policy_loss / mage_policy_loss_bwd against mage_token_stats bit for bit, against mage_cross_entropy and against the fp64
restatement (tests/policy_ref.py) evaluated with the kept set the kernel reports (which must be one of token_stats_ref.admissible_sets).

Bounds, per row.
  logprob, entropy, |N| implied by cut: mage_token_stats' bits on the same inputs (that kernel is pinned against fp64 in
    tests/test_gpu_token_stats.py).
  row_loss against the fp64 formula on the kernel's own fp32 logprob / entropy: |d| <= (4 + |logprob - b|) 2^-23 |l| -- one expf (2 ulp),
    the rounding of its argument (|logprob - b| 2^-24 relative in rho), three multiplies / adds.  The advantages are drawn with
    0.5 <= |A| <= 2 and entropy_coef <= 0.01, so |A| rho >= 0.4 stands against entropy_coef H <= 0.01 log 4096 = 0.084: the two terms of l
    never cancel to less than 0.79 of the surrogate term, and rho's error relative to l stays below 1.27 times its error relative to rho.
  cross-entropy (T = 1, no filter, A = 1): both kernels form l = lse - z_t from their own fp32 lse; "2 ulp" is taken at the larger of |l|
    and |lse| -- the operand the two fixed summation orders round differently (an ulp of a small difference l would ask for more than
    either kernel's lse holds).
  summary against the fp64 means of the kernel's own per-row outputs: one fp32 rounding, 2^-24 relative.
  dlogits against policy_ref: fp32 within 2 TOL max_j |want_ij| (TOL = token_stats_ref's 1e-5 allowance for the fixed-order fp32 mass sums),
    bf16 adds 2^-8 |want_ij| for the one bf16 store rounding; entries outside the set and outside rows are exactly 0.  Both get the
    absolute floor 2^-126: fp32 and bf16 hold no relative precision below their smallest normal number, and the +-100 row at
    temperature 0.7 asks for exp(-285) = 1e-124 against a row maximum of the same size.
Clipped-form inputs keep every rho at least 1e-3 (relative) away from both clip edges, checked in fp64 on the log-probabilities the kernel
itself sees (mage_token_stats' bits), so both sides take the same branch; b = logprob exactly (rho = 1) is its own test."""
import numpy as np
import pytest
import torch

from mage_amd import ops
from tests import helpers as H
from tests import policy_ref as P
from tests import sampling_ref as S
from tests import token_stats_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILTERS = [(0, 1.0), (20, 1.0), (0, 0.9), (20, 0.9)]
TEMPS = (0.7, 1.0, 1.5)
CLIP = (0.2, 0.3)
SMALL_ROWS = 29                                                      # 7 workgroups of 4 waves and a single wave; holds every special row


def _logits(rows, K, seed):
    """tests/test_gpu_token_stats.py's recipe: ties on a 1/4 grid, a repeated top-20 boundary value, and its special rows (+-80, -inf entries,
    a NaN, all -inf, uniform, +-100) at rows 1, 2, 8, 9, 10, 12."""
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((rows, K))).astype(np.float32)
    for r in range(0, rows, 7):
        z[r] = np.round(z[r] * 4) / 4
    for r in range(3, rows, 11):
        o = np.argsort(-z[r], kind="stable")
        if K > 22:
            z[r, o[20:23]] = z[r, o[19]]
    if rows > 12:
        z[1] = z[1] / np.abs(z[1]).max() * 80.0
        z[12] = z[12] / np.abs(z[12]).max() * 100.0
        z[2, g.integers(0, K, max(K // 3, 1))] = -np.inf
        z[8, int(g.integers(0, K))] = np.nan
        z[9, :] = -np.inf
        z[10, :] = 0.5
    return z


def _keys(s):
    """The sampler's order-preserving key of fp32 values (sample_key, mage_amd/csrc/token_row.h): NaN -> 0, -0 == +0."""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    k = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(s)] = 0
    return k


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


class Case:
    """One launch's inputs: rows of `z` (device tensor zd, row stride ld), tokens, advantages (|A| in [0.5, 2], both signs), optional b."""

    def __init__(self, z, zd, K, T, k, p, seed, clipped, adv_div, c):
        self.z, self.zd, self.K, self.T, self.k, self.p, self.c, self.adv_div = z, zd, K, T, k, p, c, adv_div
        rows = self.rows = z.shape[0]
        g = np.random.default_rng(seed)
        tok = torch.empty(rows, dtype=torch.int64, device=DEV)
        seeds = torch.from_numpy(g.integers(-2 ** 63, 2 ** 63 - 1, 1, dtype=np.int64)).to(DEV)
        ops.sample_tokens(zd, tok, seeds, rows=rows, K=K, temperature=T, top_k=k, top_p=p, pos_off=0, ld=zd.stride(0))
        tok[1::2] = torch.from_numpy(g.integers(0, K, rows)).to(DEV)[1::2]         # even rows: drawn by the sampler; odd rows: uniform
        self.tok = tok
        n_adv = -(-rows // adv_div)
        self.A = (g.uniform(0.5, 2.0, n_adv) * g.choice([-1.0, 1.0], n_adv)).astype(np.float32)
        self.Ad = torch.from_numpy(self.A).to(DEV)
        self.cmin, self.cmax = P.clip_bounds(*CLIP)
        self.stats = dict(policy_logprob=torch.empty(rows, device=DEV), policy_entropy=torch.empty(rows, device=DEV),
                          kept=torch.empty(rows, dtype=torch.int32, device=DEV))
        ops.token_stats(zd, tok, rows=rows, K=K, temperature=T, top_k=k, top_p=p, ld=zd.stride(0), **self.stats)
        self.b = self.bd = None
        if clipped:                                                  # rho on both sides of [cmin, cmax] and inside it, never within 1e-3 of an edge
            lp = self.stats["policy_logprob"].cpu().numpy().astype(np.float64)
            b = np.where(np.isfinite(lp), lp, 0.0) + g.choice([-0.35, -0.1, 0.1, 0.35], rows) * g.uniform(0.8, 1.0, rows)
            b = b.astype(np.float32)
            for _ in range(4):
                with np.errstate(invalid="ignore", over="ignore"):
                    rho = np.exp(lp - b.astype(np.float64))
                    near = (np.abs(rho / self.cmin - 1) < 1e-3) | (np.abs(rho / self.cmax - 1) < 1e-3)
                b[near] += np.float32(0.01)
            assert not near.any()
            self.b, self.bd = b, torch.from_numpy(b).to(DEV)

    def forward(self):
        return ops.policy_loss(self.zd, self.tok, self.Ad, self.bd, temperature=self.T, top_k=self.k, top_p=self.p, clip_lo=CLIP[0],
                               clip_hi=CLIP[1], entropy_coef=self.c, adv_div=self.adv_div)

    def backward(self, cut, gout, dt):
        dl = torch.empty(self.rows, self.K, device=DEV, dtype=dt)
        return ops.policy_loss_bwd(self.zd, self.tok, self.Ad, self.bd, cut, gout, dl, temperature=self.T, clip_lo=CLIP[0], clip_hi=CLIP[1],
                                   entropy_coef=self.c, adv_div=self.adv_div)

    def adv(self, r):
        return float(self.A[r // self.adv_div])


def _check(case, dt, worst):
    """Every check of the module docstring on one launch; `worst` collects the largest error / bound per quantity."""
    z, K, rows, T, k, p = case.z, case.K, case.rows, case.T, case.k, case.p
    out = case.forward()
    gout = torch.tensor([0.7], device=DEV)
    dl = case.backward(out["cut"], gout, dt)
    again, dl2 = case.forward(), case.backward(out["cut"], gout, dt)
    ops.check_device_errors(DEV)
    for n in out:                                                    # deterministic: two launches, the same bits
        assert torch.equal(_bits(out[n]), _bits(again[n])), n
    assert torch.equal(dl.view(torch.int16 if dt == torch.bfloat16 else torch.int32), dl2.view(torch.int16 if dt == torch.bfloat16 else torch.int32))
    # mage_token_stats' bits
    assert torch.equal(_bits(out["logprob"]), _bits(case.stats["policy_logprob"]))
    assert torch.equal(_bits(out["entropy"]), _bits(case.stats["policy_entropy"]))
    cut = out["cut"].cpu().numpy().view(np.uint32)
    s = (z * S.inv_temperature(T)).astype(np.float32)
    keep = _keys(s) >= cut[:, None]
    assert (cut >= 1).all() and np.array_equal(keep.sum(1), case.stats["kept"].cpu().numpy())
    tok = case.tok.cpu().numpy()
    lp32, h32 = out["logprob"].cpu().numpy().astype(np.float64), out["entropy"].cpu().numpy().astype(np.float64)
    loss = out["row_loss"].cpu().numpy().astype(np.float64)
    got_dl = dl.float().cpu().numpy().astype(np.float64)
    scale, c32 = float(np.float32(0.7)) / rows, float(np.float32(case.c))
    terms = []
    for r in range(rows):
        sets = R.admissible_sets(z[r], T, k, p)
        assert any(np.array_equal(keep[r], N) for N in sets), f"row {r}: the reported set (|N| = {keep[r].sum()}) is not admissible"
        b = None if case.b is None else float(case.b[r])
        # the loss term from the kernel's own fp32 logprob / entropy
        t = P.term(lp32[r], h32[r], case.adv(r), b, case.cmin, case.cmax, c32)
        terms.append(t)
        if np.isnan(t["loss"]):
            assert np.isnan(loss[r]), r
        else:
            bound = (4 + (abs(lp32[r] - b) if b is not None and not t["outside"] else 0.0)) * 2.0 ** -23 * abs(t["loss"])
            assert abs(loss[r] - t["loss"]) <= bound, f"row {r}: row_loss {loss[r]!r} want {t['loss']!r} bound {bound:.3e}"
            worst["row_loss"] = max(worst.get("row_loss", 0.0), abs(loss[r] - t["loss"]) / bound if bound else 0.0)
        if t["outside"]:
            assert loss[r] == 0.0 and (not keep[r][tok[r]] or np.isneginf(z[r, tok[r]]))
        # the gradient row from the fp64 restatement under the reported set
        ref = P.row(z[r], int(tok[r]), case.adv(r), b, T, keep[r], case.cmin, case.cmax, c32)
        assert ref["outside"] == t["outside"] and (np.isnan(ref["loss"]) or ref["off"] == t["off"]), r
        want = P.dlogits_row(z[r], int(tok[r]), case.adv(r), b, T, keep[r], case.cmin, case.cmax, c32, scale)
        assert np.array_equal(np.isnan(got_dl[r]), np.isnan(want)), f"row {r}: NaN pattern"
        assert (got_dl[r][~keep[r]] == 0).all() and (not t["outside"] or (got_dl[r] == 0).all()), f"row {r}: entries that must be exactly 0"
        fin = ~np.isnan(want)
        if fin.any():
            bound = 2 * R.TOL * np.abs(want[fin]).max() + (2.0 ** -8 * np.abs(want[fin]) if dt == torch.bfloat16 else 0.0) + 2.0 ** -126
            err = np.abs(got_dl[r][fin] - want[fin])
            assert (err <= bound).all(), f"row {r}: dlogits |d| {err.max():.3e} > bound (row max {np.abs(want[fin]).max():.3e})"
            if np.abs(want[fin]).max() > 0:
                worst["dlogits"] = max(worst.get("dlogits", 0.0), float((err / bound).max()))
    # summary: the fp64 means of the kernel's own per-row outputs, one fp32 rounding
    inside = np.array([not t["outside"] for t in terms])
    with np.errstate(invalid="ignore"):
        want = np.array([loss[inside].sum(), h32[inside].sum(),
                         (case.b.astype(np.float64)[inside] - lp32[inside]).sum() if case.b is not None else 0.0,
                         float(sum(t["off"] for t in terms)), float((~inside).sum())]) / rows
    got = out["summary"].cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= 2.0 ** -24 * np.abs(want[ok]) * (1 + 1e-6)).all(), (got, want)
    return out, terms


@pytest.mark.parametrize("K", [4, 260, 512, 1024, 2048, 4096])
def test_kernels_match_token_stats_and_the_restatement(K):
    worst, n_out, n_off, n_rows = {}, 0, 0, 0
    z = _logits(SMALL_ROWS, K, seed=K)
    zd = torch.from_numpy(z).to(DEV)
    i = 0
    for k, p in FILTERS:
        k = min(k, K // 2)                                          # K = 4: top_k = 2
        for T in TEMPS:
            # the twelve filter x temperature launches take turns in form, gradient dtype, advantage divisor and entropy weight
            case = Case(z, zd, K, T, k, p, seed=100 * K + i, clipped=i % 2 == 1, adv_div=(1, 5)[(i // 2) % 2], c=(0.0, 0.01)[(i // 3) % 2])
            _, terms = _check(case, (torch.float32, torch.bfloat16)[(i // 2 + i) % 2], worst)
            n_out, n_off, n_rows, i = n_out + sum(t["outside"] for t in terms), n_off + sum(t["off"] for t in terms), n_rows + len(terms), i + 1
    # several workgroups, rows not a multiple of 4, a divisor that does not divide rows, a row stride above K once; no special row (a finite summary)
    big, ld = 259, K + 4 * (K == 260)
    zb = _logits(big + 13, K, seed=K + 1)[13:]
    zbd = torch.zeros(big, ld, device=DEV)
    zbd[:, :K] = torch.from_numpy(zb).to(DEV)
    assert zbd[:, :K].stride(0) == ld
    case = Case(zb, zbd[:, :K], K, 0.7, min(20, K // 2), 0.9, seed=K + 2, clipped=True, adv_div=6, c=0.01)
    out, terms = _check(case, torch.bfloat16, worst)
    assert torch.isfinite(out["summary"]).all()
    n_out, n_off, n_rows = n_out + sum(t["outside"] for t in terms), n_off + sum(t["off"] for t in terms), n_rows + len(terms)
    assert n_out > 0 and n_off > 0 and n_rows - n_out - n_off > n_rows // 4     # every kind of row was met
    print(f"K={K}: {n_rows} rows ({n_out} outside, {n_off} clipped), largest error / bound: " + ", ".join(f"{a} {b:.3f}" for a, b in worst.items()))


@pytest.mark.parametrize("K", [4, 260, 512, 1024, 2048, 4096])
def test_unit_advantage_unfiltered_is_cross_entropy(K):
    rows = 259
    z = _logits(rows + 13, K, seed=K + 3)[13:]
    zd = torch.from_numpy(z).to(DEV)
    tok = torch.from_numpy(np.random.default_rng(K).integers(0, K, rows)).to(DEV)
    out = ops.policy_loss(zd, tok, torch.ones(1, device=DEV), None, temperature=1.0, top_k=0, top_p=1.0, entropy_coef=0.0)
    l, s = H.lib()
    ce, mean = torch.empty(rows, device=DEV), torch.empty(1, device=DEV)
    assert l.mage_cross_entropy(zd.data_ptr(), tok.data_ptr(), rows, K, ce.data_ptr(), mean.data_ptr(), s) == 0
    ops.check_device_errors(DEV)
    got, want = out["row_loss"].cpu().numpy().astype(np.float64), ce.cpu().numpy().astype(np.float64)
    lse = want + z[np.arange(rows), tok.cpu().numpy()].astype(np.float64)
    ulps = np.abs(got - want) / _ulp(np.maximum(np.abs(want), np.abs(lse)))
    print(f"K={K}: row_loss against mage_cross_entropy, largest difference {ulps.max():.2f} ulp")
    assert (ulps <= 2).all()
    assert abs(out["summary"][0].item() - mean.item()) <= np.mean(2 * _ulp(np.maximum(np.abs(want), np.abs(lse)))) + 2 * _ulp(mean.item())
    assert (out["summary"][2:] == 0).all()
    # ... and the gradient is cross-entropy's
    gout = torch.tensor([1.0], device=DEV)
    dl = ops.policy_loss_bwd(zd, tok, torch.ones(1, device=DEV), None, out["cut"], gout, torch.empty(rows, K, device=DEV), temperature=1.0)
    dce = ops.cross_entropy_bwd(zd, tok, gout, torch.empty(rows, K, device=DEV))
    bound = 2 * R.TOL * dce.abs().max(1, keepdim=True)[0]
    assert ((dl - dce).abs() <= bound).all()


def test_on_policy_ratio_is_exactly_one():
    K, rows, T, k, p, c = 512, 259, 0.9, 20, 0.9, 0.01
    z = _logits(rows + 13, K, seed=77)[13:]
    zd = torch.from_numpy(z).to(DEV)
    case = Case(z, zd, K, T, k, p, seed=78, clipped=False, adv_div=1, c=c)
    first = case.forward()
    inside = torch.isfinite(first["logprob"])
    assert inside.any() and (~inside).any()
    case.bd = torch.where(inside, first["logprob"], torch.zeros_like(first["logprob"]))      # b = logprob, bit for bit
    out = case.forward()
    ops.check_device_errors(DEV)
    assert torch.equal(_bits(out["logprob"]), _bits(first["logprob"])) and torch.equal(out["cut"], first["cut"])
    s = out["summary"].cpu().numpy()
    assert s[2] == 0.0 and s[3] == 0.0                               # approx_kl, clip_fraction: exactly 0
    assert abs(s[4] - (~inside).sum().item() / rows) <= 2.0 ** -24
    A = case.Ad.double()
    want = torch.where(inside, -A - float(np.float32(c)) * out["entropy"].double(), torch.zeros_like(A))   # rho = 1: l = -A - c H
    assert ((out["row_loss"].double() - want).abs() <= 2.0 ** -24 * want.abs()).all()
    gout = torch.tensor([1.0], device=DEV)
    dl_w = case.backward(out["cut"], gout, torch.float32)
    case_b, case.bd = case.bd, None
    dl_0 = case.backward(out["cut"], gout, torch.float32)            # the weighted form's gradient: g = -A as well
    case.bd = case_b
    assert torch.equal(_bits(dl_w), _bits(dl_0))
    assert (dl_w[~inside] == 0).all()


def test_a_rows_bits_depend_on_the_row_alone():
    """rows = 1 and rows = 5 (a single wave, a workgroup and a single wave) give the bits the same rows have in a larger launch."""
    K, rows, T, k, p = 512, 29, 0.7, 20, 0.9
    z = _logits(rows, K, seed=5)
    zd = torch.from_numpy(z).to(DEV)
    case = Case(z, zd, K, T, k, p, seed=6, clipped=True, adv_div=1, c=0.01)
    base = case.forward()
    gout = torch.tensor([0.5], device=DEV)
    dl = case.backward(base["cut"], gout, torch.float32)
    for n, r0 in ((1, 0), (1, 9), (5, 0), (5, 8)):
        sub = ops.policy_loss(zd[r0:r0 + n], case.tok[r0:r0 + n].contiguous(), case.Ad[r0:r0 + n].contiguous(), case.bd[r0:r0 + n].contiguous(),
                              temperature=T, top_k=k, top_p=p, clip_lo=CLIP[0], clip_hi=CLIP[1], entropy_coef=0.01)
        for name in ("row_loss", "logprob", "entropy", "cut"):
            assert torch.equal(_bits(sub[name]), _bits(base[name][r0:r0 + n])), (name, n, r0)
        want = sub["row_loss"].double().sum().item() / n
        assert np.isnan(want) and np.isnan(sub["summary"][0].item()) or abs(sub["summary"][0].item() - want) <= 2.0 ** -24 * abs(want) * (1 + 1e-6)
        g_n = torch.tensor([0.5 * n / rows], device=DEV)             # the same grad_out / rows: the same gradient rows
        sdl = ops.policy_loss_bwd(zd[r0:r0 + n], case.tok[r0:r0 + n].contiguous(), case.Ad[r0:r0 + n].contiguous(),
                                  case.bd[r0:r0 + n].contiguous(), sub["cut"], g_n, torch.empty(n, K, device=DEV), temperature=T,
                                  clip_lo=CLIP[0], clip_hi=CLIP[1], entropy_coef=0.01)
        bound = 2.0 ** -22 * dl[r0:r0 + n].abs()                     # (grad_out / rows itself is rounded differently: 2 roundings)
        assert torch.equal(torch.isnan(sdl), torch.isnan(dl[r0:r0 + n]))
        fin = ~torch.isnan(sdl)
        assert ((sdl - dl[r0:r0 + n]).abs()[fin] <= bound[fin]).all()
    ops.check_device_errors(DEV)


def test_token_out_of_range_surfaces_in_check_device_errors():
    K = 16
    z = torch.zeros(8, K, device=DEV)
    for bad in (K, -1):
        tok = torch.arange(8, device=DEV, dtype=torch.int64)
        tok[3] = bad
        out = ops.policy_loss(z, tok, torch.ones(8, device=DEV))
        with pytest.raises(ValueError, match="token out of range"):
            ops.check_device_errors(DEV)
        assert torch.allclose(out["row_loss"], torch.full((8,), float(np.log(K)), device=DEV))
        dl = ops.policy_loss_bwd(z, tok, torch.ones(8, device=DEV), None, out["cut"], torch.ones(1, device=DEV), torch.empty(8, K, device=DEV))
        assert torch.isfinite(dl).all()
    ops.check_device_errors(DEV)
