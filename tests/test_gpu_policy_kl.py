"""GPU: mage_policy_loss_anchored / mage_policy_loss_anchored_bwd against the plain pair bit for bit where the rule says so, and against the
fp64 restatement (tests/policy_kl_ref.py on tests/policy_ref.py) evaluated with the kept set and the fp32 log-probabilities the kernel itself
reports.  The plain pair is pinned in tests/test_gpu_policy_loss.py; what is new here is the anchor.

Inputs.  259 rows (64 workgroups of 4 waves and a ragged last one) without special logits, tokens chosen on the CPU: a member of the exact
kept set, except every seventh row (a uniform token, which a filter mostly cannot draw: the outside rows) and seven peaked rows whose
token holds all the mass in fp32 (|logprob| < 1e-5: 0, or the rounding residue of z_t / T), so that d = r - logprob can be as small as 2^-40.  The reference
log-probabilities are r = fp32(logprob + d) from the kernel's own logprob with d from +-{0, 2^-40, 1e-12, 1e-7, 1e-3, 0.5, 5, 20, 80}: exact
copies (d = 0), eight -inf, one +inf and one NaN (the unanchored rows, 3.9 %).  make_case's token choice is checked against the caps
(outside <= 25 %, unanchored <= 10 %) with the restatement alone by tests/test_policy_kl_ref_cpu.py's
test_gpu_case_recipe_keeps_the_caps, and every launch asserts both on the kernel's own outputs.

Bounds, per row, extending tests/test_gpu_policy_loss.py's.
  kl against kl_term(fp32(r - logprob)) of the kernel's own logprob: 1 fp32 ulp of the value -- the kernel's fp64 value is within 2^-40 of it
    (tests/test_policy_kl_ref_cpu.py), then one rounding.
  row_loss: the kernel rounds l_plain + kl_coef kl once from fp64.  Its error is l_plain's input error -- rho's, which that file bounds
    together with l_plain's own final rounding by (4 + |logprob - b|) 2^-23 |l_plain| -- plus what the final rounding gains from the second
    term, 2^-24 kl_coef kl (|l| <= |l_plain| + kl_coef kl; the fp64 error of the KL part, 2^-40 relative, goes into a (1 + 2^-10) factor).
    The bound is stated on the two magnitudes, not on |l|: the parts may cancel.
  dlogits: g = fp32(g_plain + kl_coef (1 - exp(d))) is one more rounding (2^-24) of a sum whose parts may cancel, and the gradient is linear in
    g, so the row is want_plain + kl_coef (1 - exp(d)) unit with unit = scale inv_t (1[j = t] - p_j); that file's 2 TOL max_j |.| allowance
    for the fixed-order fp32 mass sums is taken on |want_plain_j| + |extra_j| (2^-24 is far inside TOL = 1e-5); bf16 adds 2^-8 |want_j|, the
    floor is 2^-126.  (1 - exp(d)) uses the kernel's own fp32 d, as kl does: a peaked row's fp32 logprob is 1e-9 and more away from its
    fp64 value, which would be the whole of a d = 1e-12.
  summary: the fp64 means of the kernel's own per-row outputs, one fp32 rounding, 2^-24 relative.
Bit for bit: logprob, entropy, cut equal the plain call's always; rows with d == 0 and unanchored rows carry the plain call's row_loss and
dlogits row for kl_coef = 0.37; with kl_coef = 0 every row does; two launches agree; rows = 1 and 5 give the bits the rows have inside 259."""
import numpy as np
import pytest
import torch

from mage_amd import ops
from tests import helpers as H
from tests import policy_kl_ref as Q
from tests import policy_ref as P
from tests import sampling_ref as S
from tests import token_stats_ref as R
from tests.test_gpu_policy_loss import CLIP, _bits, _keys, _logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, KL_COEF, ENT = 259, 0.37, 0.01
FILTERS = [(0, 1.0), (20, 1.0), (0, 0.9), (20, 0.9)]
PEAKED = list(range(5, ROWS, 40))                                   # 7 rows: the token holds all the mass
MINUS_INF, PLUS_INF, A_NAN = list(range(9, ROWS, 32)), [200], [100]
WORST = {}


def make_case(K, k, p, T, seed):
    """(z fp32 [ROWS, K], tokens, exact kept sets): everything that is decided on the CPU."""
    g = np.random.default_rng(seed)
    z = _logits(ROWS + 13, K, seed)[13:].copy()
    k = min(k, K // 2)
    tok = np.zeros(ROWS, np.int64)
    for r in PEAKED:
        z[r, int(np.argmax(z[r]))] = z[r].max() + (30.0, 40.0, 60.0)[(r // 40) % 3] * max(T, 1.0)
    sets = [R.exact_set(z[r], T, k, p) for r in range(ROWS)]
    for r in range(ROWS):
        if r in PEAKED:
            tok[r] = int(np.argmax(z[r]))
        elif r % 7 == 3:
            tok[r] = int(g.integers(0, K))
        else:
            tok[r] = int(g.choice(np.flatnonzero(sets[r] & np.isfinite(z[r]))))
    return z, tok, sets, k


def reference_logprobs(lp32):
    """r = fp32(logprob + d) from the kernel's own logprob, d by the row's place; the unanchored rows on top."""
    r = np.empty(ROWS, np.float32)
    small, wide = [0.0, 2.0 ** -40, 1e-12, 1e-7], [0.0, 1e-3, 0.5, 5.0, 20.0, 80.0, 1e-7]
    for i in range(ROWS):
        mags = small if i in PEAKED else wide
        d = mags[(i // (40 if i in PEAKED else 1)) % len(mags)] * (1.0 if (i // 3) % 2 == 0 else -1.0)
        r[i] = np.float32(-1.0) if not np.isfinite(lp32[i]) else np.float32(lp32[i]) + np.float32(d)
    r[MINUS_INF], r[PLUS_INF], r[A_NAN] = -np.inf, np.inf, np.nan
    return r


def _advantages(seed):
    g = np.random.default_rng(seed)
    return (g.uniform(0.5, 2.0, ROWS) * g.choice([-1.0, 1.0], ROWS)).astype(np.float32)


def _behaviour(lp32, cmin, cmax, seed):
    """tests/test_gpu_policy_loss.py's recipe: rho on both sides of the clip range and inside it, never within 1e-3 of an edge."""
    g = np.random.default_rng(seed)
    lp = lp32.astype(np.float64)
    b = (np.where(np.isfinite(lp), lp, 0.0) + g.choice([-0.35, -0.1, 0.1, 0.35], ROWS) * g.uniform(0.8, 1.0, ROWS)).astype(np.float32)
    for _ in range(4):
        with np.errstate(invalid="ignore", over="ignore"):
            rho = np.exp(lp - b.astype(np.float64))
            near = (np.abs(rho / cmin - 1) < 1e-3) | (np.abs(rho / cmax - 1) < 1e-3)
        b[near] += np.float32(0.01)
    assert not near.any()
    return b


def _fwd(zd, tok, A, b, T, k, p, ref=None, kc=0.0, c=ENT):
    return ops.policy_loss(zd, tok, A, b, temperature=T, top_k=k, top_p=p, clip_lo=CLIP[0], clip_hi=CLIP[1], entropy_coef=c, adv_div=1,
                           reference_logprob=ref, kl_coef=kc)


def _bwd(zd, tok, A, b, cut, gout, dt, T, ref=None, kc=0.0, c=ENT):
    dl = torch.empty(zd.shape[0], zd.shape[1], device=DEV, dtype=dt)
    return ops.policy_loss_bwd(zd, tok, A, b, cut, gout, dl, temperature=T, clip_lo=CLIP[0], clip_hi=CLIP[1], entropy_coef=c, adv_div=1,
                               reference_logprob=ref, kl_coef=kc)


def _raw(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def _check_summary(out, r32, rows):
    lp = out["logprob"].cpu().numpy().astype(np.float64)
    inside = ~np.isneginf(lp)
    return inside, np.array([out["row_loss"].cpu().numpy().astype(np.float64)[inside].sum(),
                             out["entropy"].cpu().numpy().astype(np.float64)[inside].sum(), 0.0, 0.0, float((~inside).sum()),
                             out["kl"].cpu().numpy().astype(np.float64)[inside].sum(), float((inside & ~np.isfinite(r32)).sum())]) / rows


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
@pytest.mark.parametrize("k,p", FILTERS)
def test_anchored_kernels_match_the_plain_pair_and_the_restatement(K, k, p):
    T = (0.7, 1.0, 1.5)[(K + k) % 3]
    seed = K + k + int(10 * p)
    z, tok_np, _, k = make_case(K, k, p, T, seed)
    zd, tok = torch.from_numpy(z).to(DEV), torch.from_numpy(tok_np).to(DEV)
    A_np = _advantages(seed + 1)
    A = torch.from_numpy(A_np).to(DEV)
    cmin, cmax = P.clip_bounds(*CLIP)
    first = _fwd(zd, tok, A, None, T, k, p)
    lp32 = first["logprob"].cpu().numpy()
    r32 = reference_logprobs(lp32)
    ref = torch.from_numpy(r32).to(DEV)
    b_np = _behaviour(lp32, cmin, cmax, seed + 3)
    cut = first["cut"].cpu().numpy().view(np.uint32)
    keep = _keys((z * S.inv_temperature(T)).astype(np.float32)) >= cut[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        d32 = (r32 - lp32).astype(np.float64)                       # the kernel's d: one fp32 subtraction
    inside = ~np.isneginf(lp32)
    anchored = inside & np.isfinite(r32)
    same = ~anchored | (d32 == 0)                                   # rows that must carry the plain call's bits
    assert (~inside).sum() <= ROWS // 4 and (inside & ~np.isfinite(r32)).sum() <= ROWS // 10           # the caps, on the kernel's outputs
    assert (np.abs(lp32[PEAKED]) < 1e-5).all() and (anchored & (d32 == 0)).sum() >= 8 and (np.abs(d32[anchored & (d32 != 0)]).min() < 1e-11)
    kc32, c32 = float(np.float32(KL_COEF)), float(np.float32(ENT))
    gout = torch.tensor([0.7], device=DEV)
    scale = float(np.float32(0.7)) / ROWS
    for b in (None, b_np):
        bd = None if b is None else torch.from_numpy(b).to(DEV)
        plain, out, again, zero = (_fwd(zd, tok, A, bd, T, k, p), _fwd(zd, tok, A, bd, T, k, p, ref, KL_COEF),
                                   _fwd(zd, tok, A, bd, T, k, p, ref, KL_COEF), _fwd(zd, tok, A, bd, T, k, p, ref, 0.0))
        ops.check_device_errors(DEV)
        assert out["summary"].shape == (7,) and plain["summary"].shape == (5,) and "kl" not in plain
        for n in out:
            assert torch.equal(_bits(out[n]), _bits(again[n])), n                                  # two launches, the same bits
        for n in ("logprob", "entropy", "cut"):
            assert torch.equal(_bits(out[n]), _bits(plain[n])) and torch.equal(_bits(zero[n]), _bits(plain[n])), n
        assert torch.equal(_bits(zero["row_loss"]), _bits(plain["row_loss"]))                      # kl_coef = 0: the plain call's bits
        assert torch.equal(_bits(zero["kl"]), _bits(out["kl"])) and torch.equal(_bits(zero["summary"][:5]), _bits(plain["summary"]))
        sm = torch.from_numpy(same).to(DEV)
        assert torch.equal(_bits(out["row_loss"])[sm], _bits(plain["row_loss"])[sm])               # d = 0 and unanchored rows
        kl = out["kl"].cpu().numpy().astype(np.float64)
        loss, loss_plain = out["row_loss"].cpu().numpy().astype(np.float64), plain["row_loss"].cpu().numpy().astype(np.float64)
        h32 = out["entropy"].cpu().numpy().astype(np.float64)
        assert (kl[~anchored] == 0).all() and (kl[anchored & (d32 == 0)] == 0).all() and (kl >= 0).all()
        terms = []
        for r in range(ROWS):
            br = None if b is None else float(b[r])
            t = Q.term(float(lp32[r]), h32[r], float(A_np[r]), br, float(r32[r]), cmin, cmax, c32, kc32)
            t0 = P.term(float(lp32[r]), h32[r], float(A_np[r]), br, cmin, cmax, c32)
            terms.append((t, t0))
            if anchored[r]:
                want = Q.kl_term(d32[r])
                ulp = float(np.spacing(np.float32(want)))
                assert abs(kl[r] - want) <= ulp, f"row {r}: kl {kl[r]!r} want {want!r} (d = {d32[r]!r})"
                _note("kl", abs(kl[r] - want) / ulp)
            bound = ((4 + (abs(lp32[r] - br) if br is not None and not t["outside"] else 0.0)) * 2.0 ** -23 * abs(t0["loss"])
                     + 2.0 ** -24 * (1 + 2.0 ** -10) * kc32 * t["kl"])
            assert abs(loss[r] - t["loss"]) <= bound, f"row {r}: row_loss {loss[r]!r} want {t['loss']!r} bound {bound:.3e}"
            if bound:
                _note("row_loss", abs(loss[r] - t["loss"]) / bound)
            if t["outside"]:
                assert loss[r] == 0.0 and kl[r] == 0.0
        # summary: the fp64 means of the kernel's own outputs
        ins, want = _check_summary(out, r32, ROWS)
        if b is not None:
            want[2] = (b.astype(np.float64)[ins] - lp32.astype(np.float64)[ins]).sum() / ROWS
            want[3] = sum(t0["off"] for _, t0 in terms) / ROWS
        got = out["summary"].cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        assert (err <= 2.0 ** -24 * np.abs(want) * (1 + 1e-6)).all(), (got, want)
        _note("summary", (err[want != 0] / (2.0 ** -24 * np.abs(want[want != 0]))).max())
        # the gradient
        for dt in (torch.float32, torch.bfloat16):
            dl, dl2 = _bwd(zd, tok, A, bd, out["cut"], gout, dt, T, ref, KL_COEF), _bwd(zd, tok, A, bd, out["cut"], gout, dt, T, ref, KL_COEF)
            dl_plain, dl_zero = _bwd(zd, tok, A, bd, out["cut"], gout, dt, T), _bwd(zd, tok, A, bd, out["cut"], gout, dt, T, ref, 0.0)
            assert torch.equal(_raw(dl), _raw(dl2)) and torch.equal(_raw(dl_zero), _raw(dl_plain))
            assert torch.equal(_raw(dl)[sm], _raw(dl_plain)[sm])
            got_dl = dl.float().cpu().numpy().astype(np.float64)
            for r in range(ROWS):
                t, t0 = terms[r]
                if t["outside"] or not keep[r][tok_np[r]]:
                    assert (got_dl[r] == 0).all(), r
                    continue
                br = None if b is None else float(b[r])
                plain_w = P.dlogits_row(z[r], int(tok_np[r]), float(A_np[r]), br, T, keep[r], cmin, cmax, c32, scale)
                extra = np.zeros(K)
                if anchored[r] and d32[r] != 0:
                    extra = kc32 * Q.grad_factor(d32[r]) * P.dlogits_row(z[r], int(tok_np[r]), -1.0, None, T, keep[r], cmin, cmax, 0.0, scale)
                want_dl = plain_w + extra
                assert (got_dl[r][~keep[r]] == 0).all(), r
                bound = 2 * R.TOL * (np.abs(plain_w) + np.abs(extra)).max() + (2.0 ** -8 * np.abs(want_dl) if dt == torch.bfloat16 else 0.0) \
                    + 2.0 ** -126
                e = np.abs(got_dl[r] - want_dl)
                assert (e <= bound).all(), f"row {r} (d = {d32[r]!r}): dlogits |d| {e.max():.3e} > bound (row max {np.abs(want_dl).max():.3e})"
                _note("dlogits", (e / bound).max())
    print(f"K={K} top_k={k} top_p={p}: {(~inside).sum()} outside, {(inside & ~np.isfinite(r32)).sum()} unanchored rows; largest error / bound "
          "so far: " + ", ".join(f"{a} {v:.3f}" for a, v in WORST.items()))


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
def test_a_rows_bits_depend_on_the_row_alone(K):
    """rows = 1 and rows = 5 (a single wave; a workgroup and a single wave) give the bits the same rows have among 259, and their own summary."""
    T, (k, p) = 0.7, FILTERS[3]
    z, tok_np, _, k = make_case(K, k, p, T, seed=K + 7)
    zd, tok = torch.from_numpy(z).to(DEV), torch.from_numpy(tok_np).to(DEV)
    A = torch.from_numpy(_advantages(K + 8)).to(DEV)
    lp32 = _fwd(zd, tok, A, None, T, k, p)["logprob"].cpu().numpy()
    r32 = reference_logprobs(lp32)
    ref = torch.from_numpy(r32).to(DEV)
    bd = torch.from_numpy(_behaviour(lp32, *P.clip_bounds(*CLIP), K + 10)).to(DEV)
    base = _fwd(zd, tok, A, bd, T, k, p, ref, KL_COEF)
    gout = torch.tensor([0.5], device=DEV)
    dl = _bwd(zd, tok, A, bd, base["cut"], gout, torch.float32, T, ref, KL_COEF)
    for n, r0 in ((1, 5), (1, 9), (1, 3), (5, 0), (5, 6), (5, 98)):         # a peaked row, an unanchored one, a uniform token; spans with each
        sl = slice(r0, r0 + n)
        args = (zd[sl], tok[sl].contiguous(), A[sl].contiguous(), bd[sl].contiguous())
        sub = _fwd(*args, T, k, p, ref[sl].contiguous(), KL_COEF)
        for name in ("row_loss", "logprob", "entropy", "cut", "kl"):
            assert torch.equal(_bits(sub[name]), _bits(base[name][sl])), (name, n, r0)
        _, want = _check_summary(sub, r32[sl], n)
        got = sub["summary"].cpu().numpy().astype(np.float64)
        for q in (0, 1, 4, 5, 6):
            assert abs(got[q] - want[q]) <= 2.0 ** -24 * abs(want[q]) * (1 + 1e-6), (n, r0, q, got, want)
        g_n = torch.tensor([0.5 * n / ROWS], device=DEV)             # the same grad_out / rows: the same gradient rows
        sdl = _bwd(*args, sub["cut"], g_n, torch.float32, T, ref[sl].contiguous(), KL_COEF)
        assert ((sdl - dl[sl]).abs() <= 2.0 ** -22 * dl[sl].abs()).all()   # (grad_out / rows itself is rounded differently: 2 roundings)
    ops.check_device_errors(DEV)


@pytest.mark.parametrize("rows", [1, 5, 259])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_nothing_is_written_around_the_outputs(rows, dt):
    """Every output sits inside a sentinel-filled buffer, 8 elements clear of either end; the raw entry points write the rows and nothing else."""
    K, T, (k, p) = 260, 1.3, FILTERS[3]
    z, tok_np, _, k = make_case(K, k, p, T, seed=17)
    zd, tok = torch.from_numpy(z[:rows]).to(DEV), torch.from_numpy(tok_np[:rows]).to(DEV)
    A = torch.from_numpy(_advantages(18)[:rows]).to(DEV)
    ref = torch.full((rows,), -1.5, device=DEV)
    l, s = H.lib()
    pad = 8
    bufs = {n: H.sent(sz + 2 * pad, d) for n, sz, d in (("row_loss", rows, torch.float32), ("logprob", rows, torch.float32),
                                                        ("entropy", rows, torch.float32), ("cut", rows, torch.float32),
                                                        ("kl", rows, torch.float32), ("summary", 7, torch.float32), ("dl", rows * K, dt))}
    o = {n: b[pad:b.numel() - pad] for n, b in bufs.items()}
    rc = l.mage_policy_loss_anchored(zd.data_ptr(), rows, K, K, tok.data_ptr(), A.data_ptr(), 1, None, ref.data_ptr(), T, k, p, 0.2, 0.2, ENT,
                                     KL_COEF, o["row_loss"].data_ptr(), o["logprob"].data_ptr(), o["entropy"].data_ptr(), o["cut"].data_ptr(),
                                     o["kl"].data_ptr(), o["summary"].data_ptr(), s)
    assert rc == 0
    gout = torch.ones(1, device=DEV)
    rc = l.mage_policy_loss_anchored_bwd(zd.data_ptr(), rows, K, K, tok.data_ptr(), A.data_ptr(), 1, None, ref.data_ptr(), o["cut"].data_ptr(), T,
                                         0.2, 0.2, ENT, KL_COEF, gout.data_ptr(), o["dl"].data_ptr(), ops.code(o["dl"]), s)
    assert rc == 0
    ops.check_device_errors(DEV)
    for n, b in bufs.items():
        assert H.untouched(b[:pad]) and H.untouched(b[b.numel() - pad:]), n
        if n != "cut":                                              # (a threshold may take any bit pattern)
            assert H.written(o[n]), n
    want = ops.policy_loss(zd, tok, A, None, temperature=T, top_k=k, top_p=p, entropy_coef=ENT, reference_logprob=ref, kl_coef=KL_COEF)
    for n in ("row_loss", "logprob", "entropy", "kl", "summary"):
        assert torch.equal(_bits(o[n]), _bits(want[n])), n
