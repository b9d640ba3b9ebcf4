"""CPU: the reference-policy KL penalty -- the fp64 restatement (tests/policy_kl_ref.py) against 60-digit values and against central finite
differences of its own loss, the cases that pin its rule (each names the mistake it catches), the four new extension entry points in the
header and the binding table, and their argument checks (refused before anything is launched).

Bounds.
  kl_term / grad_factor against mpmath: relative 2^-40.  The fp64 forms lose at most 9 bits to the one subtraction expm1(d) - d at
    |d| = 2^-8 (2^-44) and 2^-51 to the series' truncation below it, plus a few fp64 roundings and libm's expm1 (< 1 ulp): 2^-40 leaves 16x
    room and is still 2^16 below one fp32 ulp, which is what the kernel's header promises.
  finite differences: central, step h = 1e-5 in the logit, per row (a row's loss reads its own logits only).  With scale = 0.7 / n, |A| < 3,
    kl_coef = 0.3 and |d| <= 2 a row's scaled loss f stays below 0.5 and its third derivative below 1, so the truncation error
    h^2 |f'''| / 6 is below 2e-11 and the rounding error 2^-52 |f| / h below 2e-11 as well; the bound is 1e-9.
"""
import math
import os
import re

import mpmath
import numpy as np
import pytest

from mage_amd import _lib
from tests import policy_kl_ref as Q
from tests import policy_ref as P
from tests import sampling_ref as S
from tests import token_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan
D_LIST = [0.0, 2.0 ** -40, 1e-12, 1e-7, 1e-3, 0.5, 5.0, 20.0, 80.0]


def _rel(got, want):
    if want == 0:
        return 0.0 if got == 0 else INF
    return float(abs((mpmath.mpf(got) - want) / want))


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("mag", D_LIST)
def test_restated_kl_and_factor_match_sixty_digits(mag, sign):
    d = sign * mag
    assert _rel(Q.kl_term(d), Q.kl_term_mp(d)) <= 2.0 ** -40
    assert _rel(Q.grad_factor(d), Q.grad_factor_mp(d)) <= 2.0 ** -40
    assert Q.kl_term(d) >= 0.0 and (Q.kl_term(d) == 0.0) == (d == 0.0)
    if 0 < mag <= 1e-7:
        # why the route matters: the plain fp64 form loses everything (relative error far above an fp32 ulp) where the series does not
        assert _rel(math.exp(d) - d - 1, Q.kl_term_mp(d)) > 2.0 ** -24


def test_restated_kl_and_factor_match_sixty_digits_at_random_d():
    g = np.random.default_rng(11)
    mags = np.exp(g.uniform(np.log(1e-13), np.log(85.0), 1000))
    mags[:200] = np.float32(g.uniform(2.0 ** -9, 2.0 ** -7, 200))          # around the switch between the series and expm1(d) - d
    worst = 0.0
    for d in mags * g.choice([-1.0, 1.0], 1000):
        d = float(np.float32(d))                                           # the kernel's d is an fp32 value
        worst = max(worst, _rel(Q.kl_term(d), Q.kl_term_mp(d)), _rel(Q.grad_factor(d), Q.grad_factor_mp(d)))
    print(f"largest relative error of the fp64 forms: 2^{np.log2(worst):.1f}")
    assert worst <= 2.0 ** -40


def test_overflow_and_nan_follow_the_arithmetic():
    assert Q.kl_term(800.0) == INF and Q.grad_factor(800.0) == -INF
    assert abs(Q.kl_term(-800.0) - 799.0) < 1e-12 and Q.grad_factor(-800.0) == 1.0
    assert np.isnan(Q.kl_term(NAN)) and np.isnan(Q.grad_factor(NAN))


# ------------------------------------------------------------------------------------------------ the analytic gradient
def _row_loss64(s, N, t, A, b, r, cmin, cmax, c, kl_coef):
    """One row's loss as a smooth fp64 function of its scaled logits s (the kept set N a constant mask)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = s - s[N].max()
        w = np.where(N, np.exp(d), 0.0)
        Z = w.sum()
        logp = d - np.log(Z)
        p = w / Z
        H = -np.where(p > 0, p * logp, 0.0).sum()
    lp = logp[t]
    if b is None:
        l = -A * lp - c * H
    else:
        rho = np.exp(lp - b)
        l = -min(rho * A, min(max(rho, cmin), cmax) * A) - c * H
    if np.isfinite(r):
        l += kl_coef * Q.kl_term(r - lp)
    return l


@pytest.mark.parametrize("K", [8, 260])
@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.5, 0, 0.9), (1.3, 5, 0.9)])
@pytest.mark.parametrize("clipped", [False, True])
def test_analytic_dlogits_is_the_finite_difference_of_the_loss(K, T, k, p, clipped):
    n, c, kl_coef, h = 12, 0.05, 0.3, 1e-5
    g = np.random.default_rng(K + k + int(10 * p) + 100 * clipped)
    z = (2.0 * g.standard_normal((n, K))).astype(np.float32)
    z[::3] = np.round(z[::3] * 4) / 4
    z[1, 3:6] = -INF
    tok = g.integers(0, K, n)
    idx = np.arange(n)
    A = np.abs(g.standard_normal(n)) * np.where((idx // 2) % 2 == 0, 1.0, -1.0)
    sets = [R.exact_set(z[r], T, k, p) for r in range(n)]
    for r in range(n):
        if r % 4 != 3:                                              # three rows in four: a token the policy can draw
            tok[r] = int(np.argmax(np.where(sets[r], z[r], -INF)) if r % 2 else g.choice(np.flatnonzero(sets[r] & np.isfinite(z[r]))))
        elif not sets[r].all():                                     # the fourth: one the filter cannot draw (an outside row)
            tok[r] = int(g.choice(np.flatnonzero(~sets[r])))
    cmin, cmax = P.clip_bounds(0.2, 0.3)
    lp = np.array([R.stats_for_set(z[r], int(tok[r]), T, 0, sets[r])["policy_logprob"] for r in range(n)])
    lp0 = np.where(np.isfinite(lp), lp, 0.0)
    b = None
    if clipped:                                                     # rho on both sides of [0.8, 1.3] and inside it, never near an edge
        off = np.where((idx // 4) % 2 == 0, 0.35, -0.35) * g.uniform(0.9, 1.0, n)
        off[n // 2:] *= 0.3
        b = lp0 + off
    ref = lp0 + np.array([0.0, 1e-3, -1e-3, 0.5, -0.5, 2.0, -2.0, 0.25, -INF, NAN, 1.0, -1.0])[:n]       # rows 8, 9: unanchored
    scale, inv_t = 0.7 / n, float(S.inv_temperature(T))
    seen = set()
    for r in range(n):
        t, N, br = int(tok[r]), sets[r], None if b is None else b[r]
        got = Q.dlogits_row(z[r], t, A[r], br, ref[r], T, N, cmin, cmax, c, kl_coef, scale)
        rr = Q.row(z[r], t, A[r], br, ref[r], T, N, cmin, cmax, c, kl_coef)
        seen.add((rr["outside"], rr["unanchored"]))
        if rr["outside"]:
            assert (got == 0).all() and rr["loss"] == 0.0 and rr["kl"] == 0.0
            continue
        s = R.scaled(z[r], T).astype(np.float64)
        assert abs(rr["loss"] - _row_loss64(s, N, t, A[r], br, ref[r], cmin, cmax, c, kl_coef)) < 1e-12
        cols = np.flatnonzero(np.isfinite(z[r]))
        for j in (cols if K <= 8 else np.unique(np.concatenate([[t], cols[:: max(1, len(cols) // 24)]]))):
            e = np.zeros(K)
            e[j] = h * inv_t                                        # z_j + h moves s_j by h * inv_t
            fd = scale * (_row_loss64(s + e, N, t, A[r], br, ref[r], cmin, cmax, c, kl_coef) -
                          _row_loss64(s - e, N, t, A[r], br, ref[r], cmin, cmax, c, kl_coef)) / (2 * h)
            want = fd if N[j] else 0.0                              # (outside the set the mask is the constant, not the logit)
            assert abs(got[j] - want) < 1e-9, (r, j, got[j], want)
        assert (got[~N] == 0).all()
    assert seen >= {(False, False), (False, True)} and (k == 0 and p == 1.0 or (True, False) in seen)


# ------------------------------------------------------------------------------------------------ the rule, case by case
CM = P.clip_bounds(0.2, 0.2)


def test_d_is_reference_minus_policy_not_the_reverse():
    """Catches the sign of d flipped: exp(0.5) - 1.5 = 0.1487 against exp(-0.5) - 0.5 = 0.1065."""
    t = Q.term(-1.0, 0.3, 2.0, None, -0.5, *CM, 0.0, 0.25)
    assert abs(t["kl"] - (math.exp(0.5) - 1.5)) < 1e-15
    assert abs(t["loss"] - (2.0 + 0.25 * (math.exp(0.5) - 1.5))) < 1e-15


def test_gradient_factor_is_one_minus_exp_d():
    """Catches exp(d) - 1 used for the factor: with the reference ABOVE the policy (d > 0) the penalty must push logprob UP, g < 0."""
    t = Q.term(-1.0, 0.3, 0.0, None, -0.5, *CM, 0.0, 0.25)
    assert abs(t["g"] - 0.25 * (1.0 - math.exp(0.5))) < 1e-15 and t["g"] < 0
    t = Q.term(-1.0, 0.3, 0.0, None, -1.5, *CM, 0.0, 0.25)
    assert abs(t["g"] - 0.25 * (1.0 - math.exp(-0.5))) < 1e-15 and t["g"] > 0
    # and the clip switching the surrogate's gradient off leaves the KL gradient standing
    t = Q.term(-1.0, 0.3, 2.0, -2.0, -0.5, *CM, 0.0, 0.25)          # rho = e > 1.2 with A > 0: off
    assert t["off"] and abs(t["g"] - 0.25 * (1.0 - math.exp(0.5))) < 1e-15


def test_outside_rows_get_no_kl_term():
    """Catches the KL term added to outside rows (where d = r + inf would make it infinite)."""
    t = Q.term(-INF, 0.3, 2.0, None, -0.5, *CM, 0.1, 0.25)
    assert t["outside"] and t["loss"] == 0.0 and t["g"] == 0.0 and t["kl"] == 0.0 and not t["unanchored"]
    z = np.log(np.array([0.5, 0.3, 0.15, 0.05])).astype(np.float32)
    N = R.exact_set(z, 1.0, 2, 1.0)
    assert (Q.dlogits_row(z, 3, 2.0, None, -0.5, 1.0, N, *CM, 0.1, 0.25, 1.0) == 0).all()


@pytest.mark.parametrize("r", [-INF, INF, NAN])
def test_an_unanchored_row_contributes_nothing(r):
    """Catches an unanchored row contributing: a reference value that is not finite leaves policy_ref's row, counted in its own share."""
    t, base = Q.term(-1.0, 0.3, 2.0, -1.1, r, *CM, 0.1, 0.25), P.term(-1.0, 0.3, 2.0, -1.1, *CM, 0.1)
    assert t["unanchored"] and t["kl"] == 0.0 and t["loss"] == base["loss"] and t["g"] == base["g"]
    z = np.log(np.array([0.5, 0.3, 0.15, 0.05])).astype(np.float32)
    N = np.ones(4, bool)
    assert np.array_equal(Q.dlogits_row(z, 1, 2.0, None, r, 1.0, N, *CM, 0.1, 0.25, 1.0), P.dlogits_row(z, 1, 2.0, None, 1.0, N, *CM, 0.1, 1.0))


def test_exact_copies_and_a_zero_weight_leave_the_plain_row():
    for lp in (-1.0, -1e-9, -30.0):
        t, base = Q.term(lp, 0.3, 2.0, lp - 0.1, lp, *CM, 0.1, 0.25), P.term(lp, 0.3, 2.0, lp - 0.1, *CM, 0.1)
        assert t["kl"] == 0.0 and t["loss"] == base["loss"] and t["g"] == base["g"] and not t["unanchored"]
    t, base = Q.term(-1.0, 0.3, 2.0, None, -0.5, *CM, 0.1, 0.0), P.term(-1.0, 0.3, 2.0, None, *CM, 0.1)
    assert t["kl"] > 0 and t["loss"] == base["loss"] and t["g"] == base["g"]


def test_the_kl_mean_divides_by_all_rows():
    """Catches the KL mean divided by the inside rows: two of four rows are outside."""
    def mk(lp, r):                                                  # (summary reads row(...)'s logprob and entropy beside the term)
        return dict(logprob=lp, entropy=0.3, **Q.term(lp, 0.3, 1.0, None, r, *CM, 0.0, 0.5)), 0.0
    rows = [mk(-1.0, -0.5), mk(-INF, -0.5), mk(-2.0, NAN), mk(-INF, NAN)]
    s = Q.summary(rows, False)
    k = math.exp(0.5) - 1.5
    assert s.shape == (7,) and abs(s[5] - k / 4) < 1e-16 and s[6] == 0.25 and s[4] == 0.5
    assert abs(s[0] - (1.0 + 0.5 * k + 2.0) / 4) < 1e-15                    # the loss mean includes the KL term


# ------------------------------------------------------------------------------------------------ the library's surface
NEW = ("mage_policy_loss_anchored", "mage_policy_loss_anchored_bwd", "mage_sumsq", "mage_adam_clipped")


def test_header_and_table_name_the_four_entry_points():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", header, flags=re.M))
    assert set(NEW) <= declared and declared == set(_lib.EXT_SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    for name in NEW:
        res, args = _lib.EXT_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        n_decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1).count(",") + 1
        assert n_decl == len(args), name
    # the plain pair keeps its signatures
    assert len(_lib.EXT_SIGNATURES["mage_policy_loss"][1]) == 20 and len(_lib.EXT_SIGNATURES["mage_policy_loss_bwd"][1]) == 17


PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched
FWD_ORDER = ("logits", "rows", "K", "ld", "tokens", "advantage", "adv_div", "behaviour_logprob", "reference_logprob", "temperature", "top_k",
             "top_p", "clip_lo", "clip_hi", "entropy_coef", "kl_coef", "row_loss", "logprob", "entropy", "cut", "kl", "summary")
BWD_ORDER = ("logits", "rows", "K", "ld", "tokens", "advantage", "adv_div", "behaviour_logprob", "reference_logprob", "cut", "temperature",
             "clip_lo", "clip_hi", "entropy_coef", "kl_coef", "grad_out", "dlogits", "dl_dtype")
GOOD = dict(logits=PTR, rows=8, K=512, ld=512, tokens=PTR, advantage=PTR, adv_div=4, behaviour_logprob=PTR, reference_logprob=PTR,
            temperature=1.0, top_k=20, top_p=0.9, clip_lo=0.2, clip_hi=0.2, entropy_coef=0.01, kl_coef=0.1, row_loss=PTR, logprob=PTR,
            entropy=PTR, cut=PTR, kl=PTR, summary=PTR, grad_out=PTR, dlogits=PTR, dl_dtype=_lib.BF16)
ANCHOR_BAD = [dict(reference_logprob=None), dict(reference_logprob=PTR + 2), dict(kl_coef=-0.1), dict(kl_coef=NAN), dict(kl_coef=INF),
              dict(logits=None), dict(K=6, ld=8), dict(rows=0), dict(temperature=0.0), dict(clip_lo=1.5), dict(entropy_coef=NAN)]


@pytest.mark.parametrize("bad", ANCHOR_BAD + [dict(kl=None), dict(top_k=1), dict(summary=None)])
def test_anchored_loss_refuses_bad_arguments(bad):
    a = {**GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_policy_loss_anchored(*[a[k] for k in FWD_ORDER], None)
    msg = lib.mage_last_error().decode()
    assert rc == -1 and "mage_policy_loss_anchored" in msg and "mage_init" not in msg, (bad, rc, msg)


@pytest.mark.parametrize("bad", ANCHOR_BAD + [dict(grad_out=None), dict(dlogits=PTR + 8), dict(dl_dtype=_lib.F16)])
def test_anchored_bwd_refuses_bad_arguments(bad):
    a = {**GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_policy_loss_anchored_bwd(*[a[k] for k in BWD_ORDER], None)
    assert rc == -1 and "mage_policy_loss_anchored_bwd" in lib.mage_last_error().decode(), (bad, rc)


def test_anchored_loss_accepts_what_the_rule_allows():
    """The accepted forms get past the argument rules: without an initialised device the forward call stops at the mage_init check behind them."""
    lib = _lib.load()
    for ok in (dict(), dict(kl_coef=0.0), dict(behaviour_logprob=None), dict(reference_logprob=PTR + 4), dict(kl_coef=1e30)):
        a = {**GOOD, **ok}
        rc = lib.mage_policy_loss_anchored(*[a[k] for k in FWD_ORDER], None)
        assert rc == -1 and "mage_init" in lib.mage_last_error().decode(), (ok, rc, lib.mage_last_error())


ADAM_ORDER = ("p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "sumsq", "max_norm", "norm_out")
ADAM_GOOD = dict(p=PTR, g=PTR, m=PTR, v=PTR, n=64, lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, step=1, grad_scale=1.0, sumsq=PTR, max_norm=1.0,
                 norm_out=PTR)


@pytest.mark.parametrize("bad", [dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=NAN), dict(max_norm=INF), dict(sumsq=None),
                                 dict(sumsq=PTR + 4), dict(norm_out=PTR + 2), dict(n=0), dict(step=0), dict(p=None), dict(g=PTR + 4)])
def test_adam_clipped_refuses_bad_arguments(bad):
    a = {**ADAM_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_adam_clipped(*[a[k] for k in ADAM_ORDER], None)
    assert rc == -1 and "mage_adam_clipped" in lib.mage_last_error().decode(), (bad, rc)


@pytest.mark.parametrize("bad", [dict(n=0), dict(n=-5), dict(g=None), dict(out=None), dict(g=PTR + 2), dict(out=PTR + 4)])
def test_sumsq_refuses_bad_arguments(bad):
    a = {**dict(g=PTR, n=64, out=PTR), **bad}
    lib = _lib.load()
    rc = lib.mage_sumsq(a["g"], a["n"], a["out"], None)
    assert rc == -1 and "mage_sumsq" in lib.mage_last_error().decode(), (bad, rc)


def test_ops_refuse_a_weight_without_a_reference_and_cpu_tensors():
    import torch
    from mage_amd import ops
    z, tok, A = torch.zeros(8, 16), torch.zeros(8, dtype=torch.int64), torch.ones(8)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.policy_loss(z, tok, A, reference_logprob=torch.zeros(8), kl_coef=0.1)
    with pytest.raises(ValueError, match="kl_coef needs reference_logprob"):
        ops.policy_loss(z, tok, A, kl_coef=0.1)
    with pytest.raises(ValueError, match="kl_coef needs reference_logprob"):
        ops.policy_loss_bwd(z, tok, A, None, torch.zeros(8, dtype=torch.int32), torch.ones(1), torch.empty(8, 16), kl_coef=0.1)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.sumsq(torch.zeros(8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.adam_clipped(*[torch.zeros(8) for _ in range(4)], lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, step=1,
                         sumsq=torch.zeros(1, dtype=torch.float64), max_norm=1.0)


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
@pytest.mark.parametrize("k,p", [(0, 1.0), (20, 1.0), (0, 0.9), (20, 0.9)])
def test_gpu_case_recipe_keeps_the_caps(K, k, p):
    """The restatement alone (no kernel) on the inputs of tests/test_gpu_policy_kl.py: the outside rows of make_case's tokens under the exact
    kept sets stay within 25 % of the rows and the unanchored rows within 10 %, as that test then asserts on the kernel's own outputs."""
    from tests import test_gpu_policy_kl as G
    T = (0.7, 1.0, 1.5)[(K + k) % 3]
    z, tok, sets, _ = G.make_case(K, k, p, T, seed=K + k + int(10 * p))
    outside = sum(1 for r in range(G.ROWS) if not sets[r][tok[r]])
    assert outside <= G.ROWS // 4 and len(G.MINUS_INF + G.PLUS_INF + G.A_NAN) <= G.ROWS // 10
    assert (k == 0 and p == 1.0) == (outside == 0)
