"""CPU: the grouped importance ratio -- the fp64 restatement (tests/group_ratio_ref.py) against central finite differences of its own loss,
against tests/masked_loss_ref.py at ratio_div = 1, on hand-made cases that pin the rule (each names the mistake it catches), and the
library's and the model's surface: the two entry points declared and bound, every refusal before anything is launched.

Finite differences (tests/test_policy_kl_ref_cpu.py's step and bound): central, h = 1e-5 in the logit.  A group's loss reads the logits of all
its rows (rho_g does), so the smooth function differentiated is the whole call's scale * sum_i l_i with the kept sets and the counted set as
constants.  With scale = 0.7 / n_free, |A| < 3, rho_g <= e^0.4 and kl_coef = 0.3 the third derivative of the loss along one logit stays
below 1, so the truncation error h^2 |f'''| / 6 is below 2e-11 and the rounding error 2^-52 |f| / h below 2e-11 as well; the bound is 1e-9."""
import os
import re

import numpy as np
import pytest
import torch

from mage_amd import _lib
from mage_amd.utils import synth
from tests import group_ratio_ref as G
from tests import masked_loss_ref as M
from tests import policy_kl_ref as Q
from tests import policy_ref as P
from tests import token_stats_ref as R
from tests.helpers import build_mage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


# ------------------------------------------------------------------------------------------------ the analytic gradient
def _loss64(s, sets, tok, A, b, ref, given, cnt, ratio_div, cmin, cmax, c, kl_coef):
    """sum over the free rows of l_i as a smooth fp64 function of the scaled logits s [rows, K]; the kept sets and the counted set (cnt) are
    constant masks."""
    rows = len(tok)
    lp, H = np.zeros(rows), np.zeros(rows)
    for i in np.flatnonzero(cnt):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d = s[i] - s[i][sets[i]].max()
            w = np.where(sets[i], np.exp(d), 0.0)
            logp = d - np.log(w.sum())
            p = w / w.sum()
            H[i] = -np.where(p > 0, p * logp, 0.0).sum()
        lp[i] = logp[tok[i]]
    total = 0.0
    for g in range(rows // ratio_div):
        idx = np.arange(g * ratio_div, (g + 1) * ratio_div)
        idx = idx[cnt[idx]]
        if not len(idx):
            continue
        rho = np.exp((lp[idx] - b[idx]).sum() / len(idx))
        for i in idx:
            total += -min(rho * A[i], min(max(rho, cmin), cmax) * A[i]) - c * H[i]
            if ref is not None and np.isfinite(ref[i]):
                total += kl_coef * Q.kl_term(ref[i] - lp[i])
    return total


@pytest.mark.parametrize("ratio_div,anchored", [(1, False), (3, False), (4, True), (12, True)])
@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (1.3, 5, 0.9)])
def test_analytic_dlogits_is_the_finite_difference_of_the_loss(ratio_div, anchored, T, k, p):
    K, n, c, kl_coef, h = 8, 12, 0.05, 0.3, 1e-5
    g = np.random.default_rng(ratio_div + k)
    z = (2.0 * g.standard_normal((n, K))).astype(np.float32)
    z[::3] = np.round(z[::3] * 4) / 4
    z[1, 3:6] = -INF
    sets = [R.exact_set(z[r], T, k, p) for r in range(n)]
    tok = np.array([int(g.choice(np.flatnonzero(sets[r] & np.isfinite(z[r])))) for r in range(n)])
    if not sets[7].all():
        tok[7] = int(g.choice(np.flatnonzero(~sets[7])))            # an outside row (under the filter)
    given = np.zeros(n, bool)
    given[[2, 10]] = True
    A = np.repeat(np.abs(g.standard_normal(n // ratio_div)) + 0.1, ratio_div) * np.repeat(np.where(np.arange(n // ratio_div) % 2 == 0, 1.0, -1.0),
                                                                                          ratio_div)
    cmin, cmax = P.clip_bounds(0.2, 0.3)
    lp = np.array([R.stats_for_set(z[r], int(tok[r]), T, 0, sets[r])["policy_logprob"] for r in range(n)])
    lp0 = np.where(np.isfinite(lp), lp, 0.0)
    # group means on both sides of [0.8, 1.3] and inside it (per group of the finest grouping: by rows 0-3, 4-7, 8-11), never near an edge
    b = lp0 - np.repeat([0.35, -0.35, -0.1], 4) * g.uniform(0.9, 1.0, n)
    ref = lp0 + np.array([0.0, 1e-3, -1e-3, 0.5, -0.5, 2.0, -2.0, 0.25, -INF, NAN, 1.0, -1.0]) if anchored else None
    for _ in range(4):                                              # a group within 1e-2 of a clip edge: its rows' b moved, the group kept
        m, _n = G.reduce(lp, b, given, ratio_div)
        near = (np.abs(np.exp(m) / cmin - 1) <= 1e-2) | (np.abs(np.exp(m) / cmax - 1) <= 1e-2)
        b += 0.03 * np.repeat(near, ratio_div)
    rows_, m, cnt_n = G.forward(z, tok, A, b, T, sets, cmin, cmax, c, given, ratio_div, ref, kl_coef)
    cnt = G.counted(lp, given)
    assert cnt_n.sum() == cnt.sum() and (ratio_div == 1 or (cnt_n > 1).all())
    with np.errstate(invalid="ignore"):
        rho = np.exp(m)
    assert (np.abs(rho / cmin - 1) > 1e-2).all() and (np.abs(rho / cmax - 1) > 1e-2).all()
    n_free = int((~given).sum())
    got = G.dlogits(z, tok, rows_, T, sets, c, 0.7)
    s = np.stack([R.scaled(z[r], T).astype(np.float64) for r in range(n)])
    args = (sets, tok, A, b, ref, given, cnt, ratio_div, cmin, cmax, c, kl_coef)
    assert abs(sum(r["loss"] for r in rows_ if r is not None) - _loss64(s, *args)) < 1e-12
    inv_t, scale = G.inv_t(T), 0.7 / n_free
    for r in range(n):
        if not cnt[r]:
            assert (got[r] == 0).all()
            continue
        for j in np.flatnonzero(np.isfinite(z[r])):
            e = np.zeros_like(s)
            e[r, j] = h * inv_t
            fd = scale * (_loss64(s + e, *args) - _loss64(s - e, *args)) / (2 * h)
            want = fd if sets[r][j] else 0.0
            assert abs(got[r, j] - want) < 1e-9, (r, j, got[r, j], want)
    if ratio_div > 1:
        assert ratio_div == 12 or {r["off"] for r in rows_ if r is not None and not r["outside"]} == {False, True}
        # the mistake "g_i divided by n_g": it moves dlogits by far more than the 1e-9 every entry above was held to
        wrong = G.dlogits(z, tok, [None if q is None else {**q, "g": q["g"] / cnt_n[i // ratio_div]} for i, q in enumerate(rows_)], T, sets, c, 0.7)
        assert np.abs(wrong - got).max() > 1e-4


def test_ratio_div_one_is_the_masked_restatement_exactly():
    K, n, T, c = 12, 11, 0.8, 0.01
    g = np.random.default_rng(3)
    z = (2.0 * g.standard_normal((n, K))).astype(np.float32)
    tok = g.integers(0, K, n)
    A = (g.uniform(0.5, 2.0, n) * g.choice([-1.0, 1.0], n)).astype(np.float32)
    sets = [R.admissible_sets(z[r], T, 5, 0.9)[0] for r in range(n)]
    lp = np.array([R.stats_for_set(z[r], int(tok[r]), T, 0, sets[r])["policy_logprob"] for r in range(n)])
    b = (np.where(np.isfinite(lp), lp, 0.0) + g.choice([-0.35, 0.1, 0.35], n)).astype(np.float32)
    cmin, cmax = P.clip_bounds(0.2, 0.3)
    assert np.isneginf(lp).any()
    for given in (np.zeros(n, bool), np.arange(n) % 3 == 1):
        rows_, m, cnt = G.forward(z, tok, A, b, T, sets, cmin, cmax, c, given, 1)
        want = M.policy_rows(z, tok, A, b, T, sets, cmin, cmax, c, given)
        for r in range(n):
            assert (rows_[r] is None) == (want[r] is None)
            if want[r] is not None:
                assert all(rows_[r][k] == want[r][k] for k in ("logprob", "entropy", "loss", "g", "rho", "outside", "off")), r
        assert np.array_equal(cnt, G.counted(lp, given).astype(int))
        five, share, norm = M.policy_summary(want, b, given)
        got, gnorm = G.summary(rows_, b, False)
        assert np.array_equal(got[:5], five) and (got[5:7] == 0).all() and got[7] == share and gnorm == norm
        assert np.array_equal(G.dlogits(z, tok, rows_, T, sets, c, 0.7), M.policy_dlogits(z, tok, A, b, T, sets, cmin, cmax, c, 0.7, given))


# ------------------------------------------------------------------------------------------------ cases that pin the rule
CMIN, CMAX = P.clip_bounds(0.2, 0.2)


def _flat(n, lp=-1.0):
    return np.full(n, lp), np.full(n, 0.5)                          # (logprob, entropy)


def test_split_signs_one_ratio_per_group_not_per_token():
    """Half of a group at d = +0.5, half at -0.5, clip 0.2, A > 0.  A per-token ratio clips every +0.5 row (e^0.5 = 1.65 > 1.2); the group
    ratio is exp(0) = 1: no row is clipped and every g_i = -A."""
    n, A = 8, 1.5
    lp, H = _flat(n)
    b = lp - np.where(np.arange(n) < n // 2, 0.5, -0.5)
    token = [P.term(lp[i], H[i], A, b[i], CMIN, CMAX, 0.0) for i in range(n)]
    assert [t["off"] for t in token] == [True] * 4 + [False] * 4
    rows_, m, cnt = G.terms(lp, H, np.full(n, A), b, None, n, CMIN, CMAX, 0.0)
    assert m[0] == 0.0 and cnt[0] == n
    assert all(not r["off"] and r["g"] == -A and r["loss"] == -A for r in rows_)
    s, _ = G.summary(rows_, b, False)
    assert s[3] == 0.0 and s[0] == -A
    # two groups of four: each has its own ratio again (+0.5: clipped throughout, -0.5: active throughout)
    rows_, m, cnt = G.terms(lp, H, np.full(n, A), b, None, 4, CMIN, CMAX, 0.0)
    assert np.allclose(m, [0.5, -0.5]) and [r["off"] for r in rows_] == [True] * 4 + [False] * 4
    assert G.summary(rows_, b, False)[0][3] == 0.5                  # the clipped share stays a share of rows


def test_given_and_outside_rows_are_not_counted():
    """Rows 1 (given) and 2 (outside) are not in n_g; their b changes nothing.  A mean over ratio_div instead of n_g is caught: the right
    m = 0.3 clips (e^0.3 = 1.35 > 1.2), the wrong 0.15 would not."""
    lp, H = _flat(4)
    lp[2] = -INF
    given = np.array([False, True, False, False])
    b = lp - 0.3
    b[2] = 0.0
    A = np.full(4, 2.0)
    rows_, m, cnt = G.terms(lp, H, A, b, given, 4, CMIN, CMAX, 0.0)
    assert cnt[0] == 2 and abs(m[0] - 0.3) < 1e-15
    assert rows_[1] is None and rows_[2]["outside"] and rows_[2]["loss"] == 0.0 and rows_[2]["g"] == 0.0
    assert rows_[0]["off"] and rows_[3]["off"] and rows_[0]["g"] == 0.0 and abs(rows_[0]["loss"] + 2.0 * CMAX) < 1e-15
    assert np.exp(0.3 * 2 / 4) < CMAX < np.exp(m[0])                # what a mean over ratio_div would have decided
    b2 = b.copy()
    b2[1], b2[2] = 55.0, NAN
    rows2, m2, cnt2 = G.terms(lp, H, A, b2, given, 4, CMIN, CMAX, 0.0)
    assert m2[0] == m[0] and cnt2[0] == 2 and rows2 == rows_
    s, norm = G.summary(rows_, b, False)
    assert s[7] == 0.25 and norm == np.float32(1) / np.float32(3) and abs(s[4] - 1 / 3) < 1e-15 and abs(s[3] - 2 / 3) < 1e-15


def test_a_group_with_nothing_to_count():
    lp, H = _flat(6)
    lp[3] = -INF
    given = np.array([False] * 3 + [False, True, True])
    b = lp - 0.1
    b[3] = 0.0
    rows_, m, cnt = G.terms(lp, H, np.ones(6), b, given, 3, CMIN, CMAX, 0.0)
    assert cnt.tolist() == [3, 0] and m[1] == 0.0 and not np.signbit(m[1]) and abs(m[0] - 0.1) < 1e-15
    assert rows_[3]["outside"] and rows_[4] is None and rows_[5] is None
    all_given, m, cnt = G.terms(lp, H, np.ones(6), b, np.ones(6, bool), 3, CMIN, CMAX, 0.0)
    s, norm = G.summary(all_given, b, False)
    assert cnt.tolist() == [0, 0] and (m == 0).all() and (s[:7] == 0).all() and s[7] == 1.0 and norm == 0


def test_a_nan_difference_makes_its_group_nan_and_no_other():
    lp, H = _flat(4)
    b = lp.copy()
    b[1] = NAN
    rows_, m, cnt = G.terms(lp, H, np.ones(4), b, None, 2, CMIN, CMAX, 0.0)
    assert np.isnan(m[0]) and m[1] == 0.0 and np.isnan(rows_[0]["loss"]) and rows_[0]["off"] and rows_[0]["g"] == 0.0
    assert rows_[2]["loss"] == -1.0 and rows_[2]["rho"] == 1.0


def test_anchor_is_added_per_row():
    lp, H = _flat(2)
    b, ref = lp.copy(), np.array([-0.5, NAN])
    rows_, m, cnt = G.terms(lp, H, np.full(2, 2.0), b, None, 2, CMIN, CMAX, 0.0, ref, 0.25)
    k = np.exp(0.5) - 1.5
    assert abs(rows_[0]["kl"] - k) < 1e-15 and abs(rows_[0]["loss"] - (-2.0 + 0.25 * k)) < 1e-15
    assert abs(rows_[0]["g"] - (-2.0 + 0.25 * (1.0 - np.exp(0.5)))) < 1e-15
    assert rows_[1]["unanchored"] and rows_[1]["kl"] == 0.0 and rows_[1]["loss"] == -2.0
    s, _ = G.summary(rows_, b, True)
    assert abs(s[5] - k / 2) < 1e-15 and s[6] == 0.5


# ------------------------------------------------------------------------------------------------ the library's surface
NEW = ("mage_policy_loss_grouped", "mage_policy_loss_grouped_bwd")
PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched
EINVAL = -1


def test_header_and_table_name_the_grouped_entry_points():
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
    n = lambda k: len(_lib.EXT_SIGNATURES[k][1])      # noqa: E731
    assert n("mage_policy_loss_grouped") == n("mage_policy_loss_masked") + 3           # ratio_div, group_logratio, group_count
    assert n("mage_policy_loss_grouped_bwd") == n("mage_policy_loss_masked_bwd") + 2   # ratio_div, group_logratio
    # the existing pairs keep their signatures
    assert n("mage_policy_loss") == 20 and n("mage_policy_loss_bwd") == 17 and n("mage_policy_loss_masked") == 25
    assert n("mage_policy_loss_masked_bwd") == 21


def _fwd(lib, *, rows=8, K=16, adv_div=4, b=PTR, given=PTR, norm=PTR, ref=PTR, kl=PTR, kl_coef=0.1, ratio_div=4, glr=PTR, gcount=PTR, logits=PTR,
         top_k=0):
    return lib.mage_policy_loss_grouped(logits, rows, K, 16, PTR, PTR, adv_div, b, ref, 1.0, top_k, 1.0, 0.2, 0.2, 0.0, kl_coef, PTR, PTR, PTR, PTR,
                                        kl, PTR, norm, given, ratio_div, glr, gcount, None)


def _bwd(lib, *, rows=8, K=16, adv_div=4, b=PTR, given=PTR, norm=PTR, ref=PTR, kl_coef=0.1, ratio_div=4, glr=PTR, dl=PTR, dl_dtype=0):
    return lib.mage_policy_loss_grouped_bwd(PTR, rows, K, 16, PTR, PTR, adv_div, b, ref, PTR, 1.0, 0.2, 0.2, 0.0, kl_coef, PTR, norm, dl, dl_dtype,
                                            given, ratio_div, glr, None)


def test_refusals_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.mage_last_error()               # noqa: E731
    for call in (_fwd, _bwd):
        assert call(lib, b=None) == EINVAL and b"behaviour_logprob" in err()
        for rd in (0, -4, 2 ** 31):
            assert call(lib, ratio_div=rd) == EINVAL and b"ratio_div" in err(), rd
        assert call(lib, rows=10) == EINVAL and b"rows=10" in err()                     # rows % ratio_div
        assert call(lib, adv_div=6) == EINVAL and b"adv_div=6" in err()                 # adv_div % ratio_div
        assert call(lib, adv_div=2) == EINVAL and b"adv_div=2" in err()                 # an advantage finer than the group
        assert call(lib, adv_div=0) == EINVAL
        assert call(lib, glr=None) == EINVAL and b"group_logratio" in err()
        assert call(lib, glr=PTR + 2) == EINVAL and b"group_logratio" in err()
        assert call(lib, norm=None) == EINVAL and b"norm" in err()
        assert call(lib, norm=PTR + 1) == EINVAL and b"norm" in err()
        assert call(lib, ref=None, kl_coef=0.1, **({"kl": None} if call is _fwd else {})) == EINVAL and b"kl_coef" in err()
        # the masked pair's own argument rules hold behind these
        assert call(lib, K=15) == EINVAL and b"grouped" in err()
        assert call(lib, rows=0) == EINVAL
    assert _fwd(lib, gcount=None) == EINVAL and b"group_count" in err()
    assert _fwd(lib, gcount=PTR + 2) == EINVAL and b"group_count" in err()
    assert _fwd(lib, kl=None) == EINVAL and b"together" in err()                        # a reference without kl
    assert _fwd(lib, ref=None) == EINVAL and b"together" in err()                       # kl without a reference
    assert _fwd(lib, logits=PTR + 4) == EINVAL and _fwd(lib, top_k=1) == EINVAL and b"top_k=1" in err()
    assert _bwd(lib, dl=PTR + 8) == EINVAL and _bwd(lib, dl_dtype=7) == EINVAL and b"dlogits" in err()
    # accepted forms get past every argument rule: without an initialised device the forward call stops at the mage_init check behind them
    for ok in (dict(), dict(given=None), dict(ref=None, kl=None, kl_coef=0.0), dict(ratio_div=1), dict(ratio_div=8, adv_div=8),
               dict(ratio_div=2, adv_div=8)):
        assert _fwd(lib, **ok) == EINVAL and b"mage_init" in err(), (ok, err())


# ------------------------------------------------------------------------------------------------ MAGE.policy_loss(ratio=)
def test_python_refusals_on_a_cpu_model():
    L = 4
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=16), 0)
    batch = synth.synth_batch_mnist(2, L, seed=1)
    R_ = m.image_resolution
    tokens = torch.zeros(2, L - 1, R_, R_, dtype=torch.int64)
    blp = torch.zeros(2, L - 1, R_, R_)
    a_clip, a_frame, a_tok = torch.ones(2), torch.ones(2, L - 1), torch.ones(2, L - 1, R_, R_)
    assert m.last_policy_group_logratio is None
    for bad in ("sequence", "Frame", None, 1):
        with pytest.raises(ValueError, match="ratio must be"):
            m.policy_loss(batch, tokens, a_clip, blp, ratio=bad)
    for ratio in ("frame", "clip"):
        with pytest.raises(ValueError, match="needs behaviour_logprobs"):
            m.policy_loss(batch, tokens, a_clip, ratio=ratio)
        with pytest.raises(ValueError, match="not finer than the group"):
            m.policy_loss(batch, tokens, a_tok, blp, ratio=ratio)
    with pytest.raises(ValueError, match="not finer than the group"):
        m.policy_loss(batch, tokens, a_frame, blp, ratio="clip")
    # what the rule allows reaches the last refusal, the one about the device; 'token' is today's call
    for ratio, adv in (("token", a_tok), ("token", a_clip), ("frame", a_clip), ("frame", a_frame), ("clip", a_clip)):
        with pytest.raises(ValueError, match="GPU"):
            m.policy_loss(batch, tokens, adv, blp, ratio=ratio)
    assert m.last_policy_group_logratio is None and m.last_policy_token_logprobs is None
