"""NumPy / fp64 restatement of mage_policy_loss_anchored and mage_policy_loss_anchored_bwd (include/mage_hip_ext.h states the rule), built on
policy_ref (term, row, dlogits_row, summary) and token_stats_ref.

With lp a row's log-probability under the policy and r its reference log-probability, d = r - lp:
    kl = exp(d) - d - 1   (the k3 estimate, >= 0),       d kl / d lp = 1 - exp(d)
    l  = l(policy_ref) + kl_coef kl,                     g = g(policy_ref) + kl_coef (1 - exp(d))
An outside row (lp = -inf) stays all zeros; a row whose r is not finite is unanchored: kl = 0, no KL gradient, otherwise policy_ref's row.
kl_term / grad_factor evaluate in fp64 without cancellation (expm1, and a series for small |d|); kl_term_mp / grad_factor_mp are the
same values from mpmath at 60 digits: what the fp64 forms are checked against.
"""
import math

import mpmath
import numpy as np

from tests import policy_ref as P
from tests import token_stats_ref as R

mpmath.mp.dps = 60


def delta(lp: float, r: float, fp32: bool = True) -> float:
    """d = r - lp; fp32: formed as the kernel forms it, one fp32 subtraction of the two fp32 values."""
    if fp32:
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float32(r) - np.float32(lp))
    return r - lp


def kl_term(d: float) -> float:
    """exp(d) - d - 1 in fp64, accurate for every d: the series below 2^-8 (first dropped term d^7 / 5040), expm1(d) - d above."""
    if np.isnan(d):
        return np.nan
    if abs(d) < 2.0 ** -8:
        return d * d * (1 / 2 + d * (1 / 6 + d * (1 / 24 + d * (1 / 120 + d * (1 / 720)))))
    try:
        return math.expm1(d) - d
    except OverflowError:
        return np.inf


def grad_factor(d: float) -> float:
    """1 - exp(d) = -expm1(d) in fp64."""
    if np.isnan(d):
        return np.nan
    try:
        return -math.expm1(d)
    except OverflowError:
        return -np.inf


def kl_term_mp(d: float):
    x = mpmath.mpf(d)
    return mpmath.exp(x) - x - 1


def grad_factor_mp(d: float):
    return 1 - mpmath.exp(mpmath.mpf(d))


def anchored(lp: float, r: float) -> bool:
    return not np.isneginf(lp) and bool(np.isfinite(r))


def term(lp: float, H: float, A: float, b, r: float, cmin: float, cmax: float, c: float, kl_coef: float, fp32_d: bool = True) -> dict:
    """policy_ref.term plus the anchor: adds 'kl' and 'unanchored' (an inside row whose r is not finite)."""
    t = P.term(lp, H, A, b, cmin, cmax, c)
    t["kl"], t["unanchored"] = 0.0, (not t["outside"]) and not np.isfinite(r)
    if anchored(lp, r):
        d = delta(lp, r, fp32_d)
        t["kl"] = kl_term(d)
        if kl_coef != 0.0:
            with np.errstate(invalid="ignore"):
                t["loss"] = t["loss"] + kl_coef * t["kl"]
                t["g"] = t["g"] + kl_coef * grad_factor(d)
    return t


def row(z: np.ndarray, t: int, A: float, b, r: float, temperature: float, N: np.ndarray, cmin: float, cmax: float, c: float, kl_coef: float,
        fp32_d: bool = False) -> dict:
    """logprob, entropy, loss, g, kl, ... of one row given its kept set N (d from the fp64 log-probability unless fp32_d)."""
    st = R.stats_for_set(z, t, temperature, 0, N)
    return dict(logprob=st["policy_logprob"], entropy=st["policy_entropy"],
                **term(st["policy_logprob"], st["policy_entropy"], A, b, r, cmin, cmax, c, kl_coef, fp32_d))


def dlogits_row(z: np.ndarray, t: int, A: float, b, r: float, temperature: float, N: np.ndarray, cmin: float, cmax: float, c: float,
                kl_coef: float, scale: float, fp32_d: bool = False) -> np.ndarray:
    """policy_ref.dlogits_row with the extended g: the gradient is linear in g, so the anchor adds
    scale * inv_t * kl_coef (1 - exp(d)) (1[j = t] - p_j) over the kept set."""
    base = P.dlogits_row(z, t, A, b, temperature, N, cmin, cmax, c, scale)
    if not N.any() or not N[t]:
        return base
    rr = row(z, t, A, b, r, temperature, N, cmin, cmax, c, kl_coef, fp32_d)
    if rr["outside"] or not anchored(rr["logprob"], r) or kl_coef == 0.0:
        return base
    extra = kl_coef * grad_factor(delta(rr["logprob"], r, fp32_d))
    unit = P.dlogits_row(z, t, -1.0, None, temperature, N, cmin, cmax, 0.0, scale)        # g = 1, no entropy term: scale inv_t (1[j = t] - p_j)
    return base + extra * unit


def summary(rows: list, with_b: bool) -> np.ndarray:
    """The seven means over a list of (row(...) dict, b): policy_ref.summary's five (the loss now with the KL term), the KL mean over ALL
    rows and the unanchored share."""
    n = len(rows)
    return np.concatenate([P.summary(rows, with_b), [sum(r["kl"] for r, _ in rows if not r["outside"]) / n,
                                                     sum(1.0 for r, _ in rows if r["unanchored"]) / n]])
