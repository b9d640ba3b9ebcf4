"""NumPy / fp64 restatement of mage_policy_loss and mage_policy_loss_bwd (include/mage_hip_ext.h states the rule), built on
token_stats_ref (scaled, exact_set, admissible_sets, stats_for_set).

For one row of fp32 logits z, token t, advantage A, optional behaviour log-probability b and (temperature, top_k, top_p): s = fp32(z * inv_t)
and N = the sampling rule's kept set.  In fp64, with p the softmax of s over N, logprob = log p_t (-inf for t outside N) and
H = -sum_N p_j log p_j:
    weighted form (b None):  l = -A logprob - c H,                                   g = -A
    clipped form:            l = -min(rho A, clamp(rho, cmin, cmax) A) - c H,        rho = exp(logprob - b),
                             g = -A rho where the unclipped term is the active one (A >= 0 and rho <= cmax, or A < 0 and rho >= cmin), else 0
    dlogits_j = scale * inv_t * [ g (1[j = t] - p_j) + c p_j (log p_j + H) ]  for j in N (a p_j = 0 term counts as 0), 0 for j outside N.
A row whose token lies outside a non-empty N is an outside row: l = 0 and a zero gradient row.  cmin = fp32(1 - clip_lo), cmax =
fp32(1 + clip_hi): the library's two bounds.  The kept set is an argument wherever it matters (a kernel may report any admissible one).
"""
import numpy as np

from tests import sampling_ref as S
from tests import token_stats_ref as R


def clip_bounds(clip_lo: float, clip_hi: float):
    """(cmin, cmax) as the library forms them from its fp32 arguments."""
    return float(np.float32(1.0 - float(np.float32(clip_lo)))), float(np.float32(1.0 + float(np.float32(clip_hi))))


def term(lp: float, H: float, A: float, b, cmin: float, cmax: float, c: float) -> dict:
    """One row's loss and gradient factor from its log-probability and entropy (fp64 throughout)."""
    if np.isneginf(lp):
        return dict(loss=0.0, g=0.0, rho=0.0, outside=True, off=False)
    if b is None:
        return dict(loss=-A * lp - c * H, g=-A, rho=1.0, outside=False, off=False)
    with np.errstate(over="ignore", invalid="ignore"):
        rho = float(np.exp(lp - b))
        active = (A >= 0 and rho <= cmax) or (A < 0 and rho >= cmin)
        surr = min(rho * A, min(max(rho, cmin), cmax) * A) if not np.isnan(rho) else np.nan
    return dict(loss=-surr - c * H, g=-A * rho if active else 0.0, rho=rho, outside=False, off=not active)


def row(z: np.ndarray, t: int, A: float, b, temperature: float, N: np.ndarray, cmin: float, cmax: float, c: float) -> dict:
    """logprob, entropy, loss, g, ... of one row given its kept set N."""
    st = R.stats_for_set(z, t, temperature, 0, N)
    return dict(logprob=st["policy_logprob"], entropy=st["policy_entropy"],
                **term(st["policy_logprob"], st["policy_entropy"], A, b, cmin, cmax, c))


def dlogits_row(z: np.ndarray, t: int, A: float, b, temperature: float, N: np.ndarray, cmin: float, cmax: float, c: float,
                scale: float) -> np.ndarray:
    """The analytic gradient of scale * l with respect to the row's logits; scale = grad_out / rows."""
    K = z.shape[0]
    out = np.zeros(K, np.float64)
    if not N.any() or not N[t]:
        return out
    r = row(z, t, A, b, temperature, N, cmin, cmax, c)
    if r["outside"]:                                                # (a kept token of logit -inf: logprob -inf as well)
        return out
    s = R.scaled(z, temperature).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = s - s[N].max()
        w = np.where(N, np.exp(d), 0.0)
        Z = w.sum()
        p = w / Z
        logp = d - np.log(Z)
        ent = np.where(p > 0, p * (logp + r["entropy"]), 0.0)
    score = -p
    score[t] = np.delete(w, t).sum() / Z                            # 1 - p_t from the other terms: no cancellation where p_t -> 1
    out = r["g"] * score + c * ent
    out[~N] = 0.0
    return scale * float(S.inv_temperature(temperature)) * out


def summary(rows: list, with_b: bool) -> np.ndarray:
    """The five means over a list of (row(...) dict, b): loss, entropy, b - logprob, the clipped share, the outside share.  An outside row
    counts in the last one only."""
    n = len(rows)
    inside = [(r, b) for r, b in rows if not r["outside"]]
    return np.array([sum(r["loss"] for r, _ in inside) / n, sum(r["entropy"] for r, _ in inside) / n,
                     sum(b - r["logprob"] for r, b in inside) / n if with_b else 0.0,
                     sum(1.0 for r, _ in inside if r["off"]) / n, (n - len(inside)) / n])
