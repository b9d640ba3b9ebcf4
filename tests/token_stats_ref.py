"""NumPy / fp64 restatement of mage_token_stats (include/mage_hip_ext.h states the rule), built on sampling_ref.candidates.

For one row of fp32 logits z, token t and (temperature, top_k, top_p): s = fp32(z * inv_t) and N = the sampling rule's kept set.  Then, in
fp64, s_max = max_N s, w_j = exp(s_j - s_max), Z = sum_N w_j and
    kept = |N|,   policy_logprob = s_t - (s_max + log Z) for t in N else -inf,   policy_entropy = log Z - (sum_N w_j (s_j - s_max)) / Z,
a term with w_j = 0 counting as 0 (never 0 * inf); N empty: kept 0, NaN, NaN; s_max not finite: NaN (inf - inf).  entropy is the same
formula over the whole row of z itself (temperature 1, no filter; a NaN logit makes it NaN).  top_k == 1 is greedy: N = {first maximum of z,
NaNs skipped}, policy_logprob 0 for that code and -inf for any other, policy_entropy 0.

The kernel sums its top-p masses in fp32, so at a row whose boundary mass is within rounding of top_p * W it may keep one value more or less
than the exact rule; admissible_sets returns every kept set such rounding can explain (one set -- the exact one -- for all other rows), so
that no row has to be left out of a comparison.
"""
import numpy as np

from tests import sampling_ref as S

TOL = 1e-5          # sampling_ref's: about 2.5x the rounding of <= 64 sequential adds plus 6 butterfly stages, relative to W


def scaled(z: np.ndarray, temperature: float) -> np.ndarray:
    return (np.asarray(z, dtype=np.float32) * S.inv_temperature(temperature)).astype(np.float32)


def greedy_set(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.float32)
    N = np.zeros(z.shape[0], dtype=bool)
    if not np.isnan(z).all():
        N[int(np.argmax(np.where(np.isnan(z), -np.inf, z.astype(np.float64))))] = True
    return N


def exact_set(z: np.ndarray, temperature: float, top_k: int, top_p: float) -> np.ndarray:
    if top_k == 1:
        return greedy_set(z)
    with np.errstate(invalid="ignore"):                             # (a row of -inf only: inf - inf inside)
        return S.candidates(scaled(z, temperature), top_k, top_p)[0]


def admissible_sets(z: np.ndarray, temperature: float, top_k: int, top_p: float, tol: float = TOL) -> list:
    """Every kept set the kernel may report for this row, the exact one first.  With exact masses m(v) = sum_{j in A, s_j >= v} w_j and
    target = fp32(top_p) * W, a distinct value v of A is an admissible threshold iff m(v) >= target - tol W and m(v+) < target + tol W
    (v+ the next larger distinct value, m of nothing = 0).  Top-k needs no allowance: the kernel's counts are exact."""
    sets = [exact_set(z, temperature, top_k, top_p)]
    if top_k == 1 or not top_p < 1.0:
        return sets
    s = scaled(z, temperature).astype(np.float64)
    A = S.candidates(s.astype(np.float32), top_k, 1.0)[0]
    if not A.any():
        return sets
    with np.errstate(invalid="ignore"):
        sa = s[A]
        w = np.exp(sa - sa.max())
    W = w.sum()
    if not np.isfinite(W):
        return sets
    target = float(np.float32(top_p)) * W
    vals, inv = np.unique(sa, return_inverse=True)
    mass = np.cumsum(np.bincount(inv.reshape(-1), weights=w)[::-1])         # m(v), v = the distinct values descending
    vals = vals[::-1]
    above = np.concatenate([[0.0], mass[:-1]])                              # m(v+)
    ok = (mass >= target - tol * W) & (above < target + tol * W)
    for v in vals[ok]:
        N = A & (s >= v)
        if not any(np.array_equal(N, q) for q in sets):
            sets.append(N)
    return sets


def _entropy(x: np.ndarray):
    """(log Z, entropy) of the softmax over the fp64 values x (a NaN or a non-finite maximum gives NaN)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = x - np.max(x)
        w = np.exp(d)
        Z = np.sum(w)
        return float(np.log(Z)), float(np.log(Z) - np.sum(np.where(w == 0, 0.0, w * d)) / Z)


def entropy(z: np.ndarray) -> float:
    return _entropy(np.asarray(z, dtype=np.float32).astype(np.float64))[1]


def stats_for_set(z: np.ndarray, t: int, temperature: float, top_k: int, N: np.ndarray) -> dict:
    """kept, policy_logprob, policy_entropy (and log_z, for error bounds) of one row given its kept set N."""
    kept = int(N.sum())
    if kept == 0:
        return dict(kept=0, policy_logprob=np.nan, policy_entropy=np.nan, log_z=np.nan)
    if top_k == 1:
        return dict(kept=1, policy_logprob=0.0 if N[t] else -np.inf, policy_entropy=0.0, log_z=0.0)
    s = scaled(z, temperature).astype(np.float64)
    log_z, ent = _entropy(s[N])
    with np.errstate(invalid="ignore"):
        lp = float(s[t] - (s[N].max() + log_z)) if N[t] else -np.inf
    return dict(kept=kept, policy_logprob=lp, policy_entropy=ent, log_z=log_z)


def row_stats(z: np.ndarray, t: int, temperature: float, top_k: int, top_p: float) -> dict:
    """The exact rule's statistics of one row."""
    return stats_for_set(z, t, temperature, top_k, exact_set(z, temperature, top_k, top_p))
