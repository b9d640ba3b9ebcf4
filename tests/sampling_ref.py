"""NumPy / fp64 restatement of the token-sampling rule of mage_sample_tokens (mage_amd/csrc/token_row.h states it; include/mage_hip.h).

For one row: s = fp32(z * inv_t), inv_t = fp32(1 / temperature); top-k keeps every code whose s is >= the top_k-th largest (ties kept);
top-p keeps, of those, every code whose s is >= tau, the largest value whose softmax mass from above reaches top_p * W (ties kept); the
token is the smallest j of that set maximising s_j + g_j, g_j = -log(-log(u_j)), u_j = ((hash32(seed * 0x9e3779b97f4a7c15 + pos * K + j)
>> 8) + 0.5) * 2^-24 in uint64 wrap-around arithmetic.  NaN logits are never drawn.  Everything after the fp32 multiply is fp64 here.
"""
import numpy as np

GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def hash32(v):
    """common.h's hash32 (the dropout masks' mixer) on uint64 arrays."""
    v = np.array(v, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        v ^= v >> np.uint64(33)
        v *= np.uint64(0xFF51AFD7ED558CCD)
        v ^= v >> np.uint64(33)
        v *= np.uint64(0xC4CEB9FE1A85EC53)
        v ^= v >> np.uint64(33)
    return (v & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def uniforms(seed: int, pos: int, K: int) -> np.ndarray:
    """u_j, j in [0, K), fp64 (exact: 25 significant bits)."""
    s = np.array([seed], dtype=np.int64).view(np.uint64)[0]
    with np.errstate(over="ignore"):
        base = s * GOLDEN_GAMMA + np.uint64(pos) * np.uint64(K)
        ctr = base + np.arange(K, dtype=np.uint64)
    m = hash32(ctr) >> np.uint64(8)
    return (m.astype(np.float64) + 0.5) * 2.0 ** -24


def gumbel(u: np.ndarray) -> np.ndarray:
    return -np.log(-np.log(u))


def inv_temperature(temperature: float) -> np.float32:
    """inv_t as the library computes it: (float)(1.0 / temperature) of the fp32 temperature."""
    return np.float32(1.0 / float(np.float32(temperature)))


def candidates(s: np.ndarray, top_k: int, top_p: float, tol: float = 1e-5):
    """The set N of the rule for one row of scaled logits s (fp32 values), and whether the top-k / top-p boundary is within `tol` (top-k:
    of the next value, in logit units; top-p: of top_p * W, relative to W): there a kernel's rounded sums / a perturbed logit may keep one
    value more or less."""
    K = s.shape[0]
    s = s.astype(np.float64)
    valid = ~np.isnan(s)
    A = valid.copy()
    near = False
    if 0 < top_k < K and valid.sum() >= top_k:
        vs = np.sort(s[valid])[::-1]
        kth = vs[top_k - 1]
        A &= s >= kth
        below = vs[vs < kth]
        if below.size and kth - below[0] < tol:
            near = True
    N = A
    if top_p < 1.0 and A.any():
        sa = s[A]
        w = np.exp(sa - sa.max())
        W = w.sum()
        target = float(np.float32(top_p)) * W
        vals, inv = np.unique(sa, return_inverse=True)
        mass = np.cumsum(np.bincount(inv.reshape(-1), weights=w)[::-1])     # mass(>= v), v = distinct values descending
        vals = vals[::-1]
        idx = int(np.argmax(mass >= target))                                # first (= largest v) reaching the target
        tau = vals[idx]
        if np.any(np.abs(mass - target) <= tol * W):
            near = True
        N = A & (s >= tau)
    return N, near


def sample_row(z: np.ndarray, temperature: float, top_k: int, top_p: float, seed: int, pos: int, tol: float = 1e-5):
    """(token, soft): soft = a kernel result other than `token` is explainable by rounding (the perturbed top-2 gap below `tol`, or a
    top-k / top-p boundary within `tol`)."""
    z = np.asarray(z, dtype=np.float32)
    K = z.shape[0]
    if top_k == 1:                                                  # greedy by definition (first maximum of the logits)
        zz = np.where(np.isnan(z), -np.inf, z.astype(np.float64))
        srt = np.sort(zz)[::-1]
        return int(np.argmax(zz)), bool(K > 1 and srt[0] - srt[1] < tol)
    s = (z * inv_temperature(temperature)).astype(np.float32)
    N, near = candidates(s, top_k, top_p, tol)
    if not N.any():
        return 0, near
    score = np.where(N, s.astype(np.float64) + gumbel(uniforms(seed, pos, K)), -np.inf)
    tok = int(np.argmax(score))
    if N.sum() > 1:
        top2 = np.sort(score[N])[::-1][:2]
        near = near or bool(top2[0] - top2[1] < tol)
    return tok, near


def target_distribution(z: np.ndarray, temperature: float, top_k: int, top_p: float) -> np.ndarray:
    """softmax of s over N (renormalised), fp64 [K]: the law of the token."""
    s = (np.asarray(z, dtype=np.float32) * inv_temperature(temperature)).astype(np.float32)
    N, _ = candidates(s, top_k, top_p)
    sd = s.astype(np.float64)
    p = np.where(N, np.exp(sd - sd[N].max()), 0.0)
    return p / p.sum()
