"""fp64 restatement of mage_distill_loss / mage_distill_loss_bwd (include/mage_hip_ext.h), with the error bounds the GPU tests hold the
kernels to.  numpy, one row at a time; `torch_kl` is the same rule on torch tensors (differentiable: the end-to-end oracle).

The rule for one row, student logits z and teacher logits t (fp32), temperature T:
  inv_t = fp32(1 / T);  s = fp32(z * inv_t), u = fp32(t * inv_t)            (one fp32 multiply each, as the kernel; everything after in fp64)
  per row x in (s, u):  m = max_j x_j (a NaN skipped),  d_j = x_j - m,  w_j = exp(d_j),  Z = sum_j w_j,  H = log Z - sum_j w_j d_j / Z
  forward (mode 0):  kl = A / Z_T + (log Z_S - log Z_T),  A = sum_{j: w_T,j > 0} w_T,j (d_T,j - d_S,j);    reverse (mode 1): roles swapped
  gradient of mean_i kl_i times g:  c = g / n_free * inv_t;  mode 0: c (p_S - p_T);  mode 1: c p_S ((log p_S - log p_T) - kl), 0 where p_S = 0;
  a row whose kl is not finite gets zeros.

Bounds (derived from the kernel's operation count, not from its output; TOL is token_stats_ref's allowance for one fixed-order fp32 sum of
up to 64 adds per lane and 6 butterfly stages, relative to the sum of the terms' magnitudes).  With P the first distribution of the KL, Q the
second, E_P[.] the mean under p_P over the codes of positive weight:
  a weight w_j carries expf's 2 ulp and the rounding of its d_j:                      rel(w_j) <= 2^-24 (|d_j| + 3)
  Z carries that, weighted, and its summation:                                        rel(Z)   <= TOL + 2^-24 (E|d| + 3)
  log Z turns rel(Z) into an absolute error and adds logf's 2 ulp:                    abs      <= rel(Z) + 2^-22 |log Z|
  d_P - d_Q carries the roundings of d_P, d_Q and of the difference:                  abs      <= 2^-23 (|d_P| + |d_Q|)
  A / Z_P = E_P[d_P - d_Q]:  TOL for A's sum and rel(Z_P), both relative to E_P|d_P - d_Q|, the weights' and the differences' errors,
  one division, one subtraction, one addition (2^-24 relative each, of their results):
    |d kl| <= (2 TOL + 2^-24 (E_P|d_P| + 3)) E_P|d_P - d_Q| + 2^-24 E_P[(|d_P| + 3) |d_P - d_Q|] + 2^-23 E_P[|d_P| + |d_Q|]
              + 2 TOL + 2^-24 (E_P|d_P| + E_Q|d_Q| + 6) + 2^-22 (|log Z_P| + |log Z_Q|) + 2^-24 (|A / Z_P| + |log Z_Q - log Z_P| + |kl|)
  dlogits, mode 0:  |c| [rel(p_S,j) p_S,j + rel(p_T,j) p_T,j] with rel(p_j) = rel(w_j) + rel(Z) + 2^-23 (1 / Z and the product), plus
    2^-22 |want| (c is two fp32 products; the last product);
  mode 1:  |c| p_S,j [rel(p_S,j) |b_j| + 2^-23 (|d_S,j| + |d_T,j|) + abs(log Z_S) + abs(log Z_T) + |d kl| + 2^-23 (|d_S,j - d_T,j| +
    |log Z_S - log Z_T| + |b_j|)] + 2^-22 |want|, b_j = (log p_S,j - log p_T,j) - kl;
  a bf16 store adds 2^-8 |want|; both get the absolute floor 2^-126 (tests/test_gpu_policy_loss.py: no relative precision below it)."""
import numpy as np
import torch

from tests import sampling_ref as S
from tests.token_stats_ref import TOL

E24 = 2.0 ** -24


def _side(x):
    """(d, w, Z, log Z, H, E|d|) of one scaled row in fp64; NaN throughout for a row with a NaN or without a finite maximum."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.fmax.reduce(x) if not np.isnan(x).all() else -np.inf
        d = x - m
        w = np.exp(d)
        Z = w.sum()
        pos = w > 0
        ts = (w[pos] * d[pos]).sum()
        lz = np.log(Z)
        return dict(d=d, w=w, Z=Z, lz=lz, H=lz - ts / Z, Ed=(w[pos] * np.abs(d[pos])).sum() / Z, pos=pos)


def scaled(z, T):
    return (np.asarray(z, np.float32) * S.inv_temperature(T)).astype(np.float32).astype(np.float64)


def row(z, t, T, mode):
    """One row: dict(kl, bound, teacher_entropy, entropy, agree) and the two sides (keys 'S', 'T')."""
    s, u = _side(scaled(z, T)), _side(scaled(t, T))
    P, Q = (u, s) if mode == 0 else (s, u)
    pos = P["pos"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        diff = P["d"][pos] - Q["d"][pos]
        pw = P["w"][pos] / P["Z"]
        az = (pw * diff).sum()
        ldiff = Q["lz"] - P["lz"]
        kl = az + ldiff
        bound = np.nan
        if np.isfinite(kl):
            ad, adq = np.abs(P["d"][pos]), np.abs(Q["d"][pos])
            e1 = (pw * np.abs(diff)).sum()
            bound = ((2 * TOL + E24 * (P["Ed"] + 3)) * e1 + E24 * (pw * (ad + 3) * np.abs(diff)).sum() + 2 * E24 * (pw * (ad + adq)).sum()
                     + 2 * TOL + E24 * (P["Ed"] + Q["Ed"] + 6) + 4 * E24 * (abs(P["lz"]) + abs(Q["lz"])) + E24 * (abs(az) + abs(ldiff) + abs(kl)))
    return dict(kl=kl, bound=bound, teacher_entropy=u["H"], entropy=s["H"], agree=argmax(z) == argmax(t), S=s, T=u)


def argmax(z):
    """mage_argmax's rule: NaNs skipped, the first maximum wins; a row of NaNs: 0x7fffffff."""
    z = np.asarray(z, np.float32)
    if np.isnan(z).all():
        return 0x7fffffff
    return int(np.flatnonzero(z == np.fmax.reduce(z))[0])


def dlogits_row(z, t, T, mode, c, bf16=False):
    """(want, bound) fp64 [K]: the gradient row for the scalar c = grad_out / n_free * inv_t (fp64 from the fp32 factors) and its bound."""
    r = row(z, t, T, mode)
    K = len(z)
    if not np.isfinite(r["kl"]):
        return np.zeros(K), np.zeros(K)
    s, u = r["S"], r["T"]
    ps, pt = s["w"] / s["Z"], u["w"] / u["Z"]
    rel = lambda x: E24 * (np.abs(np.where(np.isfinite(x["d"]), x["d"], 0.0)) + 3) + TOL + E24 * (x["Ed"] + 3) + 2 * E24     # noqa: E731
    if mode == 0:
        want = c * (ps - pt)
        bound = abs(c) * (rel(s) * ps + rel(u) * pt)
    else:
        with np.errstate(invalid="ignore"):
            dd = np.where(ps > 0, s["d"] - u["d"], 0.0)
            b = np.where(ps > 0, dd - (s["lz"] - u["lz"]) - r["kl"], 0.0)
            want = c * ps * b
            ad = np.where(ps > 0, np.abs(s["d"]) + np.abs(u["d"]), 0.0)
        alog = lambda x: TOL + E24 * (x["Ed"] + 3) + 4 * E24 * abs(x["lz"])      # noqa: E731
        bound = abs(c) * ps * (rel(s) * np.abs(b) + 2 * E24 * ad + alog(s) + alog(u) + r["bound"]
                               + 2 * E24 * (np.abs(dd) + abs(s["lz"] - u["lz"]) + np.abs(b)))
    bound = bound + 4 * E24 * np.abs(want) + (2.0 ** -8 * np.abs(want) if bf16 else 0.0) + 2.0 ** -126
    return want, bound


def loss(z, t, T, mode, given=None):
    """The whole call: dict(row_kl [rows], bound [rows], summary [5] (fp64 means over the free rows and the given share), n_free)."""
    rows = len(z)
    given = np.zeros(rows, bool) if given is None else np.asarray(given, bool)
    rs = [None if given[i] else row(z[i], t[i], T, mode) for i in range(rows)]
    free = [r for r in rs if r is not None]
    n = len(free)
    mean = lambda k: float(np.sum([float(r[k]) for r in free]) / n) if n else 0.0      # noqa: E731
    return dict(row_kl=np.array([0.0 if r is None else r["kl"] for r in rs]), bound=np.array([0.0 if r is None else r["bound"] for r in rs]),
                summary=np.array([mean("kl"), mean("teacher_entropy"), mean("entropy"), mean("agree"), (rows - n) / rows]), n_free=n)


def torch_kl(logits, teacher, T, mode, given=None):
    """The mean KL over the free rows on torch tensors (fp64 recommended), differentiable in `logits`: the textbook sum p (log p - log q)
    with the convention 0 log 0 = 0."""
    inv_t = float(S.inv_temperature(T))
    if given is not None:                                  # (the given rows leave before anything is computed: a +inf row has no gradient)
        logits, teacher = logits[~given], teacher[~given]
    ls, lt = torch.log_softmax(logits * inv_t, -1), torch.log_softmax(teacher * inv_t, -1)
    lp, lq = (lt, ls) if mode == 0 else (ls, lt)
    p = lp.exp()
    on, zero = p > 0, torch.zeros_like(p)                  # (the excluded codes are masked BEFORE the product: autograd never sees 0 * inf)
    kl = (p * (torch.where(on, lp, zero) - torch.where(on, lq, zero))).sum(-1)
    return kl.mean() if kl.numel() else kl.sum()
