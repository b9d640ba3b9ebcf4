"""fp64 restatement of mage_token_xent / mage_token_xent_bwd (include/mage_hip_ext.h), with the error bounds the GPU tests hold the kernels
to.  numpy, one row at a time; `torch_loss` is the same objective on torch tensors (differentiable: the end-to-end oracle).

The rule for one row of logits z (fp32), target y, class weights w (all ones when None), smoothing eps, z-loss zeta:
  m = max_j z_j (a NaN skipped),  d_j = z_j - m,  e_j = exp(d_j),  Z = sum_j e_j,  lse = m + log Z,  p_j = e_j / Z
  nll = lse - z_y;   smooth = sum_k w_k (lse - z_k);   loss = c1 w_y nll + c2 smooth,  c1 = 1 - eps, c2 = eps / K
  rank = #{j : z_j > z_y} + #{j < y : z_j == z_y} (fp32 comparisons; K when z_y is NaN)
  objective = sum_free loss / sum_free w_y + zeta mean_free lse^2
  gradient of g * objective:  d_k = A p_k - B 1[k = y] - C w_k,  B = g n0 c1 w_y,  C = g n0 c2,  A = B + C W + g n1 2 zeta lse,  W = sum_k w_k,
  n0 = 1 / sum_free w_y, n1 = 1 / n_free (the kernel's fp32 norm values, handed in).
The kernel's coefficients c1, c2 are fp32 roundings of the fp64 values (coefs(fp32=True)); fp32=False keeps them exact, for the comparison
with F.cross_entropy.

Bounds, derived from the kernel's operation count, not from its output.  E24 = 2^-24 is one fp32 rounding, relative; TOL is token_stats_ref's
allowance for one fixed-order fp32 sum of up to 64 adds per lane and 6 butterfly stages, relative to the sum of the terms' magnitudes; expf
and logf are within 2 ulp = 4 E24.
  a weight e_j carries the rounding of d_j and expf's 2 ulp:                       rel(e_j) <= E24 (|d_j| + 4)
  Z carries that, weighted, and its summation:                                     rel(Z)   <= TOL + E24 (E_p|d| + 4)
  lse = m + logf(Z): rel(Z) becomes absolute, logf's 2 ulp, one addition:          |d lse|  <= rel(Z) + 4 E24 |log Z| + E24 |lse|
  nll = z_y - lse, one subtraction:                                                |d nll|  <= |d lse| + E24 |nll|
  smooth: each t_k = lse - z_k carries |d lse| and one rounding, the sum is one fixed-order sum of fmas:
                                                                                   |d smooth| <= sum_k w_k (|d lse| + E24 |t_k|) + TOL sum_k w_k |t_k|
  loss = fma(c2, smooth, (c1 w_y) nll): two products and the fma's rounding:       |d loss| <= c1 w_y (|d nll| + 2 E24 |nll|) + c2 |d smooth| + E24 |loss|
  p_k = e_k * (1 / Z): the division and the product:                               rel(p_k) <= rel(e_k) + rel(Z) + 2 E24
  B three products, C two, W one fixed-order sum (exact without weights), the z term three products and lse's error, two fma roundings:
    |d A| <= 4 E24 (|B| + |C| W + |D|) + TOL |C| W + |g n1 2 zeta| |d lse| + E24 |A|,   D = g n1 2 zeta lse
  d_k = fma(-C, w_k, fma(A, p_k, -B 1[k = y])):
    |d d_k| <= |d A| p_k + |A| p_k rel(p_k) + E24 (|A| p_k + |B| 1[k = y]) + 3 E24 |B| 1[k = y] + 2 E24 |C| w_k + E24 |d_k|
  a bf16 store adds 2^-8 |want|; everything gets the absolute floor 2^-126 (no relative precision below it)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.token_stats_ref import TOL

E24 = 2.0 ** -24
FLOOR = 2.0 ** -126


def coefs(eps, K, fp32=True):
    """(c1, c2) = (1 - eps, eps / K): the kernel's fp32 values (as fp64) or the exact fp64 ones."""
    c1, c2 = 1.0 - float(eps), float(eps) / K
    return (float(np.float32(c1)), float(np.float32(c2))) if fp32 else (c1, c2)


def rank(z, y):
    """The target's rank among the fp32 logits: mage_argmax's order (NaNs never above, -0 == +0, the lower index first on ties)."""
    z = np.asarray(z, np.float32)
    if np.isnan(z[y]):
        return len(z)
    with np.errstate(invalid="ignore"):
        return int((z > z[y]).sum() + (z[:y] == z[y]).sum())


def row(z, y, w=None, eps=0.0, fp32=True):
    """One free row: dict(lse, nll, smooth, loss, rank, wy, b_lse, b_loss, ...) in fp64."""
    z32 = np.asarray(z, np.float32)
    z = z32.astype(np.float64)
    K = len(z)
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    c1, c2 = coefs(eps, K, fp32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.fmax.reduce(z) if not np.isnan(z).all() else -np.inf
        d = z - m
        e = np.exp(d)
        Z = e.sum()
        lz = np.log(Z)
        lse = m + lz
        nll = lse - z[y]
        t = lse - z
        smooth = (w * t).sum() if eps > 0 else 0.0
        loss = c1 * w[y] * nll + (c2 * smooth if eps > 0 else 0.0)
        pos = e > 0
        Ed = (e[pos] * np.abs(d[pos])).sum() / Z
        rel_Z = TOL + E24 * (Ed + 4)
        b_lse = rel_Z + 4 * E24 * abs(lz) + E24 * abs(lse)
        b_nll = b_lse + E24 * abs(nll)
        b_smooth = (w * (b_lse + E24 * np.abs(t))).sum() + TOL * (w * np.abs(t)).sum() if eps > 0 else 0.0
        b_loss = c1 * w[y] * (b_nll + 2 * E24 * abs(nll)) + c2 * b_smooth + E24 * abs(loss) + FLOOR
    return dict(z=z, d=d, e=e, Z=Z, lse=lse, nll=nll, smooth=smooth, loss=loss, rank=rank(z32, y), wy=w[y], w=w, y=y, c1=c1, c2=c2, rel_Z=rel_Z,
                b_lse=b_lse + FLOOR, b_loss=b_loss)


def dlogits_row(r, g, n0, n1, zeta, bf16=False):
    """(want, bound) fp64 [K] for row()'s result r: g = grad_out, n0 / n1 = norm[0] / norm[1] (fp64 from the kernel's fp32 values), zeta fp32."""
    K = len(r["z"])
    w, y = r["w"], r["y"]
    smooth = r["c2"] != 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = r["e"] / r["Z"]
        B = g * n0 * r["c1"] * r["wy"]
        C = g * n0 * r["c2"]
        W = w.sum() if smooth else 0.0
        zc = g * n1 * 2.0 * zeta
        D = zc * r["lse"] if zeta > 0 else 0.0
        A = B + C * W + D
        hot = np.zeros(K)
        hot[y] = 1.0
        want = A * p - B * hot - (C * w if smooth else 0.0)
        dfin = np.where(np.isfinite(r["d"]), np.abs(r["d"]), 0.0)
        rel_p = E24 * (dfin + 4) + r["rel_Z"] + 2 * E24
        bA = 4 * E24 * (abs(B) + abs(C) * W + abs(D)) + TOL * abs(C) * W + abs(zc) * r["b_lse"] + E24 * abs(A)
        bound = (bA * p + abs(A) * p * rel_p + E24 * (abs(A) * p + abs(B) * hot) + 3 * E24 * abs(B) * hot + 2 * E24 * abs(C) * w * smooth
                 + E24 * np.abs(want))
        bound = bound + (2.0 ** -8 * np.abs(want) if bf16 else 0.0) + FLOOR
    return want, bound


def loss(z, target, w=None, eps=0.0, zeta=0.0, given=None, fp32=True):
    """The whole forward call: per-row arrays (0 at the given rows), their bounds, the rows' dicts, n_free, sum_free w_y, and summary [5] in
    fp64 from the restatement's own rows."""
    rows = len(z)
    given = np.zeros(rows, bool) if given is None else np.asarray(given, bool)
    rs = [None if given[i] else row(z[i], int(target[i]), w, eps, fp32) for i in range(rows)]
    free = [r for r in rs if r is not None]
    n = len(free)
    col = lambda k, dt=np.float64: np.array([0 if r is None else r[k] for r in rs], dt)      # noqa: E731
    sw = float(np.sum([r["wy"] for r in free])) if n else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        mean = lambda v: float(np.sum(v) / n) if n else 0.0      # noqa: E731
        lse2 = mean([r["lse"] ** 2 for r in free])
        obj = (float(np.sum([r["loss"] for r in free])) / sw if sw > 0 else 0.0) + (zeta * lse2 if zeta > 0 else 0.0)
        summary = np.array([obj, mean([r["nll"] for r in free]), mean([r["rank"] == 0 for r in free]), lse2, (rows - n) / rows])
    return dict(row_loss=col("loss"), row_nll=col("nll"), row_lse=col("lse"), rank=col("rank", np.int64), b_loss=col("b_loss"), b_lse=col("b_lse"),
                rows=rs, n_free=n, sw=sw, summary=summary)


def norms(sw, n_free):
    """norm[0], norm[1] as the kernel rounds them: (float)(1 / sum w_y) and (float)(1 / n_free), 0 for an empty sum."""
    return np.array([1.0 / sw if sw > 0 else 0.0, 1.0 / n_free if n_free > 0 else 0.0]).astype(np.float32)


def torch_loss(logits, target, w=None, eps=0.0, zeta=0.0, given=None):
    """F.cross_entropy(weight, label_smoothing) over the free rows (ignore_index for the given ones) plus zeta * mean(logsumexp^2) over them;
    differentiable in `logits`."""
    tgt = target if given is None else torch.where(given, torch.full_like(target, -100), target)
    out = F.cross_entropy(logits, tgt, weight=w, ignore_index=-100, label_smoothing=float(eps))
    if zeta > 0:
        lse = torch.logsumexp(logits if given is None else logits[~given], -1)
        out = out + zeta * (lse ** 2).mean()
    return out
