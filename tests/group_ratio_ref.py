"""fp64 restatement of mage_policy_loss_grouped / mage_policy_loss_grouped_bwd (include/mage_hip_ext.h states the rule), built on
tests/policy_ref.py (the rows, the gradient's shape), tests/policy_kl_ref.py (the anchor) and tests/masked_loss_ref.py's conventions (given:
bool [rows], True where the row's token was given; a given row is never read).

Group g holds rows [g*ratio_div, (g+1)*ratio_div).  A row counts if it is free and inside (logprob != -inf).  Over the counted rows
    n_g = their number,   m_g = mean of d_i = logprob_i - b_i   (+0 for n_g = 0),   rho_g = exp(m_g),
and every counted row takes policy_ref.term's clipped rule with rho_g for its own rho:
    l_i = -min(rho_g A, clamp(rho_g, cmin, cmax) A) - c H_i  [+ kl_coef kl_i],      g_i = -A rho_g where the unclipped term is active, else 0
    [+ kl_coef (1 - exp(r_i - logprob_i))].
The loss is sum_i l_i / n_free; its derivative with respect to logprob_i is g_i / n_free -- NOT g_i / (n_g n_free): all n_g rows of the group
carry -rho_g A and d rho_g / d logprob_i = rho_g / n_g -- so dlogits is policy_ref.dlogits_row's formula with g_i."""
import numpy as np

from tests import policy_kl_ref as Q
from tests import policy_ref as P
from tests import sampling_ref as S
from tests import token_stats_ref as R


def counted(lp, given):
    """bool [rows]: free and inside."""
    lp = np.asarray(lp, np.float64)
    given = np.zeros(len(lp), bool) if given is None else np.asarray(given, bool)
    return ~given & ~np.isneginf(lp)


def reduce(lp, b, given, ratio_div, d=None):
    """(m fp64 [groups], n int64 [groups]).  d: the per-row differences to average (default: lp - b in fp64; a test of the kernel passes the
    kernel's own fp32 differences)."""
    lp = np.asarray(lp, np.float64)
    cnt = counted(lp, given)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(cnt, lp - np.asarray(b, np.float64), 0.0) if d is None else np.where(cnt, np.asarray(d, np.float64), 0.0)
    groups = len(lp) // ratio_div
    assert groups * ratio_div == len(lp)
    n = cnt.reshape(groups, ratio_div).sum(1)
    m = np.zeros(groups)
    for g in range(groups):
        if n[g]:
            m[g] = d[g * ratio_div:(g + 1) * ratio_div][cnt[g * ratio_div:(g + 1) * ratio_div]].sum() / n[g]
    return m, n


def term(lp, H, A, rho, r, cmin, cmax, c, kl_coef, fp32_d=False):
    """One counted or outside row under its group's rho: policy_ref.term's expressions with rho given, then policy_kl_ref.term's anchor (r
    None: the plain rule; d = r - lp in fp64, or fp32_d: as the kernel forms it, one fp32 subtraction)."""
    if np.isneginf(lp):
        return dict(loss=0.0, g=0.0, rho=0.0, outside=True, off=False, kl=0.0, unanchored=False)
    with np.errstate(over="ignore", invalid="ignore"):
        active = (A >= 0 and rho <= cmax) or (A < 0 and rho >= cmin)
        surr = min(rho * A, min(max(rho, cmin), cmax) * A) if not np.isnan(rho) else np.nan
    t = dict(loss=-surr - c * H, g=-A * rho if active else 0.0, rho=rho, outside=False, off=not active, kl=0.0,
             unanchored=r is not None and not np.isfinite(r))
    if r is not None and Q.anchored(lp, r):
        d = Q.delta(lp, r, fp32_d)
        t["kl"] = Q.kl_term(d)
        if kl_coef != 0.0:
            with np.errstate(invalid="ignore"):
                t["loss"] = t["loss"] + kl_coef * t["kl"]
                t["g"] = t["g"] + kl_coef * Q.grad_factor(d)
    return t


def terms(lp, H, A, b, given, ratio_div, cmin, cmax, c, ref=None, kl_coef=0.0, m=None, fp32_d=False):
    """Per-row dicts (None at a given row) plus (m, n) from per-row log-probabilities and entropies; A: one advantage per row.  m: the
    groups' log-ratios to use in place of the restatement's own (a test of the kernel passes the kernel's)."""
    lp = np.asarray(lp, np.float64)
    given = np.zeros(len(lp), bool) if given is None else np.asarray(given, bool)
    m0, n = reduce(lp, b, given, ratio_div)
    m = m0 if m is None else np.asarray(m, np.float64)
    with np.errstate(over="ignore"):
        rho = np.exp(m)
    out = []
    for i in range(len(lp)):
        if given[i]:
            out.append(None)
            continue
        t = term(float(lp[i]), float(H[i]), float(A[i]), float(rho[i // ratio_div]), None if ref is None else float(ref[i]), cmin, cmax, c, kl_coef,
                 fp32_d)
        out.append(dict(logprob=float(lp[i]), entropy=float(H[i]), **t))
    return out, m, n


def forward(z, tok, A, b, temperature, sets, cmin, cmax, c, given, ratio_div, ref=None, kl_coef=0.0):
    """The forward call from logits: per-row dicts (None at a given row), m, n."""
    given = np.zeros(len(tok), bool) if given is None else np.asarray(given, bool)
    lp, H = np.zeros(len(tok)), np.zeros(len(tok))
    for i in np.flatnonzero(~given):
        st = R.stats_for_set(z[i], int(tok[i]), temperature, 0, sets[i])
        lp[i], H[i] = st["policy_logprob"], st["policy_entropy"]
    return terms(lp, H, A, b, given, ratio_div, cmin, cmax, c, ref, kl_coef)


def outputs(rows_):
    """{'logprob', 'entropy', 'loss', 'kl'}: fp64 [rows] with +0 at the given rows."""
    out = {k: np.zeros(len(rows_), np.float64) for k in ("logprob", "entropy", "loss", "kl")}
    for i, row in enumerate(rows_):
        if row is not None:
            for k in out:
                out[k][i] = row[k]
    return out


def summary(rows_, b, with_ref):
    """The masked call's eight values and norm: the seven means over the FREE rows (an outside row counts in the fifth only; the sixth and
    seventh are 0 without a reference), the given share, fp32(1) / fp32(n_free)."""
    free = [(row, float(b[i])) for i, row in enumerate(rows_) if row is not None]
    n = len(free)
    out = np.zeros(8)
    out[7] = (len(rows_) - n) / len(rows_)
    if not n:
        return out, np.float32(0)
    inside = [(r, bb) for r, bb in free if not r["outside"]]
    out[0] = sum(r["loss"] for r, _ in inside) / n
    out[1] = sum(r["entropy"] for r, _ in inside) / n
    out[2] = sum(bb - r["logprob"] for r, bb in inside) / n
    out[3] = sum(1.0 for r, _ in inside if r["off"]) / n
    out[4] = (n - len(inside)) / n
    if with_ref:
        out[5] = sum(r["kl"] for r, _ in inside) / n
        out[6] = sum(1.0 for r, _ in free if r["unanchored"]) / n
    return out, np.float32(1) / np.float32(n)


def dlogits(z, tok, rows_, temperature, sets, c, grad_out):
    """dlogits [rows, K] in fp64: scale inv_t [ g_i (1[j = t] - p_j) + c p_j (log p_j + H_i) ] over the kept set with scale = grad_out /
    n_free, zeros at a given and at an outside row.  policy_ref.dlogits_row's weighted form has g = -A: it is called with A = -g_i."""
    n_free = sum(row is not None for row in rows_)
    out = np.zeros(z.shape, np.float64)
    for i, row in enumerate(rows_):
        if row is None or row["outside"]:
            continue
        out[i] = P.dlogits_row(z[i], int(tok[i]), -row["g"], None, temperature, sets[i], 0.0, 0.0, c, grad_out / n_free)
    return out


def inv_t(temperature):
    return float(S.inv_temperature(temperature))
