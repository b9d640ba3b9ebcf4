"""fp64 restatement of the masked loss entry points (include/mage_hip_ext.h: mage_policy_loss_masked, mage_policy_loss_masked_bwd,
mage_token_logprob_bwd_masked) on top of the unmasked restatements: gather the free rows, apply tests/policy_ref.py /
tests/preference_ref.py to them, take the means over n_free, put zeros at the given rows.

given: bool [rows], True where the row's token was given (not drawn).  A given row is never read: its logits, token and advantage may hold
anything (NaN, an out-of-range token)."""
import numpy as np
import torch

from tests import policy_ref as P
from tests import preference_ref as PR

ROW_KEYS = ("logprob", "entropy", "loss")


def policy_rows(z, tok, A, b, temperature, sets, cmin, cmax, c, given):
    """Per-row results of the masked forward call: policy_ref.row on every free row (sets[r]: its kept set), None at a given row.  A: one
    advantage per row; b: one behaviour log-probability per row, or None."""
    given = np.asarray(given, bool)
    return [None if given[r] else P.row(z[r], int(tok[r]), float(A[r]), None if b is None else float(b[r]), temperature, sets[r], cmin, cmax, c)
            for r in range(len(given))]


def policy_outputs(rows_, given):
    """{'logprob', 'entropy', 'loss'}: fp64 [rows] with +0 at the given rows."""
    out = {k: np.zeros(len(rows_), np.float64) for k in ROW_KEYS}
    for r, row in enumerate(rows_):
        if not given[r]:
            for k in ROW_KEYS:
                out[k][r] = row[k]
    return out


def policy_summary(rows_, b, given):
    """The masked summary's policy part: policy_ref.summary's five means over the FREE rows (sum / n_free; zeros when nothing is free),
    then the given share over all rows, and norm = fp32(1) / fp32(n_free) (0 when nothing is free) as the library forms it."""
    given = np.asarray(given, bool)
    free = [(row, None if b is None else float(b[r])) for r, row in enumerate(rows_) if not given[r]]
    five = P.summary(free, b is not None) if free else np.zeros(5)
    norm = np.float32(1) / np.float32(len(free)) if free else np.float32(0)
    return five, given.mean() if len(given) else 0.0, norm


def policy_dlogits(z, tok, A, b, temperature, sets, cmin, cmax, c, grad_out, given):
    """dlogits [rows, K] in fp64: policy_ref.dlogits_row with scale = grad_out / n_free at a free row, zeros at a given one."""
    given = np.asarray(given, bool)
    n_free = int((~given).sum())
    out = np.zeros(z.shape, np.float64)
    for r in np.flatnonzero(~given):
        out[r] = P.dlogits_row(z[r], int(tok[r]), float(A[r]), None if b is None else float(b[r]), temperature, sets[r], cmin, cmax, c,
                               grad_out / n_free)
    return out


def token_logprob_bwd(z, tg, c, given, kind="f32"):
    """(dlogits, bound) of mage_token_logprob_bwd_masked, fp64 torch tensors as preference_ref.token_logprob_bwd's (z fp64 [rows, K], tg int64
    [rows], c fp64 [rows]): that function on the free rows, zeros (bound 0) at the given ones."""
    free = ~torch.as_tensor(np.asarray(given, bool))
    out, bound = torch.zeros(z.shape, dtype=torch.float64), torch.zeros(z.shape, dtype=torch.float64)
    if free.any():
        out[free], bound[free] = PR.token_logprob_bwd(z[free], tg[free], c[free], kind)
    return out, bound


def clip_logprobs(token_logprob, given):
    """Per-clip totals over the free slots: token_logprob, given [clips, per_clip]."""
    return np.where(np.asarray(given, bool), 0.0, np.asarray(token_logprob, np.float64)).sum(1)
