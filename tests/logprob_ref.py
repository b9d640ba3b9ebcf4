"""NumPy / fp64 restatement of mage_token_logprob and mage_clip_scores (include/mage_hip.h states both rules).

Token log-probability of one row of fp32 logits z at token t: lp = z_t - (m + log sum_j exp(z_j - m)), m = max_j z_j, everything in fp64.
-inf logits add exp(-inf) = 0; a NaN logit, or a row with no finite maximum (every logit -inf, or a +inf: inf - inf), gives NaN; z_t = -inf
gives -inf.  Clip scores: the fp64 sum of a candidate's per_clip values rounded once to fp32; the pick is the largest score, the smallest
index on ties, a NaN only when every score of the clip is NaN (then candidate 0).
"""
import numpy as np


def token_logprob_row(z: np.ndarray, t: int) -> float:
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.max(z)                                               # NaN if any logit is NaN
        lse = m + np.log(np.sum(np.exp(z - m)))
        return float(z[t] - lse)


def token_logprob(z: np.ndarray, tokens: np.ndarray) -> np.ndarray:
    """z [rows, K] fp32, tokens [rows] -> fp64 [rows]."""
    z = np.asarray(z, dtype=np.float32)
    return np.array([token_logprob_row(z[r], int(tokens[r])) for r in range(z.shape[0])], dtype=np.float64)


def pick(scores: np.ndarray) -> int:
    """The winner of one clip's scores: largest, first on ties, NaN never unless all are."""
    best, bs = 0, scores[0]
    for c in range(1, len(scores)):
        s = scores[c]
        if s > bs or (np.isnan(bs) and not np.isnan(s)):
            best, bs = c, s
    return best


def clip_scores(logprob: np.ndarray, n_clips: int, n_cand: int):
    """logprob [n_clips * n_cand, per_clip] fp32 -> (fp64 sums [n_clips, n_cand], their fp32 roundings, winners int64 [n_clips])."""
    lp = np.asarray(logprob, dtype=np.float32).reshape(n_clips, n_cand, -1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        exact = lp.sum(-1)
    s32 = exact.astype(np.float32)
    return exact, s32, np.array([pick(s32[b]) for b in range(n_clips)], dtype=np.int64)
