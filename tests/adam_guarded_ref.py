"""fp64 statement of mage_adam_guarded's rule (include/mage_hip_ext.h) on numpy arrays: skip, decay, Adam, EMA.

Inputs are the kernel's fp32 arrays; the constants the kernel forms in fp32 -- 1 - beta1, 1 - beta2, 1 - ema_decay, decay_mul and the scale
rounded from the clip's fp64 coefficient -- enter as those fp32 values, everything else is fp64 and nothing is rounded on the way."""
import math

import numpy as np

F = np.float32


def scale_and_norm(sumsq, grad_scale, max_norm):
    """(scale, norm): the clip's rule from the one value sumsq (None: no sum of squares was taken, the scale is grad_scale)."""
    gs = float(F(grad_scale))
    if sumsq is None:
        return gs, None
    norm = math.sqrt(sumsq) * gs if sumsq >= 0 else float("nan")
    if not max_norm > 0:
        return gs, norm
    coef = float(F(max_norm)) / (norm + 1e-6)
    return (gs if coef >= 1.0 else float(F(gs * coef))), norm


def adam_guarded(p, g, m, v, ema=None, *, n_decay=0, lr, beta1, beta2, eps, step, grad_scale=1.0, decay_mul=1.0, ema_decay=0.0, sumsq=None,
                 max_norm=0.0, skip_nonfinite=False):
    """One call.  p, g, m, v (and ema) are fp32 arrays of one length; returns fp64 (p, m, v, ema or None, norm or None, skipped: bool).  A
    skipped call returns the inputs' values."""
    p, g, m, v = (np.asarray(a, F).astype(np.float64) for a in (p, g, m, v))
    e = None if ema is None else np.asarray(ema, F).astype(np.float64)
    scale, norm = scale_and_norm(sumsq, grad_scale, max_norm)
    if skip_nonfinite:
        assert sumsq is not None
        if not math.isfinite(sumsq):
            return p, m, v, e, norm, True
    b1, b2 = float(F(beta1)), float(F(beta2))
    one_b1, one_b2 = float(F(1) - F(beta1)), float(F(1) - F(beta2))
    i = np.arange(p.size)
    p = np.where(i < n_decay, p * float(F(decay_mul)), p)               # AdamW's order: the decay first
    ge = g * scale
    m = b1 * m + one_b1 * ge
    v = b2 * v + one_b2 * ge * ge
    bc1, bc2_sqrt = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    p = p - (float(F(lr)) / bc1) * (m / (np.sqrt(v) / bc2_sqrt + float(F(eps))))
    if e is not None:
        e = ema_rule(e, p, ema_decay)
    return p, m, v, e, norm, False


def ema_rule(ema_old, p_new, ema_decay):
    """ema = d ema + (1 - d) p_new in fp64, d and 1 - d the kernel's fp32 values."""
    d, one_d = float(F(ema_decay)), float(F(1) - F(ema_decay))
    return d * np.asarray(ema_old, np.float64) + one_d * np.asarray(p_new, np.float64)
