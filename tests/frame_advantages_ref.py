"""The rule of mage_frame_advantages (include/mage_hip_ext.h) restated in numpy: the same fp64 operations in the same order -- the
recursion from the last frame down with the product and the sum rounded separately, returns rounded to fp32 before the statistics, the
statistics added in candidate order -- so that the kernel can be asked for equal bits."""
import numpy as np


def returns(frame_reward, groups, N, gamma):
    """frame_reward [groups*N, T] fp32 -> G fp32 [groups*N, T]: S[t] = r[t] + gamma S[t+1] in fp64 (gamma widened from fp32; gamma == 0
    forms no product), G = S / T rounded once."""
    r = np.asarray(frame_reward, np.float32).reshape(groups * N, -1).astype(np.float64)
    T = r.shape[1]
    g = float(np.float32(gamma))
    S = np.empty_like(r)
    with np.errstate(invalid="ignore", over="ignore"):
        S[:, T - 1] = r[:, T - 1]
        for t in range(T - 2, -1, -1):
            S[:, t] = r[:, t] if g == 0.0 else r[:, t] + g * S[:, t + 1]
        return (S / float(T)).astype(np.float32)


def advantages(G, groups, N, mode, eps, slots=None, slot_off=0):
    """G fp32 [groups*N, T] (the returns as stored) -> advantage fp64 [groups*N, slots]: frame t in slot slot_off + t, +0 elsewhere; per
    (group, frame) the mean and population standard deviation of the N values, added in candidate order; d == 0 gives exactly 0; a
    (group, frame) holding a non-finite return is NaN for all its candidates."""
    G = np.asarray(G, np.float32)
    T = G.shape[-1]
    x = G.reshape(groups, N, T).astype(np.float64)
    slots = slot_off + T if slots is None else slots
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.zeros((groups, T))
        for c in range(N):
            s = s + x[:, c]
        mean = s / float(N)
        q = np.zeros((groups, T))
        for c in range(N):
            d = x[:, c] - mean
            q = q + d * d
        sd = np.sqrt(q / float(N))
        d = x - mean[:, None]
        a = d if mode == 0 else d / (sd[:, None] + float(np.float32(eps)))
        a = np.where(d == 0.0, 0.0, a)
        a = np.where(np.abs(s)[:, None] <= np.finfo(np.float64).max, a, np.nan)
    out = np.zeros((groups * N, slots))
    out[:, slot_off:slot_off + T] = a.reshape(groups * N, T)
    return out


def frame_advantages(frame_reward, groups, N, gamma, mode, eps, slots=None, slot_off=0):
    """(returns fp32 [groups*N, T], advantage fp64 [groups*N, slots])."""
    G = returns(frame_reward, groups, N, gamma)
    return G, advantages(G, groups, N, mode, eps, slots, slot_off)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)
