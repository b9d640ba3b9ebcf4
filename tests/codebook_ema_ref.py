"""NumPy restatement of mage_code_stats and mage_codebook_ema (include/mage_hip_ext.h): counts and per-code row sums in fp64, the EMA
update with Laplace smoothing, the restart of dead codes (common.h's hash32 and the row pick) and the usage statistics.  Every fp64
operation is one NumPy operation, in the header's order, so the fp32 results agree with the kernel's up to its own roundings."""
import math

import numpy as np

M64 = (1 << 64) - 1
SEED_MUL = 0x9e3779b97f4a7c15


def hash32(v: int) -> int:
    """csrc/common.h: the murmur3 finaliser on a uint64, its low 32 bits."""
    v &= M64
    v ^= v >> 33
    v = (v * 0xff51afd7ed558ccd) & M64
    v ^= v >> 33
    v = (v * 0xc4ceb9fe1a85ec53) & M64
    v ^= v >> 33
    return v & 0xffffffff


def restart_row(seed: int, step: int, K: int, k: int, rows: int) -> int:
    return (hash32((seed * SEED_MUL + step * K + k) & M64) * rows) >> 32


def n_chunks(rows: int) -> int:
    return min(64, (rows + 4095) // 4096)


def code_stats(ids, z, K):
    """(counts int64 [K], sums fp64 [K, D] (exact to fp64), abs fp64 [K, D] = per-code sums of |z|: the error bound's scale).  Ids outside
    [0, K) are counted nowhere.  z None: counts only."""
    ids = np.asarray(ids).reshape(-1)
    ok = (ids >= 0) & (ids < K)
    counts = np.bincount(ids[ok], minlength=K).astype(np.int64)
    if z is None:
        return counts, None, None
    z = np.asarray(z, np.float64)
    sums, mag = np.zeros((K, z.shape[1])), np.zeros((K, z.shape[1]))
    np.add.at(sums, ids[ok], z[ok])
    np.add.at(mag, ids[ok], np.abs(z[ok]))
    return counts, sums, mag


def usage(counts):
    """(perplexity, active, total) of a count vector: k ascending in fp64, a zero count adds nothing."""
    counts = np.asarray(counts, np.int64)
    total = int(counts.sum())
    h = np.float64(0.0)
    for c in counts:
        if c > 0:
            p = np.float64(c) / np.float64(total)
            h = h - p * np.float64(math.log(p))
    return (float(np.exp(h)) if total > 0 else float("nan")), int((counts > 0).sum()), total


def ema_update(codebook, cluster_size, embed_sum, counts, sums, z=None, *, decay, eps, restart_below=0.0, restart_size=None, seed=0, step=0):
    """One update.  Inputs fp32 (sums: the fp32 sums the update is fed), returns dict(codebook, cluster_size, embed_sum (fp32), restarted
    (bool [K]), rows (the row each restarted code took, -1 elsewhere), stats (perplexity, active, restarted, total))."""
    e, N, m = (np.array(a, np.float32, copy=True) for a in (codebook, cluster_size, embed_sum))
    counts = np.asarray(counts, np.int64)
    sums = np.asarray(sums, np.float32)
    K, D = e.shape
    ppl, active, total = usage(counts)
    dead = np.zeros(K, bool)
    picked = np.full(K, -1, np.int64)
    if total == 0:
        return dict(codebook=e, cluster_size=N, embed_sum=m, restarted=dead, rows=picked, stats=(ppl, 0, 0, 0))
    g = np.float64(np.float32(decay))
    omg = np.float64(1.0) - g
    eps64 = np.float64(np.float32(eps))
    Np = (g * N.astype(np.float64) + omg * counts.astype(np.float64)).astype(np.float32)
    mp = (g * m.astype(np.float64) + omg * sums.astype(np.float64)).astype(np.float32)
    n = np.float64(0.0)
    for v in Np:                                                    # k ascending
        n = n + np.float64(v)
    nhat = (Np.astype(np.float64) + eps64) / (n + np.float64(K) * eps64) * n
    with np.errstate(divide="ignore", invalid="ignore"):
        e_new = (mp.astype(np.float64) / nhat[:, None]).astype(np.float32)
    N_new, m_new = Np.copy(), mp
    rb = np.float32(restart_below)
    if rb > 0:
        rs = np.float32(rb if restart_size is None else restart_size)
        z = np.asarray(z, np.float32)
        dead = Np < rb
        for k in np.flatnonzero(dead):
            r = restart_row(seed, step, K, int(k), z.shape[0])
            picked[k] = r
            e_new[k] = z[r, :D]
            N_new[k] = rs
            m_new[k] = (np.float64(rs) * z[r, :D].astype(np.float64)).astype(np.float32)
    return dict(codebook=e_new, cluster_size=N_new, embed_sum=m_new, restarted=dead, rows=picked,
                stats=(ppl, active, int(dead.sum()), total))


def ulps(got, want):
    """Distance in fp32 units in the last place between two fp32 arrays (equal infinities / NaNs count 0)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)

    def key(a):
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(got) - key(want))
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    return np.where(same, 0, d)
