"""NumPy restatement of mage_video_noise's rule (include/mage_hip_ext.h states it; mage_amd/csrc/vq.hip implements it).

For clip b with seed s, channel c, pixel p, in uint64 wrap-around arithmetic:
    e    = c * hw + p;    base = (s ^ 2^63) * 0x9e3779b97f4a7c15
    m1   = hash32(base + 2e) >> 8,   u1 = (m1 + 0.5) 2^-24;    m2 = hash32(base + 2e + 1) >> 9
    z    = sqrt(-2 log u1) * cos(pi (m2 + 0.5) 2^-22)
The integers are exact (numpy uint64); the normal is fp64 (u1 and the angle are exact there: 25 and 24 significant bits).

The keyword arguments of `counters` / `noise` are the MUTANTS tests/test_video_noise_ref_cpu.py holds its checks against; the defaults are
the rule.
"""
import numpy as np

from tests.sampling_ref import GOLDEN_GAMMA, hash32

SEPARATION = np.uint64(0x8000000000000000)      # XORed into the seed: moves the base by exactly 2^63 (the multiplier is odd)
MAX_ABS = float(np.sqrt(2.0 * 25.0 * np.log(2.0)))   # u1 >= 2^-25: |z| <= sqrt(2 log 2^25) = 5.887...


def _u64(seeds) -> np.ndarray:
    return np.asarray(seeds, dtype=np.int64).reshape(-1).view(np.uint64)


def counters(seeds, C: int, hw: int, *, separation=SEPARATION, batch_dependent: bool = False) -> np.ndarray:
    """uint64 [B, C, hw]: the FIRST counter of every element (the second is it + 1)."""
    s = _u64(seeds)
    B = s.shape[0]
    e = np.arange(C * hw, dtype=np.uint64).reshape(1, C, hw)
    with np.errstate(over="ignore"):
        base = ((s ^ np.uint64(separation)) * GOLDEN_GAMMA).reshape(B, 1, 1)
        if batch_dependent:                      # mutant: one running index over the whole launch
            e = e + (np.arange(B, dtype=np.uint64) * np.uint64(C * hw)).reshape(B, 1, 1)
        return base + np.uint64(2) * e


def sampler_counters(seed: int, n_pos: int, K: int) -> np.ndarray:
    """uint64 [n_pos * K]: mage_sample_tokens' counters of positions 0 .. n_pos-1 (tests/sampling_ref.py's `uniforms`, all codes)."""
    s = _u64([seed])[0]
    with np.errstate(over="ignore"):
        return s * GOLDEN_GAMMA + np.arange(n_pos * K, dtype=np.uint64)


def radius_uniform(ctr: np.ndarray, *, round_u1: bool = False) -> np.ndarray:
    """u1, fp64.  round_u1 (mutant): (m1 + 0.5) 2^-24 formed in fp32, where m1 + 0.5 needs 25 bits above 2^23 and is rounded."""
    m1 = hash32(ctr) >> np.uint64(8)
    if round_u1:
        return ((m1.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)
    return (m1.astype(np.float64) + 0.5) * 2.0 ** -24


def angle(ctr: np.ndarray) -> np.ndarray:
    """(m2 + 0.5) 2^-22 in (0, 2), fp64 (exact; exact in fp32 too)."""
    with np.errstate(over="ignore"):
        m2 = hash32(ctr + np.uint64(1)) >> np.uint64(9)
    return (m2.astype(np.float64) + 0.5) * 2.0 ** -22


def noise(seeds, C: int, hw: int, **mutant) -> np.ndarray:
    """fp64 [B, C, hw]: clip b's noise under seeds[b]."""
    round_u1 = mutant.pop("round_u1", False)
    ctr = counters(seeds, C, hw, **mutant)
    u1 = radius_uniform(ctr, round_u1=round_u1)
    with np.errstate(divide="ignore"):
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.pi * angle(ctr))


def rows(z: np.ndarray) -> np.ndarray:
    """[B, C, hw] -> the channel-last rows [B * hw, C]."""
    B, C, hw = z.shape
    return np.ascontiguousarray(z.transpose(0, 2, 1)).reshape(B * hw, C)
