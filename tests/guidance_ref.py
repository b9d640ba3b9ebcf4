"""The rule of mage_guide_logits (include/mage_hip_ext.h) restated exactly, for the CPU and GPU guidance tests.

Per element, in fp32:  w = s - 1;  d = c - u;  z = c where w == 0 or d == 0, else fma(w, d, c) -- ONE rounding of the exact w*d + c.
fma_f32 does that rounding in rational arithmetic (fractions.Fraction): an fp64 `c + w*d` rounds twice (to 53 bits, then to 24) and differs
from the fma where the 53-bit sum lands on an fp32 tie.  guide_rows is the same rule over arrays: where the fp64 sum is EXACT (its TwoSum
error term is zero, the common case: a 48-bit product plus a 24-bit addend of similar magnitude) one rounding of it to fp32 is the fma;
every other element goes through fma_f32.
"""
import math
from fractions import Fraction

import numpy as np

F32_MAX = Fraction((2 ** 24 - 1) * 2 ** 104)


def round_f32(x: Fraction) -> np.float32:
    """The fp32 value nearest to the rational x, ties to even, subnormals and overflow included.  An exact zero is +0 (round to nearest)."""
    if x == 0:
        return np.float32(0.0)
    sign, a = (-1.0 if x < 0 else 1.0), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()              # 2^(e-1) <= a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                              # now 2^e <= a < 2^(e+1)
    ue = max(e - 23, -149)                                                  # exponent of the last place kept
    scaled = a / Fraction(2) ** ue
    q, r = divmod(scaled.numerator, scaled.denominator)
    r2 = 2 * r
    if r2 > scaled.denominator or (r2 == scaled.denominator and q & 1):
        q += 1
    if Fraction(q) * Fraction(2) ** ue > F32_MAX:
        return np.float32(sign * math.inf)
    return np.float32(sign * math.ldexp(float(q), ue))                      # q <= 2^24, ue >= -149: exact in fp64 and in fp32


def fma_f32(w, d, c) -> np.float32:
    """fp32 fma(w, d, c): the exact w*d + c rounded once.  Non-finite operands follow IEEE (NaN propagates, inf - inf and 0 * inf are NaN)."""
    w, d, c = np.float32(w), np.float32(d), np.float32(c)
    if not (np.isfinite(w) and np.isfinite(d) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float32(np.float64(w) * np.float64(d) + np.float64(c))   # an infinite or NaN result: no rounding is involved
    exact = Fraction(float(w)) * Fraction(float(d)) + Fraction(float(c))
    if exact == 0:
        # exact cancellation gives +0; (+-0) * x + (-0) keeps -0 only when the product is a negative zero too
        prod_neg = math.copysign(1.0, float(w)) * math.copysign(1.0, float(d)) < 0
        both_zero = (w == 0 or d == 0) and c == 0
        return np.float32(-0.0) if both_zero and prod_neg and math.copysign(1.0, float(c)) < 0 else np.float32(0.0)
    return round_f32(exact)


def guide_one(c, u, s) -> np.float32:
    """One element of the rule, scalar, through fma_f32."""
    c, u, s = np.float32(c), np.float32(u), np.float32(s)
    with np.errstate(invalid="ignore", over="ignore"):
        w, d = np.float32(s - np.float32(1.0)), np.float32(c - u)
    return c if (w == 0 or d == 0) else fma_f32(w, d, c)


def guide_rows(c: np.ndarray, u: np.ndarray, s: np.ndarray) -> np.ndarray:
    """c, u fp32 [rows, K]; s fp32 [rows] (each row's scale) -> z fp32 [rows, K], bit for bit the rule."""
    c, u = np.ascontiguousarray(c, np.float32), np.ascontiguousarray(u, np.float32)
    s = np.asarray(s, np.float32).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.broadcast_to((s - np.float32(1.0)).astype(np.float32), c.shape)
        d = (c - u).astype(np.float32)
        p = w.astype(np.float64) * d.astype(np.float64)                     # exact: 24 x 24 significand bits
        c64 = c.astype(np.float64)
        t = p + c64
        bb = t - p                                                          # TwoSum: t + err == p + c64 exactly (finite operands)
        err = (p - (t - bb)) + (c64 - bb)
        z = t.astype(np.float32)
    finite = np.isfinite(w) & np.isfinite(d) & np.isfinite(c)
    slow = finite & (err != 0)
    for i in zip(*np.nonzero(slow)):
        z[i] = fma_f32(w[i], d[i], c[i])
    keep = (w == 0) | (d == 0)
    z[keep] = c[keep]
    return z


def f32_bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
