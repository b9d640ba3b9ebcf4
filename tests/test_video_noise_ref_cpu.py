"""CPU: the restatement of mage_video_noise's rule (tests/video_noise_ref.py) on its own -- the GPU kernel is held to it, so it has to be a
standard normal, a function of (seed, channel, pixel) alone, and disjoint from the sampler's counter stream of the same seed.  Fixed seeds,
B = 5, C = 64, hw = 256 (n = 81 920 values): the statistical checks are 5-sigma conditions on fixed inputs, not measurements.  Each check
is a function, and each mutant of the rule (the separation dropped, the counter depending on the batch, u1 rounded) fails the one named
beside it."""
import numpy as np
import pytest

from tests import video_noise_ref as R

SEEDS = [0, -1, -2 ** 63, 20240917, -7046029254386353131]
B, C, HW, K = 5, 64, 256, 64
N = B * C * HW


@pytest.fixture(scope="module")
def z():
    out = R.noise(SEEDS, C, HW)
    out.setflags(write=False)
    return out


def lag1(z, axis):
    a, b = np.take(z, range(z.shape[axis] - 1), axis), np.take(z, range(1, z.shape[axis]), axis)
    return float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])


def check_moments(z):
    """mean 0 and variance 1 to 5 sigma (the variance of a normal's sample variance is 2 / n), inside the Box-Muller bound."""
    assert z.shape == (B, C, HW) and np.isfinite(z).all()
    mean, var, top = float(z.mean()), float(z.var()), float(np.abs(z).max())
    print(f"mean {mean:+.3e} (bound {5 / np.sqrt(N):.3e}), var - 1 {var - 1:+.3e} (bound {5 * np.sqrt(2 / N):.3e}), max |z| {top:.4f}")
    assert abs(mean) < 5 / np.sqrt(N)
    assert abs(var - 1) < 5 * np.sqrt(2 / N)
    assert top <= 5.89 and top <= R.MAX_ABS


def check_uncorrelated(z):
    """lag-1 correlation along the clip, channel and pixel axes, each below 5 / sqrt(n)."""
    for axis, name in ((0, "clip"), (1, "channel"), (2, "pixel")):
        r = lag1(z, axis)
        print(f"lag-1 correlation along the {name} axis {r:+.3e} (bound {5 / np.sqrt(N):.3e})")
        assert abs(r) < 5 / np.sqrt(N), name


def check_clips_differ(z):
    for i in range(z.shape[0]):
        for j in range(i + 1, z.shape[0]):
            assert not np.array_equal(z[i], z[j]) and (z[i] != z[j]).mean() > 0.99, (i, j)


def check_batch_invariance(gen):
    """a clip's values depend on its seed alone: not on B, nor on its place in the batch."""
    whole = gen(SEEDS)
    for b in (0, 2, B - 1):
        assert np.array_equal(gen(SEEDS[b:b + 1])[0], whole[b]), b
    assert np.array_equal(gen(SEEDS[::-1])[::-1], whole)
    assert np.array_equal(gen([SEEDS[4]] * 3)[2], whole[4])


def check_separation(counters):
    """for every seed the sampler's first hw * K counters (K = 64) and the noise's (both of every element) are disjoint sets."""
    for seed in SEEDS:
        first = counters([seed], C, HW).reshape(-1)
        with np.errstate(over="ignore"):
            mine = np.concatenate([first, first + np.uint64(1)])
        assert np.unique(mine).size == 2 * C * HW                     # and no element shares a counter with another
        theirs = R.sampler_counters(seed, HW, K)
        assert np.intersect1d(mine, theirs).size == 0, seed


def check_u1_exact(radius_uniform):
    """u1 = (m1 + 0.5) 2^-24 is an odd multiple of 2^-25 strictly inside (0, 1): never rounded, never 0 or 1."""
    u = radius_uniform(R.counters(SEEDS, C, HW))
    t = u * 2.0 ** 25
    assert ((u > 0) & (u < 1)).all() and np.array_equal(t, np.floor(t)) and (t.astype(np.int64) % 2 == 1).all()
    assert (u >= 0.5).mean() > 0.4                                    # the upper half, where fp32 could not hold u1, is exercised


def test_moments(z):
    check_moments(z)


def test_uncorrelated(z):
    check_uncorrelated(z)


def test_clips_differ(z):
    check_clips_differ(z)


def test_batch_invariance():
    check_batch_invariance(lambda s: R.noise(s, C, HW))


def test_separation_from_the_sampler():
    check_separation(R.counters)
    # the stated reason: the two bases of one seed are exactly 2^63 apart
    for seed in SEEDS:
        with np.errstate(over="ignore"):
            d = R.counters([seed], 1, 1).reshape(-1)[0] - R.sampler_counters(seed, 1, 1)[0]
        assert d == np.uint64(2 ** 63)


def test_u1_is_never_rounded():
    check_u1_exact(R.radius_uniform)


def test_layouts_and_angle():
    zz = R.noise(SEEDS[:2], 4, 7)
    rows = R.rows(zz)
    assert rows.shape == (2 * 7, 4) and rows[7 + 3, 2] == zz[1, 2, 3]
    a = R.angle(R.counters(SEEDS, C, HW))
    assert ((a > 0) & (a < 2)).all() and np.array_equal(a.astype(np.float32).astype(np.float64), a)   # exact in fp32
    assert (np.abs(a - 0.5) >= 2.0 ** -23).all() and (np.abs(a - 1.5) >= 2.0 ** -23).all()           # the cosine is never 0


# ---- mutants: each breaks the rule in one way and must fail the check that guards it
def test_mutant_separation_dropped_fails_the_separation_check():
    with pytest.raises(AssertionError):
        check_separation(lambda s, c, hw: R.counters(s, c, hw, separation=0))


def test_mutant_batch_dependent_counter_fails_batch_invariance():
    mutant = lambda s: R.noise(s, C, HW, batch_dependent=True)      # noqa: E731
    check_moments(mutant(SEEDS))                                      # (still a fine normal: only the invariance check can see it)
    with pytest.raises(AssertionError):
        check_batch_invariance(mutant)


def test_mutant_rounded_u1_fails_the_exactness_check():
    with pytest.raises(AssertionError):
        check_u1_exact(lambda ctr: R.radius_uniform(ctr, round_u1=True))


# ---- the entry point's argument rules (refused before anything is launched: no GPU needed, the pointers are fake)
P = 4096
VN_ORDER = ("seeds", "B", "C", "hw", "nchw", "rows")
VN_GOOD = dict(seeds=P, B=3, C=64, hw=256, nchw=P, rows=P)


@pytest.mark.parametrize("bad", [
    dict(seeds=None), dict(seeds=P + 4), dict(B=0), dict(B=-1), dict(C=0), dict(C=-64), dict(hw=0), dict(hw=-1), dict(nchw=None, rows=None),
    dict(nchw=P + 4), dict(rows=P + 8), dict(nchw=None, rows=P + 4), dict(C=2 ** 20, hw=2 ** 11), dict(hw=2 ** 31), dict(hw=2 ** 40),
    dict(B=2 ** 25), dict(B=2 ** 62),
])
def test_video_noise_refuses_bad_arguments(bad):
    from mage_amd import _lib
    a = {**VN_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_video_noise(*[a[k] for k in VN_ORDER], None)
    assert rc == -1 and "mage_video_noise" in lib.mage_last_error().decode(), (bad, rc)


def test_the_extension_table_declares_it():
    from mage_amd import _lib
    assert "mage_video_noise" in _lib.EXT_SIGNATURES and len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    assert len(_lib.EXT_SIGNATURES["mage_video_noise"][1]) == 7
