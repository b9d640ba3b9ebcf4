"""GPU: mage_frame_advantages against its fp64 restatement (tests/frame_advantages_ref.py) at the smallest shapes where it can go wrong --
one frame, more candidates than lanes, padded slots on both sides, many groups -- and the bitwise properties include/mage_hip_ext.h
promises.

Bounds.  returns: equal bits -- the restatement performs the kernel's fp64 operations in the kernel's order (the file contracts nothing,
fp64 division is correctly rounded).  advantage against the restatement applied to the rewards: the tolerance of
test_group_advantages_match_the_restatement, 2 fp32 spacings of the expected value + 1e-14.  advantage against the restatement applied to
the GPU's own returns: equal bits (sums in candidate order, correctly rounded fp64 division and square root on both sides)."""
import functools

import numpy as np
import pytest
import torch

from mage_amd import ops
from tests import frame_advantages_ref as F
from tests.test_gpu_video_metrics import _adv_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (groups, N, T, slots, slot_off): the smallest call; odd sizes; cfg2's 15 generated frames; 31 frames; lanes wrap (N > 64) with padded slots
# on both sides; more groups than CUs; the context=4 layout of 16 frames
SHAPES = [(1, 2, 1, 1, 0), (3, 3, 4, 4, 0), (5, 8, 15, 15, 0), (4, 5, 31, 31, 0), (2, 130, 3, 7, 4), (700, 4, 2, 2, 0), (3, 4, 12, 15, 3)]
MODES = [(0, 0.0), (1, 1e-6), (1, 0.0), (1, 0.5)]
GAMMAS = [0.0, 0.9, 1.0]


@functools.lru_cache(maxsize=None)
def rewards(groups, N, T):
    fr = _adv_case(groups * 1000 + N, groups, N, T)
    fr.setflags(write=False)                                                           # shared: nobody changes it
    return fr


def run(fr, groups, N, gamma, mode, eps, slots=None, slot_off=0):
    ret, adv = ops.frame_advantages(torch.tensor(fr, device=DEV), groups=groups, n_cand=N, gamma=gamma, mode=mode, eps=eps, slots=slots,
                                    slot_off=slot_off)
    return ret.cpu().numpy(), adv.cpu().numpy()


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("mode,eps", MODES)
@pytest.mark.parametrize("groups,N,T,slots,slot_off", SHAPES)
def test_frame_advantages_match_the_restatement(groups, N, T, slots, slot_off, mode, eps, gamma):
    fr = rewards(groups, N, T)
    ret, adv = run(fr, groups, N, gamma, mode, eps, slots, slot_off)
    ret2, adv2 = run(fr, groups, N, gamma, mode, eps, slots, slot_off)
    assert ret.shape == (groups * N, T) and adv.shape == (groups * N, slots)
    assert np.array_equal(F.bits(ret), F.bits(ret2)) and np.array_equal(F.bits(adv), F.bits(adv2))          # two launches
    want_r, want_a = F.frame_advantages(fr, groups, N, gamma, mode, eps, slots, slot_off)
    got = adv.astype(np.float64)
    tol = 2 * np.spacing(np.abs(want_a).astype(np.float32)).astype(np.float64) + 1e-14
    print(f"returns: {np.count_nonzero(F.bits(ret) != F.bits(want_r))} of {ret.size} differ in bits; advantage worst error / tolerance "
          f"{np.max(np.abs(got - want_a) / tol):.3f}")
    assert np.array_equal(F.bits(ret), F.bits(want_r))
    assert np.all(np.abs(got - want_a) <= tol) and np.abs(got).max() > 0
    # advantage is a function of returns alone: the restatement on the GPU's own returns, bit for bit
    own = F.advantages(ret, groups, N, mode, eps, slots, slot_off).astype(np.float32)
    assert np.array_equal(F.bits(adv), F.bits(own))
    # the slots outside the window are +0
    pad = np.r_[0:slot_off, slot_off + T:slots].astype(np.int64)
    assert np.array_equal(F.bits(adv[:, pad]), np.zeros((groups * N, pad.size), np.int32))
    # a group computed alone, as groups = 1, has the same bits
    for g in sorted({0, groups // 2, groups - 1}):
        r1, a1 = run(fr[g * N:(g + 1) * N], 1, N, gamma, mode, eps, slots, slot_off)
        assert np.array_equal(F.bits(r1), F.bits(ret[g * N:(g + 1) * N])) and np.array_equal(F.bits(a1), F.bits(adv[g * N:(g + 1) * N]))


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("groups,N,T,slots,slot_off", [(3, 3, 4, 4, 0), (2, 130, 3, 7, 4), (3, 4, 12, 15, 3)])
def test_a_reward_reaches_its_own_and_earlier_frames_only(groups, N, T, slots, slot_off, gamma):
    fr = rewards(groups, N, T)
    s, row = T // 2, 1 * N + N - 1                                                     # (the last candidate of group 1: a wrapped lane at N = 130)
    fr2 = fr.copy()
    fr2[row, s] += np.float32(0.25)
    ret, adv = run(fr, groups, N, gamma, 1, 1e-6, slots, slot_off)
    ret2, adv2 = run(fr2, groups, N, gamma, 1, 1e-6, slots, slot_off)
    same_r = [np.array_equal(F.bits(ret[:, t]), F.bits(ret2[:, t])) for t in range(T)]
    same_a = [np.array_equal(F.bits(adv[:, j]), F.bits(adv2[:, j])) for j in range(slots)]
    moved = [s] if gamma == 0.0 else list(range(s + 1))
    assert [t for t in range(T) if not same_r[t]] == moved
    assert [j for j in range(slots) if not same_a[j]] == [slot_off + t for t in moved]
    others = np.r_[0:N, 2 * N:groups * N]
    assert np.array_equal(F.bits(adv[others]), F.bits(adv2[others])) and np.array_equal(F.bits(ret[others]), F.bits(ret2[others]))


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("mode,eps", [(0, 0.0), (1, 0.0), (1, 1e-6)])
def test_equal_candidates_give_zero_and_a_non_finite_reward_stays_in_its_group_and_frames(mode, eps, gamma):
    groups, N, T, s = 4, 5, 6, 2
    fr = _adv_case(7, groups, N, T).reshape(groups, N, T)
    fr[1] = np.float32(0.3)                                                            # 0.3 is not a binary fraction: the mean must still be exact
    fr[0, :, 4:] = fr[0, :1, 4:]                                                       # group 0: equal from frame 4 on
    fr[2, 3, s] = np.inf
    fr[3, 0, T - 1] = np.nan
    ret, adv = run(fr.reshape(groups * N, T), groups, N, gamma, mode, eps, slots=T + 3, slot_off=1)
    adv, ret = adv.reshape(groups, N, T + 3), ret.reshape(groups, N, T)
    assert np.array_equal(F.bits(adv[1]), np.zeros((N, T + 3), np.int32))              # exactly +0
    assert np.array_equal(F.bits(adv[0, :, 5:]), np.zeros((N, 4), np.int32)) and np.all(adv[0, :, 1] != 0)
    assert np.array_equal(F.bits(adv[:, :, [0, T + 1, T + 2]]), np.zeros((groups, N, 3), np.int32))         # the padding, NaN groups included
    want = np.zeros((groups, N, T), bool)
    want[2, :, s if gamma == 0.0 else slice(0, s + 1)] = True
    want[3, :, T - 1 if gamma == 0.0 else slice(0, T)] = True
    assert np.array_equal(np.isnan(adv[:, :, 1:T + 1]), want) and np.isfinite(adv[:2]).all()
    assert ret[2, 3, s] == np.inf and np.isnan(ret[3, 0, T - 1]) and np.isfinite(ret[:2]).all()
    ref = F.frame_advantages(fr.reshape(groups * N, T), groups, N, gamma, mode, eps, T + 3, 1)[1].reshape(groups, N, T + 3)
    assert np.allclose(adv[0], ref[0], rtol=1e-6, atol=0)
