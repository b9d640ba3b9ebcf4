"""CPU: the numpy restatement of mage_frame_advantages (tests/frame_advantages_ref.py) against facts that do not come from the kernel, the
extension table against the header, MAGE.rollout's credit= / gamma= refusals on a CPU model, and the argument rules of the entry point
through the loaded library (nothing is launched)."""
import os
import re

import numpy as np
import pytest

from mage_amd import _lib, ops
from mage_amd.utils import synth
from tests import frame_advantages_ref as F
from tests import video_metrics_ref as R
from tests.helpers import build_mage, count_lib_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _case(seed, groups, N, T):
    """(tests/test_gpu_video_metrics.py's reward generator: a level per candidate plus per-frame noise)"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.2, 0.9, (groups, N, 1)) + 0.05 * rng.standard_normal((groups, N, T))).astype(np.float32).reshape(groups * N, T)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("mode,eps", [(0, 0.0), (1, 1e-6), (1, 0.0), (1, 0.5)])
def test_gamma_one_frame_zero_is_the_clip_level_rule(mode, eps):
    groups, N, T = 5, 8, 15
    fr = _case(1, groups, N, T)
    G, adv = F.frame_advantages(fr, groups, N, 1.0, mode, eps)
    want_r, want_a = R.group_advantages(fr, groups, N, mode, eps)
    assert R.ulps(G[:, 0], want_r.reshape(-1)).max() <= 2                             # the mean reward up to the order of the sum
    # the tolerance tests/test_gpu_video_metrics.py holds that rule's kernel to: 2 fp32 spacings of the value + 1e-14
    tol = 2 * np.spacing(np.abs(want_a).astype(np.float32)).astype(np.float64) + 1e-14
    assert np.all(np.abs(adv[:, 0] - want_a) <= tol) and np.abs(adv[:, 0]).max() > 0


def test_gamma_zero_is_the_immediate_reward():
    groups, N, T = 3, 4, 6
    fr = _case(2, groups, N, T)
    G, adv = F.frame_advantages(fr, groups, N, 0.0, 0, 0.0)
    assert np.array_equal(F.bits(G), F.bits((fr.astype(np.float64) / T).astype(np.float32)))
    g = G.astype(np.float64).reshape(groups, N, T)
    assert np.allclose(adv.reshape(groups, N, T), g - g.mean(1, keepdims=True), rtol=0, atol=1e-15)
    # and by hand, with a discount: two candidates, three frames
    fr = np.array([[1, 2, 4], [3, 2, 0]], np.float32)
    G, adv = F.frame_advantages(fr, 1, 2, 0.5, 0, 0.0)
    assert np.array_equal(G, np.array([[3, 4, 4], [4, 2, 0]], np.float32) / np.float32(3))
    assert np.allclose(adv, np.array([[-0.5, 1, 2], [0.5, -1, -2]]) / 3, rtol=0, atol=1e-7)
    _, adv1 = F.frame_advantages(fr, 1, 2, 0.5, 1, 0.0)
    assert np.allclose(adv1, [[-1, 1, 1], [1, -1, -1]], rtol=0, atol=1e-6)


@pytest.mark.parametrize("gamma", [0.0, 0.9, 1.0])
def test_a_reward_reaches_its_own_and_earlier_frames_only(gamma):
    groups, N, T, s = 3, 4, 7, 3
    fr = _case(3, groups, N, T)
    G, adv = F.frame_advantages(fr, groups, N, gamma, 1, 1e-6)
    fr2 = fr.copy()
    fr2[1 * N + 2, s] += np.float32(0.25)
    G2, adv2 = F.frame_advantages(fr2, groups, N, gamma, 1, 1e-6)
    assert np.array_equal(F.bits(G[:, s + 1:]), F.bits(G2[:, s + 1:])) and np.array_equal(adv[:, s + 1:], adv2[:, s + 1:])
    assert not np.array_equal(G[:, s], G2[:, s]) and not np.array_equal(adv[:, s], adv2[:, s])
    changed = [t for t in range(T) if not np.array_equal(G[:, t], G2[:, t])]
    assert changed == ([s] if gamma == 0.0 else list(range(s + 1)))
    others = np.r_[0:N, 2 * N:3 * N]                                                   # the other groups do not move at all
    assert np.array_equal(adv[others], adv2[others]) and np.array_equal(G[others], G2[others])


@pytest.mark.parametrize("mode,eps", [(0, 0.0), (1, 0.0)])
@pytest.mark.parametrize("gamma", [0.0, 0.9, 1.0])
def test_equal_candidates_give_plus_zero(mode, eps, gamma):
    groups, N, T = 2, 5, 4
    fr = _case(4, groups, N, T).reshape(groups, N, T)
    fr[1] = np.float32(0.3)                                                            # not a binary fraction: the mean must still be exact
    fr[0, :, 2:] = fr[0, :1, 2:]                                                       # group 0: equal from frame 2 on
    _, adv = F.frame_advantages(fr.reshape(groups * N, T), groups, N, gamma, mode, eps)
    adv = adv.reshape(groups, N, T)
    assert np.array_equal(adv[1].view(np.int64), np.zeros((N, T), np.int64))           # +0 bits
    assert np.array_equal(adv[0, :, 2:].view(np.int64), np.zeros((N, 2), np.int64))
    assert np.all(adv[0, :, 0] != 0) and np.isfinite(adv).all()


def test_slots_outside_the_window_are_plus_zero():
    groups, N, T = 3, 4, 12
    fr = _case(5, groups, N, T)
    G, adv = F.frame_advantages(fr, groups, N, 0.9, 1, 1e-6, slots=15, slot_off=3)    # the layout of context=4 at 16 frames
    assert adv.shape == (groups * N, 15) and np.array_equal(adv[:, :3].view(np.int64), np.zeros((groups * N, 3), np.int64))
    assert np.array_equal(adv[:, 3:], F.advantages(G, groups, N, 1, 1e-6))
    _, wide = F.frame_advantages(fr, groups, N, 0.9, 1, 1e-6, slots=20, slot_off=4)
    assert np.array_equal(wide[:, 4:16], adv[:, 3:]) and not wide[:, :4].any() and not wide[:, 16:].any()
    assert not np.signbit(wide[:, :4]).any() and not np.signbit(wide[:, 16:]).any()


def test_a_non_finite_reward_stays_in_its_group_and_its_frames():
    groups, N, T, s = 4, 5, 6, 2
    for gamma in (0.0, 0.9, 1.0):
        fr = _case(6, groups, N, T).reshape(groups, N, T)
        fr[2, 3, s] = INF
        fr[3, 0, T - 1] = NAN
        G, adv = F.frame_advantages(fr.reshape(groups * N, T), groups, N, gamma, 1, 1e-6)
        nan = np.isnan(adv.reshape(groups, N, T))
        want = np.zeros((groups, N, T), bool)
        want[2, :, s if gamma == 0.0 else slice(0, s + 1)] = True
        want[3, :, T - 1 if gamma == 0.0 else slice(0, T)] = True
        assert np.array_equal(nan, want), gamma
        assert np.isfinite(adv.reshape(groups, N, T)[:2]).all() and np.isfinite(G.reshape(groups, N, T)[2, :3]).all()


# ---------------------------------------------------------------- the extension table
def test_the_header_declares_what_the_table_binds():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    name = "mage_frame_advantages"
    assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES and len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M | re.S).group(1)
    C = {"const float*": _lib.C.c_void_p, "float*": _lib.C.c_void_p, "void*": _lib.C.c_void_p, "int64_t": _lib.C.c_int64, "int32_t": _lib.C.c_int32,
         "float": _lib.C.c_float}
    declared = [C[a.strip().rsplit(" ", 1)[0]] for a in decl.split(",")]
    names = [a.strip().rsplit(" ", 1)[1] for a in decl.split(",")]
    assert names == ["frame_reward", "groups", "N", "T", "gamma", "mode", "eps", "slots", "slot_off", "returns", "advantage", "stream"]
    res, args = _lib.EXT_SIGNATURES[name]
    assert res is _lib.C.c_int and args == declared
    fn = getattr(_lib.load(), name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert "frame_advantages" in ops.__all__ and callable(ops.frame_advantages)


# ---------------------------------------------------------------- Python refusals on a CPU model
def test_rollout_refuses_a_bad_credit_or_gamma_before_anything_else(monkeypatch):
    counted = count_lib_calls(monkeypatch, _lib.load())
    L = 4
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=16), 0)
    batch = synth.synth_batch_mnist(2, L, seed=0)
    m.set_sampling(0.9, top_k=8)
    state = lambda: (m.sampling, m.candidates, m.logprobs, m.logprob_policy, m.logprob_entropy, m.context_frames)      # noqa: E731
    before = state()
    for match, kw in [("credit", dict(credit="token")), ("credit", dict(credit=None)), ("gamma", dict(credit="frame", gamma=-0.5)),
                      ("gamma", dict(credit="frame", gamma=1.5)), ("gamma", dict(credit="frame", gamma=NAN)), ("gamma", dict(credit="frame", gamma=INF)),
                      ("gamma", dict(credit="frame", gamma="1")), ("gamma", dict(credit="frame", gamma=True)), ("gamma", dict(gamma=0.9)),
                      ("gamma", dict(credit="clip", gamma=0.0)), ("GPU", dict(credit="frame", gamma=0.9)), ("GPU", dict(credit="clip", gamma=1))]:
        with pytest.raises(ValueError, match=match):
            m.rollout(batch, 3, **kw)
        assert counted == [] and state() == before, kw


# ---------------------------------------------------------------- argument rules (refused before anything is launched)
P = 4096                    # a fake, aligned device address
FA_ORDER = ("frame_reward", "groups", "N", "T", "gamma", "mode", "eps", "slots", "slot_off", "returns", "advantage")
FA_GOOD = dict(frame_reward=P, groups=4, N=3, T=5, gamma=0.9, mode=1, eps=1e-6, slots=8, slot_off=2, returns=P, advantage=P)


@pytest.mark.parametrize("bad", [
    dict(frame_reward=None), dict(returns=None), dict(advantage=None), dict(groups=0), dict(groups=-1), dict(N=1), dict(N=0), dict(T=0), dict(T=-2),
    dict(slot_off=-1), dict(slots=6), dict(slots=0), dict(slots=-1), dict(slot_off=4), dict(slot_off=2 ** 31 - 1, slots=2 ** 31 - 1),
    dict(groups=2 ** 31), dict(groups=2 ** 29, N=2, slots=2, slot_off=0, T=2), dict(groups=2 ** 20, N=2 ** 10, slots=8), dict(groups=2 ** 40),
    dict(gamma=-1e-6), dict(gamma=1.0000001), dict(gamma=NAN), dict(gamma=INF), dict(gamma=-INF), dict(mode=2), dict(mode=-1), dict(eps=-1e-6),
    dict(eps=INF), dict(eps=NAN), dict(frame_reward=P + 2), dict(returns=P + 1), dict(advantage=P + 3),
])
def test_frame_advantages_refuses_bad_arguments(bad):
    a = {**FA_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_frame_advantages(*[a[k] for k in FA_ORDER], None)
    assert rc == -1 and "mage_frame_advantages" in lib.mage_last_error().decode(), (bad, rc)
