"""CPU: token log-probabilities and clip scores -- the fp64 restatement (tests/logprob_ref.py) pinned on hand-computed rows, the two entry
points' argument checks (refused before anything is launched), and the model-side switches (set_logprobs, set_sampling(candidates=),
score): validation, state, graph fingerprint, the MAGE+ refusals."""
import math

import numpy as np
import pytest

from mage_amd import _lib
from mage_amd.utils import synth
from tests import logprob_ref as R
from tests.helpers import build_mage

INF, NAN = np.inf, np.nan


def test_uniform_row_is_minus_log_k():
    for K in (4, 260, 4096):
        for c in (0.0, -3.5, 80.0):
            assert abs(R.token_logprob_row(np.full(K, c, np.float32), K // 2) + math.log(K)) < 1e-12


def test_one_hot_row_at_80():
    K = 16
    z = np.full(K, -80.0, np.float32)
    z[5] = 80.0
    # logsumexp = 80 + log(1 + 15 e^-160): the hot token ~ 0, any other ~ -160; the naive exp(80) overflows fp32, not this
    assert abs(R.token_logprob_row(z, 5)) < 1e-60 and R.token_logprob_row(z, 5) <= 0.0
    assert abs(R.token_logprob_row(z, 4) + 160.0) < 1e-12


def test_two_values_by_hand():
    z = np.array([0.0, math.log(3.0)], np.float32)
    z3 = float(z[1])
    assert abs(R.token_logprob_row(z, 0) + math.log1p(math.exp(z3))) < 1e-12
    assert abs(R.token_logprob_row(z, 1) - (z3 - math.log1p(math.exp(z3)))) < 1e-12


def test_inf_and_nan_conventions():
    z = np.array([1.0, -INF, 1.0, -INF], np.float32)
    assert abs(R.token_logprob_row(z, 0) + math.log(2.0)) < 1e-12           # -inf logits contribute nothing
    assert R.token_logprob_row(z, 1) == -INF                                # z_t = -inf
    assert math.isnan(R.token_logprob_row(np.array([1.0, NAN, 0.0, 2.0], np.float32), 0))     # one NaN poisons the row
    assert math.isnan(R.token_logprob_row(np.array([1.0, NAN, -INF, 2.0], np.float32), 2))
    assert math.isnan(R.token_logprob_row(np.full(4, -INF, np.float32), 0))                  # no finite logit
    assert math.isnan(R.token_logprob_row(np.array([INF, 0.0, 0.0, 0.0], np.float32), 1))
    got = R.token_logprob(np.array([[0.0, 0.0], [1.0, -INF]], np.float32), np.array([1, 0]))
    assert abs(got[0] + math.log(2.0)) < 1e-12 and got[1] == 0.0


def test_pick_ties_and_nan():
    f = lambda *v: R.pick(np.array(v, np.float32))      # noqa: E731
    assert f(-3.0, -1.0, -1.0, -2.0) == 1               # first of the tied maxima
    assert f(-1.0, -1.0) == 0
    assert f(NAN, -5.0, -4.0) == 2                      # a NaN never wins ...
    assert f(-5.0, NAN, -6.0) == 0
    assert f(NAN, NAN, -INF) == 2                       # ... not even against -inf
    assert f(NAN, NAN, NAN) == 0                        # ... unless nothing else is there
    assert f(-INF, -INF) == 0
    lp = np.zeros((4, 3), np.float32)
    lp[1] = [-1.0, -2.0, -3.0]
    lp[2] = [-3.0, -2.0, -1.0]
    lp[3, 0] = NAN
    exact, s32, best = R.clip_scores(lp, 2, 2)
    assert exact[0].tolist() == [0.0, -6.0] and best.tolist() == [0, 0] and math.isnan(s32[1, 1])


P = 4096                    # a fake, 16-byte aligned device address: every call below is refused before anything is launched
LP_GOOD = dict(logits=P, rows=8, K=512, ld=512, group=8, in_group_stride=8, in_off=0, tokens=P, logprob=P, tok_group_stride=8, tok_off=0)
CS_GOOD = dict(logprob=P, n_clips=2, n_cand=3, per_clip=48, scores=P, best=P)


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(tokens=None), dict(logprob=None), dict(rows=0), dict(K=0), dict(K=6, ld=8), dict(K=4100, ld=4100), dict(ld=510),
    dict(ld=256), dict(group=0), dict(logits=P + 4), dict(in_off=-1), dict(tok_off=-1), dict(tok_group_stride=-8), dict(in_group_stride=-8),
])
def test_token_logprob_refuses_bad_arguments(bad):
    a = {**LP_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_token_logprob(*[a[k] for k in LP_GOOD], None)
    assert rc == -1 and "mage_token_logprob" in lib.mage_last_error().decode(), (bad, rc)


@pytest.mark.parametrize("bad", [dict(logprob=None), dict(scores=None), dict(best=None), dict(n_clips=0), dict(n_cand=0), dict(per_clip=0)])
def test_clip_scores_refuses_bad_arguments(bad):
    a = {**CS_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_clip_scores(*[a[k] for k in CS_GOOD], None)
    assert rc == -1 and "mage_clip_scores" in lib.mage_last_error().decode(), (bad, rc)


def test_entry_points_are_bound():
    assert {"mage_token_logprob", "mage_clip_scores"} <= set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 69
    lib = _lib.load()
    assert lib.mage_abi_version() == _lib.ABI_VERSION


def _small():
    return build_mage(synth.mnist_model_config(frames_length=4, width=64, layers=1, vq_dim=32, K=16), 0)


def test_switches_validate_and_key_the_graph():
    m = _small()
    assert m.logprobs is False and m.candidates == 1 and m.last_token_logprobs is None and m.last_clip_logprob is None
    f0 = m._graph_fingerprint()
    assert m.set_logprobs(True) is m and m.logprobs is True
    f1 = m._graph_fingerprint()
    m.set_logprobs(False)
    assert m._graph_fingerprint() == f0 != f1
    with pytest.raises(ValueError, match="candidates"):
        m.set_sampling(None, candidates=2)                              # candidates need sampling on
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="candidates"):
            m.set_sampling(1.0, candidates=bad)
    assert m.sampling is None and m.candidates == 1                     # a refused call changes nothing
    m.set_sampling(0.9, top_k=8, top_p=0.9)
    f2 = m._graph_fingerprint()
    assert m.set_sampling(0.9, top_k=8, top_p=0.9, candidates=3) is m and m.candidates == 3 and m.sampling == (0.9, 8, 0.9)
    f3 = m._graph_fingerprint()
    assert len({f0, f1, f2, f3}) == 4
    with pytest.raises(ValueError):
        m.set_sampling(0.0, candidates=2)
    assert m.candidates == 3
    m.set_sampling(None)
    assert m.candidates == 1 and m._graph_fingerprint() == f0


def test_latent_model_refuses_logprobs_and_score():
    m = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)
    assert not m.use_cids
    with pytest.raises(ValueError, match="use_cids=False"):
        m.set_logprobs(True)
    assert m.logprobs is False
    m.set_logprobs(False)                                               # off stays allowed
    with pytest.raises(ValueError, match="use_cids=False"):
        m.score(synth.synth_batch_mnist(2, 4, seed=0))


def test_score_without_gpu_is_refused_loudly():
    with pytest.raises(RuntimeError):
        _small().score(synth.synth_batch_mnist(2, 4, seed=0))
