"""CPU: per-token policy statistics -- the fp64 restatement (tests/token_stats_ref.py) checked against sampling_ref and logprob_ref, the
extension table (include/mage_hip_ext.h <-> _lib.EXT_SIGNATURES, beside the frozen core table), mage_token_stats' argument checks (refused
before anything is launched) and the model-side switches (set_logprobs(policy=, entropy=)): validation, state, graph fingerprint."""
import math
import os
import re

import numpy as np
import pytest

from mage_amd import _lib
from mage_amd.utils import synth
from tests import logprob_ref as L
from tests import sampling_ref as S
from tests import token_stats_ref as R
from tests.helpers import build_mage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


def _rows(K, n, seed):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((n, K))).astype(np.float32)
    z[::3] = np.round(z[::3] * 4) / 4                               # ties
    return z, g.integers(0, K, n)


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.7, 20, 1.0), (1.5, 0, 0.9), (0.9, 20, 0.9)])
def test_policy_logprob_is_the_log_of_the_target_distribution(T, k, p):
    z, t = _rows(64, 24, seed=k + int(10 * p))
    for r in range(z.shape[0]):
        law = S.target_distribution(z[r], T, k, p)
        N = R.exact_set(z[r], T, k, p)
        assert np.array_equal(N, law > 0)
        lps = np.array([R.stats_for_set(z[r], j, T, k, N)["policy_logprob"] for j in range(64)])
        with np.errstate(divide="ignore"):
            want = np.log(law)
        assert np.array_equal(np.isinf(lps), np.isinf(want)) and np.abs(lps[N] - want[N]).max() < 1e-12
        assert abs(np.exp(lps[N]).sum() - 1.0) < 1e-12              # the kept set carries all the mass
        st = R.row_stats(z[r], int(t[r]), T, k, p)
        assert st["kept"] == int(N.sum()) and abs(st["policy_entropy"] + (law[N] * want[N]).sum()) < 1e-12


def test_unfiltered_at_temperature_1_is_the_token_logprob():
    z, t = _rows(260, 16, seed=3)
    z[2, 5:90] = -INF
    z[4, int(t[4])] = -INF
    for r in range(z.shape[0]):
        st = R.row_stats(z[r], int(t[r]), 1.0, 0, 1.0)
        want = L.token_logprob_row(z[r], int(t[r]))
        assert st["kept"] == 260 and (st["policy_logprob"] == want or abs(st["policy_logprob"] - want) < 1e-12)
        assert abs(st["policy_entropy"] - R.entropy(z[r])) < 1e-12
    assert R.row_stats(z[4], int(t[4]), 1.0, 0, 1.0)["policy_logprob"] == -INF


def test_conventions_by_hand():
    z = np.array([0.0, math.log(3.0), -INF, NAN], np.float32)
    st = R.row_stats(z, 1, 1.0, 0, 1.0)
    h = -(0.25 * math.log(0.25) + 0.75 * math.log(0.75))
    assert st["kept"] == 3 and abs(st["policy_logprob"] - math.log(0.75)) < 1e-7 and abs(st["policy_entropy"] - h) < 1e-7
    assert R.row_stats(z, 3, 1.0, 0, 1.0)["policy_logprob"] == -INF and R.row_stats(z, 2, 1.0, 0, 1.0)["policy_logprob"] == -INF
    assert math.isnan(R.entropy(z)) and abs(R.entropy(z[:3]) - h) < 1e-7        # a NaN poisons the plain entropy only
    st = R.row_stats(z, 0, 1.0, 2, 0.5)                              # top-2 = {0, log 3}; 0.75 >= 0.5: the nucleus is {1}
    assert st["kept"] == 1 and st["policy_logprob"] == -INF and st["policy_entropy"] == 0.0
    assert R.row_stats(z, 1, 1.0, 2, 0.5)["policy_logprob"] == 0.0
    st = R.row_stats(np.full(4, NAN, np.float32), 0, 1.0, 0, 1.0)
    assert st["kept"] == 0 and math.isnan(st["policy_logprob"]) and math.isnan(st["policy_entropy"])
    st = R.row_stats(np.full(4, -INF, np.float32), 0, 1.0, 0, 0.9)
    assert st["kept"] == 4 and math.isnan(st["policy_logprob"]) and math.isnan(st["policy_entropy"])
    st = R.row_stats(np.full(8, 0.5, np.float32), 3, 0.7, 0, 0.9)   # uniform: ties are kept whole
    assert st["kept"] == 8 and abs(st["policy_logprob"] + math.log(8)) < 1e-12 and abs(st["policy_entropy"] - math.log(8)) < 1e-12
    g = np.array([1.0, 3.0, NAN, 3.0], np.float32)                  # greedy: the FIRST maximum alone, whatever the temperature / top_p
    assert [R.row_stats(g, j, 0.3, 1, 0.5)["policy_logprob"] for j in range(4)] == [-INF, 0.0, -INF, -INF]
    assert R.row_stats(g, 1, 0.3, 1, 0.5)["kept"] == 1 and R.row_stats(g, 1, 0.3, 1, 0.5)["policy_entropy"] == 0.0
    assert R.row_stats(np.full(4, NAN, np.float32), 0, 1.0, 1, 1.0)["kept"] == 0


def test_admissible_thresholds():
    # masses from above: 0.5, 0.8, 0.9 (+ 1e-7 off), 1.0 -- top_p = 0.9 sits on a boundary, top_p = 0.85 does not
    law = np.array([0.5, 0.3, 0.1, 0.1 * (1 - 1e-6), 1e-7], np.float64)
    law[2] = 1.0 - law[[0, 1, 3, 4]].sum()
    z = np.log(law).astype(np.float32)
    one = R.admissible_sets(z, 1.0, 0, 0.85)
    assert len(one) == 1 and np.array_equal(one[0], R.exact_set(z, 1.0, 0, 0.85)) and one[0].sum() == 3
    two = R.admissible_sets(z, 1.0, 0, 0.9)
    assert np.array_equal(two[0], R.exact_set(z, 1.0, 0, 0.9)) and sorted(int(q.sum()) for q in two) in ([3, 4], [2, 3], [2, 3, 4])
    assert len(R.admissible_sets(z, 1.0, 2, 1.0)) == 1 and len(R.admissible_sets(z, 1.0, 1, 0.9)) == 1
    # rows that are not `near` have exactly one admissible threshold: the exact tau
    zz, _ = _rows(512, 40, seed=9)
    for r in range(40):
        s = R.scaled(zz[r], 1.5)
        _, near = S.candidates(s, 0, 0.9)
        sets = R.admissible_sets(zz[r], 1.5, 0, 0.9)
        assert near or len(sets) == 1
        sizes = [int(q.sum()) for q in sets]
        assert len(set(sizes)) == len(sizes)                        # nested sets: the size names the threshold


def _ext_header():
    return open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()


def test_extension_table_matches_its_header_and_the_library():
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", _ext_header(), flags=re.M))
    assert declared == set(_lib.EXT_SIGNATURES) and "mage_token_stats" in declared
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.mage_abi_version() == 10
    for name, (res, args) in _lib.EXT_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args


P = 4096                    # a fake, 16-byte aligned device address: every call below is refused before anything is launched
ORDER = ("logits", "rows", "K", "ld", "group", "in_group_stride", "in_off", "tokens", "tok_group_stride", "tok_off", "temperature", "top_k",
         "top_p", "policy_logprob", "policy_entropy", "kept", "entropy")
GOOD = dict(logits=P, rows=8, K=512, ld=512, group=8, in_group_stride=8, in_off=0, tokens=P, tok_group_stride=8, tok_off=0, temperature=1.0,
            top_k=20, top_p=0.9, policy_logprob=P, policy_entropy=P, kept=P, entropy=P)


@pytest.mark.parametrize("bad", [
    dict(policy_logprob=None, policy_entropy=None, kept=None, entropy=None), dict(tokens=None), dict(tokens=None, policy_entropy=None, kept=None),
    dict(logits=None), dict(K=6, ld=8), dict(K=4100, ld=4100), dict(K=0), dict(rows=0), dict(ld=510), dict(ld=256), dict(group=0),
    dict(top_k=-1), dict(top_k=513), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.5), dict(top_p=NAN),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=INF), dict(temperature=NAN), dict(temperature=1e-45),
    dict(logits=P + 4), dict(in_off=-1), dict(tok_off=-1), dict(tok_group_stride=-8), dict(in_group_stride=-8),
])
def test_token_stats_refuses_bad_arguments(bad):
    a = {**GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_token_stats(*[a[k] for k in ORDER], None)
    assert rc == -1 and "mage_token_stats" in lib.mage_last_error().decode(), (bad, rc)


def test_token_stats_accepts_what_the_rule_allows():
    """The accepted forms get past the argument rules: without an initialised device they stop at the mage_init check behind them."""
    lib = _lib.load()
    for ok in (dict(), dict(tokens=None, policy_logprob=None), dict(policy_logprob=None, policy_entropy=None, entropy=None), dict(top_k=0, top_p=1.0),
               dict(top_k=512), dict(top_k=1, temperature=0.5), dict(K=4096, ld=4096), dict(K=4, ld=8, top_k=2)):
        a = {**GOOD, **ok}
        rc = lib.mage_token_stats(*[a[k] for k in ORDER], None)
        assert rc == -1 and "mage_init" in lib.mage_last_error().decode(), (ok, rc, lib.mage_last_error())


def _small():
    return build_mage(synth.mnist_model_config(frames_length=4, width=64, layers=1, vq_dim=32, K=16), 0)


NEW_RESULTS = ("last_token_policy_logprobs", "last_clip_policy_logprob", "last_token_kept", "last_candidate_policy_scores", "last_token_entropy",
               "last_token_policy_entropy")


def test_switches_validate_and_key_the_graph():
    m = _small()
    assert m.logprob_policy is False and m.logprob_entropy is False and all(getattr(m, a) is None for a in NEW_RESULTS)
    assert set(NEW_RESULTS) <= set(m._LOGPROB_RESULTS)
    f0 = m._graph_fingerprint()
    m.set_logprobs(True)
    f1 = m._graph_fingerprint()
    assert m.set_logprobs(True, policy=True) is m and (m.logprobs, m.logprob_policy, m.logprob_entropy) == (True, True, False)
    f2 = m._graph_fingerprint()
    m.set_logprobs(True, entropy=True)
    assert (m.logprobs, m.logprob_policy, m.logprob_entropy) == (True, False, True)
    f3 = m._graph_fingerprint()
    m.set_logprobs(policy=True, entropy=True)
    f4 = m._graph_fingerprint()
    assert len({f0, f1, f2, f3, f4}) == 5
    for kw in (dict(policy=True), dict(entropy=True), dict(policy=True, entropy=True)):
        with pytest.raises(ValueError, match="on=True"):
            m.set_logprobs(False, **kw)
    assert (m.logprobs, m.logprob_policy, m.logprob_entropy) == (True, True, True)      # a refused call changes nothing
    with pytest.raises(TypeError):
        m.set_logprobs(True, True)                                                      # the new flags are keyword-only
    m.set_logprobs(False)                                                               # positional, as existing callers do: clears everything
    assert (m.logprobs, m.logprob_policy, m.logprob_entropy) == (False, False, False) and m._graph_fingerprint() == f0
    m.set_logprobs(True, policy=True)
    with pytest.raises(ValueError, match="set_sampling"):                               # policy describes a sampler: none is on
        m._want_stats()
    m.set_sampling(0.9, top_k=8, top_p=0.9)
    assert m._want_stats() == (True, False)
    m.set_logprobs(True)
    assert m._want_stats() == (False, False)                                            # plain set_logprobs(True): nothing more is launched


def test_latent_model_refuses_the_new_flags():
    m = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)
    for kw in (dict(policy=True), dict(entropy=True)):
        with pytest.raises(ValueError, match="use_cids=False"):
            m.set_logprobs(True, **kw)
    assert (m.logprobs, m.logprob_policy, m.logprob_entropy) == (False, False, False)
