"""CPU: seeded token sampling -- mage_sample_tokens' argument checks (no device touched), MAGE.set_sampling's validation and state, the graph
fingerprint, the MAGE+ refusal, and the fp64 restatement's own invariants (tests/sampling_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mage_amd import _lib
from mage_amd.utils import synth
from tests import sampling_ref as R
from tests.helpers import build_mage

P = 4096                    # a fake, 16-byte aligned device address: every call below is refused before anything is launched
GOOD = dict(logits=P, rows=8, K=512, ld=512, group=8, in_group_stride=8, in_off=0, out=P, out_group_stride=8, out_off=0, seeds=P,
            pos_off=0, temperature=1.0, top_k=0, top_p=1.0)
ORDER = list(GOOD)


def _call(**kw):
    a = {**GOOD, **kw}
    lib = _lib.load()
    return lib.mage_sample_tokens(*[a[k] for k in ORDER], None), lib.mage_last_error().decode()


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(out=None), dict(seeds=None),
    dict(rows=0), dict(K=0), dict(K=6, ld=8), dict(K=4100, ld=4100), dict(ld=510), dict(ld=256), dict(group=0), dict(logits=P + 4),
    dict(top_k=-1), dict(top_k=513),
    dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001), dict(top_p=math.nan),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf), dict(temperature=math.nan), dict(temperature=1e-45),
])
def test_sample_tokens_refuses_bad_arguments(bad):
    rc, msg = _call(**bad)
    assert rc == -1 and "mage_sample_tokens" in msg, (bad, rc, msg)


def test_abi_version_and_signature():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.mage_abi_version() == 10
    assert "mage_sample_tokens" in _lib.SIGNATURES


def _small():
    return build_mage(synth.mnist_model_config(frames_length=4, width=64, layers=2, vq_dim=32, K=32), 0)


def test_set_sampling_validates_and_restores_greedy():
    m = _small()
    assert m.sampling is None                                           # greedy is the default
    f0 = m._graph_fingerprint()
    assert m.set_sampling(0.8, top_k=5, top_p=0.9) is m and m.sampling == (0.8, 5, 0.9)
    f1 = m._graph_fingerprint()
    m.set_sampling(1.2, top_k=5, top_p=0.9)
    f2 = m._graph_fingerprint()
    assert len({f0, f1, f2}) == 3                                       # a captured graph bakes temperature / top_k / top_p in
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf), dict(temperature=math.nan),
                dict(temperature=1e-320), dict(top_k=-1), dict(top_k=33), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5),
                dict(top_p=math.nan)):
        with pytest.raises(ValueError):
            m.set_sampling(**bad)
        assert m.sampling == (1.2, 5, 0.9)                              # a refused call changes nothing
    m.set_sampling(1.0, top_k=32, top_p=1.0)                            # the edges: top_k = K, top_p = 1 (both off)
    assert m.sampling == (1.0, 32, 1.0)
    assert m.set_sampling(None) is m and m.sampling is None
    assert m._graph_fingerprint() == f0


def test_latent_model_refuses_sampling():
    m = build_mage(synth.magep_model_config(frames_length=4, width=64, layers=3), 0)
    assert not m.use_cids
    with pytest.raises(ValueError, match="use_cids=False"):
        m.set_sampling(1.0)
    assert m.sampling is None
    m.set_sampling(None)                                                # greedy stays allowed


def test_generate_without_gpu_is_still_refused_loudly():
    m = _small().set_sampling(1.0)
    b = synth.synth_batch_mnist(2, 4, seed=0)
    with pytest.raises(RuntimeError):
        m.autoregressive_generate(b)


def test_reference_restatement_invariants():
    # hash32: the splitmix finaliser's 32 low bits (a known value of the mixer, and wrap-around arithmetic)
    assert int(R.hash32(np.uint64(0))) == 0
    u = R.uniforms(-5, 1234, 4096)
    assert u.min() > 0 and u.max() < 1 and np.all((u * 2 ** 24 - 0.5) == np.floor(u * 2 ** 24))
    # the stream depends on (seed, pos, j) only: pos * K + j addresses one counter, so (pos, K) windows tile the counter line
    assert np.array_equal(R.uniforms(7, 3, 8)[4:], R.uniforms(7, 7, 4)) and not np.array_equal(R.uniforms(7, 3, 8), R.uniforms(8, 3, 8))
    z = np.array([1.0, 3.0, 3.0, 2.0, np.nan, -np.inf, 0.5, 3.0], np.float32)
    N, _ = R.candidates(z, 2, 1.0)
    assert N.tolist() == [False, True, True, False, False, False, False, True]      # ties at the top-k boundary are kept
    N, _ = R.candidates(z, 4, 1.0)
    assert N.tolist() == [False, True, True, True, False, False, False, True]
    N, _ = R.candidates(z, 0, 0.5)                                       # mass(>= 3) = 3 / W >= 0.5 W
    assert N.tolist() == [False, True, True, False, False, False, False, True]
    N, _ = R.candidates(z, 0, 1.0)
    assert not N[4] and N.sum() == 7                                    # NaN never; -inf stays a (weightless) member
    p = R.target_distribution(z, 1.0, 0, 1.0)
    assert p[4] == 0 and p[5] == 0 and abs(p.sum() - 1) < 1e-12
    tok, _ = R.sample_row(z, 1.0, 1, 1.0, 0, 0)
    assert tok == 1                                                     # top_k = 1: the first maximum
    draws = [R.sample_row(z, 1.0, 0, 1.0, 11, pos)[0] for pos in range(2000)]
    assert 4 not in draws and 5 not in draws
    torch.manual_seed(0)
