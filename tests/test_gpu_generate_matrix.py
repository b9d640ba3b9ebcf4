"""GPU, bitwise: the two AR loops of MAGE.autoregressive_generate against each other across COMBINATIONS of the generation features (each
feature's own file does it for that feature alone): sampler x set_logprobs x guidance x given tokens x batch size, fully crossed.
The model is small on purpose -- frames_length 4 (a first, a middle and a last slot), 3 axial blocks (one of each axis), width 256 (the
LayerNorm-fold route) -- in bf16, eager, one stream, fixed seeds; B = 1 and B = 2 (B = 1 is a view where B > 1 is a copy when the
incremental loop's frame-major results turn clip-major)."""
import pytest
import torch

from mage_amd.modules.mage_model import MAGE
from mage_amd.utils import synth
from tests.helpers import build_mage
from tests.test_gpu_context_invariants import LAST, _bits, _nolog, _run, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 4
SAMPLERS = {"greedy": None, "sampled": dict(candidates=1), "best_of_3": dict(candidates=3)}
GIVEN = ("free", "context2", "context3", "known")


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, width=256, layers=3), 0, DEV).set_precision("bf16")
    batch = {k: v.to(DEV) for k, v in synth.synth_batch_mnist(2, L, seed=5).items()}
    seeds = torch.tensor([4242, -977], dtype=torch.int64, device=DEV)
    R_, K = m.image_resolution, m.codebook_size
    g = torch.Generator().manual_seed(17)
    known = torch.full((2, L - 1, R_, R_), -1, dtype=torch.int64)
    sc = torch.rand(2, L - 1, R_, R_, generator=g) < 0.2                    # scattered slots of every frame ...
    sc[:, L - 2, 3, 5] = True                                               # ... one of them certainly in the last frame
    known[sc] = torch.randint(0, K, known.shape, generator=g)[sc]
    assert set(LAST) == set(MAGE._LOGPROB_RESULTS)                          # _same compares every generation result
    return m, batch, seeds, known.to(DEV)


def _reset(m):
    m.set_precision("bf16").set_guidance(None).set_sampling(None).set_logprobs(False).set_context(1)
    m.use_graph, m.streams, m.ar_mode, m.context_prefill = False, 1, "incremental", True


def _configure(m, sampler, logprobs, guided, given):
    """The settings of one cell; returns whether the call takes seeds."""
    _reset(m)
    sampled = SAMPLERS[sampler] is not None
    if sampled:
        m.set_sampling(1.0, top_k=50, top_p=0.95, **SAMPLERS[sampler])
    if logprobs:
        m.set_logprobs(True, policy=sampled, entropy=True)                  # (policy describes a sampler: only with sampling on)
    if guided:
        m.set_guidance(1.5)
    m.set_context({"context2": 2, "context3": L - 1}.get(given, 1))
    return sampled


def _call(m, mode, batch, seeds, extra):
    """One call in `mode`: (_run's results without last_logits, last_known_mask)."""
    m.ar_mode = mode
    r = _run(m, batch, seeds, **extra)
    assert (r[2] is None) == (mode == "incremental")                        # the incremental loop keeps no logits
    return _nolog(r), m.last_known_mask


def _assert_same(a, b, what):
    (ra, ma), (rb, mb) = a, b
    assert _same(ra, rb), what
    assert (ma is None) == (mb is None) and (ma is None or torch.equal(ma, mb)), what


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("logprobs", [False, True], ids=["nolp", "lp"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_incremental_equals_full(small, sampler, logprobs, guided, given, B):
    m, batch, seeds, known = small
    try:
        sampled = _configure(m, sampler, logprobs, guided, given)
        b = {k: v[:B] for k, v in batch.items()}
        s = seeds[:B] if sampled else None
        extra = {"known_tokens": known[:B]} if given == "known" else {}
        full, inc = _call(m, "full", b, s, extra), _call(m, "incremental", b, s, extra)
        _assert_same(inc, full, (sampler, logprobs, guided, given, B))
        assert (full[1] is None) == (given == "free")
        if given == "known":
            f = known[:B] >= 0
            assert torch.equal(full[1], f) and torch.equal(full[0][1][f], known[:B][f])
    finally:
        _reset(m)


@pytest.mark.parametrize("mode", ["full", "incremental"])
def test_graph_replay_equals_eager(small, mode):
    """Every feature at once: best of 3, all of set_logprobs, guidance, given tokens; the third graphed call is a replay."""
    m, batch, seeds, known = small
    try:
        _configure(m, "best_of_3", True, True, "known")
        extra = {"known_tokens": known}
        eager = _call(m, mode, batch, seeds, extra)
        m.use_graph = True
        for rep in range(3):
            got = _call(m, mode, batch, seeds, extra)
            _assert_same(got, eager, (mode, rep, m.last_call_mode))
        assert m.last_call_mode == "graph"
    finally:
        _reset(m)


def test_rollout_agrees_across_the_ar_modes(small):
    m, batch, seeds, _ = small
    try:
        _reset(m)
        m.set_sampling(1.0, top_k=50, top_p=0.95)
        outs = {}
        for mode in ("full", "incremental"):
            m.ar_mode = mode
            outs[mode] = m.rollout({**batch, "sample_seed": seeds}, 2, context=2)
        for key in ("tokens", "behaviour_logprobs", "token_logprobs", "given", "video"):
            a, b = outs["full"][key], outs["incremental"][key]
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), key
    finally:
        _reset(m)
