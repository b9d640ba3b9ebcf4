"""CPU: the preference loss -- the fp64 restatement (tests/preference_ref.py) against torch.autograd of -F.logsigmoid and of the IPO square, the
two extension entry points in the header and the binding table, their argument checks (refused before anything is launched, through fake
aligned pointers) and the validation of MAGE.preference_loss, MAGE.clip_logprobs and MAGE.rollout(pairs=) on a CPU model."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mage_amd import _lib, ops
from mage_amd.utils import synth
from tests import preference_ref as P
from tests.helpers import build_mage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


def _case(clips, n_pairs, seed):
    g = np.random.default_rng(seed)
    s = (-40 + 3 * g.standard_normal(clips)).astype(np.float32)
    r = (s + g.standard_normal(clips)).astype(np.float32)
    return s, r, g.integers(0, clips, (n_pairs, 2))


@pytest.mark.parametrize("beta", [0.05, 1.0])
@pytest.mark.parametrize("eps,mode", [(0.0, 0), (0.1, 0), (0.0, 1)])
def test_restatement_is_autograd_of_the_textbook_loss(beta, eps, mode):
    s, r, pairs = _case(12, 40, seed=int(beta * 100) + mode)
    pairs[3] = (5, 5)                                                           # no preference: no gradient
    pairs = np.concatenate([pairs, P.six_nine()])
    ref = P.pair_stage(s, r, pairs, beta, eps, mode)
    st = torch.tensor(s.astype(np.float64), requires_grad=True)
    rt = torch.tensor(r.astype(np.float64))
    w, lo = torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])
    u = (st[w] - rt[w]) - (st[lo] - rt[lo])
    bt, e = P.f32(beta), P.f32(eps)
    if mode == 0:
        per = -(1 - e) * F.logsigmoid(bt * u) - e * F.logsigmoid(-bt * u)
    else:
        per = (u - 1 / (2 * bt)) ** 2
    per.mean().backward()
    assert np.abs(ref["pair_loss"] - per.detach().numpy()).max() < 1e-12
    assert np.abs(ref["clip_coef"] - st.grad.numpy()).max() < 1e-12
    assert np.abs(ref["pair_margin"] - (bt * u).detach().numpy()).max() == 0
    assert abs(ref["summary"][0] - per.mean().item()) < 1e-12 and abs(ref["summary"][1] - (u > 0).double().mean().item()) == 0
    assert abs(ref["summary"][4] - (ref["summary"][2] - ref["summary"][3])) < 1e-12
    assert ref["u"][3] == 0.0 and ref["n_c"].max() <= 32


def test_restatement_edges():
    ref = P.pair_stage(np.float32([-3, -3, 7]), np.float32([1, 1, 0]), [[0, 1], [1, 1]], 0.1)
    assert (ref["pair_loss"] == np.log(2.0)).all() and (ref["pair_margin"] == 0).all()
    assert np.float32(ref["pair_loss"][0]) == np.float32(np.log(2.0))
    q = P.f32(0.1) / 4                                                          # beta sig(0) / P, beta the fp32 value
    assert ref["clip_coef"].tolist() == [-q, q, 0.0] and not np.signbit(ref["clip_coef"][2])               # in no pair: +0
    for beta in (0.05, 1.0):
        s, r, pairs = P.margin_case(beta)
        for eps in (0.0, 0.1):
            out = P.pair_stage(s, r, pairs, beta, eps)
            assert np.isfinite(out["pair_loss"]).all() and np.isfinite(out["clip_coef"]).all()
            assert np.abs(out["pair_margin"] - [0, 1e-3, -1e-3, 1, -1, 20, -20, 100, -100]).max() < 1e-4
            assert (out["pair_loss"] >= 0).all() and out["pair_loss"][8] > 99 * (1 - eps)


def test_token_logprob_bwd_restatement_is_autograd_of_the_weighted_sum():
    for rows, K in ((5, 64), (7, 68)):
        z, tg, w, wrow = P.lpb_inputs(rows, K, 2)
        c = (np.float32(P.LPB_GRAD_OUT) * wrow.numpy()).astype(np.float64)
        out, b = P.token_logprob_bwd(z.double(), tg, torch.from_numpy(c))
        zt = torch.nan_to_num(z.double(), nan=0.0).masked_fill(torch.isinf(z), -1e300).requires_grad_()
        ok = (tg >= 0) & (tg < K)
        lp = torch.log_softmax(zt, -1)
        lse = -torch.logsumexp(zt, -1)                                          # a token outside [0, K): no one-hot, only the normaliser
        picked = torch.where(ok, lp.gather(1, tg.clamp(0, K - 1)[:, None])[:, 0], lse)
        (torch.from_numpy(c) * picked).sum().backward()
        assert (out - zt.grad).abs().max().item() < 1e-12
        assert (out[wrow == 0] == 0).all() and (b[wrow == 0] == 0).all() and (b[wrow != 0] > 0).all()
        if rows > 2:
            assert (out[2, 1::3] == 0).all()


def test_header_and_table_name_the_two_entry_points():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", header, flags=re.M))
    assert {"mage_preference_loss", "mage_token_logprob_bwd"} <= declared and declared == set(_lib.EXT_SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    for name, n_args in (("mage_preference_loss", 13), ("mage_token_logprob_bwd", 11)):
        res, args = _lib.EXT_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and len(args) == n_args
        n_decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1).count(",") + 1
        assert n_decl == len(args)
    assert {"preference_loss", "token_logprob_bwd"} <= set(ops.__all__)


PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched
PREF_ORDER = ("clip_logprob", "reference_logprob", "clips", "pairs", "n_pairs", "beta", "label_smoothing", "mode", "pair_loss", "pair_margin",
              "clip_coef", "summary")
PREF_GOOD = dict(clip_logprob=PTR, reference_logprob=PTR, clips=8, pairs=PTR, n_pairs=3, beta=0.1, label_smoothing=0.0, mode=0, pair_loss=PTR,
                 pair_margin=PTR, clip_coef=PTR, summary=PTR)
LPB_ORDER = ("logits", "rows", "K", "ld", "tokens", "weight", "weight_div", "grad_out", "dlogits", "dl_dtype")
LPB_GOOD = dict(logits=PTR, rows=8, K=512, ld=512, tokens=PTR, weight=PTR, weight_div=4, grad_out=PTR, dlogits=PTR, dl_dtype=_lib.BF16)


@pytest.mark.parametrize("bad", [
    dict(clip_logprob=None), dict(reference_logprob=None), dict(pairs=None), dict(pair_loss=None), dict(pair_margin=None), dict(clip_coef=None),
    dict(summary=None), dict(clip_logprob=PTR + 2), dict(reference_logprob=PTR + 1), dict(pairs=PTR + 4), dict(pair_loss=PTR + 2),
    dict(pair_margin=PTR + 2), dict(clip_coef=PTR + 3), dict(summary=PTR + 2),
    dict(clips=0), dict(clips=-1), dict(clips=65537), dict(n_pairs=0), dict(n_pairs=-4), dict(n_pairs=65537),
    dict(beta=0.0), dict(beta=-0.1), dict(beta=INF), dict(beta=NAN), dict(beta=1e-46),
    dict(label_smoothing=-0.1), dict(label_smoothing=0.5), dict(label_smoothing=NAN), dict(label_smoothing=0.1, mode=1),
    dict(mode=2), dict(mode=-1)])
def test_preference_loss_refuses_bad_arguments(bad):
    a = {**PREF_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_preference_loss(*[a[k] for k in PREF_ORDER], None)
    msg = lib.mage_last_error().decode()
    assert rc == -1 and "mage_preference_loss" in msg and "mage_init" not in msg, (bad, rc, msg)


def test_preference_loss_accepts_what_the_rule_allows():
    """The accepted forms get past the argument rules: without an initialised device the call stops at the mage_init check behind them."""
    lib = _lib.load()
    for ok in (dict(), dict(clips=1, n_pairs=1), dict(clips=65536, n_pairs=65536), dict(label_smoothing=0.49), dict(mode=1), dict(beta=100.0), dict(beta=1e-45),
               dict(clip_logprob=PTR + 4, pairs=PTR + 8)):
        a = {**PREF_GOOD, **ok}
        rc = lib.mage_preference_loss(*[a[k] for k in PREF_ORDER], None)
        assert rc == -1 and "mage_init" in lib.mage_last_error().decode(), (ok, rc, lib.mage_last_error())


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(tokens=None), dict(weight=None), dict(grad_out=None), dict(dlogits=None),
    dict(K=6, ld=8), dict(K=4100, ld=4100), dict(K=0), dict(rows=0), dict(rows=-1), dict(ld=510), dict(ld=256), dict(weight_div=0),
    dict(weight_div=-1), dict(logits=PTR + 4), dict(dlogits=PTR + 8), dict(tokens=PTR + 4), dict(weight=PTR + 2), dict(grad_out=PTR + 2),
    dict(dl_dtype=_lib.F16), dict(dl_dtype=7)])
def test_token_logprob_bwd_refuses_bad_arguments(bad):
    a = {**LPB_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_token_logprob_bwd(*[a[k] for k in LPB_ORDER], None)
    assert rc == -1 and "mage_token_logprob_bwd" in lib.mage_last_error().decode(), (bad, rc)


def test_cpu_tensors_and_bad_arguments_are_refused():
    s, pairs = torch.zeros(4), torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.preference_loss(s, s, pairs)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.token_logprob_bwd(torch.zeros(8, 16), torch.zeros(8, dtype=torch.int64), torch.ones(8), torch.ones(1), torch.empty(8, 16))
    L, B = 4, 2
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=16), 0)
    batch = synth.synth_batch_mnist(B, L, seed=1)
    R_ = m.image_resolution
    tokens = torch.zeros(B, L - 1, R_, R_, dtype=torch.int64)
    pairs, ref = torch.tensor([[0, 1]]), torch.zeros(B)

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            m.preference_loss(*a, **kw)
    refused("GPU", batch, tokens, pairs, ref)
    refused("tokens", batch, tokens[:, 1:], pairs, ref)
    refused("tokens", batch, tokens.int(), pairs, ref)
    refused("pairs", batch, tokens, pairs.int(), ref)
    refused("pairs", batch, tokens, pairs.view(2), ref)
    refused("pairs", batch, tokens, pairs[:0], ref)
    refused("pairs", batch, tokens, torch.zeros(1, 3, dtype=torch.int64), ref)
    refused("reference_logprobs", batch, tokens, pairs, ref.double())
    refused("reference_logprobs", batch, tokens, pairs, torch.zeros(B + 1))
    refused("reference_logprobs", batch, tokens, pairs, None)
    for beta in (0.0, -1.0, INF, NAN, "0.1", True):
        refused("beta", batch, tokens, pairs, ref, beta=beta)
    for eps in (-0.1, 0.5, NAN, "0"):
        refused("label_smoothing", batch, tokens, pairs, ref, label_smoothing=eps)
    refused("label_smoothing", batch, tokens, pairs, ref, label_smoothing=0.1, loss="ipo")
    refused("loss", batch, tokens, pairs, ref, loss="hinge")
    refused("images", {**batch, "images": batch["images"][0]}, tokens, pairs, ref)
    m.use_cids = False
    refused("use_cids=False", batch, tokens, pairs, ref)
    m.use_cids = True
    m.set_guidance(2.0)
    refused("guidance", batch, tokens, pairs, ref)
    m.set_guidance(None)
    m.set_precision("f16")
    refused("f16", batch, tokens, pairs, ref)
    m.set_precision("fp32")
    m.randomness = True
    refused("randomness=True", batch, tokens, pairs, ref)
    with pytest.raises(ValueError, match="clip_logprobs: randomness=True"):
        m.clip_logprobs(batch, tokens)
    m.randomness = False
    with pytest.raises(ValueError, match="clip_logprobs: .*GPU"):
        m.clip_logprobs(batch, tokens)
    with pytest.raises(ValueError, match="clip_logprobs: tokens"):
        m.clip_logprobs(batch, tokens[:1])
    with pytest.raises(ValueError, match="clip_logprobs: batch"):
        m.clip_logprobs(None, tokens)
    assert m.last_preference_clip_logprobs is None and m.last_preference_clip_coef is None and m.last_preference_pair_loss is None
    assert m.last_preference_pair_margin is None and m.last_preference_token_logprobs is None
    m.set_sampling(0.9)
    with pytest.raises(ValueError, match="rollout: pairs"):
        m.rollout(batch, 2, pairs="best")
    with pytest.raises(ValueError, match="rollout: pairs"):
        m.rollout(batch, 2, pairs=True)
    m.set_sampling(None)
