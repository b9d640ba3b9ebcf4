"""GPU: MAGE.policy_loss(ratio='token' | 'frame' | 'clip') on tests/test_gpu_policy_train.py's small synthetic model (L = 5, 3 clips).

  'token' against the bare call: the same loss bits, the same gradients, the same ordered list of C-ABI calls.
  on-policy data (eval mode, behaviour = last_token_policy_logprobs of the drawing call, the same precision): see
    test_on_policy_frame_and_clip_ratios for what reproduces on this model and what is checked.
  off-policy data (behaviour shifted per frame by constants): loss, info and last_policy_group_logratio against a direct
    ops.policy_loss(..., ratio_div=) call -- bit for bit on the logits distill_targets returns (the pass policy_loss itself runs), and within
    a derived tolerance on the logits of teacher_forced_logits (the inference pass: both passes are held to 1e-4 in the logits against the
    oracle, so a log-probability moves by at most 2 x (logit + log-sum-exp) = 4e-4, tests/test_gpu_policy_train.py's argument and its 1e-3;
    a group's mean log-ratio moves by no more, and d loss / d m_g = -A rho_g: |loss diff| <= max|A| max rho_g 1e-3, plus entropy_coef times
    the entropy's own move, below 2e-4 (log K + 1) < 1e-3; run without a filter, whose kept-set boundary the two passes may decide apart).
    The shifts keep every rho_g at least 5 % away from both clip edges, so no branch flips between the passes and the clipped share is
    equal exactly.
  the README line after rollout(credit='frame', context=2, reference=ref), a FlatAdam step, and the refusals."""
import copy

import numpy as np
import pytest
import torch

from mage_amd import ops
from mage_amd.optim import FlatAdam
from mage_amd.utils import synth
from tests.helpers import build_mage, count_lib_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, TEMP = 5, 3, 0.9
SMALL = dict(width=64, layers=3, vq_dim=32, K=64)
SHIFTS = (0.30, -0.35, 0.05, -0.10)                   # per frame: rho_g = 0.74, 1.42, 0.95, 1.11 against the clip range [0.8, 1.2]


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def small():
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 41, DEV)
    return m, dev_batch(synth.synth_batch_mnist(B, L, seed=41, text_len=9, ragged_text=True))


def _reset(m):
    m.set_sampling(None).set_logprobs(False).set_precision("fp32").set_context(1)
    m.eval()
    m.zero_grad(set_to_none=True)


def _sample(m, batch, seeds):
    m.set_sampling(TEMP).set_logprobs(True, policy=True)
    m.autoregressive_generate({**batch, "sample_seed": torch.tensor(seeds, dtype=torch.int64, device=DEV)})
    tokens, blp = m.last_tokens.clone(), m.last_token_policy_logprobs.clone()
    m.set_logprobs(False)
    return tokens, blp


def _loss_and_grads(m, *a, **kw):
    m.zero_grad(set_to_none=True)
    loss, info = m.policy_loss(*a, **kw)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return loss.detach().clone(), info, grads


def _same_grads(g0, g1):
    return g0.keys() == g1.keys() and len(g0) >= 90 and all(torch.equal(_bits(g0[n]), _bits(g1[n])) for n in g0)


def test_ratio_token_is_the_bare_call(small, monkeypatch):
    m, batch = small
    _reset(m)
    tokens, blp = _sample(m, batch, [5, 6, 7])
    adv = torch.tensor([1.0, -0.5, 0.25], device=DEV)
    b = (blp + 0.3).contiguous()                                     # (some tokens clip)
    try:
        calls = count_lib_calls(monkeypatch)
        l0, i0, g0 = _loss_and_grads(m, batch, tokens, adv, b, entropy_coef=0.01)
        bare = list(calls)
        del calls[:]
        l1, i1, g1 = _loss_and_grads(m, batch, tokens, adv, b, entropy_coef=0.01, ratio="token")
        token = list(calls)
        monkeypatch.undo()
        assert bare == token and "mage_policy_loss" in bare and not [c for c in bare if "grouped" in c]
        assert torch.equal(_bits(l0), _bits(l1)) and i0 == i1 and _same_grads(g0, g1) and i0["clip_fraction"] > 0
        assert m.last_policy_group_logratio is None
    finally:
        _reset(m)


def test_on_policy_frame_and_clip_ratios(small):
    """behaviour = last_token_policy_logprobs of the drawing call.  Where the teacher-forced pass reproduces those bit for bit, rho = 1
    everywhere and 'frame' / 'clip' must give 'token''s loss and parameter gradients bit for bit.  Where it does not (the generation runs the
    incremental decoder; tests/test_gpu_policy_train.py holds the two passes to 1e-3 in the log-probabilities), every group's log-ratio must
    be within that 1e-3 of 0 with nothing clipped, and loss and log-ratios must carry the bits of the direct kernel call on the pass's own
    logits (distill_targets).  On this model it does not: the two differ by 2.4e-6 at most, so the second set of checks is the one that runs.
    Either way, b taken from the teacher-forced pass itself is on-policy exactly: 'frame' and 'clip' then give
    'token''s bits."""
    m, batch = small
    _reset(m)
    tokens, blp = _sample(m, batch, [8, 9, 10])
    adv = torch.tensor([1.0, -0.5, 0.25], device=DEV)
    hw = m.image_resolution ** 2
    try:
        lt, it, gt = _loss_and_grads(m, batch, tokens, adv, blp, entropy_coef=0.01)
        own = m.last_policy_token_logprobs.clone()
        reproduces = torch.equal(_bits(own), _bits(blp))
        print(f"the teacher-forced pass reproduces the generation's log-probabilities bit for bit: {reproduces} "
              f"(max |diff| {(own - blp).abs().max().item():.3e})")
        assert (own - blp).abs().max().item() < 1e-3
        lg = m.distill_targets(batch, tokens)
        for ratio, shape, rd in (("frame", (B, L - 1), hw), ("clip", (B,), (L - 1) * hw)):
            lgr, ig, gg = _loss_and_grads(m, batch, tokens, adv, blp, entropy_coef=0.01, ratio=ratio)
            glr = m.last_policy_group_logratio
            assert glr.shape == shape and glr.dtype == torch.float32 and set(ig) == set(it)
            if reproduces:
                assert (_bits(glr) == 0).all() and torch.equal(_bits(lt), _bits(lgr)) and ig == it and _same_grads(gt, gg), ratio
            else:
                d = ops.policy_loss(lg, tokens.reshape(-1), adv, blp.reshape(-1), temperature=TEMP, entropy_coef=0.01, ratio_div=rd)
                assert torch.equal(_bits(lgr), _bits(d["summary"][0])) and torch.equal(_bits(glr.reshape(-1)), _bits(d["group_logratio"]))
                assert glr.abs().max().item() < 1e-3 and ig["clip_fraction"] == 0.0 and ig["outside_fraction"] == 0.0
                assert abs(ig["approx_kl"]) < 1e-3 and len(gg) >= 90
        # b = the teacher-forced pass's own values: rho = 1 exactly under every ratio
        lt, it, gt = _loss_and_grads(m, batch, tokens, adv, own, entropy_coef=0.01)
        for ratio in ("frame", "clip"):
            lgr, ig, gg = _loss_and_grads(m, batch, tokens, adv, own, entropy_coef=0.01, ratio=ratio)
            assert (_bits(m.last_policy_group_logratio) == 0).all()
            assert torch.equal(_bits(lt), _bits(lgr)) and ig == it and _same_grads(gt, gg), ratio
    finally:
        _reset(m)


@pytest.mark.parametrize("ratio", ["frame", "clip"])
@pytest.mark.parametrize("way", ["plain", "anchored_given"])
def test_off_policy_against_the_direct_kernel_call(small, ratio, way):
    m, batch = small
    _reset(m)
    R_, K = m.image_resolution, m.codebook_size
    hw = R_ * R_
    try:
        top_k = 24 if way == "anchored_given" else 0                 # the filter: on the bit-for-bit route only (below)
        m.set_sampling(TEMP, top_k=top_k)
        tok, lg_tf = m.teacher_forced_logits(batch)
        tokens = tok[:, 1:].reshape(B, L - 1, R_, R_).contiguous()
        lg = m.distill_targets(batch, tokens)
        assert lg.shape == (B * (L - 1) * hw, K) and (lg - lg_tf.reshape(-1, K).float()).abs().max().item() < 1e-3
        own = m.token_policy_logprobs(batch, tokens)
        shifts = (torch.tensor(SHIFTS, device=DEV)[None, :, None, None] if ratio == "frame"
                  else torch.tensor([0.30, -0.35, 0.05], device=DEV)[:, None, None, None])
        b = (torch.where(torch.isfinite(own), own, torch.zeros_like(own)) + shifts).contiguous()
        adv = torch.tensor([-1.0, 0.5, 0.75], device=DEV)             # (clip 0: rho 0.74 with A < 0, clip 1: rho 1.42 with A > 0 -- both switched off)
        if ratio == "frame":
            adv = (adv[:, None] * torch.tensor([1.0, 1.0, -1.0, 0.5], device=DEV)[None]).contiguous()
        kw, dkw = {}, {}
        if way == "anchored_given":
            given = torch.zeros(B, L - 1, R_, R_, dtype=torch.bool, device=DEV)
            given[:, 0] = True                                       # frame 1 given: a context of 2
            given[1, 2, ::2] = True
            ref = (own - 0.05).contiguous()
            kw = dict(reference_logprobs=ref, kl_coef=0.1, given=given)
            dkw = dict(reference_logprob=ref.reshape(-1), kl_coef=0.1, given=given.reshape(-1))
        rd = hw if ratio == "frame" else (L - 1) * hw
        loss, info, grads = _loss_and_grads(m, batch, tokens, adv, b, entropy_coef=0.01, ratio=ratio, **kw)
        glr = m.last_policy_group_logratio.clone()
        args = (tokens.reshape(-1), adv.reshape(-1), b.reshape(-1))
        common = dict(temperature=TEMP, top_k=top_k, top_p=1.0, clip_lo=0.2, clip_hi=0.2, entropy_coef=0.01, ratio_div=rd, **dkw)
        d = ops.policy_loss(lg, *args, **common)
        ops.check_device_errors(DEV)
        s = d["summary"].tolist()
        assert torch.equal(_bits(loss), _bits(d["summary"][0])) and torch.equal(_bits(glr.reshape(-1)), _bits(d["group_logratio"]))
        names = ("loss", "entropy", "approx_kl", "clip_fraction", "outside_fraction") + (("kl", "unanchored_fraction") if kw else ())
        assert info == dict(zip(names, s), **({"given_fraction": s[7]} if kw else {}))
        assert 0 < info["clip_fraction"] < 1 and any(bool(g.abs().max() > 0) for g in grads.values()) and len(grads) >= 90
        assert glr.shape == ((B, L - 1) if ratio == "frame" else (B,))
        cnt = d["group_count"].view(glr.shape)
        if kw and ratio == "frame":
            assert (cnt[:, 0] == 0).all() and (_bits(glr)[:, 0] == 0).all()          # a given frame: nothing to count, log-ratio +0
        if top_k:                                                    # (a kept-set boundary is decided by logits that differ between the passes)
            return
        # the inference pass's logits: the derived tolerance of the module docstring
        t = ops.policy_loss(lg_tf.reshape(-1, K).float().contiguous(), *args, **common)
        ts = t["summary"].tolist()
        rho_max = d["group_logratio"].exp().max().item()
        assert (t["group_logratio"] - d["group_logratio"]).abs().max().item() <= 1e-3
        assert abs(ts[0] - s[0]) <= adv.abs().max().item() * rho_max * 1e-3 + 0.01 * 1e-3       # (+ entropy_coef x |dH|, |dH| <= 1e-3)
        assert ts[3] == s[3] and ts[4] == s[4] and ts[7] == s[7] and torch.equal(t["group_count"], d["group_count"])
    finally:
        _reset(m)


def test_the_documented_line_runs_as_written(small):
    _, batch0 = small
    m = build_mage(synth.mnist_model_config(frames_length=L, **SMALL), 43, DEV)                    # (its own model: the step changes the weights)
    batch = {**batch0, "sample_seed": torch.tensor([11, 12, 13], dtype=torch.int64, device=DEV)}
    _reset(m)
    ref = copy.deepcopy(m).eval()
    m.set_sampling(TEMP)
    try:
        opt = FlatAdam(m.parameters(), lr=1e-4)
        out = m.rollout(batch, 8, credit='frame', context=2, reference=ref)
        loss, info = m.policy_loss(out['batch'], out['tokens'], out['advantages'], out['behaviour_logprobs'],
                                   reference_logprobs=out['reference_logprobs'], kl_coef=0.1, given=out['given'], ratio='frame')
        assert np.isfinite(loss.item()) and np.isfinite(info["loss"]) and info["given_fraction"] == 0.25
        glr = m.last_policy_group_logratio
        assert glr.shape == (B * 8, L - 1) and (_bits(glr)[:, 0] == 0).all() and glr.abs().max().item() < 1e-3
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert sum(p.grad is not None for p in m.parameters()) >= 90
        assert all(torch.isfinite(p).all() for p in m.parameters())
    finally:
        _reset(m)


def test_refusals_launch_nothing(small, monkeypatch):
    m, batch = small
    _reset(m)
    R_ = m.image_resolution
    tokens = torch.zeros(B, L - 1, R_, R_, dtype=torch.int64, device=DEV)
    blp = torch.zeros(B, L - 1, R_, R_, device=DEV)
    a_clip, a_frame, a_tok = torch.ones(B, device=DEV), torch.ones(B, L - 1, device=DEV), torch.ones(B, L - 1, R_, R_, device=DEV)
    calls = count_lib_calls(monkeypatch)
    before = m.last_policy_group_logratio

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            m.policy_loss(batch, tokens, *a, **kw)
        assert calls == []
    for bad in ("sequence", "Frame", None, 1):
        refused("ratio must be", a_clip, blp, ratio=bad)
    for ratio in ("frame", "clip"):
        refused("needs behaviour_logprobs", a_clip, ratio=ratio)
        refused("not finer than the group", a_tok, blp, ratio=ratio)
    refused("not finer than the group", a_frame, blp, ratio="clip")
    refused("GPU", a_frame, blp.cpu(), ratio="frame")
    monkeypatch.undo()
    assert m.last_policy_group_logratio is before                    # a refused call leaves the last result alone
    _reset(m)
