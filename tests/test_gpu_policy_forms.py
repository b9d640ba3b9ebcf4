"""GPU: the table ops.policy_loss / ops.policy_loss_bwd dispatch on -- a reference or not, a mask or not, a group or not -- walked once.
Per combination: what the dispatch promises (the keys returned, the summary's length, which extra results exist) and that the backward call
of the same form accepts what the forward call left.  Across combinations, the equalities the forms owe each other, byte for byte:
  an all-False `given`   the unmasked row_loss / logprob / entropy / cut (/ kl) and the unmasked means in summary[:5] or summary[:7];
  ratio_div = 1          the token form's row_loss and dlogits (a group of one row: m_g = logprob - b exactly);
  kl_coef = 0            with a reference, the plain form's row_loss and dlogits (a zero term is not added at all).
24 rows x K = 260 at row stride 264 (two chunks of 256 with a ragged tail, six workgroups), top_k 5, temperature 0.7, the clipped rule.
Tokens: most from the row's top 5, every fifth row's from outside it (an outside row).  What the kernels compute is pinned against fp64 in
test_gpu_policy_loss.py, test_gpu_policy_kl.py, test_gpu_masked_loss.py and test_gpu_group_ratio_kernels.py; nothing here has a tolerance."""
import itertools

import numpy as np
import pytest
import torch

from mage_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, K, LD, TOP_K, TEMP = 24, 260, 264, 5, 0.7
BASE = {"row_loss", "logprob", "entropy", "cut", "summary"}
SCALARS = dict(temperature=TEMP, clip_lo=0.2, clip_hi=0.3, entropy_coef=0.01)
_CACHE = {}


def _inputs():
    if not _CACHE:
        g = np.random.default_rng(20)
        z = (2.0 * g.standard_normal((ROWS, LD))).astype(np.float32)
        order = np.argsort(-z[:, :K], axis=1, kind="stable")
        tok = order[np.arange(ROWS), g.integers(0, TOP_K, ROWS)]
        tok[::5] = order[::5, TOP_K + 3]                                      # outside the kept set: logprob -inf
        third = np.zeros(ROWS, bool)
        third[::3] = True
        _CACHE.update(
            logits=torch.from_numpy(z).to(DEV)[:, :K], tokens=torch.from_numpy(tok.astype(np.int64)).to(DEV),
            adv_row=torch.from_numpy((g.uniform(0.5, 2.0, ROWS) * g.choice([-1.0, 1.0], ROWS)).astype(np.float32)).to(DEV),
            adv_group=torch.from_numpy((g.uniform(0.5, 2.0, ROWS // 4) * g.choice([-1.0, 1.0], ROWS // 4)).astype(np.float32)).to(DEV),
            blp=torch.from_numpy((-1.2 + 0.4 * g.uniform(-1, 1, ROWS)).astype(np.float32)).to(DEV),
            ref=torch.from_numpy((-1.0 + 0.3 * g.uniform(-1, 1, ROWS)).astype(np.float32)).to(DEV),
            third=torch.from_numpy(third).to(DEV), free=torch.zeros(ROWS, dtype=torch.bool, device=DEV),
            gout=torch.tensor([0.7], device=DEV))
    return _CACHE


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _run(ref=False, given=None, ratio_div=None, kl_coef=0.1, adv="adv_row", dt=torch.float32):
    """policy_loss then policy_loss_bwd of one form on the shared inputs; returns (forward dict, dlogits)."""
    c = _inputs()
    kw = dict(SCALARS)
    if ref:
        kw.update(reference_logprob=c["ref"], kl_coef=kl_coef)
    if given is not None:
        kw.update(given=c[given])
    if ratio_div is not None:
        kw.update(ratio_div=ratio_div)
    out = ops.policy_loss(c["logits"], c["tokens"], c[adv], c["blp"], top_k=TOP_K, top_p=1.0, **kw)
    saved = {k: out[k] for k in ("norm", "group_logratio") if k in out}
    dl = ops.policy_loss_bwd(c["logits"], c["tokens"], c[adv], c["blp"], out["cut"], c["gout"], torch.empty(ROWS, K, device=DEV, dtype=dt),
                             **kw, **saved)
    ops.check_device_errors(DEV)
    return out, dl


@pytest.mark.parametrize("ref,masked,grouped", list(itertools.product((False, True), repeat=3)))
def test_what_the_dispatch_promises(ref, masked, grouped):
    out, dl = _run(ref=ref, given="third" if masked else None, ratio_div=4 if grouped else None, adv="adv_group" if grouped else "adv_row",
                   dt=torch.bfloat16)
    want = set(BASE)
    if ref:
        want.add("kl")
    if masked or grouped:
        want.add("norm")
    if grouped:
        want |= {"group_logratio", "group_count"}
    assert set(out) == want
    assert out["summary"].numel() == (8 if masked or grouped else 7 if ref else 5)
    for k in ("row_loss", "logprob", "entropy", "cut") + (("kl",) if ref else ()):
        assert out[k].numel() == ROWS, k
    if masked or grouped:
        assert out["norm"].numel() == 1
        n_free = ROWS - (ROWS + 2) // 3 if masked else ROWS
        assert out["norm"].item() == np.float32(1.0) / np.float32(n_free)
        assert out["summary"][7].item() == (np.float32((ROWS - n_free) / ROWS))
    if grouped:
        assert out["group_logratio"].numel() == ROWS // 4 and out["group_count"].numel() == ROWS // 4
        assert out["group_count"].dtype == torch.int32
    if masked:                                                                  # a given row: zeros forward and backward
        g = _inputs()["third"]
        for k in ("row_loss", "logprob", "entropy", "cut") + (("kl",) if ref else ()):
            assert not _bits(out[k])[g].any(), k
        assert not _bits(dl)[g].any()
    assert dl.shape == (ROWS, K) and dl.dtype == torch.bfloat16 and torch.isfinite(dl.float()).all()


@pytest.mark.parametrize("ref", (False, True))
def test_an_all_false_mask_is_the_unmasked_call(ref):
    plain, dl_plain = _run(ref=ref)
    masked, dl_masked = _run(ref=ref, given="free")
    for k in ("row_loss", "logprob", "entropy", "cut") + (("kl",) if ref else ()):
        _same(masked[k], plain[k], k)
    n = 7 if ref else 5
    _same(masked["summary"][:n], plain["summary"], "summary")
    assert not _bits(masked["summary"][n:]).any()                              # (no reference: sums 5 and 6 stay 0) and nothing given
    _same(dl_masked, dl_plain, "dlogits")
    grouped, dl_grouped = _run(ref=ref, ratio_div=4, adv="adv_group")           # the grouped form takes a mask or none: the same again
    both, dl_both = _run(ref=ref, given="free", ratio_div=4, adv="adv_group")
    assert set(grouped) == set(both)
    for k in grouped:
        _same(both[k], grouped[k], k)
    _same(dl_both, dl_grouped, "dlogits")


@pytest.mark.parametrize("ref,given", list(itertools.product((False, True), (None, "third"))))
@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16))
def test_a_group_of_one_row_is_the_token_form(ref, given, dt):
    token, dl_token = _run(ref=ref, given=given, dt=dt)
    group, dl_group = _run(ref=ref, given=given, ratio_div=1, dt=dt)
    for k in ("row_loss", "logprob", "entropy", "cut") + (("kl",) if ref else ()):
        _same(group[k], token[k], k)
    _same(dl_group, dl_token, "dlogits")


@pytest.mark.parametrize("given,ratio_div", list(itertools.product((None, "third"), (None, 4))))
def test_a_zero_kl_coef_is_the_plain_form(given, ratio_div):
    adv = "adv_row" if ratio_div is None else "adv_group"
    plain, dl_plain = _run(given=given, ratio_div=ratio_div, adv=adv)
    anchored, dl_anchored = _run(ref=True, kl_coef=0.0, given=given, ratio_div=ratio_div, adv=adv)
    assert set(anchored) == set(plain) | {"kl"}
    for k in ("row_loss", "logprob", "entropy", "cut"):
        _same(anchored[k], plain[k], k)
    _same(dl_anchored, dl_plain, "dlogits")
