"""GPU: the two kernels behind MAGE.preference_loss (mage_amd/csrc/preference.hip) against the fp64 restatements of tests/preference_ref.py
(formulas and the derivation of every bound are in that module's docstring).

  pref_pair_kernel + pref_coef_kernel     test_pair_stage[case-form-beta]: (clips 2, pairs 1); (clips 6, pairs 9) with a clip chosen three
                                          times, one on both sides, one in no pair, a pair (2, 2), no order; margins 0, +-1e-3, +-1, +-20,
                                          +-100; (clips 300, pairs 1000): two workgroups of clips, four of pairs, a ragged last tile
  token_logprob_bwd_kernel<NV, float |    test_token_logprob_bwd[shape-kind-div]: NV 4 (K 4, 64, 68), 8 (512), 16 (1000), 64 (4096); bf16 with
    bf16>                                 16-byte stores (K % 8 == 0) and with 8-byte ones (K 4, 68); a ragged last workgroup; ld = K + 4

Every case: each output starts filled with the NaN sentinel of its dtype with elements past its end; everything outside the written region
must still hold the sentinel, everything inside must have been written and lie within its bound.  Refused calls return MAGE_EINVAL and leave
the outputs untouched."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import preference_ref as R
from tests.helpers import DEV, bits, lib, refused, sent, untouched, within, written

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {"f32": ops.F32, "bf16": ops.BF16}
FORMS = {"dpo": (0.0, 0), "dpo_smooth": (0.1, 0), "ipo": (0.0, 1)}
PAD = 5


def _random_case(clips, n_pairs, seed):
    g = np.random.default_rng(seed)
    s = (-40 + 3 * g.standard_normal(clips)).astype(np.float32)
    r = (s + g.standard_normal(clips)).astype(np.float32)
    return s, r, g.integers(0, clips, (n_pairs, 2))


def _pair_case(name, beta):
    if name == "two_one":
        return np.float32([-31.5, -30.25]), np.float32([-31.0, -30.5]), np.array([[1, 0]])
    if name == "six_nine":
        s, r, _ = _random_case(6, 1, 3)
        return s, r, R.six_nine()
    if name == "margins":
        return R.margin_case(beta)
    return _random_case(300, 1000, 7)


def _launch(s, r, pairs, beta, eps, mode):
    l, st = lib()
    P, clips = len(pairs), len(s)
    sd, rd, pd = torch.from_numpy(s).to(DEV), torch.from_numpy(r).to(DEV), torch.from_numpy(np.ascontiguousarray(pairs, np.int64)).to(DEV)
    out = dict(pair_loss=sent(P + PAD, torch.float32), pair_margin=sent(P + PAD, torch.float32), clip_coef=sent(clips + PAD, torch.float32),
               summary=sent(5 + PAD, torch.float32))
    _lib.check(l.mage_preference_loss(sd.data_ptr(), rd.data_ptr(), clips, pd.data_ptr(), P, beta, eps, mode, out["pair_loss"].data_ptr(),
                                      out["pair_margin"].data_ptr(), out["clip_coef"].data_ptr(), out["summary"].data_ptr(), st), l)
    torch.cuda.synchronize()
    ops.check_device_errors(DEV)
    return out, dict(pair_loss=P, pair_margin=P, clip_coef=clips, summary=5)


@pytest.mark.parametrize("beta", [0.05, 1.0])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", ["two_one", "six_nine", "margins", "random"])
def test_pair_stage(case, form, beta):
    eps, mode = FORMS[form]
    s, r, pairs = _pair_case(case, beta)
    out, n = _launch(s, r, pairs, beta, eps, mode)
    ref = R.pair_stage(s, r, pairs, beta, eps, mode)
    assert ref["n_c"].max() <= 32
    for k in n:
        assert untouched(out[k][n[k]:]) and written(out[k][:n[k]]), f"{k}: footprint"
        within("mage_preference_loss", f"{case} {form} beta={beta} {k}", out[k][:n[k]], torch.from_numpy(ref[k]), torch.from_numpy(ref[k + "_bound"]))
    again, _ = _launch(s, r, pairs, beta, eps, mode)
    assert all(torch.equal(bits(out[k]), bits(again[k])) for k in n), "two launches differ"
    coef = out["clip_coef"][:n["clip_coef"]].cpu()
    idle = torch.from_numpy(ref["n_c"] == 0)
    assert (bits(coef)[idle] == 0).all(), "a clip in no pair must get +0"
    if case == "six_nine":
        assert idle.tolist() == [False] * 5 + [True] and bits(out["pair_margin"])[2].item() == 0                 # the pair (2, 2): u = 0 exactly
    if case == "margins":
        assert bits(out["pair_margin"])[0].item() == 0
        if form == "dpo":
            assert out["pair_loss"][0].item() == float(np.float32(np.log(2.0))), "u = 0: log 2"
        assert bool(torch.isfinite(out["pair_loss"][:len(pairs)]).all()) and bool(torch.isfinite(coef).all()), "saturation must stay finite"


def test_pair_stage_reports_an_index_out_of_range():
    s, r, _ = _random_case(6, 1, 3)
    with pytest.raises(ValueError, match="pair index out of range.*value 6"):
        _launch(s, r, np.array([[0, 1], [6, 2]]), 0.1, 0.0, 0)
    out, n = _launch(s, r, np.array([[0, 1], [5, 2]]), 0.1, 0.0, 0)             # what the index was clamped to; and the flag is clear again
    assert written(out["pair_loss"][:2])


def test_pair_stage_refusals():
    l, st = lib()
    x = torch.zeros(8, device=DEV)
    pairs = torch.zeros(4, 2, dtype=torch.int64, device=DEV)
    outs = [sent(8, torch.float32) for _ in range(4)]

    def call(**kw):
        a = dict(s=x.data_ptr(), r=x.data_ptr(), clips=8, pairs=pairs.data_ptr(), P=4, beta=0.1, eps=0.0, mode=0, o0=outs[0].data_ptr())
        a.update(kw)
        return lambda: _lib.check(l.mage_preference_loss(a["s"], a["r"], a["clips"], a["pairs"], a["P"], a["beta"], a["eps"], a["mode"], a["o0"],
                                                         outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), st), l)
    for kw in (dict(clips=0), dict(clips=65537), dict(P=0), dict(P=65537), dict(beta=0.0), dict(beta=float("inf")), dict(eps=0.5),
               dict(eps=0.1, mode=1), dict(mode=2), dict(s=None), dict(pairs=pairs.data_ptr() + 4), dict(o0=outs[0].data_ptr() + 2)):
        refused(call(**kw), *outs)


# ------------------------------------------------------------------------------------------------ mage_token_logprob_bwd
def _lpb(rows, K, kind, weight_div, ld=None):
    z, tg, w, wrow = R.lpb_inputs(rows, K, weight_div)
    ld = K if ld is None else ld
    zd = torch.full((rows, ld), 1.0e6, device=DEV)
    zd[:, :K] = z.to(DEV)
    out = sent((rows + 3, K), DT[kind])
    go = torch.tensor([R.LPB_GRAD_OUT], device=DEV)
    got = ops.token_logprob_bwd(zd[:, :K], tg.to(DEV), w.to(DEV), go, out[:rows], weight_div=weight_div)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and untouched(out[rows:]) and written(out[:rows]), f"rows={rows} K={K} {kind}: footprint"
    c = torch.from_numpy((np.float32(R.LPB_GRAD_OUT) * wrow.numpy()).astype(np.float64))
    ref, b = R.token_logprob_bwd(z.double(), tg, c, kind)
    got = out[:rows].cpu()
    within("mage_token_logprob_bwd", f"rows={rows} K={K} {kind} div={weight_div} ld={ld}", got, ref, b)
    assert (bits(got)[wrow == 0] == 0).all(), "a zero-weight row must be +0 everywhere"
    if rows > 2 and K > 3 and wrow[2] != 0:
        assert (got[2, 1::3] == 0).all(), "-inf logits must give exact zeros"
    return wrow


@pytest.mark.parametrize("weight_div", [1, 2])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("rows,K", R.LPB_SHAPES)
def test_token_logprob_bwd(rows, K, kind, weight_div):
    _lpb(rows, K, kind, weight_div)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_token_logprob_bwd_strided_rows(kind):
    wrow = _lpb(7, 68, kind, 1, ld=72)
    assert (wrow == 0).any() and (wrow[2] != 0)
    _lpb(3, 512, kind, 2, ld=516)


def test_token_logprob_bwd_refusals():
    l, st = lib()
    z = torch.randn(4, 68, device=DEV)
    tg = torch.zeros(4, dtype=torch.int64, device=DEV)
    w, go = torch.ones(4, device=DEV), torch.ones(1, device=DEV)
    out = sent((8, 64), torch.float32)

    def call(**kw):
        a = dict(z=z.data_ptr(), rows=4, K=64, ld=68, tg=tg.data_ptr(), w=w.data_ptr(), div=1, go=go.data_ptr(), o=out.data_ptr(), dt=ops.F32)
        a.update(kw)
        return lambda: _lib.check(l.mage_token_logprob_bwd(a["z"], a["rows"], a["K"], a["ld"], a["tg"], a["w"], a["div"], a["go"], a["o"],
                                                           a["dt"], st), l)
    for kw in (dict(rows=0), dict(K=6), dict(K=62), dict(K=4100, ld=4100), dict(ld=60), dict(ld=66), dict(div=0), dict(dt=ops.F16), dict(dt=9),
               dict(z=z.data_ptr() + 4), dict(o=out.data_ptr() + 8), dict(w=None), dict(tg=None), dict(go=None)):
        refused(call(**kw), out)
