"""CPU: the policy-gradient loss -- the fp64 restatement (tests/policy_ref.py) against torch.autograd of its own loss and against
F.cross_entropy, the two extension entry points in the header and the binding table, mage_policy_loss / mage_policy_loss_bwd's argument
checks (refused before anything is launched) and the refusal of CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mage_amd import _lib, ops
from mage_amd.utils import synth
from tests import policy_ref as P
from tests import sampling_ref as S
from tests import token_stats_ref as R
from tests.helpers import build_mage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


def _case(K, n, seed):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((n, K))).astype(np.float32)
    z[::3] = np.round(z[::3] * 4) / 4                               # ties
    z[1, 3:9] = -INF
    return g, z, g.integers(0, K, n)


def _torch_loss(z, tok, A, b, T, sets, cmin, cmax, c, scale):
    """scale * sum_i l_i in torch fp64 with the kept sets as constant masks; returns (loss, d loss / d z).  s takes the restatement's
    fp32-rounded values and the exact derivative inv_t (the rounding itself is a constant offset)."""
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    inv_t = float(S.inv_temperature(T))
    total = torch.zeros((), dtype=torch.float64)
    for r in range(z.shape[0]):
        N = torch.from_numpy(sets[r])
        if not sets[r][tok[r]] or np.isneginf(z[r, tok[r]]):
            continue                                                # an outside row: l = 0, a constant
        s32 = torch.from_numpy(R.scaled(z[r], T).astype(np.float64))
        zr = zt[r].masked_fill(torch.isinf(zt[r]), 0.0)             # (-inf logits: constants, no 0 * inf in the chain rule)
        s = torch.where(torch.isinf(s32), s32, zr * inv_t + (s32 - zr * inv_t).detach())
        logp = torch.log_softmax(s.masked_fill(~N, -INF), 0)
        p = logp.exp()
        H = -(torch.where(p > 0, p * logp.masked_fill(p == 0, 0.0), torch.zeros_like(p))).sum()
        lp = logp[tok[r]]
        if b is None:
            l = -A[r] * lp - c * H
        else:
            rho = (lp - b[r]).exp()
            l = -torch.minimum(rho * A[r], rho.clamp(cmin, cmax) * A[r]) - c * H
        total = total + scale * l
    total.backward()
    return total.item(), zt.grad.numpy()


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.7, 20, 1.0), (1.5, 0, 0.9), (1.3, 20, 0.9)])
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("c", [0.0, 0.05])
def test_analytic_dlogits_is_autograd_of_the_loss(T, k, p, clipped, c):
    K, n = 64, 24
    g, z, tok = _case(K, n, seed=k + int(10 * p) + 100 * clipped)
    idx = np.arange(n)
    A = np.abs(g.standard_normal(n)) * np.where((idx // 2) % 2 == 0, 1.0, -1.0)      # both signs ...
    sets = [R.exact_set(z[r], T, k, p) for r in range(n)]
    for r in range(0, n, 2):                                        # every other row: a token the policy can draw
        tok[r] = int(np.argmax(np.where(sets[r], z[r], -INF)))
    cmin, cmax = P.clip_bounds(0.2, 0.3)
    b = None
    if clipped:
        lp = np.array([R.stats_for_set(z[r], int(tok[r]), T, 0, sets[r])["policy_logprob"] for r in range(n)])
        off = np.where((idx // 4) % 2 == 0, 0.35, -0.35) * g.uniform(0.9, 1.0, n)      # ... on both sides of the clip range [0.8, 1.3]
        off[n // 2:] *= 0.3                                         # and inside it
        b = np.where(np.isfinite(lp), lp, 0.0) + off
    scale = 0.7 / n
    rows = [P.row(z[r], int(tok[r]), A[r], None if b is None else b[r], T, sets[r], cmin, cmax, c) for r in range(n)]
    got = np.stack([P.dlogits_row(z[r], int(tok[r]), A[r], None if b is None else b[r], T, sets[r], cmin, cmax, c, scale) for r in range(n)])
    want_loss, want = _torch_loss(z, tok, A, b, T, sets, cmin, cmax, c, scale)
    assert abs(scale * sum(r["loss"] for r in rows) - want_loss) < 1e-10
    assert np.abs(got - want).max() < 1e-10
    inside = [r for r in rows if not r["outside"]]
    assert len(inside) >= n // 2 and (k == 0 and p == 1.0 or len(inside) < n)
    if clipped:                                                     # both branches of the surrogate, for both signs of A
        assert {(r["off"], a > 0) for r, a in zip(rows, A) if not r["outside"]} == {(False, False), (False, True), (True, False), (True, True)}
        assert all(r["g"] == 0.0 for r in inside if r["off"])
    for r in range(n):
        assert (got[r][~sets[r]] == 0).all() and (sets[r][tok[r]] or (got[r] == 0).all())


def test_weighted_form_with_unit_advantage_is_cross_entropy():
    K, n = 260, 16
    g, z, tok = _case(K, n, seed=5)
    cmin, cmax = P.clip_bounds(0.2, 0.2)
    full = np.ones(K, bool)
    rows = [P.row(z[r], int(tok[r]), 1.0, None, 1.0, full, cmin, cmax, 0.0) for r in range(n)]
    want = F.cross_entropy(torch.tensor(z.astype(np.float64)), torch.from_numpy(tok), reduction="none").numpy()
    assert np.abs(np.array([r["loss"] for r in rows]) - want).max() < 1e-12
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    F.cross_entropy(zt.masked_fill(torch.isinf(zt), -1e300), torch.from_numpy(tok)).backward()
    got = np.stack([P.dlogits_row(z[r], int(tok[r]), 1.0, None, 1.0, full, cmin, cmax, 0.0, 1.0 / n) for r in range(n)])
    assert np.abs(got - zt.grad.numpy()).max() < 1e-12
    assert abs(P.summary([(r, 0.0) for r in rows], False)[0] - want.mean()) < 1e-12


def test_on_policy_ratio_is_one_and_outside_rows_count_apart():
    z = np.log(np.array([0.5, 0.3, 0.15, 0.05])).astype(np.float32)
    N = R.exact_set(z, 1.0, 2, 1.0)
    assert N.tolist() == [True, True, False, False]
    cmin, cmax = P.clip_bounds(0.2, 0.2)
    lp = R.stats_for_set(z, 1, 1.0, 0, N)["policy_logprob"]
    on = P.row(z, 1, 2.0, lp, 1.0, N, cmin, cmax, 0.0)
    assert on["rho"] == 1.0 and not on["off"] and abs(on["loss"] + 2.0) < 1e-15 and on["g"] == -2.0
    out = P.row(z, 3, 2.0, -1.0, 1.0, N, cmin, cmax, 0.1)
    assert out["outside"] and out["loss"] == 0.0 and out["g"] == 0.0
    assert (P.dlogits_row(z, 3, 2.0, -1.0, 1.0, N, cmin, cmax, 0.1, 1.0) == 0).all()
    s = P.summary([(on, lp), (out, -1.0)], True)
    assert s[4] == 0.5 and s[3] == 0.0 and abs(s[0] + 1.0) < 1e-15 and s[2] == 0.0
    hi = P.row(z, 1, 2.0, lp - 1.0, 1.0, N, cmin, cmax, 0.0)        # rho = e > 1 + clip_hi with A > 0: the clip switches the gradient off
    assert hi["off"] and hi["g"] == 0.0 and abs(hi["loss"] + 2.0 * cmax) < 1e-12


def test_header_and_table_name_the_two_entry_points():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", header, flags=re.M))
    assert {"mage_policy_loss", "mage_policy_loss_bwd"} <= declared and declared == set(_lib.EXT_SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    for name in ("mage_policy_loss", "mage_policy_loss_bwd"):
        res, args = _lib.EXT_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        n_decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1).count(",") + 1
        assert n_decl == len(args)


PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched
FWD_ORDER = ("logits", "rows", "K", "ld", "tokens", "advantage", "adv_div", "behaviour_logprob", "temperature", "top_k", "top_p", "clip_lo",
             "clip_hi", "entropy_coef", "row_loss", "logprob", "entropy", "cut", "summary")
BWD_ORDER = ("logits", "rows", "K", "ld", "tokens", "advantage", "adv_div", "behaviour_logprob", "cut", "temperature", "clip_lo", "clip_hi",
             "entropy_coef", "grad_out", "dlogits", "dl_dtype")
GOOD = dict(logits=PTR, rows=8, K=512, ld=512, tokens=PTR, advantage=PTR, adv_div=4, behaviour_logprob=PTR, temperature=1.0, top_k=20, top_p=0.9,
            clip_lo=0.2, clip_hi=0.2, entropy_coef=0.01, row_loss=PTR, logprob=PTR, entropy=PTR, cut=PTR, summary=PTR, grad_out=PTR, dlogits=PTR,
            dl_dtype=_lib.BF16)
SHARED_BAD = [
    dict(logits=None), dict(tokens=None), dict(advantage=None), dict(cut=None), dict(K=6, ld=8), dict(K=4100, ld=4100), dict(K=0), dict(rows=0),
    dict(ld=510), dict(ld=256), dict(adv_div=0), dict(adv_div=-1), dict(logits=PTR + 4),
    dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=INF), dict(temperature=NAN), dict(temperature=1e-45),
    dict(clip_lo=-0.1), dict(clip_lo=1.5), dict(clip_lo=NAN), dict(clip_hi=-0.1), dict(clip_hi=NAN), dict(entropy_coef=INF), dict(entropy_coef=NAN),
]


@pytest.mark.parametrize("bad", SHARED_BAD + [
    dict(top_k=1), dict(top_k=-1), dict(top_k=513), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=NAN),
    dict(row_loss=None), dict(logprob=None), dict(entropy=None), dict(summary=None)])
def test_policy_loss_refuses_bad_arguments(bad):
    a = {**GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_policy_loss(*[a[k] for k in FWD_ORDER], None)
    assert rc == -1 and "mage_policy_loss" in lib.mage_last_error().decode() and "mage_init" not in lib.mage_last_error().decode(), (bad, rc)


@pytest.mark.parametrize("bad", SHARED_BAD + [dict(grad_out=None), dict(dlogits=None), dict(dlogits=PTR + 8), dict(dl_dtype=_lib.F16),
                                              dict(dl_dtype=7)])
def test_policy_loss_bwd_refuses_bad_arguments(bad):
    a = {**GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_policy_loss_bwd(*[a[k] for k in BWD_ORDER], None)
    assert rc == -1 and "mage_policy_loss_bwd" in lib.mage_last_error().decode(), (bad, rc)


def test_policy_loss_accepts_what_the_rule_allows():
    """The accepted forms get past the argument rules: without an initialised device the forward call stops at the mage_init check behind
    them.  (The backward call has no such check to stop at: its accepted forms run on the GPU, tests/test_gpu_policy_loss.py.)"""
    lib = _lib.load()
    for ok in (dict(), dict(behaviour_logprob=None), dict(top_k=0, top_p=1.0), dict(top_k=512), dict(top_k=2), dict(K=4096, ld=4096),
               dict(K=4, ld=8, top_k=2), dict(clip_lo=0.0, clip_hi=0.0), dict(clip_lo=1.0, clip_hi=INF), dict(entropy_coef=-0.5), dict(adv_div=8)):
        a = {**GOOD, **ok}
        rc = lib.mage_policy_loss(*[a[k] for k in FWD_ORDER], None)
        assert rc == -1 and "mage_init" in lib.mage_last_error().decode(), (ok, rc, lib.mage_last_error())


def test_cpu_tensors_are_refused():
    z, tok, A = torch.zeros(8, 16), torch.zeros(8, dtype=torch.int64), torch.ones(8)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.policy_loss(z, tok, A)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.policy_loss_bwd(z, tok, A, None, torch.zeros(8, dtype=torch.int32), torch.ones(1), torch.empty(8, 16))
    L = 4
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=16), 0)
    batch = synth.synth_batch_mnist(2, L, seed=1)
    R_ = m.image_resolution
    tokens = torch.zeros(2, L - 1, R_, R_, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        m.policy_loss(batch, tokens, torch.ones(2))
    assert m.last_policy_token_logprobs is None
