"""CPU: the fp64 restatement of the distillation loss (tests/distill_ref.py) against torch.autograd and the textbook KL, the library's
surface (the two entry points are declared, bound, and refuse bad arguments before anything is launched) and MAGE.distill_loss /
MAGE.distill_targets' refusals on a CPU model (no library call)."""
import os
import re

import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from mage_amd.utils import synth
from tests import distill_ref as D
from tests import sampling_ref as S
from tests.helpers import build_mage, count_lib_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, K = 9, 12
NEW = ("mage_distill_loss", "mage_distill_loss_bwd")
PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched


def _pair(seed=5):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((ROWS, K))).astype(np.float32)
    t = (2.0 * g.standard_normal((ROWS, K))).astype(np.float32)
    z[3, [1, 7]] = -np.inf                                           # the student excludes two codes: forward KL +inf, reverse finite
    t[4, [0, 2, 5]] = -np.inf                                        # the teacher excludes three: forward finite, reverse +inf
    z[5, 2:6] = t[5, 2:6] = -np.inf                                  # both exclude the same codes: both finite
    return z, t


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [0.7, 1.0, 2.0])
def test_reference_matches_autograd_and_the_textbook_sum(T, mode):
    z, t = _pair()
    inv_t = float(S.inv_temperature(T))
    s = torch.tensor(D.scaled(z, T), requires_grad=True)             # the kernel's fp32 products, then fp64: autograd on the same numbers
    u = torch.tensor(D.scaled(t, T))
    ref = D.loss(z, t, T, mode)
    inf_row = 3 if mode == 0 else 4
    fin = np.arange(ROWS) != inf_row
    assert np.isposinf(ref["row_kl"][inf_row]) and np.isfinite(ref["row_kl"][fin]).all() and (ref["row_kl"][fin] > 0).all()
    given = torch.from_numpy(~fin)
    # the identity kl = A / Z_P + log Z_Q - log Z_P against sum p (log p - log q)
    lp, lq = (torch.log_softmax(u, -1), torch.log_softmax(s, -1)) if mode == 0 else (torch.log_softmax(s, -1), torch.log_softmax(u, -1))
    book = torch.where(lp.exp() > 0, lp.exp() * (lp - lq), torch.zeros_like(lp)).sum(-1).detach().numpy()
    assert np.allclose(ref["row_kl"][fin], book[fin], rtol=1e-12, atol=1e-13)
    # the gradient of the mean over the finite rows
    D.torch_kl(s, u, 1.0, mode, given).backward()
    auto = s.grad.numpy() * inv_t                                    # d / dz = inv_t d / ds
    c = 1.0 / fin.sum() * inv_t
    for i in np.flatnonzero(fin):
        want, bound = D.dlogits_row(z[i], t[i], T, mode, c)
        assert np.allclose(want, auto[i], rtol=1e-11, atol=1e-14), (i, np.abs(want - auto[i]).max())
        assert (bound > 0).all() and (bound[np.abs(want) > 1e-6] < 1e-3 * np.abs(want[np.abs(want) > 1e-6]) + 1e-4 * abs(c)).all()
    want, _ = D.dlogits_row(z[inf_row], t[inf_row], T, mode, c)     # the documented choice: a row without a finite KL gets zeros
    assert (want == 0).all()
    # the summary: means over the free rows, entropies of both sides, agreement by the first maximum
    m = D.loss(z, t, T, mode, given=~fin)
    assert m["n_free"] == ROWS - 1 and m["summary"][4] == 1 / ROWS and m["row_kl"][inf_row] == 0
    assert abs(m["summary"][0] - book[fin].mean()) < 1e-12
    ent = lambda x: -(torch.softmax(x, -1) * torch.where(torch.isinf(x), torch.zeros_like(x), torch.log_softmax(x, -1))).sum(-1)      # noqa: E731
    assert abs(m["summary"][1] - ent(u)[given.logical_not()].mean().item()) < 1e-12
    assert abs(m["summary"][2] - ent(s.detach())[given.logical_not()].mean().item()) < 1e-12
    assert m["summary"][3] == np.mean([np.argmax(z[i]) == np.argmax(t[i]) for i in np.flatnonzero(fin)])


def test_equal_rows_give_zero_and_special_rows_their_values():
    z, _ = _pair()
    for mode in (0, 1):
        for T in (0.7, 1.0, 2.0):
            r = D.loss(z, z.copy(), T, mode)
            assert (r["row_kl"] == 0).all() and not np.signbit(r["row_kl"]).any() and r["summary"][0] == 0 and r["summary"][3] == 1
            for i in range(ROWS):
                assert (D.dlogits_row(z[i], z[i], T, mode, 0.3)[0] == 0).all()
    nan = z.copy()
    nan[0, 3] = np.nan
    allinf = np.full(K, -np.inf, np.float32)
    for mode in (0, 1):
        assert np.isnan(D.row(nan[0], z[0], 1.0, mode)["kl"]) and np.isnan(D.row(z[0], nan[0], 1.0, mode)["kl"])
        assert np.isnan(D.row(allinf, z[0], 1.0, mode)["kl"]) and np.isnan(D.row(z[0], allinf, 1.0, mode)["kl"])
    assert D.argmax(np.array([1.0, np.nan, 3.0, 3.0], np.float32)) == 2 and D.argmax(np.full(4, np.nan, np.float32)) == 0x7fffffff
    assert D.argmax(allinf) == 0 and D.argmax(np.array([-0.0, 0.0], np.float32)) == 0
    g = D.loss(z, z, 1.0, 0, given=np.ones(ROWS, bool))                # everything given: zeros, no NaN
    assert g["n_free"] == 0 and (g["summary"][:4] == 0).all() and g["summary"][4] == 1


# ------------------------------------------------------------------------------------------------ the library's surface
def test_header_and_table_name_the_distillation_entry_points():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", header, flags=re.M))
    assert set(NEW) <= declared and declared == set(_lib.EXT_SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    for name in NEW:
        res, args = _lib.EXT_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        n_decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1).count(",") + 1
        assert n_decl == len(args), name
    assert len(_lib.EXT_SIGNATURES["mage_distill_loss"][1]) == 13 and len(_lib.EXT_SIGNATURES["mage_distill_loss_bwd"][1]) == 15
    assert {"distill_loss", "distill_loss_bwd"} <= set(ops.__all__)
    assert "EXACTLY +0" in header                                     # the promise tests/test_gpu_distill*.py rely on is stated


FWD = dict(logits=PTR, rows=8, K=16, ld=16, teacher=PTR, ld_t=20, temperature=1.0, mode=0, given=None, row_kl=PTR, summary=PTR, norm=PTR)
BWD = dict(logits=PTR, rows=8, K=16, ld=16, teacher=PTR, ld_t=20, temperature=1.0, mode=1, given=PTR, row_kl=PTR, grad_out=PTR, norm=PTR,
           dlogits=PTR, dl_dtype=0)
BAD = [dict(logits=None), dict(teacher=None), dict(row_kl=None), dict(norm=None), dict(rows=0), dict(K=0), dict(K=15, ld=16), dict(K=4100, ld=4100, ld_t=4100),
       dict(ld=12), dict(ld=18), dict(ld_t=12), dict(ld_t=18), dict(logits=PTR + 4), dict(teacher=PTR + 8), dict(temperature=0.0),
       dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(mode=2), dict(mode=-1),
       dict(row_kl=PTR + 2), dict(norm=PTR + 1)]


@pytest.mark.parametrize("bad", BAD + [dict(summary=None), dict(summary=PTR + 2)], ids=str)
def test_forward_refuses_bad_arguments(bad):
    lib = _lib.load()
    assert lib.mage_distill_loss(*{**FWD, **bad}.values(), None) == -1 and b"mage_distill_loss" in lib.mage_last_error(), bad


@pytest.mark.parametrize("bad", BAD + [dict(grad_out=None), dict(grad_out=PTR + 2), dict(dlogits=None), dict(dlogits=PTR + 8), dict(dl_dtype=2),
                                       dict(dl_dtype=4)], ids=str)
def test_backward_refuses_bad_arguments(bad):
    lib = _lib.load()
    assert lib.mage_distill_loss_bwd(*{**BWD, **bad}.values(), None) == -1 and b"mage_distill_loss_bwd" in lib.mage_last_error(), bad


# ------------------------------------------------------------------------------------------------ Python refusals on a CPU model
def test_distill_methods_refuse_before_any_library_call(monkeypatch):
    calls = count_lib_calls(monkeypatch, _lib.load())
    L, Kc = 4, 16
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=Kc), 0)
    batch = synth.synth_batch_mnist(2, L, seed=0)
    R = m.image_resolution
    tshape = (2, L - 1, R, R)
    tok = torch.zeros(tshape, dtype=torch.int64)
    rows = 2 * (L - 1) * R * R
    tl = torch.zeros(rows, Kc)
    fwd_before = m.forward

    def refused(match, *a, fn=None, **kw):
        with pytest.raises(ValueError, match=match):
            (fn or m.distill_loss)(*a, **kw)
        assert calls == [] and m.last_distill_token_kl is None and m.forward == fwd_before

    refused("tokens must be int64", batch, tok.int(), tl)
    refused("tokens must be int64", batch, tok[:, :1], tl)
    refused("batch must be a dict", None, tok, tl)
    refused("teacher_logits must be fp32", batch, tok, tl.double())
    refused("teacher_logits must be fp32", batch, tok, tl[:-1])
    refused("teacher_logits must be fp32", batch, tok, tl[:, :-4])
    refused("teacher_logits must be fp32", batch, tok, None)
    for bad in (0.0, -1.0, float("inf"), float("nan"), True, "1"):
        refused("temperature must be finite and > 0", batch, tok, tl, temperature=bad)
    for bad in ("fwd", 0, None):
        refused("mode must be one of", batch, tok, tl, mode=bad)
    refused("given must be bool", batch, tok, tl, given=torch.zeros(tshape))
    refused("given must be bool", batch, tok, tl, given=torch.zeros(tshape[:-1], dtype=torch.bool))
    refused("ROCm GPU", batch, tok, tl, given=torch.zeros(tshape, dtype=torch.bool))
    refused("ROCm GPU", batch, tok, tl)                               # everything is well-formed but lives on the CPU
    refused("known_tokens", {**batch, "known_tokens": tok}, tok, tl)
    m.set_context(2)
    refused("set_context", batch, tok, tl)
    refused("set_context", batch, tok, fn=m.distill_targets)
    m.set_context(1)
    m.set_guidance(2.0)
    refused("guidance is on", batch, tok, tl)                         # the student runs unguided
    refused("ROCm GPU", batch, tok, fn=m.distill_targets)             # ... the teacher may be guided: it gets as far as the device check
    m.set_guidance(None)
    refused("tokens must be int64", batch, tok.int(), fn=m.distill_targets)
    refused("ROCm GPU", batch, tok, fn=m.distill_targets)
    m.set_precision("f16")
    refused("precision 'f16'", batch, tok, tl)
