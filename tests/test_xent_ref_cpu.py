"""CPU: the fp64 restatement of the supervised loss (tests/xent_ref.py) against F.cross_entropy(weight, label_smoothing, ignore_index) and
torch.autograd, the z-loss term against zeta * mean(logsumexp^2), the library's surface (the two entry points are declared, bound, and refuse
bad arguments before anything is launched), balanced_class_weights on hand-made counts, and MAGE.set_loss / evaluate's refusals on a CPU
model (no library call)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mage_amd import _lib, ops
from mage_amd.utils import synth
from mage_amd.utils.glue import balanced_class_weights
from tests import xent_ref as X
from tests.helpers import build_mage, count_lib_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 11
NEW = ("mage_token_xent", "mage_token_xent_bwd")
PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched
RTOL = 1e-12                # a few fp64 ulps


def _inputs(K, seed=3):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((ROWS, K))).astype(np.float32)
    y = g.integers(0, K, ROWS)
    y[0], y[1] = 0, K - 1
    w = g.uniform(0.25, 3.0, K).astype(np.float32)
    w[2] = 0.0                                                       # an unused code's weight
    given = np.zeros(ROWS, bool)
    given[[3, 7, 8]] = True
    return z, y, w, given


def _grad(z, y, w, eps, zeta, given, g=0.7):
    """The restatement's dlogits for the whole call, with exact (fp64) coefficients and norms."""
    ref = X.loss(z, y, w, eps, zeta, given, fp32=False)
    n0, n1 = (1.0 / ref["sw"] if ref["sw"] > 0 else 0.0), (1.0 / ref["n_free"] if ref["n_free"] else 0.0)
    out = np.zeros(z.shape)
    for i, r in enumerate(ref["rows"]):
        if r is not None:
            out[i], bound = X.dlogits_row(r, g, n0, n1, zeta)
            assert (bound > 0).all()
    return ref, out


@pytest.mark.parametrize("K", [12, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
def test_reference_is_cross_entropy_and_its_gradient(K, weighted, eps, masked):
    z, y, w, given = _inputs(K)
    w = w if weighted else None
    given = given if masked else None
    ref, grad = _grad(z, y, w, eps, 0.0, given)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    tgt = torch.from_numpy(y.copy())
    if masked:
        tgt[torch.from_numpy(given)] = -100
    wt = None if w is None else torch.tensor(w, dtype=torch.float64)
    want = F.cross_entropy(zt, tgt, weight=wt, ignore_index=-100, label_smoothing=eps)
    assert abs(ref["summary"][0] - want.item()) <= RTOL * abs(want.item())
    (0.7 * want).backward()
    auto = zt.grad.numpy()
    assert np.abs(grad - auto).max() <= RTOL * np.abs(auto).max(), np.abs(grad - auto).max()
    if masked:
        assert (grad[given] == 0).all() and (ref["row_loss"][given] == 0).all() and ref["summary"][4] == 3 / ROWS
    # per row: reduction='none' is the row_loss, the unweighted nll and the rank are what they say
    none = F.cross_entropy(zt.detach(), tgt, weight=wt, ignore_index=-100, label_smoothing=eps, reduction="none").numpy()
    assert np.allclose(ref["row_loss"], none, rtol=RTOL, atol=1e-13)
    lsm = torch.log_softmax(zt.detach(), -1).numpy()
    free = np.ones(ROWS, bool) if given is None else ~given
    assert np.allclose(ref["row_nll"][free], -lsm[np.arange(ROWS), y][free], rtol=RTOL, atol=1e-13)
    assert abs(ref["summary"][1] - (-lsm[np.arange(ROWS), y][free]).mean()) <= 1e-12
    assert ref["summary"][2] == np.mean((z.argmax(1) == y)[free])
    order = np.argsort(-z, axis=1, kind="stable")
    assert all(ref["rank"][i] == int(np.flatnonzero(order[i] == y[i])[0]) for i in np.flatnonzero(free))


@pytest.mark.parametrize("K", [12, 64])
def test_z_loss_term(K):
    z, y, w, given = _inputs(K, seed=5)
    zeta = 1e-3
    for ww, eps, gv in ((None, 0.0, None), (w, 0.1, given)):
        ref, grad = _grad(z, y, ww, eps, zeta, gv)
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        keep = torch.ones(ROWS, dtype=torch.bool) if gv is None else torch.from_numpy(~gv)
        zterm = zeta * (torch.logsumexp(zt[keep], -1) ** 2).mean()
        plain = X.loss(z, y, ww, eps, 0.0, gv, fp32=False)
        assert abs((ref["summary"][0] - plain["summary"][0]) - zterm.item()) <= 1e-12 * max(1.0, abs(ref["summary"][0]))
        assert abs(ref["summary"][3] * zeta - zterm.item()) <= RTOL * zterm.item()
        gt = None if gv is None else torch.from_numpy(gv)
        wt = None if ww is None else torch.tensor(ww, dtype=torch.float64)
        (0.7 * X.torch_loss(zt, torch.from_numpy(y), wt, eps, zeta, gt)).backward()
        auto = zt.grad.numpy()
        assert np.abs(grad - auto).max() <= RTOL * np.abs(auto).max()


def test_special_rows_and_empty_sums():
    K = 12
    z, y, w, _ = _inputs(K)
    inf = z[0].copy()
    inf[5] = -np.inf
    assert np.isfinite(X.row(inf, 1)["loss"]) and np.isposinf(X.row(inf, 1, None, 0.1)["loss"]) and np.isposinf(X.row(inf, 5)["nll"])
    nan = z[0].copy()
    nan[4] = np.nan
    assert np.isnan(X.row(nan, 1)["loss"]) and X.row(nan, 4)["rank"] == K and X.row(nan, 1)["rank"] == int((np.delete(z[0], 4) > z[0][1]).sum())
    assert np.isnan(X.row(np.full(K, -np.inf, np.float32), 0)["lse"]) and X.rank(np.full(K, -np.inf, np.float32), 3) == 3
    ties = np.array([1.0, 2.0, 2.0, -0.0, 0.0, 2.0, np.nan, 0.5], np.float32)
    assert [X.rank(ties, j) for j in range(8)] == [3, 0, 1, 5, 6, 2, 8, 4]
    g = X.loss(z, y, w, 0.1, 1e-3, np.ones(ROWS, bool))              # everything given: zeros, no NaN
    assert g["n_free"] == 0 and (g["summary"][:4] == 0).all() and g["summary"][4] == 1 and (X.norms(g["sw"], 0) == 0).all()
    only = np.zeros(K, np.float32)                                   # every free target has weight 0: the weighted mean is +0, not 0 / 0
    only[int(y[0]) ^ 1] = 1.0
    h = X.loss(z[:1], y[:1], only, 0.0, 0.0)
    assert h["sw"] == 0 and h["summary"][0] == 0 and X.norms(h["sw"], 1)[0] == 0 and X.norms(h["sw"], 1)[1] == 1
    assert X.coefs(0.1, 64) == (float(np.float32(0.9)), float(np.float32(0.1 / 64))) and X.coefs(0.1, 64, False) == (0.9, 0.1 / 64)


def test_balanced_class_weights():
    counts = torch.tensor([100, 0, 25, 4, 0, 1], dtype=torch.int64)
    w = balanced_class_weights(counts)
    assert w.dtype == torch.float32 and w.shape == (6,) and w[1] == 0 and w[4] == 0
    raw = np.array([0.1, 0, 0.2, 0.5, 0, 1.0])
    c = counts.numpy().astype(np.float64)
    want = raw * c.sum() / (raw * c).sum()
    assert np.allclose(w.numpy(), want, rtol=1e-6)
    assert abs((w.double() * counts).sum().item() / counts.sum().item() - 1) < 1e-6          # the count-weighted mean weight is 1
    assert torch.equal(balanced_class_weights(counts, 0.0), (counts > 0).float())
    w1 = balanced_class_weights(counts, 1.0)
    used = counts > 0
    assert np.allclose((w1.double() * counts)[used].numpy(), counts.sum().item() / used.sum().item())      # equal total weight per used code
    assert (balanced_class_weights(torch.zeros(4, dtype=torch.int64)) == 0).all()
    for bad in (counts.float(), counts.view(2, 3), counts[:0], [1, 2]):
        with pytest.raises(ValueError, match="counts must be"):
            balanced_class_weights(bad)
    for bad in (-0.5, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="power must be"):
            balanced_class_weights(counts, bad)


# ------------------------------------------------------------------------------------------------ the library's surface
def test_header_and_table_name_the_entry_points():
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
    assert len(_lib.EXT_SIGNATURES["mage_token_xent"][1]) == 16 and len(_lib.EXT_SIGNATURES["mage_token_xent_bwd"][1]) == 14
    assert {"token_xent", "token_xent_bwd"} <= set(ops.__all__)
    assert "THE NEGATION OF mage_token_logprob's VALUE" in header       # the promise tests/test_gpu_xent_kernels.py relies on is stated
    src = open(os.path.join(ROOT, "mage_amd", "csrc", "Makefile")).read()
    assert "xent.hip" in re.search(r"^SRCS = (.*)$", src, flags=re.M).group(1).split()


FWD = dict(logits=PTR, rows=8, K=16, ld=20, target=PTR, class_weight=PTR, label_smoothing=0.1, z_loss=1e-3, given=None, row_loss=PTR, row_nll=PTR,
           row_lse=PTR, rank=None, summary=PTR, norm=PTR)
BWD = dict(logits=PTR, rows=8, K=16, ld=20, target=PTR, class_weight=None, label_smoothing=0.0, z_loss=0.0, given=PTR, grad_out=PTR, norm=PTR,
           dlogits=PTR, dl_dtype=0)
BAD = [dict(logits=None), dict(target=None), dict(norm=None), dict(rows=0), dict(rows=-1), dict(K=0), dict(K=15), dict(K=4100, ld=4100), dict(ld=12),
       dict(ld=18), dict(logits=PTR + 4), dict(target=PTR + 4), dict(class_weight=PTR + 8), dict(label_smoothing=-0.1), dict(label_smoothing=1.0),
       dict(label_smoothing=float("nan")), dict(z_loss=-1e-3), dict(z_loss=float("inf")), dict(z_loss=float("nan")), dict(norm=PTR + 2)]


@pytest.mark.parametrize("bad", BAD + [dict(row_loss=None), dict(row_nll=None), dict(row_lse=None), dict(summary=None), dict(row_loss=PTR + 2),
                                       dict(rank=PTR + 2), dict(summary=PTR + 1)], ids=str)
def test_forward_refuses_bad_arguments(bad):
    lib = _lib.load()
    assert lib.mage_token_xent(*{**FWD, **bad}.values(), None) == -1 and b"mage_token_xent" in lib.mage_last_error(), bad


@pytest.mark.parametrize("bad", BAD + [dict(grad_out=None), dict(grad_out=PTR + 2), dict(dlogits=None), dict(dlogits=PTR + 8), dict(dl_dtype=2),
                                       dict(dl_dtype=4)], ids=str)
def test_backward_refuses_bad_arguments(bad):
    lib = _lib.load()
    assert lib.mage_token_xent_bwd(*{**BWD, **bad}.values(), None) == -1 and b"mage_token_xent_bwd" in lib.mage_last_error(), bad


# ------------------------------------------------------------------------------------------------ Python refusals on a CPU model
def test_set_loss_and_evaluate_refuse_before_any_library_call(monkeypatch):
    calls = count_lib_calls(monkeypatch, _lib.load())
    L, Kc = 4, 16
    m = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=Kc), 0)
    batch = synth.synth_batch_mnist(2, L, seed=0)
    R = m.image_resolution
    tshape = (2, L - 1, R, R)

    def refused(match, fn, *a, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*a, **kw)
        assert calls == []

    assert m.set_loss() is m and m.loss_options is None
    for bad in (-0.1, 1.0, float("nan"), True, "0.1"):
        refused("label_smoothing must", m.set_loss, label_smoothing=bad)
    for bad in (-1e-3, float("inf"), float("nan"), True):
        refused("z_loss must", m.set_loss, z_loss=bad)
    ones = torch.ones(Kc)
    for bad in (ones.double(), ones[:-1], ones.view(4, 4), -ones, torch.zeros(Kc), torch.full((Kc,), float("nan")), [1.0] * Kc):
        refused("class_weights must", m.set_loss, class_weights=bad)
    assert m.loss_options is None                                     # a refused call changes nothing
    assert m.set_loss(0.1, 1e-3, ones) is m and m.loss_options["label_smoothing"] == 0.1 and m.loss_options["z_loss"] == 1e-3
    assert m.set_loss(class_weights=ones).loss_options["label_smoothing"] == 0.0
    assert m.set_loss().loss_options is None                          # the defaults: forward is the plain call again
    refused("ROCm GPU", m.evaluate, batch)                            # everything is well-formed but lives on the CPU
    refused("given must be bool", m.evaluate, batch, given=torch.zeros(tshape))
    refused("ROCm GPU", m.evaluate, batch, given=torch.zeros(tshape, dtype=torch.bool))
    for bad in ((), (0,), (Kc + 1,), (1.5,), 5, (True,)):
        refused("topk must", m.evaluate, batch, topk=bad)
    refused("known_tokens", m.evaluate, {**batch, "known_tokens": torch.zeros(tshape, dtype=torch.int64)})
    m.set_context(2)
    refused("set_context", m.evaluate, batch)
    m.set_context(1)
    m.set_guidance(2.0)
    refused("guidance is on", m.evaluate, batch)
    m.set_guidance(None)
    with torch.no_grad():
        refused("given must be bool", m.forward, {**batch, "given": torch.zeros(tshape)})
        refused("ROCm GPU", m.forward, {**batch, "given": torch.zeros(tshape, dtype=torch.bool)})
    # MAGE+ and a codebook that is no multiple of 4 have no rows for the kernel
    odd = build_mage(synth.mnist_model_config(frames_length=L, width=64, layers=1, vq_dim=32, K=18), 0)
    refused("multiple of 4", odd.set_loss, label_smoothing=0.1)
    refused("multiple of 4", odd.evaluate, batch)
    assert odd.set_loss() is odd                                      # restoring the defaults is always allowed
