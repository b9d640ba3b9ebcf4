"""GPU: mage_policy_loss_masked / mage_policy_loss_masked_bwd (include/mage_hip_ext.h) against the unmasked entry points, bit for bit.

The unmasked pair is pinned against fp64 in tests/test_gpu_policy_loss.py (its `_logits` recipe and `Case` are imported from there, not
restated); here a free row must carry that pair's bits and a given row must be +0 without having been read.
  all-free mask      every per-row output, summary[0..5) (plain) or [0..7) (anchored) and dlogits: the unmasked call's bits; summary[7] == 0.
  any mask, free     per-row forward outputs: the unmasked call's bits on the same rows; dlogits: the bits of the unmasked backward call run
                     on the free rows gathered into a contiguous n_free-row tensor (a row's bits depend on the row and 1.0f / (float)n_free).
  given rows         every output +0 by bits, cut 0 -- with the given rows' logits NaN and their tokens out of range (nothing is raised).
  summary            the fp64 means over the free rows of the kernel's own per-row outputs, one fp32 rounding: 2^-24 relative (the bound of
                     tests/test_gpu_policy_loss.py for the same reduction); summary[7] and norm exact.
  all given          zeros, norm == 0, no NaN.   determinism: two launches, the same bits.   refusals: MAGE_EINVAL, nothing launched."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import policy_ref as P
from tests.test_gpu_policy_loss import CLIP, Case, _bits, _logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOUT = 0.7
# (top_k, top_p, temperature, clipped, anchored, gradient dtype, adv_div, entropy_coef): both rules, both forms, both dtypes, every filter
CONFIGS = [(0, 1.0, 1.0, False, False, torch.float32, 1, 0.0),
           (20, 0.9, 0.7, True, True, torch.bfloat16, 5, 0.01),
           (0, 0.9, 1.5, True, False, torch.bfloat16, 1, 0.01),
           (20, 1.0, 0.7, False, True, torch.float32, 5, 0.0)]
KL_COEF = 0.1


def _masks(rows, seed):
    g = np.random.default_rng(seed)
    first = np.zeros(rows, bool)
    first[:13] = True                                                # the special rows of _logits (1, 2, 8, 9, 10, 12): NaN, all -inf, +-100
    return {"free": np.zeros(rows, bool), "given": np.ones(rows, bool), "alternating": np.arange(rows) % 2 == 1, "first13": first,
            "random": g.random(rows) < 0.45}


def _dbits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Launch:
    """One configuration over one set of rows: the unmasked pair's results (on the clean inputs) and what the masked pair is called with."""

    def __init__(self, z, zd, K, cfg, seed):
        k, p, T, clipped, anch, dt, adv_div, c = cfg
        k = min(k, K // 2)
        self.case = case = Case(z, zd, K, T, k, p, seed=seed, clipped=clipped, adv_div=adv_div, c=c)
        self.dt, self.anch, self.rows, self.K = dt, anch, z.shape[0], K
        self.ref = None
        if anch:                                                     # near the policy's own values; row 4 -inf, row 5 NaN (unanchored), row 6 d == 0
            g = np.random.default_rng(seed + 1)
            lp = case.stats["policy_logprob"].cpu().numpy()
            r = (np.where(np.isfinite(lp), lp, -1.0) + g.uniform(-0.3, 0.3, self.rows)).astype(np.float32)
            r[4], r[5], r[6] = -np.inf, np.nan, lp[6]
            self.ref = torch.from_numpy(r).to(DEV)
        self.kw = dict(temperature=T, clip_lo=CLIP[0], clip_hi=CLIP[1], entropy_coef=c, adv_div=adv_div,
                       **(dict(reference_logprob=self.ref, kl_coef=KL_COEF) if anch else {}))
        self.filt = dict(top_k=k, top_p=p)
        self.gout = torch.tensor([GOUT], device=DEV)
        self.U = ops.policy_loss(zd, case.tok, case.Ad, case.bd, **self.kw, **self.filt)
        self.dU = self.backward(zd, case.tok, self.U["cut"])

    def backward(self, zd, tok, cut, *, A=None, b=None, given=None, norm=None, **over):
        dl = torch.empty(zd.shape[0], self.K, device=DEV, dtype=self.dt)
        return ops.policy_loss_bwd(zd, tok, self.case.Ad if A is None else A, self.case.bd if b is None else b, cut, self.gout, dl,
                                   **{**self.kw, **over}, given=given, norm=norm)

    def gathered(self, zd, free):
        """The unmasked backward call on the free rows alone, contiguous: one advantage per row (adv_div 1)."""
        idx = torch.from_numpy(np.flatnonzero(free)).to(DEV)
        case = self.case
        A = case.Ad[idx // case.adv_div].contiguous()
        over = dict(A=A, b=None if case.bd is None else case.bd[idx].contiguous(), adv_div=1)
        if self.anch:
            over["reference_logprob"] = self.ref[idx].contiguous()
        return self.backward(zd[idx].contiguous(), case.tok[idx].contiguous(), self.U["cut"][idx].contiguous(), **over)


def _close(got, want, what):
    """2^-24 relative where the wanted value is finite; the same non-finite value otherwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (what, got, want)
    assert (np.abs(got[fin] - want[fin]) <= 2.0 ** -24 * np.abs(want[fin]) * (1 + 1e-6)).all(), (what, got, want)


def _check_mask(L, zd, name, given_np):
    case, rows, K = L.case, L.rows, L.K
    given = torch.from_numpy(given_np).to(DEV)
    free = ~given_np
    n_free = int(free.sum())
    # the given rows hold NaN logits and out-of-range tokens: they must not be read, and nothing may be raised for them
    zp, tokp = torch.empty_strided(zd.shape, zd.stride(), device=DEV), case.tok.clone()       # (the row stride is part of the case)
    zp.copy_(zd)
    zp[given] = float("nan")
    tokp[given] = torch.where(torch.arange(rows, device=DEV) % 2 == 0, K + 7, -3)[given]
    out = ops.policy_loss(zp, tokp, case.Ad, case.bd, **L.kw, **L.filt, given=given)
    dl = L.backward(zp, tokp, out["cut"], given=given, norm=out["norm"])
    again = ops.policy_loss(zp, tokp, case.Ad, case.bd, **L.kw, **L.filt, given=given)
    dl2 = L.backward(zp, tokp, again["cut"], given=given, norm=again["norm"])
    ops.check_device_errors(DEV)                                     # (raises on a recorded token: the given rows' were not looked at)
    assert set(out) == set(L.U) | {"norm"}
    for n in out:                                                    # deterministic
        assert torch.equal(_bits(out[n]), _bits(again[n])), (name, n)
    assert torch.equal(_dbits(dl), _dbits(dl2)), name
    per_row = [n for n in out if n not in ("summary", "norm")]
    for n in per_row:
        assert torch.equal(_bits(out[n])[~given], _bits(L.U[n])[~given]), (name, n, "free rows: the unmasked call's bits")
        assert (_bits(out[n])[given] == 0).all(), (name, n, "given rows: +0")
    # the gradient
    assert (_dbits(dl)[given] == 0).all(), (name, "dlogits of the given rows: +0")
    if n_free:
        want = L.gathered(zd, free)
        assert torch.equal(_dbits(dl)[~given], _dbits(want)), (name, "dlogits of the free rows: the unmasked call on the gathered rows")
    # norm and the summary
    norm = out["norm"].cpu().numpy()
    want_norm = np.float32(1) / np.float32(n_free) if n_free else np.float32(0)
    assert norm.view(np.uint32)[0] == np.array([want_norm], np.float32).view(np.uint32)[0], (name, norm, want_norm)
    got = out["summary"].cpu().numpy()
    assert got.shape == (8,) and got[7] == np.float32(given_np.sum() / rows), (name, got)
    lp, h, loss = (out[n].cpu().numpy().astype(np.float64) for n in ("logprob", "entropy", "row_loss"))
    ins = free & ~np.isneginf(lp)
    want = np.zeros(7)
    if n_free:
        with np.errstate(invalid="ignore"):
            want[0], want[1], want[4] = loss[ins].sum(), h[ins].sum(), float((free & np.isneginf(lp)).sum())
            if case.b is not None:
                want[2] = (case.b.astype(np.float64)[ins] - lp[ins]).sum()
                want[3] = float(sum(P.term(lp[r], h[r], case.adv(r), float(case.b[r]), case.cmin, case.cmax, 0.0)["off"] for r in np.flatnonzero(ins)))
            if L.anch:
                want[5] = out["kl"].cpu().numpy().astype(np.float64)[ins].sum()
                want[6] = float((~np.isfinite(L.ref.cpu().numpy()))[ins].sum())
            want = want / n_free
    _close(got[:7], want, name)
    if not n_free:
        assert (out["summary"][:7].view(torch.int32) == 0).all() and got[7] == 1 and not np.isnan(got).any()
        assert not torch.isnan(dl.float()).any()
    if name == "free":                                               # the unmasked call as a whole
        n_sum = 7 if L.anch else 5
        assert torch.equal(_bits(out["summary"][:n_sum]), _bits(L.U["summary"])) and got[7] == 0 and (got[n_sum:7] == 0).all()
        assert torch.equal(_dbits(dl), _dbits(L.dU))


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
def test_masked_pair_against_the_unmasked_one(K):
    rows = 29
    z = _logits(rows, K, seed=K)
    zd = torch.from_numpy(z).to(DEV)
    for i, cfg in enumerate(CONFIGS):
        L = Launch(z, zd, K, cfg, seed=300 * K + i)
        for name, m in _masks(rows, seed=K + i).items():
            _check_mask(L, zd, name, m)


def test_several_workgroups_and_a_row_stride_above_K():
    rows, K = 259, 260
    z = _logits(rows, K, seed=77)
    zd = torch.zeros(rows, K + 4, device=DEV)[:, :K]
    zd.copy_(torch.from_numpy(z))
    assert zd.stride(0) == K + 4
    for i, cfg in enumerate(CONFIGS[1:3]):
        L = Launch(z, zd, K, cfg, seed=911 + i)
        masks = _masks(rows, seed=5 + i)
        for name in ("free", "first13", "random"):
            _check_mask(L, zd, name, masks[name])


def test_refusals_launch_nothing():
    rows, K = 8, 16
    l = _lib.lib(0)
    z = torch.randn(rows, K, device=DEV)
    tok = torch.zeros(rows, dtype=torch.int64, device=DEV)
    A = torch.ones(rows, device=DEV)
    ref = torch.zeros(rows, device=DEV)
    given = torch.zeros(rows, dtype=torch.bool, device=DEV)
    outs = [torch.full((rows,), 7.0, device=DEV) for _ in range(3)] + [torch.full((rows,), 7, dtype=torch.int32, device=DEV),
                                                                      torch.full((rows,), 7.0, device=DEV), torch.full((8,), 7.0, device=DEV),
                                                                      torch.full((1,), 7.0, device=DEV)]
    dl = torch.full((rows, K), 7.0, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def fwd(given=given, ref=ref, kl=outs[4]):
        return l.mage_policy_loss_masked(p(z), rows, K, K, p(tok), p(A), 1, None, p(ref), 1.0, 0, 1.0, 0.2, 0.2, 0.0, 0.0, p(outs[0]), p(outs[1]),
                                         p(outs[2]), p(outs[3]), p(kl), p(outs[5]), p(outs[6]), p(given), None)

    def bwd(given=given, norm=outs[6]):
        return l.mage_policy_loss_masked_bwd(p(z), rows, K, K, p(tok), p(A), 1, None, None, p(outs[3]), 1.0, 0.2, 0.2, 0.0, 0.0, p(outs[6]),
                                             p(norm), p(dl), 0, p(given), None)

    assert fwd(given=None) == -1 and b"given" in l.mage_last_error()
    assert fwd(kl=None) == -1 and b"together" in l.mage_last_error()         # a reference without kl
    assert fwd(ref=None) == -1 and b"together" in l.mage_last_error()        # kl without a reference
    assert bwd(given=None) == -1 and bwd(norm=None) == -1
    torch.cuda.synchronize()
    assert all((o == 7).all() for o in outs) and (dl == 7).all()
    with pytest.raises(AssertionError):                              # the wrapper: the mask and the normaliser come together
        ops.policy_loss_bwd(z, tok, A, None, outs[3], outs[6], dl, given=given)
