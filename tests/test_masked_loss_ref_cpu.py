"""CPU: the masked restatement (tests/masked_loss_ref.py) against the unmasked ones it is built on -- an all-free mask is the unmasked
reference, an all-given mask is zeros, a mixed mask equals the unmasked reference on the gathered rows -- and the library's surface (the
three masked entry points are declared, bound, and refuse a null mask before anything is launched)."""
import os
import re

import numpy as np
import torch

from mage_amd import _lib
from tests import masked_loss_ref as M
from tests import policy_ref as P
from tests import preference_ref as PR
from tests import token_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, K, T, C = 11, 12, 0.8, 0.01
CMIN, CMAX = P.clip_bounds(0.2, 0.3)


def _inputs(seed=3):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((ROWS, K))).astype(np.float32)
    tok = g.integers(0, K, ROWS)
    A = (g.uniform(0.5, 2.0, ROWS) * g.choice([-1.0, 1.0], ROWS)).astype(np.float32)
    sets = [R.admissible_sets(z[r], T, 5, 0.9)[0] for r in range(ROWS)]
    lp = np.array([R.stats_for_set(z[r], int(tok[r]), T, 0, sets[r])["policy_logprob"] for r in range(ROWS)])
    b = (np.where(np.isfinite(lp), lp, 0.0) + g.choice([-0.35, 0.1, 0.35], ROWS)).astype(np.float32)
    return z, tok, A, b, sets


def _masks():
    g = np.random.default_rng(7)
    return {"free": np.zeros(ROWS, bool), "given": np.ones(ROWS, bool), "alternating": np.arange(ROWS) % 2 == 1, "random": g.random(ROWS) < 0.4}


def test_all_free_is_the_unmasked_reference():
    z, tok, A, b, sets = _inputs()
    given = _masks()["free"]
    for bb in (None, b):
        rows_ = M.policy_rows(z, tok, A, bb, T, sets, CMIN, CMAX, C, given)
        plain = [P.row(z[r], int(tok[r]), float(A[r]), None if bb is None else float(bb[r]), T, sets[r], CMIN, CMAX, C) for r in range(ROWS)]
        assert rows_ == plain
        five, share, norm = M.policy_summary(rows_, bb, given)
        assert np.array_equal(five, P.summary([(r, None if bb is None else float(bb[i])) for i, r in enumerate(plain)], bb is not None))
        assert share == 0.0 and norm == np.float32(1) / np.float32(ROWS)
        want = np.stack([P.dlogits_row(z[r], int(tok[r]), float(A[r]), None if bb is None else float(bb[r]), T, sets[r], CMIN, CMAX, C, 0.7 / ROWS)
                         for r in range(ROWS)])
        assert np.array_equal(M.policy_dlogits(z, tok, A, bb, T, sets, CMIN, CMAX, C, 0.7, given), want)


def test_all_given_is_zeros_whatever_the_rows_hold():
    z, tok, A, b, sets = _inputs()
    z[:] = np.nan                                                    # never read
    tok[:] = K + 5
    given = _masks()["given"]
    rows_ = M.policy_rows(z, tok, A, b, T, sets, CMIN, CMAX, C, given)
    out = M.policy_outputs(rows_, given)
    assert all((v == 0).all() and not np.signbit(v).any() for v in out.values())
    five, share, norm = M.policy_summary(rows_, b, given)
    assert (five == 0).all() and share == 1.0 and norm == 0
    assert (M.policy_dlogits(z, tok, A, b, T, sets, CMIN, CMAX, C, 0.7, given) == 0).all()
    dl, bound = M.token_logprob_bwd(torch.from_numpy(z).double(), torch.from_numpy(tok), torch.ones(ROWS, dtype=torch.float64), given)
    assert (dl == 0).all() and (bound == 0).all()


def test_a_mixed_mask_is_the_unmasked_reference_on_the_gathered_rows():
    z, tok, A, b, sets = _inputs()
    for name in ("alternating", "random"):
        given = _masks()[name]
        free = np.flatnonzero(~given)
        assert 0 < len(free) < ROWS
        zz = z.copy()
        zz[given] = np.nan
        rows_ = M.policy_rows(zz, tok, A, b, T, sets, CMIN, CMAX, C, given)
        plain = [(P.row(z[r], int(tok[r]), float(A[r]), float(b[r]), T, sets[r], CMIN, CMAX, C), float(b[r])) for r in free]
        five, share, norm = M.policy_summary(rows_, b, given)
        assert np.array_equal(five, P.summary(plain, True)) and share == given.mean() and norm == np.float32(1) / np.float32(len(free))
        out = M.policy_outputs(rows_, given)
        assert (out["loss"][given] == 0).all() and np.array_equal(out["loss"][free], [r["loss"] for r, _ in plain])
        dl = M.policy_dlogits(zz, tok, A, b, T, sets, CMIN, CMAX, C, 0.7, given)
        want = np.stack([P.dlogits_row(z[r], int(tok[r]), float(A[r]), float(b[r]), T, sets[r], CMIN, CMAX, C, 0.7 / len(free)) for r in free])
        assert (dl[given] == 0).all() and np.array_equal(dl[free], want)
        # the weighted log-softmax gradient: the unmasked restatement on the free rows
        c = torch.linspace(-1.0, 1.0, ROWS, dtype=torch.float64)
        zt, tt = torch.from_numpy(z).double(), torch.from_numpy(tok)
        got, bound = M.token_logprob_bwd(torch.from_numpy(zz).double(), tt, c, given)
        w, wb = PR.token_logprob_bwd(zt[free], tt[free], c[free])
        assert torch.equal(got[free], w) and torch.equal(bound[free], wb) and (got[given] == 0).all()
        full, _ = PR.token_logprob_bwd(zt, tt, c)
        assert torch.equal(got[free], full[free])                     # a row's gradient depends on the row alone
    lp = np.arange(12.0).reshape(2, 6)
    assert np.array_equal(M.clip_logprobs(lp, np.zeros((2, 6), bool)), lp.sum(1))
    assert np.array_equal(M.clip_logprobs(lp, np.ones((2, 6), bool)), [0.0, 0.0])


# ------------------------------------------------------------------------------------------------ the library's surface
NEW = ("mage_policy_loss_masked", "mage_policy_loss_masked_bwd", "mage_token_logprob_bwd_masked")
PTR = 4096                  # a fake, 16-byte aligned device address: every call below is refused before anything is launched


def test_header_and_table_name_the_masked_entry_points():
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
    # the masked pair is the anchored pair plus (norm, given); the masked log-softmax gradient is the unmasked one plus given
    n = lambda k: len(_lib.EXT_SIGNATURES[k][1])      # noqa: E731
    assert n("mage_policy_loss_masked") == n("mage_policy_loss_anchored") + 2
    assert n("mage_policy_loss_masked_bwd") == n("mage_policy_loss_anchored_bwd") + 2
    assert n("mage_token_logprob_bwd_masked") == n("mage_token_logprob_bwd") + 1


def _fwd(lib, *, given=PTR, norm=PTR, ref=PTR, kl=PTR, kl_coef=0.1):
    return lib.mage_policy_loss_masked(PTR, 8, 16, 16, PTR, PTR, 1, None, ref, 1.0, 0, 1.0, 0.2, 0.2, 0.0, kl_coef, PTR, PTR, PTR, PTR, kl, PTR,
                                       norm, given, None)


def _bwd(lib, *, given=PTR, norm=PTR, ref=PTR, kl_coef=0.1):
    return lib.mage_policy_loss_masked_bwd(PTR, 8, 16, 16, PTR, PTR, 1, None, ref, PTR, 1.0, 0.2, 0.2, 0.0, kl_coef, PTR, norm, PTR, 0, given, None)


def test_refusals_before_any_launch():
    lib = _lib.load()
    EINVAL = -1
    assert _fwd(lib, given=None) == EINVAL and b"given" in lib.mage_last_error()
    assert _fwd(lib, norm=None) == EINVAL and b"norm" in lib.mage_last_error()
    assert _fwd(lib, kl=None) == EINVAL and b"together" in lib.mage_last_error()                  # a reference without kl
    assert _fwd(lib, ref=None) == EINVAL and b"together" in lib.mage_last_error()                 # kl without a reference
    assert _fwd(lib, ref=None, kl=None, kl_coef=0.1) == EINVAL and b"kl_coef" in lib.mage_last_error()
    assert _fwd(lib, ref=None, kl=None, kl_coef=0.0, norm=PTR + 2) == EINVAL
    assert _bwd(lib, given=None) == EINVAL and b"given" in lib.mage_last_error()
    assert _bwd(lib, norm=None) == EINVAL and b"norm" in lib.mage_last_error()
    assert _bwd(lib, ref=None, kl_coef=0.1) == EINVAL and b"kl_coef" in lib.mage_last_error()
    assert lib.mage_token_logprob_bwd_masked(PTR, 8, 16, 16, PTR, PTR, 1, PTR, PTR, 0, None, None) == EINVAL
    assert b"given" in lib.mage_last_error()
    # the plain pair's size rules hold behind the mask's own
    assert lib.mage_token_logprob_bwd_masked(PTR, 8, 15, 16, PTR, PTR, 1, PTR, PTR, 0, PTR, None) == EINVAL
    assert b"mage_token_logprob_bwd_masked" in lib.mage_last_error()
