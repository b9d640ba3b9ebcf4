"""GPU: mage_code_stats and mage_codebook_ema against the fp64 restatement (tests/codebook_ema_ref.py) at the edges of their geometry: rows
below one 8-row group, a ragged group, across one and two chunk boundaries; the smallest and the two largest table sizes (64- and 32-channel
slices); channel counts below, at and across a slice, with and without a row stride; uniform ids, every row in one code, half the codes
unused, each with ids outside [0, K) mixed in.  Counts exact, sums inside the derived bound, two launches and permuted foreign rows the
same bits, the update within one fp32 ulp of the rule, restarts bit for bit -- the restart cases made by construction."""
import math

import numpy as np
import pytest
import torch

from mage_amd import ops
from tests import codebook_ema_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 7, 67, 4097, 8195)
KS = (4, 512, 1024)
DS = (4, 32, 96, 256)
PATTERNS = ("uniform", "one_code", "half_unused")
U = 2.0 ** -24


def make_ids(pattern, rows, K, g):
    if pattern == "uniform":
        ids = g.integers(0, K, rows)
    elif pattern == "one_code":
        ids = np.full(rows, K - 1)
    else:
        ids = 2 * g.integers(0, K // 2, rows)                        # the odd codes are never used
    ids = ids.astype(np.int64)
    n_bad = min(3, rows // 3)                                        # a few ids outside [0, K): counted nowhere, reported once
    if n_bad:
        where = g.choice(rows, n_bad, replace=False)
        ids[where] = np.array([-1, K, K + 12345])[:n_bad]
    return ids, n_bad


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy()


def expect_one_device_error(n_bad):
    if n_bad:
        with pytest.raises(ValueError, match="mage_code_stats: code id out of range"):
            ops.check_device_errors(DEV)
    ops.check_device_errors(DEV)                                     # reported once; clean otherwise


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_code_stats(rows, K, D):
    g = np.random.default_rng(1000 * rows + 10 * K + D)
    worst = 0.0
    for pattern in PATTERNS:
        ids, n_bad = make_ids(pattern, rows, K, g)
        zp = g.standard_normal((rows, D + 4)).astype(np.float32)
        zp[:, D:] = 1e30                                             # beyond the D columns: never read
        counts_w, sums_w, mag = R.code_stats(ids, zp[:, :D], K)
        bound = (counts_w[:, None] + R.n_chunks(rows)) * U * mag
        ids_d, zp_d = torch.from_numpy(ids).to(DEV), torch.from_numpy(zp).to(DEV)
        got = {}
        for ldz, z_d in ((D, torch.from_numpy(zp[:, :D].copy()).to(DEV)), (D + 4, zp_d[:, :D])):
            assert z_d.stride(0) == ldz
            counts, sums = ops.code_stats(ids_d, z_d, K=K)
            expect_one_device_error(n_bad)
            assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), counts_w), (pattern, ldz)
            err = np.abs(sums.cpu().numpy().astype(np.float64) - sums_w)
            assert (err <= bound).all(), (pattern, ldz, float((err - bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            counts2, sums2 = ops.code_stats(ids_d, z_d, K=K)         # two launches: the same bits
            expect_one_device_error(n_bad)
            assert np.array_equal(bits(sums2), bits(sums)) and torch.equal(counts2, counts)
            got[ldz] = sums
        assert np.array_equal(bits(got[D]), bits(got[D + 4]))        # the row stride changes no bit
        # counts-only form
        c_only, none = ops.code_stats(ids_d, K=K)
        expect_one_device_error(n_bad)
        assert none is None and np.array_equal(c_only.cpu().numpy(), counts_w)
        # the rows of one code give the same bits when the other codes' rows are permuted among themselves
        k = int(np.argmax(counts_w))
        other = np.flatnonzero(ids != k)
        if other.size > 1:
            perm = np.arange(rows)
            perm[other] = g.permutation(other)
            ids_p, z_p = torch.from_numpy(ids[perm]).to(DEV), torch.from_numpy(np.ascontiguousarray(zp[perm, :D])).to(DEV)
            _, sums_p = ops.code_stats(ids_p, z_p, K=K)
            expect_one_device_error(n_bad)
            assert np.array_equal(bits(sums_p[k]), bits(got[D][k])), pattern
    print(f"code_stats rows={rows} K={K} D={D}: largest share of the bound used {worst:.3f}")


def test_code_stats_every_id_invalid():
    ids = torch.tensor([-5, 700, 512, 1 << 40, -1], device=DEV)
    z = torch.ones(5, 32, device=DEV)
    counts, sums = ops.code_stats(ids, z, K=512)
    expect_one_device_error(1)
    assert int(counts.sum()) == 0 and float(sums.abs().sum()) == 0.0


def _ema_case(K, D, rows, seed):
    """Ids that leave chosen codes unused, and cluster sizes on both sides of restart_below = 1 for used and unused codes alike."""
    g = np.random.default_rng(seed)
    unused = np.arange(K)[1::2] if K > 4 else np.array([1, 3])       # the odd codes get no row
    ids = (2 * g.integers(0, K // 2, rows)).astype(np.int64)
    if rows >= 7:
        ids[[0, rows // 2]] = [K, -1]                                # and two ids outside the table
    N = np.full(K, 2.0, np.float32)                                  # the even codes: 0.9 * 2 >= 1 with or without rows
    N[unused[0::2]] = 0.5                                            # unused, 0.9 * 0.5 < 1: dead
    N[unused[1::2]] = 40.0                                           # unused, 0.9 * 40 >= 1: stays
    N[0] = 1e-3                                                      # used by few or many rows: dead only if its rows do not lift it
    e = g.standard_normal((K, D)).astype(np.float32)
    m = (e * N[:, None]).astype(np.float32)
    z = g.standard_normal((rows, D + 4)).astype(np.float32)
    return ids, N, e, m, z, unused


@pytest.mark.parametrize("restart_below", [1.0, 0.0])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("K", KS)
def test_codebook_ema(K, D, restart_below):
    rows = 67 if D != 96 else 4097
    ids, N, e, m, z, unused = _ema_case(K, D, rows, seed=K + D)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    ids_d, z_d = t(ids), t(z)[:, :D]                                  # ldz = D + 4
    counts, sums = ops.code_stats(ids_d, z_d, K=K)
    expect_one_device_error(2)
    cb, cs, es = t(e), t(N), t(m)
    kw = dict(decay=0.9, eps=1e-5, restart_below=restart_below, restart_size=2.5, seed=11, step=3)
    stats = ops.codebook_ema(cb, cs, es, counts, sums, z_d, **kw)
    want = R.ema_update(e, N, m, counts.cpu().numpy(), sums.cpu().numpy(), z, **kw)      # fed the kernel's own sums
    dead = want["restarted"]
    if restart_below > 0:                                             # the constructed cases are all there
        assert dead[unused[0::2]].all() and not dead[unused[1::2]].any() and not dead[2::2].any()
        assert dead[0] == bool(0.9 * 1e-3 + 0.1 * int(counts[0]) < 1.0)
    else:
        assert not dead.any()
    got = dict(codebook=cb.cpu().numpy(), cluster_size=cs.cpu().numpy(), embed_sum=es.cpu().numpy())
    for name in ("cluster_size", "embed_sum", "codebook"):
        d = R.ulps(got[name], want[name])
        assert d.max() <= 1, (name, int(d.max()), np.argwhere(d > 1)[:4])
    for k in np.flatnonzero(dead):                                    # restarted codes: bit for bit
        r = want["rows"][k]
        assert np.array_equal(got["codebook"][k].view(np.int32), z[r, :D].view(np.int32))
        assert got["cluster_size"][k] == np.float32(2.5)
        assert np.array_equal(got["embed_sum"][k], (np.float64(2.5) * z[r, :D].astype(np.float64)).astype(np.float32))
    s = stats.cpu().numpy()
    ppl, active, restarted, total = want["stats"]
    assert abs(s[0] - ppl) <= 1e-12 * ppl and (s[1], s[2], s[3]) == (active, restarted, total) and total == rows - 2
    # the same call again from the same state: the same bits (no order in the update)
    cb2, cs2, es2 = t(e), t(N), t(m)
    stats2 = ops.codebook_ema(cb2, cs2, es2, counts, sums, z_d, **kw)
    assert torch.equal(cb2, cb) and torch.equal(cs2, cs) and torch.equal(es2, es) and np.array_equal(bits(stats2), bits(stats))
    # another step draws other rows for the dead codes
    if restart_below > 0 and rows > 1:
        cb3, cs3, es3 = t(e), t(N), t(m)
        ops.codebook_ema(cb3, cs3, es3, counts, sums, z_d, **{**kw, "step": 4})
        want3 = R.ema_update(e, N, m, counts.cpu().numpy(), sums.cpu().numpy(), z, **{**kw, "step": 4})
        assert (want3["rows"][dead] != want["rows"][dead]).any()
        for k in np.flatnonzero(dead):
            assert np.array_equal(cb3[k].cpu().numpy(), z[want3["rows"][k], :D])


def test_codebook_ema_with_no_valid_id_leaves_the_state():
    K, D = 512, 32
    g = np.random.default_rng(5)
    e, N = g.standard_normal((K, D)).astype(np.float32), g.random(K).astype(np.float32)
    ids = torch.full((67,), K, device=DEV, dtype=torch.int64)
    z = torch.from_numpy(g.standard_normal((67, D)).astype(np.float32)).to(DEV)
    counts, sums = ops.code_stats(ids, z, K=K)
    expect_one_device_error(1)
    cb, cs, es = (torch.from_numpy(a.copy()).to(DEV) for a in (e, N, 2 * e))
    s = ops.codebook_ema(cb, cs, es, counts, sums, z, decay=0.9, restart_below=10.0, seed=1, step=0).cpu().numpy()
    assert math.isnan(s[0]) and s[1:].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(cb.cpu().numpy(), e) and np.array_equal(cs.cpu().numpy(), N) and np.array_equal(es.cpu().numpy(), 2 * e)
