"""CPU: the EMA codebook update -- the fp64 restatement (tests/codebook_ema_ref.py) against hand-worked cases, the extension table
(include/mage_hip_ext.h <-> _lib.EXT_SIGNATURES <-> the library's symbols) for the two new entry points, their argument checks (refused
before anything is launched) and the model-side switch (set_codebook_update): buffers, requires_grad, state_dict layout, refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import codebook_ema_ref as R
from tests.helpers import build_vqvae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
F = np.float32


# ---------------------------------------------------------------- the restatement by hand
def test_hash_and_row_pick():
    assert R.hash32(0) == 0                                          # the finaliser's fixed point
    v = 1
    v ^= v >> 33
    v = (v * 0xff51afd7ed558ccd) % 2 ** 64
    v ^= v >> 33
    v = (v * 0xc4ceb9fe1a85ec53) % 2 ** 64
    v ^= v >> 33
    assert R.hash32(1) == v % 2 ** 32
    assert R.hash32(2 ** 64 + 5) == R.hash32(5)                      # uint64 wrap-around
    for rows in (1, 7, 4097):
        picks = [R.restart_row(3, s, 512, k, rows) for s in range(4) for k in range(512)]
        assert min(picks) >= 0 and max(picks) < rows
    assert R.restart_row(3, 0, 512, 9, 1000) == (R.hash32((3 * R.SEED_MUL + 9) % 2 ** 64) * 1000) >> 32
    assert R.restart_row(3, 1, 512, 9, 1000) == R.restart_row(3, 0, 512, 521, 1000)     # the counter is step * K + k
    assert len({R.restart_row(0, s, 8, 2, 10 ** 6) for s in range(16)}) > 8           # a dead code draws again at the next step


def test_one_row():
    z = np.array([[1.0, -2.0, 0.5, 4.0]], F)
    counts, sums, mag = R.code_stats([1], z, 2)
    assert counts.tolist() == [0, 1] and np.array_equal(sums, [[0, 0, 0, 0], [1, -2, 0.5, 4]]) and np.array_equal(mag[1], [1, 2, 0.5, 4])
    e = np.array([[1, 1, 1, 1], [2, 2, 2, 2]], F)
    out = R.ema_update(e, np.ones(2, F), e.copy(), counts, sums.astype(F), decay=0.5, eps=1e-5)
    assert np.array_equal(out["cluster_size"], [0.5, 1.0])           # 0.5 * 1 + 0.5 * {0, 1}
    assert np.array_equal(out["embed_sum"], [[0.5] * 4, [1.5, 0.0, 1.25, 3.0]])
    n, eps = 1.5, float(F(1e-5))
    nhat = [(0.5 + eps) / (n + 2 * eps) * n, (1.0 + eps) / (n + 2 * eps) * n]
    want = np.array([[0.5 / nhat[0]] * 4, [v / nhat[1] for v in (1.5, 0.0, 1.25, 3.0)]]).astype(F)
    assert np.array_equal(out["codebook"], want) and not out["restarted"].any()
    assert out["stats"] == (1.0, 1, 0, 1)                            # one code used: perplexity exp(0)


def test_all_rows_in_one_code_and_a_zero_count_code():
    g = np.random.default_rng(0)
    z = g.standard_normal((40, 8)).astype(F)
    counts, sums, _ = R.code_stats(np.full(40, 2), z, 4)
    assert counts.tolist() == [0, 0, 40, 0] and np.allclose(sums[2], z.astype(np.float64).sum(0), rtol=0, atol=1e-12) and not sums[[0, 1, 3]].any()
    e = g.standard_normal((4, 8)).astype(F)
    out = R.ema_update(e, np.ones(4, F), e.copy(), counts, sums.astype(F), decay=0.9, eps=1e-5)
    ppl, active, restarted, total = out["stats"]
    assert (ppl, active, restarted, total) == (1.0, 1, 0, 40)
    N = out["cluster_size"].astype(np.float64)
    g9 = np.float64(F(0.9))                                          # the kernel's g: the fp32 decay, widened
    assert np.array_equal(out["cluster_size"], np.array([g9, g9, g9 + (1 - g9) * 40, g9]).astype(F))
    # Laplace smoothing keeps the total: sum Nhat = n
    n = N.sum()
    nhat = (N + 1e-5) / (n + 4e-5) * n
    assert abs(nhat.sum() - n) < 1e-9
    # a zero-count code: m' = g m, N' = g N, so e moves only by the smoothing (Nhat_k / N_k' - 1 ~ eps-sized and n-sized)
    assert np.allclose(out["codebook"][0], F(0.9) * e[0].astype(np.float64) / nhat[0], rtol=1e-6)


def test_every_id_invalid_leaves_the_state():
    z = np.ones((5, 4), F)
    counts, sums, _ = R.code_stats([-1, 9, 4, 100, -7], z, 4)
    assert not counts.any() and not sums.any()
    e = np.arange(16, dtype=F).reshape(4, 4)
    out = R.ema_update(e, np.full(4, 3, F), 2 * e, counts, sums.astype(F), z, decay=0.9, eps=1e-5, restart_below=10.0)
    assert np.array_equal(out["codebook"], e) and np.array_equal(out["cluster_size"], np.full(4, 3, F)) and np.array_equal(out["embed_sum"], 2 * e)
    assert math.isnan(out["stats"][0]) and out["stats"][1:] == (0, 0, 0)
    assert math.isnan(R.usage(np.zeros(3, np.int64))[0])


def test_ones_and_copy_initialisation_keeps_an_unused_code():
    """N = 1, m = e at the start: an unused code's m / N stays e under the update, exactly in m' / N' and up to the smoothing in e'.  (A
    zero-initialised N divides an unused code's m by about eps at the first step and throws it far away.)"""
    g = np.random.default_rng(1)
    e = g.standard_normal((8, 4)).astype(F)
    z = g.standard_normal((64, 4)).astype(F)
    ids = g.integers(0, 4, 64)                                      # codes 4 .. 7 unused
    counts, sums, _ = R.code_stats(ids, z, 8)
    out = R.ema_update(e, np.ones(8, F), e.copy(), counts, sums.astype(F), decay=0.99, eps=1e-5)
    ratio = out["embed_sum"][4:].astype(np.float64) / out["cluster_size"][4:, None].astype(np.float64)
    assert np.abs(ratio - e[4:]).max() < 2e-7 * np.abs(e[4:]).max()
    assert np.abs(out["codebook"][4:] - e[4:]).max() < 1e-4 * np.abs(e[4:]).max()
    zero = R.ema_update(e, np.zeros(8, F), np.zeros_like(e), counts, sums.astype(F), decay=0.99, eps=1e-5)
    assert np.abs(zero["codebook"][4:]).max() == 0.0                # what the zero start does to the same codes: gone


def test_restart_by_construction():
    g = np.random.default_rng(2)
    e = g.standard_normal((6, 4)).astype(F)
    z = g.standard_normal((30, 8)).astype(F)                        # ldz 8 > D 4: the first D columns are the row
    ids = g.integers(0, 3, 30)                                      # codes 3, 4, 5 unused
    N = np.array([1, 1, 1, 0.5, 4.0, 0.9], F)                       # after decay 0.5: 3 -> 0.25 (dead), 4 -> 2.0 (alive), 5 -> 0.45 (dead)
    counts, sums, _ = R.code_stats(ids, z[:, :4], 6)
    out = R.ema_update(e, N, e.copy(), counts, sums.astype(F), z, decay=0.5, eps=1e-5, restart_below=1.0, restart_size=2.0, seed=7, step=11)
    assert out["restarted"].tolist() == [False, False, False, True, False, True] and out["stats"][2] == 2
    for k in (3, 5):
        r = R.restart_row(7, 11, 6, k, 30)
        assert out["rows"][k] == r and np.array_equal(out["codebook"][k], z[r, :4]) and out["cluster_size"][k] == 2.0
        assert np.array_equal(out["embed_sum"][k], (2.0 * z[r, :4].astype(np.float64)).astype(F))
    assert out["cluster_size"][4] == 2.0 and out["rows"][4] == -1
    none = R.ema_update(e, N, e.copy(), counts, sums.astype(F), z, decay=0.5, eps=1e-5, restart_below=0.0)
    assert not none["restarted"].any() and np.array_equal(none["cluster_size"][[3, 5]], np.array([0.25, 0.45], F))


def test_usage_statistics():
    ppl, active, total = R.usage([5, 5, 0, 10])
    h = -(0.25 * math.log(0.25) * 2 + 0.5 * math.log(0.5))
    assert abs(ppl - math.exp(h)) < 1e-12 and (active, total) == (3, 20)
    assert abs(R.usage(np.full(512, 3))[0] - 512.0) < 1e-9           # uniform use: perplexity K
    assert R.n_chunks(1) == 1 and R.n_chunks(4096) == 1 and R.n_chunks(4097) == 2 and R.n_chunks(8195) == 3 and R.n_chunks(10 ** 7) == 64
    assert all(ops.code_stats_chunks(r) == R.n_chunks(r) for r in (1, 7, 67, 4096, 4097, 8192, 8195, 262144, 262145, 10 ** 7))
    assert R.ulps(F(1.0), np.nextafter(F(1.0), F(2.0))) == 1 and R.ulps(F(-0.0), F(0.0)) == 0 and R.ulps(F(NAN), F(NAN)) == 0


# ---------------------------------------------------------------- the extension table
NEW = ("mage_code_stats", "mage_codebook_ema")


def test_extension_table_matches_its_header_and_the_library():
    header = open(os.path.join(ROOT, "include", "mage_hip_ext.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mage_\w+)\s*\(", header, flags=re.M))
    assert set(NEW) <= declared and declared == set(_lib.EXT_SIGNATURES)
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == 69 and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.mage_abi_version() == 10
    for name in NEW:
        res, args = _lib.EXT_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(args)
    assert len(_lib.EXT_SIGNATURES["mage_code_stats"][1]) == 11 and len(_lib.EXT_SIGNATURES["mage_codebook_ema"][1]) == 18
    assert {"code_stats", "codebook_ema"} <= set(ops.__all__)
    src = open(os.path.join(ROOT, "mage_amd", "csrc", "Makefile")).read()
    assert "codebook.hip" in re.search(r"^SRCS = (.*)$", src, flags=re.M).group(1).split()


# ---------------------------------------------------------------- argument rules (refused before anything is launched)
P = 4096                    # a fake, 16-byte aligned device address
CS_ORDER = ("ids", "z", "rows", "D", "ldz", "K", "counts", "sums", "scratch", "scratch_bytes")
CS_GOOD = dict(ids=P, z=P, rows=8195, D=32, ldz=36, K=512, counts=P, sums=P, scratch=P, scratch_bytes=3 * 512 * 33 * 4)


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-3), dict(rows=2 ** 31), dict(K=0), dict(K=1025), dict(K=-1), dict(D=30), dict(D=0), dict(D=1028, ldz=1028),
    dict(ldz=31), dict(ldz=0), dict(ids=None), dict(counts=None), dict(scratch=None), dict(z=None), dict(sums=None), dict(ids=P + 4),
    dict(counts=P + 4), dict(z=P + 2), dict(sums=P + 8), dict(scratch=P + 8), dict(scratch_bytes=3 * 512 * 33 * 4 - 1), dict(scratch_bytes=0),
    dict(z=None, sums=None, scratch_bytes=3 * 512 * 4 - 1),
])
def test_code_stats_refuses_bad_arguments(bad):
    a = {**CS_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_code_stats(*[a[k] for k in CS_ORDER], None)
    msg = lib.mage_last_error().decode()
    assert rc == -1 and "mage_code_stats" in msg and "mage_init" not in msg, (bad, rc, msg)


def test_code_stats_accepts_what_the_rule_allows():
    """The accepted forms get past the argument rules: without an initialised device they stop at the mage_init check behind them."""
    lib = _lib.load()
    for ok in (dict(), dict(z=None, sums=None, scratch_bytes=3 * 512 * 4), dict(z=None, sums=None, D=7, ldz=0, scratch_bytes=3 * 512 * 4),
               dict(K=1024, scratch_bytes=3 * 1024 * 33 * 4), dict(D=1024, ldz=1024, K=4, rows=1, scratch_bytes=4 * 1025 * 4), dict(ldz=32),
               dict(rows=2 ** 31 - 1, K=1, D=4, ldz=4, scratch_bytes=64 * 5 * 4), dict(z=P + 4)):
        a = {**CS_GOOD, **ok}
        rc = lib.mage_code_stats(*[a[k] for k in CS_ORDER], None)
        assert rc == -1 and "mage_init" in lib.mage_last_error().decode(), (ok, rc, lib.mage_last_error())


EMA_ORDER = ("codebook", "cluster_size", "embed_sum", "counts", "sums", "z", "rows", "ldz", "K", "D", "decay", "eps", "restart_below",
             "restart_size", "seed", "step", "stats")
EMA_GOOD = dict(codebook=P, cluster_size=P, embed_sum=P, counts=P, sums=P, z=P, rows=4096, ldz=256, K=512, D=256, decay=0.99, eps=1e-5,
                restart_below=1.0, restart_size=1.0, seed=3, step=5, stats=P)


@pytest.mark.parametrize("bad", [
    dict(decay=1.0), dict(decay=-0.1), dict(decay=NAN), dict(decay=INF), dict(eps=0.0), dict(eps=-1e-5), dict(eps=NAN), dict(eps=INF),
    dict(restart_below=-1.0), dict(restart_below=NAN), dict(restart_below=INF), dict(restart_size=0.0), dict(restart_size=-1.0),
    dict(restart_size=NAN), dict(restart_size=INF), dict(restart_below=0.0, restart_size=0.0), dict(K=0), dict(K=1025), dict(D=0), dict(D=254),
    dict(D=1028), dict(ldz=252), dict(rows=0), dict(rows=2 ** 31), dict(z=None), dict(codebook=None), dict(cluster_size=None),
    dict(embed_sum=None), dict(counts=None), dict(sums=None), dict(stats=None), dict(codebook=P + 4), dict(embed_sum=P + 8), dict(sums=P + 4),
    dict(counts=P + 4), dict(stats=P + 4), dict(cluster_size=P + 2), dict(z=P + 1),
])
def test_codebook_ema_refuses_bad_arguments(bad):
    a = {**EMA_GOOD, **bad}
    lib = _lib.load()
    rc = lib.mage_codebook_ema(*[a[k] for k in EMA_ORDER], None)
    msg = lib.mage_last_error().decode()
    assert rc == -1 and "mage_codebook_ema" in msg and "mage_init" not in msg, (bad, rc, msg)


def test_codebook_ema_accepts_what_the_rule_allows():
    lib = _lib.load()
    for ok in (dict(), dict(decay=0.0), dict(restart_below=0.0, z=None, rows=0, ldz=0), dict(restart_size=7.5), dict(K=1024, D=1024, ldz=1024),
               dict(K=1, D=4, ldz=4), dict(ldz=260, z=P + 4), dict(seed=2 ** 64 - 1, step=2 ** 40), dict(cluster_size=P + 4)):
        a = {**EMA_GOOD, **ok}
        rc = lib.mage_codebook_ema(*[a[k] for k in EMA_ORDER], None)
        assert rc == -1 and "mage_init" in lib.mage_last_error().decode(), (ok, rc, lib.mage_last_error())


# ---------------------------------------------------------------- the model-side switch
BASE_KEYS = None


def _small(down_ratio=4):
    return build_vqvae(1 if down_ratio == 4 else 3, down_ratio, 32, 64, 5)


@pytest.mark.parametrize("down_ratio", [4, 8])
def test_switch_registers_and_removes_the_ema_state(down_ratio):
    m = _small(down_ratio)
    w = m.codebook.embedding.weight
    keys = list(m.state_dict())
    assert m.codebook_update == "grad" and w.requires_grad and not any("ema_" in k for k in keys) and m.last_codebook_stats is None
    assert m.set_codebook_update("ema", decay=0.9, restart_below=0.5) is m
    sd = m.state_dict()
    assert m.codebook_update == "ema" and not w.requires_grad
    assert [k for k in sd if k not in keys] == ["codebook.ema_cluster_size", "codebook.ema_embed_sum", "codebook.ema_step"]
    assert torch.equal(sd["codebook.ema_cluster_size"], torch.ones(64)) and torch.equal(sd["codebook.ema_embed_sum"], w.detach())
    assert sd["codebook.ema_embed_sum"].data_ptr() != w.data_ptr() and sd["codebook.ema_step"].dtype == torch.int64 and int(sd["codebook.ema_step"]) == 0
    assert m._ema["restart_size"] == 0.5                             # restart_size=None means restart_below
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["codebook.embedding.weight"]
    m.codebook.ema_cluster_size.fill_(3.0)
    m.set_codebook_update("ema", decay=0.5)                          # again: new settings, the state stays
    assert m._ema["decay"] == 0.5 and float(m.codebook.ema_cluster_size[0]) == 3.0
    m.set_codebook_update("grad")
    assert list(m.state_dict()) == keys and w.requires_grad and m.codebook_update == "grad" and m._ema is None
    m.set_codebook_update("grad")                                    # idempotent
    assert list(m.state_dict()) == keys
    w.requires_grad_(False)                                          # a codebook the caller froze stays frozen through the round trip
    m.set_codebook_update("ema").set_codebook_update("grad")
    assert not w.requires_grad


def test_switch_validates():
    m = _small()
    for kw in (dict(decay=1.0), dict(decay=-0.5), dict(decay=NAN), dict(eps=0.0), dict(eps=INF), dict(restart_below=-1.0), dict(restart_below=NAN),
               dict(restart_below=1.0, restart_size=0.0), dict(restart_below=1.0, restart_size=INF)):
        with pytest.raises(ValueError, match="set_codebook_update"):
            m.set_codebook_update("ema", **kw)
        assert m.codebook_update == "grad" and "codebook.ema_step" not in m.state_dict()        # a refused call changes nothing
    with pytest.raises(ValueError, match="'grad' or 'ema'"):
        m.set_codebook_update("kmeans")
    with pytest.raises(TypeError):
        m.set_codebook_update("ema", 0.9)                            # the settings are keyword-only


def test_checkpoint_load_order():
    src = _small().set_codebook_update("ema")
    src.codebook.ema_step.fill_(17)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    plain = _small()
    with pytest.raises(RuntimeError, match=r"set_codebook_update\('ema'"):
        plain.load_state_dict(sd)
    res = _small().load_state_dict(sd, strict=False)                 # inference on an EMA-trained checkpoint: the EMA state is dropped
    assert sorted(res.unexpected_keys) == ["codebook.ema_cluster_size", "codebook.ema_embed_sum", "codebook.ema_step"] and not res.missing_keys
    dst = _small().set_codebook_update("ema")
    dst.load_state_dict(sd)
    assert int(dst.codebook.ema_step) == 17
    with pytest.raises(RuntimeError, match="Missing key"):           # the other way round: torch's own message names the keys
        _small().set_codebook_update("ema").load_state_dict(_small().state_dict())


def test_ema_mode_refuses_more_than_one_process(monkeypatch):
    import torch.distributed as dist
    m = _small()
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="all-reduced form is out of scope"):
        m.set_codebook_update("ema")
    assert m.codebook_update == "grad" and "codebook.ema_step" not in m.state_dict()
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    assert m.set_codebook_update("ema").codebook_update == "ema"      # one process under torch.distributed is fine


def test_ops_raise_on_cpu_tensors():
    ids = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.code_stats(ids, K=4)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.codebook_ema(torch.zeros(4, 4), torch.ones(4), torch.zeros(4, 4), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        _small().code_usage(ids)
