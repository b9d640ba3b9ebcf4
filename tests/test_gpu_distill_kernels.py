"""GPU: mage_distill_loss / mage_distill_loss_bwd (include/mage_hip_ext.h) against the fp64 restatement (tests/distill_ref.py) on the same
fp32 inputs, and their bitwise promises.

Inputs: tests/test_gpu_policy_loss.py's `_logits` recipe for both buffers under different seeds; the teacher's rows are rotated by three so
that its special rows (+-80, -inf entries, a NaN, all -inf, uniform, +-100) meet ordinary student rows and the student's meet ordinary
teacher rows: a student that excludes codes the teacher holds (forward KL +inf, reverse finite), the converse, NaN on either side.  The row
strides of the two buffers exceed K and differ; the padding holds NaN (it is never read).

Bounds (tests/distill_ref.py derives them from the kernel's operation count; TOL is token_stats_ref's allowance for one fixed-order sum):
  row_kl      |d| <= distill_ref.row's bound; +inf and NaN rows must be +inf and NaN.
  dlogits     |d| <= distill_ref.dlogits_row's bound per element (2^-8 |want| more for the one bf16 store rounding, floor 2^-126); the rows
              without a finite row_kl and the given rows are +0 by bits.
  summary[0]  the fp64 mean of the kernel's own row_kl over the free rows, one fp32 rounding: 2^-24 relative.
  summary[1], [2]  the fp64 means of the restatement's entropies; per row tests/test_gpu_token_stats.py's entropy bound
              1e-5 + 2^-23 |H| + 90 * 2^-24 (H - log Z), averaged, plus the mean's one rounding.
  summary[3]  the share of rows on which mage_argmax picks the same code in both buffers, one rounding.  summary[4] and norm: exact.
  one-hot teacher  row_kl = -mage_token_logprob of that code, 2 ulp at the larger of |l| and |lse| (the cross-entropy comparison of
              tests/test_gpu_policy_loss.py: both form l from the same fp32 log Z in a different order).
The largest error / bound per quantity is printed per K."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import distill_ref as D
from tests import helpers as H
from tests import sampling_ref as S
from tests.test_gpu_masked_policy_kernels import _masks
from tests.test_gpu_policy_loss import _logits, _ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = [4, 256, 260, 512, 1028, 4096]                                   # every ladder instance; 260 and 1028: a partial last chunk
TEMPS = (0.7, 1.0, 2.0)
GOUT = 0.7
E24 = 2.0 ** -24


def _dev(a, pad):
    """The rows of `a` on the device with row stride K + pad, NaN in the padding."""
    rows, K = a.shape
    buf = torch.full((rows, K + pad), float("nan"), device=DEV)
    v = buf[:, :K]
    v.copy_(torch.from_numpy(a))
    assert v.stride(0) == K + pad
    return v


def _pair(rows, K, seed, clean=False):
    """(z, t, zd, td): student and teacher rows (numpy fp32) and their device views, row strides K + 4 and K + 8."""
    skip = 13 if clean else 0                                        # past the special rows: a finite summary
    z = _logits(rows + skip, K, seed)[skip:]
    t = np.roll(_logits(rows + skip, K, seed + 1000)[skip:], 3, axis=0)
    return z, t, _dev(z, 4), _dev(t, 8)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run(zd, td, T, mode, dt, given=None):
    out = ops.distill_loss(zd, td, temperature=T, mode=mode, given=given)
    gout = torch.tensor([GOUT], device=DEV)
    dl = ops.distill_loss_bwd(zd, td, out["row_kl"], out["norm"], gout, torch.empty(zd.shape, device=DEV, dtype=dt), temperature=T, mode=mode,
                              given=given)
    return out, dl


def _close(got, want, rel, what):
    assert np.isnan(got) == np.isnan(want), (what, got, want)
    if np.isfinite(want):
        assert abs(got - want) <= rel * abs(want) * (1 + 1e-6), (what, got, want)
    elif not np.isnan(want):
        assert got == want, (what, got, want)


def _check(z, t, zd, td, T, mode, dt, worst, given_np=None):
    """Every check of the module docstring on one launch."""
    rows, K = z.shape
    given = None if given_np is None else torch.from_numpy(given_np).to(DEV)
    out, dl = _run(zd, td, T, mode, dt, given)
    out2, dl2 = _run(zd, td, T, mode, dt, given)
    for n in out:                                                    # deterministic: two launches, the same bits
        assert torch.equal(_bits(out[n]), _bits(out2[n])), n
    assert torch.equal(_bits(dl), _bits(dl2))
    ref = D.loss(z, t, T, mode, given_np)
    free = np.ones(rows, bool) if given_np is None else ~given_np
    n_free = int(free.sum())
    kl = out["row_kl"].cpu().numpy().astype(np.float64)
    want = ref["row_kl"]
    assert np.array_equal(np.isnan(kl), np.isnan(want)) and np.array_equal(np.isposinf(kl), np.isposinf(want)) and not np.isneginf(kl).any()
    fin = np.isfinite(want) & free
    err = np.abs(kl[fin] - want[fin]) / ref["bound"][fin]
    assert (err <= 1).all(), f"row_kl: row {np.flatnonzero(fin)[err.argmax()]} |d| / bound {err.max():.3f}"
    worst["row_kl"] = max(worst.get("row_kl", 0.0), float(err.max()) if err.size else 0.0)
    assert (out["row_kl"].view(torch.int32).cpu().numpy()[~free] == 0).all()
    # norm, the given share, the means
    norm, s = out["norm"].cpu().numpy(), out["summary"].cpu().numpy()
    want_norm = np.float32(1) / np.float32(n_free) if n_free else np.float32(0)
    assert norm.view(np.uint32)[0] == np.array([want_norm], np.float32).view(np.uint32)[0]
    assert s.shape == (5,) and s[4] == np.float32((rows - n_free) / rows)
    if n_free:
        with np.errstate(invalid="ignore"):
            _close(s[0], kl[free].sum() / n_free, E24, "summary[0]")
        sides = [(D._side(D.scaled(t[i], T)), D._side(D.scaled(z[i], T))) for i in np.flatnonzero(free)]
        for q in (0, 1):
            h = np.array([x[q]["H"] for x in sides])
            hb = np.array([1e-5 + 2 * E24 * abs(x[q]["H"]) + 90 * E24 * (x[q]["H"] - x[q]["lz"]) for x in sides])
            assert np.isnan(s[1 + q]) == np.isnan(h.sum())
            if np.isfinite(h.sum()):
                assert abs(s[1 + q] - h.mean()) <= hb.mean() + E24 * abs(h.mean()), (q, s[1 + q], h.mean())
                worst["entropy"] = max(worst.get("entropy", 0.0), abs(s[1 + q] - h.mean()) / (hb.mean() + E24 * abs(h.mean())))
        am = [ops.argmax(x, torch.empty(rows, dtype=torch.int64, device=DEV), rows=rows, K=K, ld=x.stride(0)).cpu().numpy() for x in (zd, td)]
        if given_np is None:                                         # (a masked launch's given rows hold NaN: mage_argmax would read them)
            _close(s[3], float((am[0] == am[1])[free].mean()), E24, "summary[3]")
            assert ref["summary"][3] == (am[0] == am[1])[free].mean()
    else:
        assert (out["summary"][:4].view(torch.int32) == 0).all() and s[4] == 1 and norm[0] == 0
    # the gradient
    g = dl.float().cpu().numpy().astype(np.float64)
    gb = _bits(dl).cpu().numpy()
    c = float(np.float32(GOUT)) * float(want_norm) * float(S.inv_temperature(T))
    for i in range(rows):
        if not free[i] or not np.isfinite(want[i]):
            assert (gb[i] == 0).all(), f"row {i}: a given row / a row without a finite KL must be +0"
            continue
        w, b = D.dlogits_row(z[i], t[i], T, mode, c, bf16=dt == torch.bfloat16)
        e = np.abs(g[i] - w) / b
        assert (e <= 1).all(), f"dlogits: row {i} code {e.argmax()} got {g[i][e.argmax()]!r} want {w[e.argmax()]!r} |d| / bound {e.max():.3f}"
        worst["dlogits"] = max(worst.get("dlogits", 0.0), float(e.max()))
    return out, dl


@pytest.mark.parametrize("K", KS)
def test_kernels_match_the_restatement(K):
    worst = {}
    z, t, zd, td = _pair(29, K, seed=K)                              # 7 workgroups of 4 waves and a single wave; holds every special row
    i = 0
    for T in TEMPS:
        for mode in (0, 1):
            dt = (torch.float32, torch.bfloat16)[(i // 2 + i) % 2]
            base, dl = _check(z, t, zd, td, T, mode, dt, worst)
            if i % 3 == 0:                                           # rows = 1 (a lone wave) and 5 (a ragged last workgroup): the same rows' bits
                for n, r0 in ((1, 0), (1, 8), (5, 0), (5, 8)):
                    sub, _ = _check(z[r0:r0 + n], t[r0:r0 + n], zd[r0:r0 + n], td[r0:r0 + n], T, mode, dt, worst)
                    assert torch.equal(_bits(sub["row_kl"]), _bits(base["row_kl"][r0:r0 + n])), (n, r0)
            i += 1
    # several workgroups, no special row: finite means
    zc, tc, zcd, tcd = _pair(131, K, seed=K + 1, clean=True)
    out, _ = _check(zc, tc, zcd, tcd, 0.7, K // 4 % 2, torch.bfloat16, worst)
    assert torch.isfinite(out["summary"]).all() and out["summary"][0] > 0
    print(f"K={K}: largest error / bound: " + ", ".join(f"{a} {b:.3f}" for a, b in worst.items()))


@pytest.mark.parametrize("K", KS)
def test_equal_rows_give_exactly_zero(K):
    z = _logits(29, K, seed=K + 7)
    zd, td = _dev(z, 4), _dev(z, 8)
    nan_rows = np.zeros(29, bool)
    nan_rows[[8, 9]] = True                                          # a NaN; all -inf: NaN against anything, themselves included
    for T in TEMPS:
        for mode in (0, 1):
            for dt in (torch.float32, torch.bfloat16):
                out, dl = _run(zd, td, T, mode, dt)
                bits = out["row_kl"].view(torch.int32).cpu().numpy()
                assert (bits[~nan_rows] == 0).all(), (T, mode, "row_kl of equal rows: +0 by bits")
                assert torch.isnan(out["row_kl"][torch.from_numpy(nan_rows).to(DEV)]).all()
                assert (dl == 0).all(), (T, mode, dt)
    ok = torch.from_numpy(~nan_rows).to(DEV)
    out = ops.distill_loss(zd, td, temperature=0.7, mode=0, given=~ok)
    assert out["summary"][0].item() == 0.0 and out["summary"][3].item() == 1.0 and out["summary"][1].item() == out["summary"][2].item()


@pytest.mark.parametrize("K", KS)
def test_one_hot_teacher_is_the_token_logprob(K):
    rows = 67
    z = _logits(rows + 13, K, seed=K + 3)[13:]
    tok = np.random.default_rng(K).integers(0, K, rows)
    t = np.full((rows, K), -np.inf, np.float32)
    t[np.arange(rows), tok] = np.random.default_rng(K + 1).normal(size=rows).astype(np.float32)
    zd, td = _dev(z, 4), _dev(t, 8)
    out = ops.distill_loss(zd, td, temperature=1.0, mode=0)
    tokd = torch.from_numpy(tok).to(DEV)
    lp = ops.token_logprob(zd, tokd, torch.empty(rows, device=DEV), rows=rows, K=K, ld=zd.stride(0))
    ops.check_device_errors(DEV)
    got, want = out["row_kl"].cpu().numpy().astype(np.float64), -lp.cpu().numpy().astype(np.float64)
    lse = want + z[np.arange(rows), tok].astype(np.float64)
    ulps = np.abs(got - want) / _ulp(np.maximum(np.abs(want), np.abs(lse)))
    print(f"K={K}: row_kl against -mage_token_logprob, largest difference {ulps.max():.2f} ulp")
    assert (ulps <= 2).all()
    assert out["summary"][1].item() == 0.0                           # a one-hot teacher has entropy exactly 0
    # ... and its forward-KL gradient is the cross-entropy's, p - onehot
    dl = ops.distill_loss_bwd(zd, td, out["row_kl"], out["norm"], torch.ones(1, device=DEV), torch.empty(rows, K, device=DEV))
    dce = ops.cross_entropy_bwd(zd.contiguous(), tokd, torch.ones(1, device=DEV), torch.empty(rows, K, device=DEV))
    assert ((dl - dce).abs() <= 2 * D.TOL * dce.abs().max(1, keepdim=True)[0]).all()


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
def test_masks(K):
    rows = 29
    z, t, zd, td = _pair(rows, K, seed=K + 11)
    for i, (T, mode, dt) in enumerate(((0.7, 0, torch.bfloat16), (2.0, 1, torch.float32))):
        U, dU = _run(zd, td, T, mode, dt)
        for name, m in _masks(rows, seed=K + i).items():
            given = torch.from_numpy(m).to(DEV)
            zp, tp = _dev(z, 4), _dev(t, 8)
            zp[given] = float("nan")                                 # the given rows must not be read, in either buffer
            tp[given] = float("nan")
            out, dl = _run(zp, tp, T, mode, dt, given)
            out2, dl2 = _run(zp, tp, T, mode, dt, given)
            assert all(torch.equal(_bits(out[n]), _bits(out2[n])) for n in out) and torch.equal(_bits(dl), _bits(dl2)), name
            assert torch.equal(_bits(out["row_kl"])[~given], _bits(U["row_kl"])[~given]), (name, "free rows: the null-mask call's bits")
            assert (_bits(out["row_kl"])[given] == 0).all() and (_bits(dl)[given] == 0).all(), (name, "given rows: +0")
            n_free = int((~m).sum())
            want_norm = np.float32(1) / np.float32(n_free) if n_free else np.float32(0)
            assert out["norm"].cpu().numpy().view(np.uint32)[0] == np.array([want_norm], np.float32).view(np.uint32)[0]
            s = out["summary"].cpu().numpy()
            assert s[4] == np.float32(m.sum() / rows)
            if n_free:
                idx = torch.from_numpy(np.flatnonzero(~m)).to(DEV)
                zg, tg = _dev(z[~m], 4), _dev(t[~m], 8)              # the null-mask call on the gathered free rows: the same 1 / n_free
                G, dG = _run(zg, tg, T, mode, dt)
                assert torch.equal(_bits(dl)[idx], _bits(dG)), (name, "dlogits of the free rows")
                assert torch.equal(_bits(out["row_kl"])[idx], _bits(G["row_kl"]))
                with np.errstate(invalid="ignore"):
                    kl = out["row_kl"].cpu().numpy().astype(np.float64)[~m]
                    _close(s[0], kl.sum() / n_free, E24, name)
            else:
                assert (_bits(out["summary"][:4]) == 0).all() and s[4] == 1 and not np.isnan(s).any() and (_bits(dl) == 0).all()
            if name == "free":                                       # the null-mask call as a whole
                assert torch.equal(_bits(out["summary"]), _bits(U["summary"])) and s[4] == 0 and torch.equal(_bits(dl), _bits(dU))
                assert torch.equal(_bits(out["norm"]), _bits(U["norm"]))
    # a finite summary under a mask, against the restatement
    zc, tc, zcd, tcd = _pair(131, K, seed=K + 12, clean=True)
    _check(zc, tc, zcd, tcd, 1.0, 0, torch.float32, {}, _masks(131, seed=K)["random"])


def test_more_row_quads_than_workgroups():
    """Above 16384 row quads a workgroup takes several (and the summary's threads several partial sums): the rows' bits are those of two
    launches that stay below, and the means are the fp64 means of the rows."""
    rows, K, cut = 4 * 16384 + 4 * 300 + 3, 8, 40000
    g = torch.Generator(device="cpu").manual_seed(5)
    zd = torch.full((rows, K + 4), float("nan"), device=DEV)[:, :K]
    td = torch.full((rows, K + 8), float("nan"), device=DEV)[:, :K]
    zd.copy_(2 * torch.randn(rows, K, generator=g))
    td.copy_(2 * torch.randn(rows, K, generator=g))
    given = (torch.rand(rows, generator=g) < 0.3).to(DEV)
    for mask in (None, given):
        out, dl = _run(zd, td, 0.7, 0, torch.float32, mask)
        for a, b in ((0, cut), (cut, rows)):
            sub = ops.distill_loss(zd[a:b], td[a:b], temperature=0.7, mode=0, given=None if mask is None else mask[a:b].contiguous())
            assert torch.equal(_bits(out["row_kl"][a:b]), _bits(sub["row_kl"]))
        free = torch.ones(rows, dtype=torch.bool, device=DEV) if mask is None else ~mask
        n_free = int(free.sum())
        kl = out["row_kl"].double()
        _close(out["summary"][0].item(), (kl[free].sum() / n_free).item(), E24, "summary[0]")
        am = [ops.argmax(x, torch.empty(rows, dtype=torch.int64, device=DEV), rows=rows, K=K, ld=x.stride(0)) for x in (zd, td)]
        _close(out["summary"][3].item(), ((am[0] == am[1])[free].double().sum() / n_free).item(), E24, "summary[3]")
        assert out["summary"][4].item() == np.float32((rows - n_free) / rows) and out["norm"].item() == np.float32(1) / np.float32(n_free)
        p_s, p_t = torch.softmax(zd.double() * float(S.inv_temperature(0.7)), -1), torch.softmax(td.double() * float(S.inv_temperature(0.7)), -1)
        want = GOUT / n_free * float(S.inv_temperature(0.7)) * (p_s - p_t) * free[:, None]
        assert ((dl.double() - want).abs() <= 4 * D.TOL * want.abs().max() + 2.0 ** -126).all()


def test_refusals_launch_nothing():
    rows, K = 8, 16
    l = _lib.lib(0)
    z, t = torch.randn(rows, K + 4, device=DEV), torch.randn(rows, K + 8, device=DEV)
    given = torch.zeros(rows, dtype=torch.bool, device=DEV)
    row_kl, summary, norm = H.sent(rows, torch.float32), H.sent(5, torch.float32), H.sent(1, torch.float32)
    dl, dlb = H.sent((rows, K), torch.float32), H.sent((rows, K), torch.bfloat16)
    gout = torch.ones(1, device=DEV)
    kl_in, norm_in = torch.zeros(rows, device=DEV), torch.ones(1, device=DEV)
    p = lambda x: None if x is None else x if isinstance(x, int) else x.data_ptr()      # noqa: E731
    fwd0 = dict(logits=z, rows=rows, K=K, ld=K + 4, teacher=t, ld_t=K + 8, temperature=1.0, mode=0, given=given, row_kl=row_kl, summary=summary,
                norm=norm)
    bwd0 = dict(logits=z, rows=rows, K=K, ld=K + 4, teacher=t, ld_t=K + 8, temperature=1.0, mode=0, given=given, row_kl=kl_in, grad_out=gout,
                norm=norm_in, dlogits=dl, dl_dtype=ops.F32)

    def call(fn, base, over):
        a = {**base, **over}
        return lambda: _lib.check(fn(*[p(v) if k not in ("rows", "K", "ld", "ld_t", "temperature", "mode", "dl_dtype") else v for k, v in a.items()],
                                     None), l)

    both = [dict(logits=None), dict(teacher=None), dict(rows=0), dict(rows=-1), dict(K=0), dict(K=14), dict(K=4100, ld=4100, ld_t=4104),
            dict(ld=K - 4), dict(ld=K + 2), dict(ld_t=K - 4), dict(ld_t=K + 6), dict(logits=z.data_ptr() + 4), dict(teacher=t.data_ptr() + 8),
            dict(temperature=0.0), dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(mode=2)]
    for over in both + [dict(row_kl=None), dict(summary=None), dict(norm=None), dict(row_kl=row_kl.data_ptr() + 2)]:
        H.refused(call(l.mage_distill_loss, fwd0, over), row_kl, summary, norm)
    for over in both + [dict(row_kl=None), dict(grad_out=None), dict(norm=None), dict(dlogits=None), dict(dlogits=dl.data_ptr() + 8),
                        dict(dl_dtype=ops.F16), dict(dl_dtype=ops.BF16X3)]:
        H.refused(call(l.mage_distill_loss_bwd, bwd0, over), dl, dlb)
    # the wrappers' own asserts: shapes, dtypes and devices that do not fit never reach the library
    for bad in (lambda: ops.distill_loss(z[:, :K], t[:, :K + 4]), lambda: ops.distill_loss(z[:, :K].double(), t[:, :K]),
                lambda: ops.distill_loss(z[:, :K], t[:, :K], given=given[:-1]),
                lambda: ops.distill_loss_bwd(z[:, :K], t[:, :K], kl_in[:-1], norm_in, gout, torch.empty(rows, K, device=DEV))):
        with pytest.raises(AssertionError):
            bad()
    # a good call after all of that: the same arguments do run
    _lib.check(call(l.mage_distill_loss, fwd0, {})() or 0, l)
    torch.cuda.synchronize()
    assert H.written(row_kl) and H.written(summary) and H.written(norm)
