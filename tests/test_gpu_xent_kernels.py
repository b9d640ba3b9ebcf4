"""GPU: mage_token_xent / mage_token_xent_bwd (include/mage_hip_ext.h) against the fp64 restatement (tests/xent_ref.py) on the same fp32
inputs, and their bitwise promises.

Inputs: tests/test_gpu_policy_loss.py's `_logits` recipe (special rows: +-80, -inf entries, a NaN, all -inf, uniform, +-100, at rows 1, 2, 8,
9, 10, 12) with random targets, plus: the NaN row's target on the NaN itself (rank K), a target in the middle of the uniform row and of a
three-way tie (ties with an earlier and a later code), a target at 0 and one at K - 1.  The row stride is K + 4 with NaN in the padding.  The
class weights are multiples of 1/8 in [0, 3] with a zero among them, so that sum_free w_y is exact in fp64 in any order and norm can be held
to its bits.

Bounds (tests/xent_ref.py derives them from the kernel's operation count):
  row_loss, row_lse  |d| <= xent_ref.row's b_loss, b_lse; +inf and NaN rows must be +inf and NaN.
  dlogits            |d| <= xent_ref.dlogits_row's bound per element (2^-8 |want| more for the bf16 store, floor 2^-126); NaN where the
                     restatement is NaN.
  summary[0..4)      the fp64 means of the kernel's own per-row outputs, one fp32 rounding: 2^-24 relative.
By bits: row_nll == -mage_token_logprob; rank == the restatement's integer, and rank == 0 exactly where mage_argmax picks the target; given
rows +0 (rank 0); a free row's outputs whatever the other rows and the mask are; two launches; summary[4] and norm.
The largest error / bound per quantity is printed per K."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import helpers as H
from tests import xent_ref as X
from tests.test_gpu_masked_policy_kernels import _masks
from tests.test_gpu_policy_loss import _logits, _ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = [4, 256, 260, 512, 1028, 4096]                                   # every ladder instance; 260 and 1028: a partial last chunk
GOUT = 0.7
E24 = 2.0 ** -24
# (label_smoothing, z_loss, class weights, dlogits dtype): every option alone, all together, none
OPTS = [(0.0, 0.0, False, torch.float32), (0.1, 0.0, False, torch.bfloat16), (0.0, 1e-3, False, torch.bfloat16), (0.0, 0.0, True, torch.float32),
        (0.1, 1e-3, True, torch.float32), (0.3, 0.05, True, torch.bfloat16)]


def _dev(a, pad=4):
    """The rows of `a` on the device with row stride K + pad, NaN in the padding."""
    rows, K = a.shape
    buf = torch.full((rows, K + pad), float("nan"), device=DEV)
    v = buf[:, :K]
    v.copy_(torch.from_numpy(a))
    assert v.stride(0) == K + pad
    return v


def _weights(K, seed):
    w = (np.round(np.random.default_rng(seed).uniform(0.125, 3.0, K) * 8) / 8).astype(np.float32)
    w[K // 3] = 0.0
    return w


def _case(rows, K, seed, clean=False):
    """(z, y): logits and targets (numpy); clean: without the special rows (a finite summary)."""
    skip = 13 if clean else 0
    z = _logits(rows + skip, K, seed)[skip:].copy()
    y = np.random.default_rng(seed + 1).integers(0, K, rows)
    if not clean and rows > 16:
        y[8] = int(np.flatnonzero(np.isnan(z[8]))[0])                # the target is the NaN: rank K
        mid = max(K // 2, 1)
        y[10] = mid                                                  # the uniform row: ties with every earlier and later code
        y[14] = mid
        z[14, [mid - 1, mid, min(mid + 1, K - 1)]] = z[14, mid]      # a three-way tie around the target
        y[15], y[16] = 0, K - 1
    return z, y


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run(zd, yd, w, eps, zeta, dt, given=None):
    kw = dict(class_weight=w, label_smoothing=eps, z_loss=zeta, given=given)
    out = ops.token_xent(zd, yd, **kw)
    dl = ops.token_xent_bwd(zd, yd, out["norm"], torch.tensor([GOUT], device=DEV), torch.empty(zd.shape, device=DEV, dtype=dt), **kw)
    return out, dl


def _close(got, want, rel, what):
    assert np.isnan(got) == np.isnan(want), (what, got, want)
    if np.isfinite(want):
        assert abs(got - want) <= rel * abs(want) * (1 + 1e-6) + 2.0 ** -126, (what, got, want)
    elif not np.isnan(want):
        assert got == want, (what, got, want)


def _check(z, y, zd, yd, w_np, eps, zeta, dt, worst, given_np=None):
    """Every check of the module docstring on one launch."""
    rows, K = z.shape
    given = None if given_np is None else torch.from_numpy(given_np).to(DEV)
    wd = None if w_np is None else torch.from_numpy(w_np).to(DEV)
    out, dl = _run(zd, yd, wd, eps, zeta, dt, given)
    out2, dl2 = _run(zd, yd, wd, eps, zeta, dt, given)
    for n in out:                                                    # deterministic: two launches, the same bits
        assert torch.equal(_bits(out[n]), _bits(out2[n])), n
    assert torch.equal(_bits(dl), _bits(dl2))
    ref = X.loss(z, y, w_np, eps, zeta, given_np)
    free = np.ones(rows, bool) if given_np is None else ~given_np
    n_free = int(free.sum())
    got = {n: out[n].cpu().numpy().astype(np.float64) for n in ("row_loss", "row_nll", "row_lse")}
    for name, bound in (("row_loss", "b_loss"), ("row_lse", "b_lse")):
        g, want = got[name], ref[name]
        assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(np.isposinf(g), np.isposinf(want)), name
        assert np.array_equal(np.isneginf(g), np.isneginf(want)), name
        fin = np.isfinite(want) & free
        err = np.abs(g[fin] - want[fin]) / ref[bound][fin]
        assert (err <= 1).all(), f"{name}: row {np.flatnonzero(fin)[err.argmax()]} |d| / bound {err.max():.3f}"
        worst[name] = max(worst.get(name, 0.0), float(err.max()) if err.size else 0.0)
    # row_nll is mage_token_logprob with its sign turned, by bits; the rank is an integer
    lp = ops.token_logprob(zd, yd, torch.empty(rows, device=DEV), rows=rows, K=K, ld=zd.stride(0))
    fr = torch.from_numpy(free).to(DEV)
    assert torch.equal(_bits(out["row_nll"])[fr], _bits(-lp)[fr]), "row_nll == -mage_token_logprob by bits"
    rk = out["rank"].cpu().numpy()
    assert np.array_equal(rk[free], ref["rank"][free]), np.flatnonzero(rk != ref["rank"])
    am = ops.argmax(zd, torch.empty(rows, dtype=torch.int64, device=DEV), rows=rows, K=K, ld=zd.stride(0)).cpu().numpy()
    assert np.array_equal((rk == 0)[free], (am == y)[free]), "rank == 0 exactly where mage_argmax picks the target"
    for n in ("row_loss", "row_nll", "row_lse", "rank"):             # given rows: +0
        assert (out[n].view(torch.int32).cpu().numpy()[~free] == 0).all(), n
    # norm, the given share, the means of the kernel's own rows
    sw = float(np.sum((np.ones(K) if w_np is None else w_np.astype(np.float64))[y[free]]))
    want_norm = X.norms(sw, n_free)
    assert np.array_equal(out["norm"].cpu().numpy().view(np.uint32), want_norm.view(np.uint32))
    if w_np is None:
        one = np.float32(1) / np.float32(n_free) if n_free else np.float32(0)
        assert (want_norm == one).all()                              # without weights both are mage_cross_entropy's 1 / rows
    s = out["summary"].cpu().numpy()
    assert s.shape == (5,) and s[4] == np.float32((rows - n_free) / rows)
    if n_free:
        with np.errstate(invalid="ignore", over="ignore"):
            lse2 = (got["row_lse"][free] ** 2).sum() / n_free
            obj = (got["row_loss"][free].sum() / sw if sw > 0 else 0.0) + (float(np.float32(zeta)) * lse2 if zeta > 0 else 0.0)
            _close(s[0], obj, E24, "summary[0]")
            _close(s[1], got["row_nll"][free].sum() / n_free, E24, "summary[1]")
            _close(s[3], lse2, E24, "summary[3]")
        assert s[2] == np.float32((rk[free] == 0).sum() / n_free)
    else:
        assert (out["summary"][:4].view(torch.int32) == 0).all() and s[4] == 1 and (out["norm"] == 0).all()
    # the gradient
    g = dl.float().cpu().numpy().astype(np.float64)
    gb = _bits(dl).cpu().numpy()
    for i in range(rows):
        if not free[i]:
            assert (gb[i] == 0).all(), f"row {i}: a given row must be +0"
            continue
        want, bound = X.dlogits_row(ref["rows"][i], float(np.float32(GOUT)), float(want_norm[0]), float(want_norm[1]), float(np.float32(zeta)),
                                    bf16=dt == torch.bfloat16)
        assert np.array_equal(np.isnan(g[i]), np.isnan(want)), f"row {i}: NaN where the restatement is NaN"
        fin = np.isfinite(want)
        if fin.any():
            e = np.abs(g[i][fin] - want[fin]) / bound[fin]
            assert (e <= 1).all(), f"dlogits: row {i} code {np.flatnonzero(fin)[e.argmax()]} |d| / bound {e.max():.3f}"
            worst["dlogits"] = max(worst.get("dlogits", 0.0), float(e.max()))
    return out, dl


@pytest.mark.parametrize("K", KS)
def test_kernels_match_the_restatement(K):
    worst = {}
    z, y = _case(29, K, seed=K)                                      # 7 workgroups of 4 waves and a single wave; holds every special row
    zd, yd = _dev(z), torch.from_numpy(y).to(DEV)
    w = _weights(K, K)
    for i, (eps, zeta, weighted, dt) in enumerate(OPTS):
        wi = w if weighted else None
        base, _ = _check(z, y, zd, yd, wi, eps, zeta, dt, worst)
        if i in (0, 4):                                              # rows = 1 (a lone wave) and 5 (a ragged last workgroup): the same rows' bits
            for n, r0 in ((1, 0), (1, 8), (5, 0), (5, 8)):
                sub, _ = _check(z[r0:r0 + n], y[r0:r0 + n], zd[r0:r0 + n], yd[r0:r0 + n].contiguous(), wi, eps, zeta, dt, worst)
                for name in ("row_loss", "row_nll", "row_lse", "rank"):
                    assert torch.equal(_bits(sub[name]), _bits(base[name][r0:r0 + n])), (name, n, r0)
    # several workgroups, no special row: finite means
    zc, yc = _case(131, K, seed=K + 1, clean=True)
    out, _ = _check(zc, yc, _dev(zc), torch.from_numpy(yc).to(DEV), w, 0.1, 1e-3, torch.bfloat16, worst)
    assert torch.isfinite(out["summary"]).all() and out["summary"][0] > 0
    print(f"K={K}: largest error / bound: " + ", ".join(f"{a} {b:.3f}" for a, b in worst.items()))


@pytest.mark.parametrize("K", KS)
def test_plain_options_are_mage_cross_entropy(K):
    """eps = zeta = 0, no weights.  Per row both kernels form nll from an fp32 log Z and maximum in a different order: they agree to 2 ulp at
    the larger of |nll| and |lse| (tests/test_gpu_distill_kernels.py's comparison); the two means then differ by at most the mean of those
    per-row allowances plus one rounding of each mean.  The gradients agree within the two kernels' summed bounds: mage_cross_entropy_bwd
    performs the same operations (expf, one sum, 1 / Z, two products), so its bound is dlogits_row's."""
    rows = 67
    z, y = _case(rows, K, seed=K + 3, clean=True)
    zd, yd = _dev(z), torch.from_numpy(y).to(DEV)
    out = ops.token_xent(zd, yd)
    zc = zd.contiguous()
    ce = ops.cross_entropy(zc, yd)
    ops.check_device_errors(DEV)
    nll, lse = out["row_nll"].cpu().numpy().astype(np.float64), out["row_lse"].cpu().numpy().astype(np.float64)
    allow = (2 * _ulp(np.maximum(np.abs(nll), np.abs(lse)))).mean() + 2 * E24 * abs(nll.mean())
    d = abs(out["summary"][0].item() - ce.item())
    print(f"K={K}: summary[0] against mage_cross_entropy: |d| {d:.3e}, allowance {allow:.3e}")
    assert d <= allow
    assert torch.equal(_bits(out["row_loss"]), _bits(out["row_nll"])) and out["summary"][0].item() == out["summary"][1].item()
    one = torch.ones(1, device=DEV)
    dl = ops.token_xent_bwd(zd, yd, out["norm"], one, torch.empty(rows, K, device=DEV)).cpu().numpy().astype(np.float64)
    dce = ops.cross_entropy_bwd(zc, yd, one, torch.empty(rows, K, device=DEV)).cpu().numpy().astype(np.float64)
    ref = X.loss(z, y)
    n = X.norms(ref["sw"], rows)
    for i in range(rows):
        _, bound = X.dlogits_row(ref["rows"][i], 1.0, float(n[0]), float(n[1]), 0.0)
        assert (np.abs(dl[i] - dce[i]) <= 2 * bound).all(), i


@pytest.mark.parametrize("K", [4, 260, 512, 4096])
def test_masks(K):
    rows = 29
    z, y = _case(rows, K, seed=K + 11)
    yd = torch.from_numpy(y).to(DEV)
    w = _weights(K, K + 1)
    wd = torch.from_numpy(w).to(DEV)
    for i, (eps, zeta, weighted, dt) in enumerate(((0.1, 1e-3, True, torch.bfloat16), (0.0, 0.0, False, torch.float32))):
        wi, wdi = (w, wd) if weighted else (None, None)
        U, dU = _run(_dev(z), yd, wdi, eps, zeta, dt)
        for name, m in _masks(rows, seed=K + i).items():
            given = torch.from_numpy(m).to(DEV)
            zp = _dev(z)
            zp[given] = float("nan")                                 # the given rows must not be read
            yp = yd.clone()
            yp[given] = K + 7                                        # ... and their targets not range-checked
            out, dl = _run(zp, yp, wdi, eps, zeta, dt, given)
            ops.check_device_errors(DEV)
            for n in ("row_loss", "row_nll", "row_lse", "rank"):
                assert torch.equal(_bits(out[n])[~given], _bits(U[n])[~given]), (name, n, "free rows: the null-mask call's bits")
                assert (out[n].view(torch.int32)[given] == 0).all(), (name, n, "given rows: +0")
            assert (_bits(dl)[given] == 0).all(), name
            n_free = int((~m).sum())
            if n_free:
                idx = torch.from_numpy(np.flatnonzero(~m)).to(DEV)
                G, dG = _run(_dev(z[~m]), yd[idx].contiguous(), wdi, eps, zeta, dt)      # the null-mask call on the gathered free rows: the same norms
                assert torch.equal(_bits(out["norm"]), _bits(G["norm"])), name
                assert torch.equal(_bits(dl)[idx], _bits(dG)), (name, "dlogits of the free rows")
            else:
                assert (_bits(out["summary"][:4]) == 0).all() and out["summary"][4].item() == 1 and (_bits(dl) == 0).all()
                assert not torch.isnan(out["summary"]).any() and (out["norm"] == 0).all()
            if name == "free":                                       # the null-mask call as a whole
                assert torch.equal(_bits(out["summary"]), _bits(U["summary"])) and torch.equal(_bits(dl), _bits(dU))
                assert torch.equal(_bits(out["norm"]), _bits(U["norm"]))
        # a finite summary under a mask, against the restatement; a NaN inside a given row
        zc, yc = _case(131, K, seed=K + 12, clean=True)
        mk = _masks(131, seed=K)["random"]
        zcd = _dev(zc)
        zcd[torch.from_numpy(mk).to(DEV)] = float("nan")
        out, _ = _check(zc, yc, zcd, torch.from_numpy(yc).to(DEV), wi, eps, zeta, dt, {}, mk)
        assert torch.isfinite(out["summary"]).all()


def test_out_of_range_target_is_raised_and_clamped():
    K, rows = 16, 6
    z, y = _case(rows, K, seed=2, clean=True)
    zd = _dev(z)
    bad = y.copy()
    bad[2], bad[4] = K + 3, -5
    out = ops.token_xent(zd, torch.from_numpy(bad).to(DEV))
    with pytest.raises(ValueError, match="token out of range"):
        ops.check_device_errors(DEV)
    y[2], y[4] = K - 1, 0
    good = ops.token_xent(zd, torch.from_numpy(y).to(DEV))
    ops.check_device_errors(DEV)
    assert all(torch.equal(_bits(out[n]), _bits(good[n])) for n in out)


def test_more_row_quads_than_workgroups():
    """65 540 rows of K = 4 are 16 385 row quads: workgroup 0 owns two, and the summary's threads add 64 partial sums each.  The rows' bits
    are those of two launches that stay below; the means are the fp64 means of the rows; the gradient is the formula's in fp64."""
    rows, K, cut = 65540, 4, 40000
    eps, zeta = 0.1, 1e-3
    g = torch.Generator(device="cpu").manual_seed(5)
    zd = torch.full((rows, K + 4), float("nan"), device=DEV)[:, :K]
    zd.copy_(2 * torch.randn(rows, K, generator=g))
    yd = torch.randint(0, K, (rows,), generator=g).to(DEV)
    w = torch.tensor([0.5, 2.0, 1.0, 1.25], device=DEV)
    given = (torch.rand(rows, generator=g) < 0.3).to(DEV)
    for mask in (None, given):
        out, dl = _run(zd, yd, w, eps, zeta, torch.float32, mask)
        for a, b in ((0, cut), (cut, rows)):
            sub = ops.token_xent(zd[a:b], yd[a:b].contiguous(), class_weight=w, label_smoothing=eps, z_loss=zeta,
                                 given=None if mask is None else mask[a:b].contiguous())
            for n in ("row_loss", "row_nll", "row_lse", "rank"):
                assert torch.equal(_bits(out[n][a:b]), _bits(sub[n])), n
        free = torch.ones(rows, dtype=torch.bool, device=DEV) if mask is None else ~mask
        n_free = int(free.sum())
        sw = w.double()[yd][free].sum().item()                       # (quarters: exact)
        assert np.array_equal(out["norm"].cpu().numpy().view(np.uint32), X.norms(sw, n_free).view(np.uint32))
        lse2 = (out["row_lse"].double()[free] ** 2).sum().item() / n_free
        _close(out["summary"][0].item(), out["row_loss"].double()[free].sum().item() / sw + float(np.float32(zeta)) * lse2, E24, "summary[0]")
        _close(out["summary"][1].item(), out["row_nll"].double()[free].sum().item() / n_free, E24, "summary[1]")
        assert out["summary"][2].item() == np.float32((out["rank"][free] == 0).sum().item() / n_free)
        _close(out["summary"][3].item(), lse2, E24, "summary[3]")
        assert out["summary"][4].item() == np.float32((rows - n_free) / rows)
        # the gradient in fp64, by autograd through F.cross_entropy and the z term
        zz = zd.double().contiguous().requires_grad_(True)
        (GOUT * X.torch_loss(zz, yd, w.double(), eps, zeta, mask)).backward()
        want = zz.grad
        assert ((dl.double() - want).abs() <= 8 * X.TOL * want.abs().max() + 2.0 ** -126).all()
        assert (dl[~free] == 0).all()


def test_refusals_launch_nothing():
    rows, K = 8, 16
    l = _lib.lib(0)
    z = torch.randn(rows, K + 4, device=DEV)
    y = torch.zeros(rows, dtype=torch.int64, device=DEV)
    w = torch.ones(K, device=DEV)
    given = torch.zeros(rows, dtype=torch.bool, device=DEV)
    # (rank: int32 [rows] in a buffer that carries the fp32 sentinel's bits)
    outs = [H.sent(rows, torch.float32) for _ in range(4)] + [H.sent(5, torch.float32), H.sent(2, torch.float32)]
    row_loss, row_nll, row_lse, rank, summary, norm = outs
    dl, dlb = H.sent((rows, K), torch.float32), H.sent((rows, K), torch.bfloat16)
    gout, norm_in = torch.ones(1, device=DEV), torch.ones(2, device=DEV)
    p = lambda x: None if x is None else x if isinstance(x, int) else x.data_ptr()      # noqa: E731
    plain = ("rows", "K", "ld", "label_smoothing", "z_loss", "dl_dtype")
    fwd0 = dict(logits=z, rows=rows, K=K, ld=K + 4, target=y, class_weight=w, label_smoothing=0.1, z_loss=1e-3, given=given, row_loss=row_loss,
                row_nll=row_nll, row_lse=row_lse, rank=rank, summary=summary, norm=norm)
    bwd0 = dict(logits=z, rows=rows, K=K, ld=K + 4, target=y, class_weight=w, label_smoothing=0.1, z_loss=1e-3, given=given, grad_out=gout,
                norm=norm_in, dlogits=dl, dl_dtype=ops.F32)

    def call(fn, base, over):
        a = {**base, **over}
        return lambda: _lib.check(fn(*[v if k in plain else p(v) for k, v in a.items()], None), l)

    both = [dict(logits=None), dict(target=None), dict(norm=None), dict(rows=0), dict(rows=-1), dict(K=0), dict(K=14), dict(K=4100, ld=4100),
            dict(ld=K - 4), dict(ld=K + 2), dict(logits=z.data_ptr() + 4), dict(target=y.data_ptr() + 4), dict(class_weight=w.data_ptr() + 8),
            dict(label_smoothing=-0.01), dict(label_smoothing=1.0), dict(label_smoothing=float("nan")), dict(z_loss=-1.0),
            dict(z_loss=float("inf")), dict(z_loss=float("nan"))]
    for over in both + [dict(row_loss=None), dict(row_nll=None), dict(row_lse=None), dict(summary=None), dict(row_lse=row_lse.data_ptr() + 2),
                        dict(rank=rank.data_ptr() + 1)]:
        H.refused(call(l.mage_token_xent, fwd0, over), *outs)
    for over in both + [dict(grad_out=None), dict(dlogits=None), dict(dlogits=dl.data_ptr() + 8), dict(dl_dtype=ops.F16), dict(dl_dtype=ops.BF16X3)]:
        H.refused(call(l.mage_token_xent_bwd, bwd0, over), dl, dlb)
    # the wrappers' own asserts: shapes, dtypes and devices that do not fit never reach the library
    zz = z[:, :K]
    for bad in (lambda: ops.token_xent(zz.double(), y), lambda: ops.token_xent(zz, y[:-1]), lambda: ops.token_xent(zz, y.int()),
                lambda: ops.token_xent(zz, y, class_weight=w[:-4]), lambda: ops.token_xent(zz, y, given=given[:-1]),
                lambda: ops.token_xent_bwd(zz, y, norm_in[:1], gout, torch.empty(rows, K, device=DEV))):
        with pytest.raises(AssertionError):
            bad()
    # a good call after all of that: the same arguments do run
    call(l.mage_token_xent, fwd0, {})()
    call(l.mage_token_xent_bwd, bwd0, {})()
    torch.cuda.synchronize()
    assert all(H.written(o) for o in outs) and H.written(dl)
