"""GPU: mage_policy_loss_grouped / mage_policy_loss_grouped_bwd (include/mage_hip_ext.h) against the masked pair bit for bit where the rule says
so, and against the fp64 restatement (tests/group_ratio_ref.py) everywhere else.  Logits: tests/test_gpu_policy_loss.py's recipe (`_logits`,
its special rows included) and its `Case` for tokens and advantages (0.5 <= |A| <= 2, both signs).

Bounds -- derived, not measured.
  cut, logprob, entropy, kl   the masked call's bits on the same inputs (the same row kernel instances).
  group_count                 exact.
  group_logratio              against the fp64 mean of the kernel's own fp32 d_i = logprob_i - b_i:
                              |diff| <= 2^-23 |m_g| + n_g 2^-50 mean|d_i| -- the one rounding to fp32 (2^-24 |m_g|, doubled), and the order
                              of the fp64 sum, which moves it by at most about n_g 2^-53 sum|d_i| (8x that after the division by n_g).
  row_loss                    against the fp64 formula on the kernel's own logprob, entropy and group_logratio:
                              |diff| <= (4 + |m_g|) 2^-23 |l| -- tests/test_gpu_policy_loss.py's bound with m_g for logprob - b, by its
                              argument: one expf (2 ulp), the rounding of its argument (|m_g| 2^-24 relative in rho_g), three multiplies /
                              adds; 0.5 <= |A| <= 2 and entropy_coef <= 0.01 keep the entropy term from cancelling the surrogate term.  Under
                              the anchored rule l gains kl_coef kl_i >= 0; the references here stay within 0.3 of logprob and kl_coef = 0.1, so
                              that term is below 0.1 (e^0.3 - 1.3) = 0.005 against |A| rho_g >= 0.4 * 0.75: |l| stays above 0.97 of the
                              plain |l|, inside the slack the bound has (its argument uses 1.27 x 3 of the 4 + |m_g| half-ulps).
  summary                     against the fp64 means of the kernel's own per-row outputs: one fp32 rounding, 2^-24 relative; summary[7] and
                              norm exact.
  dlogits                     against the restatement under the kept set the kernel reports, its terms formed from the kernel's logprob and
                              entropy with m_g in fp64: fp32 within 2 TOL max_j |want_ij| (TOL: token_stats_ref's allowance for the fp32 mass
                              sums; an anchored row: the max of |surrogate part| + |anchor part|), bf16 adds 2^-8 |want_ij|, both the floor
                              2^-126; exact zeros outside the set, in outside rows and in given rows.
Clip edges: every rho_g is kept at least 1e-3 (relative) away from both clip edges, checked in fp64 on the kernel's own logprob, so both sides
take one branch; a group that comes closer has its rows' b moved (drawn again), never skipped."""
import numpy as np
import pytest
import torch

from mage_amd import ops
from tests import group_ratio_ref as G
from tests import helpers as H
from tests import policy_kl_ref as Q
from tests import policy_ref as P
from tests import sampling_ref as S
from tests import token_stats_ref as R
from tests.test_gpu_policy_loss import CLIP, FILTERS, Case, _bits, _keys, _logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOUT = 0.7
KL_COEF, ENT = 0.1, 0.01
TEMPS = (0.7, 1.5)
SHAPES = [(1, 29), (3, 7), (64, 5), (300, 3)]         # (ratio_div, groups): 300 > one workgroup's threads and no multiple of 64; 3 x 7 = 21 rows
#                                                       are no multiple of the 4 rows per workgroup and its groups straddle workgroups
CMIN, CMAX = P.clip_bounds(*CLIP)
WORST = {}


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def _dbits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _masks(rows, rd, seed):
    """none; random; one that gives a whole group (n_g = 0); one that leaves a single counted row in a group."""
    g = np.random.default_rng(seed)
    groups = rows // rd
    whole = g.random(rows) < 0.2
    whole[(groups - 1) * rd:] = True
    single = g.random(rows) < 0.2
    single[(groups // 2) * rd:(groups // 2 + 1) * rd] = True
    single[(groups // 2) * rd + rd // 2] = False
    return [None, g.random(rows) < 0.45, whole, single]


def _near(m):
    with np.errstate(invalid="ignore", over="ignore"):
        rho = np.exp(m)
        return (np.abs(rho / CMIN - 1) < 1e-3) | (np.abs(rho / CMAX - 1) < 1e-3)


def _behaviour(lp32, given, rd, seed):
    """b = logprob + a per-group offset (group means on both sides of the clip range and inside it) + per-row noise; a group within 1e-3 of a
    clip edge has its rows' b moved by 0.01 and is checked again.  Returns fp32 b."""
    g = np.random.default_rng(seed)
    rows = len(lp32)
    lp = lp32.astype(np.float64)
    goff = np.resize([-0.35, 0.1, 0.35, -0.1], rows // rd) * g.uniform(0.8, 1.0, rows // rd)
    b = (np.where(np.isfinite(lp), lp, 0.0) + np.repeat(goff, rd) + 0.1 * g.uniform(-1, 1, rows)).astype(np.float32)
    for _ in range(6):
        m, _n = G.reduce(lp, b, given, rd)
        near = _near(m)
        b[np.repeat(near, rd)] += np.float32(0.01)
    assert not near.any()
    return b


class Setup:
    """One launch's inputs on the device, the masked (or plain / anchored) call's results on them, and the grouped call."""

    def __init__(self, z, zd, K, T, k, p, rd, adv_mul, mask, anch, dt, seed, b=None):
        rows = z.shape[0]
        self.z, self.zd, self.K, self.T, self.k, self.p, self.rd, self.dt, self.anch, self.rows = z, zd, K, T, k, p, rd, dt, anch, rows
        self.adv_div = rd * adv_mul
        case = Case(z, zd, K, T, k, p, seed=seed, clipped=False, adv_div=self.adv_div, c=ENT)
        self.tok, self.Ad = case.tok, case.Ad
        self.A_rows = case.A[np.arange(rows) // self.adv_div].astype(np.float64)
        groups = rows // rd
        if k > 0 and groups > 2:                                     # top-k on: group 1's tokens are each row's smallest logit -- all outside
            self.tok[rd:2 * rd] = torch.from_numpy(np.argmin(np.where(np.isnan(z[rd:2 * rd]), np.inf, z[rd:2 * rd]), 1)).to(DEV)
        self.tok_np = self.tok.cpu().numpy()
        self.given_np = mask
        self.given = None if mask is None else torch.from_numpy(mask).to(DEV)
        self.filt = dict(top_k=k, top_p=p)
        self.kw = dict(temperature=T, clip_lo=CLIP[0], clip_hi=CLIP[1], entropy_coef=ENT, adv_div=self.adv_div)
        self.gout = torch.tensor([GOUT], device=DEV)
        first = ops.policy_loss(zd, self.tok, self.Ad, None, **self.kw, **self.filt, given=self.given)
        lp32 = first["logprob"].cpu().numpy()
        self.ref_np = None
        if anch:                                                     # within 0.3 of the policy's own values; one -inf, one NaN, one d == 0
            g = np.random.default_rng(seed + 1)
            r = (np.where(np.isfinite(lp32), lp32, -1.0) + g.uniform(-0.3, 0.3, rows)).astype(np.float32)
            r[4 % rows], r[5 % rows], r[6 % rows] = -np.inf, np.nan, lp32[6 % rows]
            self.ref_np = r
            self.kw.update(reference_logprob=torch.from_numpy(r).to(DEV), kl_coef=KL_COEF)
        self.b_np = _behaviour(lp32, mask, rd, seed + 2) if b is None else b(lp32)
        self.bd = torch.from_numpy(self.b_np).to(DEV)
        # the token rule on the same inputs: the masked call with a mask, the plain / anchored call without
        self.U = ops.policy_loss(zd, self.tok, self.Ad, self.bd, **self.kw, **self.filt, given=self.given)

    def forward(self, rd=None):
        return ops.policy_loss(self.zd, self.tok, self.Ad, self.bd, **self.kw, **self.filt, given=self.given, ratio_div=rd or self.rd)

    def backward(self, out, rd=None, dt=None):
        dl = torch.empty(self.rows, self.K, device=DEV, dtype=dt or self.dt)
        return ops.policy_loss_bwd(self.zd, self.tok, self.Ad, self.bd, out["cut"], self.gout, dl, **self.kw, given=self.given, norm=out["norm"],
                                   ratio_div=rd or self.rd, group_logratio=out["group_logratio"])

    def token_backward(self, dt=None):
        dl = torch.empty(self.rows, self.K, device=DEV, dtype=dt or self.dt)
        return ops.policy_loss_bwd(self.zd, self.tok, self.Ad, self.bd, self.U["cut"], self.gout, dl, **self.kw, given=self.given,
                                   norm=self.U.get("norm"))


def _close(got, want, what):
    """2^-24 relative where the wanted value is finite; the same non-finite value otherwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (what, got, want)
    assert (np.abs(got[fin] - want[fin]) <= 2.0 ** -24 * np.abs(want[fin]) * (1 + 1e-6)).all(), (what, got, want)


def _check(su):
    """Every check of the module docstring on one launch.  Returns (out, the fp64 terms)."""
    rows, rd, K, z = su.rows, su.rd, su.K, su.z
    groups = rows // rd
    given = np.zeros(rows, bool) if su.given_np is None else su.given_np
    out, again = su.forward(), su.forward()
    dl, dl2 = su.backward(out), su.backward(again)
    ops.check_device_errors(DEV)
    want_keys = {"row_loss", "logprob", "entropy", "cut", "summary", "norm", "group_logratio", "group_count"} | ({"kl"} if su.anch else set())
    assert set(out) == want_keys and out["summary"].shape == (8,) and out["group_logratio"].shape == (groups,)
    for n in out:                                                    # two launches, the same bits
        assert torch.equal(_bits(out[n]), _bits(again[n])), n
    assert torch.equal(_dbits(dl), _dbits(dl2))
    for n in ("cut", "logprob", "entropy") + (("kl",) if su.anch else ()):     # the token rule's call on the same inputs: its bits
        assert torch.equal(_bits(out[n]), _bits(su.U[n])), n
    lp32, h32 = out["logprob"].cpu().numpy(), out["entropy"].cpu().numpy().astype(np.float64)
    loss = out["row_loss"].cpu().numpy().astype(np.float64)
    m32 = out["group_logratio"].cpu().numpy()
    cnt = G.counted(lp32, given)
    # group_count and group_logratio
    assert np.array_equal(out["group_count"].cpu().numpy(), cnt.reshape(groups, rd).sum(1))
    with np.errstate(invalid="ignore", over="ignore"):
        d32 = (lp32 - su.b_np).astype(np.float32)                    # the kernel's d_i: one fp32 subtraction
    want_m, n_g = G.reduce(lp32, su.b_np, given, rd, d=d32)
    assert np.array_equal(np.isnan(m32), np.isnan(want_m))
    for g in range(groups):
        if n_g[g] == 0:
            assert m32[g] == 0 and not np.signbit(m32[g]), g
        elif not np.isnan(want_m[g]):
            sl = slice(g * rd, (g + 1) * rd)
            bound = 2.0 ** -23 * abs(want_m[g]) + n_g[g] * 2.0 ** -50 * np.abs(d32[sl][cnt[sl]].astype(np.float64)).mean()
            assert abs(float(m32[g]) - want_m[g]) <= bound, (g, m32[g], want_m[g], bound)
            if bound:
                _note("group_logratio", abs(float(m32[g]) - want_m[g]) / bound)
    # the clip edges, in fp64 on the kernel's own logprob
    m64, _n = G.reduce(lp32, su.b_np, given, rd)
    assert not _near(m64).any()
    # row_loss: the fp64 formula on the kernel's own logprob, entropy and group_logratio
    c32, kc32 = float(np.float32(ENT)), float(np.float32(KL_COEF)) if su.anch else 0.0
    own, _m, _n = G.terms(lp32, h32, su.A_rows, su.b_np, given, rd, CMIN, CMAX, c32, su.ref_np, kc32, m=m32.astype(np.float64), fp32_d=True)
    for i in range(rows):
        if own[i] is None:
            assert _bits(out["row_loss"])[i].item() == 0, i          # a given row: +0
            continue
        t = own[i]
        if t["outside"]:                                             # (whatever its group's ratio is, a NaN included)
            assert _bits(out["row_loss"])[i].item() == 0, i
            continue
        if np.isnan(t["loss"]):
            assert np.isnan(loss[i]), i
            continue
        bound = (4 + abs(float(m32[i // rd]))) * 2.0 ** -23 * abs(t["loss"])
        assert abs(loss[i] - t["loss"]) <= bound, f"row {i}: row_loss {loss[i]!r} want {t['loss']!r} bound {bound:.3e}"
        if bound:
            _note("row_loss", abs(loss[i] - t["loss"]) / bound)
    # the fp64 terms (m_g in fp64 from the kernel's logprob): the branch each row takes, and the gradient's factor
    ref64, _m, _n = G.terms(lp32, h32, su.A_rows, su.b_np, given, rd, CMIN, CMAX, c32, su.ref_np, kc32, fp32_d=True)
    for i in range(rows):
        assert ref64[i] is None or np.isnan(ref64[i]["rho"]) or ref64[i]["off"] == own[i]["off"], i
    # summary and norm
    free = ~given
    n_free = int(free.sum())
    norm = out["norm"].cpu().numpy()
    want_norm = np.float32(1) / np.float32(n_free) if n_free else np.float32(0)
    assert norm.view(np.uint32)[0] == np.array([want_norm], np.float32).view(np.uint32)[0]
    got = out["summary"].cpu().numpy()
    assert got[7] == np.float32(given.sum() / rows)
    ins = free & ~np.isneginf(lp32)
    want = np.zeros(7)
    if n_free:
        with np.errstate(invalid="ignore"):
            want[0], want[1], want[4] = loss[ins].sum(), h32[ins].sum(), float((free & np.isneginf(lp32)).sum())
            want[2] = (su.b_np.astype(np.float64)[ins] - lp32.astype(np.float64)[ins]).sum()
            want[3] = float(sum(own[i]["off"] for i in np.flatnonzero(ins)))
            if su.anch:
                want[5] = out["kl"].cpu().numpy().astype(np.float64)[ins].sum()
                want[6] = float((~np.isfinite(su.ref_np))[ins].sum())
            want = want / n_free
    _close(got[:7], want, "summary")
    # dlogits
    s = (z * S.inv_temperature(su.T)).astype(np.float32)
    keep = _keys(s) >= out["cut"].cpu().numpy().view(np.uint32)[:, None]
    got_dl = dl.float().cpu().numpy().astype(np.float64)
    scale = float(np.float32(GOUT)) * float(want_norm)
    for i in range(rows):
        t = ref64[i]
        if t is None:
            assert (_dbits(dl)[i] == 0).all(), (i, "a given row: +0")
            continue
        if t["outside"] or not keep[i][su.tok_np[i]]:
            assert (got_dl[i] == 0).all(), i
            continue
        g_anchor = 0.0
        if su.anch and kc32 and Q.anchored(float(lp32[i]), float(su.ref_np[i])):
            g_anchor = kc32 * Q.grad_factor(Q.delta(float(lp32[i]), float(su.ref_np[i]), True))
        g_surr = -su.A_rows[i] * t["rho"] if not t["off"] else 0.0
        part = P.dlogits_row(z[i], int(su.tok_np[i]), -g_surr, None, su.T, keep[i], CMIN, CMAX, c32, scale)
        extra = g_anchor * P.dlogits_row(z[i], int(su.tok_np[i]), -1.0, None, su.T, keep[i], CMIN, CMAX, 0.0, scale) if g_anchor else np.zeros(K)
        want_dl = part + extra
        assert np.array_equal(np.isnan(got_dl[i]), np.isnan(want_dl)), f"row {i}: NaN pattern"
        assert (got_dl[i][~keep[i]] == 0).all(), i
        fin = ~np.isnan(want_dl)
        if fin.any():
            bound = 2 * R.TOL * (np.abs(part[fin]) + np.abs(extra[fin])).max() + (2.0 ** -8 * np.abs(want_dl[fin]) if su.dt == torch.bfloat16 else 0.0) \
                + 2.0 ** -126
            e = np.abs(got_dl[i][fin] - want_dl[fin])
            assert (e <= bound).all(), f"row {i}: dlogits |d| {e.max():.3e} > bound (row max {np.abs(want_dl[fin]).max():.3e})"
            _note("dlogits", (e / bound).max())
    return out, own


@pytest.mark.parametrize("K", [256, 512, 4096])
@pytest.mark.parametrize("rd,groups", SHAPES)
def test_grouped_pair_against_the_restatement(K, rd, groups):
    """The four filters; temperature, adv_div (ratio_div or twice it), the mask, the rule (plain / anchored) and the gradient's dtype take
    turns over them, shifted by the shape and by K so that every value meets every shape."""
    rows = rd * groups
    z = _logits(rows, K, seed=K + rd)
    zd = torch.from_numpy(z).to(DEV)
    shift = SHAPES.index((rd, groups)) + (256, 512, 4096).index(K)
    masks = _masks(rows, rd, seed=K + rd + 1)
    n_off = n_in = n_zero = 0
    for i, (k, p) in enumerate(FILTERS):
        j = i + shift
        su = Setup(z, zd, K, TEMPS[j % 2], k, p, rd, (1, 2)[(j // 2) % 2], masks[j % 4], anch=(j // 2) % 2 == 1,
                   dt=(torch.float32, torch.bfloat16)[(i + j // 4) % 2], seed=1000 * K + 10 * rd + i)
        out, own = _check(su)
        n_off += sum(t["off"] for t in own if t is not None and not t["outside"])
        n_in += sum(1 for t in own if t is not None and not t["outside"])
        n_zero += int((out["group_count"] == 0).sum().item())
    assert 0 < n_off < n_in and (rd == 1 or n_zero > 0)              # both branches of the clip; a group with nothing to count
    print(f"K={K} ratio_div={rd} groups={groups}: {n_in} counted rows ({n_off} clipped), {n_zero} empty groups; largest error / bound so far: "
          + ", ".join(f"{a} {v:.3f}" for a, v in WORST.items()))


def test_one_workgroup_per_group_against_the_restatement():
    """ratio_div = 1100 > 1024: the group kernel's other form (one workgroup of sixteen waves per group, some threads with two rows, some with
    one), held to the same bounds; a masked anchored bf16 launch and a plain fp32 one."""
    K, rd, groups = 256, 1100, 3
    rows = rd * groups
    z = _logits(rows, K, seed=K + rd)
    zd = torch.from_numpy(z).to(DEV)
    masks = _masks(rows, rd, seed=rd)
    n_zero = 0
    for i, ((k, p), mask, anch, dt) in enumerate((((20, 0.9), masks[1], True, torch.bfloat16), ((0, 1.0), masks[2], False, torch.float32))):
        out, _ = _check(Setup(z, zd, K, TEMPS[i], k, p, rd, 1 + i, mask, anch, dt, seed=rd + i))
        n_zero += int((out["group_count"] == 0).sum().item())
    assert n_zero == 2                                               # the all-outside group of the first launch, the given group of the second


@pytest.mark.parametrize("K", [256, 4096])
def test_ratio_div_one_carries_the_token_rules_bits(K):
    """ratio_div = 1: every output of both calls carries the masked call's bits; without mask and reference the plain call's, without mask
    the anchored call's."""
    rows = 29
    z = _logits(rows, K, seed=K + 5)
    zd = torch.from_numpy(z).to(DEV)
    masks = _masks(rows, 1, seed=K)
    for i, (k, p) in enumerate(FILTERS):
        for mask, anch in ((None, False), (None, True), (masks[1], False), (masks[1], True)):
            dt = (torch.float32, torch.bfloat16)[i % 2]
            su = Setup(z, zd, K, TEMPS[i % 2], k, p, 1, 1, mask, anch, dt, seed=7 * K + i)
            out = su.forward()
            for n in su.U:
                if n == "summary":
                    assert torch.equal(_bits(out[n][:su.U[n].numel()]), _bits(su.U[n])), (n, i, anch)
                    assert mask is not None or (out[n][su.U[n].numel():] == 0).all()
                else:
                    assert torch.equal(_bits(out[n]), _bits(su.U[n])), (n, i, anch)
            assert torch.equal(_dbits(su.backward(out)), _dbits(su.token_backward())), (i, anch)
            lp32 = out["logprob"].cpu().numpy()
            cnt = G.counted(lp32, mask)
            with np.errstate(invalid="ignore"):
                d32 = np.where(cnt, lp32 - su.b_np, np.float32(0)).astype(np.float32)
            got = out["group_logratio"].cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(d32)) and (got[~np.isnan(d32)] == d32[~np.isnan(d32)]).all()
    ops.check_device_errors(DEV)


@pytest.mark.parametrize("rd,groups", [(3, 7), (64, 5), (300, 3), (1200, 2)])
def test_on_policy_groups_are_exactly_one(rd, groups):
    """b with the bits of logprob on every counted row: m_g = +0 exactly, and row_loss and dlogits carry the token call's bits (rho = 1 on
    both sides).  (1200, 2): the one-workgroup-per-group form of the group kernel."""
    K, rows = 512, rd * groups
    z = _logits(rows, K, seed=rd)
    zd = torch.from_numpy(z).to(DEV)
    mask = _masks(rows, rd, seed=rd)[1]
    on_policy = lambda lp32: np.where(np.isfinite(lp32), lp32, np.float32(0)).astype(np.float32)      # noqa: E731  (-inf, NaN: not counted / NaN group)
    for anch, dt in ((False, torch.float32), (True, torch.bfloat16)):
        su = Setup(z, zd, K, 0.7, 20, 0.9, rd, 1, mask, anch, dt, seed=rd + 3, b=on_policy)
        out = su.forward()
        lp32 = out["logprob"].cpu().numpy()
        m = out["group_logratio"].cpu().numpy()
        nan_group = np.isnan(np.where(G.counted(lp32, mask), lp32, 0)).reshape(groups, rd).any(1)
        assert (_bits(out["group_logratio"]).cpu().numpy()[~nan_group] == 0).all() and np.isnan(m[nan_group]).all()
        rows_ok = torch.from_numpy(np.repeat(~nan_group, rd)).to(DEV)
        assert rows_ok.any()
        assert torch.equal(_bits(out["row_loss"])[rows_ok], _bits(su.U["row_loss"])[rows_ok])
        assert torch.equal(_dbits(su.backward(out))[rows_ok], _dbits(su.token_backward())[rows_ok])
    ops.check_device_errors(DEV)


def test_split_signs_on_the_device():
    """Half of each group at d = +0.5, half at -0.5, clip 0.2, A > 0: the token rule switches every +0.5 row off; the group rule has
    m_g = 0 up to the rounding of b, switches nothing off, and its dlogits are those of rho = 1."""
    K, rd, groups = 256, 64, 3
    rows = rd * groups
    z = _logits(rows + 13, K, seed=9)[13:]                          # (no special row: every token is inside)
    zd = torch.from_numpy(z).to(DEV)
    tok = torch.from_numpy(np.random.default_rng(1).integers(0, K, rows)).to(DEV)
    A = torch.tensor([1.5, 0.5, 2.0], device=DEV)
    kw = dict(temperature=1.0, clip_lo=0.2, clip_hi=0.2, entropy_coef=0.0, adv_div=rd)
    lp = ops.policy_loss(zd, tok, A, None, **kw)["logprob"]
    half = torch.where(torch.arange(rows, device=DEV) % rd < rd // 2, 0.5, -0.5)
    b = (lp.double() - half.double()).float()
    token = ops.policy_loss(zd, tok, A, b, **kw)
    out = ops.policy_loss(zd, tok, A, b, **kw, ratio_div=rd)
    ops.check_device_errors(DEV)
    assert token["summary"][3].item() == 0.5 and out["summary"][3].item() == 0.0
    assert (out["group_count"] == rd).all() and (out["group_logratio"].abs() < 2.0 ** -20).all()
    want = -(A.double() * out["group_logratio"].double().exp()).repeat_interleave(rd)              # l = -rho_g A: nothing clipped
    assert ((out["row_loss"].double() - want).abs() <= 5 * 2.0 ** -23 * want.abs()).all()
    gout = torch.ones(1, device=DEV)
    dl = ops.policy_loss_bwd(zd, tok, A, b, out["cut"], gout, torch.empty(rows, K, device=DEV), **kw, norm=out["norm"], ratio_div=rd,
                             group_logratio=out["group_logratio"])
    on = ops.policy_loss_bwd(zd, tok, A, None, out["cut"], gout, torch.empty(rows, K, device=DEV), **kw)     # g = -A: rho = 1
    tk = ops.policy_loss_bwd(zd, tok, A, b, token["cut"], gout, torch.empty(rows, K, device=DEV), **kw)
    assert ((dl - on).abs() <= 2.0 ** -19 * on.abs()).all()          # g = -A rho_g, |rho_g - 1| < 2^-20 (+ its rounding)
    clipped = (half > 0)
    assert (tk[clipped] == 0).all() and (dl[clipped] != 0).any(1).all()


@pytest.mark.parametrize("rd,groups,dt", [(1, 5, torch.float32), (3, 7, torch.bfloat16), (64, 5, torch.float32), (1100, 1, torch.bfloat16)])
def test_nothing_is_written_around_the_outputs(rd, groups, dt):
    """Every output sits inside a sentinel-filled buffer, 8 elements clear of either end; the raw entry points write their rows and groups and
    nothing else (tests/test_gpu_policy_kl.py's check)."""
    K, T, (k, p) = 260, 1.3, FILTERS[3]
    rows = rd * groups
    z = _logits(rows + 13, K, seed=17)[13:]
    zd = torch.from_numpy(z).to(DEV)
    g = np.random.default_rng(18)
    tok = torch.from_numpy(g.integers(0, K, rows)).to(DEV)
    A = torch.from_numpy((g.uniform(0.5, 2.0, groups) * g.choice([-1.0, 1.0], groups)).astype(np.float32)).to(DEV)
    ref = torch.full((rows,), -5.5, device=DEV)
    b = torch.full((rows,), -5.0, device=DEV)
    given = torch.from_numpy(g.random(rows) < 0.3).to(DEV)
    l, s = H.lib()
    pad = 8
    bufs = {n: H.sent(sz + 2 * pad, d) for n, sz, d in (("row_loss", rows, torch.float32), ("logprob", rows, torch.float32),
                                                        ("entropy", rows, torch.float32), ("cut", rows, torch.float32),
                                                        ("kl", rows, torch.float32), ("summary", 8, torch.float32), ("norm", 1, torch.float32),
                                                        ("glr", groups, torch.float32), ("gcount", groups, torch.float32),
                                                        ("dl", rows * K, dt))}
    o = {n: v[pad:v.numel() - pad] for n, v in bufs.items()}
    rc = l.mage_policy_loss_grouped(zd.data_ptr(), rows, K, K, tok.data_ptr(), A.data_ptr(), rd, b.data_ptr(), ref.data_ptr(), T, k, p, 0.2, 0.2, ENT,
                                    KL_COEF, o["row_loss"].data_ptr(), o["logprob"].data_ptr(), o["entropy"].data_ptr(), o["cut"].data_ptr(),
                                    o["kl"].data_ptr(), o["summary"].data_ptr(), o["norm"].data_ptr(), given.data_ptr(), rd, o["glr"].data_ptr(),
                                    o["gcount"].data_ptr(), s)
    assert rc == 0
    gout = torch.ones(1, device=DEV)
    rc = l.mage_policy_loss_grouped_bwd(zd.data_ptr(), rows, K, K, tok.data_ptr(), A.data_ptr(), rd, b.data_ptr(), ref.data_ptr(),
                                        o["cut"].data_ptr(), T, 0.2, 0.2, ENT, KL_COEF, gout.data_ptr(), o["norm"].data_ptr(), o["dl"].data_ptr(),
                                        ops.code(o["dl"]), given.data_ptr(), rd, o["glr"].data_ptr(), s)
    assert rc == 0
    ops.check_device_errors(DEV)
    for n, v in bufs.items():
        assert H.untouched(v[:pad]) and H.untouched(v[v.numel() - pad:]), n
        if n not in ("cut", "gcount"):                               # (a threshold may take any bit pattern; a count is checked below)
            assert H.written(o[n]), n
    want = ops.policy_loss(zd, tok, A, b, temperature=T, top_k=k, top_p=p, entropy_coef=ENT, reference_logprob=ref, kl_coef=KL_COEF, given=given,
                           adv_div=rd, ratio_div=rd)
    for n, w in (("row_loss", "row_loss"), ("logprob", "logprob"), ("entropy", "entropy"), ("kl", "kl"), ("summary", "summary"), ("norm", "norm"),
                 ("glr", "group_logratio")):
        assert torch.equal(_bits(o[n]), _bits(want[w])), n
    assert torch.equal(o["gcount"].view(torch.int32), want["group_count"])


def test_refusals_launch_nothing():
    rows, K, rd = 8, 16, 4
    z = torch.randn(rows, K, device=DEV)
    tok = torch.zeros(rows, dtype=torch.int64, device=DEV)
    A, b = torch.ones(2, device=DEV), torch.zeros(rows, device=DEV)
    kw = dict(adv_div=4)
    with pytest.raises(ValueError, match="behaviour_logprob"):
        ops.policy_loss(z, tok, A, None, **kw, ratio_div=rd)
    for bad in (0, -1, 3, 16, True, 2.0):
        with pytest.raises(ValueError, match="ratio_div"):
            ops.policy_loss(z, tok, A, b, **kw, ratio_div=bad)
    with pytest.raises(ValueError, match="ratio_div"):
        ops.policy_loss(z, tok, torch.ones(4, device=DEV), b, adv_div=2, ratio_div=rd)               # an advantage finer than the group
    l, s = H.lib()
    outs = [H.sent(rows, torch.float32) for _ in range(4)] + [H.sent(8, torch.float32), H.sent(1, torch.float32), H.sent(2, torch.float32),
                                                               H.sent(2, torch.float32)]
    dl = H.sent(rows * K, torch.float32)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def fwd(b=b, rd=rd, adv_div=4, glr=outs[6], gcount=outs[7], norm=outs[5]):
        return l.mage_policy_loss_grouped(p(z), rows, K, K, p(tok), p(A), adv_div, p(b), None, 1.0, 0, 1.0, 0.2, 0.2, 0.0, 0.0, p(outs[0]),
                                          p(outs[1]), p(outs[2]), p(outs[3]), None, p(outs[4]), p(norm), None, rd, p(glr), p(gcount), s)

    def bwd(b=b, rd=rd, adv_div=4, glr=outs[6], norm=outs[5]):
        return l.mage_policy_loss_grouped_bwd(p(z), rows, K, K, p(tok), p(A), adv_div, p(b), None, p(outs[3]), 1.0, 0.2, 0.2, 0.0, 0.0, p(outs[5]),
                                              p(norm), p(dl), 0, None, rd, p(glr), s)
    for call in (fwd, bwd):
        assert call(b=None) == -1 and call(rd=0) == -1 and call(rd=3) == -1 and call(adv_div=2) == -1 and call(adv_div=6) == -1
        assert call(glr=None) == -1 and call(norm=None) == -1
    assert fwd(gcount=None) == -1
    torch.cuda.synchronize()
    assert all(H.untouched(o) for o in outs) and H.untouched(dl)
