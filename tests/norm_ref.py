"""fp64 restatements of the norm and loss entry points of the randomness branch, the MAGE+ head and the stage-1 VQ-VAE (include/mage_hip.h;
kernels in mage_amd/csrc/norm.hip and rows.hip) as closed formulas on their logical rows, with a per-element error bound for every output:
    mage_groupnorm_act / mage_groupnorm_silu, mage_groupnorm_bwd, mage_adain, mage_adain_bwd, mage_add_scaled_rowvec, mage_bn_colreduce,
    mage_bn_apply, mage_bn_bwd_apply, mage_reparam_kl, mage_reparam_kl_bwd, mage_mse, mage_mse_bwd.
The references take the exact fp32 values the kernels read.  (mean, rstd) are INPUTS of mage_groupnorm_bwd, of mage_bn_colreduce modes 1 and 2
and of mage_bn_apply / mage_bn_bwd_apply: their references use the fp32 values handed to the kernel, not statistics of their own.

Bounds.  u = 2^-24, D = 2^-53, first order in u (the one second-order term em^2 is kept, as in tests/train_ref.py).  Figures: an fp32 add,
multiply, divide, sqrtf: relative u each (a bound that counts a product's rounding AND the add's holds with or without contraction); device
expf 2 u; a fixed-order fp32 sum whose every term passes through at most n additions: n u sum|terms|; the same in double: n D sum|terms|; a
cast of a double to fp32: u; a bf16 / f16 store: one ulp of the type at |ref| (tests/helpers.py ulp).

Activations.  t carries the absolute error et.
  ReLU: max(t, 0) and the mask t > 0 are exact given the sign of t.  The input builders give data with |t| > 4 et everywhere (they ask 16 et;
        tests/test_norm_ref_cpu.py asserts 4 et on every case): the sign is certain, no element is exempt: y carries et where t > 0 and is
        exactly 0 elsewhere, the gradient is exactly dy or exactly 0.
  SiLU y = t / (1 + expf(-t)), s = 1 / (1 + e^-t): expf(-t) inherits et as a relative error, plus 2 u; the denominator 1 + e errs by
        e (et + 2 u) + u (1 + e), relative (1 - s)(et + 2 u) + u; the divide u:
                                                  |err y| <= s et + |y| ((1 - s)(et + 2 u) + 2 u) + 2^-126
        (the last term: below t ~ -88.7 expf overflows to +inf and y is -0 exactly where the true value is a subnormal: never NaN).
  SiLU' ge = dy s (1 + t (1 - s)):  s: relative rs = (1 - s)(et + 2 u) + 2 u, es = s rs;  a = 1 - s: ea = es + u a;  b = t a: eb = et a +
        |t| ea + u |t a|;  c = 1 + b: ec = eb + u |c|;  the two multiplies:
                                                  |err ge| <= |dy| (s ec + |s c| (rs + 2 u)) + 2^-126.
GroupNorm statistics (gn_stats_kernel: double accumulation of n = rows cpg widened fp32 values, two passes, one cast each):
  mean:  |mean^ - mean| <= em = u |mean| + n D mean|x|;   rstd = (float)(1 / sqrt(var + eps)) in double: relative er = u + (n + 8) D.
GroupNorm forward (gn_apply_kernel) t = ((x - mean^) rstd^) g + b (+ res), d = x - mean, xh = d rstd:
  xh:    |err| <= exh = rstd (em + u |d|) + |xh| (er + u);
  t:     et = |g| exh + u (|xh g| + |xh g + b| + |t| [with a residual]);   then the activation, then the store.
GroupNorm backward (gn_bwd_reduce_kernel, gn_bwd_apply_kernel), mean and rstd given: exh = u rstd |d| + u |xh|, et as above, ge = dy act'(t)
  with its error ege (0 for act 0 and 1).  Sums over the rows of one sample in double (n = rows terms), one cast:
  dbeta_part:   sum_r ege + rows D sum|ge| + u |dbeta|;     dgamma_part (the product ge xh is formed in double): sum_r (ege |xh| + |ge| exh)
                + rows D sum|ge xh| + u |dgamma|;
  red = (m1, m2) = mean over the group of (g ge, g ge xh), n = rows cpg:  em1 = mean(|g| ege) + (n + 4) D mean|g ge| + u |m1|,
                em2 = mean(|g| (ege |xh| + |ge| exh)) + (n + 4) D mean|g ge xh| + u |m2|;
  dx = rstd (g ge - m1^ - xh^ m2^) with the red the first kernel wrote:
                |err dx| <= rstd (|g| ege + em1 + exh |m2| + |xh| em2 + 4 u (|g ge| + |m1| + |xh m2|)) + u |dx|;   dres = ge: ege.
ADAIN (adain_kernel, adain_bwd_kernel: thread = (channel, phase); a phase adds np = ceil(P / 4) terms in order, then three additions and one
  divide; the variance is two-pass), A = mean_p |x|:
  mean:  em = (np + 4) u A;   V = var + eps: eV = (np + 7) u var + em^2 + u V (the rounding of x - mean^ 2, the square 1, np + 3 additions,
  the divide 1; the shift of the mean enters at second order only because sum_p d = 0);   rstd = 1 / sqrtf(V^): er = eV / (2 V) + 2 u.
  out = g ((x - mean^) rstd^) + b:  exh = rstd (em + u |d|) + |xh| (er + u);   |err out| <= |g| exh + u |g xh| + u |out|.
  A one-pass variance errs by ~ u np mean^2 in V: outside this bound on rows ~ N(64, 1) (tests/test_norm_ref_cpu.py).
  backward, g = dout gmap (u): m1 = mean_p g: emg = (np + 5) u mean|g|;  m2 = mean_p g xh: emgx = (np + 6) u mean|g xh| + mean(|g| exh);
  dgmap = dout xh: |dout| exh + u |dout xh|;
  dx = rstd (g - m1 - xh m2): rstd (emg + exh |m2| + |xh| emgx + 4 u (|g| + |m1| + |xh m2|)) + |dx| (er + u).
mage_add_scaled_rowvec x + s v:  u |s v| + u |out|.
BatchNorm.  bn_colreduce_kernel: workgroup p adds its rpb = ceil(rows / n_part) rows in order; mean, rstd given.
  mode 0: rpb u sum|x|;  mode 1, terms (x - m)(x - m) (3 u): (rpb + 3) u sum (x - m)^2;  mode 2, g = dy [mask > 0] (exact): rpb u sum|g| and,
  terms g ((x - m) rs) (3 u), (rpb + 3) u sum|g xh|, each over the slab.  mage_sum_partials adds n_part rows: n_part u sum|partials| more.
  ops.bn_train_stats: mean = sum / rows (u more); var likewise, about the mean it was handed; rstd = rsqrt(var^ + eps): u V for the add, one ulp
  (2 u) for the rsqrt on top of the error of var^ / (2 V).
  bn_apply t = (x - m) rs g + b (+ res): et = 3 u |xh g| + u |xh g + b| + u |t| [with a residual], then ReLU and the store.
  bn_bwd_apply dx = (g rs) (gy - s1 inv - xh (s2 inv)), inv = 1.0f / rows (u): s1 inv 2 u, xh 2 u, s2 inv 2 u and their product 1, two
  subtractions, then g rs and the last multiply:
                |err dx| <= |g rs| (4 u |s1 / rows| + 7 u |xh s2 / rows| + 2 u |gy|) + 2 u |dx|.
Reparameterisation.  out = eps expf(lv / 2) + mu (lv / 2 is exact): 3 u |eps e^(lv/2)| + u |out|.
  kl_sum = (float) sum in double of the fp32 terms 1 + lv - mu mu - expf(lv): a term errs by
  u (|1 + lv| + mu^2 + |1 + lv - mu^2| + 2 e^lv + |term|) -- it follows exp(lv); the sum: sum of these + n D sum|term| + u |kl_sum|.
  backward: dmu = dz + c mu: u |c mu| + u |dmu|;  dlogvar = A - B, A = dz/2 eps expf(lv/2) (4 u), B = c/2 (1 - expf(lv)):
  |c / 2| (2 u e^lv + u |1 - e^lv|) + u |B|;  the subtraction u |dlogvar|.
MSE.  Terms (a - b)^2 in fp32 (relative 3 u, all positive), the sum in double over n = rows cols terms, times 1 / n in double, one cast:
  (4 u + (n + 2) D) mse.   backward 2 (a - b) inv_n gout with inv_n = (float)(1 / n): 4 u |da|; padding columns exactly 0.
No constant here is fitted to a kernel's output."""
from types import SimpleNamespace

import torch

from tests.train_ref import U, f32, store_err

D = 2.0 ** -53
TINY = 2.0 ** -126


def _g(*seed):
    return torch.Generator().manual_seed(sum(int(s) * m for s, m in zip(seed, (1000003, 10007, 131, 17, 3, 1, 7919))) % (2 ** 31))


# ------------------------------------------------------------------------------------------------ activations
def act_fwd(t, et, act):
    """(y, bound) of act(t) for t with absolute error et; act 0 none, 1 ReLU (the sign of t certain), 2 SiLU."""
    if act == 0:
        return t, et
    if act == 1:
        return t.clamp(min=0), torch.where(t > 0, et, torch.zeros_like(et))
    s = torch.sigmoid(t)
    y = t * s
    return y, s * et + y.abs() * ((1 - s) * (et + 2 * U) + 2 * U) + TINY


def act_bwd(t, et, act, dy):
    """(ge, bound) of dy act'(t)."""
    if act == 0:
        return dy.clone(), torch.zeros_like(dy)
    if act == 1:
        return torch.where(t > 0, dy, torch.zeros_like(dy)), torch.zeros_like(dy)
    s = torch.sigmoid(t)
    a = torch.sigmoid(-t)                                                   # 1 - s without the cancellation
    rs = a * (et + 2 * U) + 2 * U
    es = s * rs
    ea = es + U * a
    eb = et * a + t.abs() * ea + U * (t * a).abs()
    c = 1 + t * a
    ec = eb + U * c.abs()
    return dy * s * c, dy.abs() * (s * ec + (s * c).abs() * (rs + 2 * U)) + TINY


def sign_margin(t, et):
    """min |t| / et: the ReLU cases need it above 4."""
    return float((t.abs() / et).min())


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_LADDER = ((8, 8), (8, 4), (12, 4), (64, 16), (512, 32), (256, 1))      # cpg 1, 2, 3, 4, 16, 256
GN_ROWS = (1, 5, 255, 257, 300)
GN_BWD_ROWS = (1, 3, 257)
GN_EPS = 1e-5
GN_PAD, GN_OFF = 40, 8                                                    # sample_stride_rows = rows + 40, row_off = 8
GN_YPAD, GN_YOFF = 7, 3                                                   # the output's own map
GN_SILU_CASES = tuple(dict(C=C, groups=g, rows=r, B=B, act=2, res=False, kind=k) for k in ("f32", "bf16", "f16")
                      for C, g, r, B in ((8, 4, 5, 3), (12, 4, 257, 1), (256, 1, 255, 3)))   # mage_groupnorm_silu: packed y


def gn_fwd_cases():
    """Every (C, groups) with every rows_per_sample; n_samples, act, residual and the y dtype rotate with a period (7 per rung) coprime to
    theirs, so that every value meets several cpg and several row counts.  mage_groupnorm_silu has cases of its own."""
    out, k = [], 0
    for C, groups in GN_LADDER:
        for rows in GN_ROWS:
            out.append(dict(C=C, groups=groups, rows=rows, B=(1, 3)[k % 2], act=k % 3, res=bool((k // 2) % 2), kind=("f32", "bf16", "f16")[(k // 3) % 3]))
            k += 1
        k += 2
    return out


def gn_bwd_cases():
    out, k = [], 0
    for C, groups in GN_LADDER:
        if C // groups == 3:
            continue
        for rows in GN_BWD_ROWS:
            out.append(dict(C=C, groups=groups, rows=rows, B=(3, 1)[k % 2], act=k % 3, res=bool((k // 2) % 2)))
            k += 1
        k += 2
    return out


def case_id(c):
    return "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in c.items())


def gn_view(x, groups):
    B, R, C = x.shape
    return x.reshape(B, R, groups, C // groups)


def gn_stats(x, groups, eps=GN_EPS):
    """fp64 (mean, rstd) [B, groups] of x [B, R, C] and the bounds (b_mean, b_rstd, er)."""
    xg = gn_view(x, groups)
    n = xg.shape[1] * xg.shape[3]
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = (var + f32(eps)).rsqrt()
    em = U * mean.abs() + n * D * xg.abs().mean((1, 3))
    er = U + (n + 8) * D
    return SimpleNamespace(mean=mean, rstd=rstd, em=em, er=er, b_rstd=rstd * er)


def _per_elem(v, x, groups):
    """[B, groups] -> [B, 1, C]."""
    return v.repeat_interleave(x.shape[2] // groups, 1)[:, None, :]


def gn_t(x, mean, rstd, em, er, gamma, beta, res, groups):
    """t = xh gamma + beta (+ res) in fp64 with (xh, exh, t, et); mean, rstd, em [B, groups]; er a number."""
    m, rs, e = _per_elem(mean, x, groups), _per_elem(rstd, x, groups), _per_elem(em, x, groups)
    d = x - m
    xh = d * rs
    exh = rs * (e + U * d.abs()) + xh.abs() * (er + U)
    p = xh * gamma
    t = p + beta
    et = gamma.abs() * exh + U * (p.abs() + t.abs())
    if res is not None:
        t = t + res
        et = et + U * t.abs()
    return SimpleNamespace(xh=xh, exh=exh, t=t, et=et, rstd=rs)


def groupnorm_act(x, gamma, beta, groups, res, act, kind="f32", eps=GN_EPS):
    """x [B, R, C] fp64, res [B, R, C] or None -> SimpleNamespace(y, b_y, mean, b_mean, rstd, b_rstd, t, et)."""
    s = gn_stats(x, groups, eps)
    q = gn_t(x, s.mean, s.rstd, s.em, s.er, gamma, beta, res, groups)
    y, b = act_fwd(q.t, q.et, act)
    return SimpleNamespace(y=y, b_y=b + store_err(y, kind), mean=s.mean, b_mean=s.em, rstd=s.rstd, b_rstd=s.b_rstd, t=q.t, et=q.et)


def groupnorm_bwd(x, mean, rstd, gamma, beta, groups, res, act, dy):
    """mean, rstd [B, groups]: the fp32 values handed to the kernel, in fp64.  -> dx, dres, red [B, groups, 2], dgamma_part, dbeta_part [B, C]
    and their bounds b_*; t, et."""
    B, R, C = x.shape
    cpg = C // groups
    n = R * cpg
    q = gn_t(x, mean, rstd, torch.zeros_like(mean), 0.0, gamma, beta, res, groups)
    ge, ege = act_bwd(q.t, q.et, act, dy)
    xh, exh = q.xh, q.exh
    db, dg = ge.sum(1), (ge * xh).sum(1)
    b_db = ege.sum(1) + R * D * ge.abs().sum(1) + U * db.abs()
    b_dg = (ege * xh.abs() + ge.abs() * exh).sum(1) + R * D * (ge * xh).abs().sum(1) + U * dg.abs()
    gg = ge * gamma

    def gmean(v):
        return gn_view(v, groups).mean((1, 3))
    m1, m2 = gmean(gg), gmean(gg * xh)
    em1 = gmean(gamma.abs() * ege) + (n + 4) * D * gmean(gg.abs()) + U * m1.abs()
    em2 = gmean(gamma.abs() * (ege * xh.abs() + ge.abs() * exh)) + (n + 4) * D * gmean((gg * xh).abs()) + U * m2.abs()
    M1, M2, E1, E2 = (_per_elem(v, x, groups) for v in (m1, m2, em1, em2))
    dx = q.rstd * (gg - M1 - xh * M2)
    b_dx = q.rstd * (gamma.abs() * ege + E1 + exh * M2.abs() + xh.abs() * E2 + 4 * U * (gg.abs() + M1.abs() + (xh * M2).abs())) + U * dx.abs()
    return SimpleNamespace(dx=dx, b_dx=b_dx, dres=ge, b_dres=ege, red=torch.stack([m1, m2], -1), b_red=torch.stack([em1, em2], -1),
                           dg=dg, b_dg=b_dg, db=db, b_db=b_db, t=q.t, et=q.et)


def gn_inputs(C, groups, rows, B, act, res, cold=False, seed=0):
    """x [B, rows, C] fp32 (B == 3: sample 1 ~ N(64, 1), sample 2 constant 0.5), gamma (an exact 0 in channel 0 where C / groups > 1, a
    negative entry), beta (|beta| >= 0.05; cold: beta[1] = -100, t ~ -100 there), res [B, rows, C] or None, dy.  For act 1 the data are nudged
    until every |t| exceeds 16 et of the forward bound: elements of res, or of x (never of the constant sample, whose t = beta) without one."""
    g = _g(C, groups, rows, B, act, res, seed)
    x = torch.randn(B, rows, C, generator=g) * 2 + 0.3
    if B >= 3:
        x[1] = torch.randn(rows, C, generator=g) + 64
        x[2] = 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    beta = torch.where(beta < 0, beta - 0.05, beta + 0.05)
    if C // groups > 1:
        gamma[0] = 0.0
    gamma[-1] = -gamma[-1].abs() - 0.1
    if cold:
        beta[1], gamma[1] = -100.0, 0.5
    r = torch.randn(B, rows, C, generator=g) if res else None
    dy = torch.randn(B, rows, C, generator=g)
    if act == 1:
        for _ in range(40):
            f = groupnorm_act(x.double(), gamma.double(), beta.double(), groups, None if r is None else r.double(), 0)
            bad = f.t.abs() <= 16 * f.et
            if not bool(bad.any()):
                break
            bump = 0.0625 * (1 + torch.rand(B, rows, C, generator=g))
            if r is not None:
                r = torch.where(bad, r + bump, r)
            else:
                x = torch.where(bad, x + bump, x)
        else:
            raise AssertionError("gn_inputs: could not move every t off the ReLU kink")
    return SimpleNamespace(x=x, gamma=gamma, beta=beta, res=r, dy=dy)


def padded(x, pad, off, fill=None):
    """[B, rows, C] -> the buffer [B * (rows + pad) + 3, C] of the row map (b (rows + pad) + off + r) and the bool row mask of the mapped rows."""
    B, R, C = x.shape
    buf = torch.full((B * (R + pad) + 3, C), float("nan") if fill is None else fill, dtype=x.dtype)
    rows = (torch.arange(B)[:, None] * (R + pad) + off + torch.arange(R)[None]).reshape(-1)
    buf[rows] = x.reshape(B * R, C)
    mask = torch.zeros(buf.shape[0], dtype=torch.bool)
    mask[rows] = True
    return buf, mask, rows


# ------------------------------------------------------------------------------------------------ ADAIN, row vector
ADAIN_CASES = tuple((B, P, C) for C in (64, 128) for P in (1, 2, 3, 4, 5, 257) for B in ((1, 3) if P in (1, 5, 257) else (3,)))
ADAIN_EPS = 1e-5
ROWVEC_CASES = ((3, 5, 4), (2, 65, 260))


def adain_inputs(B, P, C):
    """x [B, P, C] (B == 3: sample 1 ~ N(64, 1)), gamma / beta maps, dout."""
    g = _g(B, P, C, 5)
    x = torch.randn(B, P, C, generator=g) * 1.5 - 0.2
    if B >= 3:
        x[1] = torch.randn(P, C, generator=g) + 64
    return SimpleNamespace(x=x, gamma=torch.randn(B, P, C, generator=g) + 1, beta=torch.randn(B, P, C, generator=g), dout=torch.randn(B, P, C, generator=g))


def adain_stats(x, eps):
    P = x.shape[1]
    np_ = -(-P // 4)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    V = var + f32(eps)
    rstd = V.rsqrt()
    em = (np_ + 4) * U * x.abs().mean(1, keepdim=True)
    eV = (np_ + 7) * U * var + em * em + U * V
    er = eV / (2 * V) + 2 * U
    xh = d * rstd
    return SimpleNamespace(np=np_, d=d, rstd=rstd, er=er, xh=xh, exh=rstd * (em + U * d.abs()) + xh.abs() * (er + U))


def adain(x, gamma, beta, eps=ADAIN_EPS):
    s = adain_stats(x, eps)
    out = gamma * s.xh + beta
    return out, gamma.abs() * s.exh + U * (gamma * s.xh).abs() + U * out.abs()


def adain_bwd(x, gamma, dout, eps=ADAIN_EPS):
    """-> (dx, b_dx, dgmap, b_dgmap)."""
    s = adain_stats(x, eps)
    g = dout * gamma
    m1, m2 = g.mean(1, keepdim=True), (g * s.xh).mean(1, keepdim=True)
    emg = (s.np + 5) * U * g.abs().mean(1, keepdim=True)
    emgx = (s.np + 6) * U * (g * s.xh).abs().mean(1, keepdim=True) + (g.abs() * s.exh).mean(1, keepdim=True)
    dx = s.rstd * (g - m1 - s.xh * m2)
    b_dx = s.rstd * (emg + s.exh * m2.abs() + s.xh.abs() * emgx + 4 * U * (g.abs() + m1.abs() + (s.xh * m2).abs())) + dx.abs() * (s.er + U)
    dgm = dout * s.xh
    return dx, b_dx, dgm, dout.abs() * s.exh + U * dgm.abs()


def add_scaled_rowvec(x, s, vec):
    """x [B, P, C], s [B], vec [C]."""
    p = s[:, None, None] * vec
    out = x + p
    return out, U * p.abs() + U * out.abs()


# ------------------------------------------------------------------------------------------------ BatchNorm
BN_RED_SHAPES = ((1, 1), (7, 3), (5, 8), (1000, 4))                       # (rows, n_part)
BN_RED_C = (4, 256, 260)
BN_APPLY_ROWS = (1, 5, 257)
BN_APPLY_C = (4, 260)
BN_EPS = 1e-5
BN_TAIL = 4                                                               # rows of 1e6 behind x, dy and the mask: a read past `rows` is loud


def bn_inputs(rows, C, big=False, relu=False, res=False):
    """x [rows, C], dy, (mean, rstd) = the fp64 batch statistics rounded to fp32, gamma, beta, res or None, and a mask (a post-ReLU output:
    about half zeros) with 0.0, -0.0, -1.5 and 2^-126 planted at the flat positions 0..3.  relu: x is nudged until |t| > 16 et."""
    g = _g(rows, C, big, relu, res, 9)
    x = torch.randn(rows, C, generator=g) * (1.0 if big else 1.7) + (64.0 if big else 0.4)
    xd = x.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    mean, rstd = mean.float(), (var + f32(BN_EPS)).rsqrt().float()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    beta = torch.where(beta < 0, beta - 0.05, beta + 0.05)                  # rows == 1: t = beta
    gamma[0] = 0.0
    gamma[-1] = -gamma[-1].abs() - 0.1
    r = torch.randn(rows, C, generator=g) if res else None
    dy = torch.randn(rows, C, generator=g)
    mask = torch.randn(rows, C, generator=g).clamp(min=0)
    mask.view(-1)[:4] = torch.tensor([0.0, -0.0, -1.5, TINY])
    if relu:
        for _ in range(40):
            _, _, t, et = bn_apply(x.double(), mean.double(), rstd.double(), gamma.double(), beta.double(), None if r is None else r.double(), 0)
            bad = t.abs() <= 16 * et
            if not bool(bad.any()):
                break
            bump = 0.0625 * (1 + torch.rand(rows, C, generator=g))
            if r is not None:
                r = torch.where(bad, r + bump, r)
            else:
                x = torch.where(bad, x + bump, x)                           # gamma == 0: t = beta, never bad
        else:
            raise AssertionError("bn_inputs: could not move every t off the ReLU kink")
    return SimpleNamespace(x=x, dy=dy, mean=mean, rstd=rstd, gamma=gamma, beta=beta, res=r, mask=mask)


def bn_tail(t):
    return torch.cat([t, torch.full((BN_TAIL, t.shape[1]), 1.0e6, dtype=t.dtype)])


def bn_colreduce(mode, x, dy, mask, mean, rstd, n_part):
    """(partials [n_part, NOUT, C], bound) in fp64: the per-slab sums."""
    rows, C = x.shape
    rpb = -(-rows // n_part)
    if mode == 0:
        terms, depth = [x], [rpb]
    elif mode == 1:
        terms, depth = [(x - mean) ** 2], [rpb + 3]
    else:
        g = dy if mask is None else torch.where(mask > 0, dy, torch.zeros_like(dy))
        terms, depth = [g, g * ((x - mean) * rstd)], [rpb, rpb + 3]
    part = torch.zeros(n_part, len(terms), C, dtype=torch.float64)
    bound = torch.zeros_like(part)
    for p in range(n_part):
        sl = slice(min(rows, p * rpb), min(rows, (p + 1) * rpb))
        for k, (tm, dp) in enumerate(zip(terms, depth)):
            part[p, k] = tm[sl].sum(0)
            bound[p, k] = dp * U * tm[sl].abs().sum(0)
    return part, bound


def bn_sums(mode, x, dy, mask, mean, rstd, n_part):
    """The column sums after mage_sum_partials: (sums [NOUT, C], bound)."""
    part, b = bn_colreduce(mode, x, dy, mask, mean, rstd, n_part)
    return part.sum(0), b.sum(0) + n_part * U * part.abs().sum(0)


def bn_mean(x, n_part):
    """The mean of ops.bn_train_stats: the summed mode-0 partials divided by rows (u)."""
    s0, b0 = bn_sums(0, x, None, None, None, None, n_part)
    m = s0[0] / x.shape[0]
    return m, b0[0] / x.shape[0] + U * m.abs()


def bn_var_rstd(x, mean, n_part, eps=BN_EPS):
    """(var, b_var, rstd, b_rstd) about the fp32 mean the second pass was handed; rstd = rsqrt(var^ + eps): the add u V, the rsqrt one ulp (2 u)."""
    s1, b1 = bn_sums(1, x, None, None, mean, None, n_part)
    v = s1[0] / x.shape[0]
    bv = b1[0] / x.shape[0] + U * v
    V = v + f32(eps)
    return v, bv, V.rsqrt(), V.rsqrt() * ((bv + U * V) / (2 * V) + 2 * U)


def bn_apply(x, mean, rstd, gamma, beta, res, relu, kind="f32"):
    """-> (y, bound, t, et)."""
    p = (x - mean) * rstd * gamma
    t = p + beta
    et = 3 * U * p.abs() + U * t.abs()
    if res is not None:
        t = t + res
        et = et + U * t.abs()
    y, b = act_fwd(t, et, 1 if relu else 0)
    return y, b + store_err(y, kind), t, et


def bn_bwd_apply(x, dy, mask, mean, rstd, gamma, sums):
    rows = x.shape[0]
    g = dy if mask is None else torch.where(mask > 0, dy, torch.zeros_like(dy))
    xh = (x - mean) * rstd
    a1, a2 = sums[0] / rows, xh * sums[1] / rows
    dx = gamma * rstd * (g - a1 - a2)
    return dx, (gamma * rstd).abs() * (4 * U * a1.abs() + 7 * U * a2.abs() + 2 * U * g.abs()) + 2 * U * dx.abs()


# ------------------------------------------------------------------------------------------------ reparameterisation + KL
KL_N = (1, 63, 255, 256, 257, 1000)
KL_COEF = 0.37


def kl_inputs(B, n):
    """mu, logvar (uniform over [-20, 10], both ends present where n allows), eps, dz: [B, n]."""
    g = _g(B, n, 77)
    lv = torch.rand(B, n, generator=g) * 30 - 20
    if n >= 2:
        lv[:, 0], lv[:, -1] = -20.0, 10.0
    return SimpleNamespace(mu=torch.randn(B, n, generator=g) * 1.3, lv=lv, eps=torch.randn(B, n, generator=g), dz=torch.randn(B, n, generator=g))


def reparam_kl(mu, lv, eps):
    """-> (out, b_out, kl_sum [B], b_kl)."""
    n = mu.shape[1]
    a = eps * torch.exp(0.5 * lv)
    out = a + mu
    e = torch.exp(lv)
    term = 1 + lv - mu * mu - e
    et = U * ((1 + lv).abs() + mu * mu + (1 + lv - mu * mu).abs() + 2 * e + term.abs())
    kl = term.sum(1)
    return out, 3 * U * a.abs() + U * out.abs(), kl, et.sum(1) + n * D * term.abs().sum(1) + U * kl.abs()


def reparam_kl_bwd(mu, lv, eps, dz, coef):
    """coef: the fp32 device scalar, as a float.  -> (dmu, b_dmu, dlogvar, b_dlogvar)."""
    c = f32(coef)
    dmu = dz + c * mu
    e = torch.exp(lv)
    A = 0.5 * dz * eps * torch.exp(0.5 * lv)
    Bt = 0.5 * c * (1 - e)
    dlv = A - Bt
    return dmu, U * (c * mu).abs() + U * dmu.abs(), dlv, 4 * U * A.abs() + abs(0.5 * c) * (2 * U * e + U * (1 - e).abs()) + U * Bt.abs() + U * dlv.abs()


# ------------------------------------------------------------------------------------------------ MSE
MSE_CASES = ((1, 1, 1, 1), (7, 5, 8, 5), (33, 300, 304, 512), (300, 257, 260, 257))   # (rows, cols, lda, ldb)
MSE_GOUT = 0.83


def mse_inputs(rows, cols, lda, ldb):
    """a [rows, lda], b [rows, ldb] with 1e6 in the padding columns."""
    g = _g(rows, cols, lda, ldb)
    a, b = torch.full((rows, lda), 1.0e6), torch.full((rows, ldb), 1.0e6)
    a[:, :cols] = torch.randn(rows, cols, generator=g)
    b[:, :cols] = torch.randn(rows, cols, generator=g) * 0.5 + 0.1
    return a, b


def mse(a, b, cols):
    n = a.shape[0] * cols
    v = ((a[:, :cols] - b[:, :cols]) ** 2).mean()
    return v, (4 * U + (n + 2) * D) * v


def mse_bwd(a, b, cols, gout, ld_da):
    """-> (da [rows, ld_da], bound): zeros (bound 0) in the padding columns."""
    rows = a.shape[0]
    da = torch.zeros(rows, ld_da, dtype=torch.float64)
    da[:, :cols] = 2 * (a[:, :cols] - b[:, :cols]) / (rows * cols) * f32(gout)
    return da, 4 * U * da.abs()
