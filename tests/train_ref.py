"""fp64 restatements of six entry points of the decoder's backward pass (include/mage_hip.h; kernels in mage_amd/csrc/train.hip and
norm.hip) as closed formulas on their logical rows, with a per-element error bound for every output:
    mage_layernorm, mage_dropout_add_layernorm, mage_layernorm_bwd, mage_cross_entropy_bwd, mage_embedding_bwd, mage_group_rowsum,
    mage_row_sum.
The references take the exact values the kernels read (16-bit inputs converted from their stored bits).  Dropout masks are
keep(i) = hash32(seed * 0x9e3779b97f4a7c15 + i) >= (uint32)(p * 2^32), i = row * C + c, in uint64 wrap-around arithmetic, p the fp32 value,
kept scale the fp32 1 / (1 - p) (tests/sampling_ref.py hash32; as tests/attention_bwd_ref.py keep_scale builds it).

Bounds.  u = 2^-24, first order in u (one second-order term, em^2, is kept: a large mean makes it visible).  Figures used: an fp32
add, multiply, divide, sqrtf: relative u each (correctly rounded: no fast-math flag); a fused multiply-add rounds once, so a bound that
counts the product's rounding AND the add's holds with or without contraction; device expf 2 u; a fixed-order fp32 sum whose every term
passes through at most n additions: n u sum|terms|; a bf16 / f16 store: one ulp of the type at |ref| (tests/helpers.py ulp); a split
store: |ref| 2^-17 (bf16 pieces), |ref| 2^-21 + 2^-35 (f16 pieces), the representation error tests/test_gpu_split.py establishes.

LayerNorm statistics (layernorm_kernel, dropout_add_ln_kernel, layernorm_bwd_kernel: one wave per row, VPL = 1, 2, 4, 8 float4 per lane).
  A = mean_c |x_c|, d_c = x_c - mean, var = mean_c d_c^2, V = var + eps, rstd = V^-1/2.
  mean:  a lane adds VPL times ((v0 + v1) + (v2 + v3)) onto its sum: VPL + 2 additions above any element; the butterfly 6 more; one
         divide by (float)C (exact):              |mean^ - mean| <= em = (VPL + 9) u A.
  t_c = x_c - mean^:                              |t^_c - d_c| <= em + u |d_c|.
  sum t^2: with e = mean - mean^ (ONE number for the whole row) sum_c (d_c + e)^2 = sum d^2 + C e^2 exactly, because sum_c d_c = 0 by the
         definition of mean: the shift enters V at second order only, as em^2 (kept: at mean 64 it is not negligible against u var).
         First order: the rounding of t 2 u var, the product 1, 4 VPL sequential terms per lane and the butterfly 4 VPL + 6 additions,
         the divide by C 1, the add of eps u V:
                                                  |V^ - V| <= eV = (4 VPL + 10) u var + em^2 + u V.
  rstd = 1 / sqrtf(V^): two correctly rounded operations:  relative er = eV / (2 V) + 2 u.
LayerNorm output y_c = (t_c rstd) g_c + b_c: the error of t, (er + 2 u) on the two multiplies, u on the product before the add and u on the add:
                                                  |err y_c| <= rstd |g_c| (em + |d_c| (er + 3 u)) + u |y_c|.
  Leading term on a large-mean row: (VPL + 9) u mean|x| rstd |g|.  A one-pass variance E[x^2] - mean^2 errs by ~ u C-term-sum mean^2 in V: a
  relative u mean^2 / var in rstd, (mean / sd) times the leading term and more -- outside this bound at mean 64, sd 1
  (tests/test_train_ref_cpu.py).
LayerNorm backward, g_c = dy_c gamma_c, xh_c = d_c rstd, mg = mean_c g_c, mgx = mean_c g_c xh_c, dx_c = rstd (g_c - mg - xh_c mgx):
  xh:   |err xh_c| <= exh_c = rstd (em + u |d_c|) + |xh_c| (er + u).
  mg:   products u, 4 VPL + 6 additions, the divide:      emg  = (4 VPL + 8) u mean|g|.
  mgx:  the same with the product g xh (u more) and exh:   emgx = (4 VPL + 9) u mean|g xh| + mean(|g| exh).
  dx:   the inner difference g - mg - xh mgx: u |g| (g's product), emg, exh |mgx| + |xh| emgx, and three roundings (a product, two
        subtractions) each below u (|g| + |mg| + |xh mgx|); then rstd (er) and the last multiply (u):
        |err dx_c| <= rstd (emg + exh_c |mgx| + |xh_c| emgx + 4 u (|g_c| + |mg| + |xh_c mgx|)) + |dx_c| (er + u);
        accumulate: + u |start + dx| for the one add.
  dgamma_c = sum_rows dy xh, dbeta_c = sum_rows dy: a wave adds its rw = ceil(rows / (4 n_part)) rows in order, four waves are added as
        (w0 + w1) + (w2 + w3) (2), mage_sum_partials adds n_part rows (at most n_part additions above any term):
        |err dgamma_c| <= sum_rows |dy| exh + (rw + n_part + 3) u sum_rows |dy xh|,   |err dbeta_c| <= (rw + n_part + 2) u sum_rows |dy|.
Cross entropy backward, one wave per row: a_k = |l_k - max|, w_k = exp(l_k - max), s = sum w, P_k = w_k / s, out = (P_k - [k == target]) sc,
  sc = grad_out / rows:  the subtraction moves the exponent by u a_k, expf 2 u: relative (a_k + 2) u in w_k; s adds ceil(K / 64) terms per
  lane and the butterfly: (ceil(K / 64) + 6) u, and carries the w errors: sum_j P_j (a_j + 2) u; 1 / s u; the multiply u; the
  subtraction of the one-hot u |P_k - 1|; sc = grad_out * (1 / rows): 2 u, the last multiply u:
        |err| <= sc (P_k ((a_k + ceil(K / 64) + 10) u + sum_j P_j (a_j + 2) u) + u |P_k - hot|) + 3 u |out| + sc 2^-125
  (the last term: a weight below the normal range, 2^-126, may be flushed or lose bits; P_k = 0 exactly at -inf logits: a_k counts as 0).
  Targets outside [0, K) have no one-hot (the forward kernel reports them).
Embedding backward: dtable[id] = start + sum of the rows with that id (padding_idx and ids outside [0, n_table) contribute nothing).  Any
  order of count(id) additions (chunk sums start from an exact 0; their flush is one addition each):  count u (|start| + sum|terms|).
  The deterministic form is also checked bit for bit against embedding_det_f32: the float32 sum in the order the header states.
Grouped row sums, per chunk at most per = ceil(nper div / n_chunk) sequential terms w(r) x (product rounding 1): (per + 1) u sum|w x| over all
  chunks.  Row sums: a lane adds ceil(per / 64) terms, the butterfly 6: (ceil(per / 64) + 6) u sum|x|, per = the 8-rounded chunk width.
No constant here is fitted to a kernel's output."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers import ulp
from tests.sampling_ref import GOLDEN_GAMMA, hash32

U = 2.0 ** -24
LN_C = (4, 252, 256, 260, 512, 516, 1024, 1028, 2044, 2048)             # both sides of every step of the VPL ladder, ragged inside every VPL
P_MAX = float(np.nextafter(np.float32(1), np.float32(0)))                # the largest float below 1


def vpl(C):
    return 1 if C <= 256 else 2 if C <= 512 else 4 if C <= 1024 else 8


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ dropout
def keep_mask(rows, C, p, seed):
    """keep[row, c] (bool) of the module docstring."""
    thresh = np.uint64(int(f32(p) * 4294967296.0))
    idx = np.arange(rows * C, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = np.array([seed & (2 ** 64 - 1)], dtype=np.uint64) * GOLDEN_GAMMA + idx
    return torch.from_numpy((hash32(ctr) >= thresh).reshape(rows, C))


def inv_keep(p):
    """The fp32 1 / (1 - p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_add_exact(x, r, keep, ik):
    """(unfused, fused): the two float32 values of r + x * ik at kept elements (r at dropped ones): product rounded then added, and one
    fused multiply-add.  x, r: float32 tensors (x already widened from its stored bits)."""
    xn, rn, k = x.numpy().astype(np.float32), r.numpy().astype(np.float32), keep.numpy()
    unf = np.where(k, rn + xn * np.float32(ik), rn).astype(np.float32)
    p = xn.astype(np.float64) * float(ik)                                   # exact: 24 + 24 significand bits
    rd = rn.astype(np.float64)
    s = p + rd
    bb = s - p
    e = (p - (s - bb)) + (rd - bb)                                          # TwoSum: p + r = s + e exactly
    cand = s.astype(np.float32)
    d = s - cand.astype(np.float64)                                         # exact
    up = np.nextafter(cand, np.float32(np.inf))
    dn = np.nextafter(cand, np.float32(-np.inf))
    half = np.where(d > 0, (up.astype(np.float64) - cand) / 2, (cand - dn.astype(np.float64)) / 2)
    tie = (d != 0) & (np.abs(d) == half) & (e != 0) & (np.sign(e) == np.sign(d))   # fp64 rounded onto an fp32 midpoint the sum is beyond
    fused = np.where(tie, np.where(d > 0, up, dn), cand)
    fused = np.where(k, fused, rn).astype(np.float32)
    return torch.from_numpy(unf), torch.from_numpy(fused)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_inputs(C, rows, seed, special=None):
    """x [rows, C] fp32 with row 0 constant at 0.5 and the last row ~ N(64, 1) (rows == 1: special = 'const' | 'mean'); gamma with an
    exact 0 and a negative entry; beta."""
    g = torch.Generator().manual_seed(seed * 10007 + C * 13 + rows)
    x = torch.randn(rows, C, generator=g) * 2 + 0.3
    big = torch.randn(C, generator=g) + 64
    if rows > 1 or special == "mean":
        x[rows - 1] = big
    if rows > 1 or special == "const":
        x[0] = 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gamma[0], gamma[1] = 0.0, -gamma[1].abs() - 0.1
    return x, gamma, beta


def ln_stats(x, eps, C):
    """fp64 statistics of the rows of x [rows, C] with the error terms of the module docstring."""
    eps = f32(eps)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    V = var + eps
    rstd = V.rsqrt()
    v = vpl(C)
    em = (v + 9) * U * x.abs().mean(-1, keepdim=True)
    eV = (4 * v + 10) * U * var + em * em + U * V
    return SimpleNamespace(mean=mean, d=d, var=var, rstd=rstd, em=em, er=eV / (2 * V) + 2 * U, xh=d * rstd)


def store_err(ref, kind):
    """The error a store of kind 'f32' | 'bf16' | 'f16' | 'bf16x3' | 'f16x3' adds at |ref|."""
    if kind == "f32":
        return torch.zeros_like(ref)
    if kind == "bf16":
        return ulp(ref, torch.bfloat16)
    if kind == "f16":
        return ulp(ref, torch.float16)
    if kind == "bf16x3":
        return ref.abs() * 2.0 ** -17
    assert kind == "f16x3"
    return ref.abs() * 2.0 ** -21 + 2.0 ** -35


def layernorm(x, gamma, beta, eps, kind="f32"):
    """(y, bound) in fp64 for x [rows, C], gamma, beta [C] (fp64 of the values read)."""
    C = x.shape[-1]
    s = ln_stats(x, eps, C)
    y = s.xh * gamma + beta
    b = s.rstd * gamma.abs() * (s.em + s.d.abs() * (s.er + 3 * U)) + U * y.abs()
    return y, b + store_err(y, kind)


def layernorm_bwd(x, gamma, dy, eps, n_part, start=None):
    """dx (+ start), dgamma, dbeta in fp64 and their bounds: SimpleNamespace(dx, dg, db, b_dx, b_dg, b_db)."""
    rows, C = x.shape
    s = ln_stats(x, eps, C)
    v = vpl(C)
    g = dy * gamma
    xh = s.xh
    mg, mgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dx = s.rstd * (g - mg - xh * mgx)
    exh = s.rstd * (s.em + U * s.d.abs()) + xh.abs() * (s.er + U)
    emg = (4 * v + 8) * U * g.abs().mean(-1, keepdim=True)
    emgx = (4 * v + 9) * U * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * exh).mean(-1, keepdim=True)
    b_dx = s.rstd * (emg + exh * mgx.abs() + xh.abs() * emgx + 4 * U * (g.abs() + mg.abs() + (xh * mgx).abs())) + dx.abs() * (s.er + U)
    if start is not None:
        dx = dx + start
        b_dx = b_dx + U * dx.abs()
    rw = -(-rows // (4 * n_part))
    b_dg = (dy.abs() * exh).sum(0) + (rw + n_part + 3) * U * (dy * xh).abs().sum(0)
    b_db = (rw + n_part + 2) * U * dy.abs().sum(0)
    return SimpleNamespace(dx=dx, dg=(dy * xh).sum(0), db=dy.sum(0), b_dx=b_dx, b_dg=b_dg, b_db=b_db)


# ------------------------------------------------------------------------------------------------ cross entropy backward
CE_SHAPES = ((1, 1), (5, 63), (4, 64), (7, 65), (3, 512), (6, 1000))
CE_GRAD_OUT = 0.7


def ce_inputs(rows, K):
    """logits [rows, K] fp32 (row 1: +-80; row 2: some -inf), targets cycling through 0, K - 1, -1, K and a random code."""
    g = torch.Generator().manual_seed(rows * 1009 + K)
    z = torch.randn(rows, K, generator=g) * 3
    tg = torch.randint(0, K, (rows,), generator=g)
    special = [0, K - 1, -1, K]
    for i in range(rows):
        if i < 4:
            tg[i] = special[i]
    if rows > 1:
        z[1] = torch.where(torch.arange(K) % 2 == 0, 80.0, -80.0)
    if rows > 2 and K > 3:
        z[2, 1::3] = float("-inf")                                          # never column 0 or K - 1 ... the target of row 2 is -1 anyway
    return z, tg.long()


def cross_entropy_bwd(z, tg, grad_out, kind="f32"):
    """(dlogits, bound) in fp64; z fp64 [rows, K], tg int64 [rows]."""
    rows, K = z.shape
    sc = f32(grad_out) / rows
    mx = z.amax(-1, keepdim=True)
    P = torch.softmax(z, -1)
    a = torch.where(torch.isinf(z), torch.zeros_like(z), (z - mx).abs())
    hot = (torch.arange(K)[None, :] == tg[:, None]).double()                # no column matches a target outside [0, K)
    out = (P - hot) * sc
    n = -(-K // 64)
    b = sc * (P * ((a + n + 10) * U + (P * (a + 2)).sum(-1, keepdim=True) * U) + U * (P - hot).abs()) + 3 * U * out.abs() + sc * 2.0 ** -125
    return out, b + store_err(out, kind)


# ------------------------------------------------------------------------------------------------ embedding backward
def emb_inputs(n, n_table, C, dt, grouped, pad=3):
    """ids [n] (a hot code every 7th row; padding_idx, -3 and n_table among them), dout (extra rows under the grouped map hold 1e6),
    the start of dtable, and the row map orow [n]."""
    g = torch.Generator().manual_seed(n * 31 + n_table * 7 + C + grouped)
    ids = torch.randint(0, n_table, (n,), generator=g)
    hot = n_table // 2
    ids[::7] = hot
    pad = pad if n_table > pad else -1                                       # a one-row table: no padding code
    for k, v in ((3, pad), (5, -3), (6, n_table)):
        ids[k::11] = v
    group, stride, off = (5, 9, 2) if grouped else (n, n, 0)
    i = torch.arange(n)
    orow = (i // group) * stride + i % group + off
    d_rows = int(orow.max()) + 1 + (3 if grouped else 0)
    dout = torch.full((d_rows, C), 1.0e6)
    dout[orow] = torch.randn(n, C, generator=g)
    start = torch.randn(n_table, C, generator=g) + 0.25
    return ids.long(), dout.to(dt), start, orow, (group, stride, off), pad


def emb_valid(ids, n_table, pad):
    return (ids >= 0) & (ids < n_table) & (ids != pad)


def embedding_bwd(ids, rows_read, start, n_table, pad):
    """(dtable, bound) in fp64; rows_read [n, C] fp64: dout at the mapped rows."""
    ok = emb_valid(ids, n_table, pad)
    tab, mag = start.clone(), start.abs().clone()
    tab.index_add_(0, ids[ok], rows_read[ok])
    mag.index_add_(0, ids[ok], rows_read[ok].abs())
    cnt = torch.bincount(ids[ok], minlength=n_table).double()
    return tab, cnt[:, None] * U * mag


def emb_chunks(n):
    """(n_chunk, rows per chunk) as include/mage_hip.h states them: min(64, ceil(n / 4096)) chunks of ceil(n / n_chunk) rows rounded up to 8."""
    n_chunk = min(64, -(-n // 4096))
    return n_chunk, (-(-n // n_chunk) + 7) // 8 * 8


def embedding_det_f32(ids, rows_read, start, n_table, pad):
    """The float32 sum of the deterministic form: rows ascending inside a chunk from 0, chunks ascending onto the start."""
    n = ids.numel()
    n_chunk, rpc = emb_chunks(n)
    ok = emb_valid(ids, n_table, pad).numpy()
    idn, src = ids.numpy(), rows_read.numpy().astype(np.float32)
    out = start.numpy().astype(np.float32).copy()
    for c in range(n_chunk):
        part = np.zeros_like(out)
        for i in range(c * rpc, min(n, (c + 1) * rpc)):
            if ok[i]:
                part[idn[i]] += src[i]
        out += part
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ grouped row sums, row sums
GROUP_CASES = ((3 * 5 * 16, 64, 16, 5, False), (3 * 5 * 16 - 7, 72, 16, 5, False), (100, 260, 1, 7, False), (37, 8, 4, 1, True), (5, 4, 1, 1, False))


def group_inputs(rows, C, div, mod, scaled, dt):
    g = torch.Generator().manual_seed(rows * 17 + C)
    x = torch.randn(rows, C, generator=g).to(dt)
    rs = torch.randn(-(-rows // 4), generator=g) if scaled else None
    return x, rs


def group_rowsum(x, rows, div, mod, rs, rs_div, n_chunk):
    """(out [mod, C], bound) in fp64 for x fp64 [rows, C]."""
    r = torch.arange(rows)
    w = rs[r // rs_div] if rs is not None else torch.ones(rows, dtype=torch.float64)
    t = x * w[:, None]
    gidx = (r // div) % mod
    out = torch.zeros(mod, x.shape[1], dtype=torch.float64).index_add_(0, gidx, t)
    mag = torch.zeros(mod, x.shape[1], dtype=torch.float64).index_add_(0, gidx, t.abs())
    nper = -(-rows // (div * mod))
    per = -(-nper * div // n_chunk)
    return out, (per + 1) * U * mag


def row_chunk(n, n_chunk):
    """The chunk width of mage_row_sum: ceil(n / n_chunk) rounded up to 8."""
    return (-(-n // n_chunk) + 7) // 8 * 8


def row_sum(x, n, n_chunk):
    """(out [rows], bound) in fp64 for x fp64 [rows, ld]: the first n columns."""
    per = row_chunk(n, n_chunk)
    return x[:, :n].sum(1), (-(-per // 64) + 6) * U * x[:, :n].abs().sum(1)
