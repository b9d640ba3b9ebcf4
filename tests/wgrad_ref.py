"""fp64 restatements of nine entry points of the training path (include/mage_hip.h; kernels in mage_amd/csrc/train.hip, optim.hip,
gemm_tn.hip, gemm4.hip), written from the header's words, with a per-element error bound for every output:
    mage_transpose, mage_transpose_colsum, mage_gemm_tn, mage_colsum, mage_sum_partials, mage_act, mage_act_bwd,
    mage_dropout / mage_dropout_add (mask and exact values: tests/train_ref.py keep_mask, inv_keep, dropout_add_exact), mage_adam.
The references take the exact values the kernels read: 16-bit inputs from their stored bits, the fp32-rounded lr, beta1, beta2, eps,
grad_scale, p, and the fp32 literal 1.702f.  The case tables and the input builders that tests/test_wgrad_ref_cpu.py and
tests/test_gpu_wgrad_kernels.py share are here too.  Nothing is imported from mage_amd.ops.

Bounds.  u = 2^-24, first order in u.  Figures (tests/train_ref.py): an fp32 add, multiply, divide, sqrtf: relative u each (a fused
multiply-add rounds once, so a bound that counts the product's rounding AND the add's holds with or without contraction); device expf 2 u; a
fixed-order fp32 sum whose every term passes through at most n additions: n u sum|terms|; a bf16 store: one ulp of the type.  From
tests/test_gpu_gemm.py: an MFMA accumulation of n exact bf16 products: 2 u n sum|a||w| (how the 16-bit MFMAs round inside is not stated, so 2 u
per accumulated term is allowed); erff ASSUMED within 4 ulp, 8 u absolute, which with its argument's two roundings (the product and the
constant, each moving erf by < u / 2) is 10 u: erf-GELU forward 0.5 v (1 + erff(.)) keeps bound_fp32's figure 10 u |v|.  TINY = 2^-126:
a result or an intermediate below the normal range may be flushed or lose bits.

mage_transpose: data movement; bits are compared, no bound.
mage_transpose_colsum: colsum[p][c] adds the rows of 16 tiles of 64; a thread adds the 8 rows of its chunk per tile in order, at most 16 * 8 =
  128 terms, the 8 threads of a channel meet in 3 shuffles:          |err| <= (8 tiles_p + 3) u sum|x|,  tiles_p <= 16 the tiles of part p.
mage_gemm_tn: slice s holds t_s tokens:                                |err P| <= 2 u t_s sum_t |dy x|,   |err db| <= 2 u t_s sum_t |dy|
  (db: v_dot2 adds two tokens per instruction, 4 per 32-token step, then 2 shuffles: fewer than 2 t_s roundings above any term).  An empty
  slice: exactly 0.
mage_colsum: chunk p holds per = ceil(T / n_part) rows; a wave adds every fourth, ceil(per / 4) terms, the four waves meet as (w0 + w1) +
  (w2 + w3):                                                           |err| <= (ceil(per / 4) + 2) u sum|x|.
mage_sum_partials: the scalar kernel adds the n_part rows in order onto the start (or 0): n_part additions above any term; the 16-byte
  kernel's waves add ceil(n_part / 4) rows each, meet as (s0 + s1) + (s2 + s3), then the start: ceil(n_part / 4) + 3 <= n_part for
  n_part >= 4, the only n_part it runs at:                             |err| <= n_part u (|start| + sum|part|).
  Both are also checked bit for bit against the float32 sum in that order (sum_partials_f32).
mage_act, c = fl(1.702), s = 1 / (1 + e), e = exp(-c v):
  ReLU: exact.
  QuickGELU v / (1 + expf(-c v)): the product c v u |c v| absolute, which exp turns into relative; expf 2 u: e relative (|c v| + 2) u; 1 + e:
    relative (1 - s) (|c v| + 2) u + u (1 - s = e / (1 + e)); the divide u:
                                                                       |err| <= |y| u ((1 - s) (|c v| + 2) + 2) + FLOOR
    FLOOR = TINY + |v| 2^-128: where expf overflows (e > 2^128) the kernel returns 0 for |v| / (1 + e) < |v| 2^-128.
  erf-GELU: 10 u |v| + TINY (above).
mage_act_bwd, dx = dy D:
  ReLU: exact.   tanh, D = 1 - y^2: the square u y^2, the subtraction u |D|, the product u:    |dy| u (y^2 + |D|) + u |dx| + TINY.
  QuickGELU, D = s (1 + w q), w = c v, q = 1 - s: s relative es = u ((1 - s)(|c v| + 2) + 2) (as above); q absolute s es + u q; w u; the
    product w q: |w| (s es + u q) + 2 u |w| q; r = 1 + w q: that + u |r|; D = s r: |r| s es + s err(r) + u |D|; dx: u |dx| more:
        |err| <= |dy| (s (|w| (s es + u q) + 2 u |w| q + u |r|) + |r| s es + u |D|) + u |dx| + TINY (1 + |dy|) + |dy| 2^-128 (1 + |w|).
  erf-GELU, D = A + B, A = 0.5 (1 + erff(.)): 5 u + u A; B = v k exp(-v^2 / 2), k = fl(1 / sqrt(2 pi)): the exponent's product 0.5 v^2 u,
    expf 2 u, k's rounding, v k, the last product 1 each: |B| (0.5 v^2 + 5) u; the sum u |D|; dx u |dx|:
        |err| <= |dy| (5 u + u A + |B| (0.5 v^2 + 5) u + u |D|) + u |dx| + TINY (1 + |dy| (1 + |v|)).
  bf16: the fp32 bound e plus ulp_bf16(|ref| + e): a bf16 rounding that may fall the other way.
mage_adam, ge = g grad_scale, hyperparameters as fp32 values, one step from the state the kernel read:
  m' = b1 m + (1 - b1) ge: u |b1 m|; (1 - b1), ge and the product 3 u; the add u |m'|:    em = u (|b1 m| + 3 |(1 - b1) ge| + |m'|) + TINY.
  v' = b2 v + ((1 - b2) ge) ge: 5 roundings on the second term:                             ev = u (b2 v + 5 (1 - b2) ge^2 + v') + TINY
    (TINY: ge^2 underflows at g = 1e-30).
  bias corrections on the host: bc1 = 1 - powf(b1, t): powf 2 u on b1^t, the subtraction u: relative rb1 = (2 u b1^t + u) / (1 - b1^t);
    bc2s = sqrtf(1 - powf(b2, t)): rb2 = (2 u b2^t + u) / (2 (1 - b2^t)) + u.
  p' = p - (lr / bc1) (m' / (sqrtf(v') / bc2s + eps)):  sq = sqrt(v'): |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt|a - b|), + u sq;
    q = sq / bc2s: err(sq) / bc2s + q (rb2 + u); den = q + eps: + u den; r = m' / den: em / den + |r| (err(den) / den + u);
    upd = (lr / bc1) r: (lr / bc1) err(r) + |upd| (rb1 + 2 u); the subtraction u |p'|.
No constant here is fitted to a kernel's output."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers import ulp
from tests.train_ref import P_MAX, U, f32

TINY = 2.0 ** -126
GOLD = 0x9E3779B97F4A7C15
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
IDT = {"f32": torch.int32, "bf16": torch.int16}
# -0.0, a quiet NaN with a payload, +inf, -inf, the smallest subnormal: as integer bit patterns of the type
SPECIAL_BITS = {"f32": (-2 ** 31, 0x7FC12345, 0x7F800000, 0xFF800000 - 2 ** 32, 1), "bf16": (-2 ** 15, 0x7FC5, 0x7F80, 0xFF80 - 2 ** 16, 1)}


def cdiv(a, b):
    return -(-a // b)


def ratio(got, ref, bound):
    """The largest |got - ref| / bound over all elements (inf for a non-finite got); 0 / 0 counts as 0."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def bf16_bound(ref, e):
    return e + ulp(ref.abs() + e, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ mage_transpose
def gather_rows(M, out_h=1, out_w=None, in_h=None, in_w=None, img_stride=None, a_off=0, dy=0, dx=0, stride=1):
    """(row [M], inside [M]): the row of x that output column m reads, and whether its pixel lies inside the in_h x in_w plane."""
    out_w = M if out_w is None else out_w
    in_h = out_h if in_h is None else in_h
    in_w = out_w if in_w is None else in_w
    img_stride = in_h * in_w if img_stride is None else img_stride
    m = torch.arange(M)
    img, rem = m // (out_h * out_w), m % (out_h * out_w)
    oy, ox = rem // out_w, rem % out_w
    iy, ix = oy * stride + dy, ox * stride + dx
    inside = (iy >= 0) & (iy < in_h) & (ix >= 0) & (ix < in_w)
    row = img * img_stride + iy * in_w + ix + a_off
    return torch.where(inside, row, torch.zeros_like(row)), inside


def transpose(x, M, Mp, C, **geo):
    """y [C, Mp] of x [rows, ldx] (any dtype, integer bit patterns included): y[c, m] = x[arow(m), c], 0 outside the plane and for m >= M."""
    row, inside = gather_rows(M, **geo)
    g = x[row, :C].clone()
    g[~inside] = 0
    y = torch.zeros(C, Mp, dtype=x.dtype)
    y[:, :M] = g.t()
    return y


def planted(shape, dt, seed, specials=(0, 1, 2, 3, 4)):
    """Random bits of dtype dt ('f32' | 'bf16') as an integer tensor, the chosen SPECIAL_BITS in row 0 and in the last row."""
    g = torch.Generator().manual_seed(seed)
    b = (torch.randn(shape, generator=g) * torch.exp(2 * torch.randn(shape, generator=g))).to(TDT[dt]).view(IDT[dt]).clone()   # several decades: sums round
    for k, i in enumerate(specials):
        b[0, k % shape[1]] = SPECIAL_BITS[dt][i]
        b[-1, shape[1] - 1 - k % shape[1]] = SPECIAL_BITS[dt][i]
    return b


def tcase(name, dt, C, M, Mp, calls=None, ldx=None, ldy=None, x_off=0, y_off=0, x_rows=None):
    """calls: [(y_row0, geo)] written into ONE y buffer.  x_off / y_off: elements by which the base pointers are moved off 16-byte alignment."""
    calls = [(0, {})] if calls is None else calls
    ldx, ldy = C if ldx is None else ldx, Mp if ldy is None else ldy
    if x_rows is None:
        x_rows = max(int(gather_rows(M, **geo)[0].max()) for _, geo in calls) + 1
    t8 = dt == "bf16" and C % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0 and Mp % 8 == 0 and x_off % 8 == 0 and y_off % 8 == 0
    return SimpleNamespace(name=name, dt=dt, C=C, M=M, Mp=Mp, calls=calls, ldx=ldx, ldy=ldy, x_off=x_off, y_off=y_off, x_rows=x_rows,
                           kernel="transpose8_kernel" if t8 else "transpose_kernel<%s>" % ("bf16" if dt == "bf16" else "float"))


TAPS3 = [(t, dict(out_h=3, out_w=5, in_h=3, in_w=5, img_stride=15, dy=t // 3 - 1, dx=t % 3 - 1)) for t in range(9)]
TAPS4 = [(t, dict(out_h=3, out_w=5, in_h=6, in_w=10, img_stride=60, dy=t // 4 - 1, dx=t % 4 - 1, stride=2)) for t in range(16)]
REGROUP = dict(out_w=10, img_stride=15, a_off=5)                            # x[:, 1:] of [B, L = 3, hw = 5] rows


def transpose_cases():
    out = []
    for dt in ("f32", "bf16"):
        for C in (8, 12, 64, 72):
            for M, Mp in ((1, 8), (63, 64), (64, 64), (65, 72), (65, 128)):
                out.append(tcase(f"{dt}_C{C}_M{M}_Mp{Mp}", dt, C, M, Mp))
        out.append(tcase(f"{dt}_M1_Mp1", dt, 8, 1, 1))
        out.append(tcase(f"{dt}_row0_ldy", dt, 72, 65, 72, calls=[(5, {})], ldy=80))
        out.append(tcase(f"{dt}_regroup", dt, 8, 20, 24, calls=[(0, REGROUP)], x_rows=30))
        out.append(tcase(f"{dt}_taps3x3", dt, 8, 30, 32, calls=[(t * 8, g) for t, g in TAPS3], x_rows=30))
        out.append(tcase(f"{dt}_taps4x4_s2", dt, 8, 30, 32, calls=[(t * 8, g) for t, g in TAPS4], x_rows=120))
    out.append(tcase("bf16_taps4x4_s2_C12", "bf16", 12, 30, 30, calls=[(t * 12, g) for t, g in TAPS4], x_rows=120))
    out.append(tcase("bf16_fallback_ldx", "bf16", 64, 65, 72, ldx=68))
    out.append(tcase("bf16_fallback_ldy", "bf16", 64, 65, 72, ldy=76))
    out.append(tcase("bf16_fallback_Mp", "bf16", 64, 65, 68, ldy=72))
    out.append(tcase("bf16_fallback_x_off", "bf16", 64, 65, 72, x_off=1))
    out.append(tcase("bf16_fallback_y_off", "bf16", 64, 65, 72, y_off=1))
    return out


TRANSPOSE_CASES = transpose_cases()
Y_SPARE = 3                                                                  # sentinel rows after the last written one


def transpose_inputs(c):
    return planted((c.x_rows, c.ldx), c.dt, c.C * 131 + c.M)


def transpose_expected(c, xb, fill):
    """The whole y buffer [rows, ldy] as bits: `fill` (the sentinel's bits) wherever no call writes."""
    rows = max(r0 for r0, _ in c.calls) + c.C + Y_SPARE
    y = torch.full((rows, c.ldy), fill, dtype=xb.dtype)
    for r0, geo in c.calls:
        y[r0:r0 + c.C, :c.Mp] = transpose(xb, c.M, c.Mp, c.C, **geo)
    return y


# ------------------------------------------------------------------------------------------------ mage_transpose_colsum
TC_CASES = [SimpleNamespace(name=f"C{C}_Mp{Mp}_M{M}", C=C, M=M, Mp=Mp, geo={}, x_rows=M) for C in (8, 72) for Mp in (64, 1024, 1032) for M in (Mp, Mp - 7)]
TC_CASES.append(SimpleNamespace(name="regroup", C=8, M=1030, Mp=1032, geo=dict(REGROUP), x_rows=1545))


def tc_n_part(Mp):
    return cdiv(cdiv(Mp, 64), 16)


def tc_inputs(c):
    return planted((c.x_rows, c.C), "bf16", c.C * 7 + c.M, specials=(0, 4))   # finite values only: they are summed


def transpose_colsum(x, M, Mp, C, **geo):
    """(colsum [n_part, C], bound) in fp64 for x fp64 [rows, ldx]."""
    g = transpose(x, M, Mp, C, **geo).t()                                   # [Mp, C], zero rows from M on
    n_part = tc_n_part(Mp)
    s, b = torch.zeros(n_part, C, dtype=torch.float64), torch.zeros(n_part, C, dtype=torch.float64)
    for p in range(n_part):
        rows = g[p * 1024:min(Mp, (p + 1) * 1024)]
        tiles = cdiv(rows.shape[0], 64)
        s[p], b[p] = rows.sum(0), (8 * tiles + 3) * U * rows.abs().sum(0)
    return s, b


# ------------------------------------------------------------------------------------------------ mage_gemm_tn
GEMM_NK = ((256, 256), (512, 256), (256, 512))
GEMM_8W = ((1, 64, 1), (63, 64, 1), (64, 64, 1), (65, 64, 2), (64, 64, 3), (192, 128, 2))      # (T, tokens_per_split, n_split)
GEMM_4W = ((128, 128, 1), (256, 128, 2), (320, 192, 2))
GUARD = 64


def gemm_4w(T, tps, n_split):
    """The host condition of the one-wave-per-SIMD kernel: whole 64-token slabs, at least two in every slice."""
    return T % 64 == 0 and tps % 64 == 0 and tps >= 128 and T - (n_split - 1) * tps >= 128


def gemm_inputs(T, N, K, pad=0):
    """dy [T + GUARD, N + pad], x [T + GUARD, K + pad] bf16: NaN in the guard rows after row T - 1, 1e4 in the padding columns."""
    g = torch.Generator().manual_seed(T * 13 + N + 3 * K)
    dy, x = torch.randn(T + GUARD, N + pad, generator=g), torch.randn(T + GUARD, K + pad, generator=g)
    dy[:, N:], x[:, K:] = 1.0e4, 1.0e4
    dy[T:], x[T:] = float("nan"), float("nan")
    return dy.bfloat16(), x.bfloat16()


def gemm_tn(dy, x, T, tps, n_split):
    """P [n_split, N, K], db [n_split, N] and their bounds in fp64 for dy [>= T, N], x [>= T, K] fp64."""
    N, K = dy.shape[1], x.shape[1]
    P, bP = torch.zeros(n_split, N, K, dtype=torch.float64), torch.zeros(n_split, N, K, dtype=torch.float64)
    db, bdb = torch.zeros(n_split, N, dtype=torch.float64), torch.zeros(n_split, N, dtype=torch.float64)
    for s in range(n_split):
        t0, t1 = s * tps, min(T, (s + 1) * tps)
        if t1 <= t0:
            continue
        a, b = dy[t0:t1], x[t0:t1]
        P[s], bP[s] = a.t() @ b, 2 * U * (t1 - t0) * (a.abs().t() @ b.abs())
        db[s], bdb[s] = a.sum(0), 2 * U * (t1 - t0) * a.abs().sum(0)
    return SimpleNamespace(P=P, bP=bP, db=db, bdb=bdb)


# ------------------------------------------------------------------------------------------------ mage_colsum
COLSUM_CASES = [(C, T, 1) for C in (8, 512, 520) for T in (1, 3, 4, 5, 16, 17, 67)] + [(C, 10, 3) for C in (8, 512, 520)] + [(C, 3, 5) for C in (8, 512, 520)]


def colsum_inputs(C, T):
    """x [T + 4, C + 8] bf16: NaN in the rows after T - 1, 1e4 in the gap columns."""
    g = torch.Generator().manual_seed(C + 31 * T)
    x = torch.randn(T + 4, C + 8, generator=g) * torch.exp(2 * torch.randn(T + 4, C + 8, generator=g))      # several decades: the sums round
    x[:, C:] = 1.0e4
    x[T:] = float("nan")
    return x.bfloat16()


def colsum(x, T, n_part):
    """(partials [n_part, C], bound) in fp64 for x fp64 [>= T, C]."""
    C, per = x.shape[1], cdiv(T, n_part)
    s, b = torch.zeros(n_part, C, dtype=torch.float64), torch.zeros(n_part, C, dtype=torch.float64)
    for p in range(n_part):
        rows = x[min(T, p * per):min(T, (p + 1) * per)]
        s[p], b[p] = rows.sum(0), (cdiv(per, 4) + 2) * U * rows.abs().sum(0)
    return s, b


# ------------------------------------------------------------------------------------------------ mage_sum_partials
SP_NPART = (1, 3, 4, 5, 13, 16, 17, 20)
SP_N = (4, 250, 252, 260)
SP_EXTRA = (dict(n=252, stride=260, out_off=0), dict(n=252, stride=254, out_off=0), dict(n=252, stride=252, out_off=1))


def sp_vector(n, stride, n_part, out_off):
    """The host condition of sum_partials4_kernel."""
    return n % 4 == 0 and stride % 4 == 0 and n_part >= 4 and out_off % 4 == 0


def sp_inputs(n, stride, n_part):
    """part [n_part, stride] fp32 with values over six decades (1e6 in the gap columns from n on) and a start vector [n]."""
    g = torch.Generator().manual_seed(n * 100 + stride + n_part)
    part = torch.randn(n_part, stride, generator=g) * torch.exp(torch.randn(n_part, stride, generator=g) * 3)
    part[:, n:] = 1.0e6
    return part, torch.randn(n, generator=g) * 10


def sum_partials(part, n, start=None):
    """(out [n], bound) in fp64 for part fp64 [n_part, >= n]."""
    s, mag = part[:, :n].sum(0), part[:, :n].abs().sum(0)
    if start is not None:
        s, mag = s + start, mag + start.abs()
    return s, part.shape[0] * U * mag


def sum_partials_f32(part, n, start, vector, skip_from=None):
    """The float32 sum in the order the kernels' comments state: the 16-byte kernel ((s0 + s1) + (s2 + s3)) [+ start] with s_w = part[w] +
    part[w + 4] + ... in order from 0; the scalar kernel start (or 0) + part[0] + part[1] + ...  skip_from: a mutant that stops there."""
    F = np.float32
    p = part[:, :n].numpy().astype(F)
    n_part = p.shape[0] if skip_from is None else min(p.shape[0], skip_from)
    if vector:
        sw = []
        for w in range(4):
            s = np.zeros(n, F)
            for q in range(w, n_part, 4):
                s = s + p[q]
            sw.append(s)
        t = (sw[0] + sw[1]) + (sw[2] + sw[3])
        if start is not None:
            t = t + start.numpy().astype(F)
    else:
        t = np.zeros(n, F) if start is None else start.numpy().astype(F).copy()
        for q in range(n_part):
            t = t + p[q]
    return torch.from_numpy(t)


# ------------------------------------------------------------------------------------------------ mage_act, mage_act_bwd
ACT_N = (4, 1020, 1024, 1028)
ACTS = ("relu", "quickgelu", "gelu_erf")
ACTS_BWD = ACTS + ("tanh",)
C_QG = f32(1.702)
ACT_SPECIAL = (0.0, -0.0, 30.0, -30.0, 60.0, -60.0, -12.0, 12.0)


def act_inputs(n, dt):
    """A list of (x, dy) pairs of n elements each (dtype dt): a ladder over [-12, 12] with +-0, +-30, +-60 among it; n = 4 takes three vectors."""
    g = torch.Generator().manual_seed(n)
    if n == 4:
        xs = [torch.tensor(ACT_SPECIAL[:4]), torch.tensor(ACT_SPECIAL[4:]), torch.tensor([-1.7, -0.3, 0.45, 2.9])]
    else:
        x = torch.linspace(-12, 12, n)
        for k, v in enumerate(ACT_SPECIAL[:6]):
            x[1 + k * (n // 7)] = v
        xs = [x]
    out = []
    for x in xs:
        dy = torch.randn(x.numel(), generator=g) * 2
        dy[0] = 0.0
        out.append((x.to(TDT[dt]), dy.to(TDT[dt])))
    return out


def _sig(v):
    """(s, 1 - s, |c v|) of s = 1 / (1 + exp(-c v)), without overflow."""
    w = C_QG * v
    return torch.sigmoid(w), torch.sigmoid(-w), w.abs()


def act(v, kind):
    """(y, fp32 bound) in fp64 for v fp64 (the values read)."""
    if kind == "relu":
        return v.clamp(min=0), torch.zeros_like(v)
    if kind == "quickgelu":
        s, q, aw = _sig(v)
        y = v * s
        return y, y.abs() * U * (q * (aw + 2) + 2) + TINY + v.abs() * 2.0 ** -128
    assert kind == "gelu_erf"
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2))), 10 * U * v.abs() + TINY


def act_bwd(v, dy, kind):
    """(dx, fp32 bound) in fp64; v is the pre-activation (tanh: the output)."""
    if kind == "relu":
        return dy * (v > 0), torch.zeros_like(v)
    if kind == "tanh":
        D = 1 - v * v
        dx = dy * D
        return dx, dy.abs() * U * (v * v + D.abs()) + U * dx.abs() + TINY
    if kind == "quickgelu":
        s, q, aw = _sig(v)
        w = C_QG * v
        r = 1 + w * q
        D = s * r
        dx = dy * D
        es = U * (q * (aw + 2) + 2)
        e_r = aw * (s * es + U * q) + 2 * U * aw * q + U * r.abs()
        e = dy.abs() * (s * e_r + r.abs() * s * es + U * D.abs()) + U * dx.abs()
        return dx, e + TINY * (1 + dy.abs()) + dy.abs() * 2.0 ** -128 * (1 + aw)
    assert kind == "gelu_erf"
    A = 0.5 * (1 + torch.erf(v / math.sqrt(2)))
    B = v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    D = A + B
    dx = dy * D
    e = dy.abs() * (5 * U + U * A + B.abs() * (0.5 * v * v + 5) * U + U * D.abs()) + U * dx.abs()
    return dx, e + TINY * (1 + dy.abs() * (1 + v.abs()))


# ------------------------------------------------------------------------------------------------ mage_dropout, mage_dropout_add
DROP_P = (0.0, 0.1, 0.5, P_MAX)
DROP_SEEDS = (0, GOLD)
DROP_N = (4, 1020, 1028)


def drop_inputs(n, seed):
    """(x, r) fp32 [n]: x with an exact 0 and a -0.0, r the residual / the previous y."""
    g = torch.Generator().manual_seed(n * 3 + seed % 1000)
    x, r = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    x[0], x[n - 1] = 0.0, -0.0
    return x, r


# ------------------------------------------------------------------------------------------------ mage_adam
ADAM_N = (1, 3, 4, 5, 1023, 1024, 1027)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_SCALES = (1.0, 0.125, 1.0 / 3.0)
ADAM_HYPER = ((0.9, 0.98, 1e-6), (0.9, 0.999, 1e-8))
ADAM_LR = 1e-3


def adam_inputs(n, step, b1, b2):
    """p, g, m, v fp32 [n]: m and v as a run that reached `step` would hold them (zeros before step 1); planted from the END of the arena, where
    the scalar tail is: g = m = v = 0; g = 1e-30 (g^2 underflows in fp32); v = 1e30 -- as many of them as n leaves room for beside one
    ordinary element."""
    g_ = torch.Generator().manual_seed(n * 7 + step)
    p, g, gp = torch.randn(n, generator=g_), torch.randn(n, generator=g_) * 0.1, torch.randn(n, generator=g_) * 0.1
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = gp * (1 - f32(b1) ** (step - 1)), gp * gp * (1 - f32(b2) ** (step - 1))
    idx = SimpleNamespace(zero=None, tiny=None, big=None)
    if n >= 2:
        idx.zero = n - 1
        g[n - 1] = m[n - 1] = v[n - 1] = 0.0
    if n >= 3:
        idx.tiny = n - 2
        g[n - 2] = 1e-30
    if n >= 4:
        idx.big = n - 3
        v[n - 3] = 1e30
    return p.float(), g.float(), m.float(), v.float(), idx


def adam(p, g, m, v, lr, b1, b2, eps, step, gs):
    """One step in fp64 from the fp32 state read (p, g, m, v fp64 of those values): SimpleNamespace(p, m, v, bp, bm, bv)."""
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(gs)
    ge = g * gs
    m1 = b1 * m + (1 - b1) * ge
    v1 = b2 * v + (1 - b2) * ge * ge
    em = U * ((b1 * m).abs() + 3 * ((1 - b1) * ge).abs() + m1.abs()) + TINY
    ev = U * (b2 * v + 5 * (1 - b2) * ge * ge + v1) + TINY
    pw1, pw2 = b1 ** step, b2 ** step
    bc1, bc2s = 1 - pw1, math.sqrt(1 - pw2)
    rb1 = (2 * U * pw1 + U) / (1 - pw1)
    rb2 = (2 * U * pw2 + U) / (2 * (1 - pw2)) + U
    sq = v1.sqrt()
    e_sq = torch.minimum(torch.where(sq > 0, ev / sq, torch.full_like(sq, float("inf"))), ev.sqrt()) + U * sq
    q = sq / bc2s
    e_q = e_sq / bc2s + q * (rb2 + U)
    den = q + eps
    e_den = e_q + U * den
    r = m1 / den
    e_r = em / den + r.abs() * (e_den / den + U)
    A = lr / bc1
    upd = A * r
    e_upd = A * e_r + upd.abs() * (rb1 + 2 * U)
    p1 = p - upd
    return SimpleNamespace(p=p1, m=m1, v=v1, bp=e_upd + U * p1.abs(), bm=em, bv=ev)
