"""numpy / fp64 references of the kernels that make or score the discrete decisions, with their case tables and checkers:
    mage_vq_prepare, mage_vq_nearest (mage_amd/csrc/vq.hip), mage_argmax, mage_cross_entropy (token_heads.hip), mage_caption_mask,
    mage_row_affine (rows.hip).
Every reference takes the exact fp32 values the kernel reads and returns, beside the expected values (and a bound where the result is not
exact), the flat index of every element the kernel must write: the footprint.  The checkers take the kernel's whole output buffers, which
start filled with a sentinel (F32_SENT: the NaN of tests/helpers.py SENTINEL; I64_SENT, I32_SENT) and carry TAIL elements of slack: outside
the footprint the sentinel must remain, inside it must be gone and the value right.  The case tables live here so the CPU and the GPU tests
share them.  u = 2^-24 (the unit roundoff of fp32); no constant here is fitted to a kernel's output.

Quantiser (mage_vq_nearest): the reference FORMULA  dist[m, k] = fl32(fl32(c2[k] + x2[m]) - 2 dot[m, k]),  x2 = sum_d z_d^2, c2 = sum_d c_d^2,
  dot = sum_d z_d c_d, each an fp64 sum rounded to fp32 ONCE; the first minimum wins; margin = fl32(second smallest dist - smallest dist),
  +inf for K = 1 (0 when the minimum is attained twice).  A product of two fp32 values is exact in fp64, so the only error of a kernel's
  fp64 sum is its additions': a sum of D terms in ANY order makes at most D - 1 roundings of partial sums no larger than sum |terms|:
      |dot_kernel - dot| <= D 2^-53 sum_d |z_d c_d|,    likewise x2 (sum z_d^2) and c2 (sum c_d^2).
  (vq_nearest_kernel: D fused multiply-adds in order.  vq_nearest_mfma_kernel: v_mfma_f64_16x16x4 steps, D of them per element; its x2 is
  D / 4 multiply-adds per lane and two shuffle additions, D / 4 + 2 <= D.  vq_prepare_kernel: D in order.)  The reference evaluates the sums
  in np.longdouble (matmul: D additions in order, D eps_ld sum |terms| of its own, added to the interval).  A (row, code) pair is SOFT when the
  interval [s - h, s + h] around the reference's dot does not round to ONE fp32 value; a code / a row is soft when the interval of its c2 /
  x2 does not; a row is soft when any of its pairs, its x2 or any c2 is.  On a hard row every fp32 operand of the formula is determined, and
  the formula's two fp32 operations are IEEE: index and margin must match bit for bit (2 dot is exact; the kernels' fmaf(-2, dot, s) rounds
  once, like the subtraction).  Every committed case has ZERO soft rows (vq_case tries seeds until that holds and the CPU test asserts it), so
  nothing is exempt and the two kernels must agree with each other bit for bit as well.
mage_vq_prepare: codebook_t is the exact transpose; c2 as above, bit for bit on hard codes (all of them).
mage_argmax: NaNs are skipped; best = the largest remaining logit, index = the first code equal to it (-0 == +0); no remaining logit:
  0x7fffffff.  margin = fl32(best - second), best = the picked code's logit, second = the largest logit among the other non-NaN codes, -inf
  if there is none: 0 at a tie (IEEE's sign: (-0) - (+0) = -0 where the pick is a -0 and its rival a +0), +inf for a single candidate, NaN
  for inf - inf (two +inf, or best = -inf) and for a row of NaNs.  Exact: bit for bit (any NaN for a NaN).
mage_cross_entropy: row_loss = logsumexp(z) - z_t in fp64.  ce_rows_kernel: mx = the fp32 maximum (exact); d_k = fl32(z_k - mx) (relative u,
  which the exponential turns into a relative error u |d_k| of its term); w_k = expf(d_k); a lane adds ceil(K / 64) terms in order, 6 butterfly
  additions join the lanes: n = ceil(K / 64) + 6 additions above any term, all terms >= 0; logf; + mx; - z_t.  expf and logf get what their
  specification promises, 3 ulp (the OpenCL full-profile figure the device math library is written to meet): a relative 6 u for a term,
  3 ulp32(log s) for the logarithm.  First order in u, with s = sum_k w_k >= 1:
      |err row_loss| <= n u + sum_k w_k (6 u + u |d_k|) / s + 3 ulp32(log s) + u |log s + mx| + u |row_loss|.
  A -inf logit that is not the target adds exp(-inf) = 0 exactly; at the target row_loss = +inf exactly; a row of -inf only: NaN (inf - inf).
  loss_mean = fl32(fp64 sum of the kernel's OWN row_loss values / rows), 1 ulp32 for the double rounding (sum_kernel's fp64 order and its
  multiplication by 1 / rows move the fp64 value by rows 2^-53 relative, far below an fp32 ulp).
mage_caption_mask: keep = 1.0 where id != padding else 0.0; kv_len = the NUMBER of kept ids (not a prefix length).  Exact.
mage_row_affine: y = x rs[r] + table[(r / div) % mod] in place.  The compiler may contract the product into the sum.  Unfused:
  fl(fl(x rs) + t): u |x rs| + u |y|; fused: u |y|; rs or table alone is one operation.  The bound that allows both:
      |err y| <= u |y| + (u |x rs| if both rs and table are given)."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
TAIL = 64                                   # slack elements past every output's last mapped element
F32_SENT = 0xFFC0DEAD                       # tests/helpers.py SENTINEL[torch.float32], as uint32 bits
I64_SENT = -0x5EADBEEF0BADF00D
I32_SENT = -0x5EADBEEF
NO_CODE = 0x7fffffff
F32, F64, LD = np.float32, np.float64, np.longdouble
EXP_ULPS = LOG_ULPS = 3.0


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def case_id(c):
    return c["name"]


def ulp32(y):
    """The spacing of fp32 values at |y| (fp64 in, fp64 out)."""
    y = np.abs(np.asarray(y, F64))
    ok = (y > 0) & np.isfinite(y)
    _, e = np.frexp(np.where(ok, y, 1.0))                                    # y = m 2^e, m in [0.5, 1): floor(log2 y) = e - 1
    return np.exp2(np.maximum(np.where(ok, e - 1.0, -1000.0), -126.0) - 23.0)


# ------------------------------------------------------------------------------------------------ buffers and checkers
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def _sent(dtype):
    return {np.dtype(F32): np.uint32(F32_SENT), np.dtype(np.int64): np.int64(I64_SENT), np.dtype(np.int32): np.int32(I32_SENT)}[np.dtype(dtype)]


def sent_buf(n, dtype):
    """A host buffer of n sentinels of `dtype` (what the GPU tests fill on the device)."""
    if np.dtype(dtype) == np.dtype(F32):
        return np.full(n, F32_SENT, np.uint32).view(F32)
    return np.full(n, _sent(dtype), dtype)


def filled(size, idx, want):
    """The buffer a correct kernel leaves: `want` at `idx`, sentinels elsewhere."""
    want = np.asarray(want)
    b = sent_buf(size, want.dtype)
    b[np.asarray(idx).reshape(-1)] = want.reshape(-1)
    return b


def check_out(name, buf, idx, want, bound=None, exempt=None):
    """buf: a whole output buffer; idx: the footprint; want / bound: the values there (bound None: bit for bit, any NaN for a NaN).  exempt: footprint
    elements whose value is not checked (they must still be written).  Returns the worst |err| / bound (0.0 for an exact output)."""
    buf, idx, want = np.asarray(buf).reshape(-1), np.asarray(idx).reshape(-1), np.asarray(want).reshape(-1)
    raw, s = bits(buf), _sent(buf.dtype)
    m = np.zeros(buf.size, bool)
    m[idx] = True
    assert int(m.sum()) == idx.size, f"{name}: two outputs share an element"
    assert bool((raw[~m] == s).all()), f"{name}: wrote outside its footprint (first at {np.flatnonzero((raw != s) & ~m)[:5]})"
    assert bool((raw[m] != s).all()), f"{name}: left part of its footprint unwritten (first at {np.flatnonzero((raw == s) & m)[:5]})"
    got = buf[idx]
    keep = np.ones(idx.size, bool) if exempt is None else ~np.asarray(exempt).reshape(-1)
    if buf.dtype != F32:
        bad = (got != want) & keep
        assert not bad.any(), f"{name}: {int(bad.sum())} wrong, first at {np.flatnonzero(bad)[:5]}: got {got[bad][:5]}, want {want[bad][:5]}"
        return 0.0
    if bound is None:
        want = want.astype(F32)
        bad = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))) & keep
        assert not bad.any(), f"{name}: {int(bad.sum())} not bit for bit, first at {np.flatnonzero(bad)[:5]}: got {got[bad][:5]}, want {want[bad][:5]}"
        return 0.0
    want, bound, g = want.astype(F64), np.broadcast_to(np.asarray(bound, F64).reshape(-1), want.shape), got.astype(F64)
    fin = np.isfinite(want)
    bad = ~fin & ~((g == want) | (np.isnan(g) & np.isnan(want))) & keep
    assert not bad.any(), f"{name}: non-finite results differ, first at {np.flatnonzero(bad)[:5]}: got {g[bad][:5]}, want {want[bad][:5]}"
    assert bool(np.isfinite(g[fin]).all()), f"{name}: non-finite output where the reference is finite"
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(fin, np.abs(g - want), 0.0)
        ratio = np.where((err == 0) | ~keep, 0.0, err / bound)
    w = int(ratio.argmax()) if ratio.size else 0
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{name}: |err| {err[w]:.3e} > bound {bound[w]:.3e} at {w} (ref {want[w]:.9e}, got {g[w]:.9e})"
    return worst


# ------------------------------------------------------------------------------------------------ the quantiser
# duplicate code vectors (lower, higher); the row that IS the vector must pick the lower one with margin 0.  Code k belongs, in the matrix-core
# kernel, to wave k / (16 NT), tile (k / 16) % NT, lane k % 16 (NT = 4 up to K = 512: 64 codes per wave; 8 above: 128); in the fallback to
# thread k % 256 for the distance and to lane k % 64 for the reduction.
VQ_DUPS = ((3, 9),          # inside one 16-code tile
           (5, 21),         # two tiles of one wave
           (13, 18),        # two tiles, the lower index in the later lane (13 against 2)
           (10, 74),        # two waves' slices at 64 codes per wave (two tiles of wave 0 at 128)
           (70, 129),       # two waves; fallback: lane 6 against lane 1, the lower index in the later lane
           (260, 330),      # K > 256: waves 4 and 5 of the eight; fallback: the second code of threads 4 and 74
           (200, 328),      # waves 1 and 2 at 128 codes per wave; fallback (K > 512): thread 200 against the second code of thread 72
           (600, 1001))     # K > 1001: waves 4 and 7; fallback: the third code of thread 88, the fourth of thread 233


def _vq(name, M, D, K, exact=True):
    return dict(name=name, M=M, D=D, K=K, exact=exact)


# M on either side of the 32-row (matrix cores) and 16-row (fallback) workgroups; K on both sides of the two ladder steps 256 / 257 and
# 512 / 513 and at the limit 1024, each with a ragged M; both kernels run every case
VQ_CASES = (
    _vq("k1_d8_m33", 33, 8, 1),                     # one code: margin +inf
    _vq("k15_d4_m31", 31, 4, 15),                   # less than one tile
    _vq("k16_d8_m32", 32, 8, 16),                   # exactly one tile, exactly one workgroup
    _vq("k17_d260_m33", 33, 260, 17),               # one code in the second tile; best = the last code of a ragged K
    _vq("k255_d8_m65", 65, 8, 255),
    _vq("k256_d64_m33", 33, 64, 256),
    _vq("k257_d64_m33", 33, 64, 257),               # the first K of the 8-wave instance / of two codes per thread
    _vq("k257_d260_m31", 31, 260, 257),
    _vq("k511_d8_m1", 1, 8, 511),                   # one row: the row is the last code
    _vq("k512_d64_m31", 31, 64, 512),
    _vq("k513_d8_m65", 65, 8, 513),                 # the first K of 8 tiles per wave / of four codes per thread
    _vq("k1000_d4_m33", 33, 4, 1000),
    _vq("k1023_d8_m1_random", 1, 8, 1023, exact=False),
    _vq("k1023_d64_m32", 32, 64, 1023),
    _vq("k1024_d8_m33", 33, 8, 1024),
    _vq("k1024_d64_m65", 65, 64, 1024),
)


def vq_exact_rows(c):
    """(row, code) pairs of a case: rows that ARE a code vector, from the last row (the ragged block) backwards: first the last code, then the
    lower code of every duplicate pair that fits K, then code 0."""
    if not c["exact"]:
        return []
    K = c["K"]
    codes = [K - 1] + [lo for lo, hi in VQ_DUPS if hi < K] + ([0] if K > 1 else [])
    return [(c["M"] - 1 - i, k) for i, k in enumerate(codes[:max(1, c["M"] - 1)])]


def vq_inputs(c, seed):
    g = _rng("vq", c["name"], seed)
    z = g.standard_normal((c["M"], c["D"])).astype(F32)
    cb = g.standard_normal((c["K"], c["D"])).astype(F32)
    for lo, hi in VQ_DUPS:
        if hi < c["K"]:
            assert c["K"] - 1 not in (lo, hi)
            cb[hi] = cb[lo]
    for r, k in vq_exact_rows(c):
        z[r] = cb[k]
    return SimpleNamespace(z=z, cb=cb)


def _sum_sq(a):
    """(fl32 of the row sums of squares, soft mask) of fp32 rows a [n, D]."""
    D = a.shape[1]
    al = a.astype(LD)
    s = np.einsum("nd,nd->n", al, al)                                        # longdouble, D additions in order
    S = (a.astype(F64) ** 2).sum(1) * (1 + 1e-12)
    h = (D * 2.0 ** -53 + D * float(np.finfo(LD).eps)) * S
    return s.astype(F32), (s - h).astype(F32) != (s + h).astype(F32)


def vq_reference(i):
    """idx int64 [M], margin fp32 [M], cbt, c2, the soft-row mask and the distances of inputs i (z [M, D], cb [K, D])."""
    z, cb = i.z, i.cb
    (M, D), K = z.shape, cb.shape[0]
    x2, soft_x = _sum_sq(z)
    c2, soft_c = _sum_sq(cb)
    dot = z.astype(LD) @ cb.astype(LD).T
    S = (np.abs(z).astype(F64) @ np.abs(cb).astype(F64).T) * (1 + 1e-12)
    h = (D * 2.0 ** -53 + D * float(np.finfo(LD).eps)) * S
    soft_pair = (dot - h).astype(F32) != (dot + h).astype(F32)
    dotf = dot.astype(F32)
    s = c2[None, :] + x2[:, None]                                            # fp32 arithmetic from here on: the formula's own roundings
    dist = s - F32(2.0) * dotf
    assert s.dtype == F32 and dist.dtype == F32
    idx = dist.argmin(1).astype(np.int64)                                    # the first minimum
    if K > 1:
        two = np.partition(dist, 1, axis=1)
        with np.errstate(invalid="ignore"):
            margin = (two[:, 1] - two[:, 0]).astype(F32)
    else:
        margin = np.full(M, np.inf, F32)
    return SimpleNamespace(idx=idx, margin=margin, cbt=np.ascontiguousarray(cb.T), c2=c2, soft_codes=soft_c,
                           soft=soft_pair.any(1) | soft_x | bool(soft_c.any()), dist=dist, M=M, D=D, K=K)


@functools.lru_cache(maxsize=None)
def _vq_case(name):
    c = {c["name"]: c for c in VQ_CASES}[name]
    for seed in range(64):
        i = vq_inputs(c, seed)
        r = vq_reference(i)
        if not r.soft.any():
            return i, r, seed
    raise AssertionError(f"{name}: no seed gives inputs without soft rows")


def vq_case(c):
    """(inputs, reference) of a committed case: the first seed whose inputs have no soft row."""
    i, r, _ = _vq_case(c["name"])
    return i, r


def check_vq(name, r, idx_buf, margin_buf):
    hard = ~r.soft
    check_out(name + " idx", idx_buf, np.arange(r.M), r.idx, exempt=~hard)
    if margin_buf is not None:
        check_out(name + " margin", margin_buf, np.arange(r.M), r.margin, exempt=~hard)


def check_vq_prepare(name, r, cbt_buf, c2_buf):
    check_out(name + " cbt", cbt_buf, np.arange(r.D * r.K), r.cbt)
    check_out(name + " c2", c2_buf, np.arange(r.K), r.c2, exempt=r.soft_codes)


# ------------------------------------------------------------------------------------------------ mage_argmax
def _am(name, K, rows, ld, pat, group=None, in_stride=None, in_off=0, out_stride=None, out_off=0):
    assert len(pat) == rows
    group = rows if group is None else group
    return dict(name=name, K=K, rows=rows, ld=ld, pat=pat, group=group, in_stride=group if in_stride is None else in_stride, in_off=in_off,
                out_stride=group if out_stride is None else out_stride, out_off=out_off)


# a lane owns codes 4 lane .. 4 lane + 3 of every 256-code sweep.  Patterns: see argmax_row
ARGMAX_CASES = (
    _am("k4_r5", 4, 5, 8, ("rand", "tie_lanes", "zeros", "all_nan", "one")),                       # one lane; two workgroups
    _am("k8_r3", 8, 3, 12, ("nan_max", "inf1", "last")),
    _am("k252_r4_grouped", 252, 4, 256, ("rand", "tie_lanes", "inf2", "ninf"), group=2, in_stride=5, in_off=2, out_stride=3, out_off=1),
    _am("k256_r1", 256, 1, 260, ("last",)),                                                         # exactly one sweep
    _am("k256_r5_packed", 256, 5, 256, ("rand", "zeros_pm", "nan_max", "tie_lanes", "all_nan")),     # ld == K
    _am("k260_r3", 260, 3, 264, ("tie_sweeps", "tie_hi_lane", "last")),                             # one lane sweeps twice
    _am("k512_r5_grouped", 512, 5, 516, ("rand", "tie_sweeps", "nan_max", "one", "inf1"), group=2, in_stride=3, in_off=1, out_stride=4, out_off=2),
    _am("k516_r4", 516, 4, 520, ("tie_sweeps", "last", "zeros", "tie_hi_lane")),
    _am("k4096_r3_grouped", 4096, 3, 4100, ("tie_sweeps", "rand", "last"), group=1, in_stride=2, in_off=1, out_stride=3, out_off=0),
    _am("k8192_r4", 8192, 4, 8196, ("rand", "tie_sweeps", "last", "nan_max")),                      # past the row-in-registers heads' K <= 4096
    _am("k8192_r1_packed", 8192, 1, 8192, ("tie_hi_lane",)),
)


def argmax_row(pat, K, g):
    v = g.standard_normal(K).astype(F32)
    top = F32(np.abs(v).max() + 1.0)
    if pat == "tie_lanes":                      # the maximum twice, in two lanes (K = 4: one lane)
        v[[1, K - 2]] = top
    elif pat == "tie_sweeps":                   # ... in lane 0's first and later sweeps (K <= 256: twice inside its one chunk)
        v[[k for k in (2, 258, 514, 2 + 256 * 17) if k < K] if K > 256 else [0, 3]] = top
    elif pat == "tie_hi_lane":                  # the lower index in the higher lane: lane 62 of sweep 0 against lane 0 of sweep 1
        v[[250, 257] if K > 257 else [1, K - 2]] = top
    elif pat == "zeros":                        # -0 first, +0 last, everything else negative
        v = -np.abs(v) - F32(1.0)
        v[2], v[K - 1] = F32(-0.0), F32(0.0)
    elif pat == "zeros_pm":
        v = -np.abs(v) - F32(1.0)
        v[1], v[3] = F32(0.0), F32(-0.0)
    elif pat == "nan_max":                      # NaN where the maximum would be, and at code 0
        v[int(v.argmax())] = np.nan
        v[0] = np.nan
    elif pat == "all_nan":
        v[:] = np.nan
    elif pat == "inf1":
        v[K - 3] = np.inf
    elif pat == "inf2":
        v[[1, K - 1]] = np.inf
    elif pat == "ninf":
        v[:] = -np.inf
    elif pat == "last":
        v[K - 1] = top
    elif pat == "one":                          # a single candidate among NaNs
        x = v[K - 2]
        v[:] = np.nan
        v[K - 2] = x
    else:
        assert pat == "rand"
    return v


def argmax_maps(c):
    i = np.arange(c["rows"])
    gi, gr = i // c["group"], i % c["group"]
    return gi * c["in_stride"] + gr + c["in_off"], gi * c["out_stride"] + gr + c["out_off"]


def argmax_inputs(c):
    """The logits buffer [n, ld]: the mapped rows' K codes; every gap column holds NaN and +inf in turn, every unmapped row +inf: neither is a code."""
    g = _rng("argmax", c["name"])
    irow, _ = argmax_maps(c)
    z = np.full((int(irow.max()) + 2, c["ld"]), np.inf, F32)
    z[:, c["K"]::2] = np.nan
    for r, pat in zip(irow, c["pat"]):
        z[r, :c["K"]] = argmax_row(pat, c["K"], g)
    return z


def argmax_rows(z, K):
    """(index, margin) of rows z [n, >= K] over their first K columns."""
    idx, margin = np.empty(z.shape[0], np.int64), np.empty(z.shape[0], F32)
    for r in range(z.shape[0]):
        v = z[r, :K]
        ok = ~np.isnan(v)
        if not ok.any():
            idx[r], margin[r] = NO_CODE, np.nan
            continue
        idx[r] = int(np.flatnonzero(ok & (v == v[ok].max()))[0])
        best = v[idx[r]]                                                     # the picked code's own value: -0 where the first zero is -0
        ok[idx[r]] = False
        second = v[ok].max() if ok.any() else F32(-np.inf)
        with np.errstate(invalid="ignore"):
            margin[r] = F32(best) - F32(second)
    return idx, margin


def argmax_reference(c, z, K=None):
    irow, orow = argmax_maps(c)
    idx, margin = argmax_rows(z[irow], c["K"] if K is None else K)
    return SimpleNamespace(idx=idx, margin=margin, orow=orow, out_size=int(orow.max()) + 1 + TAIL, margin_size=c["rows"] + TAIL)


def check_argmax(name, r, out_buf, margin_buf=None):
    check_out(name + " tokens", out_buf, r.orow, r.idx)
    if margin_buf is not None:
        check_out(name + " margin", margin_buf, np.arange(r.idx.size), r.margin)


# ------------------------------------------------------------------------------------------------ mage_cross_entropy
def _ce(name, rows, K, offset=0.0, ninf=False):
    return dict(name=name, rows=rows, K=K, offset=offset, ninf=ninf)


# a wave per row, four rows per workgroup, a lane's terms 64 apart; sum_kernel: 1024 threads, one pass
CE_CASES = (
    _ce("r1_k1", 1, 1),
    _ce("r3_k3", 3, 3),
    _ce("r4_k63", 4, 63),
    _ce("r5_k64", 5, 64),
    _ce("r1023_k65", 1023, 65),
    _ce("r1024_k3", 1024, 3),
    _ce("r1025_k64", 1025, 64),
    _ce("r5_k512_plus1e4", 5, 512, offset=1e4),
    _ce("r4_k1000_minus1e4", 4, 1000, offset=-1e4),
    _ce("r3_k1000", 3, 1000),
    _ce("r1025_k1", 1025, 1),
    _ce("r5_k65_ninf", 5, 65, ninf=True),           # row 0: -inf off the target; 1: -inf at the target; 2: -inf only; 3: all but the target; 4: plain
    _ce("r4_k3_ninf", 4, 3, ninf=True),
)


def ce_inputs(c):
    g = _rng("ce", c["name"])
    z = (g.standard_normal((c["rows"], c["K"])) * 3.0 + c["offset"]).astype(F32)
    tg = g.integers(0, c["K"], c["rows"]).astype(np.int64)
    tg[-1] = c["K"] - 1
    if c["ninf"]:
        K = c["K"]
        z[0, (tg[0] + 1) % K] = -np.inf
        z[0, (tg[0] + K - 1) % K] = -np.inf
        z[1, tg[1]] = -np.inf
        z[2, :] = -np.inf
        keep = z[3, tg[3]]
        z[3, :] = -np.inf
        z[3, tg[3]] = keep
    return z, tg


def ce_reference(z, tg):
    """(row_loss fp64 [rows], bound [rows]) of fp32 logits z [rows, K] and targets tg."""
    rows, K = z.shape
    z = z.astype(F64)
    zt = z[np.arange(rows), tg]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = z.max(1)
        d = z - mx[:, None]
        w = np.exp(d)
        s = w.sum(1)
        lse = np.log(s) + mx
        loss = lse - zt
        n = -(-K // 64) + 6
        terms = np.where(w > 0, w * (EXP_ULPS * 2 * U + U * np.abs(np.where(w > 0, d, 0.0))), 0.0).sum(1)
        bound = n * U + terms / s + LOG_ULPS * ulp32(np.log(s)) + U * np.abs(lse) + U * np.abs(loss)
    return loss, bound


def ce_mean(row_loss32, rows):
    """loss_mean from the kernel's own fp32 row losses: (value fp32, 1 ulp32)."""
    with np.errstate(invalid="ignore"):
        m = F32(np.asarray(row_loss32, F64).sum() / rows)
    return m, ulp32(F64(m))


def check_ce(name, z, tg, row_buf, mean_buf):
    """Returns the worst |err| / bound of (row_loss, loss_mean)."""
    rows = z.shape[0]
    loss, bound = ce_reference(z, tg)
    w_rows = check_out(name + " row_loss", row_buf, np.arange(rows), loss, bound)
    m, b = ce_mean(np.asarray(row_buf).reshape(-1)[:rows], rows)
    w_mean = check_out(name + " loss_mean", mean_buf, np.arange(1), np.array([m], F64), np.array([b]))
    return w_rows, w_mean


# ------------------------------------------------------------------------------------------------ mage_caption_mask
def _cm(name, B, S, pad, pats, outs="both"):
    assert len(pats) == B
    return dict(name=name, B=B, S=S, pad=pad, pats=pats, outs=outs)


# one 64-lane workgroup per caption sweeps it 64 ids at a time.  Patterns: none = no padding, tail = right-padded, middle = padding inside
# the caption and real ids after it, all = padding only
CAPTION_CASES = (
    _cm("s1_b3_pad0", 3, 1, 0, ("none", "all", "none")),
    _cm("s63_b3_pad0", 3, 63, 0, ("middle", "all", "none")),
    _cm("s64_b1_pad7", 1, 64, 7, ("middle",)),
    _cm("s64_b3_pad0_kv_only", 3, 64, 0, ("tail", "none", "middle"), outs="kv_len"),
    _cm("s65_b3_pad7", 3, 65, 7, ("middle", "tail", "all")),
    _cm("s65_b1_pad0_keep_only", 1, 65, 0, ("middle",), outs="keep"),
    _cm("s130_b3_pad0", 3, 130, 0, ("middle", "none", "tail")),
    _cm("s130_b1_pad7", 1, 130, 7, ("all",)),
)


def caption_inputs(c):
    g = _rng("caption", c["name"])
    S, pad = c["S"], c["pad"]
    ids = g.integers(1, 30, (c["B"], S)).astype(np.int64)
    ids[ids == pad] = pad + 1
    for b, p in enumerate(c["pats"]):
        if p == "all":
            ids[b] = pad
        elif p == "tail":
            ids[b, S - max(1, S // 3):] = pad
        elif p == "middle" and S > 2:
            ids[b, 1:1 + max(1, S // 4)] = pad                              # the first id and the last ones are real
            ids[b, S // 2] = pad
        elif p == "middle":
            ids[b, 0] = pad
    return ids


def caption_reference(ids, pad):
    k = ids != pad
    return k.astype(F32).reshape(-1), k.sum(1).astype(np.int32)


def check_caption(name, c, ids, keep_buf, kv_buf):
    keep, kv = caption_reference(ids, c["pad"])
    if keep_buf is not None:
        check_out(name + " keep", keep_buf, np.arange(keep.size), keep)
    if kv_buf is not None:
        check_out(name + " kv_len", kv_buf, np.arange(kv.size), kv)


# ------------------------------------------------------------------------------------------------ mage_row_affine
def _ra(name, rows, C, rs, table, div=1, mod=1):
    return dict(name=name, rows=rows, C=C, rs=rs, table=table, div=div, mod=mod)


# a thread per 4 channels, 256 threads per workgroup: rows C / 4 threads
ROW_AFFINE_CASES = (
    _ra("c4_r255_both", 255, 4, True, True, div=2, mod=3),          # 255 threads; (r / 2) % 3 wraps 42 times
    _ra("c4_r256_rs", 256, 4, True, False),                         # exactly one workgroup
    _ra("c4_r257_table", 257, 4, False, True, div=1, mod=5),        # one thread in the second workgroup
    _ra("c260_r3_both", 3, 260, True, True, div=1, mod=2),          # 195 threads; row 2 wraps to table row 0
    _ra("c260_r4_both", 4, 260, True, True, div=2, mod=1),          # 260 threads: the second workgroup starts inside row 3
    _ra("c260_r4_table", 4, 260, False, True, div=1, mod=3),
    _ra("c260_r8_rs", 8, 260, True, False),
)


def row_affine_inputs(c):
    g = _rng("row_affine", c["name"])
    x = g.standard_normal((c["rows"], c["C"])).astype(F32)
    rs = g.standard_normal(c["rows"]).astype(F32) if c["rs"] else None
    if rs is not None:
        rs[::7] = 0.0                                                    # the caption mask's zeros
    table = g.standard_normal((c["mod"], c["C"])).astype(F32) if c["table"] else None
    return SimpleNamespace(x=x, rs=rs, table=table)


def row_affine_reference(c, i):
    """(y fp64 [rows, C], bound)."""
    p = i.x.astype(F64) * (i.rs.astype(F64)[:, None] if i.rs is not None else 1.0)
    y = p + (i.table.astype(F64)[(np.arange(c["rows"]) // c["div"]) % c["mod"]] if i.table is not None else 0.0)
    b = U * np.abs(y) + (U * np.abs(p) if i.rs is not None and i.table is not None else 0.0)
    return y, b
