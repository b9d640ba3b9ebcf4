"""fp64 restatements of the two entry points behind MAGE.preference_loss (include/mage_hip_ext.h; kernels in mage_amd/csrc/preference.hip)
with a per-element error bound for every output:
    mage_preference_loss (the pair stage of DPO / IPO), mage_token_logprob_bwd (the gradient of weighted token log-probabilities).

Pair stage.  Inputs: s, r fp32 [clips], pairs [P, 2] = (w, l), beta and eps as the fp32 values the call receives, widened.  In fp64:
    a = s_w - r_w,  b = s_l - r_l,  u = a - b,  h = beta u          (a, b, u: differences of fp32 values and of their differences)
    mode 0:  l = -(1 - eps) logsig(h) - eps logsig(-h),  logsig(x) = min(x, 0) - log1p(exp(-|x|));  with eps == 0 the second term is
             not formed and l = log1p(exp(-|h|)) - min(h, 0)  (the same number; a saturated pair is +0)
             g = -beta ((1 - eps) sig(-h) - eps sig(h)),  sig(|h|) = 1 / (1 + e),  sig(-|h|) = e / (1 + e),  e = exp(-|h|)
    mode 1:  l = (u - 1 / (2 beta))^2,  g = 2 (u - 1 / (2 beta))
    clip_coef[c] = (sum_{p: w = c} g_p - sum_{p: l = c} g_p) / P, the terms in increasing p, pairs with w == l left out
    summary = the means over p of l, [u > 0], beta a, beta b, h.
Bounds.  The kernel evaluates the same formulas in fp64 and rounds each output to fp32 once.  The device's exp and log1p may differ from the
host's in the last bits of an fp64 value (a few 2^-53, relative), and a handful of fp64 operations follow: relative 2^-48 covers the chain
with a factor 30 to spare.  Against the UNROUNDED fp64 reference a correctly rounded fp32 result errs by half an fp32 ulp, and 2^-48 is
2^-24 of that: every pair-stage output is held to
    one fp32 ulp of the reference  (np.spacing of its float32 value)  + 2^-126,
the last term for a result below fp32's normal range, which the conversion may flush (tests/train_ref.py makes the same allowance).
Where an output is a SUM whose terms can cancel, one ulp of the result no longer covers the fp64 error of the terms:
    clip_coef[c]:  + n_c 2^-48 max_p |g_p| / P,  n_c = the number of (w != l) pairs naming c  (n_c terms, each off by 2^-48 |g| at most, and
                   n_c fp64 additions of partial sums below n_c max|g|: n_c^2 2^-53, below the first term for n_c <= 32, which the tests
                   assert of their cases);
    summary[q]:    + 2^-48 max_p |t_p| for its terms t (P terms off by 2^-48 |t| each, divided by P; the fp64 additions add P 2^-53 mean|t|,
                   far below it for P <= 2^16): the mean margin of a symmetric set of pairs is a sum that cancels to 0.
An exact 0 in the reference (u = 0: margin 0; a clip in no pair: +0) has a bound of 2^-126 + the smallest subnormal: in effect exact, and the
tests that state exactness compare bits.

mage_token_logprob_bwd.  Row i: c_i = fp32(grad_out * weight[i / weight_div]) -- the caller forms this one fp32 product and hands it over, so
it is exact here; m = max_j z_j, w_j = exp(z_j - m), P_j = w_j / sum w, out_ij = c_i ([j = t_i] - P_ij); a row with c_i == 0 is +0 throughout.
The arithmetic is mage_cross_entropy_bwd's (fp32 expf(z - max) times the fp32 reciprocal of a fixed-order fp32 sum, one subtraction against
the one-hot, one multiply by the scale) with c_i in the place of grad_out / rows, so the bound is tests/train_ref.py cross_entropy_bwd's with
sc = |c_i| (its derivation is in that module's docstring; the scale there costs 2 u for a product and a divide, here c_i is exact: the 3 u
|out| term is kept as it stands, one u to spare):
    |err| <= |c_i| (P_k ((a_k + ceil(K / 64) + 10) u + sum_j P_j (a_j + 2) u) + u |P_k - hot|) + 3 u |out| + |c_i| 2^-125 + the store's error,
a_k = |z_k - m| (0 at a -inf logit, where P_k = 0 exactly).  The sum's term: the kernel keeps the row in the sampler's layout, 4 codes per lane
and 256-code chunk, so a lane adds NV = 4 .. 64 terms where ce_bwd_kernel's adds ceil(K / 64); a term that is exp(-inf) = 0 (the padding past
K) adds no rounding, and at the K tested here (4, 64, 68, 512, 1000, 4096) the additions above any term number at most ceil(K / 64) + 6
butterfly steps included (K = 64: 3 in the lane + 4 butterfly steps between the 16 lanes that hold codes; K = 68: 3 + 5).
No constant here is fitted to a kernel's output."""
import numpy as np
import torch

from tests import train_ref as T

U = 2.0 ** -24
TINY = 2.0 ** -126
REL64 = 2.0 ** -48


def f32(v):
    return float(np.float32(v))


def ulp32(x):
    """The spacing of float32 at |x| (fp64 array in, fp64 array out)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def logsig(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def pair_terms(s, r, pairs, beta, eps, mode):
    """(l, g, a, b, u, h) per pair in fp64; s, r float32 arrays, beta / eps the fp32 values widened."""
    s, r = np.asarray(s, np.float32).astype(np.float64), np.asarray(r, np.float32).astype(np.float64)
    pairs = np.asarray(pairs, np.int64)
    beta, eps = f32(beta), f32(eps)
    w, lo = pairs[:, 0], pairs[:, 1]
    a, b = s[w] - r[w], s[lo] - r[lo]
    u = a - b
    h = beta * u
    if mode == 1:
        d = u - 1.0 / (2.0 * beta)
        return d * d, 2.0 * d, a, b, u, h
    e = np.exp(-np.abs(h))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sp, sn = np.where(h >= 0, big, small), np.where(h >= 0, small, big)          # sig(h), sig(-h)
    if eps == 0.0:
        return np.log1p(e) - np.minimum(h, 0.0), -beta * sn, a, b, u, h
    return -(1.0 - eps) * logsig(h) - eps * logsig(-h), -beta * ((1.0 - eps) * sn - eps * sp), a, b, u, h


def pair_stage(s, r, pairs, beta, eps=0.0, mode=0):
    """The four outputs of mage_preference_loss in fp64, and their bounds under the same names + '_bound'."""
    pairs = np.asarray(pairs, np.int64)
    P, clips = pairs.shape[0], len(s)
    l, g, a, b, u, h = pair_terms(s, r, pairs, beta, eps, mode)
    coef, n_c = np.zeros(clips), np.zeros(clips)
    for p in range(P):                                                          # in increasing p
        w, lo = pairs[p]
        if w == lo:
            continue
        coef[w] += g[p]
        coef[lo] -= g[p]
        n_c[w] += 1
        n_c[lo] += 1
    coef /= P
    bt = f32(beta)
    terms = np.stack([l, (u > 0).astype(np.float64), bt * a, bt * b, h])
    summary = terms.sum(1) / P
    gmax = np.abs(np.where(pairs[:, 0] != pairs[:, 1], g, 0.0)).max()
    return dict(pair_loss=l, pair_margin=h, clip_coef=coef, summary=summary, g=g, u=u, n_c=n_c,
                pair_loss_bound=ulp32(l) + TINY, pair_margin_bound=ulp32(h) + TINY,
                clip_coef_bound=ulp32(coef) + n_c * REL64 * gmax / P + TINY,
                summary_bound=ulp32(summary) + REL64 * np.abs(terms).max(1) + TINY)


def token_logprob_bwd(z, tg, c, kind="f32"):
    """(dlogits, bound) in fp64; z fp64 [rows, K] (rows with c == 0 may hold anything), tg int64 [rows], c fp64 [rows]: the fp32 products
    grad_out * weight as the kernel forms them."""
    rows, K = z.shape
    live = (c != 0)[:, None]
    z = torch.where(live, z, torch.zeros_like(z))                               # a zero-weight row is never read
    sc = c.abs()[:, None]
    mx = z.amax(-1, keepdim=True)
    P = torch.softmax(z, -1)
    a = torch.where(torch.isinf(z), torch.zeros_like(z), (z - mx).abs())
    hot = (torch.arange(K)[None, :] == tg[:, None]).double()                    # no column matches a token outside [0, K)
    out = torch.where(live, c[:, None] * (hot - P), torch.zeros_like(z))
    n = -(-K // 64)
    b = sc * (P * ((a + n + 10) * U + (P * (a + 2)).sum(-1, keepdim=True) * U) + U * (P - hot).abs()) + 3 * U * out.abs() + sc * 2.0 ** -125
    return out, torch.where(live, b + T.store_err(out, kind), torch.zeros_like(b))


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
LPB_SHAPES = ((1, 4), (5, 64), (7, 68), (3, 512), (6, 1000), (2, 4096))
LPB_GRAD_OUT = 0.7


def lpb_inputs(rows, K, weight_div):
    """logits [rows, K] fp32 (row 1: +-80; row 2: some -inf; the rows of the zero weight hold a NaN: they must not be read), tokens cycling
    through 0, K - 1, -1, K and random codes, weights cycling through 0.7, 0.0, -1.3 (one per weight_div rows)."""
    g = torch.Generator().manual_seed(rows * 1013 + K + weight_div)
    z = torch.randn(rows, K, generator=g) * 3
    tg = torch.randint(0, K, (rows,), generator=g)
    for i, v in enumerate([0, K - 1, -1, K][:rows]):
        tg[i] = v
    n_w = -(-rows // weight_div)
    w = torch.tensor([[0.7, 0.0, -1.3][j % 3] for j in range(n_w)], dtype=torch.float32)
    wrow = w[torch.arange(rows) // weight_div]
    if rows > 1:
        z[1] = torch.where(torch.arange(K) % 2 == 0, 80.0, -80.0)
    if rows > 2 and K > 3:
        z[2, 1::3] = float("-inf")
    z[wrow == 0, 0] = float("nan")
    return z, tg.long(), w, wrow


def six_nine():
    """(clips 6, pairs 9): clip 0 chosen three times, clip 1 both chosen and rejected, clip 5 in no pair, one pair (2, 2), no order."""
    return np.array([[3, 4], [0, 1], [2, 2], [1, 3], [0, 4], [4, 2], [0, 3], [3, 1], [2, 0]], np.int64)


def margin_case(beta):
    """s, r, pairs such that h = beta u takes 0, +-1e-3, +-1, +-20, +-100 (to fp32 rounding of s): pair p = (2p, 2p + 1), r = 0."""
    hs = [0.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0]
    s = np.zeros(2 * len(hs), np.float32)
    for p, h in enumerate(hs):
        s[2 * p], s[2 * p + 1] = np.float32(-50.0 + h / beta / 2), np.float32(-50.0 - h / beta / 2)
    s[0] = s[1] = np.float32(-50.0)
    pairs = np.arange(2 * len(hs), dtype=np.int64).reshape(-1, 2)
    return s, np.zeros_like(s), pairs
