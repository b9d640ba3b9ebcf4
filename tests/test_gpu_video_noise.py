"""GPU: mage_video_noise (include/mage_hip_ext.h) against the fp64 restatement of its rule (tests/video_noise_ref.py), and the bitwise
properties the header promises.

The per-element bound.  The kernel computes z = fl(r * c), r = sqrtf(2 e), e = -logf(u1) or -log1pf(-(1 - u1)), c = cospif(a).  The
arguments u1 (or 1 - u1) and a are exact in fp32 and 2 e is an exact doubling, so the only errors are the three library functions' and the
final product's rounding.  Nothing in the project states the device math library's accuracy, so -- as tests/conv_ref.py does for tanhf --
each function gets what its specification promises, the OpenCL full-profile figures the device library is written to meet:
    logf 3 ulp, log1pf 2 ulp (the larger, 3, is used for both branches),  sqrtf 3 ulp,  cospif 4 ulp.
With u = 2^-24 (one ulp of a normal fp32 value is at most 2 u of its magnitude; none of e, r, c, z is subnormal: e >= 2^-25, |c| >= pi 2^-23
since the angle is never within 2^-23 of a zero of the cosine):
    e = e0 (1 + d1), |d1| <= 3 * 2u;      r = sqrt(2 e) (1 + d2), |d2| <= 3 * 2u  =>  r = r0 (1 + d1)^(1/2) (1 + d2): relative error
    <= 3u + 6u = 9u to first order;       c = c0 (1 + d3), |d3| <= 4 * 2u = 8u;     the product rounds once: <= u.
    |z - z0| <= |z0| (9u + 8u + u) (1 + 1e-5) = 18 u |z0| (the factor covers the second-order terms, < (18u)^2),
plus 2e-15, far above the restatement's own fp64 error (|z0| < 5.89, two fp64 library calls and three roundings: < 1e-15).  That is 1.07e-6
relative.  Measured on the MI355X (this file prints the ratio): the worst error is 0.21 of the bound.
"""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import video_noise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
LOG_ULPS, SQRT_ULPS, COSPI_ULPS = 3, 3, 4
REL = (0.5 * LOG_ULPS * 2 + SQRT_ULPS * 2 + COSPI_ULPS * 2 + 1) * U * (1 + 1e-5)

SEEDS = [0, -1, -2 ** 63, 20240917, -7046029254386353131]
SHAPES = [(3, 64, 256), (1, 64, 25), (2, 4, 7)]               # the model's; hw no multiple of 4; both axes ragged, quads misaligned
_REF = {}


def ref(B, C, hw, first=0):
    key = (B, C, hw, first)
    if key not in _REF:
        _REF[key] = R.noise(SEEDS[first:first + B], C, hw)
        _REF[key].setflags(write=False)
    return _REF[key]


def run(seeds, C, hw, nchw=True, rows=True, pad=64):
    """The raw entry point on NaN-filled buffers with `pad` floats of padding either side of each output: (nchw, rows, ok) as numpy
    (None where not asked for); ok = every padding value is still the NaN sentinel."""
    lib = _lib.lib(0)
    s = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    B, n = len(seeds), len(seeds) * C * hw
    bufs = [torch.full((n + 2 * pad,), float("nan"), device=DEV) if want else None for want in (nchw, rows)]
    ptrs = [None if b is None else b.data_ptr() + 4 * pad for b in bufs]
    with torch.cuda.device(0):
        _lib.check(lib.mage_video_noise(s.data_ptr(), B, C, hw, ptrs[0], ptrs[1], torch.cuda.current_stream().cuda_stream), lib)
    torch.cuda.synchronize()
    host = [None if b is None else b.cpu().numpy() for b in bufs]
    ok = all(np.isnan(h[:pad]).all() and np.isnan(h[n + pad:]).all() for h in host if h is not None)
    a = None if host[0] is None else host[0][pad:n + pad].reshape(B, C, hw)
    r = None if host[1] is None else host[1][pad:n + pad].reshape(B * hw, C)
    return a, r, ok


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("B,C,hw", SHAPES)
def test_values_match_the_rule_in_both_layouts(B, C, hw):
    want = ref(B, C, hw)
    a, r, ok = run(SEEDS[:B], C, hw)
    assert ok, "a store left its output"
    assert a.dtype == np.float32 and np.isfinite(a).all() and np.isfinite(r).all()
    bound = REL * np.abs(want) + 2e-15
    err = np.abs(a.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f"(B, C, hw) = {(B, C, hw)}: worst error / bound {ratio:.3f} (relative bound {REL:.3e}), max |z| {np.abs(a).max():.4f}")
    assert ratio <= 1.0
    assert np.abs(a).max() <= np.float32(5.89)
    assert np.array_equal(bits(r), bits(R.rows(a)))                       # the two layouts of one launch: the same bits
    a1, none, ok1 = run(SEEDS[:B], C, hw, rows=False)
    none2, r1, ok2 = run(SEEDS[:B], C, hw, nchw=False)
    assert ok1 and ok2 and none is None and none2 is None
    assert np.array_equal(bits(a1), bits(a)) and np.array_equal(bits(r1), bits(r))      # one at a time: the same bits again


@pytest.mark.parametrize("C,hw", [s[1:] for s in SHAPES])
def test_a_clip_does_not_know_its_batch(C, hw):
    three, rows3, _ = run(SEEDS[:3], C, hw)
    alone, rows1, _ = run(SEEDS[2:3], C, hw)
    assert np.array_equal(bits(alone[0]), bits(three[2])) and np.array_equal(bits(rows1), bits(rows3[2 * hw:]))
    again, _, _ = run([SEEDS[2], SEEDS[0], SEEDS[2]], C, hw)
    assert np.array_equal(bits(again[0]), bits(three[2])) and np.array_equal(bits(again[2]), bits(three[2]))
    assert np.array_equal(bits(again[1]), bits(three[0]))


def test_the_wrapper_returns_the_public_layout():
    s = torch.tensor(SEEDS[:2], dtype=torch.int64, device=DEV)
    a, r = ops.video_noise(s, C=64, h=16, w=16)
    assert a.shape == (2, 64, 16, 16) and r.shape == (2 * 256, 64) and a.dtype == r.dtype == torch.float32
    assert torch.equal(a.permute(0, 2, 3, 1).reshape(2 * 256, 64), r)
    want, _, _ = run(SEEDS[:2], 64, 256)
    assert np.array_equal(bits(a.cpu().numpy().reshape(2, 64, 256)), bits(want))
    a2, none = ops.video_noise(s, C=64, h=16, w=16, rows=False)
    assert none is None and torch.equal(a2, a)


def test_refusals_launch_nothing():
    lib = _lib.lib(0)
    C, hw, pad = 4, 7, 16
    s = torch.tensor(SEEDS[:2], dtype=torch.int64, device=DEV)
    a = torch.full((2 * C * hw + 2 * pad,), float("nan"), device=DEV)
    r = torch.full((2 * C * hw + 2 * pad,), float("nan"), device=DEV)
    pa, pr, ps = a.data_ptr() + 4 * pad, r.data_ptr() + 4 * pad, s.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for args in ((ps, 0, C, hw, pa, pr), (ps, -2, C, hw, pa, pr), (ps, 2, 0, hw, pa, pr), (ps, 2, C, 0, pa, pr), (ps, 2, C, -7, pa, pr),
                 (ps, 2, C, hw, None, None), (ps, 2, C, hw, pa + 4, pr), (ps, 2, C, hw, pa, pr + 8), (ps, 2, C, hw, None, pr + 4),
                 (None, 2, C, hw, pa, pr), (ps + 4, 2, C, hw, pa, pr), (ps, 2, 2 ** 20, 2 ** 11, pa, pr), (ps, 2, C, 2 ** 31, pa, pr),
                 (ps, 2 ** 37, C, hw, pa, pr)):
        rc = lib.mage_video_noise(*args, st)
        assert rc == -1 and "mage_video_noise" in lib.mage_last_error().decode(), args
    torch.cuda.synchronize()
    assert torch.isnan(a).all() and torch.isnan(r).all()                  # nothing ran: every sentinel is still there
    assert lib.mage_video_noise(ps, 2, C, hw, pa, pr, st) == 0            # and the same buffers are fine when the arguments are
    torch.cuda.synchronize()
    assert torch.isfinite(a[pad:-pad]).all() and torch.isnan(a[:pad]).all() and torch.isnan(a[-pad:]).all()
