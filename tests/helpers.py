"""Shared helpers for the parity tests: fixtures, synthetic models, oracle state dicts."""
import os

import numpy as np
import pytest
import torch

from mage_amd.utils import synth
from mage_amd.utils.util import instantiate_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def t(a):
    return torch.from_numpy(np.asarray(a))


def build_mage(cfg, seed, device="cpu"):
    """Product-side model (mage_amd.modules) with portable synthetic weights."""
    p = cfg["params"]
    m = instantiate_from_config(cfg).eval()
    synth.fill_state_dict(m, seed, d_model=p["vision_width"], n_layers=p["generate_decoder_config"]["params"]["layers"])
    return m.to(device)


def build_vqvae(input_dim, down_ratio, dim, K, seed, device="cpu"):
    from mage_amd.modules.vqvae_model import VectorQuantizedVAE
    m = VectorQuantizedVAE(input_dim, down_ratio, dim, K).eval()
    synth.fill_state_dict(m, seed)
    return m.to(device)


def cpu_sd(module):
    return {k: v.detach().cpu() for k, v in module.state_dict().items()}


def chk(x):
    x = x.double()
    return np.array([x.sum().item(), x.abs().sum().item(), (x * x).sum().item()], np.float64)


def assert_tokens(got, want, margin, tol, what):
    """Index parity: exact wherever the reference's own top-2 margin exceeds `tol`; report the rest."""
    got, want, margin = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1), np.asarray(margin).reshape(-1)
    bad = got != want
    hard = bad & (margin > tol)
    assert not hard.any(), f"{what}: {hard.sum()} index mismatches where the reference margin > {tol} " \
                           f"(first at {np.flatnonzero(hard)[:5]}, margins {margin[hard][:5]})"
    return int(bad.sum())


def unsplit(y, kind):
    """Split-precision rows [rows, 2C] (MAGE_F16X3 / MAGE_BF16X3 pieces, include/mage_hip.h) -> the fp64 values they represent [rows, C]."""
    from mage_amd import ops
    rows, c2 = y.shape
    v = y.reshape(rows, c2 // 128, 2, 64).float()
    lo = v[:, :, 1] / (2048.0 if kind == ops.F16X3 else 1.0)
    return (v[:, :, 0].double() + lo.double()).reshape(rows, c2 // 2)


# ---------------------------------------------------------------- attention cases (tests/test_gpu_attention.py, tests/attention_bwd_ref.py)
# NaN sentinels with a payload no kernel produces (negative sign, nonzero payload): 0 * inf gives the default NaN
SENTINEL = {torch.float32: (torch.int32, 0xFFC0DEAD - 2 ** 32), torch.bfloat16: (torch.int16, 0xFFDE - 2 ** 16),
            torch.float16: (torch.int16, 0xFE5A - 2 ** 16)}


def attn_case(name, kind, nq, nk, H, n_seq, inner=1, causal=False, geo="sep", lens=None, div=1, omap=False, spread=1, scale=None,
              kv_shared=False):
    """geo 'axial': q, k, v side by side in one [rows, 3C] buffer, query i and key i on one row (the decoder's axial blocks; nq == nk);
    'sep': three buffers with different leading dimensions.  spread 2 leaves a row gap between consecutive queries; omap gives out a row
    map of its own (gaps between queries and between outer blocks); kv_shared: every outer block reads the same keys (kv_outer_stride 0).
    lens: per-sequence key lengths 'edge' (nk, 1, nk - 1, a middle value, nk + 3) or 'edge0' (the same after a 0), indexed by s / div."""
    return pytest.param(dict(name=name, kind=kind, nq=nq, nk=nk, H=H, n_seq=n_seq, inner=inner, causal=causal, geo=geo, lens=lens, div=div,
                             omap=omap, spread=spread, scale=scale, kv_shared=kv_shared), id=name)


def attn_lens(c):
    nk, n = c["nk"], -(-c["n_seq"] // c["div"])
    pat = [nk, 1, max(nk - 1, 0), (nk + 1) // 2, nk + 3]
    if c["lens"] == "edge0":
        pat = [0] + pat
    g = torch.Generator().manual_seed(n * 7 + nk)
    rnd = torch.randint(0, nk + 1, (n,), generator=g)
    return torch.tensor([pat[i] if i < len(pat) else int(rnd[i]) for i in range(n)], dtype=torch.int32)


def ulp(x, dt):
    """The spacing of dt's values at |x| (bf16: 8 significand bits down to fp32's normal range; f16: 11 bits, subnormals below 2^-14)."""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, -1000.0, e.to(torch.float64) - 1)               # floor(log2 |x|)
    if dt == torch.bfloat16:
        return torch.exp2(e.clamp(min=-126) - 7)
    return torch.exp2(e.clamp(min=-14) - 10)


def attn_geometry(c):
    nq, nk, inner, n_seq = c["nq"], c["nk"], c["inner"], c["n_seq"]
    n_outer = -(-n_seq // inner)
    if c["geo"] == "axial":
        assert nq == nk and c["spread"] == 1
        g = dict(q_outer_stride=nk * inner, q_axis_stride=inner, kv_outer_stride=nk * inner, kv_axis_stride=inner)
        q_rows = kv_rows = n_outer * nk * inner
    else:
        qas = inner * c["spread"]
        g = dict(q_outer_stride=nq * qas, q_axis_stride=qas, kv_outer_stride=0 if c["kv_shared"] else nk * inner, kv_axis_stride=inner)
        q_rows, kv_rows = n_outer * nq * qas, (1 if c["kv_shared"] else n_outer) * nk * inner
    if c["omap"]:
        g.update(o_outer_stride=nq * 2 * inner + inner, o_axis_stride=2 * inner)
        o_rows = n_outer * g["o_outer_stride"]
    else:
        o_rows = q_rows
    return g, q_rows, kv_rows, o_rows + 3                                   # 3 rows past the last mapped one


def attn_row_maps(c, g):
    s = torch.arange(c["n_seq"])
    outer, inn = s // c["inner"], s % c["inner"]
    qr = (outer * g["q_outer_stride"] + inn)[:, None] + torch.arange(c["nq"])[None] * g["q_axis_stride"]
    kr = (outer * g["kv_outer_stride"] + inn)[:, None] + torch.arange(c["nk"])[None] * g["kv_axis_stride"]
    orr = (outer * g["o_outer_stride"] + inn)[:, None] + torch.arange(c["nq"])[None] * g["o_axis_stride"] if c["omap"] else qr
    return qr, kr, orr


# ---------------------------------------------------------------- kernel-against-fp64 tests (tests/test_gpu_train_kernels.py, tests/test_gpu_norm_kernels.py)
DEV = "cuda:0"
WORST = {}


def lib():
    from mage_amd import ops
    return ops._dev(torch.empty(1, device=DEV))


def sent(shape, dt):
    it, val = SENTINEL[dt]
    return torch.full(shape if isinstance(shape, tuple) else (shape,), val, dtype=it, device=DEV).view(dt)


def untouched(t):
    it, val = SENTINEL[t.dtype]
    return bool((t.view(it) == val).all())


def written(t):
    it, val = SENTINEL[t.dtype]
    return bool((t.view(it) != val).all())


def bits(t):
    return t.view(SENTINEL[t.dtype][0])


def ptr(t):
    return None if t is None else t.data_ptr()


def within(entry, name, got, ref, bound):
    """Every element finite and inside its bound; keeps the largest |err| / bound per entry point for the report."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    w = int(ratio.flatten().argmax()) if ratio.numel() else 0
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print(f"{entry} {name}: worst |err| / bound {worst:.3f} (largest so far {WORST[entry]:.3f})")
    assert worst <= 1.0, (f"{entry} {name}: |err| {float(err.flatten()[w]):.3e} > bound {float(bound.expand_as(err).flatten()[w]):.3e} at flat index {w} "
                          f"(ref {float(ref.expand_as(err).flatten()[w]):.9e}, got {float(got.flatten()[w]):.9e})")


def count_lib_calls(monkeypatch, lib=None):
    """Every C-ABI entry point of `lib` (default: the library of GPU 0) appends its name to the returned list when called; monkeypatch.undo()
    ends the counting."""
    from mage_amd import _lib
    lib = _lib.lib(0) if lib is None else lib
    calls = []

    def counted(name, fn):
        def f(*a):
            calls.append(name)
            return fn(*a)
        return f
    for name in {**_lib.SIGNATURES, **_lib.EXT_SIGNATURES}:
        if name not in ("mage_last_error", "mage_abi_version"):
            monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    return calls


def refused(call, *outs):
    with pytest.raises(ValueError):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert untouched(o), "a refused call wrote to an output"
