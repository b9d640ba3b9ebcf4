"""Shared helpers for the parity tests: fixtures, synthetic models, oracle state dicts."""
import os

import numpy as np
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
