"""GPU: mage_token_logprob_bwd_masked (include/mage_hip_ext.h) against mage_token_logprob_bwd, bit for bit: a free row carries the unmasked
kernel's bits (that kernel is pinned against fp64 in tests/test_gpu_preference.py), a given row is +0 and its logits are not read (they
hold NaN here), and an all-free mask is the unmasked call as a whole.  The logits are tests/test_gpu_policy_loss.py's recipe (special rows
1, 2, 8, 9, 10, 12 included), the weights cycle through a zero (the unmasked kernel's own zero fill) and both signs."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests.test_gpu_masked_policy_kernels import _dbits, _masks
from tests.test_gpu_policy_loss import _logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("rows", [29, 259])
@pytest.mark.parametrize("K", [4, 260, 512])
def test_free_rows_keep_their_bits_and_given_rows_are_zero(K, rows):
    g = np.random.default_rng(K * 1000 + rows)
    z = torch.from_numpy(_logits(rows, K, seed=K + rows)).to(DEV)
    tok = torch.from_numpy(g.integers(0, K, rows)).to(DEV)
    gout = torch.tensor([0.7], device=DEV)
    for weight_div in (1, 5):
        n_w = -(-rows // weight_div)
        w = torch.tensor([[0.7, 0.0, -1.3][j % 3] for j in range(n_w)], device=DEV)
        for dt in (torch.float32, torch.bfloat16):
            want = ops.token_logprob_bwd(z, tok, w, gout, torch.empty(rows, K, device=DEV, dtype=dt), weight_div=weight_div)
            for name, m in _masks(rows, seed=K + weight_div).items():
                given = torch.from_numpy(m).to(DEV)
                zp, tokp = z.clone(), tok.clone()
                zp[given] = float("nan")
                tokp[given] = K + 3
                got = ops.token_logprob_bwd(zp, tokp, w, gout, torch.full((rows, K), 7.0, device=DEV, dtype=dt), weight_div=weight_div, given=given)
                again = ops.token_logprob_bwd(zp, tokp, w, gout, torch.empty(rows, K, device=DEV, dtype=dt), weight_div=weight_div, given=given)
                assert torch.equal(_dbits(got), _dbits(again)), (name, "two launches")
                assert torch.equal(_dbits(got)[~given], _dbits(want)[~given]), (name, weight_div, dt, "free rows")
                assert (_dbits(got)[given] == 0).all(), (name, weight_div, dt, "given rows: +0")
                if name == "free":
                    assert torch.equal(_dbits(got), _dbits(want))
    ops.check_device_errors(DEV)


def test_a_null_mask_is_refused_and_nothing_is_launched():
    rows, K = 8, 16
    l = _lib.lib(0)
    z, tok = torch.randn(rows, K, device=DEV), torch.zeros(rows, dtype=torch.int64, device=DEV)
    w, gout, dl = torch.ones(rows, device=DEV), torch.ones(1, device=DEV), torch.full((rows, K), 7.0, device=DEV)
    rc = l.mage_token_logprob_bwd_masked(z.data_ptr(), rows, K, K, tok.data_ptr(), w.data_ptr(), 1, gout.data_ptr(), dl.data_ptr(), 0, None, None)
    assert rc == -1 and b"given" in l.mage_last_error()
    torch.cuda.synchronize()
    assert (dl == 7).all()
