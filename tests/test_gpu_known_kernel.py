"""GPU: mage_apply_known_tokens (include/mage_hip_ext.h) against the numpy restatement of its rule (tests/known_ref.py), bit for bit.
Every output is pre-filled with sentinels: a free slot, the gaps of a strided launch and the three entries past the last mapped index must
stay untouched.  Shapes: rows that are no multiple of the 256-thread block, group 1 / odd / 256, a clip's candidates sharing one known row
(known_clip_div 1 and 3), the full loop's strided addressing and the incremental loop's packed one."""
import numpy as np
import pytest
import torch

from mage_amd import _lib, ops
from tests import known_ref as KR
from tests.helpers import SENTINEL, bits, refused, sent, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 64
TOK_SENT = -0x0123456789ABCDEF                                      # no token and no known value looks like this
NAMES = [n for n, _, _ in KR.RESULTS]

# name -> (rows, group, tok_group_stride, tok_off, known_group_stride, known_off, known_clip_div)
CASES = {
    "one row": (1, 1, 1, 0, 1, 0, 1),
    "group 1": (7, 1, 1, 0, 1, 0, 1),
    "group 1, three candidates": (7, 1, 1, 0, 1, 0, 3),
    "odd group, odd rows": (5 * 53 + 2, 5, 5, 0, 5, 0, 1),          # 267 rows: two blocks, the second holds 11; the last group is partial
    "packed, three candidates": (6 * 256, 256, 256, 0, 5 * 256, 2 * 256, 3),       # the incremental loop: frame 2 of 2 clips x 3 candidates
    "strided, three candidates": (6 * 5, 5, 5 * 5, 3 * 5, 5 * 5, 3 * 5, 3),        # the full loop: slot 3 of [6, 5, group 5]
    "strided, group 256": (3 * 256, 256, 5 * 256, 256, 5 * 256, 256, 1),
    "all frames at once": (3 * 40 + 1, 40, 40, 0, 40, 0, 1),
}


def call(tokens, rows, group, ts, toff, known, ks, koff, kdiv, k=K, res=()):
    """The raw entry point; every pointer argument is a tensor, an address, or None."""
    lib = _lib.lib(0)
    p = lambda t: t.data_ptr() if torch.is_tensor(t) else t        # noqa: E731
    res = list(res) + [None] * (5 - len(res))
    with torch.cuda.device(0):
        _lib.check(lib.mage_apply_known_tokens(p(tokens), rows, group, ts, toff, p(known), ks, koff, kdiv, k, *[p(r) for r in res],
                                               torch.cuda.current_stream().cuda_stream), lib)


def buffers(name, fill="mixed"):
    rows, group, ts, toff, ks, koff, kdiv = CASES[name]
    t, kix = KR.indices(rows, group, ts, toff, ks, koff, kdiv)
    n_tok, n_known = int(t.max()) + 1 + 3, int(kix.max()) + 1       # three entries past the last mapped index
    g = np.random.default_rng(sum(map(ord, name)))
    if fill == "free":
        known = -1 - g.integers(0, 4, n_known)                      # -1 .. -4
    elif fill == "set":
        known = g.integers(0, K, n_known)
    else:
        known = np.where(g.random(n_known) < 0.4, g.integers(0, K, n_known), -1 - g.integers(0, 4, n_known))
    return t, kix, n_tok, known.astype(np.int64)


def fresh(n_tok, which):
    tokens = torch.full((n_tok,), TOK_SENT, dtype=torch.int64, device=DEV)
    res = [sent(n_tok, torch.float32) if n in which else None for n in NAMES]       # (kept's int32 entries under the same 32-bit sentinel)
    return tokens, res


def sent_np(n, dt):
    return np.full(n, SENTINEL[torch.float32][1], np.int32).view(dt)


def check(name, fill, which):
    rows, group, ts, toff, ks, koff, kdiv = CASES[name]
    t, kix, n_tok, known = buffers(name, fill)
    tokens, res = fresh(n_tok, which)
    call(tokens, rows, group, ts, toff, torch.from_numpy(known).to(DEV), ks, koff, kdiv, res=res)
    torch.cuda.synchronize()
    ref_res = {n: sent_np(n_tok, dt) if n in which else None for n, dt, _ in KR.RESULTS}
    want, want_res, bad = KR.apply_known(np.full(n_tok, TOK_SENT, np.int64), known, rows=rows, group=group, K=K, tok_group_stride=ts, tok_off=toff,
                                         known_group_stride=ks, known_off=koff, known_clip_div=kdiv, **ref_res)
    assert bad == 0
    assert np.array_equal(tokens.cpu().numpy(), want), f"{name} {fill}: tokens differ from the rule"
    for n, r in zip(NAMES, res):
        if r is not None:
            assert np.array_equal(bits(r).cpu().numpy(), want_res[n].view(np.int32)), f"{name} {fill}: {n} differs from the rule"
    forced = np.zeros(n_tok, bool)
    forced[t[known[kix] >= 0]] = True
    fd = torch.from_numpy(forced).to(DEV)
    assert bool((tokens[~fd] == TOK_SENT).all()) and all(r is None or untouched(r[~fd]) for r in res), f"{name} {fill}: a store left its slots"
    assert bool((tokens[-3:] == TOK_SENT).all()) and all(r is None or untouched(r[-3:]) for r in res)
    ops.check_device_errors(torch.device(DEV))
    return tokens, res, forced


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_rule_bit_for_bit_and_writes_only_forced_slots(name):
    _, res, forced = check(name, "mixed", NAMES)
    assert forced.any() or CASES[name][0] == 1
    if forced.any():
        f = torch.from_numpy(forced).to(DEV)
        assert bool((bits(res[0])[f] == 0).all()) and bool((bits(res[4])[f] == 1).all())    # +0.0 and 1, exactly


@pytest.mark.parametrize("name", ["odd group, odd rows", "strided, three candidates", "packed, three candidates"])
def test_all_free_changes_nothing_and_all_set_fills_every_mapped_slot(name):
    tokens, res, forced = check(name, "free", NAMES)
    assert not forced.any() and bool((tokens == TOK_SENT).all()) and all(untouched(r) for r in res)
    tokens, res, forced = check(name, "set", NAMES)
    t = buffers(name, "set")[0]
    assert forced[t].all() and bool((tokens[torch.from_numpy(t).to(DEV)] >= 0).all())


@pytest.mark.parametrize("which", [[n for n in NAMES if n != out] for out in NAMES] + [[]], ids=[f"no {n}" for n in NAMES] + ["no results"])
def test_each_result_pointer_may_be_null(which):
    check("odd group, odd rows", "mixed", which)
    check("strided, three candidates", "mixed", which)


def test_a_value_past_the_codebook_is_clamped_and_reported():
    name = "odd group, odd rows"
    rows, group, ts, toff, ks, koff, kdiv = CASES[name]
    t, kix, n_tok, known = buffers(name)
    known[kix[100]] = K                                             # the smallest bad value
    tokens, res = fresh(n_tok, NAMES)
    call(tokens, rows, group, ts, toff, torch.from_numpy(known).to(DEV), ks, koff, kdiv, res=res)
    torch.cuda.synchronize()
    want, _, bad = KR.apply_known(np.full(n_tok, TOK_SENT, np.int64), known, rows=rows, group=group, K=K)
    assert bad == 1 and want[t[100]] == K - 1 and np.array_equal(tokens.cpu().numpy(), want)
    assert float(res[0][t[100]]) == 0.0 and int(bits(res[4])[t[100]]) == 1
    with pytest.raises(ValueError):
        ops.check_device_errors(torch.device(DEV))
    ops.check_device_errors(torch.device(DEV))                      # reported once, then clear


def test_the_wrapper_addresses_like_the_raw_call():
    name = "strided, three candidates"
    rows, group, ts, toff, ks, koff, kdiv = CASES[name]
    t, kix, n_tok, known = buffers(name)
    kd = torch.from_numpy(known).to(DEV)
    a, ra = fresh(n_tok, NAMES)
    call(a, rows, group, ts, toff, kd, ks, koff, kdiv, res=ra)
    b, rb = fresh(n_tok, NAMES)
    got = ops.apply_known_tokens(b, kd, rows=rows, K=K, group=group, tok_group_stride=ts, tok_off=toff, known_group_stride=ks, known_off=koff,
                                 known_clip_div=kdiv, **{n: r.view(torch.int32) if n == "kept" else r for n, r in zip(NAMES, rb)})
    assert got is b and torch.equal(a, b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(ra, rb))
    with pytest.raises(AssertionError):                             # one row more than the buffers hold
        ops.apply_known_tokens(b[:t.max() + 1], kd, rows=rows + group, K=K, group=group, tok_group_stride=ts, tok_off=toff,
                               known_group_stride=ks, known_off=koff, known_clip_div=kdiv)


def test_refusals_launch_nothing():
    rows, group = 12, 4
    tokens = torch.full((rows + 3,), TOK_SENT, dtype=torch.int64, device=DEV)
    canary = sent(rows + 3, torch.float32)
    known = torch.arange(rows + 3, dtype=torch.int64, device=DEV) % K
    ok = dict(tokens=tokens, rows=rows, group=group, ts=group, toff=0, known=known, ks=group, koff=0, kdiv=1, k=K, res=[canary])
    bad = [dict(tokens=None), dict(known=None), dict(rows=-1), dict(group=0), dict(group=-3), dict(kdiv=0), dict(kdiv=-1), dict(ts=-1),
           dict(toff=-1), dict(ks=-1), dict(koff=-1), dict(k=0), dict(k=-64)]
    for b in bad:
        refused(lambda b=b: call(**{**ok, **b}), canary)
        assert bool((tokens == TOK_SENT).all())
    call(**{**ok, "rows": 0})                                       # a no-op, not an error
    torch.cuda.synchronize()
    assert untouched(canary) and bool((tokens == TOK_SENT).all())
    call(**ok)                                                      # the same arguments unbroken: accepted
    torch.cuda.synchronize()
    assert torch.equal(tokens[:rows], known[:rows]) and bool((tokens[rows:] == TOK_SENT).all())
    assert bool((canary[:rows] == 0).all()) and untouched(canary[rows:])
