"""Every output of the eight mage_policy_loss* entry points on fixed seeded inputs, written array by array: the bits of one library, to be
compared with another's.

    python tools/policy_family_dump.py --lib PATH --out DIR          # one library, one fresh process (needs the GPU)
    python tools/policy_family_dump.py --compare DIR_A DIR_B         # byte for byte; exit status 1 on any difference (no GPU)

The entry points are called through ctypes on the library at PATH (this tree's bindings: the signatures are the frozen ones).  24 rows at
ld = K + 4 for K in 256, 260, 512, 1028, 2048, 4096 (every rung of MAGE_ROW_LADDER with a ragged tail) x the filters none / top_k 5 /
top_p 0.9 / both x {no reference, a reference with kl_coef 0, with 0.1} x given {none, all free, every third row, rows 0..11: whole groups} x
ratio_div {none, 1, 4, 12}: 1 152 cases.  The remaining two-valued axes -- temperature 1 / 0.7, behaviour_logprob or none (always one
under ratio_div), entropy_coef 0 / 0.01, adv_div = ratio_div (1 without one) / 24 -- are drawn per case from a seeded generator, so each
value meets each of the above many times over.  Every case runs the forward call and its backward call in fp32 and in bf16; the entry
point pair is the one ops.policy_loss would pick.  Rows 1..7 hold a NaN, all -inf but one code, a +inf, an exact tie at the top-k boundary,
a token outside the kept set, a NaN reference and a -inf reference.  One more case, rows = 4096 x K = 256 at ratio_div = 2048, puts the
sixteen-wave group kernel in the comparison.  Outputs start from a sentinel, so an element nobody writes compares equal too."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, KS, TOP_K, TOP_P = 24, (256, 260, 512, 1028, 2048, 4096), 5, 0.9
FILTERS = ((0, 1.0), (TOP_K, 1.0), (0, TOP_P), (TOP_K, TOP_P))
REFS = (None, 0.0, 0.1)                                   # no reference / kl_coef
GIVENS = ("none", "free", "third", "groups")
RATIOS = (None, 1, 4, 12)
CLIP = (0.2, 0.3)
SENTINEL = -7.0


def inputs(rows, K, seed):
    g = np.random.default_rng(seed)
    z = (2.0 * g.standard_normal((rows, K + 4))).astype(np.float32)
    order = np.argsort(-z[:, :K], axis=1, kind="stable")
    tok = order[np.arange(rows), g.integers(0, 3, rows)].astype(np.int64)
    z[1, g.integers(0, K)] = np.nan
    keep = int(tok[2])
    z[2, :K] = -np.inf
    z[2, keep] = 0.25
    z[3, (int(tok[3]) + 1) % K] = np.inf
    z[4, order[4, TOP_K - 1:TOP_K + 2]] = z[4, order[4, TOP_K - 1]]      # ranks 5, 6, 7 tie at the top-k boundary
    tok[5] = order[5, K // 2]                                            # outside top_k 5 and top_p 0.9
    ref = (-1.0 + 0.3 * g.uniform(-1, 1, rows)).astype(np.float32)
    ref[6], ref[7] = np.nan, -np.inf
    blp = (-1.2 + 0.4 * g.uniform(-1, 1, rows)).astype(np.float32)
    adv = (g.uniform(0.5, 2.0, rows) * g.choice([-1.0, 1.0], rows)).astype(np.float32)
    return z, tok, adv, blp, ref


def mask(kind, rows):
    m = np.zeros(rows, bool)
    if kind == "third":
        m[::3] = True
    if kind == "groups":
        m[:rows // 2] = True
    return None if kind == "none" else m


def dump(lib_path, out_dir):
    import torch
    from mage_amd import _lib, ops
    assert torch.cuda.is_available(), "policy_family_dump.py --lib runs the kernels: it needs the GPU"
    _lib.load(os.path.abspath(lib_path))                  # before anything else asks for the default library
    l = _lib.lib(0)
    dev, F32, BF16 = "cuda:0", ops.F32, ops.BF16
    s = torch.cuda.current_stream().cuda_stream
    os.makedirs(out_dir, exist_ok=True)
    manifest, n_arrays = [], 0
    p = lambda t: None if t is None else t.data_ptr()     # noqa: E731

    def save(case, name, t):
        nonlocal n_arrays
        a = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
        np.save(os.path.join(out_dir, f"{case:05d}_{name}.npy"), a.cpu().numpy())
        n_arrays += 1

    def run(case, rows, K, zs, top_k, top_p, kl_coef, given_kind, ratio, T, use_blp, ent, adv_div):
        z, tok, adv, blp, ref = (torch.from_numpy(x).to(dev) for x in zs)
        ld = z.shape[1]
        adv = adv[:rows // adv_div].contiguous()
        blp = blp if use_blp else None
        ref = None if kl_coef is None else ref
        m = mask(given_kind, rows)
        given = None if m is None else torch.from_numpy(m).to(dev)
        form = "grouped" if ratio is not None else "masked" if given is not None else "anchored" if ref is not None else "plain"
        mk = lambda n, dt=torch.float32: torch.full((n,), SENTINEL, device=dev).to(dt)      # noqa: E731
        o = dict(row_loss=mk(rows), logprob=mk(rows), entropy=mk(rows), cut=mk(rows, torch.int32), summary=mk({"plain": 5, "anchored": 7}.get(form, 8)))
        if ref is not None:
            o["kl"] = mk(rows)
        if form in ("masked", "grouped"):
            o["norm"] = mk(1)
        if form == "grouped":
            o.update(group_logratio=mk(rows // ratio), group_count=mk(rows // ratio, torch.int32))
        head = [z.data_ptr(), rows, K, ld, tok.data_ptr(), adv.data_ptr(), adv_div, p(blp)]
        kl = 0.0 if kl_coef is None else kl_coef
        plain = form == "plain"
        a = head + ([] if plain else [p(ref)]) + [T, top_k, top_p, CLIP[0], CLIP[1], ent] + ([] if plain else [kl])
        a += [o[k].data_ptr() for k in ("row_loss", "logprob", "entropy", "cut")] + ([] if plain else [p(o.get("kl"))]) + [o["summary"].data_ptr()]
        if form in ("masked", "grouped"):
            a += [o["norm"].data_ptr(), p(given)]
        if form == "grouped":
            a += [ratio, o["group_logratio"].data_ptr(), o["group_count"].data_ptr()]
        entry = "mage_policy_loss" + ("" if plain else "_" + form)
        _lib.check(getattr(l, entry)(*a, s), l)
        for k, t in o.items():
            save(case, f"{entry}.{k}", t)
        gout = torch.tensor([0.7], device=dev)
        for code, dt in ((F32, torch.float32), (BF16, torch.bfloat16)):
            dl = torch.full((rows, K), SENTINEL, device=dev).to(dt)
            a = head + ([] if plain else [p(ref)]) + [o["cut"].data_ptr(), T, CLIP[0], CLIP[1], ent] + ([] if plain else [kl]) + [gout.data_ptr()]
            a += ([o["norm"].data_ptr()] if form in ("masked", "grouped") else []) + [dl.data_ptr(), code]
            if form in ("masked", "grouped"):
                a += [p(given)]
            if form == "grouped":
                a += [ratio, o["group_logratio"].data_ptr()]
            _lib.check(getattr(l, entry + "_bwd")(*a, s), l)
            save(case, f"{entry}_bwd.dlogits_{'f32' if code == F32 else 'bf16'}", dl)
        manifest.append(dict(case=case, entry=entry, rows=rows, K=K, top_k=top_k, top_p=top_p, kl_coef=kl_coef, given=given_kind, ratio_div=ratio,
                             temperature=T, behaviour=use_blp, entropy_coef=ent, adv_div=adv_div))

    pick = np.random.default_rng(21)
    case = 0
    for K in KS:
        zs = inputs(ROWS, K, seed=K)
        for (top_k, top_p), kl_coef, given_kind, ratio in itertools.product(FILTERS, REFS, GIVENS, RATIOS):
            bits = pick.integers(0, 2, 4)
            run(case, ROWS, K, zs, top_k, top_p, kl_coef, given_kind, ratio, (1.0, 0.7)[bits[0]], bool(bits[1]) or ratio is not None,
                (0.0, 0.01)[bits[2]], (ratio or 1, ROWS)[bits[3]])
            case += 1
    run(case, 4096, 256, inputs(4096, 256, seed=7), TOP_K, TOP_P, 0.1, "third", 2048, 0.7, True, 0.01, 2048)
    torch.cuda.synchronize()
    ops.check_device_errors(dev)
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f)
    print(f"{lib_path}: {case + 1} cases, {3 * (case + 1)} entry point calls, {n_arrays} arrays -> {out_dir}")


def compare(a_dir, b_dir):
    a, b = (sorted(f for f in os.listdir(d) if f.endswith(".npy")) for d in (a_dir, b_dir))
    bad = sorted(set(a) ^ set(b))
    n_bytes = 0
    for f in sorted(set(a) & set(b)):
        x, y = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
        n_bytes += x.nbytes
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(f)
    same_cases = open(os.path.join(a_dir, "manifest.json")).read() == open(os.path.join(b_dir, "manifest.json")).read()
    print(f"{len(set(a) & set(b))} arrays, {n_bytes} bytes compared; the same cases on both sides: {same_cases}; mismatching arrays: {len(bad)}")
    for f in bad[:40]:
        print("   " + f)
    return 0 if not bad and same_cases else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    assert args.lib and args.out, "--lib PATH --out DIR, or --compare DIR_A DIR_B"
    dump(args.lib, args.out)
