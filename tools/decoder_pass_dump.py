"""The bits of FlatAxialDecoder's passes on seeded synthetic weights: cases a .. i of tools/gen_decoder_plan.py run for real, each through _run
and / or an _inc_begin + _inc_step loop; per case the sha256 of the logits of every call and of every temporal cache at the end of the
incremental loop.  To be compared with another checkout's (a refactor of the passes leaves every hash as it was).

    python tools/decoder_pass_dump.py --out DIR [--tree DIR]        # one checkout (default: this one) with its library, one fresh process (GPU)
    python tools/decoder_pass_dump.py --compare DIR_A DIR_B         # byte for byte; exit status 1 on any difference (no GPU)
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump(tree, out_dir):
    import torch
    from tools import gen_decoder_plan as gen
    assert torch.cuda.is_available(), "decoder_pass_dump.py --out runs the kernels: it needs the GPU"
    mm, ops, config = gen.load(tree)
    sha = lambda t: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()      # noqa: E731
    res, n = {}, 0
    with torch.no_grad():
        for name, spec in gen.decoder_specs().items():
            for loop in spec["loops"]:
                outs, caches = gen.drive(mm, ops, config, spec, loop, dev="cuda:0")
                torch.cuda.synchronize()
                ops.check_device_errors("cuda:0")
                res[f"{name}/{loop}"] = dict(logits=[dict(shape=list(o.shape), finite=bool(torch.isfinite(o).all()), sha256=sha(o)) for o in outs],
                                             caches={str(i): dict(dtype=str(c.dtype), shape=list(c.shape), sha256=sha(c)) for i, c in sorted(caches.items())})
                n += len(outs) + len(caches)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "decoder_pass.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    bad = [k for k, v in res.items() if not all(o["finite"] for o in v["logits"])]
    print(f"{os.path.abspath(tree)}: {len(res)} cases, {n} tensors hashed -> {out_dir}; cases with non-finite logits: {bad}")
    return 1 if bad else 0


def compare(a_dir, b_dir):
    a, b = (json.load(open(os.path.join(d, "decoder_pass.json"))) for d in (a_dir, b_dir))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    n = sum(len(v["logits"]) + len(v["caches"]) for v in a.values())
    same = open(os.path.join(a_dir, "decoder_pass.json"), "rb").read() == open(os.path.join(b_dir, "decoder_pass.json"), "rb").read()
    print(f"{len(a)} / {len(b)} cases, {n} tensors compared; files byte-identical: {same}; mismatching cases: {len(bad)}")
    for k in bad[:40]:
        print("   " + k)
    return 0 if same and not bad else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    assert args.out, "--out DIR [--tree DIR], or --compare DIR_A DIR_B"
    sys.exit(dump(args.tree, args.out))
