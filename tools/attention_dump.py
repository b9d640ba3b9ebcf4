"""The bits of mage_attention at the dispatch edges: every case of CASES and FEWQ_IDENTITY of tests/test_gpu_attention.py through that
file's launch (the identity cases also with the option attn_no_fewq: the workgroup kernel at the few-query shapes); per case the sha256 of
the whole output buffer, sentinels included.  To be compared with another checkout's (a refactor of the kernels leaves every hash as it was).

    python tools/attention_dump.py --out DIR [--tree DIR]        # one checkout (default: this one) with its library, one fresh process (GPU)
    python tools/attention_dump.py --compare DIR_A DIR_B         # byte for byte; exit status 1 on any difference (no GPU)
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "attention.json"


def dump(tree, out_dir):
    import torch
    assert torch.cuda.is_available(), "attention_dump.py --out runs the kernels: it needs the GPU"
    assert "mage_amd" not in sys.modules, "another checkout's mage_amd is already imported: one tree per process"
    sys.path.insert(0, os.path.abspath(tree))
    t = importlib.import_module("tests.test_gpu_attention")
    config = importlib.import_module("mage_amd.config")
    sha = lambda o: hashlib.sha256(o.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()      # noqa: E731
    cases, identity = ([p.values[0] for p in ps] for ps in (t.CASES + t.FEWQ_IDENTITY, t.FEWQ_IDENTITY))      # pytest.param(dict, id=name)
    res = {c["name"]: sha(t.launch(c)[0]) for c in cases}
    with config.lib_option("attn_no_fewq", 1):
        res.update({c["name"] + "/attn_no_fewq": sha(t.launch(c)[0]) for c in identity})
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, NAME), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"{os.path.abspath(tree)}: {len(res)} output buffers hashed -> {out_dir}")
    return 0


def compare(a_dir, b_dir):
    a, b = (json.load(open(os.path.join(d, NAME))) for d in (a_dir, b_dir))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"{len(a)} / {len(b)} output buffers compared; mismatching: {len(bad)}")
    for k in bad:
        print("   " + k)
    return 1 if bad else 0


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
