"""The bits of one training step on seeded synthetic weights: cases a, b, d, e and g of tools/gen_train_plan.py run for real.  Per case torch is
seeded, then ``loss, _ = model(batch); loss.backward()`` (VQ-VAE: the stage-1 loss mse(x_tilde, x) + mse(z_q, z_e.detach()) +
2 mse(z_e, z_q.detach())); the sha256 of the loss and of every parameter's .grad is written.  To be compared with another checkout's (a refactor
of the training modules leaves every hash as it was), or with a second run of the same checkout (the training sums are fixed-order; the
f4 VQ-VAE's codebook gradient, an unordered scatter, is the one tensor that moves by an ulp from run to run).

    python tools/train_pass_dump.py --out DIR [--tree DIR] [--save CASE:PARAMETER ...]      # one checkout (default: this one) with its library,
                                                                                            # one fresh process (GPU)
    python tools/train_pass_dump.py --compare DIR_A DIR_B         # byte for byte; exit status 1 on any difference (no GPU)

--save keeps the named gradients themselves beside the hashes (DIR/saved/): for a tensor that differs between two runs of the SAME checkout
(a scatter whose additions are not ordered).  --compare prints, for a mismatching tensor both sides saved, the largest difference, to be held
against that checkout's own run-to-run spread; the exit status stays 1.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TIME_LIMIT = 300          # seconds for one checkout's process: the cases take seconds each


def dump(tree, out_dir, save=()):
    import torch
    import torch.nn.functional as F
    from tools import gen_train_plan as gen
    assert torch.cuda.is_available(), "train_pass_dump.py --out runs the kernels: it needs the GPU"
    m, dev = gen.load(tree), "cuda:0"
    sha = lambda t: hashlib.sha256(t.detach().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()      # noqa: E731
    res, n = {}, 0
    for name, spec in gen.specs().items():
        if name[0] not in "abdeg":
            continue
        torch.manual_seed(47)
        if spec["kind"] == "vq":
            model, x = gen.vq_setup(m, spec, dev)
            model.zero_grad()
            x_tilde, z_e, z_q = model(x)
            loss = F.mse_loss(x_tilde, x) + F.mse_loss(z_q, z_e.detach()) + 2.0 * F.mse_loss(z_e, z_q.detach())
        else:
            model, batch = gen.mage_setup(m, spec, dev)
            model.zero_grad()
            with m.config.override(**gen.CONFIG_DEFAULTS):
                loss, _ = model(batch)
        with m.config.override(**gen.CONFIG_DEFAULTS):
            loss.backward()
        torch.cuda.synchronize()
        m.ops.check_device_errors(dev)
        grads = {k: "none" if p.grad is None else sha(p.grad) for k, p in model.named_parameters()}
        finite = bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
        for key in save:
            case, param = key.split(":")
            if case == name:
                os.makedirs(os.path.join(out_dir, "saved"), exist_ok=True)
                torch.save(dict(model.named_parameters())[param].grad.cpu(), os.path.join(out_dir, "saved", f"{case}__{param}.pt"))
        res[name] = dict(loss=sha(loss), loss_value=loss.item(), finite=finite, grads=grads)
        n += 1 + len(grads)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "train_pass.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    bad = [k for k, v in res.items() if not v["finite"]]
    print(f"{os.path.abspath(tree)}: {len(res)} cases, {n} tensors hashed -> {out_dir}; cases with a non-finite loss or gradient: {bad}")
    return 1 if bad else 0


def compare(a_dir, b_dir):
    a, b = (json.load(open(os.path.join(d, "train_pass.json"))) for d in (a_dir, b_dir))
    n = sum(1 + len(v["grads"]) for v in a.values())
    same = open(os.path.join(a_dir, "train_pass.json"), "rb").read() == open(os.path.join(b_dir, "train_pass.json"), "rb").read()
    bad = []
    for k in sorted(set(a) | set(b)):
        va, vb = a.get(k, {}), b.get(k, {})
        if va.get("loss") != vb.get("loss"):
            bad.append(f"{k}: loss")
        ga, gb = va.get("grads", {}), vb.get("grads", {})
        bad += [f"{k}: {p}.grad" for p in sorted(set(ga) | set(gb)) if ga.get(p) != gb.get(p)]
    print(f"{len(a)} / {len(b)} cases, {n} tensors compared; files byte-identical: {same}; mismatching tensors: {len(bad)}")
    for k in bad[:40]:
        print("   " + k)
        saved = [os.path.join(d, "saved", k.replace(": ", "__")[:-len(".grad")] + ".pt") for d in (a_dir, b_dir)]
        if all(os.path.exists(f) for f in saved):
            import torch
            ta, tb = (torch.load(f).double() for f in saved)
            print(f"      saved on both sides: max |a - b| = {(ta - tb).abs().max().item():.3e}, max |a| = {ta.abs().max().item():.3e}, "
                  f"elements that differ: {int((ta != tb).sum())} of {ta.numel()}")
    return 0 if same and not bad else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--save", nargs="*", default=[], metavar="CASE:PARAMETER")
    ap.add_argument("--in-process", action="store_true", help="what --out starts: the dump itself, in this process")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    assert args.out, "--out DIR [--tree DIR], or --compare DIR_A DIR_B"
    if args.in_process:
        sys.exit(dump(args.tree, args.out, args.save))
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--in-process", "--tree", args.tree, "--out", args.out, "--save",
                             *args.save], timeout=TIME_LIMIT).returncode)
