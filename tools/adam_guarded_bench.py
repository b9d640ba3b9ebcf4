"""Times mage_adam_guarded (skip of non-finite steps, decoupled decay, EMA) against the launches it stands beside, and the whole step.

    python tools/adam_guarded_bench.py [--out profiles/r22_adam_guarded.txt] [--baseline-root DIR] [--skip-e2e]

(a) The optimizer launches on flat fp32 arenas of 148 MB (cfg2) and 539 MB (caterv1), HIP events around each variant, the variants
    alternating inside each of 31 windows after 3 warm-up windows; us: median (min .. max).  Variants: mage_sumsq + mage_adam_clipped;
    mage_sumsq + mage_adam_guarded with the clip and the guard on (the same bytes); the pair a user would otherwise write for an average,
    the clipped step followed by torch.Tensor.lerp_ over the arena (28 + 12 bytes per element); the guarded step with the EMA fused (36);
    the same with every element decayed; a skipped step (a NaN in the gradient) with and without its mage_sumsq.
(b) policy_loss + backward + FlatAdam.step on cfg2 (16 frames, width 512, 6 layers, K = 512; bf16, 8 clips x 8 candidates), whole steps
    between two synchronisations, ms: median (min .. max) of 7 alternating repeats after 2 warm-ups -- defaults with max_grad_norm, and
    skip_nonfinite + ema_decay + weight_decay on.
--baseline-root DIR (a built checkout of the commit before the feature) times mage_sumsq + mage_adam_clipped and the default step on
THAT tree's package and library, in a child process started after this one's measurements, the same way.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                  # (the child of --baseline-root: import that tree's package instead of this one's)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from mage_amd import ops  # noqa: E402
from mage_amd.optim import FlatAdam  # noqa: E402
from mage_amd.utils import synth  # noqa: E402
from mage_amd.utils.util import instantiate_from_config  # noqa: E402

DEV = "cuda:0"
ARENAS = [("148 MB (cfg2)", 148_000_000 // 4), ("539 MB (caterv1)", 539_000_000 // 4)]
ADAM = dict(lr=1e-5, beta1=0.9, beta2=0.98, eps=1e-6, step=3)
L, CLIPS, CAND = 16, 8, 8


def windows(fns, warm=3, reps=31):
    """Sorted us of each fn: HIP events around one call, the fns alternating inside every window."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        evs = []
        for fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        if r >= warm:
            for t, (e0, e1) in zip(ts, evs):
                t.append(e0.elapsed_time(e1) * 1e3)
    return [sorted(t) for t in ts]


def timed(fns, warm=2, reps=7):
    """Sorted ms of each fn: whole calls between two synchronisations, the fns alternating inside every repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [sorted(t) for t in ts]


def med(t):
    return t[len(t) // 2]


def arena(n):
    g = torch.Generator(DEV).manual_seed(0)
    p, grad, m = (torch.randn(n, device=DEV, generator=g) * s for s in (1.0, 1e-3, 1e-4))
    v = torch.rand(n, device=DEV, generator=g) * 1e-6
    return p, grad, m, v


def kernels(n, baseline):
    p, g, m, v = arena(n)
    norm = torch.zeros(1, device=DEV)

    def clipped():
        ops.adam_clipped(p, g, m, v, sumsq=ops.sumsq(g), max_norm=1.0, norm_out=norm, **ADAM)
    if baseline:
        return dict(clipped=windows([clipped])[0])
    ema = p.clone()
    bad = g.clone()
    bad[n // 2] = float("nan")
    ss_bad = ops.sumsq(bad)
    skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
    guard = dict(max_norm=1.0, skip_nonfinite=True, norm_out=norm, skipped=skipped, **ADAM)
    fns = dict(
        clipped=clipped,
        guarded=lambda: ops.adam_guarded(p, g, m, v, sumsq=ops.sumsq(g), **guard),
        clipped_lerp=lambda: (clipped(), ema.lerp_(p, 0.001)),
        guarded_ema=lambda: ops.adam_guarded(p, g, m, v, ema=ema, ema_decay=0.999, sumsq=ops.sumsq(g), **guard),
        guarded_ema_decay=lambda: ops.adam_guarded(p, g, m, v, ema=ema, ema_decay=0.999, n_decay=n, decay_mul=0.9999, sumsq=ops.sumsq(g), **guard),
        skipped=lambda: ops.adam_guarded(p, bad, m, v, ema=ema, ema_decay=0.999, sumsq=ops.sumsq(bad), **guard),
        skipped_launch=lambda: ops.adam_guarded(p, bad, m, v, ema=ema, ema_decay=0.999, sumsq=ss_bad, **guard),
        sumsq=lambda: ops.sumsq(g),
    )
    out = dict(zip(fns, windows(list(fns.values()))))
    assert torch.isfinite(p).all() and skipped.item() > 0
    return out


def steps(baseline):
    def build(**kw):
        m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
        synth.fill_state_dict(m, 0)
        m = m.to(DEV).set_precision("bf16").set_sampling(1.0)
        return m, FlatAdam(m.parameters(), lr=1e-5, max_grad_norm=1.0, **kw)
    n = CLIPS * CAND
    b = {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(n, L, seed=3).items()}
    built = dict(defaults=build())
    if not baseline:
        built["all_options"] = build(skip_nonfinite=True, ema_decay=0.999, weight_decay=0.01)
    m0 = built["defaults"][0]
    R = m0.image_resolution
    g = torch.Generator(DEV).manual_seed(1)
    tokens = torch.randint(0, m0.codebook_size, (n, L - 1, R, R), device=DEV, generator=g)
    adv = torch.randn(n, device=DEV, generator=g)

    def step(m, opt):
        def f():
            opt.zero_grad()
            m.policy_loss(b, tokens, adv)[0].backward()
            opt.step()
        return f
    return dict(zip(built, timed([step(*mo) for mo in built.values()])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adam_guarded_bench.py measures on the GPU"
    res = {name: kernels(n, bool(a.root)) for name, n in ARENAS}
    torch.cuda.empty_cache()
    e2e = None if a.skip_e2e else steps(bool(a.root))
    if a.root:
        print("BASELINE " + json.dumps(dict(kernels=res, e2e=e2e)))
        return
    row = "{:104s}{:>10.1f}{:>10.1f}{:>10.1f}{:>9s}"
    lines = ["(a) optimizer launches on a flat fp32 arena, HIP events, 31 alternating windows after 3, us: median, min, max; TB/s at the median"]
    labels = [("clipped", "mage_sumsq + mage_adam_clipped", 32), ("guarded", "mage_sumsq + mage_adam_guarded (clip + guard; the same bytes)", 32),
              ("clipped_lerp", "mage_sumsq + mage_adam_clipped, then ema.lerp_(p, 1 - d) (4 + 28 + 12 B per element)", 44),
              ("guarded_ema", "mage_sumsq + mage_adam_guarded with the EMA (4 + 36 B per element)", 40),
              ("guarded_ema_decay", "the same with every element decayed", 40),
              ("skipped", "a skipped step: mage_sumsq + mage_adam_guarded on a gradient holding a NaN", 4),
              ("skipped_launch", "the skipped mage_adam_guarded launch alone (it loads one double)", 0), ("sumsq", "mage_sumsq alone", 4)]
    for name, n in ARENAS:
        lines.append(f"  {name}, n = {n}{'':80s}"[:106] + f"{'us':>8s}{'min':>10s}{'max':>10s}{'TB/s':>9s}")
        for key, text, nbytes in labels:
            t = res[name][key]
            lines.append(row.format("    " + text, med(t), t[0], t[-1], f"{nbytes * n / med(t) * 1e-6:.2f}" if nbytes else ""))
        c, g_, cl, ge = (res[name][k] for k in ("clipped", "guarded", "clipped_lerp", "guarded_ema"))
        lines.append(f"    guarded - clipped {med(g_) - med(c):+.1f} us (spread of clipped, max - min: {c[-1] - c[0]:.1f}); fused EMA - (clipped + lerp_) "
                     f"{med(ge) - med(cl):+.1f} us")
    if e2e:
        lines += [f"(b) policy_loss + backward + FlatAdam.step, cfg2, bf16, {CLIPS * CAND} clips, whole steps between two synchronisations, ms: median, "
                  "min, max of 7 alternating repeats after 2"]
        for key, text in (("defaults", "FlatAdam(max_grad_norm=1.0): mage_sumsq + mage_adam_clipped"),
                          ("all_options", "+ skip_nonfinite, ema_decay=0.999, weight_decay=0.01: mage_sumsq + mage_adam_guarded")):
            t = e2e[key]
            lines.append("{:104s}{:>10.2f}{:>10.2f}{:>10.2f}".format("    " + text, med(t), t[0], t[-1]))
    if a.baseline_root:
        torch.cuda.empty_cache()
        cmd = [sys.executable, os.path.abspath(__file__), "--root", a.baseline_root] + (["--skip-e2e"] if a.skip_e2e else [])
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
        base = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])
        lines.append("(c) the commit before the feature, its own package and library, in a child process on the same visit")
        for name, n in ARENAS:
            t, here, g_ = base["kernels"][name]["clipped"], res[name]["clipped"], res[name]["guarded"]
            lines.append(row.format(f"    {name}: mage_sumsq + mage_adam_clipped", med(t), t[0], t[-1], f"{32 * n / med(t) * 1e-6:.2f}"))
            lines.append(f"      clipped here - there {med(here) - med(t):+.1f} us; guarded here - clipped there {med(g_) - med(t):+.1f} us; spread there "
                         f"(max - min) {t[-1] - t[0]:.1f} us")
        if e2e and base.get("e2e"):
            t = base["e2e"]["defaults"]
            lines.append("{:104s}{:>10.2f}{:>10.2f}{:>10.2f}".format("    the default step, ms", med(t), t[0], t[-1]))
            lines.append(f"      defaults here - there {med(e2e['defaults']) - med(t):+.2f} ms; all options here - there "
                         f"{med(e2e['all_options']) - med(t):+.2f} ms; spread there (max - min) {t[-1] - t[0]:.2f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
