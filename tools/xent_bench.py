"""Times the supervised-loss kernels (mage_token_xent / _bwd) beside mage_cross_entropy / _bwd, and one cfg2 training step with and without
MAGE.set_loss options.

    python tools/xent_bench.py [--out profiles/r31_xent.txt] [--baseline-root DIR] [--only NAME]

cfg2 (16 frames, width 512, 6 layers, K = 512), bf16, 64 clips: 64 x 15 x 256 = 245 760 rows of 512 logits.  Every number is the median
(min .. max) of five repeats after two warm-ups, the variants alternating inside every repeat.
(a) The kernels on one set of buffers, HIP events around ten calls (us per call): mage_token_xent + mage_token_xent_bwd (bf16 gradients) with
    every option off and with all on (label_smoothing 0.1, z_loss 1e-3, class weights, no mask), beside mage_cross_entropy +
    mage_cross_entropy_bwd on the same buffers, with the bytes each pair must move (one fp32 read per pass, one bf16 write).
(b) One training step (MAGE.forward, loss.backward(), FlatAdam.step()), whole steps between two synchronisations (ms): the defaults
    (mage_cross_entropy: the launches of the commit before) and all options on.
--baseline-root DIR (a built checkout of the commit before the feature) times the default step on THAT tree's package and library in a
child process started after this one's measurements, then this tree's in a child process of its own, then DIR's again, all the same way:
the default step here runs the same launches, so the trees should differ by less than the call-to-call spread, which is printed beside
them, and a process differs from the next by what the two runs of DIR show.  --only NAME runs one step variant in a loop of five steps after two
warm-ups and prints nothing else: the command a profiler wraps (default, options).
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
L, K, CLIPS = 16, 512, 64
EPS, ZETA = 0.1, 1e-3


def timed(fns, warm=2, reps=5):
    """Sorted ms of each fn: whole calls between two synchronisations, the fns alternating inside every repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [sorted(t) for t in ts]


def timed_events(fns, inner=10, warm=2, reps=5):
    """Sorted us per call of each fn: HIP events around `inner` calls, the fns alternating inside every repeat."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                ts[i].append(e0.elapsed_time(e1) * 1e3 / inner)
    return [sorted(t) for t in ts]


def med(t):
    return t[len(t) // 2]


def model_and_batch():
    m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).train()
    synth.fill_state_dict(m, 0)
    m = m.to(DEV).set_precision("bf16")
    b = {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(CLIPS, L, seed=3).items()}
    return m, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--only", default=None, choices=["default", "options"])
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "xent_bench.py measures on the GPU"
    m, b = model_and_batch()
    opt = FlatAdam(m.parameters(), lr=1e-5)

    def step():
        opt.zero_grad()
        loss, _ = m(b)
        loss.backward()
        opt.step()
    if a.root:                                            # the child: the tree at --root, its default step only
        (t0,) = timed([step])
        print("BASELINE " + json.dumps(dict(step=t0)))
        return
    from mage_amd.utils.glue import balanced_class_weights
    tok = m.first_stage_encode(b["images"])
    weights = balanced_class_weights(torch.bincount(tok.reshape(-1), minlength=K))

    options = m.set_loss(EPS, ZETA, weights).loss_options   # validated once, as a training loop does; the variants then only switch it
    m.set_loss()

    def with_options():
        m.loss_options = options
        step()
        m.loss_options = None
    variants = {"default": step, "options": with_options}
    if a.only:
        for _ in range(7):
            variants[a.only]()
        torch.cuda.synchronize()
        return
    # the kernels alone, on one set of buffers
    rows = tok[:, 1:].numel()
    g = torch.Generator(DEV).manual_seed(2)
    logits = torch.randn(rows, K, device=DEV, generator=g) * 2
    tgt = tok[:, 1:].reshape(-1).contiguous()
    dl16 = torch.empty(rows, K, device=DEV, dtype=torch.bfloat16)
    gout = torch.ones(1, device=DEV)
    on = dict(class_weight=weights, label_smoothing=EPS, z_loss=ZETA)
    norm = ops.token_xent(logits, tgt, rank=False)["norm"]
    norm_on = ops.token_xent(logits, tgt, rank=False, **on)["norm"]

    def pair_off():
        ops.token_xent(logits, tgt, rank=False)
        ops.token_xent_bwd(logits, tgt, norm, gout, dl16)

    def pair_on():
        ops.token_xent(logits, tgt, rank=False, **on)
        ops.token_xent_bwd(logits, tgt, norm_on, gout, dl16, **on)

    def pair_ce():
        ops.cross_entropy(logits, tgt)
        ops.cross_entropy_bwd(logits, tgt, gout, dl16)
    kern = [("mage_token_xent + mage_token_xent_bwd, every option off", pair_off),
            (f"mage_token_xent + mage_token_xent_bwd, label_smoothing {EPS}, z_loss {ZETA}, class weights", pair_on),
            ("mage_cross_entropy + mage_cross_entropy_bwd: the yardstick", pair_ce)]
    ks = timed_events([k[1] for k in kern])
    mb = rows * K * (4 + 4 + 2) / 1e6                     # two fp32 reads of the logits, one bf16 write of the gradient
    f2 = "{:100s}{:>10.2f}{:>10.2f}{:>10.2f}"
    lines = [f"cfg2 (16 frames, width 512, 6 layers), bf16, {CLIPS} clips = {rows} rows x {K}; median, min, max of 5 alternating repeats after 2 "
             "warm-ups",
             f"{'':100s}{'median':>10s}{'min':>10s}{'max':>10s}",
             f"(a) forward + backward kernels on one set of buffers (bf16 gradients), HIP events around 10 pairs, us per pair; a pair moves {mb:.0f} MB"]
    for (name, _), t in zip(kern, ks):
        lines += [f2.format("   " + name, med(t), t[0], t[-1]), f"      {mb / med(t):.2f} TB/s at the median; spread (max - min) {t[-1] - t[0]:.2f} us"]
    lines.append(f"   options off - yardstick {med(ks[0]) - med(ks[2]):+.2f} us; all on - off {med(ks[1]) - med(ks[0]):+.2f} us")
    td, to = timed([variants["default"], variants["options"]])
    lines += ["(b) one training step (forward, backward, FlatAdam.step), whole steps between two synchronisations, ms",
              f2.format("   defaults (mage_cross_entropy: the launches of the commit before)", med(td), td[0], td[-1]),
              f2.format(f"   set_loss({EPS}, {ZETA}, balanced class weights)", med(to), to[0], to[-1]),
              f"   options - defaults {med(to) - med(td):+.3f} ms; spread (max - min, the larger of the two) {max(td[-1] - td[0], to[-1] - to[0]):.3f} ms"]
    if a.baseline_root:
        del m, b, opt, logits, dl16
        torch.cuda.empty_cache()
        child = lambda root: json.loads([ln for ln in subprocess.run(      # noqa: E731
            [sys.executable, os.path.abspath(__file__), "--root", root], check=True, capture_output=True, text=True,
            timeout=600).stdout.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])["step"]
        tb, tc, tb2 = child(a.baseline_root), child(ROOT), child(a.baseline_root)
        spread = max(t[-1] - t[0] for t in (tb, tc, tb2))
        lines += ["(c) the default step in child processes on the same visit, one after the other: the commit before the feature (its own package "
                  "and library), this tree, the commit before again",
                  f2.format("   the commit before, ms", med(tb), tb[0], tb[-1]),
                  f2.format("   this tree, ms", med(tc), tc[0], tc[-1]),
                  f2.format("   the commit before, second run, ms", med(tb2), tb2[0], tb2[-1]),
                  f"   this tree - the commit before {med(tc) - med(tb):+.3f} and {med(tc) - med(tb2):+.3f} ms; the commit before against itself "
                  f"{med(tb2) - med(tb):+.3f} ms; largest call-to-call spread (max - min) of the three {spread:.3f} ms: "
                  f"{'inside' if max(abs(med(tc) - med(tb)), abs(med(tc) - med(tb2))) <= spread else 'OUTSIDE'} it",
                  f"   this process's default step (b) - this tree's child {med(td) - med(tc):+.3f} ms: the process-to-process difference"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
