"""Times generation with given frames and tokens (MAGE.set_context, batch['known_tokens'], MAGE.generate_long) against the plain call.

    python tools/context_bench.py [--out profiles/r15_context.txt] [--baseline-root DIR] [--clips 64] [--only NAME]

cfg2 (16 frames, width 512, 6 layers), bf16, incremental, eager, B = --clips.  Every number is a whole call between two synchronisations
(wall clock, ms): median (min .. max) of five repeats after two warm-ups, the variants alternating inside every repeat.
(a) The cost of the switch: the unconstrained call, and the call with an all-free known_tokens -- the same tokens, L-1 more launches
    (mage_apply_known_tokens) and the input checks.  The kernel alone at one frame's size, with HIP events, 50 repeats after 10.
(b) The prefill: set_context(8) with the anchor and the 8 given frames as one window, against the one-position-at-a-time form
    (context_prefill = False) and against the unconstrained call.
(c) generate_long(frames = 46, overlap = 1): three windows, against three plain calls (what the chain costs without the device hand-over is
    those plus two VQ encodes of a frame and the host's work between them).
--baseline-root DIR (a built checkout of the commit before the feature) times the unconstrained call on THAT tree's package and library, in a
child process started after this one's measurements, the same way.  --only NAME runs one variant in a loop of five calls after two warm-ups
and prints nothing else: the command a profiler wraps (plain, free, prefill, steps, long).
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
from mage_amd.utils import synth  # noqa: E402
from mage_amd.utils.util import instantiate_from_config  # noqa: E402

DEV = "cuda:0"
L, K = 16, 512


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


def med(t):
    return t[len(t) // 2]


def model_and_batch(n):
    m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
    synth.fill_state_dict(m, 0)
    m = m.to(DEV).set_precision("bf16")
    m.use_graph, m.ar_mode, m.streams = False, "incremental", 1
    return m, {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(n, L, seed=3).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--only", default=None, choices=["plain", "free", "prefill", "steps", "long"])
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "context_bench.py measures on the GPU"
    n = a.clips
    m, b = model_and_batch(n)
    plain = lambda: m.autoregressive_generate(b)          # noqa: E731
    if a.root:                                            # the child: the tree at --root, the yardstick only
        (tp,) = timed([plain])
        print("BASELINE " + json.dumps(dict(plain=tp)))
        return
    R = m.image_resolution
    free = {**b, "known_tokens": torch.full((n, L - 1, R, R), -1, dtype=torch.int64, device=DEV)}

    def ctx(k, prefill):
        def f():
            m.set_context(k)
            m.context_prefill = prefill
            try:
                return m.autoregressive_generate(b)
            finally:
                m.set_context(1)
                m.context_prefill = True
        return f
    variants = {"plain": plain, "free": lambda: m.autoregressive_generate(free), "prefill": ctx(8, True), "steps": ctx(8, False),
                "long": lambda: m.generate_long(b, frames=3 * L - 2, overlap=1)}
    if a.only:
        for _ in range(7):
            variants[a.only]()
        torch.cuda.synchronize()
        return
    f2 = "{:100s}{:>10.2f}{:>10.2f}{:>10.2f}"
    sp = lambda *ts: max(t[-1] - t[0] for t in ts)        # noqa: E731
    tp, tf = timed([plain, variants["free"]])
    tokens = torch.zeros(n * R * R, dtype=torch.int64, device=DEV)
    known = free["known_tokens"].view(-1)
    evs = []
    for i in range(60):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.apply_known_tokens(tokens, known, rows=n * R * R, K=K, group=R * R, known_group_stride=(L - 1) * R * R, known_off=3 * R * R)
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    tk = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs[10:])
    lines = [f"cfg2 (16 frames, width 512, 6 layers), bf16, incremental, eager, B = {n}; whole calls between two synchronisations, ms: median, min, "
             "max of 5 alternating repeats after 2 warm-ups",
             f"{'':100s}{'ms':>10s}{'min':>10s}{'max':>10s}",
             "(a) the cost of the switch",
             f2.format("   unconstrained call", med(tp), tp[0], tp[-1]),
             f2.format("   all-free known_tokens (the same tokens; 15 mage_apply_known_tokens launches and the input checks more)", med(tf), tf[0], tf[-1]),
             f"   difference {med(tf) - med(tp):+.3f} ms against a call-to-call spread (max - min, the larger of the two) of {sp(tp, tf):.3f} ms",
             f"   mage_apply_known_tokens alone, one frame of {n} clips ({n * R * R} rows, all free), HIP events, 50 repeats after 10: "
             f"{med(tk):.1f} us (min {tk[0]:.1f}, max {tk[-1]:.1f}) -> 15 launches {15 * med(tk) / 1e3:.3f} ms"]
    t8, t1, tp2 = timed([variants["prefill"], variants["steps"], plain])
    lines += ["(b) set_context(8): frames 8 .. 15 generated, 8 decoder steps instead of 15",
              f2.format("   prefilled: the anchor and the 8 given frames as ONE 9-position window", med(t8), t8[0], t8[-1]),
              f2.format("   one position at a time, no pick (context_prefill = False)", med(t1), t1[0], t1[-1]),
              f2.format("   unconstrained call (15 steps)", med(tp2), tp2[0], tp2[-1]),
              f"   prefilled - one at a time {med(t8) - med(t1):+.3f} ms; prefilled - unconstrained {med(t8) - med(tp2):+.3f} ms; spread "
              f"{sp(t8, t1, tp2):.3f} ms"]

    def three():
        for _ in range(3):
            m.autoregressive_generate(b)
    tl, t3 = timed([variants["long"], three])
    lines += ["(c) generate_long(frames = 46, overlap = 1): three windows",
              f2.format("   generate_long", med(tl), tl[0], tl[-1]),
              f2.format("   three plain calls (a chain by hand adds two VQ encodes of a frame and the host's work between them)", med(t3), t3[0], t3[-1]),
              f"   generate_long - three plain calls {med(tl) - med(t3):+.3f} ms; spread {sp(tl, t3):.3f} ms"]
    if a.baseline_root:
        del m, b, free
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root, "--clips", str(n)], check=True,
                             capture_output=True, text=True, timeout=600).stdout
        tb = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])["plain"]
        lines += ["(d) the commit before the feature, its own package and library, in a child process on the same visit",
                  f2.format("   unconstrained call", med(tb), tb[0], tb[-1]),
                  f"   unconstrained here - there {med(tp) - med(tb):+.3f} ms (spread there {tb[-1] - tb[0]:.3f} ms); all-free here - unconstrained there "
                  f"{med(tf) - med(tb):+.3f} ms; prefilled here - unconstrained there {med(t8) - med(tb):+.3f} ms; generate_long here - 3 x "
                  f"unconstrained there {med(tl) - 3 * med(tb):+.3f} ms"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
