"""Times per-frame credit (mage_frame_advantages, MAGE.rollout(credit='frame')) against the per-clip form it stands beside.

    python tools/frame_credit_bench.py [--out profiles/r18_frame_credit.txt] [--baseline-root DIR] [--clips 64] [--only NAME]

cfg2's rollout size: 64 clips x 8 candidates x 15 generated frames (16 frames, width 512, 6 layers), bf16, incremental.
(a) The kernels: mage_group_advantages and mage_frame_advantages on the same [512, 15] rewards through their Python wrappers (two output
    allocations each), HIP events, 50 launches after 10.  Two events around one launch time the launch, not the kernel: the kernels' own
    durations come from a profiler run over --only kernels.
(b) End to end: rollout(credit='clip') and rollout(credit='frame') under the same seeds, whole calls between two synchronisations (wall
    clock, ms), median (min .. max) of five repeats after two warm-ups, the two alternating inside every repeat.
--baseline-root DIR (a built checkout of the commit before the feature) times mage_group_advantages and rollout on THAT tree's package and
library, in a child process started after this one's measurements, the same way.  --only NAME runs one variant in a loop and prints
nothing else: the command a profiler wraps (kernels: 60 launches of each kernel; clip, frame: 7 rollouts).
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
L, N = 16, 8


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


def events(fn, warm=10, reps=50):
    """Sorted us of fn between two HIP events."""
    evs = []
    for _ in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs[warm:])


def med(t):
    return t[len(t) // 2]


def model_and_batch(n):
    m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
    synth.fill_state_dict(m, 0)
    m = m.to(DEV).set_precision("bf16").set_sampling(0.9)
    m.use_graph, m.ar_mode, m.streams = False, "incremental", 1
    b = {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(n, L, seed=3).items()}
    return m, {**b, "sample_seed": torch.arange(n, dtype=torch.int64) * N}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--only", default=None, choices=["kernels", "clip", "frame"])
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frame_credit_bench.py measures on the GPU"
    n = a.clips
    g = torch.Generator(device=DEV).manual_seed(0)
    fr = (torch.rand(n * N, 1, device=DEV, generator=g) * 0.7 + 0.2 + 0.05 * torch.randn(n * N, L - 1, device=DEV, generator=g)).contiguous()
    group = lambda: ops.group_advantages(fr, groups=n, n_cand=N)           # noqa: E731
    frame = lambda: ops.frame_advantages(fr, groups=n, n_cand=N, gamma=0.9)  # noqa: E731
    if a.only == "kernels":
        for _ in range(60):
            group()
            if not a.root:
                frame()
        torch.cuda.synchronize()
        return
    m, b = model_and_batch(n)
    clip = lambda: m.rollout(b, N)                        # noqa: E731
    if a.root:                                            # the child: the tree at --root, the yardsticks only
        tg = events(group)
        (tc,) = timed([clip])
        print("BASELINE " + json.dumps(dict(group=tg, clip=tc)))
        return
    per_frame = lambda: m.rollout(b, N, credit="frame", gamma=0.9)         # noqa: E731
    if a.only:
        for _ in range(7):
            (clip if a.only == "clip" else per_frame)()
        torch.cuda.synchronize()
        return
    f1 = "{:100s}{:>10.1f}{:>10.1f}{:>10.1f}"
    f2 = "{:100s}{:>10.2f}{:>10.2f}{:>10.2f}"
    tg, tf = events(group), events(frame)
    lines = [f"cfg2's rollout size: {n} clips x {N} candidates x {L - 1} generated frames; bf16, incremental, eager",
             "(a) one launch through the Python wrapper (two output allocations), HIP events around it, us: median, min, max of 50 after 10",
             f"{'':100s}{'us':>10s}{'min':>10s}{'max':>10s}",
             f1.format(f"   ops.group_advantages, [{n * N}, {L - 1}] rewards -> [{n}, {N}] rewards + [{n * N}] advantages", med(tg), tg[0], tg[-1]),
             f1.format(f"   ops.frame_advantages, the same rewards -> [{n * N}, {L - 1}] returns + [{n * N}, {L - 1}] advantages", med(tf), tf[0], tf[-1])]
    tc, tp = timed([clip, per_frame])
    spread = max(tc[-1] - tc[0], tp[-1] - tp[0])
    lines += ["(b) rollout, whole calls between two synchronisations, ms: median, min, max of 5 alternating repeats after 2 warm-ups",
              f"{'':100s}{'ms':>10s}{'min':>10s}{'max':>10s}",
              f2.format("   rollout(batch, 8): credit='clip'", med(tc), tc[0], tc[-1]),
              f2.format("   rollout(batch, 8, credit='frame', gamma=0.9): one launch and two allocations more", med(tp), tp[0], tp[-1]),
              f"   frame - clip {med(tp) - med(tc):+.3f} ms against a call-to-call spread (max - min, the larger of the two) of {spread:.3f} ms"]
    if a.baseline_root:
        del m, b
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root, "--clips", str(n)], check=True,
                             capture_output=True, text=True, timeout=600).stdout
        base = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])
        bg, bc = base["group"], base["clip"]
        lines += ["(c) the commit before the feature, its own package and library, in a child process on the same visit",
                  f1.format("   ops.group_advantages, us", med(bg), bg[0], bg[-1]),
                  f2.format("   rollout(batch, 8), ms", med(bc), bc[0], bc[-1]),
                  f"   clip here - there {med(tc) - med(bc):+.3f} ms; frame here - there {med(tp) - med(bc):+.3f} ms (spread there "
                  f"{bc[-1] - bc[0]:.3f} ms)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
