"""Host time of the decoder's Python launch loop, one checkout against another: time for autoregressive_generate() to RETURN (all launches
enqueued) and time until the GPU has finished (the method of tools/cpu_enqueue_probe.py), at the MNIST config, L = 16, in three settings:
the one-clip incremental call in bf16 and in f16x3 (eager: use_graph = False, so that every call runs the Python loop) and the 64-clip full
loop in bf16.  Tuning only.

    python tools/decoder_enqueue_probe.py --tree DIR                           # one checkout, one process: a JSON line of per-setting medians (ms)
    python tools/decoder_enqueue_probe.py --alternate DIR_A DIR_B [--repeats 5]  # fresh child processes, A B A B ..; the table, and B against A

The bound of --alternate: B's median over the repeats may exceed A's by no more than A's max - min over its repeats."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

SETTINGS = (("inc_1clip_bf16", 1, "bf16", "incremental", 3, 7), ("inc_1clip_f16x3", 1, "f16x3", "incremental", 3, 7),
            ("full_64clip_bf16", 64, "bf16", "full", 1, 3))           # name, clips, precision, ar_mode, warm-up calls, timed calls
L = 16


def one(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config
    dev = torch.device("cuda", 0)
    model = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
    synth.fill_state_dict(model, 0)
    model = model.to(dev)
    res = {}
    for name, B, prec, mode, warm, timed in SETTINGS:
        model.set_precision(prec)
        model.ar_mode, model.use_graph = mode, False
        batch = {k: v.to(dev) for k, v in synth.synth_batch_mnist(B, L, seed=100).items()}
        for _ in range(warm):
            model.autoregressive_generate(batch)
        torch.cuda.synchronize()
        enq, done = [], []
        for _ in range(timed):
            t0 = time.perf_counter()
            model.autoregressive_generate(batch)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enq.append(1e3 * (t1 - t0))
            done.append(1e3 * (t2 - t0))
        res[name] = dict(enqueue_ms=statistics.median(enq), done_ms=statistics.median(done))
    print("PROBE " + json.dumps(res))


def alternate(a, b, repeats):
    runs = {a: [], b: []}
    for _ in range(repeats):
        for tree in (a, b):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree], capture_output=True, text=True, timeout=600)
            if r.returncode:                               # (a failed child: nothing more is started)
                print(r.stdout[-2000:], r.stderr[-2000:])
                return 2
            runs[tree].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1][6:]))
            print(tree, json.dumps(runs[tree][-1]), flush=True)
    miss = 0
    print(f"ms: median (min .. max) of {repeats} alternating fresh processes, each the median of its timed calls; margin = A's max - min")
    for name, *_ in SETTINGS:
        for what in ("enqueue_ms", "done_ms"):
            va, vb = ([r[name][what] for r in runs[t]] for t in (a, b))
            ma, mb, margin = statistics.median(va), statistics.median(vb), max(va) - min(va)
            ok = mb <= ma + margin
            miss += not ok
            print(f"{name:18s} {what:10s} A {ma:9.3f} ({min(va):9.3f} .. {max(va):9.3f})   B {mb:9.3f} ({min(vb):9.3f} .. {max(vb):9.3f})   "
                  f"margin {margin:7.3f}  {'within' if ok else 'MISS'}")
    print(f"A = {a}, B = {b}; rows outside the margin: {miss}")
    return 1 if miss else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree")
    ap.add_argument("--alternate", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.alternate:
        sys.exit(alternate(*args.alternate, args.repeats))
    one(args.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
