"""Seeded token sampling vs greedy argmax at BASELINE cfg2 (B = 64, L = 16, bf16, incremental loop: 16 384 rows x 512 codes per step).

  kernels   one warm-up call each, then 3 greedy + 3 sampled calls; run it under
            rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/sample_profile.py kernels
  micro     the four sampler instances (none / top-k / top-p / both) and argmax_kernel on random [16384, 512] logits, 50 launches each
            (under rocprofv3 as above, in a run of its own)
  summary CSV [CSV ...]   per-launch time of sample_kernel<..> and argmax_kernel from rocprofv3's kernel_stats.csv
  calls [N] profiler off: 2 warm-up calls each, then N (default 7) greedy / sampled calls alternating in one process; median ms per call
The sampled setting is temperature 1, top_k 50, top_p 0.95, per-clip seeds on the device."""
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLED = dict(temperature=1.0, top_k=50, top_p=0.95)


def _setup():
    import torch
    from mage_amd.utils import synth
    from tests.helpers import build_mage
    dev = "cuda:0"
    m = build_mage(synth.mnist_model_config(frames_length=16), 0, dev).set_precision("bf16")
    m.ar_mode, m.use_graph = "incremental", False
    batch = {k: v.to(dev) for k, v in synth.synth_batch_mnist(64, 16, seed=3).items()}
    seeds = torch.arange(64, dtype=torch.int64, device=dev) * 7919 + 1
    return m, batch, seeds


def _call(m, batch, seeds, sampled):
    import torch
    if sampled:
        m.set_sampling(**SAMPLED)
        b = {**batch, "sample_seed": seeds}
    else:
        m.set_sampling(None)
        b = batch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.autoregressive_generate(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernels():
    m, batch, seeds = _setup()
    for s in (False, True):
        _call(m, batch, seeds, s)
    for _ in range(3):
        _call(m, batch, seeds, False)
        _call(m, batch, seeds, True)
    print("kernels: done (1 + 3 greedy, 1 + 3 sampled calls)")


def micro():
    import torch
    from mage_amd import ops
    rows, K = 16384, 512
    g = torch.Generator(device="cuda:0").manual_seed(0)
    z = 2.0 * torch.randn(rows, K, device="cuda:0", generator=g)
    out = torch.empty(rows, dtype=torch.int64, device="cuda:0")
    seeds = torch.arange(64, dtype=torch.int64, device="cuda:0")
    for _ in range(50):
        ops.argmax(z, out, rows=rows, K=K)
    for k, p in ((0, 1.0), (50, 1.0), (0, 0.95), (50, 0.95)):
        for _ in range(50):
            ops.sample_tokens(z, out, seeds, rows=rows, K=K, temperature=1.0, top_k=k, top_p=p, group=256)
    torch.cuda.synchronize()
    print("micro: done (50 launches each)")


def summary(paths):
    for path in paths:
        print(f"--- {os.path.basename(path)}")
        for r in csv.DictReader(open(path)):
            name = r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            if "sample_kernel" in name or "argmax_kernel" in name:
                print(f"{name:40s} launches {int(r['Calls']):5d}  avg {float(r['AverageNs']) / 1e3:7.2f} us  "
                      f"min {float(r['MinNs']) / 1e3:7.2f} us  max {float(r['MaxNs']) / 1e3:7.2f} us")


def calls(n):
    m, batch, seeds = _setup()
    for _ in range(2):
        _call(m, batch, seeds, False)
        _call(m, batch, seeds, True)
    g, s = [], []
    for _ in range(n):
        g.append(_call(m, batch, seeds, False))
        s.append(_call(m, batch, seeds, True))
    mg, ms = statistics.median(g), statistics.median(s)
    print(f"greedy  ms/call: median {mg:.3f}  all {' '.join(f'{v:.3f}' for v in g)}")
    print(f"sampled ms/call: median {ms:.3f}  all {' '.join(f'{v:.3f}' for v in s)}  (T=1, top_k=50, top_p=0.95)")
    print(f"sampled / greedy: {ms / mg:.4f}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "calls"
    if mode == "kernels":
        kernels()
    elif mode == "micro":
        micro()
    elif mode == "summary":
        summary(sys.argv[2:])
    else:
        calls(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
