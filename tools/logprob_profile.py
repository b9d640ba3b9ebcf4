"""Cost of token log-probabilities and best-of-N at BASELINE cfg2 (L = 16, bf16, incremental loop).

  calls [N]   B = 64: 2 warm-up calls each, then N (default 7) greedy calls with set_logprobs off / on alternating in one process; median ms
  micro [N]   mage_token_logprob against mage_argmax on the same random [16384, 512] fp32 logits (both read the same 33.5 MB): N (default 200)
              launches each between device events, alternating in blocks of 20; µs per launch, the ratio, bytes / s
  cand [N]    B = 16 clips: one candidates=4 call (64 rows through the loop, 16 decodes) against four separate candidates=1 calls with
              set_logprobs on (4 x 16 rows, 64 decodes, four prologues); N (default 5) alternating repeats, median ms
Run on the GPU with the profiler off; every figure is printed, nothing is asserted."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
SAMPLED = dict(temperature=1.0, top_k=50, top_p=0.95)


def _setup(B):
    import torch
    from mage_amd.utils import synth
    from tests.helpers import build_mage
    m = build_mage(synth.mnist_model_config(frames_length=16), 0, DEV).set_precision("bf16")
    m.ar_mode, m.use_graph = "incremental", False
    batch = {k: v.to(DEV) for k, v in synth.synth_batch_mnist(B, 16, seed=3).items()}
    seeds = torch.arange(B, dtype=torch.int64, device=DEV) * 7919 + 1
    return m, batch, seeds


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _line(name, v):
    print(f"{name:28s} ms/call: median {statistics.median(v):.3f}  all {' '.join(f'{x:.3f}' for x in v)}")
    return statistics.median(v)


def calls(n):
    m, batch, _ = _setup(64)

    def call(on):
        m.set_logprobs(on)
        return _timed(lambda: m.autoregressive_generate(batch))
    for _ in range(2):
        call(False)
        call(True)
    off, on = [], []
    for _ in range(n):
        off.append(call(False))
        on.append(call(True))
    a, b = _line("set_logprobs off", off), _line("set_logprobs on", on)
    print(f"on / off: {b / a:.4f}  (+{b - a:.3f} ms: 15 mage_token_logprob launches of 16384 x 512 and one mage_clip_scores)")


def micro(n):
    import torch
    from mage_amd import ops
    rows, K = 16384, 512
    z = 2.0 * torch.randn(rows, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    tok = torch.empty(rows, dtype=torch.int64, device=DEV)
    lp = torch.empty(rows, device=DEV)
    run = {"mage_argmax": lambda: ops.argmax(z, tok, rows=rows, K=K),
           "mage_token_logprob": lambda: ops.token_logprob(z, tok, lp, rows=rows, K=K)}
    for f in run.values():
        for _ in range(20):
            f()
    us = {k: [] for k in run}
    for _ in range(max(n // 20, 1)):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / 20)
    nbytes = rows * K * 4
    med = {}
    for k, v in us.items():
        med[k] = statistics.median(v)
        print(f"{k:20s} {rows} x {K}: median {med[k]:.2f} us per launch (back to back, blocks of 20: min {min(v):.2f} max {max(v):.2f}), "
              f"{nbytes / med[k] / 1e6:.2f} TB/s of logits")
    print(f"mage_token_logprob / mage_argmax: {med['mage_token_logprob'] / med['mage_argmax']:.3f}")


def cand(n):
    import torch
    B, N = 16, 4
    m, batch, seeds = _setup(B)

    def best_of():
        m.set_logprobs(False).set_sampling(candidates=N, **SAMPLED)
        m.autoregressive_generate({**batch, "sample_seed": seeds})

    def separate():
        m.set_sampling(candidates=1, **SAMPLED).set_logprobs(True)
        for c in range(N):
            m.autoregressive_generate({**batch, "sample_seed": seeds + c})
    for _ in range(2):
        _timed(best_of)
        _timed(separate)
    a, b = [], []
    for _ in range(n):
        a.append(_timed(best_of))
        b.append(_timed(separate))
    x, y = _line(f"candidates={N}, B={B}", a), _line(f"{N} calls of B={B}, logprobs on", b)
    print(f"candidates={N} / {N} separate calls: {x / y:.4f}")
    m.set_sampling(None)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "calls"
    arg = int(sys.argv[2]) if len(sys.argv) > 2 else None
    if mode == "micro":
        micro(arg or 200)
    elif mode == "cand":
        cand(arg or 5)
    else:
        calls(arg or 7)
