"""Cost of token log-probabilities and best-of-N at BASELINE cfg2 (L = 16, bf16, incremental loop).

  calls [N]   B = 64: 2 warm-up calls each, then N (default 7) greedy calls with set_logprobs off / on alternating in one process; median ms
  micro [N]   mage_token_logprob against mage_argmax on the same random [16384, 512] fp32 logits (both read the same 33.5 MB): N (default 200)
              launches each between device events, alternating in blocks of 20; µs per launch, the ratio, bytes / s
  cand [N]    B = 16 clips: one candidates=4 call (64 rows through the loop, 16 decodes) against four separate candidates=1 calls with
              set_logprobs on (4 x 16 rows, 64 decodes, four prologues); N (default 5) alternating repeats, median ms
  stats [N]   mage_token_stats (all four outputs, then each filter and each single output) against mage_token_logprob and mage_sample_tokens
              on the same [16384, 512] buffer, timed as in `micro`; then B = 64 sampled calls with set_logprobs(True) against
              set_logprobs(True, policy=True, entropy=True), as in `calls` (max(N // 30, 5) of each)
  sampler [N] mage_sample_tokens alone, K = 256 .. 4096 on the same 33.5 MB of logits, unfiltered / top-50 / top-p 0.95 / both: N (default 200)
              launches in blocks of 20 between device events, median µs and the sum of the drawn tokens.  Run on two checkouts it gives the
              before / after table of a change to the sampler (equal checksums: equal draws)
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
    med = _micro_time(run, n, rows, K)
    print(f"mage_token_logprob / mage_argmax: {med['mage_token_logprob'] / med['mage_argmax']:.3f}")


def _micro_time(run, n, rows, K):
    """Median µs per launch of every entry of `run`: 20 warm-up launches each, then blocks of 20 between device events, alternating."""
    import torch
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
        print(f"{k:44s} {rows} x {K}: median {med[k]:.2f} us per launch (back to back, blocks of 20: min {min(v):.2f} max {max(v):.2f}), "
              f"{nbytes / med[k] / 1e6:.2f} TB/s of logits")
    return med


def stats(n):
    import torch
    from mage_amd import ops
    rows, K = 16384, 512
    z = 2.0 * torch.randn(rows, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    tok = torch.empty(rows, dtype=torch.int64, device=DEV)
    seeds = torch.arange(rows // 256, dtype=torch.int64, device=DEV)
    out = dict(policy_logprob=torch.empty(rows, device=DEV), policy_entropy=torch.empty(rows, device=DEV),
               kept=torch.empty(rows, dtype=torch.int32, device=DEV), entropy=torch.empty(rows, device=DEV))
    ops.sample_tokens(z, tok, seeds, rows=rows, K=K, group=256, **SAMPLED)
    run = {"mage_token_logprob": lambda: ops.token_logprob(z, tok, out["entropy"], rows=rows, K=K),
           "mage_sample_tokens top-50 top-p 0.95": lambda: ops.sample_tokens(z, tok, seeds, rows=rows, K=K, group=256, **SAMPLED),
           "mage_sample_tokens unfiltered": lambda: ops.sample_tokens(z, tok, seeds, rows=rows, K=K, group=256),
           "mage_token_stats top-50 top-p 0.95, all": lambda: ops.token_stats(z, tok, rows=rows, K=K, **SAMPLED, **out)}
    for name, kw in (("top-50", dict(top_k=50)), ("top-p 0.95", dict(top_p=0.95)), ("unfiltered", {}), ("top_k = 1", dict(top_k=1))):
        run[f"mage_token_stats {name}, all"] = lambda kw=kw: ops.token_stats(z, tok, rows=rows, K=K, **kw, **out)
    for name in out:
        run[f"mage_token_stats top-50 top-p 0.95, {name}"] = lambda name=name: ops.token_stats(z, tok, rows=rows, K=K, **SAMPLED, **{name: out[name]})
    med = _micro_time(run, n, rows, K)
    a = med["mage_token_stats top-50 top-p 0.95, all"]
    print(f"mage_token_stats / mage_sample_tokens (top-50 top-p 0.95): {a / med['mage_sample_tokens top-50 top-p 0.95']:.3f}; "
          f"/ mage_token_logprob: {a / med['mage_token_logprob']:.3f}")
    m, batch, sd = _setup(64)
    m.set_sampling(**SAMPLED)
    b = {**batch, "sample_seed": sd}

    def call(flags):
        m.set_logprobs(True, policy=flags, entropy=flags)
        return _timed(lambda: m.autoregressive_generate(b))
    for _ in range(2):
        call(False)
        call(True)
    off, on = [], []
    for _ in range(max(n // 30, 5)):
        off.append(call(False))
        on.append(call(True))
    x, y = _line("sampled, set_logprobs(True)", off), _line("... policy=True, entropy=True", on)
    n_rows = batch["images"].shape[0] * m.image_resolution ** 2
    print(f"with / without: {y / x:.4f}  (+{y - x:.3f} ms: {m.frames_length - 1} mage_token_stats launches of {n_rows} x {m.codebook_size} "
          f"and one mage_clip_scores)")
    m.set_sampling(None).set_logprobs(False)


def sampler(n):
    import torch
    from mage_amd import ops
    for K in (256, 512, 1024, 2048, 4096):
        rows = 16384 * 512 // K
        z = 2.0 * torch.randn(rows, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(K))
        tok = torch.empty(rows, dtype=torch.int64, device=DEV)
        seeds = torch.arange(rows // 256, dtype=torch.int64, device=DEV)
        for name, kw in (("unfiltered", {}), ("top-50", dict(top_k=50)), ("top-p 0.95", dict(top_p=0.95)), ("top-50 top-p 0.95", dict(top_k=50, top_p=0.95))):
            def f():
                ops.sample_tokens(z, tok, seeds, rows=rows, K=K, group=256, **kw)
            for _ in range(20):
                f()
            us = []
            for _ in range(max(n // 20, 1)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    f()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / 20)
            print(f"K={K:4d} rows={rows:6d} {name:18s} median {statistics.median(us):8.2f} us (min {min(us):.2f} max {max(us):.2f}) checksum {int(tok.sum())}")


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
    elif mode == "stats":
        stats(arg or 200)
    elif mode == "sampler":
        sampler(arg or 200)
    elif mode == "cand":
        cand(arg or 5)
    else:
        calls(arg or 7)
