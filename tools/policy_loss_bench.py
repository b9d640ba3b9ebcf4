"""Times the policy-gradient loss kernels against their yardsticks at the cfg2 training shape (rows = 64 * 15 * 256, K = 512), with HIP
events: 20 launches after 5 warm-ups, for no filter and for top-k 50 + top-p 0.95.

    python tools/policy_loss_bench.py [--out profiles/r09_policy_loss.txt] [--rows N] [--K K]

Rows of the table: mage_policy_loss (all three launches: the row kernel and the two summary stages), mage_policy_loss_bwd (bf16 dlogits),
mage_cross_entropy + mage_cross_entropy_bwd (bf16), mage_token_stats (policy_logprob, policy_entropy, kept).  The last column is the share
of the HBM peak (8 TB/s) the bytes every launch must move account for: the fp32 logits read once forward (rows * K * 4), and read once
plus rows * K * 2 written backward."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mage_amd import ops  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=64 * 15 * 256)
    ap.add_argument("--K", type=int, default=512)
    a = ap.parse_args()
    rows, K = a.rows, a.K
    g = torch.Generator(device=DEV).manual_seed(0)
    z = 2.0 * torch.randn(rows, K, device=DEV, generator=g)
    tok = torch.randint(0, K, (rows,), device=DEV, generator=g)
    adv = torch.randn(rows // (15 * 256) if rows % (15 * 256) == 0 else rows, device=DEV, generator=g)
    gout = torch.ones(1, device=DEV)
    dl = torch.empty(rows, K, device=DEV, dtype=torch.bfloat16)
    st = dict(policy_logprob=torch.empty(rows, device=DEV), policy_entropy=torch.empty(rows, device=DEV),
              kept=torch.empty(rows, dtype=torch.int32, device=DEV))
    fwd_b, bwd_b = rows * K * 4, rows * K * 6
    lines = [f"policy loss kernels, rows = {rows}, K = {K}: median (min .. max) us of 20 launches after 5 warm-ups, HIP events",
             f"{'':44s}{'us':>9s}{'min':>9s}{'max':>9s}{'GB/s':>8s}{'of HBM peak':>13s}"]

    def row(name, fn, nbytes):
        med, lo, hi = timed(fn)
        lines.append(f"{name:44s}{med:9.1f}{lo:9.1f}{hi:9.1f}{nbytes / med / 1e3:8.0f}{nbytes / (med * 1e-6) / HBM_PEAK:13.3f}")
        return med

    for label, (T, k, p) in (("no filter", (1.0, 0, 1.0)), ("top-k 50 + top-p 0.95", (1.0, 50, 0.95))):
        lines.append(f"-- {label} (temperature {T}, top_k {k}, top_p {p})")
        ops.token_stats(z, tok, rows=rows, K=K, temperature=T, top_k=k, top_p=p, **st)
        blp = torch.where(torch.isfinite(st["policy_logprob"]), st["policy_logprob"], torch.zeros_like(st["policy_logprob"])) + 0.1
        kw = dict(temperature=T, clip_lo=0.2, clip_hi=0.2, entropy_coef=0.01)
        out = ops.policy_loss(z, tok, adv, blp, top_k=k, top_p=p, **kw)
        t_stats = row("mage_token_stats (policy outputs)", lambda: ops.token_stats(z, tok, rows=rows, K=K, temperature=T, top_k=k, top_p=p, **st), fwd_b)
        t_fwd = row("mage_policy_loss (clipped, + summary)", lambda: ops.policy_loss(z, tok, adv, blp, top_k=k, top_p=p, **kw), fwd_b)
        t_bwd = row("mage_policy_loss_bwd (bf16 dlogits)", lambda: ops.policy_loss_bwd(z, tok, adv, blp, out["cut"], gout, dl, **kw), bwd_b)
        lines.append(f"   forward / mage_token_stats = {t_fwd / t_stats:.3f}")
        if k == 0 and p == 1.0:
            t_ce = row("mage_cross_entropy", lambda: ops.cross_entropy(z, tok), fwd_b)
            t_ceb = row("mage_cross_entropy_bwd (bf16 dlogits)", lambda: ops.cross_entropy_bwd(z, tok, gout, dl), bwd_b)
            lines.append(f"   forward / mage_cross_entropy = {t_fwd / t_ce:.3f}, backward / mage_cross_entropy_bwd = {t_bwd / t_ceb:.3f}")
    ops.check_device_errors(DEV)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
