"""Times the preference loss against the policy-gradient loss it sits beside, with HIP events.

    python tools/preference_bench.py [--out profiles/r13_preference.txt] [--baseline-root DIR] [--clips 8] [--candidates 8]

(a) The two new kernels.  mage_token_logprob_bwd (bf16 dlogits) at the cfg2 training shape, rows = clips * candidates * 15 * 256, K = 512,
    with every weight non-zero -- then it moves mage_cross_entropy_bwd's bytes (the fp32 logits read once, bf16 dlogits written once) --
    beside mage_cross_entropy_bwd on the same buffers, the two alternating; and with best_worst weights (two non-zero clips per group: the
    other rows are a zero fill).  mage_preference_loss (both launches) at the rollout's size and at its limits (65536 clips, 65536 random
    pairs).  50 repeats after 10 warm-ups.
(b) One fine-tuning step at cfg2 (16 frames, width 512, 6 layers), bf16, eval(), on the clips * candidates rows of a rollout with
    best_worst pairs: preference_loss + backward against policy_loss + backward (the reward-weighted form) on the same rows, five
    repeats each, alternating, after two warm-ups.  Both run the same encoder and decoder passes; they differ in the loss kernels only.
--baseline-root DIR (a built checkout of the commit before the feature) also times policy_loss + backward and mage_cross_entropy_bwd on THAT
tree's package and library, in a child process started after this one's measurements, with the same repeats.
"""
import argparse
import json
import os
import subprocess
import sys

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


def timed(fns, warm, reps):
    """Sorted us of each fn, the fns alternating inside every repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    evs = []
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((i, a, b))
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for i, a, b in evs:
        ts[i].append(a.elapsed_time(b) * 1e3)
    return [sorted(t) for t in ts]


def med(t):
    return t[len(t) // 2]


def step_inputs(n):
    m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
    synth.fill_state_dict(m, 0)
    m = m.to(DEV).set_precision("bf16")
    b = {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(n, L, seed=3).items()}
    g = torch.Generator(device=DEV).manual_seed(5)
    R = m.image_resolution
    tokens = torch.randint(0, K, (n, L - 1, R, R), device=DEV, generator=g)
    return m, b, tokens, torch.randn(n, device=DEV, generator=g)


def policy_step(m, b, tokens, adv):
    def f():
        loss, _ = m.policy_loss(b, tokens, adv)
        loss.backward()
        m.zero_grad(set_to_none=True)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "preference_bench.py measures on the GPU"
    n, N = a.clips * a.candidates, a.candidates
    rows = n * (L - 1) * 256
    g = torch.Generator(device=DEV).manual_seed(1)
    z = 2.0 * torch.randn(rows, K, device=DEV, generator=g)
    tok = torch.randint(0, K, (rows,), device=DEV, generator=g)
    gout = torch.ones(1, device=DEV)
    dl = torch.empty(rows, K, device=DEV, dtype=torch.bfloat16)
    if a.root:                                            # the child: the tree at --root, the yardsticks only
        (tc,) = timed([lambda: ops.cross_entropy_bwd(z, tok, gout, dl)], 10, 50)
        del z, dl
        torch.cuda.empty_cache()
        (tp,) = timed([policy_step(*step_inputs(n))], 2, 5)
        print("BASELINE " + json.dumps(dict(ce_bwd=tc, policy=tp)))
        return
    fmt = "{:96s}{:>10.1f}{:>10.1f}{:>10.1f}{:>10s}"
    lines = ["(a) median (min .. max) us of 50 repeats after 10 warm-ups, HIP events; GB/s = bytes the kernel must move / median",
             f"{'':96s}{'us':>10s}{'min':>10s}{'max':>10s}{'GB/s':>10s}",
             f"rows = {n} * 15 * 256 = {rows}, K = {K}, bf16 dlogits: {rows * K * 6 / 1e6:.0f} MB at full weights"]
    w_full = torch.randn(n, device=DEV, generator=g) + 3.0
    w_bw = torch.zeros(n, device=DEV)
    w_bw[0::N], w_bw[1::N] = -0.05, 0.05
    live = int((w_bw != 0).sum())
    tl, tc, tz = timed([lambda: ops.token_logprob_bwd(z, tok, w_full, gout, dl), lambda: ops.cross_entropy_bwd(z, tok, gout, dl),
                        lambda: ops.token_logprob_bwd(z, tok, w_bw, gout, dl)], 10, 50)
    nb, nz = rows * K * 6, (rows // n) * K * (live * 6 + (n - live) * 2)
    lines += [fmt.format("   mage_token_logprob_bwd, every weight non-zero", med(tl), tl[0], tl[-1], f"{nb / med(tl) / 1e3:.0f}"),
              fmt.format("   mage_cross_entropy_bwd on the same buffers (alternating with it)", med(tc), tc[0], tc[-1], f"{nb / med(tc) / 1e3:.0f}"),
              f"   mage_token_logprob_bwd / mage_cross_entropy_bwd = {med(tl) / med(tc):.3f}; run-to-run spread (max - min) {tl[-1] - tl[0]:.1f} / "
              f"{tc[-1] - tc[0]:.1f} us",
              fmt.format(f"   mage_token_logprob_bwd, best_worst weights ({live} of {n} clips non-zero: the rest is a zero fill)", med(tz), tz[0],
                         tz[-1], f"{nz / med(tz) / 1e3:.0f}")]
    del z, dl
    torch.cuda.empty_cache()
    for clips, P in ((n, a.clips), (65536, 65536)):
        s = -3000 + 30 * torch.randn(clips, device=DEV, generator=g)
        r = s + torch.randn(clips, device=DEV, generator=g)
        pairs = torch.randint(0, clips, (P, 2), device=DEV, generator=g)
        (tp,) = timed([lambda: ops.preference_loss(s, r, pairs, beta=0.1)], 10, 50)
        lines.append(fmt.format(f"   mage_preference_loss, clips = {clips}, pairs = {P} (both launches + four output allocations)", med(tp), tp[0],
                                tp[-1], ""))
    ops.check_device_errors(DEV)

    # (b) the step
    m, b, tokens, adv = step_inputs(n)
    rw = adv.view(a.clips, N)
    base = torch.arange(a.clips, device=DEV) * N
    pairs = torch.stack([base + rw.argmax(1), base + rw.argmin(1)], 1).contiguous()
    with torch.no_grad():
        ref_lp = (m.clip_logprobs(b, tokens) + torch.randn(n, device=DEV, generator=g)).contiguous()

    def pref_step():
        loss, _ = m.preference_loss(b, tokens, pairs, ref_lp, beta=0.1)
        loss.backward()
        m.zero_grad(set_to_none=True)
    tq, tp = timed([pref_step, policy_step(m, b, tokens, adv)], 2, 5)
    f2 = "{:96s}{:>10.1f}{:>10.1f}{:>10.1f}"
    sp = max(tq[-1] - tq[0], tp[-1] - tp[0])
    lines += [f"(b) cfg2 (16 frames, width 512, 6 layers), bf16, eval(), {a.clips} clips x {N} candidates = {n} rows, {a.clips} best_worst pairs; "
              "us, median (min .. max) of 5 alternating repeats after 2 warm-ups",
              f2.format("   preference_loss + backward", med(tq), tq[0], tq[-1]),
              f2.format("   policy_loss + backward (reward-weighted form) on the same rows", med(tp), tp[0], tp[-1]),
              f"   preference / policy = {med(tq) / med(tp):.3f}; difference {med(tq) - med(tp):+.1f} us against a call-to-call spread (max - min over "
              f"five repeats, the larger of the two) of {sp:.1f} us"]
    if a.baseline_root:
        del m, b
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root, "--clips", str(a.clips), "--candidates",
                              str(N)], check=True, capture_output=True, text=True, timeout=600).stdout
        tb = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])
        lines += ["(c) the commit before the feature, its own package and library, in a child process",
                  fmt.format("   mage_cross_entropy_bwd (50 repeats after 10; the yardstick of (a))", med(tb["ce_bwd"]), tb["ce_bwd"][0],
                             tb["ce_bwd"][-1], f"{nb / med(tb['ce_bwd']) / 1e3:.0f}"),
                  f"   mage_token_logprob_bwd here / mage_cross_entropy_bwd there = {med(tl) / med(tb['ce_bwd']):.3f}",
                  f2.format("   policy_loss + backward (5 repeats after 2)", med(tb["policy"]), tb["policy"][0], tb["policy"][-1]),
                  f"   policy step here / there = {med(tp) / med(tb['policy']):.3f}; preference step here / policy step there = "
                  f"{med(tq) / med(tb['policy']):.3f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
