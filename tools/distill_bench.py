"""Times the distillation kernels (mage_distill_loss / _bwd) against their yardsticks and MAGE.distill_loss / distill_targets end to end.

    python tools/distill_bench.py [--out profiles/r17_distill.txt] [--baseline-root DIR] [--only NAME]

cfg2 (16 frames, width 512, 6 layers, K = 512), bf16, 8 clips x 8 candidates: 64 x 15 x 256 = 245 760 rows of 512 logits.  Every number is
the median (min .. max) of five repeats after two warm-ups, the variants alternating inside every repeat.
(a) The kernels on one set of buffers, HIP events around ten calls (us per call), with the bytes each must move and the rate that makes:
    mage_distill_loss (both modes; two fp32 reads: 8 bytes per logit) beside mage_policy_loss (sampling off; one read: 4 bytes), and
    mage_distill_loss_bwd (both modes, bf16 and fp32 dlogits: 8 + 2 or 4 bytes) beside mage_token_logprob_bwd (bf16: 4 + 2 bytes).
    The condition: a new kernel's rate is no lower than its yardstick's by more than the two kernels' spreads (max - min, as rates) added.
(b) End to end, whole calls between two synchronisations (ms): distill_loss + backward beside policy_loss + backward on the same tokens, and
    distill_targets without and with guidance (the second pass over the negative caption and one mage_guide_logits launch).
--baseline-root DIR (a built checkout of the commit before the feature) times policy_loss + backward on THAT tree's package and library, in
a child process started after this one's measurements, the same way.  --only NAME runs one end-to-end variant in a loop of five calls after
two warm-ups and prints nothing else: the command a profiler wraps (distill, policy, targets, guided).
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
L, K, CLIPS, CAND = 16, 512, 8, 8
TEMP, SCALE = 2.0, 3.0


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


def model_and_inputs():
    m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
    synth.fill_state_dict(m, 0)
    m = m.to(DEV).set_precision("bf16")
    n = CLIPS * CAND
    b = {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(n, L, seed=3).items()}
    R = m.image_resolution
    g = torch.Generator(DEV).manual_seed(1)
    tokens = torch.randint(0, K, (n, L - 1, R, R), device=DEV, generator=g)
    adv = torch.randn(n, device=DEV, generator=g)
    return m, b, tokens, adv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--only", default=None, choices=["distill", "policy", "targets", "guided"])
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "distill_bench.py measures on the GPU"
    m, b, tokens, adv = model_and_inputs()

    def policy():
        m.zero_grad(set_to_none=True)
        loss, _ = m.policy_loss(b, tokens, adv)
        loss.backward()
    if a.root:                                            # the child: the tree at --root, its policy_loss + backward only
        (tp,) = timed([policy])
        print("BASELINE " + json.dumps(dict(policy=tp)))
        return
    with torch.no_grad():
        teacher = m.set_guidance(SCALE).distill_targets(b, tokens)
    m.set_guidance(None)

    def distill():
        m.zero_grad(set_to_none=True)
        loss, _ = m.distill_loss(b, tokens, teacher, temperature=TEMP)
        loss.backward()

    def targets(scale):
        def f():
            m.set_guidance(scale).distill_targets(b, tokens)
            m.set_guidance(None)
        return f
    variants = {"distill": distill, "policy": policy, "targets": targets(None), "guided": targets(SCALE)}
    if a.only:
        for _ in range(7):
            variants[a.only]()
        torch.cuda.synchronize()
        return
    # the kernels alone, on one set of buffers
    rows = tokens.numel()
    g = torch.Generator(DEV).manual_seed(2)
    logits = torch.randn(rows, K, device=DEV, generator=g) * 2
    tl = (logits + torch.randn(rows, K, device=DEV, generator=g)).contiguous()
    tok = tokens.view(-1)
    dl16, dl32 = torch.empty(rows, K, device=DEV, dtype=torch.bfloat16), torch.empty(rows, K, device=DEV)
    gout, w = torch.ones(1, device=DEV), torch.randn(CLIPS * CAND, device=DEV, generator=g)
    res = [ops.distill_loss(logits, tl, temperature=TEMP, mode=md) for md in (0, 1)]
    kern = [("mage_distill_loss, forward KL", 8, lambda: ops.distill_loss(logits, tl, temperature=TEMP, mode=0)),
            ("mage_distill_loss, reverse KL", 8, lambda: ops.distill_loss(logits, tl, temperature=TEMP, mode=1)),
            ("mage_policy_loss (sampling off): the forward yardstick", 4, lambda: ops.policy_loss(logits, tok, adv)),
            ("mage_distill_loss_bwd, forward KL, bf16", 10,
             lambda: ops.distill_loss_bwd(logits, tl, res[0]["row_kl"], res[0]["norm"], gout, dl16, temperature=TEMP, mode=0)),
            ("mage_distill_loss_bwd, reverse KL, bf16", 10,
             lambda: ops.distill_loss_bwd(logits, tl, res[1]["row_kl"], res[1]["norm"], gout, dl16, temperature=TEMP, mode=1)),
            ("mage_distill_loss_bwd, forward KL, fp32", 12,
             lambda: ops.distill_loss_bwd(logits, tl, res[0]["row_kl"], res[0]["norm"], gout, dl32, temperature=TEMP, mode=0)),
            ("mage_token_logprob_bwd, bf16: the backward yardstick", 6, lambda: ops.token_logprob_bwd(logits, tok, w, gout, dl16))]
    ks = timed_events([k[2] for k in kern])
    rate = lambda i, us: rows * K * kern[i][1] / us / 1e6     # noqa: E731  (TB/s)
    f2 = "{:100s}{:>10.2f}{:>10.2f}{:>10.2f}"
    lines = [f"cfg2 (16 frames, width 512, 6 layers), bf16, {CLIPS} clips x {CAND} candidates = {rows} rows x {K}; temperature {TEMP}, teacher "
             f"guided at scale {SCALE}; median, min, max of 5 alternating repeats after 2 warm-ups",
             f"{'':100s}{'median':>10s}{'min':>10s}{'max':>10s}",
             "(a) the kernels on one set of buffers, HIP events around 10 calls, us per call; then the bytes moved and the rate at the median"]
    for i, (name, bpl, _) in enumerate(kern):
        t = ks[i]
        lines += [f2.format("   " + name, med(t), t[0], t[-1]),
                  f"      {rows * K * bpl / 1e6:.0f} MB ({bpl} bytes per logit): {rate(i, med(t)):.2f} TB/s (spread {rate(i, t[0]) - rate(i, t[-1]):.2f} TB/s)"]
    for new, yard in ((0, 2), (1, 2), (3, 6), (4, 6), (5, 6)):
        allow = (rate(new, ks[new][0]) - rate(new, ks[new][-1])) + (rate(yard, ks[yard][0]) - rate(yard, ks[yard][-1]))
        gap = rate(yard, med(ks[yard])) - rate(new, med(ks[new]))
        lines.append(f"   {kern[new][0]}: yardstick - this = {gap:+.2f} TB/s, the two spreads added {allow:.2f} TB/s: "
                     f"{'within' if gap <= allow else 'SHORT OF'} the condition")
    td, tp, tt, tg = timed([variants["distill"], variants["policy"], variants["targets"], variants["guided"]])
    sp = lambda *ts: max(t[-1] - t[0] for t in ts)        # noqa: E731
    lines += ["(b) end to end, whole calls between two synchronisations, ms",
              f2.format("   distill_loss + backward", med(td), td[0], td[-1]),
              f2.format("   policy_loss + backward (sampling off, one advantage per clip): the yardstick", med(tp), tp[0], tp[-1]),
              f"   distill - policy {med(td) - med(tp):+.3f} ms; spread (max - min, the larger of the two) {sp(td, tp):.3f} ms",
              f2.format("   distill_targets, guidance off (one no-grad pass)", med(tt), tt[0], tt[-1]),
              f2.format(f"   distill_targets, guidance {SCALE} (two passes and mage_guide_logits)", med(tg), tg[0], tg[-1]),
              f"   guided / unguided {med(tg) / med(tt):.2f}x; spread {sp(tt, tg):.3f} ms"]
    if a.baseline_root:
        del m, b, logits, tl, dl16, dl32, teacher, res
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root], check=True, capture_output=True, text=True,
                             timeout=600).stdout
        tb = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])["policy"]
        lines += ["(c) the commit before the feature, its own package and library, in a child process on the same visit",
                  f2.format("   policy_loss + backward, ms", med(tb), tb[0], tb[-1]),
                  f"   policy_loss + backward here - there {med(tp) - med(tb):+.3f} ms (spread there {tb[-1] - tb[0]:.3f} ms); distill_loss + backward "
                  f"here - policy_loss + backward there {med(td) - med(tb):+.3f} ms"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
