"""Times what classifier-free guidance adds to token generation, with HIP events.

    python tools/guidance_bench.py [--out profiles/r12_guidance.txt] [--baseline-root DIR]

(a) mage_guide_logits in place on cond at two shapes, K = 512: rows = 64 * 256 (one incremental step of 64 clips) and rows = 64 * 15 * 256
    (the full loop's last iteration), 12 bytes per element (two loads, one store), beside one mage_token_logprob launch on the same rows
    (4 bytes per element: a known memory-bound neighbour).  The small shape's two buffers (67 MB) fit the 256 MiB Infinity Cache, and in a
    generation the head GEMM has just written them: it is timed both ways -- on the same buffers every repeat ("cache-warm") and rotating
    through eight buffer pairs (537 MB, "rotating").  The large shape (1 GB per pair) is past the cache by itself.  50 repeats after 10.
(b) The guided call at cfg2, bf16, incremental, B = 32 (64 decoder clips) against the unguided call at B = 64 (the same 64 decoder clips;
    with guidance off the call is launch for launch the one before the feature existed), five repeats each, alternating, after two
    warm-ups.  Expectation: guided(32) <= unguided(64) + [its own guide_logits launches and token copies] + [the second half of the
    prologue: 64 captions instead of 32] + [the call-to-call spread of unguided(64)].  The two bracketed times are measured by themselves:
    the 15 guide launches and 14 token copies of a B = 32 call back to back, and the prologue (text encoder, motion-anchor encoder, speed
    term) over 64 rows minus the same over 32.  --baseline-root DIR (a built checkout of another commit, e.g. the one before the feature)
    also times the unguided B = 64 call on THAT tree's package and library, in a child process started after this one's measurements,
    the same five repeats after two warm-ups.
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


def timed(fns, warm, reps):
    """Sorted us of each fn, the fns alternating inside every repeat; fn(r) gets the repeat number."""
    for r in range(warm):
        for fn in fns:
            fn(r)
    evs = []
    for r in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(r)
            b.record()
            evs.append((i, a, b))
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for i, a, b in evs:
        ts[i].append(a.elapsed_time(b) * 1e3)
    return [sorted(t) for t in ts]


def med(t):
    return t[len(t) // 2]


def cfg2_model(L):
    m = instantiate_from_config(synth.mnist_model_config(frames_length=L)).eval()
    synth.fill_state_dict(m, 0)
    m = m.to(DEV).set_precision("bf16")
    m.ar_mode, m.use_graph, m.streams = "incremental", False, 1
    return m, {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(64, L, seed=3).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "guidance_bench.py measures on the GPU"
    if a.root:                                            # the child: the unguided B = 64 call of the tree at --root, nothing else
        m, b64 = cfg2_model(16)
        (tu,) = timed([lambda r: m.autoregressive_generate(b64)], 2, 5)
        print("BASELINE " + json.dumps(tu))
        return
    K = 512
    fmt = "{:92s}{:>10.1f}{:>10.1f}{:>10.1f}{:>10s}"
    lines = ["(a) median (min .. max) us of 50 repeats after 10 warm-ups, HIP events; GB/s = bytes the kernel must move / median",
             f"{'':92s}{'us':>10s}{'min':>10s}{'max':>10s}{'GB/s':>10s}"]
    g = torch.Generator(device=DEV).manual_seed(1)
    for label, rows, sets in (("rows = 64*256 (one incremental step of 64 clips)", 64 * 256, 8),
                              ("rows = 64*15*256 (the full loop's last iteration)", 64 * 15 * 256, 1)):
        cs = [torch.randn(rows, K, device=DEV, generator=g) for _ in range(sets)]
        us = [torch.randn(rows, K, device=DEV, generator=g) for _ in range(sets)]
        scale = torch.full((64,), 1.25, device=DEV)
        tok = torch.randint(0, K, (rows,), device=DEV, generator=g)
        lp = torch.empty(rows, device=DEV)
        n = rows * K
        lines.append(f"{label}, K = {K}: {n * 12 / 1e6:.0f} MB guided, {n * 4 / 1e6:.0f} MB scored")
        variants = [("rotating through 8 buffer pairs" if sets > 1 else "one buffer pair (1 GB: past the Infinity Cache)", lambda r: r % sets)]
        if sets > 1:
            variants.append(("cache-warm: the same pair every repeat", lambda r: 0))
        for what, pick in variants:
            tg, tl = timed([lambda r: ops.guide_logits(cs[pick(r)], us[pick(r)], scale, rows=rows, K=K, scale_div=rows // 64),
                            lambda r: ops.token_logprob(cs[pick(r)], tok, lp, rows=rows, K=K)], 10, 50)
            lines += [fmt.format(f"   mage_guide_logits, in place on cond, {what}", med(tg), tg[0], tg[-1], f"{n * 12 / med(tg) / 1e3:.0f}"),
                      fmt.format(f"   mage_token_logprob on the same rows, {what}", med(tl), tl[0], tl[-1], f"{n * 4 / med(tl) / 1e3:.0f}")]
        del cs, us
    torch.cuda.empty_cache()

    # (b) the guided call
    L = 16
    m, b64 = cfg2_model(L)
    b32 = {k_: v[:32] for k_, v in b64.items()}

    def unguided(r):
        m.set_guidance(None)
        m.autoregressive_generate(b64)

    def guided(r):
        m.set_guidance(3.0)
        m.autoregressive_generate(b32)
    tu, tg = timed([unguided, guided], 2, 5)
    m.set_guidance(None)
    hw, Lm1 = m.image_resolution ** 2, L - 1
    logits = torch.randn(64 * hw, K, device=DEV, generator=g)
    scale = torch.full((32,), 3.0, device=DEV)
    toks = torch.zeros(64, hw, dtype=torch.int64, device=DEV)

    def own(r):
        for i in range(Lm1):
            ops.guide_logits(logits, logits[32 * hw:], scale, rows=32 * hw, K=K, scale_div=hw)
            if i != Lm1 - 1:
                toks[32:].copy_(toks[:32])

    def prologue(bt):
        tok0 = m.first_stage_encode(bt["images"][:, 0:1])[:, 0].reshape(bt["images"].shape[0], hw)
        return m._motion_anchor(tok0, bt, None)
    with torch.no_grad():
        to, p64, p32 = timed([own, lambda r: prologue(b64), lambda r: prologue(b32)], 3, 10)
    spread = tu[-1] - tu[0]
    half = med(p64) - med(p32)
    allowed = med(tu) + med(to) + half + spread
    f2 = "{:92s}{:>10.1f}{:>10.1f}{:>10.1f}"
    lines += ["(b) cfg2 (16 frames, width 512, 6 layers), bf16, incremental, eager; us, median (min .. max) of 5 alternating repeats after 2 warm-ups",
              f2.format("   unguided call, B = 64 (guidance off: the launches of the call before the feature)", med(tu), tu[0], tu[-1]),
              f2.format("   guided call, B = 32, scale 3, null caption (64 decoder clips)", med(tg), tg[0], tg[-1]),
              f2.format("   its 15 mage_guide_logits launches + 14 token copies, back to back (10 repeats)", med(to), to[0], to[-1]),
              f2.format("   prologue over 64 rows (frame-0 encode, text + motion-anchor encoders, speed; 10 repeats)", med(p64), p64[0], p64[-1]),
              f2.format("   prologue over 32 rows", med(p32), p32[0], p32[-1]),
              f"   the four numbers: unguided(64) {med(tu):.1f} + guide launches and copies {med(to):.1f} + second half of the prologue {half:.1f} "
              f"+ spread of unguided(64) over five repeats {spread:.1f} = {allowed:.1f} us",
              f"   guided(32) {med(tg):.1f} us = {med(tg) / med(tu):.3f} x unguided(64); guided(32) - allowance {med(tg) - allowed:+.1f} us "
              f"({'within' if med(tg) <= allowed else 'ABOVE'} the expectation)"]
    if a.baseline_root:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root], check=True, capture_output=True, text=True,
                             timeout=300).stdout
        tb = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])
        lines += [f2.format("   unguided call, B = 64, on the baseline tree (the commit before the feature; child process)", med(tb), tb[0], tb[-1]),
                  f"   unguided(64) here / on the baseline tree {med(tu) / med(tb):.3f}; guided(32) against the baseline's unguided(64) + the other "
                  f"three numbers: {med(tg) - (med(tb) + med(to) + half + spread):+.1f} us"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
