"""Times the grouped-ratio kernels (mage_policy_loss_grouped / _bwd) and MAGE.policy_loss(ratio=) against the masked pair and ratio='token'.

    python tools/group_ratio_bench.py [--out profiles/r19_group_ratio.txt] [--baseline-root DIR] [--only NAME]

cfg2 (16 frames, width 512, 6 layers, K = 512), bf16, 8 clips x 8 candidates: 64 x 15 x 256 = 245 760 rows of 512 logits; ratio_div = 256 (a
frame: 960 groups, one wave each) and 3840 (a clip: 64 groups, one workgroup each).  Every number is the median (min .. max) of five
repeats after two warm-ups, the variants alternating inside every repeat.
(a) The kernels on one set of buffers, HIP events around ten forward + backward pairs (us per pair): the masked entry points with an
    all-free mask, and the grouped ones on the same rows and mask at both group sizes.  The priced extra of the grouped pair: one launch
    (the group kernel) and its traffic, about 16 bytes per row (logprob, b and the mask read, logprob and entropy read again and row_loss
    written for the rewrite), at the bandwidth the masked pair reaches in the same run.
(b) policy_loss + backward end to end (wall clock between two synchronisations, ms) under ratio 'token', 'frame' and 'clip'.
--baseline-root DIR (a built checkout of the commit before the feature) times the masked kernel pair of (a) and the end-to-end call without
ratio= on THAT tree's package and library, in a child process started after this one's measurements, the same way.  --only NAME runs one
end-to-end variant in a loop of five calls after two warm-ups and prints nothing else: the command a profiler wraps (token, frame, clip).
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
TEMP, TOP_K, TOP_P = 1.0, 50, 0.95
LAUNCH_US = 5.0                                           # what one more small launch on a busy stream is priced at


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
    m = m.to(DEV).set_precision("bf16").set_sampling(TEMP, top_k=TOP_K, top_p=TOP_P)
    n = CLIPS * CAND
    b = {k_: v.to(DEV) for k_, v in synth.synth_batch_mnist(n, L, seed=3).items()}
    R = m.image_resolution
    g = torch.Generator(DEV).manual_seed(1)
    tokens = torch.randint(0, K, (n, L - 1, R, R), device=DEV, generator=g)
    adv = torch.randn(n, device=DEV, generator=g)
    with torch.no_grad():
        blp = m.token_policy_logprobs(b, tokens)
    blp = torch.where(torch.isfinite(blp), blp, torch.zeros_like(blp)).contiguous()         # (random tokens: many lie outside the filter)
    return m, b, tokens, adv, blp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--only", default=None, choices=["token", "frame", "clip"])
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "group_ratio_bench.py measures on the GPU"
    m, b, tokens, adv, blp = model_and_inputs()
    ref = (blp - 0.05).contiguous()

    def e2e(**kw):
        def f():
            m.zero_grad(set_to_none=True)
            loss, _ = m.policy_loss(b, tokens, adv, blp, reference_logprobs=ref, kl_coef=0.1, **kw)
            loss.backward()
        return f
    # the kernels alone, on one set of buffers
    rows = tokens.numel()
    n, R = CLIPS * CAND, m.image_resolution
    frame, clip = R * R, (L - 1) * R * R
    g = torch.Generator(DEV).manual_seed(2)
    logits = torch.randn(rows, K, device=DEV, generator=g) * 2
    tok, b1, r1 = tokens.view(-1), blp.view(-1), ref.view(-1)
    free = torch.zeros(rows, dtype=torch.bool, device=DEV)
    dl = torch.empty(rows, K, device=DEV, dtype=torch.bfloat16)
    gout = torch.ones(1, device=DEV)
    kw = dict(temperature=TEMP, clip_lo=0.2, clip_hi=0.2, entropy_coef=0.0, reference_logprob=r1, kl_coef=0.1, given=free)

    def pair(rd):
        def f():
            g_ = {} if rd is None else {"ratio_div": rd}
            out = ops.policy_loss(logits, tok, adv, b1, top_k=TOP_K, top_p=TOP_P, **kw, **g_)
            if rd is not None:
                g_["group_logratio"] = out["group_logratio"]
            ops.policy_loss_bwd(logits, tok, adv, b1, out["cut"], gout, dl, **kw, norm=out["norm"], **g_)
        return f
    if a.root:                                            # the child: the tree at --root, the masked kernels and the call without ratio= only
        (km,) = timed_events([pair(None)])
        (tp,) = timed([e2e()])
        print("BASELINE " + json.dumps(dict(token=tp, kernels=km)))
        return
    variants = {"token": e2e(ratio="token"), "frame": e2e(ratio="frame"), "clip": e2e(ratio="clip")}
    if a.only:
        for _ in range(7):
            variants[a.only]()
        torch.cuda.synchronize()
        return
    km, kf, kc = timed_events([pair(None), pair(frame), pair(clip)])
    sp = lambda *ts: max(t[-1] - t[0] for t in ts)        # noqa: E731
    f2 = "{:100s}{:>10.2f}{:>10.2f}{:>10.2f}"
    pair_bytes, extra_bytes = rows * K * 10, rows * 21       # two fp32 reads + one bf16 write; logprob, b, mask + logprob, entropy, reference, row_loss
    bw = pair_bytes / (med(km) * 1e-6)
    priced = LAUNCH_US + extra_bytes / bw * 1e6
    lines = [f"cfg2 (16 frames, width 512, 6 layers), bf16, {CLIPS} clips x {CAND} candidates = {rows} rows x {K}; sampler {TEMP} / {TOP_K} / "
             f"{TOP_P}, clipped surrogate with a reference (kl_coef 0.1), all-free mask; median, min, max of 5 alternating repeats after 2 warm-ups",
             f"{'':100s}{'median':>10s}{'min':>10s}{'max':>10s}",
             "(a) the kernels: forward + backward (bf16 dlogits) on one set of buffers, HIP events around 10 pairs, us per pair",
             f2.format("   mage_policy_loss_masked + _bwd", med(km), km[0], km[-1]),
             f2.format(f"   mage_policy_loss_grouped + _bwd, ratio_div = {frame} (a frame: {rows // frame} groups, one wave each)", med(kf), kf[0], kf[-1]),
             f2.format(f"   mage_policy_loss_grouped + _bwd, ratio_div = {clip} (a clip: {rows // clip} groups, one workgroup each)", med(kc), kc[0],
                       kc[-1]),
             f"   frame - masked {med(kf) - med(km):+.2f} us; clip - masked {med(kc) - med(km):+.2f} us; spread (max - min, the largest of the three) "
             f"{sp(km, kf, kc):.2f} us",
             f"   priced extra: one launch ({LAUNCH_US:.0f} us) + {extra_bytes / 1e6:.1f} MB (21 bytes per row) at the masked pair's {bw / 1e12:.2f} TB/s "
             f"({pair_bytes / 1e6:.0f} MB per pair) = {priced:.2f} us"]
    tt, tf, tc = timed([variants["token"], variants["frame"], variants["clip"]])
    lines += ["(b) policy_loss + backward end to end, whole calls between two synchronisations, ms",
              f2.format("   ratio='token'", med(tt), tt[0], tt[-1]),
              f2.format("   ratio='frame'", med(tf), tf[0], tf[-1]),
              f2.format("   ratio='clip'", med(tc), tc[0], tc[-1]),
              f"   frame - token {med(tf) - med(tt):+.3f} ms; clip - token {med(tc) - med(tt):+.3f} ms; spread {sp(tt, tf, tc):.3f} ms"]
    if a.baseline_root:
        del m, b, logits, dl
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root], check=True, capture_output=True, text=True,
                             timeout=600).stdout
        base = json.loads([ln for ln in out.splitlines() if ln.startswith("BASELINE ")][-1][len("BASELINE "):])
        tb, kb = base["token"], base["kernels"]
        lines += ["(c) the commit before the feature, its own package and library, in a child process on the same visit",
                  f2.format("   mage_policy_loss_masked + _bwd, us per pair", med(kb), kb[0], kb[-1]),
                  f"   masked kernels here - there {med(km) - med(kb):+.2f} us (spread there {kb[-1] - kb[0]:.2f} us); grouped here - masked there: "
                  f"frame {med(kf) - med(kb):+.2f} us, clip {med(kc) - med(kb):+.2f} us against the priced {priced:.2f} us",
                  f2.format("   policy_loss + backward, ms (no ratio= there)", med(tb), tb[0], tb[-1]),
                  f"   'token' here - there {med(tt) - med(tb):+.3f} ms (spread there {tb[-1] - tb[0]:.3f} ms); 'frame' here - there "
                  f"{med(tf) - med(tb):+.3f} ms; 'clip' here - there {med(tc) - med(tb):+.3f} ms"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
