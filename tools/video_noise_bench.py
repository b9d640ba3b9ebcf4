"""Times the pieces policy-gradient fine-tuning on randomness=True models adds, with HIP events: 50 repeats after 10 warm-ups, the two sides of
every comparison alternating in one process.

    python tools/video_noise_bench.py [--out profiles/r11_video_noise.txt]

1. mage_video_noise at cfg4's rollout shape (32 clips x 8 candidates, 64 x 16 x 16, both layouts in one launch) against what it replaces:
   torch.randn of the NCHW tensor plus the permute(0, 2, 3, 1).contiguous() copy into channel-last rows.  The floor is writing both layouts
   once (8 bytes per value at 8 TB/s); the kernel's own work is two hashes, a logarithm, a square root and a cospi per value.
2. The prologue tail (conv_d2, the four ADAIN convolutions, ADAIN, the speed term) on the 256 candidate rows of rollout(noise='candidate')
   against the 32 per-clip rows of noise='clip', on the cfg4 model (width 512), fp32 as the prologue always is.
3. One MAGE.policy_loss forward + backward on the cfg4-family model at a fine-tuning batch (8 clips of 8 frames, bf16) with the randomness
   branch against the same configuration with randomness=False.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mage_amd import ops  # noqa: E402
from mage_amd.utils import synth  # noqa: E402
from mage_amd.utils.util import instantiate_from_config  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12


def timed_pair(fns, warm=10, reps=50):
    """Median (min, max) us of each fn, the fns alternating inside every repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    evs = []
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((i, a, b))
    torch.cuda.synchronize()
    for i, a, b in evs:
        ts[i].append(a.elapsed_time(b) * 1e3)
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def build(cfg):
    m = instantiate_from_config(cfg).eval()
    synth.fill_state_dict(m, 0)
    return m.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fmt = "{:72s}{:>10.1f}{:>10.1f}{:>10.1f}"
    lines = ["median (min .. max) us of 50 repeats after 10 warm-ups, HIP events, the sides of a comparison alternating",
             f"{'':72s}{'us':>10s}{'min':>10s}{'max':>10s}"]

    # 1. the kernel
    Bn, C, R = 32 * 8, 64, 16
    seeds = torch.arange(Bn, device=DEV, dtype=torch.int64) * 7919 - 1000
    (k, r, k1) = timed_pair([lambda: ops.video_noise(seeds, C=C, h=R, w=R),
                             lambda: torch.randn(Bn, C, R, R, device=DEV).permute(0, 2, 3, 1).reshape(Bn * R * R, C).contiguous(),
                             lambda: ops.video_noise(seeds, C=C, h=R, w=R, nchw=False)])
    n = Bn * C * R * R
    floor = n * 8 / HBM_PEAK * 1e6
    lines += [f"1. noise of {Bn} clips x {C} x {R} x {R} ({n} values; writing both layouts once at 8 TB/s: {floor:.1f} us)",
              fmt.format("   mage_video_noise, NCHW + channel-last rows in one launch", *k),
              fmt.format("   mage_video_noise, rows only", *k1),
              fmt.format("   torch.randn + permute(0, 2, 3, 1).contiguous()", *r),
              f"   kernel / replaced {k[0] / r[0]:.2f}, kernel / write floor {k[0] / floor:.1f}"]

    # 2. the prologue tail
    m = build(synth.cater_model_config(frames_length=32))
    Cc, hw = m.vision_width, m.image_resolution ** 2
    g = torch.Generator(device=DEV).manual_seed(1)
    res = []
    with torch.no_grad():
        sides = []
        for rows in (32, 256):
            ma = torch.randn(rows * hw, Cc, device=DEV, generator=g)
            sd = torch.arange(rows, device=DEV, dtype=torch.int64) + 5
            sp = torch.rand(rows, device=DEV, generator=g)
            sides.append(lambda ma=ma, sd=sd, sp=sp, rows=rows: m._anchor_tail(ma.clone(), {}, None, rows, noise_seed=sd, speed=sp))
        res = timed_pair(sides)
    lines += ["2. prologue tail on the cfg4 model (noise kernel, conv_d2, four ADAIN convolutions, ADAIN, speed term; fp32; incl. one clone of ma)",
              fmt.format("   32 rows  (noise='clip': one draw per clip)", *res[0]),
              fmt.format("   256 rows (noise='candidate': 32 clips x 8 candidates)", *res[1]),
              f"   256 rows / 32 rows {res[1][0] / res[0][0]:.2f} (8x the rows)"]
    del m

    # 3. policy_loss forward + backward
    Bp, Lp = 8, 8
    batch = {k_: v.to(DEV) for k_, v in synth.synth_batch_cater(Bp, Lp, seed=3).items()}
    models = {rnd: build(synth.cater_model_config(frames_length=Lp, randomness=rnd)).set_precision("bf16") for rnd in (True, False)}
    R_, K_ = models[True].image_resolution, models[True].codebook_size
    tokens = torch.randint(0, K_, (Bp, Lp - 1, R_, R_), device=DEV, generator=g)
    adv = torch.randn(Bp, device=DEV, generator=g)
    blp = -torch.rand(Bp, Lp - 1, R_, R_, device=DEV, generator=g) * 6
    noise = ops.video_noise(torch.arange(Bp, device=DEV, dtype=torch.int64), C=64, h=R_, w=R_, rows=False)[0]

    def step(rnd):
        mm = models[rnd]
        mm.zero_grad(set_to_none=True)
        loss, _ = mm.policy_loss({**batch, "video_noise": noise} if rnd else batch, tokens, adv, blp)
        loss.backward()
    for mm in models.values():
        mm.set_sampling(1.0)
    res = timed_pair([lambda: step(True), lambda: step(False)], warm=5, reps=20)
    lines += [f"3. MAGE.policy_loss forward + backward, cfg4-family model (width 512, 6 layers), {Bp} clips x {Lp} frames, bf16, 20 repeats after 5",
              fmt.format("   randomness=True  (recorded noise -> conv_d2 -> ADAIN, and their backward)", *res[0]),
              fmt.format("   randomness=False", *res[1]),
              f"   with / without the branch {res[0][0] / res[1][0]:.3f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
