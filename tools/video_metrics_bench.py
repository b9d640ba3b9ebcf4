"""Times mage_video_metrics (the reward of MAGE.rollout) against its two yardsticks, with HIP events: 20 launches after 5 warm-ups.

    python tools/video_metrics_bench.py [--out profiles/r10_video_metrics.txt]

Two shapes: cfg2's rollout (64 clips x 8 candidates x 15 generated frames of 1 x 64 x 64, the candidates of a clip sharing one ground truth:
tgt_div 8, the target being frames 1 .. 15 of the [64, 16, 1, 64, 64] batch) and cfg4's frames (32 clips x 31 frames of 3 x 128 x 128).
Yardsticks, both from code that was there before the kernel: the HBM floor of reading both sides once (8 bytes per pixel at 8 TB/s), and
MAGE.first_stage_decode of the same frames (bf16, the benchmark's precision; and fp32) in the same process: the reward follows that decode
in a rollout, so its cost matters as a share of it."""
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
    a = ap.parse_args()
    lines = ["mage_video_metrics: median (min .. max) us of 20 launches after 5 warm-ups, HIP events",
             f"{'':52s}{'us':>10s}{'min':>10s}{'max':>10s}{'x HBM floor':>13s}{'of decode (bf16)':>18s}"]
    g = torch.Generator(device=DEV).manual_seed(0)
    for label, cfg, B, N, L in (("cfg2 rollout: 64 clips x 8 candidates x 15 frames of 1 x 64 x 64", synth.mnist_model_config(frames_length=16), 64, 8, 16),
                                ("cfg4 frames: 32 clips x 31 frames of 3 x 128 x 128", synth.cater_model_config(frames_length=32), 32, 1, 32)):
        m = instantiate_from_config(cfg).eval()
        synth.fill_state_dict(m, 0)
        m = m.to(DEV)
        R, K = m.image_resolution, m.codebook_size
        tokens = torch.randint(0, K, (B * N, L - 1, R, R), device=DEV, generator=g)
        dec = {}
        for prec in ("bf16", "fp32"):
            m.set_precision(prec)
            video = m.first_stage_decode(tokens)
            dec[prec] = timed(lambda: m.first_stage_decode(tokens))
        video = video.float().contiguous()
        _, T, C, H, W = video.shape
        images = torch.rand(B, L, C, H, W, device=DEV, generator=g) * 2 - 1
        floor = video.numel() * 8 / HBM_PEAK * 1e6
        lines.append(f"-- {label}: {B * N * T} frames, {video.numel() * 8 / 1e6:.0f} MB read once = {floor:.1f} us at 8 TB/s")
        for name, kw in (("mse + psnr + ssim (what rollout launches)", {}), ("ssim alone", dict(mse=False, psnr=False)), ("mse + psnr alone", dict(ssim=False))):
            med, lo, hi = timed(lambda: ops.video_metrics(video, images[:, 1:], tgt_div=N, **kw))
            lines.append(f"{'mage_video_metrics, ' + name:52s}{med:10.1f}{lo:10.1f}{hi:10.1f}{med / floor:13.2f}{med / dec['bf16'][0]:18.4f}")
        for prec in ("bf16", "fp32"):
            med, lo, hi = dec[prec]
            lines.append(f"{'first_stage_decode of the same frames, ' + prec:52s}{med:10.1f}{lo:10.1f}{hi:10.1f}{med / floor:13.2f}{med / dec['bf16'][0]:18.4f}")
        del m, video, images, tokens
        torch.cuda.empty_cache()
    ops.check_device_errors(DEV)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
