#!/usr/bin/env python
"""One launch of the decoder's temporal attention at cfg2's shapes (B 64, 16 x 16 positions, 16 heads, 16 frames): µs per launch.

    python tools/fewq_probe.py [--kind bf16|f16|f16x3] [--nq N] [--tree DIR] [--reps R]

--nq 1 or 2 (default 1): the incremental step -- attention_mfma_fewq_kernel, N new positions against a K,V cache of nk = 1 .. 16.
--nq 16: the full pass -- attention_mfma_kernel, nq = nk = 16.  --kind picks the operand policy; --tree another checkout with its library
(one tree per process).  The timed window is R (default 200) launches between two device events, after 10 warm-up launches of the shape."""
import argparse
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--kind", default="bf16", choices=("bf16", "f16", "f16x3"))
ap.add_argument("--nq", type=int, default=1, choices=(1, 2, 16))
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from mage_amd import ops  # noqa: E402

B, L, hw, Cc, H = 64, 16, 256, 512, 16
dev = "cuda:0"
torch.manual_seed(0)
full = args.nq > 2                                        # q rows: every position of the clip, or the step's new ones
q = torch.randn(B * (L if full else args.nq) * hw, Cc, device=dev)
kv = torch.randn(B * L * hw, 2 * Cc, device=dev)
if args.kind == "f16x3":                                  # split rows: two f16 pieces per value, 2 physical columns per logical one
    q, kv, P = ops.split(q, ops.F16X3), ops.split(kv, ops.F16X3), 2
    extra = dict(out_split=ops.F16X3, split_kind=ops.F16X3)
else:
    dt = torch.bfloat16 if args.kind == "bf16" else torch.float16
    q, kv, P, extra = q.to(dt), kv.to(dt), 1, {}
ao = torch.empty_like(q)


def run(nk):
    ops.attention(q, kv, kv[:, P * Cc:], ao, ldq=P * Cc, ldk=2 * P * Cc, ldv=2 * P * Cc, ldo=P * Cc, n_seq=B * hw, inner=hw, nq=args.nq, nk=nk,
                  n_head=H, q_outer_stride=q.shape[0] // B, q_axis_stride=hw, kv_outer_stride=L * hw, kv_axis_stride=hw, causal=True, **extra)


for nk in ((16,) if full else (1, 2, 4, 8, 12, 16)):
    for _ in range(10):
        run(nk)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        run(nk)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / args.reps * 1e3
    mb = (B * hw * args.nq * Cc * 2 * 2 + nk * B * hw * 2 * Cc * 2) * P / 1e6          # q and out rows, nk K and V rows
    print(f"{args.kind} nq={args.nq:2d} nk={nk:2d}: {us:7.1f} us   {mb:6.1f} MB -> {mb / us:.2f} TB/s")
