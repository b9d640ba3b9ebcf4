"""Times the codebook kernels (mage_code_stats, mage_codebook_ema) beside mage_embedding_bwd and one f4 stage-1 training step in 'ema' and
'grad' mode (VectorQuantizedVAE.set_codebook_update); reports the kernels' registers from the gfx950 build.

    python tools/codebook_profile.py [--out profiles/r30_codebook_ema.txt] [--baseline-root DIR] [--no-gpu]

(a) Kernels, stage-1 sizes: K = 512, D = 256, rows = 64 * 16 * 16 and 256 * 16 * 16, uniform ids.  HIP events around ten calls on fixed
    buffers, median (min .. max) of five repeats after two warm-ups, the three kernels alternating inside every repeat; us per call, the bytes
    each call must move (inputs once, outputs once, the chunks' partial tables written and read) and the rate that makes.  mage_embedding_bwd
    (deterministic form, the same rows scattered into a [K, D] table) is the yardstick of mage_code_stats: the same reads, no counts.
(b) End to end: one f4 training step (dim 256, K 512, 64 frames of 64 x 64: forward, the three-term loss, backward, FlatAdam), whole steps
    between two synchronisations, ms, median (min .. max) of five repeats after three warm-ups, 'grad' and 'ema' alternating.  'ema' replaces
    one scatter launch and the codebook's share of Adam by two small launches and one more rebuild of the derived weights.
    --baseline-root DIR (a built checkout of the parent commit) times 'grad' on THAT tree in a child process, the same way; the acceptance
    line is the parent's median plus the measured spread (max - min) of the two, not a fixed number.
(c) Registers, LDS and scratch of the four kernels, from `hipcc -S` of csrc/codebook.hip for gfx950 (no GPU needed: --no-gpu prints only this).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                  # (the child of --baseline-root: import that tree's package instead of this one's)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

DEV = "cuda:0"
K, D, DIM, FRAMES = 512, 256, 256, 64


def fmt(ts, unit):
    return f"{ts[len(ts) // 2]:9.2f} ({ts[0]:.2f} .. {ts[-1]:.2f}) {unit}"


def resources():
    """(kernel, vgprs, sgprs, LDS bytes, scratch bytes, spills) of csrc/codebook.hip built for gfx950."""
    src = os.path.join(ROOT, "mage_amd", "csrc", "codebook.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "codebook.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                        "-S", src, "-o", out], check=True)
        text = open(out).read()
    rows = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size:", text, flags=re.S):
        get = lambda key: re.search(r"\." + key + r":\s+(\S+)", blk).group(1)      # noqa: E731
        rows.append((get("name"), int(get("vgpr_count")), int(get("sgpr_count")), int(get("group_segment_fixed_size")),
                     int(get("private_segment_fixed_size")), int(get("vgpr_spill_count"))))
    return rows


def kernels(lines):
    import torch
    from mage_amd import _lib, ops
    l = _lib.lib(0)
    s = torch.cuda.current_stream().cuda_stream
    for rows in (64 * 16 * 16, 256 * 16 * 16):
        g = torch.Generator().manual_seed(rows)
        ids = torch.randint(0, K, (rows,), generator=g).to(DEV)
        z = torch.randn(rows, D, generator=g).to(DEV)
        n_chunk = ops.code_stats_chunks(rows)
        counts, sums = torch.empty(K, device=DEV, dtype=torch.int64), torch.empty(K, D, device=DEV)
        scratch = torch.empty(n_chunk * K * (D + 1), device=DEV)
        cb, cs, es = torch.randn(K, D, device=DEV), torch.ones(K, device=DEV), torch.randn(K, D, device=DEV)
        stats = torch.empty(4, device=DEV, dtype=torch.float64)
        table, scr_e = torch.zeros(K, D, device=DEV), torch.empty(min(64, (rows + 4095) // 4096) * K * D, device=DEV)

        def f_stats():
            _lib.check(l.mage_code_stats(ids.data_ptr(), z.data_ptr(), rows, D, D, K, counts.data_ptr(), sums.data_ptr(), scratch.data_ptr(),
                                         scratch.numel() * 4, s), l)

        def f_ema():
            _lib.check(l.mage_codebook_ema(cb.data_ptr(), cs.data_ptr(), es.data_ptr(), counts.data_ptr(), sums.data_ptr(), z.data_ptr(), rows, D, K, D,
                                           0.99, 1e-5, 1.0, 1.0, 0, 0, stats.data_ptr(), s), l)

        def f_emb():
            _lib.check(l.mage_embedding_bwd(ids.data_ptr(), z.data_ptr(), ops.F32, table.data_ptr(), rows, D, K, -1, rows, rows, 0, scr_e.data_ptr(),
                                            scr_e.numel(), s), l)
        fns = (f_stats, f_ema, f_emb)
        ts = [[] for _ in fns]
        for r in range(2 + 5):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(10):
                    fn()
                b.record()
                torch.cuda.synchronize()
                if r >= 2:
                    ts[i].append(a.elapsed_time(b) * 100.0)         # ms per ten calls -> us per call
        part = n_chunk * K * D * 4
        nbytes = (rows * (D * 4 + 8) + 2 * part + 2 * n_chunk * K * 4 + K * D * 4 + K * 8,      # code_stats: rows, ids, partials out and in, results
                  4 * K * D * 4 + K * (4 + 4 + 8) + 32,                                           # ema: m and sums in, m and e out, N in and out, counts
                  rows * (D * 4 + 8) + 2 * part + 2 * K * D * 4)                                  # embedding_bwd: rows, ids, partials, table in and out
        lines.append(f"rows = {rows} ({n_chunk} chunks), K = {K}, D = {D}")
        for name, t, nb in zip(("mage_code_stats", "mage_codebook_ema", "mage_embedding_bwd"), ts, nbytes):
            t.sort()
            lines.append(f"  {name:20s} {fmt(t, 'us')}   {nb / 1e6:8.2f} MB   {nb / t[len(t) // 2] / 1e3:8.1f} GB/s")


def step_times(modes):
    """Sorted ms of one f4 training step per mode, the modes alternating inside every repeat."""
    import torch
    import torch.nn.functional as F
    from mage_amd.modules.vqvae_model import VectorQuantizedVAE
    from mage_amd.optim import FlatAdam
    from mage_amd.utils import synth
    x = synth.synth_batch_mnist(FRAMES, 1, seed=1)["images"][:, 0].contiguous().to(DEV)
    runs = []
    for mode in modes:
        torch.manual_seed(0)
        m = VectorQuantizedVAE(1, 4, DIM, K)
        synth.fill_state_dict(m, 3)
        m = m.to(DEV).train()
        if mode == "ema":
            m.set_codebook_update("ema", restart_below=1.0)
        opt = FlatAdam(m.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)

        def step(m=m, opt=opt):
            opt.zero_grad()
            x_tilde, z_e, z_q = m(x)
            loss = F.mse_loss(x_tilde, x) + F.mse_loss(z_q, z_e.detach()) + 0.25 * F.mse_loss(z_e, z_q.detach())
            loss.backward()
            opt.step()
        runs.append(step)
    for _ in range(3):
        for fn in runs:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in runs]
    for _ in range(5):
        for i, fn in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [sorted(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--baseline-root")
    ap.add_argument("--root")
    ap.add_argument("--child", action="store_true", help="print the 'grad' step times of --root's tree as JSON and exit")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("CHILD " + json.dumps(step_times(["grad"])[0]))
        return
    lines = ["(c) kernels of csrc/codebook.hip, gfx950: vgprs, sgprs, static LDS bytes, scratch bytes, spills"]
    for name, v, sg, lds, scr, sp in resources():
        lines.append(f"  {name:60s} {v:4d} {sg:4d} {lds:7d} {scr:4d} {sp:3d}")
    if not a.no_gpu:
        lines.append("(a) kernels: us per call, median (min .. max); bytes per call; rate")
        kernels(lines)
        lines.append(f"(b) one f4 training step, dim {DIM}, K {K}, {FRAMES} frames of 64 x 64: ms, median (min .. max)")
        grad, ema = step_times(["grad", "ema"])
        lines.append(f"  grad {fmt(grad, 'ms')}")
        lines.append(f"  ema  {fmt(ema, 'ms')}")
        if a.baseline_root:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline_root, "--child"], capture_output=True, text=True,
                               timeout=600)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
            if p.returncode or not got:
                lines.append(f"  parent: child process failed (exit {p.returncode}): {p.stderr[-300:]}")
            else:
                par = json.loads(got[0][6:])
                spread = max(par[-1] - par[0], ema[-1] - ema[0])
                lines.append(f"  parent, grad {fmt(par, 'ms')}")
                lines.append(f"  acceptance: ema median {ema[2]:.2f} <= parent median {par[2]:.2f} + spread {spread:.2f} = {par[2] + spread:.2f}: "
                             f"{'met' if ema[2] <= par[2] + spread else 'NOT met'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
