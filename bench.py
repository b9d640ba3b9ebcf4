#!/usr/bin/env python
"""Headline benchmark: generated frames/sec of MAGE.autoregressive_generate on synthetic Moving-MNIST-shaped
clips (BASELINE.json: 64x64, 16-frame clips; cfg2 = MNIST f4 VQ-VAE + MAGE, batch 64 per GPU, bf16 MFMA).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg2|cfg3] [--scaling weak|strong]
                    [--batch 64] [--global-batch 256] [--frames 16] [--precision bf16|fp32] [--ar-mode full|incremental]
                    [--dump-outputs DIR] [--full]

A plain run measures the headline only: it sets up, runs the W warm-up calls and the K timed calls, writes --dump-outputs and
prints the line (frames/s, ms_per_step, and the roofline and per-kernel figures read from the HIP events of the last warm-up call
and of the timed calls).  --full adds the secondary measurements, each of which takes runs of its own (minutes in all; the --no-*
options skip single ones): the other AR mode, the f16x3 / fp32 parity modes and the f16 mode, the VQ-VAE decode roofline, the
training step, the cfg4 object, the B = 1 latency table, the CPU baseline and the GPU-vs-oracle token agreement.

One "step" = one autoregressive_generate(batch) call: VQ-VAE encode of the first frames + text encoder +
motion-anchor encoder + the reference's L-1 full decoder recomputes + VQ-VAE decode of the L-1 generated
frames (nothing skipped, inputs resident in HBM).

N > 1: one process per GPU.  Under torchrun (RANK / WORLD_SIZE in the environment) this process is one rank; started
plainly with --gpus N it launches the N ranks itself (mage_amd.utils.dist.launch_ranks -> python -m
torch.distributed.run, the counterpart of the reference's mp.spawn, main_mage.py:279-295).  Clips are sharded across
ranks, no data-path collective (clips are independent); RCCL carries the barrier, the max-over-ranks timing and the
`ranks_seen` all-reduce.  --scaling weak (default, the driver's contract): --batch clips per GPU; --scaling strong:
--global-batch clips split evenly (cfg3 = Double Moving MNIST, 256 clips, ragged 16/18/20-token captions).
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3        # fp32-input MFMA = fp32 vector peak
PEAK_HBM_GBS = 8000.0          # HBM3E (MI355X_MICROARCH.md)
DEC_FLOP_PER_FRAME = 1.216e9   # f4 VQ-VAE decode (forward hooks on the reference modules)
DEC_BYTES_PER_FRAME = {"bf16": 2.2365e6, "fp32": 4.473e6}   # layer-materialised traffic model of SURVEY.md 8d


def call_flops(B, L, d=512, K=512, hw=256):
    """FLOPs of one autoregressive_generate call as the reference computes it:
    (L-1) * (F_step + F_conv) + VQ-VAE encode of B frames + decode of B(L-1) frames (the once-per-clip prologue, < 0.1 %,
    is left out).  F_step = N_tok (2 d^2 + 6 * 24 d^2) + N_tok 4 d (2 L + 64) + B (L-1) hw 2 d K."""
    n_tok = B * L * hw
    f_step = n_tok * (2 * d * d + 6 * 24 * d * d) + n_tok * 4 * d * (2 * L + 64) + B * (L - 1) * hw * 2 * d * K
    f_conv = B * (L - 1) * hw * 18 * d * d
    f_tab = (L - 1) * (f_conv + B * (L - 1) * hw * 2 * d * d)     # frame conv + in_linear: not executed when they run as a table sum
    return (L - 1) * (f_step + f_conv) + B * DEC_FLOP_PER_FRAME + B * (L - 1) * DEC_FLOP_PER_FRAME, f_step, f_tab


def hbm_view(key, dom):
    """The same launches against the HBM roof: algorithmic bytes (every operand of every timed launch once: A + W + output(s) + the
    fp32 residual, summed by mage_amd.ops.gemm over the launches actually made, so the out_proj : c_proj mix is the real one)
    over the summed launch time.  Reported BESIDE the MFMA fraction (SURVEY 8d assigns the transformer step the MFMA roof)."""
    if not dom.get("bytes"):
        return None
    bytes_per_launch = dom["bytes"] / dom["calls"]
    us = dom["ms"] * 1e3 / dom["calls"]
    gbs = bytes_per_launch / (us * 1e-6) / 1e9
    return {"bound": "hbm", "algorithmic_bytes_per_launch": bytes_per_launch, "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(gbs / PEAK_HBM_GBS, 4), "flop_per_byte": round(dom["flops"] / dom["calls"] / bytes_per_launch, 1),
            "machine_balance_flop_per_byte": round(PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9), 1)}


def train_step_probe(args, dev, rank, world, B, L, wl_kw, D):
    import gc
    from mage_amd.optim import FlatAdam
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config
    gc.collect()
    torch.cuda.empty_cache()
    tm = instantiate_from_config(synth.mnist_model_config(frames_length=L))
    synth.fill_state_dict(tm, 0)
    tm = tm.to(dev).set_precision("bf16").train()
    opt = FlatAdam(tm.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-6)          # main_mage.py:121; sharded over the ranks when world > 1
    tb = {k: v.to(dev) for k, v in synth.synth_batch_mnist(B, L, seed=300 + rank, **wl_kw).items()}

    def one():
        opt.zero_grad()
        loss, _ = tm(tb)
        loss.backward()
        opt.step()
        return loss
    losses = [one().item() for _ in range(2)]                     # warm-up (allocator, derived weight copies, RCCL channels)
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 4
    for _ in range(n):
        last = one()
    D.barrier()
    torch.cuda.synchronize()
    dtt = D.max_over_ranks(time.perf_counter() - t0, dev)
    losses.append(last.item())
    n_par = sum(p.numel() for p in tm.parameters() if p.requires_grad)
    out = {"value": round(world * B * L * n / dtt, 1), "unit": "frames/s trained", "ms_per_step": round(dtt / n * 1e3, 2), "steps": n,
           "batch_per_gpu": B, "frames": L, "dtype": "bf16", "scaling": "weak", "trainable_parameters": n_par,
           "exchange": (f"reduce_scatter + all_gather of the {n_par * 4 / 2**20:.0f} MiB fp32 arena over RCCL, {world} ranks" if world > 1
                        else "none (1 rank)"),
           "loss_first_last": [round(losses[0], 4), round(losses[-1], 4)],
           "note": "secondary measurement (the reference's training loop body on the HIP path, synthetic batch resident on the device); "
                   "not part of `value`"}
    del tm, opt, tb
    gc.collect()
    torch.cuda.empty_cache()
    return out


def train_strokes_model(dev, L, train_steps, B, cfg_kw=None, style="strokes", s1_steps=None):
    """The in-tree trained model of the token-agreement legs (trained_token_agreement below, tools/f16_attribution.py): stage 1 (VQ-VAE) and
    stage 2 (MAGE) trained with the HIP training path on synthetic 'strokes' clips, everything seeded.  Returns (model in eval mode on dev,
    CPU fp32 state_dict, info dict: loss trajectories, the weights' sha256, stage-1 facts)."""
    from mage_amd.optim import FlatAdam
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config
    from oracle import mage_oracle as O
    import torch.nn.functional as F
    from mage_amd.modules.vqvae_model import VectorQuantizedVAE
    torch.manual_seed(20250930)                                                # MAGE.forward draws its dropout seeds from torch's generator
    cfg = synth.mnist_model_config(frames_length=L, **(cfg_kw or {}))          # cfg_kw: a smaller model (tests)
    fsp = cfg["params"]["first_stage_config"]["params"]
    tm = instantiate_from_config(cfg)
    synth.fill_state_dict(tm, 0, d_model=cfg["params"]["vision_width"], n_layers=cfg["params"]["generate_decoder_config"]["params"]["layers"])
    pool = [{k: v.to(dev) for k, v in synth.synth_batch_mnist(B, L, seed=1000 + i, style=style).items()} for i in range(8)]
    # stage 1 (train_vqvae.py:13-35 on the HIP path)
    vq = VectorQuantizedVAE(fsp["input_dim"], fsp["down_ratio"], fsp["dim"], fsp["K"])
    synth.fill_state_dict(vq, 0)
    vq = vq.to(dev).train()
    opt1 = FlatAdam(vq.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    frames = torch.cat([b["images"].reshape(-1, 1, 64, 64) for b in pool], 0)
    s1_losses = []
    s1_steps = max(50, train_steps) if s1_steps is None else s1_steps
    reseed_at = 20 if style == "strokes" else -1
    gidx = torch.Generator().manual_seed(0)
    for it in range(s1_steps):
        x = frames[torch.randperm(frames.shape[0], generator=gidx)[:256].to(dev)].contiguous()
        opt1.zero_grad()
        x_tilde, z_e, z_q = vq(x)
        l1 = F.mse_loss(x_tilde, x) + F.mse_loss(z_q, z_e.detach()) + 2.0 * F.mse_loss(z_e, z_q.detach())
        l1.backward()
        opt1.step()
        if it == reseed_at:
            # data-dependent codebook initialisation: K encoder outputs, half of them from pixels that are not background (harness plumbing:
            # which rows of z_e to copy)
            with torch.no_grad():
                ze = z_e.detach().permute(0, 2, 3, 1).reshape(-1, z_e.shape[1]).float()
                fg = (F.max_pool2d(x, 4) > -0.45).permute(0, 2, 3, 1).reshape(-1)
                gsel = torch.Generator().manual_seed(1)
                idx_fg, idx_all = fg.nonzero().flatten().cpu(), torch.arange(ze.shape[0])
                pick = torch.cat([idx_fg[torch.randperm(idx_fg.numel(), generator=gsel)[:fsp["K"] * 3 // 4]],
                                  idx_all[torch.randperm(idx_all.numel(), generator=gsel)[:fsp["K"]]]])[:fsp["K"]]
                vq.codebook.embedding.weight.copy_(ze[pick.to(dev)])
        if it % max(1, s1_steps // 4) == 0 or it == s1_steps - 1:
            s1_losses.append(round(l1.item(), 5))
    vq.eval()
    tm.first_stage_model.load_state_dict(vq.state_dict())
    del opt1
    tm = tm.to(dev).set_precision("bf16").train()
    opt = FlatAdam(tm.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-6)
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(train_steps):
        opt.zero_grad()
        loss, _ = tm(pool[it % len(pool)])
        loss.backward()
        opt.step()
        if it % max(1, train_steps // 6) == 0 or it == train_steps - 1:
            losses.append(round(loss.item(), 4))
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    tm.eval()
    sd = {k: v.detach().float().cpu().clone() for k, v in tm.state_dict().items()}
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(sd[k].numpy().tobytes())
    info = dict(train_seconds=round(t_train, 1), loss_trajectory=losses, trained_weights_sha256=h.hexdigest()[:16], s1_steps=s1_steps,
                s1_losses=s1_losses, reseed_at=reseed_at)
    del opt, pool
    return tm, sd, info


def trained_token_agreement(dev, L, train_steps, B, clips, threads, cfg_kw=None, style="strokes", s1_steps=None):
    """north_star asks for reference-matching VQ token sequences; with RANDOM-INIT weights the decoder's top-2 logit margins (6e-6 .. 3e-4)
    sit below any 16-bit mode's logit error, so those modes must diverge there whatever the kernels do.  This leg gives the weights a trained
    model's margins: stage 1 (VQ-VAE, train_vqvae.py:13-35) and stage 2 (MAGE, main_mage.py:139-154) are trained with the in-tree HIP
    training path on synthetic clips, then HELD-OUT clips are generated free-running by the HIP path in bf16, f16 and f16x3 and by the CPU
    oracle (fp32, the reference's algorithm) from the same weights.

    The task (style 'strokes', mage_amd.utils.synth): stroke drawings of ten shape classes with random width, intensity and shading, moved by
    the reference's bounce rule, the caption naming the class and the motion (so the next frame is predictable); the codebook is re-seeded
    from encoder outputs early in stage 1 (a data-dependent initialisation: a random-init codebook collapses onto a handful of codes, which
    made round 4's task trivial -- 8 codes, median margin 12).  Everything is seeded (torch.manual_seed for the dropout seeds; the embedding
    gradients are fixed-order sums): the same weights, hence the same figures, from run to run on one box.

    Reported per mode: free-running token agreement with the oracle, clips identical, where each clip first leaves the oracle's sequence and
    the oracle's margin there, the teacher-forced max |d logit| against the oracle's own per-step logits; and the oracle's margin
    distribution."""
    import gc
    from mage_amd.utils import synth
    from oracle import mage_oracle as O
    tm, sd, tinfo = train_strokes_model(dev, L, train_steps, B, cfg_kw=cfg_kw, style=style, s1_steps=s1_steps)
    losses, t_train, s1_losses, s1_steps, reseed_at = (tinfo["loss_trajectory"], tinfo["train_seconds"], tinfo["s1_losses"], tinfo["s1_steps"],
                                                       tinfo["reseed_at"])
    held = synth.synth_batch_mnist(clips, L, seed=5000, style=style)
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    with torch.no_grad():
        _, o_tok, _, o_trace = O.mage_generate(sd, held, L, return_trace=True)
    t_cpu = time.perf_counter() - t0
    top2 = o_trace.topk(2, dim=-1)[0]
    margin = (top2[..., 0] - top2[..., 1]).abs()
    hb = {k: v.to(dev) for k, v in held.items()}
    tm.ar_mode = "full"
    R = tm.image_resolution

    def teacher_forced_err(prec):
        """max |d logit| of one decoder pass in `prec` fed the ORACLE's token sequence, against the oracle's own per-step logits (by causality
        the logits its AR loop saw at each step)."""
        tm.set_precision(prec)
        dt_ = tm._dt()
        tok0 = tm.first_stage_encode(hb["images"][:, 0:1])[:, 0].reshape(clips, -1)
        ctx = torch.cat([tok0[:, None, :], o_tok.to(dev).reshape(clips, L - 1, -1)[:, :L - 2]], 1).contiguous()
        ma = tm._motion_anchor(tok0.contiguous(), hb, None)
        feats = tm._frame_source(ctx, dt_)
        lg = tm.generate_model._run(ma if dt_ == torch.float32 else ma.to(dt_), feats, B=clips, hh=R, ww=R).view(clips, L - 1, R, R, -1)
        lg = lg.float().cpu()
        am = lg.argmax(-1)
        bad = am != o_tok.reshape(am.shape)
        err_ = float((lg - o_trace.reshape(lg.shape)).abs().max())
        # per-DECISION agreement (every position sees the oracle's context: no compounding), and whether every disagreement sits at a
        # decision the oracle took by less than twice this mode's measured error
        return err_, {"token_agreement": round(1.0 - bad.float().mean().item(), 6), "mismatches": int(bad.sum()),
                      "mismatches_where_oracle_margin_above_twice_the_error": int((bad & (margin.reshape(am.shape) > 2 * err_)).sum()),
                      "largest_margin_of_a_mismatch": round(float(margin.reshape(am.shape)[bad].max()), 6) if bad.any() else None}
    out, errs, tfs = {}, {}, {}
    for prec in ("bf16", "f16", "f16x3"):
        try:
            errs[prec], tfs[prec] = teacher_forced_err(prec)
        except Exception as e:
            errs[prec], tfs[prec] = None, None
            out[prec + "_error"] = f"{type(e).__name__}: {e}"[:200]
    for prec in ("bf16", "f16", "f16x3"):
        tm.set_precision(prec)
        tm.autoregressive_generate(hb)
        got = tm.last_tokens.cpu()
        eq = got == o_tok
        first_bad = [int((~eq[c]).flatten().nonzero()[0]) if (~eq[c]).any() else -1 for c in range(clips)]
        per_frame = [round(eq[:, f].float().mean().item(), 4) for f in range(eq.shape[1])]
        err = errs.get(prec)
        out[prec] = {"all_positions": round(eq.float().mean().item(), 5), "clips_identical": round(eq.flatten(1).all(1).float().mean().item(), 5),
                     "clips_identical_count": f"{int(eq.flatten(1).all(1).sum())} of {clips}",
                     "teacher_forced_max_logit_error_vs_oracle": err,
                     "teacher_forced": tfs.get(prec),
                     "agreement_per_generated_frame": per_frame,
                     # a free-running sequence re-seeds itself at its first flipped token (every later position sees other inputs), so the
                     # question for a clip is where its FIRST divergence happens: at a decision the oracle itself took by less than the
                     # mode's logit error, or not
                     "first_divergences_inside_twice_the_modes_logit_error": (all(i < 0 or float(margin[c].flatten()[i]) <= 2 * err
                                                                                   for c, i in enumerate(first_bad)) if err is not None else None),
                     "first_divergence_margin": [round(float(margin[c].flatten()[i]), 6) if i >= 0 else None for c, i in enumerate(first_bad)],
                     "first_divergence_position": first_bad}
    out["bf16"]["first_divergences_inside_twice_the_bf16_logit_error"] = out["bf16"]["first_divergences_inside_twice_the_modes_logit_error"]
    q = torch.quantile(margin.flatten().double(), torch.tensor([0.001, 0.01, 0.1, 0.5, 0.9], dtype=torch.float64)).tolist()
    # the same quantiles over the decisions that are not 'background stays background' (the oracle's token differs from the clip's most
    # frequent token): the sprite's positions, where the task is
    bg = torch.mode(o_tok.reshape(clips, -1), dim=1)[0].view(clips, *([1] * (o_tok.dim() - 1)))
    fgm = margin[o_tok != bg]
    qf = (torch.quantile(fgm.flatten().double(), torch.tensor([0.001, 0.01, 0.1, 0.5, 0.9], dtype=torch.float64)).tolist()
          if fgm.numel() else [None] * 5)
    with torch.no_grad():
        codes_used = int(torch.unique(tm.first_stage_encode(hb["images"])).numel())
    res = dict(out, task=style, train_steps=train_steps, train_batch=B, train_seconds=t_train, loss_trajectory=losses,
               trained_weights_sha256=tinfo["trained_weights_sha256"],
               stage1={"steps": s1_steps, "batch_frames": 256, "loss_trajectory": s1_losses, "codes_used_on_the_held_out_clips": codes_used,
                       "distinct_tokens_in_the_oracle_sequences": int(torch.unique(o_tok).numel()),
                       "codebook_reseeded_from_encoder_outputs_at_step": reseed_at if reseed_at >= 0 else None},
               clips=clips, positions=int(o_tok.numel()), oracle_seconds=round(t_cpu, 1), bf16_teacher_forced_max_logit_error=errs.get("bf16"),
               oracle_top2_margin_quantiles={"0.1%": q[0], "1%": q[1], "10%": q[2], "50%": q[3], "90%": q[4], "min": float(margin.min())},
               oracle_top2_margin_quantiles_non_background={"positions": int(fgm.numel()), "0.1%": qf[0], "1%": qf[1], "10%": qf[2], "50%": qf[3],
                                                            "90%": qf[4]},
               positions_with_margin_below={"1e-3": int((margin < 1e-3).sum()), "1e-2": int((margin < 1e-2).sum()), "3e-2": int((margin < 3e-2).sum()),
                                            "1e-1": int((margin < 1e-1).sum())},
               note="cfg2 model TRAINED in-tree (HIP forward / backward / FlatAdam, bf16; seeded, fixed-order gradient sums: `trained_weights_sha256` "
                    "repeats from run to run) on synthetic stroke clips, then held-out clips generated free-running: HIP bf16, f16 and f16x3 against "
                    "the CPU oracle on the same trained weights.  A free-running sequence can only stay identical while every decision's margin "
                    "exceeds the mode's logit error (teacher_forced_max_logit_error_vs_oracle); the margin quantiles say how many decisions of this "
                    "trained model sit below that")
    del tm
    gc.collect()
    torch.cuda.empty_cache()
    return res


F8_DEC_FLOP_PER_FRAME, F8_ENC_FLOP_PER_FRAME = 11.333e9, 14.185e9          # f8 VQ-VAE, 128x128 RGB
F8_DEC_BYTES_PER_FRAME = {"bf16": 51.1e6, "fp32": 102.2e6}                 # layer-materialised traffic model of SURVEY.md 8d (fp32: 102.2 MB)
F8_ENC_BYTES_PER_FRAME = {"bf16": 52.25e6, "fp32": 104.5e6}


def build_cfg4_model(dev):
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config
    m4 = instantiate_from_config(synth.cater_model_config(frames_length=32)).eval()
    synth.fill_state_dict(m4, 0)
    return m4.to(dev)


def cfg4_probe(m4, dev, B=32, L=32):
    """BASELINE cfg4 (config/mage_caterv1.yaml: CATER-GEN-v1 128x128, 32 frames, batch 32, f8 VQ-VAE, randomness branch with the noise
    injected) on this GPU, on the driver's clock: ms per autoregressive_generate call in both AR modes (bf16, f16), and the f8 VQ-VAE
    decode / encode stacks on their own against SURVEY 8d's per-frame FLOPs and bytes."""
    from mage_amd.utils import synth
    batch = {k: v.to(dev) for k, v in synth.synth_batch_cater(B, L, seed=1).items()}
    batch["video_noise"] = torch.randn(B, 64, 16, 16, generator=torch.Generator().manual_seed(9)).to(dev)
    saved = (m4.precision, m4.ar_mode, m4.use_graph)
    m4.use_graph = False
    out = {"workload": f"cfg4: CATER-GEN-v1-shaped clips 128x128, {L} frames, batch={B}, f8 VQ-VAE (dim 256, codebook D = 1024) + MAGE "
                       "(randomness branch, injected noise), random-init weights", "unit": "ms per autoregressive_generate call"}

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    toks = {}
    for prec in ("bf16", "f16"):
        m4.set_precision(prec)
        row = {}
        for mode, n in (("full", 3), ("incremental", 3)):
            m4.ar_mode = mode
            ms = timed(lambda: m4.autoregressive_generate(batch), n)
            toks[(prec, mode)] = m4.last_tokens.clone()
            row[mode] = {"ms_per_call": round(ms, 2), "frames_per_s": round(B * L / ms * 1e3, 1), "calls_timed": n}
        row["incremental_tokens_identical_to_full"] = bool(torch.equal(toks[(prec, "full")], toks[(prec, "incremental")]))
        out[prec] = row
    # the f8 stacks alone (bf16 decode of the B*(L-1) generated frames; the encoder runs on B first frames per call, timed on B*(L-1) too)
    m4.set_precision("bf16")
    gen = toks[("bf16", "full")]
    frames = gen.shape[0] * gen.shape[1]
    ms_d = timed(lambda: m4.first_stage_decode(gen), 5)
    tf = F8_DEC_FLOP_PER_FRAME * frames / (ms_d * 1e-3) / 1e12
    gbs = F8_DEC_BYTES_PER_FRAME["bf16"] * frames / (ms_d * 1e-3) / 1e9
    out["roofline_decode_f8"] = {"frames": frames, "ms": round(ms_d, 3), "dtype": "bf16",
                                 "mfma": {"achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4)},
                                 "hbm_model": {"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                                               "bytes_model_per_frame": F8_DEC_BYTES_PER_FRAME["bf16"]},
                                 "flop_per_frame": F8_DEC_FLOP_PER_FRAME,
                                 "note": "VectorQuantizedVAE.decode (f8: 1024-wide codebook rows -> 4 bottleneck DecoderBlocks, 3 of them behind a nearest upsampling "
                                         "that is folded into the block's gathers -> 1x1 RGB head + tanh) of the call's generated frames; 221 FLOP per byte of the "
                                         "layer-materialised model: MFMA-bound, the HBM figure is SURVEY 8d's bf16 byte model over the same time.  Launches per "
                                         "block: 1x1 (leading ReLU on its operand fragments), two 3x3 64 -> 64 tile convolutions (csrc/conv_tile.hip: input window "
                                         "and weights resident in LDS), closing 3x3 in the padded-taps form with the identity path added in its epilogue; the last "
                                         "block's closing convolution also takes the decoder's ReLU and the RGB head on its tile (its 8 MB-per-frame output never stored)"}
    imgs = batch["images"].reshape(-1, 3, 128, 128)[:frames // 4].contiguous()      # a quarter of the frames (the exact-fp32 encoder: 16x the MFMA time)
    ms_e = timed(lambda: m4.first_stage_model.encode(imgs), 2)
    tfe = F8_ENC_FLOP_PER_FRAME * imgs.shape[0] / (ms_e * 1e-3) / 1e12
    out["encode_f8"] = {"frames": int(imgs.shape[0]), "ms": round(ms_e, 3), "dtype": "fp32 (exact-fp32 MFMA chains: the f8 encoder keeps token indices bit-exact in every precision mode)",
                        "achieved": round(tfe, 1), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": round(tfe / PEAK_F32_TFLOPS, 4),
                        "flop_per_frame": F8_ENC_FLOP_PER_FRAME}
    m4.set_precision(saved[0])
    m4.ar_mode, m4.use_graph = saved[1], saved[2]
    # the cfg4 TRAINING step (main_mage.py:142-154 on the HIP path: MAGE.forward with the randomness branch, backward, FlatAdam), bf16, and the
    # share of it that is the frozen f8 encoder tokenising the batch's B*L frames (mage_model.py:579; exact-fp32 chains)
    try:
        # (MAGE.forward's video prior collapses the clip with four stride-2 Conv3d blocks, mage_model.py:496-501,592-594: at most 16 frames, the
        # reference's own configs train on 10: the step is timed on the first 16 frames of the cfg4 batch)
        Lt = min(L, 16)
        out["train_step"] = cfg4_train_probe(dev, B, Lt, {k: (v[:, :Lt].contiguous() if k == "images" else v) for k, v in batch.items()})
    except Exception as e:                          # the generation figures above stay
        out["train_step"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return out


def cfg4_train_probe(dev, B, L, batch):
    import gc
    from mage_amd.optim import FlatAdam
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config
    gc.collect()
    torch.cuda.empty_cache()
    torch.manual_seed(4)
    tm = instantiate_from_config(synth.cater_model_config(frames_length=L))
    synth.fill_state_dict(tm, 0)
    tm = tm.to(dev).set_precision("bf16").train()
    opt = FlatAdam(tm.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-6)
    tb = {k: v for k, v in batch.items() if k != "video_noise"}

    def one():
        opt.zero_grad()
        loss, _ = tm(tb)
        loss.backward()
        opt.step()
        return loss
    l0 = one().item()
    one()                                            # second warm-up: the caching allocator and the arena hand-over settle in the first two steps
    n = 4
    per = []
    for _ in range(n):                               # per-step wall times, median: one step in a few hits an allocator refill (seen: 395 vs 180 ms)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = one()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(per)[n // 2]
    with torch.no_grad():
        tm.first_stage_encode(tb["images"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tm.first_stage_encode(tb["images"])
        torch.cuda.synchronize()
        ms_enc = (time.perf_counter() - t0) * 1e3
    res = {"ms_per_step": round(ms, 2), "frames_per_s_trained": round(B * L / ms * 1e3, 1), "steps_timed": n, "batch": B, "frames": L, "dtype": "bf16",
           "ms_per_step_each": [round(x, 1) for x in per], "encode_ms": round(ms_enc, 2), "encode_share": round(ms_enc / ms, 3), "loss_first_last": [round(l0, 4), round(last.item(), 4)],
           "trainable_parameters": sum(p.numel() for p in tm.parameters() if p.requires_grad),
           "note": "secondary: the reference's training loop body at cfg4 (randomness branch: Conv3d video prior, KL term), 1 GPU; encode = the frozen f8 "
                   "VQ-VAE tokenising the step's B*L frames on exact-fp32 chains"}
    del tm, opt
    gc.collect()
    torch.cuda.empty_cache()
    return res


def latency_b1(model2, dev, L, m4=None):
    """The reference's own sampling shape (main_mage.py:205,239-241: DataLoader(batch_size=1), one autoregressive_generate call per
    clip): wall milliseconds per clip at B = 1, HIP-graph replay on (the call is launch-bound at this size), for the cfg2 model
    (MNIST f4, L frames of 64x64) and the cfg4 model (config/mage_caterv1.yaml, 32 frames of 128x128, randomness branch with the
    noise injected), both AR modes, the bf16 mode and the fast parity mode f16x3.  Median of 7 replays after warm-up + capture."""
    import gc
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config

    def measure(model, batch):
        out = {}
        saved = (model.precision, model.ar_mode, model.use_graph, model.streams)
        model.streams = 1
        for prec in ("bf16", "f16x3"):
            model.set_precision(prec)
            for mode in ("full", "incremental"):
                model.ar_mode = mode
                row = {}
                for graph in (True, False):
                    model.use_graph = graph
                    for _ in range(3):                       # eager warm-up, capture, first replay
                        model.autoregressive_generate(batch)
                    torch.cuda.synchronize()
                    ts = []
                    for _ in range(7):
                        t0 = time.perf_counter()
                        model.autoregressive_generate(batch)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    row["graph" if graph else "eager"] = round(sorted(ts)[3], 3)
                    row["replayed"] = row.get("replayed", False) or (graph and getattr(model, "last_call_mode", "eager") == "graph")
                out[f"{prec}/{mode}"] = {"ms_per_clip": row["graph"] if row["replayed"] else row["eager"], "ms_per_clip_eager": row["eager"],
                                         "graph_replayed": row["replayed"]}
        model.set_precision(saved[0])
        model.ar_mode, model.use_graph, model.streams = saved[1], saved[2], saved[3]
        model._graphs = {}
        return out
    res = {"unit": "ms per clip (B = 1), wall, median of 7",
           "note": "the reference samples one clip per call (main_mage.py:205,239-241); B = 1 equals row 0 of a larger batch bitwise "
                   "(tests/test_gpu_parity.py::test_single_clip_equals_row_of_a_batch)"}
    b2 = {k: v.to(dev) for k, v in synth.synth_batch_mnist(1, L, seed=77).items()}
    res["cfg2_model"] = dict(measure(model2, b2), clip=f"{L} frames of 64x64")
    gc.collect()
    torch.cuda.empty_cache()
    L4 = 32
    if m4 is None:
        m4 = build_cfg4_model(dev)
    b4 = {k: v.to(dev) for k, v in synth.synth_batch_cater(1, L4, seed=78).items()}
    b4["video_noise"] = torch.randn(1, 64, 16, 16, generator=torch.Generator().manual_seed(9)).to(dev)
    res["cfg4_model"] = dict(measure(m4, b4), clip=f"{L4} frames of 128x128 (config/mage_caterv1.yaml, f8 VQ-VAE)")
    del m4, b4
    gc.collect()
    torch.cuda.empty_cache()
    return res


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg3"],
                    help="cfg2: Single Moving MNIST (one digit, 11-token captions); cfg3: Double Moving MNIST (two digits, "
                         "captions of 16/18/20 tokens right-padded to 20)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--batch", type=int, default=64, help="clips per GPU (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=256, help="clips in total (strong scaling; split evenly over the ranks)")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16", "fp32", "f16x3", "bf16x3"])
    ap.add_argument("--ar-mode", default="full", choices=["full", "incremental"],
                    help="full = the reference's per-iteration full recompute (headline); incremental = temporal KV cache")
    ap.add_argument("--streams", type=int, default=1,
                    help="clip groups on concurrent HIP streams inside one generate call (2: +4 %% frames/s, but per-kernel "
                         "event times then overlap: the roofline object needs 1)")
    ap.add_argument("--graph", type=int, default=0,
                    help="1: replay each call from ONE captured HIP graph (MAGE.use_graph).  Measured on MI355X (profiles/r02_graph_probe.txt): "
                         "no gain in either AR mode -- the launch loop is GPU-bound (3 %% idle in incremental mode, 2 %% in full mode) -- and "
                         "ROCm cannot capture timing events as graph nodes, so the per-kernel events of the roofline need eager launches")
    ap.add_argument("--events", default="dominant", choices=["dominant", "all"],
                    help="HIP events inside the timed region: around the dominant GEMM symbol's launches only (it is found, "
                         "and the per-kernel table filled, in the last warm-up call, which brackets every launch), or around "
                         "every GEMM / attention / LayerNorm launch (~1 %% slower)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run the secondary measurements below (a plain run times the headline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-mode", action="store_true", help="skip the second AR mode (clean rocprofv3 runs)")
    ap.add_argument("--no-parity-mode", action="store_true", help="skip the fp32 (parity-gated) pass and the bf16-vs-fp32 token agreement")
    ap.add_argument("--no-decode-roofline", action="store_true")
    ap.add_argument("--no-train-step", action="store_true", help="skip the secondary training-step measurement")
    ap.add_argument("--no-latency-b1", action="store_true", help="skip the B = 1 latency table (rank 0 at N = 1 only)")
    ap.add_argument("--no-cfg4", action="store_true", help="skip the secondary BASELINE cfg4 object (CATER 128x128, 32 frames, batch 32; rank 0 at N = 1 only)")
    ap.add_argument("--trained-steps", type=int, default=300, help="training steps of the trained-weights token-agreement leg (0 = skip; rank 0 at N = 1, with the CPU baseline)")
    ap.add_argument("--cpu-clips", type=int, default=4, help="clips of the CPU baseline sample (4 = SURVEY cfg1, the reference's CPU-runnable batch)")
    ap.add_argument("--trained-clips", type=int, default=16, help="held-out clips of the trained-weights token-agreement leg (each costs ~6 s of CPU oracle)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed autoregressive_generate call returned as DIR/<name>.npy "
                         "(float32: video [B,L,C,H,W], tokens [B,L-1,16,16]; rank r > 0 of a multi-GPU run adds _rank<r>).  The inputs "
                         "and weights are seeded, so two builds run with the same arguments can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


def dump_outputs(out_dir, arrays, rank, world):
    """The timed path's outputs as float32 .npy files (at the default shapes 16.8 MB of video + 61 KB of tokens per rank)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = f"_rank{rank}" if world > 1 else ""
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a.detach().to("cpu", torch.float32).contiguous().numpy())


def without_notes(obj):
    """The result line without its prose ("note", "*_note" and the kernel legend): every number stays, and the line stays short
    enough for drivers that read a bounded tail of the output."""
    if isinstance(obj, dict):
        return {k: without_notes(v) for k, v in obj.items() if not (k == "note" or k.endswith("_note"))}
    if isinstance(obj, list):
        return [without_notes(v) for v in obj]
    return obj


def main():
    args = parse()
    _t = {"last": time.perf_counter(), "sec": {}}

    def tick(name):
        """wall seconds since the previous tick, kept per section (bench_sections_s of the line: where a default run's minutes go)"""
        now = time.perf_counter()
        _t["sec"][name] = round(_t["sec"].get(name, 0.0) + now - _t["last"], 1)
        _t["last"] = now
    from mage_amd.utils import dist as D
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not under a launcher: start the N ranks ourselves (one process per GPU) and relay the exit code
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            sys.exit(f"bench.py --gpus {args.gpus}: only {n_dev} GPU(s) visible")
        sys.exit(D.launch_ranks([os.path.abspath(__file__)] + sys.argv[1:], args.gpus))
    rank, local_rank, world = D.env_rank_world()
    if world != args.gpus and rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    D.init_from_env("nccl", dev)            # backend "nccl" is RCCL on ROCm; only barrier / max-reduce / ranks_seen use it
    seen = D.ranks_seen(dev)

    from mage_amd import ops
    from mage_amd.utils import synth
    from mage_amd.utils.util import instantiate_from_config

    L = args.frames
    wl_kw = dict(digits=1) if args.workload == "cfg2" else dict(digits=2, caption_lengths=(16, 18, 20))
    if args.scaling == "strong":
        if args.global_batch % world:
            sys.exit(f"--global-batch {args.global_batch} is not divisible by {world} ranks")
        B = args.global_batch // world
        batch = D.shard_batch(synth.synth_batch_mnist(args.global_batch, L, seed=100, **wl_kw), rank, world)
    else:
        B = args.batch
        batch = synth.synth_batch_mnist(B, L, seed=100 + rank, **wl_kw)
    cfg = synth.mnist_model_config(frames_length=L)
    model = instantiate_from_config(cfg).eval()
    synth.fill_state_dict(model, 0)
    cpu_sd = ({k: v.detach().clone() for k, v in model.state_dict().items()}
              if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline else None)      # CPU baseline: rank 0 at N=1 only
    model = model.to(dev).set_precision(args.precision)
    model.ar_mode = args.ar_mode
    model.streams = args.streams
    if hasattr(model, "use_graph"):
        model.use_graph = bool(args.graph)
    batch = {k: v.to(dev) for k, v in batch.items()}

    def sync_all():
        D.barrier()
        torch.cuda.synchronize()

    def prime():
        """Graph replay: the first call of a (shape, mode, profiling) combination is eager, the second captures the graph;
        both happen here, outside any timed region."""
        if getattr(model, "use_graph", False):
            model.autoregressive_generate(batch)
            model.autoregressive_generate(batch)

    for _ in range(max(args.warmup - 1, 0)):
        model.autoregressive_generate(batch)
    sync_all()
    # last warm-up call (or an extra one): every instrumented launch bracketed by HIP events -> the per-kernel table and the
    # dominant GEMM symbol.  Not timed.  (Events bracket eager launches: graph replay is off for this one call.)
    ops.PROFILE.reset(enabled=True)
    model.autoregressive_generate(batch)
    warm_prof = ops.PROFILE.summary()
    warm_gemms = {k: v for k, v in warm_prof.items() if k.startswith(("gemm_kernel", "gemm8_kernel", "gemm4_kernel", "gemm4h_kernel", "gemm_split"))}
    dom_warm = max(warm_gemms, key=lambda k: warm_gemms[k]["ms"]) if warm_gemms else None
    sync_all()
    # timed region: HIP events on the launch stream around the dominant symbol's launches (--events all: around all).  With
    # graph replay the event pairs are event-record nodes of the captured graph (same stream, same positions).
    ops.PROFILE.reset(enabled=True, only=None if (args.events == "all" or dom_warm is None) else [dom_warm, "decoder_step"])
    prime()
    ops.PROFILE.clear()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = model.autoregressive_generate(batch)
    sync_all()
    dt = time.perf_counter() - t0
    ops.PROFILE.enabled = False
    dt = D.max_over_ranks(dt, dev)
    assert tuple(out.shape) == (B, L, 1, 64, 64)
    tok_main = model.last_tokens.clone()
    if args.dump_outputs:                      # outside the timed region, before any other call can touch the model's buffers
        dump_outputs(args.dump_outputs, {"video": out, "tokens": tok_main}, rank, world)
    prof = ops.PROFILE.summary()
    replayed = getattr(model, "last_call_mode", "eager") == "graph"

    # the other AR mode, same batch, reported next to the headline (identical tokens: tests/test_gpu_parity.py)
    other_mode = "incremental" if args.ar_mode == "full" else "full"
    other = None
    tick("build_warmup_and_timed_headline")
    if args.full and not args.no_other_mode:
        model.ar_mode = other_mode
        model.streams = 1 if other_mode == "incremental" else args.streams     # small launches: concurrency only adds gaps
        model.autoregressive_generate(batch)
        same_tokens = bool(torch.equal(model.last_tokens, tok_main))
        prime()
        sync_all()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            model.autoregressive_generate(batch)
        sync_all()
        dt_other = D.max_over_ranks(time.perf_counter() - t1, dev)
        model.ar_mode = args.ar_mode
        model.streams = args.streams
        other = {"ar_mode": other_mode, "value": round(world * B * L * args.steps / dt_other, 2), "unit": "frames/s",
                 "ms_per_step": round(dt_other / args.steps * 1e3, 3), "tokens_identical_to_headline_mode": same_tokens}

    # the parity-gated precisions on the same batch: 'f16x3' (split-precision operands, three f16 MFMA products per K slab: passes
    # every fp32-mode golden gate of tests/ -- reference token sequences bit-exact, logits within 1e-4) timed in both AR modes, the
    # exact-fp32 MFMA mode beside it, and how far the free-running bf16 token sequence is from them
    parity = None
    if args.full and args.precision == "bf16" and not args.no_parity_mode:
        def timed(n):
            prime()
            sync_all()
            t_ = time.perf_counter()
            for _ in range(n):
                model.autoregressive_generate(batch)
            sync_all()
            return D.max_over_ranks(time.perf_counter() - t_, dev)

        def agreement(a_, b_):
            eq = (a_ == b_)
            v = torch.tensor([eq.float().mean().item(), eq[:, 0].float().mean().item(), eq.flatten(1).all(1).float().mean().item()],
                             dtype=torch.float64, device=dev)
            if world > 1:
                torch.distributed.all_reduce(v)
                v /= world
            return {"all_positions": round(v[0].item(), 5), "first_generated_frame": round(v[1].item(), 5), "clips_identical": round(v[2].item(), 5)}
        n3 = max(1, min(args.steps, 3))
        model.set_precision("f16x3")
        model.autoregressive_generate(batch)
        tok3 = model.last_tokens.clone()
        dt3 = timed(n3)
        model.ar_mode = other_mode
        model.autoregressive_generate(batch)
        same3 = bool(torch.equal(model.last_tokens, tok3))
        dt3o = timed(n3)
        model.ar_mode = args.ar_mode
        model.set_precision("fp32")
        model.autoregressive_generate(batch)
        tok32 = model.last_tokens.clone()
        dt32 = timed(1)
        model.set_precision(args.precision)
        parity = {"dtype": "f16x3", "value": round(world * B * L * n3 / dt3, 2), "unit": "frames/s", "ms_per_step": round(dt3 / n3 * 1e3, 3),
                  "steps": n3, "ar_mode": args.ar_mode,
                  "note": "f16x3 = the fast parity mode: fp32 everywhere except that the decoder's Linear layers and the frame convolution multiply "
                          "split-precision operands (x = hi + lo/2^11 in two f16 pieces; A_hi W_lo + A_lo W_hi, scaled, + A_hi W_hi on "
                          "v_mfma_f32_16x16x32_f16, fp32 accumulation).  It passes every fp32-mode golden gate (reference token sequences "
                          "bit-exact incl. the 7680-decision L=16 clip, logits within 1e-4: tests/test_gpu_split.py; measured 4.1e-6 vs the "
                          "exact-fp32 mode's 7.5e-6, profiles/r03_parity_report_{f16x3,fp32}.txt); its axial attention also runs as three f16 MFMA "
                          "passes per product on split q / k / v rows",
                  "other_ar_mode": {"ar_mode": other_mode, "value": round(world * B * L * n3 / dt3o, 2), "ms_per_step": round(dt3o / n3 * 1e3, 3),
                                    "tokens_identical": same3},
                  "exact_fp32": {"dtype": "fp32", "value": round(world * B * L / dt32, 2), "ms_per_step": round(dt32 * 1e3, 3), "steps": 1,
                                 "note": "v_mfma_f32_16x16x4_f32 chains (1/16 of the bf16 rate): round 1-2's parity mode"},
                  "speedup_vs_exact_fp32": round(dt32 / (dt3 / n3), 3),
                  "f16x3_vs_exact_fp32_token_agreement": agreement(tok3, tok32),
                  "bf16_free_running_token_agreement": dict(agreement(tok_main, tok3), note=(
                      "fraction of the HEADLINE (bf16) run's VQ tokens equal to the f16x3 run's on this batch; frame 1 has identical inputs in "
                      "both runs, later frames feed back each run's own tokens (one flip changes the rest of the clip).  With random-init "
                      "weights the top-2 logit margins (3e-6 .. 3e-4) are below the bf16 error, so bf16 must flip: the headline `value` is a "
                      "throughput number, the reference-matching-tokens number is parity_mode.value")),
                  "token_agreement_note": "two fp32-class evaluations differ where the top-2 margin is inside fp32 rounding noise (a few "
                                          "positions per 245760); each such flip re-seeds the rest of its clip"}

    # the single-pass f16 mode on the same batch: the bf16 kernels with IEEE half operands (same MFMA rate, 8x smaller roundings)
    f16m = None
    if args.full and args.precision == "bf16" and not args.no_parity_mode:
        try:
            nf = max(1, min(args.steps, 5))
            model.set_precision("f16")
            model.ar_mode = args.ar_mode
            model.autoregressive_generate(batch)
            tok16 = model.last_tokens.clone()
            prime()
            sync_all()
            t_ = time.perf_counter()
            for _ in range(nf):
                model.autoregressive_generate(batch)
            sync_all()
            dt16 = D.max_over_ranks(time.perf_counter() - t_, dev)
            model.ar_mode = other_mode
            model.autoregressive_generate(batch)
            same16 = bool(torch.equal(model.last_tokens, tok16))
            prime()
            sync_all()
            t_ = time.perf_counter()
            for _ in range(nf):
                model.autoregressive_generate(batch)
            sync_all()
            dt16o = D.max_over_ranks(time.perf_counter() - t_, dev)
            model.ar_mode = args.ar_mode
            model.set_precision(args.precision)
            f16m = {"dtype": "f16", "value": round(world * B * L * nf / dt16, 2), "unit": "frames/s", "ms_per_step": round(dt16 / nf * 1e3, 3),
                    "steps": nf, "ar_mode": args.ar_mode, "vs_headline": round((dt / args.steps) / (dt16 / nf), 4),
                    "other_ar_mode": {"ar_mode": other_mode, "value": round(world * B * L * nf / dt16o, 2), "ms_per_step": round(dt16o / nf * 1e3, 3),
                                      "tokens_identical": same16},
                    "free_running_token_agreement_with_f16x3": (agreement(tok16, tok3) if parity is not None else None),
                    "note": "set_precision('f16'): every kernel, schedule and buffer of the bf16 mode with IEEE half operands and rows "
                            "(v_mfma_f32_16x16x32_f16: the bf16 opcode's rate; 11 significand bits instead of 8).  Teacher-forced logits against "
                            "the reference's goldens: 0.002 (bf16: 0.016, tests/test_gpu_f16.py); on trained weights most held-out clips keep "
                            "the CPU oracle's exact token sequence where bf16 keeps hardly any (this line's cpu_baseline.gpu_tokens_vs_oracle_trained_weights: "
                            "clips_identical_count per mode).  "
                            "Which mode to run: 'f16x3' when the reference's tokens are wanted bit for bit (parity_mode); 'f16' for throughput "
                            "-- it costs nothing against 'bf16' and is 8x closer to the reference; 'bf16' only if activations could leave "
                            "f16's range (+-65504)"}
        except Exception as e:
            model.ar_mode = args.ar_mode
            model.set_precision(args.precision)
            f16m = {"error": f"{type(e).__name__}: {e}"[:300]}

    # VQ-VAE decode of this call's B*(L-1) generated frames on its own: HBM roofline under SURVEY 8d's traffic model + MFMA fraction
    decode = None
    tick("other_ar_mode_parity_mode_f16_mode")
    if args.full and not args.no_decode_roofline:
        gen = tok_main.view(B, L - 1, 16, 16)
        model.first_stage_decode(gen)
        torch.cuda.synchronize()
        reps = 10
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in evs:
            a.record()
            model.first_stage_decode(gen)
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]
        frames = B * (L - 1)
        by = DEC_BYTES_PER_FRAME["bf16" if args.precision == "bf16" else "fp32"] * frames
        gbs = by / (ms * 1e-3) / 1e9
        tf = DEC_FLOP_PER_FRAME * frames / (ms * 1e-3) / 1e12
        peak = PEAK_BF16_TFLOPS if args.precision == "bf16" else PEAK_F32_TFLOPS
        # HBM bytes of one decode call from PMC counters (tools/pmc_decode.sh: two rocprofv3 --pmc passes over tools/bench_vqvae.py at 960
        # frames, corrected as the guide prescribes); reported only for the size it was measured at
        dec_traffic, dec_src = None, None
        for dec_name in ("r05_pmc_decode.json", "r04_pmc_decode.json"):
            dec_pmc = os.path.join(ROOT, "profiles", dec_name)
            if os.path.exists(dec_pmc) and args.precision == "bf16" and dec_traffic is None:
                pj = json.load(open(dec_pmc))
                if pj.get("frames") == frames:
                    dec_traffic = pj.get("hbm_bytes_per_call")
                    dec_src = f"profiles/{dec_name} (builder's rocprofv3 --pmc passes via tools/pmc_decode.sh; not re-measured in this run)"
        decode = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                  "traffic": dec_traffic, "traffic_source": dec_src, "frames": frames, "ms": round(ms, 4), "bytes_model_per_frame": DEC_BYTES_PER_FRAME["bf16" if args.precision == "bf16" else "fp32"],
                  "mfma": {"achieved": round(tf, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4)},
                  "note": "VectorQuantizedVAE.decode of the call's generated frames (median of 10, HIP events); bytes = SURVEY 8d's "
                          "layer-materialised model (sum over the 6 conv layers of input+output activations at the storage dtype); "
                          "the same stack is 1.216 GFLOP/frame, so the MFMA fraction is reported beside it.  The bf16 path is 5 launches "
                          "(first ResBlock as one table-sum + MFMA kernel, the second block's 3x3 GEMM, its tail as a row kernel, ONE launch for the four "
                          "sub-pixel phases of the transposed convolution with the last transposed convolution's taps taken in its epilogue, fold + tanh): "
                          "the 4x-resolution activation, t and the embedded frames of the byte model never reach HBM, so the byte model counts more than is "
                          "moved (traffic = the measured bytes) and the HBM fraction is an upper bound; the MFMA fraction is the one to read"}

    # one more object, never the metric: the reference's training step (main_mage.py:139-154: forward, loss.backward(), Adam) on the same
    # model family and batch shape, per rank, with the gradient exchange of the data-parallel path -- reduce-scatter of the flat gradient
    # arena, Adam on this rank's shard, all-gather of the parameters, over RCCL when there is more than one rank (mage_amd.optim.FlatAdam).
    # This is the only place of the path with a real exchange step, so it is what an N > 1 run of this script measures RCCL with.
    train = None
    tick("decode_roofline")
    if args.full and args.precision == "bf16" and not args.no_train_step:
        try:
            train = train_step_probe(args, dev, rank, world, B, L, wl_kw, D)
        except Exception as e:                                   # never lets the secondary measurement take the bench line down
            train = {"error": f"{type(e).__name__}: {e}"[:300]}

    lat = cfg4 = None
    tick("train_step")
    if args.full and rank == 0 and world == 1 and args.precision == "bf16" and not (args.no_latency_b1 and args.no_cfg4):
        m4 = None
        try:
            m4 = build_cfg4_model(dev)
        except Exception as e:
            lat = cfg4 = {"error": f"{type(e).__name__}: {e}"[:300]}
        if m4 is not None and not args.no_cfg4:
            try:
                cfg4 = cfg4_probe(m4, dev)
            except Exception as e:
                cfg4 = {"error": f"{type(e).__name__}: {e}"[:300]}
        if m4 is not None and not args.no_latency_b1:
            try:
                lat = latency_b1(model, dev, L, m4)
            except Exception as e:
                lat = {"error": f"{type(e).__name__}: {e}"[:300]}
        del m4

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = world * B * L * args.steps / dt
        gemms = {k: v for k, v in prof.items() if k.startswith(("gemm_kernel", "gemm8_kernel", "gemm4_kernel", "gemm4h_kernel", "gemm_split"))}
        dom_key = max(gemms, key=lambda k: gemms[k]["ms"]) if gemms else None
        all_src, all_div = (gemms, args.steps) if args.events == "all" else (warm_gemms, 1)
        peak = PEAK_BF16_TFLOPS if args.precision in ("bf16", "f16") else PEAK_F32_TFLOPS
        roofline = None
        # HBM bytes per launch of the dominant kernel come from PMC counters (FETCH_SIZE x2-corrected + WRITE_SIZE), which
        # only rocprofv3 can read: tools/pmc_bench.sh collects them on this same command in two separate --pmc passes
        # and the summary is committed under profiles/; bench.py reports it only for the matching workload and says where from.
        traffic, traffic_source = None, None
        for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
            pmc_path = os.path.join(ROOT, "profiles", name)
            if dom_key and os.path.exists(pmc_path) and (B, L, args.precision, args.ar_mode, args.workload) == (64, 16, "bf16", "full", "cfg2"):
                traffic = json.load(open(pmc_path)).get(dom_key, {}).get("hbm_bytes_per_launch")
                if traffic is not None:
                    traffic_source = f"profiles/{name} (builder's rocprofv3 --pmc passes of this command via tools/pmc_bench.sh; not re-measured in this run)"
                    break
        if dom_key:
            dom = gemms[dom_key]
            ach = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
            allf, allms = sum(v["flops"] for v in all_src.values()), sum(v["ms"] for v in all_src.values())
            legend = ("  [gemm4_kernel<act, epilogue kind, LayerNorm fold, bf16 residual stream>: the one-wave-per-SIMD bf16 256x256 GEMM (4 waves of "
                      "128x128 outputs, all 256 accumulator registers: QKV at full-loop sizes, csrc/gemm4.hip); gemm4h_kernel<act, LayerNorm fold, f16>: its "
                      "split-half form with the epilogue under the K loop (c_fc at full-loop sizes, csrc/gemm4h.hip); "
                      "gemm8_kernel<act, epilogue kind, split-K, padded taps, LayerNorm fold, split precision(, bf16 residual stream)>: the 8-phase "
                      "ping-pong bf16 256x256 GEMM; gemm_kernel<dtype, gather, act, m-tiles/wave, epilogue kind, split-K, LayerNorm fold, n-waves, "
                      "split precision(, bf16 residual stream)>: the lockstep one.  act 2 = QuickGELU (c_fc).  Epilogue kind 1 = x + Linear(.): "
                      "attention out_proj and MLP c_proj of the decoder stack, the residual x loaded into the accumulators (bf16 rows when the "
                      "last argument is true: the bf16 mode keeps x in bf16 between the blocks); LayerNorm fold 1 = it also writes the row partial "
                      "sums the next Linear normalises with (2 = that consumer: QKV, c_fc)]")
            # the GEMM symbol with the second-largest time, same accounting (the x + Linear(.) producers when c_fc leads, or the reverse)
            second = None
            src2 = gemms if len(gemms) > 1 else warm_gemms            # --events dominant: the other symbols were bracketed in the last warm-up call
            rest = sorted((k for k in src2 if k != dom_key), key=lambda k: -src2[k]["ms"])
            if rest:
                g2 = src2[rest[0]]
                a2 = g2["flops"] / (g2["ms"] * 1e-3) / 1e12
                second = {"kernel": rest[0], "achieved": round(a2, 2), "frac": round(a2 / peak, 4),
                          "measured_in": "timed region" if src2 is gemms else "last warm-up call",
                          "launches_per_step": g2["calls"] // (args.steps if src2 is gemms else 1),
                          "avg_launch_us": round(g2["ms"] * 1e3 / g2["calls"], 2), "flops_per_launch": g2["flops"] / g2["calls"],
                          "hbm_view": hbm_view(rest[0], g2)}
            roofline = {"bound": "mfma", "kernel": dom_key, "kernel_note": legend.strip(),
                        "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                        "traffic": traffic, "traffic_source": traffic_source, "launches_per_step": dom["calls"] // args.steps,
                        "avg_launch_us": round(dom["ms"] * 1e3 / dom["calls"], 2),
                        "flops_per_launch": dom["flops"] / dom["calls"],
                        "hbm_view": hbm_view(dom_key, dom),
                        "second_kernel": second,
                        "all_gemm_kernels": {"achieved": round(allf / (allms * 1e-3) / 1e12, 2), "frac": round(allf / (allms * 1e-3) / 1e12 / peak, 4),
                                             "ms_per_step": round(allms / all_div, 3),
                                             "measured_in": "timed region" if args.events == "all" else "last warm-up call"}}
        f_call, f_step, f_tab = call_flops(B, L)
        tables_on = bool(getattr(model, "frame_table", False)) and model._frame_tables().get("ft.T2") is not None
        f_exec = f_call - (f_tab if tables_on else 0.0)
        whole = {"flops_per_call": f_exec, "decoder_step_flops": f_step,
                 "achieved": round(f_exec / (ms_per_step * 1e-3) / 1e12, 1), "peak": peak, "unit": "TFLOP/s",
                 "frac": round(f_exec / (ms_per_step * 1e-3) / 1e12 / peak, 4),
                 "reference_formula": {"flops_per_call": f_call, "achieved": round(f_call / (ms_per_step * 1e-3) / 1e12, 1),
                                       "frac": round(f_call / (ms_per_step * 1e-3) / 1e12 / peak, 4),
                                       "note": "the FLOPs the REFERENCE spends on this call (SURVEY 8d formula) over the same wall time"},
                 "frame_table": tables_on,
                 "note": "EXECUTED matrix-core FLOPs of one autoregressive_generate call per GPU over its wall time (full AR mode = the "
                         "reference's (L-1) full recomputes; incl. LayerNorm / attention / casts in the time).  With frame_table the frame "
                         "convolution + in_linear (11 % of the reference's FLOPs) are a gather-sum over precomputed tables "
                         "(mage_table_conv): they leave the numerator, the call gets faster, the fraction falls"
                 } if args.ar_mode == "full" else None
        tstep = None
        if args.ar_mode == "full" and prof.get("decoder_step", {}).get("calls"):
            ds = prof["decoder_step"]
            f_dec = f_step - (B * (L - 1) * 256 * 2 * 512 * 512 if tables_on else 0)       # in_linear leaves with the table sum
            t_dec = ds["ms"] / ds["calls"]
            tstep = {"ms": round(t_dec, 3), "calls": ds["calls"] // args.steps, "flops": f_dec, "achieved": round(f_dec / (t_dec * 1e-3) / 1e12, 1),
                     "peak": peak, "unit": "TFLOP/s", "frac": round(f_dec / (t_dec * 1e-3) / 1e12 / peak, 4),
                     "note": "north_star's 'transformer step': one FlatAxialDecoder pass (frame slots via the table sum, context_linear, 6 axial "
                             "blocks incl. LayerNorm / attention, head) over all L slots = one of the L-1 recomputes of the reference loop; HIP events "
                             "around each pass inside the timed region; executed FLOPs (SURVEY 8d F_step, minus in_linear when it is folded into "
                             "the table)"}
        wl_name = ("cfg2: Single Moving MNIST" if args.workload == "cfg2" else "cfg3: Double Moving MNIST (two digits, captions 16/18/20 tokens padded to 20)")
        res = {
            "metric": "generated frames/sec (64x64, 16-frame clips)", "value": round(value, 2), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": f"{wl_name} 64x64, {L} frames, batch={B}/GPU, MNIST f4 VQ-VAE + MAGE "
                                   f"(d=512, 6 axial blocks), AR loop: {'reference full recompute per iteration' if args.ar_mode == 'full' else 'incremental (temporal KV cache)'}, random-init weights",
                       "global_batch": world * B, "frames": L, "parallelism": f"clip-sharded x{world} (no data-path collective)",
                       "ranks_seen": seen, "ar_mode": model.ar_mode, "streams_per_gpu": args.streams,
                       "frame_table": bool(getattr(model, "frame_table", False)),
                       "residual_stream": ("bf16 (x kept in bf16 between the blocks; LayerNorm sums from the fp32 values before rounding; "
                                           "MAGE_STREAM_FP32=1 restores the fp32 stream + bf16 copy)"
                                           if args.precision == "bf16" and model.generate_model._stream_bf16() else "fp32"),
                       "graph_replay": replayed,
                       "frame_count_convention": "B*L frames per call: the output clip [B,L,C,H,W] incl. the passed-through first frame "
                                                 "(SURVEY 8d, reference mage_model.py:691); generated-only = value * (L-1)/L",
                       "generated_only_value": round(value * (L - 1) / L, 2)},
            "roofline": roofline,
            "whole_call": whole,
            "transformer_step": tstep,
            "roofline_decode": decode,
            "parity_mode": parity,
            "kernel_time_ms_per_step": ({k: round(v["ms"] / args.steps, 3) for k, v in sorted(prof.items())} if args.events == "all"
                                        else {k: round(v["ms"], 3) for k, v in sorted(warm_prof.items())}),
            "kernel_time_measured_in": "timed region" if args.events == "all" else "last warm-up call (every launch bracketed)",
            "other_ar_mode": other,
            "train_step": train,
            "latency_b1": lat,
            "cfg4": cfg4,
            "f16_mode": f16m,
        }
        if replayed:
            res["config"]["graph_replay_note"] = ("the timed calls replay ONE captured HIP graph of the whole autoregressive_generate call "
                                                  "(same kernels, same order, bit-identical results; tests/test_gpu_parity.py)")
        tick("cfg4_and_latency_b1")
        if cpu_sd is not None:
            res["cpu_baseline"], oracle_tok, oracle_margin = cpu_baseline(cpu_sd, L, args.cpu_clips)
            tick("cpu_baseline")
            # the same clips through the HIP path: do the GPU token sequences equal the CPU oracle's (= the reference's algorithm, pinned
            # by the goldens)?  north_star: "reference-matching VQ token sequences on Single Moving MNIST"
            try:
                cb = {k: v.to(dev) for k, v in synth.synth_batch_mnist(args.cpu_clips, L, seed=100).items()}
                agree = {}
                saved = (model.precision, model.ar_mode)
                model.ar_mode = "full"
                for prec in ("f16x3", "fp32", "f16", "bf16"):
                    model.set_precision(prec)
                    model.autoregressive_generate(cb)
                    got = model.last_tokens.cpu()
                    eq = got == oracle_tok
                    bad = ~eq
                    agree[prec] = {"all_positions": round(eq.float().mean().item(), 5), "clips_identical": round(eq.flatten(1).all(1).float().mean().item(), 5),
                                   "mismatches_where_oracle_margin_above_2e-5": int((bad & (oracle_margin > 2e-5)).sum())}
                model.set_precision(saved[0])
                model.ar_mode = saved[1]
                res["cpu_baseline"]["gpu_tokens_vs_oracle"] = dict(agree, clips=args.cpu_clips, positions=int(oracle_tok.numel()),
                                                                   oracle_min_top2_margin=float(oracle_margin.min()),
                                                                   note="free-running AR token sequences of the HIP path against the CPU oracle's on the "
                                                                        "baseline sample's clips (same weights, same inputs)")
            except Exception as e:
                res["cpu_baseline"]["gpu_tokens_vs_oracle"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            tick("gpu_tokens_vs_oracle")
            if args.trained_steps > 0 and world == 1 and args.workload == "cfg2":
                try:
                    res["cpu_baseline"]["gpu_tokens_vs_oracle_trained_weights"] = trained_token_agreement(
                        dev, L, args.trained_steps, 64, args.trained_clips, res["cpu_baseline"]["cores"])
                except Exception as e:
                    res["cpu_baseline"]["gpu_tokens_vs_oracle_trained_weights"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        tick("trained_weights_token_leg")
        res["bench_sections_s"] = dict(_t["sec"], note="wall seconds of this run per section (model builds, warm-ups and CPU work included)")
        # the headline secondary numbers once more as flat scalars (tools that keep only top-level scalars of this line still see them)
        res["parity_mode_frames_per_s"] = parity["value"] if parity else None
        res["parity_mode_dtype"] = parity["dtype"] if parity else None
        res["incremental_mode_frames_per_s"] = (other["value"] if other and other["ar_mode"] == "incremental" else
                                                (round(value, 2) if args.ar_mode == "incremental" else None))
        gto = res.get("cpu_baseline", {}).get("gpu_tokens_vs_oracle", {}) if cpu_sd is not None else {}
        res["parity_mode_tokens_equal_cpu_oracle"] = (gto.get("f16x3", {}).get("all_positions") == 1.0) if "f16x3" in gto else None
        gtt = res.get("cpu_baseline", {}).get("gpu_tokens_vs_oracle_trained_weights", {}) if cpu_sd is not None else {}
        res["bf16_trained_weights_token_agreement"] = gtt.get("bf16", {}).get("all_positions") if "bf16" in gtt else None
        res["bf16_trained_weights_clips_identical"] = gtt.get("bf16", {}).get("clips_identical") if "bf16" in gtt else None
        res["f16_mode_frames_per_s"] = f16m.get("value") if f16m else None
        res["f16_trained_weights_token_agreement"] = gtt.get("f16", {}).get("all_positions") if "f16" in gtt else None
        res["f16_trained_weights_clips_identical"] = gtt.get("f16", {}).get("clips_identical") if "f16" in gtt else None
        res["f16_trained_weights_teacher_forced_token_agreement"] = ((gtt.get("f16", {}).get("teacher_forced") or {}).get("token_agreement")
                                                                     if "f16" in gtt else None)
        res["cfg4_bf16_incremental_ms_per_call"] = ((cfg4 or {}).get("bf16", {}).get("incremental", {}).get("ms_per_call")
                                                    if isinstance(cfg4, dict) and "bf16" in cfg4 else None)
        print(json.dumps(without_notes(res)))
    if world > 1:
        D.barrier()
        torch.distributed.destroy_process_group()


def _cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sd, L, clips):
    """The CPU oracle (validated against the reference's golden vectors) timed on this box's host cores on a
    bounded sample of the same workload: `clips` clips of the cfg shape through the reference's full AR loop, with the
    thread count chosen by calibration, and one clip on ONE thread."""
    from mage_amd.utils import synth
    from oracle import mage_oracle as O
    batch = synth.synth_batch_mnist(clips, L, seed=100)
    # torch's intra-op pool oversubscribes badly on a 256-thread host (measured: 128 threads 4x slower than 16):
    # calibrate the thread count on one decoder pass of the actual shape, then time the whole generate call.
    ma = torch.zeros(clips, 16, 16, 512)
    imgs = torch.zeros(clips, L - 1, 16, 16, 512)
    best = (float("inf"), 1)
    ncpu = os.cpu_count() or 1
    with torch.no_grad():
        for th in (8, 16, 32, 64, 128):
            if th > ncpu:
                break
            torch.set_num_threads(th)
            O.flat_axial_decoder(sd, "generate_model.", ma, imgs)
            t0 = time.perf_counter()
            O.flat_axial_decoder(sd, "generate_model.", ma, imgs)
            t_th = time.perf_counter() - t0
            best = min(best, (t_th, th))
            if t_th > 1.5 * best[0]:                    # past the optimum (oversubscription only gets worse): stop calibrating
                break
        torch.set_num_threads(best[1])
        t0 = time.perf_counter()
        _, o_tok, _, o_trace = O.mage_generate(sd, batch, L, return_trace=True)
        dt = time.perf_counter() - t0
        # SURVEY 8d asks for "all physical cores": one decoder pass of the same shape on every physical core (host threads / 2 with SMT),
        # scaled by the calibrated run's (whole call / one decoder pass) ratio -- the figure beside the calibrated one, labelled as such
        phys = max(1, ncpu // 2)
        all_cores = None
        if phys > best[1]:
            torch.set_num_threads(phys)
            O.flat_axial_decoder(sd, "generate_model.", ma, imgs)
            t1 = time.perf_counter()
            O.flat_axial_decoder(sd, "generate_model.", ma, imgs)
            t_pass_phys = time.perf_counter() - t1
            torch.set_num_threads(best[1])
            all_cores = {"threads": phys, "decoder_pass_s": round(t_pass_phys, 3), "decoder_pass_s_at_calibrated_threads": round(best[0], 3),
                         "value_estimated": round(clips * L / (dt * t_pass_phys / best[0]), 3), "unit": "frames/s",
                         "note": "one decoder pass timed on all physical cores; frames/s = the calibrated run's scaled by the pass-time ratio "
                                 "(torch's intra-op pool oversubscribes: more threads are slower on this host)"}
        top2 = o_trace.topk(2, dim=-1)[0]
        o_margin = (top2[..., 0] - top2[..., 1]).abs()
        # one thread, one clip: first a SHORT clip (6 frames); if that predicts < 40 s for the full clip length (the loop's
        # cost grows ~L^2), the full-length clip is timed too and reported instead.  The sample is stated, never extrapolated.
        torch.set_num_threads(1)

        def one_thread(L1):
            sd1 = dict(sd)
            sd1["generate_model.T_positional_embedding"] = sd["generate_model.T_positional_embedding"][:L1].clone()
            b1 = synth.synth_batch_mnist(1, L1, seed=100)
            t0 = time.perf_counter()
            O.mage_generate(sd1, b1, L1)
            return time.perf_counter() - t0
        L1 = min(L, 6)
        dt1 = one_thread(L1)
        if L1 < L and dt1 * (L * (L - 1)) / (L1 * (L1 - 1)) < 40.0:
            L1 = L
            dt1 = one_thread(L1)
        torch.set_num_threads(best[1])
    return ({"value": round(clips * L / dt, 3), "unit": "frames/s", "cores": best[1], "kind": "port", "cpu": _cpu_model_name(),
            "host_threads": ncpu, "all_physical_cores": all_cores,
            "sample": f"{clips} clips x {L} frames (same model, fp32, oracle/mage_oracle.py mage_generate = the reference's "
                      f"full-recompute AR loop, torch {torch.__version__} CPU ops, {best[1]} of {ncpu} host threads "
                      f"chosen by calibration), {dt:.1f} s",
            "one_thread": {"value": round(L1 / dt1, 3), "unit": "frames/s", "cores": 1,
                           "sample": f"1 clip x {L1} frames on 1 thread (same model and loop" +
                                     ("" if L1 == L else "; shorter clip so that the sample stays bounded: the loop's cost grows ~L^2") +
                                     f"), {dt1:.1f} s"}}, o_tok, o_margin)


if __name__ == "__main__":
    main()
