#!/usr/bin/env python
"""The launch plan of FlatAxialDecoder, MAEncoder and TransformerTextEncoder: every call they make into mage_amd.ops, in order, with its
arguments and with which buffer goes where -- recorded on CPU tensors, no GPU and no library.  tests/golden/decoder_plan.json keeps it per case
(tests/test_decoder_plan_cpu.py compares); a refactor of the orchestration in mage_model.py leaves the file byte-identical.

    python tools/gen_decoder_plan.py --tree DIR [--out FILE]      # DIR: the checkout whose mage_amd is recorded (default: this one)

The fixture is generated from the PARENT of the commit that is being checked (git worktree add DIR <parent>), never from the code under test.

What is recorded.  ops.gemm, attention, layernorm, row_stats, ln_stats, table_conv, groupnorm_silu, gemm_attn_fused_qkv, mlp_fused, split (and,
for the text encoder, embedding, row_affine, caption_mask) are replaced by recorders that return their output argument.  Each call is bound to
the real function's signature with the defaults applied, so spelling a default out is no difference.  A tensor is recorded as dtype, shape,
strides, storage offset and the ordinal of its storage's first appearance within the case; every tensor is held until the case ends, so no
address is reused.  ops.gemm_is_small answers a constant per case, torch.cuda.get_device_properties answers 256 CUs.  Beside the calls, `routes`
lists what _fold, _stream_bf16, _stats_inline, _qkv_fuse, _mlp_fuse and _attn_split answered, in the order the passes asked.  Every case runs once
unrecorded first: the weight copies that are built on first use (split pieces, f16) are not part of the plan.

The cases (decoder_specs, encoder cases in plan()) are the smallest shapes at which a route can still differ:
  a  C = 128, 8 x 8 frames, B = 1, L = 4: no LayerNorm fold (C % 256), the split embed without the padded-taps form;
  b  C = 512, 16 x 16 frames, B = 2, L = 3, qkv_fuse_tiles = mlp_fuse_tiles = 0: the fold with statistics rows, both fused launches in the 16-bit
     full loop, the pair in the incremental loop, the padded-taps embed in the split modes;
  c  b at the default thresholds: the pair everywhere;      d  b with B = 1 and gemm_is_small true: inline statistics;
  e  b with stream_bf16 = False (bf16, f16) and under ln_fold=False (bf16);      f  b in f16x3 under attn_split=False;
  g  b with use_cids=False, full loop only;      h  b with a first _inc_step of nf = 2;      i  b in bf16 with FrameTokens;
  j  MAEncoder._run at d_model 64 and 128, split_kind 0 / F16X3, mage_plus off / on, both row orders;
  k  TransformerTextEncoder.forward at width 64, split_kind 0 / F16X3.
a .. d run in all five precisions; every decoder case runs through _run and through an _inc_begin + _inc_step loop unless it says otherwise.
drive() is also what tools/decoder_pass_dump.py runs for real on the GPU."""
import argparse
import contextlib
import hashlib
import importlib
import inspect
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("fp32", "bf16", "f16", "bf16x3", "f16x3")
RECORDED = ("gemm", "attention", "layernorm", "row_stats", "ln_stats", "table_conv", "groupnorm_silu", "gemm_attn_fused_qkv", "mlp_fused",
            "split", "embedding", "row_affine", "caption_mask")
OUTPUT_ARG = dict(gemm="y", attention="out", layernorm="y", row_stats="stats", ln_stats="stats", table_conv="y", groupnorm_silu="y",
                  gemm_attn_fused_qkv="y", mlp_fused="y", embedding="out", row_affine="x")
ROUTES = ("_fold", "_stream_bf16", "_stats_inline", "_qkv_fuse", "_mlp_fuse", "_attn_split")
CONFIG_DEFAULTS = dict(ln_fold=True, stream_16bit=True, qk_fuse=True, mlp_fuse=True, attn_split=True)


def load(tree=ROOT):
    """(mage_model, ops, config) of the checkout at `tree`."""
    tree = os.path.abspath(tree)
    assert "mage_amd" not in sys.modules or os.path.abspath(sys.modules["mage_amd"].__file__).startswith(tree + os.sep), \
        "another checkout's mage_amd is already imported: one tree per process"
    if tree not in sys.path:
        sys.path.insert(0, tree)
    mm = importlib.import_module("mage_amd.modules.mage_model")
    return mm, importlib.import_module("mage_amd.ops"), importlib.import_module("mage_amd.config")


def decoder_specs():
    """Cases a .. i: name -> what drive() takes."""
    specs = {}
    big = dict(C=512, R=16, B=2, L=3, tiles=0)

    def add(name, prec, **kw):
        specs[f"{name}-{prec}"] = dict(dict(prec=prec, tiles=None, small=False, cfg={}, stream=True, use_cids=True, loops=("run", "inc"), nf0=1,
                                            tokens=False), **kw)

    for p in PRECS:
        add("a", p, C=128, R=8, B=1, L=4)
        add("b", p, **big)
        add("c", p, **dict(big, tiles=None))
        add("d", p, **dict(big, B=1), small=True)
    for p in ("bf16", "f16"):
        add("e-stream32", p, **big, stream=False)
    add("e-nofold", "bf16", **big, cfg=dict(ln_fold=False))
    add("f-attn32", "f16x3", **big, cfg=dict(attn_split=False))
    for p in ("fp32", "bf16", "f16x3"):
        add("g-latents", p, **big, use_cids=False, loops=("run",))
    for p in ("bf16", "f16x3"):
        add("h-prefill", p, **big, nf0=2, loops=("inc",))
    add("i-tokens", "bf16", **big, tokens=True)
    return specs


_DECODERS = {}


def _decoder(mm, spec, dev):
    """One decoder per geometry and device: the cases share its weights and its derived copies."""
    key = (spec["C"], spec["L"], spec["use_cids"], str(dev))
    if key not in _DECODERS:
        _DECODERS[key] = _new_decoder(mm, spec, dev)
    return _DECODERS[key]


def _new_decoder(mm, spec, dev):
    torch.manual_seed(7)
    dec = mm.FlatAxialDecoder(64, spec["C"], 64 if spec["use_cids"] else 4, frames_length=spec["L"], layers=3, context_channels=64,
                              use_cids=spec["use_cids"]).eval()
    with torch.no_grad():
        for p_ in dec.parameters():          # LayerNorm / GroupNorm gains and every bias off their 1 / 0; the zero-initialised MAGE+ head off zero
            if p_.dim() == 1 or not p_.any():
                p_.add_(0.1 * torch.randn(p_.shape))
    return dec.to(dev)


def drive(mm, ops, config, spec, loop, dev="cpu"):
    """One decoder case through one loop ('run': _run; 'inc': _inc_begin + _inc_step until the window is full) on seeded weights and inputs.
    Returns (the logits of every call, the temporal caches at the end)."""
    dt, sk = mm.PRECISIONS[spec["prec"]]
    dec = _decoder(mm, spec, dev)
    dec.compute_dtype, dec.split_kind, dec.stream_bf16 = dt, sk, spec["stream"]
    dec.qkv_fuse_tiles = dec.mlp_fuse_tiles = 8 if spec["tiles"] is None else spec["tiles"]      # (None: the default thresholds)
    B, R, L = spec["B"], spec["R"], spec["L"]
    hw = R * R
    g = torch.Generator().manual_seed(11)
    T2 = (0.1 * torch.randn(9, 32, spec["C"], generator=g)).to(dev).to(dt)
    P2 = (0.1 * torch.randn(hw, spec["C"], generator=g)).to(dev)

    def frames(n):
        """n frames per clip as the model hands them over: FrameTokens, split rows where the padded-taps embed takes them, else rows in dt."""
        if spec["tokens"]:
            return mm.FrameTokens(torch.randint(0, 32, (B * n, hw), generator=g).to(dev), T2, P2, R)
        x = torch.randn(B * n * hw, 64, generator=g).to(dev)
        if dec._split_on() and dec._taps_ok(B * n * hw):
            return ops.split(x, sk)
        return x.to(dt)

    motion = torch.randn(B * hw, 64, generator=g).to(dev).to(dt)
    outs, caches = [], {}
    with config.override(**dict(CONFIG_DEFAULTS, **spec["cfg"])):
        if loop == "run":
            outs.append(dec._run(motion, frames(L - 1), B=B, hh=R, ww=R))
        else:
            st = dec._inc_begin(B, R, R)
            outs.append(dec._inc_step(st, motion, frames(spec["nf0"]), nf=spec["nf0"]))
            while st["p"] < L:
                outs.append(dec._inc_step(st, None, frames(1)))
            caches = st["kv"]
    return outs, caches


class Recorder:
    """The ops of one checkout replaced by recorders (install()); `calls` and `routes` of the case since begin()."""

    def __init__(self, mm, ops):
        self.mm, self.ops, self.on, self.small = mm, ops, False, False
        self.sigs = {n: inspect.signature(getattr(ops, n)) for n in RECORDED}
        self.begin()

    def begin(self):
        self.calls, self.routes, self.keep, self.storages = [], [], [], {}

    def norm(self, v):
        if isinstance(v, torch.Tensor):
            self.keep.append(v)
            o = self.storages.setdefault(v.untyped_storage()._cdata, len(self.storages))
            return ["tensor", str(v.dtype), list(v.shape), list(v.stride()), v.storage_offset(), o]
        if isinstance(v, (list, tuple)):
            return [self.norm(x) for x in v]
        if isinstance(v, dict):
            return {k: self.norm(x) for k, x in sorted(v.items())}
        return v if v is None or isinstance(v, (bool, int, str)) else repr(v)

    def fake(self, name):
        ops, sig = self.ops, self.sigs[name]

        def call(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            if self.on:
                self.calls.append([name, {k: self.norm(v) for k, v in b.arguments.items()}])
            args = b.arguments
            if name == "split":
                x = args["x"]
                return args["out"] if args["out"] is not None else ops.split_empty(x.shape[0], x.shape[1], args["kind"], x.device)
            if name == "caption_mask":
                n, s = args["ids"].shape
                return torch.empty(n, dtype=torch.int32), torch.empty(n * s)
            return args[OUTPUT_ARG[name]]
        return call

    def route(self, name, real):
        def ask(dec, *a, **kw):
            r = real(dec, *a, **kw)
            if self.on:
                self.routes.append([name, bool(r)])
            return r
        return ask

    @contextlib.contextmanager
    def install(self):
        mm, ops, dec = self.mm, self.ops, self.mm.FlatAxialDecoder
        saved = [(ops, n, getattr(ops, n)) for n in RECORDED + ("gemm_is_small",)] + [(dec, n, getattr(dec, n)) for n in ROUTES]
        saved += [(mm, "_need_gpu", mm._need_gpu), (torch.cuda, "get_device_properties", torch.cuda.get_device_properties)]
        try:
            for n in RECORDED:
                setattr(ops, n, self.fake(n))
            for n in ROUTES:
                setattr(dec, n, self.route(n, getattr(dec, n)))
            ops.gemm_is_small = lambda a, M, N, K: self.small
            mm._need_gpu = lambda t, who: None
            torch.cuda.get_device_properties = lambda device=None: types.SimpleNamespace(multi_processor_count=256)
            yield self
        finally:
            for o, n, v in saved:
                setattr(o, n, v)

    def case(self, fn, small=False):
        """fn once unrecorded (weight copies built on first use), then recorded: {routes, ops, sha256} and the full calls."""
        self.small = small
        self.on = False
        fn()
        self.begin()
        self.on = True
        fn()
        self.on = False
        lines = [json.dumps(c, sort_keys=True) for c in self.calls]
        full = json.dumps(self.routes) + "\n" + "\n".join(lines)
        entry = dict(routes=self.routes, ops=[f"{c[0]}:{hashlib.sha256(l.encode()).hexdigest()[:8]}" for c, l in zip(self.calls, lines)],
                     sha256=hashlib.sha256(full.encode()).hexdigest())
        calls = self.calls
        self.begin()
        return entry, calls


def plan(mm, ops, config):
    """({case: {routes, ops: ['name:digest of the call', ...], sha256 of the whole trace}}, {case: the full calls})."""
    rec, out, full = Recorder(mm, ops), {}, {}

    def add(name, fn, small=False):
        out[name], full[name] = rec.case(fn, small)

    with rec.install(), torch.no_grad():
        for name, spec in decoder_specs().items():
            for loop in spec["loops"]:
                add(f"{name}/{loop}", lambda: drive(mm, ops, config, spec, loop), spec["small"])
        for Cc in (64, 128):
            for sk in (0, ops.F16X3):
                for plus in (False, True):
                    for seq_first in (False, True):
                        torch.manual_seed(3)
                        enc = mm.MAEncoder(2, Cc).eval()
                        enc.split_kind, enc.mage_plus = sk, plus
                        q, kv = torch.randn(2 * 4, Cc), torch.randn(2 * 6, Cc)
                        add(f"j-C{Cc}-sk{sk}-{'plus' if plus else 'plain'}-{'seq' if seq_first else 'batch'}_first",
                            lambda: enc._run(q, kv, B=2, nq=4, nk=6, seq_first=seq_first))
        for sk in (0, ops.F16X3):
            torch.manual_seed(5)
            enc = mm.TransformerTextEncoder(50, 64, 2, 64, context_length=8).eval()
            enc.split_kind = sk
            text = torch.randint(0, 50, (2, 8))
            add(f"k-sk{sk}", lambda: enc(text))
    return out, full


def dumps(p):
    return json.dumps(p, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decoder_plan.json"))
    args = ap.parse_args()
    p, _ = plan(*load(args.tree))
    with open(args.out, "w") as f:
        f.write(dumps(p))
    print(f"{len(p)} cases, {sum(len(c['ops']) for c in p.values())} calls from {os.path.abspath(args.tree)} -> {args.out}")
