#!/usr/bin/env python
"""The launch plan of the training path -- mage_train.train_forward / train_backward (with mage_train_prior behind them) and vqvae_train's
vq_train_* / vq8_train_* pairs: every call they make into mage_amd.ops, in order, with its arguments and with which buffer goes where --
recorded on CPU tensors, no GPU and no library.  tests/golden/train_plan.json keeps it per case (tests/test_train_plan_cpu.py compares); a
refactor of the orchestration in mage_train.py, mage_train_prior.py and vqvae_train.py leaves the file byte-identical.

    python tools/gen_train_plan.py --tree DIR [--out FILE]      # DIR: the checkout whose mage_amd is recorded (default: this one)

The fixture is generated from the PARENT of the commit that is being checked (git worktree add DIR <parent>), never from the code under test.

What is recorded.  ops._dev answers a library whose every entry point returns 0, so the real ops functions run: they make their assertions and
allocate their own outputs; every public function of ops is wrapped by a recorder, nested calls (gemm_tn's sum_partials) included.  Each call
is bound to the function's signature with the defaults applied and normalised as tools/gen_decoder_plan.py's Recorder.norm does (a tensor: dtype,
shape, strides, storage offset, the ordinal of its storage's first appearance within the case; every tensor is held until the case ends).
mage_model._need_gpu and VectorQuantizedVAE._check_input are no-ops, torch.cuda.get_device_properties answers 256 CUs, and PIDControl.pid
answers a constant beta (MAGE+'s controller takes exp() of the KL value, which here is uninitialised memory).  The passes are driven
directly, under torch.no_grad(), with torch.manual_seed set per case (_Run draws its dropout seed from the torch generator).  Values are
uninitialised memory: nothing in the orchestration branches on them.  Every case runs once unrecorded first: the weight copies that are built
on first use are not part of the plan.

The cases (specs()) are the smallest shapes at which a route can still differ; MAGE models have 3 decoder layers:
  a  mnist, width 64, vq_dim 32, K 64, B = 2, L = 4 in fp32 eval, fp32 train (dropout on), bf16 eval and bf16 train: _res_linear's three forms,
     the dual c_fc epilogue, the QUICKGELU_GRAD epilogue, _emit_next, the f16x3 encoder products;
  b  mnist, width 256, B = 4, L = 4 (4096 rows), bf16 train: the ops.gemm_tn route of _wgrad, the padded-taps frame convolution both ways;
  c  b under train_wgrad_transpose=True and under train_taps=False; a in bf16 train under train_emit=False, train_dual=False,
     train_f32_branch=True and train_enc_split=False, one at a time;
  d  cater (randomness branch, f8 first stage), width 64, bf16 train and fp32 eval (auto_beta is off there: the pass refuses a batch without
     'speed', so only with it);
  e  MAGE+ (magep_model_config), width 64, bf16 train and fp32 eval, with and without batch['speed']: the MSE head, the GroupNorm head, emb_lin,
     ln_q / ln_kv;
  f  the given-token heads on a in bf16 eval: PolicyHead plain and with reference, given and ratio_div together, PreferenceHead with and without
     given, DistillHead, LogitsHead (forward only); on d, PolicyHead with batch['video_noise'] (modulate_forward / modulate_backward without dz);
  g  VQ-VAE training at dim 32, K 64, 32 x 32 images, B = 2: the f4 stack with 1 and with 3 input channels, the f8 stack with 3.
mage_setup() / vq_setup() are also what tools/train_pass_dump.py runs for real on the GPU."""
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
sys.path.insert(0, ROOT)
from tools import gen_decoder_plan as gen  # noqa: E402

TRAIN_MODULES = ("mage_train.py", "mage_train_prior.py", "vqvae_train.py")
CONFIG_DEFAULTS = dict(train_wgrad_transpose=False, train_emit=True, train_dual=True, train_taps=True, train_f32_branch=False,
                       train_enc_split=True)


def load(tree=ROOT):
    """The modules of the checkout at `tree`: a namespace of mm (mage_model), ops, config, synth, util, mt (mage_train), vt (vqvae_train), vm."""
    mm, ops, config = gen.load(tree)
    imp = importlib.import_module
    return types.SimpleNamespace(mm=mm, ops=ops, config=config, synth=imp("mage_amd.utils.synth"), util=imp("mage_amd.utils.util"),
                                 mt=imp("mage_amd.modules.mage_train"), vt=imp("mage_amd.modules.vqvae_train"),
                                 vm=imp("mage_amd.modules.vqvae_model"))


def specs():
    """name -> what mage_setup() / vq_setup() take, in the order of the module docstring."""
    out = {}

    def mage(name, family, width, B, prec, train, cfg=None, speed=True, head=None):
        out[name] = dict(kind="mage", family=family, width=width, B=B, L=4, prec=prec, train=train, cfg=cfg or {}, speed=speed, head=head)

    for prec in ("fp32", "bf16"):
        for train in (False, True):
            mage(f"a-{prec}-{'train' if train else 'eval'}", "mnist", 64, 2, prec, train)
    mage("b-bf16-train", "mnist", 256, 4, "bf16", True)
    mage("c-b-wgrad_transpose", "mnist", 256, 4, "bf16", True, cfg=dict(train_wgrad_transpose=True))
    mage("c-b-no_taps", "mnist", 256, 4, "bf16", True, cfg=dict(train_taps=False))
    for key, val in (("train_emit", False), ("train_dual", False), ("train_f32_branch", True), ("train_enc_split", False)):
        mage(f"c-a-{key}={val}", "mnist", 64, 2, "bf16", True, cfg={key: val})
    for family, tag in (("cater", "d"), ("magep", "e")):
        mage(f"{tag}-bf16-train", family, 64, 2, "bf16", True)
        mage(f"{tag}-fp32-eval", family, 64, 2, "fp32", False)
    mage("e-bf16-train-nospeed", "magep", 64, 2, "bf16", True, speed=False)
    mage("e-fp32-eval-nospeed", "magep", 64, 2, "fp32", False, speed=False)
    for head in ("policy", "policy-all", "preference", "preference-given", "distill", "logits"):
        mage(f"f-{head}", "mnist", 64, 2, "bf16", False, head=head)
    mage("f-d-policy-noise", "cater", 64, 2, "bf16", False, head="policy-noise")
    for name, cin, down in (("g-f4-1ch", 1, 4), ("g-f4-3ch", 3, 4), ("g-f8-3ch", 3, 8)):
        out[name] = dict(kind="vq", cin=cin, down=down)
    return out


_MODELS = {}


def mage_setup(m, spec, dev="cpu"):
    """(model in the case's precision and mode, batch) on seeded synthetic weights and inputs; one model per family, width and device."""
    family, width, B, L = spec["family"], spec["width"], spec["B"], spec["L"]
    key = (family, width, str(dev))
    if key not in _MODELS:
        small = dict(frames_length=L, width=width, layers=3)
        cfg = m.synth.magep_model_config(**small) if family == "magep" else \
            getattr(m.synth, family + "_model_config")(vq_dim=32, K=64, **small)
        model = m.util.instantiate_from_config(cfg)
        m.synth.fill_state_dict(model, 31, d_model=width, n_layers=3)
        _MODELS[key] = model.to(dev)
    model = _MODELS[key].set_precision(spec["prec"]).train(spec["train"])
    if family == "mnist":
        batch = m.synth.synth_batch_mnist(B, L, seed=41)
    else:
        batch = m.synth.synth_batch_cater(B, L, seed=41, **({"vocab": 50} if family == "magep" else {}))
    if not spec["speed"]:
        del batch["speed"]
    return model, {k: v.to(dev) for k, v in batch.items()}


def make_head(m, model, spec, batch, dev="cpu"):
    """The loss head of a case f (None: the model's own); 'policy-noise' also puts the recorded noise into the batch."""
    kind = spec["head"]
    if kind is None:
        return None
    B, L, R, K = spec["B"], spec["L"], model.image_resolution, model.codebook_size
    rows, g = B * (L - 1) * R * R, torch.Generator().manual_seed(43)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)                                   # noqa: E731
    tokens = torch.randint(0, K, (B, L - 1, R, R), generator=g).to(dev)
    scalars = dict(temperature=1.0, top_k=0, top_p=1.0, clip_lo=0.2, clip_hi=0.2, entropy_coef=0.01)
    if kind in ("policy", "policy-noise"):
        if kind == "policy-noise":
            batch["video_noise"] = rnd(B, 64, R, R)
        return m.mt.PolicyHead(tokens, advantage=rnd(B), behaviour=None, **scalars)
    if kind == "policy-all":
        return m.mt.PolicyHead(tokens, advantage=rnd(B * (L - 1)), behaviour=-rnd(rows).abs(), reference=-rnd(rows).abs(), kl_coef=0.1,
                               given=(torch.rand(rows, generator=g) < 0.25).to(dev), ratio_div=R * R, **scalars)
    if kind in ("preference", "preference-given"):
        given = (torch.rand(rows, generator=g) < 0.25).to(dev) if kind == "preference-given" else None
        return m.mt.PreferenceHead(tokens, pairs=torch.tensor([[0, 1]]).to(dev), reference=rnd(B), beta=0.1, label_smoothing=0.0, mode=0,
                                   given=given)
    if kind == "distill":
        return m.mt.DistillHead(tokens, teacher=rnd(rows, K), temperature=1.0, mode=0)
    assert kind == "logits", kind
    return m.mt.LogitsHead(tokens)


def vq_setup(m, spec, dev="cpu"):
    """(VectorQuantizedVAE in training mode, images [2, cin, 32, 32])."""
    key = ("vq", spec["cin"], spec["down"], str(dev))
    if key not in _MODELS:
        vq = m.vm.VectorQuantizedVAE(spec["cin"], spec["down"], 32, 64)
        m.synth.fill_state_dict(vq, 23)
        _MODELS[key] = vq.to(dev)
    x = torch.rand(2, spec["cin"], 32, 32, generator=torch.Generator().manual_seed(23)) * 2 - 1
    return _MODELS[key].train(), x.to(dev)


def run_case(m, spec):
    """One case through its forward and backward pass, called directly."""
    torch.manual_seed(47)
    if spec["kind"] == "vq":
        vq, x = vq_setup(m, spec)
        fwd, bwd = (m.vt.vq_train_forward, m.vt.vq_train_backward) if spec["down"] == 4 else (m.vt.vq8_train_forward, m.vt.vq8_train_backward)
        x_tilde, z_e, zq, tape = fwd(vq, x)
        bwd(vq, tape, torch.ones_like(x_tilde), torch.ones_like(z_e), torch.ones_like(zq))
        return
    model, batch = mage_setup(m, spec)
    head = make_head(m, model, spec, batch)
    with m.config.override(**dict(CONFIG_DEFAULTS, **spec["cfg"])):
        loss, tape = m.mt.train_forward(model, batch, head)
        if spec["head"] != "logits":
            m.mt.train_backward(model, tape, torch.ones(()))


class _NullLibrary:
    """libmage_hip.so's stand-in: every entry point returns 0 (success) and launches nothing."""

    def __getattr__(self, name):
        return lambda *args: 0


class TrainRecorder(gen.Recorder):
    """Every public function of one checkout's ops wrapped by a recorder (install()); `calls` of the case since begin()."""

    def __init__(self, m):
        self.m, self.on = m, False
        self.names = sorted(n for n, f in vars(m.ops).items() if inspect.isfunction(f) and f.__module__ == m.ops.__name__ and n[0] != "_")
        self.begin()

    def begin(self):
        super().begin()
        self.mine = []

    def wrap(self, name, real):
        sig = inspect.signature(real)

        def call(*a, **kw):
            if self.on:
                b = sig.bind(*a, **kw)
                b.apply_defaults()
                f = sys._getframe(1)
                if f.f_code.co_name == "_conv":                     # VectorQuantizedVAE._conv: the call is its caller's
                    f = f.f_back
                self.mine.append(os.path.basename(f.f_code.co_filename) in TRAIN_MODULES)
                self.calls.append([name, {k: self.norm(v) for k, v in b.arguments.items()}])
            return real(*a, **kw)
        return call

    @contextlib.contextmanager
    def install(self):
        m, null = self.m, _NullLibrary()
        saved = [(m.ops, n, getattr(m.ops, n)) for n in self.names + ["_dev"]]
        saved += [(m.mm, "_need_gpu", m.mm._need_gpu), (m.vm.VectorQuantizedVAE, "_check_input", m.vm.VectorQuantizedVAE._check_input),
                  (torch.cuda, "get_device_properties", torch.cuda.get_device_properties), (m.mm.PIDControl, "pid", m.mm.PIDControl.pid)]
        try:
            for n in self.names:
                setattr(m.ops, n, self.wrap(n, getattr(m.ops, n)))
            m.ops._dev = lambda t: (null, 0)
            m.mm._need_gpu = lambda t, who: None
            m.vm.VectorQuantizedVAE._check_input = lambda vq, x: None
            m.mm.PIDControl.pid = lambda pid, exp_kl, kl, **kw: (0.5, 0.0)
            torch.cuda.get_device_properties = lambda device=None: types.SimpleNamespace(multi_processor_count=256)
            yield self
        finally:
            for o, n, v in saved:
                setattr(o, n, v)

    def case(self, fn):
        """fn once unrecorded (weight copies built on first use), then recorded: {ops, sha256} and the full calls."""
        self.on = False
        fn()
        self.begin()
        self.on = True
        fn()
        self.on = False
        lines = [json.dumps(c, sort_keys=True) for c in self.calls]
        own = [i for i, mine in enumerate(self.mine) if mine]
        entry = dict(ops=[f"{self.calls[i][0]}:{hashlib.sha256(lines[i].encode()).hexdigest()[:8]}" for i in own], n_calls=len(lines),
                     sha256=hashlib.sha256("\n".join(lines).encode()).hexdigest())
        calls = [self.calls[i] for i in own]
        self.begin()
        return entry, calls


def plan(m):
    """({case: {ops: ['name:digest of the call', ...], sha256 of the whole trace}}, {case: the full calls})."""
    rec, out, full = TrainRecorder(m), {}, {}
    with rec.install(), torch.no_grad():
        for name, spec in specs().items():
            out[name], full[name] = rec.case(lambda: run_case(m, spec))
    return out, full


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_plan.json"))
    args = ap.parse_args()
    p, _ = plan(load(args.tree))
    with open(args.out, "w") as f:
        f.write(gen.dumps(p))
    print(f"{len(p)} cases, {sum(len(c['ops']) for c in p.values())} calls from {os.path.abspath(args.tree)} -> {args.out}")
