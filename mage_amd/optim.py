"""Optimizer of the training path: Adam over flat fp32 arenas, sharded across the data-parallel ranks.

The reference trains with ``optim.Adam(model.parameters(), lr, betas=(0.9, 0.98), eps=1e-6)`` under
``DistributedDataParallel`` (main_mage.py:95,121,150-153): every rank all-reduces every gradient and then repeats the same
Adam step on all parameters.  On one MI355X node (xGMI is point-to-point: ring collectives are per-link bound, so fewer and
larger transfers win) the same update is done as

    reduce-scatter(flat gradient arena)  ->  Adam on this rank's 1/W shard  ->  all-gather(flat parameter arena)

over RCCL: the gradient crosses the links once (an all-reduce is a reduce-scatter plus an all-gather of the GRADIENT; here the
second half moves the updated PARAMETERS instead and the optimizer state and arithmetic are divided by W).  All parameters
live in one contiguous fp32 arena (``p.data`` are views into it), all gradients in another (``p.grad`` are views), so each
collective is ONE call on a 16-byte aligned buffer (148 MB at the MNIST config, 539 MB at caterv1) and the step is ONE
``mage_adam`` launch per shard.

``FlatAdam`` keeps ``torch.optim.Optimizer``'s surface (``param_groups[...]['lr']`` for the reference's
``adjust_learning_rate``, ``zero_grad``, ``step``, ``state_dict`` / ``load_state_dict`` for its checkpoints).

Four options make the step one that can be left alone; with all four at their defaults every launch is the one described above.
``skip_nonfinite=True`` skips a step whose (all-rank) gradient holds an inf or a NaN -- decided on the device from the sum of squares, never
read on the host; ``skipped_steps`` counts them.  ``weight_decay=`` is AdamW's decoupled decay on the parameters with ``ndim >= 2`` (minus
``no_decay``), which the arena then holds first.  ``ema_decay=`` keeps an exponential moving average of the parameters, sharded like the
moments; ``swap_ema()`` runs the model on it and ``ema_tensors()`` returns it.  Any of them (and ``max_grad_norm`` beside them) is served by
ONE ``mage_adam_guarded`` launch per shard.
"""
from __future__ import annotations

import contextlib
import math
from typing import Iterable, Optional

import torch
import torch.distributed as dist

from . import ops
from .modules import vqvae_model as _vq

__all__ = ["FlatAdam"]


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.98), eps: float = 1e-6,
                 process_group: Optional[dist.ProcessGroup] = None, shard: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 weight_decay: Optional[float] = None, no_decay: Optional[Iterable[torch.nn.Parameter]] = None,
                 ema_decay: Optional[float] = None, skip_nonfinite: bool = False):
        # The reference hands EVERY parameter to optim.Adam (main_mage.py:121: model.parameters(), the frozen first stage included -- its
        # parameters follow MAGE's three top-level nn.Parameters), so the indices of its checkpoint's 'state' and 'param_groups' count the
        # frozen ones too.  Keep that numbering: `all_params` is the caller's order, `index[i]` the position of trainable parameter i in it.
        all_params = list(params)
        if any(isinstance(p, dict) for p in all_params):
            raise ValueError("FlatAdam: one parameter group (an iterable of tensors), as the reference's optim.Adam call")
        plist = [p for p in all_params if p.requires_grad]
        if not plist:
            raise ValueError("FlatAdam: no trainable parameters")
        # max_grad_norm: clip the norm of the averaged gradient inside the step (torch.nn.utils.clip_grad_norm_'s rule, on the device);
        # it lives in param_groups[0] beside lr, so a schedule can change it.  None: no clipping, the plain mage_adam step.
        self._check_max_grad_norm(max_grad_norm)
        # weight_decay (AdamW's, decoupled), ema_decay and skip_nonfinite live there too.  Whether the arena is laid out for decay and whether
        # an EMA buffer exists is fixed here, at construction: the group entries can change the values later, not switch the two on.
        self._check_weight_decay(weight_decay, lr)
        self._check_ema_decay(ema_decay)
        if no_decay is not None and weight_decay is None:
            raise ValueError("FlatAdam: no_decay without weight_decay (pass weight_decay=0.0 to lay the arena out for a schedule that switches it on)")
        no_decay = list(no_decay) if no_decay is not None else []
        for q_ in no_decay:
            if not any(q_ is p for p in plist):
                raise ValueError("FlatAdam: every no_decay entry must be one of this optimizer's trainable parameters")
        super().__init__(all_params, dict(lr=lr, betas=tuple(betas), eps=eps, max_grad_norm=max_grad_norm, weight_decay=weight_decay,
                                          ema_decay=ema_decay, skip_nonfinite=bool(skip_nonfinite)))
        self.all_params = all_params
        self.index = [i for i, p in enumerate(all_params) if p.requires_grad]
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        # shard=None: shard whenever there is more than one rank; shard=True forces the reduce-scatter / all-gather path on any
        # initialised process group (a 1-rank group still goes through RCCL: used by the single-GPU test of the collective path)
        self.sharded = (self.world > 1) if shard is None else (bool(shard) and dist.is_initialized())
        dev = plist[0].device
        if any(p.device != dev or p.dtype != torch.float32 for p in plist):
            raise ValueError("FlatAdam: parameters must be fp32 tensors on one device")
        self.params = plist
        n = sum(p.numel() for p in plist)
        q = 4 * self.world                                       # every shard starts 16-byte aligned
        self.n, self.n_pad = n, (n + q - 1) // q * q
        self.flat_p = torch.zeros(self.n_pad, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(self.n_pad, device=dev, dtype=torch.float32)
        # The arena is FlatAdam's own: with weight_decay the decayed parameters (ndim >= 2, not in no_decay) come first, so that the kernel's
        # rule is "element i < n_decay" and a shard's is a clamp.  `offsets` stays per parameter in the caller's order (checkpoints address
        # parameters through it and never see the layout); without weight_decay the arena keeps the caller's order and n_decay is 0.
        self._decay_layout = weight_decay is not None
        decayed = [self._decay_layout and p.ndim >= 2 and not any(p is q_ for q_ in no_decay) for p in plist]
        order = [j for j, d_ in enumerate(decayed) if d_] + [j for j, d_ in enumerate(decayed) if not d_]
        self.n_decay = sum(plist[j].numel() for j, d_ in enumerate(decayed) if d_)
        self.offsets = [0] * len(plist)
        off = 0
        with torch.no_grad():
            for j in order:
                p = plist[j]
                k = p.numel()
                self.flat_p[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[off:off + k].view(p.shape)             # parameters become views into the arena
                p.grad = self.flat_g[off:off + k].view(p.shape)
                self.offsets[j] = off
                off += k
        self.shard_n = self.n_pad // self.world if self.sharded else self.n_pad
        self.shard_off = self.rank * self.shard_n if self.sharded else 0
        self.m = torch.zeros(self.shard_n, device=dev, dtype=torch.float32)
        self.v = torch.zeros(self.shard_n, device=dev, dtype=torch.float32)
        self.shard_g = torch.empty(self.shard_n, device=dev, dtype=torch.float32) if self.sharded else None
        self.steps = 0
        # fp32 [1] on the device after every clipped step: the norm of the averaged gradient before the clip; never read on the host here
        self.last_grad_norm: Optional[torch.Tensor] = None
        # int64 [1] on the device once skip_nonfinite is on: how many steps the kernel skipped; the library never reads it
        self.skipped_steps: Optional[torch.Tensor] = torch.zeros(1, device=dev, dtype=torch.int64) if skip_nonfinite else None
        self._consolidated = None                                # (steps, exp_avg, exp_avg_sq, ema) gathered by consolidate_state_dict
        self._swapped = False                                    # inside swap_ema(): flat_p holds the EMA
        if self.world > 1:
            # DistributedDataParallel broadcasts rank 0's parameters when it wraps a model (main_mage.py:95); a bare model + FlatAdam
            # gets the same guarantee here: replicas that were initialised differently start from rank 0's weights
            dist.broadcast(self.flat_p, src=dist.get_global_rank(self.pg, 0) if self.pg is not None else 0, group=self.pg)
            _vq.bump_weights_epoch()
        # fp32 [shard_n], sharded like m and v: the moving average starts from the parameters every rank now agrees on
        self.ema: Optional[torch.Tensor] = (self.flat_p[self.shard_off:self.shard_off + self.shard_n].clone() if ema_decay is not None else None)

    # ------------------------------------------------------------------ gradients
    def zero_grad(self, set_to_none: bool = True):
        """``set_to_none=True`` (torch.optim's default, what the reference's bare ``optimizer.zero_grad()`` gets, main_mage.py:150): drop the
        ``.grad`` views -- autograd then hands each gradient over by reference instead of launching one in-place add per parameter into a
        zeroed arena (149 launches per step at the MNIST config), and ``step`` gathers them into the arena with one multi-tensor copy.
        ``set_to_none=False``: zero the arena in one launch; ``.grad`` stays a view into it (autograd accumulates in place)."""
        if set_to_none:
            for p in self.params:
                p.grad = None
            return
        self.flat_g.zero_()
        for p, off in zip(self.params, self.offsets):
            view = self.flat_g[off:off + p.numel()].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                p.grad = view

    def _collect_grads(self):
        """Bring gradients that live outside the arena (set_to_none, or a .grad autograd REPLACED) back into it: one multi-tensor copy."""
        src, dst = [], []
        for p, off in zip(self.params, self.offsets):
            view = self.flat_g[off:off + p.numel()].view(p.shape)
            if p.grad is None:
                view.zero_()
            elif p.grad.data_ptr() != view.data_ptr():
                if p.grad.dtype == view.dtype and p.grad.device == view.device:
                    src.append(p.grad.detach())
                    dst.append(view)
                else:
                    view.copy_(p.grad)
            p.grad = view
        if src:
            torch._foreach_copy_(dst, src)

    # ------------------------------------------------------------------ the update
    def _adam(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale):
        """One fused launch over a flat shard (libmage_hip.so mage_adam).  No CPU path."""
        if not p.is_cuda:
            raise RuntimeError("FlatAdam runs on libmage_hip.so (mage_adam): the parameters must live on a ROCm GPU")
        ops.adam(p, g, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, step=step, grad_scale=grad_scale)

    @staticmethod
    def _check_max_grad_norm(c):
        if c is not None and not (isinstance(c, (int, float)) and not isinstance(c, bool) and 0 < c < 3.4e38):
            raise ValueError(f"FlatAdam: max_grad_norm must be None or a finite number > 0, got {c!r}")

    @staticmethod
    def _check_weight_decay(w, lr):
        if w is None:
            return
        if not (isinstance(w, (int, float)) and not isinstance(w, bool) and math.isfinite(w) and w >= 0 and lr * w < 1):
            raise ValueError(f"FlatAdam: weight_decay must be None or a finite number >= 0 with lr * weight_decay < 1, got {w!r} (lr {lr!r})")

    @staticmethod
    def _check_ema_decay(d):
        if d is not None and not (isinstance(d, (int, float)) and not isinstance(d, bool) and 0 < d < 1):
            raise ValueError(f"FlatAdam: ema_decay must be None or a number in (0, 1), got {d!r}")

    def _sumsq(self, g):
        """fp64 [1] on g's device: the sum of squares of a flat gradient (libmage_hip.so mage_sumsq).  No CPU path."""
        if not g.is_cuda:
            raise RuntimeError("FlatAdam runs on libmage_hip.so (mage_sumsq): the parameters must live on a ROCm GPU")
        return ops.sumsq(g)

    def _adam_clipped(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale, sumsq, max_norm, norm_out):
        """_adam with the gradient scaled by clip_grad_norm_'s rule from the device value sumsq (libmage_hip.so mage_adam_clipped)."""
        if not p.is_cuda:
            raise RuntimeError("FlatAdam runs on libmage_hip.so (mage_adam_clipped): the parameters must live on a ROCm GPU")
        ops.adam_clipped(p, g, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, step=step, grad_scale=grad_scale, sumsq=sumsq, max_norm=max_norm,
                         norm_out=norm_out)

    def _adam_guarded(self, p, g, m, v, ema, n_decay, lr, b1, b2, eps, step, grad_scale, decay_mul, ema_decay, sumsq, max_norm, skip, norm_out,
                      skipped):
        """_adam_clipped (max_norm 0: _adam) with the skip of a non-finite step, the decay of the first n_decay elements and the EMA
        (libmage_hip.so mage_adam_guarded).  No CPU path."""
        if not p.is_cuda:
            raise RuntimeError("FlatAdam runs on libmage_hip.so (mage_adam_guarded): the parameters must live on a ROCm GPU")
        ops.adam_guarded(p, g, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, step=step, grad_scale=grad_scale, ema=ema, ema_decay=ema_decay,
                         n_decay=n_decay, decay_mul=decay_mul, sumsq=sumsq, max_norm=max_norm, skip_nonfinite=skip, norm_out=norm_out,
                         skipped=skipped)

    def _update(self, p, g, m, v, all_reduce_sumsq: bool):
        """The Adam launch over one flat shard: plain, or -- with param_groups[0]['max_grad_norm'] -- the shard's sum of squares (summed over
        the ranks where each holds a different shard), then the clipped launch; with weight_decay, ema_decay or skip_nonfinite the sum of
        squares where the clip or the guard needs it (all-reduced: every rank takes the same skip decision), then the guarded launch.
        Everything stays on the device."""
        g0 = self.param_groups[0]
        lr, (b1, b2), eps, c = g0["lr"], g0["betas"], g0["eps"], g0.get("max_grad_norm")
        wd, d, skip = g0.get("weight_decay"), g0.get("ema_decay"), bool(g0.get("skip_nonfinite"))
        if wd is not None or d is not None or skip or self.ema is not None:
            return self._update_guarded(p, g, m, v, all_reduce_sumsq, lr, b1, b2, eps, c, wd, d, skip)
        if c is None:
            return self._adam(p, g, m, v, lr, b1, b2, eps, self.steps, 1.0 / self.world)
        self._check_max_grad_norm(c)
        ss = self._sumsq(g)
        if all_reduce_sumsq:
            dist.all_reduce(ss, op=dist.ReduceOp.SUM, group=self.pg)
        if self.last_grad_norm is None:
            self.last_grad_norm = torch.zeros(1, device=p.device, dtype=torch.float32)
        self._adam_clipped(p, g, m, v, lr, b1, b2, eps, self.steps, 1.0 / self.world, ss, float(c), self.last_grad_norm)

    def _update_guarded(self, p, g, m, v, all_reduce_sumsq, lr, b1, b2, eps, c, wd, d, skip):
        self._check_max_grad_norm(c)
        self._check_weight_decay(wd, lr)
        self._check_ema_decay(d)
        if wd is not None and not self._decay_layout:
            raise ValueError("FlatAdam: param_groups[0]['weight_decay'] was set on an optimizer constructed with weight_decay=None; the arena's "
                             "layout (decayed parameters first) is fixed at construction: construct with weight_decay=0.0 and schedule it")
        if (d is None) != (self.ema is None):
            raise ValueError("FlatAdam: param_groups[0]['ema_decay'] can change the decay, not switch the EMA on or off: the buffer exists "
                             "exactly when the optimizer was constructed with ema_decay")
        ss = None
        if c is not None or skip:
            ss = self._sumsq(g)
            if all_reduce_sumsq:
                dist.all_reduce(ss, op=dist.ReduceOp.SUM, group=self.pg)
            if self.last_grad_norm is None:
                self.last_grad_norm = torch.zeros(1, device=p.device, dtype=torch.float32)
        if skip and self.skipped_steps is None:
            self.skipped_steps = torch.zeros(1, device=p.device, dtype=torch.int64)
        # AdamW's p *= 1 - lr * weight_decay as one fp32 factor (0.0 is a number: a factor of exactly 1)
        decay_mul = 1.0 if wd is None else float(torch.tensor(1.0 - float(lr) * float(wd), dtype=torch.float64).float())
        n_decay = 0 if wd is None else min(max(self.n_decay - self.shard_off, 0), self.shard_n)
        self._adam_guarded(p, g, m, v, self.ema, n_decay, lr, b1, b2, eps, self.steps, 1.0 / self.world, decay_mul, 0.0 if d is None else float(d),
                           ss, 0.0 if c is None else float(c), skip, self.last_grad_norm if ss is not None else None,
                           self.skipped_steps if skip else None)

    @torch.no_grad()
    def step(self, closure=None):
        if self._swapped:
            raise RuntimeError("FlatAdam.step() inside swap_ema(): the arena holds the averaged weights, not the ones being trained")
        loss = closure() if closure is not None else None
        self._collect_grads()
        self.steps += 1
        if self.sharded:
            # gradient: summed over ranks, each rank keeps its shard (the mean's 1/W is folded into the Adam kernel)
            dist.reduce_scatter_tensor(self.shard_g, self.flat_g, op=dist.ReduceOp.SUM, group=self.pg)
            p_shard = self.flat_p[self.shard_off:self.shard_off + self.shard_n]
            self._update(p_shard, self.shard_g, self.m, self.v, all_reduce_sumsq=True)
            dist.all_gather_into_tensor(self.flat_p, p_shard.clone(), group=self.pg)
        else:
            if self.world > 1:                                   # replicated state: plain all-reduce of the arena
                dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM, group=self.pg)
            self._update(self.flat_p, self.flat_g, self.m, self.v, all_reduce_sumsq=False)   # (the arena is the whole summed gradient already)
        _vq.bump_weights_epoch()                                 # the kernels' derived weight copies are stale now
        return loss

    # ------------------------------------------------------------------ the averaged weights
    def _full_ema(self):
        """The whole EMA arena [n_pad]; COLLECTIVE when the state is sharded."""
        if self.ema is None:
            raise RuntimeError("FlatAdam: no EMA is kept (construct with ema_decay=)")
        if not self.sharded:
            return self.ema.clone()
        full = torch.empty(self.n_pad, device=self.ema.device, dtype=torch.float32)
        dist.all_gather_into_tensor(full, self.ema, group=self.pg)
        return full

    @contextlib.contextmanager
    def swap_ema(self):
        """``with opt.swap_ema(): video = model.autoregressive_generate(batch)`` -- the model runs on the averaged weights inside the block
        (the parameters are views into the arena, which holds the all-gathered EMA meanwhile) and on the raw ones again after it.  COLLECTIVE
        when the state is sharded (every rank enters).  step() inside the block raises."""
        if self._swapped:
            raise RuntimeError("FlatAdam.swap_ema(): already inside swap_ema()")
        with torch.no_grad():
            full = self._full_ema()
            stash = self.flat_p.clone()
            self.flat_p.copy_(full)
        self._swapped = True
        _vq.bump_weights_epoch()
        try:
            yield self
        finally:
            with torch.no_grad():
                self.flat_p.copy_(stash)
            self._swapped = False
            _vq.bump_weights_epoch()

    @torch.no_grad()
    def ema_tensors(self):
        """One detached clone of the averaged weights per trainable parameter, in the caller's order (what an averaged checkpoint saves).
        COLLECTIVE when the state is sharded."""
        full = self._full_ema()
        return [full[off:off + p.numel()].view(p.shape).clone() for p, off in zip(self.params, self.offsets)]

    # ------------------------------------------------------------------ checkpoints (main_mage.py:189-199)
    def consolidate_state_dict(self, to: int = 0):
        """COLLECTIVE (every rank calls it, like torch's ZeroRedundancyOptimizer.consolidate_state_dict): gather the sharded moments so that
        rank `to` can build the checkpoint.  The reference saves from inside its rank-0 branch (main_mage.py:186-193); a sharded optimizer
        cannot gather there without hanging the other ranks in RCCL, so the loop calls this on all ranks first:

            optimizer.consolidate_state_dict()          # all ranks
            if rank == 0: torch.save({... 'optimizer': optimizer.state_dict()}, path)

        A no-op when the state is not sharded (one rank, or shard=False)."""
        if not self.sharded or self.world == 1:
            return
        m = torch.empty(self.n_pad, device=self.m.device, dtype=torch.float32)
        v = torch.empty(self.n_pad, device=self.m.device, dtype=torch.float32)
        dist.all_gather_into_tensor(m, self.m, group=self.pg)
        dist.all_gather_into_tensor(v, self.v, group=self.pg)
        e = self._full_ema() if self.ema is not None else None
        self._consolidated = (self.steps, m[:self.n], v[:self.n], None if e is None else e[:self.n]) if self.rank == to else None

    def _full_moments(self):
        if not self.sharded or self.world == 1:
            return self.m[:self.n].clone(), self.v[:self.n].clone(), None if self.ema is None else self.ema[:self.n].clone()
        if self._consolidated is None or self._consolidated[0] != self.steps:
            raise RuntimeError("FlatAdam.state_dict(): the optimizer state is sharded over the ranks; call optimizer.consolidate_state_dict() on "
                               "EVERY rank first (a collective), then state_dict() on the rank that saves -- state_dict() itself is local")
        return self._consolidated[1:]

    def state_dict(self):
        """torch.optim.Adam's layout, numbered over ALL parameters the optimizer was given (frozen ones included, as the reference's
        optim.Adam(model.parameters()) numbers them): state[i] = {step, exp_avg, exp_avg_sq} for every TRAINABLE parameter i, and
        param_groups[0]['params'] = range(len(all parameters)) -- so the 'optimizer' entry of a checkpoint is interchangeable with the
        reference's (main_mage.py:121,189-199,210-228) and independent of the world size it was written with.  LOCAL: with sharded state
        call consolidate_state_dict() on every rank first.  With an EMA, state[i] also carries 'ema' (torch.optim.Adam.load_state_dict carries
        an unknown state key along), and param_groups[0] always carries weight_decay, ema_decay and skip_nonfinite."""
        m, v, ema = self._full_moments()
        state = {}
        for i, p, off in zip(self.index, self.params, self.offsets):
            k = p.numel()
            state[i] = {"step": torch.tensor(float(self.steps)), "exp_avg": m[off:off + k].view(p.shape).clone(),
                        "exp_avg_sq": v[off:off + k].view(p.shape).clone()}
            if ema is not None:
                state[i]["ema"] = ema[off:off + k].view(p.shape).clone()
        # 'flat_adam_numbering': an explicit marker of the index space; torch.optim.Adam ignores unknown group keys on load
        groups = [dict({k: v_ for k, v_ in g.items() if k != "params"}, params=list(range(len(self.all_params))), flat_adam_numbering="all")
                  for g in self.param_groups]
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Accepts torch.optim.Adam's per-parameter layout (written by this class at ANY world size, or by the reference's optim.Adam over
        model.parameters()): entries are matched by their index in the full parameter list (a checkpoint numbered over the TRAINABLE
        parameters only -- this class's layout before it counted frozen ones -- is recognised by its length and re-indexed); a parameter without an entry (one that never
        received a gradient, e.g. ln_q / ln_kv under find_unused_parameters=True) starts from zero moments; an entry for a frozen parameter
        or with a different shape is an error, never a silent reassignment.  An entry's 'ema' is taken when this optimizer keeps an EMA;
        where it is absent (or for a parameter without an entry) the EMA starts again from the current parameter.
        The group keys weight_decay, ema_decay and skip_nonfinite: a checkpoint without them (an older one, torch.optim.Adam's -- whose
        'weight_decay' is its L2 term, not this one) keeps the constructor's values.  One with them restores skip_nonfinite; weight_decay where
        this optimizer's arena was laid out for it (a non-None value is an error otherwise); ema_decay where both sides keep an EMA."""
        st = {int(k): e for k, e in sd["state"].items()}
        groups = sd.get("param_groups") or []
        n_ckpt = len(groups[0]["params"]) if groups and "params" in groups[0] else None
        numbering = groups[0].get("flat_adam_numbering") if groups else None
        if numbering not in (None, "all", "trainable"):
            raise ValueError(f"FlatAdam.load_state_dict: unknown flat_adam_numbering {numbering!r}")
        legacy = numbering == "trainable" or (numbering is None and n_ckpt is not None and n_ckpt == len(self.index) and n_ckpt != len(self.all_params))
        if legacy:
            # the layout this class wrote before it numbered frozen parameters too: entry j belongs to the j-th TRAINABLE parameter.  Recognised
            # by the marker, or (checkpoints older than the marker) by its length -- then EVERY entry must be in range and match its
            # parameter's shape, so that a foreign checkpoint of the same length is refused instead of remapped
            bad = [j for j in st if not 0 <= j < len(self.index)]
            if bad:
                raise ValueError(f"FlatAdam.load_state_dict: state entries {bad[:5]} are outside the {len(self.index)} trainable parameters of the "
                                 f"legacy (trainable-only) numbering this checkpoint appears to use")
            for j, e in st.items():
                pj = self.params[j]
                if tuple(e["exp_avg"].shape) != tuple(pj.shape):
                    raise ValueError(f"FlatAdam.load_state_dict: legacy-numbered state {j} has shape {tuple(e['exp_avg'].shape)}, trainable parameter {j} "
                                     f"{tuple(pj.shape)}: not a checkpoint of this parameter list")
            st = {self.index[j]: e for j, e in st.items()}
        elif n_ckpt is not None and n_ckpt != len(self.all_params):
            raise ValueError(f"FlatAdam.load_state_dict: the checkpoint's optimizer was built over {n_ckpt} parameters, "
                             f"this one over {len(self.all_params)} (pass the same model.parameters())")
        trainable = set(self.index)
        for i in st:
            if i not in trainable:
                raise ValueError(f"FlatAdam.load_state_dict: state entry {i} belongs to a parameter that is frozen (or absent) here")
        m = torch.zeros(self.n_pad, device=self.m.device, dtype=torch.float32)
        v = torch.zeros(self.n_pad, device=self.m.device, dtype=torch.float32)
        ema = self.flat_p.clone() if self.ema is not None else None
        steps = 0
        for i, p, off in zip(self.index, self.params, self.offsets):
            e = st.get(i)
            if e is None:
                continue
            if ema is not None and "ema" in e:
                if tuple(e["ema"].shape) != tuple(p.shape):
                    raise ValueError(f"FlatAdam.load_state_dict: state {i} has an 'ema' of shape {tuple(e['ema'].shape)}, parameter {tuple(p.shape)}")
                ema[off:off + p.numel()].copy_(e["ema"].reshape(-1))
            if tuple(e["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"FlatAdam.load_state_dict: state {i} has shape {tuple(e['exp_avg'].shape)}, parameter {tuple(p.shape)}")
            k = p.numel()
            m[off:off + k].copy_(e["exp_avg"].reshape(-1))
            v[off:off + k].copy_(e["exp_avg_sq"].reshape(-1))
            steps = max(steps, int(float(e["step"])))
        self.steps = steps
        self._consolidated = None
        self.m.copy_(m[self.shard_off:self.shard_off + self.shard_n])
        self.v.copy_(v[self.shard_off:self.shard_off + self.shard_n])
        if ema is not None:
            self.ema.copy_(ema[self.shard_off:self.shard_off + self.shard_n])
        for g, sg in zip(self.param_groups, groups):
            mine = {k: g.get(k) for k in ("weight_decay", "ema_decay", "skip_nonfinite")}
            g.update({k: v_ for k, v_ in sg.items() if k not in ("params", "flat_adam_numbering")})
            g["max_grad_norm"] = sg.get("max_grad_norm")         # a checkpoint without the key (torch.optim.Adam's, an older one): no clipping
            g.update(mine)
            if "skip_nonfinite" in sg:                           # written by this class with the three keys
                g["skip_nonfinite"] = bool(sg["skip_nonfinite"])
                if self._decay_layout:
                    g["weight_decay"] = sg.get("weight_decay")
                elif sg.get("weight_decay") is not None:
                    raise ValueError("FlatAdam.load_state_dict: the checkpoint trains with weight_decay, this optimizer was constructed with "
                                     "weight_decay=None (its arena is not laid out for decay)")
                if self.ema is not None and sg.get("ema_decay") is not None:
                    g["ema_decay"] = sg["ema_decay"]
