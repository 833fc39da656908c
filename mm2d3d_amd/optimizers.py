"""Optimiser / scheduler factory with the reference's API (lib/optimizers.py:11-42).

``Optimizer(name, **kw).set_scheduler(name, **kw).build(params) -> (optimizer, scheduler | None)``.
The four names of the reference's registry build flat optimisers: ``adamw`` -> :class:`FlatAdamW`, ``adam`` -> :class:`FlatAdam`
(weight decay as L2, torch.optim.Adam), ``sgd`` -> :class:`FlatSGD`, ``rmsprop`` -> :class:`FlatRMSprop`.  Parameters, gradients
and the optimiser's state live in flat fp32 arenas (one allocation each), so the update is ONE fused HIP kernel per step
(csrc/optim.hip k_optim, one kernel family for all four) instead of torch's per-tensor loop
(SURVEY.md K16), the data-parallel all-reduce runs on slices of the same gradient arena without packing copies
(mm2d3d_amd/ddp.py), backward kernels may accumulate straight into it (mm2d3d_amd/gradsink.py) and the loss scale of the fp16
mode can skip a step on the device (mm2d3d_amd/amp.py).  ``param_groups`` / ``defaults`` carry the keys of torch's classes, and
every hyper-parameter is read from ``param_groups`` on each step: schedulers are torch's own host-side classes, as in the
reference (``one_cycle`` cycles lr AND momentum, or beta1 where the optimiser has ``betas``).
"""
from __future__ import annotations

import torch
from torch import optim
from torch.optim import lr_scheduler

from . import _lib
from ._lib import check, ptr, stream
from .clip import clip_grad_norm_, clip_grad_value_

__all__ = ["Optimizer", "FlatAdamW", "FlatAdam", "FlatSGD", "FlatRMSprop", "clip_grad_norm_", "clip_grad_value_"]


def _only_supported(name, maximize=False, **flags):
    """Arguments torch accepts that do not apply to a fused flat update: fine when None / False."""
    if maximize:
        raise NotImplementedError(f"{name}: maximize=True is not implemented")
    for k, v in flags.items():
        if v:
            raise NotImplementedError(f"{name}: {k}=True does not apply (the update is one fused HIP kernel over flat arenas)")


class _FlatOptimizer(optim.Optimizer):
    """What the flat optimisers share: the arenas (``params, p, g, spans, touched`` + the state arrays named by
    ``_state_names(group)``, allocated only when the hyper-parameters need them), the gradient sinks, the step counter that
    lives on the host or on the device, and the checkpoint format.  A subclass supplies ``_state_names``, ``_coef_bytes`` and
    the three launches ``_plain`` / ``_prepare`` / ``_scaled``."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._arenas = []
        self._step = 0
        self._own = None  # device state of step(skip_words=): unit scale, step counter, coefficient rows, a zero flag word
        self._clip_scale = None  # clip.clip_grad_norm_: the effective scale (device) the NEXT step takes in place of the loss scale
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                self._arenas.append(None)
                continue
            dev = ps[0].device  # CPU arenas are allowed (gloo tests of the reducer); step() itself is HIP-only
            n = sum(p.numel() for p in ps)
            flat_p = torch.empty(n, dtype=torch.float32, device=dev)
            flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
            spans, off = [], 0
            for p in ps:
                k = p.numel()
                flat_p[off : off + k].copy_(p.data.reshape(-1))
                p.data = flat_p[off : off + k].view(p.shape)
                p.grad = flat_g[off : off + k].view(p.shape)
                spans.append((off, off + k))
                off += k
            arena = dict(params=ps, p=flat_p, g=flat_g, spans=spans, touched=[False] * len(ps), state=())
            self._ensure_state(group, arena)
            for i, p in enumerate(ps):
                hook = self._make_hook(arena, i)
                p.register_post_accumulate_grad_hook(hook)
                # gradient sink (mm2d3d_amd/gradsink.py): backward kernels may accumulate straight into the arena slice and
                # skip autograd's per-parameter add kernels; the same hooks fire when the last contribution has landed
                lo, hi = spans[i]
                p._mm_sink = flat_g[lo:hi].view(p.shape)
                p._mm_pending = 0
                p._mm_hooks = [hook]
            self._arenas.append(arena)

    # ------------------------------------------------------------------ what a subclass supplies
    def _state_names(self, group):
        raise NotImplementedError

    def _coef_bytes(self):
        """Size of one parameter group's device coefficients (mm2d3d_amd/amp.py sizes its buffer by it)."""
        return int(_lib.lib().mm_optim_coef_bytes())

    def _plain(self, L, group, a, lo, hi, grad_scale, skip_words):
        raise NotImplementedError

    def _prepare(self, L, group, scale_dev, found_dev, step_dev, advance, grad_scale, coef):
        raise NotImplementedError

    def _scaled(self, L, group, a, lo, hi, coef):
        raise NotImplementedError

    # a skipped step(skip_words=) does not use up a step of the counter (FlatAdamW without amsgrad keeps its host counter)
    _skips_on_device = True

    # ------------------------------------------------------------------ arenas
    def _ensure_state(self, group, a):
        """State arrays the group's CURRENT hyper-parameters need (a scheduler may have switched momentum on): zero-filled."""
        for name in self._state_names(group):
            if name not in a:
                a[name] = torch.zeros_like(a["p"])
                a["state"] = a["state"] + (name,)

    @staticmethod
    def _make_hook(arena, i):
        def hook(param):
            arena["touched"][i] = True
            lo, hi = arena["spans"][i]
            if param.grad is None:  # contribution(s) arrived through the gradient sink
                param.grad = arena["g"][lo:hi].view(param.shape)
            elif param.grad.data_ptr() != arena["g"].data_ptr() + 4 * lo:
                # autograd replaced .grad (it was None): fold it back into the arena
                arena["g"][lo:hi].copy_(param.grad.reshape(-1))
                param.grad = arena["g"][lo:hi].view(param.shape)

        return hook

    def grad_arenas(self):
        """Flat gradient buffers (one per param group) - what the data-parallel all-reduce works on."""
        return [a["g"] for a in self._arenas if a is not None]

    def zero_grad(self, set_to_none: bool = False):
        from . import gradsink

        gradsink.reset_deferred()
        self._clip_scale = None  # a clip coefficient belongs to the gradients it was formed from
        for a in self._arenas:
            if a is None:
                continue
            a["g"].zero_()
            a["touched"] = [False] * len(a["params"])
            for (lo, hi), p in zip(a["spans"], a["params"]):
                p._mm_pending = 0
                if p.grad is None or p.grad.data_ptr() != a["g"].data_ptr() + 4 * lo:
                    p.grad = a["g"][lo:hi].view(p.shape)

    def mark_all_touched(self):
        for a in self._arenas:
            if a is not None:
                a["touched"] = [True] * len(a["params"])

    @staticmethod
    def _touched_ranges(a):
        """Parameters that took part in no backward keep weights and state (torch skips grad=None params)."""
        ranges, cur = [], None
        for t, (lo, hi) in zip(a["touched"], a["spans"]):
            if t:
                cur = [lo, hi] if cur is None else [cur[0], hi]
            elif cur is not None:
                ranges.append(cur)
                cur = None
        if cur is not None:
            ranges.append(cur)
        return ranges

    def _require_gpu(self, what):
        if any(a is not None and a["p"].device.type != "cuda" for a in self._arenas):
            raise RuntimeError(f"{type(self).__name__}.{what}: parameters must be on the GPU (the update is a HIP kernel, no CPU fallback)")

    # ------------------------------------------------------------------ steps
    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0, skip_words=None):
        """``skip_words``: device int32 words (<= 16) - the update is a no-op on the device when any of them is nonzero (the
        data-parallel reducer's collective flags, ddp.GradAllReducer.skip_words: no read-back, the host never waits).  The step
        then runs in the form of ``step_scaled`` with a unit scale and the counter on the device, so a skipped step does not use
        up a step of the counter (Adam's bias corrections, SGD's first-step rule).  A step after ``clip.clip_grad_norm_`` takes that
        form too, for every optimiser: the clip coefficient exists on the device only."""
        loss = closure() if closure is not None else None
        self._require_gpu("step")
        if self._clip_scale is not None or (skip_words is not None and self._skips_on_device):
            if self._own is None:
                dev = next(a["p"].device for a in self._arenas if a is not None)
                self._own = (torch.ones(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                             torch.zeros((max(1, len(self.param_groups)), self._coef_bytes()), dtype=torch.uint8, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev))
            self.step_scaled(self._own[0], self._own[3] if skip_words is None else skip_words, self._own[1], self._own[2], grad_scale)
            return loss
        L = _lib.lib()
        if getattr(self, "_dev_step", None) is not None:
            # plain step after device-counted ones: the device counter is the truth (skipped steps never advanced it); one
            # read-back, then the host counter leads again
            self._step = int(self._dev_step.item())
            self._dev_step = None
        self._step += 1
        from . import conv2d as _c2d

        _c2d.PARAM_EPOCH[0] += 1  # packed bf16 weight copies are stale after this update
        for group, a in zip(self.param_groups, self._arenas):
            if a is None:
                continue
            self._ensure_state(group, a)
            for lo, hi in self._touched_ranges(a):
                self._plain(L, group, a, lo, hi, float(grad_scale), skip_words)
        return loss

    @torch.no_grad()
    def step_scaled(self, scale_dev, found_dev, step_dev, coef_dev, grad_scale: float = 1.0):
        """The update of ``step`` under a device-resident loss scale (mm2d3d_amd/amp.py): gradients are multiplied by
        ``grad_scale / scale``, and nothing is updated when ANY word of ``found_dev`` is set (the non-finite flags of every optimiser
        of the step + the caller's skip words: one decision for all, as the reference's HybridOptim gets from Lightning's
        GradScaler, train.py:627-636) - decided on the device; the step counter (``step_dev``) advances only when the step is
        taken.  After ``clip.clip_grad_norm_`` the clip's effective scale ``scale / c`` stands in for ``scale_dev``, once."""
        self._require_gpu("step_scaled")
        L = _lib.lib()
        if self._clip_scale is not None:
            scale_dev, self._clip_scale = self._clip_scale, None
        if getattr(self, "_dev_step", None) is not step_dev:
            if getattr(self, "_dev_step", None) is not None:  # another device counter led until now (one read-back)
                self._step = int(self._dev_step.item())
            # first device-counted step, or the first after plain steps / a restored checkpoint: the host counter is the truth until now
            step_dev.fill_(int(self._step))
        self._dev_step = step_dev
        self._dev_coef = coef_dev  # gate_coef(): the rows this step's decision is written to
        self._opt_called = True  # what torch's lr schedulers look at to tell "step() before scheduler.step()"
        from . import conv2d as _c2d

        _c2d.PARAM_EPOCH[0] += 1
        first = True
        for gi, (group, a) in enumerate(zip(self.param_groups, self._arenas)):
            if a is None:
                continue
            self._ensure_state(group, a)
            self._prepare(L, group, scale_dev, found_dev, step_dev, 1 if first else 0, float(grad_scale), coef_dev[gi])
            first = False
            for lo, hi in self._touched_ranges(a):
                self._scaled(L, group, a, lo, hi, coef_dev[gi])

    # ------------------------------------------------------------------ what the last step decided (mm2d3d_amd/ema.py)
    def gate_coef(self):
        """The device coefficient row (csrc/optim.hip OptCoef) of the last step when that step was device-counted: its ``skip``
        field is the decision the update was gated by (non-finite gradients of any optimiser of the step, the caller's skip
        words).  None after a plain step, which has no such row: its skip words alone gated it."""
        if getattr(self, "_dev_step", None) is None:
            return None
        gi = next((i for i, a in enumerate(self._arenas) if a is not None), None)
        return None if gi is None else self._dev_coef[gi]

    def step_counter(self):
        """The count of taken steps: the device counter (int64[1]) while device-counted steps lead, else the host's int."""
        dev = getattr(self, "_dev_step", None)
        return self._step if dev is None else dev

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        sd = super().state_dict()
        sd["flat"] = [None if a is None else {name: a[name].clone() for name in a["state"]} for a in self._arenas]
        if getattr(self, "_dev_step", None) is not None:  # device-counted steps: the device counter is the truth (skipped steps)
            self._step = int(self._dev_step.item())
        sd["step"] = self._step
        return sd

    def load_state_dict(self, sd):
        flat, step = sd.get("flat"), sd.get("step", 0)
        super().load_state_dict({k: v for k, v in sd.items() if k not in ("flat", "step")})
        self._step = step
        self._dev_step = None  # a device counter from before the restore is stale
        if flat:
            for a, f in zip(self._arenas, flat):
                if a is not None and f is not None:
                    for name, t in f.items():
                        if name not in a:
                            a[name] = torch.zeros_like(a["p"])
                            a["state"] = a["state"] + (name,)
                        a[name].copy_(t)


def _range(a, names, lo, hi):
    """Pointers of the slices [lo, hi) of the named arrays; None for a name the arena does not hold."""
    return [ptr(a[n][lo:hi]) if n is not None else None for n in names]


class FlatAdamW(_FlatOptimizer):
    """AdamW (decoupled weight decay, torch.optim.AdamW semantics) over flat arenas: state ``m``, ``v`` and, with ``amsgrad``,
    ``vmax``.  The bias corrections are keyed to the optimiser's step counter, not to a parameter's own: a parameter that first
    receives a gradient on a later step differs from torch there.  The update is the Adam kernel of csrc/optim.hip with decoupled
    decay.  Without ``amsgrad``, ``step(skip_words=)`` is a plain launch that keeps the counter on the host, which advances also
    when the device skipped the update (the trainer raises one step later, train.py); with it - and for :class:`FlatAdam` always -
    the counter is on the device.  No kernel asks for that split any more: it is kept because the device-counted form would add
    a ``k_optim_prepare`` launch per group to the data-parallel bf16 step and move its counter."""

    _decoupled = 1

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        _only_supported(type(self).__name__, maximize, foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=bool(self._decoupled)))

    def _state_names(self, group):
        return ("m", "v", "vmax") if group.get("amsgrad") else ("m", "v")

    @property
    def _skips_on_device(self):
        # FlatAdam (not decoupled) has always counted on the device; FlatAdamW does only for amsgrad (class docstring)
        return not self._decoupled or any(g.get("amsgrad") for g in self.param_groups)

    @staticmethod
    def _hp(group):
        b1, b2 = group["betas"]
        return float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"])

    @staticmethod
    def _arrays(group):
        return ("p", "g", "m", "v", "vmax" if group.get("amsgrad") else None)

    def _plain(self, L, group, a, lo, hi, grad_scale, skip_words):
        nskip = 0 if skip_words is None else int(skip_words.numel())
        check(L.mm_adam_step(*_range(a, self._arrays(group), lo, hi), hi - lo, *self._hp(group), self._decoupled, self._step,
                             grad_scale, ptr(skip_words), nskip, stream()), "adam_step")

    def _prepare(self, L, group, scale_dev, found_dev, step_dev, advance, grad_scale, coef):
        check(L.mm_adam_prepare(ptr(scale_dev), ptr(found_dev), int(found_dev.numel()), ptr(step_dev), advance, *self._hp(group),
                                self._decoupled, grad_scale, ptr(coef), stream()), "adam_prepare")

    def _scaled(self, L, group, a, lo, hi, coef):
        check(L.mm_adam_step_dev(*_range(a, self._arrays(group), lo, hi), hi - lo, self._decoupled, ptr(coef), stream()),
              "adam_step_dev")


class FlatAdam(FlatAdamW):
    """torch.optim.Adam over flat arenas: weight decay is L2 (added to the gradient); ``amsgrad`` adds the state ``vmax``.  Bias
    corrections are keyed to the optimiser's step counter, as :class:`FlatAdamW`'s are."""

    _decoupled = 0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if decoupled_weight_decay:
            raise NotImplementedError("FlatAdam: decoupled_weight_decay=True is FlatAdamW (adamw)")
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, foreach=foreach, capturable=capturable,
                         differentiable=differentiable, fused=fused)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD over flat arenas: state ``buf`` (the momentum buffer) when ``momentum != 0``.  torch's first-step rule
    (``buf = g``, no dampening) is keyed to the optimiser's counter of TAKEN steps - on the device in the loss-scaled form and
    under ``step(skip_words=)``, so a skipped step does not use it up - not to a parameter's own: with ``dampening != 0`` a
    parameter that first receives a gradient on a later step (or a momentum that a scheduler switches on later) differs from
    torch there.  :class:`FlatAdamW`'s bias corrections are keyed the same way."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        _only_supported("FlatSGD", maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused))

    def _state_names(self, group):
        return ("buf",) if group["momentum"] != 0 else ()

    @staticmethod
    def _hp(group):
        return float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"])

    def _plain(self, L, group, a, lo, hi, grad_scale, skip_words):
        check(L.mm_sgd_step(*_range(a, ("p", "g", "buf" if group["momentum"] != 0 else None), lo, hi), hi - lo, *self._hp(group),
                            int(bool(group["nesterov"])), self._step, grad_scale, ptr(skip_words),
                            0 if skip_words is None else int(skip_words.numel()), stream()), "sgd_step")

    def _prepare(self, L, group, scale_dev, found_dev, step_dev, advance, grad_scale, coef):
        check(L.mm_sgd_prepare(ptr(scale_dev), ptr(found_dev), int(found_dev.numel()), ptr(step_dev), advance, *self._hp(group),
                               grad_scale, ptr(coef), stream()), "sgd_prepare")

    def _scaled(self, L, group, a, lo, hi, coef):
        check(L.mm_sgd_step_dev(*_range(a, ("p", "g", "buf" if group["momentum"] != 0 else None), lo, hi), hi - lo,
                                int(bool(group["nesterov"])), ptr(coef), stream()), "sgd_step_dev")


class FlatRMSprop(_FlatOptimizer):
    """torch.optim.RMSprop over flat arenas: state ``sq``, plus ``gavg`` when ``centered`` and ``buf`` when ``momentum > 0``."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False):
        _only_supported("FlatRMSprop", maximize, foreach=foreach, capturable=capturable, differentiable=differentiable)
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                                      capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable))

    def _state_names(self, group):
        return ("sq",) + (("gavg",) if group["centered"] else ()) + (("buf",) if group["momentum"] > 0 else ())

    @staticmethod
    def _hp(group):
        return float(group["lr"]), float(group["alpha"]), float(group["eps"]), float(group["weight_decay"]), float(group["momentum"])

    @staticmethod
    def _arrays(group):
        return ("p", "g", "sq", "gavg" if group["centered"] else None, "buf" if group["momentum"] > 0 else None)

    def _plain(self, L, group, a, lo, hi, grad_scale, skip_words):
        check(L.mm_rmsprop_step(*_range(a, self._arrays(group), lo, hi), hi - lo, *self._hp(group), grad_scale, ptr(skip_words),
                                0 if skip_words is None else int(skip_words.numel()), stream()), "rmsprop_step")

    def _prepare(self, L, group, scale_dev, found_dev, step_dev, advance, grad_scale, coef):
        check(L.mm_rmsprop_prepare(ptr(scale_dev), ptr(found_dev), int(found_dev.numel()), ptr(step_dev), advance, *self._hp(group),
                                   grad_scale, ptr(coef), stream()), "rmsprop_prepare")

    def _scaled(self, L, group, a, lo, hi, coef):
        check(L.mm_rmsprop_step_dev(*_range(a, self._arrays(group), lo, hi), hi - lo, ptr(coef), stream()), "rmsprop_step_dev")


class Optimizer:
    def __init__(self, name: str, **kwargs):
        self._optim_name = name
        self._optim_args = kwargs
        self._use_scheduler = False

    def set_scheduler(self, name: str, **kwargs):
        self._scheduler_name = name
        self._scheduler_args = kwargs
        self._use_scheduler = True
        return self

    def build(self, params):
        table = {"adamw": FlatAdamW, "adam": FlatAdam, "sgd": FlatSGD, "rmsprop": FlatRMSprop}
        optimizer = table[self._optim_name](params, **self._optim_args)
        scheduler = None
        if self._use_scheduler:
            scheduler = {
                "step": lr_scheduler.StepLR,
                "cosine_annealing": lr_scheduler.CosineAnnealingLR,
                "cyclic": lr_scheduler.CyclicLR,
                "reduce_on_plateau": lr_scheduler.ReduceLROnPlateau,
                "multi_step_lr": lr_scheduler.MultiStepLR,
                "one_cycle": lr_scheduler.OneCycleLR,
            }[self._scheduler_name](optimizer, **self._scheduler_args)
        return optimizer, scheduler
