"""Loss scaling for the fp16 kind of the 16-bit activation mode.

The reference trains with ``precision: 16`` (/root/reference/.../config/train.yaml:11): Lightning's native-AMP plugin, i.e. fp16
autocast + ``torch.cuda.amp.GradScaler`` (init_scale 65536, growth_factor 2, backoff_factor 0.5, growth_interval 2000; an
optimiser whose gradients hold an inf / nan skips its step, ``update()`` then halves the scale, 2000 clean steps double it).
IEEE fp16 gradient rows need that scale (bf16 rows do not: the default 16-bit kind here), so ``GradScaler`` below restates
those semantics for the flat optimisers of :mod:`mm2d3d_amd.optimizers` (adamw, adam, sgd, rmsprop; a mixed list takes ONE joint
decision) - with the scale, the non-finite flags, the clean-step tracker and the optimisers' step counters RESIDENT ON THE DEVICE
(csrc/optim.hip k_grad_nonfinite / k_optim_prepare / k_optim<., ., ., true> / k_amp_update): a skipped step costs no read-back,
the host never waits for the GPU.

    scaler = GradScaler(device)
    (loss * scaler.scale_tensor).backward()          # or scaler.scale(loss).backward()
    scaler.step_all(optimizers, grad_scale)          # checks every gradient arena; ONE decision: all update, or none does
    scaler.update()

``clip=`` of ``step`` / ``step_all`` clips the unscaled gradients between the check and the update (mm2d3d_amd/clip.py: a max
norm, or ``("norm" | "value", x)``; the norm is joint over the optimisers of the call and is left in ``last_grad_norm``, a device
tensor).  The norm kernel raises the non-finite flags itself, so a norm-clipped step reads the gradients once before the update,
as an unclipped one does; the update kernels get ``scale / c`` for the scale, ``update()`` keeps the real one.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, ptr, stream


class GradScaler:
    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        if growth_factor <= 1.0 or not (0.0 < backoff_factor < 1.0) or growth_interval < 1:
            raise ValueError("GradScaler: growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self.enabled = bool(enabled)
        self.device = torch.device(device)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.scale_tensor = torch.full((1,), float(init_scale), dtype=torch.float32, device=self.device)
        self._tracker = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._flags = torch.zeros(16, dtype=torch.int32, device=self.device)  # one non-finite flag per optimiser (views below)
        self._found = {}   # id(optimizer) -> int32[1] flag of the current step
        self._steps = {}   # id(optimizer) -> int64[1] device step counter (advances only on steps that are taken)
        self._coef = {}    # id(optimizer) -> uint8 coefficient rows, one per parameter group
        self.last_grad_norm = None  # clip=("norm", x): the gradient norm of the last step before clipping (0-dim device tensor)

    def scale(self, loss):
        return loss * self.scale_tensor.to(loss.dtype) if self.enabled else loss

    def _state(self, opt):
        k = id(opt)
        if k not in self._found:
            nb = opt._coef_bytes()  # one coefficient struct per parameter group (csrc/optim.hip OptCoef)
            if len(self._found) >= self._flags.numel() - self.N_SKIP:
                raise RuntimeError("GradScaler: more than 12 optimisers")
            self._found[k] = self._flags[len(self._found) : len(self._found) + 1]
            self._steps[k] = torch.full((1,), int(getattr(opt, "_step", 0)), dtype=torch.int64, device=self.device)
            self._coef[k] = torch.zeros((max(1, len(opt.param_groups)), nb), dtype=torch.uint8, device=self.device)
        return self._found[k], self._steps[k], self._coef[k]

    @staticmethod
    def _require_flat(opt):
        if not hasattr(opt, "step_scaled"):
            raise TypeError(f"GradScaler.step: {type(opt).__name__} is not a flat optimiser (mm2d3d_amd.optimizers: adamw, adam, sgd, "
                            "rmsprop); other optimisers have no device-side skip")

    def _check_and_clip(self, opts, founds, grad_scale, clip):
        """The non-finite check of every arena into its optimiser's flag word and, between it and the update, the clip.  A step
        that the flags veto stays skipped whatever the clip makes of its gradients."""
        from .clip import clip_grad_norm_, clip_grad_value_, parse_clip

        clip = parse_clip(clip)
        if clip is not None and clip[0] == "norm":  # mm_grad_sqnorm raises the flags: no separate pass over the gradients
            self.last_grad_norm = clip_grad_norm_(opts, clip[1], scaler=self, grad_scale=grad_scale, found=founds)
            return
        L = _lib.lib()
        for o, found in zip(opts, founds):
            for g in o.grad_arenas():
                check(L.mm_grad_nonfinite(ptr(g), g.numel(), ptr(found), stream()), "grad_nonfinite")
        if clip is not None:
            clip_grad_value_(opts, clip[1], scaler=self, grad_scale=grad_scale)

    def step(self, opt, grad_scale: float = 1.0, clip=None):
        """``opt.step()`` on the unscaled gradients unless one of ITS gradients is inf / nan (decided and applied on the device):
        the per-optimiser form of torch's GradScaler.step.  A trainer whose optimisers are one HybridOptim uses ``step_all``.
        ``clip``: see the module's docstring."""
        if not self.enabled:
            self._clip_unscaled([opt], grad_scale, clip)
            return opt.step(grad_scale=grad_scale)
        self._require_flat(opt)
        found, steps, coef = self._state(opt)
        found.zero_()
        self._check_and_clip([opt], [found], grad_scale, clip)
        opt.step_scaled(self.scale_tensor, found, steps, coef, grad_scale)

    def _clip_unscaled(self, opts, grad_scale, clip):
        """A disabled scaler: the clip of steps without a loss scale (a non-flat optimiser raises TypeError)."""
        from .clip import clip_grad_norm_, clip_grad_value_, parse_clip

        clip = parse_clip(clip)
        if clip is not None and clip[0] == "norm":
            self.last_grad_norm = clip_grad_norm_(opts, clip[1], grad_scale=grad_scale)
        elif clip is not None:
            clip_grad_value_(opts, clip[1], grad_scale=grad_scale)

    N_SKIP = 4  # words [12, 16) of the flag buffer: the caller's extra skip words (ddp.GradAllReducer.skip_words)

    def step_all(self, opts, grad_scale: float = 1.0, skip_words=None, clip=None):
        """The steps of ALL optimisers of a training step under one decision: the reference's HybridOptim is ONE
        optimiser to Lightning's GradScaler (``param_groups`` is the concatenation, train.py:627-636), so a non-finite gradient
        in either network skips both updates.  ``skip_words``: up to 4 more device int32 words that veto the step (the
        data-parallel reducer's collective "gradients invalid" flags) - they do not touch the loss scale.  ``clip``: see the
        module's docstring; one norm over all of ``opts``."""
        if not self.enabled:
            self._clip_unscaled(opts, grad_scale, clip)
            for o in opts:
                o.step(grad_scale=grad_scale, skip_words=skip_words) if hasattr(o, "step_scaled") else o.step()
            return
        for o in opts:
            self._require_flat(o)
        states =[self._state(o) for o in opts]
        n = len(self._found)
        if n > self._flags.numel() - self.N_SKIP:
            raise RuntimeError("GradScaler: more than 12 optimisers")
        self._flags.zero_()  # every optimiser's flag and the skip words: one fill
        if skip_words is not None:
            k = int(skip_words.numel())
            if k > self.N_SKIP:
                raise ValueError("GradScaler.step_all: at most 4 skip words")
            self._flags[self._flags.numel() - self.N_SKIP : self._flags.numel() - self.N_SKIP + k].copy_(skip_words)
        self._check_and_clip(opts, [found for found, _, _ in states], grad_scale, clip)
        for o, (_, steps, coef) in zip(opts, states):
            o.step_scaled(self.scale_tensor, self._flags, steps, coef, grad_scale)

    def update(self):
        if not self.enabled or not self._found:
            return
        L = _lib.lib()
        flags = self._flags[: len(self._found)]  # the optimisers' flags are consecutive views of one buffer
        check(L.mm_amp_update(ptr(self.scale_tensor), ptr(self._tracker), ptr(flags), flags.numel(), self.growth_factor,
                              self.backoff_factor, self.growth_interval, stream()), "amp_update")

    # host views (each one a read-back: logging / tests / checkpoints only)
    def get_scale(self):
        return float(self.scale_tensor.item())

    def steps_taken(self, opt):
        return int(self._state(opt)[1].item())

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(self._tracker.item())}

    def load_state_dict(self, sd):
        self.scale_tensor.fill_(float(sd["scale"]))
        self._tracker.fill_(int(sd.get("_growth_tracker", 0)))
        self.growth_factor = float(sd.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(sd.get("backoff_factor", self.backoff_factor))
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
