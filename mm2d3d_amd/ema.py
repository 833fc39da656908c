"""Mean-teacher weights: an exponential moving average (EMA) of everything the flat optimisers train.

    ema = WeightEMA(optimizers, model, decay=0.999, warmup=True)
    ...optimiser steps...
    ema.update(skip_words)            # ONE launch (csrc/optim.hip k_ema_update) over every arena and floating-point buffer
    with ema.applied():               # the teacher's weights stand in the model, the student's wait in the teacher's arrays
        model(batch)

The parameters of a flat optimiser are views into its arenas (mm2d3d_amd/optimizers.py ``arena["p"]``), so the teacher is one more
array per arena, plus a copy of every floating-point module buffer (the batch norms' running statistics).  Whether a training
step happens is decided on the device (the loss scale's overflow flags, the data-parallel reducer's skip words: the host never
learns the outcome), so the average is gated on the device by the same decision: the coefficient row of the first optimiser's
last device-counted step and the caller's skip words.  A skipped step is neither averaged in nor counted by the warm-up, whose
``t`` is that optimiser's own counter of taken steps.  One exception follows from the optimiser, not from here: ``FlatAdamW``
without amsgrad keeps its counter on the host under ``step(skip_words=)`` and advances it also when the device skipped the update
(its class docstring); there the skip words alone gate the average, and the warm-up counts what that counter counts.

``swap`` exchanges CONTENTS, never pointers: the captured HIP graphs of the 2D trunk hold the parameters' addresses.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

__all__ = ["WeightEMA"]

_ROW_ELEMS = 1024  # elements per workgroup (csrc/optim.hip: 256 threads of four)


def _named_modules(modules):
    """(prefix, module) pairs: one module keeps its own keys, a dict / list prefixes them as nn.ModuleDict / nn.ModuleList do."""
    if isinstance(modules, torch.nn.Module):
        return [("", modules)]
    if isinstance(modules, dict):
        return [(f"{k}.", m) for k, m in modules.items()]
    return [(f"{i}.", m) for i, m in enumerate(modules)]


class WeightEMA:
    def __init__(self, optimizers, modules, decay, warmup=False):
        optimizers = list(optimizers)
        for o in optimizers:
            if not hasattr(o, "grad_arenas"):
                raise TypeError(f"WeightEMA: {type(o).__name__} is not a flat optimiser (mm2d3d_amd.optimizers: adamw, adam, sgd, "
                                "rmsprop); its update is not decided on the device")
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightEMA: decay must be in [0, 1), not {decay!r}")
        self.decay, self.warmup = decay, bool(warmup)
        self.optimizers = optimizers
        self._modules = _named_modules(modules)
        # the arenas: (optimiser, arena, teacher array)
        self._arenas = [(o, a, a["p"].clone()) for o in optimizers for a in o._arenas if a is not None]
        self._slices = {}  # id(parameter) -> (teacher array, lo, hi)
        for _, a, e in self._arenas:
            for p, (lo, hi) in zip(a["params"], a["spans"]):
                self._slices[id(p)] = (e, lo, hi)
        # floating-point buffers: (key, live buffer, teacher copy); integer buffers and parameters outside the arenas are shared
        self._buffers, seen = [], set()
        for prefix, m in self._modules:
            for k, b in m.named_buffers():
                if b is None or not b.dtype.is_floating_point or id(b) in seen:
                    continue
                if b.dtype != torch.float32 or not b.is_contiguous():
                    raise TypeError(f"WeightEMA: buffer {prefix}{k} must be contiguous float32, not {b.dtype}")
                seen.add(id(b))
                self._buffers.append((prefix + k, b, b.detach().clone()))
        self._table, self._nrows, self._nblocks = None, 0, 0
        self._depth = 0  # applied() contexts entered
        self._build_table()

    # ------------------------------------------------------------------ the table (built once, uploaded once)
    def _pairs(self):
        return [(e, a["p"]) for _, a, e in self._arenas] + [(c, b) for _, b, c in self._buffers]

    def _build_table(self):
        pairs = self._pairs()
        devs = {t.device for pair in pairs for t in pair}
        if len(devs) > 1:
            raise ValueError(f"WeightEMA: arenas and buffers live on several devices: {sorted(map(str, devs))}")
        self.device = devs.pop() if devs else torch.device("cpu")
        self._nrows = len(pairs)
        if self.device.type != "cuda" or not pairs:
            return  # update() / swap() refuse CPU tensors; an empty table needs no launch
        nb = int(_lib.lib().mm_ema_row_bytes())
        assert nb == 32, nb  # csrc/optim.hip EmaRow: dst, src, n, first
        rows = np.zeros((len(pairs), 4), dtype=np.int64)
        first = 0
        for i, (e, p) in enumerate(pairs):
            rows[i] = (e.data_ptr(), p.data_ptr(), p.numel(), first)
            first += -(-p.numel() // _ROW_ELEMS)
        self._nblocks = first
        self._table = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(self.device)

    def _require_gpu(self, what):
        if self.device.type != "cuda":
            raise RuntimeError(f"WeightEMA.{what}: parameters must be on the GPU (the update is a HIP kernel, no CPU fallback)")

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def update(self, skip_words=None):
        """After the optimiser steps of a training step, with the skip words those steps were given: one launch."""
        self._require_gpu("update")
        if not self._nblocks:
            return
        first = self.optimizers[0] if self.optimizers else None
        coef = first.gate_coef() if first is not None else None
        t = first.step_counter() if first is not None else 0
        t_dev, t_host = (t, 0) if torch.is_tensor(t) else (None, int(t))
        nskip = 0 if skip_words is None else int(skip_words.numel())
        check(_lib.lib().mm_ema_update(ptr(self._table), self._nrows, self._nblocks, self.decay, int(self.warmup), t_host, ptr(t_dev),
                                       ptr(coef), ptr(skip_words), nskip, stream()), "ema_update")

    @torch.no_grad()
    def swap(self):
        """Teacher <-> student, by content.  The packed 16-bit weight copies are stale afterwards (conv2d.PARAM_EPOCH)."""
        self._require_gpu("swap")
        from . import conv2d as _c2d

        check(_lib.lib().mm_ema_swap(ptr(self._table), self._nrows, self._nblocks, stream()), "ema_swap")
        _c2d.PARAM_EPOCH[0] += 1

    @contextlib.contextmanager
    def applied(self):
        """The model computes with the teacher's weights and buffers inside; the student's come back on the way out, also
        when the body raises.  Re-entrant: only the outermost context swaps (a whole evaluation loop may sit in one
        ``applied()`` around a trainer whose ``ema_eval`` steps enter it again, and pays the two swaps once)."""
        self._depth += 1
        try:
            if self._depth == 1:
                self.swap()
            try:
                yield self
            finally:
                if self._depth == 1:
                    self.swap()
        finally:
            self._depth -= 1

    @torch.no_grad()
    def reset(self):
        """Teacher = the weights and buffers as they are now (after loading a checkpoint that holds no teacher)."""
        for e, p in self._pairs():
            e.copy_(p)

    # ------------------------------------------------------------------ checkpoints
    def teacher_state_dict(self):
        """The teacher under the modules' own ``state_dict`` keys (copies); what is not tracked is the student's."""
        copies = {id(b): c for _, b, c in self._buffers}
        out = {}
        for prefix, m in self._modules:
            for k, v in m.state_dict(keep_vars=True).items():
                if id(v) in self._slices:
                    e, lo, hi = self._slices[id(v)]
                    out[prefix + k] = e[lo:hi].view(v.shape).clone()
                else:
                    out[prefix + k] = copies.get(id(v), v).detach().clone()
        return out

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "arenas": [e.clone() for _, _, e in self._arenas],
                "buffers": {k: c.clone() for k, _, c in self._buffers}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        arenas, buffers = sd["arenas"], sd["buffers"]
        if len(arenas) != len(self._arenas) or any(t.numel() != e.numel() for t, (_, _, e) in zip(arenas, self._arenas)):
            raise ValueError("WeightEMA.load_state_dict: the arenas do not match this trainer's")
        missing = [k for k, _, _ in self._buffers if k not in buffers]
        if missing:
            raise KeyError(f"WeightEMA.load_state_dict: no teacher copy of {missing[:3]}")
        self.decay, self.warmup = float(sd["decay"]), bool(sd["warmup"])
        for t, (_, _, e) in zip(arenas, self._arenas):
            e.copy_(t)
        for k, _, c in self._buffers:
            c.copy_(buffers[k])
