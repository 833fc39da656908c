"""Gradient clipping for the flat optimisers: Lightning's ``gradient_clip_val`` / ``gradient_clip_algorithm`` (the reference's
``pl.Trainer`` arguments, run.py:262-288) where ``torch.nn.utils.clip_grad_norm_`` cannot be used - the arenas of
:mod:`mm2d3d_amd.optimizers` hold gradients that still carry the loss scale (mm2d3d_amd/amp.py) and, under data parallelism,
the sum over ranks; both factors are folded into the update on the device and never visible to the host.

``clip_grad_norm_`` (csrc/clip.hip) reads every gradient arena once: ``mm_grad_sqnorm`` leaves double partial sums, and the
one-workgroup ``mm_clip_finalize`` turns the partials of ALL optimisers passed (one joint norm, as Lightning clips the
reference's HybridOptim, whose ``param_groups`` is the concatenation of both networks', train.py:587-592) into the norm of the
true gradient ``g * grad_scale / scale``, torch's coefficient ``c = min(1, max_norm / (norm + 1e-6))`` and the EFFECTIVE SCALE
``scale / c``.  Nothing is written to the gradients: each optimiser's next step takes the effective scale in place of the loss
scale, so its prepare kernel forms ``grad_scale * c / scale`` and the update kernels run unchanged.  A clipped step therefore
always takes the device-coefficient form of ``step_scaled`` (without a loss scaler: a unit scale, the optimiser's own device
counter).  A parameter that took part in no backward holds zeros after ``zero_grad`` and contributes nothing (torch's
``grad is None`` rule).  No read-back anywhere; the returned norm is a device tensor.

With a non-finite norm the coefficient is 0 (inf) or NaN (nan), as ``clip_grad_norm_(error_if_nonfinite=False)`` leaves it:
under a ``GradScaler`` the flags veto that step anyway, without one the weights take the NaN as they would in torch.

    norm = clip_grad_norm_(optimizers, 1.0, grad_scale=reducer.grad_scale)     # then o.step(...) for each of them
    scaler.step_all(optimizers, grad_scale, clip=("norm", 1.0))                 # under the loss scale; see amp.GradScaler
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

__all__ = ["clip_grad_norm_", "clip_grad_value_", "parse_clip"]


def parse_clip(clip):
    """``clip=`` of GradScaler.step / step_all and the trainer: None, a number (max norm) or ``(algorithm, value)`` with Lightning's
    algorithm names -> ``(algorithm, value)`` or None."""
    if clip is None:
        return None
    algo, val = clip if isinstance(clip, (tuple, list)) else ("norm", clip)
    if algo not in ("norm", "value"):
        raise ValueError(f"gradient_clip_algorithm: 'norm' or 'value', not {algo!r}")
    if val is None:
        return None
    if not float(val) >= 0.0:
        raise ValueError(f"gradient_clip_val must be >= 0, not {val!r}")
    return algo, float(val)


def _flat(optimizers, what):
    opts = [optimizers] if isinstance(optimizers, torch.optim.Optimizer) else list(optimizers)
    for o in opts:
        if not hasattr(o, "grad_arenas") or not hasattr(o, "step_scaled"):
            raise TypeError(f"{what}: {type(o).__name__} is not a flat optimiser (mm2d3d_amd.optimizers: adamw, adam, sgd, rmsprop)")
        o._require_gpu(what)
    if not opts or not any(o.grad_arenas() for o in opts):
        raise ValueError(f"{what}: no gradients")
    return opts


def _scale_of(scaler, dev):
    if scaler is not None and scaler.enabled:
        return scaler.scale_tensor
    one = _UNIT.get(dev)
    if one is None:
        one = _UNIT[dev] = torch.ones(1, dtype=torch.float32, device=dev)
    return one


_UNIT = {}  # device -> the unit scale of steps without a loss scaler (read-only)
_WS = {}    # (device, stream) -> double partials, grow-only: kernels of one stream run in order


def _partials(count, dev):
    key = (dev, stream())
    ws = _WS.get(key)
    if ws is None or ws.numel() < count:
        ws = _WS[key] = torch.empty(count, dtype=torch.float64, device=dev)
    return ws


@torch.no_grad()
def clip_grad_norm_(optimizers, max_norm, norm_type=2.0, *, scaler=None, grad_scale: float = 1.0, found=None):
    """Clips the joint 2-norm of the true gradients of ``optimizers`` (one flat optimiser or several) to ``max_norm`` on their NEXT
    step and returns the norm before clipping: a 0-dim device tensor, no read-back.  ``scaler``: the GradScaler whose scale the
    arenas carry; ``grad_scale``: the data-parallel reducer's 1 / world size.  ``found``: one device int32 word per optimiser that
    the norm kernel raises on an inf / nan (what GradScaler passes so that it needs no separate check)."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: norm_type={norm_type!r} is not implemented (only 2)")
    if not float(max_norm) >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be >= 0, not {max_norm!r}")
    opts = _flat(optimizers, "clip_grad_norm_")
    L = _lib.lib()
    arenas = [(g, None if found is None else found[i]) for i, o in enumerate(opts) for g in o.grad_arenas()]
    dev = arenas[0][0].device
    counts = np.array([int(L.mm_grad_sqnorm_ws_bytes(g.numel())) // 8 for g, _ in arenas], dtype=np.int64)
    ws = _partials(int(counts.sum()), dev)
    slot = 0
    for (g, f), k in zip(arenas, counts):
        check(L.mm_grad_sqnorm(ptr(g), g.numel(), ptr(ws), slot, ptr(f), stream()), "grad_sqnorm")
        slot += int(k)
    out = torch.empty(2, dtype=torch.float32, device=dev)  # [norm, effective scale]: fresh each call, as torch returns a new tensor
    check(L.mm_clip_finalize(ptr(ws), counts.ctypes.data, len(arenas), ptr(_scale_of(scaler, dev)), float(grad_scale), float(max_norm),
                             ptr(out[0:1]), ptr(out[1:2]), stream()), "clip_finalize")
    for o in opts:
        o._clip_scale = out[1:2]  # taken by the optimiser's next step (optimizers._FlatOptimizer.step_scaled), dropped by zero_grad
    return out[0]


@torch.no_grad()
def clip_grad_value_(optimizers, clip_value, *, scaler=None, grad_scale: float = 1.0):
    """Clamps the true gradients of ``optimizers`` to ``[-clip_value, clip_value]``: the arenas in place, to
    ``+-clip_value * scale / grad_scale`` (torch.nn.utils.clip_grad_value_; a NaN stays)."""
    if not float(clip_value) >= 0.0:
        raise ValueError(f"clip_grad_value_: clip_value must be >= 0, not {clip_value!r}")
    opts = _flat(optimizers, "clip_grad_value_")
    L = _lib.lib()
    for o in opts:
        for g in o.grad_arenas():
            check(L.mm_grad_clip_value(ptr(g), g.numel(), float(clip_value), ptr(_scale_of(scaler, g.device)), float(grad_scale),
                                       stream()), "grad_clip_value")
