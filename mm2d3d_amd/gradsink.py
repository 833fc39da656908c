"""Gradient sinks: backward kernels accumulate parameter gradients directly into the optimiser's flat gradient arena.

torch's autograd would otherwise (1) sum the contributions of the two forward passes of a step (source, target) in an
InputBuffer and (2) add the result into ``param.grad`` - two elementwise kernels per parameter per step, ~900 launches
for the ~490 parameters of the two nets.  When a parameter has a sink (``FlatAdamW`` installs ``_mm_sink`` = its slice of
the arena, zeroed by ``zero_grad``) the autograd Functions of this package pass the slice to their weight-gradient
kernels with ``accumulate=1`` and return ``None`` for that input.  The post-accumulate hooks (optimiser bookkeeping,
data-parallel bucket countdown) are fired by hand once the LAST contribution of the step has been issued.
"""
from __future__ import annotations

import contextlib

import torch


def claim(ctx, param, needs_grad):
    """Call in Function.forward.  Returns True when backward should write into ``param._mm_sink``."""
    use = bool(needs_grad) and not _SUSPENDED[0] and hasattr(param, "_mm_sink")
    if use:
        param._mm_pending += 1
    return use


_SUSPENDED = [0]


@contextlib.contextmanager
def suspended():
    """Forwards inside claim nothing.  For a forward under no_grad BETWEEN ``zero_grad`` and the step's backward (the mean teacher's,
    train.py ``pseudo_label_source="teacher"``): ``needs_input_grad`` is set there all the same, the grad mode cannot be read inside
    ``Function.forward`` (it is always off there), and no backward would ever release the claim - the parameter's hooks would
    not fire at the end of the student's backward, and a captured backward would miss its sunk gradients."""
    _SUSPENDED[0] += 1
    try:
        yield
    finally:
        _SUSPENDED[0] -= 1


_COLLECT = [None]


def done(param):
    """Call in Function.backward after the kernel accumulating into ``param._mm_sink`` has been enqueued."""
    param._mm_pending -= 1
    if param._mm_pending == 0:
        if _COLLECT[0] is not None:  # a backward pass that is being CAPTURED into a HIP graph (graph2d.py): the hooks are per-step
            _COLLECT[0].append(param)  # Python work - the caller fires them after every replay
            return
        for h in param._mm_hooks:
            h(param)


def collect_hooks():
    """From now on ``done`` records the parameters whose last contribution has been issued instead of firing their hooks."""
    _COLLECT[0] = []
    return _COLLECT[0]


def release_hooks(token):
    """Ends ``collect_hooks``; returns the recorded parameters (in completion order)."""
    _COLLECT[0] = None
    return list(token)


def claim_affine(ctx, weight, bias, needs_grad):
    """``claim`` for the (weight, bias) pair of a batch norm: the pair when both exist and the weight is claimed, else None."""
    if weight is not None and bias is not None and claim(ctx, weight, needs_grad):
        claim(ctx, bias, True)
        return (weight, bias)
    return None


def affine_targets(sinks, C, device, has_weight=True, has_bias=True):
    """(dwt, dbt, accumulate, dw, db) for a batch norm's backward kernel: what it writes dgamma / dbeta into and what the Function
    returns for them - the sink slices (accumulate = 1, nothing to return) or fresh fp32 [C] tensors (accumulate = 0)."""
    if sinks is not None:  # straight into the optimiser's gradient arena
        return sinks[0]._mm_sink, sinks[1]._mm_sink, 1, None, None
    dw = torch.empty(C, dtype=torch.float32, device=device) if has_weight else None
    db = torch.empty(C, dtype=torch.float32, device=device) if has_bias else None
    return dw, db, 0, dw, db


def done_all(sinks):
    """``done`` for every parameter of ``sinks`` (what ``claim_affine`` returned: None = nothing was claimed)."""
    for p in sinks or ():
        done(p)


# deferred gradient work (DeferredSums: the slab sums of a whole backward pass in one launch; graph2d: graphs with a backward in flight)
# registers a reset here; FlatAdamW.zero_grad calls them, so that what an aborted backward pass left behind never reaches the next
# step's gradients
RESETTERS = []


def reset_deferred():
    for r in RESETTERS:
        r()


class DeferredSums:
    """Weight-gradient slab sums of a whole backward pass, issued as few batched launches at its end (conv2d._WgBatch, scn.ops._DwBatch).

    A backward node ``add``s an item - its slabs, the sink slice(s) they sum into, what the kernel needs, the parameter(s) - and
    returns None for the weight; an end-of-backward callback of the autograd engine ``flush``es: one ``_launch`` per group of items,
    then ``done`` for every parameter in item order.  A subclass says where an item keeps its destinations and its parameters, and
    launches a group."""

    def __init__(self):
        self.items = []
        self.cb_queued = False
        RESETTERS.append(self.reset)

    def _dests(self, item):
        """Addresses of the sink slices the item's slabs are summed into (one, or two for a paired launch)."""
        raise NotImplementedError

    def _params(self, item):
        """The parameters behind ``_dests``, in the same order."""
        raise NotImplementedError

    def _launch(self, group):
        raise NotImplementedError

    def add(self, item):
        self.items.append(item)
        if not self.cb_queued:
            self.cb_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)

    def _end_of_backward(self):
        self.cb_queued = False
        self.flush()

    def reset(self):
        """Forget slabs whose backward pass never reached its end (an exception in between): called by FlatAdamW.zero_grad.  The
        autograd engine skips the final callbacks of a graph task that raised, so ``_end_of_backward`` never ran and never cleared
        ``cb_queued``: left set, no later backward pass would queue it again - the deferred sums would never launch, the weight
        gradients stay zero and their hooks never fire."""
        self.items = []
        self.cb_queued = False

    def flush(self):
        items, self.items = self.items, []
        if not items:
            return
        # A weight that took part in the forward pass twice (the literal two-call sequence of the two domains, train.py:186-292;
        # gradient accumulation) has two slab sets that ADD into one gradient: they must not share a launch (two blocks would
        # read-modify-write the same words) - a new launch starts whenever a destination repeats.  The joint-domain step uses every
        # weight once: one launch.
        groups, seen = [[]], set()
        for it in items:
            dst = set(self._dests(it))
            if dst & seen:
                groups.append([])
                seen = set()
            seen |= dst
            groups[-1].append(it)
        for g in groups:
            self._launch(g)
        for it in items:
            for prm in self._params(it):
                done(prm)
