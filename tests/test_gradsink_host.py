"""Host side of the gradient sinks (mm2d3d_amd/gradsink.py): the deferred slab-sum batches' protocol - grouping, one end-of-backward
callback per pass, recovery after a backward pass that raised, the 3D batch's early trigger - and the batch norms' affine-parameter
helpers.  CPU tensors stand in for parameters; the launches are recorded, not issued."""
import pytest
import torch

from mm2d3d_amd import conv2d, gradsink
from mm2d3d_amd.scn import ops


def _param(fired, n=4):
    p = torch.zeros(n, requires_grad=True)
    p._mm_sink = torch.zeros(n)
    p._mm_pending = 0
    p._mm_hooks = [fired.append]
    return p


def _record_launches(batch, fired):
    """``batch._launch`` records (its group, how many hooks had fired by then)."""
    batch.launches = []
    batch._launch = lambda group: batch.launches.append((list(group), len(fired)))
    return batch


class _Sums(gradsink.DeferredSums):
    """Items: (dW, dW1 or None, params)."""

    def _dests(self, it):
        return (it[0].data_ptr(),) if it[1] is None else (it[0].data_ptr(), it[1].data_ptr())

    def _params(self, it):
        return it[2]


class _EarlySums(_Sums):
    """The early trigger of scn.ops._DwBatch, restated."""

    def __init__(self):
        super().__init__()
        self.expected = 0

    def add(self, item):
        super().add(item)
        self.expected -= 1
        if self.expected == 0:
            self.flush()

    def _end_of_backward(self):
        self.expected = 0
        super()._end_of_backward()

    def reset(self):
        super().reset()
        self.expected = 0


@pytest.fixture
def batches():
    """Builds batches whose ``_launch`` records ("dw": the real 3D batch, its launch replaced); their resets leave gradsink.RESETTERS
    again."""
    fired, made = [], []

    def make(kind):
        made.append(_record_launches({"plain": _Sums, "early": _EarlySums, "dw": ops._DwBatch}[kind](), fired))
        return made[-1]

    make.fired = fired
    yield make
    for b in made:
        gradsink.RESETTERS.remove(b.reset)


def _item(batch, *params):
    """An item of ``batch``'s layout that sums into the sinks of ``params`` (one, or the two of a paired launch)."""
    for p in params:
        p._mm_pending += 1  # what gradsink.claim did in the layer's forward
    if isinstance(batch, _Sums):
        return (params[0]._mm_sink, params[1]._mm_sink if len(params) > 1 else None, tuple(params))
    (p,) = params
    return (torch.zeros(1), p._mm_sink, p.numel(), 1, None, p)  # scn.ops._DwBatch: (partial, sink, ne, K, row, param)


class _Layer(torch.autograd.Function):
    """Identity whose backward files one item, as a convolution's backward files its slabs."""

    @staticmethod
    def forward(ctx, x, batch, item, log):
        ctx.batch, ctx.item, ctx.log = batch, item, log
        if hasattr(batch, "expected"):
            batch.expected += 1
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.batch.add(ctx.item)
        ctx.log.append(len(ctx.batch.launches))  # launches issued by the time this add returns
        return g, None, None, None


class _Boom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("boom")


def _chain(batch, params, log, boom_before=None):
    """loss over a chain of layers; backward visits them last to first.  ``boom_before`` = i: a node that raises sits in front of
    layer i, so the backward pass files the items of the layers from i on, then raises, and never reaches the layers before i."""
    y = torch.ones(2, requires_grad=True)
    for i, ps in enumerate(params):
        if i == boom_before:
            y = _Boom.apply(y)
        y = _Layer.apply(y, batch, _item(batch, *ps), log)
    return y.sum()


def _sinks(group, batch):
    return [batch._dests(it) for it in group]


def test_a_repeated_destination_starts_a_new_launch_and_done_fires_in_item_order_after_all_launches(batches):
    batch = batches("plain")
    a, b, c = (_param(batches.fired) for _ in range(3))
    A, B, C = (p._mm_sink.data_ptr() for p in (a, b, c))
    # backward visits the layers last to first: destinations a, b, a, c, b in item order
    _chain(batch, [(b,), (c,), (a,), (b,), (a,)], []).backward()
    assert [_sinks(g, batch) for g, _ in batch.launches] == [[(A,), (B,)], [(A,), (C,), (B,)]]
    assert [n for _, n in batch.launches] == [0, 0]  # no hook before the last launch
    assert [id(p) for p in batches.fired] == [id(a), id(c), id(b)]  # each once, when its LAST contribution's item is done
    assert all(p._mm_pending == 0 for p in (a, b, c))
    assert batch.items == [] and not batch.cb_queued


def test_a_paired_item_starts_a_new_launch_when_either_destination_repeats(batches):
    batch = batches("plain")
    a, b, c, d = (_param(batches.fired) for _ in range(4))
    A, B, C, D = (p._mm_sink.data_ptr() for p in (a, b, c, d))
    # item order: (a, b), c, (d, b) - its SECOND destination repeats: a new launch, which (a, c) joins (a fresh ``seen`` set)
    _chain(batch, [(a, c), (d, b), (c,), (a, b)], []).backward()
    assert [_sinks(g, batch) for g, _ in batch.launches] == [[(A, B), (C,)], [(D, B), (A, C)]]
    batch.launches.clear()
    # ... and the first destination of a pair: (a, b), (a, c) -> two launches
    _chain(batch, [(a, c), (a, b)], []).backward()
    assert [_sinks(g, batch) for g, _ in batch.launches] == [[(A, B)], [(A, C)]]
    # done in item order, both parameters of a pair, each hook when the parameter's count returns to zero
    assert [id(p) for p in batches.fired] == [id(d), id(b), id(a), id(c), id(b), id(a), id(c)]


def test_one_flush_per_backward_pass(batches):
    batch = batches("plain")
    ps = [_param(batches.fired) for _ in range(3)]
    log = []
    _chain(batch, [(p,) for p in ps], log).backward()
    assert log == [0, 0, 0]  # nothing launched while the pass was running
    assert len(batch.launches) == 1 and len(batch.launches[0][0]) == 3
    _chain(batch, [(p,) for p in ps], log).backward()  # the callback is queued again by the next pass
    assert len(batch.launches) == 2 and len(batch.launches[1][0]) == 3
    assert len(batches.fired) == 6


@pytest.mark.parametrize("kind", ["plain", "early", "dw"])
def test_a_backward_pass_that_raised_after_work_was_queued_is_forgotten_by_reset_deferred(batches, kind):
    batch = batches(kind)
    a, b, c = (_param(batches.fired) for _ in range(3))
    log = []
    with pytest.raises(RuntimeError, match="boom"):
        _chain(batch, [(c,), (a,), (b,)], log, boom_before=1).backward()
    # two adds ran, then a node nearer the leaf raised: the engine dropped the end-of-backward callback
    assert len(batch.items) == 2 and batch.cb_queued and batch.launches == [] and batches.fired == []
    early = kind != "plain"
    if early:
        assert batch.expected == 1  # the first layer went forward, its backward was never reached: the count is offset
    stale = list(batch.items)
    batch.launches.clear()
    batches.fired.clear()
    gradsink.reset_deferred()
    assert batch.items == [] and not batch.cb_queued
    if early:
        assert batch.expected == 0
    for p in (a, b, c):
        p._mm_pending = 0  # FlatAdamW.zero_grad, which calls reset_deferred, also does this
    log.clear()
    _chain(batch, [(a,), (b,)], log).backward()
    assert len(batch.launches) == 1  # exactly one flush ...
    group = batch.launches[0][0]
    assert len(group) == 2 and not any(it is s for it in group for s in stale)  # ... with the new items only
    assert [id(p) for p in batches.fired] == [id(b), id(a)]
    if early:
        assert log == [0, 1]  # the flush came inside the last add, not at the end of the pass


@pytest.mark.parametrize("kind", ["early", "dw"])
def test_without_the_reset_the_early_trigger_never_comes(batches, kind):
    """What the reset is for: the state a raised pass leaves behind, carried into the next pass."""
    batch = batches(kind)
    a, b = _param(batches.fired), _param(batches.fired)
    batch.expected, batch.cb_queued = 1, True  # one forward never saw its backward; the callback was dropped
    log = []
    _chain(batch, [(a,), (b,)], log).backward()
    assert log == [0, 0] and batch.launches == [] and batches.fired == []  # offset count: no early flush; flag set: no callback
    assert len(batch.items) == 2
    batch.reset()
    assert batch.items == [] and not batch.cb_queued and batch.expected == 0


@pytest.mark.parametrize("kind", ["early", "dw"])
def test_early_trigger_flushes_inside_the_last_add_and_the_callback_heals_a_lost_backward(batches, kind):
    batch = batches(kind)
    ps = [_param(batches.fired) for _ in range(3)]
    log = []
    _chain(batch, [(p,) for p in ps], log).backward()
    assert batch.expected == 0
    assert log == [0, 0, 1]  # flushed inside the third add ...
    assert len(batch.launches) == 1 and len(batch.launches[0][0]) == 3  # ... and the end-of-backward flush had nothing left
    assert len(batches.fired) == 3 and not batch.cb_queued
    # a forward that never sees its backward: the early trigger cannot come, the callback flushes and sets the count right
    batch.launches.clear()
    log.clear()
    batch.expected += 1  # what that forward left behind
    _chain(batch, [(p,) for p in ps], log).backward()
    assert log == [0, 0, 0] and len(batch.launches) == 1 and batch.expected == 0
    _chain(batch, [(p,) for p in ps], log).backward()
    assert log[3:] == [1, 1, 2]  # early again


def test_constructing_a_batch_registers_its_reset(batches):
    n = len(gradsink.RESETTERS)
    batch = batches("plain")
    assert len(gradsink.RESETTERS) == n + 1 and gradsink.RESETTERS[-1] == batch.reset
    dw = batches("dw")
    assert gradsink.RESETTERS[-1] == dw.reset
    for b in (conv2d._WGB, ops._DWB):
        assert isinstance(b, gradsink.DeferredSums) and b.reset in gradsink.RESETTERS


def test_affine_helpers_with_and_without_sinks():
    fired = []
    w, b = _param(fired, 5), _param(fired, 5)

    class Ctx:
        pass

    sinks = gradsink.claim_affine(Ctx(), w, b, True)
    assert sinks is not None and sinks[0] is w and sinks[1] is b and (w._mm_pending, b._mm_pending) == (1, 1)
    again = gradsink.claim_affine(Ctx(), w, b, True)  # the second forward of a step
    assert (w._mm_pending, b._mm_pending) == (2, 2)
    dwt, dbt, acc, dw, db = gradsink.affine_targets(sinks, 5, torch.device("cpu"))
    assert dwt.data_ptr() == w._mm_sink.data_ptr() and dbt.data_ptr() == b._mm_sink.data_ptr() and acc == 1 and dw is None and db is None
    gradsink.done_all(sinks)
    assert fired == [] and (w._mm_pending, b._mm_pending) == (1, 1)
    gradsink.done_all(again)
    assert [id(p) for p in fired] == [id(w), id(b)] and (w._mm_pending, b._mm_pending) == (0, 0)

    # nothing claimed: no gradient wanted, no sink on the weight, or no affine parameters at all
    plain = torch.zeros(5, requires_grad=True)
    assert gradsink.claim_affine(Ctx(), w, b, False) is None
    assert gradsink.claim_affine(Ctx(), plain, b, True) is None
    assert gradsink.claim_affine(Ctx(), None, None, True) is None and gradsink.claim_affine(Ctx(), w, None, True) is None
    assert (w._mm_pending, b._mm_pending) == (0, 0)
    gradsink.done_all(None)
    assert len(fired) == 2
    dwt, dbt, acc, dw, db = gradsink.affine_targets(None, 5, torch.device("cpu"))
    assert dwt is dw and dbt is db and acc == 0 and dw is not db
    for t in (dw, db):
        assert t.dtype == torch.float32 and tuple(t.shape) == (5,) and t.data_ptr() not in (w._mm_sink.data_ptr(), b._mm_sink.data_ptr())
    assert gradsink.affine_targets(None, 5, torch.device("cpu"), has_weight=False, has_bias=False) == (None, None, 0, None, None)
    dwt, dbt, acc, dw, db = gradsink.affine_targets(None, 5, torch.device("cpu"), has_bias=False)
    assert dwt is dw and tuple(dw.shape) == (5,) and dbt is None and db is None and acc == 0
