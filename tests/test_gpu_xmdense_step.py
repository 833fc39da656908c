"""Sparse-to-dense cross-modal matching in the training step: train_kwargs["xm_window"] (mm2d3d_amd/xmdense.py,
losses.cross_modal_dense, lifting.lift_at).  Shapes and helpers of tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with 48x64
images, 6 classes, fp16, dropout p = 0.  The matched terms are held to ``kl_to_detached`` on rows gathered at the logged selection
from the maps and rows the heads produced in that very step (forward hooks): the same kernels on the same values, so the same bits;
tests/test_gpu_xmdense.py holds the search itself to the float64 reference."""
import copy
import socket

import pytest
import torch

import _step_util as T
import _xmdense_ref as R
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)
from test_gpu_xmdense import _room_on_the_device  # noqa: F401  (module-scoped, autouse: once more before this module's first test)

pytestmark = pytest.mark.gpu

OLD_KEYS = ("train/loss_segmentation", "train/loss_segmentation_3d", "train/xm_loss_src_2d", "train/xm_loss_tgt_2d", "train/xm_loss_src_3d",
            "train/xm_loss_tgt_3d")
NEW_KEYS = ("train/xm_moved_2d", "train/xm_shift_2d", "train/xm_moved_3d", "train/xm_shift_3d")
BINDINGS = ("mm_xm_search_ws_bytes", "mm_xm_search", "mm_lift_sort_keys")


def _trainer(n2, n3, **kw):
    _BUILT.append(T._trainer(n2, n3, **kw))
    return _BUILT[-1]


class _CountCalls:
    """Counts the entries into the new bindings of the loaded library."""

    def __init__(self, monkeypatch):
        from mm2d3d_amd import _lib

        L = _lib.lib()
        self.n = {}
        for name in BINDINGS:
            self.n[name] = 0
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)

        return call


def _hook(tm):
    """What the heads produced in every forward of the two networks, in call order: the two dense maps and the lifted main rows of
    the 2D network, the main and the aux rows of the 3D network - copies, kept on the device."""
    seen = {"2d_net": [], "3d_net": []}
    keep = lambda t: t.detach().clone()
    tm.model["2d_net"].register_forward_hook(lambda m, i, out: seen["2d_net"].append(
        dict(main=keep(out[0]["seg_logit_2d"]), avg=keep(out[3]["seg_logit_avg_2d"]), rows=keep(out[0]["seg_logit"]))))
    tm.model["3d_net"].register_forward_hook(lambda m, i, out: seen["3d_net"].append(
        dict(main=keep(out[0]["seg_logit"]), aux=keep(out[2]["seg_logit_point"]))))
    return seen


def _at(dense, key):
    """Rows of a [B, C, H, W] map at pixel keys."""
    return dense.permute(0, 2, 3, 1).reshape(-1, dense.shape[1])[key.long()].contiguous()


def _check_matched_terms(tm, seen, P, joint, plain_logs):
    """Every logged xm_loss_* is kl_to_detached on the rows gathered at last_match's selection, bit for bit, and does not exceed the
    plain term of the twin by more than the two kernels' float32 rounding (2 x the per-row bound of tests/test_gpu_xmdense.py)."""
    from mm2d3d_amd.losses import kl_to_detached

    m = tm.last_match
    N = int(m["sel_2d"].shape[0])
    assert set(m) == {"sel_2d", "sel_3d", "klmin_2d", "klmin_3d", "moved", "shift", "split"} and m["split"] == P and 0 < P < N
    assert all(m[k].is_cuda and m[k].shape == (N,) for k in ("sel_2d", "sel_3d", "klmin_2d", "klmin_3d"))
    assert m["moved"].shape == m["shift"].shape == (2, 2) and m["moved"].dtype == torch.int64 and m["moved"].is_cuda
    assert len(seen["2d_net"]) == len(seen["3d_net"]) == (1 if joint else 2)
    for tag, (lo, hi) in (("src", (0, P)), ("tgt", (P, N))):
        call = 0 if joint or tag == "src" else 1
        d2, d3 = seen["2d_net"][call], seen["3d_net"][call]
        rows = slice(lo, hi) if joint else slice(None)  # the two calls hold one domain each
        want_2d = kl_to_detached(_at(d2["avg"], m["sel_2d"][lo:hi]), d3["main"][rows])
        want_3d = kl_to_detached(d3["aux"][rows], _at(d2["main"], m["sel_3d"][lo:hi]))
        for d, want in (("2d", want_2d), ("3d", want_3d)):
            got, plain = tm.last_logs[f"train/xm_loss_{tag}_{d}"], T._f(plain_logs[f"train/xm_loss_{tag}_{d}"])
            print(f"xm_loss_{tag}_{d}: matched {T._f(got):.7g}, plain {plain:.7g}")
            assert T._same(got, want), (tag, d)
            assert 0.0 <= T._f(got) <= plain + 2 * R.KLMIN_BOUND * (1.0 + plain)
        # the search's own row values: their mean is the logged term up to the two kernels' rounding
        for d, want in (("2d", want_2d), ("3d", want_3d)):
            mean = float(m[f"klmin_{d}"][lo:hi].double().mean())
            assert abs(mean - T._f(want)) <= 2 * R.KLMIN_BOUND * (1.0 + mean)
    n_moved = m["moved"].sum(1).tolist()
    for i, d in enumerate(("2d", "3d")):
        moved, shift = T._f(tm.last_logs[f"train/xm_moved_{d}"]), T._f(tm.last_logs[f"train/xm_shift_{d}"])
        print(f"{d}: {moved:.4f} of the rows matched off-centre, mean displacement {shift:.4f}")
        assert 0.0 <= moved <= 1.0 and abs(moved - n_moved[i] / N) < 1e-6
        assert (1.0 <= shift <= tm.xm_window) if n_moved[i] else shift == 0.0
    assert sum(n_moved) > 0  # random heads: some point finds a better pixel next door


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_window_zero_is_the_step_without_the_option(monkeypatch, joint):
    dev = T._dev()
    n2, n3 = T._nets(dev)
    A = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), joint_domains=joint)
    B = _trainer(n2, n3, joint_domains=joint, xm_window=0)
    calls = _CountCalls(monkeypatch)
    for s in range(2):
        la, lb = A.fit_step(T._batch(dev)), B.fit_step(T._batch(dev))
        assert T._same(la, lb), s
        assert list(A.last_logs) == list(B.last_logs) == list(OLD_KEYS)
        T._assert_same_dicts(A.last_logs, B.last_logs, f"logs of step {s}")
    torch.cuda.synchronize()
    T._assert_same_dicts(A.model.state_dict(), B.model.state_dict(), "weights and running statistics")
    assert A.last_match is None and B.last_match is None
    assert calls.n == {name: 0 for name in BINDINGS}
    # the counter counts: the same trainer with the window opened enters the bindings - two searches, one sort per matched lift
    B.xm_window = 2
    B.fit_step(T._batch(dev))
    assert calls.n["mm_xm_search"] == (2 if joint else 4) and calls.n["mm_lift_sort_keys"] == (1 if joint else 2)
    assert B.last_match is not None and "train/xm_moved_2d" in B.last_logs


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_window_two_matches_every_point_and_logs_the_matched_terms(joint):
    dev = T._dev()
    n2, n3 = T._nets(dev, head_scale=8.0)
    off = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), joint_domains=joint)
    tm = _trainer(n2, n3, joint_domains=joint, xm_window=2)
    seen = _hook(tm)
    batch = T._batch(dev)
    P = int(batch["source"]["x"][0].shape[0])
    loss, base = tm.fit_step(batch), off.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    assert list(tm.last_logs) == list(OLD_KEYS) + list(NEW_KEYS) and all(v.is_cuda and v.dim() == 0 for v in tm.last_logs.values())
    for k in OLD_KEYS[:2]:
        assert T._same(tm.last_logs[k], off.last_logs[k]), k
    _check_matched_terms(tm, seen, P, joint, off.last_logs)
    assert T._f(loss) <= T._f(base) * (1 + 1e-5) and T._f(loss) == T._f(loss)
    # the step learnt something else than the twin's, and nothing broke
    differ = 0
    for (k, a), (_, b) in zip(tm.model.state_dict().items(), off.model.state_dict().items()):
        assert torch.isfinite(a.float()).all(), k
        differ += int(not T._same(a, b))
    assert differ > 100


def test_composes_with_pseudo_labels_and_minent():
    dev = T._dev()

    def batch():
        b = T._batch(dev)
        n = int(b["target"]["x"][0].shape[0])
        g = torch.Generator().manual_seed(5)
        for k in ("pseudo_label_2d", "pseudo_label_3d"):
            y = torch.randint(0, 6, (n,), generator=g)
            y[torch.rand(n, generator=g) < 0.5] = -100
            b["target"][k] = y.to(dev)
        return b

    others = dict(lambda_pl=0.5, lambda_minent=0.3)
    n2, n3 = T._nets(dev, head_scale=8.0)
    plain = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), **others)
    both = _trainer(n2, n3, xm_window=2, **others)
    seen = _hook(both)
    b = batch()
    P = int(b["source"]["x"][0].shape[0])
    la, lb = plain.fit_step(batch()), both.fit_step(b)
    torch.cuda.synchronize()
    assert [k for k in both.last_logs if k not in NEW_KEYS] == list(plain.last_logs) and set(NEW_KEYS) <= set(both.last_logs)
    extra = [k for k in plain.last_logs if k not in OLD_KEYS]
    assert len(extra) >= 3  # the pseudo-label terms and the entropy terms
    for k in list(OLD_KEYS[:2]) + extra:  # every other term unchanged in every bit
        assert T._same(both.last_logs[k], plain.last_logs[k]), k
    _check_matched_terms(both, seen, P, True, plain.last_logs)
    assert T._f(lb) == T._f(lb) and T._f(lb) <= T._f(la) * (1 + 1e-5)


def test_teacher_and_evaluation_passes_never_match(monkeypatch):
    """The mean teacher labels the target batch in a pass of its own inside the step, and validation, test and ``predict_step`` run
    the networks too: the only entries into the search are the two of the student's joined pass."""
    dev = T._dev()
    tm = _trainer(*T._nets(dev), xm_window=2, lambda_pl=1.0, pseudo_label_source="teacher")
    calls = _CountCalls(monkeypatch)
    tm.fit_step(T._batch(dev))
    assert calls.n["mm_xm_search"] == 2 and calls.n["mm_lift_sort_keys"] == 1 and tm.last_teacher is not None
    match = tm.last_match
    tm.validation_step(T._batch(dev)["source"])
    tm.test_step(T._batch(dev)["source"])
    tm.predict_step(T._batch(dev)["target"])
    tm.model.train()
    torch.cuda.synchronize()
    assert calls.n["mm_xm_search"] == 2 and calls.n["mm_lift_sort_keys"] == 1 and tm.last_match is match
    assert not any("xm_" in k for k in tm.last_logs)


def test_works_with_exact_fp32_maps():
    """``precision: 32``: the two dense maps are stand-alone NCHW tensors, not the halves of one NHWC buffer."""
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    dev = T._dev()

    def trainer(n2, n3, **kw):
        tm = TrainModel({"2d_net": n2, "3d_net": n3}, {k: Optimizer("adamw", lr=1e-3) for k in ("2d_net", "3d_net")}, Loss(T.CE),
                        dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, precision=32, **kw))
        _BUILT.append(tm)
        return tm

    n2, n3 = T._nets(dev, head_scale=8.0)
    off, tm = trainer(copy.deepcopy(n2), copy.deepcopy(n3)), trainer(n2, n3, xm_window=2)
    seen = _hook(tm)
    batch = T._batch(dev)
    P = int(batch["source"]["x"][0].shape[0])
    tm.fit_step(batch), off.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    assert seen["2d_net"][0]["avg"].dtype == torch.float32
    assert list(tm.last_logs) == list(OLD_KEYS) + list(NEW_KEYS)
    for k in OLD_KEYS[:2]:
        assert T._same(tm.last_logs[k], off.last_logs[k]), k
    _check_matched_terms(tm, seen, P, True, off.last_logs)
    assert not T._same(tm.model["2d_net"].aux.con1_1_avg.weight, off.model["2d_net"].aux.con1_1_avg.weight)
    assert all(torch.isfinite(v.float()).all() for v in tm.model.state_dict().values())


def test_works_under_a_forced_one_rank_reducer(monkeypatch):
    """A pure loss: nothing of it is reduced over ranks.  The reducer forced on in a process group of one rank, as
    tests/test_gpu_clip_step.py runs it: the matched step equals the matched step without the reducer, bit for bit."""
    import torch.distributed as dist

    from mm2d3d_amd import conv2d as _c2d

    dev = T._dev()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    was = _c2d.WGRAD_BATCH[0]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        n2, n3 = T._nets(dev, head_scale=8.0)
        tk = dict(bn2d_fused=0, bn3d_fused=0, xm_window=2)  # both on the three-kernel batch norms (what the reducer selects)
        monkeypatch.setenv("MM_DDP_FORCE", "1")
        ddp = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), **tk)
        ddp.configure_optimizers()
        monkeypatch.setenv("MM_DDP_FORCE", "0")
        plain = _trainer(n2, n3, **tk)
        plain.configure_optimizers()
        assert ddp.reducer.active and not plain.reducer.active
        for step in range(2):
            la, lb = ddp.fit_step(T._batch(dev)), plain.fit_step(T._batch(dev))
            torch.cuda.synchronize()
            assert T._f(la) == T._f(lb), (step, T._f(la), T._f(lb))
            T._assert_same_dicts(ddp.last_logs, plain.last_logs, f"logs of step {step}")
            assert torch.equal(ddp.last_match["sel_2d"], plain.last_match["sel_2d"])
        T._assert_same_dicts(ddp.model.state_dict(), plain.model.state_dict(), "weights and running statistics")
    finally:
        dist.destroy_process_group()
        _c2d.WGRAD_BATCH[0] = was


def test_captured_trunk_agrees_with_the_eager_trunk_on_the_aux_head():
    """With the 2D trunk replayed as HIP graphs the matched lift's backward writes the aux half of the graph's static gradient buffer
    and files its per-channel sum for the head's bias: after steps on both sides of the capture the aux head's weight AND bias, and
    everything else, equal the eager twin's bit for bit - the agreement tests/test_gpu_graph2d.py demands of graph against eager."""
    from mm2d3d_amd import graph2d

    dev = T._dev()
    n2, n3 = T._nets(dev, head_scale=8.0)
    steps = graph2d.WARMUP_CALLS + 3
    was = graph2d.ENABLED[0]
    try:
        graph2d.ENABLED[0] = True
        ga = _trainer(n2, n3, xm_window=2)
        la = [T._f(ga.fit_step(T._batch(dev))) for _ in range(steps)]
        st = graph2d._STATE.get(id(ga.model["2d_net"]))
        assert st is not None and len(st["graphs"]) == 1, "the trunk was not captured"
        graph2d.ENABLED[0] = False
        n2b, n3b = T._nets(dev, head_scale=8.0)
        eb = _trainer(n2b, n3b, xm_window=2)
        lb = [T._f(eb.fit_step(T._batch(dev))) for _ in range(steps)]
        torch.cuda.synchronize()
        assert la == lb, (la, lb)
        ha, hb = ga.model["2d_net"].aux.con1_1_avg, eb.model["2d_net"].aux.con1_1_avg
        assert T._same(ha.weight, hb.weight) and T._same(ha.bias, hb.bias)
        assert not T._same(ha.bias, T._nets(dev, head_scale=8.0)[0].aux.con1_1_avg.bias)  # the bias did move
        T._assert_same_dicts(ga.model.state_dict(), eb.model.state_dict(), "weights and running statistics")
        T._assert_same_dicts(ga.last_logs, eb.last_logs, "logs of the last step")
    finally:
        graph2d.ENABLED[0] = was
        graph2d.reset()
