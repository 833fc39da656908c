"""Self-adaptive per-class pseudo-label thresholds in the training step: train_kwargs["pl_threshold"] = "adaptive" with
["pl_threshold_momentum"] / ["pl_threshold_warmup"] (mm2d3d_amd/train.py, pselab.AdaptiveThreshold).  Shapes and helpers of
tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with 48x64 images, 6 classes, fp16, dropout p = 0, ema_decay 0.9;
heads scaled by 4 as in tests/test_gpu_soft_step.py (confidences spread out), and a small momentum so that the thresholds bite
from the first step.

Hard targets: a twin on the batch source, handed the adaptive trainer's labels, stays bit-identical - the update and the
per-class label launch leave nothing else behind.  Soft targets: a stand-alone AdaptiveThreshold fed the step's teacher logits
reproduces the step's thresholds bit for bit, and the rows the loss calls kept are the rows pselab.predict's confidences give."""
import copy

import pytest
import torch

import _step_util as T
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)

pytestmark = pytest.mark.gpu

STEPS = 3
PL_KEYS = ("train/pl_loss_tgt_2d", "train/pl_loss_tgt_3d")
KEPT_KEYS = ("train/pl_kept_2d", "train/pl_kept_3d")
TAU_KEYS = ("train/pl_tau_2d", "train/pl_tau_3d")


def _trainer(n2, n3, **kw):
    _BUILT.append(T._trainer(n2, n3, **kw))
    return _BUILT[-1]


def _adaptive_trainer(n2, n3, **kw):
    return _trainer(n2, n3, lambda_pl=1.0, pseudo_label_source="teacher", pl_threshold="adaptive", **kw)


def _kept_from_predict(l2, l3, thr, ens):
    """Rows with p >= thr[o][y], p and y the float32 confidence and class pselab.predict gives output o."""
    from mm2d3d_amd import pselab

    ref = pselab.predict(l2, l3)
    keys = (("probs_ensemble", "pseudo_label_ensemble"),) * 2 if ens else (("probs_2d", "pseudo_label_2d"), ("probs_3d", "pseudo_label_3d"))
    return [int((ref[pk] >= thr[o][ref[yk].long()]).sum()) for o, (pk, yk) in enumerate(keys)]


TWINS = {
    "joined_own": dict(pseudo_labels="own", pl_threshold_momentum=0.0),
    "joined_ensemble": dict(pseudo_labels="ensemble", pl_threshold_momentum=0.5, pl_threshold_warmup=True),
    "two_calls": dict(pseudo_labels="own", joint_domains=False, pl_threshold_momentum=0.0),
}


@pytest.mark.parametrize("case", list(TWINS))
def test_hard_targets_twin_fed_the_labels_stays_bit_identical(case):
    dev = T._dev()
    kw = TWINS[case]
    shared = {k: v for k, v in kw.items() if not k.startswith("pl_threshold")}
    ens = kw["pseudo_labels"] == "ensemble"
    n2, n3 = T._nets(dev, head_scale=4.0)
    b2, b3 = copy.deepcopy(n2), copy.deepcopy(n3)
    A = _adaptive_trainer(n2, n3, **kw)
    B = _trainer(b2, b3, lambda_pl=1.0, pseudo_label_source="batch", **shared)
    assert A.pl_adaptive is None and B.pl_adaptive is None
    A.configure_optimizers(), B.configure_optimizers()
    batches_a, batches_b = [T._batch(dev) for _ in range(STEPS)], [T._batch(dev) for _ in range(STEPS)]
    for s in range(STEPS):
        torch.manual_seed(100 + s)
        la = A.fit_step(batches_a[s])
        got = {k: v.clone() for k, v in A.last_teacher.items()}
        assert set(got) == {"label_2d", "label_3d", "kept", "threshold"} and all(v.is_cuda for v in got.values())
        n_trg = int(batches_a[s]["target"]["x"][0].shape[0])
        assert got["threshold"].shape == (2, 6) and got["threshold"].dtype == torch.float32
        assert got["label_2d"].shape == (n_trg,) and got["label_2d"].dtype == torch.int64
        kept = [int((got[k] != -100).sum()) for k in ("label_2d", "label_3d")]
        print(f"{case} step {s}: kept {kept} of {n_trg}, thresholds {got['threshold'].tolist()}")
        assert got["kept"].tolist() == kept
        assert A.pl_adaptive is not None and A.pl_adaptive.count.tolist() == [s + 1, s + 1] and A.pl_adaptive.num_classes == 6
        if kw["pl_threshold_momentum"] == 0.0:  # tau is this batch's mean confidence: rows lie on both sides of it
            assert all(0 < k < n_trg for k in kept), kept
        if ens:
            assert torch.equal(got["label_2d"], got["label_3d"]) and torch.equal(got["threshold"][0], got["threshold"][1])
        assert A.model.training and all(m.training for m in A.model.modules()) and A.ema._depth == 0
        trg = batches_b[s]["target"]
        if ens:
            trg["pseudo_label_ensemble"] = got["label_2d"]
        else:
            trg["pseudo_label_2d"], trg["pseudo_label_3d"] = got["label_2d"], got["label_3d"]
        torch.manual_seed(100 + s)
        lb = B.fit_step(batches_b[s])
        assert T._same(la, lb), (case, s, T._f(la), T._f(lb))
        common = [k for k in A.last_logs if k in B.last_logs]
        assert len(common) == 8 and set(PL_KEYS) <= set(common)
        assert set(A.last_logs) - set(common) == set(KEPT_KEYS) | set(TAU_KEYS)
        for k in common:
            assert T._same(A.last_logs[k], B.last_logs[k]), (case, s, k, T._f(A.last_logs[k]), T._f(B.last_logs[k]))
        # the logged share is the labels' kept share, the logged tau this step's state
        for o, k in enumerate(KEPT_KEYS):
            assert A.last_logs[k].is_cuda and T._f(A.last_logs[k]) == T._f(torch.tensor(kept[o], dtype=torch.float32, device=dev) / n_trg)
        for o, k in enumerate(TAU_KEYS):
            assert A.last_logs[k].is_cuda and A.last_logs[k].dim() == 0
            assert T._f(A.last_logs[k]) == float(A.pl_adaptive.state[o, 0].to(torch.float32))
    torch.cuda.synchronize()
    T._assert_same_dicts(A.model.state_dict(), B.model.state_dict(), case)
    T._assert_same_dicts(A.ema.teacher_state_dict(), B.ema.teacher_state_dict(), case + " teacher")
    assert B.pl_adaptive is None and "pl_adaptive" not in B.checkpoint() and set(A.checkpoint()["pl_adaptive"]) == {"num_classes", "state", "count"}


@pytest.mark.parametrize("case", ["joined_own", "joined_ensemble", "two_calls"])
def test_soft_targets_thresholds_are_a_stand_alone_objects(case):
    from mm2d3d_amd import pselab

    dev = T._dev()
    kw = TWINS[case]
    ens = kw["pseudo_labels"] == "ensemble"
    A = _adaptive_trainer(*T._nets(dev, head_scale=4.0), pl_targets="soft", pl_temperature=2.0, **kw)
    alone = pselab.AdaptiveThreshold(6, momentum=kw["pl_threshold_momentum"], warmup=kw.get("pl_threshold_warmup", False), device=dev)
    for s in range(STEPS):
        A.fit_step(T._batch(dev))
        got = A.last_teacher
        assert set(got) == {"logit_2d", "logit_3d", "kept", "threshold"}
        n_trg = int(got["logit_2d"].shape[0])
        thr = alone.update(got["logit_2d"], got["logit_3d"], ensemble=ens)
        assert T._same(thr, got["threshold"]), (case, s)
        assert torch.equal(alone.state.view(torch.int64), A.pl_adaptive.state.view(torch.int64)) and torch.equal(alone.count, A.pl_adaptive.count)
        want = _kept_from_predict(got["logit_2d"], got["logit_3d"], got["threshold"], ens)
        print(f"{case} step {s}: kept {got['kept'].tolist()} of {n_trg}, thresholds {got['threshold'].tolist()}")
        assert got["kept"].tolist() == want
        if kw["pl_threshold_momentum"] == 0.0:
            assert all(0 < k < n_trg for k in want), want
        for o, k in enumerate(KEPT_KEYS):
            assert T._f(A.last_logs[k]) == T._f(torch.tensor(want[o], dtype=torch.float32, device=dev) / n_trg)
        for o, k in enumerate(TAU_KEYS):
            assert T._f(A.last_logs[k]) == float(alone.state[o, 0].to(torch.float32))
        assert all(torch.isfinite(A.last_logs[k]) for k in PL_KEYS)


@pytest.mark.parametrize("targets", ["hard", "soft"])
def test_checkpoint_round_trip_resumes_the_thresholds(targets):
    dev = T._dev()
    kw = dict(pl_targets=targets, pl_threshold_momentum=0.5, pl_threshold_warmup=True)
    n2, n3 = T._nets(dev, head_scale=4.0)
    f2, f3 = copy.deepcopy(n2), copy.deepcopy(n3)
    A = _adaptive_trainer(n2, n3, **kw)
    for _ in range(2):
        A.fit_step(T._batch(dev))
    ck = A.checkpoint()
    assert ck["pl_adaptive"]["state"].data_ptr() != A.pl_adaptive.state.data_ptr() and ck["pl_adaptive"]["count"].tolist() == [2, 2]
    C = _adaptive_trainer(f2, f3, **kw)
    C.load_checkpoint(ck)
    assert C.pl_adaptive is not None  # built from the checkpoint: no teacher pass has run in this trainer
    assert torch.equal(C.pl_adaptive.state.view(torch.int64), A.pl_adaptive.state.view(torch.int64)) and C.pl_adaptive.count.tolist() == [2, 2]
    la, lc = A.fit_step(T._batch(dev)), C.fit_step(T._batch(dev))
    torch.cuda.synchronize()
    assert T._same(A.last_teacher["threshold"], C.last_teacher["threshold"])
    assert torch.equal(C.pl_adaptive.state.view(torch.int64), A.pl_adaptive.state.view(torch.int64)) and C.pl_adaptive.count.tolist() == [3, 3]
    assert T._same(A.last_teacher["kept"], C.last_teacher["kept"]) and T._same(la, lc)
    # a checkpoint without the key: the thresholds start over
    C.load_checkpoint({k: v for k, v in ck.items() if k != "pl_adaptive"})
    assert torch.equal(C.pl_adaptive.state, torch.full((2, 7), 1.0 / 6, dtype=torch.float64, device=dev)) and C.pl_adaptive.count.tolist() == [0, 0]


def test_lambda_pl_zero_builds_and_launches_nothing():
    dev = T._dev()
    tm = _trainer(*T._nets(dev), lambda_pl=0.0, pseudo_label_source="teacher", pl_threshold="adaptive")
    plain = _trainer(*T._nets(dev))
    la, lb = tm.fit_step(T._batch(dev)), plain.fit_step(T._batch(dev))
    assert tm.pl_adaptive is None and tm.last_teacher is None and "pl_adaptive" not in tm.checkpoint()
    assert T._same(la, lb) and list(tm.last_logs) == list(plain.last_logs)
