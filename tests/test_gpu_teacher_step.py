"""The mean teacher labels the target batch inside the step: train_kwargs["pseudo_label_source"] = "teacher" and ["pl_threshold"]
(mm2d3d_amd/train.py).  Shapes of tests/test_gpu_ema.py: 1 + 1 synthetic nuScenes scenes with 48x64 images, 6 classes, fp16,
dropout p = 0.

The main check is a twin: trainer A labels its target batch itself, trainer B (the same nets, seed and ``ema_decay``) is handed A's
labels as the batch's ``pseudo_label_*`` keys.  If the teacher pass leaves anything behind - a running statistic, a gated feature
row, a stale packed weight, a dropout draw - the two part ways; they must stay equal bit for bit."""
import copy

import numpy as np
import pytest
import torch

from _step_util import _alone_logits, _assert_same_dicts, _batch, _dev, _f, _nets, _restore_precision, _same, _trainer  # noqa: F401  (_restore_precision: the autouse fixture, for this module too)

pytestmark = pytest.mark.gpu

STEPS = 3
PL_KEYS = ("train/pl_loss_tgt_2d", "train/pl_loss_tgt_3d")
KEPT_KEYS = ("train/pl_kept_2d", "train/pl_kept_3d")


def _teacher_trainer(n2, n3, **kw):
    return _trainer(n2, n3, lambda_pl=1.0, pseudo_label_source="teacher", **kw)


def _gap64(logits):
    """float64 gap between the two largest softmax probabilities of every row."""
    x = logits.detach().cpu().double().numpy()
    e = np.exp(x - x.max(1, keepdims=True))
    p = np.sort(e / e.sum(1, keepdims=True), axis=1)
    return p[:, -1] - p[:, -2]


# ---------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("case", ["joined_own", "joined_ensemble", "two_calls", "prefetched"])
def test_twin_fed_the_teachers_labels_stays_bit_identical(case):
    dev = _dev()
    kw = dict(pseudo_labels="ensemble" if case == "joined_ensemble" else "own", joint_domains=case != "two_calls")
    n2, n3 = _nets(dev)
    b2, b3 = copy.deepcopy(n2), copy.deepcopy(n3)
    A = _teacher_trainer(n2, n3, **kw)
    B = _trainer(b2, b3, lambda_pl=1.0, pseudo_label_source="batch", **kw)
    A.configure_optimizers(), B.configure_optimizers()
    ptrs = [p.data_ptr() for p in A.model.parameters()] + [b.data_ptr() for b in A.model.buffers()]
    ahead = case == "prefetched"
    batches_a = [_batch(dev) for _ in range(STEPS)]
    batches_b = [_batch(dev) for _ in range(STEPS)]
    for s in range(STEPS):
        nxt = dict(next_batch=batches_a[s + 1]) if ahead and s + 1 < STEPS else {}
        torch.manual_seed(100 + s)
        la = A.fit_step(batches_a[s], **nxt)
        labels = {k: v.clone() for k, v in A.last_teacher.items()}
        assert set(labels) == {"label_2d", "label_3d", "kept"} and all(v.is_cuda for v in labels.values())
        n_trg = int(batches_a[s]["target"]["x"][0].shape[0])
        assert labels["label_2d"].shape == (n_trg,) and labels["label_2d"].dtype == torch.int64
        assert labels["kept"].tolist() == [n_trg, n_trg]  # no threshold: every label is kept
        if kw["pseudo_labels"] == "ensemble":
            assert torch.equal(labels["label_2d"], labels["label_3d"])
        # the model is the student's again
        assert A.model.training and all(m.training for m in A.model.modules()) and A.ema._depth == 0
        assert [p.data_ptr() for p in A.model.parameters()] + [b.data_ptr() for b in A.model.buffers()] == ptrs
        trg = batches_b[s]["target"]
        if kw["pseudo_labels"] == "ensemble":
            trg["pseudo_label_ensemble"] = labels["label_2d"]
        else:
            trg["pseudo_label_2d"], trg["pseudo_label_3d"] = labels["label_2d"], labels["label_3d"]
        nxt = dict(next_batch=batches_b[s + 1]) if ahead and s + 1 < STEPS else {}
        torch.manual_seed(100 + s)
        lb = B.fit_step(batches_b[s], **nxt)
        assert _same(la, lb), (case, s, _f(la), _f(lb))
        common = [k for k in A.last_logs if k in B.last_logs]
        assert len(common) == 8 and set(PL_KEYS) <= set(common) and set(A.last_logs) - set(common) == set(KEPT_KEYS)
        for k in common:
            assert _same(A.last_logs[k], B.last_logs[k]), (case, s, k, _f(A.last_logs[k]), _f(B.last_logs[k]))
        assert all(_f(A.last_logs[k]) == 1.0 for k in KEPT_KEYS)
    torch.cuda.synchronize()
    assert all(np.isfinite(_f(A.last_logs[k])) and _f(A.last_logs[k]) > 0.0 for k in PL_KEYS)
    # weights, running statistics and num_batches_tracked moved exactly as in B: the teacher pass updated nothing
    _assert_same_dicts(A.model.state_dict(), B.model.state_dict(), case)
    _assert_same_dicts(A.ema.teacher_state_dict(), B.ema.teacher_state_dict(), case + " teacher")
    assert int(A.optimizers[0].step_counter().item()) == int(B.optimizers[0].step_counter().item())
    nbt = [int(v) for k, v in A.model.state_dict().items() if k.endswith("num_batches_tracked")]
    assert nbt and max(nbt) <= 2 * STEPS  # the student's own forwards only: source and target once per step


# ---------------------------------------------------------------------------------------------- whose labels they are
def test_two_call_labels_are_the_teachers_and_not_the_students():
    from mm2d3d_amd import pselab

    dev = _dev()
    n2, n3 = _nets(dev, head_scale=4.0)
    tm = _teacher_trainer(n2, n3, lr=1e-2, joint_domains=False)
    for _ in range(2):
        tm.fit_step(_batch(dev))
    assert int(tm.optimizers[0].step_counter().item()) >= 1  # the student has moved away from the teacher
    l2, l3 = _alone_logits(tm, dev)
    want = pselab.teacher_labels(l2, l3)
    # the student's labels of the same batch, for contrast
    trg = _batch(dev)["target"]
    with torch.no_grad(), tm._use():
        tm.model.eval()
        student = pselab.teacher_labels(tm(trg, model_name="2d_net")[0]["seg_logit"], tm(trg, model_name="3d_net")[0]["seg_logit"])
    tm.model.train()
    tm.fit_step(_batch(dev))
    got = tm.last_teacher
    torch.cuda.synchronize()
    assert torch.equal(got["label_2d"], want["label_2d"]) and torch.equal(got["label_3d"], want["label_3d"])
    differ = [int((student[k] != want[k]).sum()) for k in ("label_2d", "label_3d")]
    print(f"rows on which teacher and student disagree: 2D {differ[0]}, 3D {differ[1]} of {want['label_2d'].numel()}")
    # With these nets the 3D argmax differs on 2291 of 34880 rows and the 2D argmax on none: the random-init 2D net gives every
    # pixel one class.  The 2D side is made to tell rows apart by the confidence cut of the next test.
    assert differ[0] + differ[1] > 0


@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_median_cut_tells_the_2d_rows_apart_and_is_the_teachers_on_the_target_images(joint):
    """pl_threshold="median" keeps a row or not by its own confidence, so label_2d varies from row to row also where the argmax
    is one class everywhere.  The 2D branch of the teacher pass runs on the target images alone on both step paths: its labels
    equal the alone forward's exactly, differ from the student's, and differ from what the SOURCE images would have given."""
    from mm2d3d_amd import pselab

    dev = _dev()
    # a SMALL 2D head: with the plain (or a larger) one the 2D softmax of these nets saturates at 1.0 on every row (36 distinct
    # confidences over 34880 rows were measured) and no cut by confidence can tell rows apart
    n2, n3 = _nets(dev, head_scale=4.0, head_scale_2d=0.02)
    tm = _teacher_trainer(n2, n3, joint_domains=joint, pl_threshold="median")
    for _ in range(2):
        tm.fit_step(_batch(dev))
    assert int(tm.optimizers[0].step_counter().item()) >= 1

    def refined(l2, l3):
        r = pselab.teacher_labels(l2, l3, with_probs=True)
        return [pselab.refine_pseudo_labels(r[f"prob_{o}"], r[f"label_{o}"], num_classes=6, device=dev) for o in ("2d", "3d")], r

    l2, l3 = _alone_logits(tm, dev)
    want, ref = refined(l2, l3)
    n = want[0].numel()
    print(f"joint {joint}: {ref['prob_2d'].unique().numel()} distinct 2D confidences in [{float(ref['prob_2d'].min()):.6f}, "
          f"{float(ref['prob_2d'].max()):.6f}], {ref['label_2d'].unique().numel()} 2D classes")
    assert ref["prob_2d"].unique().numel() > n // 100  # the confidences do vary over the rows
    b = _batch(dev)
    wrong_images = dict(b["target"], img=b["source"]["img"], depth=b["source"]["depth"])  # the target's points on the source's images
    with torch.no_grad(), tm._use():
        tm.model.eval()
        s2 = tm(_batch(dev)["target"], model_name="2d_net")[0]["seg_logit"].clone()
        s3 = tm(_batch(dev)["target"], model_name="3d_net")[0]["seg_logit"].clone()
        with tm.ema.applied():
            w2 = tm(wrong_images, model_name="2d_net")[0]["seg_logit"].clone()
    tm.model.train()
    student, _ = refined(s2, s3)
    wrong, _ = refined(w2, l3)
    tm.fit_step(_batch(dev))
    got = tm.last_teacher
    torch.cuda.synchronize()
    kept2d = int((want[0] != -100).sum())
    differ = [int((student[j] != want[j]).sum()) for j in range(2)]
    print(f"joint {joint}: 2D kept {kept2d} of {n}; teacher and student differ on 2D {differ[0]}, 3D {differ[1]} rows; "
          f"source images would differ on {int((wrong[0] != want[0]).sum())} 2D rows")
    assert 0 < kept2d < n
    assert torch.equal(got["label_2d"], want[0])
    assert int(got["kept"][0]) == kept2d and _f(tm.last_logs["train/pl_kept_2d"]) == float(torch.tensor(kept2d, dtype=torch.float32) / n)
    # measured: about half of the 34880 rows kept; teacher and student differ on 22413 2D and 4371 3D rows; the source's images
    # would change 11136 2D rows
    assert differ[0] > 0 and differ[1] > 0  # per head: these are the teacher's labels, not the student's
    assert int((wrong[0] != want[0]).sum()) > 0  # and the teacher saw the target's images, not the source's
    if not joint:  # the 3D rows too are computed alone on this path
        assert torch.equal(got["label_3d"], want[1])


@pytest.mark.parametrize("mode", ["own", "ensemble"])
def test_joined_labels_equal_the_alone_forward_where_the_gap_is_clear(mode):
    """In the joined pass the target's 3D rows are computed inside a larger batch (another engine may be chosen): equal wherever
    the alone forward's float64 top-two gap is >= 1e-4; at most 5 % of the rows may fall below that, checked first."""
    from mm2d3d_amd import pselab

    dev = _dev()
    n2, n3 = _nets(dev, head_scale=4.0)
    tm = _teacher_trainer(n2, n3, lr=1e-2, pseudo_labels=mode)
    for _ in range(2):
        tm.fit_step(_batch(dev))
    l2, l3 = _alone_logits(tm, dev)
    want = pselab.teacher_labels(l2, l3, ensemble=mode == "ensemble", with_probs=True)
    if mode == "ensemble":
        x2, x3 = l2.cpu().double().numpy(), l3.cpu().double().numpy()
        sm = lambda x: np.exp(x - x.max(1, keepdims=True)) / np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)
        p = np.sort(0.5 * (sm(x2) + sm(x3)), axis=1)
        gaps = [p[:, -1] - p[:, -2]] * 2
    else:
        gaps = [_gap64(l2), _gap64(l3)]
    unclear = [g < 1e-4 for g in gaps]
    print(f"{mode}: rows below the gap: 2D {int(unclear[0].sum())}, 3D {int(unclear[1].sum())} of {len(gaps[0])}")
    assert all(u.mean() <= 0.05 for u in unclear)
    tm.fit_step(_batch(dev))
    got = tm.last_teacher
    torch.cuda.synchronize()
    for k, u in zip(("label_2d", "label_3d"), unclear):
        g, w = got[k].cpu().numpy(), want[k].cpu().numpy()
        assert np.array_equal(g[~u], w[~u]), (mode, k, int((g != w)[~u].sum()))
    if mode == "own":  # the 2D branch runs on the target images alone in both: the same kernels on the same numbers
        assert torch.equal(got["label_2d"], want["label_2d"])


# ---------------------------------------------------------------------------------------------- thresholds
@pytest.mark.parametrize("mode", ["own", "ensemble"])
def test_fixed_threshold_and_median_rule(mode):
    from mm2d3d_amd import pselab

    dev = _dev()
    n2, n3 = _nets(dev, head_scale=4.0)
    fresh = [(copy.deepcopy(n2), copy.deepcopy(n3)) for _ in range(2)]
    ens = mode == "ensemble"
    # the first step's teacher is the initial weights: the alone forward of any of these trainers, before its step
    tm = _teacher_trainer(n2, n3, joint_domains=False, pseudo_labels=mode, pl_threshold=0.9)
    tm.configure_optimizers()
    l2, l3 = _alone_logits(tm, dev)
    ref = pselab.teacher_labels(l2, l3, ensemble=ens, with_probs=True)
    n = ref["label_2d"].numel()
    thr = torch.tensor(0.9, dtype=torch.float32, device=dev)
    loss = tm.fit_step(_batch(dev))
    for j, out in enumerate(("2d", "3d")):
        want = torch.where(ref[f"prob_{out}"] >= thr, ref[f"label_{out}"], torch.full_like(ref[f"label_{out}"], -100))
        assert torch.equal(tm.last_teacher[f"label_{out}"], want), out
        kept = int((want != -100).sum())
        print(f"{mode} 0.9: {kept} of {n} {out} labels kept")
        assert int(tm.last_teacher["kept"][j]) == kept
        share = tm.last_logs[f"train/pl_kept_{out}"]
        assert share.is_cuda and float(share) == float(torch.tensor(kept, dtype=torch.float32) / n)
    assert np.isfinite(_f(loss))
    # "median": the loaders' refinement of the unthresholded labels and confidences of this batch
    med = _teacher_trainer(*fresh[0], joint_domains=False, pseudo_labels=mode, pl_threshold="median")
    loss = med.fit_step(_batch(dev))
    for j, out in enumerate(("2d", "3d")):
        want = pselab.refine_pseudo_labels(ref[f"prob_{out}"], ref[f"label_{out}"], num_classes=6, device=dev)
        assert torch.equal(med.last_teacher[f"label_{out}"], want), out
        kept = int((want != -100).sum())
        print(f"{mode} median: {kept} of {n} {out} labels kept")
        assert 0 < kept < n and int(med.last_teacher["kept"][j]) == kept
        assert _f(med.last_logs[f"train/pl_kept_{out}"]) == float(torch.tensor(kept, dtype=torch.float32) / n)
    assert np.isfinite(_f(loss)) and all(_f(med.last_logs[k]) > 0.0 for k in PL_KEYS)
    # every label refused: the terms are 0 (not 0/0) and the step is finite
    none = _teacher_trainer(*fresh[1], pseudo_labels=mode, pl_threshold=1.0)
    loss = none.fit_step(_batch(dev))
    torch.cuda.synchronize()
    assert float(ref["prob_2d"].max()) < 1.0 and float(ref["prob_3d"].max()) < 1.0  # non-degenerate logits
    assert none.last_teacher["kept"].tolist() == [0, 0] and bool((none.last_teacher["label_2d"] == -100).all())
    assert all(_f(none.last_logs[k]) == 0.0 for k in PL_KEYS + KEPT_KEYS)
    assert np.isfinite(_f(loss)) and all(bool(torch.isfinite(p).all()) for p in none.model.parameters())


# ---------------------------------------------------------------------------------------------- switched off, and skipped steps
def test_teacher_source_with_lambda_pl_zero_is_the_step_without_the_option():
    dev = _dev()
    n2, n3 = _nets(dev)
    plain = _trainer(copy.deepcopy(n2), copy.deepcopy(n3))
    off = _trainer(n2, n3, lambda_pl=0.0, pseudo_label_source="teacher", pl_threshold="median", pseudo_labels="ensemble")
    for s in range(2):
        la, lb = off.fit_step(_batch(dev)), plain.fit_step(_batch(dev))
        assert _same(la, lb), s
        assert list(off.last_logs) == list(plain.last_logs) and len(off.last_logs) == 6
        for k in plain.last_logs:
            assert _same(off.last_logs[k], plain.last_logs[k]), (s, k)
    torch.cuda.synchronize()
    assert off.last_teacher is None
    _assert_same_dicts(off.model.state_dict(), plain.model.state_dict(), "weights")
    _assert_same_dicts(off.ema.teacher_state_dict(), plain.ema.teacher_state_dict(), "teacher")


def test_an_overflowing_step_skips_student_and_teacher_and_the_next_labels_are_unchanged():
    """An inflated initial loss scale: the 16-bit gradients overflow, the device skips the optimiser step and the teacher's
    update.  The batch is the same every step, so the next step's labels are those of the unchanged teacher: the same."""
    dev = _dev()
    n2, n3 = _nets(dev)
    tm = _teacher_trainer(n2, n3, loss_scale=dict(init_scale=2.0 ** 40))
    tm.configure_optimizers()
    weights0 = {k: v.detach().clone() for k, v in tm.model.state_dict().items() if v.dtype.is_floating_point and "running" not in k}
    teacher0 = {k: v.clone() for k, v in tm.ema.teacher_state_dict().items()}
    tm.fit_step(_batch(dev))
    first = {k: v.clone() for k, v in tm.last_teacher.items()}
    assert int(tm.optimizers[0].step_counter().item()) == 0  # skipped on the device
    tm.fit_step(_batch(dev))
    torch.cuda.synchronize()
    assert int(tm.optimizers[0].step_counter().item()) == 0
    for k in first:
        assert torch.equal(first[k], tm.last_teacher[k]), k
    now = tm.model.state_dict()
    for k, v in weights0.items():
        assert _same(v, now[k]), k
    for k, v in tm.ema.teacher_state_dict().items():
        if v.dtype.is_floating_point:
            assert _same(v, teacher0[k]), k
    assert tm.model.training and tm.ema._depth == 0
