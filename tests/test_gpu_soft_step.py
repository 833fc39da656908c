"""Soft mean-teacher targets in the training step: train_kwargs["pl_targets"] = "soft" and ["pl_temperature"] (mm2d3d_amd/train.py,
losses.cross_entropy_soft_pair).  Shapes and helpers of tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with 48x64
images, 6 classes, fp16, dropout p = 0, ema_decay 0.9.

The main check is a twin: trainer A takes its soft targets from its own teacher pass, trainer B (the same nets, seed and
``ema_decay``) is handed clones of A's teacher logits as the batch's ``teacher_logit_*`` keys.  If the teacher pass leaves anything
behind, or the logits A's loss calls read were overwritten before they read them, the two part ways; they must stay equal bit for
bit."""
import copy

import numpy as np
import pytest
import torch

from _step_util import _alone_logits, _assert_same_dicts, _batch, _dev, _f, _nets, _restore_precision, _same, _trainer  # noqa: F401  (_restore_precision: the autouse fixture, for this module too)

pytestmark = pytest.mark.gpu

STEPS = 3
PL_KEYS = ("train/pl_loss_tgt_2d", "train/pl_loss_tgt_3d")
KEPT_KEYS = ("train/pl_kept_2d", "train/pl_kept_3d")


def _soft_trainer(n2, n3, **kw):
    return _trainer(n2, n3, lambda_pl=1.0, pseudo_label_source="teacher", pl_targets="soft", **kw)


# ---------------------------------------------------------------------------------------------- the twin
TWINS = {
    "joined_own_T2": dict(pseudo_labels="own", pl_temperature=2.0),
    "joined_ensemble_thr": dict(pseudo_labels="ensemble", pl_threshold=0.5),
    "two_calls": dict(pseudo_labels="own", joint_domains=False),
    "prefetched": dict(pseudo_labels="own"),
}


@pytest.mark.parametrize("case", list(TWINS))
def test_twin_fed_the_teachers_logits_stays_bit_identical(case):
    dev = _dev()
    kw = TWINS[case]
    # the ensemble case cuts by confidence: with both heads scaled by 4 the initial teacher's ensemble confidences lie on both sides
    # of 0.5 (measured: minimum 0.236, 10th percentile 0.504, median 0.568, maximum 0.582 over the 34880 rows)
    n2, n3 = _nets(dev, head_scale=4.0) if "pl_threshold" in kw else _nets(dev)
    b2, b3 = copy.deepcopy(n2), copy.deepcopy(n3)
    A = _soft_trainer(n2, n3, **kw)
    B = _trainer(b2, b3, lambda_pl=1.0, pseudo_label_source="batch", pl_targets="soft", **kw)
    A.configure_optimizers(), B.configure_optimizers()
    ptrs = [p.data_ptr() for p in A.model.parameters()] + [b.data_ptr() for b in A.model.buffers()]
    ahead = case == "prefetched"
    batches_a = [_batch(dev) for _ in range(STEPS)]
    batches_b = [_batch(dev) for _ in range(STEPS)]
    for s in range(STEPS):
        nxt = dict(next_batch=batches_a[s + 1]) if ahead and s + 1 < STEPS else {}
        torch.manual_seed(100 + s)
        la = A.fit_step(batches_a[s], **nxt)
        got = A.last_teacher
        assert set(got) == {"logit_2d", "logit_3d", "kept"} and all(v.is_cuda for v in got.values())
        n_trg = int(batches_a[s]["target"]["x"][0].shape[0])
        assert got["logit_2d"].shape == got["logit_3d"].shape == (n_trg, 6) and got["logit_2d"].dtype == torch.float32
        assert got["kept"].shape == (2,) and got["kept"].dtype == torch.int64
        kept = got["kept"].tolist()
        print(f"{case} step {s}: kept {kept} of {n_trg}")
        if "pl_threshold" not in kw:
            assert kept == [n_trg, n_trg]  # no threshold: every row with finite teacher logits
        else:
            assert kept[0] == kept[1] and 0 <= kept[0] <= n_trg  # the ensemble judges both heads' rows by one confidence
            assert s > 0 or 0 < kept[0] < n_trg  # the initial teacher: some rows kept, some refused
        # the model is the student's again
        assert A.model.training and all(m.training for m in A.model.modules()) and A.ema._depth == 0
        assert [p.data_ptr() for p in A.model.parameters()] + [b.data_ptr() for b in A.model.buffers()] == ptrs
        trg = batches_b[s]["target"]
        trg["teacher_logit_2d"], trg["teacher_logit_3d"] = got["logit_2d"].clone(), got["logit_3d"].clone()
        nxt = dict(next_batch=batches_b[s + 1]) if ahead and s + 1 < STEPS else {}
        torch.manual_seed(100 + s)
        lb = B.fit_step(batches_b[s], **nxt)
        assert B.last_teacher is None
        assert _same(la, lb), (case, s, _f(la), _f(lb))
        assert list(A.last_logs) == list(B.last_logs) and len(A.last_logs) == 10
        assert set(PL_KEYS) | set(KEPT_KEYS) <= set(A.last_logs)
        assert all(A.last_logs[k].is_cuda for k in PL_KEYS + KEPT_KEYS)
        for k in A.last_logs:
            assert _same(A.last_logs[k], B.last_logs[k]), (case, s, k, _f(A.last_logs[k]), _f(B.last_logs[k]))
        for j, k in enumerate(KEPT_KEYS):
            assert _f(A.last_logs[k]) == float(torch.tensor(kept[j], dtype=torch.float32) / n_trg)
    torch.cuda.synchronize()
    assert all(np.isfinite(_f(A.last_logs[k])) for k in PL_KEYS)
    if "pl_threshold" not in kw:
        assert all(_f(A.last_logs[k]) > 0.0 for k in PL_KEYS)
    _assert_same_dicts(A.model.state_dict(), B.model.state_dict(), case)
    _assert_same_dicts(A.ema.teacher_state_dict(), B.ema.teacher_state_dict(), case + " teacher")
    assert int(A.optimizers[0].step_counter().item()) == int(B.optimizers[0].step_counter().item())
    nbt = [int(v) for k, v in A.model.state_dict().items() if k.endswith("num_batches_tracked")]
    assert nbt and max(nbt) <= 2 * STEPS  # the student's own forwards only: the teacher pass updated no running statistic


# ---------------------------------------------------------------------------------------------- the logits outlive the step
@pytest.mark.parametrize("joint", [True, False], ids=["joined", "two_calls"])
def test_teacher_logits_survive_the_students_forward_and_backward(joint):
    """The loss calls read the teacher's logits after the student's forward was queued, and the backward reads them again: what
    ``last_teacher`` holds after the step must still be the teacher's alone forward of the target batch taken before the step."""
    dev = _dev()
    n2, n3 = _nets(dev, head_scale=4.0)
    tm = _soft_trainer(n2, n3, lr=1e-2, joint_domains=joint)
    for _ in range(2):
        tm.fit_step(_batch(dev))
    assert int(tm.optimizers[0].step_counter().item()) >= 1  # the student has moved away from the teacher
    l2, l3 = _alone_logits(tm, dev)
    tm.fit_step(_batch(dev))
    got = tm.last_teacher
    torch.cuda.synchronize()
    d2 = (got["logit_2d"] - l2).abs().max().item()
    d3 = (got["logit_3d"] - l3).abs().max().item()
    print(f"joint {joint}: max |logit after the step - alone forward| 2D {d2:.3e}, 3D {d3:.3e}; rows differing 2D "
          f"{int((got['logit_2d'] != l2).any(1).sum())}, 3D {int((got['logit_3d'] != l3).any(1).sum())} of {l2.shape[0]}")
    assert _same(got["logit_2d"], l2)
    assert _same(got["logit_3d"], l3)


# ---------------------------------------------------------------------------------------------- the default is untouched
def test_hard_targets_given_or_not_are_the_same_step():
    dev = _dev()
    n2, n3 = _nets(dev)
    given = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), lambda_pl=1.0, pseudo_label_source="teacher", pl_targets="hard", pl_temperature=1.0)
    plain = _trainer(n2, n3, lambda_pl=1.0, pseudo_label_source="teacher")
    for s in range(2):
        la, lb = given.fit_step(_batch(dev)), plain.fit_step(_batch(dev))
        assert _same(la, lb), s
        assert list(given.last_logs) == list(plain.last_logs) and len(given.last_logs) == 10
        for k in plain.last_logs:
            assert _same(given.last_logs[k], plain.last_logs[k]), (s, k)
        assert set(given.last_teacher) == set(plain.last_teacher) == {"label_2d", "label_3d", "kept"}
        for k in plain.last_teacher:
            assert torch.equal(given.last_teacher[k], plain.last_teacher[k]), (s, k)
    torch.cuda.synchronize()
    _assert_same_dicts(given.model.state_dict(), plain.model.state_dict(), "weights")
    _assert_same_dicts(given.ema.teacher_state_dict(), plain.ema.teacher_state_dict(), "teacher")


# ---------------------------------------------------------------------------------------------- further step checks
def test_soft_losses_differ_from_the_hard_ones_on_the_same_weights():
    dev = _dev()
    n2, n3 = _nets(dev, head_scale=4.0, head_scale_2d=0.02)
    hard = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), lambda_pl=1.0, pseudo_label_source="teacher")
    soft = _soft_trainer(n2, n3)
    hard.fit_step(_batch(dev)), soft.fit_step(_batch(dev))
    torch.cuda.synchronize()
    n = int(_batch(dev)["target"]["x"][0].shape[0])
    for j, (k, kk) in enumerate(zip(PL_KEYS, KEPT_KEYS)):
        h, s = _f(hard.last_logs[k]), _f(soft.last_logs[k])
        print(f"{k}: hard {h:.6f}, soft {s:.6f}; kept {int(soft.last_teacher['kept'][j])} of {n}")
        assert np.isfinite(h) and np.isfinite(s) and h != s
        # the same teacher, the same confidences, the same threshold: the same rows
        assert torch.equal(soft.last_teacher["kept"], hard.last_teacher["kept"])
        assert _f(soft.last_logs[kk]) == float(soft.last_teacher["kept"][j].to(torch.float32) / n) == _f(hard.last_logs[kk])


@pytest.mark.parametrize("mode", ["own", "ensemble"])
def test_threshold_one_keeps_nothing_and_the_step_stays_finite(mode):
    dev = _dev()
    n2, n3 = _nets(dev, head_scale=4.0, head_scale_2d=0.02)
    tm = _soft_trainer(n2, n3, pseudo_labels=mode, pl_threshold=1.0)
    tm.configure_optimizers()
    from mm2d3d_amd import pselab

    l2, l3 = _alone_logits(tm, dev)  # the first step's teacher is the initial weights
    ref = pselab.teacher_labels(l2, l3, ensemble=mode == "ensemble", with_probs=True)
    assert float(ref["prob_2d"].max()) < 1.0 and float(ref["prob_3d"].max()) < 1.0  # non-degenerate logits
    loss = tm.fit_step(_batch(dev))
    torch.cuda.synchronize()
    assert tm.last_teacher["kept"].tolist() == [0, 0]
    assert all(_f(tm.last_logs[k]) == 0.0 for k in PL_KEYS + KEPT_KEYS)
    assert np.isfinite(_f(loss)) and all(bool(torch.isfinite(p).all()) for p in tm.model.parameters())


def test_soft_options_with_lambda_pl_zero_are_the_step_without_them():
    dev = _dev()
    n2, n3 = _nets(dev)
    plain = _trainer(copy.deepcopy(n2), copy.deepcopy(n3))
    off = _trainer(n2, n3, lambda_pl=0.0, pseudo_label_source="teacher", pl_targets="soft", pl_temperature=2.0, pl_threshold=0.9,
                   pseudo_labels="ensemble")
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
