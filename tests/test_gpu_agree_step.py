"""Pseudo-label losses weighted by 2D/3D agreement in the training step: train_kwargs["pl_agreement"] (mm2d3d_amd/selftrain.py,
pselab.agreement_weights, losses.cross_entropy_pair / cross_entropy_soft_pair with row weights).  Shapes and helpers of
tests/_step_util.py: 1 + 1 synthetic nuScenes scenes with 48x64 images, 6 classes, fp16, dropout p = 0, ema_decay 0.9; heads scaled
by 4 as in tests/test_gpu_soft_step.py (confidences and divergences spread out).

The logits the weights come from: the teacher's (teacher source: its alone forward of the target batch, bit-identical to the
pass inside the step - tests/test_gpu_soft_step.py), or the student's own target rows (batch source with hard labels), which a
spy on ``SelfTraining.losses`` records as the step hands them over.  The logged pseudo-label losses are compared with the float64
reference of tests/_agree_ref.py on those logits and weights at 1e-5 * max(1, |ref|), the tolerance of test_gpu_ce_pair.py; the
soft reference takes the kept rows from pselab.predict's float32 confidences (the gate is not what this file checks; pl_kept_*
against the step without the option is)."""
import copy

import numpy as np
import pytest
import torch

import _agree_ref as R
import _step_util as T
from _step_util import _BUILT, _release_memory, _restore_precision  # noqa: F401  (the autouse fixtures, for this module too)

pytestmark = pytest.mark.gpu

BETA = 0.25
PL_KEYS = ("train/pl_loss_tgt_2d", "train/pl_loss_tgt_3d")
KEPT_KEYS = ("train/pl_kept_2d", "train/pl_kept_3d")
AGREE_KEYS = ("train/pl_agree_w", "train/pl_agree_div")
CONFIGS = {
    "teacher_hard": dict(pseudo_label_source="teacher"),
    "teacher_soft_adaptive": dict(pseudo_label_source="teacher", pl_targets="soft", pl_threshold="adaptive", pl_threshold_momentum=0.5,
                                  pl_threshold_warmup=True),
    "batch_hard": dict(pseudo_label_source="batch"),
}


def _trainer(n2, n3, **kw):
    _BUILT.append(T._trainer(n2, n3, lambda_pl=1.0, **kw))
    return _BUILT[-1]


def _pseudo(batch, step):
    """Seeded pseudo labels for the batch source, about half of them -100 (tests/test_gpu_pl_step.py)."""
    n = int(batch["target"]["x"][0].shape[0])
    g = torch.Generator().manual_seed(50 + step)
    for k in ("pseudo_label_2d", "pseudo_label_3d"):
        y = torch.randint(0, 6, (n,), generator=g)
        y[torch.rand(n, generator=g) < 0.5] = -100
        batch["target"][k] = y.to(batch["target"]["x"][0].device)
    return batch


def _spy(tm):
    """Records the logits and targets ``SelfTraining.losses`` is handed (clones: the step goes on as it would)."""
    seen, orig = {}, tm.selftrain.losses

    def losses(l2, l3, split, targets, *a, **k):
        seen.update(l2=l2.detach().float().clone(), l3=l3.detach().float().clone(), split=int(split), targets=targets)
        return orig(l2, l3, split, targets, *a, **k)

    tm.selftrain.losses = losses
    return seen


def _np(t):
    return t.detach().float().cpu().numpy()


def _close(got, ref):
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------------- without the option
def test_no_key_and_none_are_the_same_step():
    dev = T._dev()
    n2, n3 = T._nets(dev, head_scale=4.0)
    plain = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), pseudo_label_source="teacher")
    none = _trainer(n2, n3, pseudo_label_source="teacher", pl_agreement=None)
    for s in range(2):
        la, lb = none.fit_step(T._batch(dev)), plain.fit_step(T._batch(dev))
        assert T._same(la, lb), s
        assert list(none.last_logs) == list(plain.last_logs) and len(none.last_logs) == 10 and not set(AGREE_KEYS) & set(none.last_logs)
        for k in plain.last_logs:
            assert T._same(none.last_logs[k], plain.last_logs[k]), (s, k)
        assert none.last_agreement is None and plain.last_agreement is None and none.selftrain._agree is None
    torch.cuda.synchronize()
    T._assert_same_dicts(none.model.state_dict(), plain.model.state_dict(), "weights")
    T._assert_same_dicts(none.ema.teacher_state_dict(), plain.ema.teacher_state_dict(), "teacher")


# ---------------------------------------------------------------------------------------------- with a value of beta
@pytest.mark.parametrize("case", list(CONFIGS))
def test_weights_losses_and_kept_rows_of_the_weighted_step(case):
    from mm2d3d_amd import pselab

    dev = T._dev()
    kw = CONFIGS[case]
    teacher, soft = kw["pseudo_label_source"] == "teacher", kw.get("pl_targets") == "soft"
    n2, n3 = T._nets(dev, head_scale=4.0)
    A = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), pl_agreement=BETA, **kw)
    B = _trainer(n2, n3, **kw)  # the same step without the option
    A.configure_optimizers(), B.configure_optimizers()
    assert A.pl_agreement == BETA and A.last_agreement is None
    seen = _spy(A)
    for s in range(2):
        batch = T._batch(dev) if teacher else _pseudo(T._batch(dev), s)
        n_trg = int(batch["target"]["x"][0].shape[0])
        l2, l3 = T._alone_logits(A, dev) if teacher else (None, None)  # the teacher before the step
        A.fit_step(batch)
        P, x2, x3 = seen["split"], seen["l2"], seen["l3"]
        assert x2.shape[0] - P == n_trg
        if not teacher:  # the student's own main-head target rows of this step
            l2, l3 = x2[P:], x3[P:]
        got = A.last_agreement
        assert set(got) == {"weight", "mean_weight", "mean_div"} and all(v.is_cuda and not v.requires_grad for v in got.values())
        want = pselab.agreement_weights(l2, l3, BETA)
        assert got["weight"].shape == (n_trg,) and T._same(got["weight"], want["weight"]), (case, s)
        assert T._same(got["mean_weight"], want["mean_weight"]) and T._same(got["mean_div"], want["mean_div"])
        ref = R.agreement(_np(l2), _np(l3), BETA)
        w = _np(got["weight"]).astype(np.float64)
        assert np.abs(w - ref["weight"]).max() <= 1e-5 and int(want["finite"]) == n_trg
        logs = A.last_logs
        assert all(logs[k].is_cuda and logs[k].dim() == 0 for k in AGREE_KEYS + PL_KEYS)
        assert T._same(logs[AGREE_KEYS[0]], got["mean_weight"]) and T._same(logs[AGREE_KEYS[1]], got["mean_div"])
        assert 0.0 < T._f(got["mean_weight"]) < 1.0 and T._f(got["mean_div"]) > 0.0  # the two modalities do disagree here
        # the logged pseudo-label losses: the reference on the step's own logits, targets and weights
        for o, (k, x) in enumerate(zip(PL_KEYS, (x2, x3))):
            xt = _np(x[P:]).astype(np.float64)
            if soft:
                t = A.last_teacher
                ta, thr = (t["logit_2d"], t["logit_3d"])[o], t["threshold"][o]
                pred = pselab.predict(ta)
                keep = (pred["probs_2d"] >= thr[pred["pseudo_label_2d"].long()]).cpu().numpy()
                r = R.soft_tail(xt, _np(ta), None, 1.0, None, w, keep=keep)
                assert r["K"] == int(t["kept"][o]) and r["K"] > 0, (case, s, o, r["K"], n_trg)
            else:
                y = A.last_teacher[("label_2d", "label_3d")[o]] if teacher else batch["target"][("pseudo_label_2d", "pseudo_label_3d")[o]]
                r = R.hard_tail(xt, y.cpu().numpy(), None, w)
                unweighted = R.hard_tail(xt, y.cpu().numpy(), None, None)
                assert r["loss"] < unweighted["loss"]  # weights <= 1 outside the denominator: the batch pulls less
            print(f"{case} step {s} {k}: logged {T._f(logs[k]):.7f}, reference {r['loss']:.7f}; mean w {T._f(got['mean_weight']):.4f}, "
                  f"mean D {T._f(got['mean_div']):.4f}")
            assert _close(T._f(logs[k]), r["loss"]), (case, s, k)
        if s == 0:  # the same weights on both sides: the thresholds count and keep the same rows
            B.fit_step(T._batch(dev) if teacher else _pseudo(T._batch(dev), s))
            assert B.last_agreement is None and [k for k in logs if k not in B.last_logs] == list(AGREE_KEYS)
            assert (set(KEPT_KEYS) <= set(logs)) == teacher
            for k in KEPT_KEYS:
                if teacher:
                    assert T._same(logs[k], B.last_logs[k]), (case, k)
            for k in PL_KEYS:
                assert T._f(logs[k]) != T._f(B.last_logs[k])
            if teacher:
                T._assert_same_dicts({k: v for k, v in A.last_teacher.items() if torch.is_tensor(v)},
                                     {k: v for k, v in B.last_teacher.items() if torch.is_tensor(v)}, case + " last_teacher")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in A.model.parameters())
    assert "pl_agreement" not in A.checkpoint()  # no state


def test_identical_teacher_outputs_give_the_unweighted_losses_bit_for_bit():
    """Batch source with soft targets whose two teacher matrices are the same: every weight is exactly 1, and x * 1.0f is exact."""
    dev = T._dev()
    n2, n3 = T._nets(dev, head_scale=4.0)
    kw = dict(pseudo_label_source="batch", pl_targets="soft", pl_threshold=0.4, pl_temperature=2.0)
    A = _trainer(copy.deepcopy(n2), copy.deepcopy(n3), pl_agreement=BETA, **kw)
    B = _trainer(n2, n3, **kw)
    for s in range(2):
        batches = [T._batch(dev), T._batch(dev)]
        n = int(batches[0]["target"]["x"][0].shape[0])
        t = (3.0 * torch.randn(n, 6, generator=torch.Generator().manual_seed(60 + s))).to(dev)
        for b in batches:
            b["target"]["teacher_logit_2d"], b["target"]["teacher_logit_3d"] = t.clone(), t.clone()
        la, lb = A.fit_step(batches[0]), B.fit_step(batches[1])
        assert bool((A.last_agreement["weight"] == 1.0).all()) and T._f(A.last_agreement["mean_weight"]) == 1.0
        assert T._f(A.last_agreement["mean_div"]) == 0.0
        assert T._same(la, lb), s
        for k in B.last_logs:
            assert T._same(A.last_logs[k], B.last_logs[k]), (s, k)
        assert 0.0 < T._f(A.last_logs[KEPT_KEYS[0]]) < 1.0
    torch.cuda.synchronize()
    T._assert_same_dicts(A.model.state_dict(), B.model.state_dict(), "weights")
