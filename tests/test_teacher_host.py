"""Host checks of the online mean-teacher pseudo labels: the C ABI of mm_teacher_labels (include/mm2d3d.h, csrc/pselab.hip) and
train_kwargs["pseudo_label_source"] / ["pl_threshold"] (mm2d3d_amd/selftrain.py, through the trainer).  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(optimizer=None, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, optimizer, Loss("cross_entropy"),
                      dict(gc_freeze=False, **kw))


def test_header_declares_and_the_binding_matches_the_fifteen_arguments():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "int64_t*": _lib.vp, "unsigned long long*": _lib.vp, "mm_stream_t": _lib.vp,
             "int": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32}
    assert hasattr(lib, "mm_teacher_labels"), "mm_teacher_labels is not exported"
    m = re.search(r"\bint\s+mm_teacher_labels\s*\(([^)]*)\)\s*;", txt)
    assert m, "mm_teacher_labels is not declared in include/mm2d3d.h"
    params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
    res, args = _lib._PROTOS["mm_teacher_labels"]
    assert res is _lib.i32 and len(args) == len(params) == 15
    assert args == [ctype[p] for p in params], params


def test_argument_errors_come_before_any_launch():
    """Every refusal is decided on the host: these calls return without touching a device (there is none here)."""
    from mm2d3d_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_double * 64)()  # never read or written: every call below is refused, or has N == 0
    p = ctypes.addressof(buf)

    def call(l2=p, ld2=6, l3=p, ld3=6, N=8, C=6, y2=p, y3=p):
        return L.mm_teacher_labels(l2, ld2, l3, ld3, N, C, 0, 0.5, -100, y2, y3, None, None, None, None)

    bad = [dict(C=0), dict(C=-1), dict(C=33), dict(N=-1), dict(N=128 * 0x7FFFFFFF + 1), dict(l2=None), dict(l3=None), dict(y2=None),
           dict(y3=None), dict(ld2=5), dict(ld3=5), dict(ld2=0), dict(C=32, ld2=31, ld3=32)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"teacher_labels:" in L.mm_last_error(), (kw, L.mm_last_error())
    # N == 0 is no error and launches nothing, whatever the pointers are
    assert call(N=0) == 0
    assert call(N=0, l2=None, l3=None, y2=None, y3=None) == 0
    assert call(N=0, C=33) == -1  # ... but the class count is checked first


def test_constructor_accepts_and_refuses_the_source():
    tm = _trainer()
    assert tm.pseudo_label_source == "batch" and tm.pl_threshold is None and tm.last_teacher is None
    tm = _trainer(pseudo_label_source="batch", lambda_pl=1.0)
    assert tm.pseudo_label_source == "batch"
    tm = _trainer(pseudo_label_source="teacher", ema_decay=0.9, lambda_pl=1.0, pseudo_labels="ensemble")
    assert tm.pseudo_label_source == "teacher" and tm.pseudo_labels == "ensemble"
    for bad in ("student", "file", None, "", 1):
        with pytest.raises(ValueError, match="pseudo_label_source"):
            _trainer(pseudo_label_source=bad, ema_decay=0.9)
    for kw, word in ((dict(), "ema_decay"), (dict(ema_decay=None), "ema_decay"), (dict(ema_decay=0.9, overlap_metadata=True), "overlap_metadata"),
                     (dict(ema_decay=0.9, overlap_branches=1), "overlap_branches"), (dict(ema_decay=0.9, overlap_branches=2), "overlap_branches")):
        with pytest.raises(ValueError, match="pseudo_label_source") as e:
            _trainer(pseudo_label_source="teacher", lambda_pl=1.0, **kw)
        assert word in str(e.value), (kw, str(e.value))
    # the side-stream modes stay available to the batch source
    assert _trainer(pseudo_label_source="batch", overlap_branches=2, lambda_pl=1.0).overlap_branches == 2
    # the refusals of the label mode stand as they were
    with pytest.raises(ValueError, match="pseudo_labels"):
        _trainer(pseudo_label_source="teacher", ema_decay=0.9, pseudo_labels="3d")
    with pytest.raises(ValueError, match="pseudo_labels"):
        _trainer(pseudo_label_source="teacher", ema_decay=0.9, lambda_pl=1.0, pseudo_labels=None)


def test_constructor_accepts_and_refuses_the_threshold():
    for good in (None, "median", 0.5, 0.9, 1.0, 1, 1e-6):
        assert _trainer(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold=good).pl_threshold == good
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf"), "mean", "0.9", True, [0.9]):
        with pytest.raises(ValueError, match="pl_threshold"):
            _trainer(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold=bad)


def test_lambda_pl_zero_with_the_teacher_source_builds_what_ema_decay_alone_builds():
    from mm2d3d_amd.optimizers import Optimizer

    def make(**kw):
        torch.manual_seed(1)
        return _trainer({"2d_net": Optimizer("sgd", lr=0.1), "3d_net": Optimizer("adamw", lr=0.1)}, **kw)

    with_source = make(ema_decay=0.9, pseudo_label_source="teacher", pl_threshold=0.9, lambda_pl=0.0)
    plain = make(ema_decay=0.9)
    assert with_source.ema is None and with_source.lambda_pl == 0.0  # built with the optimisers, as always
    with_source.configure_optimizers(), plain.configure_optimizers()
    assert with_source.ema is not None and with_source.ema.decay == plain.ema.decay == 0.9
    assert with_source.ema._nrows == plain.ema._nrows and with_source.last_teacher is None
    assert set(vars(with_source)) == set(vars(plain))  # no state beyond the options themselves
    assert set(vars(with_source.selftrain)) == set(vars(plain.selftrain))  # ... nor in the policy object that holds them


def test_a_suspended_forward_claims_no_gradient_sink():
    """The teacher's forward runs between zero_grad and the student's backward: a claim it made would never be released, and the
    parameter's hooks (optimiser bookkeeping, the captured backward's accounting) would never fire."""
    from mm2d3d_amd import gradsink

    p = torch.nn.Parameter(torch.zeros(3))
    p._mm_sink, p._mm_pending = torch.zeros(3), 0
    with gradsink.suspended():
        with gradsink.suspended():
            assert gradsink.claim(None, p, True) is False
        assert gradsink.claim(None, p, True) is False and p._mm_pending == 0
        assert gradsink.claim_affine(None, p, p, True) is None and p._mm_pending == 0
    with pytest.raises(ZeroDivisionError):
        with gradsink.suspended():
            1 / 0
    assert gradsink.claim(None, p, True) is True and p._mm_pending == 1
    assert gradsink.claim(None, p, False) is False and p._mm_pending == 1


def test_the_label_helper_refuses_to_run_before_the_teacher_exists():
    """The teacher is built with the optimisers (fit_step does it); the helper raises rather than building them itself."""
    tm = _trainer(pseudo_label_source="teacher", ema_decay=0.9, lambda_pl=1.0)
    with pytest.raises(RuntimeError, match="configure_optimizers"):
        tm.selftrain.teacher_targets(tm, {}, {})
    assert tm.ema is None and not tm.optimizers


def test_a_threshold_tensor_is_checked_before_anything_else():
    """pselab.teacher_labels(threshold=tensor): float32 [2, C] on the logits' device, or a ValueError that names the argument -
    decided from the arguments alone (a tensor that passes gets as far as the refusal of logits that are not on a GPU)."""
    from mm2d3d_amd import pselab

    l = torch.zeros(5, 6)
    for bad in (torch.zeros(2, 6, dtype=torch.float64), torch.zeros(2, 6, dtype=torch.int64), torch.zeros(6), torch.zeros(2, 5),
                torch.zeros(1, 6), torch.zeros(6, 2), torch.zeros(2, 6, device="meta")):
        with pytest.raises(ValueError, match="threshold"):
            pselab.teacher_labels(l, l, threshold=bad)
    with pytest.raises(RuntimeError, match="logits_2d must live on the GPU"):
        pselab.teacher_labels(l, l, threshold=torch.zeros(2, 6))
