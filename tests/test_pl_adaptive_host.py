"""Host checks of the self-adaptive per-class pseudo-label thresholds: the float64 oracle (tests/_adaptive_ref.py) on an example
worked by hand, train_kwargs["pl_threshold"] = "adaptive" in the constructor (mm2d3d_amd/selftrain.py), and the argument checks of the
three new entry-point families (include/mm2d3d.h: mm_pl_adapt, mm_teacher_labels_cls, mm_ce2s_fwd_cls / mm_ce2s_bwd_cls), every one
of which is decided before any device call.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from _adaptive_ref import AdaptiveRef


def _trainer(optimizer=None, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, optimizer, Loss("cross_entropy"),
                      dict(gc_freeze=False, **kw))


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_on_a_hand_worked_two_class_example():
    """C = 2, two rows, momentum 0.5 from tau = pt = 1/2.
    2D: softmax rows (0.25, 0.75) and (0.9, 0.1): mean p = 0.825, tau = 0.6625; mean q = (0.575, 0.425), pt = (0.5375, 0.4625);
        thr = (0.6625, 0.4625 / 0.5375 * 0.6625).  Row 0: class 1, 0.75 >= 0.5700.. kept; row 1: class 0, 0.9 >= 0.6625 kept.
    3D: softmax rows (0.5, 0.5) and (0.8, 0.2): mean p = 0.65, tau = 0.575; mean q = (0.65, 0.35), pt = (0.575, 0.425);
        thr = (0.575, 0.425).  Row 0: a tie, the first class wins, 0.5 < 0.575 refused; row 1: class 0, 0.8 kept."""
    l2 = np.array([[0.0, math.log(3.0)], [math.log(9.0), 0.0]])
    l3 = np.array([[0.0, 0.0], [math.log(4.0), 0.0]])
    ref = AdaptiveRef(2, momentum=0.5)
    assert np.array_equal(ref.state, np.full((2, 3), 0.5)) and ref.count.tolist() == [0, 0]
    out = ref.labels(l2, l3)
    np.testing.assert_allclose(ref.state, [[0.6625, 0.5375, 0.4625], [0.575, 0.575, 0.425]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(out["threshold"], [[0.6625, 0.4625 / 0.5375 * 0.6625], [0.575, 0.425]], rtol=0, atol=1e-7)
    assert out["threshold"].dtype == np.float32 and ref.count.tolist() == [1, 1]
    assert out["label"].tolist() == [[1, 0], [-100, 0]] and out["kept"].tolist() == [2, 1]
    # the ensemble: rows (0.375, 0.625) and (0.85, 0.15) for both outputs
    ens = AdaptiveRef(2, momentum=0.5)
    out = ens.labels(l2, l3, ensemble=True)
    np.testing.assert_allclose(ens.state[0], [0.5 * 0.5 + 0.5 * 0.7375, 0.25 + 0.5 * 0.6125, 0.25 + 0.5 * 0.3875], rtol=0, atol=1e-15)
    assert np.array_equal(ens.state[0], ens.state[1]) and np.array_equal(out["label"][0], out["label"][1])
    assert out["label"][0].tolist() == [1, 0]  # thr = (0.61875, 0.61875 * 0.44375 / 0.55625 = 0.4936..): 0.625 and 0.85 pass
    # warm-up: the first update takes momentum min(0.5, 1 / 10)
    warm = AdaptiveRef(2, momentum=0.5, warmup=True)
    warm.update(l2, l3)
    np.testing.assert_allclose(warm.state[0, 0], 0.1 * 0.5 + 0.9 * 0.825, rtol=0, atol=1e-15)
    # rows without a confidence are not counted; a batch of them alone leaves state and count as they are
    bad = np.array([[np.nan, 0.0], [np.inf, 0.0]])
    before = warm.state.copy()
    thr = warm.update(bad, bad)
    assert np.array_equal(warm.state, before) and warm.count.tolist() == [1, 1]
    assert np.array_equal(thr, warm.thresholds())
    one = AdaptiveRef(2, momentum=0.0)
    one.update(np.vstack([l2, bad[:1]]), np.vstack([l3, [[-np.inf, 0.0]]]))  # -inf alone stays finite: softmax (0, 1)
    np.testing.assert_allclose(one.state[0, 0], 0.825, rtol=0, atol=1e-15)
    np.testing.assert_allclose(one.state[1], [(0.5 + 0.8 + 1.0) / 3, (0.5 + 0.8) / 3, (0.5 + 0.2 + 1.0) / 3], rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------- the constructor
def test_constructor_accepts_adaptive_with_the_teacher_source():
    for kw in (dict(), dict(pl_targets="soft"), dict(pseudo_labels="ensemble"), dict(pl_targets="soft", pseudo_labels="ensemble"),
               dict(pl_targets="soft", pl_temperature=2.0), dict(lambda_pl=0.0), dict(lambda_pl=1.0)):
        tm = _trainer(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold="adaptive", **kw)
        assert tm.pl_threshold == "adaptive" and tm.pl_adaptive is None  # built lazily, with the first teacher pass
        assert tm.pl_threshold_momentum == 0.999 and tm.pl_threshold_warmup is False
    tm = _trainer(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold="adaptive", pl_threshold_momentum=0.5, pl_threshold_warmup=True)
    assert tm.pl_threshold_momentum == 0.5 and tm.pl_threshold_warmup is True
    assert _trainer(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold="adaptive", pl_threshold_momentum=0).pl_threshold_momentum == 0.0


def test_constructor_refuses_adaptive_with_the_batch_source():
    for kw in (dict(), dict(pseudo_label_source="batch"), dict(pseudo_label_source="batch", pl_targets="soft"),
               dict(pseudo_label_source="batch", lambda_pl=1.0, ema_decay=0.9)):
        with pytest.raises(ValueError, match="pl_threshold") as e:
            _trainer(pl_threshold="adaptive", **kw)
        assert "teacher" in str(e.value)
    # the teacher source's own refusals stand
    with pytest.raises(ValueError, match="pseudo_label_source"):
        _trainer(pseudo_label_source="teacher", pl_threshold="adaptive")
    # and other strings are still no thresholds
    for bad in ("Adaptive", "adaptive ", "freematch"):
        with pytest.raises(ValueError, match="pl_threshold"):
            _trainer(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold=bad)


def test_constructor_validates_the_momentum_whenever_given():
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf"), "0.9", None, True, [0.9]):
        for kw in (dict(pseudo_label_source="teacher", ema_decay=0.9, pl_threshold="adaptive"), dict()):  # also with the option off
            with pytest.raises(ValueError, match="pl_threshold_momentum"):
                _trainer(pl_threshold_momentum=bad, **kw)
    assert _trainer(pl_threshold_momentum=0.9).pl_threshold_momentum == 0.9


def test_the_option_adds_no_attribute_and_lambda_zero_builds_nothing():
    from mm2d3d_amd.optimizers import Optimizer

    def make(**kw):
        torch.manual_seed(1)
        return _trainer({"2d_net": Optimizer("sgd", lr=0.1), "3d_net": Optimizer("adamw", lr=0.1)}, **kw)

    plain = make()
    teacher = make(ema_decay=0.9, pseudo_label_source="teacher", pl_threshold=0.9, lambda_pl=1.0)
    adaptive = make(ema_decay=0.9, pseudo_label_source="teacher", pl_threshold="adaptive", lambda_pl=0.0, pl_threshold_warmup=True)
    assert set(vars(plain)) == set(vars(teacher)) == set(vars(adaptive))
    assert set(vars(plain.selftrain)) == set(vars(teacher.selftrain)) == set(vars(adaptive.selftrain))  # where the options live
    assert "pl_adaptive" in vars(plain.selftrain) and plain.pl_adaptive is None and teacher.pl_adaptive is None
    adaptive.configure_optimizers(), teacher.configure_optimizers()
    assert set(vars(teacher)) == set(vars(adaptive)) and adaptive.pl_adaptive is None
    assert set(vars(teacher.selftrain)) == set(vars(adaptive.selftrain))
    # lambda_pl == 0: a checkpoint is taken and loaded without the object
    ckpt = adaptive.checkpoint()
    assert "pl_adaptive" not in ckpt
    adaptive.load_checkpoint(dict(ckpt, pl_adaptive={"num_classes": 2, "state": torch.zeros(2, 3, dtype=torch.float64),
                                                     "count": torch.zeros(2, dtype=torch.int64)}))
    assert adaptive.pl_adaptive is None


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_bindings_match():
    import os
    import re

    from mm2d3d_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "double*": _lib.vp, "int64_t*": _lib.vp, "const int64_t*": _lib.vp,
             "unsigned long long*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp, "int": _lib.i32, "int64_t": _lib.i64,
             "float": _lib.f32, "double": _lib.f64, "size_t": _lib.sz}
    for name, n in (("mm_pl_adapt", 15), ("mm_teacher_labels_cls", 15), ("mm_ce2s_fwd_cls", 19), ("mm_ce2s_bwd_cls", 19)):
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is _lib.i32 and len(args) == len(params) == n, name
        assert args == [ctype[p] for p in params], (name, params)
    assert hasattr(lib, "mm_pl_adapt_ws_bytes") and _lib._PROTOS["mm_pl_adapt_ws_bytes"] == (_lib.sz, [])


def _buf():
    buf = (ctypes.c_double * 256)()  # never read or written: every call below is refused before a device call
    return buf, ctypes.addressof(buf)


def test_pl_adapt_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep, p = _buf()
    need = int(L.mm_pl_adapt_ws_bytes())
    assert need >= 256 * 2 * 33 * 8 + 256 * 2 * 8  # at least 256 workgroups' fp64 sums and integer counts at C = 32

    def call(l2=p, ld2=6, l3=p, ld3=6, N=8, C=6, m=0.5, state=p, count=p, thr=p, ws=p, ws_bytes=need):
        return L.mm_pl_adapt(l2, ld2, l3, ld3, N, C, 0, m, 0, state, count, thr, ws, ws_bytes, None)

    bad = [dict(C=0), dict(C=-1), dict(C=33), dict(N=-1), dict(N=128 * 0x7FFFFFFF + 1), dict(m=1.0), dict(m=-0.001), dict(m=1.5),
           dict(m=float("nan")), dict(m=float("inf")), dict(l2=None), dict(l3=None), dict(state=None), dict(count=None), dict(thr=None),
           dict(ld2=5), dict(ld3=5), dict(ld2=0), dict(C=32, ld2=31, ld3=32), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
           # N == 0 launches the update alone: it still needs its state, a momentum and a workspace
           dict(N=0, state=None), dict(N=0, thr=None), dict(N=0, m=1.0), dict(N=0, C=33), dict(N=0, ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"pl_adapt:" in L.mm_last_error(), (kw, L.mm_last_error())


def test_teacher_labels_cls_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep, p = _buf()

    def call(l2=p, ld2=6, l3=p, ld3=6, N=8, C=6, thr=p, y2=p, y3=p):
        return L.mm_teacher_labels_cls(l2, ld2, l3, ld3, N, C, 0, thr, -100, y2, y3, None, None, None, None)

    bad = [dict(C=0), dict(C=-1), dict(C=33), dict(N=-1), dict(N=128 * 0x7FFFFFFF + 1), dict(l2=None), dict(l3=None), dict(y2=None),
           dict(y3=None), dict(thr=None), dict(ld2=5), dict(ld3=5), dict(ld2=0), dict(C=32, ld2=31, ld3=32)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"teacher_labels_cls:" in L.mm_last_error(), (kw, L.mm_last_error())
    # as mm_teacher_labels: N == 0 is no error and launches nothing, but the class count is checked first
    assert call(N=0) == 0 and call(N=0, l2=None, l3=None, y2=None, y3=None, thr=None) == 0
    assert call(N=0, C=33) == -1


def test_ce2s_cls_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep, p = _buf()
    need = int(L.mm_ce2s_ws_bytes())

    def fwd(x=p, ld=6, N=8, P=4, C=6, ta=p, ld_a=6, tb=None, ld_b=0, T=1.0, thr=p, stats=p, ws_bytes=need):
        return L.mm_ce2s_fwd_cls(x, ld, N, P, C, None, None, -100, ta, ld_a, tb, ld_b, T, thr, stats, None, p, ws_bytes, None)

    def bwd(x=p, ld=6, N=8, P=4, C=6, ta=p, ld_a=6, tb=None, ld_b=0, T=1.0, thr=p, stats=p, g=p, d=p, ld_d=6):
        return L.mm_ce2s_bwd_cls(x, ld, N, P, C, None, None, -100, ta, ld_a, tb, ld_b, T, thr, stats, g, d, ld_d, None)

    bad = [dict(C=0), dict(C=33), dict(ld=5), dict(N=-1), dict(P=9), dict(P=-1), dict(x=None), dict(ta=None), dict(ld_a=5),
           dict(tb=p, ld_b=5), dict(T=0.0), dict(T=float("nan")), dict(T=float("inf")), dict(thr=None), dict(stats=None)]
    for kw in bad:
        assert fwd(**kw) == -1, kw
        assert b"ce2s:" in L.mm_last_error(), (kw, L.mm_last_error())
        assert bwd(**kw) == -1, kw
    assert bwd(ld_d=5) == -1 and bwd(g=None) == -1 and bwd(d=None) == -1
    # a short workspace is the scalar pair's refusal, code and text: the two share it
    assert fwd(ws_bytes=need // 2) == L.mm_ce2s_fwd(p, 6, 8, 4, 6, None, None, -100, p, 6, None, 0, 1.0, 0.5, p, None, p, need // 2, None) < 0
    assert b"workspace" in L.mm_last_error()
    assert bwd(N=0, P=0, x=None, ta=None) == 0  # nothing to write, as mm_ce2s_bwd
    # the scalar entry points keep their own threshold check
    assert L.mm_ce2s_fwd(p, 6, 8, 4, 6, None, None, -100, p, 6, None, 0, 1.0, 1.5, p, None, p, need, None) == -1
    assert b"threshold" in L.mm_last_error()
