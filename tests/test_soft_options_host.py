"""Host checks of the soft mean-teacher targets: train_kwargs["pl_targets"] / ["pl_temperature"] (mm2d3d_amd/selftrain.py) and the C ABI
of the two-segment cross entropy with a soft tail (include/mm2d3d.h mm_ce2s_*).  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"), dict(gc_freeze=False, **kw))


def test_defaults_are_hard_targets_at_temperature_one():
    tm = _trainer()
    assert tm.pl_targets == "hard" and tm.pl_temperature == 1.0 and isinstance(tm.pl_temperature, float)
    tm = _trainer(lambda_pl=1.0, pl_targets="hard", pl_temperature=1)
    assert tm.pl_targets == "hard" and tm.pl_temperature == 1.0


def test_pl_targets_accepts_only_hard_and_soft():
    assert _trainer(pl_targets="soft").pl_targets == "soft"
    assert _trainer(pl_targets="soft", lambda_pl=1.0, pseudo_label_source="teacher", ema_decay=0.9, pseudo_labels="ensemble").pl_targets == "soft"
    for bad in ("Soft", "kl", "", None, 1, True, ["soft"]):
        with pytest.raises(ValueError, match="pl_targets"):
            _trainer(pl_targets=bad)


def test_pl_temperature_must_be_positive_and_is_refused_with_hard_targets():
    for good in (0.5, 1, 1.0, 2.0, 1e-3, 100):
        assert _trainer(pl_targets="soft", pl_temperature=good).pl_temperature == float(good)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2", None, True, [2.0]):
        with pytest.raises(ValueError, match="pl_temperature"):
            _trainer(pl_targets="soft", pl_temperature=bad)
    for hard in (dict(), dict(pl_targets="hard")):
        for T in (0.5, 2.0, 1.0000001):
            with pytest.raises(ValueError, match="pl_temperature") as e:
                _trainer(pl_temperature=T, **hard)
            assert "hard" in str(e.value)
        with pytest.raises(ValueError, match="pl_temperature"):
            _trainer(pl_temperature=0.0, **hard)


def test_soft_targets_refuse_the_median_rule():
    with pytest.raises(ValueError, match="pl_threshold") as e:
        _trainer(pl_targets="soft", pl_threshold="median", pseudo_label_source="teacher", ema_decay=0.9)
    assert "median" in str(e.value) and "soft" in str(e.value)
    with pytest.raises(ValueError, match="pl_threshold"):
        _trainer(pl_targets="soft", pl_threshold="median")
    for good in (None, 0.5, 1.0):
        assert _trainer(pl_targets="soft", pl_threshold=good).pl_threshold == good
    # the rule stays available to hard targets
    assert _trainer(pl_threshold="median", pseudo_label_source="teacher", ema_decay=0.9).pl_threshold == "median"


def test_a_batch_without_teacher_logits_is_refused_before_anything_is_queued():
    """Raised from the batch dict alone: the networks below are never called (a torch.nn.Linear could not take the batch)."""
    tm = _trainer(lambda_pl=1.0, pl_targets="soft", pseudo_label_source="batch")
    st = tm.selftrain
    x = [torch.zeros(5, 4, dtype=torch.int64), torch.zeros(5, 3)]
    l = torch.zeros(5, 6)
    src = {"x": x, "img": torch.zeros(1, 3, 4, 4), "depth": torch.zeros(1, 1, 4, 4), "seg_label": torch.zeros(5, dtype=torch.int64)}
    with pytest.raises(KeyError, match="teacher_logit_2d"):
        tm.training_step({"source": src, "target": {"x": x, "teacher_logit_3d": l}})
    with pytest.raises(KeyError, match="teacher_logit_3d"):
        st.batch_targets({"x": x, "teacher_logit_2d": l})
    with pytest.raises(ValueError, match="5 point rows"):
        st.batch_targets({"x": x, "teacher_logit_2d": l[:4], "teacher_logit_3d": l})
    with pytest.raises(ValueError, match="5 point rows"):
        st.batch_targets({"x": x, "teacher_logit_2d": l, "teacher_logit_3d": torch.zeros(5, dtype=torch.int64)})
    with pytest.raises(ValueError, match="teacher_logit_3d"):
        st.batch_targets({"x": x, "teacher_logit_2d": l, "teacher_logit_3d": torch.zeros(5, 7)})
    batch = {"x": x, "teacher_logit_2d": l, "teacher_logit_3d": l + 1}
    a, b = batch["teacher_logit_2d"], batch["teacher_logit_3d"]
    own = st.batch_targets(batch)
    assert own[0].value is l and float(own[1].value[0, 0]) == 1.0
    assert [tuple(t) for t in own] == [(a, None, None), (b, None, None)]  # per head (teacher, teacher_other, threshold)
    ens = _trainer(lambda_pl=1.0, pl_targets="soft", pseudo_labels="ensemble").selftrain
    assert [tuple(t) for t in ens.batch_targets(batch)] == [(a, b, None), (a, b, None)]
    cut = _trainer(lambda_pl=1.0, pl_targets="soft", pseudo_labels="ensemble", pl_threshold=0.5).selftrain
    assert [t.threshold for t in cut.batch_targets(batch)] == [0.5, 0.5]  # a fixed threshold travels with each head's target
    # hard targets of the same batch still ask for labels, and lambda_pl = 0 consults nothing of this
    with pytest.raises(KeyError, match="pseudo_label_2d"):
        _trainer(lambda_pl=1.0).selftrain.batch_targets({"x": x, "teacher_logit_2d": l, "teacher_logit_3d": l})
    assert _trainer(pl_targets="soft", pl_temperature=2.0).lambda_pl == 0.0


def test_header_declares_and_the_binding_matches_the_three_symbols():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp,
             "int": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.sz, "float": _lib.f32}
    want = {"mm_ce2s_ws_bytes": 0, "mm_ce2s_fwd": 19, "mm_ce2s_bwd": 19}
    for name, n_args in want.items():
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [] if m.group(2).strip() == "void" else [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctype[m.group(1)] and len(args) == len(params) == n_args, name
        assert args == [ctype[p] for p in params], (name, params)
    assert "T^2" in txt[txt.index("SOFT tail"):txt.index("mm_ce2s_ws_bytes")]  # the header says that there is no such factor


def test_argument_errors_come_before_any_launch():
    """Every refusal is decided on the host: these calls return without touching a device (there is none here)."""
    from mm2d3d_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_double * 64)()  # never read or written: every call below is refused
    p = ctypes.addressof(buf)
    big = 1 << 20

    def fwd(x=p, ld=6, N=10, P=5, C=6, ta=p, ld_a=6, tb=None, ld_b=0, T=1.0, thr=0.0, stats=p, ws_bytes=big):
        return L.mm_ce2s_fwd(x, ld, N, P, C, None, None, -100, ta, ld_a, tb, ld_b, T, thr, stats, None, p, ws_bytes, None)

    def bwd(x=p, ld=6, N=10, P=5, C=6, ta=p, ld_a=6, tb=None, ld_b=0, T=1.0, thr=0.0, ld_d=6, d=p):
        return L.mm_ce2s_bwd(x, ld, N, P, C, None, None, -100, ta, ld_a, tb, ld_b, T, thr, p, p, d, ld_d, None)

    assert int(L.mm_ce2s_ws_bytes()) >= 1024 * 4 * 8
    bad = [(dict(C=0), b"bad C"), (dict(C=33, ld=33, ld_a=33), b"bad C"), (dict(ld=5), b"bad C"), (dict(P=11), b"split"), (dict(P=-1), b"split"),
           (dict(N=-1, P=0), b"split"), (dict(x=None), b"null logits"), (dict(ta=None), b"teacher"), (dict(ld_a=5), b"pitch"),
           (dict(tb=p, ld_b=5), b"pitch"), (dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"), (dict(T=float("nan")), b"temperature"),
           (dict(T=float("inf")), b"temperature"), (dict(thr=-0.5), b"threshold"), (dict(thr=1.5), b"threshold"),
           (dict(thr=float("nan")), b"threshold"), (dict(N=10, P=10, ta=None, tb=p, ld_b=6), b"teacher")]
    for kw, word in bad:
        for fn in (fwd, bwd):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert b"ce2s:" in L.mm_last_error() and word in L.mm_last_error(), (kw, L.mm_last_error())
    assert fwd(stats=None) == -1 and b"stats" in L.mm_last_error()
    assert fwd(ws_bytes=16) != 0 and b"workspace" in L.mm_last_error()
    assert bwd(ld_d=5) == -1 and b"pitch" in L.mm_last_error()
    assert bwd(d=None) == -1 and b"null" in L.mm_last_error()
    # no rows: the backward launches nothing, whatever the pointers are (an empty tail needs no teacher)
    assert L.mm_ce2s_bwd(None, 6, 0, 0, 6, None, None, -100, None, 0, None, 0, 1.0, 0.0, None, None, None, 6, None) == 0
