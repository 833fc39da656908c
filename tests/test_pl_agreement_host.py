"""Host checks of the pseudo-label losses weighted by 2D/3D agreement: the float64 reference (tests/_agree_ref.py) against its own
properties and central differences, a float32 restatement of the weight kernel's formula against float64, the option
``train_kwargs["pl_agreement"]`` (mm2d3d_amd/selftrain.py), the ``row_weight`` arguments of the two pair losses
(mm2d3d_amd/losses.py) and the C ABI (include/mm2d3d.h mm_pl_agree, mm_ce2_*_w, mm_ce2s_*_w).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _agree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W6 = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]


def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"), dict(gc_freeze=False, **kw))


# ---------------------------------------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("C", [2, 6, 32])
def test_reference_weight_properties(C):
    a, b = R.make_pair(300, C, 11 + C)
    ref = R.agreement(a, b, 2.0)
    w, d = ref["weight"], ref["div"]
    assert (d >= 0).all() and ((w > 0) & (w <= 1)).all() and ref["finite"] == 300
    same = R.agreement(a, a, 2.0)
    assert (same["div"] == 0).all() and (same["weight"] == 1.0).all() and same["mean_weight"] == 1.0 and same["mean_div"] == 0.0
    assert np.array_equal(R.agreement(b, a, 2.0)["weight"], w)  # (p - q)(lp - lq) = (q - p)(lq - lp), term by term
    w1, w4 = R.agreement(a, b, 1.0)["weight"], R.agreement(a, b, 4.0)["weight"]
    assert (w1 > w).all() and (w > w4).all()  # decreasing in beta wherever D > 0
    assert (d > 0).all()
    shift = np.random.default_rng(5).uniform(-20, 20, (300, 1))
    shifted = R.agreement(a.astype(np.float64) + shift, b.astype(np.float64) - 3 * shift, 2.0)["weight"]
    assert np.abs(shifted - w).max() <= 1e-12  # a per-row shift of either matrix changes no softmax
    assert ref["mean_weight"] == float(w.mean()) and ref["mean_div"] == float(d.mean())


def test_reference_gives_a_row_that_is_not_finite_weight_zero_and_leaves_it_out_of_the_mean():
    a, b = R.make_pair(10, 6, 3)
    clean = R.agreement(a, b, 1.5)
    a[2, 1], b[5], a[7, 0], b[8, 3] = np.inf, np.nan, -np.inf, np.nan
    ref = R.agreement(a, b, 1.5)
    bad = [2, 5, 7, 8]
    good = [i for i in range(10) if i not in bad]
    assert (ref["weight"][bad] == 0).all() and np.array_equal(ref["weight"][good], clean["weight"][good])
    assert ref["finite"] == 6 and ref["mean_div"] == float(clean["div"][good].mean())
    assert ref["mean_weight"] == float(clean["weight"][good].sum() / 10)  # over ALL rows
    empty = R.agreement(np.zeros((0, 6)), np.zeros((0, 6)), 1.0)
    assert empty["mean_weight"] == 0.0 and empty["mean_div"] == 0.0 and empty["finite"] == 0


def _central(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


@pytest.mark.parametrize("C", [2, 6])
def test_weighted_reference_gradients_match_central_differences(C):
    """h = 1e-6 in float64: truncation h^2 |f'''| / 6 ~ 1e-12 / n and rounding eps / h ~ 1e-10; the bound is the 1e-8 absolute of
    the InfoMax reference.  Observed: hard 6.9e-11 (C = 2), 2.6e-10 (C = 6); soft with a scalar threshold 6.5e-11, 3.0e-10; soft
    with a threshold per class 7.5e-11, 5.4e-10."""
    rng = np.random.default_rng(40 + C)
    n = 12
    x = 3 * rng.standard_normal((n, C))
    y = rng.integers(0, C, n)
    y[[2, 9]] = -100
    cw = W6[:C]
    rw = R.make_row_weights(n, 7)
    hard = R.hard_tail(x, y, cw, rw, grad_out=0.7)
    err = np.abs(hard["dlogits"] - _central(lambda v: 0.7 * R.hard_tail(v, y, cw, rw)["loss"], x)).max()
    print(f"C {C} hard: max |analytic - central difference| {err:.2e}")
    assert err <= 1e-8 and (hard["dlogits"][[2, 9]] == 0).all() and (hard["dlogits"][rw == 0] == 0).all()
    ta, tb = 3 * rng.standard_normal((n, C)), 3 * rng.standard_normal((n, C))
    for name, thr in (("scalar", 0.55), ("per class", np.linspace(0.5, 0.7, C))):
        soft = R.soft_tail(x, ta, tb, 2.0, thr, rw, grad_out=1.3)
        assert 0 < soft["K"] < n
        err = np.abs(soft["dlogits"] - _central(lambda v: 1.3 * R.soft_tail(v, ta, tb, 2.0, thr, rw)["loss"], x)).max()
        print(f"C {C} soft {name}: K {soft['K']}, max |analytic - central difference| {err:.2e}")
        assert err <= 1e-8 and (soft["dlogits"][~soft["keep"]] == 0).all()


def test_weighted_reference_without_weights_is_the_reference_of_the_parents():
    rng = np.random.default_rng(9)
    x, y = 3 * rng.standard_normal((40, 6)), rng.integers(0, 6, 40)
    from _loss_ref import ce

    base = ce(x, y, W6, -100, 0.5)
    for rw in (None, np.ones(40, np.float32)):
        got = R.hard_tail(x, y, W6, rw, grad_out=0.5)
        assert abs(got["loss"] - base["loss"]) <= 1e-15 and np.array_equal(got["dlogits"], base["dlogits"]) and got["sum_w"] == base["sum_w"]
    half = R.hard_tail(x, y, W6, np.full(40, 0.5, np.float32), grad_out=0.5)
    assert abs(half["loss"] - 0.5 * base["loss"]) <= 1e-15 and half["sum_w"] == base["sum_w"]  # the weights are not in the denominator


@pytest.mark.parametrize("C", [2, 6, 11, 32])
def test_float32_restatement_of_the_weight_against_float64(C):
    """The kernel's formula in numpy float32 on 3 * randn logits, 20000 rows, beta = 2: what float32 alone costs.  Observed largest
    |w32 - w64|: 1.1e-7 (C = 2), 1.2e-7 (6), 9.9e-8 (11), 1.3e-7 (32); largest |D32 - D64|: 1.3e-6, 2.3e-6, 3.1e-6, 6.5e-6 (D up
    to about 15; relative to max(1, D) at most 5.9e-7).  The GPU tests allow 1e-5 absolute on w (the cross-entropy pair's
    tolerance): eighty times this, which leaves room for the device's expf / logf (a few ulp each)."""
    a, b = R.make_pair(20000, C, 100 + C)
    ref = R.agreement(a, b, 2.0)
    d32, w32 = R.agreement_fp32(a, b, 2.0)
    ew = np.abs(w32.astype(np.float64) - ref["weight"]).max()
    ed = np.abs(d32.astype(np.float64) - ref["div"]).max()
    er = (np.abs(d32.astype(np.float64) - ref["div"]) / np.maximum(1.0, ref["div"])).max()
    print(f"C {C}: max |w32 - w64| {ew:.2e}, max |D32 - D64| {ed:.2e} (relative to max(1, D) {er:.2e}), max D {ref['div'].max():.2f}")
    assert ew <= 5e-7 and er <= 1e-6
    same = R.agreement_fp32(a, a, 2.0)
    assert (same[0] == 0).all() and (same[1] == 1).all()  # identical rows: exactly 1 in float32 too


# ---------------------------------------------------------------------------------------------- the option
def test_pl_agreement_defaults_to_none_and_leaves_nothing_behind():
    tm = _trainer()
    assert tm.pl_agreement is None and tm.last_agreement is None
    tm = _trainer(lambda_pl=1.0, pl_agreement=None)
    assert tm.pl_agreement is None and tm.last_agreement is None and tm.selftrain._agree is None


def test_pl_agreement_takes_a_finite_positive_number_whatever_lambda_pl_is():
    for good in (0.5, 1, 2.0, 1e-3, 100):
        for kw in (dict(), dict(lambda_pl=1.0), dict(lambda_pl=1.0, pseudo_label_source="teacher", ema_decay=0.9, pl_targets="soft",
                                                     pl_threshold="adaptive", pseudo_labels="ensemble")):
            tm = _trainer(pl_agreement=good, **kw)
            assert tm.pl_agreement == float(good) and isinstance(tm.pl_agreement, float) and tm.last_agreement is None
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "2", True, False, [2.0]):
        for kw in (dict(), dict(lambda_pl=1.0)):
            with pytest.raises(ValueError, match="pl_agreement") as e:
                _trainer(pl_agreement=bad, **kw)
            assert "finite number > 0" in str(e.value) and repr(bad) in str(e.value)


def test_the_state_is_forwarded_by_name():
    tm = _trainer(pl_agreement=2.0)
    assert tm.pl_agreement is tm.selftrain.pl_agreement
    tm.selftrain.last_agreement = {"weight": None}
    assert tm.last_agreement is tm.selftrain.last_agreement


def test_agreement_weights_refuses_bad_arguments_by_name():
    from mm2d3d_amd import pselab

    for bad in (0, -1.0, float("inf"), float("nan"), "2", True, None):
        with pytest.raises(ValueError, match="beta must be a finite number > 0"):
            pselab.agreement_weights(torch.zeros(4, 6), torch.zeros(4, 6), bad)
    with pytest.raises(RuntimeError, match="GPU"):  # no CPU fall-back
        pselab.agreement_weights(torch.zeros(4, 6), torch.zeros(4, 6), 1.0)


# ---------------------------------------------------------------------------------------------- the row weights of the pairs
def test_row_weights_are_checked_before_anything_else_looks_at_the_call():
    """Raised on the host from the arguments alone (the logits live on the CPU here: a launch would be refused, it is never reached)."""
    from mm2d3d_amd.losses import cross_entropy_pair, cross_entropy_soft_pair

    x, y, t = torch.zeros(10, 6), torch.zeros(6, dtype=torch.int64), torch.zeros(6, 6)
    calls = {"row_weight_tail": lambda w: cross_entropy_pair(x, 4, None, y, row_weight_tail=w),
             "row_weight": lambda w: cross_entropy_soft_pair(x, 4, None, t, row_weight=w)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name + r" requires grad.*not differentiated"):
            call(torch.ones(6, requires_grad=True))
        for bad in (torch.ones(5), torch.ones(7), torch.ones(6, 1), torch.ones(())):
            with pytest.raises(ValueError, match=name + r" must be a float32 tensor \[6\]"):
                call(bad)
        for bad in (torch.ones(6, dtype=torch.float64), torch.ones(6, dtype=torch.float16), torch.ones(6, dtype=torch.int64), [1.0] * 6, 1.0):
            with pytest.raises(ValueError, match=name + r" must be a float32 tensor \[6\]"):
                call(bad)
        with pytest.raises(RuntimeError, match="GPU"):  # a good weight vector passes the check; the CPU logits are refused next
            call(torch.ones(6))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_bindings_match():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp,
             "int": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.sz, "float": _lib.f32}
    want = {"mm_pl_agree_ws_bytes": 0, "mm_pl_agree": 13, "mm_ce2_fwd_w": 16, "mm_ce2_bwd_w": 16, "mm_ce2s_fwd_w": 21, "mm_ce2s_bwd_w": 21}
    for name, n_args in want.items():
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [] if m.group(2).strip() == "void" else [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctype[m.group(1)] and len(args) == len(params) == n_args, name
        assert args == [ctype[p] for p in params], (name, params)
    # the parents' argument lists plus row_w (the soft pair: plus thr_cls too)
    for parent, child, extra in (("mm_ce2_fwd", "mm_ce2_fwd_w", 1), ("mm_ce2_bwd", "mm_ce2_bwd_w", 1), ("mm_ce2s_fwd", "mm_ce2s_fwd_w", 2),
                                 ("mm_ce2s_bwd", "mm_ce2s_bwd_w", 2)):
        assert len(_lib._PROTOS[child][1]) == len(_lib._PROTOS[parent][1]) + extra


def test_pl_agree_argument_errors_come_before_any_launch():
    """Every refusal is decided on the host: these calls return without touching a device (there is none here)."""
    from mm2d3d_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_double * 64)()  # never read or written: every call below is refused
    p = ctypes.addressof(buf)
    need = int(L.mm_pl_agree_ws_bytes())
    assert need >= 1024 * 3 * 8

    def call(a=p, ld2=6, b=p, ld3=6, N=8, C=6, beta=1.0, w=p, stats=p, finite=p, ws=p, ws_bytes=need):
        return L.mm_pl_agree(a, ld2, b, ld3, N, C, beta, w, stats, finite, ws, ws_bytes, None)

    bad = [(dict(C=1, ld2=1, ld3=1), b"C must lie in [2, 32]"), (dict(C=33, ld2=33, ld3=33), b"C must lie in [2, 32]"), (dict(C=0), b"C must lie"),
           (dict(ld2=5), b"row pitch below C"), (dict(ld3=5), b"row pitch below C"), (dict(beta=0.0), b"beta"), (dict(beta=-1.0), b"beta"),
           (dict(beta=float("inf")), b"beta"), (dict(beta=float("nan")), b"beta"), (dict(N=-1), b"N * C"),
           (dict(N=(1 << 31) // 6 + 1), b"N * C must stay below 2^31"), (dict(N=1 << 26, C=32, ld2=32, ld3=32), b"N * C"),
           (dict(a=None), b"null logits"), (dict(b=None), b"null logits"), (dict(w=None), b"null logits or w"), (dict(stats=None), b"null stats"),
           (dict(ws=None), b"workspace"), (dict(ws_bytes=need - 1), b"workspace")]
    for kw, word in bad:
        assert call(**kw) == -1, kw
        assert b"pl_agree:" in L.mm_last_error() and word in L.mm_last_error(), (kw, L.mm_last_error())


def test_row_weight_entry_points_refuse_what_their_parents_refuse():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 20
    for kw in (dict(C=0), dict(C=33), dict(P=11), dict(P=-1)):
        a = dict(C=6, P=5)
        a.update(kw)
        assert L.mm_ce2_fwd_w(p, 40, 10, a["P"], a["C"], None, None, p, None, -100, 2, p, p, p, big, None) == -1
        assert b"ce2:" in L.mm_last_error()
        assert L.mm_ce2_bwd_w(p, 40, 10, a["P"], a["C"], None, None, p, None, -100, p, p, p, p, 40, None) == -1
        assert L.mm_ce2s_fwd_w(p, 40, 10, a["P"], a["C"], None, None, -100, p, 40, None, 0, 1.0, 0.0, None, p, p, None, p, big, None) == -1
        assert b"ce2s:" in L.mm_last_error()
        assert L.mm_ce2s_bwd_w(p, 40, 10, a["P"], a["C"], None, None, -100, p, 40, None, 0, 1.0, 0.0, None, p, p, p, p, 40, None) == -1
    # the scalar threshold is checked only where it is used: a non-NULL thr_cls wins
    assert L.mm_ce2s_fwd_w(p, 6, 10, 5, 6, None, None, -100, p, 6, None, 0, 1.0, 1.5, None, p, p, None, p, big, None) == -1
    assert b"threshold" in L.mm_last_error()
    assert L.mm_ce2s_fwd_w(p, 6, 10, 5, 6, None, None, -100, p, 6, None, 0, 1.0, 1.5, p, p, None, None, p, big, None) == -1
    assert b"null stats" in L.mm_last_error()  # past the threshold check
    assert L.mm_ce2_bwd_w(None, 6, 0, 0, 6, None, None, None, None, -100, None, None, None, None, 6, None) == 0  # no rows: no launch
