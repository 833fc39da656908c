"""Host checks of the correlation-alignment losses: the float64 reference (tests/_coral_ref.py) against central differences of its
own loss and against the closed form, train_kwargs["lambda_coral"] / ["coral"] / ["coral_eps"] in the constructor
(mm2d3d_amd/coral.py), the refusals of losses.coral, and the declarations and argument checks of mm_coral_fwd / mm_coral_bwd
(include/mm2d3d.h), every one of which is decided before any device call.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _coral_ref as R


def _trainer(optimizer=None, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, optimizer, Loss("cross_entropy"),
                      dict(gc_freeze=False, **kw))


def _rows(N, d, seed):
    """Seeded randn rows mixed by a seeded d x d matrix: the covariances are not diagonal."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, d)) @ rng.standard_normal((d, d)) + rng.standard_normal(d)


def _cases():
    well = _rows(40, 4, 1)
    well[25:] *= 1.7  # the two domains differ
    deficient = _rows(16, 5, 2)  # P = 13: n_t = 3 < d, the target's covariance has rank 2 and the ridge carries it
    holes = _rows(30, 3, 3)
    holes[4, 1] = np.nan  # one non-finite row per segment
    holes[20] = np.inf
    return {"well_conditioned": (well, 25), "rank_deficient": (deficient, 13), "non_finite_rows": (holes, 12)}


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("mode", ["plain", "log"])
@pytest.mark.parametrize("name", list(_cases()))
def test_reference_gradient_matches_central_differences(name, mode):
    """h = 1e-5 in float64, bound 1e-5 * max(1, max |g|), set by the hardest case, the rank-deficient one in log mode.  Rounding:
    its eigenvalues eps = 1e-4 carry eigh's absolute error, 2^-53 * ||C|| (about 10) * a few = 1e-15, that is 1e-11 relative, which
    the logarithm hands to a loss of order 10 as 1e-10; divided by h: 1e-5.  Truncation: (h / h*)^2 with h* = sqrt(eps) = 1e-2, the
    scale on which a row that leaves the span of its segment moves an eps eigenvalue: 1e-6.  A wrong term of the gradient shows at
    the size of the gradient itself, 0.1 to 1."""
    x, P = _cases()[name]
    eps = 1e-4
    f = R.evaluate(x, P, mode, eps)
    num = R.numeric_gradient(x, P, mode, eps, h=1e-5)
    err, top = np.abs(f["grad"] - num).max(), np.abs(num).max()
    print(f"{name} {mode}: loss {f['loss']:.6g}  max |g| {top:.3e}  max |analytic - central difference| {err:.2e}")
    assert f["loss"] > 0.0 and top > 0.0
    assert err <= 1e-5 * max(1.0, top)
    dead = ~R.counted_rows(x)
    assert not f["grad"][dead].any() and dead.sum() == (2 if name == "non_finite_rows" else 0)
    if name == "non_finite_rows":
        assert f["count"] == [11, 17]
    if name == "rank_deficient":
        assert f["count"] == [13, 3] and np.linalg.matrix_rank(f["cov"][1]) == 2


def test_plain_equals_the_closed_form_computed_directly():
    x, P = _cases()["well_conditioned"]
    d = x.shape[1]
    cs, ct = np.cov(x[:P].T), np.cov(x[P:].T)  # unbiased, 1 / (n - 1)
    f = R.evaluate(x, P, "plain")
    np.testing.assert_allclose(f["cov"], np.stack((cs, ct)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(f["mean"], np.stack((x[:P].mean(0), x[P:].mean(0))), rtol=0, atol=1e-14)
    assert abs(f["loss"] - ((cs - ct) ** 2).sum() / (4 * d * d)) <= 1e-12 * f["loss"]
    # by hand, d = 2: C_s = diag(1, 4) -> rows (+-1, +-2) / sqrt(2) ...; C_t = I: loss = (0 + 9) / 16
    s = np.array([[1.0, 2.0], [-1.0, 2.0], [1.0, -2.0], [-1.0, -2.0]]) * np.sqrt(3.0 / 4.0)
    t = np.array([[1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]]) * np.sqrt(3.0 / 4.0)
    g = R.evaluate(np.concatenate((s, t)), 4, "plain")
    np.testing.assert_allclose(g["cov"], [np.diag([1.0, 4.0]), np.eye(2)], rtol=0, atol=1e-15)
    assert abs(g["loss"] - 9.0 / 16.0) < 1e-15
    # ... and the log form of the same: log C_s - log C_t = diag(0, ln 4) up to the ridge
    lg = R.evaluate(np.concatenate((s, t)), 4, "log", eps=1e-9)
    assert abs(lg["loss"] - np.log(4.0) ** 2 / 4.0) < 1e-8
    # identical domains: no loss, no gradient, in both modes (equal eigenvalues divide cleanly)
    for mode in ("plain", "log"):
        same = R.evaluate(np.concatenate((x[:P], x[:P])), P, mode)
        assert same["loss"] <= 1e-25 and np.abs(same["grad"]).max() <= 1e-12


@pytest.mark.parametrize("mode", ["plain", "log"])
def test_fewer_than_two_counted_rows_give_zero(mode):
    x = _rows(9, 3, 4)
    for P in (0, 1, 8, 9):
        f = R.evaluate(x, P, mode)
        assert f["loss"] == 0.0 and not f["grad"].any() and not f["aux"].any() and f["count"] == [P, 9 - P]
    y = x.copy()
    y[1:4] = np.nan  # the source keeps one counted row of four
    f = R.evaluate(y, 4, mode)
    assert f["loss"] == 0.0 and not f["grad"].any() and f["count"] == [1, 5] and not f["cov"][0].any() and f["cov"][1].any()
    e = R.evaluate(np.zeros((0, 3)), 0, mode)
    assert e["loss"] == 0.0 and e["count"] == [0, 0] and not e["mean"].any()


# ---------------------------------------------------------------------------------------------- the constructor
def test_constructor_defaults_and_values():
    tm = _trainer()
    assert tm.lambda_coral == 0.0 and tm.coral == "log" and tm.coral_eps == 1e-4 and tm.last_coral is None and not tm.alignment.active
    assert tm.alignment.terms(None, None, 0) is None  # the weight 0: nothing is consulted
    tm = _trainer(lambda_coral=1, coral="plain", coral_eps=1e-3)
    assert tm.lambda_coral == 1.0 and tm.coral == "plain" and tm.coral_eps == 1e-3 and tm.alignment.active
    tm.lambda_coral = 0.5  # forwarded to the policy object, as the other options are
    assert tm.alignment.lambda_coral == 0.5
    # independent of the self-training and the entropy options: they compose
    tm = _trainer(lambda_coral=0.1, lambda_minent=0.2, lambda_pl=1.0, pseudo_label_source="teacher", ema_decay=0.9)
    assert tm.lambda_coral == 0.1 and tm.lambda_minent == 0.2 and tm.lambda_pl == 1.0
    plain, on = _trainer(), _trainer(lambda_coral=0.3, coral="plain")
    assert set(vars(plain)) == set(vars(on)) and set(vars(plain.alignment)) == set(vars(on.alignment))


def test_constructor_refuses_every_bad_option_by_name():
    for bad in (-0.1, -1, float("nan"), float("inf"), "0.1", None, True, [0.1]):
        with pytest.raises(ValueError, match="lambda_coral"):
            _trainer(lambda_coral=bad)
    for bad in ("Log", "logcoral", "", None, 1, True, ["log"]):
        for kw in (dict(), dict(lambda_coral=1.0)):  # whatever the weight is: a schedule must not hide an option that cannot run
            with pytest.raises(ValueError, match=r"train_kwargs\['coral'\]"):
                _trainer(coral=bad, **kw)
    for bad in (0.0, -1e-4, float("nan"), float("inf"), "1e-4", None, True, [1e-4]):
        for kw in (dict(), dict(lambda_coral=1.0)):
            with pytest.raises(ValueError, match="coral_eps"):
                _trainer(coral_eps=bad, **kw)


# ---------------------------------------------------------------------------------------------- losses.coral
def test_coral_refusals_come_before_any_launch():
    from mm2d3d_amd.losses import coral

    with pytest.raises(RuntimeError, match="GPU"):
        coral(torch.zeros(10, 6), 5)
    meta = torch.zeros(10, 6, device="meta")  # refused on their values before the device is looked at
    for bad in (torch.zeros(10, device="meta"), torch.zeros(10, 1, device="meta"), torch.zeros(10, 33, device="meta"), [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="coral"):
            coral(bad, 0)
    for bad in (-1, 11, 1.0, True, None):
        with pytest.raises(ValueError, match="first_row"):
            coral(meta, bad)
    for bad in ("Log", "", None, 1):
        with pytest.raises(ValueError, match="mode"):
            coral(meta, 5, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1e-4", None, True):
        with pytest.raises(ValueError, match="eps"):
            coral(meta, 5, "log", bad)
    with pytest.raises(ValueError, match=r"2\^31"):
        coral(torch.zeros((1 << 31) // 32, 32, device="meta"), 5)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_bindings_match():
    import os
    import re

    from mm2d3d_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp, "int": _lib.i32,
             "int64_t": _lib.i64, "size_t": _lib.sz, "float": _lib.f32}
    for name, n in (("mm_coral_fwd", 15), ("mm_coral_bwd", 10)):
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is _lib.i32 and len(args) == len(params) == n, name
        assert args == [ctype[p] for p in params], (name, params)
    assert hasattr(lib, "mm_coral_ws_bytes") and _lib._PROTOS["mm_coral_ws_bytes"] == (_lib.sz, [_lib.i32])
    assert re.search(r"\bsize_t\s+mm_coral_ws_bytes\s*\(\s*int\s+d\s*\)\s*;", txt)


def test_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep = (ctypes.c_double * 256)()  # never read or written: every call below is refused before a device call
    p = ctypes.addressof(keep)
    need = int(L.mm_coral_ws_bytes(6))
    assert need >= 1024 * 2 * (6 + 21) * 8 + 1024 * 2 * 8  # 1024 workgroups' fp64 sums and integer counts of both segments
    assert int(L.mm_coral_ws_bytes(32)) >= 1024 * 2 * (32 + 528) * 8 + 1024 * 2 * 8
    assert [int(L.mm_coral_ws_bytes(d)) for d in (1, 0, -1, 33)] == [0, 0, 0, 0]

    def fwd(x=p, ld=6, N=8, P=4, d=6, mode=1, eps=1e-4, loss=p, count=p, mean=p, cov=p, aux=p, ws=p, ws_bytes=need):
        return L.mm_coral_fwd(x, ld, N, P, d, mode, eps, loss, count, mean, cov, aux, ws, ws_bytes, None)

    def bwd(x=p, ld=6, N=8, P=4, d=6, aux=p, g=p, dx=p, ld_dx=6):
        return L.mm_coral_bwd(x, ld, N, P, d, aux, g, dx, ld_dx, None)

    shared = [dict(d=1), dict(d=0), dict(d=-1), dict(d=33), dict(ld=5), dict(ld=0), dict(d=32, ld=31), dict(N=-1), dict(P=-1), dict(P=9),
              dict(N=(1 << 31) // 6 + 1, P=0), dict(N=1 << 40, P=0), dict(x=None), dict(aux=None)]
    for kw in shared:
        assert fwd(**kw) == -1, kw
        assert b"coral_fwd:" in L.mm_last_error(), (kw, L.mm_last_error())
        assert bwd(**kw) == -1, kw
        assert b"coral_bwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    for kw in (dict(mode=2), dict(mode=-1), dict(eps=0.0), dict(eps=-1e-4), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(loss=None), dict(count=None), dict(mean=None), dict(cov=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(d=7, ld=7), dict(N=0, P=0, loss=None), dict(N=0, P=0, ws_bytes=0), dict(N=0, P=0, d=33)):  # N == 0 still runs the finish
        assert fwd(**kw) == -1, kw
        assert b"coral_fwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    for kw in (dict(ld_dx=5), dict(ld_dx=0), dict(g=None), dict(dx=None), dict(N=0, P=0, d=1)):
        assert bwd(**kw) == -1, kw
        assert b"coral_bwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    assert bwd(N=0, P=0, x=None, dx=None) == 0  # nothing to write
