"""Host checks of the target-domain entropy and diversity losses: the float64 reference (tests/_infomax_ref.py) against central
differences and against examples worked by hand, train_kwargs["lambda_minent"] / ["lambda_div"] / ["div_prior"] in the constructor
(mm2d3d_amd/infomax.py), the refusals of losses.target_entropy, and the argument checks of mm_im_fwd / mm_im_bwd
(include/mm2d3d.h), every one of which is decided before any device call.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _infomax_ref as R

N, P = 37, 11


def _trainer(optimizer=None, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, optimizer, Loss("cross_entropy"),
                      dict(gc_freeze=False, **kw))


def _logits(C):
    rng = np.random.default_rng(77 + C)
    x = 3.0 * rng.standard_normal((N, C))
    x[P + 3] = np.nan  # a NaN row and a +inf row among the target rows
    x[P + 9, C - 1] = np.inf
    x[2, 0] = np.nan  # and one in the head, which nothing reads
    return x, rng.uniform(0.2, 2.0, C)


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("with_prior", [False, True], ids=["uniform", "prior"])
@pytest.mark.parametrize("C", [2, 5, 6, 32])
def test_reference_gradient_matches_central_differences(C, with_prior):
    """h = 1e-6 in float64: truncation h^2 |f'''| / 6 ~ 1e-12 / n and rounding eps / h ~ 1e-10; the bound is 1e-8 absolute."""
    x, w = _logits(C)
    prior = w if with_prior else None
    f = R.forward(x, P, prior)
    assert f["count"] == N - P - 2 and 0.0 < f["ent"] < 1.0 and f["div"] > 0.0 and abs(f["mass"].sum() - 1.0) < 1e-12
    de, dd = R.gradients(x, P, prior)
    ne, nd = R.numeric_gradients(x, P, prior, h=1e-6)
    err = max(np.abs(de - ne).max(), np.abs(dd - nd).max())
    print(f"C {C} prior {with_prior}: max |analytic - central difference| {err:.2e}")
    assert err <= 1e-8
    dead = ~R.counted_rows(x, P)
    assert dead[:P].all() and dead[P + 3] and dead[P + 9] and dead.sum() == P + 2
    assert not de[dead].any() and not dd[dead].any() and np.abs(de[~dead]).max() > 0 and np.abs(dd[~dead]).max() > 0


def test_reference_on_examples_worked_by_hand():
    ln2 = math.log(2.0)
    # C = 2, rows softmax (0.25, 0.75) and (0.9, 0.1): H = -(.25 ln .25 + .75 ln .75), -(.9 ln .9 + .1 ln .1); mass (0.575, 0.425)
    x = np.array([[7.0, 7.0], [0.0, math.log(3.0)], [math.log(9.0), 0.0]])
    f = R.forward(x, 1)
    H = [-(0.25 * math.log(0.25) + 0.75 * math.log(0.75)), -(0.9 * math.log(0.9) + 0.1 * math.log(0.1))]
    assert f["count"] == 2 and abs(f["ent"] - sum(H) / (2 * ln2)) < 1e-15
    np.testing.assert_allclose(f["mass"], [0.575, 0.425], rtol=0, atol=1e-15)
    assert abs(f["div"] - (0.575 * math.log(0.575 / 0.5) + 0.425 * math.log(0.425 / 0.5)) / ln2) < 1e-15
    # a prior equal to the mass: no divergence; priors are normalised
    assert abs(R.forward(x, 1, [5.75, 4.25])["div"]) < 1e-15
    # all-zero logits: the uniform prediction, entropy 1 and divergence 0
    z = R.forward(np.zeros((9, 5)), 2)
    assert z["count"] == 7 and abs(z["ent"] - 1.0) < 1e-15 and abs(z["div"]) < 1e-15
    # saturated rows stay finite (0 * log 0 = 0); the issue's figures
    s = R.forward(np.array([[90.0, -90.0, 0.0], [-80.0, 80.0, 80.0], [0.0, 0.0, 0.0]]), 0)
    assert abs(s["ent"] - 0.54364) < 5e-6 and abs(s["div"] - 0.02418) < 5e-6
    # nothing counted: zeros, never 0 / 0
    for bad in (np.full((4, 3), np.nan), np.zeros((0, 3)), np.array([[0.0, -np.inf, 1.0]])):
        e = R.forward(bad, 0)
        assert e == dict(ent=0.0, div=0.0, mass=e["mass"], count=0) and not e["mass"].any()
        assert not any(g.any() for g in R.gradients(bad, 0))
    e = R.forward(x, 3)  # P == N
    assert e["count"] == 0 and e["ent"] == 0.0 and e["div"] == 0.0


# ---------------------------------------------------------------------------------------------- the constructor
def test_constructor_defaults_and_values():
    tm = _trainer()
    assert tm.lambda_minent == 0.0 and tm.lambda_div == 0.0 and tm.div_prior is None and tm.last_target_mass is None
    assert not tm.target_entropy.active
    tm = _trainer(lambda_minent=0.3, lambda_div=1, div_prior=[1, 1, 2])
    assert tm.lambda_minent == 0.3 and tm.lambda_div == 1.0 and tm.div_prior == (0.25, 0.25, 0.5) and tm.target_entropy.active
    assert _trainer(lambda_div=0.1).target_entropy.active and _trainer(lambda_minent=0.1).target_entropy.active
    assert _trainer(div_prior=torch.tensor([1.0, 3.0])).div_prior == (0.25, 0.75)
    tm.lambda_div = 0.5  # forwarded to the policy object, as the self-training options are
    assert tm.target_entropy.lambda_div == 0.5
    # independent of the self-training options: they compose
    tm = _trainer(lambda_minent=0.1, lambda_pl=1.0, pseudo_label_source="teacher", ema_decay=0.9, pl_threshold="adaptive")
    assert tm.lambda_minent == 0.1 and tm.lambda_pl == 1.0


def test_constructor_refuses_bad_weights_and_priors():
    for name in ("lambda_minent", "lambda_div"):
        for bad in (-0.1, -1, float("nan"), float("inf"), "0.1", None, True, [0.1]):
            with pytest.raises(ValueError, match=name):
                _trainer(**{name: bad})
    for bad in ([1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, float("inf")], [], "uniform", 0.5, [[0.5, 0.5]], [True, 1.0],
                torch.ones(2, 2), torch.tensor([1.0, 0.0])):
        for kw in (dict(), dict(lambda_div=0.2)):  # also with the terms off: a schedule must not hide a prior that cannot run
            with pytest.raises(ValueError, match="div_prior"):
                _trainer(div_prior=bad, **kw)


def test_a_prior_of_the_wrong_length_is_refused_by_name_of_the_class_count():
    tm = _trainer(lambda_div=0.2, div_prior=[1.0, 1.0, 1.0])  # heads: Linear(2, 2)
    with pytest.raises(ValueError, match=r"div_prior.*3 entries.*C = 2"):
        tm.target_entropy.begin_step(tm)
    ok = _trainer(lambda_div=0.2, div_prior=[1.0, 3.0])
    ok.target_entropy.begin_step(ok)
    off = _trainer(div_prior=[1.0, 1.0, 1.0])  # both weights 0: nothing is consulted
    off.target_entropy.begin_step(off)
    assert off.target_entropy.terms(None, None, 0) is None
    named = _trainer(lambda_minent=0.2, div_prior=[1.0, 1.0, 1.0], num_classes=6)
    with pytest.raises(ValueError, match="C = 6"):
        named.target_entropy.begin_step(named)


def test_the_options_add_no_attribute():
    plain, on = _trainer(), _trainer(lambda_minent=0.3, lambda_div=0.2, div_prior=[1.0, 2.0])
    assert set(vars(plain)) == set(vars(on)) and set(vars(plain.target_entropy)) == set(vars(on.target_entropy))


# ---------------------------------------------------------------------------------------------- losses.target_entropy
def test_target_entropy_refusals_come_before_any_launch():
    from mm2d3d_amd.losses import target_entropy

    x = torch.zeros(10, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        target_entropy(x)
    meta = torch.zeros(10, 6, device="meta")  # refused on their values before the device is looked at
    for bad in (torch.zeros(10, device="meta"), torch.zeros(10, 1, device="meta"), torch.zeros(10, 33, device="meta"), [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="target_entropy"):
            target_entropy(bad)
    for bad in (-1, 11, 1.0, True, None):
        with pytest.raises(ValueError, match="first_row"):
            target_entropy(meta, bad)
    for bad in ([1.0] * 5, [1.0] * 7, torch.ones(5)):
        with pytest.raises(ValueError, match="C = 6"):
            target_entropy(meta, 0, bad)
    for bad in ([1.0, 1.0, 1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0, float("nan")], "uniform", 1.0, torch.ones(1, 6)):
        with pytest.raises(ValueError, match="prior"):
            target_entropy(meta, 0, bad)
    with pytest.raises(ValueError, match=r"2\^31"):
        target_entropy(torch.zeros((1 << 31) // 32, 32, device="meta"))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_bindings_match():
    import os
    import re

    from mm2d3d_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp, "int": _lib.i32,
             "int64_t": _lib.i64, "size_t": _lib.sz}
    for name, n in (("mm_im_fwd", 13), ("mm_im_bwd", 10)):
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is _lib.i32 and len(args) == len(params) == n, name
        assert args == [ctype[p] for p in params], (name, params)
    assert hasattr(lib, "mm_im_ws_bytes") and _lib._PROTOS["mm_im_ws_bytes"] == (_lib.sz, [])
    assert re.search(r"\bsize_t\s+mm_im_ws_bytes\s*\(\s*void\s*\)\s*;", txt)


def test_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep = (ctypes.c_double * 256)()  # never read or written: every call below is refused before a device call
    p = ctypes.addressof(keep)
    need = int(L.mm_im_ws_bytes())
    assert need >= 1024 * 33 * 8 + 1024 * 8  # 1024 workgroups' fp64 sums and integer counts at C = 32

    def fwd(x=p, ld=6, N=8, P=4, C=6, prior=None, stats=p, mass=p, count=p, aux=p, ws=p, ws_bytes=need):
        return L.mm_im_fwd(x, ld, N, P, C, prior, stats, mass, count, aux, ws, ws_bytes, None)

    def bwd(x=p, ld=6, N=8, P=4, C=6, aux=p, g=p, d=p, ld_d=6):
        return L.mm_im_bwd(x, ld, N, P, C, aux, g, d, ld_d, None)

    shared = [dict(C=1), dict(C=0), dict(C=-1), dict(C=33), dict(ld=5), dict(ld=0), dict(C=32, ld=31), dict(N=-1), dict(P=-1), dict(P=9),
              dict(N=(1 << 31) // 6 + 1, P=0), dict(N=1 << 40, P=0), dict(x=None), dict(aux=None)]
    for kw in shared:
        assert fwd(**kw) == -1, kw
        assert b"im_fwd:" in L.mm_last_error(), (kw, L.mm_last_error())
        assert bwd(**kw) == -1, kw
        assert b"im_bwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    for kw in (dict(stats=None), dict(mass=None), dict(count=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(N=0, P=0, stats=None), dict(N=0, P=0, ws_bytes=0), dict(N=0, P=0, C=33)):  # N == 0 still runs the finalise
        assert fwd(**kw) == -1, kw
        assert b"im_fwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    for kw in (dict(ld_d=5), dict(ld_d=0), dict(g=None), dict(d=None), dict(N=0, P=0, C=1)):
        assert bwd(**kw) == -1, kw
        assert b"im_bwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    assert bwd(N=0, P=0, x=None, d=None) == 0  # nothing to write
