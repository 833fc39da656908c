"""Host checks of the adversarial output alignment: the float64 reference (tests/_adv_ref.py) against torch float64 autograd of the
same composition, the kink condition of the fixtures it shares with tests/test_gpu_adv.py, train_kwargs["lambda_adv"] /
["adv_*"] in the constructor (mm2d3d_amd/adversarial.py), the parameter layout and the seeded initialisation, the refusals of
losses.adversarial, and the declarations and argument checks of mm_adv_fwd / mm_adv_bwd (include/mm2d3d.h), every one of which is
decided before any device call.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _adv_ref as R


def _trainer(optimizer=None, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, optimizer, Loss("cross_entropy"),
                      dict(gc_freeze=False, **kw))


# ---------------------------------------------------------------------------------------------- the reference
def _torch_composition(x, P, params, C, H, mode):
    """The same arithmetic from torch ops in float64 on the CPU, differentiated by autograd: (loss_d, loss_g, dparams, gx, z1, z2)."""
    ok = torch.from_numpy(R.counted_rows(x))
    xt = torch.from_numpy(np.asarray(x, np.float64))[ok].requires_grad_(True)
    trg = (torch.arange(x.shape[0]) >= P)[ok]
    th = torch.from_numpy(np.asarray(params, np.float64)).requires_grad_(True)
    o = np.cumsum([0, H * C, H, H * H, H, H, 1])
    W1, b1, W2, b2, w3, b3 = (th[o[i]:o[i + 1]] for i in range(6))
    p = torch.softmax(xt, dim=1)
    u = p if mode == "softmax" else -p * torch.log_softmax(xt, dim=1) / math.log(C)
    z1 = F.linear(u, W1.view(H, C), b1)
    z2 = F.linear(F.leaky_relu(z1, 0.2), W2.view(H, H), b2)
    a = F.linear(F.leaky_relu(z2, 0.2), w3.view(1, H), b3).reshape(-1)
    zero = a.new_zeros(())
    # loss_D = 0.5 mean_src softplus(a) + 0.5 mean_trg softplus(-a): a source row is labelled 0, a target row 1
    ls =F.binary_cross_entropy_with_logits(a[~trg], torch.zeros_like(a[~trg])) if (~trg).any() else zero
    lt = F.binary_cross_entropy_with_logits(a[trg], torch.ones_like(a[trg])) if trg.any() else zero
    loss_d = 0.5 * ls + 0.5 * lt
    loss_g = F.binary_cross_entropy_with_logits(a[trg], torch.zeros_like(a[trg])) if trg.any() else zero
    (dparams,) = torch.autograd.grad(loss_d, th, retain_graph=True, allow_unused=True) if loss_d.requires_grad else (torch.zeros_like(th),)
    (gx,) = torch.autograd.grad(loss_g, xt, allow_unused=True) if loss_g.requires_grad else (None,)
    full = np.zeros(x.shape)
    if gx is not None:
        full[ok.numpy()] = gx.numpy()
    return float(loss_d.detach()), float(loss_g.detach()), dparams.numpy(), full, z1.detach().numpy(), z2.detach().numpy()


SMALL = [n for n in R.CASES if not n.startswith("131208")]


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_float64_autograd_of_the_same_composition(name, mode):
    c = R.case(name)
    ref = c["ref"][mode]
    ld, lg, dparams, gx, z1, z2 = _torch_composition(c["x"], c["P"], c["params"], c["C"], c["H"], mode)

    def close(a, b):
        return np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0) <= 1e-10 * max(np.abs(np.asarray(b)).max(initial=0.0), 1e-300)

    assert close(ref["loss_d"], ld) and close(ref["loss_g"], lg), (name, mode)
    assert close(ref["dparams"], dparams) and close(ref["gx"], gx), (name, mode)
    # the reference decides every LeakyReLU branch itself, from its own pre-activations, and they are torch's
    assert np.array_equal(ref["s1"], np.where(ref["z1"] > 0, 1.0, 0.2)) and np.array_equal(ref["s2"], np.where(ref["z2"] > 0, 1.0, 0.2))
    assert np.array_equal(ref["z1"] > 0, z1 > 0) and np.array_equal(ref["z2"] > 0, z2 > 0)
    ok = R.counted_rows(c["x"])
    n_s, n_t = int(ok[:c["P"]].sum()), int(ok[c["P"]:].sum())
    assert ref["count"] == [n_s, n_t] and 0 <= ref["correct"][0] <= n_s and 0 <= ref["correct"][1] <= n_t
    assert not ref["gx"][:c["P"]].any() and not ref["gx"][~ok].any()  # source and uncounted rows carry no generator gradient
    if n_t:
        assert ref["loss_g"] > 0.0 and np.abs(ref["gx"]).max() > 0.0
    if n_s + n_t:
        assert ref["loss_d"] > 0.0 and np.abs(ref["dparams"]).max() > 0.0
    else:
        assert ref["loss_d"] == 0.0 and not ref["dparams"].any()


def test_reference_handles_a_class_of_probability_zero():
    """A logit far below the maximum: p_c underflows to 0 in float64 too; u_c and its gradient share are 0, never NaN."""
    x = np.array([[0.0, -2000.0, 1.0], [0.5, 0.25, -1800.0]], np.float32)
    params = R.initial(3, 16)
    for mode in R.MODES:
        ref = R.evaluate(x, 0, params, 16, mode)
        assert np.isfinite(ref["gx"]).all() and np.isfinite(ref["dparams"]).all() and np.isfinite(ref["loss_g"])
        assert ref["gx"][0, 1] == 0.0 and ref["gx"][1, 2] == 0.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_kink_condition_holds_for_every_fixture(name):
    c = R.case(name)
    for mode, ref in c["ref"].items():
        s1, s2 = R.kink_shares(ref)
        print(f"{name} {mode}: share of units within their margin of 0: layer 1 {s1:.2e}, layer 2 {s2:.2e}; rows with |a| within its margin {R.uncertain_rows(ref)}")
        assert s1 <= R.KINK_CAP and s2 <= R.KINK_CAP, (name, mode)
        if not name.startswith("131208"):
            assert R.uncertain_rows(ref) == 0, (name, mode)
        bp, bg = R.bounds(ref)
        assert bp.shape == ref["dparams"].shape and bg.shape == ref["gx"].shape and np.isfinite(bp).all() and np.isfinite(bg).all()
        # the bounds are rounding bounds: far below the values they guard
        if ref["dparams"].any():
            assert np.median(bp / np.maximum(np.abs(ref["dparams"]), 1e-300)) < 1e-2, (name, mode)


# ---------------------------------------------------------------------------------------------- layout and initialisation
def test_parameter_layout_and_count():
    from mm2d3d_amd import _lib
    from mm2d3d_amd.losses import adversarial_param_count

    L = _lib.lib()
    for C, H in ((2, 16), (6, 64), (11, 32), (32, 64)):
        n = H * C + H * H + 3 * H + 1
        assert adversarial_param_count(C, H) == R.param_count(C, H) == int(L.mm_adv_param_count(C, H)) == n
        flat = np.arange(n, dtype=np.float64)
        W1, b1, W2, b2, w3, b3 = R.split(flat, C, H)
        assert W1.shape == (H, C) and W1[1, 0] == C and b1[0] == H * C and W2.shape == (H, H) and W2[0, 0] == H * C + H
        assert W2[1, 0] == H * C + 2 * H and b2[0] == H * C + H + H * H and w3[0] == b2[0] + H and b3 == n - 1
        assert np.array_equal(R.join(W1, b1, W2, b2, w3, b3), flat)
    assert [int(L.mm_adv_param_count(C, H)) for C, H in ((1, 16), (33, 16), (6, 8), (6, 48), (6, 128), (0, 0))] == [0] * 6


def test_seeded_initialisation_is_reproducible_and_private():
    from mm2d3d_amd.adversarial import OutputAdversary, initial_parameters

    torch.manual_seed(123)
    before = torch.get_rng_state()
    a = initial_parameters(6, 64, torch.Generator().manual_seed(0))
    b = initial_parameters(6, 64, torch.Generator().manual_seed(0))
    c = initial_parameters(6, 64, torch.Generator().manual_seed(1))
    adv = OutputAdversary(dict(lambda_adv=0.5, adv_seed=0))
    adv._build(6, torch.device("cpu"))
    assert torch.equal(torch.get_rng_state(), before)  # the global stream, and with it the dropout masks, is untouched
    assert a.dtype == torch.float32 and a.shape == (R.param_count(6, 64),) and torch.equal(a, b) and not torch.equal(a, c)
    # the two discriminators come from ONE private stream, the 2D head's first: they differ, and the first is the seed's first draw
    assert torch.equal(adv.params[0].detach(), a) and not torch.equal(adv.params[1].detach(), a)
    W1, b1, W2, b2, w3, b3 = R.split(a.numpy(), 6, 64)
    for part, fan_in in ((W1, 6), (b1, 6), (W2, 64), (b2, 64), (w3, 64)):  # nn.Linear's rule: uniform in +-1 / sqrt(fan_in)
        k = 1.0 / math.sqrt(fan_in)
        assert np.abs(part).max() <= k and np.abs(part).max() > 0.9 * k and abs(part.mean()) < 0.2 * k
    assert abs(b3) <= 1.0 / 8.0


# ---------------------------------------------------------------------------------------------- the constructor
def test_constructor_defaults_and_values():
    tm = _trainer()
    assert (tm.lambda_adv, tm.adv_input, tm.adv_hidden, tm.adv_lr, tm.adv_betas, tm.adv_seed) == (0.0, "selfinfo", 64, 1e-4, (0.9, 0.99), 0)
    assert tm.last_adversary is None and not tm.adversary.active and not tm.adversary.built
    assert tm.adversary.terms(None, None, 0) is None  # the weight 0: nothing is consulted
    assert "adversary" not in tm.checkpoint()
    tm = _trainer(lambda_adv=1, adv_input="softmax", adv_hidden=16, adv_lr=2e-4, adv_betas=[0.5, 0.9], adv_seed=7)
    assert (tm.lambda_adv, tm.adv_input, tm.adv_hidden, tm.adv_lr, tm.adv_betas, tm.adv_seed) == (1.0, "softmax", 16, 2e-4, (0.5, 0.9), 7)
    assert tm.adversary.active and not tm.adversary.built  # built at the first call, when C is known
    tm.lambda_adv = 0.5  # forwarded to the policy object, as the other options are
    assert tm.adversary.lambda_adv == 0.5
    tm = _trainer(lambda_adv=0.1, lambda_coral=0.1, lambda_minent=0.2, lambda_pl=1.0, pseudo_label_source="teacher", ema_decay=0.9)
    assert tm.lambda_adv == 0.1 and tm.lambda_coral == 0.1 and tm.lambda_minent == 0.2 and tm.lambda_pl == 1.0
    plain, on = _trainer(), _trainer(lambda_adv=0.3, adv_input="softmax")
    assert set(vars(plain)) == set(vars(on)) and set(vars(plain.adversary)) == set(vars(on.adversary))
    with torch.no_grad():  # outside a step with gradients nothing is built or called
        assert on.adversary.terms(torch.zeros(4, 6), torch.zeros(4, 6), 2) is None and not on.adversary.built


def test_constructor_refuses_every_bad_option_by_name():
    for bad in (-0.1, -1, float("nan"), float("inf"), "0.1", None, True, [0.1]):
        with pytest.raises(ValueError, match=r"train_kwargs\['lambda_adv'\] must be a finite number >= 0"):
            _trainer(lambda_adv=bad)
    for kw in (dict(), dict(lambda_adv=1.0)):  # whatever the weight is: a schedule must not hide an option that cannot run
        for bad in ("Softmax", "entropy", "", None, 1, True, ["softmax"]):
            with pytest.raises(ValueError, match=r"train_kwargs\['adv_input'\] must be \"selfinfo\" or \"softmax\""):
                _trainer(adv_input=bad, **kw)
        for bad in (8, 48, 128, 64.0, "64", None, True):
            with pytest.raises(ValueError, match=r"train_kwargs\['adv_hidden'\] must be 16, 32 or 64"):
                _trainer(adv_hidden=bad, **kw)
        for bad in (-1e-4, float("nan"), float("inf"), "1e-4", None, True):
            with pytest.raises(ValueError, match=r"train_kwargs\['adv_lr'\]"):
                _trainer(adv_lr=bad, **kw)
        for bad in (0.9, (0.9,), (0.9, 1.0), (-0.1, 0.9), (0.9, 0.99, 0.999), ("0.9", 0.99), None, (True, 0.9)):
            with pytest.raises(ValueError, match=r"train_kwargs\['adv_betas'\]"):
                _trainer(adv_betas=bad, **kw)
        for bad in (0.5, "0", None, True):
            with pytest.raises(ValueError, match=r"train_kwargs\['adv_seed'\]"):
                _trainer(adv_seed=bad, **kw)


# ---------------------------------------------------------------------------------------------- losses.adversarial
def test_adversarial_refusals_come_before_any_launch():
    from mm2d3d_amd.losses import adversarial

    n = R.param_count(6, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        adversarial(torch.zeros(10, 6), 5, torch.zeros(n))
    meta, params = torch.zeros(10, 6, device="meta"), torch.zeros(n, device="meta")
    for bad in (torch.zeros(10, device="meta"), torch.zeros(10, 1, device="meta"), torch.zeros(10, 33, device="meta"), [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="adversarial"):
            adversarial(bad, 0, params)
    for bad in (-1, 11, 1.0, True, None):
        with pytest.raises(ValueError, match="first_row"):
            adversarial(meta, bad, params)
    for bad in ("Selfinfo", "", None, 1):
        with pytest.raises(ValueError, match="mode"):
            adversarial(meta, 5, params, bad)
    for bad in (8, 48, 64.0, None, True):
        with pytest.raises(ValueError, match="hidden"):
            adversarial(meta, 5, params, "selfinfo", bad)
    for bad in (torch.zeros(n - 1, device="meta"), torch.zeros(n, dtype=torch.float64, device="meta"), torch.zeros(1, n, device="meta"),
                torch.zeros(2 * n, device="meta")[::2], None, torch.zeros(R.param_count(6, 16), device="meta")):
        with pytest.raises(ValueError, match="params"):
            adversarial(meta, 5, bad)
    with pytest.raises(ValueError, match=r"2\^31"):
        adversarial(torch.zeros((1 << 31) // 32, 32, device="meta"), 5, torch.zeros(R.param_count(32, 64), device="meta"))


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
    for name, n in (("mm_adv_fwd", 17), ("mm_adv_bwd", 8)):
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is _lib.i32 and len(args) == len(params) == n, name
        assert args == [ctype[p] for p in params], (name, params)
    assert hasattr(lib, "mm_adv_ws_bytes") and _lib._PROTOS["mm_adv_ws_bytes"] == (_lib.sz, [_lib.i32, _lib.i32])
    assert hasattr(lib, "mm_adv_param_count") and _lib._PROTOS["mm_adv_param_count"] == (_lib.i64, [_lib.i32, _lib.i32])
    assert re.search(r"\bsize_t\s+mm_adv_ws_bytes\s*\(\s*int\s+C\s*,\s*int\s+H\s*\)\s*;", txt)
    assert re.search(r"\bint64_t\s+mm_adv_param_count\s*\(\s*int\s+C\s*,\s*int\s+H\s*\)\s*;", txt)


def test_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep = (ctypes.c_double * 256)()  # never read or written: every call below is refused before a device call
    p = ctypes.addressof(keep)
    need = int(L.mm_adv_ws_bytes(6, 64))
    assert need >= 2 * (R.param_count(6, 64) + 3) * 8  # at least two workgroups' slabs: the grid is capped, not one
    assert [int(L.mm_adv_ws_bytes(C, H)) for C, H in ((1, 16), (33, 64), (6, 8), (6, 48), (6, 0), (-1, 16))] == [0] * 6
    assert int(L.mm_adv_ws_bytes(32, 64)) > need > int(L.mm_adv_ws_bytes(6, 16)) > 0

    def fwd(x=p, ld=6, N=8, P=4, C=6, H=64, mode=1, params=p, stats=p, count=p, correct=p, dparams=p, gx=p, ld_gx=6, ws=p, ws_bytes=need):
        return L.mm_adv_fwd(x, ld, N, P, C, H, mode, params, stats, count, correct, dparams, gx, ld_gx, ws, ws_bytes, None)

    def bwd(gx=p, ld_gx=6, N=8, C=6, g=p, dx=p, ld_dx=6):
        return L.mm_adv_bwd(gx, ld_gx, N, C, g, dx, ld_dx, None)

    for kw in (dict(C=1), dict(C=0), dict(C=33), dict(H=8), dict(H=48), dict(H=128), dict(H=0), dict(ld=5), dict(ld_gx=5), dict(C=32, ld=31),
               dict(N=-1), dict(P=-1), dict(P=9), dict(N=(1 << 31) // 6 + 1, P=0), dict(N=1 << 40, P=0), dict(x=None), dict(gx=None),
               dict(mode=2), dict(mode=-1), dict(params=None), dict(stats=None), dict(count=None), dict(correct=None), dict(dparams=None),
               dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(N=0, P=0, stats=None), dict(N=0, P=0, ws_bytes=0),
               dict(N=0, P=0, C=33)):  # N == 0 still runs the finish
        assert fwd(**kw) == -1, kw
        assert b"adv_fwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    for kw in (dict(C=1), dict(C=33), dict(ld_gx=5), dict(ld_dx=5), dict(ld_dx=0), dict(N=-1), dict(N=(1 << 31) // 6 + 1), dict(g=None),
               dict(gx=None), dict(dx=None), dict(N=0, C=1)):
        assert bwd(**kw) == -1, kw
        assert b"adv_bwd:" in L.mm_last_error(), (kw, L.mm_last_error())
    assert bwd(N=0, gx=None, dx=None) == 0  # nothing to write
