"""CPU checks of what tests/test_gpu_bn_rows.py relies on: the float64 reference of tests/_bn_ref.py against torch's batch norm and
autograd, the guard band and the exactness of every GPU case's inputs, the fp32 restatements' error (the constants the GPU bounds
are eight times of), the case table's claims and the prototypes of the entries."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as B
import test_gpu_bn_rows as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = G.cases(G.MI355X_CUS)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _torch_bn(x, dy, N, Ns, w, b, rm, rv, eps, keep, leak):
    """Two statistics groups are two consecutive calls of torch's batch norm on the same module state."""
    xt = torch.from_numpy(x).requires_grad_(True)
    wt = None if w is None else torch.from_numpy(w).requires_grad_(True)
    bt = None if b is None else torch.from_numpy(b).requires_grad_(True)
    rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    ys = []
    for a, e in B.groups(N, Ns):
        if e - a == 1:  # torch refuses one value per channel in training mode; the kernels' rule is variance 0 (include/mm2d3d.h)
            v = torch.zeros_like(xt[a:e]) * (1.0 if wt is None else wt) + (0.0 if bt is None else bt)
            rmt, rvt = keep * rmt + (1 - keep) * xt[a:e].detach()[0], keep * rvt
        else:
            v = F.batch_norm(xt[a:e], rmt, rvt, wt, bt, True, 1.0 - keep, eps)
        ys.append(F.leaky_relu(v, leak))
    y = torch.cat(ys)
    y.backward(torch.from_numpy(dy))
    return (y.detach().numpy(), xt.grad.numpy(), None if wt is None else wt.grad.numpy(), None if bt is None else bt.grad.numpy(),
            rmt.numpy(), rvt.numpy())


@pytest.mark.parametrize("N, Ns, C, weight, bias, leak, keep", [
    (257, 0, 5, True, True, 0.333, 0.9), (257, 100, 5, True, True, 0.0, 0.99), (64, 63, 3, True, True, 0.333, 0.9),
    (300, 0, 4, False, True, 0.333, 0.9), (300, 7, 4, True, False, 0.0, 0.9), (300, 299, 4, False, False, 0.333, 0.99)])
def test_reference_matches_torch_batch_norm_and_autograd(N, Ns, C, weight, bias, leak, keep):
    d = B.make_inputs(f"host_{N}_{Ns}_{C}", N, Ns, C, "fp32", "normal", weight, bias, 1e-4, leak)
    r = B.bn_ref(d["x"], d["dy"], N, Ns, d["weight"], d["bias"], d["rm0"], d["rv0"], 1e-4, keep, leak, 1, d["dw0"], d["db0"])
    y, dx, dw, db, rm, rv = _torch_bn(d["x"], d["dy"], N, Ns, d["weight"], d["bias"], d["rm0"], d["rv0"], 1e-4, keep, leak)
    errs = dict(y=_rel(r["y"], y), dx=_rel(r["dx"], dx), rm=_rel(r["running_mean"], rm), rv=_rel(r["running_var"], rv))
    if weight:
        errs["dw"] = _rel(r["dweight"] - d["dw0"], dw)
    if bias:
        errs["db"] = _rel(r["dbias"] - d["db0"], db)
    print(errs)
    assert max(errs.values()) <= 1e-12, errs
    # without accumulation the previous contents do not enter
    r0 = B.bn_ref(d["x"], d["dy"], N, Ns, d["weight"], d["bias"], d["rm0"], d["rv0"], 1e-4, keep, leak, 0, d["dw0"], d["db0"])
    assert np.array_equal(r0["dweight"], r["S2"].sum(0)) and np.array_equal(r0["dbias"], r["S1"].sum(0))
    # eval, from the running buffers
    ye = B.bn_eval_ref(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], 1e-4, leak)
    wt, bt = (None if a is None else torch.from_numpy(a) for a in (d["weight"], d["bias"]))
    yt = F.leaky_relu(F.batch_norm(torch.from_numpy(d["x"]), torch.from_numpy(d["rm0"]), torch.from_numpy(d["rv0"]), wt, bt, False, 0.1, 1e-4), leak)
    assert _rel(ye, yt.numpy()) <= 1e-12


def test_zero_takes_the_leak_branch_and_a_group_of_one_row_has_variance_zero():
    x = np.array([[1.0], [-1.0], [0.0], [0.0]])
    r = B.bn_ref(x, np.ones((4, 1)), 4, 0, None, None, np.zeros(1), np.ones(1), 1e-4, 0.9, 0.25)
    assert (r["y"][2:] == 0).all() and (r["g"][:, 0] == [1.0, 0.25, 0.25, 0.25]).all()
    r = B.bn_ref(np.array([[3.0, -2.0]]), None, 1, 0, None, None, np.zeros(2), np.ones(2), 1e-4, 0.9, 0.0)
    assert (r["var"] == 0).all() and np.allclose(r["running_var"], 0.9) and np.allclose(r["running_mean"], [0.3, -0.2])
    assert np.allclose(r["save_invstd"], 100.0)


def test_formats_round_once_to_nearest_even():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 3, 20000), [0.0, 1.0, 1.00390625, 2.0 ** -15, 6e-8]])
    for dt in ("bf16", "fp16"):
        a32 = a.astype(np.float32)
        assert np.array_equal(B.round16(a32.astype(np.float64), dt), B.cast32(a32, dt)), dt  # from fp32 values torch rounds once
        got = B.round16(a, dt)
        assert (np.abs(got - a) <= 0.5 * B.ulp16(a, dt)).all() and np.array_equal(B.quantise(got, dt), got)


@pytest.fixture(scope="module")
def measured():
    """One pass over every GPU case: guard band, exactness, the restatements' error per row type and their 16-bit shares."""
    out = dict(guard={}, worst={dt: dict(y=0.0, eval=0.0, dx=0.0) for dt in B.RESTATE_MAX}, share={}, ulp={})
    for name, c in CASES.items():
        d = G.case_inputs(c)
        N, Ns, dt = c["N"], c["Ns"], c["dtype"]
        eps, leak = G.F32(c["eps"]), G.F32(c["leak"])
        r = G.case_reference(c, d)
        out["guard"][name] = B.guard_ok(d, N, Ns, eps, leak, r) + (d.get("exact"),)
        y32 = B.fwd_fp32(d["x"], N, Ns, r["save_mean"], r["save_invstd"], d["weight"], d["bias"], leak)
        e32 = B.eval_fp32(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], eps, leak)
        dx32 = B.bwd_fp32(d["x"], d["dy"], N, Ns, r["save_mean"], r["save_invstd"], d["weight"], d["bias"], leak, r["S1"], r["S2"])
        ye = B.bn_eval_ref(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], eps, leak)
        w = out["worst"][dt]
        w["y"] = max(w["y"], B.worst(y32 - r["y"], B.scale_y(d["x"], r, N, Ns, d["weight"], d["bias"])))
        w["eval"] = max(w["eval"], B.worst(e32 - ye, B.scale_eval(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], eps)))
        w["dx"] = max(w["dx"], B.worst(dx32 - r["dx"], B.scale_dx(d["x"], r, N, Ns, d["weight"])))
        if dt != "fp32":
            for key, v32, v64 in (("y", y32, r["y"]), ("eval", e32, ye), ("dx", dx32, r["dx"])):
                got = B.cast32(v32, dt)
                out["share"][name, key] = float((got != B.round16(v64, dt)).mean())
                out["ulp"][name, key] = float((np.abs(got - v64) / B.ulp16(v64, dt)).max())
    return out


def test_every_gpu_case_keeps_the_guard_band_or_is_exact(measured):
    """No |y_ref| below 1e-4 in any case (for the 16-bit types on the quantised x), except the exact zeros of the grid cases, whose sums
    are exact in fp32 (asserted by the maker)."""
    for name, (inside, smallest, exact) in measured["guard"].items():
        assert inside == 0 and smallest >= B.GUARD, (name, inside, smallest)
        assert (exact is not None) == (CASES[name]["kind"] == "grid"), name
    zeros = [n for n, c in CASES.items() if c["kind"] == "grid" and c["leak"] != 0.0]
    assert zeros and all((G.case_inputs(CASES[n])["x"] == 0).any() for n in zeros)


def test_restatement_maxima_are_the_recorded_constants(measured):
    """The measurement behind RESTATE_MAX of tests/_bn_ref.py: the kernels' per-element arithmetic in numpy float32 against float64, in
    units of each output's scale, largest over all GPU cases of a row type.  The recorded constant is that figure rounded up."""
    print("fp32 restatement against float64:", {dt: {k: f"{v:.3e}" for k, v in w.items()} for dt, w in measured["worst"].items()})
    print("16-bit: largest share of elements the restatement does not round correctly:",
          {dt: {key: f"{max(v for (n, k), v in measured['share'].items() if n.endswith(dt) and k == key):.2e}" for key in ("y", "eval", "dx")}
           for dt in ("bf16", "fp16")})
    print("16-bit: largest error of the cast restatement in ulp of the format:",
          {dt: {key: f"{max(v for (n, k), v in measured['ulp'].items() if n.endswith(dt) and k == key):.3f}" for key in ("y", "eval", "dx")}
           for dt in ("bf16", "fp16")})
    for dt, w in measured["worst"].items():
        for key, v in w.items():
            assert np.isfinite(v) and v > 0, (dt, key, v)
            assert v <= B.RESTATE_MAX[dt][key] <= 1.25 * v, (dt, key, v, B.RESTATE_MAX[dt][key])


def test_the_case_table_covers_what_it_claims():
    for cus in (G.MI355X_CUS, 304, 64):  # the edge cases sit on their edges on other chips too
        t = G.cases(cus)
        assert list(t) == G.CASE_NAMES
        for lo, C in ((8, 16), (13, 112), (20, 512), (36, 16)):
            a, b = t[f"fused_edge_R{lo}_c{C}"], t[f"fused_edge_R{lo + 1}_c{C}"]
            assert G.fused_shape(cus, a["N"], 0, C)[0] == lo and G.fused_shape(cus, b["N"], 0, C)[0] == lo + 1 and b["N"] == a["N"] + 1
        for R in (8, 9):
            c = t[f"fused_edge_R{R}_two_groups"]
            got, R0, R1 = G.fused_shape(cus, c["N"], c["Ns"], 16)
            assert got == R1 == R and R0 < R
    t = CASES
    assert max(c["N"] * max(c["ld_x"], c["ld_dx"], c["ld_dy"]) * 4 for c in t.values()) < 90e6  # bytes of the largest tensor
    assert [G.fused_shape(256, t[f"fused_G{g}"]["N"], 0, 16)[0] for g in (7, 8, 9)] == [6, 6, 6]
    assert G.stat_rows_per_thread(t["k3_max_part"]) == [40] and G.stat_rows_per_thread(t["k3_max_part_two_groups"]) == [40, 40]
    assert [G.stat_rows_per_thread(t[f"k3_rows_per_slot_{j}"]) for j in range(1, 6)] == [[j] for j in range(1, 6)]
    assert G.vec_width(t["k3_c16_unaligned"]) == 1 and G.vec_width(t["k3_c256_odd_pitch"]) == 1 and G.vec_width(t["k3_c516"]) == 4
    assert G.vec_width(t["k3_c1024"]) == 4 and G.vec_width(t["fused_pitched"]) == 4
    for p in ("fused", "k3"):
        assert {t[f"{p}_leak{l}_mom{m}"]["Ns"] > 0 for l in (0.0, 0.333) for m in (0.9, 0.99)} == {True, False}
    for dt in ("bf16", "fp16"):
        assert sum(c["dtype"] == dt for c in t.values()) == len(G.REDUCED) and all(t[f"{n}_{dt}"]["opt"] == 0 for n in G.REDUCED)
    assert all(c["R"] == 0 for c in t.values() if c["opt"] == 0) and all(c["R"] != 0 or "R37" in n for n, c in t.items() if c["opt"] == 3)


def test_prototypes_and_workspace_of_the_bn_entries():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    want = {"mm_bn_ws_bytes": 1, "mm_bn_fused_rows": 5}
    for sfx in ("", "_bf16", "_f16"):
        want.update({"mm_bn_fwd_train" + sfx: 20, "mm_bn_fwd_eval" + sfx: 13, "mm_bn_bwd" + sfx: 21})
    for name, n_args in want.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        res, args = _lib._PROTOS[name]
        assert len(m.group(1).split(",")) == len(args) == n_args, name
        assert hasattr(L, name)
    for C in (1, 7, 16, 255, 1024):  # the fp64 partials of 1,024 blocks, then the per-group sums
        assert int(L.mm_bn_ws_bytes(C)) >= -(-1024 * 2 * C * 8 // 256) * 256 + 4 * C * 4
    assert int(L.mm_bn_fused_rows(None, 100, 0, 16, 0)) == -1  # what is no handle is refused before anything is read
