"""Host checks behind tests/test_gpu_lovasz.py: the references of tests/_lovasz_ref.py against each other and against torch float64
autograd, what the case table promises, the measurement the bounds come from, the C ABI of the mm_lovasz_* entries
(include/mm2d3d.h against mm2d3d_amd/_lib.py), their refusals, and the registry entry of mm2d3d_amd/losses.py.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _loss_ref as L
import _lovasz_ref as R
import test_gpu_lovasz as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = [n for n, c in G.CASES.items() if c["n"] <= 4096]  # the references' own properties: every case but the largest


# --------------------------------------------------------------------------------------------------------------- references
def test_closed_form_equals_the_definition():
    worst = 0.0
    for name in G.CASES:
        c, d = G.CASES[name], G.inputs(name)
        err, live = R.errors(d["x"], d["labels"])
        a = R.loss_by_definition(err, d["labels"], c["classes"])
        b = R.rank_stage(err, d["labels"], c["classes"])
        n = max(a["n_included"], 1)
        worst = max(worst, abs(a["loss"] - b["loss"]), np.abs(a["coef"] / n - b["coef"]).max(initial=0.0))
        assert a["n_included"] == b["n_included"] and a["counted"] == b["counted"] == live.sum()
        # the increments of an included class are >= 0 and sum to the Jaccard loss of the whole order: 1 with foreground rows
        for k in range(c["c"]):
            s = np.abs(b["coef"][k]).sum() * n
            assert (s == 0 and not a["per_class"][k]) or abs(s - 1) <= 1e-12, (name, k, s)
    print(f"closed form against the definition: {worst:.3e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("name", ["n3079_c6", "n1025_c2", "absent_all", "n1023_c11"])
def test_loss_is_unchanged_by_the_order_inside_tied_groups(name):
    c, d = G.CASES[name], G.inputs(name)
    err = R.err_fp32(d["x"], d["labels"])
    live = L.counted(d["labels"], c["c"], -100)
    assert max(len(np.unique(e[live])) for e in err) < live.sum(), "no ties in this case"
    base = R.rank_stage(err, d["labels"], c["classes"])
    # a random permutation of the rows permutes every tied group: the stable order by row index is then another order of the ties
    perm = np.random.default_rng(3).permutation(c["n"])
    moved = R.rank_stage(err[:, perm], d["labels"][perm], c["classes"])
    assert abs(moved["loss"] - base["loss"]) <= 1e-14
    back = np.empty_like(perm)
    back[perm] = np.arange(c["n"])
    assert not np.array_equal(moved["coef"][:, back], base["coef"]), "the weights of single rows do depend on the order"


def _composite(x, labels, classes):
    """(loss, softmax) of the loss composed from torch ops: softmax, sort, cumsum, difference (the paper's lovasz_softmax_flat)."""
    C = x.shape[1]
    live = (labels >= 0) & (labels < C)
    full = torch.softmax(x, 1)
    p, y = full[live], labels[live]
    if p.shape[0] == 0:
        return x.sum() * 0.0, full
    losses = []
    for c in range(C):
        fg = (y == c).to(x.dtype)
        if classes == "present" and fg.sum() == 0:
            continue
        e = (fg - p[:, c]).abs()
        es, order = torch.sort(e, dim=0, descending=True, stable=True)
        fs = fg[order]
        inter = fs.sum() - fs.cumsum(0)
        union = fs.sum() + (1 - fs).cumsum(0)
        jac = 1 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    return torch.stack(losses).mean(), full


@pytest.mark.parametrize("name", HOST_CASES)
def test_float64_backward_equals_torch_autograd_of_the_composite(name):
    c, d = G.CASES[name], G.inputs(name)
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    lab = torch.from_numpy(d["labels"].copy())
    lab[lab == -100] = -1
    loss, p = _composite(x, lab, c["classes"])
    (-2.5 * loss).backward()
    # a row's weight depends on the order of near-tied errors: the reference ranks the errors of torch's OWN softmax values
    err = np.abs((d["labels"][None, :] == np.arange(c["c"])[:, None]) - p.detach().numpy().T)
    ref = R.rank_stage(err, d["labels"], c["classes"])
    assert abs(ref["loss"] - loss.item()) <= 1e-12
    assert np.abs(R.backward(d["x"], ref["coef"], -2.5) - x.grad.numpy()).max(initial=0.0) <= 1e-12


# -------------------------------------------------------------------------------------------------------------------- cases
def test_the_case_table_covers_what_it_claims():
    src = open(os.path.join(ROOT, "mm2d3d_amd", "csrc", "lovasz.hip")).read()
    for name, v in (("T", R.T), ("ITEMS", R.ITEMS), ("BITS", R.BITS), ("PASSES", R.PASSES), ("SCAN_PER", R.SCAN_PER)):
        assert re.search(rf"constexpr int {name} = {v};", src), name
    assert "TILE = T * ITEMS" in src and "SCAN_BLK = T * SCAN_PER" in src and "RADIX = 1 << BITS" in src
    assert (R.TILE, R.SCAN_BLK, R.RADIX) == (1024, 2048, 1024) and R.BITS * R.PASSES == 30
    shapes = {(c["n"], c["c"]) for c in G.CASES.values()}
    assert shapes >= {(n, k) for n in (0, 1, 2, R.TILE - 1, R.TILE, R.TILE + 1, 3 * R.TILE + 7) for k in (1, 2, 6, 11, 32)}
    assert R.scan_blocks(R.TILE) == 1 and R.scan_blocks(G.N_TWO_SCAN_GROUPS) == 2  # more than one workgroup in the offset scan
    assert R.scan_blocks(G.N_EVERY_LEVEL - 1) == R.T and R.scan_blocks(G.N_EVERY_LEVEL) == R.T + 1  # the sums' scan carries
    assert [c["c"] for c in G.CASES.values() if c["n"] > 4096] == [2] and max(c["n"] for c in G.CASES.values()) == G.N_EVERY_LEVEL
    assert {c["classes"] for c in G.CASES.values()} == {"present", "all"} and any(c["ld"] > c["c"] for c in G.CASES.values())
    assert {c["labels"] for c in G.CASES.values()} == {"mix", "all_ignored", "absent", "one_class"}
    assert {b["g"] for b in G.BWD_CASES.values()} == {1.0, -0.5, 65536.0} and {b["src"] for b in G.BWD_CASES.values()} == {"grid", "stage_b"}
    assert any(len({b["ld"], b["ld_d"], G.CASES[b["case"]]["c"]}) == 3 for b in G.BWD_CASES.values())
    assert all(b["case"] in G.CASES for b in G.BWD_CASES.values())
    assert len(G.CASES) <= 50 and len(G.BWD_CASES) <= 24
    for n, c in ((279040, 6), (0, 1), (1, 32), (1 << 24, 2)):
        assert R.ws_bytes(n, c) > 16 * c * n


def test_every_case_holds_what_its_maker_promises():
    for name, c in G.CASES.items():
        d = G.inputs(name)
        x, lab = d["x"], d["labels"]
        assert x.shape == (c["n"], c["c"]) and x.dtype == np.float32 and lab.dtype == np.int64
        live = L.counted(lab, c["c"], -100)
        present = set(lab[live].tolist())
        if c["labels"] == "all_ignored":
            assert not live.any()
        elif c["labels"] == "absent":
            assert present == set(range(c["c"])) - {1}
        elif c["labels"] == "one_class":
            assert present == {c["c"] - 1}
        elif c["n"] >= R.TILE - 1:
            assert {-100, -1, c["c"], c["c"] + 5} <= set(lab.tolist()) and live.any() and not live.all(), name
        if c["n"] >= 16 and c["c"] >= 2:
            err = R.err_fp32(x, lab)
            assert (x[6] == x[6, 0]).all()
            assert np.array_equal(x[4::5], x[1::5][: len(x[4::5])]) and np.array_equal(lab[4::5], lab[1::5][: len(lab[4::5])])
            if live.any():
                e = err[:, live]
                assert (e == 0).sum() >= 8 and (e == 1).sum() >= 8, name  # whole runs of exact 0 and exact 1
                assert len(np.unique(e[0])) < e.shape[1]  # exact ties


# ------------------------------------------------------------------------------------------------------------ measurement
def _round_up(v):
    """Up to two significant digits."""
    if v == 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def measured_fp32_errors():
    """Largest error of the float32 restatements against float64, per quantity, over all cases of the GPU file.
    err: |err32 - err64|.  bwd: per entry, relative to |grad_out| * max |coef|.  loss: the err figure plus the summation term, the
    largest |float32 evaluation of the weights and the sum - float64 evaluation| on the SAME float32 errors; since the loss moves
    by at most max |delta e|, their sum bounds the distance of the kernels' loss from the float64 definition on float64 errors."""
    worst = {"err": 0.0, "bwd": 0.0}
    summation = 0.0
    for name, c in G.CASES.items():
        d = G.inputs(name)
        ref, live = R.errors(d["x"], d["labels"])
        err32 = R.err_fp32(d["x"], d["labels"])
        worst["err"] = max(worst["err"], np.abs(err32.astype(np.float64) - ref)[:, live].max(initial=0.0))
        a, b = R.rank_stage(err32, d["labels"], c["classes"], fp32=True), R.rank_stage(err32, d["labels"], c["classes"])
        summation = max(summation, abs(a["loss"] - b["loss"]))
        assert np.abs(a["coef"] - b["coef"]).max(initial=0.0) <= R.COEF_REL * np.abs(b["coef"]).max(initial=1.0)
        # the distance the summation term and the err figure bound together
        full = R.loss_by_definition(ref, d["labels"], c["classes"])
        assert abs(a["loss"] - full["loss"]) <= np.abs(err32 - ref)[:, live].max(initial=0.0) + abs(a["loss"] - b["loss"]) + 1e-15
    for name, b in G.BWD_CASES.items():
        c, d = G.CASES[b["case"]], G.inputs(b["case"])
        if b["src"] == "grid":
            coef = G.grid_coef(b["case"])
        else:
            coef = R.rank_stage(R.err_fp32(d["x"], d["labels"]), d["labels"], c["classes"], fp32=True)["coef"]
        unit = abs(b["g"]) * np.abs(coef).max(initial=0.0)
        diff = np.abs(R.bwd_fp32(d["x"], coef, b["g"]).astype(np.float64) - R.backward(d["x"], coef, b["g"])).max(initial=0.0)
        assert unit > 0 or diff == 0
        if unit > 0:
            worst["bwd"] = max(worst["bwd"], diff / unit)
    worst["loss"] = worst["err"] + summation
    return worst


def test_lovasz_bounds_are_eight_times_the_measured_fp32_error():
    """A bound must be at least what is measured here and at most 8 x that, rounded up to two digits; exp of the restatement is the
    correctly rounded float32 function, so the figures are the same on every machine."""
    worst = measured_fp32_errors()
    print("fp32 restatement against float64:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(G.LOVASZ_BOUNDS)
    for k, v in worst.items():
        assert v <= G.LOVASZ_BOUNDS[k] <= _round_up(8 * v) * (1 + 1e-12), (k, v, G.LOVASZ_BOUNDS[k])


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_the_binding_matches_the_three_symbols():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp,
             "int": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.sz, "float": _lib.f32}
    want = {"mm_lovasz_ws_bytes": 2, "mm_lovasz_fwd": 13, "mm_lovasz_bwd": 9}
    for name, n_args in want.items():
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [] if m.group(2).strip() == "void" else [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctype[m.group(1)] and len(args) == len(params) == n_args, name
        assert args == [ctype[p] for p in params], (name, params)


def test_workspace_size_follows_the_documented_formula():
    from mm2d3d_amd import _lib

    L_ = _lib.lib()
    for n, c in ((0, 1), (1, 1), (1024, 6), (1025, 6), (279040, 6), (279040, 11), (1 << 24, 32)):
        assert int(L_.mm_lovasz_ws_bytes(n, c)) == R.ws_bytes(n, c), (n, c)
    for n, c in ((10, 0), (10, 33), (-1, 6), ((1 << 24) + 1, 2), (10, -1)):
        assert int(L_.mm_lovasz_ws_bytes(n, c)) == 0, (n, c)


def test_argument_errors_come_before_any_launch():
    """Every refusal is decided on the host: these calls return without touching a device (there is none here)."""
    from mm2d3d_amd import _lib

    L_ = _lib.lib()
    buf = (ctypes.c_double * 64)()  # never read or written: every call below is refused
    p = ctypes.addressof(buf)
    big = 1 << 40

    def fwd(x=p, ld=6, N=10, C=6, lab=p, err=p, coef=p, stats=p, ws=p, ws_bytes=big):
        return L_.mm_lovasz_fwd(x, ld, N, C, lab, -100, 0, err, coef, stats, ws, ws_bytes, None)

    def bwd(x=p, ld=6, N=10, C=6, coef=p, g=p, d=p, ld_d=6):
        return L_.mm_lovasz_bwd(x, ld, N, C, coef, g, d, ld_d, None)

    bad = [(dict(C=0), b"bad C"), (dict(C=33, ld=33), b"bad C"), (dict(C=-1), b"bad C"), (dict(ld=5), b"bad C"), (dict(N=-1), b"N outside"),
           (dict(N=(1 << 24) + 1), b"N outside"), (dict(x=None), b"null"), (dict(coef=None), b"null")]
    for kw, word in bad:
        for fn in (fwd, bwd):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert b"lovasz:" in L_.mm_last_error() and word in L_.mm_last_error(), (kw, L_.mm_last_error())
    for kw, word in ((dict(lab=None), b"null"), (dict(err=None), b"null"), (dict(stats=None), b"null"), (dict(ws=None), b"null")):
        assert fwd(**kw) == -1 and b"lovasz:" in L_.mm_last_error() and word in L_.mm_last_error(), kw
    assert fwd(ws_bytes=16) != 0 and b"lovasz: workspace" in L_.mm_last_error()
    assert bwd(ld_d=5) == -1 and b"pitch" in L_.mm_last_error()
    assert bwd(d=None) == -1 and b"null" in L_.mm_last_error()
    assert bwd(g=None) == -1 and b"null" in L_.mm_last_error()
    assert L_.mm_lovasz_bwd(None, 6, 0, 6, None, None, None, 6, None) == 0  # no rows: nothing is launched


# ---------------------------------------------------------------------------------------------------------------- registry
def test_registry_builds_prints_splits_and_updates_the_new_loss(monkeypatch):
    from mm2d3d_amd import losses

    one = losses.Loss("lovasz_softmax")
    assert str(one) == "lovasz_softmax" and type(one._losses[0][2]) is losses.LovaszSoftmax and one._losses[0][1] == "segmentation"
    both = losses.Loss([{"name": "cross_entropy", "args": {"weight": [1.0, 2.0]}}, {"name": "lovasz_softmax", "weight": 0.5},
                        {"name": "l1"}])
    assert str(both) == "cross_entropy[weight=[1.0, 2.0]]+0.5lovasz_softmax+l1"
    split = both.split_by_target()
    assert set(split) == {"segmentation", "depth"} and [l.name for _, _, l in split["segmentation"]._losses] == ["cross_entropy", "lovasz_softmax"]
    seen = []
    monkeypatch.setattr(losses, "lovasz_softmax", lambda pred, gt, classes="present", ignore_index=-100: seen.append(classes) or 0.0)
    assert one("segmentation", pred="p", gt="g") == 0.0 and seen == ["present"]
    one.update_loss_params("lovasz_softmax", "segmentation", classes="all")
    one("segmentation", pred="p", gt="g")
    assert seen == ["present", "all"] and str(one) == "lovasz_softmax[classes=all]"
    with pytest.raises(KeyError):
        losses.Loss("lovasz_hinge")


def test_lovasz_softmax_refuses_bad_arguments_before_touching_a_device():
    from mm2d3d_amd.losses import lovasz_softmax

    x, y = torch.zeros(5, 6), torch.zeros(5, dtype=torch.int64)
    for kw in (dict(classes="some"), dict(classes=None), dict(classes=["all"]), dict(classes=True)):
        with pytest.raises(ValueError, match="lovasz_softmax"):
            lovasz_softmax(x, y, **kw)
    for pred, gt in ((torch.zeros(5, 33), y), (torch.zeros(5, 0), y), (torch.zeros(5), y), (x, y[:4]), (x, torch.zeros(5, 1, dtype=torch.int64)), (x, [0] * 5)):
        with pytest.raises(ValueError, match="lovasz_softmax"):
            lovasz_softmax(pred, gt)
    with pytest.raises(RuntimeError, match="GPU"):
        lovasz_softmax(x, y)  # no CPU fallback
