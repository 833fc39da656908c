"""Host checks behind tests/test_gpu_loss_rows.py and tests/test_gpu_lift_index.py: the float64 references of tests/_loss_ref.py
against torch float64 autograd and against oracle.net2d_ref.lift, the conditions the input makers promise for every case of the GPU
files' tables, the measurement from which the loss bounds come, and the C ABI of the loss and lifting entries (include/mm2d3d.h
against mm2d3d_amd/_lib.py).  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _loss_ref as R
import test_gpu_lift_index as GL
import test_gpu_loss_rows as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, what, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.abs(got - want).max(initial=0.0) <= tol * max(np.abs(want).max(initial=0.0), 1e-300), what


# --------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("C,N,weight,ignore", [(6, 300, "grid", -100), (6, 300, None, 0), (2, 77, "zero", -100), (32, 50, "usa_sing", -100),
                                               (1, 9, None, -100)])
def test_cross_entropy_reference_matches_torch_float64_autograd(C, N, weight, ignore):
    if weight == "usa_sing":
        C = 6
    d = R.make_ce(N, C, 5, weight, "mix", ignore)
    ref = R.ce(d["x"], d["labels"], d["weight"], ignore, -2.5)
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    lab = torch.from_numpy(d["labels"]).clone()
    lab[(lab < 0) | (lab >= C) | (lab == ignore)] = -100  # torch refuses labels outside [0, C); the kernels skip them
    w = None if d["weight"] is None else torch.tensor(d["weight"], dtype=torch.float64)
    loss = F.cross_entropy(x, lab, weight=w, ignore_index=-100)
    (-2.5 * loss).backward()
    _close(ref["loss"], loss.item(), "loss")
    _close(ref["dlogits"], x.grad.numpy(), "dlogits")
    live = (lab != -100).numpy()
    assert np.array_equal(ref["live"], live) and (N < 20 or 0 < live.sum() < N)
    assert ref["sum_w"] == (np.ones(C) if w is None else w.numpy())[d["labels"][live]].sum()
    assert ref["abs_mean"] == pytest.approx(ref["loss"], rel=1e-14)  # every nll is >= 0


def test_cross_entropy_reference_without_counted_rows_and_without_rows():
    for n in (0, 5):
        d = R.make_ce(n, 6, 1, "grid", "all_ignored")
        ref = R.ce(d["x"], d["labels"], d["weight"], -100)
        assert math.isnan(ref["loss"]) and ref["sum_w"] == 0 and not ref["dlogits"].any() and not ref["live"].any()
        got = R.ce_fp32(d["x"], d["labels"], d["weight"], -100)
        assert np.isnan(got["loss"]) and got["sum_w"] == 0 and not got["dlogits"].any()
        assert R.ce_errors(ref, got["loss"], got["dlogits"], 1.0) == dict(ce_loss=0.0, ce_grad=0.0)
    with pytest.raises(AssertionError, match="not exactly zero"):
        R.ce_errors(ref, got["loss"], got["dlogits"] + 1e-30, 1.0)


@pytest.mark.parametrize("C,N,kind", [(6, 300, "plain"), (2, 77, "plain"), (32, 50, "wide"), (6, 40, "same"), (1, 9, "plain")])
def test_kl_reference_matches_torch_float64_autograd(C, N, kind):
    d = R.make_kl(N, C, 6, kind)
    ref = R.kl(d["pred"], d["tgt"], -2.5)
    p = torch.tensor(d["pred"], dtype=torch.float64, requires_grad=True)
    t = torch.tensor(d["tgt"], dtype=torch.float64)
    loss = F.kl_div(F.log_softmax(p, 1), F.softmax(t, 1), reduction="none").sum(1).mean()
    (-2.5 * loss).backward()
    if kind == "same":  # the reference subtracts equal numbers; torch's xlogy form leaves a rounding residue
        assert ref["loss"] == 0 and abs(loss.item()) <= 1e-15
        assert not ref["dpred"].any() and np.abs(p.grad.numpy()).max() <= 1e-15
    else:
        _close(ref["loss"], loss.item(), "loss", 1e-11)
        _close(ref["dpred"], p.grad.numpy(), "dpred", 1e-11)
    assert math.isnan(R.kl(np.zeros((0, C)), np.zeros((0, C)))["loss"])


def test_lift_references_agree_with_the_oracle_on_the_small_case():
    """The case of test_gpu_step.py test_lifting_gather_and_duplicate_accumulating_backward."""
    from oracle.net2d_ref import lift as ref_lift

    g = np.random.default_rng(0)
    B, C, H, W = 3, 6, 17, 23
    idx = [np.stack([g.integers(0, H, n), g.integers(0, W, n)], 1) for n in (400, 1, 700)]
    seg = torch.randn(B, C, H, W, dtype=torch.float64, requires_grad=True)
    out = ref_lift(seg, idx)
    key, err = R.lift_keys(np.concatenate(idx), [400, 1, 700], H, W)
    assert err == 0
    b, r, c = R.key_pixels(key, H, W)
    assert np.array_equal(b, np.repeat([0, 1, 2], [400, 1, 700])) and np.array_equal(np.stack([r, c], 1), np.concatenate(idx))
    assert np.array_equal(R.lift_gather(seg.detach().numpy(), key), out.detach().numpy())
    nhwc = np.ascontiguousarray(seg.detach().numpy().transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)  # any strides
    assert np.array_equal(R.lift_gather(nhwc, key), out.detach().numpy())
    dout = R.make_scatter_grid(len(key), C, key, 3)
    out.backward(torch.from_numpy(dout))
    sums, touched = R.lift_scatter(dout, key, (B, C, H, W))
    assert np.array_equal(sums, seg.grad.numpy()) and not sums[~np.broadcast_to(touched[:, None], sums.shape)].any()
    skey, order = R.lift_sorted(key)
    assert np.array_equal(key[order], skey) and (np.diff(skey) >= 0).all() and (np.diff(order)[np.diff(skey) == 0] > 0).all()
    # clamping and the error flag
    k2, e2 = R.lift_keys([[-1, 3], [H, W], [2 ** 40, -5]], [1, 0, 2], H, W)
    assert e2 == 1 and k2.tolist() == [3, (2 * H + H - 1) * W + W - 1, (2 * H + H - 1) * W]


# ----------------------------------------------------------------------------------------------------------------- makers
def test_every_loss_case_satisfies_what_its_maker_promises():
    shipped = R.shipped_class_weights()
    assert sorted(shipped) == ["day_night", "usa_sing", "vkitti_skitti"] and all(len(v) == 6 and min(v) == 1.0 for v in shipped.values())
    for name, c in G.CE_CASES.items():
        d = G.ce_inputs(name)  # the maker asserts that the weight sum on the 1/8 grid is a float32 number
        assert d["x"].shape == (c["n"], c["c"]) and d["x"].dtype == np.float32 and d["labels"].dtype == np.int64
        assert d["on_grid"] == (c["weight"] in (None, "grid", "zero"))
        live = R.counted(d["labels"], c["c"], c["ignore"])
        if c["labels"] == "all_ignored":
            assert not live.any()
        elif c["n"] >= 255:
            lab = set(d["labels"].tolist())
            assert {-100, -1, -7, c["c"], c["c"] + 5} <= lab and live.any() and not live.all(), name
            assert c["ignore"] == -100 or (d["labels"] == c["ignore"]).any()
        if c["weight"] == "zero":
            assert (d["weight"] == 0).sum() == 1 and (d["labels"][live] == int(np.argmin(d["weight"]))).any()
        assert d["x"].nbytes <= 9 << 20, name
    for name, c in G.KL_CASES.items():
        d = G.kl_inputs(name)  # the maker asserts the spread of 120 and the underflow of the wide cases
        assert d["pred"].shape == d["tgt"].shape == (c["n"], c["c"])
        assert c["n"] == 0 or (c["kind"] == "same") == np.array_equal(d["pred"], d["tgt"]), name
        assert len({c["ld_p"], c["ld_t"], c["ld_d"]}) == 3 or c["ld_p"] == c["ld_t"] == c["ld_d"] == c["c"]


def test_every_confusion_row_is_decided_and_no_row_is_left_out():
    for name, c in G.CM_CASES.items():
        d = G.cm_inputs(name)  # the maker asserts that every row passes the margin or is an exact tie
        n, C = c["n"], c["c"]
        assert d["pred"].shape == (3, n) and d["a"].shape == d["b"].shape == (n, C)
        assert d["redrawn"] <= max(8, 0.004 * n), (name, d["redrawn"])  # rows without a planted tie: a fraction of a percent
        if n >= 2047 and C >= 2:
            kinds = set(d["ties"].values())
            assert kinds == ({"same_pos", "a_is_b", "swap"} if C == 2 else {"same_pos", "diff_pos", "a_is_b"}), name
            e = R.ensemble64(d["a"], d["b"])
            for r, k in d["ties"].items():
                if k != "diff_pos":  # exactly tied in float64, and the FIRST of the tied classes is expected
                    top = np.flatnonzero(e[r] == e[r].max())
                    assert len(top) == 2 and d["pred"][2, r] == top[0], (name, r, k)
            lab = set(d["labels"].tolist())
            assert {-100, -1, C, C + 5} <= lab
        if n and n <= 4096:
            # float32 arithmetic as in pointpred.h gives the expected class in every row (strict >: the first maximum wins)
            def sm32(v):
                ex = R.exp32(v - v.max(1, keepdims=True))
                s = np.zeros(n, np.float32)
                for k in range(C):
                    s = s + ex[:, k]
                return ex / s[:, None]

            e32 = np.float32(0.5) * (sm32(d["a"]) + sm32(d["b"]))
            assert np.array_equal(e32.argmax(1), d["pred"][2]), name
            assert np.abs(e32 - R.ensemble64(d["a"], d["b"])).max() <= 2.5e-7
        cm = R.confusion(d["pred"], d["labels"], C, c["ignore"])
        assert cm.sum() == 3 * R.counted(d["labels"], C, c["ignore"]).sum()
    assert G.CM_CASES["ignore_is_class_1"]["ignore"] == 1 and (G.cm_inputs("ignore_is_class_1")["labels"] == 1).any()


def test_every_lift_case_is_what_it_claims():
    bits = {}
    for name, c in GL.INDEX_CASES.items():
        d = GL.index_inputs(name)  # asserts the key range and, for the "last" cases, a point on the map's last pixel
        bits[name] = GL.key_bits(c)
        assert len(d["key"]) == sum(c["counts"]) and np.array_equal(d["key"][d["order"]], d["skey"])
    assert bits["map_of_one_pixel"] == 1 and bits["map_2pow11"] == 11 and bits["map_2pow10_plus_1"] == 11
    assert bits["map_2pow15_n20000"] == 15 and bits["map_2pow15_plus_1_n20000"] == 16 and bits["keys_31_bits_sparse"] == 31
    assert GL.index_inputs("keys_31_bits_n20k")["key"].max() == 2 ** 31 - 2 ** 20 - 1 and len(GL.index_inputs("keys_31_bits_n20k")["key"]) > GL.MERGE_LIMIT
    assert set(GL.INDEX_CASES["keys_31_bits_sparse"]["counts"]) == {0, 1}
    assert len(np.unique(GL.index_inputs("dup7_n4097")["key"])) <= 7 and len(np.unique(GL.index_inputs("one_pixel_n5000")["key"])) == 1
    ns = {sum(c["counts"]) for c in GL.INDEX_CASES.values()}
    assert ns >= {0, 1, 2, 255, 256, 257, 2049, 4097, 16383, 16384, 16385, 150001, 5000}
    cl = GL.index_inputs("clamped")
    assert cl["err"] == 1 and sum(GL.index_inputs(n)["err"] for n in GL.INDEX_CASES) == 1
    for big in (False, True):
        p = GL.map_points(big)
        assert np.array_equal(p["key"][p["order"]], p["skey"]) and p["key"].max() < GL.MAP_B * GL.MAP_H * GL.MAP_W
    assert {C for C, _ in GL.MAP_CASES} == {1, 3, 6, 17, 32} and (6, "slice") in GL.MAP_CASES
    with pytest.raises(AssertionError, match="2\\^24"):
        R.make_scatter_grid(3 << 20, 1, np.zeros(3 << 20, np.int64), 0)


def _loss_blocks(n):
    """loss_blocks of csrc/loss.hip: blocks of 1024 rows, at most MAX_PART = 1024 of them."""
    return min(max(-(-n // 1024), 1), 1024)


def test_the_case_tables_cover_what_they_claim():
    for cases in (G.CE_CASES, G.KL_CASES):
        assert {(c["n"], c["c"]) for c in cases.values()} >= {(n, k) for n in (0, 1, 255, 256, 257, 1024, 1025) for k in (1, 2, 6, 20, 32)}
        big = {c["n"] for c in cases.values() if c["n"] > 65536}
        assert big == {65537, 1048576 + 1025} and all(c["c"] == 2 for c in cases.values() if c["n"] > 65536)
        assert _loss_blocks(1024) == 1 and _loss_blocks(1025) == 2 and _loss_blocks(65537) == 65 and _loss_blocks(1048576 + 1025) == 1024
        assert -(-(1048576 + 1025) // 1024) > 1024
        assert {c["g"] for c in cases.values()} == {1.0, 0.0, -2.5, 65536.0}
        assert any(c["twice"] and c["n"] == 65537 for c in cases.values()) and any(c["twice"] and c["n"] > 1 << 20 for c in cases.values())
    ce = G.CE_CASES.values()
    assert {c["weight"] for c in ce} == {None, "grid", "zero", "w6", "usa_sing", "day_night", "vkitti_skitti"}
    assert {k for k in (1, 2, 6, 20, 32) if any(c["c"] == k and c["ld"] == k + 3 and c["ld_d"] == k + 5 for c in ce)} == {1, 2, 6, 20, 32}
    assert any(c["ignore"] == 0 for c in ce) and any(c["labels"] == "all_ignored" for c in ce)
    kl = G.KL_CASES.values()
    assert {c["kind"] for c in kl} == {"plain", "same", "wide"}
    assert all(len({c["ld_p"], c["ld_t"], c["ld_d"], c["c"]}) == 4 for n, c in G.KL_CASES.items() if n.startswith("pitched"))
    cm = G.CM_CASES.values()
    assert {(c["n"], c["c"]) for c in cm} >= {(n, k) for n in (0, 1, 2047, 2048, 2049) for k in (1, 2, 6, 32)}
    assert [c["c"] for c in cm if c["n"] > 4096] == [2] and -(-G.N_GRID_CAPPED // 2048) > 1024
    assert any(len({c["ld2"], c["ld3"], c["c"]}) == 3 for c in cm) and any(0 <= c["ignore"] < c["c"] for c in cm)
    assert len(G.CE_CASES) + len(G.KL_CASES) + len(G.CM_CASES) <= 160


# ------------------------------------------------------------------------------------------------------------ measurement
def _round_up(v):
    """Up to two significant digits."""
    if v == 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def measured_fp32_errors():
    """Largest error of the float32 restatements against the float64 references, per quantity, over all loss cases."""
    worst = {}
    for name, c in G.CE_CASES.items():
        d = G.ce_inputs(name)
        ref = R.ce(d["x"], d["labels"], d["weight"], c["ignore"], c["g"])
        got = R.ce_fp32(d["x"], d["labels"], d["weight"], c["ignore"], c["g"])
        if d["on_grid"]:
            assert float(got["sum_w"]) == ref["sum_w"]
        for k, v in R.ce_errors(ref, got["loss"], got["dlogits"], c["g"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    for name, c in G.KL_CASES.items():
        d = G.kl_inputs(name)
        got = R.kl_fp32(d["pred"], d["tgt"], c["g"])
        assert c["n"] == 0 or (np.isfinite(got["loss"]) and np.isfinite(got["dpred"]).all())
        for k, v in R.kl_errors(R.kl(d["pred"], d["tgt"], c["g"]), got["loss"], got["dpred"], c["g"], c["n"], c["kind"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def test_loss_bounds_are_eight_times_the_measured_fp32_error():
    """The measurement the bounds of test_gpu_loss_rows.py come from.  A bound must be at least what is measured here and at most
    8 x that, rounded up to two digits.  exp and log of the restatement are correctly rounded, so the figures are the same on
    every machine."""
    worst = measured_fp32_errors()
    print("fp32 restatement against float64:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(G.LOSS_BOUNDS)
    for k, v in worst.items():
        assert v <= G.LOSS_BOUNDS[k] <= _round_up(8 * v) * (1 + 1e-12), (k, v, G.LOSS_BOUNDS[k])
    assert worst["kl_same_loss"] == 0.0 == G.LOSS_BOUNDS["kl_same_loss"]
    assert _round_up(1.344e-6) == pytest.approx(1.4e-6) and _round_up(2.0e-7) == pytest.approx(2.0e-7) and _round_up(0) == 0


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_prototypes_of_the_loss_and_lift_entries_and_the_retired_ones_are_gone():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    assert int(L.mm_loss_ws_bytes()) >= 1024 * 2 * 8
    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    want = {"mm_loss_ws_bytes": 0, "mm_ce_fwd": 11, "mm_ce_bwd": 12, "mm_kl_fwd": 10, "mm_kl_bwd": 10, "mm_eval_confusion": 10,
            "mm_lift_index_ws_bytes": 1, "mm_lift_index": 14, "mm_lift_gather_key": 12, "mm_lift_scatter_key": 13}
    for name, n_args in want.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        res, args = _lib._PROTOS[name]
        declared = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(declared) == len(args) == n_args, name
        assert res is (_lib.sz if name.endswith("_ws_bytes") else _lib.i32), name
        assert hasattr(L, name)
    # the three entries lift.hip replaced have no caller and are gone: from the header, the binding, the sources and the library
    sources = [os.path.join(ROOT, "include", "mm2d3d.h")]
    for base, _, files in os.walk(os.path.join(ROOT, "mm2d3d_amd")):
        sources += [os.path.join(base, f) for f in files if f.endswith((".py", ".hip", ".h"))]
    for retired in ("mm_lift_gather", "mm_lift_scatter", "mm_lift_scatter_runs", "k_lift_gather", "k_lift_scatter", "k_lift_scatter_runs"):
        assert retired not in _lib._PROTOS and not hasattr(L, retired), retired
        for path in sources:
            assert not re.search(r"\b" + retired + r"\b", open(path).read()), (retired, path)
