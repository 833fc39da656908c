"""Host checks behind tests/test_gpu_misc2d.py: the float64 references of tests/_misc2d_ref.py against torch float64 (max_pool2d with
its indices, autograd of avg_pool2d + conv2d), the conditions the input makers promise for every case of the GPU file's tables,
the measurement from which the head bounds come, and the C ABI of the glue entries (include/mm2d3d.h against mm2d3d_amd/_lib.py).
No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _misc2d_ref as R
import test_gpu_misc2d as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


# --------------------------------------------------------------------------------------------------------------- references
def test_round16_is_torch_rounding_to_nearest_even():
    assert R.round16([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], "bf16").tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    assert R.round16([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -26], "fp16").tolist() == [1.0, 1 + 2.0 ** -9, 2.0 ** -24, 0.0]
    v = np.random.default_rng(0).standard_normal(1000)
    for fmt in R.FMT:
        r = R.round16(np.sort(v), fmt)
        assert (np.diff(r) >= 0).all() and np.array_equal(R.round16(r, fmt), r)
    assert R.bits16([0.0, -0.0, -np.inf], "fp16").tolist() == [0, -32768, -1024]


def test_least_allowance_is_the_threshold_of_the_interval_test():
    g = np.random.default_rng(2)
    ref, a = g.standard_normal(4000), np.abs(g.standard_normal(4000)) + 1.0
    for fmt in R.FMT:
        got = R.round16(ref + 3e-3 * a * g.uniform(-1, 1, 4000), fmt)
        e = R.least_allowance(got, ref, a, fmt)
        assert 0 < e < 3e-3 and R.in_interval(got, ref, e * (1 + 1e-6) * a, fmt).all() and not R.in_interval(got, ref, e * 0.98 * a, fmt).all()
        assert R.least_allowance(R.round16(ref, fmt), ref, a, fmt) == 0 and R.least_allowance(np.zeros(3), np.zeros(3), np.zeros(3), fmt) == 0


@pytest.mark.parametrize("kind", R.MAP_KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 1, 7, 8), (2, 2, 2, 8), (1, 3, 3, 8), (3, 4, 5, 16), (2, 7, 8, 8), (2, 15, 18, 8)])
def test_maxpool_reference_matches_torch_float64_values_taps_and_gradient(shape, kind):
    B, H, W, C = shape
    x = R.make_map(kind, shape, 3, "fp16")
    y, idx = R.maxpool(x)
    xt = _nchw(x).requires_grad_(True)
    yt, flat = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    assert np.array_equal(R.bits16(y, "fp16"), R.bits16(_nhwc(yt), "fp16")), "values (signed zeros included)"
    flat = _nhwc(flat)
    oy, ox = np.arange(R.pooled(H))[None, :, None, None], np.arange(R.pooled(W))[None, None, :, None]
    taps = (flat // W - (2 * oy - 1)) * 3 + (flat % W - (2 * ox - 1))  # torch's flat index iy * W + ix as the tap kh * 3 + kw
    assert np.array_equal(idx, taps), "winning taps"
    if kind in ("relu", "equal", "signed_zero") and max(H, W) >= 3:
        assert (idx < 4).any()  # ties exist, and a tap ahead of the centre wins them
    g1, g2 = R.make_grid(y.shape, 4), R.make_grid(y.shape, 5)
    yt.backward(_nchw(g1 + g2))
    s, a, n = R.maxpool_bwd(g1, g2, idx, H, W)
    assert np.array_equal(s, _nhwc(xt.grad)) and n.sum() == 2 * idx.size and (a >= np.abs(s)).all()
    s1, a1, n1 = R.maxpool_bwd(g1, None, idx, H, W)
    assert n1.sum() == idx.size and np.array_equal(n1 > 0, n > 0) and not s[n == 0].any() and not np.signbit(s[n == 0]).any()


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (4, 4), (5, 5), (17, 17), (2, 5), (17, 4)])
@pytest.mark.parametrize("crop", [False, True])
def test_head_references_match_torch_float64_autograd(h, w, crop):
    B, C, NJ = 2, 8, 5
    Hp, Wp = (h + 2, w + 3) if crop else (h, w)
    d = R.make_heads(B, Hp, Wp, C, NJ, h, w, 9, "bf16")
    xin = np.nan_to_num(d["x"], nan=7.0)  # numbers outside the crop, which must not matter
    x = _nchw(xin).contiguous().requires_grad_(True)  # a plain NCHW float64 tensor
    Wt, bt = torch.from_numpy(d["Wj"]).reshape(NJ, C, 1, 1).requires_grad_(True), torch.from_numpy(d["bias"]).requires_grad_(True)
    out = F.conv2d(F.avg_pool2d(x[..., :h, :w], 5, 1, 2), Wt, bt)
    out.backward(_nchw(d["dout"]))
    ref, a = R.heads(d["x"], d["Wj"], d["bias"], h, w)
    rb = R.heads_bwd(d["x"], d["Wj"], d["dout"], h, w, Hp, Wp)
    for got, want, what in ((ref, _nhwc(out), "out"), (rb["dx"], _nhwc(x.grad), "dx"), (rb["dW"], Wt.grad.reshape(NJ, C).numpy(), "dW"),
                            (d["dout"].sum((0, 1, 2)), bt.grad.numpy(), "dbias")):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300), what
    assert not rb["dx"][:, h:].any() and not rb["dx"][:, :, w:].any() and not rb["dx_abs"][:, h:].any()
    assert (a >= np.abs(ref) * (1 - 1e-15)).all() and (rb["dx_abs"] >= np.abs(rb["dx"]) * (1 - 1e-15)).all() and (rb["dW_abs"] >= np.abs(rb["dW"]) * (1 - 1e-15)).all()
    nb, _ = R.heads(d["x"], d["Wj"], None, h, w)
    assert np.allclose(nb + d["bias"], ref, rtol=0, atol=1e-15)


def test_the_restatements_follow_the_kernels_dispatch():
    assert R.is_mfma(64, 16) and not R.is_mfma(64, 20) and not R.is_mfma(32, 5) and not R.is_mfma(128, 12)
    assert R.head_bwd_blocks(1) == (1, 1) and R.head_bwd_blocks(128) == (1, 128) and R.head_bwd_blocks(129) == (2, 65)
    assert R.head_bwd_blocks(520 * 512) == (2048, 130) and 520 * 512 > 2048 * 128 and 130 % 64
    for fmt in R.FMT:
        w = np.random.default_rng(1).uniform(-0.125, 0.125, (12, 64)).astype(np.float32)
        hi, lo = R.split16(w, fmt)
        assert np.array_equal(R.round16(hi, fmt), hi) and np.array_equal(R.round16(lo, fmt), lo)
        assert np.abs(hi.astype(np.float64) + lo - w).max() <= 2.0 ** -17 * 0.125  # "2^-17 relative" (csrc/misc2d.hip)
    hi, lo = R.split16(np.full((1, 64), 1e-3, np.float32), "fp16")
    assert 0 < abs(lo[0, 0]) < 2.0 ** -14, "the small-weights case does not reach the fp16 subnormals"
    # the sliding and the 25-tap box agree to rounding, and exactly on the grid
    z = R.make_grid((2, 17, 9, 4), 2).astype(np.float32)
    assert np.array_equal(R._box5(z), R._box5_rowmajor32(z)) and np.array_equal(R._box5(z.astype(np.float64)), R._box5(z))


# ------------------------------------------------------------------------------------------------------------------- makers
def test_every_pool_case_satisfies_what_its_maker_promises():
    assert {(c["B"], c["H"], c["W"]) for c in G.POOL_CASES.values()} == set(G.POOL_SHAPES) == {
        (1, 1, 1), (1, 1, 7), (2, 2, 2), (1, 3, 3), (3, 4, 5), (2, 7, 8), (2, 15, 18)}
    assert {(c["C"], c["ld"] - c["C"]) for c in G.POOL_CASES.values()} == {(C, p) for C in (8, 64, 72) for p in (0, 8)}
    threads = {G.pool_threads(c) for c in G.POOL_CASES.values()}
    assert any(t > 256 and t % 256 for t in threads) and any(t < 64 for t in threads) and any(t % 256 == 0 for t in threads)
    assert set(R.MAP_KINDS) == {"relu", "negative", "equal", "signed_zero", "neginf", "normal"}
    for name, c in G.POOL_CASES.items():
        for fmt in G.BUILDS:
            for kind in R.MAP_KINDS:
                d = G.pool_inputs(name, kind, fmt)  # the maker asserts its condition
                assert d["x"].shape == (c["B"], c["H"], c["W"], c["C"]) and d["idx"].dtype == np.uint8 and d["idx"].max() <= 8
                n = d["x"].size
                if kind == "relu" and n >= 64:
                    assert (d["x"] == 0).mean() >= 0.3 and (d["x"] > 0).any()
                if kind == "negative":
                    assert (d["x"] < 0).all() and (d["y"] < 0).all()
                if kind == "equal":
                    assert len(np.unique(d["x"])) == 1
                    oy, ox = np.indices(d["idx"].shape[1:3])
                    first = np.where(oy == 0, 3, 0) + np.where(ox == 0, 1, 0)  # the first tap inside the image
                    assert (d["idx"] == first[None, :, :, None]).all()
                if kind == "signed_zero" and n >= 64:
                    assert (d["x"] == 0).all() and np.signbit(d["x"]).any() and not np.signbit(d["x"]).all()
                    assert np.signbit(d["y"]).any() and not np.signbit(d["y"]).all()
                if kind == "neginf" and n >= 64:
                    assert np.isneginf(d["x"]).any() and (np.isneginf(d["y"]).any() or c["H"] * c["W"] > 100)
    with pytest.raises(AssertionError):
        R.make_map("no such kind", (1, 1, 1, 8), 0, "fp16")


def test_the_grid_is_exact_in_float32_sums_of_eight():
    g = R.make_grid((1000, 8), 1)
    assert set(np.unique(g * 8)) <= set(range(-32, 33)) and g.min() == -4 and g.max() == 4
    s = np.zeros(1000, np.float32)
    for k in range(8):
        s = s + g[:, k].astype(np.float32)
    assert np.array_equal(s, g.sum(1))


def test_the_copy_and_colsum_tables_cover_what_they_claim():
    assert [sum(p) // 8 for p in G.CAT_PARTS] == [1, 8, 32, 40, 4, 256] and 256 % 40 and {len(p) for p in G.CAT_PARTS} == {1, 2, 3, 4}
    for p in G.CAT_PARTS:
        r = G.cat_rows_per_block(p)
        assert G.cat_ns(p) == (0, 1, r - 1, r, r + 1, 3001) and r == (256 // (sum(p) // 8)) * 8
        for i in range(len(p)):
            v = G._cat_part(40, p, i)
            assert np.abs(v).max() <= 1019 and np.array_equal(R.round16(v, "fp16"), v)
    wide = np.concatenate([G._cat_part(50, (64, 192, 64), i) for i in range(3)], 1)
    # a chunk that lands in another place of its row, or in another of the rows near it, shows
    assert all(len(np.unique(r)) == r.size for r in wide) and all((wide[i] != wide[k]).all() for i in range(50) for k in range(i + 1, min(i + 6, 50)))
    assert G.COLSUM_C == (8, 64, 512, 2048)
    for C in G.COLSUM_C:
        r = (256 // (C // 8)) * 16
        assert G.colsum_ns(C) == (0, 1, r - 1, r, r + 1, 5 * r + 3)
    C, n = G.COLSUM_CAPPED
    assert (C, n) == (512, 2048 * 64 + 65) and -(-n // G.colsum_rows_per_block(C)) > 2048


def test_every_head_case_is_what_it_claims():
    f = G.HEAD_FWD_CASES.values()
    assert {(c["C"], c["NJ"]) for c in f} == {(64, nj) for nj in (1, 5, 8, 10, 12, 16, 20, 24, 32)} | {(C, nj) for C in (32, 128) for nj in (5, 12, 20)}
    for C, NJ in G.HEAD_CNJ:
        mine = [c for c in f if (c["C"], c["NJ"]) == (C, NJ) and c["scale"] == 1.0]
        assert {(c["h"], c["w"]) for c in mine} == {(1, 1), (2, 3), (4, 4), (5, 5), (16, 7), (17, 9), (33, 5)}
        assert {(c["Hp"] - c["h"], c["Wp"] - c["w"]) for c in mine} == {(0, 0), (2, 3)}
        assert {c["ld"] - C for c in mine} == {0, 8} and {c["bias"] for c in mine} == {True, False}
        px = {c["B"] * c["h"] * c["w"] for c in mine}
        assert min(px) < 16 and any(p > 16 and p % 16 for p in px)
    small = [c for c in f if c["scale"] != 1.0]
    assert len(small) == 1 and R.is_mfma(small[0]["C"], small[0]["NJ"]) and G.head_class(small[0], "out") == "out_mfma_small"
    b = G.HEAD_BWD_CASES
    assert {c["NJ"] for c in b.values()} == {1, 5, 8, 10, 12, 16, 20, 24, 32} and all(c["C"] == 64 for c in b.values())
    for NJ in G.HEAD_NJ:
        mine = [c for c in b.values() if c["NJ"] == NJ]
        assert {c["B"] * c["Hp"] * c["Wp"] for c in mine} >= {1, 127, 128, 129, 1000}
        assert {c["ld"] for c in mine} == {64, 72} and any(c["h"] < c["Hp"] or c["w"] < c["Wp"] for c in mine)
    cap = b["capped_nj20"]
    assert R.head_bwd_blocks(cap["B"] * cap["Hp"] * cap["Wp"]) == (2048, 130) and cap["h"] < cap["Hp"] and cap["w"] < cap["Wp"]
    for table, inputs in ((G.HEAD_FWD_CASES, G.head_fwd_inputs), (b, G.head_bwd_inputs)):
        for name, c in table.items():
            if name.startswith("capped"):
                continue
            for fmt in G.BUILDS:
                d = inputs(name, fmt)  # the maker asserts NaN outside the crop, numbers inside, the range of the weights
                assert d["x"].shape == (c["B"], c["Hp"], c["Wp"], c["C"]) and d["Wj"].shape == (c["NJ"], c["C"])
                assert (d["bias"] is not None) == c["bias"] and np.array_equal(R.round16(d["x"][:, :c["h"], :c["w"]], fmt), d["x"][:, :c["h"], :c["w"]])
    assert len(G.HEAD_FWD_CASES) + len(G.HEAD_BWD_CASES) <= 270


# -------------------------------------------------------------------------------------------------------------- measurement
def _round_up(v):
    """Up to two significant digits."""
    if v == 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def measured_fp32_errors():
    """Largest error of the float32 restatements against the float64 references, per quantity, over all head cases and both formats."""
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    for fmt in G.BUILDS:
        for name, c in G.HEAD_FWD_CASES.items():
            d = G.head_fwd_inputs(name, fmt)
            ref, a = R.heads(d["x"], d["Wj"], d["bias"], c["h"], c["w"])
            note(G.head_class(c, "out"), R.rel_error(R.heads_fp32(d["x"], d["Wj"], d["bias"], c["h"], c["w"], fmt), ref, a))
        for name, c in G.HEAD_BWD_CASES.items():
            d = G.head_bwd_inputs(name, fmt)
            ref = R.heads_bwd(d["x"], d["Wj"], d["dout"], c["h"], c["w"], c["Hp"], c["Wp"])
            got = R.heads_bwd_fp32(d["x"], d["Wj"], d["dout"], c["h"], c["w"], c["Hp"], c["Wp"])
            note(G.head_class(c, "dx"), R.rel_error(got["dx"], ref["dx"], ref["dx_abs"]))
            note(G.head_class(c, "dW"), R.rel_error(got["dW"], ref["dW"], ref["dW_abs"]))
    return worst


def test_head_bounds_are_eight_times_the_measured_fp32_error_and_the_docstring_says_so():
    """The measurement the bounds of test_gpu_misc2d.py come from.  A bound must be at least what is measured here and at most 8 x
    that, rounded up to two digits, and the table of the GPU file's docstring must show both figures."""
    worst = measured_fp32_errors()
    print("fp32 restatement against float64:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(G.HEAD_BOUNDS)
    for k, v in worst.items():
        assert 0 < v <= G.HEAD_BOUNDS[k] <= _round_up(8 * v) * (1 + 1e-12), (k, v, G.HEAD_BOUNDS[k])
        row = re.search(r"^\s+" + k + r"\s+(\S+)\s+(\S+)", G.__doc__, re.M)
        assert row and row.group(1) == f"{v:.2e}" and float(row.group(2)) == G.HEAD_BOUNDS[k], (k, f"{v:.2e}", row and row.groups())
    assert _round_up(1.344e-6) == pytest.approx(1.4e-6) and _round_up(2.0e-7) == pytest.approx(2.0e-7) and _round_up(0) == 0


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_prototypes_of_the_glue_entries_in_header_and_binding():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    ctype = {"int": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.sz, "mm_stream_t": _lib.vp}
    want = {"mm_copy_rows_bf16": 7, "mm_concat_bf16": 7, "mm_maxpool3x3s2_fwd": 9, "mm_maxpool3x3s2_bwd": 11, "mm_head_ws_bytes": 7,
            "mm_head_fwd": 15, "mm_head_bwd": 16, "mm_colsum_bf16": 9}
    twins = {n: _lib.H16_2D[n] for n in want if n in _lib.H16_2D}
    assert set(want) - set(twins) == {"mm_copy_rows_bf16", "mm_concat_bf16"}  # 2-byte copies: one build serves both formats
    assert twins["mm_colsum_bf16"] == "mm_colsum_f16" and all(t == n + "_f16" for n, t in twins.items() if n != "mm_colsum_bf16")
    for base, n_args in want.items():
        for name in (base, twins.get(base)):
            if name is None:
                continue
            m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
            assert m, f"{name} is not declared in include/mm2d3d.h"
            res, args = _lib._PROTOS[name]
            declared = [a.strip() for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            assert len(declared) == len(args) == n_args, name
            assert res is ctype[m.group(1)], name
            for a, t in zip(declared, args):  # pointers are void pointers to the binding, scalars keep their width
                base_type = re.sub(r"\bconst\b", "", a).rsplit(None, 1)[0].strip()
                assert t is (_lib.vp if "*" in a else ctype[base_type]), (name, a)
            assert hasattr(L, name)
            assert (res, args) == _lib._PROTOS[base]
