"""Host checks behind tests/test_gpu_spconv_rows.py: the float64 references of tests/_spconv_ref.py against torch float64 (index_add_,
einsum, autograd), the tile-table reference against a per-row loop, the conditions the makers promise for every case of the GPU
file's tables, the branch of the host dispatch every case is there for (csrc/spconv.hip and csrc/osconv.hip restated in Python),
the measurement from which the bounds come, the condition that a lost bf16 term exceeds the terms bound, and the C ABI of the
sparse engines (include/mm2d3d.h against mm2d3d_amd/_lib.py).  No GPU."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import _spconv_ref as R
import test_gpu_spconv_rows as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------------- references
def _torch_flat(W, tr, kflip, gap):
    """The flat weight buffer built with torch alone: slabs [Cin][Cout] or [Cout][Cin], ``gap`` NaN behind each, slabs reversed."""
    K = W.shape[0]
    buf = torch.full((K, W.shape[1] * W.shape[2] + gap), float("nan"), dtype=torch.float64)
    buf[:, : W.shape[1] * W.shape[2]] = (W.transpose(1, 2) if tr else W).reshape(K, -1)
    return (buf.flip(0) if kflip else buf).reshape(-1).numpy()


def _torch_apply(x, W, rb, n_out):
    out = torch.zeros(n_out, W.shape[2], dtype=torch.float64)
    off = rb["offsets"]
    for k in range(rb["K"]):
        s, d = (torch.from_numpy(rb[n][off[k]: off[k + 1]].astype(np.int64)) for n in ("src", "dst"))
        out.index_add_(0, d, torch.einsum("rc,cd->rd", x[s], W[k]))
    return out


@pytest.mark.parametrize("tr,kflip,gap", [(False, 0, 0), (True, 0, 0), (False, 1, 0), (False, 0, 5), (True, 1, 3)])
@pytest.mark.parametrize("unique", [False, True])
def test_apply_and_dw_references_match_torch_float64(tr, kflip, gap, unique):
    K, Cin, Cout, n_out, n_in = 5, 6, 4, 60, 40
    rb = R.make_rulebook(K, n_out, n_in, (0, 7, 12, 1, 9), 3, unique)
    g = np.random.default_rng(1)
    x = torch.from_numpy(g.standard_normal((n_in, Cin))).requires_grad_(True)
    W = torch.from_numpy(g.standard_normal((K, Cin, Cout))).requires_grad_(True)
    dout = g.standard_normal((n_out, Cout))
    lay = R.layout(K, Cin, Cout, tr, kflip, gap)
    flat = _torch_flat(W.detach(), tr, kflip, gap)
    assert np.array_equal(np.nan_to_num(R.put_weights(W.detach().numpy(), lay), nan=7.0), np.nan_to_num(flat, nan=7.0))
    assert np.isnan(flat).sum() == K * gap
    out = _torch_apply(x, W, rb, n_out)
    ref, a = R.apply(x.detach().numpy(), flat, lay, rb, n_out)
    assert np.abs(ref - out.detach().numpy()).max() <= 1e-13 and (a >= np.abs(ref) * (1 - 1e-15)).all()
    assert not ref[(rb["nbr"] >= 0).sum(0) == 0].any()
    (out * torch.from_numpy(dout)).sum().backward()
    gw, ga = R.dw(x.detach().numpy(), dout, rb)
    assert np.abs(gw - W.grad.numpy()).max() <= 1e-13 and (ga >= np.abs(gw) * (1 - 1e-15)).all()
    assert not gw[np.diff(rb["offsets"]) == 0].any()
    # the other role assignment (Deconvolution, the data gradient): src and dst exchanged, the weights read transposed
    layT = R.layout(K, Cout, Cin, not tr, kflip, gap)
    dx, dxa = R.apply(dout, flat, layT, R.swapped(rb, n_in), n_in)
    assert np.abs(dx - x.grad.numpy()).max() <= 1e-13 and (dxa >= np.abs(dx) * (1 - 1e-15)).all()
    assert np.array_equal(R.get_weights(flat, layT), np.swapaxes(W.detach().numpy(), 1, 2))


def test_derived_lists_and_csr_are_what_a_loop_gives():
    rb = R.make_rulebook(4, 30, 9, (3, 0, 10, 5), 5, False)
    src, dst, rows = [], [], [[] for _ in range(30)]
    for k in range(4):
        for o in range(30):
            if rb["nbr"][k, o] >= 0:
                rows[o].append(len(src))
                src.append(rb["nbr"][k, o])
                dst.append(o)
    assert rb["src"].tolist() == src and rb["dst"].tolist() == dst and rb["offsets"].tolist() == [0, 3, 3, 13, 18]
    assert rb["csr_pos"].tolist() == [p for r in rows for p in r] and np.diff(rb["csr_off"]).tolist() == [len(r) for r in rows]


@pytest.mark.parametrize("K,n", [(27, 1), (27, 63), (8, 64), (27, 65), (8, 300), (27, 1000)])
def test_os_table_reference_against_a_per_row_loop(K, n):
    rb = R.make_nbr_mixture(K, n, max(n // 2, 1), 11)
    t = R.os_table(rb["nbr"])
    masks = [sum(1 << k for k in range(K) if rb["nbr"][k, o] >= 0) for o in range(n)]
    order = sorted(range(n), key=lambda o: (masks[o], o))
    nt = -(-n // 64)
    assert t["nt"] == nt and t["npad"] == nt * 64 and t["dst"].tolist() == order + [-1] * (nt * 64 - n)
    for j in range(nt * 64):
        col = rb["nbr"][:, order[j]].tolist() if j < n else [-1] * K
        assert t["nbrp"][:, j].tolist() == col
    for i in range(nt):
        m = 0
        for o in order[i * 64: (i + 1) * 64]:
            m |= masks[o]
        assert int(t["tmask"][i]) == m


# ------------------------------------------------------------------------------------------------------------------- makers
def test_every_rulebook_is_what_the_table_says():
    want = {"ragged27": (27, 1500, 1300, False), "ragged8u": (8, 3000, 900, True), "k1": (1, 200, 200, True), "k32": (32, 200, 200, False),
            "empty": (27, 70, 70, True), "big_lo": (27, 16384, 16384, False), "big_hi": (27, 16384, 16384, False),
            "big_tr256": (27, 12000, 12000, False)}
    assert {n: (c["K"], c["n_out"], c["n_in"], c["unique"]) for n, c in G.RULEBOOKS.items()} == want
    assert G.RULEBOOKS["ragged27"]["sizes"] == (0, 1, 15, 16, 17, 0, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 0, 511, 513, 1, 33, 1024,
                                                1025, 700, 31, 2, 0)
    assert G.RULEBOOKS["ragged8u"]["sizes"] == (0, 1, 16, 17, 255, 257, 1000, 64) and G.RULEBOOKS["k1"]["sizes"] == (130,)
    assert G.RULEBOOKS["k32"]["sizes"] == tuple(32 * (k % 5) for k in range(32)) and not any(G.RULEBOOKS["empty"]["sizes"])
    assert sum(G.RULEBOOKS["big_lo"]["sizes"]) == 199999 and sum(G.RULEBOOKS["big_hi"]["sizes"]) == 200000
    assert len(set(G.RULEBOOKS["big_hi"]["sizes"])) > 5 and sum(G.RULEBOOKS["big_tr256"]["sizes"]) >= 262144
    for name, c in G.RULEBOOKS.items():
        rb = G.rulebook(name)  # the maker asserts the sizes, the rows without a rule, the uniqueness
        R.check_rulebook(rb, c["sizes"])
        assert rb["nbr"].shape == (c["K"], c["n_out"]) and rb["offsets"].dtype == rb["src"].dtype == rb["csr_pos"].dtype == np.int32
        again = R.derive(rb["nbr"])
        assert all(np.array_equal(again[k], rb[k]) for k in ("src", "dst", "offsets", "csr_off", "csr_pos"))
    with pytest.raises(AssertionError):
        R.make_rulebook(2, 10, 10, (3, 4), 0, True)  # 7 unique destinations and 5 rows without a rule do not fit in 10


def test_input_kinds_keep_their_promises():
    g = R.grid((500, 40), 1)
    assert set(np.unique(g * 8)) == set(range(-8, 9))
    for fmt in ("bf16", "fp16"):
        assert np.array_equal(R.round16(g, fmt), g)
    with pytest.raises(AssertionError):
        R.assert_grid_exact(np.array([2.0 ** 18]))
    for terms in (1, 2, 3):
        v = R.term_values(4000, 5, terms)  # asserts the exact three-term split
        t = R.split_bf16(v.astype(np.float32), 3)
        if terms >= 2:
            assert (np.abs(t[1]) >= 1.5 * 2.0 ** -9 * np.abs(t[0])).all()
        if terms == 3:
            assert (np.abs(t[2]) >= 1.5 * 2.0 ** -18 * np.abs(t[0])).all()
    rb = G.rulebook("ragged8u")
    for kind in R.TERM_KINDS:
        x, W = R.make_terms(kind, rb, 48, 16, 9)
        assert ((x != 0).sum(1) == 1).all() and (W != 0).all() and len(np.unique(np.flatnonzero(x)[:48] % 48)) == 48
    with pytest.raises(AssertionError):
        R.make_terms("full", G.rulebook("ragged27"), 32, 16, 0)  # more than one rule per row: not single products


def test_every_case_satisfies_what_its_maker_promises():
    for name, c in G.APPLY_CASES.items():
        rb = G.rulebook(c["rb"])
        assert c["path"] == "csr" or rb["unique"], name
        assert c["ld_in"] >= c["Cin"] and c["ld_out"] >= c["Cout"] and set(c["kinds"]) <= {"grid", "normal"} and "grid" in c["kinds"]
        for kind in c["kinds"]:
            d = G.apply_inputs(name, kind)  # asserts the grid condition
            assert d["x"].shape == (rb["n_in"], c["Cin"]) and np.isnan(d["flat"]).sum() == rb["K"] * c["gap"]
            assert np.array_equal(d["x"].astype(np.float32), d["x"]) and (d["abs"] >= np.abs(d["ref"]) * (1 - 1e-15)).all()
    for name in G.APPLY_TERMS:
        c = G.APPLY_CASES[name]
        assert G.rulebook(c["rb"])["unique"] and G.apply_class(c) == "apply_split"
    assert {G.APPLY_CASES[n]["path"] for n in G.APPLY_TERMS} == {"csr", "unique"}
    for name, c in G.DW_CASES.items():
        assert c["rows"] in ("fp32", "bf16", "fp16") and "grid" in c["kinds"]
        for kind in c["kinds"]:
            d = G.dw_inputs(name, kind)
            if c["rows"] != "fp32":
                assert np.array_equal(R.round16(d["x"], c["rows"]), d["x"]) and np.array_equal(R.round16(d["g"], c["rows"]), d["g"])
    for name, c in G.OS_TABLES.items():
        rb = G.os_rulebook(name)
        cnt = (rb["nbr"] >= 0).sum(0)
        assert rb["nbr"].shape == (c["K"], c["n"])
        if c["up"]:
            assert (cnt == 1).all()
        elif c["n"] >= 1000:
            assert 0.07 < (cnt == c["K"]).mean() < 0.13 and 5 <= (cnt == 0).sum() and set(np.unique(cnt)) == {0, 1, 2, 3, 4, c["K"]}
    assert {(c["K"], c["n"]) for c in G.OS_TABLES.values() if not c["up"]} >= {(K, n) for K in (27, 8) for n in (1, 63, 64, 65, 1000, 65536, 131072)}
    for name in G.OS_TERMS:
        assert G.os_rulebook(G.OS_CASES[name]["table"])["unique"]
    assert {G.OS_CASES[n]["Cin"] for n in G.OS_CASES} >= {16, 48, 80, 224}


def test_every_kernel_family_meets_every_crossing():
    """Transposed strides, kflip, w_kstride > Cin * Cout and ld_out > Cout: at least one of each per kernel family."""
    fam = {}
    for c in G.APPLY_CASES.values():
        f = fam.setdefault(c["want"].split()[0] + (" edge" if " edge" in c["want"] else ""), set())
        f |= {k for k, v in (("tr", c["tr"]), ("kflip", c["kflip"]), ("gap", c["gap"]), ("ld_out", c["ld_out"] > c["Cout"])) if v}
    fam["k_generic"] = fam.pop("k_generic_rows") | fam.pop("k_generic_rules")
    assert set(fam) == {"k_rows_narrow", "k_gather_gemm edge", "k_gather_gemm_direct", "k_gather_gemm", "k_gather_gemm_s3", "k_generic"}
    assert all(v == {"tr", "kflip", "gap", "ld_out"} for v in fam.values()), fam


# ------------------------------------------------------------------------------------------------------------- reachability
def _apply_branch(c, mode=None):
    rb = G.RULEBOOKS[c["rb"]]
    return R.apply_branch(sum(rb["sizes"]), c["Cin"], c["Cout"], rb["K"], c["path"] == "unique", c["ld_in"], c["ld_out"], c["in_off"], 0,
                          c["mode"] if mode is None else mode)


def test_every_apply_case_reaches_the_branch_its_comment_names():
    for name, c in G.APPLY_CASES.items():
        br, want = _apply_branch(c), c["want"].split()
        assert br["kernel"] == want[0], (name, br)
        for tok in want[1:]:
            if tok == "edge":
                assert br["edge"], name
            elif tok == "beyond_preload":
                assert br["beyond_preload"], name
            elif tok.startswith("k_csr_reduce"):
                assert br["reduce"] == tok, (name, br)
            else:
                k, v = tok.split("=")
                assert br[k] == int(v), (name, tok, br)
        if want[0] in ("k_gather_gemm", "k_gather_gemm_direct") and "edge" not in want:
            assert not br["edge"], name
        if want[0] == "k_gather_gemm_s3":
            assert br["terms"] == (2 if c["mode"] == G.TWO_TERMS else 3) and ("beyond_preload" in want) == br["beyond_preload"], name
        assert (br["reduce"] is None) == (c["path"] == "unique" or want[0] in ("k_rows_narrow", "k_generic_rows")), name
    lo, hi = G.APPLY_CASES["direct_16_16_big_lo"], G.APPLY_CASES["staged_16_16_big_hi"]
    assert (lo["Cin"], lo["Cout"]) == (hi["Cin"], hi["Cout"]) and sum(G.RULEBOOKS["big_hi"]["sizes"]) - sum(G.RULEBOOKS["big_lo"]["sizes"]) == 1
    # every other s3 case runs with fewer rules per workgroup than big_tr256; the halving loop ends at 64, 128 and 256
    assert {_apply_branch(c)["tr"] for c in G.APPLY_CASES.values() if c["want"].startswith("k_gather_gemm_s3")} == {64, 256}
    assert _apply_branch(G.APPLY_CASES["s3_64_64_big_tr256"])["tr"] == 256
    assert R.apply_branch(262144 - 256, 64, 64, 27, False, 68, 64)["tr"] == 128
    for name in G.APPLY_TERMS:  # the control runs the same kernel with two terms
        assert _apply_branch(G.APPLY_CASES[name], G.TWO_TERMS)["terms"] == 2 and _apply_branch(G.APPLY_CASES[name], G.DEFAULT)["terms"] == 3
    for name in ("s3_48_48", "direct_16_16", "s3_32_16_unique"):  # the least workspace of the refusal test follows the branch
        assert (_apply_branch(G.APPLY_CASES[name])["kernel"] == "k_gather_gemm_s3") == name.startswith("s3")
    seen = {(_apply_branch(c)["kernel"], _apply_branch(c).get("ncbw")) for c in G.APPLY_CASES.values()}
    assert {n for k, n in seen if k == "k_gather_gemm_s3"} >= {1, 2, 3, 4, 5, 6} and {n for k, n in seen if k == "k_gather_gemm_direct"} >= {1, 2, 4, 8}


def test_every_dw_case_reaches_the_branch_its_comment_names():
    for name, c in G.DW_CASES.items():
        Rn = sum(G.RULEBOOKS[c["rb"]]["sizes"])
        rows = {"fp32": 0, "bf16": 1, "fp16": 2}[c["rows"]]
        br, want = R.dw_branch(Rn, c["Cin"], c["Cout"], rows, c["mode"]), c["want"].split()
        assert br["kernel"] == want[0], (name, br)
        assert br["wide"] == ("wide" in want), (name, br)
        tile = [t for t in want if t.startswith("tile=")]
        if tile:
            assert br["tile"] == tuple(int(v) for v in tile[0][5:].split("x")), (name, br)
        if c["twin"] == G.DW_NARROW:
            tw = R.dw_branch(Rn, c["Cin"], c["Cout"], rows, c["mode"] | c["twin"])
            assert not tw["wide"] and max(tw["tile"]) <= 4 and tw["kernel"] == br["kernel"] and tw["chunk"] == br["chunk"]
            assert br["wide"] == (c["rb"] == "big_hi")  # one rule fewer (big_lo) keeps the <= 4 x 4 tiles
        if c["twin"] == G.DW16_ELEM:
            tw = R.dw_branch(Rn, c["Cin"], c["Cout"], rows, c["mode"] | c["twin"])
            assert tw["kernel"] == "k_dw_direct_s3" and tw["tile"] == br["tile"] and tw["chunk"] == br["chunk"] and br["terms"] == rows
    tiles = {R.dw_branch(sum(G.RULEBOOKS[c["rb"]]["sizes"]), c["Cin"], c["Cout"], 0, c["mode"])["tile"] for c in G.DW_CASES.values() if c["rows"] == "fp32"}
    assert {(5, 5), (6, 3), (1, 6), (4, 3), (3, 3), (1, 3), (1, 1), (2, 3), (2, 2)} <= tiles
    assert R.dw_tiles(10, 5, True) == (5, 5) and R.dw_tiles(10, 5, False) == (4, 3) and R._dw_tile(5) == 3 and R._dw_tile(7) == 4


def test_every_os_case_reaches_the_form_its_comment_names():
    for name, c in G.OS_CASES.items():
        t = G.OS_TABLES[c["table"]]
        br, want = R.os_branch(-(-t["n"] // 64), c["Cout"], t["K"]), c["want"].split()
        assert br["nw"] == int(want[0][3:]), (name, br)
        assert [(w, cnt) for w, cnt, _ in br["launches"]] == [tuple(int(v) for v in tok.split("x")) for tok in want[1:]], (name, br)
        assert sum(w * cnt for w, cnt, _ in br["launches"]) == c["Cout"] // 16
        assert all(eff == br["nw"] for _, _, eff in br["launches"]), (name, br)  # no launch falls back to four waves
    forms = {(R.os_branch(-(-G.OS_TABLES[c["table"]]["n"] // 64), c["Cout"], G.OS_TABLES[c["table"]]["K"])["nw"], w)
             for c in G.OS_CASES.values() for w, _, _ in R.os_branch(-(-G.OS_TABLES[c["table"]]["n"] // 64), c["Cout"], G.OS_TABLES[c["table"]]["K"])["launches"]}
    assert forms == {(16, 1), (8, 1), (8, 2), (4, 1), (4, 2), (4, 3)}


def test_the_four_block_instance_of_the_os_engine_cannot_be_selected():
    """parts >= ceil(ncb / 3) and the parts are near-equal: no launch is four blocks wide, whatever the arguments."""
    widths = {w for nt in (1, 2, 15, 16, 100, 341, 342, 511, 512, 683, 1023, 1024, 2047, 2048, 5000) for ncb in range(1, 33) for K in (8, 27)
              for w, _, _ in R.os_branch(nt, 16 * ncb, K)["launches"]}
    assert widths == {1, 2, 3}


# -------------------------------------------------------------------------------------------------------------- measurement
def _round_up(v):
    """Up to two significant digits."""
    if v == 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def _live(c):
    rb = G.rulebook(c["rb"])
    return (rb["nbr"] >= 0).sum(0) > 0 if c["path"] == "unique" else np.ones(rb["n_out"], bool)


def _apply_restated(name, kind, pairs=R.PAIRS3):
    c, d = G.APPLY_CASES[name], G.apply_inputs(name, kind)
    rb = G.rulebook(c["rb"])
    if G.apply_class(c) == "apply_split":
        return R.apply_split(d["x"], d["flat"], d["lay"], rb, rb["n_out"], pairs)
    return R.apply_fp32(d["x"], d["flat"], d["lay"], rb, rb["n_out"])


def _dw_restated(name, acc):
    c, d = G.DW_CASES[name], G.dw_inputs(name, "normal")
    rows = {"fp32": 0, "bf16": 1, "fp16": 2}[c["rows"]]
    br = R.dw_branch(sum(G.RULEBOOKS[c["rb"]]["sizes"]), c["Cin"], c["Cout"], rows, c["mode"])
    kind = {"k_dw_generic": "generic", "k_dw_direct": "direct"}.get(br["kernel"], "split")
    pairs = {3: R.PAIRS3, 2: R.PAIRS2}.get(br.get("terms"), R.PAIRS1)
    return R.dw_fp32(d["x"], d["g"], G.rulebook(c["rb"]), br["chunk"], kind, pairs, c["rows"] if rows else "bf16", d["prev"] if acc else None)


@functools.lru_cache(maxsize=None)
def measured_fp32_errors():
    """Largest error of the restatements against float64 per class, over all its normal (terms) cases."""
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    for name, c in G.APPLY_CASES.items():
        if "normal" in c["kinds"]:
            d, live = G.apply_inputs(name, "normal"), _live(c)
            note(G.apply_class(c), R.rel_error(_apply_restated(name, "normal")[live], d["ref"][live], d["abs"][live]))
    for name in G.APPLY_TERMS:
        for kind in R.TERM_KINDS:
            d, live = G.apply_inputs(name, kind), _live(dict(G.APPLY_CASES[name], path="unique"))
            note("apply_split_terms", R.rel_error(_apply_restated(name, kind)[live], d["ref"][live], d["abs"][live]))
    for name, c in G.DW_CASES.items():
        if "normal" in c["kinds"]:
            d = G.dw_inputs(name, "normal")
            for acc in (0, 1):
                want, allow = d["ref"] + (d["prev"] if acc else 0.0), d["abs"] + (np.abs(d["prev"]) if acc else 0.0)
                note(G.dw_class(c), R.rel_error(_dw_restated(name, acc), want, allow))
    for name, c in G.OS_CASES.items():
        rb = G.os_rulebook(c["table"])
        for fmt in G.OS_FMTS:
            if "normal" in c["kinds"]:
                d = G.os_inputs(name, "normal", fmt)
                got = R.apply_split(d["x"], d["flat"], d["lay"], rb, rb["n_out"], R.PAIRS3 if fmt == "fp32" else R.PAIRS1, "bf16" if fmt == "fp32" else fmt)
                note(G.os_class(fmt), R.rel_error(got, d["ref"], d["abs"]))
    for name in G.OS_TERMS:
        rb = G.os_rulebook(G.OS_CASES[name]["table"])
        for kind in R.TERM_KINDS:
            d = G.os_inputs(name, kind, "fp32")
            note("os_split_terms", R.rel_error(R.apply_split(d["x"], d["flat"], d["lay"], rb, rb["n_out"]), d["ref"], d["abs"]))
    return worst


def test_bounds_are_eight_times_the_measured_fp32_error_and_the_docstring_says_so():
    """The measurement the bounds of test_gpu_spconv_rows.py come from: a recorded bound is 8 x the figure measured here, rounded up
    to two digits, and the table of the GPU file's docstring shows both."""
    worst = measured_fp32_errors()
    print("fp32 restatement against float64:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(G.BOUNDS)
    for k, v in worst.items():
        assert v > 0 and G.BOUNDS[k] == pytest.approx(_round_up(8 * v), rel=1e-9), (k, v, _round_up(8 * v), G.BOUNDS[k])
        row = re.search(r"^\s+" + k + r"\s+(\S+)\s+(\S+)", G.__doc__, re.M)
        assert row and row.group(1) == f"{v:.2e}" and float(row.group(2)) == G.BOUNDS[k], (k, f"{v:.2e}", row and row.groups())
    assert _round_up(1.344e-6) == pytest.approx(1.4e-6) and _round_up(2.0e-7) == pytest.approx(2.0e-7) and _round_up(0) == 0


# -------------------------------------------------------------------------------------------------------------------- teeth
DROP_X1W3 = tuple(p for p in R.PAIRS3 if p != (2, 0))  # pairs are (weight term, row term)
DROP_X3W1 = tuple(p for p in R.PAIRS3 if p != (0, 2))


@pytest.mark.parametrize("name", G.APPLY_TERMS)
def test_a_lost_term_exceeds_the_terms_bound_four_times(name):
    """A condition on the inputs: with two terms, or with three and either 2^-18 product dropped, the restatement is wrong by at
    least 4 x the terms bound on the sub-kinds that isolate the lost products."""
    bound = G.BOUNDS["apply_split_terms"]
    live = _live(dict(G.APPLY_CASES[name], path="unique"))

    def err(kind, pairs):
        d = G.apply_inputs(name, kind)
        return R.rel_error(_apply_restated(name, kind, pairs)[live], d["ref"][live], d["abs"][live])

    for kind in R.TERM_KINDS:  # two terms lose x1w3 (xb_wf), x3w1 (xf_wb), x2w2 (x2_w2) and all three (full)
        assert err(kind, R.PAIRS2) >= 4 * bound, (name, kind, "two terms", err(kind, R.PAIRS2))
        assert err(kind, R.PAIRS3) <= bound / 8 * (1 + 1e-9)
    for kind in ("xb_wf", "full"):
        assert err(kind, DROP_X1W3) >= 4 * bound, (name, kind, "x1w3 dropped", err(kind, DROP_X1W3))
    for kind in ("xf_wb", "full"):
        assert err(kind, DROP_X3W1) >= 4 * bound, (name, kind, "x3w1 dropped", err(kind, DROP_X3W1))
    assert err("xf_wb", DROP_X1W3) <= bound and err("xb_wf", DROP_X3W1) <= bound  # the sub-kinds isolate what they name


# -------------------------------------------------------------------------------------------------------------------- C ABI
def test_prototypes_of_the_sparse_engines_in_header_and_binding():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mm2d3d.h")).read(), flags=re.S)
    ctype = {"int": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.sz, "mm_stream_t": _lib.vp}
    found = re.findall(r"\b(int|size_t|int64_t)\s+(mm_spconv_\w+|mm_os_table_\w+|mm_up_neighbors)\s*\(([^)]*)\)\s*;", txt)
    names = [n for _, n, _ in found]
    assert len(names) == len(set(names)) == 27 and {"mm_spconv_apply", "mm_spconv_apply_packed", "mm_spconv_dw_partial", "mm_os_table_build",
                                                     "mm_up_neighbors", "mm_spconv_os_apply_f16", "mm_spconv_dw_reduce_batch"} <= set(names)
    assert {n for n in _lib._PROTOS if re.match(r"mm_spconv_|mm_os_table_|mm_up_neighbors", n)} == set(names)
    for res, name, arglist in found:
        pres, pargs = _lib._PROTOS[name]
        declared = [a.strip() for a in arglist.split(",") if a.strip() not in ("", "void")]
        assert len(declared) == len(pargs), name
        assert pres is ctype[res], name
        for a, t in zip(declared, pargs):  # pointers are void pointers to the binding, scalars keep their width
            base_type = re.sub(r"\bconst\b", "", a).rsplit(None, 1)[0].strip()
            assert t is (_lib.vp if "*" in a else ctype[base_type]), (name, a)
        assert hasattr(L, name)
