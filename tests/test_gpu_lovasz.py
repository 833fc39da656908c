"""The Lovasz-softmax kernels through the C ABI (include/mm2d3d.h mm_lovasz_*, csrc/lovasz.hip), stage by stage, against the float64
references of tests/_lovasz_ref.py.

A single row's weight depends on the order of near-tied errors, so no test compares the weights of the kernels with weights
computed from other errors: Stage A checks the errors, Stage B takes the kernel's OWN float32 errors and checks the sort, the scan
and the closed forms on them (exact in the order), Stage C checks the backward row kernel on given coefficients, and the end-to-end
test checks the loss alone, which does not depend on the order of ties and is 1-Lipschitz in max |delta e|.

The bounds are stated in the units of tests/test_lovasz_host.py, which measures the float32 restatements against float64 over all
cases of this file and holds each bound between that figure and 8 x it."""
import functools

import numpy as np
import pytest
import torch

import _lovasz_ref as R
from _gpu_rows import SENTINEL, Ints, Rows, abi, dev, vec

gpu = pytest.mark.gpu

# err: absolute (against 1);  bwd: per entry, relative to |grad_out| * max |coef|;  loss: the err bound plus the summation term
LOVASZ_BOUNDS = {"err": 3.3e-6, "bwd": 1.9e-6, "loss": 3.6e-6}

TILE, SCAN_BLK, T = R.TILE, R.SCAN_BLK, R.T
N_TWO_SCAN_GROUPS = 2 * TILE + 1  # 3 tiles: 3072 counters per pass, two workgroups of the offset scan
N_EVERY_LEVEL = (T * SCAN_BLK // R.RADIX) * TILE + 1  # 513 tiles: 257 block sums, the one-workgroup scan walks them in two rounds
SHAPES = (0, 1, 2, TILE - 1, TILE, TILE + 1, N_TWO_SCAN_GROUPS, 3 * TILE + 7)
CLASSES = (1, 2, 6, 11, 32)


def _cases():
    cases = {}
    for n in SHAPES:
        for c in CLASSES:
            cases[f"n{n}_c{c}"] = dict(n=n, c=c, labels="mix", classes="all" if (n + c) % 2 else "present", ld=c if c % 2 else c + 3)
    cases["every_scan_level_c2"] = dict(n=N_EVERY_LEVEL, c=2, labels="mix", classes="present", ld=2)
    for classes in ("present", "all"):
        cases[f"all_ignored_{classes}"] = dict(n=TILE + 1, c=6, labels="all_ignored", classes=classes, ld=6)
        cases[f"absent_{classes}"] = dict(n=3 * TILE + 7, c=6, labels="absent", classes=classes, ld=9)
        cases[f"one_class_{classes}"] = dict(n=TILE + 1, c=6, labels="one_class", classes=classes, ld=6)
    return cases


CASES = _cases()
# Stage C: (case, source of coef, grad_out, ld, ld_d)
BWD_CASES = {f"{name}_{src}_g{g}": dict(case=name, src=src, g=g, ld=ld, ld_d=ld_d)
             for name, ld, ld_d in (("n1_c6", 6, 6), ("n1025_c1", 1, 4), ("n1025_c2", 5, 2), ("n3079_c6", 9, 11), ("n3079_c11", 11, 11),
                                    ("n1023_c32", 35, 37), ("absent_all", 6, 8), ("all_ignored_present", 6, 6))
             for src, g in (("grid", 1.0), ("stage_b", -0.5), ("grid", 65536.0))}


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name]
    d = R.make(c["n"], c["c"], 11 + c["n"] % 97 + c["c"], c["labels"])
    for v in d.values():
        v.setflags(write=False)
    return d


def grid_coef(name):
    """Coefficients on the 1/64 grid in [-1, 1], zero in every 4th row: products with float32 p stay float32-sized."""
    c = CASES[name]
    rng = np.random.default_rng(5 + c["n"])
    coef = rng.integers(-64, 65, size=(c["c"], c["n"])).astype(np.float64) / 64
    coef[:, np.arange(c["n"]) % 4 == 1] = 0.0
    return coef


def _forward(name):
    c, d = CASES[name], inputs(name)
    L, _lib = abi()
    n, C = c["n"], c["c"]
    x = Rows(d["x"].copy(), n, C, c["ld"])  # the shared inputs are read-only: torch wants writable arrays
    lab = Ints(d["labels"].copy(), dtype=torch.int64, fill=0)
    err, coef, stats = vec(None, n * C), vec(None, n * C), vec(None, 3)
    nbytes = int(L.mm_lovasz_ws_bytes(n, C))
    assert nbytes == R.ws_bytes(n, C)
    ws = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev())
    ws[nbytes:] = 0x5A
    rc = L.mm_lovasz_fwd(x.ptr, c["ld"], n, C, lab.ptr, -100, 1 if c["classes"] == "all" else 0, err.ptr, coef.ptr, stats.ptr,
                         ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert rc == 0, L.mm_last_error()
    assert err.padding_untouched() and coef.padding_untouched() and stats.padding_untouched() and lab.padding_untouched()
    assert bool((ws[nbytes:] == 0x5A).all()), "written behind the workspace"
    return dict(err=err.get32().reshape(C, n), coef=coef.get32().reshape(C, n), stats=stats.get32().reshape(3))


@functools.lru_cache(maxsize=None)
def run(name):
    """The forward of a case, run TWICE (asserted bit-identical), shared by the tests of the case and left unchanged."""
    a, b = _forward(name), _forward(name)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k}: two calls differ"
        a[k].setflags(write=False)
    return a


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stage_a_errors_and_counted_rows(name):
    c, d, got = CASES[name], inputs(name), run(name)
    ref, live = R.errors(d["x"], d["labels"])
    assert np.array_equal(got["err"][:, ~live], np.full((c["c"], int((~live).sum())), -1, np.float32))
    worst = np.abs(got["err"][:, live].astype(np.float64) - ref[:, live]).max(initial=0.0)
    print(f"{name}: err {worst:.3e}")
    assert worst <= LOVASZ_BOUNDS["err"]
    assert ((got["err"][:, live] >= 0) & (got["err"][:, live] <= 1)).all()
    assert got["stats"][2] == live.sum()


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stage_b_sort_scan_and_closed_forms_on_the_kernels_own_errors(name):
    c, d, got = CASES[name], inputs(name), run(name)
    ref = R.rank_stage(got["err"], d["labels"], c["classes"])
    coef = got["coef"].astype(np.float64)
    assert np.array_equal(np.sign(coef), np.sign(ref["coef"]))
    rel = np.abs(coef - ref["coef"]) / np.where(ref["coef"] == 0, 1.0, np.abs(ref["coef"]))
    print(f"{name}: coef rel {rel.max(initial=0.0):.3e} loss {got['stats'][0]:.7f} ref {ref['loss']:.7f}")
    assert rel.max(initial=0.0) <= R.COEF_REL
    assert abs(float(got["stats"][0]) - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    assert got["stats"][1] == ref["n_included"] and got["stats"][2] == ref["counted"]
    inc, G, live = R.included_classes(d["labels"], c["c"], c["classes"])
    assert not coef[~inc].any() and not coef[:, ~live].any()
    if c["labels"] == "all_ignored":
        assert not got["stats"].any() and not coef.any()
    if c["labels"] in ("absent", "one_class"):
        for k in np.flatnonzero(G == 0):
            want = 0 if c["classes"] == "present" else 1
            assert (coef[k] != 0).sum() == want and (np.abs(coef[k]).max() == np.float32(1) / np.float32(c["c"]) or not want)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end_loss_against_the_float64_definition(name):
    c, d, got = CASES[name], inputs(name), run(name)
    ref = R.loss_by_definition(R.errors(d["x"], d["labels"])[0], d["labels"], c["classes"])
    print(f"{name}: loss {got['stats'][0]:.7f} definition {ref['loss']:.7f} diff {abs(float(got['stats'][0]) - ref['loss']):.3e}")
    assert abs(float(got["stats"][0]) - ref["loss"]) <= LOVASZ_BOUNDS["loss"]
    assert got["stats"][1] == ref["n_included"]


@gpu
@pytest.mark.parametrize("name", list(BWD_CASES))
def test_stage_c_backward_row_kernel(name):
    b = BWD_CASES[name]
    c, d = CASES[b["case"]], inputs(b["case"])
    L, _lib = abi()
    n, C = c["n"], c["c"]
    coef = grid_coef(b["case"]) if b["src"] == "grid" else run(b["case"])["coef"].astype(np.float64)
    x = Rows(d["x"].copy(), n, C, b["ld"])
    cf, g = vec(coef, n * C), vec([b["g"]], 1)
    out = Rows(None, n, C, b["ld_d"], off=3, fill=SENTINEL)
    rc = L.mm_lovasz_bwd(x.ptr, b["ld"], n, C, cf.ptr, g.ptr, out.ptr, b["ld_d"], None)
    torch.cuda.synchronize()
    assert rc == 0, L.mm_last_error()
    assert out.padding_untouched() and cf.padding_untouched()
    ref = R.backward(d["x"], coef, b["g"])
    unit = abs(b["g"]) * np.abs(coef).max(initial=0.0)
    got = out.get()
    if unit == 0:
        assert not got.any()
        return
    worst = np.abs(got - ref).max() / unit
    print(f"{name}: bwd {worst:.3e}")
    assert worst <= LOVASZ_BOUNDS["bwd"]
    assert not got[~coef.any(0)].any()


@gpu
def test_no_rows_launches_nothing_harmful():
    L, _lib = abi()
    stats = vec(None, 3)
    ws = torch.empty(int(L.mm_lovasz_ws_bytes(0, 6)), dtype=torch.uint8, device=dev())
    assert L.mm_lovasz_fwd(None, 6, 0, 6, None, -100, 1, None, None, stats.ptr, ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert not stats.get32().any() and stats.padding_untouched()
    assert L.mm_lovasz_bwd(None, 6, 0, 6, None, None, None, 6, None) == 0
