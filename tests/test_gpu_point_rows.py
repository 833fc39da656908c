"""The per-point / per-voxel row kernels of csrc/point.hip, called straight through the C ABI (mm_gate_fwd, mm_gate_bwd,
mm_segment_reduce, mm_row_gather, mm_linear_fwd, mm_linear_bwd) against the float64 numpy references of tests/_point_ref.py.

Linear, segment sum and row gather run on GRID inputs (multiples of 1/8, or integers above 65,536 rows) for which every fp32
operation of the kernels is exact in any order (the makers assert the condition): the results must EQUAL the float64 reference.
Segment mean and the gather that divides by the count are one fp32 division of an exact sum: within 1 ulp of
np.float32(sum) / np.float32(count).  Observed on an MI355X: 0 ulp in every case (the division is correctly rounded).

Pitched operands are views into wider buffers; inputs carry NaN in their padding, outputs a sentinel that must survive.

Gate: sigmoid goes through expf, so the comparison has a tolerance, and it is not invented.  tests/_point_ref.py gate_fp32 restates
the kernels' formulas in numpy float32; its largest error against the float64 reference over ALL the cases of GATE_CASES, in the
units of _point_ref.gate_errors, measured on the CPU (test_point_rows_host.py repeats the measurement), is

    quantity   fp32 restatement   bound = 8 x (rounded up)
    mask       1.68e-07           1.4e-06     absolute
    y          1.87e-07           1.5e-06     relative to |x|
    dx         1.18e-07           9.5e-07     relative to |dy| + sum_c |dy_c x_c| |w|
    dw         1.98e-07           1.6e-06     relative to sum_rows |dz x| + |dw0|
    db         1.09e-07           8.8e-07     relative to sum_rows |dz| + |db0|

The kernel is allowed 8 x that: another expf and another summation order cost a few ulp each."""
import functools

import numpy as np
import pytest
import torch

import _point_ref as R
from _gpu_rows import SENTINEL, Rows as _Rows, abi as _abi, dev as _dev, ints as _ints, vec as _vec  # shared with the loss and lift files

pytestmark = pytest.mark.gpu

GATE_BOUNDS = dict(mask=1.4e-06, y=1.5e-06, dx=9.5e-07, dw=1.6e-06, db=8.8e-07)


# --------------------------------------------------------------------------------------------------------------- case tables
def _lin(cin, cout, n, **kw):
    c = dict(cin=cin, cout=cout, n=n, ld_x=cin, ld_y=cout, ld_dy=cout, ld_dx=cin, off_x=0, off_dx=0, bias=True, dx=True, dw=True,
             db=True, acc_dx=0, acc_w=0, k=3)
    assert not set(kw) - set(c)
    c.update(kw)
    return c


def _linear_cases():
    t = {}
    # row counts around the 256-thread block, the 64-row tile and the rows-per-block of the weight gradient (2048 generic, 4096 in
    # the 16-wide form): 1, 2, 7, 8 and 9 blocks of partial sums on either path (k_sum_partials loads them eight at a time)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 2049, 4097, 14337, 16385, 24577, 28673, 32769):
        t[f"16x6_n{n}"] = _lin(16, 6, n)
    for n in (0, 1, 63, 64, 65, 255, 257, 2049, 4097, 12289, 14337, 16385):
        t[f"5x7_n{n}"] = _lin(5, 7, n)
    for cin, cout, n in ((16, 16, 257), (16, 16, 4097), (16, 17, 257), (16, 17, 2049), (32, 16, 65), (32, 16, 256), (3, 1, 1),
                         (3, 1, 255), (3, 1, 2049)):
        t[f"{cin}x{cout}_n{n}"] = _lin(cin, cout, n)
    # which kernels run: pointer alignment and leading dimensions
    t["16x6_ldx20"] = _lin(16, 6, 257, ld_x=20, ld_dx=20)  # 16-wide form on pitched rows
    t["16x6_ldx18"] = _lin(16, 6, 257, ld_x=18)  # ld_x % 4 != 0: generic
    t["16x6_xoff1"] = _lin(16, 6, 257, off_x=1)  # x not 16-byte aligned: generic
    t["16x6_dxoff1"] = _lin(16, 6, 257, off_dx=1)  # 16-wide weight gradient, generic dx
    t["16x6_lddx18"] = _lin(16, 6, 4097, ld_dx=18)  # the same through the leading dimension of dx
    t["16x6_ldy9"] = _lin(16, 6, 257, ld_y=9, ld_dy=11)
    t["5x7_pitched"] = _lin(5, 7, 257, ld_x=8, ld_y=9, ld_dy=10, ld_dx=6)
    # modes
    t["16x6_nobias"] = _lin(16, 6, 257, bias=False)
    t["5x7_nobias"] = _lin(5, 7, 257, bias=False)
    t["16x6_nodx"] = _lin(16, 6, 257, dx=False)
    t["5x7_nodx"] = _lin(5, 7, 257, dx=False)
    t["16x6_nodb"] = _lin(16, 6, 4097, db=False)
    t["5x7_nodb"] = _lin(5, 7, 2049, db=False)
    t["16x6_dxonly"] = _lin(16, 6, 257, dw=False)
    t["5x7_dxonly"] = _lin(5, 7, 257, dw=False)
    t["16x6_accdx"] = _lin(16, 6, 257, acc_dx=1)  # 16-wide dx, accumulating
    t["16x6_accdx_ld20"] = _lin(16, 6, 4097, acc_dx=1, ld_dx=20)
    t["16x16_accdx"] = _lin(16, 16, 65, acc_dx=1)
    t["16x6_accdx_dxoff1"] = _lin(16, 6, 257, acc_dx=1, off_dx=1)
    t["5x7_accdx"] = _lin(5, 7, 257, acc_dx=1)
    t["16x6_accw"] = _lin(16, 6, 4097, acc_w=1)
    t["5x7_accw"] = _lin(5, 7, 2049, acc_w=1)
    t["16x6_accw_nodb"] = _lin(16, 6, 257, acc_w=1, db=False)
    t["5x7_accboth"] = _lin(5, 7, 257, acc_w=1, acc_dx=1, ld_dx=6)
    # one row block past each cap of the partial-sum grid (128 blocks in the 16-wide form, MAX_PART = 512), integer inputs
    t["16x6_cap128"] = _lin(16, 6, 524289 + 4096, k=0)
    t["5x7_cap512"] = _lin(5, 7, 1048577 + 2048, k=0)
    # 64 * (Cin + Cout) * 4 bytes of LDS: above 64 KiB the kernel's dynamic-LDS limit is raised; 150 KiB is the widest allowed
    t["160x112_lds"] = _lin(160, 112, 130)
    t["400x200_lds_max"] = _lin(400, 200, 130)
    return t


LINEAR_CASES = _linear_cases()


def linear_paths(c):
    """What csrc/point.hip selects for a case (linear16_ok and the block counts of mm_linear_bwd), restated."""
    fast = c["cin"] == 16 and c["cout"] <= 16 and c["ld_x"] % 4 == 0 and c["off_x"] % 4 == 0
    fast_dx = fast and c["ld_dx"] % 4 == 0 and c["off_dx"] % 4 == 0
    nblk = min(max(-(-c["n"] // (4096 if fast else 2048)), 1), 128 if fast else 512)
    return dict(fwd="fast" if fast else "generic", dx="fast" if fast_dx else "generic", w="fast" if fast else "generic", nblk=nblk,
                capped=-(-c["n"] // (4096 if fast else 2048)) > (128 if fast else 512))


@functools.lru_cache(maxsize=None)
def linear_inputs(name):
    """Grid inputs of a case (exactness asserted by the maker): made once, shared, never modified."""
    c = LINEAR_CASES[name]
    return R.make_linear(c["cin"], c["cout"], c["n"], c["k"], 100 + list(LINEAR_CASES).index(name))


def _seg(c, n_vox, n_free=5, big=False, ld_f=None, ld_o=None, ld_v=None, ld_g=None):
    return dict(c=c, n_vox=n_vox, n_free=n_free, big=big, ld_f=ld_f or c, ld_o=ld_o or c, ld_v=ld_v or c, ld_g=ld_g or c)


# channel counts at which gid / C crosses the 256-thread block boundary in the middle of a row (3, 17, 96) and at which it does not
SEGMENT_CASES = {
    "c1_v0": _seg(1, 0),
    "c1_v257": _seg(1, 257, big=True),
    "c3_v1": _seg(3, 1, n_free=0),
    "c3_v255": _seg(3, 255, big=True, ld_f=5, ld_o=4, ld_v=7, ld_g=6),
    "c3_v1000": _seg(3, 1000),
    "c16_v255": _seg(16, 255),
    "c16_v257": _seg(16, 257, big=True, ld_f=20, ld_o=17, ld_v=16, ld_g=24),
    "c17_v1": _seg(17, 1, ld_f=19, ld_o=18, ld_v=20, ld_g=17),
    "c17_v0": _seg(17, 0, ld_f=19, ld_o=18, ld_v=20, ld_g=21),
    "c17_v1000": _seg(17, 1000, big=True, ld_f=19, ld_o=17, ld_v=18, ld_g=23),
    "c96_v257": _seg(96, 257, ld_f=97, ld_o=100, ld_v=96, ld_g=99),
    "c96_v1000": _seg(96, 1000, big=True),
}


def segment_lengths(name):
    c = SEGMENT_CASES[name]
    n_vox = c["n_vox"]
    lens = np.random.default_rng(7).choice([1, 2, 7], size=n_vox)
    if n_vox == 1:
        lens[:] = 100
    if n_vox >= 255:
        lens[[0, 77, n_vox - 1]] = (100, 100, 7)
        lens[[1, 2, 3]] = (1, 2, 7)
    if c["big"]:
        lens[200] = 5000
    return lens


@functools.lru_cache(maxsize=None)
def segment_inputs(name):
    c = SEGMENT_CASES[name]
    return R.make_segments(c["c"], c["n_vox"], segment_lengths(name), c["n_free"], 300 + list(SEGMENT_CASES).index(name))


# (C, N); 1,050,625 rows = 513 blocks of 8 * 256 rows: one past the 512-block cap, so the grid-stride loop runs
GATE_CASES = {"c1_n0": (1, 0), "c1_n257": (1, 257), "c1_n2049": (1, 2049), "c4_n1": (4, 1), "c4_n255": (4, 255), "c4_n2049": (4, 2049),
              "c8_n0": (8, 0), "c8_n1": (8, 1), "c8_n257": (8, 257), "c8_n2049": (8, 2049), "c4_n1050625": (4, 1050625)}


@functools.lru_cache(maxsize=None)
def gate_inputs(name):
    c, n = GATE_CASES[name]
    return R.make_gate(c, n, 500 + list(GATE_CASES).index(name))


# ------------------------------------------------------------------------------------------------------------------ helpers
def _workspace(L, cin, cout):
    return torch.empty(int(L.mm_point_ws_bytes(cin, cout)), dtype=torch.uint8, device=_dev())


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("name", list(LINEAR_CASES))
def test_linear_forward_and_backward_equal_float64_on_grid_inputs(name):
    c, d = LINEAR_CASES[name], linear_inputs(name)
    L, lib = _abi()
    n, cin, cout = c["n"], c["cin"], c["cout"]
    x = _Rows(d["x"], n, cin, c["ld_x"], c["off_x"])
    w, b = _vec(d["w"], fill=float("nan")), (_vec(d["b"], fill=float("nan")) if c["bias"] else None)
    y = _Rows(None, n, cout, c["ld_y"], 4, fill=SENTINEL)
    lib.check(L.mm_linear_fwd(x.ptr, c["ld_x"], n, cin, cout, w.ptr, b.ptr if b else None, y.ptr, c["ld_y"], lib.stream()), "linear_fwd")
    dy = _Rows(d["dy"], n, cout, c["ld_dy"], 4)
    dx = _Rows(d["dx0"], n, cin, c["ld_dx"], c["off_dx"], fill=SENTINEL) if c["dx"] else None
    dw = _vec(d["dw0"]) if c["dw"] else None
    db = _vec(d["db0"]) if c["dw"] and c["db"] else None
    ws = _workspace(L, cin, cout)
    lib.check(L.mm_linear_bwd(x.ptr, c["ld_x"], dy.ptr, c["ld_dy"], n, cin, cout, w.ptr, dx.ptr if dx else None, c["ld_dx"],
                              c["acc_dx"], dw.ptr if dw else None, db.ptr if db else None, c["acc_w"], ws.data_ptr(), ws.numel(),
                              lib.stream()), "linear_bwd")
    torch.cuda.synchronize()
    rdx, rdw, rdb = R.linear_bwd(d["x"], d["dy"], d["w"])
    bad = []
    if not _same(y.get(), R.linear_fwd(d["x"], d["w"], d["b"] if c["bias"] else None)):
        bad.append("y")
    if dx is not None and not _same(dx.get(), rdx + c["acc_dx"] * d["dx0"]):
        bad.append(f"dx (max |got - want| = {np.abs(dx.get() - rdx - c['acc_dx'] * d['dx0']).max() if n else 0})")
    if dw is not None and not _same(dw.get().reshape(cout, cin), rdw + c["acc_w"] * d["dw0"]):
        bad.append("dw")
    if db is not None and not _same(db.get().reshape(cout), rdb + c["acc_w"] * d["db0"]):
        bad.append("db")
    for nm, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        if t is not None and not t.padding_untouched():
            bad.append(f"padding of {nm}")
    assert not bad, f"{name} {linear_paths(c)}: {', '.join(bad)} differ from the float64 reference"


def test_linear_error_returns_come_before_any_launch():
    """Widths past 150 KiB of LDS and a workspace that is too small are refused, and a refused call has written nothing."""
    L, lib = _abi()
    n = 64
    for cin, cout in ((401, 200), (400, 201)):
        x, dy, w = _Rows(None, n, cin, cin, fill=1.0), _Rows(None, n, cout, cout, fill=1.0), _vec(None, cin * cout, fill=1.0)
        dx, dw, db = _Rows(None, n, cin, cin, fill=SENTINEL), _vec(None, cin * cout), _vec(None, cout)
        ws = _workspace(L, cin, cout)
        with pytest.raises(RuntimeError, match="channels too wide"):
            lib.check(L.mm_linear_bwd(x.ptr, cin, dy.ptr, cout, n, cin, cout, w.ptr, dx.ptr, cin, 0, dw.ptr, db.ptr, 0, ws.data_ptr(),
                                      ws.numel(), lib.stream()), "linear_bwd")
        torch.cuda.synchronize()
        assert dx.padding_untouched() and dw.padding_untouched() and db.padding_untouched()
    for cin, cout in ((16, 6), (5, 7)):
        x, dy, w = _Rows(None, n, cin, cin, fill=1.0), _Rows(None, n, cout, cout, fill=1.0), _vec(None, cin * cout, fill=1.0)
        dx, dw, db = _Rows(None, n, cin, cin, fill=SENTINEL), _vec(None, cin * cout), _vec(None, cout)
        ws = _workspace(L, cin, cout)
        for dxp, dbp, ws_bytes in ((None, db.ptr, 0), (dx.ptr, db.ptr, 0), (dx.ptr, None, (cin * cout + cout) * 8)):
            with pytest.raises(RuntimeError, match="workspace too small"):
                lib.check(L.mm_linear_bwd(x.ptr, cin, dy.ptr, cout, n, cin, cout, w.ptr, dxp, cin, 0, dw.ptr, dbp, 0, ws.data_ptr(),
                                          ws_bytes, lib.stream()), "linear_bwd")
            torch.cuda.synchronize()
            # full-size buffers whose every element is padding: nothing was written, dx included
            assert torch.equal(dx.flat, torch.full_like(dx.flat, SENTINEL)), (cin, cout, "dx written before the error return")
            assert torch.equal(dw.flat, torch.full_like(dw.flat, SENTINEL)) and torch.equal(db.flat, torch.full_like(db.flat, SENTINEL))


def test_linear_function_without_bias_matches_f_linear():
    """Autograd level (scn/ops.py LinearFunction, b = None) on grid inputs: equal to float64 F.linear and its gradients."""
    import torch.nn.functional as F

    from mm2d3d_amd.scn.ops import LinearFunction

    d = linear_inputs("16x6_n257")
    dev = _dev()
    x = torch.from_numpy(d["x"]).float().to(dev).requires_grad_(True)
    w = torch.from_numpy(d["w"]).float().to(dev).requires_grad_(True)
    y = LinearFunction.apply(x, w, None)
    y.backward(torch.from_numpy(d["dy"]).float().to(dev))
    torch.cuda.synchronize()
    x64 = torch.from_numpy(d["x"]).requires_grad_(True)
    w64 = torch.from_numpy(d["w"]).requires_grad_(True)
    y64 = F.linear(x64, w64)
    y64.backward(torch.from_numpy(d["dy"]))
    assert torch.equal(y.detach().cpu().double(), y64.detach())
    assert torch.equal(x.grad.cpu().double(), x64.grad) and torch.equal(w.grad.cpu().double(), w64.grad)


# ------------------------------------------------------------------------------------------------- segment reduce, row gather
def _ulps(got, want32):
    """|got - want| in units of the spacing of fp32 numbers at ``want`` (both fp32-valued)."""
    got32 = got.astype(np.float32)
    assert np.array_equal(got32.astype(np.float64), got)
    diff = np.abs(got32.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
    return float(diff.max()) if diff.size else 0.0


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_segment_sum_is_exact_and_mean_is_one_division(name):
    c, d = SEGMENT_CASES[name], segment_inputs(name)
    L, lib = _abi()
    C, n_vox, n_items = c["c"], c["n_vox"], len(d["p2v"])
    feats = _Rows(d["feats"], n_items, C, c["ld_f"], 4)
    off, items = _ints(d["csr_off"]), _ints(d["csr_items"])
    want = R.segment_sum(np.nan_to_num(d["feats"]), d["csr_off"], d["csr_items"])
    counts = np.diff(d["csr_off"]).astype(np.float32)[:, None]
    for mean in (0, 1):
        out = _Rows(None, n_vox, C, c["ld_o"], 4, fill=SENTINEL)
        lib.check(L.mm_segment_reduce(feats.ptr, c["ld_f"], C, off.data_ptr(), items.data_ptr(), n_vox, mean, out.ptr, c["ld_o"],
                                      lib.stream()), "segment_reduce")
        torch.cuda.synchronize()
        got = out.get()
        assert out.padding_untouched()
        if mean:
            u = _ulps(got, want.astype(np.float32) / counts)
            print(f"{name}: segment mean differs from fp32 sum / count by {u} ulp at most")
            assert u <= 1.0
        else:
            assert _same(got, want)


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_row_gather_copies_the_voxel_row_and_zeroes_points_without_voxel(name):
    c, d = SEGMENT_CASES[name], segment_inputs(name)
    L, lib = _abi()
    C, n_vox, p2v = c["c"], c["n_vox"], d["p2v"]
    vox = _Rows(d["vox"], n_vox, C, c["ld_v"], 4)
    off, p2v_d = _ints(d["csr_off"]), _ints(p2v)
    counts = np.diff(d["csr_off"]).astype(np.float32)
    for div in (0, 1):
        for n in (len(p2v), 0):
            out = _Rows(None, n, C, c["ld_g"], 4, fill=SENTINEL)
            lib.check(L.mm_row_gather(vox.ptr, c["ld_v"], C, p2v_d.data_ptr(), off.data_ptr(), div, n, out.ptr, c["ld_g"], lib.stream()),
                      "row_gather")
            torch.cuda.synchronize()
            got = out.get()
            assert out.padding_untouched()
            assert _same(got[p2v[:n] < 0], np.zeros((int((p2v[:n] < 0).sum()), C)))
            live = p2v[:n] >= 0
            if div:
                want32 = d["vox"].astype(np.float32)[p2v[:n][live]] / counts[p2v[:n][live]][:, None]
                u = _ulps(got[live], want32)
                print(f"{name}: gather / count differs from the fp32 quotient by {u} ulp at most")
                assert u <= 1.0
                assert np.abs(got - R.row_gather(d["vox"], p2v[:n], d["csr_off"], 1)).max(initial=0.0) <= 2.0 ** -22
            else:
                assert _same(got, R.row_gather(d["vox"], p2v[:n], d["csr_off"], 0))


@pytest.mark.parametrize("name", ["c3_v255", "c16_v257", "c17_v1000"])
def test_input_layer_round_trip_mean_forward_gather_backward(name):
    """What scn/ops.py InputMeanFunction does: out = mean(feats) forward, dfeats = gather(dout) / count backward.  Each is within one
    ulp of its reference, so <out, dout> and <feats, dfeats> (equal in exact arithmetic: the adjoint identity) agree to
    2^-23 * (sum |out dout| + sum |feats dfeats|)."""
    c, d = SEGMENT_CASES[name], segment_inputs(name)
    L, lib = _abi()
    C, n_vox, n_items = c["c"], c["n_vox"], len(d["p2v"])
    f64 = np.nan_to_num(d["feats"])
    feats = _Rows(f64, n_items, C, c["ld_f"], 4)
    dout = _Rows(d["vox"], n_vox, C, c["ld_v"], 4)
    off, items, p2v = _ints(d["csr_off"]), _ints(d["csr_items"]), _ints(d["p2v"])
    out = _Rows(None, n_vox, C, c["ld_o"], 4, fill=SENTINEL)
    dfeats = _Rows(None, n_items, C, c["ld_g"], 4, fill=SENTINEL)
    lib.check(L.mm_segment_reduce(feats.ptr, c["ld_f"], C, off.data_ptr(), items.data_ptr(), n_vox, 1, out.ptr, c["ld_o"], lib.stream()),
              "segment_reduce")
    lib.check(L.mm_row_gather(dout.ptr, c["ld_v"], C, p2v.data_ptr(), off.data_ptr(), 1, n_items, dfeats.ptr, c["ld_g"], lib.stream()),
              "row_gather")
    torch.cuda.synchronize()
    o, g = out.get(), dfeats.get()
    assert out.padding_untouched() and dfeats.padding_untouched()
    assert np.abs(o - R.segment_mean(f64, d["csr_off"], d["csr_items"])).max() <= 2.0 ** -23 * np.abs(o).max()
    lhs, rhs = (o * d["vox"]).sum(), (f64 * g).sum()
    # (1.001: the two sums of magnitudes are taken over the computed values, each within 2^-23 of the exact ones)
    assert abs(lhs - rhs) <= 1.001 * 2.0 ** -23 * (np.abs(o * d["vox"]).sum() + np.abs(f64 * g).sum())


# --------------------------------------------------------------------------------------------------------------------- gate
def _check_gate(name, what, errs):
    print(f"{name} {what}: " + "  ".join(f"{k} {v:.2e} (bound {GATE_BOUNDS[k]:.1e})" for k, v in errs.items()))
    over = {k: v for k, v in errs.items() if not v <= GATE_BOUNDS[k]}
    assert not over, f"{name} {what}: {over} exceed {GATE_BOUNDS}"


@pytest.mark.parametrize("name", list(GATE_CASES))
def test_gate_forward_and_backward_against_float64(name):
    (C, n), d = GATE_CASES[name], gate_inputs(name)
    L, lib = _abi()
    x, dy = _Rows(d["x"], n, C, C, 4), _Rows(d["dy"], n, C, C, 4)
    w, b = _vec(d["w"], fill=float("nan")), _vec([d["b"]], fill=float("nan"))
    y, mask = _Rows(None, n, C, C, 4, fill=SENTINEL), _Rows(None, n, 1, 1, 4, fill=SENTINEL)
    lib.check(L.mm_gate_fwd(x.ptr, n, C, w.ptr, b.ptr, y.ptr, mask.ptr, lib.stream()), "gate_fwd")
    ws = _workspace(L, C, 1)
    # 1: dx, dw and db over old contents that must go   2: dx = None, accumulating onto dw0, db0
    dx, dw, db = _Rows(None, n, C, C, 4, fill=SENTINEL), _vec(d["dw0"]), _vec([d["db0"]])
    lib.check(L.mm_gate_bwd(x.ptr, mask.ptr, dy.ptr, n, C, w.ptr, dx.ptr, dw.ptr, db.ptr, 0, ws.data_ptr(), ws.numel(), lib.stream()),
              "gate_bwd")
    dw2, db2 = _vec(d["dw0"]), _vec([d["db0"]])
    lib.check(L.mm_gate_bwd(x.ptr, mask.ptr, dy.ptr, n, C, w.ptr, None, dw2.ptr, db2.ptr, 1, ws.data_ptr(), ws.numel(), lib.stream()),
              "gate_bwd")
    torch.cuda.synchronize()
    for t in (y, mask, dx, dw, db, dw2, db2):
        assert t.padding_untouched()
    m = mask.get()
    assert np.isfinite(m * (1 - m)).all() and (m >= 0).all() and (m <= 1).all()
    _check_gate(name, "overwrite", R.gate_errors(d["x"], d["w"], d["b"], d["dy"], dict(y=y.get(), mask=m, dx=dx.get(), dw=dw.get(), db=db.get())))
    _check_gate(name, "accumulate", R.gate_errors(d["x"], d["w"], d["b"], d["dy"], dict(dw=dw2.get(), db=db2.get()), d["dw0"], d["db0"]))
    # accumulating onto zeros is the overwriting call
    dw3, db3 = _vec(np.zeros(C)), _vec([0.0])
    lib.check(L.mm_gate_bwd(x.ptr, mask.ptr, dy.ptr, n, C, w.ptr, None, dw3.ptr, db3.ptr, 1, ws.data_ptr(), ws.numel(), lib.stream()),
              "gate_bwd")
    torch.cuda.synchronize()
    assert _same(dw3.get(), dw.get()) and _same(db3.get(), db.get())


def test_gate_error_returns_come_before_any_launch():
    L, lib = _abi()
    n = 64
    for C in (0, 9):
        x, dy, w, b = _Rows(None, n, 9, 9, fill=1.0), _Rows(None, n, 9, 9, fill=1.0), _vec(None, 9, fill=1.0), _vec(None, 1, fill=1.0)
        y, mask, dx = _Rows(None, n, 9, 9, fill=SENTINEL), _Rows(None, n, 1, 1, fill=SENTINEL), _Rows(None, n, 9, 9, fill=SENTINEL)
        dw, db, ws = _vec(None, 10), _vec(None, 1), _workspace(L, 9, 1)
        with pytest.raises(RuntimeError, match=r"C must be in \[1,8\]"):
            lib.check(L.mm_gate_fwd(x.ptr, n, C, w.ptr, b.ptr, y.ptr, mask.ptr, lib.stream()), "gate_fwd")
        with pytest.raises(RuntimeError, match=r"C must be in \[1,8\]"):
            lib.check(L.mm_gate_bwd(x.ptr, mask.ptr, dy.ptr, n, C, w.ptr, dx.ptr, dw.ptr, db.ptr, 0, ws.data_ptr(), ws.numel(),
                                    lib.stream()), "gate_bwd")
        torch.cuda.synchronize()
        for t in (y, mask, dx, dw, db):
            assert torch.equal(t.flat, torch.full_like(t.flat, SENTINEL))
    C = 4
    x, dy, w, mask = _Rows(None, n, C, C, fill=1.0), _Rows(None, n, C, C, fill=1.0), _vec(None, C, fill=1.0), _Rows(None, n, 1, 1, fill=0.5)
    dx, dw, db, ws = _Rows(None, n, C, C, fill=SENTINEL), _vec(None, C), _vec(None, 1), _workspace(L, C, 1)
    with pytest.raises(RuntimeError, match="workspace too small"):
        lib.check(L.mm_gate_bwd(x.ptr, mask.ptr, dy.ptr, n, C, w.ptr, dx.ptr, dw.ptr, db.ptr, 0, ws.data_ptr(), 0, lib.stream()), "gate_bwd")
    torch.cuda.synchronize()
    for t in (dx, dw, db):
        assert torch.equal(t.flat, torch.full_like(t.flat, SENTINEL))


def test_gate_function_with_input_gradient_matches_float64_autograd():
    """Autograd level (scn/ops.py GateFunction): the network gates its input features, which need no gradient, so the dx branch runs
    only here."""
    from mm2d3d_amd.scn.ops import GateFunction

    d = gate_inputs("c4_n2049")
    dev = _dev()
    x = torch.from_numpy(d["x"]).to(dev).requires_grad_(True)
    w = torch.from_numpy(d["w"]).reshape(1, -1).to(dev).requires_grad_(True)
    b = torch.tensor([float(d["b"])], device=dev).requires_grad_(True)
    y, mask = GateFunction.apply(x, w, b)
    y.backward(torch.from_numpy(d["dy"]).to(dev))
    torch.cuda.synchronize()
    x64 = torch.from_numpy(d["x"]).double().requires_grad_(True)
    w64 = torch.from_numpy(d["w"]).double().reshape(1, -1).requires_grad_(True)
    b64 = torch.tensor([float(d["b"])], dtype=torch.float64, requires_grad=True)
    m64 = torch.sigmoid(x64 @ w64.t() + b64)
    (x64 * m64).backward(torch.from_numpy(d["dy"]).double())
    assert w.grad.shape == w.shape and b.grad.shape == b.shape and mask.shape == (2049, 1)
    ref = dict(y=(x64 * m64).detach().numpy(), mask=m64.detach().numpy(), dx=x64.grad.numpy(), dw=w64.grad.numpy(), db=b64.grad.numpy())
    got = dict(y=y.detach().cpu().numpy(), mask=mask.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dw=w.grad.cpu().numpy(),
               db=b.grad.cpu().numpy())
    _check_gate("c4_n2049", "GateFunction", R.gate_errors(d["x"], d["w"], d["b"], d["dy"], got, ref=ref))
