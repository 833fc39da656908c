"""The sparse-row batch norm + (leaky) ReLU of csrc/bn.hip, called straight through the C ABI (mm_bn_fwd_train, mm_bn_bwd, mm_bn_fwd_eval
and their _bf16 / _f16 forms) against the float64 reference of tests/_bn_ref.py; the bounds and where they come from are written
there.  Every case runs the training forward, the backward and the eval forward on the same operands, checks that padding and
sentinels survive and that no grid barrier gave up, runs everything a second time and wants the same bits.

Which kernel ran is asked, not assumed: mm_bn_fused_rows reports the rows per thread R of the single-launch kernel (0: the reduce /
finalize / apply kernels), and a case that names a path asserts it.

The backward runs from the REFERENCE's statistics rounded to fp32, so its inputs are exactly those of the fp32 restatement and the
guard band of the inputs (no |y_ref| below 1e-4) decides the sign of y for both; the forward's own statistics are bounded one by
one.

16-bit rows.  A kernel value within the fp32 bound of the reference, cast to nearest, lies within
max(1 ulp, 1/2 ulp + fp32 bound) of it, ulp = the format's spacing at |ref|: the 1-ulp rule wherever fp32 arithmetic can meet it
(where an output cancels to less than 2^11 (fp16) or 2^8 (bf16) times the fp32 bound, half an ulp is less than that bound).  The
share of elements that are not the correctly rounded value of the float64 per-element formula (taken from the same fp32 statistics
and sums the kernel used, so the step is judged alone) is at most 8 x the share of the fp32 restatement; a share counted on n
elements resolves 1 / n, so a restatement without a miss counts as one miss.

The literal rule "within 1 ulp at |ref|" cannot be met by fp32 arithmetic where an output cancels: the fp32 restatement itself, from
exact statistics, is up to 1.03 (bf16 eval), 11.3 (fp16 y, the offset case), 1.60 (fp16 eval) and 1.08 (fp16 dx) ulp away
(test_bn_rows_host.py prints these).  The number of elements beyond 1 ulp is printed per case.

Observed on an MI355X, largest over the cases, as a fraction of the bound: save_mean 0.12, save_invstd 0.57, running_mean 0.76,
running_var 0.87, dweight 0.17, dbias 0.77, y 0.071, eval 0.11, dx 0.079; in units of the outputs' scales y 1.9e-06, eval 2.2e-07,
dx 1.2e-05 (the statistics' error included).  Offset case (x ~ 100 + N(0, 1)): save_invstd at 0.011 (single launch, k = 5) and
0.012 (three kernels, k = 16) of its bound, y at 2.9e-06 of its scale, 0.012 of its bound.  16-bit rows: every output at 0.50 of
max(1 ulp, 1/2 ulp + fp32 bound); beyond 1 ulp: bf16 eval 1 element (1.02 ulp), bf16 dx 39 (1.22 ulp), fp16 eval 14 (1.17 ulp),
fp16 dx 24 (1.77 ulp), fp16 y of the offset case 2,239 of 16,000 (the statistics' error at |y| near the guard band); largest share
of elements not correctly rounded, kernel | restatement: bf16 y 1.4e-04 | 1.4e-04, eval 2.4e-04 | 1.2e-04, dx 8.7e-03 | 8.7e-03;
fp16 y 2.7e-04 | 3.1e-04, eval 2.7e-04 | 9.6e-04, dx 4.8e-03 | 4.8e-03.

Sizes are taken from the chip: ``cus`` is its number of compute units (256 on an MI355X, which CASES of the host test assumes)."""
import functools

import numpy as np
import pytest
import torch

import _bn_ref as B
from _gpu_rows import SENTINEL, Rows as _Rows, abi as _abi, dev as _dev, vec as _vec

pytestmark = pytest.mark.gpu

MI355X_CUS = 256
MM_ERR_ARG, MM_ERR_WORKSPACE = -1, -3
F32 = lambda v: float(np.float32(v))  # noqa: E731  what a float argument of the C ABI holds
NAN = float("nan")


# ------------------------------------------------------------------------------------------- the library's geometry, restated
def _cdiv(a, b):
    return -(-a // b)


def fused_shape(cus, N, Ns, C):
    """(R, R of group 0, R of group 1) of csrc/fused_bn.h fused_shape: used to BUILD cases that sit on an edge; what ran is asked of
    mm_bn_fused_rows."""
    rs = 512 // (C // 4)
    two = 0 < Ns < N
    G = max(min(_cdiv(N, rs * 6), cus), 2 if two else 1)
    if not two:
        R = _cdiv(_cdiv(N, G), rs)
        return R, R, 0
    G0 = min(max(int(G * Ns / N + 0.5), 1), G - 1)
    R0, R1 = _cdiv(_cdiv(Ns, G0), rs), _cdiv(_cdiv(N - Ns, G - G0), rs)
    return max(R0, R1), R0, R1


def vec_width(c):
    """4 when the entry takes its 4-element kernels: C, every pitch and every pointer a multiple of 4 elements."""
    return 4 if c["C"] % 4 == 0 and all(c[k] % 4 == 0 for k in ("ld_x", "ld_y", "ld_dy", "ld_dx", "off")) else 1


def stat_rows_per_thread(c):
    """k of the three-kernel path per statistics group: ceil(rows per block / row slots), with the block count of stat_blocks /
    split_blocks (one block per 32 rows of every slot, at most MAX_PART = 1024, or 512 each for two groups)."""
    CV = c["C"] // vec_width(c)
    rs = 256 // CV
    gs = B.groups(c["N"], c["Ns"])
    ks = []
    for a, e in gs:
        nb = min(max(_cdiv(e - a, rs * 32), 1), 1024 if len(gs) == 1 else 512)
        ks.append(_cdiv(_cdiv(e - a, nb), rs))
    return ks


# --------------------------------------------------------------------------------------------------------------- case table
def _case(t, name, N, C, **kw):
    c = dict(name=name, N=N, Ns=0, C=C, dtype="fp32", opt=3, ld_x=C, ld_y=C, ld_dy=C, ld_dx=C, off=8, x_tight=False, weight=True, bias=True,
             running=True, dweight=True, dbias=True, accumulate=1, leak=(0.333, 0.0)[len(t) % 2], momentum=(0.9, 0.99)[len(t) // 2 % 2],
             eps=1e-4, kind="normal", R=None)
    assert not set(kw) - set(c), set(kw) - set(c)
    c.update(kw)
    if c["opt"] == 0:
        c["R"] = 0
    elif c["R"] is None:
        c["R"] = (1, 8)  # the shape rule aims at six rows per thread
    assert name not in t
    t[name] = c


def _two_group_edge(cus, C, R, thin):
    """(N, Ns) of two uneven groups whose SECOND group decides R.  The workgroups are dealt in proportion to the rows, so group 0 is
    made small enough for one workgroup (four rows per thread) and group 1 fills the other cus - 1 to R rows per thread (thin: R - 1
    and one row more)."""
    rs = 512 // (C // 4)
    Ns, N1 = 3 * rs + 1, (cus - 1) * rs * (R - 1 if thin else R) + (1 if thin else 0)
    assert fused_shape(cus, Ns + N1, Ns, C) == (R, 4, R)
    return Ns + N1, Ns


@functools.lru_cache(maxsize=None)
def cases(cus=MI355X_CUS):
    t = {}
    # ---- a. single-launch path, fp32, option 3
    C, rs = 16, 128
    _case(t, "fused_n1", 1, C)
    _case(t, "fused_n2_ns1", 2, C, Ns=1)  # two groups of one row
    _case(t, "fused_6rs_1", 6 * rs + 1, C)
    for G in (7, 8, 9):  # the two-level barrier changes shape at 8 workgroups
        _case(t, f"fused_G{G}", 6 * rs * G - 5, C)
    _case(t, "fused_ns1", 20 * rs + 3, C, Ns=1)  # a group of one row
    _case(t, "fused_ns_n_1", 20 * rs + 3, C, Ns=20 * rs + 2)
    for nm, Ns in (("0", 0), ("neg", -3), ("n", 6 * rs + 1), ("above", 6 * rs + 6)):
        _case(t, f"fused_one_group_ns_{nm}", 6 * rs + 1, C, Ns=Ns)
    for C in (4, 16, 112, 256, 260, 512):
        _case(t, f"fused_c{C}", 13 * (512 // (C // 4)) + 1, C, Ns=(0, 5 * (512 // (C // 4)) + 2)[C in (112, 260)])
    for (lo, C) in ((8, 16), (13, 112), (20, 512), (36, 16)):  # template (8, 20, 36) and LDS (13) boundaries: the whole chip
        rs = 512 // (C // 4)
        _case(t, f"fused_edge_R{lo}_c{C}", cus * rs * lo, C, R=(lo, lo))
        _case(t, f"fused_edge_R{lo + 1}_c{C}", cus * rs * lo + 1, C, R=(lo + 1, lo + 1) if lo < 36 else 0)
    for thin in (False, True):
        R = 9 if thin else 8
        N, Ns = _two_group_edge(cus, 16, R, thin)
        _case(t, f"fused_edge_R{R}_two_groups", N, 16, Ns=Ns, R=(R, R))
    # x: a channel slice that ends with its allocation's last element; y, dy, dx each with a pitch of their own
    _case(t, "fused_pitched", 13 * 128 + 1, 16, ld_x=24, ld_y=20, ld_dy=28, ld_dx=32, x_tight=True)
    _case(t, "fused_pitched_two_groups", 13 * 128 + 1, 16, Ns=700, ld_x=24, ld_y=20, ld_dy=28, ld_dx=32, x_tight=True)
    # ---- b. three-kernel path, option 0; the 16-bit types run the names in REDUCED
    C, rs = 16, 64  # CV = 4: 64 row slots per block
    _case(t, "k3_stat_1block", 32 * rs, C, opt=0)
    _case(t, "k3_stat_2blocks", 32 * rs + 1, C, opt=0)
    for j in range(1, 6):  # rows per slot 1..5: the 4-row and 2-row unrolls and their remainders
        _case(t, f"k3_rows_per_slot_{j}", j * rs - 7, C, opt=0)
    _case(t, "k3_max_part", 40000, 255, opt=0)  # 1,250 blocks wanted, 1,024 given
    _case(t, "k3_max_part_two_groups", 40000, 255, Ns=20000, opt=0)  # 625 wanted, 512 given, each
    _case(t, "k3_apply_1block", 8 * rs, C, opt=0)
    _case(t, "k3_apply_2blocks", 8 * rs + 1, C, opt=0)
    _case(t, "k3_apply_group_inside_block", 1500, C, Ns=700, opt=0)
    _case(t, "k3_c7", 1000, 7, opt=0)
    _case(t, "k3_c255", 300, 255, opt=0)
    _case(t, "k3_c256_odd_pitch", 300, 256, opt=0, ld_x=257, ld_y=259, ld_dy=261, ld_dx=257)
    _case(t, "k3_c516", 300, 516, opt=0)
    _case(t, "k3_c1024", 100, 1024, opt=0)
    _case(t, "k3_c16_unaligned", 1000, 16, opt=0, off=9)  # a pointer one element off: the scalar kernels
    # ---- c. operands, both paths
    for p, opt, N in (("fused", 3, 13 * 128 + 1), ("k3", 0, 1000)):
        kw = dict(opt=opt)
        _case(t, f"{p}_no_weight", N, 16, weight=False, **kw)
        _case(t, f"{p}_no_bias", N, 16, bias=False, Ns=400, **kw)
        _case(t, f"{p}_no_weight_no_bias", N, 16, weight=False, bias=False, **kw)
        _case(t, f"{p}_no_running", N, 16, running=False, Ns=400, **kw)
        _case(t, f"{p}_no_dweight", N, 16, dweight=False, **kw)
        _case(t, f"{p}_no_dbias", N, 16, dbias=False, Ns=400, **kw)
        _case(t, f"{p}_no_dweight_no_dbias", N, 16, dweight=False, dbias=False, **kw)
        _case(t, f"{p}_overwrite", N, 16, accumulate=0, **kw)
        _case(t, f"{p}_overwrite_two_groups", N, 16, accumulate=0, Ns=400, **kw)
        for leak in (0.0, 0.333):
            for mom in (0.9, 0.99):
                _case(t, f"{p}_leak{leak}_mom{mom}", N, 16, leak=leak, momentum=mom, Ns=(0, 400)[mom == 0.9], **kw)
        _case(t, f"{p}_exact_zero", 1024, 16, kind="grid", leak=0.333, **kw)  # y == 0 where x == 0: the backward passes leak * dy
        _case(t, f"{p}_grid", 512 + 256, 16, Ns=512, kind="grid", leak=0.0, **kw)
        _case(t, f"{p}_group_of_one_row", 65, 16, Ns=64, **kw)
        _case(t, f"{p}_offset", N, 16, kind="offset", **kw)
    # the 16-bit entries
    for name in REDUCED:
        for dt in ("bf16", "fp16"):
            c = dict(t[name], dtype=dt)
            del c["name"]
            N, C = c.pop("N"), c.pop("C")
            _case(t, f"{name}_{dt}", N, C, **c)
    return t


REDUCED = ("k3_stat_1block", "k3_stat_2blocks", "k3_max_part", "k3_apply_2blocks", "k3_apply_group_inside_block", "k3_c7", "k3_c1024",
           "k3_c16_unaligned", "k3_no_weight_no_bias", "k3_no_running", "k3_overwrite_two_groups", "k3_leak0.333_mom0.9",
           "k3_group_of_one_row", "k3_offset")
CASE_NAMES = list(cases())  # the names do not depend on the chip; the sizes of the fused_edge cases do


def case_inputs(c):
    return B.make_inputs(c["name"], c["N"], c["Ns"], c["C"], c["dtype"], c["kind"], c["weight"], c["bias"], F32(c["eps"]), F32(c["leak"]))


def case_reference(c, d):
    return B.bn_ref(d["x"], d["dy"], c["N"], c["Ns"], d["weight"], d["bias"], d["rm0"] if c["running"] else None,
                    d["rv0"] if c["running"] else None, F32(c["eps"]), F32(c["momentum"]), F32(c["leak"]), c["accumulate"], d["dw0"], d["db0"])


# ------------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _handle(opt):
    _, lib = _abi()
    return lib.Handle(_dev(), bn3d_fused=opt)


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


def _entries(L, dtype):
    sfx = {"fp32": "", "bf16": "_bf16", "fp16": "_f16"}[dtype]
    return getattr(L, "mm_bn_fwd_train" + sfx), getattr(L, "mm_bn_bwd" + sfx), getattr(L, "mm_bn_fwd_eval" + sfx)


def _workspace(L, C):
    return torch.zeros(int(L.mm_bn_ws_bytes(C)), dtype=torch.uint8, device=_dev())


def _p(t):
    return None if t is None else t.ptr


def _run(c, d, ref):
    """Training forward, backward (from the reference's statistics in fp32) and eval forward (from the initial running buffers) of
    one case.  Returns the operands that were written, and the kernel's per-group sums read back from the workspace."""
    L, lib = _abi()
    h = _handle(c["opt"])
    fwd, bwd, evl = _entries(L, c["dtype"])
    N, Ns, C, dt, G = c["N"], c["Ns"], c["C"], c["dtype"], len(B.groups(c["N"], c["Ns"]))
    eps, mom, leak = F32(c["eps"]), F32(c["momentum"]), F32(c["leak"])
    x = _Rows(d["x"], N, C, c["ld_x"], c["off"], dtype=dt, tight=c["x_tight"])
    dy = _Rows(d["dy"], N, C, c["ld_dy"], c["off"], dtype=dt)
    w = _vec(d["weight"], fill=NAN) if c["weight"] else None
    b = _vec(d["bias"], fill=NAN) if c["bias"] else None
    o = dict(y=_Rows(None, N, C, c["ld_y"], c["off"], fill=SENTINEL, dtype=dt), y_eval=_Rows(None, N, C, c["ld_y"], c["off"], fill=SENTINEL, dtype=dt),
             dx=_Rows(None, N, C, c["ld_dx"], c["off"], fill=SENTINEL, dtype=dt), save_mean=_vec(None, G * C), save_invstd=_vec(None, G * C),
             running_mean=_vec(d["rm0"]) if c["running"] else None, running_var=_vec(d["rv0"]) if c["running"] else None,
             dweight=_vec(d["dw0"]) if c["dweight"] else None, dbias=_vec(d["db0"]) if c["dbias"] else None)
    ws = _workspace(L, C)
    s = lib.stream()
    lib.check(fwd(h.h, x.ptr, c["ld_x"], N, Ns, C, _p(w), _p(b), _p(o["running_mean"]), _p(o["running_var"]), eps, mom, leak, o["y"].ptr,
                  c["ld_y"], o["save_mean"].ptr, o["save_invstd"].ptr, ws.data_ptr(), ws.numel(), s), "bn_fwd_train")
    sm, si = _vec(ref["save_mean"], fill=NAN), _vec(ref["save_invstd"], fill=NAN)
    lib.check(bwd(h.h, x.ptr, c["ld_x"], dy.ptr, c["ld_dy"], N, Ns, C, _p(w), _p(b), sm.ptr, si.ptr, leak, o["dx"].ptr, c["ld_dx"],
                  _p(o["dweight"]), _p(o["dbias"]), c["accumulate"], ws.data_ptr(), ws.numel(), s), "bn_bwd")
    rm, rv = _vec(d["rm0"], fill=NAN), _vec(d["rv0"], fill=NAN)
    lib.check(evl(x.ptr, c["ld_x"], N, C, _p(w), _p(b), rm.ptr, rv.ptr, eps, leak, o["y_eval"].ptr, c["ld_y"], s), "bn_fwd_eval")
    torch.cuda.synchronize()
    need = -(-1024 * 2 * C * 8 // 256) * 256  # the per-group sums [G][2][C] fp32 follow the fp64 partials in the workspace
    sums = ws[need: need + G * 2 * C * 4].view(torch.float32).cpu().double().numpy().reshape(G, 2, C)
    return o, sums, h


def _ratio(err, bound):
    """max err / bound (an element with bound 0 must have no error)."""
    return B.worst(err, bound)


def _check16(name, what, got, ref64, fp32_bound, exact64, restated32, dt, report, bad):
    """The two rules of a 16-bit output (see the module's docstring)."""
    ulp = B.ulp16(ref64, dt)
    r = _ratio(got - ref64, np.maximum(ulp, 0.5 * ulp + fp32_bound))
    want = B.round16(exact64, dt)
    miss, miss_restated = int((got != want).sum()), int((B.cast32(restated32, dt) != want).sum())
    report[what] = dict(ratio=r, in_ulp=float((np.abs(got - ref64) / ulp).max()), beyond_1ulp=int((np.abs(got - ref64) > ulp).sum()),
                        share=miss / got.size, share_restated=miss_restated / got.size)
    if not r <= 1.0:
        bad.append(f"{what}: {r:.3f} x max(1 ulp, 1/2 ulp + fp32 bound)")
    if not miss <= 8 * max(miss_restated, 1):
        bad.append(f"{what}: {miss} of {got.size} elements are not correctly rounded, the restatement misses {miss_restated}")


# -------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_backward_and_eval_against_float64(name):
    c = cases(_cus())[name]
    L, lib = _abi()
    N, Ns, C, dt = c["N"], c["Ns"], c["C"], c["dtype"]
    d = case_inputs(c)
    ref = case_reference(c, d)
    eps, mom, leak = F32(c["eps"]), F32(c["momentum"]), F32(c["leak"])
    rmax = B.RESTATE_MAX[dt]
    o, sums, h = _run(c, d, ref)
    bad, report = [], {}
    # which kernel ran
    Rf, Rb = int(L.mm_bn_fused_rows(h.h, N, Ns, C, 0)), int(L.mm_bn_fused_rows(h.h, N, Ns, C, 1))
    if c["R"] == 0:
        assert Rf == 0 and Rb == 0, f"{name}: the three-kernel path is named, mm_bn_fused_rows says R = {Rf}, {Rb}"
    else:
        assert dt == "fp32" and vec_width(c) == 4
        assert c["R"][0] <= Rf <= c["R"][1] and Rb == Rf, f"{name}: single-launch kernel with R in {c['R']} is named, R = {Rf}, {Rb}"
    k = [Rf] * len(ref["groups"]) if Rf else stat_rows_per_thread(c)
    # nothing but the rows was written, no barrier gave up
    for key, t in o.items():
        if t is not None and not t.padding_untouched():
            bad.append(f"padding of {key}")
    assert h.fault_poll() == 0, "a grid barrier ran out of time"
    # statistics
    sb = B.stat_bounds(ref, k, eps, mom)
    gb = B.grad_bounds(ref, k, c["accumulate"])
    got = {key: t.get().reshape(np.shape(ref[key])) for key, t in o.items() if t is not None and key in ref and key not in ("y", "dx")}
    for key in ("save_mean", "save_invstd", "running_mean", "running_var"):
        if key in got:
            report[key] = _ratio(got[key] - ref[key], sb[key])
    for key in ("dweight", "dbias"):
        if key in got:
            report[key] = _ratio(got[key] - ref[key], gb[key])
    report["S1"], report["S2"] = _ratio(sums[:, 0] - ref["S1"], gb["S1"]), _ratio(sums[:, 1] - ref["S2"], gb["S2"])
    if c["kind"] == "grid":  # exact sums: the statistics that are sums equal the float64 reference rounded to fp32
        if not np.array_equal(got["save_mean"], ref["save_mean"].astype(np.float32).astype(np.float64)):
            bad.append("save_mean is not the exact mean")
        if leak == 0.0:
            if not np.array_equal(sums[:, 0], ref["S1"]):
                bad.append("sum g is not exact")
            if "dbias" in got and not np.array_equal(got["dbias"], ref["dbias"]):
                bad.append("dbias is not exact")
    # y, eval, dx
    y, ye, dx = o["y"].get(), o["y_eval"].get(), o["dx"].get()
    yb = B.y_bound(d["x"], ref, N, Ns, d["weight"], d["bias"], sb, rmax["y"])
    ye_ref = B.bn_eval_ref(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], eps, leak)
    ye_scale = B.scale_eval(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], eps)
    yeb = 8 * rmax["eval"] * ye_scale
    dxb = B.dx_bound(d["x"], ref, N, Ns, d["weight"], gb, rmax["dx"])
    if dt == "fp32":
        report["y"], report["y_eval"], report["dx"] = _ratio(y - ref["y"], yb), _ratio(ye - ye_ref, yeb), _ratio(dx - ref["dx"], dxb)
        report["y_in_scale"] = B.worst(y - ref["y"], B.scale_y(d["x"], ref, N, Ns, d["weight"], d["bias"]))
        report["dx_in_scale"] = B.worst(dx - ref["dx"], B.scale_dx(d["x"], ref, N, Ns, d["weight"]))
        report["y_eval_in_scale"] = B.worst(ye - ye_ref, ye_scale)
    else:
        ksm, ksi = got["save_mean"], got["save_invstd"]
        _check16(name, "y", y, ref["y"], yb, B.fwd_given(d["x"], N, Ns, ksm, ksi, d["weight"], d["bias"], leak),
                 B.fwd_fp32(d["x"], N, Ns, ksm, ksi, d["weight"], d["bias"], leak), dt, report, bad)
        _check16(name, "y_eval", ye, ye_ref, yeb, ye_ref, B.eval_fp32(d["x"], d["weight"], d["bias"], d["rm0"], d["rv0"], eps, leak), dt, report, bad)
        m32, i32 = (ref[key].astype(np.float32).astype(np.float64) for key in ("save_mean", "save_invstd"))
        _check16(name, "dx", dx, ref["dx"], dxb, B.bwd_given(d["x"], d["dy"], N, Ns, m32, i32, d["weight"], d["bias"], leak, sums[:, 0], sums[:, 1]),
                 B.bwd_fp32(d["x"], d["dy"], N, Ns, m32, i32, d["weight"], d["bias"], leak, sums[:, 0], sums[:, 1]), dt, report, bad)
    if c["kind"] == "grid" and leak != 0.0:  # the exact-zero case: y is exactly 0 where x == 0, and the gradient there is leak * dy
        zero = d["x"] == 0
        assert zero.any() and (ref["y"][zero] == 0).all() and (ref["g"][zero] == leak * d["dy"][zero]).all()
        if not (y[zero] == 0).all():
            bad.append("y != 0 where x equals the exact mean")
    print(f"{name}: R {Rf} k {k} observed / bound: " + "  ".join(
        f"{key} {v:.3g}" if isinstance(v, float) else f"{key} {v}" for key, v in report.items()))
    for key, v in report.items():
        if isinstance(v, float) and not key.endswith("in_scale") and not v <= 1.0:
            bad.append(f"{key}: {v:.3f} x its bound")
    # the same call again gives the same bits
    o2, sums2, _ = _run(c, d, ref)
    for key, t in o.items():
        if t is not None and not np.array_equal(t.bits(), o2[key].bits()):
            bad.append(f"{key} differs between two runs")
    assert h.fault_poll() == 0
    assert not bad, f"{name} (R = {Rf}, k = {k}): " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusal_operands(dt, N, C, ld):
    n = max(N, 1)
    return dict(x=_Rows(None, n, C, ld, 8, fill=1.0, dtype=dt), dy=_Rows(None, n, C, ld, 8, fill=1.0, dtype=dt),
                y=_Rows(None, n, C, ld, 8, fill=SENTINEL, dtype=dt), dx=_Rows(None, n, C, ld, 8, fill=SENTINEL, dtype=dt),
                w=_vec(None, C, fill=1.0), b=_vec(None, C, fill=1.0), rm=_vec(None, C), rv=_vec(None, C), sm=_vec(None, 2 * C), si=_vec(None, 2 * C),
                sm_in=_vec(None, 2 * C, fill=1.0), dw=_vec(None, C), db=_vec(None, C))


def _call_all(dt, t, h, N, C, ld, ws, ws_bytes, accumulate=1, off=0, ld_out=None):
    """The three entries of a row type on operands ``t``; returns their return codes (forward, backward, eval)."""
    L, lib = _abi()
    fwd, bwd, evl = _entries(L, dt)
    es = 4 if dt == "fp32" else 2
    ld_out = ld if ld_out is None else ld_out
    px, pdy, py, pdx = (t[k].ptr + off * es for k in ("x", "dy", "y", "dx"))
    s = lib.stream()
    rc = (fwd(h, px, ld, N, 0, C, t["w"].ptr, t["b"].ptr, t["rm"].ptr, t["rv"].ptr, F32(1e-4), F32(0.9), 0.0, py, ld_out, t["sm"].ptr, t["si"].ptr,
              ws.data_ptr(), ws_bytes, s),
          bwd(h, px, ld, pdy, ld, N, 0, C, t["w"].ptr, t["b"].ptr, t["sm_in"].ptr, t["sm_in"].ptr, 0.0, pdx, ld_out, t["dw"].ptr, t["db"].ptr,
              accumulate, ws.data_ptr(), ws_bytes, s),
          evl(px, ld, N, C, t["w"].ptr, t["b"].ptr, t["sm_in"].ptr, t["sm_in"].ptr, F32(1e-4), 0.0, py, ld_out, s))
    torch.cuda.synchronize()
    return rc


def _nothing_written(t, keys=("y", "dx", "rm", "rv", "sm", "si", "dw", "db")):
    return [k for k in keys if not t[k].untouched()]


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_refusals_come_before_any_launch(dt):
    """Every refused call returns its error and has written nothing: outputs, statistics, gradients and both running buffers keep
    their fill."""
    L, lib = _abi()
    h = _handle(3).h
    ws = _workspace(L, 1028)
    full = ws.numel()
    #        what                   N    C     ld    buffers as for (C, ld)   extra
    table = (("C = 0",              64,  0,    16,   (16, 16),                {}),
             ("C = 1028",           64,  1028, 1028, (1028, 1028),            {}),
             ("C = 257 unaligned",  64,  257,  257,  (257, 257),              {}),
             ("C = 260, pointer off by one", 64, 260, 260, (260, 264),        dict(off=1)),
             ("pitch < C",          64,  16,   12,   (16, 16),                {}),
             ("output pitch < C",   64,  16,   16,   (16, 16),                dict(ld_out=15)),
             ("N = -1",             -1,  16,   16,   (16, 16),                {}))
    for what, N, C, ld, (bc, bld), extra in table:
        t = _refusal_operands(dt, 64, bc, bld)
        rc = _call_all(dt, t, h, N, C, ld, ws, full, **extra)
        assert rc == (MM_ERR_ARG,) * 3, (what, rc, L.mm_last_error())
        assert not _nothing_written(t), (what, _nothing_written(t))
    # a workspace one byte short (the eval entry takes none)
    t = _refusal_operands(dt, 64, 16, 16)
    rc = _call_all(dt, t, h, 64, 16, 16, ws, int(L.mm_bn_ws_bytes(16)) - 1)
    assert rc[:2] == (MM_ERR_WORKSPACE,) * 2 and rc[2] == 0, rc
    assert not _nothing_written(t, ("dx", "rm", "rv", "sm", "si", "dw", "db"))
    # what is no handle
    t = _refusal_operands(dt, 64, 16, 16)
    rc = _call_all(dt, t, None, 64, 16, 16, ws, full)
    assert rc[:2] == (MM_ERR_ARG,) * 2 and rc[2] == 0, rc
    assert not _nothing_written(t, ("dx", "rm", "rv", "sm", "si", "dw", "db"))
    assert int(L.mm_bn_fused_rows(None, 64, 0, 16, 0)) == MM_ERR_ARG


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("opt", [3, 0])
def test_no_rows_is_no_work(dt, opt):
    """N == 0: MM_OK; the forward calls write nothing (the running buffers keep their values); the backward zeroes dweight / dbias
    when it does not accumulate and leaves them alone when it does."""
    L, lib = _abi()
    h = _handle(opt).h
    ws = _workspace(L, 16)
    t = _refusal_operands(dt, 0, 16, 16)
    assert _call_all(dt, t, h, 0, 16, 16, ws, ws.numel(), accumulate=1) == (0, 0, 0)
    assert not _nothing_written(t), _nothing_written(t)
    assert _call_all(dt, t, h, 0, 16, 16, ws, ws.numel(), accumulate=0) == (0, 0, 0)
    assert not _nothing_written(t, ("y", "dx", "rm", "rv", "sm", "si"))
    for k in ("dw", "db"):
        assert t[k].padding_untouched() and np.array_equal(t[k].get32(), np.zeros((1, 16), np.float32)), k
    assert int(L.mm_bn_fused_rows(h, 0, 0, 16, 0)) == 0


def test_fused_rows_query_follows_the_handles_option_and_touches_nothing():
    """mm_bn_fused_rows answers from the handle's option bits and the shape alone."""
    L, lib = _abi()
    cus = _cus()
    h = lib.Handle(_dev(), bn3d_fused=3)
    N = 13 * 128 + 1
    want = fused_shape(cus, N, 0, 16)[0]
    assert int(L.mm_bn_fused_rows(h.h, N, 0, 16, 0)) == want == int(L.mm_bn_fused_rows(h.h, N, 0, 16, 1))
    for mask, fb in ((0, (0, 0)), (1, (want, 0)), (2, (0, want)), (3, (want, want))):
        h.set(lib.OPT_BN3D_FUSED, mask)
        assert (int(L.mm_bn_fused_rows(h.h, N, 0, 16, 0)), int(L.mm_bn_fused_rows(h.h, N, 0, 16, 1))) == fb, mask
    for C in (0, 2, 6, 516, 1024):  # no 16-byte pieces, or beyond the layout of the single-launch kernels
        assert int(L.mm_bn_fused_rows(h.h, N, 0, C, 0)) == 0, C
    assert int(L.mm_bn_fused_rows(h.h, cus * 128 * 36, 0, 16, 0)) == 36 and int(L.mm_bn_fused_rows(h.h, cus * 128 * 36 + 1, 0, 16, 0)) == 0
    assert int(L.mm_bn_fused_rows(h.h, -1, 0, 16, 0)) == 0
    assert h.fault_poll() == 0
    h.close()
