"""The two cross-entropy pairs with row weights on their tail rows (csrc/loss.hip: mm_ce2_fwd_w / mm_ce2_bwd_w, mm_ce2s_fwd_w /
mm_ce2s_bwd_w), called straight through the C ABI, against the float64 numpy references of tests/_agree_ref.py (built on
tests/_loss_ref.py), and losses.cross_entropy_pair(row_weight_tail=) / cross_entropy_soft_pair(row_weight=) on top of them.

Tolerances are those of test_gpu_ce_pair.py / test_gpu_ce_soft.py: a loss within 1e-5 * max(1, |ref|); a gradient row times its
segment's denominator (the weight sum; K, the kept rows, for the soft tail) within 1e-5 absolute.  The soft reference gates in
float64; every soft case asserts that no confidence lies within 1e-6 of its threshold, so the kernel's float32 gate keeps exactly
the reference's rows.

Row weights: uniform in [0, 1], seeded, with exact zeros and exact ones among them.  Three identities are checked bit for bit:
row_w == NULL through the _w entry points is the parent entry point; row_w all 1.0f is too (x * 1.0f is exact); and the _w soft
pair with a non-NULL thr_cls is mm_ce2s_*_cls, with NULL mm_ce2s_*.

Sizes: the hard pair's forward takes 1024 rows per workgroup of at most 1024 (1049601 rows: the grid-stride loop runs); the soft
pair's tiles are 64 rows for at most 2048 workgroups (131201 rows: 2051 tiles)."""
import functools

import numpy as np
import pytest
import torch

import _agree_ref as R
from _gpu_rows import SENTINEL, Rows, abi as _abi, dev as _dev, ints, vec
from _loss_ref import ce

pytestmark = pytest.mark.gpu

W6 = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]  # config.yaml class weights
G = (0.75, 1.5)  # the two upstream gradients
PER_CLASS = "per_class"

# name: (N, P, C, ld, ld_d, tail labels)
HARD = {
    "777_300_6": (777, 300, 6, 6, 6, "mix"),
    "129_0_6": (129, 0, 6, 6, 6, "mix"),  # no head rows
    "128_128_6": (128, 128, 6, 6, 6, "mix"),  # no tail rows
    "257_100_32": (257, 100, 32, 32, 32, "mix"),
    "1_0_2": (1, 0, 2, 2, 2, "all"),
    "pitched": (777, 300, 6, 9, 8, "mix"),
    "all_ignored_tail": (300, 100, 6, 6, 6, "ignored"),
    "capped_c2": (1048576 + 1025, 500000, 2, 2, 2, "mix"),
}
# name: (N, P, C, T, thr, ensemble, ld (of all three inputs), ld_d)
SOFT = {
    "777_300_6_thr": (777, 300, 6, 2.0, 0.6, True, 6, 6),
    "777_300_6_own": (777, 300, 6, 1.0, None, False, 6, 6),
    "777_300_6_cls": (777, 300, 6, 2.0, PER_CLASS, True, 6, 6),
    "777_300_6_cls_own": (777, 300, 6, 0.5, PER_CLASS, False, 6, 6),
    "129_0_6": (129, 0, 6, 2.0, 0.6, True, 6, 6),
    "128_128_6": (128, 128, 6, 2.0, 0.6, True, 6, 6),
    "129_1_32": (129, 1, 32, 1.0, PER_CLASS, True, 32, 32),
    "pitched": (777, 300, 6, 2.0, 0.6, True, 9, 8),
    "capped": (131201, 60000, 6, 1.0, 0.6, True, 6, 6),
}


def _class_weights(C):
    return np.asarray([W6[c % 6] for c in range(C)], np.float32)


def _close(got, ref):
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


def _f32(t):
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- the hard pair
@functools.lru_cache(maxsize=None)
def _hard(name):
    """Seeded inputs and the float64 reference of a case: made once, shared, never modified."""
    N, P, C, ld, ld_d, kind = HARD[name]
    rng = np.random.default_rng(3000 + list(HARD).index(name))
    x = (3 * rng.standard_normal((N, C))).astype(np.float32)
    y0, y1 = rng.integers(0, C, P), rng.integers(0, C, N - P)
    y0[rng.random(P) < 0.05] = -100
    if kind == "mix":
        y1[rng.random(N - P) < 0.3] = -100
        y1[5::97] = C + 3  # outside [0, C): skipped like ignore_index
    elif kind == "ignored":
        y1[:] = -100
    cw, rw = _class_weights(C), R.make_row_weights(N - P, 17 + N)
    head = ce(x[:P], y0, cw, -100, G[0])
    tail = R.hard_tail(x[P:], y1, None, rw, grad_out=G[1])  # the pseudo-label tail carries no class weights ...
    tail_cw = R.hard_tail(x[P:], y1, cw, rw, grad_out=G[1])  # ... but the entry point takes them
    return dict(name=name, N=N, P=P, C=C, ld=ld, ld_d=ld_d, x=x, y0=y0, y1=y1, cw=cw, rw=rw, head=head, tail=tail, tail_cw=tail_cw)


def _run_hard(L, lib, c, row_w, entry, tail_weights=False):
    """(stats [4], gradient [N, C]) of one forward and backward through ``entry`` ("w": mm_ce2_*_w, "parent": mm_ce2_*)."""
    N, P, C = c["N"], c["P"], c["C"]
    x, dl = Rows(c["x"], N, C, c["ld"]), Rows(None, N, C, c["ld_d"], fill=SENTINEL)
    y0, y1, cw, rw, g = ints(c["y0"], np.int64), ints(c["y1"], np.int64), _f32(c["cw"]), _f32(row_w), _f32(G)
    w1 = cw if tail_weights else None
    stats = vec(None, 4)
    ws = torch.empty(int(L.mm_ce2_ws_bytes()), dtype=torch.uint8, device=_dev())
    s = lib.stream()
    if entry == "w":
        lib.check(L.mm_ce2_fwd_w(x.ptr, c["ld"], N, P, C, _ptr(y0), _ptr(cw), _ptr(y1), _ptr(w1), -100, 2, _ptr(rw), stats.ptr, ws.data_ptr(),
                                 ws.numel(), s), "ce2_fwd_w")
        lib.check(L.mm_ce2_bwd_w(x.ptr, c["ld"], N, P, C, _ptr(y0), _ptr(cw), _ptr(y1), _ptr(w1), -100, _ptr(rw), stats.ptr, _ptr(g), dl.ptr,
                                 c["ld_d"], s), "ce2_bwd_w")
    else:
        assert row_w is None
        lib.check(L.mm_ce2_fwd(x.ptr, c["ld"], N, P, C, _ptr(y0), _ptr(cw), _ptr(y1), _ptr(w1), -100, 2, stats.ptr, ws.data_ptr(), ws.numel(),
                               s), "ce2_fwd")
        lib.check(L.mm_ce2_bwd(x.ptr, c["ld"], N, P, C, _ptr(y0), _ptr(cw), _ptr(y1), _ptr(w1), -100, stats.ptr, _ptr(g), dl.ptr, c["ld_d"], s),
                  "ce2_bwd")
    torch.cuda.synchronize()
    assert stats.padding_untouched() and dl.padding_untouched(), c["name"]  # every row written once, nothing else
    grad = dl.get32()
    assert not (grad == np.float32(SENTINEL)).any()
    return stats.get32().reshape(-1), grad


def _check_segment(what, loss, ref_loss, grad, ref_grad, denom):
    err = float(np.abs(grad.astype(np.float64) * denom - ref_grad * denom).max(initial=0.0))
    print(f"{what}: loss {loss:.7f} ref {ref_loss:.7f}; max |denominator * (dgrad - ref)| {err:.2e}")
    assert (np.isnan(loss) and np.isnan(ref_loss)) or _close(float(loss), ref_loss), what
    assert err <= 1e-5, what


@pytest.mark.parametrize("tail_weights", [False, True], ids=["plain_tail", "class_weighted_tail"])
@pytest.mark.parametrize("name", list(HARD))
def test_hard_pair_matches_float64(name, tail_weights):
    L, lib = _abi()
    c = _hard(name)
    P, tail = c["P"], c["tail_cw" if tail_weights else "tail"]
    stats, grad = _run_hard(L, lib, c, c["rw"], "w", tail_weights)
    if P:
        _check_segment(f"{name} head", stats[0], c["head"]["loss"], grad[:P], c["head"]["dlogits"], c["head"]["sum_w"])
        assert _close(float(stats[1]), c["head"]["sum_w"])
    _check_segment(f"{name} tail", stats[2], tail["loss"], grad[P:], tail["dlogits"], max(tail["sum_w"], 1.0))
    assert _close(float(stats[3]), tail["sum_w"])  # the class weights of the counted rows: the row weights are not in it
    live = R.counted(c["y1"], c["C"], -100)
    assert (grad[P:][~live] == 0).all() and (grad[P:][c["rw"] == 0] == 0).all()  # a row of weight 0 is written, as zeros
    if name == "all_ignored_tail":
        assert stats[2] == 0.0 and stats[3] == 0.0 and (grad[P:] == 0).all()  # zero_if_empty, as in the parent
    if c["N"] == P:
        assert stats[2] == 0.0 and stats[3] == 0.0


@pytest.mark.parametrize("name", ["777_300_6", "129_0_6", "128_128_6", "pitched", "all_ignored_tail", "capped_c2"])
def test_hard_pair_without_weights_and_with_unit_weights_is_the_parent_bit_for_bit(name):
    L, lib = _abi()
    c = _hard(name)
    for tw in (False, True):
        want = _run_hard(L, lib, c, None, "parent", tw)
        for what, rw in (("row_w == NULL", None), ("row_w all 1.0f", np.ones(c["N"] - c["P"], np.float32))):
            got = _run_hard(L, lib, c, rw, "w", tw)
            assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (name, what, "stats")
            assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), (name, what, "gradient")
    if c["N"] > c["P"] and name != "all_ignored_tail":
        assert not np.array_equal(_run_hard(L, lib, c, c["rw"], "w", True)[1], want[1])  # and real weights do change the rows


# ---------------------------------------------------------------------------------------------- the soft pair
@functools.lru_cache(maxsize=None)
def _soft(name):
    N, P, C, T, thr, ens, ld, ld_d = SOFT[name]
    rng = np.random.default_rng(4000 + list(SOFT).index(name))
    x = (3 * rng.standard_normal((N, C))).astype(np.float32)
    ta = (3 * rng.standard_normal((N - P, C))).astype(np.float32)
    tb = (3 * rng.standard_normal((N - P, C))).astype(np.float32) if ens else None
    if N - P > 70:
        ta[[3, 64, 70]] = np.nan  # teacher rows that are not finite: never kept
    y0 = rng.integers(0, C, P)
    y0[rng.random(P) < 0.05] = -100
    thr = np.linspace(0.35, 0.8, C).astype(np.float32) if thr == PER_CLASS else thr
    cw, rw = _class_weights(C), R.make_row_weights(N - P, 23 + N)
    head = ce(x[:P], y0, cw, -100, G[0])
    tail = R.soft_tail(x[P:], ta, tb, T, thr, rw, grad_out=G[1])
    return dict(name=name, N=N, P=P, C=C, T=T, thr=thr, ld=ld, ld_d=ld_d, x=x, ta=ta, tb=tb, y0=y0, cw=cw, rw=rw, head=head, tail=tail)


def _run_soft(L, lib, c, row_w, entry):
    """(stats [4], kept, gradient) through ``entry``: "w" (mm_ce2s_*_w), "parent" (mm_ce2s_*) or "cls" (mm_ce2s_*_cls)."""
    N, P, C, T, ld = c["N"], c["P"], c["C"], c["T"], c["ld"]
    x, dl = Rows(c["x"], N, C, ld), Rows(None, N, C, c["ld_d"], fill=SENTINEL)
    ta = Rows(c["ta"], N - P, C, ld) if N > P else None
    tb = Rows(c["tb"], N - P, C, ld) if N > P and c["tb"] is not None else None
    per_class = isinstance(c["thr"], np.ndarray)
    thr = 0.0 if per_class or c["thr"] is None else float(c["thr"])
    tc = _f32(c["thr"]) if per_class else None
    y0, cw, rw, g = ints(c["y0"], np.int64), _f32(c["cw"]), _f32(row_w), _f32(G)
    stats, kept = vec(None, 4), torch.full((3,), -7, dtype=torch.int64, device=_dev())
    ws = torch.empty(int(L.mm_ce2s_ws_bytes()), dtype=torch.uint8, device=_dev())
    s = lib.stream()
    pa, pb, ldb = ta.ptr if ta else None, tb.ptr if tb else None, ld if tb else 0
    if entry == "w":
        lib.check(L.mm_ce2s_fwd_w(x.ptr, ld, N, P, C, _ptr(y0), _ptr(cw), -100, pa, ld, pb, ldb, T, thr, _ptr(tc), _ptr(rw), stats.ptr,
                                  kept.data_ptr() + 8, ws.data_ptr(), ws.numel(), s), "ce2s_fwd_w")
        lib.check(L.mm_ce2s_bwd_w(x.ptr, ld, N, P, C, _ptr(y0), _ptr(cw), -100, pa, ld, pb, ldb, T, thr, _ptr(tc), _ptr(rw), stats.ptr, _ptr(g),
                                  dl.ptr, c["ld_d"], s), "ce2s_bwd_w")
    else:
        assert row_w is None and (entry == "cls") == per_class
        fwd, bwd = (L.mm_ce2s_fwd_cls, L.mm_ce2s_bwd_cls) if per_class else (L.mm_ce2s_fwd, L.mm_ce2s_bwd)
        t = _ptr(tc) if per_class else thr
        lib.check(fwd(x.ptr, ld, N, P, C, _ptr(y0), _ptr(cw), -100, pa, ld, pb, ldb, T, t, stats.ptr, kept.data_ptr() + 8, ws.data_ptr(),
                      ws.numel(), s), "ce2s_fwd")
        lib.check(bwd(x.ptr, ld, N, P, C, _ptr(y0), _ptr(cw), -100, pa, ld, pb, ldb, T, t, stats.ptr, _ptr(g), dl.ptr, c["ld_d"], s), "ce2s_bwd")
    torch.cuda.synchronize()
    assert stats.padding_untouched() and dl.padding_untouched() and kept[0] == -7 and kept[2] == -7, c["name"]
    grad = dl.get32()
    assert not (grad == np.float32(SENTINEL)).any()
    return stats.get32().reshape(-1), int(kept[1]), grad


@pytest.mark.parametrize("name", list(SOFT))
def test_soft_pair_matches_float64(name):
    L, lib = _abi()
    c = _soft(name)
    P, tail = c["P"], c["tail"]
    print(f"{name}: smallest |confidence - threshold| {tail['dist']:.2e}, reference keeps {tail['K']} of {c['N'] - P} rows")
    assert tail["dist"] > 1e-6  # (choose another seed if a row ever lies this close: the float32 gate could then differ)
    stats, kept, grad = _run_soft(L, lib, c, c["rw"], "w")
    assert kept == tail["K"] == int(stats[3])  # K ignores the row weights
    if P:
        _check_segment(f"{name} head", stats[0], c["head"]["loss"], grad[:P], c["head"]["dlogits"], c["head"]["sum_w"])
    _check_segment(f"{name} tail", stats[2], tail["loss"], grad[P:], tail["dlogits"], max(tail["K"], 1))
    assert (grad[P:][~tail["keep"]] == 0).all() and (grad[P:][c["rw"] == 0] == 0).all()
    if c["N"] > P + 70:
        assert 0 < tail["K"] < c["N"] - P and not tail["keep"][[3, 64, 70]].any()
    if c["N"] == P:
        assert stats[2] == 0.0 and kept == 0


@pytest.mark.parametrize("name", ["777_300_6_thr", "777_300_6_own", "777_300_6_cls", "777_300_6_cls_own", "128_128_6", "pitched", "capped"])
def test_soft_pair_without_weights_and_with_unit_weights_is_the_parent_bit_for_bit(name):
    """Also the thr / thr_cls rule of the one entry point: a non-NULL thr_cls gives mm_ce2s_*_cls, NULL gives mm_ce2s_*."""
    L, lib = _abi()
    c = _soft(name)
    want = _run_soft(L, lib, c, None, "cls" if isinstance(c["thr"], np.ndarray) else "parent")
    for what, rw in (("row_w == NULL", None), ("row_w all 1.0f", np.ones(c["N"] - c["P"], np.float32))):
        got = _run_soft(L, lib, c, rw, "w")
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (name, what, "stats")
        assert got[1] == want[1], (name, what, "kept")
        assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32)), (name, what, "gradient")
    if c["N"] > c["P"]:
        assert not np.array_equal(_run_soft(L, lib, c, c["rw"], "w")[2], want[2])


@pytest.mark.parametrize("name", ["777_300_6_thr", "capped"])
def test_two_weighted_runs_are_bit_identical(name):
    L, lib = _abi()
    c, h = _soft(name), _hard("777_300_6")
    a, b = _run_soft(L, lib, c, c["rw"], "w"), _run_soft(L, lib, c, c["rw"], "w")
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and a[1] == b[1] and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    a, b = _run_hard(L, lib, h, h["rw"], "w"), _run_hard(L, lib, h, h["rw"], "w")
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


# ---------------------------------------------------------------------------------------------- through losses.* with autograd
def test_cross_entropy_pair_with_row_weights_is_the_abi_call_and_nothing_flows_to_the_weights():
    from mm2d3d_amd.losses import cross_entropy_pair

    L, lib = _abi()
    c, dev = _hard("777_300_6"), _dev()
    x = torch.from_numpy(c["x"]).to(dev).requires_grad_(True)
    rw = torch.from_numpy(c["rw"]).to(dev)
    lh, lt = cross_entropy_pair(x, c["P"], torch.from_numpy(c["y0"]), torch.from_numpy(c["y1"]), weight_head=c["cw"].tolist(), row_weight_tail=rw)
    (G[0] * lh + G[1] * lt).backward()
    stats, grad = _run_hard(L, lib, c, c["rw"], "w")
    assert lh.item() == float(stats[0]) and lt.item() == float(stats[2])
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), grad.view(np.int32))
    assert rw.grad is None and not rw.requires_grad
    above = {fn for fn, _ in (lh + lt).grad_fn.next_functions if fn is not None}
    assert len(above) == 1 and "CrossEntropyPair" in type(above.pop()).__name__  # still one node, one backward launch
    # None is the call without the option
    x2 = torch.from_numpy(c["x"]).to(dev).requires_grad_(True)
    lh2, lt2 = cross_entropy_pair(x2, c["P"], torch.from_numpy(c["y0"]), torch.from_numpy(c["y1"]), weight_head=c["cw"].tolist(), row_weight_tail=None)
    (G[0] * lh2 + G[1] * lt2).backward()
    want = _run_hard(L, lib, c, None, "parent")
    assert lt2.item() == float(want[0][2]) and np.array_equal(x2.grad.cpu().numpy().view(np.int32), want[1].view(np.int32))
    with pytest.raises(ValueError, match="requires grad"):
        cross_entropy_pair(x, c["P"], None, torch.from_numpy(c["y1"]), row_weight_tail=rw.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="lives on"):
        cross_entropy_pair(x, c["P"], None, torch.from_numpy(c["y1"]), row_weight_tail=rw.cpu())


@pytest.mark.parametrize("name", ["777_300_6_thr", "777_300_6_cls_own", "pitched"])
def test_cross_entropy_soft_pair_with_row_weights_is_the_abi_call_and_nothing_flows_to_the_weights(name):
    from mm2d3d_amd.losses import cross_entropy_soft_pair

    L, lib = _abi()
    c, dev = _soft(name), _dev()
    per_class = isinstance(c["thr"], np.ndarray)
    if c["ld"] != c["C"]:  # row-pitched views, read in place
        leaf = Rows(c["x"], c["N"], c["C"], c["ld"]).flat.requires_grad_(True)
        x = leaf.as_strided((c["N"], c["C"]), (c["ld"], 1), 0)
        ta = Rows(c["ta"], c["N"] - c["P"], c["C"], c["ld"]).view
        tb = Rows(c["tb"], c["N"] - c["P"], c["C"], c["ld"]).view
    else:
        leaf = x = torch.from_numpy(c["x"]).to(dev).requires_grad_(True)
        ta, tb = torch.from_numpy(c["ta"]).to(dev), (torch.from_numpy(c["tb"]).to(dev) if c["tb"] is not None else None)
    rw = torch.from_numpy(c["rw"]).to(dev)
    thr = _f32(c["thr"]) if per_class else c["thr"]
    lh, lt, kept = cross_entropy_soft_pair(x, c["P"], torch.from_numpy(c["y0"]), ta, tb, weight_head=c["cw"].tolist(), temperature=c["T"],
                                           threshold=thr, row_weight=rw)
    (G[0] * lh + G[1] * lt).backward()
    stats, k, grad = _run_soft(L, lib, c, c["rw"], "w")
    assert lh.item() == float(stats[0]) and lt.item() == float(stats[2]) and int(kept) == k
    got = leaf.grad.as_strided((c["N"], c["C"]), (c["ld"], 1), 0) if c["ld"] != c["C"] else leaf.grad
    assert np.array_equal(got.cpu().contiguous().numpy().view(np.int32), grad.view(np.int32))
    assert rw.grad is None and not rw.requires_grad and not kept.requires_grad
    with pytest.raises(ValueError, match="requires grad"):
        cross_entropy_soft_pair(x, c["P"], None, ta, tb, row_weight=rw.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"float32 tensor \["):
        cross_entropy_soft_pair(x, c["P"], None, ta, tb, row_weight=rw[:-1])
