"""The window search of the sparse-to-dense cross-modal matching (csrc/xmdense.hip mm_xm_search), the sort of caller-supplied keys
(mm_lift_sort_keys) and lifting.lift_at, through the bindings, against the float64 numpy reference of tests/_xmdense_ref.py.

Shapes: maps of B = 3 images of 7 x 9 pixels, N = 4000 points (not a multiple of 64, drawn with replacement, corners and edges
included), logits 3 * randn, C in {2, 6, 11, 32}, r in {1, 2, 3}, both directions, both layouts (the channel slice of a joint
[B, H, W, 2C] buffer whose other half is NaN, and a stand-alone NCHW map), P in {0, 1700, N}.

Selection: equal to float64 on every row whose float64 best-to-second gap is >= 1e-5; at most 2 % of a case's rows may be left out
(on these inputs: 1.1 % at C = 2, r = 3, under 0.1 % for C >= 6 or r = 1; the float32 restatement disagreed with float64 only below
a gap of 1e-9 - tests/test_xmdense_host.py).  Exact ties are compared on every row.

klmin against float64: the bound of the direct KL test (tests/test_gpu_loss_rows.py) is one for a MEAN over rows in units of the
mean of sum_c q (|log q| + |log p|), which a single saturated row can make arbitrarily small: it does not fit a per-row value.  So:
the float32 restatement of the kernel's expressions (_xmdense_ref.kl32) deviates from float64 on exactly these inputs by at most
9.6e-7 in units of (1 + klmin) (measured on the CPU, repeated by tests/test_xmdense_host.py); the kernel is allowed 8 x that,
7.7e-6 - the device's expf / logf and the compiler's contractions are worth a few ulp each.

lift_at backward: a pixel's gradient is a fixed-order float32 sum of its k row gradients, so it is within k * 2^-24 * sum |terms| of
the float64 index_put(accumulate=True); pixels nobody chose are +0; two runs give the same bits."""
import numpy as np
import pytest
import torch

import _xmdense_ref as R
from _gpu_rows import SENTINEL, Ints, Rows, abi as _abi, dev as _dev, ints, vec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _room_on_the_device():
    """The suite runs in one process and these files run late in it: by then the captured 2D trunks of earlier files (graph2d keeps
    them, with their private memory pools and their networks, until they are reset) and the allocator's cache hold most of the
    device.  Nothing of that is in use between two test modules, so it is handed back before this module's first test."""
    import gc

    from mm2d3d_amd import graph2d

    _dev()
    before = torch.cuda.memory_reserved()
    graph2d.reset()
    gc.collect()
    torch.cuda.empty_cache()
    print(f"device memory reserved by this process: {before / 2 ** 30:.1f} GiB before, {torch.cuda.memory_reserved() / 2 ** 30:.1f} GiB after the reset")
    yield


class _Map:
    """seg [B, H, W, C] on the device in one of the two layouts; ``strides`` = (sb, sy, sx, sc) in elements."""

    def __init__(self, seg, layout, half):
        B, H, W, C = seg.shape
        t = torch.from_numpy(np.ascontiguousarray(seg))
        if layout == "slice":
            joint = torch.full((B, H, W, 2 * C), float("nan"))
            joint[..., half * C:(half + 1) * C] = t
            self.buf = joint.to(_dev())
            self.ptr, self.strides = self.buf.data_ptr() + 4 * half * C, (H * W * 2 * C, W * 2 * C, 2 * C, 1)
        else:
            self.buf = t.permute(0, 3, 1, 2).contiguous().to(_dev())
            self.ptr, self.strides = self.buf.data_ptr(), (C * H * W, W, 1, H * W)


def _search(seg, key, rows, r, direction, P, layout="slice"):
    L, lib = _abi()
    B, H, W, C = seg.shape
    N = len(key)
    m = _Map(seg, layout, 1 - direction)  # the aux map is the second half of the joint buffer, the main map the first
    x = Rows(rows, N, C, C + 3)
    k = ints(key)
    sel, klmin, counts = Ints(None, N), vec(None, N), Ints(None, 4, dtype=torch.int64)
    ws = lib.workspace.get(int(L.mm_xm_search_ws_bytes()), _dev())
    lib.check(L.mm_xm_search(m.ptr, *m.strides, B, H, W, C, k.data_ptr(), x.ptr, C + 3, N, P, r, direction, sel.ptr, klmin.ptr, counts.ptr,
                             ws.data_ptr(), ws.numel(), lib.stream()), "xm_search")
    torch.cuda.synchronize()
    assert sel.padding_untouched() and klmin.padding_untouched() and counts.padding_untouched()
    return dict(sel=sel.get().astype(np.int64), klmin=klmin.get32().reshape(-1), bits=klmin.bits().reshape(-1), counts=counts.get())


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("r", R.RADII)
@pytest.mark.parametrize("C", R.CLASSES)
def test_search_against_float64(C, r, direction):
    seg, key, rows = R.case(C)
    ref = R.case_ref(C, r, direction)
    keep = ref["gap"] >= R.GAP
    left = 1.0 - keep.mean()
    got = _search(seg, key, rows, r, direction, 1700)
    err = R.klmin_error(got["klmin"], ref, keep)
    wrong = int((got["sel"][keep] != ref["sel"][keep]).sum())
    print(f"C={C} r={r} dir={direction}: left out {left:.4f} (max {R.LEFT_OUT_MAX}), wrong matches {wrong}, klmin error {err:.3e} "
          f"(bound {R.KLMIN_BOUND:.1e})")
    assert left <= R.LEFT_OUT_MAX
    assert wrong == 0
    assert err <= R.KLMIN_BOUND
    # every match is a candidate of its own point: inside the image, inside the window
    b, y, x = R.decode(key, R.H, R.W)
    sb, sy, sx = R.decode(got["sel"], R.H, R.W)
    assert (sb == b).all() and (np.abs(sy - y) <= r).all() and (np.abs(sx - x) <= r).all()
    # klmin never exceeds the kernel's own value of the centre (an r = 0 call), and is that value, bit for bit, where the point stayed
    centre = _search(seg, key, rows, 0, direction, 1700)
    assert (centre["sel"] == key).all() and centre["counts"].tolist() == [0, 0, 0, 0]
    assert (got["klmin"] <= centre["klmin"]).all()
    stay = got["sel"] == key
    assert (got["bits"][stay] == centre["bits"][stay]).all()
    assert R.klmin_error(centre["klmin"], R.case_ref(C, 0, direction), np.ones(R.N, bool)) <= R.KLMIN_BOUND
    # the counters: exact against the reference's when no row was left out, and always those of the kernel's own selection
    cheb = np.maximum(np.abs(sy - y), np.abs(sx - x))
    for P in R.SPLITS:
        c = got["counts"] if P == 1700 else _search(seg, key, rows, r, direction, P)["counts"]
        head = np.arange(R.N) < P
        assert c.tolist() == [int((~stay & head).sum()), int((~stay & ~head).sum()), int(cheb[head].sum()), int(cheb[~head].sum())], P
        if keep.all():
            rp = R.case_ref(C, r, direction, P)
            assert c.tolist() == rp["moved"].tolist() + rp["shift"].tolist(), P
    # the other layout, a second run: the same bits
    for layout in ("nchw", "slice"):
        again = _search(seg, key, rows, r, direction, 1700, layout)
        assert (again["sel"] == got["sel"]).all() and (again["bits"] == got["bits"]).all() and (again["counts"] == got["counts"]).all(), layout


@pytest.mark.parametrize("layout", ["slice", "nchw"])
@pytest.mark.parametrize("direction", [0, 1])
def test_exact_ties_and_nan_on_every_row(direction, layout):
    C = 6
    seg, key, rows = R.case(C)
    # a constant map: every candidate has the centre's value, every point stays
    const = np.broadcast_to(seg[0, 0, 0], seg.shape).copy()
    for r in R.RADII:
        got = _search(const, key, rows, r, direction, 1700, layout)
        assert (got["sel"] == key).all() and got["counts"].tolist() == [0, 0, 0, 0], r
    # two bit-identical best pixels, (2, 3) and (4, 5) of every image: the earlier candidate wins.  From (3, 4) both are in reach
    # at every radius ((2, 3) is candidate 1); from (3, 5) only (4, 5) is at r = 1, both are from r = 2 on.
    good, bad = np.asarray([5.0, -2.0, 0.5, 1.0, -1.0, 0.0], np.float32), np.asarray([-4.0, 3.0, 1.0, -2.0, 2.0, 0.5], np.float32)
    two = np.tile(bad, (R.B, R.H, R.W, 1))
    two[:, 2, 3] = good
    two[:, 4, 5] = good
    n = 300
    rng = np.random.default_rng(7)
    b = rng.integers(0, R.B, n)
    at34 = np.arange(n) % 2 == 0
    k2 = ((b * R.H + 3) * R.W + np.where(at34, 4, 5)).astype(np.int32)
    r2 = (good + 0.1 * rng.standard_normal((n, C))).astype(np.float32)
    for r in R.RADII:
        got, ref = _search(two, k2, r2, r, direction, 100, layout), R.search(two, k2, r2, r, direction, 100)
        want = (b * R.H + np.where(at34 | (r >= 2), 2, 4)) * R.W + np.where(at34 | (r >= 2), 3, 5)
        assert (ref["sel"] == want).all() and (got["sel"] == want).all(), r
        assert got["counts"].tolist() == ref["moved"].tolist() + ref["shift"].tolist(), r
    # NaN: pixels with a NaN logit are never matched (unless a point has nothing else: none here), a point on such a pixel moves
    # away, a point row with a NaN keeps its centre and its klmin is NaN
    holes = seg.copy()
    holes[0, 3, 4, 2] = holes[1, 0, 0, 5] = holes[2, 6, 8, 0] = holes[2, 2, 2, 1] = np.nan
    rows_n = rows.copy()
    dead = np.arange(R.N) % 97 == 5
    rows_n[dead, 3] = np.nan
    rows_n[np.arange(R.N) % 194 == 5] = np.nan
    hole_keys = {(0 * R.H + 3) * R.W + 4, (1 * R.H + 0) * R.W + 0, (2 * R.H + 6) * R.W + 8, (2 * R.H + 2) * R.W + 2}
    on_hole = np.isin(key, list(hole_keys))
    assert on_hole.sum() >= 40 and dead.sum() >= 40
    for r in R.RADII:
        got, ref = _search(holes, key, rows_n, r, direction, 1700, layout), R.search(holes, key, rows_n, r, direction, 1700)
        keep = (ref["gap"] >= R.GAP) | dead
        assert keep.mean() >= 1.0 - R.LEFT_OUT_MAX
        assert (got["sel"][keep] == ref["sel"][keep]).all(), r
        assert (got["sel"][dead] == key[dead]).all() and np.isnan(got["klmin"][dead]).all()
        assert not np.isin(got["sel"][~dead], list(hole_keys)).any() and not np.isnan(got["klmin"][~dead]).any()
        assert (got["sel"][on_hole & ~dead] != key[on_hole & ~dead]).all()
        assert R.klmin_error(got["klmin"], ref, keep & ~dead) <= R.KLMIN_BOUND


@pytest.mark.parametrize("no_spin", [0, 1])
@pytest.mark.parametrize("n", [1, 4000, 20000])  # 20000: past the 16384 keys below which the radix configuration sorts in one block
def test_sort_of_given_keys_is_ascending_a_permutation_and_stable(n, no_spin):
    L, lib = _abi()
    nkeys = R.B * R.H * R.W
    key = np.random.default_rng(11 + n).integers(0, nkeys, n).astype(np.int32)
    k, skey, order = ints(key), Ints(None, n), Ints(None, n)
    ws = lib.workspace.get(int(L.mm_lift_index_ws_bytes(n)), _dev())
    lib.check(L.mm_lift_sort_keys(k.data_ptr(), n, nkeys, no_spin, skey.ptr, order.ptr, ws.data_ptr(), ws.numel(), lib.stream()), "sort")
    torch.cuda.synchronize()
    assert skey.padding_untouched() and order.padding_untouched()
    s, o = skey.get(), order.get()
    assert (np.diff(s) >= 0).all() and sorted(o.tolist()) == list(range(n))
    want = np.argsort(key, kind="stable")
    assert (o == want).all() and (s == key[want]).all()


def _index(rng, n_per_image):
    from mm2d3d_amd.lifting import PixelIndex

    rc = [np.stack([rng.integers(0, R.H, n), rng.integers(0, R.W, n)], 1).astype(np.int64) for n in n_per_image]
    return PixelIndex(rc, R.H, R.W, _dev())


@pytest.mark.parametrize("layout", ["slice", "nchw"])
@pytest.mark.parametrize("C", [2, 6, 32])
def test_lift_at_forward_gathers_and_backward_sums_per_chosen_pixel(C, layout):
    from mm2d3d_amd.lifting import lift_at, pop_colsum

    rng = np.random.default_rng(20 + C)
    index = _index(rng, (1300, 0, 2700)[:R.B])
    n, npix = index.n, R.B * R.H * R.W
    assert n == R.N
    sel = rng.integers(0, npix // 2, n).astype(np.int32)  # the second half of the pixels is chosen by nobody
    seg = (3 * rng.standard_normal((R.B, R.H, R.W, C))).astype(np.float32)
    wgt = rng.standard_normal((n, C)).astype(np.float32)
    runs = []
    for _ in range(2):
        if layout == "slice":
            leaf = torch.zeros((R.B, R.H, R.W, 2 * C), device=_dev())
            leaf[..., C:] = torch.from_numpy(seg).to(_dev())
            leaf.requires_grad_()
            m = leaf.permute(0, 3, 1, 2)[:, C:]
        else:
            leaf = torch.from_numpy(seg).to(_dev()).permute(0, 3, 1, 2).contiguous().requires_grad_()
            m = leaf
        out = lift_at(m, index, ints(sel))
        assert np.array_equal(out.detach().cpu().numpy(), R.gather(seg, sel))
        (out * torch.from_numpy(wgt).to(_dev())).sum().backward()
        g = leaf.grad
        if layout == "slice":
            assert not g[..., :C].any()
            g = g[..., C:]
            # the per-channel sum filed for the bias behind the map (nn2d._HeadsFn.backward pops it by the gradient map's address)
            filed = pop_colsum(index, index._joint[leaf.data_ptr()].permute(0, 3, 1, 2)[:, C:])
            assert filed is not None and np.abs(filed.cpu().numpy() - wgt.astype(np.float64).sum(0)).max() <= n * 2.0 ** -24 * np.abs(wgt).sum(0).max()
        else:
            g = g.permute(0, 2, 3, 1)
        runs.append(g.contiguous().cpu().numpy().reshape(npix, C))
    dense, mag, k = R.scatter64(wgt, sel, npix)
    err = np.abs(runs[0].astype(np.float64) - dense)
    tol = k[:, None] * 2.0 ** -24 * mag
    print(f"C={C} {layout}: up to {k.max()} terms per pixel, largest error / tolerance {np.max(err[k > 0] / tol[k > 0]):.3f}")
    assert (err <= tol).all()
    empty = k == 0
    assert empty.sum() >= npix // 2 and (runs[0][empty].view(np.int32) == 0).all()  # +0, not -0
    assert (runs[0].view(np.int32) == runs[1].view(np.int32)).all()


def test_an_index_that_serves_several_steps_keeps_no_gradient_of_an_earlier_selection():
    """One PixelIndex, one joint buffer, three backward passes in a row - at a selection, at another selection, at the points' own
    pixels: each gradient map holds its own pass alone (the scatter stores at the pixels of its keys and touches no other)."""
    from mm2d3d_amd.lifting import lift, lift_at

    C = 6
    rng = np.random.default_rng(31)
    index = _index(rng, (1300, 0, 2700))
    n, npix = index.n, R.B * R.H * R.W
    leaf = torch.randn((R.B, R.H, R.W, 2 * C), device=_dev()).requires_grad_()
    m = leaf.permute(0, 3, 1, 2)[:, C:]
    wgt = rng.standard_normal((n, C)).astype(np.float32)
    own = index.key.cpu().numpy()[:n]
    for sel in (rng.integers(0, npix // 2, n).astype(np.int32), rng.integers(npix // 2, npix, n).astype(np.int32), None):
        leaf.grad = None
        out = lift(m, index) if sel is None else lift_at(m, index, ints(sel))
        (out * torch.from_numpy(wgt).to(_dev())).sum().backward()
        dense, mag, k = R.scatter64(wgt, own if sel is None else sel, npix)
        g = leaf.grad[..., C:].cpu().numpy().reshape(npix, C)
        assert (np.abs(g - dense) <= k[:, None] * 2.0 ** -24 * mag).all() and not g[k == 0].any()
    assert len(index._joint) == 1


def test_lift_at_refuses_keys_of_another_shape():
    from mm2d3d_amd.lifting import lift_at

    index = _index(np.random.default_rng(3), (10, 20, 30))
    seg = torch.zeros((R.B, 4, R.H, R.W), device=_dev())
    for bad in (torch.zeros(59, dtype=torch.int32, device=_dev()), torch.zeros(60, dtype=torch.int64, device=_dev())):
        with pytest.raises(ValueError, match="selected keys"):
            lift_at(seg, index, bad)


def test_argument_errors_launch_nothing():
    L, lib = _abi()
    C, N = 6, 500
    seg, key, rows = R.make_case(9, R.B, R.H, R.W, C, N)
    m, x, k = _Map(seg, "slice", 1), Rows(rows, N, C, C), ints(key)
    sel, klmin, counts = Ints(None, N), vec(None, N), Ints(None, 4, dtype=torch.int64)
    ws = lib.workspace.get(int(L.mm_xm_search_ws_bytes()), _dev())

    def call(r=2, C=C, P=100, N=N, direction=0, ld=C, sel_ptr=sel.ptr):
        return L.mm_xm_search(m.ptr, *m.strides, R.B, R.H, R.W, C, k.data_ptr(), x.ptr, ld, N, P, r, direction, sel_ptr, klmin.ptr,
                              counts.ptr, ws.data_ptr(), ws.numel(), lib.stream())

    for kw in (dict(r=-1), dict(r=4), dict(C=1), dict(C=33), dict(P=-1), dict(P=N + 1), dict(N=1 << 31), dict(N=(1 << 31) // C + 1, P=0),
               dict(direction=2), dict(ld=C - 1), dict(sel_ptr=None)):
        assert call(**kw) == -1, kw
        assert b"xm_search:" in L.mm_last_error()
    torch.cuda.synchronize()
    assert sel.untouched() and klmin.untouched() and counts.untouched()
    assert call(r=0) == 0
    torch.cuda.synchronize()
    assert (sel.get() == key).all() and counts.get().tolist() == [0, 0, 0, 0]
