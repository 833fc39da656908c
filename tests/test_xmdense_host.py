"""Host checks of the sparse-to-dense cross-modal matching: properties of the float64 reference (tests/_xmdense_ref.py) that follow
from the definition, the float32 restatement against it on the inputs of tests/test_gpu_xmdense.py (where that test's tolerance
comes from), train_kwargs["xm_window"] in the constructor (mm2d3d_amd/xmdense.py), and the declarations and argument checks of
mm_xm_search / mm_lift_sort_keys (include/mm2d3d.h), every one of which is decided before any device call.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _xmdense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the reference
def test_candidate_order_is_centre_first_then_row_major():
    assert R.window(0) == [(0, 0)]
    assert R.window(1) == [(0, 0), (-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    for r in (2, 3):
        w = R.window(r)
        assert len(w) == len(set(w)) == (2 * r + 1) ** 2 and w[0] == (0, 0) and w[1:] == sorted(w[1:])


@pytest.mark.parametrize("direction", [0, 1])
def test_radius_zero_is_the_plain_gather_and_kl(direction):
    seg, key, rows = R.make_case(1, 2, 5, 6, 4, 300)
    f = R.search(seg, key, rows, 0, direction)
    pix = R.gather(seg, key)
    kl = R.kl64(rows, pix)[0] if direction == 0 else R.kl64(pix, rows)[0]
    assert (f["sel"] == key).all() and (f["ord"] == 0).all() and (f["klmin"] == kl).all()
    assert f["moved"].tolist() == [0, 0] and f["shift"].tolist() == [0, 0]


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_matched_kl_never_exceeds_the_centre_kl(r, direction):
    seg, key, rows = R.make_case(2, 2, 5, 6, 4, 300)
    f, centre = R.search(seg, key, rows, r, direction), R.search(seg, key, rows, 0, direction)
    assert (f["klmin"] <= centre["klmin"]).all() and (f["klmin"] < centre["klmin"]).any()
    # ... and a wider window never does worse than a narrower one
    if r > 1:
        assert (f["klmin"] <= R.search(seg, key, rows, r - 1, direction)["klmin"]).all()


@pytest.mark.parametrize("direction", [0, 1])
def test_constant_map_keeps_every_point_on_its_centre(direction):
    seg, key, rows = R.make_case(3, 2, 5, 6, 4, 300)
    seg[:] = seg[0, 0, 0]
    for precision in (64, 32):
        f = R.search(seg, key, rows, 3, direction, P=100, precision=precision)
        assert (f["sel"] == key).all() and f["moved"].tolist() == [0, 0] and f["shift"].tolist() == [0, 0]


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_good_pixel_in_a_window_corner_is_found_and_clipped_at_the_image_corners(r, direction):
    """One point in the middle of a 9 x 9 image with the only good pixel in each corner of its window in turn; then one point in each
    corner of the image, whose window is clipped to (r + 1)^2 pixels, with the good pixel in the far corner of what is left."""
    H = W = 9
    C = 3
    row = np.asarray([[4.0, -1.0, 0.5]], np.float32)
    bad = np.asarray([-3.0, 2.0, 1.0], np.float32)
    for y, x in ((4, 4), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        for sy, sx in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
            gy, gx = y + sy * r, x + sx * r
            seg = np.tile(bad, (1, H, W, 1))
            inside = 0 <= gy < H and 0 <= gx < W
            if inside:
                seg[0, gy, gx] = row[0]
            f = R.search(seg, [y * W + x], row, r, direction)
            n_in = int(f["inside"].sum())
            assert n_in == (min(y, r) + min(H - 1 - y, r) + 1) * (min(x, r) + min(W - 1 - x, r) + 1)
            if inside:
                assert f["sel"][0] == gy * W + gx and f["klmin"][0] == 0.0 and f["moved"].tolist() == [1, 0] and f["shift"].tolist() == [r, 0]
            else:  # the good pixel would lie outside the image: everything in reach is equally bad, the point stays
                assert f["sel"][0] == y * W + x and f["moved"].tolist() == [0, 0]


@pytest.mark.parametrize("direction", [0, 1])
def test_window_never_reads_a_neighbouring_image(direction):
    """Image 1 is all perfect matches, image 0 all bad: the points on the last row of image 0 (next to image 1 in memory) and
    on the first row of image 2 stay inside their own images."""
    B, H, W, C = 3, 4, 5, 3
    row = np.asarray([4.0, -1.0, 0.5], np.float32)
    seg = np.tile(np.asarray([-3.0, 2.0, 1.0], np.float32), (B, H, W, 1))
    seg[1] = row
    key = np.asarray([(0 * H + H - 1) * W + x for x in range(W)] + [(2 * H + 0) * W + x for x in range(W)])
    f = R.search(seg, key, np.tile(row, (len(key), 1)), 3, direction)
    assert (f["sel"] // (H * W) == key // (H * W)).all() and (f["sel"] == key).all() and (f["klmin"] > 1.0).all()


def test_nan_candidates_are_skipped_and_an_all_nan_point_keeps_the_centre():
    seg, key, rows = R.make_case(5, 1, 5, 6, 4, 40)
    key[:] = 2 * 6 + 3
    seg[0, 1, 2, 0] = np.nan  # candidate 1 of the window of (2, 3)
    rows[7] = np.nan
    for precision in (64, 32):
        f = R.search(seg, key, rows, 1, 0, precision=precision)
        assert (f["sel"] != 1 * 6 + 2).all() and f["sel"][7] == key[7] and np.isnan(f["klmin"][7]) and not np.isnan(np.delete(f["klmin"], 7)).any()


def test_float32_restatement_agrees_on_the_gpu_tests_inputs():
    """Where tests/test_gpu_xmdense.py takes its numbers from: on its inputs the float32 restatement picks the float64 match on every
    row whose float64 gap is >= GAP (it disagreed only below a gap of 1e-9), at most LEFT_OUT_MAX of a case's rows are left out, and
    its klmin deviates from float64 by at most KLMIN_FP32 in units of (1 + klmin)."""
    worst, left = 0.0, 0.0
    for C in R.CLASSES:
        seg, key, rows = R.case(C)
        for r in R.RADII:
            for direction in (0, 1):
                a, b = R.case_ref(C, r, direction), R.search(seg, key, rows, r, direction, precision=32)
                keep = a["gap"] >= R.GAP
                assert (a["sel"][keep] == b["sel"][keep]).all(), (C, r, direction)
                left = max(left, 1.0 - keep.mean())
                worst = max(worst, R.klmin_error(b["klmin"], a, keep))
    print(f"float32 restatement: klmin error {worst:.3e} (recorded {R.KLMIN_FP32:.1e}), largest share left out {left:.4f}")
    assert left <= R.LEFT_OUT_MAX
    assert 0.5 * R.KLMIN_FP32 <= worst <= R.KLMIN_FP32


# ---------------------------------------------------------------------------------------------- the option
def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"),
                      dict(gc_freeze=False, **kw))


def test_constructor_defaults_values_and_refusals():
    tm = _trainer()
    assert tm.xm_window == 0 and tm.last_match is None and not tm.dense_xm.active
    for r in (1, 2, 3):
        tm = _trainer(xm_window=r)
        assert tm.xm_window == r and tm.dense_xm.xm_window == r and tm.dense_xm.active and tm.last_match is None
    for bad in (-1, 4, 1.0, 2.5, "2", None, True, [1], float("nan")):
        with pytest.raises(ValueError, match="xm_window"):
            _trainer(xm_window=bad)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_library_exports_the_entry_points():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mm_xm_search_ws_bytes", "mm_xm_search", "mm_lift_sort_keys"):
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", txt), f"{name} is not declared in include/mm2d3d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib._PROTOS
    decl = re.search(r"int mm_xm_search\(([^;]*)\);", txt).group(1)
    assert len(decl.split(",")) == len(_lib._PROTOS["mm_xm_search"][1])
    decl = re.search(r"int mm_lift_sort_keys\(([^;]*)\);", txt).group(1)
    assert len(decl.split(",")) == len(_lib._PROTOS["mm_lift_sort_keys"][1])


def test_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep = (ctypes.c_double * 8192)()  # never read or written: every call below is refused before a device call
    p = ctypes.addressof(keep)
    need = int(L.mm_xm_search_ws_bytes())
    assert need >= 1024 * 4 * 8  # 1024 workgroups' four integer counters

    def search(**kw):
        a = dict(seg=p, B=3, H=7, W=9, C=6, key=p, rows=p, ld=6, N=100, P=40, r=2, direction=0, sel=p, klmin=p, counts=p, ws=p, ws_bytes=need)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.mm_xm_search(a["seg"], a["H"] * a["W"] * 2 * a["C"], a["W"] * 2 * a["C"], 2 * a["C"], 1, a["B"], a["H"], a["W"], a["C"], a["key"],
                              a["rows"], a["ld"], a["N"], a["P"], a["r"], a["direction"], a["sel"], a["klmin"], a["counts"], a["ws"],
                              a["ws_bytes"], None)

    for kw in (dict(r=-1), dict(r=4), dict(C=1), dict(C=33, ld=33), dict(P=-1), dict(P=101), dict(N=-1, P=0), dict(N=(1 << 31) // 6 + 1),
               dict(N=1 << 31), dict(direction=2), dict(direction=-1), dict(ld=5), dict(seg=None), dict(key=None), dict(rows=None),
               dict(sel=None), dict(klmin=None), dict(counts=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=-3), dict(B=1 << 15, H=1 << 8, W=1 << 8)):
        assert search(**kw) == -1, kw
        assert b"xm_search:" in L.mm_last_error(), (kw, L.mm_last_error())
    assert search(ws_bytes=need - 1) == -3

    def sort(**kw):
        a = dict(key=p, n=100, nkeys=189, skey=p, order=p, ws=p, ws_bytes=1 << 30)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.mm_lift_sort_keys(a["key"], a["n"], a["nkeys"], 0, a["skey"], a["order"], a["ws"], a["ws_bytes"], None)

    for kw in (dict(n=-1), dict(n=1 << 31), dict(nkeys=0), dict(nkeys=1 << 31), dict(key=None), dict(skey=None), dict(order=None), dict(ws=None)):
        assert sort(**kw) == -1, kw
        assert b"lift_sort_keys:" in L.mm_last_error(), (kw, L.mm_last_error())
    assert sort(ws_bytes=16) == -3
    assert sort(n=0, key=None, skey=None, order=None, ws=None) == 0  # nothing to sort
