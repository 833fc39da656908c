"""The 2D -> 3D lifting of csrc/lift.hip, called straight through the C ABI (mm_lift_index, mm_lift_gather_key,
mm_lift_scatter_key) and once through the autograd wrapper, against the numpy references of tests/_loss_ref.py.  Every assertion
is exact.

Index: the keys are integers, the sort is stable, so key, skey and order must EQUAL (b*H + r)*W + c, np.sort and the stable
np.argsort, with either sort configuration (no_spin 0: merge sort up to 16,384 keys, Onesweep radix sort above; no_spin 1: merge
sort throughout) and at the edges of the number of key bits the host computes from nb*H*W.

Gather: a copy.  Scatter: on grid inputs (multiples of 1/8, exact run sums asserted by the maker) the sums equal float64
np.add.at; on unrestricted float32 inputs they equal np.add.at on a float32 array bit for bit, because np.add.at adds one point
after the other in index order, which is the kernel's contract (ascending point order within a pixel).  Maps are views as
lifting._LiftFn passes them: NCHW, NHWC, and a channel slice of a wider NHWC buffer whose other channels hold NaN (inputs) or a
sentinel that must survive (gradients); pixels without points keep the sentinel too."""
import functools

import numpy as np
import pytest
import torch

import _loss_ref as R
from _gpu_rows import SENTINEL, Ints, Rows, abi as _abi, dev as _dev

pytestmark = pytest.mark.gpu

MERGE_LIMIT = 16384  # SortCfg of csrc/lift.hip: up to this many keys the radix sort hands over to a merge sort
MAXB = 1024


# --------------------------------------------------------------------------------------------------------------- case tables
def _split(n, nb):
    """n points over nb scenes, uneven."""
    cuts = sorted((n * (i * i + 1)) // (nb * nb + 1) for i in range(1, nb))
    return np.diff([0] + cuts + [n]).tolist()


def _ix(nb, H, W, counts, kind="random", bad=None):
    assert len(counts) == nb
    return dict(nb=nb, H=H, W=W, counts=list(counts), kind=kind, bad=bad)


def _index_cases():
    t = {}
    for n in (0, 1, 2, 255, 256, 257, 2049, 4097, MERGE_LIMIT - 1, MERGE_LIMIT, MERGE_LIMIT + 1, 150001):
        t[f"n{n}"] = _ix(3, 97, 131, _split(n, 3), "last" if n else "random")
    t["n0_no_scene"] = _ix(0, 97, 131, [])
    t["dup7_n4097"] = _ix(1, 97, 131, [4097], "dup7")  # stability decides the order
    t["dup7_n20001"] = _ix(2, 97, 131, [1, 20000], "dup7")
    t["one_pixel_n5000"] = _ix(1, 17, 23, [5000], "one")
    t["one_pixel_n20000"] = _ix(2, 17, 23, [0, 20000], "one")
    t["map_of_one_pixel"] = _ix(1, 1, 1, [300])  # nb*H*W = 1
    t["map_2pow11"] = _ix(4, 16, 32, _split(1000, 4), "last")  # nb*H*W = 2^11: 11 key bits, the last pixel is 2^11 - 1
    t["map_2pow10_plus_1"] = _ix(5, 5, 41, _split(1000, 5), "last")  # 2^10 + 1: 11 key bits, the last pixel is 2^10
    t["map_2pow15_n20000"] = _ix(8, 64, 64, _split(20000, 8), "last")
    t["map_2pow15_plus_1_n20000"] = _ix(1, 1, 32769, [20000], "last")
    counts = [(1 if b % 3 == 0 else 0) for b in range(MAXB)]
    counts[0], counts[MAXB - 1] = 0, 1
    t["keys_31_bits_sparse"] = _ix(MAXB, 1024, 2047, counts, "last")  # 0 or 1 points per scene; the last key is nb*H*W - 1
    counts = [((11 * b) % 61 if b % 5 else 0) for b in range(MAXB)]
    counts[MAXB - 1] = 3
    t["keys_31_bits_n20k"] = _ix(MAXB, 1024, 2047, counts, "last")
    t["empty_scenes"] = _ix(6, 17, 23, [0, 300, 0, 0, 500, 0])
    t["empty_scenes_n20000"] = _ix(7, 97, 131, [0, 0, 9000, 0, 11000, 0, 0])
    # rows / cols outside the map, on the device side: clamped, and the error flag is raised
    t["clamped"] = _ix(2, 17, 23, [300, 300], bad={5: (-1, 3), 6: (17, 3), 299: (3, -1), 300: (3, 23), 301: (2 ** 40, 2 ** 40), 599: (-2 ** 40, 22)})
    return t


INDEX_CASES = _index_cases()


@functools.lru_cache(maxsize=None)
def index_inputs(name):
    c = INDEX_CASES[name]
    rc = R.make_points(c["nb"], c["H"], c["W"], c["counts"], 1300 + list(INDEX_CASES).index(name), c["kind"])
    for p, v in (c["bad"] or {}).items():
        rc[p] = v
    key, err = R.lift_keys(rc, c["counts"], c["H"], c["W"])
    assert err == int(bool(c["bad"])) and (len(key) == 0 or (key.min() >= 0 and key.max() < c["nb"] * c["H"] * c["W"] < 2 ** 31))
    if c["kind"] == "last":
        assert key.max() == c["nb"] * c["H"] * c["W"] - 1
    skey, order = R.lift_sorted(key)
    return dict(rc=rc, key=key, skey=skey, order=order, err=err)


def key_bits(c):
    """The number of key bits mm_lift_index sorts by, restated."""
    bits = 1
    while bits < 32 and (1 << bits) < c["nb"] * c["H"] * c["W"]:
        bits += 1
    return bits


# (C, layout): every width in both plain layouts, and the production layout: channels [6, 12) of a 12-channel NHWC buffer
MAP_CASES = [(C, lay) for C in (1, 3, 6, 17, 32) for lay in ("nchw", "nhwc")] + [(6, "slice"), (3, "slice")]
MAP_B, MAP_H, MAP_W = 3, 17, 23


@functools.lru_cache(maxsize=None)
def map_points(big_run=False):
    """Points of 3 scenes on a 17 x 23 map with an empty scene in the middle: many short runs of equal pixels, pixels without a point
    and (big_run) one run of 5000 points."""
    counts = [700, 0, 401 + (5000 if big_run else 0)]
    rc = R.make_points(MAP_B, MAP_H, MAP_W, counts, 77 + big_run)
    if big_run:
        rc[np.random.default_rng(5).choice(np.arange(700, sum(counts)), 5000, replace=False)] = (11, 13)
    rc[rc[:, 0] == 5] = (6, 1)  # row 5 of every map stays without points
    key, _ = R.lift_keys(rc, counts, MAP_H, MAP_W)
    skey, order = R.lift_sorted(key)
    runs = np.diff(np.flatnonzero(np.diff(skey, prepend=-1, append=-1)))
    assert (not big_run or runs.max() >= 5000) and (runs == 1).any() and (runs == 2).any()
    return dict(key=key, skey=skey, order=order, n=len(key))


def _device_map(C, layout, fill):
    """A [B, C, H, W] view on the device laid out as ``layout``, and the buffer it lives in (filled with ``fill``)."""
    if layout == "nchw":
        buf = torch.full((MAP_B, C, MAP_H, MAP_W), fill, dtype=torch.float32, device=_dev())
        return buf, buf
    pitch, off = (C, 0) if layout == "nhwc" else (2 * C, C)
    buf = torch.full((MAP_B, MAP_H, MAP_W, pitch), fill, dtype=torch.float32, device=_dev())
    return buf[..., off:off + C].permute(0, 3, 1, 2), buf


def _strides(seg):
    """In the order lifting._LiftFn passes them: batch, row, column, channel."""
    return seg.stride(0), seg.stride(2), seg.stride(3), seg.stride(1)


# -------------------------------------------------------------------------------------------------------------------- index
def _run_index(L, lib, c, d, no_spin):
    n = len(d["key"])
    rc, counts = Ints(d["rc"], dtype=torch.int64), Ints(np.asarray(c["counts"], np.int64), dtype=torch.int64)
    key, skey, order, err = Ints(None, n), Ints(None, n), Ints(None, n), Ints(np.zeros(1, np.int32))
    ws = torch.empty(int(L.mm_lift_index_ws_bytes(n)), dtype=torch.uint8, device=_dev())
    lib.check(L.mm_lift_index(rc.ptr, counts.ptr, c["nb"], n, c["H"], c["W"], no_spin, key.ptr, skey.ptr, order.ptr, err.ptr,
                              ws.data_ptr(), ws.numel(), lib.stream()), "lift_index")
    torch.cuda.synchronize()
    return key, skey, order, err


@pytest.mark.parametrize("no_spin", [0, 1])
@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_index_keys_sorted_keys_and_stable_order_equal_numpy(name, no_spin):
    c, d = INDEX_CASES[name], index_inputs(name)
    L, lib = _abi()
    key, skey, order, err = _run_index(L, lib, c, d, no_spin)
    for t in (key, skey, order, err):
        assert t.padding_untouched()
    what = f"{name} (n = {len(d['key'])}, {key_bits(c)} key bits, no_spin = {no_spin})"
    assert np.array_equal(key.get(), d["key"]), f"{what}: keys"
    assert np.array_equal(skey.get(), d["skey"]), f"{what}: sorted keys"
    got = order.get()
    if not np.array_equal(got, d["order"]):
        assert np.array_equal(np.sort(got), np.arange(len(got))), f"{what}: order is no permutation"
        assert np.array_equal(d["key"][got], d["skey"]), f"{what}: order does not sort the keys"
        raise AssertionError(f"{what}: the sort is not stable")
    assert int(err.get()[0]) == d["err"], f"{what}: error flag"


# ------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("C,layout", MAP_CASES)
def test_gather_copies_the_pixel_of_every_point(C, layout):
    L, lib = _abi()
    pts = map_points()
    n = pts["n"]
    seg, buf = _device_map(C, layout, float("nan"))
    values = torch.from_numpy(np.random.default_rng(C).standard_normal((MAP_B, C, MAP_H, MAP_W)).astype(np.float32))
    seg.copy_(values.to(_dev()))
    assert layout != "slice" or bool(torch.isnan(buf[..., :C]).all())
    key, out = Ints(pts["key"]), Rows(None, n, C, C, 4, fill=SENTINEL)
    lib.check(L.mm_lift_gather_key(seg.data_ptr(), *_strides(seg), key.ptr, n, C, MAP_H, MAP_W, out.ptr, lib.stream()), "lift_gather")
    torch.cuda.synchronize()
    assert out.padding_untouched()
    assert np.array_equal(out.get32(), R.lift_gather(values.numpy(), pts["key"]))
    none = Rows(None, 0, C, C, 4, fill=SENTINEL)
    lib.check(L.mm_lift_gather_key(seg.data_ptr(), *_strides(seg), key.ptr, 0, C, MAP_H, MAP_W, none.ptr, lib.stream()), "lift_gather")
    torch.cuda.synchronize()
    assert none.untouched()


# ------------------------------------------------------------------------------------------------------------------ scatter
def _scatter(C, layout, pts, dout):
    L, lib = _abi()
    n = pts["n"]
    dseg, buf = _device_map(C, layout, SENTINEL)
    d = Rows(dout, n, C, C, 4)
    order, skey = Ints(pts["order"]), Ints(pts["skey"])
    lib.check(L.mm_lift_scatter_key(d.ptr, C, order.ptr, skey.ptr, n, MAP_H, MAP_W, *_strides(dseg), dseg.data_ptr(), lib.stream()),
              "lift_scatter")
    torch.cuda.synchronize()
    return dseg.cpu().numpy(), buf.cpu().numpy()


def _expected_map(sums, touched):
    want = np.where(touched[:, None], sums, SENTINEL).astype(np.float32)
    assert not touched[:, 5].any() and touched.any()
    return want


@pytest.mark.parametrize("C,layout", MAP_CASES)
def test_scatter_sums_equal_float64_on_grid_inputs(C, layout):
    pts = map_points()
    dout = R.make_scatter_grid(pts["n"], C, pts["key"], 1500 + C)
    got, buf = _scatter(C, layout, pts, dout)
    sums, touched = R.lift_scatter(dout, pts["key"], (MAP_B, C, MAP_H, MAP_W))
    assert np.array_equal(got.astype(np.float64), _expected_map(sums, touched).astype(np.float64))
    if layout == "slice":
        assert (buf[..., :C] == SENTINEL).all(), "the other channels of the wide buffer were written"


@pytest.mark.parametrize("C,layout", [(6, "slice"), (17, "nhwc"), (3, "nchw")])
def test_scatter_adds_in_ascending_point_order_bit_for_bit(C, layout):
    pts = map_points(big_run=True)
    dout = (3 * np.random.default_rng(C).standard_normal((pts["n"], C))).astype(np.float32)
    got, buf = _scatter(C, layout, pts, dout)
    sums, touched = R.lift_scatter(dout, pts["key"], (MAP_B, C, MAP_H, MAP_W), np.float32)
    want = _expected_map(sums, touched)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got != want).sum())} sums differ from the sequential float32 sum"
    # the order matters for this input: the float64 sum rounds differently somewhere
    exact, _ = R.lift_scatter(dout, pts["key"], (MAP_B, C, MAP_H, MAP_W))
    assert (exact.astype(np.float32) != sums).any()
    if layout == "slice":
        assert (buf[..., :C] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------ wrapper level
def test_lift_of_two_channel_slices_shares_one_joint_gradient_buffer():
    """What nn2d.fused_heads and the lifting do in production: the two heads are the halves of ONE [B, h, w, 12] buffer, each is
    lifted, and the two backward passes write their halves of ONE joint gradient buffer."""
    from mm2d3d_amd.lifting import PixelIndex, lift, pop_colsum

    dev = _dev()
    pts = map_points()
    counts = [700, 0, 401]
    _, r, c = R.key_pixels(pts["key"], MAP_H, MAP_W)
    rc = np.stack([r, c], 1)
    idx = [rc[sum(counts[:i]): sum(counts[:i + 1])] for i in range(3)]
    index = PixelIndex(idx, MAP_H, MAP_W, dev)
    rng = np.random.default_rng(9)
    values = rng.standard_normal((MAP_B, MAP_H, MAP_W, 12)).astype(np.float32)
    wide = torch.from_numpy(values).to(dev).requires_grad_(True)
    douts = [R.make_scatter_grid(pts["n"], 6, pts["key"], 1600 + i) for i in range(2)]
    heads = [wide[..., 6 * i: 6 * i + 6].permute(0, 3, 1, 2) for i in range(2)]
    grads = {}
    for i, h in enumerate(heads):  # the gradient maps as the lifting backward hands them on, before autograd adds them into wide.grad
        h.register_hook(lambda g, i=i: grads.__setitem__(i, g))
    outs = [lift(h, index) for h in heads]
    for i in range(2):
        assert np.array_equal(outs[i].detach().cpu().numpy(), R.lift_gather(values.transpose(0, 3, 1, 2)[:, 6 * i: 6 * i + 6], pts["key"]))
    sum((o * torch.from_numpy(d).float().to(dev)).sum() for o, d in zip(outs, douts)).backward()
    torch.cuda.synchronize()
    g0, g1 = grads[0], grads[1]
    assert g0.shape == g1.shape == (MAP_B, 6, MAP_H, MAP_W)
    # views of one joint [B, H, W, 12] buffer: the same storage, 6 floats apart, NHWC strides of pitch 12
    assert g1.data_ptr() - g0.data_ptr() == 6 * 4 and g0.stride() == g1.stride() == (MAP_H * MAP_W * 12, 1, MAP_W * 12, 12)
    assert g0.untyped_storage().data_ptr() == g1.untyped_storage().data_ptr()
    assert len(index._joint) == 1
    want = []
    for i, g in enumerate((g0, g1)):
        sums, _ = R.lift_scatter(douts[i], pts["key"], (MAP_B, 6, MAP_H, MAP_W))
        assert np.array_equal(g.cpu().numpy().astype(np.float64), sums), f"gradient of head {i}"
        want.append(sums)
    assert np.array_equal(wide.grad.cpu().numpy().astype(np.float64), np.concatenate(want, 1).transpose(0, 2, 3, 1))
    # the per-channel sums filed for the 1x1 heads' bias gradients: for the right map, and not for another shape at the same address
    col1 = pop_colsum(index, g1)
    assert col1 is not None and np.array_equal(col1.cpu().numpy().astype(np.float64), douts[1].sum(0))
    assert pop_colsum(index, g1) is None, "a sum is handed out once"
    assert g0[:, :3].data_ptr() == g0.data_ptr() and pop_colsum(index, g0[:, :3]) is None


# ---------------------------------------------------------------------------------------------------------- refused arguments
def test_lift_error_returns_come_before_any_launch():
    """Points without a scene, a channel count of 0 and negative point counts are refused, and a refused call has written nothing.
    The buffers are sized so that a call that was wrongly accepted would still stay inside them.  (The refusals of null pointers
    and of H or W = 0 are not tried: accepted by mistake, such a call would read or write outside every buffer.)"""
    L, lib = _abi()
    n, H, W = 64, 17, 23
    rc, counts = Ints(np.zeros((n, 2), np.int64), dtype=torch.int64), Ints(np.asarray([n], np.int64), dtype=torch.int64)
    key, skey, order, err = Ints(None, n), Ints(None, n), Ints(None, n), Ints(None, 1)
    ws = torch.empty(int(L.mm_lift_index_ws_bytes(n)), dtype=torch.uint8, device=_dev())
    s = lib.stream()
    seg = torch.ones((1, 4, H, W), dtype=torch.float32, device=_dev())
    zkey = Ints(np.zeros(n, np.int32))
    zorder = Ints(np.arange(n, dtype=np.int32))
    out, dseg = Rows(None, n, 4, 4, fill=SENTINEL), Rows(None, 4 * H, W, W, fill=SENTINEL)
    calls = [
        ("lift_index nb = 0", "points in no scene", lambda: L.mm_lift_index(rc.ptr, counts.ptr, 0, n, H, W, 0, key.ptr, skey.ptr, order.ptr,
                                                                               err.ptr, ws.data_ptr(), ws.numel(), s)),
        ("lift_gather C = 0", "too many elements", lambda: L.mm_lift_gather_key(seg.data_ptr(), 4 * H * W, W, 1, H * W, zkey.ptr, n, 0, H, W,
                                                                                  out.ptr, s)),
        ("lift_gather N = -1", "too many elements", lambda: L.mm_lift_gather_key(seg.data_ptr(), 4 * H * W, W, 1, H * W, zkey.ptr, -1, 4, H, W,
                                                                                   out.ptr, s)),
        ("lift_scatter C = 0", "too many elements", lambda: L.mm_lift_scatter_key(out.ptr, 0, zorder.ptr, zkey.ptr, n, H, W, 4 * H * W, W, 1,
                                                                                    H * W, dseg.ptr, s)),
        ("lift_scatter N = -1", "too many elements", lambda: L.mm_lift_scatter_key(out.ptr, 4, zorder.ptr, zkey.ptr, -1, H, W, 4 * H * W, W, 1,
                                                                                     H * W, dseg.ptr, s)),
    ]
    accepted = []
    for what, msg, call in calls:
        try:
            lib.check(call(), what)
            accepted.append(what)
        except RuntimeError as e:
            assert "rc=-1" in str(e) and msg in str(e), (what, str(e))
    torch.cuda.synchronize()
    assert not accepted, f"accepted: {accepted}"
    for t in (key, skey, order, err, out, dseg):
        assert t.untouched(), "a refused call has written"
