"""The dense 2D glue kernels of csrc/misc2d.hip (mm_copy_rows_bf16, mm_concat_bf16, mm_maxpool3x3s2_fwd / _bwd, mm_head_fwd / _bwd)
and mm_colsum_bf16 of csrc/bn2d.hip, called straight through the C ABI in both 16-bit builds (the plain symbols store bf16, the
_f16 symbols IEEE fp16) against the float64 references of tests/_misc2d_ref.py.

Pitched operands are views into wider buffers; inputs carry NaN in their padding (and in the pixels a head's crop leaves out),
outputs a sentinel that must survive; workspaces are filled with NaN before a call.

Bit for bit: the copies; the max-pool's y and idx (idx = first maximum in scan order over the taps inside the image); the max-pool's
dx for gradients on the 1/8 grid (any float32 sum of 8 of them is exact, so dx = round16 of the exact sum); +0 in every dx pixel
that no window selects and in every head dx pixel outside the crop; column sums of grid values.

Max-pool backward with normal gradients: dx within [round16(ref - e), round16(ref + e)], e = 7 * 2^-24 * abs_sum, the worst case of
an 8-term float32 sum; rounding is monotone, so that interval is the whole allowance.

Column sums: 2^-23 of the column's abs_sum (+ |out| before the call when accumulate = 1): one float32 rounding of the float64 total
and one float32 add.  (Below the float64 partials a thread adds the rows_per_block / rows-in-flight <= 17 sixteen-bit numbers of
its column slot in float32, which is exact unless their exponents spread over more than 24 - 11 - 5 bits.)

Heads: errors per element relative to that element's abs_sum (the same sum with every term's absolute value); out and dW directly,
dx (16 bits) in the interval form with e = bound * abs_sum.  The bounds are not invented: _misc2d_ref.heads_fp32 / heads_bwd_fp32
restate the kernels' formulas in float32, in the kernels' order, and their largest error against the float64 reference over ALL
cases of HEAD_FWD_CASES and HEAD_BWD_CASES and both formats, measured on the CPU (test_misc2d_host.py repeats the measurement), is

    quantity         fp32 restatement   bound = 8 x (rounded up)   observed on an MI355X
    out              1.08e-07           8.7e-07                    1.08e-07
    out_mfma         8.41e-07           6.8e-06                    8.41e-07
    out_mfma_small   2.36e-06           1.9e-05                    2.36e-06
    dx               1.18e-07           9.5e-07                    4.70e-08
    dx_mfma          1.80e-07           1.5e-06                    9.99e-08
    dW               1.14e-07           9.2e-07                    1.14e-07
    dW_mfma          1.22e-07           9.8e-07                    1.22e-07

Observed: the largest error over the same cases on the device; for dx the smallest bound its 16-bit values would pass
(_misc2d_ref.least_allowance).  out and dW agree with the restatement to the digits shown, the small-weights case included: the MFMA
units keep fp16 subnormals.  The column sums' largest error was 5.96e-08 (bound 2^-23 = 1.19e-07).

"_mfma" are the cases with C = 64 and NJ <= 16, whose forward projection runs on the MFMA units with each float32 weight as two
16-bit terms hi + lo (their backward is the same code as the others': the split of the cases is kept so that every quantity has
the bound of its own cases).  out_mfma_small is the case with |W| ~ 1e-3: in the fp16 build lo falls into fp16 subnormals there and
keeps 3 bits or none, which the restatement models (torch's conversion keeps subnormals), hence the wider figure.  The kernel is
allowed 8 x the restatement's error: another summation order and another fma contraction cost a few ulp each."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _misc2d_ref as R
from _gpu_rows import SENTINEL, Rows, abi as _abi, dev as _dev, vec

pytestmark = pytest.mark.gpu

BUILDS = ("bf16", "fp16")
MM_ERR_ARG = -1
NAN = float("nan")
BYTE = 0xEE  # sentinel of the tap buffers

HEAD_BOUNDS = dict(out=8.7e-07, out_mfma=6.8e-06, out_mfma_small=1.9e-05, dx=9.5e-07, dx_mfma=1.5e-06, dW=9.2e-07, dW_mfma=9.8e-07)


def _fn(name, fmt):
    L, lib = _abi()
    return getattr(L, name if fmt == "bf16" else lib.H16_2D[name])


def _nan_ws(nbytes):
    return torch.full(((int(nbytes) + 3) // 4,), NAN, dtype=torch.float32, device=_dev())


def _map(a, ld, fmt, fill=NAN):
    """[B, H, W, C] (or None with a shape in ``a``) as pixel rows ``ld`` apart, 16 bytes into a wider buffer."""
    if isinstance(a, tuple):
        n, c, a = int(np.prod(a[:-1])), a[-1], None
    else:
        n, c = int(np.prod(a.shape[:-1])), a.shape[-1]
        a = a.reshape(n, c)
    return Rows(a, n, c, ld, 8, fill=fill, dtype=fmt)


# ------------------------------------------------------------------------------------------------------------------ max-pool
POOL_SHAPES = ((1, 1, 1), (1, 1, 7), (2, 2, 2), (1, 3, 3), (3, 4, 5), (2, 7, 8), (2, 15, 18))
POOL_CASES = {f"b{B}_{H}x{W}_c{C}_ld{ld}": dict(B=B, H=H, W=W, C=C, ld=ld)
              for B, H, W in POOL_SHAPES for C in (8, 64, 72) for ld in (C, C + 8)}


def pool_threads(c):
    return c["B"] * R.pooled(c["H"]) * R.pooled(c["W"]) * (c["C"] // 8)


@functools.lru_cache(maxsize=None)
def pool_inputs(name, kind, fmt):
    """The map of a case (its condition asserted by the maker) with its reference: made once, shared, never modified."""
    c = POOL_CASES[name]
    x = R.make_map(kind, (c["B"], c["H"], c["W"], c["C"]), 100 * list(POOL_CASES).index(name) + R.MAP_KINDS.index(kind), fmt)
    y, idx = R.maxpool(x)
    return dict(x=x, y=y, idx=idx)


def _pool_fwd(c, d, fmt):
    L, lib = _abi()
    B, H, W, C = d["x"].shape
    x = _map(d["x"], c["ld"], fmt)
    y = _map(d["y"].shape, C, fmt, fill=SENTINEL)
    idx = _map(d["idx"].shape, C, "u8", fill=BYTE)
    lib.check(_fn("mm_maxpool3x3s2_fwd", fmt)(x.ptr, c["ld"], B, H, W, C, y.ptr, idx.ptr, lib.stream()), "maxpool_fwd")
    torch.cuda.synchronize()
    return y, idx


@pytest.mark.parametrize("fmt", BUILDS)
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_maxpool_forward_values_and_taps_are_the_reference_bit_for_bit(name, fmt):
    c = POOL_CASES[name]
    for kind in R.MAP_KINDS:
        d = pool_inputs(name, kind, fmt)
        y, idx = _pool_fwd(c, d, fmt)
        assert y.padding_untouched() and idx.padding_untouched(), (name, kind)
        want = R.bits16(d["y"], fmt).reshape(-1, c["C"])
        bad = np.argwhere(y.bits() != want)
        assert not len(bad), f"{name} {kind}: {len(bad)} values differ, first at (pixel, channel) {bad[0]}"
        got = idx.bits()
        bad = np.argwhere(got != d["idx"].reshape(-1, c["C"]))
        assert not len(bad), (f"{name} {kind}: {len(bad)} taps differ, first at (pixel, channel) {bad[0]}: "
                              f"{got[tuple(bad[0])]} instead of {d['idx'].reshape(-1, c['C'])[tuple(bad[0])]}")


@pytest.mark.parametrize("fmt", BUILDS)
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_maxpool_backward_sums_the_selected_gradients(name, fmt):
    L, lib = _abi()
    c = POOL_CASES[name]
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    ld_dy, ld_dy2 = C + 8, C + 16
    for k, kind in enumerate(R.MAP_KINDS):
        d = pool_inputs(name, kind, fmt)
        _, idx = _pool_fwd(c, d, fmt)  # the forward's taps, as they lie on the device
        assert np.array_equal(idx.bits(), d["idx"].reshape(-1, C)), (name, kind)
        seed = 7000 + 10 * list(POOL_CASES).index(name) + k
        for grads in ("grid", "grid2", "normal2"):
            if grads.startswith("grid"):
                g1, g2 = R.make_grid(d["y"].shape, seed), R.make_grid(d["y"].shape, seed + 1)
            else:
                g1, g2 = R.make_map("normal", d["y"].shape, seed + 2, fmt), R.make_map("normal", d["y"].shape, seed + 3, fmt)
            if not grads.endswith("2"):
                g2 = None
            dy, dy2 = _map(g1, ld_dy, fmt), (None if g2 is None else _map(g2, ld_dy2, fmt))
            dx = _map((B, H, W, C), C, fmt, fill=SENTINEL)
            lib.check(_fn("mm_maxpool3x3s2_bwd", fmt)(dy.ptr, ld_dy, dy2.ptr if dy2 else None, ld_dy2 if dy2 else 0, idx.ptr, B, H, W, C,
                                                      dx.ptr, lib.stream()), "maxpool_bwd")
            torch.cuda.synchronize()
            what = f"{name} {kind} {grads}"
            assert dx.padding_untouched(), what
            s, a, n = (v.reshape(-1, C) for v in R.maxpool_bwd(g1, g2, d["idx"], H, W))
            assert n.sum() == d["idx"].size * (2 if g2 is not None else 1)
            got_bits = dx.bits()
            assert not got_bits[n == 0].any(), f"{what}: a pixel that no window selects is not +0"
            if grads.startswith("grid"):
                bad = np.argwhere(got_bits != R.bits16(s, fmt))
                assert not len(bad), f"{what}: {len(bad)} sums differ from the exact ones, first at (pixel, channel) {bad[0]}"
            else:
                ok = R.in_interval(dx.get(), s, 7 * 2.0 ** -24 * a, fmt)
                assert ok.all(), f"{what}: {(~ok).sum()} sums outside the interval of an 8-term float32 sum, first at {np.argwhere(~ok)[0]}"


# ------------------------------------------------------------------------------------------------------- concat, split, copy
CAT_PARTS = ((8,), (64,), (64, 128, 64), (64, 192, 64), (8, 8, 8, 8), (1024, 1024))


def cat_rows_per_block(parts):
    return (256 // (sum(parts) // 8)) * 8


def cat_ns(parts):
    r = cat_rows_per_block(parts)
    return (0, 1, r - 1, r, r + 1, 3001)


def _cat_part(n, parts, i):
    """Integers below 1020 (16-bit numbers in either format) that name their place in the wide row."""
    ct, off = sum(parts), sum(parts[:i])
    r, col = np.arange(n)[:, None], np.arange(parts[i])[None, :]
    return (((r * ct + off + col) * 7) % 2039 - 1019).astype(np.float64)  # 2039 is prime: rows less than 2039 apart differ


@pytest.mark.parametrize("parts", CAT_PARTS, ids=lambda p: "+".join(map(str, p)))
def test_concat_and_split_move_every_chunk_to_its_place(parts):
    L, lib = _abi()
    k, ct = len(parts), sum(parts)
    chans = (ctypes.c_int * k)(*parts)
    for n in cat_ns(parts):
        data = [_cat_part(n, parts, i) for i in range(k)]
        src = [Rows(data[i], n, parts[i], parts[i], 8, dtype="fp16") for i in range(k)]
        wide = Rows(None, n, ct, ct, 8, fill=SENTINEL, dtype="fp16")
        lib.check(L.mm_concat_bf16((ctypes.c_void_p * k)(*[s.ptr for s in src]), chans, k, wide.ptr, n, 0, lib.stream()), "concat")
        back = [Rows(None, n, parts[i], parts[i], 8, fill=SENTINEL, dtype="fp16") for i in range(k)]
        lib.check(L.mm_concat_bf16((ctypes.c_void_p * k)(*[b.ptr for b in back]), chans, k, wide.ptr, n, 1, lib.stream()), "split")
        torch.cuda.synchronize()
        assert wide.padding_untouched() and all(b.padding_untouched() for b in back), (parts, n)
        if n == 0:
            assert wide.untouched() and all(b.untouched() for b in back)
            continue
        want = np.concatenate(data, 1)
        bad = np.argwhere(wide.bits() != R.bits16(want, "fp16"))
        assert not len(bad), f"concat {parts} N = {n}: {len(bad)} elements differ, first at (row, channel) {bad[0]}"
        for i in range(k):
            assert np.array_equal(back[i].bits(), src[i].bits()), f"split {parts} N = {n}: part {i} is not restored"


@pytest.mark.parametrize("C", [8, 72])
def test_copy_rows_between_two_pitches(C):
    L, lib = _abi()
    ld_s, ld_d = C + 8, C + 16
    for n in (0, 1, 257):
        data = _cat_part(n, (C,), 0)
        src, dst = Rows(data, n, C, ld_s, 8, dtype="fp16"), Rows(None, n, C, ld_d, 8, fill=SENTINEL, dtype="fp16")
        lib.check(L.mm_copy_rows_bf16(src.ptr, ld_s, dst.ptr, ld_d, n, C, lib.stream()), "copy_rows")
        torch.cuda.synchronize()
        assert dst.padding_untouched(), (C, n)
        assert np.array_equal(dst.bits(), src.bits()), (C, n)


# --------------------------------------------------------------------------------------------------------------------- heads
HEAD_NJ = (1, 5, 8, 10, 12, 16, 20, 24, 32)
HEAD_CNJ = tuple((64, nj) for nj in HEAD_NJ) + tuple((c, nj) for c in (32, 128) for nj in (5, 12, 20))
HEAD_HW = ((1, 1), (2, 3), (4, 4), (5, 5), (16, 7), (17, 9), (33, 5))


def _head(C, NJ, B, Hp, Wp, h, w, ld=None, bias=True, scale=1.0):
    return dict(C=C, NJ=NJ, B=B, Hp=Hp, Wp=Wp, h=h, w=w, ld=ld or C, bias=bias, scale=scale)


def _head_fwd_cases():
    t, i = {}, 0
    for C, NJ in HEAD_CNJ:
        for h, w in HEAD_HW:
            for crop in (False, True):
                B = 1 if h * w < 16 else 1 + i % 3  # 1 and 6 pixels: below one MFMA group of 16; most other counts are no multiple of 16
                t[f"c{C}_nj{NJ}_{h}x{w}_{'crop' if crop else 'whole'}"] = _head(
                    C, NJ, B, h + 2 if crop else h, w + 3 if crop else w, h, w, C + 8 * (i % 2), bias=i % 4 < 2)
                i += 1
    t["small_weights_c64_nj12"] = _head(64, 12, 2, 19, 12, 17, 9, 72, scale=1.0 / 128)
    return t


HEAD_FWD_CASES = _head_fwd_cases()
HEAD_BWD_MAPS = ((1, 1, 1, 1, 1), (1, 1, 127, 1, 120), (2, 8, 8, 7, 6), (1, 3, 43, 3, 43), (3, 43, 1, 40, 1), (2, 20, 25, 18, 22))


def _head_bwd_cases():
    t = {}
    for i, NJ in enumerate(HEAD_NJ):
        for k, (B, Hp, Wp, h, w) in enumerate(HEAD_BWD_MAPS):
            t[f"nj{NJ}_p{B * Hp * Wp}_{h}x{w}"] = _head(64, NJ, B, Hp, Wp, h, w, 64 + 8 * ((i + k) % 2))
    t["capped_nj20"] = _head(64, 20, 1, 520, 512, 517, 509, 64)  # 2048 blocks of 130 pixels: 8 or 9 trips per pixel slot
    return t


HEAD_BWD_CASES = _head_bwd_cases()


def head_class(c, q):
    if c["scale"] != 1.0:
        return q + "_mfma_small"
    return q + "_mfma" if R.is_mfma(c["C"], c["NJ"]) else q


def _head_make(table, name, fmt):
    c = table[name]
    return R.make_heads(c["B"], c["Hp"], c["Wp"], c["C"], c["NJ"], c["h"], c["w"], 3000 + list(table).index(name), fmt, c["scale"], c["bias"])


@functools.lru_cache(maxsize=None)
def _head_small(table_is_fwd, name, fmt):
    return _head_make(HEAD_FWD_CASES if table_is_fwd else HEAD_BWD_CASES, name, fmt)


def head_fwd_inputs(name, fmt):
    return _head_small(True, name, fmt)


def head_bwd_inputs(name, fmt):
    """(The capped case is 136 MB in float64: made when asked for, not kept.)"""
    return _head_make(HEAD_BWD_CASES, name, fmt) if name.startswith("capped") else _head_small(False, name, fmt)


def _head_ws(c, fmt):
    return _nan_ws(_fn("mm_head_ws_bytes", fmt)(c["B"], c["h"], c["w"], c["Hp"], c["Wp"], c["C"], c["NJ"]))


OBSERVED = {}


def _note(key, v):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), v)
    print(f"{key}: {v:.3e} (bound {HEAD_BOUNDS[key]:.1e}, largest so far {OBSERVED[key]:.3e})")


def _run_head_fwd(c, d, fmt):
    L, lib = _abi()
    x = _map(d["x"], c["ld"], fmt)
    Wj, bias = vec(d["Wj"], fill=NAN), (vec(d["bias"], fill=NAN) if d["bias"] is not None else None)
    out, ws = vec(None, c["B"] * c["h"] * c["w"] * c["NJ"]), _head_ws(c, fmt)
    lib.check(_fn("mm_head_fwd", fmt)(x.ptr, c["B"], c["Hp"], c["Wp"], c["ld"], c["h"], c["w"], c["C"], Wj.ptr, bias.ptr if bias else None, c["NJ"],
                                      out.ptr, ws.data_ptr(), ws.numel() * 4, lib.stream()), "head_fwd")
    torch.cuda.synchronize()
    assert out.padding_untouched()
    return out.get().reshape(c["B"], c["h"], c["w"], c["NJ"])


@pytest.mark.parametrize("fmt", BUILDS)
@pytest.mark.parametrize("name", list(HEAD_FWD_CASES))
def test_head_forward_against_float64(name, fmt):
    c, d = HEAD_FWD_CASES[name], head_fwd_inputs(name, fmt)
    got = _run_head_fwd(c, d, fmt)
    assert np.isfinite(got).all(), f"{name}: a pixel outside the crop, padding or workspace garbage was read"
    ref, a = R.heads(d["x"], d["Wj"], d["bias"], c["h"], c["w"])
    key = head_class(c, "out")
    err = R.rel_error(got, ref, a)
    _note(key, err)
    assert err <= HEAD_BOUNDS[key], f"{name}: {key} {err:.3e} exceeds {HEAD_BOUNDS[key]:.1e}"


def _run_head_bwd(c, d, fmt):
    L, lib = _abi()
    n = c["B"] * c["Hp"] * c["Wp"]
    x = _map(d["x"], c["ld"], fmt)
    dx = Rows(None, n, c["C"], c["ld"], 8, fill=SENTINEL, dtype=fmt)
    Wj, dout = vec(d["Wj"], fill=NAN), vec(d["dout"], fill=NAN)
    dW, ws = vec(None, c["NJ"] * c["C"]), _head_ws(c, fmt)
    lib.check(_fn("mm_head_bwd", fmt)(x.ptr, c["B"], c["Hp"], c["Wp"], c["ld"], c["h"], c["w"], c["C"], Wj.ptr, c["NJ"], dout.ptr, dx.ptr,
                                      dW.ptr, ws.data_ptr(), ws.numel() * 4, lib.stream()), "head_bwd")
    torch.cuda.synchronize()
    assert dx.padding_untouched() and dW.padding_untouched()
    return dx, dW.get().reshape(c["NJ"], c["C"])


def _check_head_bwd(name, c, d, fmt, dx, dW):
    B, Hp, Wp, C, h, w = c["B"], c["Hp"], c["Wp"], c["C"], c["h"], c["w"]
    ref = R.heads_bwd(d["x"], d["Wj"], d["dout"], h, w, Hp, Wp)
    outside = np.ones((B, Hp, Wp), bool)
    outside[:, :h, :w] = False
    assert not dx.bits().reshape(B, Hp, Wp, C)[outside].any(), f"{name}: dx outside the crop is not +0"
    got = dx.get().reshape(B, Hp, Wp, C)
    assert np.isfinite(got).all() and np.isfinite(dW).all(), name
    kx, kw = head_class(c, "dx"), head_class(c, "dW")
    ok = R.in_interval(got, ref["dx"], HEAD_BOUNDS[kx] * ref["dx_abs"], fmt)
    _note(kx, R.least_allowance(got, ref["dx"], ref["dx_abs"], fmt))  # the smallest bound this dx would pass
    assert ok.all(), f"{name}: {(~ok).sum()} elements of dx outside [round16(ref - e), round16(ref + e)], first at {np.argwhere(~ok)[0]}"
    err = R.rel_error(dW, ref["dW"], ref["dW_abs"])
    _note(kw, err)
    assert err <= HEAD_BOUNDS[kw], f"{name}: {kw} {err:.3e} exceeds {HEAD_BOUNDS[kw]:.1e}"


@pytest.mark.parametrize("fmt", BUILDS)
@pytest.mark.parametrize("name", list(HEAD_BWD_CASES))
def test_head_backward_against_float64(name, fmt):
    c, d = HEAD_BWD_CASES[name], head_bwd_inputs(name, fmt)
    dx, dW = _run_head_bwd(c, d, fmt)
    _check_head_bwd(name, c, d, fmt, dx, dW)


# -------------------------------------------------------------------------------------------------------------------- colsum
COLSUM_C = (8, 64, 512, 2048)
COLSUM_CAPPED = (512, 2048 * 64 + 65)  # 2049 blocks of 64 rows wanted: past the cap of 2048 partials, 65 rows per block


def colsum_rows_per_block(C):
    return (256 // (C // 8)) * 16


def colsum_ns(C):
    r = colsum_rows_per_block(C)
    return (0, 1, r - 1, r, r + 1, 5 * r + 3)


def _colsum(fmt, data, n, C, ld, prev):
    L, lib = _abi()
    x = Rows(data, n, C, ld, 8, dtype=fmt)
    out = vec(prev) if prev is not None else vec(None, C)
    ws = _nan_ws(_fn("mm_bn2d_ws_bytes", fmt)(C))
    lib.check(_fn("mm_colsum_bf16", fmt)(x.ptr, ld, n, C, out.ptr, 0 if prev is None else 1, ws.data_ptr(), ws.numel() * 4, lib.stream()), "colsum")
    torch.cuda.synchronize()
    assert out.padding_untouched()
    return out.get()[0]


def _check_colsum(fmt, n, C, ld, seed):
    g = np.random.default_rng(seed)
    for acc in (0, 1):
        what = f"C = {C} N = {n} ld = {ld} accumulate = {acc}"
        grid, prev = R.make_grid((n, C), seed + acc), (R.make_grid((C,), seed + 2) if acc else None)
        got = _colsum(fmt, grid, n, C, ld, prev)
        want = grid.sum(0) + (prev if acc else 0.0)
        assert np.abs(grid).sum(0).max(initial=0) < 2 ** 21  # every partial sum is a float32 number
        assert np.array_equal(got, want), f"{what}: grid sums are not exact, first at column {np.flatnonzero(got != want)[:1]}"
        x = R.round16(g.standard_normal((n, C)), fmt)
        prev = g.standard_normal(C).astype(np.float32).astype(np.float64) if acc else None
        got = _colsum(fmt, x, n, C, ld, prev)
        if n == 0:
            assert np.array_equal(got, prev if acc else np.zeros(C)), what
        err = R.rel_error(got, x.sum(0) + (prev if acc else 0.0), np.abs(x).sum(0) + (np.abs(prev) if acc else 0.0))
        print(f"colsum {what}: {err:.3e}")
        assert err <= 2.0 ** -23, f"{what}: {err:.3e} of the column's abs_sum"


@pytest.mark.parametrize("fmt", BUILDS)
@pytest.mark.parametrize("C", COLSUM_C)
def test_colsum_against_float64(C, fmt):
    for i, n in enumerate(colsum_ns(C)):
        for ld in (C, C + 8):
            _check_colsum(fmt, n, C, ld, 5000 + 10 * i + C)


@pytest.mark.parametrize("fmt", BUILDS)
def test_colsum_past_the_cap_of_2048_partials(fmt):
    C, n = COLSUM_CAPPED
    assert -(-n // colsum_rows_per_block(C)) > 2048
    L, lib = _abi()
    g = torch.Generator().manual_seed(11)
    # made in 16 bits on the CPU (134 MB), summed in float64 by torch
    for kind in ("grid", "normal"):
        if kind == "grid":
            x = (torch.randint(-32, 33, (n, C), generator=g, dtype=torch.int16).float() / 8).to(R.FMT[fmt])
        else:
            x = torch.randn((n, C), generator=g).to(R.FMT[fmt])
        want, a = x.double().sum(0).numpy(), x.double().abs().sum(0).numpy()
        xd, out = x.to(_dev()), vec(None, C)
        ws = _nan_ws(_fn("mm_bn2d_ws_bytes", fmt)(C))
        lib.check(_fn("mm_colsum_bf16", fmt)(xd.data_ptr(), C, n, C, out.ptr, 0, ws.data_ptr(), ws.numel() * 4, lib.stream()), "colsum")
        torch.cuda.synchronize()
        got = out.get()[0]
        assert out.padding_untouched()
        if kind == "grid":
            assert a.max() < 2 ** 21 and np.array_equal(got, want), "capped: grid sums are not exact"
        else:
            err = R.rel_error(got, want, a)
            print(f"colsum capped: {err:.3e}")
            assert err <= 2.0 ** -23, f"capped: {err:.3e} of the column's abs_sum"


# ------------------------------------------------------------------------------------------------------- module-level wrappers
class _OneBuffer(torch.autograd.Function):
    """Hands the two heads' outputs gradients that are the halves of ONE [B, h, w, 2 nc] buffer, as lifting's backward does."""

    @staticmethod
    def forward(ctx, o1, o2, g):
        ctx.g = g
        return (o1 * g.permute(0, 3, 1, 2)[:, :o1.shape[1]]).sum() + (o2 * g.permute(0, 3, 1, 2)[:, o1.shape[1]:]).sum()

    @staticmethod
    def backward(ctx, up):
        v = ctx.g.permute(0, 3, 1, 2)
        nc = v.shape[1] // 2
        return v[:, :nc], v[:, nc:], None


@pytest.mark.parametrize("one_buffer", [False, True], ids=["two_gradients", "one_buffer"])
@pytest.mark.parametrize("nc", [5, 10, 16])
def test_fused_heads_module_against_float64(nc, one_buffer, half2d):
    from mm2d3d_amd import nn2d

    fmt = "fp16" if half2d == torch.float16 else "bf16"
    dev = _dev()
    B, C, Hp, Wp, h, w = 2, 64, 12, 20, 11, 18
    d = R.make_heads(B, Hp, Wp, C, 2 * nc, h, w, 40 + nc, fmt)
    xin = np.nan_to_num(d["x"], nan=3.0)  # the module's map has numbers outside the crop; they must not matter
    x = torch.from_numpy(xin).permute(0, 3, 1, 2).to(half2d).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    c1, c2 = nn2d.Conv2d(64, nc, 1).to(dev), nn2d.Conv2d(64, nc, 1).to(dev)
    with torch.no_grad():
        for m, lo in ((c1, 0), (c2, nc)):
            m.weight.copy_(torch.from_numpy(d["Wj"][lo:lo + nc]).reshape(nc, C, 1, 1))
            m.bias.copy_(torch.from_numpy(d["bias"][lo:lo + nc]))
    o1, o2 = nn2d.fused_heads(x, h, w, c1, c2)
    got = torch.cat([o1, o2], 1).detach().permute(0, 2, 3, 1).double().cpu().numpy()
    ref, a = R.heads(d["x"], d["Wj"], d["bias"], h, w)
    c = dict(C=C, NJ=2 * nc, scale=1.0)
    key = head_class(c, "out")
    err = R.rel_error(got, ref, a)
    assert err <= HEAD_BOUNDS[key], f"out: {err:.3e} exceeds {HEAD_BOUNDS[key]:.1e}"
    g = torch.from_numpy(d["dout"]).float().to(dev)  # [B, h, w, 2 nc]
    if one_buffer:
        _OneBuffer.apply(o1, o2, g).backward()
    else:
        gp = g.permute(0, 3, 1, 2)
        ((o1 * gp[:, :nc].contiguous()).sum() + (o2 * gp[:, nc:].contiguous()).sum()).backward()
    rb = R.heads_bwd(d["x"], d["Wj"], d["dout"], h, w, Hp, Wp)
    dx = x.grad.permute(0, 2, 3, 1).double().cpu().numpy()
    assert not dx[:, h:].any() and not dx[:, :, w:].any()
    ok = R.in_interval(dx, rb["dx"], HEAD_BOUNDS[head_class(c, "dx")] * rb["dx_abs"], fmt)
    assert ok.all(), f"{(~ok).sum()} elements of dx outside their interval"
    dW = torch.cat([c1.weight.grad, c2.weight.grad], 0).reshape(2 * nc, C).double().cpu().numpy()
    kw = head_class(c, "dW")
    err = R.rel_error(dW, rb["dW"], rb["dW_abs"])
    assert err <= HEAD_BOUNDS[kw], f"dW: {err:.3e} exceeds {HEAD_BOUNDS[kw]:.1e}"
    # the bias gradients are a float32 sum of B * h * w numbers in an order of torch's: at most n roundings of 2^-24 of the abs_sum
    db = torch.cat([c1.bias.grad, c2.bias.grad], 0).double().cpu().numpy()
    err = R.rel_error(db, d["dout"].sum((0, 1, 2)), np.abs(d["dout"]).sum((0, 1, 2)))
    assert err <= B * h * w * 2.0 ** -24, f"dbias: {err:.3e}"


def test_fused_heads_refuses_more_than_32_outputs(half2d):
    from mm2d3d_amd import nn2d

    dev = _dev()
    x = torch.zeros(1, 64, 4, 4, device=dev).to(half2d).contiguous(memory_format=torch.channels_last)
    c1, c2 = nn2d.Conv2d(64, 17, 1).to(dev), nn2d.Conv2d(64, 17, 1).to(dev)
    with pytest.raises(RuntimeError, match="rc=-1"):
        nn2d.fused_heads(x, 4, 4, c1, c2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- refused arguments
@pytest.mark.parametrize("fmt", BUILDS)
def test_refusals_come_before_any_launch(fmt):
    """Every call here is refused with MM_ERR_ARG and a message, and has written nothing.  Nothing is launched; the buffers are
    nevertheless large enough for every call, had it been accepted by mistake."""
    L, lib = _abi()
    s = lib.stream()
    B, Hp, Wp, C = 1, 4, 4, 64
    x = Rows(None, 64, 512, 520, 8, fill=1.0, dtype=fmt)  # 64 pixels of up to 512 channels
    Wj, bias, dout = vec(None, 33 * 512, fill=0.5), vec(None, 64, fill=0.5), vec(None, 8192, fill=0.5)
    out, dW = vec(None, 8192), vec(None, 33 * 512)
    dx = Rows(None, 64, 512, 520, 8, fill=SENTINEL, dtype=fmt)
    ws = _nan_ws(_fn("mm_head_ws_bytes", fmt)(2, 8, 8, 8, 8, 512, 33))
    fwd, bwd = _fn("mm_head_fwd", fmt), _fn("mm_head_bwd", fmt)

    def head_fwd(xp=x.ptr, Hp=Hp, Wp=Wp, ld=C, h=4, w=4, C=C, NJ=12):
        return fwd(xp, B, Hp, Wp, ld, h, w, C, Wj.ptr, bias.ptr, NJ, out.ptr, ws.data_ptr(), ws.numel() * 4, s)

    def head_bwd(xp=x.ptr, dxp=dx.ptr, Hp=Hp, Wp=Wp, ld=C, h=4, w=4, C=C, NJ=12):
        return bwd(xp, B, Hp, Wp, ld, h, w, C, Wj.ptr, NJ, dout.ptr, dxp, dW.ptr, ws.data_ptr(), ws.numel() * 4, s)

    pool_y, pool_dx = Rows(None, 64, 64, 64, 8, fill=SENTINEL, dtype=fmt), Rows(None, 64, 64, 64, 8, fill=SENTINEL, dtype=fmt)
    pool_idx = Rows(None, 64, 64, 64, 8, fill=BYTE, dtype="u8")
    pfwd, pbwd = _fn("mm_maxpool3x3s2_fwd", fmt), _fn("mm_maxpool3x3s2_bwd", fmt)

    def pool_fwd(xp=x.ptr, yp=pool_y.ptr, ld=64):
        return pfwd(xp, ld, 1, 4, 4, 64, yp, pool_idx.ptr, s)

    def pool_bwd(dyp=x.ptr, dy2p=None, dxp=pool_dx.ptr, ld=64, ld2=0):
        return pbwd(dyp, ld, dy2p, ld2, pool_idx.ptr, 1, 4, 4, 64, dxp, s)

    calls = {
        "head_fwd h > Hp": lambda: head_fwd(h=5), "head_fwd w > Wp": lambda: head_fwd(w=5), "head_fwd ld < C": lambda: head_fwd(ld=56),
        "head_fwd ld % 8": lambda: head_fwd(ld=68), "head_fwd x alignment": lambda: head_fwd(xp=x.ptr + 8),
        "head_fwd NJ > 32": lambda: head_fwd(NJ=33), "head_fwd NJ * C * 4 > 60 KB": lambda: head_fwd(C=512, ld=512, NJ=32),
        "head_fwd C % 8": lambda: head_fwd(C=60),
        "head_bwd h > Hp": lambda: head_bwd(h=5), "head_bwd w > Wp": lambda: head_bwd(w=5), "head_bwd ld < C": lambda: head_bwd(ld=56),
        "head_bwd ld % 8": lambda: head_bwd(ld=68), "head_bwd x alignment": lambda: head_bwd(xp=x.ptr + 8),
        "head_bwd dx alignment": lambda: head_bwd(dxp=dx.ptr + 8), "head_bwd NJ > 32": lambda: head_bwd(NJ=33),
        "head_bwd C = 32": lambda: head_bwd(C=32), "head_bwd C = 128": lambda: head_bwd(C=128, ld=128),
        "maxpool_fwd x alignment": lambda: pool_fwd(xp=x.ptr + 8), "maxpool_fwd y alignment": lambda: pool_fwd(yp=pool_y.ptr + 8),
        "maxpool_fwd ld < C": lambda: pool_fwd(ld=56), "maxpool_fwd ld % 8": lambda: pool_fwd(ld=68),
        "maxpool_bwd dy alignment": lambda: pool_bwd(dyp=x.ptr + 8), "maxpool_bwd dy2 alignment": lambda: pool_bwd(dy2p=x.ptr + 8, ld2=64),
        "maxpool_bwd dx alignment": lambda: pool_bwd(dxp=pool_dx.ptr + 8), "maxpool_bwd ld_dy % 8": lambda: pool_bwd(ld=68),
        "maxpool_bwd ld_dy < C": lambda: pool_bwd(ld=56),
    }
    parts = (ctypes.c_void_p * 5)(*[x.ptr] * 5)
    wide = Rows(None, 64, 2056, 2056, 8, fill=SENTINEL, dtype=fmt)
    for what, chans in (("concat 0 parts", ()), ("concat 5 parts", (8,) * 5), ("concat C % 8", (8, 12)), ("concat 2056 channels", (1024, 1032))):
        calls[what] = lambda chans=chans: L.mm_concat_bf16(parts, (ctypes.c_int * 5)(*chans), len(chans), wide.ptr, 16, 0, s)
    wrong = {}
    for what, call in calls.items():
        rc = int(call())
        msg = L.mm_last_error() or b""
        if rc != MM_ERR_ARG or what.split("_")[0].split(" ")[0].encode() not in msg:
            wrong[what] = (rc, msg)
    torch.cuda.synchronize()
    assert not wrong, f"not refused with MM_ERR_ARG and a message of their own: {wrong}"
    assert all(b.untouched() for b in (out, dW, dx, pool_y, pool_dx, pool_idx, wide)), "a refused call has written"
