"""The host half of the GPU JPEG decoder (mm2d3d_amd/jpeg.py) against Pillow, and a numpy restatement of what csrc/jpeg.hip
computes - libjpeg-turbo's Huffman decode (jdhuff.c), DC prediction, jidctint.c jpeg_idct_islow, jdsample.c fancy upsampling
and jdcolor.c ycc_rgb_convert - equal to ``np.asarray(Image.open(f))`` bit for bit.  No GPU needed.  JPEGs are encoded here
with PIL from seeded arrays."""
import io
import os
import tempfile

import numpy as np
import pytest
from PIL import Image

from mm2d3d_amd import jpeg

QUALITIES = (5, 50, 90, 100)
SIZES = ((1, 1), (7, 9), (15, 17), (16, 16), (17, 33), (160, 90), (192, 121))
SMALL = ((1, 1), (7, 9), (15, 17), (16, 16), (17, 33), (40, 23))


def texture(W, H, kind="noise", seed=0):
    """uint8 [H][W][3] test images: smooth + noise, uniform noise, flat, hard 0/255 edges."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (H, W, 3)).copy()
    if kind == "edges":
        y, x = np.mgrid[:H, :W]
        a = np.where(((x // 3 + y // 5) % 2)[..., None] == 0, 0, 255).astype(np.uint8)
        return np.repeat(a, 3, 2) ^ np.array([0, 255, 0], np.uint8)
    y, x = np.mgrid[:H, :W]  # "smooth": gradients plus a little noise
    a = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 127 // max(W + H - 2, 1)], -1)
    return np.clip(a + rng.integers(-8, 9, a.shape), 0, 255).astype(np.uint8)


def encode(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a, "RGB").save(b, "JPEG", **kw)
    return b.getvalue()


def pil(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def matrix():
    """(id, encoder keywords) of the parser / decoder matrix."""
    cases = [(f"q{q}-s{s}", dict(quality=q, subsampling=s)) for q in QUALITIES for s in (0, 1, 2)]
    cases += [("opt-s2", dict(quality=75, subsampling=2, optimize=True)), ("opt-s0", dict(quality=95, subsampling=0, optimize=True)),
              ("rst-blocks", dict(quality=90, subsampling=2, restart_marker_blocks=1)),
              ("rst-rows", dict(quality=90, subsampling=1, restart_marker_rows=1)),
              ("rst-blocks3-opt", dict(quality=80, subsampling=0, restart_marker_blocks=3, optimize=True)),
              ("qt-ones", dict(qtables=[[1] * 64, [1] * 64], subsampling=2)),
              ("qt-255", dict(qtables=[[255] * 64, [255] * 64], subsampling=1))]
    return cases


# ---------------------------------------------------------------------------------------------------- numpy restatement
def entropy_intervals(seg):
    """Unstuffed restart intervals of an entropy-coded segment (FF 00 -> FF, fill FF dropped, split at RST0-7)."""
    out, cur, i = [], bytearray(), 0
    while i < len(seg):
        b = seg[i]
        if b == 0xFF:
            nx = seg[i + 1] if i + 1 < len(seg) else 0xFF
            if nx == 0x00:
                cur.append(0xFF)
                i += 2
            elif 0xD0 <= nx <= 0xD7:
                out.append(bytes(cur))
                cur = bytearray()
                i += 2
            else:
                i += 1
            continue
        cur.append(b)
        i += 1
    out.append(bytes(cur))
    return out


class Bits:
    """MSB-first bit reader over one interval; bits past its end read as 0 (libjpeg's fill after a marker)."""

    def __init__(self, data):
        self.d, self.n, self.pos = bytes(data) + b"\0" * 8, len(data) * 8, 0

    def peek(self, k):
        p = self.pos >> 3
        w = int.from_bytes(self.d[p : p + 5], "big") if p < len(self.d) else 0
        return (w >> (40 - (self.pos & 7) - k)) & ((1 << k) - 1)

    def get(self, k):
        v = self.peek(k) if k else 0
        self.pos += k
        return v


def huff_decode(bits, t):
    """One symbol with the device table layout of jpeg.huff_table (fast 9-bit lookup, then maxcode / valoffset)."""
    w = bits.peek(16)
    e = int(t[w >> 7])
    if e:
        bits.pos += e >> 8
        return e & 255
    for l in range(10, 17):
        code = w >> (16 - l)
        if code <= t[512 + l]:
            bits.pos += l
            return int(t[548 + ((code + t[530 + l]) & 255)])
    raise ValueError("invalid Huffman code")


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(data):
    """(header, int32 [blocks][64] natural-order coefficients with predicted DC, blocks in scan order) - jdhuff.c
    decode_mcu_slow for every MCU, DC predictors reset at every restart interval."""
    h = jpeg.parse(data)
    assert h.reason is None, h.reason
    bpm, mx, my, n_iv, _ = jpeg.geometry(h)
    hs, vs = h.components[0][1], h.components[0][2]
    comp_of_slot = [0] * (hs * vs) + [1, 2]
    tabs = [(jpeg.huff_table(*h.dc[td]), jpeg.huff_table(*h.ac[ta])) for _, td, ta in h.scan]
    ivs = entropy_intervals(data[h.entropy[0] : h.entropy[1]])
    assert len(ivs) == n_iv
    nmcu = mx * my
    per = h.restart or nmcu
    coef = np.zeros((nmcu * bpm, 64), np.int32)
    blk = 0
    for iv, raw in enumerate(ivs):
        bits = Bits(raw)
        pred = [0, 0, 0]
        for _ in range(min(per, nmcu - iv * per)):
            for slot in range(bpm):
                c = comp_of_slot[slot]
                dct, act = tabs[c]
                s = huff_decode(bits, dct)
                pred[c] += extend(bits.get(s), s)
                coef[blk, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = huff_decode(bits, act)
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        coef[blk, jpeg.ZIGZAG[min(k, 63)]] = extend(bits.get(s), s)
                    elif r != 15:
                        break
                    else:
                        k += 15
                    k += 1
                blk += 1
        assert bits.pos <= bits.n, "ran past the end of the interval"
    return h, coef


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_1d(x, shift):
    """jidctint.c jpeg_idct_islow, one pass over axis 1 of x int64 [N][8][...]; results DESCALEd by ``shift``."""
    C = 13
    z2, z3 = x[:, 2], x[:, 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[:, 0] + x[:, 4]) << C
    tmp1 = (x[:, 0] - x[:, 4]) << C
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x[:, 7], x[:, 5], x[:, 3], x[:, 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([descale(o, shift) for o in out], 1)


def idct_islow(coef, q):
    """uint8 [N][8][8] samples of int32 [N][64] natural-order coefficients dequantised by q [64] (natural order)."""
    d = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)  # [N][row v][col u]
    ws = idct_1d(d, 13 - 2)  # pass 1: columns (axis 1 = v), PASS1_BITS 2
    out = idct_1d(ws.transpose(0, 2, 1), 13 + 2 + 3).transpose(0, 2, 1)  # pass 2: rows
    v = ((out & 1023) ^ 512) - 512  # range_limit[x & RANGE_MASK] with CENTERJSAMPLE = clamp of the wrapped value + 128
    return np.clip(v + 128, 0, 255).astype(np.uint8)


def planes(h, coef):
    """The three component planes (uint8, whole MCUs) of the decoded blocks."""
    bpm, mx, my, _, _ = jpeg.geometry(h)
    hs, vs = h.components[0][1], h.components[0][2]
    blocks = coef.reshape(my, mx, bpm, 64)
    out = []
    for c, (ci, _, _) in enumerate(h.scan):
        q = jpeg.quant_natural(h.qtables[h.components[ci][3]])
        if c == 0:
            b = blocks[:, :, : hs * vs].reshape(my, mx, vs, hs, 64)
            px = idct_islow(b.reshape(-1, 64), q).reshape(my, mx, vs, hs, 8, 8)
            out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8))
        else:
            px = idct_islow(blocks[:, :, hs * vs + c - 1].reshape(-1, 64), q).reshape(my, mx, 8, 8)
            out.append(px.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return out


def upsample(p, W, H, hs, vs):
    """jdsample.c: fullsize, h2v1 / h2v2 fancy (downsampled width > 2) or box upsampling of a chroma plane to [H][W]."""
    p = p.astype(np.int32)
    dw, dh = -(-W // hs), -(-H // vs)
    p = p[:dh, :dw]
    if hs == 1:
        return p[:H, :W]
    if dw <= 2:  # h2v1_upsample / h2v2_upsample
        return np.repeat(np.repeat(p, vs, 0), 2, 1)[:H, :W]
    if vs == 2:
        y = np.arange(H)
        near = p[y >> 1]
        far = p[np.clip(np.where(y & 1, (y >> 1) + 1, (y >> 1) - 1), 0, dh - 1)]  # jdmainct.c context rows replicate the edges
        cs = near * 3 + far
        prev, nxt = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        even = (cs * 3 + prev + 8) >> 4
        even[:, 0] = (cs[:, 0] * 4 + 8) >> 4
        odd = (cs * 3 + nxt + 7) >> 4
        odd[:, -1] = (cs[:, -1] * 4 + 7) >> 4
    else:
        prev, nxt = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
        even = (p * 3 + prev + 1) >> 2
        even[:, 0] = p[:, 0]
        odd = (p * 3 + nxt + 2) >> 2
        odd[:, -1] = p[:, -1]
    return np.stack([even, odd], 2).reshape(even.shape[0], -1)[:H, :W]


def ycc_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert with build_ycc_rgb_table's fixed-point tables (SCALEBITS 16)."""
    y, xb, xr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * xr + 32768) >> 16)
    g = y + ((-46802 * xr + (-22554 * xb + 32768)) >> 16)
    b = y + ((116130 * xb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """The restated decoder: uint8 [H][W][3]."""
    h, coef = coefficients(data)
    W, H = h.size
    hs, vs = h.components[0][1], h.components[0][2]
    yp, cbp, crp = planes(h, coef)
    return ycc_rgb(yp[:H, :W], upsample(cbp, W, H, hs, vs), upsample(crp, W, H, hs, vs))


# ---------------------------------------------------------------------------------------------------- the parser
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("case,kw", matrix(), ids=[c for c, _ in matrix()])
def test_parser_agrees_with_pil(case, kw, size):
    data = encode(texture(*size, kind="smooth", seed=size[0]), **kw)
    im = Image.open(io.BytesIO(data))
    h = jpeg.parse(data)
    assert h.reason is None
    assert h.size == im.size
    assert [(c[0], c[1], c[2], c[3]) for c in h.components] == [tuple(l) for l in im.layer]
    assert not im.info.get("progressive") and not h.progressive
    assert {k: list(jpeg.quant_natural(v)) for k, v in h.qtables.items()} == {k: list(v) for k, v in im.quantization.items()}
    first, end = h.entropy
    assert data[first - 2 : first] != b"" and data[end : end + 2] == b"\xff\xd9"
    if "restart_marker_blocks" in kw or "restart_marker_rows" in kw:
        assert h.restart > 0
        bpm, mx, my, n_iv, _ = jpeg.geometry(h)
        assert len(entropy_intervals(data[first:end])) == n_iv
    else:
        assert h.restart == 0


def test_parser_routes_ineligible_files_to_the_host():
    a = texture(40, 24, seed=1)
    assert jpeg.parse(encode(a, progressive=True)).reason == "progressive"
    b = io.BytesIO()
    Image.fromarray(a[..., 0], "L").save(b, "JPEG")
    assert jpeg.parse(b.getvalue()).reason == "1 components"
    # 4:4:0 (luma 1x2): Pillow cannot write it; patch the luma sampling byte of a 4:4:4 file's SOF (the header is all we read)
    d = bytearray(encode(a, subsampling=0))
    sof = d.index(b"\xff\xc0")
    assert d[sof + 11] == 0x11
    d[sof + 11] = 0x12
    assert jpeg.parse(bytes(d)).reason.startswith("sampling factors")
    b = io.BytesIO()
    Image.fromarray(a, "RGB").convert("CMYK").save(b, "JPEG")
    assert jpeg.parse(b.getvalue()).reason == "4 components"


def test_parser_rejects_truncated_and_inconsistent_files():
    d = encode(texture(40, 24, seed=2), quality=80)
    for cut in (len(d) - 2, len(d) // 2, 300, 30):
        with pytest.raises(ValueError, match="x.jpg"):
            jpeg.parse(d[:cut], "x.jpg")
    # a scan that names a Huffman table no DHT defined
    sos = d.index(b"\xff\xda")
    bad = bytearray(d)
    bad[sos + 6] = 0x23
    with pytest.raises(ValueError, match="referenced but not defined"):
        jpeg.parse(bytes(bad), "x.jpg")


def test_parser_rejects_a_huffman_table_with_an_all_ones_code():
    """jdhuff.c jpeg_make_d_derived_tbl rejects a table whose codes fill every bit pattern of their longest length (PIL
    cannot decode such a file, so neither may the GPU path)."""
    d = bytearray(encode(texture(16, 16, seed=3), quality=80))
    dht = d.index(b"\xff\xc4")
    bits = d[dht + 5 : dht + 21]  # the first table of the segment: DC luma, 12 codes of lengths 2..9
    assert sum(bits) == 12
    bits = bytes([1] * 10 + [2] + [0] * 5)  # 0, 10, 110, ..., 1111111110, then 11111111110 and the all-ones 11111111111
    d[dht + 5 : dht + 21] = bits
    with pytest.raises(ValueError, match="code overflow"):
        jpeg.parse(bytes(d), "x.jpg")
    with pytest.raises(Exception):
        pil(bytes(d))


def test_huffman_tables_decode_every_code():
    """Every code of an optimised table (lengths up to 16 bits) through the fast table and the maxcode / valoffset path."""
    bits = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3]  # one code per length 2..15, three of 16 bits
    vals = list(range(1, 18))
    t = jpeg.huff_table(bits, vals)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            b = Bits(((code << (32 - l)) | ((1 << (32 - l)) - 1)).to_bytes(4, "big"))
            assert huff_decode(b, t) == vals[k] and b.pos == l
            code, k = code + 1, k + 1
        code <<= 1


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("size", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
@pytest.mark.parametrize("case,kw", matrix(), ids=[c for c, _ in matrix()])
def test_restated_decoder_equals_pil(case, kw, size):
    data = encode(texture(*size, kind="smooth", seed=size[1]), **kw)
    assert np.array_equal(decode(data), pil(data))


@pytest.mark.parametrize("kind", ["noise", "flat", "edges"])
@pytest.mark.parametrize("s", [0, 1, 2])
def test_restated_decoder_equals_pil_on_hard_textures(kind, s):
    """Uniform noise (long codes, ZRL, FF bytes in the data), flat (DC-only blocks), 0/255 edges (range limit)."""
    for q in (50, 100):
        data = encode(texture(37, 29, kind=kind, seed=s), quality=q, subsampling=s)
        if kind == "noise" and q == 100:
            assert b"\xff\x00" in data[jpeg.parse(data).entropy[0] :]
        assert np.array_equal(decode(data), pil(data)), (kind, q)


def test_restated_decoder_equals_pil_on_the_loader_fixtures():
    root = os.path.join(os.path.dirname(__file__), "golden", "mini_ds")
    for sub in ("nuscenes", "a2d2"):
        for dp, _, fs in os.walk(os.path.join(root, sub)):
            for f in sorted(fs)[:2]:
                if f.endswith(".jpg"):
                    data = open(os.path.join(dp, f), "rb").read()
                    assert jpeg.parse(data).reason is None
                    assert np.array_equal(decode(data), pil(data)), f


# ---------------------------------------------------------------------------------------------------- host plumbing
def test_plan_routes_and_offsets_for_a_mixed_batch():
    """Eligible JPEGs go to the GPU decoder; a progressive JPEG, a PNG and a JPEG whose header the parser rejects go to the host
    decode; each image gets its place in the source buffer in batch order, as imageprep.build_tables expects."""
    from mm2d3d_amd import dataprep, imageprep

    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, (fmt, kw, size) in enumerate([("JPEG", dict(quality=90), (48, 32)), ("JPEG", dict(progressive=True), (40, 24)),
                                             ("PNG", {}, (16, 8)), ("JPEG", dict(quality=70, subsampling=0), (33, 17)),
                                             ("JPEG", dict(quality=90), (24, 16))]):
            p = os.path.join(d, f"{i}.{fmt.lower()}")
            Image.fromarray(texture(*size, seed=i), "RGB").save(p, fmt, **kw)
            paths.append(p)
        with open(paths[4], "rb") as f:  # no EOI: the header parser rejects it, PIL keeps deciding what happens to it
            data = f.read()
        with open(paths[4], "wb") as f:
            f.write(data[: len(data) - 40])
        plans = [imageprep.ImagePlan(Image.open(p)) for p in paths]
        route = dataprep.read_jpegs(plans)[2]
        assert [r.reason is None if r is not None else None for r in route] == [True, False, None, True, False]
        assert route[1].reason == "progressive" and route[4].reason.startswith("header: ") and "4.jpeg" in route[4].reason
        offs = dataprep.source_offsets(plans)
        sizes = [48 * 32 * 3, 40 * 24 * 3, 16 * 8 * 3, 33 * 17 * 3, 24 * 16 * 3]
        assert list(offs) == list(np.concatenate([[0], np.cumsum(sizes)[:-1]]))
