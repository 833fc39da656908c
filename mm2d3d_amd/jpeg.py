"""Host side of the baseline-JPEG decoder on the GPU (``gpu_batch(..., image="gpu")``; csrc/jpeg.hip).

The host reads each camera file into one pinned buffer and parses its header (the marker segments up to SOS); the GPU does
everything from the entropy-coded bytes on: unstuffing, restart-marker location, Huffman decode, DC prediction, the islow
IDCT, fancy upsampling and the YCbCr -> RGB conversion of libjpeg-turbo, the library Pillow decodes JPEGs with.  The batch
equals ``np.asarray(Image.open(path))`` bit for bit.

Eligible for the GPU decoder (:func:`parse` returns ``reason=None``): SOF0 / SOF1, 8-bit samples, Huffman coding, three
components that libjpeg reads as YCbCr, one scan that interleaves all three in frame order (Ss 0, Se 63, Ah = Al = 0), luma
sampling (1,1), (2,1) or (2,2) and chroma (1,1), 8-bit quantisation tables, any restart interval.  Every other file keeps the
host decode; the choice is made from the header alone.  A file that is truncated or inconsistent raises ``ValueError``.
"""
from __future__ import annotations

import os
import struct

import numpy as np

DESC_FIELDS = 32  # int64 words per image of the descriptor table (include/mm2d3d.h, MM_JPG_*)
(J_SEG_OFF, J_SEG_LEN, J_W, J_H, J_HS, J_VS, J_MCUS_X, J_MCUS_Y, J_RESTART, J_N_IV, J_IV0, J_SUB0, J_SUB_CAP, J_BLK0, J_PLANE_OFF,
 J_OUT_OFF, J_QT0, J_QT1, J_QT2, J_DC0, J_DC1, J_DC2, J_AC0, J_AC1, J_AC2) = range(25)
SUBSEQ_BITS = 2048  # bits of entropy-coded data per decoding lane (csrc/jpeg.hip SUBSEQ_BITS)
HUFF_WORDS = 1024   # int32 words per Huffman table: fast[512], maxcode[18], valoffset[18], huffval[256], padding
FAST_BITS = 9

# zigzag index -> natural index (jutils.c jpeg_natural_order)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63], np.int32)

_SOF_OTHER = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential", 0xC6: "differential progressive",
              0xC7: "differential lossless", 0xC9: "arithmetic coding", 0xCA: "progressive arithmetic coding",
              0xCB: "lossless arithmetic coding", 0xCD: "differential arithmetic coding",
              0xCE: "differential progressive arithmetic coding", 0xCF: "differential lossless arithmetic coding"}


class JpegHeader:
    """What :func:`parse` found: ``size`` (W, H), ``components`` [(id, h, v, tq)], ``qtables`` {id: 64 values in zigzag order},
    ``dc`` / ``ac`` {id: (bits[16], huffval)}, ``scan`` [(component index, td, ta)], ``restart`` (MCUs per interval, 0 =
    none), ``entropy`` (first byte, end byte) of the entropy-coded segment, ``reason`` (None = eligible for the GPU decoder,
    else why not), ``progressive``."""

    __slots__ = ("size", "components", "qtables", "qbits", "dc", "ac", "scan", "restart", "entropy", "reason", "progressive", "sof",
                 "jfif", "adobe_transform")

    def __init__(self):
        self.size, self.components, self.qtables, self.qbits, self.dc, self.ac = None, [], {}, {}, {}, {}
        self.scan, self.restart, self.entropy, self.reason, self.progressive, self.sof = [], 0, None, None, False, None
        self.jfif, self.adobe_transform = False, None

    @property
    def sampling(self):
        return tuple((h, v) for _, h, v, _ in self.components)

    def mcus(self):
        hs, vs = self.components[0][1], self.components[0][2]
        W, H = self.size
        return -(-W // (8 * hs)), -(-H // (8 * vs))


def _ineligible(hdr, reason):
    if hdr.reason is None:
        hdr.reason = reason


def parse(data, path="<bytes>"):
    """Parses the marker segments of a JPEG file (``bytes`` / ``memoryview`` / uint8 array) up to SOS and finds the end of
    the entropy-coded segment.  Returns a :class:`JpegHeader`; raises ``ValueError`` naming ``path`` for a truncated or
    inconsistent file."""
    buf = memoryview(data).cast("B") if not isinstance(data, np.ndarray) else memoryview(np.ascontiguousarray(data, np.uint8))
    n = len(buf)

    def bad(msg):
        raise ValueError(f"{path}: {msg}")

    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        bad("not a JPEG file (no SOI)")
    hdr = JpegHeader()
    p = 2
    while True:
        while p < n and buf[p] != 0xFF:  # libjpeg skips garbage before a marker (with a warning)
            p += 1
        while p < n and buf[p] == 0xFF:
            p += 1
        if p >= n:
            bad("file ends before the scan (no SOS)")
        m = buf[p]
        p += 1
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            bad("EOI before the scan")
        if p + 2 > n:
            bad(f"segment of marker {m:#04x} truncated")
        L = (buf[p] << 8) | buf[p + 1]
        if L < 2 or p + L > n:
            bad(f"segment of marker {m:#04x} truncated")
        seg = bytes(buf[p + 2 : p + L])
        p += L
        if m in (0xC0, 0xC1):
            _sof(hdr, m, seg, bad)
        elif m in _SOF_OTHER:
            hdr.progressive = m in (0xC2, 0xCA)
            _ineligible(hdr, _SOF_OTHER[m])
            _sof(hdr, m, seg, bad)
        elif m == 0xDB:
            _dqt(hdr, seg, bad)
        elif m == 0xC4:
            _dht(hdr, seg, bad)
        elif m == 0xCC:
            _ineligible(hdr, "arithmetic coding")
        elif m == 0xDD:
            if len(seg) < 2:
                bad("DRI truncated")
            hdr.restart = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            hdr.jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            hdr.adobe_transform = seg[11]
        elif m == 0xDA:
            _sos(hdr, seg, bad)
            hdr.entropy = (p, _entropy_end(buf, p, bad))
            break
    _check(hdr, bad)
    return hdr


def _sof(hdr, m, seg, bad):
    if hdr.sof is not None:
        bad("two frame headers")
    hdr.sof = m
    if len(seg) < 6:
        bad("SOF truncated")
    P, H, W, nf = struct.unpack(">BHHB", seg[:6])
    if len(seg) < 6 + 3 * nf:
        bad("SOF truncated")
    if H == 0 or W == 0:
        bad(f"bad image size {W}x{H}")
    hdr.size = (W, H)
    for i in range(nf):
        cid, hv, tq = seg[6 + 3 * i : 9 + 3 * i]
        h, v = hv >> 4, hv & 15
        if not (1 <= h <= 4 and 1 <= v <= 4) or tq > 3:
            bad("bad component parameters in SOF")
        hdr.components.append((cid, h, v, tq))
    if P != 8:
        _ineligible(hdr, f"{P}-bit samples")
    if nf != 3:
        _ineligible(hdr, f"{nf} components")


def _dqt(hdr, seg, bad):
    i = 0
    while i < len(seg):
        pq, tq = seg[i] >> 4, seg[i] & 15
        size = 128 if pq else 64
        if tq > 3 or pq > 1 or i + 1 + size > len(seg):
            bad("bad DQT segment")
        if pq:
            q = np.frombuffer(seg[i + 1 : i + 1 + size], ">u2").astype(np.int32)
        else:
            q = np.frombuffer(seg[i + 1 : i + 1 + size], np.uint8).astype(np.int32)
        hdr.qtables[tq] = q
        hdr.qbits[tq] = 16 if pq else 8
        i += 1 + size


def _dht(hdr, seg, bad):
    i = 0
    while i < len(seg):
        if i + 17 > len(seg):
            bad("bad DHT segment")
        tc, th = seg[i] >> 4, seg[i] & 15
        bits = list(seg[i + 1 : i + 17])
        count = sum(bits)
        if tc > 1 or th > 3 or count > 256 or i + 17 + count > len(seg):
            bad("bad DHT segment")
        vals = list(seg[i + 17 : i + 17 + count])
        (hdr.ac if tc else hdr.dc)[th] = (bits, vals)
        i += 17 + count


def _sos(hdr, seg, bad):
    if hdr.sof is None:
        bad("SOS before the frame header")
    if len(seg) < 1 or len(seg) < 1 + 2 * seg[0] + 3:
        bad("SOS truncated")
    ns = seg[0]
    ids = [c[0] for c in hdr.components]
    for j in range(ns):
        cid, t = seg[1 + 2 * j], seg[2 + 2 * j]
        if cid not in ids:
            bad(f"scan component {cid} is not in the frame")
        hdr.scan.append((ids.index(cid), t >> 4, t & 15))
    ss, se, a = seg[1 + 2 * ns : 4 + 2 * ns]
    if hdr.reason is None and (ss, se, a) != (0, 63, 0):
        _ineligible(hdr, "spectral selection / successive approximation")


def _entropy_end(buf, start, bad):
    """End (exclusive) of the entropy-coded segment: the first marker after SOS that is not RST0-7.  It must be EOI: a DHT /
    SOS / DNL there means a second scan (such files go to the host decode, see :func:`_check`)."""
    a = np.frombuffer(buf, np.uint8, offset=start)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nxt = a[ff + 1]
    mk = ff[(nxt != 0x00) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    if mk.size == 0:
        bad("the scan is not terminated (no EOI)")
    return start + int(mk[0]) if a[mk[0] + 1] == 0xD9 else -(start + int(mk[0]))


def _check(hdr, bad):
    if hdr.reason is not None:  # tables are checked for the files this decoder reads
        hdr.entropy = (hdr.entropy[0], abs(hdr.entropy[1]))
        return
    for cid, h, v, tq in hdr.components:
        if tq not in hdr.qtables:
            bad(f"quantisation table {tq} is referenced but not defined")
    for ci, td, ta in hdr.scan:
        if td not in hdr.dc or ta not in hdr.ac:
            bad(f"Huffman table {td}/{ta} is referenced but not defined")
    first, end = hdr.entropy
    if end < 0:
        _ineligible(hdr, "more than one scan")
        hdr.entropy = (first, -end)
    if [c for c, _, _ in hdr.scan] != [0, 1, 2]:
        _ineligible(hdr, "not one scan interleaving all three components in frame order")
    cids = tuple(c[0] for c in hdr.components)
    ycc = hdr.jfif or (hdr.adobe_transform != 0 if hdr.adobe_transform is not None else cids != (82, 71, 66))
    if not ycc:
        _ineligible(hdr, "RGB colour space (Adobe transform 0 or component ids R, G, B)")
    s = hdr.sampling
    if s[0] not in ((1, 1), (2, 1), (2, 2)) or s[1] != (1, 1) or s[2] != (1, 1):
        _ineligible(hdr, f"sampling factors {s}")
    if abs(end) - first >= 1 << 28:  # csrc/jpeg.hip keeps bit positions in int
        _ineligible(hdr, "entropy-coded segment of 256 MiB or more")
    if any(hdr.qbits[c[3]] != 8 for c in hdr.components):
        _ineligible(hdr, "16-bit quantisation table")
    for _, td, ta in hdr.scan:
        for tab, dc in ((hdr.dc[td], True), (hdr.ac[ta], False)):
            _check_table(tab, dc, bad)


def _check_table(tab, dc, bad):
    """jdhuff.c jpeg_make_d_derived_tbl's checks: codes must fit their lengths with the all-ones code unused; DC symbols <= 15."""
    bits, vals = tab
    code = 0
    for l in range(1, 17):
        code += bits[l - 1]
        if code >= (1 << l):  # jpeg_make_d_derived_tbl: an all-ones code is invalid
            bad("bad Huffman table (code overflow)")
        code <<= 1
    if dc and any(v > 15 for v in vals):
        bad("bad Huffman table (DC symbol > 15)")


# ---------------------------------------------------------------------------------------------------- device tables
def huff_table(bits, vals):
    """int32 [HUFF_WORDS]: fast[2^9] = (length << 8 | symbol) for codes of at most 9 bits, 0 otherwise; then libjpeg's
    maxcode[0..17] (maxcode[17] = sentinel) and valoffset[0..17] (jdhuff.c jpeg_make_d_derived_tbl), then huffval[256]."""
    t = np.zeros(HUFF_WORDS, np.int32)
    fast, maxcode, valoff, hv = t[:512], t[512:530], t[530:548], t[548:804]
    hv[: len(vals)] = vals
    maxcode[:] = -1
    code, k = 0, 0
    for l in range(1, 17):
        nb = bits[l - 1]
        if nb:
            valoff[l] = k - code
            for _ in range(nb):
                if l <= FAST_BITS:
                    lo = code << (FAST_BITS - l)
                    fast[lo : lo + (1 << (FAST_BITS - l))] = (l << 8) | vals[k]
                code += 1
                k += 1
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0x7FFFFFFF
    return t


def quant_natural(q):
    """The 64 zigzag-ordered DQT values in natural (row-major) order."""
    out = np.zeros(64, np.int32)
    out[ZIGZAG] = q
    return out


def geometry(hdr):
    """(blocks per MCU, MCUs x, MCUs y, intervals, bytes of the three component planes) of an eligible header."""
    hs, vs = hdr.components[0][1], hdr.components[0][2]
    mx, my = hdr.mcus()
    n_iv = -(-(mx * my) // hdr.restart) if hdr.restart else 1
    plane = mx * hs * 8 * my * vs * 8 + 2 * mx * 8 * my * 8
    return hs * vs + 2, mx, my, n_iv, plane


def build_tables(headers, data_offs, out_offs):
    """Descriptor int64 [B][DESC_FIELDS], Huffman tables int32 [T][HUFF_WORDS], quantisation tables int32 [Q][64] (natural
    order) and the totals (intervals, lane slots, blocks, plane bytes) for eligible ``headers`` whose files sit at
    ``data_offs`` of the data buffer and whose RGB output goes to ``out_offs`` of the source buffer."""
    B = len(headers)
    desc = np.zeros((B, DESC_FIELDS), np.int64)
    huff, qt = [], []
    n_iv = n_sub = n_blk = n_plane = 0
    for b, h in enumerate(headers):
        d = desc[b]
        first, end = h.entropy
        bpm, mx, my, niv, plane = geometry(h)
        d[J_SEG_OFF], d[J_SEG_LEN] = int(data_offs[b]) + first, end - first
        d[J_W], d[J_H] = h.size
        d[J_HS], d[J_VS] = h.components[0][1], h.components[0][2]
        d[J_MCUS_X], d[J_MCUS_Y] = mx, my
        d[J_RESTART], d[J_N_IV], d[J_IV0] = h.restart, niv, n_iv
        cap = -(-(end - first) * 8 // SUBSEQ_BITS) + niv
        d[J_SUB0], d[J_SUB_CAP] = n_sub, cap
        d[J_BLK0], d[J_PLANE_OFF], d[J_OUT_OFF] = n_blk, n_plane, int(out_offs[b])
        n_iv, n_sub, n_blk, n_plane = n_iv + niv, n_sub + cap, n_blk + mx * my * bpm, n_plane + plane
        for c, (ci, td, ta) in enumerate(h.scan):
            d[J_QT0 + c] = len(qt)
            qt.append(quant_natural(h.qtables[h.components[ci][3]]))
            d[J_DC0 + c] = len(huff)
            huff.append(huff_table(*h.dc[td]))
            d[J_AC0 + c] = len(huff)
            huff.append(huff_table(*h.ac[ta]))
    return desc, np.stack(huff).astype(np.int32), np.stack(qt).astype(np.int32), (n_iv, n_sub, n_blk, n_plane)


def jpeg_file(image):
    """The path of a PIL image that was opened from a JPEG file, else None."""
    if getattr(image, "format", None) != "JPEG":
        return None
    fn = getattr(image, "filename", None)
    return fn if isinstance(fn, (str, os.PathLike)) and fn and os.path.isfile(fn) else None


def read_into(path, view):
    """Reads the file at ``path`` into the uint8 array ``view`` (exactly its size)."""
    with open(path, "rb", buffering=0) as f:
        got = f.readinto(memoryview(view))
    if got != view.size:
        raise ValueError(f"{path}: read {got} of {view.size} bytes")
