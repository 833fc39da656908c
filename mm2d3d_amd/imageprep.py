"""Host side of the camera-image preparation on the GPU (``gpu_batch(..., image="gpu")``; csrc/imageprep.hip).

The host path of the loaders opens the camera image with PIL, crops and resizes it (``datasets._apply_window`` /
``datasets._resize``), applies the colour jitter (``color_jitter.ColorJitter``), converts to float, flips and normalises.
The GPU path keeps everything that decides WHAT is done on the host and moves the per-pixel work to three kernels:

    host                                                   device (csrc/imageprep.hip, one launch each over the batch)
    ---------------------------------------------------    ------------------------------------------------------------
    ImagePlan: header only (size), one integer source      1. horizontal BILINEAR pass, uint8 -> uint8, only the source rows
       window, at most one target size                        the vertical pass reads
    jitter / flip / 3D draws in the host path's order      2. vertical pass + the jitter operations before Contrast
    decode (PIL, a few threads) into one pinned buffer,       + per-scene int64 sums of L (the Contrast mean)
       one H2D copy                                         3. Contrast + the remaining operations, [3][256] LUT (float
    Q22 resize coefficients, per-scene LUT                     conversion + normalisation), fliplr, NCHW fp32 store

Every step is the arithmetic of Pillow 12 (libImaging/Resample.c, Blend.c, Convert.c) and of numpy's float32 rules, so the
batch equals the host path's bit for bit (tests/test_imageprep_host.py pins the tables and restatements against PIL on the
CPU; tests/test_gpu_imageprep.py the kernels against PIL).
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

PRECISION_BITS = 22  # Resample.c: 32 - 8 bits of the pixel - 2 bits of headroom
DESC_FIELDS = 16     # int64 words per scene of the descriptor table (include/mm2d3d.h, MM_IMG_*)
# descriptor word indices (include/mm2d3d.h)
(D_SRC_OFF, D_SRC_PITCH, D_WIN_W, D_WIN_H, D_TMP_ROWS, D_YBOX_FIRST, D_KX, D_KY, D_HCOEF, D_VCOEF, D_TMP_OFF, D_OPS, D_NOPS, D_NPRE,
 D_HUE_SHIFT, D_FLIP) = range(DESC_FIELDS)


class ImagePlan:
    """A camera image that is opened (header read) but not decoded, with the crop / resize the front end asked for.

    Exposes the part of the PIL surface ``datasets._apply_window`` / ``_resize`` / ``_crop`` use: ``size``, ``crop(box)``,
    ``resize(size, BILINEAR)``.  Records one integer source window (left, top, right, bottom) and at most one target size."""

    __slots__ = ("image", "window", "target")

    def __init__(self, image, window=None, target=None):
        if image.mode != "RGB":
            raise NotImplementedError(f"gpu_batch(image='gpu') decodes RGB images only (got mode {image.mode!r}): use image='host'")
        self.image = image
        self.window = window if window is not None else (0, 0) + tuple(image.size)
        self.target = target

    @property
    def size(self):
        if self.target is not None:
            return self.target
        l, t, r, b = self.window
        return (r - l, b - t)

    def crop(self, box):
        if self.target is not None:
            raise NotImplementedError("ImagePlan: a crop after a resize is not supported (no dataset does that)")
        l, t, r, b = (int(v) for v in box)
        if tuple(box) != (l, t, r, b):
            raise NotImplementedError("ImagePlan: crop boxes must be integers")
        W, H = self.size
        if not (0 <= l < r <= W and 0 <= t < b <= H):
            raise NotImplementedError(f"ImagePlan: crop box {box} leaves the {W}x{H} image (PIL would pad): use image='host'")
        ol, ot = self.window[:2]
        return ImagePlan(self.image, (ol + l, ot + t, ol + r, ot + b))

    def resize(self, size, resample=None):
        from PIL import Image

        if resample != Image.BILINEAR:
            raise NotImplementedError("ImagePlan: only the BILINEAR filter is implemented")
        if self.target is not None:
            raise NotImplementedError("ImagePlan: one resize per image")
        return ImagePlan(self.image, self.window, (int(size[0]), int(size[1])))


# ---------------------------------------------------------------------------------------------------- resize coefficients
def resize_coeffs(in_size, out_size, in0=0.0, in1=None):
    """``precompute_coeffs`` + ``normalize_coeffs_8bpc`` of Pillow's Resample.c for the BILINEAR filter (support 1), all in
    float64 as there.  Returns (bounds int32 [out][2] = (first source index, tap count), kk int32 [out][ksize] in Q22)."""
    in1 = float(in_size) if in1 is None else float(in1)
    scale = (in1 - float(in0)) / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = float(in0) + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)  # C's (int) truncates
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None]
    w = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((w < 1.0) & (x < xmax[:, None]), 1.0 - w, 0.0)
    ww = np.zeros(out_size)
    for j in range(ksize):  # Resample.c sums in tap order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    q = w * (1 << PRECISION_BITS)
    kk = np.where(q < 0, np.trunc(-0.5 + q), np.trunc(0.5 + q)).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return bounds, kk


def identity_coeffs(n):
    """One tap of weight 1.0 per output index: the pass reproduces its input exactly ((v << 22) + (1 << 21)) >> 22 = v."""
    return np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], 1), np.full((n, 1), 1 << PRECISION_BITS, np.int32)


def plan_coeffs(plan):
    """(hbounds, hkk, vbounds, vkk, ybox_first, tmp_rows) of one plan; vbounds already shifted by ybox_first (Resample.c
    ImagingResampleInner).  An unchanged axis gets the identity coefficients."""
    l, t, r, b = plan.window
    win_w, win_h = r - l, b - t
    out_w, out_h = plan.size
    hb, hk = resize_coeffs(win_w, out_w) if out_w != win_w else identity_coeffs(win_w)
    vb, vk = resize_coeffs(win_h, out_h) if out_h != win_h else identity_coeffs(win_h)
    ybox_first = int(vb[0, 0])
    ybox_last = int(vb[-1, 0] + vb[-1, 1])
    vb = vb.copy()
    vb[:, 0] -= ybox_first
    return hb, hk, vb, vk, ybox_first, ybox_last - ybox_first


# ---------------------------------------------------------------------------------------------------- per-scene tables
def lut(float_image, normalise):
    """[3][256] fp32: the host path's ``normalise(np.array(u8_image, float32) / 255.0)`` for every byte value per channel."""
    v = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)[None]  # a 1x256 RGB image holding every value in every channel
    return np.ascontiguousarray(np.asarray(normalise(float_image(v)), dtype=np.float32)[0].T)


def jitter_ops(draw):
    """(ops packed 4 bits each in drawn order, count, count before Contrast, factors fp32 [4], hue shift) of one
    ``ColorJitter.draw()`` (None: no jitter)."""
    factors = np.zeros(4, np.float32)
    if draw is None:
        return 0, 0, 0, factors, 0
    order, f = draw
    ops = [op for op in order if f[op] is not None]
    packed = 0
    for j, op in enumerate(ops):
        packed |= op << (4 * j)
        factors[op] = np.float32(f[op])
        if float(factors[op]) != f[op]:
            raise ValueError("jitter factors are float32 draws")
    n_pre = ops.index(1) if 1 in ops else len(ops)
    hue = int(f[3] * 255) % 256 if f[3] is not None else 0
    return packed, len(ops), n_pre, factors, hue


def decode_into(plans, staging, threads=4):
    """Decode every plan's image into ``staging`` (uint8, images back to back, each [H][W][3]) with ``threads`` workers
    (Pillow releases the GIL while it decodes).  Returns the byte offset of each image."""
    sizes = [p.image.size[0] * p.image.size[1] * 3 for p in plans]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if offs[-1] > staging.size:
        raise ValueError("decode_into: staging buffer too small")

    def one(i):
        a = np.asarray(plans[i].image)
        if a.dtype != np.uint8 or a.shape != (plans[i].image.size[1], plans[i].image.size[0], 3):
            raise NotImplementedError(f"gpu_batch(image='gpu') decodes 8-bit RGB images only (got {a.dtype} {a.shape}): use image='host'")
        staging[offs[i] : offs[i + 1]] = a.reshape(-1)

    threads = max(1, int(threads))
    if threads == 1 or len(plans) == 1:
        for i in range(len(plans)):
            one(i)
    else:
        with ThreadPoolExecutor(max_workers=min(threads, len(plans))) as ex:
            list(ex.map(one, range(len(plans))))
    return offs[:-1]


def build_tables(plans, draws, flips, luts, src_offs):
    """Descriptor int64 [B][DESC_FIELDS], coefficient table int32, factors fp32 [B][4], LUTs fp32 [B][3][256] and the
    temp size (bytes) of the horizontal pass, for plans whose images sit at ``src_offs`` of the staging buffer."""
    B = len(plans)
    desc = np.zeros((B, DESC_FIELDS), np.int64)
    factors = np.zeros((B, 4), np.float32)
    coef, coef_len, tmp = [], 0, 0
    out_size = plans[0].size
    for b, p in enumerate(plans):
        if p.size != out_size:
            raise ValueError("gpu_batch: every image of a batch must come out at the same size")
        W = p.image.size[0]
        l, t, r, bt = p.window
        hb, hk, vb, vk, y0, rows = plan_coeffs(p)
        ops, nops, npre, f, hue = jitter_ops(draws[b])
        d = desc[b]
        d[D_SRC_OFF] = int(src_offs[b]) + (t * W + l) * 3
        d[D_SRC_PITCH] = W * 3
        d[D_WIN_W], d[D_WIN_H] = r - l, bt - t
        d[D_TMP_ROWS], d[D_YBOX_FIRST] = rows, y0
        d[D_KX], d[D_KY] = hk.shape[1], vk.shape[1]
        d[D_HCOEF] = coef_len
        coef += [hb.reshape(-1), hk.reshape(-1)]
        coef_len += hb.size + hk.size
        d[D_VCOEF] = coef_len
        coef += [vb.reshape(-1), vk.reshape(-1)]
        coef_len += vb.size + vk.size
        d[D_TMP_OFF] = tmp
        tmp += rows * out_size[0] * 3
        d[D_OPS], d[D_NOPS], d[D_NPRE], d[D_HUE_SHIFT], d[D_FLIP] = ops, nops, npre, hue, 1 if flips[b] else 0
        factors[b] = f
    return desc, np.concatenate(coef).astype(np.int32), factors, np.ascontiguousarray(np.stack(luts), np.float32), tmp
