"""Host half of ``gpu_batch(image="gpu")`` (mm2d3d_amd/imageprep.py) against Pillow, on the CPU.

The kernels of csrc/imageprep.hip restate Pillow's libImaging arithmetic; here the same restatements in numpy are pinned
against PIL itself: the Q22 coefficient tables + two int32 passes against ``Image.resize(..., BILINEAR)``, and RGB -> L,
``Image.blend``, RGB -> HSV and HSV -> RGB over all 2^24 colours.  The LUT and the plan-recording front ends are checked
against the host path (tests/test_loader_golden.CASES)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from mm2d3d_amd import imageprep

import test_loader_golden as tlg

RESIZES = [((1600, 900), (400, 225)), ((1920, 1208), (480, 302)), ((317, 143), (96, 60)), ((40, 24), (96, 60)), ((123, 77), (123, 40)),
           ((200, 100), (199, 100))]


# ---------------------------------------------------------------------------------------------------- numpy restatements
def np_resize(src, plan):
    """Resample.c for an ImagePlan over ``src`` uint8 [H][W][3]: horizontal pass over the rows the vertical pass reads,
    then the vertical pass, int32 accumulators from 1 << 21, clip(acc >> 22)."""
    l, t, r, b = plan.window
    win = src[t:b, l:r].astype(np.int32)
    hb, hk, vb, vk, y0, rows = imageprep.plan_coeffs(plan)
    win = win[y0 : y0 + rows]

    def one_pass(img, bounds, kk, axis):
        n_in = img.shape[axis]
        acc = np.full(img.shape[:axis] + (len(bounds),) + img.shape[axis + 1 :], 1 << 21, np.int32)
        for j in range(kk.shape[1]):
            idx = np.minimum(bounds[:, 0] + j, n_in - 1)
            w = np.where(j < bounds[:, 1], kk[:, j], 0).astype(np.int32)
            shape = [1, 1, 1]
            shape[axis] = len(bounds)
            acc += np.take(img, idx, axis=axis) * w.reshape(shape)
        return np.clip(acc >> 22, 0, 255)

    return one_pass(one_pass(win, hb, hk, 1), vb, vk, 0).astype(np.uint8)


def np_luma(rgb):
    rgb = rgb.astype(np.int64)
    return ((rgb[..., 0] * 19595 + rgb[..., 1] * 38470 + rgb[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def np_blend(a, b, f):
    f = np.float32(f)
    t = a.astype(np.float32) + f * (b.astype(np.int32) - a.astype(np.int32)).astype(np.float32)
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def np_rgb2hsv(rgb):
    r, g, b = (rgb[..., c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(np.float32)
        s = cr / mx.astype(np.float32)
        rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
        f64 = lambda x: x.astype(np.float64)
        h = np.where(r == mx, bc - gc, np.where(g == mx, (2.0 + f64(rc) - f64(bc)).astype(np.float32),
                                                 (4.0 + f64(gc) - f64(rc)).astype(np.float32)))
        h = np.fmod(f64(h) / 6.0 + 1.0, 1.0).astype(np.float32)
        H = np.clip(np.trunc(f64(h) * 255.0), 0, 255)
        S = np.clip(np.trunc(f64(s) * 255.0), 0, 255)
    same = mx == mn
    return np.stack([np.where(same, 0, H), np.where(same, 0, S), mx], -1).astype(np.uint8)


def c_round(x):  # C round(): half away from zero (x >= 0 here)
    fl = np.floor(x)
    return fl + (x - fl >= 0.5)


def np_hsv2rgb(hsv):
    h, s, v = (hsv[..., c].astype(np.float64) for c in range(3))
    h6 = h * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(np.float32)
    fs = (s / 255.0).astype(np.float32)
    p = np.clip(c_round(v * (1.0 - fs.astype(np.float64))), 0, 255)
    q = np.clip(c_round(v * (1.0 - (fs * f).astype(np.float64))), 0, 255)
    t = np.clip(c_round(v * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))), 0, 255)
    i = i.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(hsv.shape, np.float64)
    for k, chans in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(i == k, chans[c], out[..., c])
    out = np.where((hsv[..., 1] == 0)[..., None], v[..., None], out)
    return out.astype(np.uint8)


def all_colours():
    """A 4096x4096 RGB image holding each of the 2^24 colours once."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.fixture(scope="module")
def colours():
    return all_colours()


def _random_image(w, h, seed):
    rng = np.random.default_rng(seed)
    # smooth gradients plus noise: interpolation and rounding both matter
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7) % 256], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("src_size,dst_size", RESIZES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in RESIZES])
def test_resize_tables_and_int32_passes_equal_pil(src_size, dst_size):
    a = _random_image(*src_size, seed=src_size[0])
    im = Image.fromarray(a, "RGB")
    ref = np.asarray(im.resize(dst_size, Image.BILINEAR))
    got = np_resize(a, imageprep.ImagePlan(im).resize(dst_size, Image.BILINEAR))
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("box,dst_size", [((13, 7, 301, 131), (96, 60)), ((0, 40, 160, 90), (40, 24)), ((5, 0, 60, 30), (120, 70))])
def test_crop_then_resize_equals_pil(box, dst_size):
    a = _random_image(317, 143, seed=5)
    im = Image.fromarray(a, "RGB")
    ref = np.asarray(im.crop(box).resize(dst_size, Image.BILINEAR))
    plan = imageprep.ImagePlan(im).crop(box)
    assert plan.size == (box[2] - box[0], box[3] - box[1])
    got = np_resize(a, plan.resize(dst_size, Image.BILINEAR))
    assert np.array_equal(got, ref)


def test_crop_only_and_untouched_plans_copy_the_window():
    a = _random_image(64, 40, seed=1)
    im = Image.fromarray(a, "RGB")
    assert np.array_equal(np_resize(a, imageprep.ImagePlan(im)), a)
    assert np.array_equal(np_resize(a, imageprep.ImagePlan(im).crop((3, 30, 50, 40))), a[30:40, 3:50])


def test_plan_refuses_what_it_cannot_record():
    im = Image.fromarray(_random_image(64, 40, seed=2), "RGB")
    p = imageprep.ImagePlan(im).resize((32, 20), Image.BILINEAR)
    with pytest.raises(NotImplementedError):
        p.crop((0, 0, 8, 8))
    with pytest.raises(NotImplementedError):
        imageprep.ImagePlan(im).resize((32, 20), Image.NEAREST)
    with pytest.raises(NotImplementedError):
        imageprep.ImagePlan(im).crop((-1, 0, 8, 8))
    with pytest.raises(NotImplementedError, match="image='host'"):
        imageprep.ImagePlan(im.convert("L"))


# ---------------------------------------------------------------------------------------------------- pointwise operations
def test_luma_equals_pil(colours):
    ref = np.asarray(Image.fromarray(colours, "RGB").convert("L"))
    assert np.array_equal(np_luma(colours), ref)


@pytest.mark.parametrize("f", [0.0, 0.37, 0.6000000238418579, 1.0, 1.0000001192092896, 1.3999999761581421, 1.7, -0.25, 2.5])
def test_blend_equals_pil(f):
    """Every (a, b) byte pair in each channel, factors inside and outside [0, 1]."""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    A = np.stack([a, b, (a + b) % 256], -1).astype(np.uint8)
    Bm = np.stack([b, a, (a * 7 + b) % 256], -1).astype(np.uint8)
    ref = np.asarray(Image.blend(Image.fromarray(A, "RGB"), Image.fromarray(Bm, "RGB"), f))
    assert np.array_equal(np_blend(A, Bm, f), ref)


@pytest.mark.parametrize("f", [0.6000000238418579, 1.3999999761581421])
def test_enhance_operations_equal_pil_over_all_colours(colours, f):
    im = Image.fromarray(colours, "RGB")
    L = np_luma(colours)[..., None]
    assert np.array_equal(np_blend(np.zeros_like(colours), colours, f), np.asarray(ImageEnhance.Brightness(im).enhance(f)))
    assert np.array_equal(np_blend(np.broadcast_to(L, colours.shape), colours, f), np.asarray(ImageEnhance.Color(im).enhance(f)))
    mean = int(L.astype(np.int64).sum() / L.size + 0.5)
    assert np.array_equal(np_blend(np.full_like(colours, mean), colours, f), np.asarray(ImageEnhance.Contrast(im).enhance(f)))


def test_rgb_to_hsv_equals_pil(colours):
    ref = np.asarray(Image.fromarray(colours, "RGB").convert("HSV"))
    assert np.array_equal(np_rgb2hsv(colours), ref)


def test_hsv_to_rgb_equals_pil(colours):
    chans = [Image.fromarray(np.ascontiguousarray(colours[..., c]), "L") for c in range(3)]
    ref = np.asarray(Image.merge("HSV", chans).convert("RGB"))
    assert np.array_equal(np_hsv2rgb(colours), ref)


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("norm", [None, tlg.NORM])
def test_lut_equals_the_host_float_conversion_and_normalisation(norm):
    from mm2d3d_amd.datasets import _Scenes

    ds = _Scenes()
    ds.image_normalizer = norm
    ds.color_jitter = None
    lut = imageprep.lut(ds._to_float, ds._normalise)
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    img = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, 2)
    ref = ds._normalise(ds._float_image(Image.fromarray(img, "RGB")))[0]  # [256][3]
    assert np.array_equal(lut.T, ref)


def test_jitter_ops_follow_the_drawn_order():
    ops, n, npre, f, hue = imageprep.jitter_ops(([2, 1, 0, 3], [np.float32(0.7).item(), np.float32(1.2).item(), None, None]))
    assert (ops & 15, (ops >> 4) & 15, n, npre, hue) == (1, 0, 2, 0, 0)
    ops, n, npre, f, hue = imageprep.jitter_ops(([3, 0, 2, 1], [None, None, np.float32(0.9).item(), np.float32(-0.1).item()]))
    assert (ops & 15, (ops >> 4) & 15, n, npre, hue) == (3, 2, 2, 2, int(np.float32(-0.1).item() * 255) % 256)


# ---------------------------------------------------------------------------------------------------- plan-recording front ends
@pytest.mark.parametrize("name", sorted(tlg.CASES))
def test_plan_front_end_equals_the_pil_front_end(name):
    """The front end with image plans: same points, pixel coordinates, intrinsics, keep mask, image size and RNG states as
    with PIL images, and the plan's window + resize applied to the decoded image (numpy restatement) = the PIL image."""
    z = np.load(os.path.join(tlg.G, f"loader_{name}.npz"))
    ds, _ = tlg._dataset(name)
    idx = [int(i) for i in z["indices"]]

    def run(plans):
        np.random.seed(int(z["seed"]))
        torch.manual_seed(int(z["seed"]))
        ds._plan_images = plans
        try:
            ws = [ds._front(i) for i in idx]
        finally:
            ds._plan_images = False
        return ws, np.random.get_state(), torch.get_rng_state()

    host, hs, ht = run(False)
    plan, ps, pt = run(True)
    assert all(a == b if not isinstance(a, np.ndarray) else np.array_equal(a, b) for a, b in zip(hs, ps)) and torch.equal(ht, pt)
    for h, p in zip(host, plan):
        assert isinstance(p.image, imageprep.ImagePlan)
        for k in ("points", "cam", "pimg", "label", "intr", "keep"):
            tlg._same(getattr(p, k), getattr(h, k), k)
        assert p.image.size == h.image.size
        got = np_resize(np.asarray(p.image.image), p.image)
        assert np.array_equal(got, np.asarray(h.image)), name
