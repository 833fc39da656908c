"""csrc/imageprep.hip against Pillow on an MI355X: every kernel operation over all 2^24 colours, the BILINEAR resize sweep,
and ``gpu_batch(image="gpu")`` against the reference fixtures and against ``gpu_batch(image="host")``."""
import importlib.util
import os
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

import test_imageprep_host as hostp
import test_loader_golden as tlg
from mm2d3d_amd import dataprep, imageprep
from mm2d3d_amd.color_jitter import ColorJitter

pytestmark = pytest.mark.gpu
IDENTITY_LUT = np.repeat(np.arange(256, dtype=np.float32)[None], 3, 0)  # img = the uint8 value, as float


def _f32(x):
    return float(np.float32(x))


def _run(plans, draws, flips=None):
    """prepare_images with the identity LUT -> uint8 [B][H][W][3] on the host."""
    flips = flips or [False] * len(plans)
    img = dataprep.prepare_images(plans, draws, flips, [IDENTITY_LUT] * len(plans), "cuda")
    out = img.permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(out, np.round(out)) and out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def _one_op(op, f):
    fs = [None] * 4
    fs[op] = f
    return ([op] + [o for o in range(4) if o != op], fs)


@pytest.fixture(scope="module")
def colours():
    return Image.fromarray(hostp.all_colours(), "RGB")


def test_luma_and_blends_equal_pil_over_all_colours(colours):
    plan = imageprep.ImagePlan(colours)
    L = np.asarray(colours.convert("L"))
    got = _run([plan], [_one_op(2, 0.0)])[0]  # Color at factor 0 = the L image
    assert np.array_equal(got, np.repeat(L[..., None], 3, 2)), "L"
    for f in (_f32(0.6), 1.0, _f32(1.4), _f32(0.0), _f32(1.75)):
        for op, cls in ((0, ImageEnhance.Brightness), (1, ImageEnhance.Contrast), (2, ImageEnhance.Color)):
            got = _run([plan], [_one_op(op, f)])[0]
            assert np.array_equal(got, np.asarray(cls(colours).enhance(f))), (cls.__name__, f)


def test_hue_round_trip_equals_pil_over_all_colours(colours):
    cj = ColorJitter(hue=0.5)
    for f in (0.0, _f32(0.1), _f32(-0.25), _f32(0.49)):
        cj.draw = lambda f=f: ([3, 0, 1, 2], [None, None, None, f])
        got = _run([imageprep.ImagePlan(colours)], [([3, 0, 1, 2], [None, None, None, f])])[0]
        assert np.array_equal(got, np.asarray(cj(colours))), f


def test_jitter_sequences_with_contrast_between_other_operations_equal_pil():
    """Four scenes in one launch, each with all four operations in a different drawn order (Contrast's mean is taken on the
    image as it stands when Contrast comes), flips on two of them."""
    a = hostp._random_image(97, 61, seed=11)
    im = Image.fromarray(a, "RGB")
    orders = [[1, 0, 2, 3], [0, 2, 1, 3], [3, 2, 0, 1], [2, 3, 1, 0]]
    fs = [_f32(0.7), _f32(1.3), _f32(0.8), _f32(0.05)]
    draws = [(o, fs) for o in orders]
    flips = [False, True, False, True]
    got = _run([imageprep.ImagePlan(im)] * 4, draws, flips)
    cj = ColorJitter(0.4, 0.4, 0.4, 0.1)
    for b, d in enumerate(draws):
        cj.draw = lambda d=d: d
        ref = np.asarray(cj(im))
        assert np.array_equal(got[b], ref[:, ::-1] if flips[b] else ref), b


@pytest.mark.parametrize("src_size,dst_size", hostp.RESIZES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in hostp.RESIZES])
def test_resize_equals_pil(src_size, dst_size):
    a = hostp._random_image(*src_size, seed=src_size[0])
    im = Image.fromarray(a, "RGB")
    got = _run([imageprep.ImagePlan(im).resize(dst_size, Image.BILINEAR)], [None])[0]
    assert np.array_equal(got, np.asarray(im.resize(dst_size, Image.BILINEAR)))


def test_crop_windows_then_resize_in_one_batch_equal_pil():
    a = hostp._random_image(317, 143, seed=5)
    im = Image.fromarray(a, "RGB")
    boxes = [(13, 7, 301, 131), (0, 40, 160, 90), (5, 0, 60, 30), (0, 0, 317, 143)]
    plans = [imageprep.ImagePlan(im).crop(b).resize((96, 60), Image.BILINEAR) for b in boxes]
    got = _run(plans, [None] * 4)
    for g, b in zip(got, boxes):
        assert np.array_equal(g, np.asarray(im.crop(b).resize((96, 60), Image.BILINEAR))), b


def _rng_states():
    return np.random.get_state(), torch.get_rng_state()


def _same_rng(a, b):
    (na, ta), (nb, tb) = a, b
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(na, nb)), "numpy RNG state"
    assert torch.equal(ta, tb), "torch RNG state"


def _same_batches(g, h):
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert set(g) == set(h), set(g) ^ set(h)
    for k in g:
        a, b = g[k], h[k]
        if isinstance(a, list):
            assert len(a) == len(b), k
            for i, (x, y) in enumerate(zip(a, b)):
                tlg._same(host(x), host(y), f"{k}[{i}]")
        else:
            tlg._same(host(a), host(b), k)


@pytest.mark.parametrize("name", tlg.GPU_CASES)
def test_gpu_images_equal_the_reference_batch_and_the_host_images(name):
    z = np.load(os.path.join(tlg.G, f"loader_{name}.npz"))
    ds, kw = tlg._dataset(name)
    idx = [int(i) for i in z["indices"]]
    np.random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    g = ds.gpu_batch(idx, want_seg2d=True, image="gpu")
    g_rng = _rng_states()
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    tlg._same(host(g["x"][0]), z["batch/x0"], "locs")
    tlg._same(host(g["x"][1]), z["batch/x1"], "feats")
    for k in ("seg_label", "img", "depth", "intrinsics", "seg_labels_2d", "min_values", "offsets", "rotation_matrices", "points", "coords"):
        tlg._same(host(g[k]), z[f"batch/{k}"], k)
    for k in ["img_indices"] + (["orig_seg_label", "orig_points_idx"] if kw.get("output_orig") else []):
        assert len(g[k]) == int(z[f"batch/{k}/len"])
        for i, e in enumerate(g[k]):
            tlg._same(host(e), z[f"batch/{k}/{i}"], f"{k}[{i}]")
    if "batch/pseudo_label_2d" in z.files:
        tlg._same(host(g["pseudo_label_2d"]), z["batch/pseudo_label_2d"], "pseudo_label_2d")
        tlg._same(host(g["pseudo_label_ensemble"]), z["batch/pseudo_label_ensemble"], "pseudo_label_ensemble")
    np.random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    h = ds.gpu_batch(idx, want_seg2d=True, image="host")
    _same_rng(g_rng, _rng_states())
    _same_batches(g, h)


def test_sixteen_nuscenes_sized_scenes_equal_the_host_path():
    """16 scenes of synthetic 1600x900 JPEGs -> 400x225 with jitter, flips and normalisation: multi-scene descriptors and
    the order of the threaded decode."""
    spec = importlib.util.spec_from_file_location("bench_imageprep", os.path.join(tlg.G, "..", "..", "tools", "bench_imageprep.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from mm2d3d_amd import datasets

    with tempfile.TemporaryDirectory() as root:
        cls, kw = bench.make_dataset(root, "nuscenes")
        ds = getattr(datasets, cls)(**kw)
        idx = [(7 * i) % len(ds) for i in range(16)]
        np.random.seed(5)
        torch.manual_seed(5)
        g = ds.gpu_batch(idx, want_seg2d=True, image="gpu", decode_threads=4)
        g_rng = _rng_states()
        np.random.seed(5)
        torch.manual_seed(5)
        h = ds.gpu_batch(idx, want_seg2d=True, image="host")
        _same_rng(g_rng, _rng_states())
        assert g["img"].shape == (16, 3, 225, 400) and any(g["fliplr"]) and not all(g["fliplr"])
        _same_batches(g, h)
