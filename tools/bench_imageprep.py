"""Host time of ``gpu_batch`` per batch with the image half on the host (PIL + numpy) and on the GPU (csrc/imageprep.hip).

Writes temporary full-size datasets from the miniature ones of tests/golden/mini_ds: nuScenes-shaped (the train_usa pkl with
``points_img`` scaled to 1600x900, JPEGs re-encoded at 1600x900 q90, resize (400, 225)) and A2D2-shaped (1920x1208 ->
480x302), and prints one JSON line per dataset: ms per 16-scene ``gpu_batch`` (wall clock, synchronised) for
``image="host"`` and for ``image="gpu"`` with 1 and 4 host decode threads, and the GPU ms of the three image kernels (events).
``gpu_decode_ms``: ``image="gpu"`` with the JPEGs decoded on the GPU (csrc/jpeg.hip), and ``decode_ms`` the GPU ms of the
decoder (events).  The variants alternate within each repetition.

``vkitti``: the source domain of the vkitti -> skitti experiment (VirtualKITTISCN with camera_coords, so float64 points;
downsample 10000, 1242x375 PNGs, bottom crop (480, 302), fliplr, colour jitter, the 3D augmentation, use_rgb=False) on
synthetic scenes of 20-40k points inside the camera's frustum.  Its line adds ``loader_ms``, the host loader plus
``collate_scn_base`` (``[ds[i] for i in indices]``), and ``voxelize_ms``, the GPU ms of ``dataprep.voxelize_batch`` on the
batch's float64 points (events; the fp64 voxeliser kernels and the read-back of the kept counts) in place of ``kernels_ms``.

    python tools/bench_imageprep.py [--scenes 16] [--reps 5] [--kind nuscenes a2d2 vkitti]
"""
import argparse
import json
import os
import pickle
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MINI = os.path.join(ROOT, "tests", "golden", "mini_ds")
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
KINDS = {  # source size of the miniature images -> full size, network size
    "nuscenes": dict(full=(1600, 900), resize=(400, 225)),
    "a2d2": dict(full=(1920, 1208), resize=(480, 302)),
    "vkitti": dict(full=(1242, 375), resize=(480, 302)),  # resize = the bottom crop
}
VKITTI_PROJ = ((725.0, 0.0, 620.5), (0.0, 725.0, 187.0))  # VirtualKITTISCN.proj_matrix


def _upscale(src, dst, size, seed):
    """The miniature image upscaled to ``size`` with some per-pixel noise (texture for the JPEG coder), JPEG q90."""
    from PIL import Image

    a = np.asarray(Image.open(src).convert("RGB").resize(size, Image.BICUBIC)).astype(np.int16)
    a = a + np.random.default_rng(seed).integers(-12, 13, a.shape)
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), "RGB").save(dst, quality=90)


def make_vkitti(root, n_scenes=16, seed=0):
    """A VirtualKITTI-format dataset of ``n_scenes`` synthetic scenes: 20-40k LiDAR points each, placed by drawing a pixel
    and a depth and back-projecting through the fixed camera (so every point projects inside the 1242x375 image; most land
    in the rows a bottom crop keeps), labels with some 99s, and one noisy PNG per scene and weather."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    W, H = KINDS["vkitti"]["full"]
    (fx, _, cx), (_, fy, cy) = VKITTI_PROJ
    data = []
    for i in range(n_scenes):
        n = int(rng.integers(20000, 40001))
        u = rng.uniform(1.0, W - 1.0, n)
        v = np.where(rng.random(n) < 0.9, rng.uniform(H - 300.0, H - 1.0, n), rng.uniform(1.0, H - 1.0, n))
        x = rng.uniform(4.0, 80.0, n)
        pts = np.stack([x, -(u - cx) / fx * x, -(v - cy) / fy * x], 1).astype(np.float32)
        labels = rng.integers(0, 14, n).astype(np.uint8)
        labels[rng.random(n) < 0.03] = 99
        scene, frame = f"{i // 4 + 1:04d}", f"{i:05d}"
        base = np.kron(rng.integers(0, 256, (-(-H // 25), -(-W // 25), 3)), np.ones((25, 25, 1), np.int16))[:H, :W]
        for weather in ("clone", "fog"):
            d = os.path.join(root, "vkitti_1.3.1_rgb", scene, weather)
            os.makedirs(d, exist_ok=True)
            img = np.clip(base + rng.integers(-10, 11, base.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img, "RGB").save(os.path.join(d, frame + ".png"), compress_level=1)
        data.append({"points": pts, "seg_labels": labels, "scene_id": scene, "frame_id": frame})
    with open(os.path.join(root, "train.pkl"), "wb") as f:
        pickle.dump(data, f)
    return "VirtualKITTISCN", dict(split=("train",), preprocess_dir=root, virtual_kitti_dir=root, merge_classes=True,
                                   merge_classes_style="VirtualKITTI", downsample=(10000,), crop_size=KINDS["vkitti"]["resize"],
                                   bottom_crop=True, fliplr=0.5, color_jitter=(0.4, 0.4, 0.4), random_weather=("clone", "fog"),
                                   camera_coords=True, use_rgb=False, noisy_rot=0.1, flip_x=0.5, rot=6.2831, transl=True)


def make_dataset(root, kind):
    """Writes the full-size variant of mini_ds/<kind> under ``root``; returns the dataset's constructor keywords."""
    if kind == "vkitti":
        return make_vkitti(root)
    full = KINDS[kind]["full"]
    if kind == "nuscenes":
        src_dir, pkl_rel = os.path.join(MINI, "nuscenes"), "train_usa.pkl"
    else:
        src_dir, pkl_rel = os.path.join(MINI, "a2d2"), os.path.join("preprocess", "train.pkl")
        for f in ("cams_lidars.json", "class_list.json"):
            shutil.copy(os.path.join(src_dir, f), os.path.join(root, f))
    with open(os.path.join(src_dir, pkl_rel), "rb") as f:
        data = pickle.load(f)
    for k, d in enumerate(data):
        src = os.path.join(src_dir, d["camera_path"])
        w0, h0 = __import__("PIL.Image").Image.open(src).size
        d["points_img"] = (d["points_img"] * np.array([full[1] / h0, full[0] / w0])).astype(d["points_img"].dtype)
        dst = os.path.join(root, d["camera_path"])
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        _upscale(src, dst, full, k)
    os.makedirs(os.path.dirname(os.path.join(root, pkl_rel)), exist_ok=True)
    with open(os.path.join(root, pkl_rel), "wb") as f:
        pickle.dump(data, f)
    common = dict(resize=KINDS[kind]["resize"], image_normalizer=NORM, fliplr=0.5, color_jitter=(0.4, 0.4, 0.4), use_rgb=True,
                  noisy_rot=0.1, flip_x=0.5, rot=6.2831, transl=True)
    if kind == "nuscenes":
        return "NuScenesLidarSegSCN", dict(split=("train_usa",), preprocess_dir=root, nuscenes_dir=root, merge_classes=True, **common)
    return "A2D2SCN", dict(split=("train",), preprocess_dir=root, merge_classes=True, **common)


def _kernel_ms(ds, indices, device):
    """GPU ms of the three image kernels for the plans and draws of one batch (events around mm_image_prepare)."""
    from mm2d3d_amd import dataprep, imageprep

    ds._plan_images = True
    try:
        works = [ds._front(i) for i in indices]
    finally:
        ds._plan_images = False
    draws = [ds.color_jitter.draw() for _ in works]
    flips = [bool(np.random.rand() < ds.fliplr) for _ in works]
    lut = imageprep.lut(ds._to_float, ds._normalise)
    timing = {}
    dataprep.prepare_images([w.image for w in works], draws, flips, [lut] * len(works), device, 4, timing=timing)
    return timing


def _voxelize_ms(ds, indices, device):
    """GPU ms of ``dataprep.voxelize_batch`` on the points of one batch (host front end and draws as gpu_batch makes them)."""
    import torch

    from mm2d3d_amd import dataprep

    works = [ds._front(i) for i in indices]
    draws = [dataprep.augmentation_draws(**ds._augmentation()) for _ in works]
    pts = torch.from_numpy(np.concatenate([w.points for w in works])).to(device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    dataprep.voxelize_batch(pts, [len(w.points) for w in works], [r for r, _ in draws], [u for _, u in draws], ds.scale, ds.full_scale)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def _loader_ms(ds, indices, reps):
    """Host loader plus collate (the reference's DataLoader work for one batch, in one process)."""
    from mm2d3d_amd.datasets import collate_scn_base

    times = []
    for r in range(reps + 1):
        np.random.seed(r)
        t0 = time.perf_counter()
        collate_scn_base([ds[i] for i in indices], output_orig=False)
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 2)


def main():
    import torch

    from mm2d3d_amd import datasets

    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kind", nargs="+", default=list(KINDS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind in args.kind:
        with tempfile.TemporaryDirectory() as root:
            cls, kw = make_dataset(root, kind)
            ds = getattr(datasets, cls)(**kw)
            indices = [i % len(ds) for i in range(args.scenes)]
            res = {"kind": kind, "scenes": args.scenes, "full": KINDS[kind]["full"], "resize": KINDS[kind]["resize"]}
            if kind == "vkitti":
                res["loader_ms"] = _loader_ms(ds, indices, args.reps)
            from mm2d3d_amd import dataprep

            variants = [("host", "host", 1, False), ("gpu_1thread", "gpu", 1, False), ("gpu_4threads", "gpu", 4, False)]
            if kind != "vkitti":
                variants.append(("gpu_decode", "gpu", 4, True))
            times = {name: [] for name, _, _, _ in variants}
            for r in range(args.reps + 1):  # the first round warms up; the variants alternate
                for name, image, threads, gpu_jpeg in variants:
                    dataprep.GPU_JPEG = gpu_jpeg
                    try:
                        np.random.seed(r)
                        torch.manual_seed(r)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        ds.gpu_batch(indices, device=dev, want_seg2d=True, image=image, decode_threads=threads)
                        torch.cuda.synchronize()
                    finally:
                        dataprep.GPU_JPEG = True
                    if r:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            for name in times:
                res[f"{name}_ms"] = round(float(np.median(times[name])), 2)
            if kind == "vkitti":
                res["voxelize_ms"] = round(float(np.median([_voxelize_ms(ds, indices, dev) for _ in range(args.reps + 1)][1:])), 3)
            else:
                tm = [_kernel_ms(ds, indices, dev) for _ in range(args.reps + 1)][1:]
                res["kernels_ms"] = round(float(np.median([t["kernels_ms"] for t in tm])), 3)
                res["decode_ms"] = round(float(np.median([t["decode_ms"] for t in tm])), 3)
                res["gpu_decoded"] = tm[-1]["gpu_decoded"]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
