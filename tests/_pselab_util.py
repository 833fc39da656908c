"""Helpers shared by tests/test_pselab_host.py and tests/test_gpu_pselab.py (no tests here)."""
import os
import pickle

import numpy as np

GOLDEN_CASES = ("even_odd", "small", "single_class")  # the cases of tests/golden/pselab.npz

# constructor keywords of the miniature dataset: no augmentation, nothing that drops points
KW = dict(resize=(80, 45), image_normalizer=((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), use_rgb=True,
          label_mapping=[0, 0, 1, 1, 2, 3, -100, 3])


def write_scenes(root, n_scenes=3, split="train_day"):
    """A miniature dataset in the reference's on-disk format (<split>.pkl + JPEG camera images); no pseudo-label file."""
    from PIL import Image

    from mm2d3d_amd.synthetic import lidar_sweep

    rng = np.random.default_rng(13)
    W0, H0 = 160, 90
    data = []
    os.makedirs(os.path.join(root, "cams"), exist_ok=True)
    for i in range(n_scenes):
        pts = lidar_sweep(40 + i, "nuscenes")[:: 45 + i].copy()
        n = len(pts)
        path = os.path.join("cams", f"img{i}.jpg")
        Image.fromarray((rng.random((H0, W0, 3)) * 255).astype(np.uint8)).save(os.path.join(root, path), quality=92)
        data.append({
            "points": pts, "pts_cam_coord": (pts[:, [1, 2, 0]] * np.float32(1.0)).copy(),
            "points_img": np.stack([rng.uniform(0, H0 - 1e-2, n), rng.uniform(0, W0 - 1e-2, n)], 1).astype(np.float32),
            "seg_labels": rng.integers(0, 8, n).astype(np.uint8), "camera_path": path,
            "calib": {"cam_intrinsic": np.array([[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])},
        })
    with open(os.path.join(root, split + ".pkl"), "wb") as f:
        pickle.dump(data, f)
    return data
