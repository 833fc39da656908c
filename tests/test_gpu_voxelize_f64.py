"""Float64 points on an MI355X (csrc/dataprep.hip, the _f64 entries): ``gpu_batch`` for VirtualKITTI with camera_coords
against the reference fixtures and the host path (batch and RNG states), the fp64 voxeliser against the reference's
``augment_and_scale_3d``, and one batch shaped like the vkitti -> skitti experiment's source domain."""
import importlib.util
import os
import tempfile

import numpy as np
import pytest
import torch

import test_gpu_imageprep as tgi
import test_loader_golden as tlg
from test_voxelize_f64_host import F64_CASES, VOX_F64_CASES

pytestmark = pytest.mark.gpu
KEYS = ("seg_label", "img", "depth", "intrinsics", "seg_labels_2d", "min_values", "offsets", "rotation_matrices", "points", "coords")


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dataset(name):
    if name in F64_CASES:
        cls, sub, kw = F64_CASES[name]
        from mm2d3d_amd import datasets

        kw = {k: (v.replace("{root}", os.path.join(tlg.MINI, sub)) if isinstance(v, str) else v) for k, v in kw.items()}
        return getattr(datasets, cls)(**kw)
    return tlg._dataset(name)[0]


def _same_as_host_collate(g, h):
    """gpu_batch dict g against collate_scn_base dict h (the keys the collate produces)."""
    tlg._same(_host(g["x"][0]), _host(h["x"][0]), "locs")
    tlg._same(_host(g["x"][1]), _host(h["x"][1]), "feats")
    for k in KEYS:
        tlg._same(_host(g[k]), _host(h[k]), k)
    assert len(g["img_indices"]) == len(h["img_indices"])
    for i, (a, b) in enumerate(zip(g["img_indices"], h["img_indices"])):
        tlg._same(_host(a), _host(b), f"img_indices[{i}]")


@pytest.mark.parametrize("image", ["host", "gpu"])
@pytest.mark.parametrize("name", ["vkitti_rand_crop"] + sorted(F64_CASES))
def test_gpu_batch_on_float64_points_equals_the_reference_batch(name, image):
    """Every tensor of the reference's collated batch, bit for bit (float64 points and min_values included), and the numpy /
    torch RNG states afterwards equal those after the host loader."""
    z = np.load(os.path.join(tlg.G, f"loader_{name}.npz"))
    ds = _dataset(name)
    idx = [int(i) for i in z["indices"]]
    assert ds.data[idx[0]]["points"].dtype == np.float32 and ds.camera_coords  # float64 arises in the front end
    np.random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    g = ds.gpu_batch(idx, want_seg2d=True, image=image)
    g_rng = tgi._rng_states()
    assert g["points"].dtype == torch.float64 and g["min_values"].dtype == torch.float64
    tlg._same(_host(g["x"][0]), z["batch/x0"], "locs")
    tlg._same(_host(g["x"][1]), z["batch/x1"], "feats")
    for k in KEYS:
        tlg._same(_host(g[k]), z[f"batch/{k}"], k)
    assert len(g["img_indices"]) == int(z["batch/img_indices/len"])
    for i, e in enumerate(g["img_indices"]):
        tlg._same(_host(e), z[f"batch/img_indices/{i}"], f"img_indices[{i}]")
    np.random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    [ds[i] for i in idx]
    tgi._same_rng(g_rng, tgi._rng_states())


@pytest.mark.parametrize("name", sorted(VOX_F64_CASES))
def test_gpu_voxeliser_float64_bit_exact_vs_reference_golden(name):
    from mm2d3d_amd.dataprep import augmentation_draws, voxelize_batch

    z = np.load(os.path.join(tlg.G, "voxelize_f64.npz"))
    pts = z["points"]
    np.random.seed(1234)
    rot, u = augmentation_draws(**VOX_F64_CASES[name])
    # two copies of the scene in one batch: the second scene must give the same voxels with batch index 1
    out = voxelize_batch(torch.from_numpy(np.concatenate([pts, pts])).cuda(), [len(pts), len(pts)], [rot, rot], [u, u], 20, 4096)
    vox, mask = z[f"{name}/voxels"], z[f"{name}/mask"]
    n = len(vox)
    assert out["counts"] == [n, n]
    locs = _host(out["locs"])
    tlg._same(locs[:n, :3], vox, "locs scene 0")
    tlg._same(locs[n:, :3], vox, "locs scene 1")
    assert np.all(locs[:n, 3] == 0) and np.all(locs[n:, 3] == 1)
    keep = _host(out["keep"])
    assert np.array_equal(keep[:n], np.nonzero(mask)[0]) and np.array_equal(keep[n:], np.nonzero(mask)[0] + len(pts))
    for b in range(2):
        tlg._same(_host(out["min_value"])[b], z[f"{name}/min_value"], "min_value")
        tlg._same(_host(out["offset"])[b], z[f"{name}/offset"], "offset")


def test_experiment_shaped_batch_equals_the_host_loader():
    """16 scenes of 20-40k points, downsample 10000, 1242x375 PNGs, bottom crop (480, 302), the experiment's augmentation
    and use_rgb=False: gpu_batch with the image half on the host and on the GPU = the host loader + collate_scn_base."""
    spec = importlib.util.spec_from_file_location("bench_imageprep", os.path.join(tlg.G, "..", "..", "tools", "bench_imageprep.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from mm2d3d_amd import datasets

    with tempfile.TemporaryDirectory() as root:
        cls, kw = bench.make_dataset(root, "vkitti")
        ds = getattr(datasets, cls)(**kw)
        idx = list(range(16))
        np.random.seed(8)
        torch.manual_seed(8)
        h = datasets.collate_scn_base([ds[i] for i in idx], output_orig=False)
        h_rng = tgi._rng_states()
        assert h["points"].dtype == torch.float64 and h["img"].shape == (16, 3, 302, 480)
        for image in ("host", "gpu"):
            np.random.seed(8)
            torch.manual_seed(8)
            g = ds.gpu_batch(idx, want_seg2d=True, image=image)
            tgi._same_rng(h_rng, tgi._rng_states())
            _same_as_host_collate(g, h)
