"""Float64 points (VirtualKITTI with camera_coords) on the host: the restatement against fixtures produced by the REFERENCE
(tests/golden/make_golden_f64.py), and the float64 product that the GPU voxeliser (csrc/dataprep.hip, fp64 entries)
restates, checked against this machine's numpy with exact arithmetic."""
import os
from fractions import Fraction

import numpy as np
import pytest

import test_loader_golden as tlg

G = tlg.G
AUG3D_CAM = dict(noisy_rot=0.1, flip_x=0.5, rot_y=6.2831, transl=True)
VOX_F64_CASES = {"plain": dict(), "flip_only": dict(flip_x=0.5), "transl_only": dict(transl=True), "vkitti_cam": AUG3D_CAM}

# the constructor keywords of make_golden_f64.CASES (kept in step by test_cases_match_the_generator)
VK = dict(split=("train",), preprocess_dir="{root}", virtual_kitti_dir="{root}", merge_classes=True, merge_classes_style="VirtualKITTI",
          downsample=(1500,), crop_size=(200, 60), bottom_crop=True, fliplr=0.5, color_jitter=(0.4, 0.4, 0.4),
          random_weather=("clone", "fog"), camera_coords=True, noisy_rot=0.1, flip_x=0.5, rot=6.2831, transl=True)
F64_CASES = {
    "vkitti_cam_aug": ("VirtualKITTISCN", "virtual_kitti", dict(VK, use_rgb=False)),
    "vkitti_cam_aug_rgb": ("VirtualKITTISCN", "virtual_kitti", dict(VK, use_rgb=True)),
}


def test_cases_match_the_generator():
    src = open(os.path.join(G, "make_golden_f64.py")).read()
    gen = {}
    exec(src[src.index("AUG3D_CAM = dict(") : src.index("\ndef camera_points")], gen)  # the generator's literal case tables
    assert gen["VOX_CASES"] == VOX_F64_CASES
    assert {k: v[0] for k, v in gen["CASES"].items()} == {k: v[2] for k, v in F64_CASES.items()}


@pytest.mark.parametrize("name", sorted(VOX_F64_CASES))
def test_host_voxeliser_equals_the_reference_on_float64_points(name):
    """voxelize.augment_and_scale_3d + voxelize_points on float64 camera-frame points = the reference's, dtype included; the
    draws of dataprep.augmentation_draws (the GPU path's host half) give the same rotation."""
    from mm2d3d_amd.dataprep import augmentation_draws
    from mm2d3d_amd.voxelize import augment_and_scale_3d, voxelize_points

    z = np.load(os.path.join(G, "voxelize_f64.npz"))
    pts = z["points"]
    assert pts.dtype == np.float64
    np.random.seed(1234)
    coords, min_value, offset, rot = augment_and_scale_3d(pts.copy(), 20, 4096, **VOX_F64_CASES[name])
    tlg._same(coords, z[f"{name}/coords_f"], "coords_f")
    tlg._same(min_value, z[f"{name}/min_value"], "min_value")
    tlg._same(offset, z[f"{name}/offset"], "offset")
    tlg._same(rot, z[f"{name}/rot"], "rot")
    vox, mask = voxelize_points(coords, 4096)
    tlg._same(vox, z[f"{name}/voxels"], "voxels")
    tlg._same(mask, z[f"{name}/mask"], "mask")
    np.random.seed(1234)
    r, u = augmentation_draws(**VOX_F64_CASES[name])
    tlg._same(r, z[f"{name}/rot"], "augmentation_draws rot")
    assert (u is not None) == bool(VOX_F64_CASES[name].get("transl", False))


@pytest.mark.parametrize("name", sorted(F64_CASES))
def test_host_samples_and_collate_equal_the_reference(name, monkeypatch):
    """VirtualKITTISCN.__getitem__ + collate_scn_base with the experiment's settings (camera_coords, 3D augmentation, fliplr,
    colour jitter, bottom crop, downsample) = the reference's, key by key and bit for bit."""
    monkeypatch.setitem(tlg.CASES, name, F64_CASES[name])
    tlg.test_host_samples_and_collate_equal_the_reference(name)


def test_prepare_batch_rejects_a_mix_of_float32_and_float64_points():
    """Raised before anything reaches a device."""
    from mm2d3d_amd import dataprep

    sc = lambda dt: dict(points=np.zeros((4, 3), dt), points_img=np.zeros((4, 2), np.float32), depth=np.ones(4, np.float32),
                         seg_label=np.zeros(4, np.int64), img=np.zeros((3, 2, 2), np.float32))
    with pytest.raises(ValueError, match="float64"):
        dataprep.prepare_batch([sc(np.float32), sc(np.float64)])


def _fma(a, b, c):
    """float64 fused multiply-add, rounded once (exact rational arithmetic; int / int division in Python rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_numpy_float64_dot_is_the_k_order_fma_form():
    """numpy's float64 ``points.dot(rot)`` (OpenBLAS dgemm) = fma(p2, r2j, fma(p1, r1j, p0 * r0j)), the form the fp64 GPU
    voxeliser computes.  If this fails, this machine's BLAS dispatches a kernel with another summation order, and the
    float64 fixtures and GPU comparisons against the host path are not expected to hold here."""
    from mm2d3d_amd.dataprep import augmentation_draws

    # full float64 mantissas: with float32-valued points (VirtualKITTI's) every product is exact and the fused and unfused
    # forms agree, so only the k order would be checked
    pts = np.random.default_rng(9).standard_normal((3000, 3)) * 30
    np.random.seed(4)
    rot, _ = augmentation_draws(**AUG3D_CAM)
    got = pts.dot(rot)
    r = rot.astype(np.float64)
    want = np.empty_like(got)
    for i, (p0, p1, p2) in enumerate(pts.tolist()):
        for j in range(3):
            want[i, j] = _fma(p2, float(r[2, j]), _fma(p1, float(r[1, j]), p0 * float(r[0, j])))
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} elements differ from the k-order fma form"
    unfused = pts[:, :1] * r[0] + pts[:, 1:2] * r[1] + pts[:, 2:3] * r[2]
    assert (unfused != want).any(), "the check must be able to tell the fused form from the unfused one"
