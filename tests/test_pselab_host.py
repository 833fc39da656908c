"""CPU checks of the pseudo-label export (mm2d3d_amd/pselab.py, csrc/pselab.hip): the numpy restatement of the radix select against
a sort, the threshold rule against the fixture the reference's own function produced, the file format through the loaders,
the C ABI, and the kernels' register / scratch use as the gfx950 compiler reports it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _pselab_util import GOLDEN_CASES, KW, write_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
F09 = np.float32(0.9)


def _sorted_medians(probs, labels, C):
    med, present = np.zeros(C, np.float32), np.zeros(C, bool)
    for c in range(C):
        p = probs[labels == c]
        if len(p):
            med[c], present[c] = np.sort(p)[(len(p) - 1) // 2], True
    return med, present


def _constructed():
    """name -> (probs float32, labels int64, C)"""
    rng = np.random.default_rng(4)
    f = lambda *v: np.array(v, dtype=np.float32)
    tiny = np.float32(1e-45)  # the smallest denormal
    low = np.float32(0.7).view(np.uint32)
    low_byte = np.array([low + k for k in (5, 0, 255 - (int(low) & 255), 3, 1, 2, 4)], dtype=np.uint32).view(np.float32)  # same upper 3 bytes
    assert len({int(v) >> 8 for v in low_byte.view(np.uint32)}) == 1
    above, below = np.nextafter(F09, np.float32(1)), np.nextafter(F09, np.float32(0))
    cases = {
        "one_element": (f(0.3), np.array([0]), 1),
        "all_equal": (np.full(9, 0.625, np.float32), np.zeros(9, np.int64), 1),
        "two_values_even": (f(0.2, 0.8, 0.2, 0.8), np.zeros(4, np.int64), 1),
        "two_values_odd": (f(0.8, 0.2, 0.8, 0.2, 0.8), np.zeros(5, np.int64), 1),
        "two_values_two_classes": (f(0.2, 0.8, 0.2, 0.8, 0.8, 0.2, 0.8), np.array([0, 0, 1, 1, 1, 0, 0]), 2),
        "lowest_byte": (low_byte, np.zeros(len(low_byte), np.int64), 1),
        "around_0.9": (np.array([below, F09, above, F09, above, below, F09, above, above], np.float32), np.array([0, 0, 0, 1, 1, 1, 2, 2, 2]), 3),
        "exactly_0.9": (np.array([F09, F09, F09, below], np.float32), np.zeros(4, np.int64), 1),
        "denormals_and_zero": (np.array([0.0, tiny, 2 * tiny, 0.0, 1e-39, 0.5, 0.0], np.float32), np.array([0, 0, 0, 1, 1, 1, 1]), 2),
        "absent_class": (rng.random(50).astype(np.float32), rng.choice([0, 2, 4], 50), 6),
        "ignored_present": (rng.random(200).astype(np.float32), np.where(rng.random(200) < 0.3, -100, rng.integers(0, 4, 200)), 4),
    }
    return cases


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_radix_select_restatement_equals_the_sorted_lower_median_on_the_golden(name):
    from mm2d3d_amd import pselab

    z = np.load(os.path.join(G, "pselab.npz"))
    probs, labels = z[f"{name}/probs"], z[f"{name}/labels"]
    C = int(labels.max()) + 1
    med, present = pselab.radix_select_medians(probs, labels, C)
    ref, ref_present = _sorted_medians(probs, labels, C)
    assert np.array_equal(present, ref_present) and np.array_equal(med.view(np.uint32), ref.view(np.uint32))
    # the threshold rule on those medians reproduces the reference's refined labels exactly
    out = pselab.refine_with_medians(probs, labels, med, present)
    assert out.dtype == np.int64 and np.array_equal(out, z[f"{name}/refined"])


@pytest.mark.parametrize("name", sorted(_constructed()))
def test_radix_select_restatement_on_constructed_inputs(name):
    from mm2d3d_amd import pselab
    from mm2d3d_amd.datasets import refine_pseudo_labels as host_refine

    probs, labels, C = _constructed()[name]
    med, present = pselab.radix_select_medians(probs, labels, C)
    ref, ref_present = _sorted_medians(probs, labels, C)
    assert np.array_equal(present, ref_present), (present, ref_present)
    assert np.array_equal(med[present], ref[present]), (med, ref)  # by value: +0.0 == -0.0
    out = pselab.refine_with_medians(probs, labels, med, present)
    # the host function treats -100 as one more class; with it masked out of the comparison the two rules agree
    valid = labels >= 0
    assert np.array_equal(out[valid], host_refine(probs[valid], labels[valid]))
    assert np.array_equal(out[~valid], labels[~valid])
    if name == "around_0.9":  # medians 0.9, 0.9, nextafter(0.9): thresholds all float32(0.9)
        assert list(out) == [-100, 0, 0, 1, 1, -100, 2, 2, 2]
    if name == "absent_class":
        assert not present[1] and not present[3] and not present[5]


def test_float_keys_preserve_the_order():
    from mm2d3d_amd import pselab

    v = np.array([-np.inf, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1e-39, 0.5, 0.9, 1.0, np.inf], dtype=np.float32)
    k = pselab.float_keys(v).astype(np.int64)
    assert (np.diff(k) > 0).all()


# ---------------------------------------------------------------------------------------------------- the file, through the loader
@pytest.mark.parametrize("with_3d", [True, False])
def test_writer_round_trip_through_the_loader(tmp_path, with_3d):
    from mm2d3d_amd import pselab
    from mm2d3d_amd.datasets import PreprocessedScenes, refine_pseudo_labels

    data = write_scenes(str(tmp_path))
    rng = np.random.default_rng(5)
    path = str(tmp_path / "pselab_out.npy")
    w = pselab.PseudoLabelWriter(path, with_3d=with_3d)
    written = []
    for d in data:
        n = len(d["points"])
        args = []
        for _ in range(3):
            args += [rng.random(n).astype(np.float64), rng.integers(0, 4, n)]  # the writer converts to float32 / uint8
        w.add_scene(*args)
        written.append(args)
    with pytest.raises(ValueError):
        w.add_scene(written[0][0], written[0][1][:-1], *written[0][2:])  # lengths must agree
    assert not os.path.exists(path)
    assert w.close() == path and os.path.exists(path) and not os.path.exists(path + ".npy")
    arr = np.load(path, allow_pickle=True)
    assert arr.dtype == object and arr.shape == (len(data),)
    for d, args in zip(arr, written):
        assert list(d) == list(pselab.KEYS)
        for j, k in enumerate(pselab.KEYS):
            if not with_3d and k in ("probs_3d", "pseudo_label_3d"):
                assert d[k] is None
                continue
            assert d[k].dtype == (np.float32 if k.startswith("probs") else np.uint8) and d[k].shape == (len(args[0]),)
            assert np.array_equal(d[k], args[j].astype(d[k].dtype))
    ds = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), pselab_paths=path, output_orig=True, **KW)
    assert ds.pselab_length_key == "seg_labels"
    bounds = np.concatenate([[0], np.cumsum([len(d["points"]) for d in data])])
    for j, name in enumerate(("2d", "3d", "ensemble")):
        if name == "3d" and not with_3d:
            continue
        refined = refine_pseudo_labels(np.concatenate([a[2 * j].astype(np.float32) for a in written]),
                                       np.concatenate([a[2 * j + 1] for a in written]).astype(np.int64))
        assert (refined == -100).any()
        for i in range(len(data)):
            s = ds[i]
            assert np.array_equal(s[f"pseudo_label_{name}"], refined[bounds[i] : bounds[i + 1]][s["orig_points_idx"]])
    if not with_3d:
        assert ds[0]["pseudo_label_3d"] is None


def test_dataset_without_a_pseudo_label_file_still_names_its_length_key(tmp_path):
    from mm2d3d_amd.datasets import PreprocessedScenes

    write_scenes(str(tmp_path))
    ds = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), **KW)
    assert ds.pselab_data is None and ds.pselab_length_key == "seg_labels"


def test_gpu_refinement_refuses_other_dtypes_by_naming_the_host_function():
    from mm2d3d_amd import pselab

    with pytest.raises(TypeError, match="datasets.refine_pseudo_labels"):
        pselab.refine_pseudo_labels(np.zeros(4, np.float64), np.zeros(4, np.int64))


# ---------------------------------------------------------------------------------------------------- ABI and compiler report
def test_abi_exports_the_three_entry_points_with_the_declared_signatures():
    import ctypes

    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "uint8_t*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp,
             "mm_stream_t": _lib.vp, "int": _lib.i32, "int64_t": _lib.i64, "size_t": _lib.sz}
    for name in ("mm_pselab_predict", "mm_pselab_refine_ws_bytes", "mm_pselab_refine"):
        assert hasattr(lib, name), name
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctype[m.group(1)], name
        assert args == [ctype[p] for p in params], (name, params)
    L = _lib.lib()
    assert int(L.mm_pselab_refine_ws_bytes(11)) >= 11 * 256 * 8 and int(L.mm_pselab_refine_ws_bytes(33)) == 0
    # argument errors are reported before anything is launched (no GPU needed): class count above the library's limit
    assert L.mm_pselab_predict(None, 33, None, 0, 10, 33, None, None, None, None, None, None, None) == -1 and b"pselab_predict" in L.mm_last_error()
    assert L.mm_pselab_refine(None, None, 10, 33, -100, None, None, 0, None) == -1 and b"pselab_refine" in L.mm_last_error()


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """hipcc's kernel-resource-usage remarks for csrc/pselab.hip on gfx950: every kernel reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found (the library is built with it)"
    src = os.path.join(ROOT, "mm2d3d_amd", "csrc", "pselab.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(tmp_path / "pselab.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = {}
    cur = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = " ".join(kernels)
    for k in ("k_pselab_predictILb1", "k_pselab_predictILb0", "k_refine_hist", "k_refine_select", "k_refine_apply"):
        assert k in names, (k, names)
    for name, res in kernels.items():
        assert res["ScratchSize [bytes/lane]"] == 0 and res["SGPRs Spill"] == 0 and res["VGPRs Spill"] == 0, (name, res)
        assert 0 < res["VGPRs"] <= 64, (name, res)
    print({n: r_["VGPRs"] for n, r_ in kernels.items()})
