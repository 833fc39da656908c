"""Pseudo-label export on the GPU (mm2d3d_amd/pselab.py, csrc/pselab.hip): the prediction kernel against torch's float64 softmax
and against the evaluation kernel, the radix-select refinement against the host function, and the export end to end."""
import os

import numpy as np
import pytest
import torch

from _pselab_util import GOLDEN_CASES, KW, write_scenes

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
MINI = os.path.join(G, "mini_ds")
SETS = (("probs_2d", "pseudo_label_2d"), ("probs_3d", "pseudo_label_3d"), ("probs_ensemble", "pseudo_label_ensemble"))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _logits(N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return 3 * torch.randn(N, C, generator=g), 3 * torch.randn(N, C, generator=g)


def _ref64(a, b):
    sa, sb = torch.softmax(a.double(), 1), torch.softmax(b.double(), 1)
    return sa, sb, 0.5 * (sa + sb)


@pytest.mark.parametrize("C", [5, 6, 10, 11])
def test_predict_against_float64_softmax(C):
    """Labels equal float64's wherever its top-two gap is >= 1e-6 (the points left out: at most 1e-4 of N); probabilities within
    (D + C + 3) * 2^-24 relative, D = the largest max-minus-min spread of a logit row."""
    from mm2d3d_amd import pselab

    dev, N = _dev(), 400_000
    a, b = _logits(N, C, 100 + C)
    out = pselab.predict(a.to(dev), b.to(dev))
    D = max(float((x.max(1).values - x.min(1).values).max()) for x in (a, b))
    bound = (D + C + 3) * 2.0 ** -24
    for (pk, lk), ref in zip(SETS, _ref64(a, b)):
        assert out[pk].dtype == torch.float32 and out[lk].dtype == torch.uint8 and out[pk].shape == (N,) and out[lk].shape == (N,)
        top2 = ref.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) >= 1e-6
        left_out = 1.0 - float(sure.double().mean())
        got_l, got_p = out[lk].cpu().long(), out[pk].cpu().double()
        rel = float(((got_p - top2[:, 0]).abs() / top2[:, 0]).max())
        print(f"C={C} {lk}: left out {left_out:.2e} of N, label mismatches among the rest {int((got_l != ref.argmax(1))[sure].sum())}, "
              f"max relative probability error {rel:.3e} (bound {bound:.3e}, D = {D:.2f})")
        assert left_out <= 1e-4
        assert torch.equal(got_l[sure], ref.argmax(1)[sure])
        assert rel <= bound


def test_predict_ties_take_the_first_maximum():
    from mm2d3d_amd import pselab

    dev = _dev()
    for C in (3, 6, 7, 11):
        eq = torch.full((70, C), 1.25)
        out = pselab.predict(eq.to(dev), eq.to(dev))
        for pk, lk in SETS:
            assert int(out[lk].max()) == 0
            assert torch.equal(out[pk].cpu(), torch.full((70,), np.float32(1) / np.float32(C)))
        # the maximum occurs twice: at classes 1 and C - 1
        x = torch.zeros(300, C)
        x[:, 1] = 2.0
        x[:, C - 1] = 2.0
        out = pselab.predict(x.to(dev), x.to(dev))
        for _, lk in SETS:
            assert torch.equal(out[lk].cpu(), torch.ones(300, dtype=torch.uint8))


@pytest.mark.parametrize("C", [6, 11])
def test_predicted_labels_are_the_labels_evaluation_counts(C):
    from mm2d3d_amd import pselab
    from mm2d3d_amd.metrics import SegIoU

    dev, N = _dev(), 400_000
    a, b = _logits(N, C, 7 + C)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(1))
    y[::9] = -100
    m = SegIoU(C, dev)
    m.update(a.to(dev), b.to(dev), y.to(dev))
    out = pselab.predict(a.to(dev), b.to(dev))
    keep = y != -100
    for i, (_, lk) in enumerate(SETS):
        cm = torch.bincount(y[keep] * C + out[lk].cpu().long()[keep], minlength=C * C).reshape(C, C)
        assert torch.equal(m.cm[i].cpu(), cm)


def test_predict_strided_inputs_and_2d_only():
    from mm2d3d_amd import pselab

    dev, N, C = _dev(), 10_007, 6
    a, b = _logits(N, C, 3)
    wide_a = torch.full((N, 16), 99.0, device=dev)
    wide_b = torch.full((N, 9), 99.0, device=dev)
    wide_a[:, 4:10] = a.to(dev)
    wide_b[:, :6] = b.to(dev)
    ref = pselab.predict(a.to(dev), b.to(dev))
    got = pselab.predict(wide_a[:, 4:10], wide_b[:, :6])
    for k in pselab.KEYS:
        assert torch.equal(ref[k], got[k]), k
    only = pselab.predict(wide_a[:, 4:10])
    assert torch.equal(only["probs_2d"], ref["probs_2d"]) and torch.equal(only["pseudo_label_2d"], ref["pseudo_label_2d"])
    assert all(only[k] is None for k in pselab.KEYS[2:])
    # one row, columns strided: nothing about the layout may depend on the row count
    one = torch.full((1, 2 * C), 99.0, device=dev)
    one[:, ::2] = a[:1].to(dev)
    got1 = pselab.predict(one[:, ::2], wide_b[:1, :6])
    for k in pselab.KEYS:
        assert torch.equal(got1[k], ref[k][:1]), k
    empty = pselab.predict(torch.zeros(0, C, device=dev), torch.zeros(0, C, device=dev))
    assert all(empty[k].shape == (0,) for k in pselab.KEYS)
    with pytest.raises(RuntimeError, match="bad C"):
        pselab.predict(torch.zeros(4, 33, device=dev))


def _refine_cases():
    rng = np.random.default_rng(17)
    n = 2_000_000
    probs = rng.random(n).astype(np.float32)
    labels = rng.integers(0, 11, n)
    gone = labels.copy()
    gone[(gone == 3) | (gone == 10)] = 5
    gone[rng.random(n) < 0.05] = -100
    z = np.load(os.path.join(G, "pselab.npz"))
    cases = {f"golden_{k}": (z[f"{k}/probs"], z[f"{k}/labels"]) for k in GOLDEN_CASES}
    cases.update(random=(probs, labels), ties=(np.floor(probs * 64).astype(np.float32) / np.float32(64), labels), absent_and_ignored=(probs, gone),
                 one=(np.array([0.4], np.float32), np.array([2])))
    return cases


@pytest.mark.parametrize("name", ["golden_even_odd", "golden_small", "golden_single_class", "random", "ties", "absent_and_ignored", "one"])
def test_refine_equals_the_host_function(name):
    from mm2d3d_amd import pselab
    from mm2d3d_amd.datasets import refine_pseudo_labels

    probs, labels = _refine_cases()[name]
    want = refine_pseudo_labels(probs, labels)  # (an ignore label is one more "class" to the host function: its rows stay as they are)
    got = pselab.refine_pseudo_labels(probs, labels, device=_dev())
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())
    again = pselab.refine_pseudo_labels(probs, labels, device=_dev())
    assert np.array_equal(got, again)
    if name.startswith("golden"):
        assert np.array_equal(got, np.load(os.path.join(G, "pselab.npz"))[name[len("golden_"):] + "/refined"])
    if name == "random":  # device tensors in, device tensor out; an explicit class count above the largest label
        t = pselab.refine_pseudo_labels(torch.from_numpy(probs).to(_dev()), torch.from_numpy(labels).to(_dev()), num_classes=16)
        assert t.is_cuda and t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), want)


def _write_pselab(path, data, seed=2, with_3d=True):
    from mm2d3d_amd import pselab

    rng = np.random.default_rng(seed)
    w = pselab.PseudoLabelWriter(path, with_3d=with_3d)
    for d in data:
        n = len(d["points"])
        w.add_scene(*[v for _ in range(3) for v in (np.floor(rng.random(n) * 32).astype(np.float32) / 32, rng.integers(0, 4, n))])
    return w.close()


@pytest.mark.parametrize("with_3d", [True, False])
def test_dataset_refined_on_the_gpu_equals_the_host_refined_one(tmp_path, with_3d):
    from mm2d3d_amd.datasets import PreprocessedScenes

    data = write_scenes(str(tmp_path), 4)
    path = _write_pselab(str(tmp_path / "ps.npy"), data, with_3d=with_3d)
    host = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), pselab_paths=path, **KW)
    gpu = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), pselab_paths=path, pselab_refine_device="cuda", **KW)
    refined_any = False
    for dh, dg in zip(host.pselab_data, gpu.pselab_data):
        assert list(dh) == list(dg)
        for k in dh:
            if dh[k] is None:
                assert dg[k] is None and not with_3d
                continue
            assert dh[k].dtype == dg[k].dtype and np.array_equal(dh[k], dg[k]), k
            refined_any |= k.startswith("pseudo") and bool((dg[k] == -100).any())
    assert refined_any
    bh, bg = host.gpu_batch([3, 0, 1]), gpu.gpu_batch([3, 0, 1])
    for k in ("pseudo_label_2d", "pseudo_label_3d", "pseudo_label_ensemble"):
        if k == "pseudo_label_3d" and not with_3d:
            assert bh[k] == [] and bg[k] == []
            continue
        assert torch.equal(bh[k], bg[k]), k


def _trainer(dev, C=6):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg
    from mm2d3d_amd.train import TrainModel

    torch.manual_seed(0)
    kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
    n2, n3 = Net2DSeg(C, pretrained=False).to(dev), Net3DSeg(C, True, kw).to(dev)
    return TrainModel({"2d_net": n2, "3d_net": n3}, None, Loss([{"name": "cross_entropy", "target": "segmentation", "args": {}}]),
                      dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, num_classes=C))


def test_export_end_to_end(tmp_path):
    from mm2d3d_amd import pselab
    from mm2d3d_amd.datasets import PreprocessedScenes

    dev = _dev()
    data = write_scenes(str(tmp_path), 6)
    ds = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), output_orig=True, **KW)
    tm = _trainer(dev)
    path, path2 = str(tmp_path / "round1.npy"), str(tmp_path / "round1_again.npy")
    summary = pselab.export_pseudo_labels(tm, ds, path, batch_size=4, device=dev)
    arr = np.load(path, allow_pickle=True)
    assert arr.shape == (6,) and [len(d["probs_2d"]) for d in arr] == [len(d["points"]) for d in data]
    assert summary["scenes"] == 6 and summary["points"] == sum(len(d["points"]) for d in data) and summary["num_classes"] == 6
    for key, lk in (("hist_2d", "pseudo_label_2d"), ("hist_3d", "pseudo_label_3d"), ("hist_ensemble", "pseudo_label_ensemble")):
        assert np.array_equal(summary[key], np.bincount(np.concatenate([d[lk] for d in arr]), minlength=6))
    for d in arr:
        assert list(d) == list(pselab.KEYS)
        for k in pselab.KEYS:
            assert d[k].dtype == (np.float32 if k.startswith("probs") else np.uint8)
        assert d["pseudo_label_2d"].max() < 6 and (d["probs_ensemble"] > 1.0 / 6 - 1e-6).all() and (d["probs_ensemble"] <= 1.0).all()
    # entry i = predict_step on the batch that contained scene i, cut at the scene boundaries
    for indices in ([0, 1, 2, 3], [4, 5]):
        batch = ds.gpu_batch(indices, device=dev)
        out = tm.predict_step(batch)
        bounds = np.concatenate([[0], np.cumsum([len(t) for t in batch["img_indices"]])])
        for b, i in enumerate(indices):
            for k in pselab.KEYS:
                assert np.array_equal(arr[i][k], out[k][bounds[b] : bounds[b + 1]].cpu().numpy()), (i, k)
    # the same export again: the same file
    pselab.export_pseudo_labels(tm, ds, path2, batch_size=4, device=dev)
    assert open(path, "rb").read() == open(path2, "rb").read()
    # ... which the loader accepts, on either refinement path
    for where in (None, "cuda"):
        nxt = PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), pselab_paths=path, pselab_refine_device=where, **KW)
        assert len(nxt.pselab_data) == 6 and nxt[2]["pseudo_label_ensemble"].dtype == np.int64


def test_export_refusals_name_the_scene_and_leave_no_file(tmp_path):
    from mm2d3d_amd import datasets, pselab

    dev = _dev()
    write_scenes(str(tmp_path), 3)
    tm = _trainer(dev)
    path = str(tmp_path / "refused.npy")
    no_orig = datasets.PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), **KW)
    with pytest.raises(ValueError, match=r"PreprocessedScenes.*output_orig.*before scene 0"):
        pselab.export_pseudo_labels(tm, no_orig, path, batch_size=2, device=dev)
    small = datasets.PreprocessedScenes("train_day", str(tmp_path), str(tmp_path), output_orig=True, full_scale=256, **KW)
    with pytest.raises(ValueError, match=r"scene \d+.*voxel range"):
        pselab.export_pseudo_labels(tm, small, path, batch_size=2, device=dev)
    root = os.path.join(MINI, "semantic_kitti")
    cropped = datasets.SemanticKITTISCN(split=("train",), preprocess_dir=root, semantic_kitti_dir=root, merge_classes_style="A2D2",
                                        crop_size=(48, 30), bottom_crop=True, use_rgb=True, output_orig=True)
    assert cropped.pselab_length_key == "points"
    np.random.seed(0)
    with pytest.raises(ValueError, match=r"scene \d+.*cropping"):
        pselab.export_pseudo_labels(tm, cropped, path, batch_size=2, device=dev)
    root = os.path.join(MINI, "a2d2")
    source_only = datasets.A2D2SCN(split=("train",), preprocess_dir=root, merge_classes=True, use_rgb=True)
    with pytest.raises(ValueError, match=r"A2D2SCN.*source-only"):
        pselab.export_pseudo_labels(tm, source_only, path, batch_size=2, device=dev)
    assert not os.path.exists(path) and not os.path.exists(path + ".npy")
