"""The pipelined loader on an MI355X (mm2d3d_amd/pipeline.py, csrc/dataprep.hip ``_dev``): the device-count collect kernels
against the host-count forms, ``begin_gpu_batch(...).result()`` and ``BatchStream`` against the same ``gpu_batch`` calls bit
for bit, no synchronising call on the way, training fed by the stream, and the loader's errors."""
import copy
import os
import shutil

import numpy as np
import pytest
import torch

import test_loader_golden as tlg
from mm2d3d_amd import _lib, dataprep, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rng_states():
    return np.random.get_state(), torch.get_rng_state()


def _same_rng(a, b):
    (na, ta), (nb, tb) = a, b
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(na, nb)), "numpy RNG state"
    assert torch.equal(ta, tb), "torch RNG state"


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


def _same_value(a, b, what):
    assert type(a) is type(b), f"{what}: {type(a)} != {type(b)}"
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_value(x, y, f"{what}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.device == b.device, f"{what}: {a.device} != {b.device}"
        assert a.dtype == b.dtype, f"{what}: {a.dtype} != {b.dtype}"
        tlg._same(a.cpu().numpy(), b.cpu().numpy(), what)
    elif isinstance(a, np.ndarray):
        tlg._same(a, b, what)
    else:
        assert a == b, what


def _same_batches(g, h):
    assert list(g) == list(h), (list(g), list(h))
    for k in g:
        _same_value(g[k], h[k], k)


def _indices(name):
    z = np.load(os.path.join(tlg.G, f"loader_{name}.npz"))
    return [int(i) for i in z["indices"]], int(z["seed"])


# ---------------------------------------------------------------------------------------------------- collect kernels
def _scene(n, rng, kept):
    """Points of one scene for scale 1, full_scale 64, no translation: all inside the range, or - every point with one
    coordinate far outside while the scene's minimum stays 0 on every axis - all outside."""
    p = rng.uniform(0, 50, (n, 3))
    if not kept:
        far = rng.integers(0, 3, n)
        far[:3] = [0, 1, 2]  # every axis has a point at its minimum and a point far out
        p[np.arange(n), far] = 1000.0
        p[3, :] = [0.0, 0.0, 1000.0]
        p[4, :] = [0.0, 1000.0, 0.0]
        p[5, :] = [1000.0, 0.0, 0.0]
    return p


@pytest.mark.parametrize("mask", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["all_kept", "second_scene_masked", "first_scene_masked", "nothing_kept"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_device_count_collect_equals_the_host_count_form(dtype, mask):
    L = _lib.lib()
    rng = np.random.default_rng(7)
    lengths = [257, 63]  # 320 rows: not a multiple of the 256-thread block, two blocks
    B, n, H, W, C = 2, sum(lengths), 9, 13, 3
    pts = torch.from_numpy(np.concatenate([_scene(m, rng, k) for m, k in zip(lengths, mask)])).to(DEV, dtype)
    rots = [np.eye(3, dtype=np.float32)] * B
    vox = dataprep.voxelize_batch(pts, lengths, rots, [None] * B, scale=1, full_scale=64)
    want = [m if k else 0 for m, k in zip(lengths, mask)]
    assert vox["counts"] == want, (vox["counts"], want)
    kept = sum(want)
    pimg = torch.from_numpy(np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(rng.integers(-100, 10, n)).to(DEV)
    idx_all, _, _, err = dataprep.project_batch(pimg, torch.ones(n, device=DEV), labels, lengths, H, W, [False, True], False, vox["scene_off"])
    image = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)).to(DEV)
    # the workspace-backed outputs of voxelize_batch at their full size (locs / keep beyond `kept` are never read)
    keep_full = torch.zeros(n, dtype=torch.int32, device=DEV)
    keep_full[:kept] = vox["keep"]
    locs_full = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
    locs_full[:kept] = vox["locs"]
    counts = vox["counts_dev"]

    def outputs():
        return (torch.full((n, 2), -7, dtype=torch.int64, device=DEV), torch.full((n,), -7, dtype=torch.int64, device=DEV),
                torch.full((n, C), -7.0, dtype=torch.float32, device=DEV), torch.full((n, 3), -7.0, dtype=dtype, device=DEV))

    ref = outputs()
    host_form = L.mm_collect_points_f64 if dtype == torch.float64 else L.mm_collect_points
    _lib.check(host_form(keep_full.data_ptr(), counts[B:].data_ptr(), kept, locs_full.data_ptr(), idx_all.data_ptr(), labels.data_ptr(),
                         image.data_ptr(), C, H, W, pts.data_ptr(), ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(),
                         ref[3].data_ptr(), _lib.stream()), "collect_points")
    for width, np_dt in ((8, np.int64), (1, np.uint8)):
        got = outputs()
        extra = [torch.from_numpy(rng.integers(0, 120, n).astype(np_dt)).to(DEV) for _ in range(3 if width == 8 else 2)]
        extra_out = [torch.full((n,), 99, dtype=e.dtype, device=DEV) for e in extra]
        pipeline.collect_points_dev(keep_full, counts, B, n, locs_full, idx_all, labels, image, H, W, pts, got[0], got[1], got[2], got[3],
                                    extra, extra_out)
        torch.cuda.synchronize()
        for a, b, what in zip(got, ref, ("img_indices", "labels", "feats", "points")):
            assert torch.equal(a[:kept].view(torch.uint8), b[:kept].view(torch.uint8)), what  # the kept rows, bit for bit
            assert bool((a[kept:] == -7).all()), f"{what}: rows beyond the kept count were written"
            assert bool((b[kept:] == -7).all()), what
        for e, o in zip(extra, extra_out):
            assert torch.equal(o[:kept], e[keep_full[:kept].long()])
            assert bool((o[kept:] == 99).all())
    if kept:  # the kept rows are what the inputs say, not merely the same in both forms
        rows = keep_full[:kept].long()
        assert torch.equal(ref[3][:kept], pts[rows]) and torch.equal(ref[1][:kept], labels[rows])
        assert torch.equal(ref[0][:kept], idx_all[rows])
    assert int(err.item()) == 0


# ---------------------------------------------------------------------------------------------------- batch identity
@pytest.mark.parametrize("image", ["host", "gpu"])
@pytest.mark.parametrize("name", sorted(tlg.CASES))
def test_pending_batch_equals_gpu_batch(name, image):
    ds, _ = tlg._dataset(name)
    idx, seed = _indices(name)
    _seed(seed)
    want = ds.gpu_batch(idx, want_seg2d=True, image=image)
    want_rng = _rng_states()
    _seed(seed)
    pending = ds.begin_gpu_batch(idx, want_seg2d=True, image=image)
    _same_rng(want_rng, _rng_states())
    assert pending.queue() is pending  # idempotent
    got = pending.result()
    assert pending.result() is got
    _same_rng(want_rng, _rng_states())
    _same_batches(got, want)
    if image == "gpu" and ("nuscenes" in name or "a2d2" in name):
        assert len(pending.gpu_idx) == len(idx)  # the JPEG files took the GPU decoder here as well


def test_pending_batch_without_seg2d_and_unqueued():
    ds, _ = tlg._dataset("a2d2_train")
    idx, seed = _indices("a2d2_train")
    _seed(seed)
    want = ds.gpu_batch(idx, image="gpu")
    _seed(seed)
    pending = ds.begin_gpu_batch(idx, image="gpu", queue=False)
    _same_batches(pending.result(), want)  # result() queues what was not queued
    assert "seg_labels_2d" not in want


# ---------------------------------------------------------------------------------------------------- stream identity
def _stream_steps(src, trg, n):
    return [{"source": (src, [k % len(src), (k + 1) % len(src)]), "target": (trg, [(k + 2) % len(trg), k % len(trg), (k + 1) % len(trg)])}
            for k in range(n)]


@pytest.fixture(scope="module")
def sequential_batches():
    src, _ = tlg._dataset("nuscenes_train")
    trg, _ = tlg._dataset("a2d2_train")
    _seed(21)
    out = [{name: ds.gpu_batch(idx, image="gpu") for name, (ds, idx) in step.items()} for step in _stream_steps(src, trg, 4)]
    return out, _rng_states()


@pytest.mark.parametrize("depth", [1, 2])
def test_stream_equals_sequential_gpu_batches(depth, sequential_batches):
    want, want_rng = sequential_batches
    src, _ = tlg._dataset("nuscenes_train")
    trg, _ = tlg._dataset("a2d2_train")
    _seed(21)
    got, announced = [], None
    with pipeline.BatchStream(_stream_steps(src, trg, 4), depth=depth, timing=True, image="gpu") as stream:
        for k, (batch, nxt) in enumerate(stream):
            assert k == 0 or batch is announced
            announced = nxt
            got.append(batch)
    assert announced is None and len(got) == 4
    _same_rng(want_rng, _rng_states())
    for k, (g, w) in enumerate(zip(got, want)):
        assert list(g) == ["source", "target"]
        for name in g:
            _same_batches(g[name], w[name])
    assert len(stream.stats) == 4 and all(s["gpu_ms"] > 0 and s["host_ms"] > 0 for s in stream.stats)


# ---------------------------------------------------------------------------------------------------- no hidden wait
@pytest.mark.parametrize("name", ["nuscenes_train", "skitti_val"])
def test_queue_and_result_make_no_synchronising_call(name):
    """torch's sync debug mode turns every synchronising torch call into an error: ``gpu_batch`` trips it (control), two
    batches queued back to back and - once their events have completed - their ``result()`` do not."""
    ds, _ = tlg._dataset(name)
    idx, seed = _indices(name)
    _seed(seed)
    ds.begin_gpu_batch(idx, want_seg2d=True, image="gpu").result()  # warm: library, workspaces, staging ring
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            ds.gpu_batch(idx, want_seg2d=True, image="gpu")
            tripped = False
        except RuntimeError as e:
            tripped = "synchroniz" in str(e)
            if not tripped:
                raise
        finally:
            torch.cuda.set_sync_debug_mode(old)
        torch.cuda.synchronize()
        if not tripped:
            pytest.skip("this torch build does not raise for gpu_batch's synchronising calls under set_sync_debug_mode('error')")
        torch.cuda.set_sync_debug_mode("error")
        a = ds.begin_gpu_batch(idx, want_seg2d=True, image="gpu")
        b = ds.begin_gpu_batch(idx[::-1], want_seg2d=True, image="host")
        torch.cuda.set_sync_debug_mode(old)
        a.event.synchronize()
        b.event.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        ra, rb = a.result(), b.result()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert ra["x"][0].shape[0] > 0 and rb["x"][0].shape[0] > 0
    assert a.wait_ms < 50 and b.wait_ms < 50


# ---------------------------------------------------------------------------------------------------- training identity
def test_three_steps_fed_by_the_stream_equal_steps_fed_by_gpu_batch():
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    dev = torch.device("cuda:0")
    ds, _ = tlg._dataset("nuscenes_train")
    torch.manual_seed(3)
    kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
    n2, n3 = Net2DSeg(6, pretrained=False).to(dev), Net3DSeg(6, True, kw).to(dev)
    for m in n2.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    n2b, n3b = copy.deepcopy(n2), copy.deepcopy(n3)

    def opts():
        out = {}
        for k in ("2d_net", "3d_net"):
            o = Optimizer("adamw", lr=0.001)
            o.set_scheduler("one_cycle", max_lr=0.005, total_steps=100)
            out[k] = o
        return out

    loss = Loss([{"name": "cross_entropy", "target": "segmentation", "args": {}}])
    tk = dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False)
    piped = TrainModel({"2d_net": n2, "3d_net": n3}, opts(), loss, dict(tk))
    plain = TrainModel({"2d_net": n2b, "3d_net": n3b}, opts(), loss, dict(tk))
    steps = [{"source": (ds, [k % 3, (k + 1) % 3]), "target": (ds, [(k + 2) % 3, k % 3])} for k in range(3)]
    _seed(77)
    la = []
    with pipeline.BatchStream(steps, depth=2, image="gpu") as stream:
        for batch, nxt in stream:
            la.append(float(piped.fit_step(batch, next_batch=nxt).detach()))
    _seed(77)
    lb = []
    for step in steps:
        batch = {name: d.gpu_batch(idx, image="gpu") for name, (d, idx) in step.items()}
        lb.append(float(plain.fit_step(batch).detach()))
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for net, ref in ((n2, n2b), (n3, n3b)):
        for (k, p), (_, q) in zip(net.state_dict().items(), ref.state_dict().items()):
            assert torch.equal(p, q), k


# ---------------------------------------------------------------------------------------------------- errors
def test_damaged_jpeg_raises_from_result_and_from_the_stream(tmp_path):
    """A JPEG whose entropy-coded segment is cut short (header intact, EOI kept: the decoder reports it in its status words and
    reads nothing out of bounds, tests/test_gpu_jpeg.py) raises the loader's RuntimeError naming the file; the stream closes;
    the dataset goes on working."""
    from mm2d3d_amd import datasets, jpeg

    root = str(tmp_path / "nuscenes")
    shutil.copytree(os.path.join(tlg.MINI, "nuscenes"), root)
    cls, sub, kw = tlg.CASES["nuscenes_train"]
    kw = {k: (v.replace("{root}", root) if isinstance(v, str) else v) for k, v in kw.items()}
    ds = getattr(datasets, cls)(**kw)
    path = os.path.join(root, ds.data[1]["camera_path"])
    data = open(path, "rb").read()
    first, end = jpeg.parse(data).entropy
    cut = data[: first + (end - first) // 10] + data[end:]
    assert jpeg.parse(cut).reason is None
    with open(path, "wb") as f:
        f.write(cut)
    name = os.path.basename(path)
    _seed(1)
    with pytest.raises(RuntimeError, match=name):
        ds.gpu_batch([0, 1], image="gpu")  # what the loader raises today
    with pytest.raises(RuntimeError, match=name):
        ds.begin_gpu_batch([0, 1], image="gpu").result()
    stream = pipeline.BatchStream([{"source": (ds, [0, 2])}, {"source": (ds, [1, 2])}, {"source": (ds, [2, 0])}], depth=2, image="gpu")
    seen = []
    with pytest.raises(RuntimeError, match=name):
        for batch, nxt in stream:
            seen.append(batch)
    assert seen == [] and not stream._thread.is_alive()
    _seed(2)
    want = ds.gpu_batch([0, 2], image="gpu")
    _seed(2)
    _same_batches(ds.begin_gpu_batch([0, 2], image="gpu").result(), want)
