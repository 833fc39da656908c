"""Host side of the pipelined loader (mm2d3d_amd/pipeline.py) without a GPU: the host phase draws what ``ds[i]`` draws, the
staging blocks hold what was packed at 16-byte offsets, and ``BatchStream`` orders host phases, queues and yields as documented."""
import os
import threading

import numpy as np
import pytest
import torch

import test_loader_golden as tlg
from mm2d3d_amd import dataprep, pipeline

RNG_CASES = ["nuscenes_train", "vkitti_rand_crop", "skitti_rand_crop"]


def _rng_states():
    return np.random.get_state(), torch.get_rng_state()


def _same_rng(a, b):
    (na, ta), (nb, tb) = a, b
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(na, nb)), "numpy RNG state"
    assert torch.equal(ta, tb), "torch RNG state"


def _indices(name):
    return [int(i) for i in np.load(f"{tlg.G}/loader_{name}.npz")["indices"]]


@pytest.mark.parametrize("image", ["host", "gpu"])
@pytest.mark.parametrize("name", RNG_CASES)
def test_host_phase_leaves_the_rng_states_of_the_host_loader(name, image):
    ds, _ = tlg._dataset(name)
    idx = _indices(name)
    np.random.seed(11)
    torch.manual_seed(11)
    [ds[i] for i in idx]
    want = _rng_states()
    np.random.seed(11)
    torch.manual_seed(11)
    p = ds.begin_gpu_batch(idx, image=image, queue=False)
    try:
        _same_rng(want, _rng_states())
        assert p.f64 == (name == "vkitti_rand_crop")
    finally:
        p.cancel()


@pytest.mark.parametrize("image", ["host", "gpu"])
@pytest.mark.parametrize("name", RNG_CASES)
def test_scene_loop_leaves_the_rng_states_of_the_host_loader(name, image):
    """``_Scenes._draw_scenes``, the scene loop of ``gpu_batch`` and of the pipelined loader, on its own."""
    ds, _ = tlg._dataset(name)
    idx = _indices(name)
    np.random.seed(11)
    torch.manual_seed(11)
    [ds[i] for i in idx]
    want = _rng_states()
    np.random.seed(11)
    torch.manual_seed(11)
    d = ds._draw_scenes(idx, image == "gpu")
    _same_rng(want, _rng_states())
    assert ds._plan_images is False
    assert all(len(v) == len(idx) for v in (d.scenes, d.works, d.intrinsics, d.flips, d.rots, d.us))
    assert len(d.jitter) == (len(idx) if image == "gpu" else 0)
    H, W = d.HW
    assert all(("img" not in s) if image == "gpu" else (s["img"].shape == (3, H, W)) for s in d.scenes)


@pytest.mark.parametrize("on_gpu", [False, True])
def test_scene_loop_resets_the_image_plans_when_a_scene_raises(on_gpu):
    ds, _ = tlg._dataset("skitti_rand_crop")
    idx = _indices("skitti_rand_crop")
    ds.data[idx[1]] = dict(ds.data[idx[1]], seg_labels=None)  # an unlabelled scene (a test split), after a labelled one
    with pytest.raises(ValueError) as e:
        ds._draw_scenes(idx, on_gpu)
    assert str(e.value) == "gpu_batch needs labelled scenes (the 2D label map and seg_label are part of the batch)"
    assert ds._plan_images is False


def test_jpeg_read_helpers_fill_a_caller_buffer_as_read_jpegs_fills_its_own(tmp_path):
    from PIL import Image

    from mm2d3d_amd import imageprep, jpeg

    ds, _ = tlg._dataset("nuscenes_train")
    paths = [os.path.join(tlg.MINI, "nuscenes", d["camera_path"]) for d in ds.data]
    cut = str(tmp_path / "cut.jpg")
    with open(paths[0], "rb") as f:
        data = f.read()
    with open(cut, "wb") as f:
        f.write(data)
    paths.insert(1, cut)
    plans = [imageprep.ImagePlan(Image.open(p)) for p in paths]  # PIL has read the headers: the plans know format and size
    with open(cut, "wb") as f:
        f.write(data[: jpeg.parse(data).entropy[0] - 20])  # the file now ends inside its header
    pinned, offs, want = dataprep.read_jpegs(plans)
    files, file_offs = dataprep.jpeg_files(plans)
    assert files == paths
    assert file_offs.dtype == np.int64 and list(file_offs) == [0] + list(np.cumsum([os.path.getsize(p) for p in paths]))
    tlg._same(file_offs[:-1], offs, "offsets")
    total = int(file_offs[-1])
    buf = np.full(total + 7, 0xAB, np.uint8)
    got = dataprep.read_jpeg_files(files, file_offs, buf)
    contents = []
    for p in paths:
        with open(p, "rb") as f:
            contents.append(f.read())
    assert bytes(buf[:total]) == b"".join(contents) and bytes(pinned.numpy()[:total]) == b"".join(contents)
    assert bool((buf[total:] == 0xAB).all())  # nothing written past the files
    assert len(got) == len(want) == len(paths)
    for g, w in zip(got, want):
        for field in jpeg.JpegHeader.__slots__:
            assert repr(getattr(g, field)) == repr(getattr(w, field)), field
    assert got[1].reason.startswith("header:") and "cut.jpg" in got[1].reason
    assert [h.reason for i, h in enumerate(got) if i != 1] == [None] * (len(paths) - 1)
    assert got[0].size == Image.open(paths[0]).size and got[0].entropy is not None
    assert dataprep.split_decoders(got) == ([i for i in range(len(paths)) if i != 1], [1])
    assert dataprep.split_decoders([None, got[0], None]) == ([1], [0, 2])


@pytest.mark.parametrize("name,image", [("nuscenes_train", "gpu"), ("skitti_bottom_crop", "host"), ("vkitti_rand_crop", "gpu"),
                                        ("nuscenes_val_pselab", "gpu")])
def test_host_phase_packs_the_arrays_of_the_scene_loop(name, image):
    """What the kernels will read is what ``gpu_batch`` would have uploaded: checked against the scene loop run again."""
    ds, _ = tlg._dataset(name)
    idx = _indices(name)
    np.random.seed(5)
    torch.manual_seed(5)
    p = ds.begin_gpu_batch(idx, image=image, queue=False)
    try:
        for block in (p.small, p.images):
            assert block.layout and block.nbytes <= block.buf.numel()
            ends = 0
            for key, (off, dtype, shape) in block.layout.items():
                assert off % 16 == 0 and off >= ends, key
                ends = off + dtype.itemsize * int(np.prod(shape))
        np.random.seed(5)
        torch.manual_seed(5)
        ds._plan_images = image == "gpu"
        try:
            pts, lab, pimg = [], [], []
            for i in idx:
                w = ds._front(i)
                if image == "gpu":
                    if ds.color_jitter is not None:
                        ds.color_jitter.draw()
                else:
                    ds._float_image(w.image)
                np.random.rand()
                dataprep.augmentation_draws(**ds._augmentation())
                pts.append(w.points), lab.append(w.label), pimg.append(np.trunc(w.pimg))
        finally:
            ds._plan_images = False
        sm = p.small
        assert sm.host("points").dtype == (np.float64 if name == "vkitti_rand_crop" else np.float32)
        tlg._same(sm.host("points"), np.concatenate(pts).astype(sm.host("points").dtype), "points")
        tlg._same(sm.host("labels"), np.concatenate(lab).astype(np.int64), "labels")
        tlg._same(sm.host("pimg"), np.concatenate(pimg).astype(np.float32), "pimg")
        tlg._same(sm.host("off"), np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int32), "off")
        tlg._same(sm.host("rot"), np.stack(p.rots).reshape(len(idx), 9), "rot")
        tlg._same(sm.host("flip"), np.array(p.flips, np.uint8), "flip")
        if name == "nuscenes_val_pselab":
            assert p.pselab[:2] == ["pseudo_label_2d", "pseudo_label_ensemble"]
            for key in p.pselab:
                assert sm.host(key).shape == (p.n,)
        if image == "gpu":
            assert sm.host("img_desc").shape == (len(idx), 16) and sm.host("img_lut").shape == (len(idx), 3, 256)
            assert len(p.gpu_idx) + len(p.host_idx) == len(idx)
        else:
            assert p.images.host("img").shape[:2] == (len(idx), 3)
    finally:
        p.cancel()


def test_block_views_read_back_what_was_packed_at_aligned_offsets():
    rng = np.random.default_rng(0)
    arrays = {
        "a": rng.integers(0, 255, 7, dtype=np.uint8), "b": rng.standard_normal((5, 3)), "c": rng.integers(-9, 9, 3).astype(np.int32),
        "d": rng.standard_normal((2, 3, 5)).astype(np.float32), "e": rng.integers(-100, 20, 11), "f": np.zeros((0, 3), np.float32),
        "g": rng.integers(0, 2, 1, dtype=np.uint8),
    }
    ring = pipeline.PinnedRing()
    blk = pipeline.Block(ring)
    for k, v in arrays.items():
        blk.add(k, v)
    off_r = blk.reserve("r", np.uint8, (33,))
    blk.seal()
    blk.host("r")[...] = np.arange(33, dtype=np.uint8)
    assert off_r % 16 == 0
    whole = blk.buf[: blk.nbytes].clone()  # what an upload would carry
    for k, v in arrays.items():
        off, dtype, shape = blk.layout[k]
        assert off % 16 == 0 and dtype == v.dtype and shape == v.shape
        tlg._same(blk.host(k), v, k)
        tlg._same(blk.device(whole, k).numpy(), v, k + " through the block view")
    tlg._same(blk.device(whole, "r").numpy(), np.arange(33, dtype=np.uint8), "r")
    buf = blk.buf
    blk.release()
    assert ring.acquire(16) is buf  # nothing in flight: reusable at once


class _Event:
    def __init__(self):
        self.done = False

    def query(self):
        return self.done


def test_ring_reuses_a_block_only_after_its_event():
    ring = pipeline.PinnedRing()
    a = ring.acquire(100)
    ev = _Event()
    ring.release(a, ev)
    ring.reclaim()
    b = ring.acquire(100)
    assert b is not a
    ev.done = True
    ring.reclaim()
    assert ring.acquire(100) is a
    assert ring.acquire(10 * a.numel()).numel() >= 10 * a.numel()
    bufs = [ring.acquire(5000 * (k + 1)) for k in range(ring.KEEP + 3)]  # more free buffers than the ring keeps: the smallest go
    for buf in bufs:
        ring.release(buf)
    assert len(ring._free) == ring.KEEP and min(b.numel() for b in ring._free) > bufs[0].numel()


# ---------------------------------------------------------------------------------------------------- stream ordering (fakes)
class _Pending:
    def __init__(self, ds, indices):
        self.ds, self.indices, self.queued, self.cancelled = ds, list(indices), False, False
        self.batch = {"who": ds.name, "indices": self.indices}

    def queue(self):
        self.ds.log.append(("queue", self.ds.name, self.indices[0], threading.current_thread().name))
        self.queued = True
        return self

    def result(self):
        assert self.queued
        self.ds.log.append(("result", self.ds.name, self.indices[0]))
        if self.ds.fail_result == self.indices[0]:
            raise RuntimeError("result failed")
        return self.batch

    def cancel(self):
        self.cancelled = True


class _FakeDataset:
    def __init__(self, name, log, fail_host=None, fail_result=None):
        self.name, self.log, self.fail_host, self.fail_result, self.made = name, log, fail_host, fail_result, []

    def begin_gpu_batch(self, indices, queue=True, **kw):
        assert queue is False and kw == {"image": "gpu"}
        self.log.append(("host", self.name, indices[0], threading.current_thread().name))
        if self.fail_host == indices[0]:
            raise ValueError("front end failed")
        self.made.append(_Pending(self, indices))
        return self.made[-1]


def _steps(src, trg, n):
    return [{"source": (src, [k, k + 100]), "target": (trg, [k, k + 200])} for k in range(n)]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_stream_orders_host_phases_and_keeps_depth_batches_queued_ahead(depth):
    log = []
    src, trg = _FakeDataset("s", log), _FakeDataset("t", log)
    n = 6
    main = threading.current_thread().name
    seen, prev_next = [], None
    with pipeline.BatchStream(_steps(src, trg, n), depth=depth, image="gpu") as stream:
        for k, (batch, nxt) in enumerate(stream):
            assert list(batch) == ["source", "target"] and batch["source"]["indices"] == [k, k + 100]
            if k:
                assert batch is prev_next  # the very object announced as next_batch
            assert (nxt is None) == (k == n - 1)
            prev_next = nxt
            queued = {e[2] for e in log if e[0] == "queue"}
            assert max(queued) <= k + depth, (k, sorted(queued))
            assert max(queued) == min(k + depth, n - 1)  # and not fewer: the stream stays ahead
            seen.append(k)
    assert seen == list(range(n))
    hosts = [e for e in log if e[0] == "host"]
    assert [(e[1], e[2]) for e in hosts] == [(w, k) for k in range(n) for w in ("s", "t")]  # step order, dict order
    assert all(e[3] != main for e in hosts) and len({e[3] for e in hosts}) == 1
    queues = [e for e in log if e[0] == "queue"]
    assert [(e[1], e[2]) for e in queues] == [(w, k) for k in range(n) for w in ("s", "t")]
    assert all(e[3] == main for e in queues)
    assert not stream._thread.is_alive()


def test_worker_exception_surfaces_from_the_iteration_and_closes_the_stream():
    log = []
    src, trg = _FakeDataset("s", log), _FakeDataset("t", log, fail_host=2)
    stream = pipeline.BatchStream(_steps(src, trg, 5), depth=2, image="gpu")
    got = []
    with pytest.raises(ValueError, match="front end failed"):
        for batch, nxt in stream:
            got.append(batch["source"]["indices"][0])
    assert got == [0]  # step 1 needs step 2 as its next_batch
    assert not stream._thread.is_alive()
    assert src.made[2].cancelled  # the half-made step gave its staging back
    assert ("host", "s", 3) not in [(e[0], e[1], e[2]) for e in log]


def test_result_error_surfaces_and_closes_the_stream():
    log = []
    src, trg = _FakeDataset("s", log, fail_result=1), _FakeDataset("t", log)
    stream = pipeline.BatchStream(_steps(src, trg, 8), depth=1, image="gpu")
    with pytest.raises(RuntimeError, match="result failed"):
        for batch, nxt in stream:
            pass
    assert not stream._thread.is_alive()
    with pytest.raises(RuntimeError, match="iterated once"):
        iter(stream)


def test_close_joins_the_thread_and_drops_what_is_in_flight():
    log = []
    src, trg = _FakeDataset("s", log), _FakeDataset("t", log)
    stream = pipeline.BatchStream(_steps(src, trg, 50), depth=2, image="gpu")
    it = iter(stream)
    batch, nxt = next(it)
    assert batch["source"]["indices"][0] == 0 and nxt["source"]["indices"][0] == 1
    stream.close()
    assert not stream._thread.is_alive()
    hosted = len(src.made)
    assert hosted < 50
    assert all(p.queued or p.cancelled for p in src.made)  # whatever was hosted and not queued was cancelled
    stream.close()  # idempotent
    assert len(src.made) == hosted
    with pytest.raises(StopIteration):
        next(it)


def test_empty_stream_yields_nothing():
    with pipeline.BatchStream([], depth=2) as stream:
        assert list(stream) == []
    assert not stream._thread.is_alive()
