"""csrc/jpeg.hip against Pillow on an MI355X: the decoder alone on the CPU tests' matrix and on textures that stress the coder,
``gpu_batch(image="gpu")`` with every JPEG decoded on the GPU against the reference fixtures and ``image="host"``, batches
that mix GPU- and host-decoded images, and a corrupted entropy-coded segment."""
import importlib.util
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import test_jpeg_host as hj
import test_loader_golden as tlg
from mm2d3d_amd import dataprep, imageprep

pytestmark = pytest.mark.gpu
JPEG_CASES = [c for c in tlg.GPU_CASES if "nuscenes" in c or "a2d2" in c]


def _gpu_decode(paths):
    """Every file through mm_jpeg_decode in one batch -> (list of uint8 [H][W][3], status words)."""
    plans = [imageprep.ImagePlan(Image.open(p)) for p in paths]
    data, offs, headers = dataprep.read_jpegs(plans)
    assert all(h is not None and h.reason is None for h in headers), [h.reason for h in headers]
    src_offs = dataprep.source_offsets(plans)
    n = sum(p.image.size[0] * p.image.size[1] * 3 for p in plans)
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    status = dataprep._decode_jpegs(plans, list(range(len(plans))), headers, data, offs, src, src_offs, torch.device("cuda"), None)
    out, st = src.cpu().numpy(), status.cpu().numpy()
    imgs = [out[o : o + p.image.size[0] * p.image.size[1] * 3].reshape(p.image.size[1], p.image.size[0], 3) for o, p in zip(src_offs, plans)]
    return imgs, st


def _check(files):
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, data in enumerate(files):
            paths.append(os.path.join(d, f"{i}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(data)
        got, st = _gpu_decode(paths)
        assert not st.any(), st
        for i, (g, data) in enumerate(zip(got, files)):
            assert np.array_equal(g, hj.pil(data)), i


@pytest.mark.parametrize("case,kw", hj.matrix(), ids=[c for c, _ in hj.matrix()])
def test_decoder_equals_pil_on_the_matrix(case, kw):
    _check([hj.encode(hj.texture(*size, kind="smooth", seed=size[1]), **kw) for size in hj.SIZES])


def test_decoder_equals_pil_on_hard_textures():
    files = []
    for kind in ("noise", "flat", "edges", "smooth"):
        for s in (0, 1, 2):
            for q in (50, 100):
                files.append(hj.encode(hj.texture(203, 77, kind=kind, seed=s), quality=q, subsampling=s))
    assert any(b"\xff\x00" in f[hj.jpeg.parse(f).entropy[0] :] for f in files)
    _check(files)


def test_decoder_equals_pil_at_1600x900():
    a = hj.texture(1600, 900, kind="smooth", seed=3)
    a = np.clip(a.astype(np.int16) + np.random.default_rng(3).integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    _check([hj.encode(a, quality=90, subsampling=s) for s in (0, 1, 2)] + [hj.encode(a, quality=95, restart_marker_rows=2)])


def test_corrupted_entropy_segment_raises():
    """Header intact, entropy-coded data cut short (EOI kept): the status words report it, nothing is read out of bounds."""
    data = hj.encode(hj.texture(96, 64, kind="noise", seed=9), quality=100)
    first, end = hj.jpeg.parse(data).entropy
    cut = data[: first + (end - first) // 10] + data[end:]
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "broken.jpg")
        with open(p, "wb") as f:
            f.write(cut)
        plan = imageprep.ImagePlan(Image.open(p))
        assert hj.jpeg.parse(cut).reason is None
        with pytest.raises(RuntimeError, match="broken.jpg"):
            dataprep.prepare_images([plan], [None], [False], [np.zeros((3, 256), np.float32)], "cuda")


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


@pytest.mark.parametrize("name", JPEG_CASES)
def test_gpu_decoded_batch_equals_the_reference_and_the_host_batch(name):
    z = np.load(os.path.join(tlg.G, f"loader_{name}.npz"))
    ds, kw = tlg._dataset(name)
    idx = [int(i) for i in z["indices"]]
    np.random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    timing = {}
    g = ds.gpu_batch(idx, want_seg2d=True, image="gpu", timing=timing)
    g_rng = _rng_states()
    assert timing["gpu_decoded"] == len(idx) and timing["host_decoded"] == 0, timing
    tlg._same(g["img"].cpu().numpy(), z["batch/img"], "img")
    np.random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    h = ds.gpu_batch(idx, want_seg2d=True, image="host")
    _same_rng(g_rng, _rng_states())
    _same_batches(g, h)


def test_sixteen_nuscenes_sized_scenes_and_a_mixed_batch_equal_the_host_path():
    """16 scenes of 1600x900 JPEGs -> 400x225, all decoded on the GPU; then with two files re-written as a progressive JPEG
    and a PNG (host decode) in the same batch."""
    spec = importlib.util.spec_from_file_location("bench_imageprep", os.path.join(tlg.G, "..", "..", "tools", "bench_imageprep.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from mm2d3d_amd import datasets

    def both(ds, idx, seed):
        np.random.seed(seed)
        torch.manual_seed(seed)
        timing = {}
        g = ds.gpu_batch(idx, want_seg2d=True, image="gpu", decode_threads=4, timing=timing)
        g_rng = _rng_states()
        np.random.seed(seed)
        torch.manual_seed(seed)
        h = ds.gpu_batch(idx, want_seg2d=True, image="host")
        _same_rng(g_rng, _rng_states())
        _same_batches(g, h)
        return timing

    with tempfile.TemporaryDirectory() as root:
        cls, kw = bench.make_dataset(root, "nuscenes")
        ds = getattr(datasets, cls)(**kw)
        idx = [(7 * i) % len(ds) for i in range(16)]
        t = both(ds, idx, 5)
        assert t["gpu_decoded"] == 16 and t["host_decoded"] == 0, t
        paths = sorted({os.path.join(root, ds.data[i]["camera_path"]) for i in idx})
        im = Image.open(paths[0]).convert("RGB")
        im.save(paths[0] + ".tmp", "JPEG", quality=85, progressive=True)
        shutil.move(paths[0] + ".tmp", paths[0])
        Image.open(paths[1]).convert("RGB").save(paths[1] + ".tmp", "PNG", compress_level=1)
        shutil.move(paths[1] + ".tmp", paths[1])
        t = both(ds, idx, 6)
        n_host = sum(os.path.join(root, ds.data[i]["camera_path"]) in paths[:2] for i in idx)
        assert 0 < t["host_decoded"] == n_host and t["gpu_decoded"] == 16 - n_host, t
