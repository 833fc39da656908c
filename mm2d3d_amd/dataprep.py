"""GPU-side sample preparation and collation (csrc/dataprep.hip).

The reference prepares every sample in DataLoader workers with numpy (``NuScenesLidarSegSCN.__getitem__``,
lib/dataset/nuscenes_dataloader.py:236-369; ``augment_and_scale_3d``, lib/utils/augmentation_3d.py:83-158) and
collates on the host (``collate_scn_base``, lib/dataset/__init__.py:27-123).  Once a training step takes ~50 ms for 16
scenes that host path is the next wall, so here the per-point work of a whole batch runs as a short chain of HIP kernels
on arrays that were uploaded once (pinned host buffers -> device), and the result is the reference's batch dict, on the
device, bit-identical to the host restatement (mm2d3d_amd/projection.py + synthetic.collate):

    host (O(1) per scene, the reference's numpy RNG order)     device (per point / per pixel)
    -----------------------------------------------------     -------------------------------------------------------
    fliplr draw, rotation matrix, rand(3) translation draws     points.rot, *scale, -min, +offset, int cast, range mask,
    image decode / resize / normalise (caller), or the          order-preserving compaction + batch index column (a1, a2)
    decode only (prepare_images)                                pixel indices, fliplr remap, last-write-wins depth and
                                                                2D label maps, RGB features under the points (a16)
                                                                prepare_images: crop, resize, jitter, float, fliplr,
                                                                normalisation (csrc/imageprep.hip)
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream


def augmentation_draws(noisy_rot=0.0, flip_x=0.0, flip_y=0.0, rot_z=0.0, rot_y=0.0, transl=False):
    """The random part of ``augment_and_scale_3d`` (augmentation_3d.py:106-155) in the reference's draw order:
    randn(3,3) | randint x | randint y | rand z | rand y | rand(3).  Returns (rot float32 [3,3], u float64 [3] or None)."""
    rot = np.eye(3, dtype=np.float32)
    if noisy_rot > 0:
        rot += np.random.randn(3, 3) * noisy_rot
    if flip_x > 0:
        rot[0][0] *= np.random.randint(0, 2) * 2 - 1
    if flip_y > 0:
        rot[1][1] *= np.random.randint(0, 2) * 2 - 1
    if rot_z > 0:
        t = np.random.rand() * rot_z
        c, s = np.cos(t), np.sin(t)
        rot = rot.dot(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32))
    if rot_y > 0:
        t = np.random.rand() * rot_y
        c, s = np.cos(t), np.sin(t)
        rot = rot.dot(np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float32))
    u = np.random.rand(3) if transl else None
    return rot, u


PSELAB_KEYS = ("pseudo_label_2d", "pseudo_label_ensemble", "pseudo_label_3d")  # the order the loaders' batches carry them in


def scene_offsets(lengths):
    """int32 [B+1]: first row of every scene in the concatenated per-point arrays, and the total."""
    off = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=off[1:])
    return off


def _offsets(lengths, dev):
    off = scene_offsets(lengths)
    return off, torch.from_numpy(off).to(dev)


def draw_tables(rots, us):
    """The draws as the voxelisation kernels read them: (rot fp32 [B,9], u fp64 [B,3] or zeros, whether u was drawn)."""
    transl = any(u is not None for u in us)
    if transl and not all(u is not None for u in us):
        raise ValueError("voxelize_batch: translation must be drawn for every scene of the batch or for none")
    rot = np.stack([np.asarray(r, np.float32).reshape(9) for r in rots])
    return rot, np.stack([np.asarray(u if u is not None else np.zeros(3), np.float64) for u in us]), transl


def scene_arrays(scenes):
    """Yields the per-point inputs of the kernels, scenes back to back, as contiguous numpy arrays: points [n,3], points_img
    fp32 [n,2], depth fp32 [n], seg_label int64 [n]; one at a time, so a caller that uploads each as it comes holds only one.
    float64 points (VirtualKITTI with camera_coords) stay float64 and take the fp64 kernels; any other dtype becomes float32."""
    f64 = [np.asarray(s["points"]).dtype == np.float64 for s in scenes]
    if any(f64) and not all(f64):
        raise ValueError("prepare_batch: the scenes of one batch must all have float64 points or none (the reference voxelises "
                         "float64 and float32 points with different arithmetic)")
    pdt = np.float64 if any(f64) else np.float32
    for key, dt in (("points", pdt), ("points_img", np.float32), ("depth", np.float32), ("seg_label", np.int64)):
        yield np.ascontiguousarray(np.concatenate([np.asarray(s[key]) for s in scenes], 0).astype(dt))


# One launcher per entry point of csrc/dataprep.hip, jpeg.hip and imageprep.hip, for both loaders.  Every tensor already lives on
# the device (``desc``: the host copy of ``desc_d``); nothing is allocated besides the workspace, copied or waited for.
def _launch_voxelize(points, off_d, off_h, rot_d, u_d, transl, scale, full_scale, locs, keep, counts, minv, offset):
    L = _lib.lib()
    B = len(off_h) - 1
    ws_bytes, run = ((L.mm_voxelize_ws_bytes_f64, L.mm_voxelize_batch_f64) if points.dtype == torch.float64 else
                     (L.mm_voxelize_ws_bytes, L.mm_voxelize_batch))
    ws = _lib.workspace.get(int(ws_bytes(int(off_h[B]), B)), points.device)
    check(run(ptr(points), ptr(off_d), off_h.ctypes.data, B, ptr(rot_d), ptr(u_d), 1 if transl else 0, float(scale), int(full_scale),
              ptr(locs), ptr(keep), ptr(counts), ptr(minv), ptr(offset), ptr(ws), ws.numel(), stream()), "voxelize_batch")


def _launch_project(points_img, depth_vals, labels, off_d, off_h, flip_d, idx, depth, seg2d, winner, err):
    B, _, H, W = depth.shape
    check(_lib.lib().mm_project_batch(ptr(points_img), ptr(depth_vals), ptr(labels), ptr(off_d), off_h.ctypes.data, B, H, W, ptr(flip_d),
                                      ptr(idx), ptr(depth), ptr(seg2d), ptr(winner), ptr(err), stream()), "project_batch")


def _launch_jpeg_decode(data_d, desc_d, desc, huff_d, qt_d, totals, src, status):
    L = _lib.lib()
    nj = status.numel()  # totals: the four counts of jpeg.build_tables
    ws = _lib.workspace.get(int(L.mm_jpeg_ws_bytes(nj, data_d.numel(), *totals)), src.device, "jpeg")
    check(L.mm_jpeg_decode(ptr(data_d), data_d.numel(), ptr(desc_d), desc.ctypes.data, nj, ptr(huff_d), huff_d.shape[0], ptr(qt_d),
                           qt_d.shape[0], ptr(src), src.numel(), ptr(status), ptr(ws), ws.numel(), stream()), "jpeg_decode")


def _launch_image_prepare(src, src_bytes, desc_d, desc, coef_d, fac_d, lut_d, tmp, mid, sums, img):
    B, _, H, W = img.shape  # src_bytes: the decoded bytes of the batch (src may be longer)
    check(_lib.lib().mm_image_prepare(ptr(src), src_bytes, ptr(desc_d), desc.ctypes.data, B, H, W, ptr(coef_d), coef_d.numel(), ptr(fac_d),
                                      ptr(lut_d), ptr(tmp), tmp.numel(), ptr(mid), ptr(sums), ptr(img), stream()), "image_prepare")


def collect_points(keep, total_d, kept, locs, idx_all, labels, image, H, W, points, idx_out, lab_out, feats_out, points_out):
    """``mm_collect_points`` / ``_f64`` (csrc/dataprep.hip): the rows ``keep[:kept]`` of the per-point arrays and the RGB features
    under them (``feats_out`` None: none) gathered into the outputs; ``total_d``: the device word that holds ``kept``."""
    L = _lib.lib()
    fn = L.mm_collect_points_f64 if points.dtype == torch.float64 else L.mm_collect_points
    check(fn(ptr(keep), ptr(total_d), kept, ptr(locs), ptr(idx_all), ptr(labels), ptr(image), image.shape[1], H, W, ptr(points),
             ptr(idx_out), ptr(lab_out), ptr(feats_out), ptr(points_out), stream()), "collect_points")


def collect_points_dev(keep, counts, B, n_total, locs, idx_all, labels, image, H, W, points, idx_out, lab_out, feats_out, points_out,
                       extra_in=(), extra_out=()):
    """``mm_collect_points_dev`` / ``_f64_dev`` (csrc/dataprep.hip): :func:`collect_points` launched over ``n_total`` rows with
    the kept total read from ``counts[B]`` on the device; ``extra_in`` -> ``extra_out``: up to three per-point arrays of one
    dtype gathered by ``keep`` in the same launch.  Any of labels / feats / points outputs may be None."""
    L = _lib.lib()
    _lib.require_cuda(keep, "keep")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError("collect_points_dev: points must be float32 or float64")
    if len(extra_in) != len(extra_out) or len(extra_in) > 3:
        raise ValueError("collect_points_dev: at most three extra arrays, one output each")
    for a, b in zip(extra_in, extra_out):
        if a.dtype != b.dtype or a.dtype != extra_in[0].dtype or a.numel() < n_total or b.numel() < n_total or not (
                a.is_contiguous() and b.is_contiguous()):
            raise ValueError("collect_points_dev: extra arrays must be contiguous, of one dtype and hold n_total elements")
    for t, rows in ((keep, 1), (locs, 4), (idx_all, 2), (idx_out, 2), (lab_out, 1), (points, 3), (points_out, 3)):
        if t is not None and t.numel() < n_total * rows:
            raise ValueError("collect_points_dev: an array is shorter than n_total rows")
    if counts.numel() < B + 1:
        raise ValueError("collect_points_dev: counts holds B + 1 words")
    C = 0
    if feats_out is not None:
        C = int(image.shape[1])
        if feats_out.numel() < n_total * C:
            raise ValueError("collect_points_dev: feats_out is shorter than n_total rows")
    ne = len(extra_in)
    arr = ctypes.c_void_p * max(ne, 1)
    ein, eout = arr(*[t.data_ptr() for t in extra_in]), arr(*[t.data_ptr() for t in extra_out])
    fn = L.mm_collect_points_f64_dev if points.dtype == torch.float64 else L.mm_collect_points_dev
    check(fn(ptr(keep), ptr(counts), int(B), int(n_total), ptr(locs), ptr(idx_all), ptr(labels), ptr(image), C, int(H), int(W), ptr(points),
             ptr(idx_out), ptr(lab_out), ptr(feats_out), ptr(points_out), ctypes.cast(ein, ctypes.c_void_p),
             ctypes.cast(eout, ctypes.c_void_p), ne, extra_in[0].element_size() if ne else 0, stream()), "collect_points_dev")
    return idx_out


def voxelize_batch(points, lengths, rots, us, scale=20, full_scale=4096):
    """points fp32 or fp64 [n_total,3] on the GPU (scenes back to back), lengths = points per scene, rots / us = the
    per-scene draws of :func:`augmentation_draws`.  Returns dict(locs int64 [kept,4], keep int32 [kept], counts list,
    min_value [B,3] of the points' dtype, offset fp64 [B,3]); one small device->host copy (the kept counts) sizes the
    outputs.  fp64 points (VirtualKITTI with camera_coords) follow numpy's float64 arithmetic (mm_voxelize_batch_f64)."""
    _lib.require_cuda(points, "points")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError("voxelize_batch: points must be float32 (the dtype the reference's pickles hold) or float64 (VirtualKITTI "
                        "with camera_coords)")
    dev = points.device
    points = points.contiguous()
    B, n = len(lengths), int(sum(lengths))
    assert points.shape == (n, 3)
    off_h, off_d = _offsets(lengths, dev)
    rot, u, transl = draw_tables(rots, us)
    rot_d, u_d = torch.from_numpy(rot).to(dev), torch.from_numpy(u).to(dev)
    locs = torch.empty((n, 4), dtype=torch.int64, device=dev)
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    counts = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    minv = torch.empty((B, 3), dtype=points.dtype, device=dev)
    offset = torch.empty((B, 3), dtype=torch.float64, device=dev)
    _launch_voxelize(points, off_d, off_h, rot_d, u_d, transl, scale, full_scale, locs, keep, counts, minv, offset)
    ch = counts.cpu().tolist()  # the only read-back: how many points survived the range mask
    kept = ch[B]
    return dict(locs=locs[:kept], keep=keep[:kept], counts=ch[:B], counts_dev=counts, min_value=minv, offset=offset,
                scene_off=(off_h, off_d))


def project_batch(points_img, depth_vals, labels, lengths, H, W, flips=None, want_seg2d=False, scene_off=None):
    """points_img fp32 [n_total,2] (row, col; already scaled to the network image), depth_vals fp32 [n_total] (camera z).
    Returns (img_indices int64 [n_total,2], depth fp32 [B,1,H,W], seg2d fp64 [B,H,W] or None)."""
    _lib.require_cuda(points_img, "points_img")
    dev = points_img.device
    B = len(lengths)
    off_h, off_d = scene_off if scene_off is not None else _offsets(lengths, dev)
    n = int(off_h[B])
    points_img = points_img.to(torch.float32).contiguous()
    depth_vals = depth_vals.to(torch.float32).contiguous()
    flip_d = torch.tensor([1 if f else 0 for f in flips], dtype=torch.uint8, device=dev) if flips is not None and any(flips) else None
    idx = torch.empty((n, 2), dtype=torch.int64, device=dev)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    seg2d = torch.empty((B, H, W), dtype=torch.float64, device=dev) if want_seg2d else None
    winner = torch.empty(B * H * W, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _launch_project(points_img, depth_vals, labels, off_d, off_h, flip_d, idx, depth, seg2d, winner, err)
    return idx, depth, seg2d, err


GPU_JPEG = True  # eligible JPEG files decode on the GPU (csrc/jpeg.hip); False: every image on the host (the benchmark's A/B lever)


def source_sizes(plans):  # bytes of each plan's decoded [H][W][3] image
    return [p.image.size[0] * p.image.size[1] * 3 for p in plans]


def source_offsets(plans):
    """Byte offset of each plan's decoded [H][W][3] image in the source buffer: the images back to back in batch order."""
    return np.concatenate([[0], np.cumsum(source_sizes(plans))[:-1]]).astype(np.int64)


def jpeg_files(plans):
    """(the file behind each plan whose image is a JPEG file, else None; int64 [B+1] offsets of the files back to back)."""
    from . import jpeg

    paths = [jpeg.jpeg_file(p.image) for p in plans]
    sizes = [os.path.getsize(f) if f is not None else 0 for f in paths]
    return paths, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def read_jpeg_files(paths, offs, buf):
    """Reads the files of :func:`jpeg_files` into the uint8 numpy buffer ``buf`` (at least ``offs[-1]`` bytes) and parses their
    headers: :class:`jpeg.JpegHeader` per path, None where the path is None.  A file whose header :func:`jpeg.parse` rejects
    (truncated or inconsistent) gets a header whose ``reason`` says why: it goes to the host decode, where PIL decides as it did
    before, and never reaches a kernel."""
    from . import jpeg

    headers = []
    for i, f in enumerate(paths):
        if f is None:
            headers.append(None)
            continue
        part = buf[offs[i] : offs[i + 1]]
        jpeg.read_into(f, part)
        try:
            headers.append(jpeg.parse(part, f))
        except ValueError as e:
            h = jpeg.JpegHeader()
            h.reason = f"header: {e}"
            headers.append(h)
    return headers


def read_jpegs(plans):
    """:func:`jpeg_files` + :func:`read_jpeg_files` into one pinned buffer.  Returns (pinned uint8 tensor, byte offset per plan,
    header or None per plan)."""
    paths, offs = jpeg_files(plans)
    data = torch.empty(max(int(offs[-1]), 1), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    return data, offs[:-1], read_jpeg_files(paths, offs, data.numpy())


def split_decoders(headers):
    """(gpu_idx, host_idx): the plans the GPU decoder takes (a header without a ``reason``) and the ones PIL decodes."""
    gpu_idx = [i for i, h in enumerate(headers) if h is not None and h.reason is None]
    on_gpu = set(gpu_idx)
    return gpu_idx, [i for i in range(len(headers)) if i not in on_gpu]


def _decode_jpegs(plans, idx, headers, data, data_offs, src, src_offs, dev, timing):
    """Queues csrc/jpeg.hip for the plans ``idx``; returns the device status words."""
    from . import jpeg

    desc, huff, qt, totals = jpeg.build_tables([headers[i] for i in idx], [data_offs[i] for i in idx], [src_offs[i] for i in idx])
    data_d = data.to(dev, non_blocking=True)
    desc_d = torch.from_numpy(desc).to(dev)
    huff_d = torch.from_numpy(huff).to(dev)
    qt_d = torch.from_numpy(qt).to(dev)
    status = torch.empty(len(idx), dtype=torch.int32, device=dev)
    if timing is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
    _launch_jpeg_decode(data_d, desc_d, desc, huff_d, qt_d, totals, src, status)
    if timing is not None:
        ev[1].record()
        timing["_decode_events"] = ev
    return status


def prepare_images(plans, draws, flips, luts, device="cuda", decode_threads=4, timing=None, checks=None):
    """The image half of a batch on the GPU (csrc/imageprep.hip): ``plans`` = :class:`imageprep.ImagePlan` per scene (window +
    target size), ``draws`` = ``ColorJitter.draw()`` per scene (or None), ``flips`` = fliplr per scene, ``luts`` = fp32
    [3][256] per scene (:func:`imageprep.lut`).  Baseline JPEG files (:mod:`jpeg`) are read into one pinned buffer, copied to
    the device in one H2D copy and decoded there (csrc/jpeg.hip); every other image is decoded with ``decode_threads``
    threads into a second pinned buffer and copied.  Both kinds land in one device source buffer, then the three kernels run.
    Returns img fp32 [B,3,H,W] on ``device``, already flipped.  ``timing``: a dict that receives the GPU ms of the three
    kernels (``"kernels_ms"``) and of the JPEG decode (``"decode_ms"``, events; synchronises) and the number of images decoded
    each way (``"gpu_decoded"``, ``"host_decoded"``).  A JPEG whose entropy-coded data the GPU decoder cannot decode raises
    ``RuntimeError`` naming the file: here, which waits for the stream, or - when ``checks`` is a list - in a callable
    appended to it, for a caller that reads back from the stream anyway (``gpu_batch`` calls it after its own read-back)."""
    from . import imageprep

    dev = torch.device(device)
    B = len(plans)
    W, H = plans[0].size
    sizes = source_sizes(plans)
    nbytes = sum(sizes)
    src_offs = source_offsets(plans)
    headers, status = [None] * B, None
    if GPU_JPEG:
        data, data_offs, headers = read_jpegs(plans)
    gpu_idx, host_idx = split_decoders(headers)
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    if gpu_idx:
        status = _decode_jpegs(plans, gpu_idx, headers, data, data_offs, src, src_offs, dev, timing)
    if host_idx:
        hplans = [plans[i] for i in host_idx]
        staging = torch.empty(sum(sizes[i] for i in host_idx), dtype=torch.uint8, pin_memory=True)
        hoffs = imageprep.decode_into(hplans, staging.numpy(), decode_threads)
        if not gpu_idx:
            src[: staging.numel()].copy_(staging, non_blocking=True)  # same layout: one copy
        else:
            for j, i in enumerate(host_idx):
                src[src_offs[i] : src_offs[i] + sizes[i]].copy_(staging[hoffs[j] : hoffs[j] + sizes[i]], non_blocking=True)
    desc, coef, factors, lut, tmp_bytes = imageprep.build_tables(plans, draws, flips, luts, src_offs)
    desc_d = torch.from_numpy(desc).to(dev)
    coef_d = torch.from_numpy(coef).to(dev)
    fac_d = torch.from_numpy(factors).to(dev)
    lut_d = torch.from_numpy(lut).to(dev)
    tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
    mid = torch.empty(B * H * W * 3, dtype=torch.uint8, device=dev)
    sums = torch.empty(B, dtype=torch.int64, device=dev)
    img = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    if timing is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
    _launch_image_prepare(src, nbytes, desc_d, desc, coef_d, fac_d, lut_d, tmp, mid, sums, img)
    if timing is not None:
        ev[1].record()
        ev[1].synchronize()
        timing["kernels_ms"] = ev[0].elapsed_time(ev[1])
        dec = timing.pop("_decode_events", None)
        timing["decode_ms"] = dec[0].elapsed_time(dec[1]) if dec else 0.0
        timing["gpu_decoded"], timing["host_decoded"] = len(gpu_idx), len(host_idx)
    if status is not None:  # the one read-back of the decoder, queued after every image kernel
        st_h = torch.empty(status.numel(), dtype=torch.int32, pin_memory=True)
        st_h.copy_(status, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        paths = [jpeg_path(plans[i]) for i in gpu_idx]

        def check_status():
            done.synchronize()
            check_jpeg_status(paths, st_h.tolist())

        if checks is None:
            check_status()
        else:
            checks.append(check_status)
    return img


def jpeg_path(plan):
    return getattr(plan.image, "filename", "<image>")


def _prepare(scenes, scale, full_scale, aug, fliplr, want_seg2d, dev, use_rgb, img):
    """The kernel chain of :func:`prepare_batch`.  Returns (the device tensors of the batch under the names
    :func:`finish_batch` reads, rots, flips)."""
    B = len(scenes)
    lengths = [int(s["points"].shape[0]) for s in scenes]
    flips, rots, us = [], [], []
    for sc in scenes:
        if "draws" in sc:
            f, r, u = sc["draws"]
        else:
            f = bool(np.random.rand() < fliplr)
            r, u = augmentation_draws(**aug)
        flips.append(bool(f))
        rots.append(r)
        us.append(u)
    pts, pimg, dvals, labels = (torch.from_numpy(a).to(dev) for a in scene_arrays(scenes))
    if img is None:
        img = torch.stack([torch.as_tensor(s["img"]) for s in scenes]).to(dev, torch.float32)
        if any(flips):
            img = torch.stack([im.flip(-1) if f else im for im, f in zip(img, flips)])
    elif img.device.type != dev.type or img.dtype != torch.float32 or img.dim() != 4 or img.shape[0] != B:
        raise ValueError("prepare_batch: img must be a float32 [B,3,H,W] tensor on the batch's device")
    H, W = img.shape[-2:]
    vox = voxelize_batch(pts, lengths, rots, us, scale, full_scale)
    idx_all, depth, seg2d, err = project_batch(pimg, dvals, labels, lengths, H, W, flips, want_seg2d, vox["scene_off"])
    kept = vox["locs"].shape[0]
    idx = torch.empty((kept, 2), dtype=torch.int64, device=dev)
    lab = torch.empty(kept, dtype=torch.int64, device=dev)
    feats = torch.empty((kept, img.shape[1]), dtype=torch.float32, device=dev) if use_rgb else None
    pkept = torch.empty((kept, 3), dtype=pts.dtype, device=dev)
    collect_points(vox["keep"], vox["counts_dev"][B:], kept, vox["locs"], idx_all, labels, img.contiguous(), H, W, pts, idx, lab, feats,
                   pkept)
    check_projection(err.item())
    if not use_rgb:
        feats = torch.ones((int(sum(lengths)), 1), dtype=torch.float32, device=dev)
    t = dict(locs=vox["locs"], feats=feats, seg_label=lab, img=img, depth=depth, seg2d=seg2d, img_indices=idx, counts=vox["counts"],
             points=pkept, min_values=vox["min_value"], offsets=vox["offset"], keep=vox["keep"])
    return t, rots, flips


def prepare_batch(scenes, scale=20, full_scale=4096, augmentation=None, fliplr=0.0, want_seg2d=False, device="cuda", use_rgb=True,
                  img=None):
    """The reference's ``__getitem__`` (per scene) + ``collate_scn_base`` for a list of decoded scenes, on the GPU.

    Each scene: dict(points [n,3] f32 (or f64 in every scene of the batch) = the coordinates that are voxelised (camera or
    LiDAR frame, as the dataset is configured), points_img [n,2] (row, col) scaled to the network image, depth [n] = camera z, seg_label [n] int64,
    img [3,H,W] f32 already normalised and, when this scene's fliplr draw says so, NOT yet flipped).  RNG draws per
    scene in the reference's order: fliplr ``rand()`` first (nuscenes_dataloader.py:291), then ``augment_and_scale_3d``'s;
    a scene that carries ``draws = (flip, rot, u)`` was drawn by the caller (datasets.gpu_batch draws scene by scene, between
    each scene's crop draws, as the reference's ``__getitem__`` sequence does).  ``use_rgb=False``: the constant feature of
    nuscenes_dataloader.py:365-368, ones [n, 1] with n = the scene's point count BEFORE the range mask (as in the reference).
    ``img``: a device fp32 [B,3,H,W] batch image that is ALREADY flipped per the scenes' draws (:func:`prepare_images`); the
    scenes then carry no "img".  Returns the batch dict of lib/dataset/__init__.py:95-121 with every tensor on ``device`` (img_indices: list of
    device int64 [n_i,2]; use ``[t.cpu().numpy() for t in ...]`` where numpy arrays are required)."""
    t, rots, flips = _prepare(scenes, scale, full_scale, dict(augmentation or {}), fliplr, want_seg2d, torch.device(device), use_rgb, img)
    return _batch_dict(t, _per_scene(t["points"], t["counts"]), np.stack(rots), flips)


def _per_scene(rows, counts):
    bounds = np.concatenate([[0], np.cumsum(counts)])
    return [rows[bounds[i] : bounds[i + 1]] for i in range(len(counts))]


def _batch_dict(t, points, rotation_matrices, flips):
    out = {
        "x": [t["locs"], t["feats"]],
        "seg_label": t["seg_label"],
        "img": t["img"],
        "depth": t["depth"],
        "img_indices": _per_scene(t["img_indices"], t["counts"]),
        "points": points,
        "min_values": t["min_values"], "offsets": t["offsets"], "rotation_matrices": rotation_matrices, "fliplr": flips,
        "keep": t["keep"],  # original row (in the concatenated input) of every kept point
    }
    if t["seg2d"] is not None:
        out["seg_labels_2d"] = t["seg2d"]
    return out


def finish_batch(t, rots, flips, intrinsics, works=None, kept_rows=None, pselab=None):
    """The batch dict of the dataset loaders: ``gpu_batch`` and ``PendingBatch.result`` end here.  ``t``: the device tensors of
    :func:`_prepare` (seg2d already fp32) and ``counts``, the kept rows per scene; rots / flips / intrinsics: per scene, host.
    ``works`` + ``kept_rows`` (``keep`` on the host): adds the labels before the range mask and the mask itself, per scene.
    ``pselab``: the kept pseudo-label rows by key; a key of :data:`PSELAB_KEYS` that is missing becomes ``[]``."""
    batch = _batch_dict(t, t["points"], torch.from_numpy(np.stack(rots)), list(flips))
    batch["intrinsics"] = torch.from_numpy(np.stack(intrinsics))
    batch["coords"] = t["locs"][:, :3]
    if works is not None:
        off = scene_offsets([len(w.points) for w in works])
        masks = [np.zeros(len(w.points), dtype=bool) for w in works]
        for b, m in enumerate(masks):
            m[kept_rows[(kept_rows >= off[b]) & (kept_rows < off[b + 1])] - off[b]] = True
        batch["orig_seg_label"] = [w.label for w in works]
        batch["orig_points_idx"] = masks
    if pselab is not None:
        for key in PSELAB_KEYS:
            batch[key] = pselab.get(key, [])
    return batch


def check_projection(err):  # err: the error word of mm_project_batch, read back
    if int(err) != 0:
        raise AssertionError("projected point outside the image (nuscenes_dataloader.py:279-283)")


def check_jpeg_status(paths, status):  # status: the words of mm_jpeg_decode, read back; paths: the files they belong to
    bad = [(p, s) for p, s in zip(paths, status) if s]
    if bad:
        raise RuntimeError("JPEG decode failed (entropy-coded data; include/mm2d3d.h MM_JPG_ST_* bits): " +
                           ", ".join(f"{p} (status {s})" for p, s in bad))
