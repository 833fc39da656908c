"""``gpu_batch`` in three phases, and a stream of such batches that stays ahead of ``fit_step`` (csrc/dataprep.hip ``_dev``).

``ds.gpu_batch(indices)`` is written for an idle GPU: it uploads from pageable memory and reads the kept counts back before it
sizes its outputs, and each of those waits for everything queued on the stream - inside a training loop, for the whole previous
step.  The same batch is produced here without a host wait:

    host phase     no stream call, any thread    the scene loop of ``gpu_batch`` (``_front``, jitter, flip and 3D draws in the
                                                 same RNG order), file reads, JPEG headers, PIL decodes, the kernels' tables;
                                                 every host array packed into two pinned staging blocks (small arrays, image bytes)
    queue phase    caller's thread and stream    two ``non_blocking`` uploads (the device arrays are views into them), the kernel
                                                 chain of ``gpu_batch`` with the collect step in its device-count form, outputs
                                                 allocated at the batch's point count, ONE read-back into pinned memory + an event
    result phase   caller's thread               waits for that event, raises the loader's errors, narrows the outputs to the kept
                                                 count (row-prefix views), builds the batch dict of ``gpu_batch``

``ds.begin_gpu_batch(indices)`` returns the :class:`PendingBatch`; :class:`BatchStream` runs the host phases on one worker thread
and keeps ``depth`` batches queued ahead of the one it yields.  Everything is queued on the current stream: the single-launch
batch norms of the training step need the CUs they expect, so no side stream is used and the worker launches nothing.
"""
from __future__ import annotations

import collections
import os
import queue as _queue
import threading
import time

import numpy as np
import torch

ALIGN = 16  # bytes: every sub-array of a staging block starts at a multiple (int64 / float64 views need 8)


def _round_up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------- pinned staging ring
class PinnedRing:
    """Pinned host buffers that are reused only after the event recorded behind their last copy has completed (the pattern of
    ``scn.metadata._Readback``).  ``acquire`` touches no stream and no event, so the worker thread may call it; ``release`` and
    ``reclaim`` belong to the thread that queues the copies.  Without a GPU the buffers are ordinary memory."""

    KEEP = 8  # free buffers kept; beyond that the smallest are dropped

    def __init__(self):
        self._lock = threading.Lock()
        self._free, self._busy = [], []
        self.made = 0

    def acquire(self, nbytes):
        nbytes = max(int(nbytes), ALIGN)
        with self._lock:
            fit = [b for b in self._free if b.numel() >= nbytes]
            if fit:
                buf = min(fit, key=lambda b: b.numel())
                self._free = [b for b in self._free if b is not buf]
                return buf
            self.made += 1
        return torch.empty(_round_up(nbytes * 5 // 4 + 4096, 4096), dtype=torch.uint8, pin_memory=torch.cuda.is_available())

    def release(self, buf, event=None):
        """``event``: recorded behind the copy that reads or writes ``buf``; None = nothing is in flight."""
        with self._lock:
            if event is None:
                self._put(buf)
            else:
                self._busy.append((buf, event))

    def reclaim(self):
        with self._lock:
            busy = []
            for buf, ev in self._busy:
                if ev.query():
                    self._put(buf)
                else:
                    busy.append((buf, ev))
            self._busy = busy

    def _put(self, buf):
        self._free.append(buf)
        if len(self._free) > self.KEEP:
            drop = min(self._free, key=lambda b: b.numel())
            self._free = [b for b in self._free if b is not drop]


STAGING = PinnedRing()   # host -> device blocks
READBACK = PinnedRing()  # device -> host blocks


# ---------------------------------------------------------------------------------------------------- staging blocks
class Block:
    """Named host arrays back to back in one buffer, each at a multiple of ``ALIGN`` bytes.  ``add`` reserves, ``seal`` takes
    the buffer from the ring and copies the reserved arrays in; ``reserve`` + ``host`` give a region to fill in place (file
    reads, decodes)."""

    def __init__(self, ring=None):
        self.ring = STAGING if ring is None else ring
        self.layout = {}  # name -> (byte offset, numpy dtype, shape)
        self._pending = {}
        self.nbytes = 0
        self.buf = None

    def reserve(self, name, dtype, shape):
        dtype, shape = np.dtype(dtype), tuple(int(s) for s in np.atleast_1d(shape))
        off = _round_up(self.nbytes)
        self.layout[name] = (off, dtype, shape)
        self.nbytes = off + dtype.itemsize * int(np.prod(shape, dtype=np.int64))
        return off

    def add(self, name, array):
        array = np.ascontiguousarray(array)
        self.reserve(name, array.dtype, array.shape)
        self._pending[name] = array

    def seal(self):
        self.buf = self.ring.acquire(self.nbytes)
        for name, array in self._pending.items():
            self.host(name)[...] = array
        self._pending = {}
        return self

    def host(self, name):
        off, dtype, shape = self.layout[name]
        n = dtype.itemsize * int(np.prod(shape, dtype=np.int64))
        return self.buf.numpy()[off : off + n].view(dtype).reshape(shape)

    def upload(self, dev):
        """Queues the copy of the used part; returns the device block (uint8)."""
        return self.buf[: max(self.nbytes, 1)].to(dev, non_blocking=True)

    def device(self, block_d, name):
        """The view of ``name`` in the uploaded block: no copy."""
        off, dtype, shape = self.layout[name]
        n = dtype.itemsize * int(np.prod(shape, dtype=np.int64))
        return block_d[off : off + n].view(_TORCH_DTYPE[dtype]).view(shape)

    def release(self, event=None):
        if self.buf is not None:
            self.ring.release(self.buf, event)
            self.buf = None


_TORCH_DTYPE = {np.dtype(k): v for k, v in {
    np.uint8: torch.uint8, np.int8: torch.int8, np.int16: torch.int16, np.int32: torch.int32, np.int64: torch.int64,
    np.float32: torch.float32, np.float64: torch.float64, np.bool_: torch.bool}.items()}

_PSELAB_KEYS = ("pseudo_label_2d", "pseudo_label_ensemble", "pseudo_label_3d")


# ---------------------------------------------------------------------------------------------------- one batch
class PendingBatch:
    """The batch ``ds.gpu_batch(indices, ...)`` would return, on its way.  The constructor runs the host phase (on the calling
    thread: the numpy and torch CPU RNGs advance exactly as in ``gpu_batch``); ``queue()`` enqueues the uploads, the kernels and
    the read-back on the current stream without waiting for it; ``result()`` waits for the read-back and returns the dict.
    ``host_ms`` / ``wait_ms``: wall time of the host phase and of the wait inside ``result()``; ``timing = True`` before
    ``queue()`` brackets the queued work with events (``gpu_ms`` after ``result()``)."""

    def __init__(self, ds, indices, device="cuda", want_seg2d=False, image="host", decode_threads=4):
        if image not in ("host", "gpu"):
            raise ValueError(f"begin_gpu_batch: image must be 'host' or 'gpu', not {image!r}")
        self.ds, self.indices = ds, [int(i) for i in indices]
        self.device, self.want_seg2d, self.on_gpu, self.decode_threads = device, bool(want_seg2d), image == "gpu", decode_threads
        self.timing, self.gpu_ms, self.wait_ms = False, None, None
        self._state = "host"
        self.small, self.images = Block(), Block()
        t0 = time.perf_counter()
        try:
            self._host()
        except BaseException:
            self.cancel()
            raise
        self.host_ms = (time.perf_counter() - t0) * 1e3

    # ------------------------------------------------------------------ host phase
    def _host(self):
        from . import dataprep, imageprep

        ds, on_gpu = self.ds, self.on_gpu
        scenes, works, jitter = [], [], []
        self.intrinsics, self.flips, self.rots = [], [], []
        us = []
        ds._plan_images = on_gpu
        try:
            for i in self.indices:  # the scene loop of _Scenes.gpu_batch, draw for draw
                w = ds._front(i)
                if on_gpu:
                    jitter.append(ds.color_jitter.draw() if ds.color_jitter is not None else None)
                    W, H = w.image.size
                else:
                    arr = ds._float_image(w.image)
                    H, W = arr.shape[:2]
                flip = bool(np.random.rand() < ds.fliplr)
                rot, u = dataprep.augmentation_draws(**ds._augmentation())
                intr = w.intr
                if flip:
                    intr = intr.copy()
                    intr[0, 2] = W - intr[0, 2]
                    intr[1, 2] = H - intr[0, 1]
                if w.label is None:
                    raise ValueError("gpu_batch needs labelled scenes (the 2D label map and seg_label are part of the batch)")
                sc = dict(points=np.ascontiguousarray(w.points), points_img=np.trunc(w.pimg), depth=w.cam[:, 2], seg_label=w.label)
                if not on_gpu:
                    sc["img"] = np.ascontiguousarray(np.moveaxis(ds._normalise(arr), -1, 0))
                scenes.append(sc)
                works.append(w)
                self.intrinsics.append(intr)
                self.flips.append(flip)
                self.rots.append(rot)
                us.append(u)
        finally:
            ds._plan_images = False
        self.works = works
        B = self.B = len(scenes)
        if B == 0:
            raise ValueError("begin_gpu_batch: no scenes")
        self.HW = (H, W)
        lengths = [int(s["points"].shape[0]) for s in scenes]
        self.off = np.zeros(B + 1, np.int32)
        np.cumsum(lengths, out=self.off[1:])
        self.n = int(self.off[B])
        self.transl = any(u is not None for u in us)
        if self.transl and not all(u is not None for u in us):
            raise ValueError("voxelize_batch: translation must be drawn for every scene of the batch or for none")
        f64 = [np.asarray(s["points"]).dtype == np.float64 for s in scenes]
        if any(f64) and not all(f64):
            raise ValueError("prepare_batch: the scenes of one batch must all have float64 points or none (the reference voxelises "
                             "float64 and float32 points with different arithmetic)")
        self.f64 = any(f64)
        cat = lambda key, dt: np.concatenate([np.asarray(s[key]) for s in scenes], 0).astype(dt)
        sm = self.small
        sm.add("off", self.off)
        sm.add("rot", np.stack([np.asarray(r, np.float32).reshape(9) for r in self.rots]))
        sm.add("u", np.stack([np.asarray(u if u is not None else np.zeros(3), np.float64) for u in us]))
        sm.add("flip", np.array([1 if f else 0 for f in self.flips], np.uint8))
        sm.add("points", cat("points", np.float64 if self.f64 else np.float32).reshape(self.n, 3))
        sm.add("pimg", cat("points_img", np.float32).reshape(self.n, 2))
        sm.add("depth", cat("depth", np.float32))
        sm.add("labels", cat("seg_label", np.int64))
        self.pselab = []
        if ds.has_pselab and ds.pselab_data is not None:
            for key in _PSELAB_KEYS:
                if ds.pselab_data[self.indices[0]][key] is None:
                    continue
                rows = np.concatenate([np.asarray(ds.pselab_data[i][key])[w.keep] for i, w in zip(self.indices, works)])
                if rows.shape != (self.n,):
                    raise AssertionError("pseudo labels and points of a batch have different lengths")
                self.pselab.append(key)
                sm.add(key, rows)
            if len({sm.layout[k][1] for k in self.pselab}) > 1:
                raise TypeError("begin_gpu_batch: the pseudo-label arrays of a dataset must share one dtype")
        if on_gpu:
            self._host_images([w.image for w in works], jitter, imageprep.lut(ds._to_float, ds._normalise))
        else:
            self.images.add("img", np.stack([s["img"] for s in scenes]).astype(np.float32))
            self.images.seal()
        sm.seal()
        self._state = "hosted"

    def _host_images(self, plans, jitter, lut):
        """The host half of ``dataprep.prepare_images``: files, headers, decodes and tables; nothing is launched."""
        from . import dataprep, imageprep, jpeg

        B, sm, im = self.B, self.small, self.images
        sizes = [p.image.size[0] * p.image.size[1] * 3 for p in plans]
        self.src_bytes = int(sum(sizes))
        src_offs = dataprep.source_offsets(plans)
        self.gpu_idx, headers, files, data_offs = [], [None] * B, None, None
        if dataprep.GPU_JPEG:
            paths = [jpeg.jpeg_file(p.image) for p in plans]
            fsz = [os.path.getsize(f) if f is not None else 0 for f in paths]
            data_offs = np.concatenate([[0], np.cumsum(fsz)]).astype(np.int64)
            files = np.empty(max(int(data_offs[-1]), 1), np.uint8)
            for i, f in enumerate(paths):
                if f is None:
                    continue
                buf = files[data_offs[i] : data_offs[i + 1]]
                jpeg.read_into(f, buf)
                try:
                    headers[i] = jpeg.parse(buf, f)
                except ValueError as e:  # PIL decides on the host, as in read_jpegs
                    headers[i] = jpeg.JpegHeader()
                    headers[i].reason = f"header: {e}"
            self.gpu_idx = [i for i, h in enumerate(headers) if h is not None and h.reason is None]
        on_gpu = set(self.gpu_idx)
        self.host_idx = [i for i in range(B) if i not in on_gpu]
        self.jpeg_paths = [dataprep.jpeg_path(plans[i]) for i in self.gpu_idx]
        if self.gpu_idx:
            self.data_bytes = int(files.size)
            im.reserve("jpeg", np.uint8, (self.data_bytes,))  # first: at the block's own (allocator) alignment
            desc, huff, qt, self.jpeg_totals = jpeg.build_tables([headers[i] for i in self.gpu_idx], [data_offs[i] for i in self.gpu_idx],
                                                                 [src_offs[i] for i in self.gpu_idx])
            self.jpeg_desc = desc
            sm.add("jpeg_desc", desc)
            sm.add("jpeg_huff", huff)
            sm.add("jpeg_qt", qt)
        hplans = [plans[i] for i in self.host_idx]
        if hplans:
            im.reserve("decoded", np.uint8, (sum(sizes[i] for i in self.host_idx),))
        im.seal()
        if self.gpu_idx:
            im.host("jpeg")[...] = files
        self.host_offs = imageprep.decode_into(hplans, im.host("decoded"), self.decode_threads) if hplans else []
        self.sizes, self.src_offs = sizes, src_offs
        desc, coef, factors, luts, self.tmp_bytes = imageprep.build_tables(plans, jitter, self.flips, [lut] * B, src_offs)
        self.img_desc, self.coef_size = desc, int(coef.size)
        sm.add("img_desc", desc)
        sm.add("img_coef", coef)
        sm.add("img_fac", factors)
        sm.add("img_lut", luts)

    def cancel(self):
        """Gives the staging blocks back without queuing anything (a batch that is dropped after its host phase)."""
        if self._state in ("host", "hosted"):
            self.small.release()
            self.images.release()
            self._state = "cancelled"

    # ------------------------------------------------------------------ queue phase
    def queue(self):
        """Enqueues the batch on the current stream; waits for nothing.  Idempotent."""
        if self._state != "hosted":
            if self._state in ("queued", "done"):
                return self
            raise RuntimeError(f"PendingBatch.queue: the batch is {self._state}")
        from . import _lib
        from ._lib import check, ptr, stream

        L = _lib.lib()
        dev = torch.device(self.device)
        B, n, (H, W), sm, im = self.B, self.n, self.HW, self.small, self.images
        STAGING.reclaim()
        READBACK.reclaim()
        if self.timing:
            self._ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            self._ev[0].record()
        sm_d, im_d = sm.upload(dev), im.upload(dev)
        copied = torch.cuda.Event()
        copied.record()
        sm.release(copied)
        im.release(copied)
        self._state = "queued"
        d = lambda name: sm.device(sm_d, name)
        # the read-back block: kept counts [B+1] | projection error word | JPEG status words | keep rows (output_orig)
        nj = len(self.gpu_idx) if self.on_gpu else 0
        keep_host = bool(self.ds.output_orig)
        nk = max(n, 1)
        rb = torch.empty(B + 2 + nj + (nk if keep_host else 0), dtype=torch.int32, device=dev)
        counts, err, status = rb[: B + 1], rb[B + 1 : B + 2], rb[B + 2 : B + 2 + nj]
        keep = rb[B + 2 + nj :] if keep_host else torch.empty(nk, dtype=torch.int32, device=dev)
        counts.zero_()
        # ---- images
        if self.on_gpu:
            if self.gpu_idx:
                src = torch.empty(max(self.src_bytes, 1), dtype=torch.uint8, device=dev)
                n_iv, n_sub, n_blk, n_plane = self.jpeg_totals
                ws = _lib.workspace.get(int(L.mm_jpeg_ws_bytes(nj, self.data_bytes, n_iv, n_sub, n_blk, n_plane)), dev, "jpeg")
                huff, qt = d("jpeg_huff"), d("jpeg_qt")
                check(L.mm_jpeg_decode(ptr(im.device(im_d, "jpeg")), self.data_bytes, ptr(d("jpeg_desc")), self.jpeg_desc.ctypes.data, nj,
                                       ptr(huff), huff.shape[0], ptr(qt), qt.shape[0], ptr(src), src.numel(), ptr(status), ptr(ws),
                                       ws.numel(), stream()), "jpeg_decode")
                if self.host_idx:
                    dec = im.device(im_d, "decoded")
                    for j, i in enumerate(self.host_idx):
                        m = self.sizes[i]
                        src[self.src_offs[i] : self.src_offs[i] + m].copy_(dec[self.host_offs[j] : self.host_offs[j] + m], non_blocking=True)
            else:
                src = im.device(im_d, "decoded")  # every image decoded on the host: the upload already has the source layout
            tmp = torch.empty(max(self.tmp_bytes, 1), dtype=torch.uint8, device=dev)
            mid = torch.empty(B * H * W * 3, dtype=torch.uint8, device=dev)
            sums = torch.empty(B, dtype=torch.int64, device=dev)
            img = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
            check(L.mm_image_prepare(ptr(src), self.src_bytes, ptr(d("img_desc")), self.img_desc.ctypes.data, B, H, W, ptr(d("img_coef")),
                                     self.coef_size, ptr(d("img_fac")), ptr(d("img_lut")), ptr(tmp), tmp.numel(), ptr(mid), ptr(sums),
                                     ptr(img), stream()), "image_prepare")
        else:
            img = im.device(im_d, "img")
            if any(self.flips):
                img = torch.stack([t.flip(-1) if f else t for t, f in zip(img, self.flips)])
        C = img.shape[1]
        # ---- voxelisation and projection: the kernels of prepare_batch, unchanged
        pts, off_d, labels = d("points"), d("off"), d("labels")
        pdt = pts.dtype
        locs = torch.empty((nk, 4), dtype=torch.int64, device=dev)
        minv = torch.empty((B, 3), dtype=pdt, device=dev)
        offset = torch.empty((B, 3), dtype=torch.float64, device=dev)
        ws_bytes, run = (L.mm_voxelize_ws_bytes_f64, L.mm_voxelize_batch_f64) if self.f64 else (L.mm_voxelize_ws_bytes, L.mm_voxelize_batch)
        ws = _lib.workspace.get(int(ws_bytes(n, B)), dev)
        check(run(ptr(pts), ptr(off_d), self.off.ctypes.data, B, ptr(d("rot")), ptr(d("u")), 1 if self.transl else 0, float(self.ds.scale),
                  int(self.ds.full_scale), ptr(locs), ptr(keep), ptr(counts), ptr(minv), ptr(offset), ptr(ws), ws.numel(), stream()),
              "voxelize_batch")
        idx_all = torch.empty((nk, 2), dtype=torch.int64, device=dev)
        depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        seg2d = torch.empty((B, H, W), dtype=torch.float64, device=dev) if self.want_seg2d else None
        winner = torch.empty(B * H * W, dtype=torch.int32, device=dev)
        check(L.mm_project_batch(ptr(d("pimg")), ptr(d("depth")), ptr(labels), ptr(off_d), self.off.ctypes.data, B, H, W, ptr(d("flip")),
                                 ptr(idx_all), ptr(depth), ptr(seg2d), ptr(winner), ptr(err), stream()), "project_batch")
        # ---- collect: launched over the point count, the kept total is read on the device
        idx = torch.empty((nk, 2), dtype=torch.int64, device=dev)
        lab = torch.empty(nk, dtype=torch.int64, device=dev)
        feats = torch.empty((nk, C), dtype=torch.float32, device=dev) if self.ds.use_rgb else None
        pkept = torch.empty((nk, 3), dtype=pdt, device=dev)
        pl_in = [d(k) for k in self.pselab]
        pl_out = [torch.empty(nk, dtype=t.dtype, device=dev) for t in pl_in]
        out = collect_points_dev(keep, counts, B, n, locs, idx_all, labels, img.contiguous() if feats is not None else None, H, W, pts, idx,
                                 lab, feats, pkept, pl_in, pl_out)
        del out
        if not self.ds.use_rgb:
            feats = torch.ones((n, 1), dtype=torch.float32, device=dev)
        if seg2d is not None:
            seg2d = seg2d.float()
        # ---- the one read-back
        nbytes = rb.numel() * 4
        self._rb_buf = READBACK.acquire(nbytes)
        self._rb_host = self._rb_buf[:nbytes].view(torch.int32)
        self._rb_host.copy_(rb, non_blocking=True)
        if self.timing:
            self._ev[1].record()
        self.event = torch.cuda.Event()
        self.event.record()
        self._dev = dict(locs=locs, keep=keep, idx=idx, lab=lab, feats=feats, pkept=pkept, img=img, depth=depth, seg2d=seg2d, minv=minv,
                         offset=offset, pselab=pl_out, rb=rb, blocks=(sm_d, im_d))
        self._rb_layout = (nj, keep_host)
        return self

    # ------------------------------------------------------------------ result phase
    def result(self):
        """Waits for the batch's event (the only wait), raises what ``gpu_batch`` raises, returns the batch dict."""
        if self._state == "done":
            return self._result
        if self._state == "hosted":
            self.queue()
        if self._state != "queued":
            raise RuntimeError(f"PendingBatch.result: the batch is {self._state}")
        t0 = time.perf_counter()
        self.event.synchronize()
        self.wait_ms = (time.perf_counter() - t0) * 1e3
        r = self._rb_host.numpy().copy()
        READBACK.release(self._rb_buf)
        self._rb_buf = self._rb_host = None
        if self.timing:
            self.gpu_ms = self._ev[0].elapsed_time(self._ev[1])
        B, d = self.B, self._dev
        nj, keep_host = self._rb_layout
        counts, kept = r[:B].tolist(), int(r[B])
        self._state = "failed"
        if int(r[B + 1]) != 0:
            raise AssertionError("projected point outside the image (nuscenes_dataloader.py:279-283)")
        bad = [(p, s) for p, s in zip(self.jpeg_paths if nj else [], r[B + 2 : B + 2 + nj].tolist()) if s]
        if bad:
            raise RuntimeError("JPEG decode failed (entropy-coded data; include/mm2d3d.h MM_JPG_ST_* bits): " +
                               ", ".join(f"{p} (status {s})" for p, s in bad))
        bounds = np.concatenate([[0], np.cumsum(counts)])
        locs, idx, pkept = d["locs"][:kept], d["idx"][:kept], d["pkept"][:kept]
        batch = {
            "x": [locs, d["feats"][:kept] if self.ds.use_rgb else d["feats"]],
            "seg_label": d["lab"][:kept],
            "img": d["img"],
            "depth": d["depth"],
            "img_indices": [idx[bounds[i] : bounds[i + 1]] for i in range(B)],
            "points": pkept,
            "min_values": d["minv"], "offsets": d["offset"], "rotation_matrices": torch.from_numpy(np.stack(self.rots)),
            "fliplr": list(self.flips),
            "keep": d["keep"][:kept],
        }
        if d["seg2d"] is not None:
            batch["seg_labels_2d"] = d["seg2d"]
        batch["intrinsics"] = torch.from_numpy(np.stack(self.intrinsics))
        batch["coords"] = locs[:, :3]
        if keep_host:
            rows = r[B + 2 + nj : B + 2 + nj + kept]
            masks = []
            for b, w in enumerate(self.works):
                m = np.zeros(len(w.points), dtype=bool)
                m[rows[(rows >= self.off[b]) & (rows < self.off[b + 1])] - self.off[b]] = True
                masks.append(m)
            batch["orig_seg_label"] = [w.label for w in self.works]
            batch["orig_points_idx"] = masks
        if self.ds.has_pselab and self.ds.pselab_data is not None:
            got = dict(zip(self.pselab, d["pselab"]))
            for key in _PSELAB_KEYS:
                batch[key] = got[key][:kept] if key in got else []
        self._dev = self.works = None
        self._result, self._state = batch, "done"
        return batch


def collect_points_dev(keep, counts, B, n_total, locs, idx_all, labels, image, H, W, points, idx_out, lab_out, feats_out, points_out,
                       extra_in=(), extra_out=()):
    """``mm_collect_points_dev`` / ``_f64_dev`` (csrc/dataprep.hip): the collect step of ``prepare_batch`` launched over
    ``n_total`` rows with the kept total read from ``counts[B]`` on the device; ``extra_in`` -> ``extra_out``: up to three
    per-point arrays of one dtype gathered by ``keep`` in the same launch.  Any of labels / feats / points outputs may be None."""
    import ctypes

    from . import _lib

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
    _lib.check(fn(_lib.ptr(keep), _lib.ptr(counts), int(B), int(n_total), _lib.ptr(locs), _lib.ptr(idx_all), _lib.ptr(labels), _lib.ptr(image),
                  C, int(H), int(W), _lib.ptr(points), _lib.ptr(idx_out), _lib.ptr(lab_out), _lib.ptr(feats_out), _lib.ptr(points_out),
                  ctypes.cast(ein, ctypes.c_void_p), ctypes.cast(eout, ctypes.c_void_p), ne, extra_in[0].element_size() if ne else 0,
                  _lib.stream()), "collect_points_dev")
    return idx_out


# ---------------------------------------------------------------------------------------------------- the stream
class BatchStream:
    """Batches from files, kept in flight ahead of the training step::

        steps = ({"source": (src, si), "target": (trg, ti)} for si, ti in ddp.paired_shards(...))
        with BatchStream(steps, depth=2, image="gpu") as stream:
            for batch, next_batch in stream:
                trainer.fit_step(batch, next_batch=next_batch)

    ``steps``: an iterable of dicts ``name -> (dataset, indices)``.  One worker thread runs the host phases
    (``dataset.begin_gpu_batch(indices, queue=False, **gpu_batch_kwargs)``) in step order and, within a step, in the dict's
    order; the iterating thread queues each step as soon as its host phase is done and keeps at most ``depth`` steps queued ahead
    of the one it yields.  It yields ``(batch, next_batch)`` with ``batch = {name: batch dict}``; ``next_batch`` is the very
    object the next iteration yields as ``batch`` (None at the end), so the trainer's metadata prefetch works unchanged.
    ``depth=2`` is the smallest depth at which ``next_batch`` is ready without waiting for the step before it.

    While a stream is open its worker owns the global numpy and torch CPU RNGs (the loaders draw from them, in the order of the
    same ``gpu_batch`` calls made one after the other): do not draw from them on other threads until it is closed or exhausted.
    The datasets are the worker's as well: no ``gpu_batch`` / ``__getitem__`` on them meanwhile.

    An exception in the worker, in ``queue()`` or in a ``result()`` is raised from the iteration and closes the stream (a step that
    failed in the worker or in ``queue()``: after the steps before it that still have a ``next_batch`` have been yielded).
    ``close()`` (or leaving the ``with`` block) joins the thread and drops what is in flight.  ``timing=True`` measures the
    queued GPU work of every batch with events; ``stats`` collects ``host_ms`` / ``wait_ms`` / ``gpu_ms`` per step."""

    def __init__(self, steps, depth=2, timing=False, **gpu_batch_kwargs):
        if int(depth) < 1:
            raise ValueError("BatchStream: depth must be at least 1")
        self.depth, self.timing, self.kwargs = int(depth), bool(timing), dict(gpu_batch_kwargs)
        self.stats = []
        self._steps = iter(steps)
        self._hosted = _queue.Queue(maxsize=self.depth)  # host phases done, not yet queued
        self._stop = threading.Event()
        self._closed = False
        self._iterating = False
        self._thread = threading.Thread(target=self._work, name="mm2d3d-batchstream", daemon=True)
        self._thread.start()

    # ---- worker thread: host phases only
    def _put(self, item):
        while not self._stop.is_set():
            try:
                self._hosted.put(item, timeout=0.05)
                return True
            except _queue.Full:
                continue
        return False

    def _work(self):
        try:
            for step in self._steps:
                if self._stop.is_set():
                    return
                pend = {}
                try:
                    for name, (ds, indices) in step.items():
                        pend[name] = ds.begin_gpu_batch(indices, queue=False, **self.kwargs)
                except BaseException:
                    _cancel(pend)
                    raise
                if not self._put(("step", pend)):
                    _cancel(pend)
                    return
            self._put(("end", None))
        except BaseException as e:  # handed to the iterating thread
            self._put(("error", e))

    # ---- iterating thread
    def _take(self):
        """The next hosted step, queued; None at the end."""
        if self._ended or self._closed:
            return None
        kind, item = self._hosted.get()
        if kind == "end":
            self._ended = True
            return None
        if kind == "error":
            self._ended = True
            raise item
        for p in item.values():
            if self.timing and hasattr(p, "timing"):
                p.timing = True
            p.queue()
        return item

    def _resolve(self, pend):
        out = {name: p.result() for name, p in pend.items()}
        self.stats.append({k: sum(getattr(p, k, None) or 0.0 for p in pend.values()) for k in ("host_ms", "wait_ms", "gpu_ms")})
        return out

    def __iter__(self):
        if self._iterating or self._closed:
            raise RuntimeError("BatchStream: a stream is iterated once")
        self._iterating, self._ended = True, False
        return self._run()

    def _run(self):
        ahead = collections.deque()  # queued steps after the current one: [pending dict, resolved dict or None]
        try:
            first = self._take()
            if first is None:
                return
            cur = self._resolve(first)
            error = None
            while True:
                while len(ahead) < self.depth and error is None:
                    try:
                        nxt = self._take()
                    except BaseException as e:  # raised once the steps before it have been yielded
                        error = e
                        break
                    if nxt is None:
                        break
                    ahead.append([nxt, None])
                if ahead and ahead[0][1] is None:
                    ahead[0][1] = self._resolve(ahead[0][0])
                if not ahead and error is not None:  # the current step has no next_batch to announce: the stream ends here
                    raise error
                yield cur, (ahead[0][1] if ahead else None)
                if self._closed or not ahead:
                    return
                cur = ahead.popleft()[1]
        finally:
            self.close()

    def close(self):
        if self._closed:
            return
        self._closed = True
        self._stop.set()
        while self._thread.is_alive():  # let a blocked put through, give the dropped batches' staging back
            try:
                kind, item = self._hosted.get(timeout=0.05)
            except _queue.Empty:
                continue
            if kind == "step":
                _cancel(item)
        self._thread.join()
        while True:
            try:
                kind, item = self._hosted.get_nowait()
            except _queue.Empty:
                break
            if kind == "step":
                _cancel(item)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _cancel(pend):
    for p in pend.values():
        cancel = getattr(p, "cancel", None)
        if cancel is not None:
            cancel()
