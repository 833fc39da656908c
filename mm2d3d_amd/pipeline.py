"""``gpu_batch`` in three phases, and a stream of such batches that stays ahead of ``fit_step`` (csrc/dataprep.hip ``_dev``).

``ds.gpu_batch(indices)`` is written for an idle GPU: it uploads from pageable memory and reads the kept counts back before it
sizes its outputs, and each of those waits for everything queued on the stream - inside a training loop, for the whole previous
step.  The same batch is produced here without a host wait, from the same parts (mm2d3d_amd/dataprep.py):

    host phase     no stream call, any thread    ``ds._draw_scenes`` (the scene loop, its RNG draws), ``scene_arrays``, the JPEG
                                                 read helpers, PIL decodes, the kernels' tables; every host array packed into
                                                 two pinned staging blocks (small arrays, image bytes)
    queue phase    caller's thread and stream    two ``non_blocking`` uploads (the device arrays are views into them), the
                                                 ``_launch_*`` chain with ``collect_points_dev``, outputs allocated at the
                                                 batch's point count, ONE read-back into pinned memory + an event
    result phase   caller's thread               waits for that event, ``check_projection`` / ``check_jpeg_status``, narrows the
                                                 outputs to the kept count (row-prefix views), ``finish_batch``

``ds.begin_gpu_batch(indices)`` returns the :class:`PendingBatch`; :class:`BatchStream` runs the host phases on one worker thread
and keeps ``depth`` batches queued ahead of the one it yields.  Everything is queued on the current stream: the single-launch
batch norms of the training step need the CUs they expect, so no side stream is used and the worker launches nothing.
"""
from __future__ import annotations

import collections
import queue as _queue
import threading
import time

import numpy as np
import torch

from . import dataprep, imageprep, jpeg
from .dataprep import collect_points_dev  # noqa: F401  (also importable from here)

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
        ds, sm = self.ds, self.small
        drawn = ds._draw_scenes(self.indices, self.on_gpu)
        scenes, self.works, self.intrinsics, self.flips, self.rots, self.HW = [getattr(drawn, k) for k in (
            "scenes", "works", "intrinsics", "flips", "rots", "HW")]
        B = self.B = len(scenes)
        if B == 0:
            raise ValueError("begin_gpu_batch: no scenes")
        self.off = dataprep.scene_offsets([int(s["points"].shape[0]) for s in scenes])
        self.n = int(self.off[B])
        rot, u, self.transl = dataprep.draw_tables(self.rots, drawn.us)
        arrays = tuple(dataprep.scene_arrays(scenes))
        self.f64 = arrays[0].dtype == np.float64
        flip = np.array([1 if f else 0 for f in self.flips], np.uint8)
        for name, array in zip(("off", "rot", "u", "flip", "points", "pimg", "depth", "labels"), (self.off, rot, u, flip) + arrays):
            sm.add(name, array)
        self.pselab = []
        if ds.has_pselab and ds.pselab_data is not None:
            for key, rows in ds._pselab_rows(self.indices, self.works).items():
                if rows.shape != (self.n,):
                    raise AssertionError("pseudo labels and points of a batch have different lengths")
                self.pselab.append(key)
                sm.add(key, rows)
            if len({sm.layout[k][1] for k in self.pselab}) > 1:
                raise TypeError("begin_gpu_batch: the pseudo-label arrays of a dataset must share one dtype")
        self.gpu_idx, self.jpeg_paths = [], []
        if self.on_gpu:
            self._host_images([w.image for w in self.works], drawn.jitter, imageprep.lut(ds._to_float, ds._normalise))
        else:
            self.images.add("img", np.stack([s["img"] for s in scenes]).astype(np.float32))
            self.images.seal()
        sm.seal()
        self._state = "hosted"

    def _host_images(self, plans, jitter, lut):
        """The host half of ``dataprep.prepare_images`` into the staging blocks; nothing is launched."""
        B, sm, im = self.B, self.small, self.images
        sizes = self.sizes = dataprep.source_sizes(plans)
        self.src_bytes = int(sum(sizes))
        src_offs = self.src_offs = dataprep.source_offsets(plans)
        headers = [None] * B
        if dataprep.GPU_JPEG:
            paths, data_offs = dataprep.jpeg_files(plans)
            files = np.empty(max(int(data_offs[-1]), 1), np.uint8)
            headers = dataprep.read_jpeg_files(paths, data_offs, files)
        self.gpu_idx, self.host_idx = dataprep.split_decoders(headers)
        self.jpeg_paths = [dataprep.jpeg_path(plans[i]) for i in self.gpu_idx]
        if self.gpu_idx:
            im.reserve("jpeg", np.uint8, (files.size,))  # first: at the block's own (allocator) alignment
            self.jpeg_desc, huff, qt, self.jpeg_totals = jpeg.build_tables(
                [headers[i] for i in self.gpu_idx], [data_offs[i] for i in self.gpu_idx], [src_offs[i] for i in self.gpu_idx])
            sm.add("jpeg_desc", self.jpeg_desc)
            sm.add("jpeg_huff", huff)
            sm.add("jpeg_qt", qt)
        hplans = [plans[i] for i in self.host_idx]
        if hplans:
            im.reserve("decoded", np.uint8, (sum(sizes[i] for i in self.host_idx),))
        im.seal()
        if self.gpu_idx:
            im.host("jpeg")[...] = files
        self.host_offs = imageprep.decode_into(hplans, im.host("decoded"), self.decode_threads) if hplans else []
        *tables, self.tmp_bytes = imageprep.build_tables(plans, jitter, self.flips, [lut] * B, src_offs)
        self.img_desc = tables[0]
        for name, array in zip(("img_desc", "img_coef", "img_fac", "img_lut"), tables):
            sm.add(name, array)

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
        nj, keep_host = len(self.gpu_idx), bool(self.ds.output_orig)
        nk = max(n, 1)
        rb = torch.empty(B + 2 + nj + (nk if keep_host else 0), dtype=torch.int32, device=dev)
        counts, err, status = rb[: B + 1], rb[B + 1 : B + 2], rb[B + 2 : B + 2 + nj]
        keep = rb[B + 2 + nj :] if keep_host else torch.empty(nk, dtype=torch.int32, device=dev)
        counts.zero_()
        # ---- images
        if self.on_gpu:
            if self.gpu_idx:
                src = torch.empty(max(self.src_bytes, 1), dtype=torch.uint8, device=dev)
                dataprep._launch_jpeg_decode(im.device(im_d, "jpeg"), d("jpeg_desc"), self.jpeg_desc, d("jpeg_huff"), d("jpeg_qt"),
                                             self.jpeg_totals, src, status)
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
            dataprep._launch_image_prepare(src, self.src_bytes, d("img_desc"), self.img_desc, d("img_coef"), d("img_fac"), d("img_lut"),
                                           tmp, mid, sums, img)
        else:
            img = im.device(im_d, "img")
            if any(self.flips):
                img = torch.stack([t.flip(-1) if f else t for t, f in zip(img, self.flips)])
        C = img.shape[1]
        # ---- voxelisation and projection
        pts, off_d, labels = d("points"), d("off"), d("labels")
        pdt = pts.dtype
        locs = torch.empty((nk, 4), dtype=torch.int64, device=dev)
        minv = torch.empty((B, 3), dtype=pdt, device=dev)
        offset = torch.empty((B, 3), dtype=torch.float64, device=dev)
        dataprep._launch_voxelize(pts, off_d, self.off, d("rot"), d("u"), self.transl, self.ds.scale, self.ds.full_scale, locs, keep,
                                  counts, minv, offset)
        idx_all = torch.empty((nk, 2), dtype=torch.int64, device=dev)
        depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        seg2d = torch.empty((B, H, W), dtype=torch.float64, device=dev) if self.want_seg2d else None
        winner = torch.empty(B * H * W, dtype=torch.int32, device=dev)
        dataprep._launch_project(d("pimg"), d("depth"), labels, off_d, self.off, d("flip"), idx_all, depth, seg2d, winner, err)
        # ---- collect: launched over the point count, the kept total is read on the device
        idx = torch.empty((nk, 2), dtype=torch.int64, device=dev)
        lab = torch.empty(nk, dtype=torch.int64, device=dev)
        feats = torch.empty((nk, C), dtype=torch.float32, device=dev) if self.ds.use_rgb else None
        pkept = torch.empty((nk, 3), dtype=pdt, device=dev)
        pl_in = [d(k) for k in self.pselab]
        pl_out = [torch.empty(nk, dtype=t.dtype, device=dev) for t in pl_in]
        collect_points_dev(keep, counts, B, n, locs, idx_all, labels, img.contiguous() if feats is not None else None, H, W, pts, idx, lab,
                           feats, pkept, pl_in, pl_out)
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
        self._dev = dict(locs=locs, feats=feats, seg_label=lab, img=img, depth=depth, seg2d=seg2d, img_indices=idx, points=pkept,
                         min_values=minv, offsets=offset, keep=keep)
        self._held = (pl_out, rb, sm_d, im_d)  # what the queued kernels read and write stays allocated until result()
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
        B, t = self.B, self._dev
        nj, keep_host, kept = len(self.gpu_idx), bool(self.ds.output_orig), int(r[B])
        self._state = "failed"
        dataprep.check_projection(r[B + 1])
        dataprep.check_jpeg_status(self.jpeg_paths, r[B + 2 : B + 2 + nj].tolist())
        for key in ("locs", "seg_label", "img_indices", "points", "keep") + (("feats",) if self.ds.use_rgb else ()):
            t[key] = t[key][:kept]  # outputs were allocated at the batch's point count
        pselab = None
        if self.ds.has_pselab and self.ds.pselab_data is not None:
            pselab = {key: rows[:kept] for key, rows in zip(self.pselab, self._held[0])}
        batch = dataprep.finish_batch(dict(t, counts=r[:B].tolist()), self.rots, self.flips, self.intrinsics,
                                      self.works if keep_host else None, r[B + 2 + nj : B + 2 + nj + kept], pselab)
        self._held = None
        self._dev = self.works = None
        self._result, self._state = batch, "done"
        return batch


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
