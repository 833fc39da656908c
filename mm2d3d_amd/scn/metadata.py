"""Device-side sparse metadata: active sets per scale, voxel hashes and rulebooks.

SparseConvNet keeps this in a C++ ``Metadata`` object filled by host hash maps
(reference call sites: scn_unet.py:113 InputLayer, :43/:68/:75 convolutions).  Here every
structure is built by HIP kernels (csrc/meta.hip) and stays in HBM; the host only learns the
row counts (two small D2H copies per batch: one after the dedupe chain, one after the rulebooks).
"""
from __future__ import annotations

import contextlib
import os

import weakref

import numpy as np
import torch

from .. import _lib, domains
from .._lib import check, ptr, stream

I32 = torch.int32
# 1 while a build runs on a side stream beside grid-barrier kernels: the ``no_spin`` / ``sort_merge`` argument of the metadata entry
# points (include/mm2d3d.h) - only kernels whose workgroups never wait for each other.  An explicit argument of every call: the
# library keeps no switch.
NO_SPIN = [0]


@contextlib.contextmanager
def no_spin():
    """Metadata built inside uses only kernels that never wait across workgroups (merge sort, three-kernel scans)."""
    prev, NO_SPIN[0] = NO_SPIN[0], 1
    try:
        yield
    finally:
        NO_SPIN[0] = prev


class _Readback:
    """A small device -> host copy that does not stall the host when it is issued: the counts go into a persistent pinned
    buffer by an asynchronous copy on the current stream, followed by an event; ``wait()`` blocks only if the GPU has not
    reached that point yet.  (``Tensor.cpu()`` waits for everything queued before it, and a fresh ``pin_memory()`` costs
    milliseconds: the buffers are a per-device ring, reused once their reader has consumed them.)"""

    _ring = {}
    SLOT = 512  # int32 per slot: 2 * levels + 1 counts, or levels x 37 bucket offsets

    def __init__(self, dev_tensor):
        n = dev_tensor.numel()
        if n > self.SLOT:
            raise ValueError("read-back larger than a staging slot")
        dev = dev_tensor.device
        ring = self._ring.setdefault(dev.index, {"free": [], "made": 0})
        if ring["free"]:
            self.buf = ring["free"].pop()
        else:
            self.buf = torch.empty(self.SLOT, dtype=I32).pin_memory()
            ring["made"] += 1
        self.dev_index, self.n, self.shape = dev.index, n, tuple(dev_tensor.shape)
        self.buf[:n].copy_(dev_tensor.reshape(-1), non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(dev))
        self._keep = dev_tensor  # the source must stay allocated until the copy has run

    def wait(self):
        self.event.synchronize()
        out = self.buf[: self.n].numpy().copy().reshape(self.shape)
        self._ring[self.dev_index]["free"].append(self.buf)
        self.buf = self._keep = None
        return out


class Rulebook:
    """k-major rule lists + CSR over destination rows (csrc/spconv.hip header)."""

    __slots__ = ("K", "rin", "rout", "offsets_dev", "offsets_host", "csr_off", "csr_pos", "n_rules", "n_out", "_keep", "os",
                 "os_up", "nbr")

    def __init__(self, K):
        self.K = K
        self.nbr = None    # the [K, n_out] neighbour table, kept only while the CSR has not been built (ensure_csr)
        self.os = None     # OsTable over the rulebook's destination rows (csrc/ostable.hip): the output-stationary engine
        self.os_up = None  # strided rulebooks only: OsTable with the roles swapped (destination = fine rows)

    @property
    def offsets_ptr(self):
        return self.offsets_host.ctypes.data

    def ensure_csr(self):
        """The destination-row CSR of the gather + reduce engine.  Rulebooks whose destination rows have an output-stationary
        table are built without it (every convolution over them normally takes that engine); the first call that does fall back
        to the rulebook engine builds it here from the retained neighbour table."""
        if self.csr_pos is not None:
            return
        L = _lib.lib()
        dev = self.nbr.device
        self.csr_pos = torch.empty(max(self.n_rules, 1), dtype=I32, device=dev)
        self.csr_off = torch.empty(self.n_out + 1, dtype=I32, device=dev)
        ws = _lib.workspace.get(int(L.mm_rulebook_ws_bytes(self.n_out, self.K)), dev)
        check(L.mm_rulebook_csr(ptr(self.nbr), self.K, self.n_out, ptr(self.csr_off), ptr(self.csr_pos), NO_SPIN[0], ptr(ws), ws.numel(), stream()),
              "rulebook_csr")
        self.nbr = None


class OsTable:
    """Tile table of the output-stationary engine: destination rows sorted by neighbour bitmask, cut into tiles."""

    __slots__ = ("K", "n_dst", "tile_rows", "n_tiles", "dst", "nbrp", "tmask")


# The output-stationary engine pays off on the large levels (measured on 16 NuScenes-shaped scenes: SubM levels 0-2, strided
# convolutions into levels 1-2); below ~200k destination rows the k-major rulebook engines keep the chip busier.
OS_MIN_ROWS = int(os.environ.get("MM_OS_MIN_ROWS", "200000"))
OS_BUILD_UP = os.environ.get("MM_OS_UP", "0") != "0"


def os_tile_rows(n):
    """Rows per workgroup tile of the output-stationary engine (csrc/osconv.hip: four 16-row MFMA sub-blocks, one per wave)."""
    return 64


class Level:
    """One spatial scale: n active sites, int32 coords [n,4] (x,y,z,batch), hash table, rulebooks."""

    def __init__(self, spatial_size):
        self.spatial_size = int(spatial_size)
        self.n = 0
        self.coords = None
        self.tkeys = self.tvals = None
        self.cap = 0
        self.item2vox = None   # items of the finer level (points for level 0) -> site id here
        self.csr_off = None    # site -> items (ascending)
        self.csr_items = None
        self.n_items = 0
        self.seg_rows = None   # rows [0, seg_rows) belong to the first statistics group (mm2d3d_amd/domains.py)
        self.subm = None
        self.down = None       # Rulebook (K=8) to self.coarse
        self.coarse = None
        self._fine = None      # weak: coarse <-> fine strong references would be a cycle, and a step's hash tables / rulebooks
                               # (hundreds of MB) would wait for a full pass of Python's cyclic collector instead of dying with the step


def _get_fine(self):
    return self._fine() if self._fine is not None else None


def _set_fine(self, lv):
    self._fine = weakref.ref(lv) if lv is not None else None


Level.fine = property(_get_fine, _set_fine)


class Metadata:
    def __init__(self, device, spatial_size, prebuild_levels=7, act16=False):
        self.act16 = bool(act16)  # 16-bit activation mode: every level gets output-stationary tables, both directions
        self.device = device
        self.spatial_size = int(spatial_size)
        self.prebuild_levels = prebuild_levels
        self.levels = []
        self._rulebooks_built = False
        self.ready = None   # event of the stream that built it (prebuild on a side stream)
        self.n_points = 0
        self.split = None
        self._pending_levels = None     # (read-back, nlev): begin_levels has queued the kernels, finish_levels reads the counts
        self._pending_rulebooks = None  # (read-back, [(level, subm, down)])

    # ------------------------------------------------------------------ active sets
    @classmethod
    def prebuild(cls, coords_i64, spatial_size, prebuild_levels=7, side_stream=None, after=None, act16=False):
        """Active sets and every rulebook of the level chain for ``coords``, optionally on ``side_stream`` (its kernels
        and its two small host read-backs then overlap whatever the caller already queued on the current stream, e.g. the
        2D branch).  ``after``: event the side stream waits for first (so that it cannot run ahead into memory the previous
        step still uses).  The result carries ``ready``: consumers on another stream wait for it (InputLayer does)."""
        md = cls(coords_i64.device, spatial_size, prebuild_levels, act16=act16)
        if side_stream is None:
            md.build_levels(coords_i64)
            md.build_rulebooks()
            return md
        cur = torch.cuda.current_stream(coords_i64.device)
        if after is not None:
            side_stream.wait_event(after)
        coords_i64.record_stream(side_stream)  # allocated on the caller's stream, read by the side stream's kernels
        # Nothing on the side stream may spin-wait across workgroups (the caller's stream may run single-launch batch norms,
        # csrc/fused_bn.h): the tile-table sort switches from Onesweep to the merge sort, everything else here is already free of
        # inter-workgroup waits (three-kernel scans, bounded CAS loops).
        prev, NO_SPIN[0] = NO_SPIN[0], 1
        try:
            with torch.cuda.stream(side_stream), _lib.workspace_slot("meta"):
                md.build_levels(coords_i64)
                md.build_rulebooks()
                md.ready = side_stream.record_event()
        finally:
            NO_SPIN[0] = prev
        # the tensors were allocated on the side stream and are consumed on ``cur``: tell the caching allocator
        for t in md.tensors():
            t.record_stream(cur)
        return md

    @staticmethod
    def _rulebook_tensors(rb):
        for name in Rulebook.__slots__:
            t = getattr(rb, name, None)
            if torch.is_tensor(t):
                yield t
            elif isinstance(t, OsTable):
                yield from (t.dst, t.nbrp, t.tmask)
            elif isinstance(t, (list, tuple)):
                for u in t:
                    if torch.is_tensor(u):
                        yield u

    def tensors(self):
        for lv in self.levels:
            for t in (lv.coords, lv.tkeys, lv.tvals, lv.item2vox, lv.csr_off, lv.csr_items):
                if t is not None:
                    yield t
            for rb in (lv.subm, lv.down):
                if rb is not None:
                    yield from self._rulebook_tensors(rb)

    def pending_tensors(self):
        """Device tensors of rulebooks that begin_rulebooks has queued and finish_rulebooks has not yet attached to their levels."""
        if self._pending_rulebooks is not None:
            for _lv, subm, down in self._pending_rulebooks[1]:
                for rb in (subm, down):
                    if rb is not None:
                        yield from self._rulebook_tensors(rb)

    def build_levels(self, coords_i64: torch.Tensor):
        """Dedupe chain: points -> level 0 -> level 1 ... (A.8 i, ii).  One host sync at the end."""
        self.begin_levels(coords_i64)
        return self.finish_levels()

    def ensure(self):
        """Completes whatever a pipelined build (begin_levels / begin_rulebooks, mm2d3d_amd/train.py ``fit_step(next_batch=)``)
        has left pending.  Returns level 0."""
        if self._pending_levels is not None:
            self.finish_levels()
        if self._pending_rulebooks is not None:
            self.finish_rulebooks()
        return self.levels[0]

    def begin_levels(self, coords_i64: torch.Tensor):
        """Queues the dedupe chain and an asynchronous read-back of the level sizes; nothing here waits for the GPU."""
        L = _lib.lib()
        dev = self.device
        n_pts = self.n_points = coords_i64.shape[0]
        nlev = max(1, min(self.prebuild_levels, max(1, int(np.log2(max(self.spatial_size, 2))))))
        counts = torch.empty(2 * nlev + 1, dtype=I32, device=dev)  # [n_0..n_{L-1}, err, seg_0..seg_{L-1}]
        split = self.split = domains.current()  # scenes [0, split) / [split, B) keep their own batch-norm statistics
        cap = int(L.mm_hash_capacity(n_pts))
        ws = _lib.workspace.get(int(L.mm_dedupe_levels_ws_bytes(n_pts, nlev)), dev)
        # one array per kind, a row per level: the whole chain is one call (no level waits for the size of the one before)
        n1 = max(n_pts, 1)
        tkeys = torch.empty((nlev, cap), dtype=torch.int64, device=dev)
        tvals = torch.empty((nlev, cap), dtype=I32, device=dev)
        item2vox = torch.empty((nlev, n1), dtype=I32, device=dev)
        coords = torch.empty((nlev, n1, 4), dtype=I32, device=dev)
        csr_off = torch.empty((nlev, n_pts + 1), dtype=I32, device=dev)
        csr_items = torch.empty((nlev, n1), dtype=I32, device=dev)
        check(
            L.mm_voxel_dedupe_levels(ptr(coords_i64), n_pts, nlev, ptr(tkeys), ptr(tvals), cap, ptr(item2vox), ptr(coords), ptr(csr_off),
                                     ptr(csr_items), -1 if split is None else split, ptr(counts), NO_SPIN[0], ptr(ws), ws.numel(), stream()),
            "voxel_dedupe_levels",
        )
        S = self.spatial_size
        prev = None
        for l in range(nlev):
            lv = Level(S)
            lv.cap = cap
            lv.tkeys, lv.tvals, lv.item2vox, lv.coords, lv.csr_off, lv.csr_items = tkeys[l], tvals[l], item2vox[l], coords[l], csr_off[l], csr_items[l]
            if prev is not None:
                prev.coarse, lv.fine = lv, prev
            self.levels.append(lv)
            prev = lv
            S = max(S // 2, 1)
        self._pending_levels = (_Readback(counts), nlev, n_pts, split)

    def finish_levels(self):
        """Host half of the level build: reads the sizes (blocks only if the GPU has not reached the read-back yet)."""
        rb_, nlev, n_pts, split = self._pending_levels
        self._pending_levels = None
        host = rb_.wait()  # sync #1
        if host[nlev] != 0:
            raise ValueError("InputLayer: coordinates must satisfy 0 <= x,y,z,batch < 65536")
        n_items = n_pts
        for l, lv in enumerate(self.levels):
            lv.n = int(host[l])
            lv.seg_rows = int(host[nlev + 1 + l]) if split is not None else None
            lv.n_items = n_items
            lv.coords = lv.coords[: lv.n]
            lv.item2vox = lv.item2vox[:n_items]
            lv.csr_off = lv.csr_off[: lv.n + 1]
            lv.csr_items = lv.csr_items[:n_items]
            n_items = lv.n
        return self.levels[0]

    def _extend(self, fine: Level):
        """Lazily add one more (coarser) level beyond the prebuilt chain."""
        L = _lib.lib()
        dev = self.device
        n = fine.n
        lv = Level(max(fine.spatial_size // 2, 1))
        lv.cap = int(L.mm_hash_capacity(n))
        lv.tkeys = torch.empty(lv.cap, dtype=torch.int64, device=dev)
        lv.tvals = torch.empty(lv.cap, dtype=I32, device=dev)
        lv.item2vox = torch.empty(max(n, 1), dtype=I32, device=dev)
        lv.coords = torch.empty((max(n, 1), 4), dtype=I32, device=dev)
        lv.csr_off = torch.empty(n + 1, dtype=I32, device=dev)
        lv.csr_items = torch.empty(max(n, 1), dtype=I32, device=dev)
        cnt = torch.zeros(3, dtype=I32, device=dev)
        ws = _lib.workspace.get(int(L.mm_dedupe_ws_bytes(n)), dev)
        check(
            L.mm_voxel_dedupe(ptr(fine.coords), 0, n, None, 1, ptr(lv.tkeys), ptr(lv.tvals), lv.cap, ptr(lv.item2vox),
                              ptr(lv.coords), ptr(lv.csr_off), ptr(lv.csr_items), ptr(cnt[0:1]), ptr(cnt[1:2]), NO_SPIN[0], ptr(ws),
                              ws.numel(), stream()),
            "voxel_dedupe",
        )
        if fine.seg_rows is not None:
            check(L.mm_batch_lower_bound(ptr(lv.coords), ptr(cnt[0:1]), self.split, ptr(cnt[2:3]), stream()), "batch_lower_bound")
        hc = cnt.cpu().numpy()
        lv.n = int(hc[0])
        lv.seg_rows = int(hc[2]) if fine.seg_rows is not None else None
        lv.n_items = n
        lv.coords = lv.coords[: lv.n]
        lv.csr_off = lv.csr_off[: lv.n + 1]
        fine.coarse, lv.fine = lv, fine
        self.levels.append(lv)
        return lv

    # ------------------------------------------------------------------ rulebooks
    def _takes_os(self, n):
        """Destination rows served by the output-stationary engine: their rulebook is built without the CSR."""
        return n != 0 and (n >= OS_MIN_ROWS or self.act16)

    def _os_table(self, nbr, K, n):
        if not self._takes_os(n):
            return None
        L = _lib.lib()
        dev = self.device
        t = OsTable()
        t.K, t.n_dst, t.tile_rows = K, n, os_tile_rows(n)
        t.n_tiles = -(-n // t.tile_rows)
        npad = t.n_tiles * t.tile_rows
        t.dst = torch.empty(npad, dtype=I32, device=dev)
        t.nbrp = torch.empty(K * npad, dtype=I32, device=dev)
        t.tmask = torch.empty(t.n_tiles, dtype=I32, device=dev)
        ws = _lib.workspace.get(int(L.mm_os_table_ws_bytes(n, K)), dev)
        check(L.mm_os_table_build(ptr(nbr), K, n, t.tile_rows, NO_SPIN[0], ptr(t.dst), ptr(t.nbrp), ptr(t.tmask), ptr(ws), ws.numel(),
                                  stream()), "os_table_build")
        return t

    def build_rulebooks(self, levels=None):
        """Submanifold (K=27) rulebook of every level + strided (K=8) rulebook between consecutive levels."""
        self.begin_rulebooks(levels)
        self.finish_rulebooks()

    def begin_rulebooks(self, levels=None):
        """Queues the rulebook / tile-table kernels of the levels and an asynchronous read-back of the bucket offsets."""
        if self._pending_levels is not None:
            self.finish_levels()
        if self._pending_rulebooks is not None:
            self.finish_rulebooks()
        L = _lib.lib()
        dev = self.device
        levels = [lv for lv in (levels or self.levels) if lv.subm is None]
        if not levels:
            return
        offs = torch.zeros((len(levels), 28 + 9), dtype=I32, device=dev)
        # The neighbour tables of every rulebook of the build lie back to back in one array (submanifold [27][n], strided
        # [8][n_coarse]), the rule lists at the same words of rin / rout, the CSRs of the tables that take one back to back in
        # csr_off / csr_pos: one launch per stage for all of them (mm_neighbors_batch, mm_rulebook_compact_batch).
        pending, tabs = [], []  # tabs: (rulebook, level, first table word, first csr_off word or -1, first csr_pos word, word in offs)
        total = rows = npos = 0
        for j, lv in enumerate(levels):
            subm, down = Rulebook(27), None
            subm.n_out = lv.n
            if lv.coarse is not None and lv.down is None:
                down = Rulebook(8)
                down.n_out = lv.coarse.n
            for rb, o in ((subm, 37 * j), (down, 37 * j + 28)):
                if rb is None:
                    continue
                csr = not self._takes_os(rb.n_out)
                tabs.append((rb, lv, total, rows if csr else -1, npos, o))
                total += rb.K * rb.n_out
                if csr:
                    rows += rb.n_out + 1
                    npos += rb.K * rb.n_out
            pending.append((lv, subm, down))
        nbr, rin, rout = (torch.empty(max(total, 1), dtype=I32, device=dev) for _ in range(3))
        csr_off = torch.empty(max(rows, 1), dtype=I32, device=dev)
        csr_pos = torch.empty(max(npos, 1), dtype=I32, device=dev)
        nd, rd = (_lib.NbrDesc * len(tabs))(), (_lib.RulebookDesc * len(tabs))()
        for i, (rb, lv, start, row0, pos0, o) in enumerate(tabs):
            w = rb.K * rb.n_out
            rb.nbr, rb.rin, rb.rout = nbr[start : start + w], rin[start : start + w], rout[start : start + w]
            rb.offsets_dev = offs.view(-1)[o : o + rb.K + 1]
            if row0 >= 0:
                rb.csr_off, rb.csr_pos = csr_off[row0 : row0 + rb.n_out + 1], csr_pos[pos0 : pos0 + w]
            else:
                rb.csr_off = rb.csr_pos = None
            if rb.K == 27:
                nd[i] = _lib.NbrDesc(ptr(lv.coords), ptr(lv.tkeys), ptr(lv.tvals), None, ptr(rb.nbr), lv.n, 0, lv.cap, lv.spatial_size, 27)
            else:
                nd[i] = _lib.NbrDesc(ptr(lv.coords), None, None, ptr(lv.coarse.item2vox), ptr(rb.nbr), lv.n, lv.coarse.n, 0, 0, 8)
            rd[i] = _lib.RulebookDesc(start, rb.n_out, row0, pos0, rb.K, o)
        check(L.mm_neighbors_batch(nd, len(tabs), stream()), "neighbors_batch")
        for rb, lv, *_ in tabs:  # the tile tables stay one call per table (csrc/ostable.hip)
            rb.os = self._os_table(rb.nbr, rb.K, rb.n_out)
            if rb.K == 8 and (OS_BUILD_UP or self.act16):  # unique-destination direction: the rulebook engine's direct scatter measured faster
                nbr_up = torch.empty(max(8 * lv.n, 1), dtype=I32, device=dev)
                check(L.mm_up_neighbors(ptr(lv.coords), lv.n, ptr(lv.coarse.item2vox), ptr(nbr_up), stream()), "up_neighbors")
                rb.os_up = self._os_table(nbr_up, 8, lv.n)
        ws = _lib.workspace.get(int(L.mm_rulebook_batch_ws_bytes(total, rows)), dev)
        check(L.mm_rulebook_compact_batch(ptr(nbr), rd, len(tabs), ptr(rin), ptr(rout), ptr(offs), ptr(csr_off), ptr(csr_pos), NO_SPIN[0],
                                          ptr(ws), ws.numel(), stream()), "rulebook_compact_batch")
        for rb, *_ in tabs:
            if rb.csr_pos is not None:
                rb.nbr = None  # kept only while the CSR has not been built (ensure_csr)
        self._pending_rulebooks = (_Readback(offs), pending)

    def finish_rulebooks(self):
        if self._pending_rulebooks is None:
            return
        rb_, pending = self._pending_rulebooks
        self._pending_rulebooks = None
        host = rb_.wait()  # sync #2
        for j, (lv, subm, down) in enumerate(pending):
            for rb, row in ((subm, host[j, :28]), (down, host[j, 28:37])):
                if rb is None:
                    continue
                rb.offsets_host = np.ascontiguousarray(row[: rb.K + 1], dtype=np.int32)
                rb.n_rules = int(rb.offsets_host[rb.K])
                rb.rin = rb.rin[: max(rb.n_rules, 1)]
                rb.rout = rb.rout[: max(rb.n_rules, 1)]
                if rb.csr_pos is not None:
                    rb.csr_pos = rb.csr_pos[: max(rb.n_rules, 1)]
            lv.subm = subm
            if down is not None:
                lv.down = down

    def subm_rulebook(self, lv: Level) -> Rulebook:
        if self._pending_rulebooks is not None:
            self.finish_rulebooks()
        if lv.subm is None:
            self.build_rulebooks()
            if lv.subm is None:
                self.build_rulebooks([lv])
        return lv.subm

    def down_rulebook(self, lv: Level):
        if self._pending_rulebooks is not None:
            self.finish_rulebooks()
        if lv.coarse is None:
            self._extend(lv)
        if lv.down is None:
            self.build_rulebooks()
            if lv.down is None:  # level added lazily after the batch build
                lv.subm = None
                self.build_rulebooks([lv])
        return lv.down, lv.coarse
