"""The batched metadata build (one launch per stage for every level: mm_voxel_dedupe_levels, mm_neighbors_batch,
mm_rulebook_compact_batch) against the per-level entry points it replaces in ``Metadata`` (mm_voxel_dedupe, mm_subm_neighbors,
mm_down_neighbors, mm_rulebook_compact, called here through the C ABI level after level) and against the CPU oracle.
Every comparison is integer-exact."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scn_ref  # noqa: E402

I32 = torch.int32


def _dev():
    import mm2d3d_amd  # noqa: F401  (fails loudly when libmm2d3d_hip.so is missing)

    return torch.device("cuda:0")


def _random(seed, S, B, n, dup):
    g = np.random.default_rng(seed)
    coords = np.concatenate([g.integers(0, S, (n, 3)), g.integers(0, B, (n, 1))], 1).astype(np.int64)
    if dup:
        coords = np.concatenate([coords, coords[g.integers(0, n, dup)]], 0)
    return coords


@functools.lru_cache(maxsize=None)
def _case(name):
    """coords int64 [n,4] (numpy), spatial size, levels, domains.split argument"""
    if name == "random":
        return _random(0, 64, 3, 3000, 1000), 64, 5, None
    if name == "lidar":
        from mm2d3d_amd.synthetic import make_batch

        return make_batch(1, 2, "nuscenes", img_hw=(32, 48))["x"][0].numpy().astype(np.int64), 4096, 7, None
    if name == "single_point":
        return np.array([[5, 6, 7, 0]], dtype=np.int64), 16, 3, None
    if name == "empty":
        return np.zeros((0, 4), dtype=np.int64), 16, 2, None
    if name == "collapse":  # level 4 of a 16^3 grid: one voxel per scene
        return _random(1, 16, 2, 200, 0), 16, 5, None
    assert name == "collapse_split"  # batch-sorted, as the collate function delivers it
    c = _random(2, 16, 3, 200, 0)
    return c[np.argsort(c[:, 3], kind="stable")], 16, 5, 1


CASES = ["random", "lidar", "single_point", "empty", "collapse", "collapse_split"]


def _np(t):
    return t.cpu().numpy()


def _per_level(coords_np, S, nlev, split, no_spin):
    """The chain and the rulebooks through the per-level entry points, as Metadata built them before the batched calls."""
    from mm2d3d_amd import _lib
    from mm2d3d_amd._lib import check, ptr, stream

    L, dev = _lib.lib(), _dev()
    e = lambda *shape, dt=I32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    pts = torch.from_numpy(coords_np).to(dev).contiguous()
    n_pts = pts.shape[0]
    cap = int(L.mm_hash_capacity(n_pts))
    counts = torch.zeros(2 * nlev + 1, dtype=I32, device=dev)
    ws = e(int(L.mm_dedupe_ws_bytes(n_pts)), dt=torch.uint8)
    n1 = max(n_pts, 1)
    lv = []
    for l in range(nlev):
        d = dict(tkeys=e(cap, dt=torch.int64), tvals=e(cap), item2vox=e(n1), coords=e(n1, 4), csr_off=e(n_pts + 1), csr_items=e(n1))
        src, is64, ndev, shift = (pts, 1, None, 0) if l == 0 else (lv[-1]["coords"], 0, ptr(counts[l - 1 : l]), 1)
        check(L.mm_voxel_dedupe(ptr(src), is64, n_pts, ndev, shift, ptr(d["tkeys"]), ptr(d["tvals"]), cap, ptr(d["item2vox"]), ptr(d["coords"]),
                                ptr(d["csr_off"]), ptr(d["csr_items"]), ptr(counts[l : l + 1]), ptr(counts[nlev : nlev + 1]), no_spin, ptr(ws),
                                ws.numel(), stream()), "voxel_dedupe")
        if split is not None:
            check(L.mm_batch_lower_bound(ptr(d["coords"]), ptr(counts[l : l + 1]), split, ptr(counts[nlev + 1 + l : nlev + 2 + l]), stream()), "lb")
        lv.append(d)
    host = _np(counts)
    assert host[nlev] == 0
    n_items = n_pts
    for l, d in enumerate(lv):
        d["n"], d["n_items"], d["seg_rows"] = int(host[l]), n_items, int(host[nlev + 1 + l]) if split is not None else None
        n_items = d["n"]

    def rulebook(nbr, K, n):
        r = dict(nbr=nbr, rin=e(max(K * n, 1)), rout=e(max(K * n, 1)), offsets=torch.zeros(K + 1, dtype=I32, device=dev), csr_off=e(n + 1),
                 csr_pos=e(max(K * n, 1)))
        w = e(int(L.mm_rulebook_ws_bytes(n, K)), dt=torch.uint8)
        check(L.mm_rulebook_compact(ptr(nbr), K, n, ptr(r["rin"]), ptr(r["rout"]), ptr(r["offsets"]), ptr(r["csr_off"]), ptr(r["csr_pos"]), no_spin,
                                    ptr(w), w.numel(), stream()), "rulebook_compact")
        if n:  # the tile table of the output-stationary engine from this table
            nt = -(-n // 64)
            r["os"] = (e(nt * 64), e(K * nt * 64), e(nt))
            w = e(int(L.mm_os_table_ws_bytes(n, K)), dt=torch.uint8)
            check(L.mm_os_table_build(ptr(nbr), K, n, 64, no_spin, *(ptr(t) for t in r["os"]), ptr(w), w.numel(), stream()), "os_table_build")
        return r

    S_l = S
    for l, d in enumerate(lv):
        n = d["n"]
        nbr = e(max(27 * n, 1))
        check(L.mm_subm_neighbors(ptr(d["coords"]), n, S_l, ptr(d["tkeys"]), ptr(d["tvals"]), cap, ptr(nbr), stream()), "subm_neighbors")
        d["subm"] = rulebook(nbr, 27, n)
        if l + 1 < nlev:
            c = lv[l + 1]
            nbr8 = e(max(8 * c["n"], 1))
            check(L.mm_down_neighbors(ptr(d["coords"]), n, ptr(c["item2vox"]), c["n"], ptr(nbr8), stream()), "down_neighbors")
            d["down"] = rulebook(nbr8, 8, c["n"])
        S_l = max(S_l // 2, 1)
    return lv


def _batched(coords_np, S, nlev, split, no_spin, os_min_rows, pipelined=False):
    from mm2d3d_amd import domains
    from mm2d3d_amd.scn import metadata

    dev = _dev()
    old = metadata.OS_MIN_ROWS
    metadata.OS_MIN_ROWS = os_min_rows
    try:
        with domains.split(split), (metadata.no_spin() if no_spin else contextlib.nullcontext()):
            md = metadata.Metadata(dev, S, nlev)
            pts = torch.from_numpy(coords_np).to(dev).contiguous()
            if pipelined:
                md.begin_levels(pts)
                md.begin_rulebooks()
                md.ensure()
            else:
                md.build_levels(pts)
                md.build_rulebooks()
            while len(md.levels) < nlev:  # levels past log2(S) come from the lazy per-level path, reading the batched tables
                md.down_rulebook(md.levels[-1])
            md.subm_rulebook(md.levels[-1])
    finally:
        metadata.OS_MIN_ROWS = old
    return md


def _lookup(tkeys, tvals, keys):
    """Open-addressing lookups on the host: csrc/meta.hip hash_find."""
    M = np.uint64(len(tkeys) - 1)
    k = keys.copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xFF51AFD7ED558CCD)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xC4CEB9FE1A85EC53)
    k ^= k >> np.uint64(33)
    slot = k & M
    out = np.full(len(keys), -1, dtype=np.int64)
    todo = np.arange(len(keys))
    for _ in range(len(tkeys)):
        if not len(todo):
            break
        hit = tkeys[slot[todo]] == keys[todo]
        out[todo[hit]] = tvals[slot[todo[hit]]]
        todo = todo[~hit & (tkeys[slot[todo]] != np.uint64(0xFFFFFFFFFFFFFFFF))]
        slot[todo] = (slot[todo] + np.uint64(1)) & M
    return out


def _same_rulebook(what, g, r, csr):
    R = int(_np(r["offsets"])[-1])
    assert np.array_equal(g.offsets_host, _np(r["offsets"])), what
    assert g.n_rules == R and np.array_equal(_np(g.rin)[:R], _np(r["rin"])[:R]) and np.array_equal(_np(g.rout)[:R], _np(r["rout"])[:R]), what
    n = g.n_out
    if csr:
        assert g.os is None and g.nbr is None
        assert np.array_equal(_np(g.csr_off), _np(r["csr_off"])[: n + 1]) and np.array_equal(_np(g.csr_pos)[:R], _np(r["csr_pos"])[:R]), what
    elif n:
        assert g.csr_pos is None and np.array_equal(_np(g.nbr), _np(r["nbr"])[: g.K * n]), what
        for a, b in zip((g.os.dst, g.os.nbrp, g.os.tmask), r["os"]):
            assert np.array_equal(_np(a), _np(b)), what


def _same(md, ref, csr):
    assert len(md.levels) == len(ref)
    for l, (g, r) in enumerate(zip(md.levels, ref)):
        n, ni = r["n"], r["n_items"]
        assert (g.n, g.n_items, g.seg_rows) == (n, ni, r["seg_rows"]), l
        assert np.array_equal(_np(g.coords), _np(r["coords"])[:n]), l
        assert np.array_equal(_np(g.item2vox)[:ni], _np(r["item2vox"])[:ni]), l
        assert np.array_equal(_np(g.csr_off)[: n + 1], _np(r["csr_off"])[: n + 1]) and np.array_equal(_np(g.csr_items)[:ni], _np(r["csr_items"])[:ni]), l
        keys = scn_ref.pack_keys(_np(g.coords).astype(np.int64).reshape(-1, 4))
        assert np.array_equal(_lookup(_np(g.tkeys).view(np.uint64), _np(g.tvals), keys), np.arange(n)), l
        _same_rulebook(("subm", l), g.subm, r["subm"], csr)
        if l + 1 < len(ref):
            _same_rulebook(("down", l), g.down, r["down"], csr)


@pytest.mark.parametrize("no_spin", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_batched_build_equals_the_per_level_entry_points(case, no_spin):
    coords, S, nlev, split = _case(case)
    ref = _per_level(coords, S, nlev, split, no_spin)
    _same(_batched(coords, S, nlev, split, no_spin, 1 << 60), ref, csr=True)
    _same(_batched(coords, S, nlev, split, no_spin, 0), ref, csr=False)  # every table with rows feeds a tile table


@pytest.mark.parametrize("no_spin", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_batched_build_equals_the_oracle(case, no_spin):
    coords, S, nlev, split = _case(case)
    md = _batched(coords, S, nlev, split, no_spin, 1 << 60, pipelined=bool(no_spin))
    p2v, first = scn_ref.first_occurrence_ids(scn_ref.pack_keys(coords))
    lv = scn_ref.Level(coords[first], S)
    assert np.array_equal(_np(md.levels[0].item2vox), p2v)
    for l in range(nlev):
        g = md.levels[l]
        assert g.n == lv.n, (l, g.n, lv.n)
        assert np.array_equal(_np(g.coords).astype(np.int64).reshape(-1, 4), lv.coords)
        rb = scn_ref.subm_rulebook(lv)
        assert np.array_equal(g.subm.offsets_host.astype(np.int64), rb.offsets)
        R = rb.n_rules
        assert np.array_equal(_np(g.subm.rin)[:R], rb.rin) and np.array_equal(_np(g.subm.rout)[:R], rb.rout)
        if l + 1 < nlev:
            rb8, coarse = scn_ref.down_rulebook(lv)
            assert np.array_equal(g.down.offsets_host.astype(np.int64), rb8.offsets)
            assert np.array_equal(_np(g.down.rin)[: rb8.n_rules], rb8.rin) and np.array_equal(_np(g.down.rout)[: rb8.n_rules], rb8.rout)
            lv = coarse


@pytest.mark.parametrize("case", CASES)
def test_pipelined_build_equals_the_inline_one(case):
    coords, S, nlev, split = _case(case)
    a = _batched(coords, S, nlev, split, 0, 1 << 60)
    b = _batched(coords, S, nlev, split, 0, 1 << 60, pipelined=True)
    for g, h in zip(a.levels, b.levels):
        assert (g.n, g.n_items, g.seg_rows) == (h.n, h.n_items, h.seg_rows)
        for name in ("coords", "item2vox", "csr_off", "csr_items"):
            assert torch.equal(getattr(g, name), getattr(h, name)), name
        for x, y in ((g.subm, h.subm), (g.down, h.down)):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(x.offsets_host, y.offsets_host)
                for name in ("rin", "rout", "csr_off", "csr_pos"):
                    assert torch.equal(getattr(x, name), getattr(y, name)), name


@pytest.mark.parametrize("no_spin", [0, 1])
def test_out_of_range_coordinates_raise(no_spin):
    from mm2d3d_amd.scn import metadata

    dev = _dev()
    for bad in ([-1, 0, 0, 0], [0, 65536, 0, 0], [0, 0, 0, -2]):
        md = metadata.Metadata(dev, 16, 2)
        with pytest.raises(ValueError), (metadata.no_spin() if no_spin else contextlib.nullcontext()):
            md.build_levels(torch.tensor([[1, 2, 3, 0], bad], device=dev))
