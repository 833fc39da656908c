"""Host checks behind tests/test_gpu_point_rows.py: the float64 references of tests/_point_ref.py against torch float64 autograd,
the exactness condition of the grid inputs for every case of the GPU file's tables, the measurement from which the gate bounds come,
and the C ABI of the point-row entries (include/mm2d3d.h against mm2d3d_amd/_lib.py).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _point_ref as R
import test_gpu_point_rows as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, what):
    """1e-12 relative to the largest magnitude of the quantity."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(np.abs(want).max(initial=0.0), 1e-300), what


def _pitched(a, ld, off):
    """``a`` as a view of rows ``ld`` apart in a NaN-filled flat buffer."""
    n, c = a.shape
    flat = np.full(off + n * ld + 3, np.nan)
    v = R.rows(flat, n, c, ld, off)
    v[...] = a
    return v


@pytest.mark.parametrize("C,N", [(1, 5), (4, 300), (8, 77)])
def test_gate_reference_matches_torch_float64_autograd(C, N):
    rng = np.random.default_rng(C)
    x, w, b, dy = 3 * rng.standard_normal((N, C)), rng.standard_normal(C), rng.standard_normal(), rng.standard_normal((N, C))
    xt, wt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, w, b))
    m = torch.sigmoid(xt @ wt + bt)
    (xt * m[:, None]).backward(torch.from_numpy(dy))
    y, mask = R.gate_fwd(x, w, b)
    dx, dw, db = R.gate_bwd(x, w, b, dy)
    _close(y, (xt * m[:, None]).detach().numpy(), "y")
    _close(mask, m.detach().numpy(), "mask")
    _close(dx, xt.grad.numpy(), "dx")
    _close(dw, wt.grad.numpy(), "dw")
    _close(db, bt.grad.numpy(), "db")
    # saturated rows stay finite, and the stable forms agree with the plain ones where those are accurate
    xs = np.array([[200.0] * C, [-200.0] * C, [0.0] * C])
    ys, ms = R.gate_fwd(xs, np.ones(C), 0.0)
    assert np.isfinite(ys).all() and ms[0] == 1.0 and 0.0 <= ms[1] < 1e-80 and ms[2] == 0.5
    assert np.isfinite(R.gate_bwd(xs, np.ones(C), 0.0, np.ones((3, C)))[0]).all()


@pytest.mark.parametrize("cin,cout,N,ld", [(16, 6, 50, 20), (5, 7, 33, 9), (3, 1, 1, 3)])
def test_linear_reference_matches_f_linear_and_honours_leading_dimensions(cin, cout, N, ld):
    rng = np.random.default_rng(cin)
    x, w, b, dy = rng.standard_normal((N, cin)), rng.standard_normal((cout, cin)), rng.standard_normal(cout), rng.standard_normal((N, cout))
    xt, wt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, w, b))
    yt = F.linear(xt, wt, bt)
    yt.backward(torch.from_numpy(dy))
    xp, dyp = _pitched(x, ld, 1), _pitched(dy, ld, 2)
    assert not xp.flags["C_CONTIGUOUS"] or N == 1
    _close(R.linear_fwd(xp, w, b), yt.detach().numpy(), "y")
    _close(R.linear_fwd(xp, w), F.linear(xt, wt).detach().numpy(), "y without bias")
    dx, dw, db = R.linear_bwd(xp, dyp, w)
    _close(dx, xt.grad.numpy(), "dx")
    _close(dw, wt.grad.numpy(), "dw")
    _close(db, bt.grad.numpy(), "db")


def test_segment_and_gather_references_match_index_ops_and_are_adjoint():
    rng = np.random.default_rng(3)
    n_vox, C = 40, 5
    lens = rng.choice([1, 2, 7, 30], size=n_vox)
    off, items, p2v = R.make_csr(n_vox, lens, 6, 11)
    n = len(p2v)
    assert n == lens.sum() + 6 and (p2v < 0).sum() == 6
    for v in range(n_vox):  # ascending inside a voxel; the lists of different voxels interleave
        seg = items[off[v]: off[v + 1]]
        assert (np.diff(seg) > 0).all() and (p2v[seg] == v).all()
    assert (np.diff(items) < 0).any()
    f, g = _pitched(rng.standard_normal((n, C)), 8, 1), _pitched(rng.standard_normal((n_vox, C)), 7, 0)
    ft = torch.tensor(np.ascontiguousarray(f), requires_grad=True)
    live = torch.from_numpy(p2v.astype(np.int64)) >= 0
    idx = torch.from_numpy(p2v.astype(np.int64))[live]
    st = torch.zeros(n_vox, C, dtype=torch.float64).index_add(0, idx, ft[live])
    mt = st / torch.from_numpy(lens.astype(np.float64))[:, None]
    _close(R.segment_sum(f, off, items), st.detach().numpy(), "segment sum")
    _close(R.segment_mean(f, off, items), mt.detach().numpy(), "segment mean")
    mt.backward(torch.from_numpy(np.ascontiguousarray(g)))
    _close(R.row_gather(g, p2v, off, 1), ft.grad.numpy(), "gather / count = gradient of the mean")
    plain = R.row_gather(g, p2v, off, 0)
    assert np.array_equal(plain[p2v >= 0], np.ascontiguousarray(g)[p2v[p2v >= 0]]) and not plain[p2v < 0].any()
    # <mean(f), g> = <f, gather_div(g)>
    lhs, rhs = (R.segment_mean(f, off, items) * g).sum(), (f * R.row_gather(g, p2v, off, 1)).sum()
    assert abs(lhs - rhs) <= 1e-12 * np.abs(f).sum()


def test_grid_inputs_of_every_gpu_case_satisfy_the_exactness_condition():
    for name, c in G.LINEAR_CASES.items():
        d = G.linear_inputs(name)  # the maker asserts sum |terms| / q^2 < 2^24 for y, dx, dw, db
        q = 2.0 ** -c["k"]
        for key in ("x", "dy", "w", "b", "dx0", "dw0", "db0"):
            a = d[key]
            assert np.array_equal(a, np.round(a / q) * q) and np.abs(a).max(initial=0.0) <= 2, (name, key)
        assert max(d["exact"].values()) < R.LIMIT
        assert c["k"] == 0 or c["n"] <= 65536, name
        assert d["x"].shape == (c["n"], c["cin"]) and d["dy"].shape == (c["n"], c["cout"])
        assert max(d["x"].nbytes, d["dy"].nbytes) // 2 <= 35 << 20, name  # the largest operand, as fp32 on the device
    for name, c in G.SEGMENT_CASES.items():
        d = G.segment_inputs(name)
        assert d["exact"]["sum"] < R.LIMIT and len(d["csr_off"]) == c["n_vox"] + 1
        assert (d["p2v"] < 0).sum() == c["n_free"] and np.isnan(d["feats"][d["p2v"] < 0]).all()
    with pytest.raises(AssertionError, match="2\\^24"):
        R.assert_exact(np.array([2.0 ** 24 / 64]), 1 / 64, "too large")
    with pytest.raises(AssertionError, match="2\\^24"):
        R.make_linear(16, 6, 400000, 3, 0)  # multiples of 1/8 over 400,000 rows: the weight gradient is past the condition


def test_the_case_tables_cover_what_they_claim():
    paths = {n: G.linear_paths(c) for n, c in G.LINEAR_CASES.items()}
    for path in ("fast", "generic"):
        nblk = {p["nblk"] for n, p in paths.items() if p["w"] == path and G.LINEAR_CASES[n]["dw"]}
        assert {1, 2, 7, 8, 9} <= nblk, (path, sorted(nblk))
        assert any(p["capped"] for p in paths.values() if p["w"] == path)
        for acc in (0, 1):
            assert any(p["dx"] == path and G.LINEAR_CASES[n]["acc_dx"] == acc and G.LINEAR_CASES[n]["dx"] for n, p in paths.items())
            assert any(p["w"] == path and G.LINEAR_CASES[n]["acc_w"] == acc for n, p in paths.items())
    assert paths["16x6_cap128"]["nblk"] == 128 and paths["5x7_cap512"]["nblk"] == 512
    assert any(p["w"] == "fast" and p["dx"] == "generic" for p in paths.values())
    assert paths["16x6_ldx20"]["fwd"] == "fast" and paths["16x6_ldx18"]["fwd"] == paths["16x6_xoff1"]["fwd"] == "generic"
    assert {(c["cin"], c["cout"]) for c in G.LINEAR_CASES.values()} >= {(16, 6), (16, 16), (16, 17), (5, 7), (32, 16), (3, 1)}
    assert {c["n"] for c in G.LINEAR_CASES.values()} >= {0, 1, 63, 64, 65, 255, 256, 257, 2049, 4097, 14337, 16385}
    assert any(64 * (c["cin"] + c["cout"]) * 4 > 65536 for c in G.LINEAR_CASES.values())
    assert len(G.LINEAR_CASES) <= 80
    lens = set()
    for name in G.SEGMENT_CASES:
        lens |= set(G.segment_lengths(name).tolist())
    assert lens >= {1, 2, 7, 100, 5000}
    assert {c["c"] for c in G.SEGMENT_CASES.values()} == {1, 3, 16, 17, 96}
    assert {c["n_vox"] for c in G.SEGMENT_CASES.values()} == {0, 1, 255, 257, 1000}
    assert {c for c, _ in G.GATE_CASES.values()} == {1, 4, 8} and {n for _, n in G.GATE_CASES.values()} == {0, 1, 255, 257, 2049, 1050625}
    # the rows that saturate the sigmoid are where they are meant to be
    d = G.gate_inputs("c4_n2049")
    z = d["x"].astype(np.float64) @ d["w"].astype(np.float64) + float(d["b"])
    for t in (0.0, 20.0, -20.0, 90.0, -90.0):
        assert np.abs(z - t).min() < 1e-3 * max(1.0, abs(t)), t


def test_gate_bounds_are_eight_times_the_measured_fp32_error():
    """The measurement the bounds of test_gpu_point_rows.py come from: the kernels' formulas in numpy float32 against the float64
    reference, largest error per quantity over all gate cases.  numpy's float32 exp differs by an ulp between CPU kinds, so the
    recorded bound must lie between 4 x and 16 x what is measured here (it was set to 8 x)."""
    worst = {}
    for name in G.GATE_CASES:
        d = G.gate_inputs(name)
        got = R.gate_fp32(d["x"], d["w"], d["b"], d["dy"])
        acc = R.gate_fp32(d["x"], d["w"], d["b"], d["dy"], d["dw0"], d["db0"])
        m = got["mask"].astype(np.float64)
        assert np.isfinite(m * (1 - m)).all()
        for errs in (R.gate_errors(d["x"], d["w"], d["b"], d["dy"], got),
                     R.gate_errors(d["x"], d["w"], d["b"], d["dy"], dict(dw=acc["dw"], db=acc["db"]), d["dw0"], d["db0"])):
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("fp32 restatement against float64:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(G.GATE_BOUNDS)
    for k, v in worst.items():
        assert 4 * v <= G.GATE_BOUNDS[k] <= 16 * v, (k, v, G.GATE_BOUNDS[k])


def test_workspace_size_and_prototypes_of_the_point_row_entries():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    pairs = {(c["cin"], c["cout"]) for c in G.LINEAR_CASES.values()} | {(c, 1) for c, _ in G.GATE_CASES.values()}
    for cin, cout in sorted(pairs):
        assert int(L.mm_point_ws_bytes(cin, cout)) >= 512 * (cin * cout + cout) * 8 + cout * 4, (cin, cout)
    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    want = {"mm_point_ws_bytes": 2, "mm_gate_fwd": 8, "mm_gate_bwd": 13, "mm_segment_reduce": 10, "mm_row_gather": 10, "mm_linear_fwd": 10,
            "mm_linear_bwd": 17}
    for name, n_args in want.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        res, args = _lib._PROTOS[name]
        assert len(m.group(1).split(",")) == len(args) == n_args, name
        assert res is (_lib.sz if name == "mm_point_ws_bytes" else _lib.i32), name
        assert hasattr(L, name)
