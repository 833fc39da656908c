"""float64 numpy references of the per-point row kernels (csrc/point.hip) and makers of their test inputs; shared by
tests/test_point_rows_host.py and tests/test_gpu_point_rows.py (no tests here).

Operands are 2-D arrays.  A leading dimension is a property of the array handed in: ``rows(flat, n, c, ld, off)`` is the [n, c]
view of a flat buffer whose rows are ``ld`` elements apart, and every reference reads and writes through such views unchanged.

Grid inputs: every value is a multiple of a quantum q = 2^-k of small magnitude.  A product of two is a multiple of q^2, and while
sum |terms| / q^2 < 2^24 every partial sum of such terms, taken in any order, is a multiple of q^2 below 2^24 * q^2: an fp32 (and
fp64) number.  So every fp32 FMA, fp32 partial sum and fp64 combination of the kernels is exact and the result equals the float64
reference bit for bit.  The makers assert that condition for every reduction of the case (``assert_exact``)."""
import numpy as np

LIMIT = float(1 << 24)


# ------------------------------------------------------------------------------------------------------------------ views
def rows(flat, n, c, ld, off=0):
    """The [n, c] view of rows ``ld`` apart that starts ``off`` elements into the 1-D array ``flat``."""
    assert c <= ld or n <= 1
    assert flat.ndim == 1 and (n == 0 or off + (n - 1) * ld + c <= flat.size)
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(n, c), strides=(ld * flat.itemsize, flat.itemsize))


# -------------------------------------------------------------------------------------------------------------- references
def gate_fwd(x, w, b):
    """y = x * sigmoid(x.w + b); returns (y [N, C], mask [N])."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1)
    z = x @ w + float(b)
    e = np.exp(-np.abs(z))  # 1 / (1 + exp(-z)) without overflow at either end
    mask = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return x * mask[:, None], mask


def gate_bwd_terms(x, w, b, dy):
    """(dx [N, C], per-row terms of dw [N, C], per-row terms of db [N]) of y = x * sigmoid(x.w + b)."""
    x, w, dy = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1), np.asarray(dy, np.float64)
    _, m = gate_fwd(x, w, b)
    z = x @ w + float(b)
    e = np.exp(-np.abs(z))
    dsig = e / (1.0 + e) ** 2  # m * (1 - m) without cancellation where m rounds to 1
    dz = (dy * x).sum(1) * dsig
    return dy * m[:, None] + dz[:, None] * w[None, :], dz[:, None] * x, dz


def gate_bwd(x, w, b, dy):
    """(dx [N, C], dw [C], db scalar)."""
    dx, tw, tb = gate_bwd_terms(x, w, b, dy)
    return dx, tw.sum(0), tb.sum()


def segment_sum(feats, csr_off, csr_items):
    """out[v] = sum of feats[i] over i in csr_items[csr_off[v] : csr_off[v + 1]]."""
    feats = np.asarray(feats, np.float64)
    n_vox = len(csr_off) - 1
    out = np.zeros((n_vox, feats.shape[1]))
    seg = np.repeat(np.arange(n_vox), np.diff(csr_off))
    np.add.at(out, seg, feats[np.asarray(csr_items[: len(seg)], np.int64)])
    return out


def segment_mean(feats, csr_off, csr_items):
    return segment_sum(feats, csr_off, csr_items) / np.diff(csr_off).astype(np.float64)[:, None]


def row_gather(vox, p2v, csr_off, div_count):
    """out[p] = vox[p2v[p]] (divided by the voxel's item count when ``div_count``); a row with p2v < 0 is zero."""
    vox, p2v = np.asarray(vox, np.float64), np.asarray(p2v, np.int64)
    out = np.zeros((len(p2v), vox.shape[1]))
    live = p2v >= 0
    out[live] = vox[p2v[live]]
    if div_count:
        out[live] /= np.diff(csr_off).astype(np.float64)[p2v[live]][:, None]
    return out


def linear_fwd(x, w, b=None):
    """y = x W^T + b with W [Cout, Cin]."""
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    return y if b is None else y + np.asarray(b, np.float64)[None, :]


def linear_bwd(x, dy, w):
    """(dx [N, Cin], dw [Cout, Cin], db [Cout])."""
    x, dy, w = np.asarray(x, np.float64), np.asarray(dy, np.float64), np.asarray(w, np.float64)
    return dy @ w, dy.T @ x, dy.sum(0)


# ------------------------------------------------------------------------------------------------------- fp32 restatements
def _f32(a):
    return np.asarray(a, np.float32)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in fp64, so one fp64 add and one rounding to fp32 follow."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gate_fp32(x, w, b, dy, dw0=None, db0=None):
    """The kernels' formulas step by step in numpy float32 (rows summed in fp64, as the kernels do): what fp32 arithmetic alone
    costs against the float64 reference.  Returns dict(y, mask, dx, dw, db)."""
    x, w, dy = _f32(x), _f32(w).reshape(-1), _f32(dy)
    N, C = x.shape
    z = np.full(N, np.float32(b), np.float32)
    for c in range(C):
        z = _fma32(x[:, c], np.broadcast_to(w[c], (N,)), z)
    with np.errstate(over="ignore"):
        m = (np.float32(1) / (np.float32(1) + np.exp(-z, dtype=np.float32))).astype(np.float32)
    y = x * m[:, None]
    dm = np.zeros(N, np.float32)
    for c in range(C):
        dm = _fma32(dy[:, c], x[:, c], dm)
    dz = (dm * m).astype(np.float32) * (np.float32(1) - m)
    dx = (dy * m[:, None]).astype(np.float32) + (dz[:, None] * w[None, :]).astype(np.float32)
    dw = _f32((dz[:, None] * x).astype(np.float32).astype(np.float64).sum(0))
    db = _f32(dz.astype(np.float64).sum())
    if dw0 is not None:
        dw, db = _f32(dw0) + dw, np.float32(db0) + db
    return dict(y=y, mask=m, dx=dx, dw=dw, db=db)


def gate_errors(x, w, b, dy, got, dw0=None, db0=None, ref=None):
    """Largest error of ``got`` (dict of y, mask, dx, dw, db; any may be missing) against the float64 reference (or against ``ref``, a
    dict of the same five from another float64 implementation), per quantity, each in the unit in which fp32 rounding of that
    quantity is bounded:
      mask  absolute (it lies in [0, 1])
      y     per element, relative to |x|                              (y = x * mask)
      dx    per element, relative to |dy| + sum_c |dy_c x_c| * |w|    (dx = dy * mask + dz * w, |mask| <= 1)
      dw    per channel, relative to sum_rows |dz x| (+ |dw0|)        (sum |terms|)
      db    relative to sum_rows |dz| (+ |db0|)"""
    x64, w64, dy64 = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1), np.asarray(dy, np.float64)
    y, m = gate_fwd(x64, w64, b)
    dx, tw, tb = gate_bwd_terms(x64, w64, b, dy64)
    dw, db = tw.sum(0), tb.sum()
    if ref is not None:
        y, m, dx = (np.asarray(ref[k], np.float64).reshape(s) for k, s in (("y", y.shape), ("mask", m.shape), ("dx", dx.shape)))
        dw, db = np.asarray(ref["dw"], np.float64).reshape(-1), float(np.asarray(ref["db"]).reshape(-1)[0])
    sw, sb = np.abs(tw).sum(0), np.abs(tb).sum()
    if dw0 is not None:
        dw, db = dw + np.asarray(dw0, np.float64), db + float(db0)
        sw, sb = sw + np.abs(np.asarray(dw0, np.float64)), sb + abs(float(db0))

    def worst(err, scale):
        err, scale = np.asarray(err, np.float64).reshape(-1), np.asarray(scale, np.float64).reshape(-1)
        assert np.isfinite(err).all(), "a result is not finite"
        assert (err[scale == 0] == 0).all(), "an element whose terms are all zero is not zero"
        live = scale > 0
        return float((err[live] / scale[live]).max()) if live.any() else 0.0

    out = {}
    if got.get("mask") is not None:
        out["mask"] = worst(np.abs(np.asarray(got["mask"], np.float64).reshape(-1) - m), np.ones_like(m))
    if got.get("y") is not None:
        out["y"] = worst(np.abs(np.asarray(got["y"], np.float64) - y), np.abs(x64))
    if got.get("dx") is not None:
        scale = np.abs(dy64) + np.abs(dy64 * x64).sum(1)[:, None] * np.abs(w64)[None, :]
        out["dx"] = worst(np.abs(np.asarray(got["dx"], np.float64) - dx), scale)
    if got.get("dw") is not None:
        out["dw"] = worst(np.abs(np.asarray(got["dw"], np.float64).reshape(-1) - dw), sw)
        out["db"] = worst(np.abs(float(np.asarray(got["db"], np.float64).reshape(-1)[0]) - db), sb)
    return out


# ------------------------------------------------------------------------------------------------------------ input makers
def grid(rng, shape, k=3, lim=2):
    """float64 multiples of 2^-k in [-lim, lim]."""
    return rng.integers(-lim << k, (lim << k) + 1, size=shape).astype(np.float64) / float(1 << k)


def assert_exact(sum_abs_terms, q_out, what):
    """The condition under which a reduction is exact in fp32 in any order: sum |terms| / q_out < 2^24."""
    worst = float(np.max(sum_abs_terms)) if np.size(sum_abs_terms) else 0.0
    assert worst / q_out < LIMIT, f"{what}: sum|terms| / q = {worst / q_out:.0f} is not below 2^24"
    return worst / q_out


def make_linear(cin, cout, n, k, seed):
    """Grid inputs of one linear case (k = 3: multiples of 1/8; k = 0: integers), with previous contents of dx, dw, db for the
    accumulating modes; asserts exactness of the forward, of dx, dw and db, each with and without accumulation and bias."""
    rng = np.random.default_rng(seed)
    d = dict(x=grid(rng, (n, cin), k), dy=grid(rng, (n, cout), k), w=grid(rng, (cout, cin), k), b=grid(rng, (cout,), k),
             dx0=grid(rng, (n, cin), k), dw0=grid(rng, (cout, cin), k), db0=grid(rng, (cout,), k))
    q2 = 2.0 ** (-2 * k)
    ax, ady, aw = np.abs(d["x"]), np.abs(d["dy"]), np.abs(d["w"])
    d["exact"] = dict(
        y=assert_exact(ax @ aw.T + np.abs(d["b"])[None, :], q2, "linear_fwd"),
        dx=assert_exact(ady @ aw + np.abs(d["dx0"]), q2, "linear_bwd dx"),
        dw=assert_exact(ady.T @ ax + np.abs(d["dw0"]), q2, "linear_bwd dw"),
        db=assert_exact(ady.sum(0) + np.abs(d["db0"]), q2, "linear_bwd db"))
    return d


def make_csr(n_vox, lengths, n_free, seed):
    """A voxel -> items CSR whose item lists are ascending and interleaved across voxels, over n_items = sum(lengths) + n_free
    items; the ``n_free`` items belong to no voxel (p2v = -1).  Returns (csr_off int32 [n_vox + 1], csr_items int32, p2v int32)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    assert len(lengths) == n_vox and (lengths >= 1).all()
    p2v = np.concatenate([np.repeat(np.arange(n_vox, dtype=np.int64), lengths), np.full(n_free, -1, np.int64)])
    rng.shuffle(p2v)
    order = np.argsort(p2v, kind="stable")  # items of a voxel in ascending order; the free items (-1) come first
    csr_items = order[n_free:]
    csr_off = np.concatenate([[0], np.cumsum(lengths)])
    return csr_off.astype(np.int32), csr_items.astype(np.int32), p2v.astype(np.int32)


def make_segments(c, n_vox, lengths, n_free, seed, k=3):
    """Grid inputs of one segment-reduce / row-gather case.  Rows of ``feats`` that belong to no voxel hold NaN: no kernel may read
    them.  Asserts exactness of every segment sum."""
    rng = np.random.default_rng(seed)
    csr_off, csr_items, p2v = make_csr(n_vox, lengths, n_free, seed + 1)
    feats = grid(rng, (len(p2v), c), k)
    q = 2.0 ** (-k)
    worst = assert_exact(segment_sum(np.abs(feats), csr_off, csr_items), q, "segment sum")
    feats[p2v < 0] = np.nan
    vox = grid(rng, (n_vox, c), k)
    return dict(feats=feats, vox=vox, csr_off=csr_off, csr_items=csr_items, p2v=p2v, exact=dict(sum=worst))


def make_gate(c, n, seed, special=True):
    """fp32-valued inputs of one gate case: x = 3 * randn, and (from 255 rows on) rows moved along w so that z = x.w + b lands near
    0, +-20 and +-90, where the sigmoid saturates in fp32."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(c).astype(np.float32)
    w[np.abs(w) < 0.25] = 0.5
    b = np.float32(0.5 * rng.standard_normal())
    x = (3 * rng.standard_normal((n, c))).astype(np.float32)
    dy = rng.standard_normal((n, c)).astype(np.float32)
    targets = [0.0, 1e-4, 20.0, -20.0, 17.5, 90.0, -90.0, 88.0, -104.0]
    if special and n >= 255:
        w64 = w.astype(np.float64)
        for i, t in enumerate(targets):
            r = 3 + 31 * i if i < 7 else n - 9 + i  # rows of all four waves of the first block and the last two rows
            z = x[r].astype(np.float64) @ w64 + float(b)
            x[r] = (x[r].astype(np.float64) + (t - z) * w64 / (w64 @ w64)).astype(np.float32)
    dw0 = grid(rng, (c,), 3)
    db0 = float(grid(rng, (), 3))
    return dict(x=x, w=w, b=b, dy=dy, dw0=dw0, db0=db0)
