"""numpy reference of the sparse-to-dense cross-modal matching (include/mm2d3d.h mm_xm_search, losses.cross_modal_dense): the window
search in float64, the same in float32 in the kernel's order of operations, the counters, and the dense gradient of a lift at
selected keys.  No tests here; importing this needs no GPU.

Definition.  Point i has pixel key (b*H + y)*W + x.  Its candidates are the pixels (b, y+dy, x+dx), |dy|, |dx| <= r, inside image
b, in the order: the centre, then the others row-major (dy ascending, then dx).  direction 0: value_j = KL(softmax(row_i) ||
softmax(map_j)); direction 1: value_j = KL(softmax(map_j) || softmax(row_i)).  The match is the candidate of the smallest value, the
earliest among equal ones; a NaN value is skipped; nothing left: the centre."""
import numpy as np

F32, F64 = np.float32, np.float64


def window(r):
    """The (dy, dx) of the candidates in their order."""
    rest = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
    return [(0, 0)] + rest


def decode(key, H, W):
    key = np.asarray(key, np.int64)
    return key // (H * W), (key % (H * W)) // W, key % W


def _log_softmax64(x):
    x = np.asarray(x, F64)
    with np.errstate(invalid="ignore"):
        m = x.max(-1, keepdims=True)
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def kl64(teacher, student):
    """Row-wise KL(softmax(teacher) || softmax(student)) in float64 and its scale sum_c q (|log q| + |log p|)."""
    lq, lp = _log_softmax64(teacher), _log_softmax64(student)
    with np.errstate(invalid="ignore"):
        q = np.exp(lq)
        return (q * (lq - lp)).sum(-1), (q * (np.abs(lq) + np.abs(lp))).sum(-1)


def _lse32(x):
    """rows.h row_lse and the caller's m + logf(s) in float32: fmaxf from x[0] on, the sum ascending in c."""
    x = np.asarray(x, F32)
    m = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        m = np.fmax(m, x[:, c])
    s = np.zeros(x.shape[0], F32)
    for c in range(x.shape[1]):
        s = (s + np.exp((x[:, c] - m).astype(F32)).astype(F32)).astype(F32)
    return (m + np.log(s).astype(F32)).astype(F32)


def kl32(teacher, student):
    """The kernel's expression in float32: sum_c expf(lq_c) * (lq_c - (p_c - lp)), c ascending."""
    t, p = np.asarray(teacher, F32), np.asarray(student, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lt, lp = _lse32(t), _lse32(p)
        a = np.zeros(t.shape[0], F32)
        for c in range(t.shape[1]):
            lq = (t[:, c] - lt).astype(F32)
            a = (a + (np.exp(lq).astype(F32) * (lq - (p[:, c] - lp).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    return a


def search(seg, key, rows, r, direction, P=None, precision=64):
    """seg [B, H, W, C], key [N], rows [N, C].  Returns dict: ``values`` [N, n_cand] (NaN where not counted), ``inside`` [N, n_cand],
    ``ord`` [N] the match's place in the order, ``sel`` [N] its key, ``klmin`` [N] (the centre's own value when nothing is counted),
    ``scale`` [N] the matched KL's sum_c q (|log q| + |log p|), ``gap`` [N] second-smallest minus smallest counted value (inf with
    fewer than two), ``moved`` / ``shift`` [2] over the rows [0, P) and [P, N)."""
    seg, rows = np.asarray(seg), np.asarray(rows)
    B, H, W, C = seg.shape
    key = np.asarray(key, np.int64)
    N = key.shape[0]
    P = N if P is None else P
    b, y, x = decode(key, H, W)
    cands = window(r)
    values = np.full((N, len(cands)), np.nan, F64 if precision == 64 else F32)
    scale = np.zeros((N, len(cands)), F64)
    inside = np.zeros((N, len(cands)), bool)
    for j, (dy, dx) in enumerate(cands):
        yy, xx = y + dy, x + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        inside[:, j] = ok
        pix = seg[b, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        t, s = (rows, pix) if direction == 0 else (pix, rows)
        if precision == 64:
            v, sc = kl64(t, s)
            scale[:, j] = sc
        else:
            v = kl32(t, s)
        values[:, j] = np.where(ok, v, np.nan)
    raw_centre = values[:, 0].copy()
    counted = inside & ~np.isnan(values)
    big = np.where(counted, values, np.inf)
    # argmin returns the first of equal entries: the earliest candidate; an uncounted one (inf here) only wins when nothing is
    # counted or every counted value is +inf - then take the first COUNTED one, else the centre
    order = np.argmin(big, 1)
    for i in np.nonzero(~counted[np.arange(N), order])[0]:
        c = np.nonzero(counted[i])[0]
        order[i] = c[0] if len(c) else 0
    none = ~counted.any(1)
    klmin = np.where(none, raw_centre, values[np.arange(N), order])
    two = np.sort(big, 1)[:, :2] if len(cands) > 1 else np.concatenate([big, np.full((N, 1), np.inf)], 1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isinf(two[:, 1]), np.inf, two[:, 1] - two[:, 0])
    dyx = np.asarray(cands, np.int64)[order]
    sel = key + dyx[:, 0] * W + dyx[:, 1]
    cheb = np.abs(dyx).max(1)
    seg_of = (np.arange(N) >= P).astype(np.int64)
    moved = np.asarray([int(((order != 0) & (seg_of == s)).sum()) for s in (0, 1)], np.int64)
    shift = np.asarray([int(cheb[(order != 0) & (seg_of == s)].sum()) for s in (0, 1)], np.int64)
    return dict(values=values, inside=inside, ord=order, sel=sel.astype(np.int64), klmin=klmin, scale=scale[np.arange(N), order], gap=gap,
                moved=moved, shift=shift)


def gather(seg, key):
    """Rows of seg [B, H, W, C] at pixel keys."""
    B, H, W, C = seg.shape
    return np.asarray(seg).reshape(B * H * W, C)[np.asarray(key, np.int64)]


def scatter64(drows, key, n_pixels):
    """index_put(accumulate=True) in float64: ``(dense [n_pixels, C], abs [n_pixels, C] the sums of |terms|, k [n_pixels] the
    number of terms)``."""
    d = np.asarray(drows, F64)
    key = np.asarray(key, np.int64)
    dense, mag = np.zeros((n_pixels, d.shape[1])), np.zeros((n_pixels, d.shape[1]))
    np.add.at(dense, key, d)
    np.add.at(mag, key, np.abs(d))
    return dense, mag, np.bincount(key, minlength=n_pixels)


# ------------------------------------------------------------------------------------------------------------- input makers
def make_points(rng, B, H, W, N):
    """N pixel keys drawn with replacement (many points share pixels); the first points sit on the corners and edges of every image."""
    fixed = [(b, y, x) for b in range(B) for y in (0, H - 1) for x in (0, W - 1)]
    fixed += [(b, y, x) for b in range(B) for y, x in ((0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1))]
    f = np.asarray(fixed, np.int64)
    b = np.concatenate([f[:, 0], rng.integers(0, B, N - len(f))])
    y = np.concatenate([f[:, 1], rng.integers(0, H, N - len(f))])
    x = np.concatenate([f[:, 2], rng.integers(0, W, N - len(f))])
    return ((b * H + y) * W + x).astype(np.int32)


def make_case(seed, B, H, W, C, N):
    """``(seg [B, H, W, C], key [N], rows [N, C])``: float32 logits 3 * randn."""
    rng = np.random.default_rng(seed)
    seg = (3 * rng.standard_normal((B, H, W, C))).astype(F32)
    rows = (3 * rng.standard_normal((N, C))).astype(F32)
    return seg, make_points(rng, B, H, W, N), rows


# the shapes of tests/test_gpu_xmdense.py; one set of inputs per class count, shared by every radius and both directions
B, H, W, N = 3, 7, 9, 4000
CLASSES, RADII, SPLITS = (2, 6, 11, 32), (1, 2, 3), (0, 1700, N)
GAP = 1e-5  # rows whose float64 best-to-second gap is smaller are left out of the selection comparison
LEFT_OUT_MAX = 0.02  # ... and they may be at most this share of a case's rows
# The share of rows left out is a property of the inputs alone (float64), and at C = 2 mostly of the 189 pixel rows of the map: both
# distributions of a pair are then often saturated, their KL is tiny and so are the gaps.  Over six draws of the C = 2 map it
# ranged from 1.0 % to 2.3 % at r = 3; the seed below gives 1.1 % (C = 2, r = 3) and under 0.1 % for C >= 6 or r = 1.
SEED = 300
# |klmin - float64| in units of (1 + float64 klmin), over the rows that are not left out, of every case here: the float32
# restatement (kl32: the kernel's expressions in numpy float32) reaches KLMIN_FP32 (measured on the CPU, rounded up;
# test_xmdense_host.py repeats the measurement); the kernel is allowed 8 x that - another expf / logf and the compiler's
# contractions cost a few ulp each.
KLMIN_FP32 = 9.6e-07
KLMIN_BOUND = 8 * KLMIN_FP32
_CASES = {}


def case(C):
    if C not in _CASES:
        _CASES[C] = make_case(SEED + C, B, H, W, C, N)
    return _CASES[C]


_REFS = {}


def case_ref(C, r, direction, P=None):
    """The float64 search of a case: computed once, shared, never modified."""
    k = (C, r, direction, P)
    if k not in _REFS:
        seg, key, rows = case(C)
        _REFS[k] = search(seg, key, rows, r, direction, P)
    return _REFS[k]


def klmin_error(got, ref, rows):
    """The largest |got - klmin| over ``rows`` in units of (1 + klmin)."""
    return float((np.abs(np.asarray(got, F64)[rows] - ref["klmin"][rows]) / (1.0 + ref["klmin"][rows])).max())
