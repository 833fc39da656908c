"""float64 numpy references of the row-wise loss, confusion and lifting kernels (csrc/loss.hip, csrc/lift.hip), float32
restatements of the loss formulas, and makers of their test inputs; shared by tests/test_loss_rows_host.py,
tests/test_gpu_loss_rows.py and tests/test_gpu_lift_index.py (no tests here).

Cross entropy and KL go through expf / logf, so their comparison has a tolerance.  ``ce_fp32`` / ``kl_fp32`` restate the kernels'
formulas step by step in float32 (maximum, exp, sum in class order, log, the per-row term cast to float64 before it is summed);
exp and log are the correctly rounded float32 functions (computed in float64 and rounded once), so the measurement does not depend
on the exp of the machine's numpy.  ``ce_errors`` / ``kl_errors`` give the error of a result in the units the bounds are stated in.

Everything else is exact: weight sums on multiples of 1/8, integer confusion counts, integer keys, gathers, and scatter sums that
are either taken on grid inputs (any order gives the same bits) or compared with a sequential float32 sum in point order."""
import json
import os

import numpy as np

from _point_ref import assert_exact, grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64


def _f32(a):
    return np.asarray(a, F32)


def exp32(v):
    """Correctly rounded float32 exp of float32 arguments."""
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(v, F32).astype(F64)).astype(F32)


def log32(v):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(v, F32).astype(F64)).astype(F32)


def shipped_class_weights():
    """The class-weight lists of the three shipped experiment configurations, by experiment name."""
    with open(os.path.join(GOLDEN, "class_weights.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------- cross entropy
def counted(labels, C, ignore):
    labels = np.asarray(labels, np.int64)
    return (labels != ignore) & (labels >= 0) & (labels < C)


def _lse(x):
    m = x.max(1)
    return m + np.log(np.exp(x - m[:, None]).sum(1))


def ce(logits, labels, weight, ignore, grad_out=1.0):
    """Weighted-mean cross entropy over the counted rows and its gradient scaled by ``grad_out``, in float64.
    Returns dict(loss, sum_w, dlogits, live, abs_mean = sum w |nll| / sum w, w_max = the largest class weight)."""
    x = np.asarray(logits, F64)
    N, C = x.shape
    live = counted(labels, C, ignore)
    y = np.where(live, np.asarray(labels, np.int64), 0)
    wv = np.ones(C) if weight is None else np.asarray(weight, F64).reshape(C)
    w = np.where(live, wv[y], 0.0)
    lse = _lse(x) if N else np.zeros(0)
    nll = np.where(live, lse - x[np.arange(N), y], 0.0)
    sum_w = float(w.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = float(np.float64((w * nll).sum()) / np.float64(sum_w))
        abs_mean = float(np.float64((w * np.abs(nll)).sum()) / np.float64(sum_w))
    d = np.zeros_like(x)
    if sum_w > 0:
        p = np.exp(x - lse[:, None])
        p[np.arange(N), y] -= 1.0
        d = float(grad_out) * (w / sum_w)[:, None] * p
        d[~live] = 0.0
    return dict(loss=loss, sum_w=sum_w, dlogits=d, live=live, abs_mean=abs_mean, w_max=float(wv.max()))


def _softmax_parts32(x):
    """(m, s, e) of the kernels: row maximum, s = sum_c expf(x_c - m) added in class order, e_c = expf(x_c - m)."""
    N, C = x.shape
    m = x.max(1) if C else np.zeros(N, F32)
    e = exp32(x - m[:, None])
    s = np.zeros(N, F32)
    for c in range(C):
        s = (s + e[:, c]).astype(F32)
    return m, s, e


def ce_fp32(logits, labels, weight, ignore, grad_out=1.0):
    """k_ce_fwd / k_ce_finalize / k_ce_bwd in numpy float32.  Returns dict(loss, sum_w, dlogits), all float32."""
    x = _f32(logits)
    N, C = x.shape
    live = counted(labels, C, ignore)
    y = np.where(live, np.asarray(labels, np.int64), 0)
    wv = np.ones(C, F32) if weight is None else _f32(weight).reshape(C)
    w = wv[y]
    m, s, e = _softmax_parts32(x)
    nll = ((m + log32(s)).astype(F32) - x[np.arange(N), y]).astype(F32)
    a = float((w * nll).astype(F32).astype(F64)[live].sum())
    b = float(w.astype(F64)[live].sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss, sum_w = F32(np.float64(a) / np.float64(b)), F32(b)
        k = ((F32(grad_out) * w).astype(F32) / sum_w).astype(F32)
        inv = (F32(1) / s).astype(F32)
        onehot = np.zeros((N, C), F32)
        onehot[np.arange(N), y] = 1
        d = (k[:, None] * ((e * inv[:, None]).astype(F32) - onehot).astype(F32)).astype(F32)
    d[~live] = 0
    return dict(loss=loss, sum_w=sum_w, dlogits=d)


def _unit_error(err, unit, what):
    """max err / unit; where the unit is 0 (no term contributes) the error must be 0."""
    err = np.asarray(err, F64).reshape(-1)
    assert np.isfinite(err).all(), f"{what}: a result is not finite"
    if not unit > 0:
        assert not err.any(), f"{what}: not exactly zero although every term is zero"
        return 0.0
    return float(err.max(initial=0.0) / unit)


def ce_errors(ref, loss, dlogits, grad_out):
    """Errors of a computed (loss, dlogits) against ``ref`` = ce(...): the loss relative to sum w |nll| / sum w, the gradient entries
    relative to |grad_out| * w_max / sum_w.  Nothing counted: the loss must be NaN and the gradient zero."""
    out = {}
    if ref["sum_w"] > 0:
        out["ce_loss"] = _unit_error(abs(float(loss) - ref["loss"]), ref["abs_mean"], "ce loss")
        unit = abs(float(grad_out)) * ref["w_max"] / ref["sum_w"]
    else:
        assert np.isnan(loss), "ce loss: not NaN although no row is counted"
        out["ce_loss"], unit = 0.0, 0.0
    if dlogits is not None:
        out["ce_grad"] = _unit_error(np.abs(np.asarray(dlogits, F64) - ref["dlogits"]), unit, "ce gradient")
    return out


# ------------------------------------------------------------------------------------------------------------------ KL
def kl(pred, tgt, grad_out=1.0):
    """mean_i sum_c q (log q - log p), q = softmax(tgt), p = softmax(pred), and g / N (p - q), in float64.
    Returns dict(loss, dpred, abs_mean = mean_i sum_c q (|log q| + |log p|))."""
    p, t = np.asarray(pred, F64), np.asarray(tgt, F64)
    N, C = p.shape
    if N == 0:
        return dict(loss=float("nan"), dpred=np.zeros_like(p), abs_mean=0.0)
    lp, lq = p - _lse(p)[:, None], t - _lse(t)[:, None]
    q = np.exp(lq)
    return dict(loss=float((q * (lq - lp)).sum(1).mean()), dpred=float(grad_out) / N * (np.exp(lp) - q),
                abs_mean=float((q * (np.abs(lq) + np.abs(lp))).sum(1).mean()))


def kl_fp32(pred, tgt, grad_out=1.0):
    """k_kl_fwd / k_kl_finalize / k_kl_bwd in numpy float32.  Returns dict(loss, dpred)."""
    p, t = _f32(pred), _f32(tgt)
    N, C = p.shape
    mp, sp, ep = _softmax_parts32(p)
    mt, st, et = _softmax_parts32(t)
    lp, lt = (mp + log32(sp)).astype(F32), (mt + log32(st)).astype(F32)
    r = np.zeros(N, F32)
    for c in range(C):
        lq = (t[:, c] - lt).astype(F32)
        r = (r + (exp32(lq) * (lq - (p[:, c] - lp).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = F32(np.float64(r.astype(F64).sum()) / np.float64(N))
        k = F32(grad_out) / F32(N)
    ip, it = (F32(1) / sp).astype(F32), (F32(1) / st).astype(F32)
    d = (k * ((ep * ip[:, None]).astype(F32) - (et * it[:, None]).astype(F32)).astype(F32)).astype(F32)
    return dict(loss=loss, dpred=d)


def kl_errors(ref, loss, dpred, grad_out, N, kind="plain"):
    """The loss relative to mean_i sum_c q (|log q| + |log p|), the gradient entries relative to |grad_out| / N.  The keys carry the
    kind of the case: the pred == tgt and the wide-range losses have bounds of their own."""
    key = {"plain": "kl_loss", "same": "kl_same_loss", "wide": "kl_wide_loss"}[kind]
    out = {}
    if N == 0:
        assert np.isnan(loss)
        return {key: 0.0}
    out[key] = _unit_error(abs(float(loss) - ref["loss"]), ref["abs_mean"], "kl loss")
    if dpred is not None:
        out["kl_wide_grad" if kind == "wide" else "kl_grad"] = _unit_error(np.abs(np.asarray(dpred, F64) - ref["dpred"]),
                                                                           abs(float(grad_out)) / N, "kl gradient")
    return out


# -------------------------------------------------------------------------------------------------------- loss input makers
def _logits(rng, n, c):
    return (3 * rng.standard_normal((n, c))).astype(F32)


def make_labels(rng, n, c, kind):
    """int64 labels.  mix: valid classes with -100, -1, -7, C and C + 5 sprinkled in;  all_ignored: only -100, -1 and C."""
    lab = rng.integers(0, c, size=n).astype(np.int64)
    i = np.arange(n)
    if kind == "all_ignored":
        return np.choose(i % 3, [-100, -1, c]).astype(np.int64)
    assert kind == "mix"
    for mod, at, v in ((9, 4, -100), (31, 7, -1), (43, 17, -7), (37, 11, c), (41, 13, c + 5)):
        lab[i % mod == at] = v
    return lab


def make_weight(rng, c, kind):
    """None; grid: multiples of 1/8 in [1/8, 2]; zero: the same with one class at 0; w6: the list of loss_ce.npz; any other name: a
    shipped list.  Returns float32 values (or None)."""
    if kind is None:
        return None
    if kind in ("grid", "zero"):
        w = rng.integers(1, 17, size=c).astype(F64) / 8
        if kind == "zero":
            w[min(1, c - 1)] = 0.0
        return w.astype(F32)
    if kind == "w6":
        w = np.load(os.path.join(GOLDEN, "loss_ce.npz"))["ce_w6/weight"]
    else:
        w = np.asarray(shipped_class_weights()[kind])
    assert len(w) == c, (kind, c)
    return w.astype(F32)


def make_ce(n, c, seed, weight=None, labels="mix", ignore=-100):
    """Inputs of one cross-entropy case.  A single row is labelled with its least likely class.  From 255 rows on, three rows are extreme: the label's logit 60 below the others, 80 above
    them, and all logits equal.  With no weights or weights on the 1/8 grid the weight sum must be a float32 number (asserted):
    then the float64 partial sums of the kernel are exact in any order and so is their cast."""
    rng = np.random.default_rng(seed)
    x, lab, w = _logits(rng, n, c), make_labels(rng, n, c, labels), make_weight(rng, c, weight)
    if n == 1 and labels == "mix":
        lab[0] = int(x[0].argmin())  # a loss of order 1: the unit of ce_errors must not be tiny against the rounding of the logits
    if n >= 255:
        for r, shift in ((3, -60.0), (34, 80.0), (65, None)):
            y = int(lab[r]) if 0 <= lab[r] < c else 0
            if shift is None:
                x[r] = x[r, 0]
            else:
                x[r, y] += F32(shift)
    ref = ce(x, lab, w, ignore)
    on_grid = w is None or weight in ("grid", "zero")
    if on_grid:
        assert w is None or np.array_equal(w * 8, np.round(w * 8))
        assert float(F32(ref["sum_w"])) == ref["sum_w"], f"the weight sum {ref['sum_w']} is not a float32 number"
    return dict(x=x, labels=lab, weight=w, ignore=ignore, on_grid=on_grid)


def make_kl(n, c, seed, kind="plain"):
    """plain: pred, tgt = 3 * randn (a single row: tgt = -pred);  same: tgt is pred;  wide: uniform in [-60, 60] with, in every row of both, one class at +60 and
    (C >= 2) one at -60: a spread of 120 (asserted), at which float32 target probabilities underflow to 0."""
    rng = np.random.default_rng(seed)
    if kind == "wide":
        both = []
        for _ in range(2):
            v = rng.uniform(-60, 60, size=(n, c)).astype(F32)
            if c >= 2 and n:
                hi = rng.integers(0, c, size=n)
                lo = (hi + rng.integers(1, c, size=n)) % c
                v[np.arange(n), hi], v[np.arange(n), lo] = 60.0, -60.0
                assert ((v.max(1) - v.min(1)) == 120).all()
            both.append(v)
        pred, tgt = both
        if c >= 2 and n:
            assert (exp32(tgt - tgt.max(1, keepdims=True)) == 0).any(), "no target probability underflows"
    else:
        pred = _logits(rng, n, c)
        tgt = pred.copy() if kind == "same" else _logits(rng, n, c)
        if n == 1 and kind == "plain":
            tgt = -pred  # a single row disagrees with its target: a loss of order 1, for the same reason as in make_ce
    return dict(pred=pred, tgt=tgt)


# ----------------------------------------------------------------------------------------------------------- confusion
MARGIN = 1e-4
TIE_KINDS = ("same_pos", "diff_pos", "a_is_b", "swap")


def ensemble64(a, b):
    def sm(v):
        v = np.asarray(v, F64)
        e = np.exp(v - v.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)

    return 0.5 * (sm(a) + sm(b))


def _plant(rng, a, b, r, kind):
    """Makes row r of (a, b) a tie row.  Returns the set of classes among which the ensemble is EXACTLY tied in any precision
    (None: the ensemble is not tied, its winner must clear the margin like any other row's)."""
    c = a.shape[1]
    a[r], b[r] = _logits(rng, 1, c)[0], _logits(rng, 1, c)[0]
    if kind == "swap":
        assert c == 2
        b[r] = a[r, ::-1]  # e0 = (pa0 + pb0) / 2 = (pb1 + pa1) / 2 = e1: addition commutes
        return (0, 1)
    j = np.sort(rng.choice(c, 2, replace=False))
    a[r, j] = np.floor(a[r].max()) + 2  # a small integer above every other logit of the row: two equal maxima
    if kind == "a_is_b":
        b[r] = a[r]
        return tuple(j)
    k = j
    while kind == "diff_pos" and tuple(k) == tuple(j):
        k = np.sort(rng.choice(c, 2, replace=False))
    b[r, k] = np.floor(b[r].max()) + 2
    return tuple(j) if kind == "same_pos" else None


def make_confusion(n, c, seed, labels="mix", tie_rows=4096):
    """Two logit matrices whose three predictions are decided beyond doubt: np.argmax of the float32 logits for a and b (the first
    maximum), and for the ensemble either an exact tie (rows planted among the first ``tie_rows`` rows, every 4th row, kinds in turn)
    or a float64 margin of at least MARGIN between the winner and every class outside the tied set.  Rows that miss the margin are
    drawn again; in the end EVERY row passes (asserted).  Returns dict(a, b, labels, pred [3, n], redrawn = how many rows without
    a planted tie were drawn again, ties = {row: kind})."""
    rng = np.random.default_rng(seed)
    a, b = _logits(rng, n, c), _logits(rng, n, c)
    kinds = [] if c < 2 else ["same_pos", "a_is_b", "swap"] if c == 2 else ["same_pos", "diff_pos", "a_is_b"]
    tie_kind = {r: kinds[(r // 4) % len(kinds)] for r in range(1, min(n, tie_rows), 4)} if kinds else {}
    tied = {r: _plant(rng, a, b, r, k) for r, k in tie_kind.items()}
    redrawn = 0
    for _ in range(100):
        e = ensemble64(a, b)
        in_set = np.zeros((n, c), bool)
        in_set[np.arange(n), e.argmax(1)] = True
        for r, t in tied.items():
            if t is not None:
                in_set[r] = False
                in_set[r, list(t)] = True
        top = np.where(in_set, e, np.inf).min(1) if n else np.zeros(0)
        exact = np.where(in_set, e, -np.inf).max(1) == top if n else np.zeros(0, bool)
        rest = np.where(in_set, -np.inf, e).max(1) if n else np.zeros(0)  # -inf where every class is in the set
        ok = exact & (top - rest >= MARGIN)
        bad = np.flatnonzero(~ok)
        if not len(bad):
            break
        redrawn += sum(1 for r in bad if r not in tie_kind)
        for r in bad:
            if r in tie_kind:
                tied[r] = _plant(rng, a, b, r, tie_kind[r])
            else:
                a[r], b[r] = _logits(rng, 1, c)[0], _logits(rng, 1, c)[0]
    assert n == 0 or ok.all(), "a row is left without a decided ensemble prediction"
    pred = np.stack([a.argmax(1), b.argmax(1), in_set.argmax(1)]) if n else np.zeros((3, 0), np.int64)
    for r, k in tie_kind.items():  # the planted rows are what they claim to be
        assert (a[r] == a[r].max()).sum() == 2 or k == "swap"
        if k != "swap":
            assert (b[r] == b[r].max()).sum() == 2
        if k == "diff_pos":
            assert set(np.flatnonzero(a[r] == a[r].max())) != set(np.flatnonzero(b[r] == b[r].max()))
        if k in ("same_pos", "a_is_b"):
            assert np.array_equal(a[r] == a[r].max(), b[r] == b[r].max())
    return dict(a=a, b=b, labels=make_labels(rng, n, c, labels), pred=pred, redrawn=redrawn, ties=tie_kind)


def confusion(pred, labels, c, ignore):
    """int64 [3, C, C] counts [target][prediction] over the counted rows."""
    live = counted(labels, c, ignore)
    cm = np.zeros((3, c, c), np.int64)
    for k in range(3):
        np.add.at(cm[k], (np.asarray(labels)[live], pred[k][live]), 1)
    return cm


# -------------------------------------------------------------------------------------------------------------- lifting
def lift_keys(rc, counts, H, W):
    """(key int64 [n], err): key = (b * H + row) * W + col with rows / cols clamped into the map; err = 1 if one was outside."""
    rc, counts = np.asarray(rc, np.int64).reshape(-1, 2), np.asarray(counts, np.int64)
    b = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    assert len(b) == len(rc)
    r, c = rc[:, 0], rc[:, 1]
    err = int(((r < 0) | (r >= H) | (c < 0) | (c >= W)).any())
    return (b * H + np.clip(r, 0, H - 1)) * W + np.clip(c, 0, W - 1), err


def lift_sorted(key):
    """(skey, order): the keys ascending and the stable argsort."""
    order = np.argsort(key, kind="stable")
    return key[order], order


def key_pixels(key, H, W):
    key = np.asarray(key, np.int64)
    return key // (H * W), key % (H * W) // W, key % W


def lift_gather(seg, key):
    """seg [B, C, H, W] (any strides) -> [n, C]: the channel vector at every point's pixel."""
    B, C, H, W = seg.shape
    b, r, c = key_pixels(key, H, W)
    return seg[b, :, r, c]


def lift_scatter(dout, key, shape, dtype=F64):
    """(sum [B, C, H, W], touched [B, H, W]): np.add.at of the points' rows onto zeros of ``dtype``, in point order."""
    B, C, H, W = shape
    b, r, c = key_pixels(key, H, W)
    acc = np.zeros((B, H, W, C), dtype)
    np.add.at(acc, (b, r, c), np.asarray(dout, dtype))
    touched = np.zeros((B, H, W), bool)
    touched[b, r, c] = True
    return acc.transpose(0, 3, 1, 2), touched


def make_points(nb, H, W, counts, seed, kind="random"):
    """int64 [n, 2] (row, col) of the points of ``nb`` scenes.  random: uniform over the map;  dup7: only 7 pixels of the map are
    used;  one: a single pixel;  last: random, and the last point of the last non-empty scene sits on the map's last pixel."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    assert len(counts) == nb
    n = int(counts.sum())
    rc = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1).astype(np.int64)
    if kind == "dup7":
        pix = np.stack([rng.integers(0, H, 7), rng.integers(0, W, 7)], 1)
        rc = pix[rng.integers(0, 7, n)].astype(np.int64)
    elif kind == "one":
        rc[:] = (H // 2, W // 3)
    elif kind == "last":
        rc[n - 1] = (H - 1, W - 1)
    else:
        assert kind == "random"
    return rc


def make_scatter_grid(n, C, key, seed):
    """dout on the 1/8 grid in [-2, 2]; asserts that the sum of every run of points of one pixel is exact in float32."""
    rng = np.random.default_rng(seed)
    dout = grid(rng, (n, C), 3)
    pixels, run = np.unique(np.asarray(key, np.int64), return_inverse=True)
    runs = np.zeros((len(pixels), C))
    np.add.at(runs, run.reshape(-1), np.abs(dout))
    assert_exact(runs, 1 / 8, "lift scatter run sum")
    return dout
