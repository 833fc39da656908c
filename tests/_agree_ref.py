"""float64 numpy references of the 2D/3D agreement weights (csrc/pselab.hip mm_pl_agree) and of the two cross-entropy pairs with
row weights (csrc/loss.hip mm_ce2_*_w, mm_ce2s_*_w), a float32 restatement of the weight kernel's formula, and the makers of their
test inputs; shared by tests/test_pl_agreement_host.py, test_gpu_pl_agree.py, test_gpu_ce_rowweight.py and test_gpu_agree_step.py
(no tests here; importing this needs no GPU).

The weighted pairs are built on tests/_loss_ref.py: ``ce`` gives a segment's weight sum and its unweighted gradient rows (a row
weight scales a row, the denominators do not change), ``_lse`` and ``counted`` the per-row terms."""
import numpy as np

from _loss_ref import _lse, _softmax_parts32, ce, counted, exp32, log32

F32, F64 = np.float32, np.float64


def _log_softmax(x):
    return x - _lse(x)[:, None]


def finite_rows(a, b):
    return np.isfinite(np.asarray(a, F64)).all(1) & np.isfinite(np.asarray(b, F64)).all(1)


def divergence(a, b):
    """float64 D [N] = 0.5 * sum_c (p_c - q_c) (lp_c - lq_c) of the rows of a and b; NaN for a row that is not finite."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    ok = finite_rows(a, b)
    d = np.full(a.shape[0], np.nan)
    if ok.any():
        lp, lq = _log_softmax(a[ok]), _log_softmax(b[ok])
        d[ok] = 0.5 * ((np.exp(lp) - np.exp(lq)) * (lp - lq)).sum(1)
    return d


def agreement(a, b, beta):
    """dict(weight [N] (0 for a row that is not finite), mean_weight over all N rows, mean_div over the finite rows, finite)."""
    d = divergence(a, b)
    ok = np.isfinite(d)
    w = np.where(ok, np.exp(-float(beta) * np.where(ok, d, 0.0)), 0.0)
    n = int(ok.sum())
    return dict(weight=w, div=d, mean_weight=float(w.mean()) if len(w) else 0.0, mean_div=float(d[ok].mean()) if n else 0.0, finite=n)


def agreement_fp32(a, b, beta):
    """k_pl_agree's per-row formula in numpy float32 (finite rows only): maxima, exp, sums in class order, log, the terms added in
    class order; exp and log correctly rounded.  Returns (D, w), float32."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    ma, sa, ea = _softmax_parts32(a)
    mb, sb, eb = _softmax_parts32(b)
    la, lb = (ma + log32(sa)).astype(F32), (mb + log32(sb)).astype(F32)
    d = np.zeros(a.shape[0], F32)
    for c in range(a.shape[1]):
        dp = ((ea[:, c] / sa).astype(F32) - (eb[:, c] / sb).astype(F32)).astype(F32)
        dl = ((a[:, c] - la).astype(F32) - (b[:, c] - lb).astype(F32)).astype(F32)
        d = (d + (dp * dl).astype(F32)).astype(F32)
    d = np.maximum((F32(0.5) * d).astype(F32), F32(0))
    return d, exp32((-F32(beta) * d).astype(F32))


# ------------------------------------------------------------------------------------------------- the weighted pairs
def _rw(row_w, n):
    return np.ones(n) if row_w is None else np.asarray(row_w, F64).reshape(n)


def hard_tail(x, labels, weight, row_w, ignore=-100, grad_out=1.0, zero_if_empty=True):
    """The tail of mm_ce2_*_w over its own rows: loss = sum_i row_w_i w[y_i] ce_i / sum_w, sum_w = the class weights of the counted
    rows (the row weights are not in it); gradient rows = row_w_i times those of ``ce``.  Returns dict(loss, sum_w, dlogits)."""
    x = np.asarray(x, F64)
    n, C = x.shape
    base = ce(x, labels, weight, ignore, grad_out)
    rw = _rw(row_w, n)
    if not base["sum_w"] > 0:
        return dict(loss=0.0 if zero_if_empty else float("nan"), sum_w=base["sum_w"], dlogits=np.zeros_like(x))
    live = counted(labels, C, ignore)
    y = np.where(live, np.asarray(labels, np.int64), 0)
    wv = np.ones(C) if weight is None else np.asarray(weight, F64).reshape(C)
    nll = _lse(x) - x[np.arange(n), y]
    loss = float((rw * wv[y] * nll)[live].sum() / base["sum_w"])
    return dict(loss=loss, sum_w=base["sum_w"], dlogits=rw[:, None] * base["dlogits"])


def soft_tail(x, ta, tb, T, thr, row_w, grad_out=1.0, keep=None):
    """The tail of mm_ce2s_*_w over its own rows, gated in float64: a row is kept iff its confidence (largest probability of
    softmax(ta), or of the average with softmax(tb), at temperature 1) is >= thr - a scalar, None, or [C] per arg-max class.
    ``keep`` (bool [n]): the kept rows are given (a caller that takes the gate from the float32 confidences) and thr is ignored.
    loss = (1 / K) sum over the kept rows of row_w_i sum_c q_c (lse - x_c); gradient row grad_out row_w_i / K (softmax(x) - q).
    Returns dict(loss, K, dlogits, keep, dist = the smallest distance of a finite confidence to its threshold)."""
    x, ta = np.asarray(x, F64), np.asarray(ta, F64)
    n, C = x.shape
    rw = _rw(row_w, n)
    out = dict(loss=0.0, K=0, dlogits=np.zeros_like(x), keep=np.zeros(n, bool), dist=float("inf"))
    if n == 0:
        return out
    with np.errstate(invalid="ignore"):
        p = np.exp(_log_softmax(ta))
        if tb is not None:
            p = 0.5 * (p + np.exp(_log_softmax(np.asarray(tb, F64))))
        conf = p.max(1)
        arg = np.where(np.isfinite(conf), np.nan_to_num(p, nan=-1.0).argmax(1), 0)
        bar = np.zeros(n) if thr is None else np.asarray(thr, F64)[arg] if np.ndim(thr) else np.full(n, float(thr))
        given = keep is not None
        keep = np.asarray(keep, bool) if given else conf >= bar  # a NaN confidence compares false
    ok = np.isfinite(conf)
    if thr is not None and not given and ok.any():
        out["dist"] = float(np.abs(conf[ok] - bar[ok]).min())
    K = int(keep.sum())
    out.update(K=K, keep=keep)
    if K == 0:
        return out
    q = np.exp(_log_softmax(ta[keep] / T))
    if tb is not None:
        q = 0.5 * (q + np.exp(_log_softmax(np.asarray(tb, F64)[keep] / T)))
    lsm = _log_softmax(x[keep])
    out["loss"] = float((rw[keep] * -(q * lsm).sum(1)).sum() / K)
    out["dlogits"][keep] = float(grad_out) * (rw[keep] / K)[:, None] * (np.exp(lsm) - q)
    return out


# ------------------------------------------------------------------------------------------------- input makers
def make_pair(n, c, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((n, c))).astype(F32), (scale * rng.standard_normal((n, c))).astype(F32)


def make_row_weights(n, seed):
    """float32 [n] uniform in [0, 1] with exact zeros and exact ones among them (every 5th from 1 and every 7th from 3, if any)."""
    w = np.random.default_rng(seed).uniform(0.0, 1.0, n).astype(F32)
    w[1::5], w[3::7] = 0.0, 1.0
    return w
