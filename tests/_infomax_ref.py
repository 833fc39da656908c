"""float64 numpy reference of the target-domain entropy and diversity losses (include/mm2d3d.h mm_im_fwd / mm_im_bwd,
losses.target_entropy).  No tests here; importing this needs no GPU.

Counted rows: the rows of [P, N) whose C logits are all finite, n of them.  p = softmax(x) per counted row,
    ent  = sum_i H_i / (n ln C),  H_i = -sum_c p_ic log p_ic
    mass = (1 / n) sum_i p_i
    div  = sum_c mass_c (ln mass_c - ln pi_c) / ln C        (a class with mass_c == 0 contributes 0)
n == 0: everything is 0."""
import numpy as np


def _prior(prior, C):
    if prior is None:
        return np.full(C, 1.0 / C)
    pi = np.asarray(prior, np.float64)
    assert pi.shape == (C,) and np.all(pi > 0) and np.all(np.isfinite(pi))
    return pi / pi.sum()


def counted_rows(x, P):
    x = np.asarray(x, np.float64)
    k = np.isfinite(x).all(1)
    k[:P] = False
    return k


def _log_softmax(x):
    d = x - x.max(1, keepdims=True)
    return d - np.log(np.exp(d).sum(1, keepdims=True))


def forward(x, P, prior=None):
    """dict(ent, div, mass [C], count) of the logits ``x`` [N, C] (any float dtype; computed in float64)."""
    x = np.asarray(x, np.float64)
    N, C = x.shape
    k = counted_rows(x, P)
    n = int(k.sum())
    if n == 0:
        return dict(ent=0.0, div=0.0, mass=np.zeros(C), count=0)
    lp = _log_softmax(x[k])
    p = np.exp(lp)
    H = -(p * np.where(p > 0, lp, 0.0)).sum(1)
    mass = p.sum(0) / n
    pi = _prior(prior, C)
    pos = mass > 0
    div = float((mass[pos] * (np.log(mass[pos]) - np.log(pi[pos]))).sum() / np.log(C))
    return dict(ent=float(H.sum() / (n * np.log(C))), div=div, mass=mass, count=n)


def gradients(x, P, prior=None):
    """(d ent / d x, d div / d x), each [N, C]: the analytic formulas of the definition; zero rows where a row is not counted."""
    x = np.asarray(x, np.float64)
    N, C = x.shape
    k = counted_rows(x, P)
    n = int(k.sum())
    de, dd = np.zeros((N, C)), np.zeros((N, C))
    if n == 0:
        return de, dd
    lp = _log_softmax(x[k])
    p = np.exp(lp)
    lp0 = np.where(p > 0, lp, 0.0)
    H = -(p * lp0).sum(1, keepdims=True)
    mass = p.sum(0) / n
    pi = _prior(prior, C)
    g = np.zeros(C)
    pos = mass > 0
    g[pos] = np.log(mass[pos] / pi[pos])
    scale = 1.0 / (n * np.log(C))
    de[k] = -p * (lp0 + H) * scale
    dd[k] = p * (g - (p * g).sum(1, keepdims=True)) * scale
    return de, dd


def numeric_gradients(x, P, prior=None, h=1e-6):
    """Central differences of ``forward`` over the entries of the counted rows (the others do not enter it)."""
    x = np.array(x, np.float64)
    k = counted_rows(x, P)
    de, dd = np.zeros_like(x), np.zeros_like(x)
    for i in np.nonzero(k)[0]:
        for c in range(x.shape[1]):
            keep = x[i, c]
            x[i, c] = keep + h
            a = forward(x, P, prior)
            x[i, c] = keep - h
            b = forward(x, P, prior)
            x[i, c] = keep
            de[i, c] = (a["ent"] - b["ent"]) / (2 * h)
            dd[i, c] = (a["div"] - b["div"]) / (2 * h)
    return de, dd
