"""float64 numpy reference of the correlation-alignment losses (include/mm2d3d.h mm_coral_fwd / mm_coral_bwd, losses.coral): Deep
CORAL and Deep LogCORAL of the rows [0, P) against the rows [P, N) of x [N, d].  The forward diagonalises with numpy.linalg.eigh; the
gradient is the analytic Daleckii-Krein form with the equal-eigenvalue rule, not autograd (which divides by zero on repeated
eigenvalues).  No tests here."""
import numpy as np


def counted_rows(x, P=None):
    """Rows whose values are all finite."""
    return np.isfinite(np.asarray(x, np.float64)).all(axis=1)


def _segment(x):
    """n, mean, covariance (zeros where undefined) and the centred counted rows of one segment."""
    d = x.shape[1]
    xc = x[counted_rows(x)]
    n = xc.shape[0]
    m = xc.mean(axis=0) if n > 0 else np.zeros(d)
    c = xc - m
    cov = c.T @ c / (n - 1) if n >= 2 else np.zeros((d, d))
    return n, m, cov, c


def _divided_differences(lam, raised):
    """K of the Daleckii-Krein formula for log: K_ii = 1 / lam_i (0 where the eigenvalue was raised to eps), K_ij = (log lam_i -
    log lam_j) / (lam_i - lam_j) as log1p(t) / (t lo) from the smaller of the two, with the series for tiny t."""
    lo, hi = np.minimum.outer(lam, lam), np.maximum.outer(lam, lam)
    t = (hi - lo) / lo
    small = t < 1e-5
    ts = np.where(small, 1.0, t)
    f = np.where(small, 1.0 - t * (0.5 - t * (1.0 / 3.0 - 0.25 * t)), np.log1p(ts) / ts)
    K = f / lo
    K[np.diag_indices_from(K)] = np.where(raised, 0.0, 1.0 / lam)
    return K


def _eig(cov, eps):
    lam, V = np.linalg.eigh(cov + eps * np.eye(cov.shape[0]))
    raised = lam < eps
    return np.where(raised, eps, lam), V, raised


def evaluate(x, P, mode="log", eps=1e-4):
    """dict(loss, count [2], mean [2, d], cov [2, d, d], aux [2, d, d], grad [N, d]): ``aux`` are the matrices 2 / (n_a - 1) * G_a,
    ``grad`` is dloss/dx (zero rows where a row is not counted)."""
    x = np.asarray(x, np.float64)
    N, d = x.shape
    segs = [_segment(x[:P]), _segment(x[P:])]
    n = [s[0] for s in segs]
    out = dict(count=n, mean=np.stack([s[1] for s in segs]), cov=np.stack([s[2] for s in segs]), loss=0.0, aux=np.zeros((2, d, d)),
               grad=np.zeros((N, d)))
    if min(n) < 2:
        return out
    if mode == "plain":
        D = segs[0][2] - segs[1][2]
        out["loss"] = float((D * D).sum() / (4.0 * d * d))
        G = [D / (2.0 * d * d), -D / (2.0 * d * d)]
    else:
        eig = [_eig(s[2], eps) for s in segs]
        logs = [(V * np.log(lam)) @ V.T for lam, V, _ in eig]
        D = logs[0] - logs[1]
        out["loss"] = float((D * D).sum() / (d * d))
        G = [sign * (2.0 / (d * d)) * V @ ((V.T @ D @ V) * _divided_differences(lam, raised)) @ V.T
             for sign, (lam, V, raised) in zip((1.0, -1.0), eig)]
    for a, (lo, hi) in enumerate(((0, P), (P, N))):
        out["aux"][a] = 2.0 / (n[a] - 1) * G[a]
        rows = np.flatnonzero(counted_rows(x[lo:hi])) + lo
        out["grad"][rows] = segs[a][3] @ out["aux"][a]
    return out


def loss(x, P, mode="log", eps=1e-4):
    return evaluate(x, P, mode, eps)["loss"]


def numeric_gradient(x, P, mode="log", eps=1e-4, h=1e-6):
    """Central differences of ``loss`` in every finite element of a counted row."""
    x = np.asarray(x, np.float64)
    g = np.zeros_like(x)
    for i in np.flatnonzero(counted_rows(x)):
        for j in range(x.shape[1]):
            hi, lo = x.copy(), x.copy()
            hi[i, j] += h
            lo[i, j] -= h
            g[i, j] = (loss(hi, P, mode, eps) - loss(lo, P, mode, eps)) / (2.0 * h)
    return g


def gradient_bound(x, P, ref, margin=4):
    """The fp32 bound of the backward's d-term dot products, from the reference's float64 quantities: (d + margin) * 2^-24 *
    sum_j |x_ij - m_j| |aux_jk| plus one fp32 ulp of the reference value."""
    x = np.asarray(x, np.float64)
    N, d = x.shape
    b = np.zeros((N, d))
    for a, (lo, hi) in enumerate(((0, P), (P, N))):
        rows = np.flatnonzero(counted_rows(x[lo:hi])) + lo
        b[rows] = (d + margin) * 2.0 ** -24 * (np.abs(x[rows] - ref["mean"][a]) @ np.abs(ref["aux"][a]))
    return b + np.spacing(np.abs(ref["grad"]).astype(np.float32)).astype(np.float64)
