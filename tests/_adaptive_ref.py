"""A float64 numpy oracle of the self-adaptive per-class pseudo-label thresholds (train_kwargs["pl_threshold"] = "adaptive";
include/mm2d3d.h at mm_pl_adapt has the definition), written from the definition and sharing nothing with the kernels.

Per output o (0: 2D, 1: 3D): tau_o and pt_o[c], all 1 / C at the start, t_o = 0 updates taken.  A batch of teacher logits:
  1. q2 = softmax(l2), q3 = softmax(l3), or with ``ensemble`` both 0.5 * (softmax(l2) + softmax(l3)); p = max q, y = the first
     arg-max;
  2. a row is counted iff p >= 0 (a row with a non-finite probability is not);
  3. if n_o > 0: m_t = m, or with warm-up min(m, (1 + t_o) / (10 + t_o)); tau_o <- m_t tau_o + (1 - m_t) mean p;
     pt_o[c] <- m_t pt_o[c] + (1 - m_t) mean q[c]; t_o += 1;
  4. thr_o[c] = float32((pt_o[c] / max pt_o) * tau_o), always;
  5. a row is kept iff p >= thr_o[y]."""
import numpy as np


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)


def distributions(l2, l3, ensemble):
    """(q of the 2D output, q of the 3D output), float64 [N, C]."""
    s2, s3 = softmax64(l2), softmax64(l3)
    if ensemble:
        e = 0.5 * (s2 + s3)
        return e, e
    return s2, s3


def top(q):
    """(p, y, counted, gap): the largest probability, its first index, whether the row is counted, and the gap to the runner-up
    (inf for one class).  A row with a non-finite probability has no confidence: not counted, p = nan."""
    q = np.asarray(q, dtype=np.float64)
    n = len(q)
    finite = np.isfinite(q).all(1)
    safe = np.where(finite[:, None], q, 0.0)
    y = safe.argmax(1)
    p = safe[np.arange(n), y]
    if q.shape[1] > 1:
        rest = safe.copy()
        rest[np.arange(n), y] = -np.inf
        gap = p - rest.max(1)
    else:
        gap = np.full(n, np.inf)
    p = np.where(finite, p, np.nan)
    return p, y, finite & (p >= 0), gap


class AdaptiveRef:
    def __init__(self, C, momentum=0.999, warmup=False):
        self.C, self.m, self.warmup = C, float(momentum), bool(warmup)
        self.state = np.full((2, 1 + C), 1.0 / C, dtype=np.float64)  # (tau, pt) per output
        self.count = np.zeros(2, dtype=np.int64)

    def thresholds(self):
        pt, tau = self.state[:, 1:], self.state[:, :1]
        return ((pt / pt.max(1, keepdims=True)) * tau).astype(np.float32)

    def update(self, l2, l3, ensemble=False):
        """Steps 1 - 4; returns thr float32 [2, C]."""
        for o, q in enumerate(distributions(l2, l3, ensemble)):
            p, _, counted, _ = top(q)
            n = int(counted.sum())
            if n == 0:
                continue
            t = int(self.count[o])
            m = min(self.m, (1.0 + t) / (10.0 + t)) if self.warmup else self.m
            self.state[o, 0] = m * self.state[o, 0] + (1.0 - m) * p[counted].mean()
            self.state[o, 1:] = m * self.state[o, 1:] + (1.0 - m) * q[counted].mean(0)
            self.count[o] += 1
        return self.thresholds()

    def labels(self, l2, l3, ensemble=False, ignore=-100):
        """Steps 1 - 5: dict(label [2, N] int64, kept [2], threshold float32 [2, C], p [2, N], gap [2, N], margin [2, N]);
        ``margin`` = |p - thr[y]| in float64, ``gap`` = the top-two gap: rows where either is tiny are not decidable in float32."""
        thr = self.update(l2, l3, ensemble)
        labels, ps, gaps, margins = [], [], [], []
        for o, q in enumerate(distributions(l2, l3, ensemble)):
            p, y, counted, gap = top(q)
            t = thr[o].astype(np.float64)[y]
            keep = counted & (np.where(counted, p, -1.0) >= t)
            labels.append(np.where(keep, y, ignore).astype(np.int64))
            ps.append(p), gaps.append(gap), margins.append(np.abs(np.where(counted, p, np.inf) - t))
        labels = np.stack(labels)
        return dict(label=labels, kept=(labels != ignore).sum(1), threshold=thr, p=np.stack(ps), gap=np.stack(gaps),
                    margin=np.stack(margins))
