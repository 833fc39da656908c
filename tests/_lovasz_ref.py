"""float64 numpy references of the Lovasz-softmax loss (csrc/lovasz.hip), float32 restatements of its row kernels and of the
evaluation of the Jaccard increments, and the makers of the test inputs; shared by tests/test_lovasz_host.py,
tests/test_gpu_lovasz.py and tests/test_gpu_lovasz_step.py (no tests here).

The loss does not depend on the order inside a group of tied errors (the group telescopes) and moves by at most max |delta e| per
class (the increments of a class sum to at most 1), but a single row's weight does depend on that order.  So nothing here compares
the weights of two different computations of the errors: ``rank_stage`` takes float32 errors AS GIVEN and orders them stably by
the row index, which is what the kernels do with the same values."""
import numpy as np

import _loss_ref as L

F32, F64 = np.float32, np.float64
# the kernel's own constants (asserted against csrc/lovasz.hip by tests/test_lovasz_host.py)
T, ITEMS, SCAN_PER, BITS, PASSES = 256, 4, 8, 10, 3
TILE, SCAN_BLK, RADIX = T * ITEMS, T * SCAN_PER, 1 << BITS
COEF_REL = 4 * 2.0 ** -23  # one int -> float conversion, one product and one division, each at most half an ulp, with headroom


def ntiles(n):
    return -(-max(n, 1) // TILE)


def scan_blocks(n):
    """Workgroups of the offset scan of one pass: RADIX counters per tile, SCAN_BLK counters per workgroup."""
    return -(-RADIX * ntiles(n) // SCAN_BLK)


def ws_bytes(n, c):
    """mm_lovasz_ws_bytes: two (key, row) buffers of C * N words each, the digit counters, their block sums, the foreground count
    per tile, the class counts and the fp64 partials, each rounded up to 256 bytes, plus 256."""
    al = lambda b: -(-b // 256) * 256
    kv = al(4 * c * max(n, 1))
    return 4 * kv + al(4 * c * RADIX * ntiles(n)) + al(4 * c * scan_blocks(n)) + al(4 * c * ntiles(n)) + al(4 * 33) + al(8 * c * ntiles(n)) + 256


# ------------------------------------------------------------------------------------------------------------ float64
def softmax64(x):
    x = np.asarray(x, F64)
    e = np.exp(x - x.max(1, keepdims=True)) if x.size else x
    return e / e.sum(1, keepdims=True) if x.size else e


def errors(logits, labels, ignore=-100):
    """(err [C, N] float64 with -1 in the uncounted rows, live [N])."""
    x = np.asarray(logits, F64)
    N, C = x.shape
    live = L.counted(labels, C, ignore)
    fg = np.asarray(labels)[None, :] == np.arange(C)[:, None]
    err = np.abs(fg - softmax64(x).T)
    err[:, ~live] = -1.0
    return err, live


def definition(e, fg):
    """Weights of the rows of one class by the definition: sort, cumsum, difference of the Jaccard loss (the paper's
    lovasz_grad).  Returns (order, g along the order)."""
    order = np.argsort(-e, kind="stable")
    fs = fg[order].astype(F64)
    gts = fs.sum()
    inter = gts - np.cumsum(fs)
    union = gts + np.cumsum(1.0 - fs)
    jac = 1.0 - inter / union
    if len(jac) > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return order, jac


def closed_form(fg_sorted, fp32=False):
    """The same weights from integers: 1 / U, I / (U (U - 1)), and 1 for the first row of a class without foreground.
    ``fp32``: in the kernel's float32 steps (returned as float64 values)."""
    fg_sorted = np.asarray(fg_sorted, bool)
    n = len(fg_sorted)
    G = int(fg_sorted.sum())
    r = np.arange(1, n + 1, dtype=np.int64)
    if G == 0:
        return (r == 1).astype(F64)
    f = np.cumsum(fg_sorted.astype(np.int64))
    U, I = G + r - f, G - f
    with np.errstate(divide="ignore", invalid="ignore"):
        if fp32:
            bg = I.astype(F32) / (U.astype(F32) * (U - 1).astype(F32)).astype(F32)
            g = np.where(fg_sorted, F32(1) / U.astype(F32), bg).astype(F32)
        else:
            g = np.where(fg_sorted, 1.0 / U, I / (U * (U - 1.0)))
    return g.astype(F64)


def included_classes(labels, C, classes, ignore=-100):
    live = L.counted(labels, C, ignore)
    G = np.array([(np.asarray(labels)[live] == c).sum() for c in range(C)], np.int64)
    inc = (G > 0) if classes == "present" else np.full(C, bool(live.any()))
    return inc, G, live


def _stage(err, labels, classes, ignore, weights):
    err = np.asarray(err)
    C, N = err.shape
    inc, G, live = included_classes(labels, C, classes, ignore)
    idx = np.flatnonzero(live)
    n_inc = int(inc.sum())
    coef = np.zeros((C, N), F64)
    per_class = np.zeros(C, F64)
    lab = np.asarray(labels)[idx]
    for c in np.flatnonzero(inc):
        e, fg = err[c, idx].astype(F64), lab == c
        order, g = weights(e, fg)
        per_class[c] = float((e[order] * g).sum())
        coef[c, idx[order]] = np.where(fg[order], -g, g)
    loss = float(per_class.sum() / n_inc) if n_inc else 0.0
    return dict(loss=loss, coef=coef, n_included=n_inc, counted=int(live.sum()), per_class=per_class, G=G)


def loss_by_definition(err, labels, classes="present", ignore=-100):
    """dict(loss, coef = signed weights NOT yet divided by n_included, n_included, counted, per_class, G)."""
    return _stage(err, labels, classes, ignore, definition)


def rank_stage(err32, labels, classes="present", ignore=-100, fp32=False):
    """The errors as given (float32 values of a kernel or of ``err_fp32``), ordered descending and stably by the row index, weighted
    by the closed form.  Returns dict(loss, coef [C, N] = (fg ? -1 : +1) g / n_included, n_included, counted, ...).
    ``fp32``: g, the division by n_included and the final loss in the kernel's float32 steps."""

    def weights(e, fg):
        order = np.argsort(-e, kind="stable")
        return order, closed_form(fg[order], fp32)

    out = _stage(err32, labels, classes, ignore, weights)
    if out["n_included"]:
        if fp32:
            out["coef"] = (out["coef"].astype(F32) / F32(out["n_included"])).astype(F64)
            out["loss"] = float(F32(out["loss"]))
        else:
            out["coef"] = out["coef"] / out["n_included"]
    return out


def backward(logits, coef, grad_out=1.0):
    """dlogits [N, C] = grad_out * p * (coef^T - sum_c coef_c p_c), float64."""
    p = softmax64(logits)
    ct = np.asarray(coef, F64).T
    return float(grad_out) * p * (ct - (ct * p).sum(1, keepdims=True)) if p.size else np.zeros_like(p)


# ------------------------------------------------------------------------------------------------------------ float32
def _p32(x):
    x = np.asarray(x, F32)
    m, s, e = L._softmax_parts32(x)
    inv = (F32(1) / s).astype(F32)
    return (e * inv[:, None]).astype(F32)


def err_fp32(logits, labels, ignore=-100):
    """k_lv_keys in numpy float32: err [C, N] with -1 in the uncounted rows."""
    x = np.asarray(logits, F32)
    N, C = x.shape
    live = L.counted(labels, C, ignore)
    fg = (np.asarray(labels)[:, None] == np.arange(C)[None, :]).astype(F32)
    err = np.abs((fg - _p32(x)).astype(F32)).T.copy()
    err[:, ~live] = -1
    return err


def bwd_fp32(logits, coef, grad_out=1.0):
    """k_lv_bwd in numpy float32: the dot product added in class order, then g * p * (coef - dot)."""
    x = np.asarray(logits, F32)
    N, C = x.shape
    p, ct = _p32(x), np.asarray(coef, F32).T
    dot = np.zeros(N, F32)
    for c in range(C):
        dot = (dot + (ct[:, c] * p[:, c]).astype(F32)).astype(F32)
    with np.errstate(over="ignore"):
        d = ((F32(grad_out) * p).astype(F32) * (ct - dot[:, None]).astype(F32)).astype(F32)
    d[~ct.any(1)] = 0
    return d


# ------------------------------------------------------------------------------------------------------------- makers
def make(n, c, seed, labels="mix"):
    """3 * randn logits and int64 labels.  labels: mix (valid classes with -100, -1, -7, C, C + 5 sprinkled in), all_ignored,
    absent (mix without class min(1, C - 1); C >= 2), one_class (every counted row has class C - 1).  From 16 rows on and C >= 2:
    rows 3, 10, 17, ... have one logit 40 above the row's maximum, every other one on the row's own class (float32 p is exactly 1:
    runs of e == 0 and e == 1), row 6 has
    all logits equal, and rows 4, 9, 14, ... are copies (logits and label) of the row three before them (exact ties)."""
    rng = np.random.default_rng(seed)
    x = L._logits(rng, n, c)
    lab = L.make_labels(rng, n, c, "all_ignored" if labels == "all_ignored" else "mix")
    live = L.counted(lab, c, -100)
    if labels == "absent":
        assert c >= 2
        a = min(1, c - 1)
        lab[lab == a] = (a + 1) % c
    elif labels == "one_class":
        lab[live] = c - 1
    else:
        assert labels in ("mix", "all_ignored")
    if n >= 16 and c >= 2:
        i = np.arange(n)
        big = i[i % 7 == 3]
        own = L.counted(lab[big], c, -100) & (big % 14 == 3)  # every other one of them on the row's own class: e == 0 there
        k = np.where(own, lab[big], big % c)
        x[big, k] = x[big].max(1) + F32(40)
        x[6] = x[6, 0]
        dup = i[i % 5 == 4]
        x[dup], lab[dup] = x[dup - 3], lab[dup - 3]
    return dict(x=x, labels=lab)
