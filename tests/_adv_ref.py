"""float64 numpy reference of the point discriminator (include/mm2d3d.h mm_adv_fwd / mm_adv_bwd, losses.adversarial), the error
bounds of its fp32 kernels, and the fixtures that tests/test_adv_host.py and tests/test_gpu_adv.py share.  No tests here; importing
this needs no GPU.

The bounds follow the kernel's summation structure (csrc/adv.hip), with e = 2^-24 and every magnitude taken from the float64
reference.  A dot product of n fp32 fused multiply-adds that starts from a bias is within (n + 1) e sum |terms|; an error E of an
operand enters as |weight| E.  Row by row:
  softmax      p_c = expf(d_c) / s, d_c = x_c - m: the argument's rounding e |d_c| and two ulps of expf, the C-term sum of positive
               terms (C + 1) e, the reciprocal and the product: E_p = (C + 6 + |d_c|) e p_c.
  selfinfo     ln p_c = d_c - logf(s): E_lp = e |d_c| + (C + 2) e + e |ln s| + e |ln p_c|;  u_c = -p_c ln p_c / ln C:
               E_u = (E_p |ln p_c| + p_c E_lp) / ln C + 3 e |u_c|.  (softmax input: E_u = E_p.)
  layer 1      E_z1 = (C + 1) e (|W1| |u| + |b1|) + |W1| E_u;  E_h1 = E_z1 + e |h1| (the product with the slope).
  layer 2      E_z2 = (H + 1) e (|W2| |h1| + |b2|) + |W2| E_h1;  E_h2 = E_z2 + e |h2|.
  logit        E_a = (H + 1) e (|w3| |h2| + |b3|) + |w3| E_h2.
  dloss/da     g = k sigmoid(+-a): the sigmoid moves by at most sigmoid' E_a, its evaluation (expf, sum, quotient) and the products
               with k = 0.5 / n, itself rounded, add 8 e |g|:  E_g = |k| sigmoid (1 - sigmoid) E_a + 8 e |g|.
  backward     e2 = w3 lrelu'(z2) (one rounding), e1 = (W2T e2) lrelu'(z1): E_e1 = ((H + 1) e |W2|T |e2| + |W2|T e |e2|) s1 + e |e1|;
               delta2 = g e2: E_d2 = E_g |e2| + 2 e |delta2|;  delta1 = g e1: E_d1 = E_g |e1| + |g| E_e1 + e |delta1|.
A weight-gradient entry is the sum over the rows of delta[r][j] act[r][k]: fp32 within a tile of at most T = 128 rows, rows
ascending, so (T + 1) e sum_r |delta| |act|; fp64 across tiles and workgroups, which adds nothing at this scale; one rounding of the
fp32 result.  The operands' errors enter as sum_r (E_delta |act| + |delta| E_act).  The bias gradients are the same sums with act = 1.
  gx           da/du = W1T e1: E_eu = (H + 1) e |W1|T |e1| + |W1|T E_e1;  v = da/du * t, t = 1 or -(ln p + 1) / ln C with
               E_t = (E_lp + 2 e |ln p + 1|) / ln C;  w = p v: E_w = E_p |v| + p E_v + e |w|;  S = sum_c w_c: E_S = sum E_w + C e sum |w|;
               inner_k = w_k - p_k S: E_in = E_w + E_p |S| + p E_S + 2 e (|w_k| + p_k |S|);  gx = gG inner:
               E_gx = E_gG (|w_k| + p_k |S|) + |gG| E_in + 2 e |gx|.
The LeakyReLU kink: a unit whose reference pre-activation lies within its rounding margin of 0 may take the other branch on the
GPU, and its slope is then 1 where the reference has 0.2 or the reverse.  Margins: layer 1, m1 = 32 e (|W1| |u| + |b1|); layer 2,
m2 = |W2| m1 + 32 e (|W2| |h1| + |b2|); the logit, ma = |w3| m2 + 32 e (|w3| |h2| + |b3|).  A flagged unit adds 0.8 of its
slope-1 contribution to every element it feeds: 0.8 |g| |w3_j| to delta2[r][j] and 0.8 |w3_j| |W2[j][k]| to e1[r][k] for a layer-2
unit, 0.8 |W2T e2|[r][k] to e1[r][k] for a layer-1 unit; from there they travel like E_d2 and E_e1.  The share of flagged units is a
condition of the fixtures (at most 1e-4 per layer), not a tolerance."""
import functools

import numpy as np

E32 = 2.0 ** -24
SLOPE = 0.2
TILE = 128  # rows of a tile of k_adv_rows: the longest fp32 sum of a weight-gradient entry
MODES = {"softmax": 0, "selfinfo": 1}
KINK_CAP = 1e-4


def param_count(C, H):
    return H * C + H * H + 3 * H + 1


def split(params, C, H):
    """The flat buffer as W1 [H, C], b1 [H], W2 [H, H], b2 [H], w3 [H], b3 (float64)."""
    p = np.asarray(params, np.float64).reshape(-1)
    assert p.size == param_count(C, H)
    o = np.cumsum([0, H * C, H, H * H, H, H, 1])
    return (p[o[0]:o[1]].reshape(H, C), p[o[1]:o[2]], p[o[2]:o[3]].reshape(H, H), p[o[3]:o[4]], p[o[4]:o[5]], float(p[o[5]]))


def join(dW1, db1, dW2, db2, dw3, db3):
    return np.concatenate([np.ravel(dW1), np.ravel(db1), np.ravel(dW2), np.ravel(db2), np.ravel(dw3), np.reshape(db3, 1)])


def counted_rows(x):
    return np.isfinite(np.asarray(x, np.float64)).all(axis=1)


def _softplus(a):
    return np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a)))


def _sigmoid(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def evaluate(x, P, params, H, mode):
    """Everything mm_adv_fwd writes, in float64, and the intermediates the bounds need.  The reference decides every LeakyReLU
    branch itself: ``s1`` / ``s2`` are 1 where its own pre-activation is > 0 and 0.2 elsewhere, and the backward uses them."""
    x = np.asarray(x, np.float64)
    N, C = x.shape
    W1, b1, W2, b2, w3, b3 = split(params, C, H)
    ok = counted_rows(x)
    idx = np.flatnonzero(ok)
    xs = x[idx]
    trg = idx >= P
    n_s, n_t = int((~trg).sum()), int(trg.sum())
    lnC = np.log(C)
    m = xs.max(axis=1, keepdims=True) if idx.size else np.zeros((0, 1))
    d = xs - m
    s = np.exp(d).sum(axis=1, keepdims=True)
    p = np.exp(d) / s
    lp = d - np.log(s)
    if MODES[mode] == 0:
        u, t = p, np.ones_like(p)
    else:
        u = np.where(p > 0, -p * lp / lnC, 0.0)
        t = -(lp + 1.0) / lnC
    z1 = u @ W1.T + b1
    s1 = np.where(z1 > 0, 1.0, SLOPE)
    h1 = z1 * s1
    z2 = h1 @ W2.T + b2
    s2 = np.where(z2 > 0, 1.0, SLOPE)
    h2 = z2 * s2
    a = h2 @ w3 + b3
    sig = _sigmoid(a)
    ks, kt, kg = (0.5 / n_s if n_s else 0.0), (0.5 / n_t if n_t else 0.0), (1.0 / n_t if n_t else 0.0)
    loss_d = ks * _softplus(a[~trg]).sum() + kt * _softplus(-a[trg]).sum()
    loss_g = kg * _softplus(a[trg]).sum()
    g = np.where(trg, -kt * (1.0 - sig), ks * sig)  # dloss_D / da
    gG = np.where(trg, kg * sig, 0.0)  # dloss_G / da
    e2 = w3 * s2
    e1raw = e2 @ W2
    e1 = e1raw * s1
    d2, d1 = g[:, None] * e2, g[:, None] * e1
    dparams = join(d1.T @ u, d1.sum(0), d2.T @ h1, d2.sum(0), g @ h2, g.sum())
    eu = e1 @ W1
    v = eu * t
    w = np.where(p > 0, p * v, 0.0)
    S = w.sum(axis=1, keepdims=True)
    gx = np.zeros((N, C))
    gx[idx] = gG[:, None] * (w - p * S)
    return dict(N=N, C=C, H=H, P=P, mode=mode, idx=idx, trg=trg, count=[n_s, n_t], loss_d=float(loss_d), loss_g=float(loss_g),
                correct=[int((a[~trg] <= 0).sum()), int((a[trg] > 0).sum())], dparams=dparams, gx=gx, a=a, s1=s1, s2=s2, z1=z1, z2=z2,
                inter=dict(d=d, s=s, p=p, lp=lp, u=u, t=t, h1=h1, h2=h2, sig=sig, g=g, gG=gG, e2=e2, e1raw=e1raw, e1=e1, d2=d2, d1=d1,
                           eu=eu, v=v, w=w, S=S, k=(ks, kt, kg)),
                params=(W1, b1, W2, b2, w3, b3))


def margins(ref):
    """The kink margins of the module docstring: ``(m1 [n, H], m2 [n, H], ma [n])`` over the counted rows."""
    W1, b1, W2, b2, w3, b3 = (np.abs(v) for v in ref["params"])
    it = ref["inter"]
    m1 = 32 * E32 * (np.abs(it["u"]) @ W1.T + b1)
    m2 = m1 @ W2.T + 32 * E32 * (np.abs(it["h1"]) @ W2.T + b2)
    ma = m2 @ w3 + 32 * E32 * (np.abs(it["h2"]) @ w3 + b3)
    return m1, m2, ma


def kinks(ref):
    """``(flag1, flag2)``: the units whose reference pre-activation lies within its margin of 0."""
    m1, m2, _ = margins(ref)
    return np.abs(ref["z1"]) <= m1, np.abs(ref["z2"]) <= m2


def kink_shares(ref):
    f1, f2 = kinks(ref)
    return (float(f1.mean()) if f1.size else 0.0, float(f2.mean()) if f2.size else 0.0)


def uncertain_rows(ref):
    """The number of counted rows whose logit lies within its margin of 0: what ``correct`` may differ by."""
    return int((np.abs(ref["a"]) <= margins(ref)[2]).sum())


def bounds(ref):
    """``(bound of dparams [np], bound of gx [N, C])``, element by element, as the module docstring derives them."""
    C, H = ref["C"], ref["H"]
    W1, b1, W2, b2, w3, b3 = (np.abs(v) for v in ref["params"])
    it = {k: (np.abs(v) if isinstance(v, np.ndarray) else v) for k, v in ref["inter"].items()}
    e, lnC = E32, np.log(C)
    p, lp, u, h1, h2, sig = it["p"], it["lp"], it["u"], it["h1"], it["h2"], ref["inter"]["sig"]
    E_p = (C + 6 + it["d"]) * e * p
    E_lp = e * it["d"] + (C + 2) * e + e * np.abs(np.log(ref["inter"]["s"])) + e * lp
    if MODES[ref["mode"]] == 0:
        E_u, E_t = E_p, np.zeros_like(p)
    else:
        E_u = (E_p * lp + p * E_lp) / lnC + 3 * e * u
        E_t = (E_lp + 2 * e * np.abs(ref["inter"]["lp"] + 1.0)) / lnC
    E_h1 = (C + 1) * e * (u @ W1.T + b1) + E_u @ W1.T + e * h1
    E_h2 = (H + 1) * e * (h1 @ W2.T + b2) + E_h1 @ W2.T + e * h2
    E_a = (H + 1) * e * (h2 @ w3 + b3) + E_h2 @ w3
    ks, kt, kg = it["k"]
    trg = ref["trg"]
    g, gG, e2, e1, s1 = it["g"], it["gG"], it["e2"], it["e1"], ref["s1"]
    E_g = np.where(trg, kt, ks) * sig * (1.0 - sig) * E_a + 8 * e * g
    E_gG = np.where(trg, kg, 0.0) * sig * (1.0 - sig) * E_a + 8 * e * gG
    f1, f2 = kinks(ref)
    E_e1 = ((H + 1) * e * (e2 @ W2) + (e * e2) @ W2) * s1 + e * e1
    E_e1 = E_e1 + ((0.8 * f2 * w3) @ W2) * np.where(f1, 1.0, s1) + 0.8 * f1 * it["e1raw"]
    E_d2 = E_g[:, None] * e2 + 2 * e * it["d2"] + 0.8 * f2 * g[:, None] * w3
    E_d1 = E_g[:, None] * e1 + g[:, None] * E_e1 + e * it["d1"]
    T = (TILE + 1) * e

    def outer(delta, E_delta, act, E_act):
        return E_delta.T @ act + delta.T @ E_act + T * (delta.T @ act)

    one, zero = np.ones((g.size, 1)), np.zeros((g.size, 1))
    bp = join(outer(it["d1"], E_d1, u, E_u), outer(it["d1"], E_d1, one, zero), outer(it["d2"], E_d2, h1, E_h1),
              outer(it["d2"], E_d2, one, zero), outer(g[:, None], E_g[:, None], h2, E_h2), outer(g[:, None], E_g[:, None], one, zero))
    bp = bp + np.spacing(np.abs(ref["dparams"]).astype(np.float32)).astype(np.float64)
    E_eu = (H + 1) * e * (e1 @ W1) + E_e1 @ W1
    v, w, S = it["v"], it["w"], it["S"]
    E_v = E_eu * it["t"] + it["eu"] * E_t + e * v
    E_w = E_p * v + p * E_v + e * w
    E_S = E_w.sum(axis=1, keepdims=True) + C * e * w.sum(axis=1, keepdims=True)
    E_in = E_w + E_p * S + p * E_S + 2 * e * (w + p * S)
    bg = np.zeros((ref["N"], C))
    bg[ref["idx"]] = E_gG[:, None] * (w + p * S) + gG[:, None] * E_in
    bg = bg + 2 * e * np.abs(ref["gx"]) + np.spacing(np.abs(ref["gx"]).astype(np.float32)).astype(np.float64)
    return bp, bg


# ---------------------------------------------------------------------------------------------- the fixtures
# (N, P, C, H)
CASES = {
    "0_0_6": (0, 0, 6, 16),
    "1_0_2": (1, 0, 2, 16),  # no source row
    "3_1_2": (3, 1, 2, 16),
    "64_32_2": (64, 32, 2, 16),
    "300_173_11": (300, 173, 11, 64),  # the split inside a tile and off a wave boundary
    "257_120_32": (257, 120, 32, 32),  # widest rows; the LDS pitch C | 1 = 33 stays odd
    "131208_65543_5": (131072 + 129 + 7, 65543, 5, 64),  # 1026 tiles for a grid of 512 workgroups: accumulators carried over
    "300_173_11_holes": (300, 173, 11, 64),  # a NaN row and an infinite row in each segment
}
SEED = 0  # of the parameters; if a seed breaks the kink condition, change the seed, not the cap


def initial(C, H, seed=SEED):
    """The seeded initialisation of mm2d3d_amd/adversarial.py as a float32 numpy vector."""
    import torch

    from mm2d3d_amd.adversarial import initial_parameters

    return initial_parameters(C, H, torch.Generator().manual_seed(seed)).numpy()


def rows(N, C, P, seed, shift=0.5):
    """Seeded fp32 rows 3 * randn, the target's scaled by 1.5 and shifted so that the domains differ."""
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((N, C))
    x[P:] = 1.5 * x[P:] + shift
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """The rows, the parameters and the float64 reference in both modes: computed once, never modified."""
    N, P, C, H = CASES[name]
    x = rows(N, C, P, 7000 + sorted(CASES).index(name.replace("_holes", "")))
    if name.endswith("_holes"):
        x[5] = np.nan
        x[127, 3] = np.inf
        x[P + 1, 0] = -np.inf
        x[N - 1, C - 1] = np.nan
    params = initial(C, H)
    return dict(N=N, P=P, C=C, H=H, x=x, params=params, ref={m: evaluate(x, P, params, H, m) for m in MODES})
