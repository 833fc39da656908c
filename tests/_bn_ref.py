"""float64 numpy reference of the sparse-row batch norm + (leaky) ReLU (csrc/bn.hip), fp32 restatements of its per-element
arithmetic, the error bounds derived from them and the input makers; shared by tests/test_bn_rows_host.py and
tests/test_gpu_bn_rows.py (no tests here; importing this needs no GPU).

Conventions of the kernels, restated here from include/mm2d3d.h:
  rows [0, Ns) and [Ns, N) are statistics groups 0 and 1 (Ns <= 0 or Ns >= N: one group); save_mean / save_invstd are [G][C];
  momentum is the fraction of the old running value that is KEPT; the running buffers are updated group 0 first, then group 1, with
  the unbiased variance var * Ng / (Ng - 1), or var itself for a group of one row; y = v > 0 ? v : leak * v, so v == 0 takes the
  leak branch, in the forward and in the gradient mask alike; dweight / dbias are the totals over the groups.

The C ABI takes eps, momentum and leak as floats: callers hand the reference float(np.float32(value)), the number the kernel gets.

Bounds (U = 2^-24, the unit roundoff of fp32; none is taken from a kernel's output).  A thread adds at most k rows in fp32 by
recursive summation, everything across threads is fp64 and costs nothing at this scale:
  sum x        |err| <= gamma_k sum|x|,  gamma_k = k U / (1 - k U)            (Higham, Accuracy and Stability, section 4.2)
  sum x^2      |err| <= gamma_k sum x^2                                        (one rounding per fma)
  save_mean    (k + 1) U mean|x|                                               (the sum, then the cast to fp32)
  var          d_var = gamma_k mean x^2 + 2 |mean| gamma_k mean|x| + (gamma_k mean|x|)^2     (E[x^2] - mean^2, clamped at 0)
  save_invstd  the interval 1 / sqrt(var -+ d_var + eps) around the reference, plus U for the cast
  running_*    r' = keep r + (1 - keep) s in fp32: (1 - keep) d_s + U (|keep r| + |(1 - keep) s| + |r'|), chained over the groups
  sum g        d_S1 = gamma_k sum|g| + U |S1|
  sum g xhat   d_S2 = (gamma_k + 3 U) sum|g xhat| + U |mean| invstd sum|g| + U |S2|
               (xhat = fl(fl(x - m32) invstd32): U |mean| invstd from rounding the mean to fp32, 3 U relative from the rest)
  dbias        sum over the groups of d_S1, + U |total| for the fp32 addition of two groups, + U |result| when accumulating
  dweight      the same with d_S2
Every derived bound is multiplied by 1 + 2^-10 for the terms of second order.

y, dx and the eval output are bounded per element by  8 x RESTATE_MAX x scale  + the statistics' own error carried through the
formula, where scale is the sum of the magnitudes that enter the element:
  y     (|x| + |mean|) invstd |w| + |b|
  dx    |w| invstd (|g| + |S1| / Ng + (|x| + |mean|) invstd |S2| / Ng)
RESTATE_MAX is the largest error, in those units, of the fp32 restatements below against float64 over all cases of
test_gpu_bn_rows.py; 8 x covers FMA contraction and another order of operations (the convention of test_gpu_point_rows.py)."""
import zlib

import numpy as np
import torch

from _point_ref import assert_exact, grid

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
GUARD = 1e-4  # no |y_ref| (before the activation, which maps half of them to 0 when leak == 0) below this: the backward recomputes
# the sign of y in another operation order than the forward

# Largest error of the fp32 restatements against float64, in units of the output's scale (see above), over all cases of
# test_gpu_bn_rows.py (CASES of a 256-CU chip) per row type, before the cast to the row type.  Measured with numpy on the CPU by
# tests/test_bn_rows_host.py test_restatement_maxima_are_the_recorded_constants, which repeats the measurement; rounded up.
RESTATE_MAX = {
    "fp32": dict(y=2.4e-07, eval=2.5e-07, dx=3.6e-07),  # measured 2.335e-07, 2.416e-07, 3.527e-07
    "bf16": dict(y=2.1e-07, eval=2.0e-07, dx=2.9e-07),  # measured 2.070e-07, 1.972e-07, 2.882e-07
    "fp16": dict(y=2.2e-07, eval=2.3e-07, dx=3.7e-07),  # measured 2.151e-07, 2.248e-07, 3.680e-07
}

TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
FORMAT = {"bf16": (7, -126), "fp16": (10, -14)}  # explicit mantissa bits, exponent of the smallest normal number


# ------------------------------------------------------------------------------------------------------------------ formats
def quantise(a, dtype):
    """float64 values of ``a`` rounded to the row type (torch's CPU cast: nearest even)."""
    a = np.asarray(a, np.float64)
    if dtype == "fp32":
        return a.astype(np.float32).astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH[dtype]).double().numpy()


def cast32(a32, dtype):
    """A float32 array cast to the row type as the kernels do (one rounding to nearest even), back as float64."""
    return torch.from_numpy(np.ascontiguousarray(a32, np.float32)).to(TORCH[dtype]).double().numpy()


def ulp16(a, dtype):
    """Spacing of the 16-bit format at |a|."""
    bits, emin = FORMAT[dtype]
    _, e = np.frexp(np.abs(np.asarray(a, np.float64)))  # |a| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 1, emin) - bits)


def round16(a, dtype):
    """float64 -> 16-bit format in ONE rounding to nearest even (torch's cast from float64 goes through float32)."""
    a = np.asarray(a, np.float64)
    q = ulp16(a, dtype)
    return np.rint(a / q) * q


# ---------------------------------------------------------------------------------------------------------------- reference
def groups(N, Ns):
    return [(0, N)] if Ns <= 0 or Ns >= N else [(0, Ns), (Ns, N)]


def _params(C, weight, bias):
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64).reshape(C)
    b = np.zeros(C) if bias is None else np.asarray(bias, np.float64).reshape(C)
    return w, b


def bn_ref(x, dy, N, Ns, weight, bias, rm, rv, eps, momentum, leak, accumulate=0, dw0=None, db0=None):
    """Training forward and backward in float64.  ``dy`` None: forward only; ``rm`` None: no running buffers.  Returns a dict:
    y, v (y before the activation), save_mean [G][C], save_invstd [G][C], var [G][C], running_mean, running_var, dx, dweight, dbias,
    the per-group sums S1 = sum g and S2 = sum g xhat [G][C], g (the masked gradient) and xhat, and the condition numbers
    mean_abs_x, mean_sq_x, sum_abs_g, sum_abs_gx, each [G][C]."""
    x = np.asarray(x, np.float64).reshape(N, -1)
    C = x.shape[1]
    w, b = _params(C, weight, bias)
    gs = groups(N, Ns)
    G = len(gs)
    r = dict(y=np.empty_like(x), v=np.empty_like(x), xhat=np.empty_like(x), save_mean=np.zeros((G, C)), save_invstd=np.zeros((G, C)),
             var=np.zeros((G, C)), mean_abs_x=np.zeros((G, C)), mean_sq_x=np.zeros((G, C)), groups=gs)
    if rm is not None:
        r["running_mean"], r["running_var"] = np.array(rm, np.float64).reshape(C), np.array(rv, np.float64).reshape(C)
        r["running_steps"] = []  # (old value, statistic) per group: what the bound of the fp32 update needs
    if dy is not None:
        dy = np.asarray(dy, np.float64).reshape(N, C)
        r.update(dx=np.empty_like(x), g=np.empty_like(x), S1=np.zeros((G, C)), S2=np.zeros((G, C)), sum_abs_g=np.zeros((G, C)),
                 sum_abs_gx=np.zeros((G, C)))
    for gi, (a, e) in enumerate(gs):
        xg, Ng = x[a:e], e - a
        mean = xg.mean(0)
        var = np.square(xg - mean).mean(0)  # two passes: no cancellation in the reference
        invstd = 1.0 / np.sqrt(var + eps)
        xh = (xg - mean) * invstd
        v = xh * w + b
        pos = v > 0
        r["y"][a:e] = np.where(pos, v, leak * v)
        r["xhat"][a:e], r["v"][a:e] = xh, v
        r["save_mean"][gi], r["save_invstd"][gi], r["var"][gi] = mean, invstd, var
        r["mean_abs_x"][gi], r["mean_sq_x"][gi] = np.abs(xg).mean(0), np.square(xg).mean(0)
        if rm is not None:
            unbiased = var * Ng / (Ng - 1) if Ng > 1 else var
            r["running_steps"].append((r["running_mean"].copy(), mean, r["running_var"].copy(), unbiased))
            r["running_mean"] = momentum * r["running_mean"] + (1.0 - momentum) * mean
            r["running_var"] = momentum * r["running_var"] + (1.0 - momentum) * unbiased
        if dy is not None:
            g = np.where(pos, dy[a:e], leak * dy[a:e])
            S1, S2 = g.sum(0), (g * xh).sum(0)
            r["g"][a:e] = g
            r["S1"][gi], r["S2"][gi] = S1, S2
            r["sum_abs_g"][gi], r["sum_abs_gx"][gi] = np.abs(g).sum(0), np.abs(g * xh).sum(0)
            r["dx"][a:e] = w * invstd * (g - S1 / Ng - xh * (S2 / Ng))
    if dy is not None:
        r["dweight"], r["dbias"] = r["S2"].sum(0), r["S1"].sum(0)
        if accumulate:
            r["dweight"] = r["dweight"] + np.asarray(dw0, np.float64)
            r["dbias"] = r["dbias"] + np.asarray(db0, np.float64)
    return r


def pre_activation(x, N, Ns, weight, bias, eps):
    """v = xhat * w + b alone, in float64 (what the guard band is about): the same formulas as bn_ref."""
    x = np.asarray(x, np.float64).reshape(N, -1)
    w, b = _params(x.shape[1], weight, bias)
    v = np.empty_like(x)
    for a, e in groups(N, Ns):
        mean = x[a:e].mean(0)
        np.subtract(x[a:e], mean, out=v[a:e])
        v[a:e] *= w / np.sqrt(np.square(v[a:e]).mean(0) + eps)
        v[a:e] += b
    return v


def bn_eval_ref(x, weight, bias, rm, rv, eps, leak):
    """y of the eval mode, from the running buffers, in float64."""
    x = np.asarray(x, np.float64)
    w, b = _params(x.shape[1], weight, bias)
    v = (x - np.asarray(rm, np.float64)) * (1.0 / np.sqrt(np.asarray(rv, np.float64) + eps)) * w + b
    return np.where(v > 0, v, leak * v)


def fwd_given(x, N, Ns, save_mean, save_invstd, weight, bias, leak):
    """y in float64 from GIVEN statistics [G][C] (the per-element step alone)."""
    x = np.asarray(x, np.float64)
    w, b = _params(x.shape[1], weight, bias)
    y = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        v = (x[a:e] - save_mean[gi]) * save_invstd[gi] * w + b
        y[a:e] = np.where(v > 0, v, leak * v)
    return y


def bwd_given(x, dy, N, Ns, save_mean, save_invstd, weight, bias, leak, S1, S2):
    """dx in float64 from GIVEN statistics and sums [G][C] (the per-element step alone)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    w, b = _params(x.shape[1], weight, bias)
    dx = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        xh = (x[a:e] - save_mean[gi]) * save_invstd[gi]
        g = np.where(xh * w + b > 0, dy[a:e], leak * dy[a:e])
        dx[a:e] = w * save_invstd[gi] * (g - S1[gi] / (e - a) - xh * (S2[gi] / (e - a)))
    return dx


# ------------------------------------------------------------------------------------------------------- fp32 restatements
def _f32(a):
    return np.asarray(a, np.float32)


def _params32(C, weight, bias):
    w, b = _params(C, weight, bias)
    return _f32(w), _f32(b)


def fwd_fp32(x, N, Ns, save_mean, save_invstd, weight, bias, leak):
    """(x - m) * (invstd * w) + b, then the activation, step by step in numpy float32, from statistics rounded to fp32."""
    x = _f32(x)
    w, b = _params32(x.shape[1], weight, bias)
    y = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        m, sc = _f32(save_mean[gi]), _f32(save_invstd[gi]) * w
        v = (x[a:e] - m) * sc + b
        y[a:e] = np.where(v > 0, v, v * np.float32(leak))
    return y


def eval_fp32(x, weight, bias, rm, rv, eps, leak):
    """The eval kernel: invstd = 1 / sqrtf(running_var + eps) in fp32, then the forward arithmetic."""
    x = _f32(x)
    w, b = _params32(x.shape[1], weight, bias)
    invstd = np.float32(1) / np.sqrt(_f32(rv) + np.float32(eps), dtype=np.float32)
    v = (x - _f32(rm)) * (invstd * w) + b
    return np.where(v > 0, v, v * np.float32(leak))


def bwd_fp32(x, dy, N, Ns, save_mean, save_invstd, weight, bias, leak, S1, S2):
    """xh = (x - m) * invstd; yy = xh * w + b; dx = w * invstd * (g - s1 - xh * s2) in numpy float32, with s = fp32(S) * (1 / Ng)."""
    x, dy = _f32(x), _f32(dy)
    w, b = _params32(x.shape[1], weight, bias)
    dx = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        m, inv = _f32(save_mean[gi]), _f32(save_invstd[gi])
        inv_n = np.float32(1) / np.float32(e - a)
        s1, s2 = _f32(S1[gi]) * inv_n, _f32(S2[gi]) * inv_n
        xh = (x[a:e] - m) * inv
        yy = xh * w + b
        g = np.where(yy > 0, dy[a:e], dy[a:e] * np.float32(leak))
        dx[a:e] = (w * inv) * (g - s1 - xh * s2)
    return dx


# ------------------------------------------------------------------------------------------------------- scales and bounds
def scale_y(x, r, N, Ns, weight, bias):
    x = np.asarray(x, np.float64)
    w, b = _params(x.shape[1], weight, bias)
    out = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        out[a:e] = (np.abs(x[a:e]) + np.abs(r["save_mean"][gi])) * (r["save_invstd"][gi] * np.abs(w)) + np.abs(b)
    return out


def scale_eval(x, weight, bias, rm, rv, eps):
    x = np.asarray(x, np.float64)
    w, b = _params(x.shape[1], weight, bias)
    return (np.abs(x) + np.abs(rm)) / np.sqrt(np.asarray(rv, np.float64) + eps) * np.abs(w) + np.abs(b)


def scale_dx(x, r, N, Ns, weight):
    x = np.asarray(x, np.float64)
    w, _ = _params(x.shape[1], weight, None)
    out = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        m, inv, Ng = r["save_mean"][gi], r["save_invstd"][gi], e - a
        out[a:e] = np.abs(w) * inv * (np.abs(r["g"][a:e]) + np.abs(r["S1"][gi]) / Ng + (np.abs(x[a:e]) + np.abs(m)) * inv * np.abs(r["S2"][gi]) / Ng)
    return out


def worst(err, scale):
    """max err / scale; an element whose scale is zero must have no error."""
    err, scale = np.abs(np.asarray(err, np.float64)).reshape(-1), np.asarray(scale, np.float64).reshape(-1)
    assert np.isfinite(err).all(), "a result is not finite"
    assert (err[scale == 0] == 0).all(), "an element whose terms are all zero is not zero"
    live = scale > 0
    return float((err[live] / scale[live]).max()) if live.any() else 0.0


def gamma(k):
    return k * U / (1.0 - k * U)


def stat_bounds(r, k, eps, momentum):
    """Bounds of save_mean, save_invstd [G][C], running_mean, running_var [C] (when the reference has them) for a path whose threads
    add at most k[g] rows of group g in fp32."""
    G, C = r["save_mean"].shape
    out = dict(save_mean=np.zeros((G, C)), save_invstd=np.zeros((G, C)))
    e_rm, e_rv = np.zeros(C), np.zeros(C)
    for gi, (a, e) in enumerate(r["groups"]):
        Ng, gk = e - a, gamma(k[gi])
        mean, var, inv = r["save_mean"][gi], r["var"][gi], r["save_invstd"][gi]
        d_sum = gk * r["mean_abs_x"][gi]
        d_mean = (k[gi] + 1) * U * r["mean_abs_x"][gi]
        d_var = gk * r["mean_sq_x"][gi] + 2 * np.abs(mean) * d_sum + d_sum ** 2
        hi, lo = 1.0 / np.sqrt(np.maximum(var - d_var, 0.0) + eps), 1.0 / np.sqrt(var + d_var + eps)
        out["save_mean"][gi] = d_mean * SLACK
        out["save_invstd"][gi] = (np.maximum(hi - inv, inv - lo) + U * hi) * SLACK
        if "running_mean" in r:
            rm_old, s_m, rv_old, s_v = r["running_steps"][gi]
            d_unb = d_var * (Ng / (Ng - 1) if Ng > 1 else 1.0)
            d_unb = d_unb + U * (np.abs(s_v) + d_unb)  # the cast of the unbiased variance to fp32
            keep, take = momentum, 1.0 - momentum
            rm_new, rv_new = keep * rm_old + take * s_m, keep * rv_old + take * s_v
            e_rm = keep * e_rm + take * d_mean + U * (np.abs(keep * rm_old) + np.abs(take * s_m) + np.abs(rm_new))
            e_rv = keep * e_rv + take * d_unb + U * (np.abs(keep * rv_old) + np.abs(take * s_v) + np.abs(rv_new))
    if "running_mean" in r:
        out["running_mean"], out["running_var"] = e_rm * SLACK, e_rv * SLACK
    return out


def grad_bounds(r, k, accumulate):
    """Bounds of the per-group sums d_S1, d_S2 [G][C] and of dbias, dweight [C]."""
    G, C = r["S1"].shape
    d1, d2 = np.zeros((G, C)), np.zeros((G, C))
    for gi in range(G):
        gk = gamma(k[gi])
        d1[gi] = gk * r["sum_abs_g"][gi] + U * np.abs(r["S1"][gi])
        d2[gi] = ((gk + 3 * U) * r["sum_abs_gx"][gi] + U * np.abs(r["save_mean"][gi]) * r["save_invstd"][gi] * r["sum_abs_g"][gi]
                  + U * np.abs(r["S2"][gi]))
    out = dict(S1=d1 * SLACK, S2=d2 * SLACK)
    for key, d, S in (("dbias", d1, r["S1"]), ("dweight", d2, r["S2"])):
        b = d.sum(0) + (U * np.abs(S.sum(0)) if G > 1 else 0.0)
        if accumulate:
            b = b + U * np.abs(r[key])
        out[key] = b * SLACK
    return out


def y_bound(x, r, N, Ns, weight, bias, sb, restate_max):
    """Per-element bound of y: the fp32 arithmetic, plus the error of the kernel's own statistics carried through the formula."""
    x = np.asarray(x, np.float64)
    w, _ = _params(x.shape[1], weight, bias)
    out = scale_y(x, r, N, Ns, weight, bias)
    out *= 8 * restate_max
    for gi, (a, e) in enumerate(groups(N, Ns)):
        out[a:e] += np.abs(w) * SLACK * (r["save_invstd"][gi] * sb["save_mean"][gi] + np.abs(x[a:e] - r["save_mean"][gi]) * sb["save_invstd"][gi])
    return out


def dx_bound(x, r, N, Ns, weight, gb, restate_max):
    """Per-element bound of dx (backward run from the reference's statistics rounded to fp32): the fp32 arithmetic, plus the error of
    the kernel's own sums carried through the formula."""
    x = np.asarray(x, np.float64)
    w, _ = _params(x.shape[1], weight, None)
    carried = np.empty_like(x)
    for gi, (a, e) in enumerate(groups(N, Ns)):
        carried[a:e] = np.abs(w) * r["save_invstd"][gi] * (gb["S1"][gi] + np.abs(r["xhat"][a:e]) * gb["S2"][gi]) / (e - a)
    return 8 * restate_max * scale_dx(x, r, N, Ns, weight) + carried * SLACK


# ------------------------------------------------------------------------------------------------------------ input makers
def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def make_inputs(name, N, Ns, C, dtype="fp32", kind="normal", weight=True, bias=True, eps=1e-4, leak=0.0):
    """Operands of one case, as float64 arrays holding values of the row type (x, dy) or of fp32 (everything else):
      normal  x ~ N(0, 1) (group 1 of two: 0.5 + 1.7 N(0, 1)), parameters of order 1
      offset  x ~ 100 + N(0, 1): an ill-conditioned variance
      grid    multiples of 1/8 (dy too), every group a power of two rows with mean exactly 0 and some x == 0; weight 1, bias 0
    Guard band (normal, offset): every x whose |y_ref| < GUARD (y before the activation) is drawn again, the reference recomputed, at
    most 10 rounds; none may be left.  grid: y is exactly 0 where x == 0 and at least 1/8 invstd elsewhere."""
    rng = np.random.default_rng(seed_of(name))
    gs = groups(N, Ns)
    d = dict(kind=kind)
    d["weight"] = _f32(1.0 + 0.25 * rng.standard_normal(C)).astype(np.float64) if weight else None
    d["bias"] = _f32(0.5 * rng.standard_normal(C)).astype(np.float64) if bias else None
    d["rm0"] = _f32(0.3 * rng.standard_normal(C)).astype(np.float64)
    d["rv0"] = _f32(0.5 + rng.random(C)).astype(np.float64)
    d["dw0"], d["db0"] = grid(rng, (C,), 3), grid(rng, (C,), 3)
    if kind == "grid":
        assert dtype == "fp32"
        x = np.empty((N, C))
        for a, e in gs:
            Ng = e - a
            assert Ng >= 4 and Ng & (Ng - 1) == 0, "grid groups are powers of two"
            half = grid(rng, (Ng // 2, C), 3)
            half[: max(Ng // 8, 1)] = 0.0
            x[a:e] = np.concatenate([half, -half[rng.permutation(Ng // 2)]], 0)[rng.permutation(Ng)] + 0.0  # no -0.0
            assert (x[a:e].sum(0) == 0).all()
        d["weight"], d["bias"] = (np.ones(C) if weight else None), (np.zeros(C) if bias else None)
        d["x"], d["dy"] = x, grid(rng, (N, C), 3)
        d["exact"] = dict(sum_x=assert_exact(np.abs(x).sum(0), 2.0 ** -3, "sum x"), sum_xx=assert_exact(np.square(x).sum(0), 2.0 ** -6, "sum x^2"),
                          sum_dy=assert_exact(np.abs(d["dy"]).sum(0), 2.0 ** -3, "sum dy"))
        return d

    def draw(shape, gi):
        z = rng.standard_normal(shape, dtype=np.float32).astype(np.float64)
        if kind == "offset":
            z = 100.0 + z
        elif gi == 1:
            z = 0.5 + 1.7 * z
        return quantise(z, dtype)

    x = np.concatenate([draw((e - a, C), gi) for gi, (a, e) in enumerate(gs)], 0) if N else np.zeros((0, C))
    for _ in range(10):
        close = np.abs(pre_activation(x, N, Ns, d["weight"], d["bias"], eps)) < GUARD
        if not close.any():
            break
        for gi, (a, e) in enumerate(gs):
            idx = np.nonzero(close[a:e])
            x[a:e][idx] = draw((len(idx[0]),), gi)
    d["x"] = x
    d["dy"] = quantise(rng.standard_normal((N, C), dtype=np.float32), dtype)
    return d


def guard_ok(d, N, Ns, eps, leak, ref=None):
    """The guard-band property of a case's inputs: (elements inside the band that are not exact zeros of a grid case, smallest |y|
    outside the exact zeros).  ``ref``: the case's reference, when the caller has it already."""
    y = (ref or bn_ref(d["x"], None, N, Ns, d["weight"], d["bias"], None, None, eps, 0.0, leak))["v"]
    inside = np.abs(y) < GUARD
    if d["kind"] == "grid":
        inside &= ~((d["x"] == 0) & (y == 0))
    rest = np.abs(y[np.abs(y) >= GUARD]) if N else np.zeros(0)
    return int(inside.sum()), float(rest.min()) if rest.size else float("inf")
