"""Float64 references, float32 restatements and input makers of the dense 2D glue kernels (csrc/misc2d.hip: concat, max-pool,
fused heads; mm_colsum_* of csrc/bn2d.hip) for tests/test_misc2d_host.py and tests/test_gpu_misc2d.py.  numpy and torch on the
CPU; importing this needs no GPU.  Maps are NHWC arrays [B, H, W, C]; "fmt" is the 16-bit storage format, "bf16" or "fp16"."""
import numpy as np
import torch

FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
F32 = np.float32


def round16(x, fmt):
    """x rounded to the 16-bit format (nearest even), as float64.  torch converts through float32, so a float64 number within 2^-29
    of a tie may go to the even side; float32 numbers, which is all a kernel rounds, are rounded once.  Monotone either way."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return t.to(FMT[fmt]).double().numpy()


def bits16(x, fmt):
    """The int16 words of x in the 16-bit format (signed zeros and infinities kept)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return t.to(FMT[fmt]).contiguous().view(torch.int16).numpy()


# ------------------------------------------------------------------------------------------------------------------ max-pool
def pooled(n):
    return (n - 1) // 2 + 1


def _taps(n, k):
    """Input coordinate of tap k for every output coordinate, and whether it lies inside [0, n)."""
    i = 2 * np.arange(pooled(n)) - 1 + k
    return np.clip(i, 0, n - 1), (i >= 0) & (i < n)


def maxpool(x):
    """3x3 stride 2 pad 1.  y and idx [B, Ho, Wo, C]; idx = kh * 3 + kw of the first maximum in scan order over the taps INSIDE the
    image (a later tap wins only if it is strictly greater: -0.0 does not beat +0.0, and a window of -inf keeps its first tap)."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    best, idx, seen = None, None, None
    for kh in range(3):
        iy, vy = _taps(H, kh)
        for kw in range(3):
            ix, vx = _taps(W, kw)
            v = x[:, iy][:, :, ix]
            valid = np.broadcast_to((vy[:, None] & vx[None, :])[None, :, :, None], v.shape)
            if best is None:
                best, idx, seen = v.copy(), np.zeros(v.shape, np.uint8), valid.copy()
                continue
            take = valid & (~seen | (v > best))
            best = np.where(take, v, best)
            idx[take] = kh * 3 + kw
            seen = seen | valid
    assert seen.all()  # the centre tap is always inside
    return best, idx


def maxpool_bwd(dy, dy2, idx, H, W):
    """dx[b, iy, ix, c] = sum of dy (+ dy2) over the windows whose winning tap is that pixel: (sum, abs_sum, number of terms).  The
    float64 sums of at most 8 sixteen-bit numbers of comparable size are exact."""
    dy = np.asarray(dy, np.float64)
    B, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == (pooled(H), pooled(W)) and idx.shape == dy.shape
    s, a, n = np.zeros((B, H, W, C)), np.zeros((B, H, W, C)), np.zeros((B, H, W, C), np.int64)
    for kh in range(3):
        iy, vy = _taps(H, kh)
        for kw in range(3):
            ix, vx = _taps(W, kw)
            oy, ox = np.flatnonzero(vy), np.flatnonzero(vx)
            sel = (idx == kh * 3 + kw)[:, oy][:, :, ox]
            dst = (slice(None), iy[oy][:, None], ix[ox][None, :])  # injective for one tap: plain += is right
            for g in (dy,) if dy2 is None else (dy, np.asarray(dy2, np.float64)):
                t = np.where(sel, g[:, oy][:, :, ox], 0.0)
                s[dst] += t
                a[dst] += np.abs(t)
                n[dst] += sel
    return s, a, n


# --------------------------------------------------------------------------------------------------------------------- heads
def _box5(z, add=np.add):
    """Zero-padded 5 x 5 box SUM of [B, h, w, J] in the array's precision: rows left to right, then the five rows top to bottom
    (k_box5_slide; adding the zeros of the padding changes no bit of a sum)."""
    B, h, w, J = z.shape
    p = np.zeros((B, h + 4, w + 4, J), z.dtype)
    p[:, 2:h + 2, 2:w + 2] = z
    hs = np.zeros((B, h + 4, w, J), z.dtype)
    for d in range(5):
        hs = add(hs, p[:, :, d:d + w])
    out = np.zeros((B, h, w, J), z.dtype)
    for d in range(5):
        out = add(out, hs[:, d:d + h])
    return out


def _box5_rowmajor32(z):
    """k_box5 (output counts that are no multiple of 4): ONE float32 accumulator over the 25 taps, row by row."""
    B, h, w, J = z.shape
    p = np.zeros((B, h + 4, w + 4, J), F32)
    p[:, 2:h + 2, 2:w + 2] = z
    s = np.zeros((B, h, w, J), F32)
    for dy in range(5):
        for dx in range(5):
            s = s + p[:, dy:dy + h, dx:dx + w]
    return s


def heads(x, Wj, bias, h, w):
    """out = box5(x[:, :h, :w] @ Wj.T) / 25 + bias (zero padding, count_include_pad) and its abs_sum, [B, h, w, NJ] float64."""
    x, Wj = np.asarray(x, np.float64)[:, :h, :w], np.asarray(Wj, np.float64)
    b = np.zeros(len(Wj)) if bias is None else np.asarray(bias, np.float64)
    return _box5(x @ Wj.T) / 25 + b, _box5(np.abs(x) @ np.abs(Wj).T) / 25 + np.abs(b)


def heads_bwd(x, Wj, dout, h, w, Hp, Wp):
    """dz = box5(dout) / 25; dx = dz @ Wj inside the crop, 0 outside; dW = sum over pixels of dz^T x.  Each with its abs_sum."""
    x, Wj, dout = np.asarray(x, np.float64)[:, :h, :w], np.asarray(Wj, np.float64), np.asarray(dout, np.float64)
    B, C = x.shape[0], x.shape[3]
    dz, az = _box5(dout) / 25, _box5(np.abs(dout)) / 25
    dx, ax = np.zeros((B, Hp, Wp, C)), np.zeros((B, Hp, Wp, C))
    dx[:, :h, :w], ax[:, :h, :w] = dz @ Wj, az @ np.abs(Wj)
    dW = np.einsum("bhwj,bhwc->jc", dz, x, optimize=True)
    aW = np.einsum("bhwj,bhwc->jc", az, np.abs(x), optimize=True)
    return dict(dx=dx, dx_abs=ax, dW=dW, dW_abs=aW)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 numbers is exact in float64; the one float64 rounding of the sum before
    the float32 one can differ from a true fma only at an exact tie of the second rounding."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def split16(Wj, fmt):
    """The two 16-bit terms hi + lo the MFMA projection feeds (k_head_proj_mfma): hi = (h16)w, lo = (h16)(w - (float)hi), as float32.
    torch's CPU conversion keeps fp16 subnormals, as the code claims of the kernel."""
    w = torch.from_numpy(np.ascontiguousarray(Wj, dtype=F32))
    hi = w.to(FMT[fmt]).float()
    lo = (w - hi).to(FMT[fmt]).float()
    return hi.numpy(), lo.numpy()


def is_mfma(C, NJ):
    return C == 64 and NJ <= 16


def _project32(x, Wj, fmt):
    """z [B, h, w, NJ] float32 as the kernels form it.  Generic: one fmaf per channel, in channel order.  MFMA (C = 64, NJ <= 16):
    four 32-channel products lo[0:32], lo[32:64], hi[0:32], hi[32:64], each an exact dot product (16-bit factors) rounded once into
    the float32 accumulator."""
    x = np.asarray(x, F32)
    C, NJ = x.shape[3], len(Wj)
    if is_mfma(C, NJ):
        hi, lo = split16(Wj, fmt)
        acc = np.zeros(x.shape[:3] + (NJ,), F32)
        for wt, c0 in ((lo, 0), (lo, 32), (hi, 0), (hi, 32)):
            acc = (acc.astype(np.float64) + x[..., c0:c0 + 32].astype(np.float64) @ wt[:, c0:c0 + 32].astype(np.float64).T).astype(F32)
        return acc
    Wj = np.asarray(Wj, F32)
    acc = np.zeros(x.shape[:3] + (NJ,), F32)
    for c in range(C):
        acc = _fma32(x[..., c:c + 1], Wj[None, None, None, :, c], acc)
    return acc


def _box32(z, bias):
    """launch_box5 in float32: the sliding kernel for NJ % 4 == 0, else the 25-tap one; s * (1/25) + bias is one fma."""
    NJ = z.shape[3]
    s = _box5(z.astype(F32)) if NJ % 4 == 0 else _box5_rowmajor32(z.astype(F32))
    b = np.zeros(NJ, F32) if bias is None else np.asarray(bias, F32)
    return _fma32(s, np.full_like(s, F32(1.0) / F32(25.0)), np.broadcast_to(b, s.shape))


def heads_fp32(x, Wj, bias, h, w, fmt):
    return _box32(_project32(np.asarray(x)[:, :h, :w], Wj, fmt), bias)


def head_bwd_blocks(total):
    """(blocks, pixels per block) of mm_head_bwd: 128 pixels per block, at most 2048 blocks."""
    nblk = min(max(-(-total // 128), 1), 2048)
    return nblk, -(-total // nblk)


def heads_bwd_fp32(x, Wj, dout, h, w, Hp, Wp):
    """k_head_bwd in float32: dx = fmaf over j in order (not yet rounded to 16 bits); dW: a block of ppb pixels has 16 pixel slots,
    a slot takes every 16th pixel with one fmaf each, the slots of a wave are folded (s0 + s1) + (s2 + s3), the four waves added in
    order, the blocks in float64."""
    x32, W32 = np.asarray(x, F32), np.asarray(Wj, F32)
    B, C, NJ = x32.shape[0], x32.shape[3], len(W32)
    dz = _box32(np.asarray(dout, F32), None)
    o = np.zeros((B, h, w, C), F32)
    for j in range(NJ):
        o = _fma32(dz[..., j:j + 1], W32[None, None, None, j], o)
    dx = np.zeros((B, Hp, Wp, C), F32)
    dx[:, :h, :w] = o
    total = B * Hp * Wp
    nblk, ppb = head_bwd_blocks(total)
    trips = -(-ppb // 16)
    gz, gx = np.zeros((nblk * ppb, NJ), F32), np.zeros((nblk * ppb, C), F32)  # outside the crop: no term (fmaf(0, 0, acc) = acc)
    full = np.zeros((B, Hp, Wp, NJ), F32)
    full[:, :h, :w] = dz
    gz[:total] = full.reshape(total, NJ)
    full = np.zeros((B, Hp, Wp, C), F32)
    full[:, :h, :w] = x32[:, :h, :w]
    gx[:total] = full.reshape(total, C)
    dW = np.zeros((NJ, C))
    step = 256  # blocks at a time (memory)
    for b0 in range(0, nblk, step):
        nb = min(step, nblk - b0)
        pz = np.zeros((nb, trips * 16, NJ), F32)
        px = np.zeros((nb, trips * 16, C), F32)
        pz[:, :ppb] = gz[b0 * ppb:(b0 + nb) * ppb].reshape(nb, ppb, NJ)
        px[:, :ppb] = gx[b0 * ppb:(b0 + nb) * ppb].reshape(nb, ppb, C)
        pz, px = pz.reshape(nb, trips, 16, NJ), px.reshape(nb, trips, 16, C)
        acc = np.zeros((nb, 16, NJ, C), F32)
        for t in range(trips):
            acc = _fma32(pz[:, t, :, :, None], px[:, t, :, None, :], acc)
        a = acc.reshape(nb, 4, 4, NJ, C)  # [block, wave, slot of the wave]
        wave = (a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])
        blk = np.zeros((nb, NJ, C), F32)
        for wv in range(4):
            blk = blk + wave[:, wv]
        dW += blk.astype(np.float64).sum(0)
    return dict(dx=dx, dW=dW.astype(F32))


def rel_error(got, ref, abs_sum):
    """Largest |got - ref| / abs_sum; where abs_sum is 0 the result has no term and must be exactly 0."""
    got, ref, abs_sum = (np.asarray(v, np.float64) for v in (got, ref, abs_sum))
    d = np.abs(got - ref)
    dead = abs_sum == 0
    assert not d[dead].any(), "a result without terms is not exactly zero"
    return float((d[~dead] / abs_sum[~dead]).max(initial=0.0))


def in_interval(got, ref, e, fmt):
    """got within [round16(ref - e), round16(ref + e)], element by element (rounding is monotone: the interval is the whole
    allowance of a 16-bit result whose unrounded value is within e of ref)."""
    got = np.asarray(got, np.float64)
    return (got >= round16(ref - e, fmt)) & (got <= round16(ref + e, fmt))


def least_allowance(got, ref, abs_sum, fmt):
    """The smallest e / abs_sum for which in_interval holds everywhere: how far ref lies outside the set of numbers that round to the
    16-bit result (bounded by the midpoints to its two neighbours), relative to abs_sum.  The figure to report next to a bound."""
    t = torch.from_numpy(np.ascontiguousarray(got, dtype=np.float64)).to(FMT[fmt]).contiguous()
    bits = t.view(torch.int16).to(torch.int32)
    key = torch.where(bits >= 0, bits, -(bits & 0x7FFF))  # ordered like the values

    def value(k):
        return torch.where(k >= 0, k, (-k) | 0x8000).to(torch.int16).view(FMT[fmt]).double().numpy()

    got = t.double().numpy()
    lo, hi = (got + value(key - 1)) / 2, (got + value(key + 1)) / 2
    need = np.maximum(np.maximum(lo - ref, ref - hi), 0.0)
    live = abs_sum > 0
    return float((need[live] / abs_sum[live]).max(initial=0.0))


# -------------------------------------------------------------------------------------------------------------------- makers
MAP_KINDS = ("relu", "negative", "equal", "signed_zero", "neginf", "normal")


def make_map(kind, shape, seed, fmt):
    """A map of 16-bit numbers (float64 array).  Each kind asserts what it promises."""
    g = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "relu":  # coarse, so that equal positive values meet as well
        x = round16(np.maximum(np.round(g.standard_normal(shape) * 4) / 4, 0.0), fmt)
        x = np.abs(x)  # max(-0.0, 0.0): keep +0
        x.reshape(-1)[g.permutation(n)[:-(-3 * n // 10)]] = 0.0  # (a small map may have drawn fewer)
        assert (x == 0).mean() >= 0.3 and (x >= 0).all()
    elif kind == "negative":
        x = round16(-np.abs(g.standard_normal(shape)) - 0.125, fmt)
        assert (x < 0).all()
    elif kind == "equal":
        x = np.full(shape, -1.5)
        assert len(np.unique(x)) == 1
    elif kind == "signed_zero":
        x = np.where(g.random(shape) < 0.5, 0.0, -0.0)
        x.reshape(-1)[g.permutation(n)[:2]] = (0.0, -0.0)
        sign = np.signbit(x)
        assert (x == 0).all() and sign.any() and not sign.all()
    elif kind == "neginf":
        x = round16(g.standard_normal(shape), fmt)
        x[g.random(shape) < 0.6] = -np.inf
        x.reshape(-1)[g.permutation(n)[0]] = -np.inf
        assert np.isneginf(x).any() and not np.isposinf(x).any()
    else:
        assert kind == "normal"
        x = round16(g.standard_normal(shape), fmt)
    assert np.array_equal(bits16(x, fmt), bits16(round16(x, fmt), fmt)) and not np.isnan(x).any()
    return x


def make_grid(shape, seed):
    """Multiples of 1/8 in [-4, 4]: 16-bit numbers in both formats, and any float32 sum of 8 of them is exact (asserted)."""
    x = np.random.default_rng(seed).integers(-32, 33, shape) / 8.0
    assert (x * 8 == np.round(x * 8)).all() and np.abs(x).max(initial=0) <= 4
    assert float(F32(8 * 4.0) + F32(0.125)) == 32.125  # the largest sum of 8 still resolves the grid in float32
    for fmt in FMT:
        assert np.array_equal(round16(x, fmt), x)
    return x


def make_heads(B, Hp, Wp, C, NJ, h, w, seed, fmt, scale=1.0, bias=True):
    """x [B, Hp, Wp, C] of 16-bit numbers, NaN outside the h x w crop; Wj ~ U(-1/8, 1/8) * scale (a 1x1 convolution's initial
    range at 64 inputs), bias, dout ~ N(0, 1): float32 numbers held in float64."""
    g = np.random.default_rng(seed)
    x = round16(g.standard_normal((B, Hp, Wp, C)), fmt)
    x[:, h:], x[:, :, w:] = np.nan, np.nan
    Wj = (g.uniform(-0.125, 0.125, (NJ, C)) * scale).astype(F32)
    assert np.abs(Wj).max() <= 0.125 * scale and (scale == 1.0 or np.abs(Wj).max() < 2e-3)
    bj = g.uniform(-0.5, 0.5, NJ).astype(F32) if bias else None
    dout = g.standard_normal((B, h, w, NJ)).astype(F32)
    assert not np.isnan(x[:, :h, :w]).any() and (h == Hp or np.isnan(x[:, h:]).all()) and (w == Wp or np.isnan(x[:, :, w:]).all())
    return dict(x=x, Wj=Wj.astype(np.float64), bias=None if bj is None else bj.astype(np.float64), dout=dout.astype(np.float64))
