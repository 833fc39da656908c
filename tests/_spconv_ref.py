"""Rulebook and neighbour-table makers, float64 references and float32 restatements of the sparse convolution engines
(csrc/spconv.hip, csrc/osconv.hip, csrc/ostable.hip) for tests/test_spconv_host.py and tests/test_gpu_spconv_rows.py.  numpy and
torch on the CPU, independent of csrc/meta.hip; importing this needs no GPU.

A rulebook is a dict: nbr[K][n_out] (int32, -1 = absent), the k-major lists src / dst, offsets[K + 1], the row CSR (csr_off over
n_out rows, csr_pos = the rule positions of a row in ascending k).  Weights travel as the ABI takes them: a flat buffer and
(w_kstride, s_ci, s_co, kflip); element (k, ci, co) = W[kk * w_kstride + ci * s_ci + co * s_co], kk = kflip ? K - 1 - k : k."""
import numpy as np
import torch

from _misc2d_ref import FMT, bits16, in_interval, least_allowance, rel_error, round16  # noqa: F401  (re-exported)

F32, F64 = np.float32, np.float64
TILE = 64
MAXK = 32


# --------------------------------------------------------------------------------------------------------------- rulebooks
def derive(nbr):
    """k-major rule lists, bucket offsets and the row CSR of a neighbour table, in plain numpy."""
    nbr = np.ascontiguousarray(nbr, np.int32)
    K, n_out = nbr.shape
    pres = nbr >= 0
    sizes = pres.sum(1)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    dst = np.concatenate([np.flatnonzero(pres[k]) for k in range(K)]).astype(np.int32)
    src = np.concatenate([nbr[k][pres[k]] for k in range(K)]).astype(np.int32)
    pos = np.full((K, n_out), -1, np.int64)
    pos[pres] = np.arange(int(offsets[K]))  # boolean assignment runs k-major, rows ascending: the order of the lists
    pt = pos.T  # [row][k]
    csr_pos = pt[pt >= 0].astype(np.int32)  # rows ascending, k ascending inside a row
    csr_off = np.concatenate([[0], np.cumsum(pres.sum(0))]).astype(np.int32)
    return dict(nbr=nbr, K=K, n_out=n_out, src=src, dst=dst, offsets=offsets, csr_off=csr_off, csr_pos=csr_pos)


def make_rulebook(K, n_out, n_in, sizes, seed, unique):
    """Bucket k gets exactly sizes[k] distinct destination rows and random sources; with ``unique`` a destination row appears in at
    most one bucket.  At least 5 destination rows, row 0 and the last row among them, have no rule at all."""
    sizes = [int(s) for s in sizes]
    assert len(sizes) == K and 0 < K <= MAXK and n_out >= 6
    g = np.random.default_rng(seed)
    bare = np.unique(np.concatenate([[0, n_out - 1], 1 + g.choice(n_out - 2, 3, replace=False)]))
    free = np.setdiff1d(np.arange(n_out), bare)
    nbr = np.full((K, n_out), -1, np.int32)
    if unique:
        assert sum(sizes) <= len(free)
        order, at = g.permutation(free), 0
    for k, s in enumerate(sizes):
        assert s <= len(free)
        if unique:
            rows, at = order[at: at + s], at + s
        else:
            rows = g.choice(free, s, replace=False)
        nbr[k, rows] = g.integers(0, n_in, s)
    rb = derive(nbr)
    rb.update(n_in=n_in, unique=bool(unique))
    check_rulebook(rb, sizes)
    return rb


def check_rulebook(rb, sizes):
    """What a case promises, asserted."""
    K, n_out, off = rb["K"], rb["n_out"], rb["offsets"]
    assert np.diff(off).tolist() == list(sizes), "bucket sizes"
    per_row = (rb["nbr"] >= 0).sum(0)
    assert (per_row == 0).sum() >= 5 and per_row[0] == 0 and per_row[-1] == 0, "rows without a rule"
    if rb["unique"]:
        assert per_row.max(initial=0) <= 1 and len(np.unique(rb["dst"])) == len(rb["dst"]), "unique destinations"
    for k in range(K):
        d = rb["dst"][off[k]: off[k + 1]]
        assert len(np.unique(d)) == len(d), "distinct destinations inside a bucket"
    assert rb["src"].min(initial=0) >= 0 and rb["src"].max(initial=0) < rb["n_in"]
    assert np.array_equal(np.diff(rb["csr_off"]), per_row) and len(rb["csr_pos"]) == off[K]


def make_nbr_mixture(K, n, n_in, seed, one_per_row=False):
    """A neighbour table whose masks are a mixture: about 10 % of the rows have all K offsets, the rest 1 - 4, a few none (row 0
    and the last row among them when n >= 8).  ``one_per_row``: the shape of mm_up_neighbors, one offset per row."""
    g = np.random.default_rng(seed)
    cnt = g.integers(1, 5, n)
    if one_per_row:
        cnt[:] = 1
    else:
        cnt[g.random(n) < 0.1] = K
        if n >= 8:
            cnt[[0, n - 1]] = 0
            cnt[1 + g.choice(n - 2, 3, replace=False)] = 0
    cnt = np.minimum(cnt, K)
    rank = np.argsort(g.random((K, n)), axis=0).argsort(axis=0)  # a random permutation of the offsets per row
    pres = rank < cnt[None, :]
    nbr = np.where(pres, g.integers(0, n_in, (K, n)), -1).astype(np.int32)
    assert np.array_equal((nbr >= 0).sum(0), cnt)
    if not one_per_row and n >= 8:
        assert (cnt == 0).sum() >= 5 and cnt[0] == 0 and cnt[-1] == 0
    rb = derive(nbr)
    rb.update(n_in=n_in, unique=bool(cnt.max(initial=0) <= 1))
    return rb


def swapped(rb, n_in):
    """The same rules with the roles of src and dst exchanged (Deconvolution, the data gradient of Convolution): destinations
    are the old sources, so several rules of a bucket may meet in one row.  Lists and offsets only."""
    return dict(K=rb["K"], n_out=n_in, n_in=rb["n_out"], src=rb["dst"], dst=rb["src"], offsets=rb["offsets"], unique=False)


def os_table(nbr, tile_rows=TILE):
    """The tile table of mm_os_table_build: rows in a stable order of their neighbour bitmask."""
    nbr = np.asarray(nbr, np.int32)
    K, n = nbr.shape
    mask = np.zeros(n, np.uint32)
    for k in range(K):
        mask |= (nbr[k] >= 0).astype(np.uint32) << np.uint32(k)
    perm = np.argsort(mask, kind="stable")
    nt = -(-n // tile_rows)
    npad = nt * tile_rows
    dst = np.full(npad, -1, np.int32)
    dst[:n] = perm
    nbrp = np.full((K, npad), -1, np.int32)
    nbrp[:, :n] = nbr[:, perm]
    ms = np.zeros(npad, np.uint32)
    ms[:n] = mask[perm]
    tmask = np.bitwise_or.reduce(ms.reshape(nt, tile_rows), axis=1).astype(np.uint32) if nt else np.zeros(0, np.uint32)
    return dict(dst=dst, nbrp=nbrp, tmask=tmask, nt=nt, npad=npad)


# ----------------------------------------------------------------------------------------------------------------- weights
def layout(K, Cin, Cout, transposed=False, kflip=0, gap=0):
    """(w_kstride, s_ci, s_co, kflip) of a weight buffer: [K][Cin][Cout] rows, or [K][Cout][Cin] (``transposed``: what the data
    gradient reads), ``gap`` unused floats behind every slab."""
    s_ci, s_co = (1, Cin) if transposed else (Cout, 1)
    return dict(K=K, Cin=Cin, Cout=Cout, w_kstride=Cin * Cout + gap, s_ci=s_ci, s_co=s_co, kflip=int(kflip))


def _windex(lay):
    K, Cin, Cout = lay["K"], lay["Cin"], lay["Cout"]
    k = np.arange(K)
    kk = (K - 1 - k) if lay["kflip"] else k
    return (kk[:, None, None] * lay["w_kstride"] + np.arange(Cin)[None, :, None] * lay["s_ci"] + np.arange(Cout)[None, None, :] * lay["s_co"])


def put_weights(W, lay):
    """The flat buffer that holds the tensor W[K][Cin][Cout] under ``lay``; NaN wherever the layout leaves a hole."""
    flat = np.full(lay["K"] * lay["w_kstride"], np.nan)
    flat[_windex(lay)] = W
    return flat


def get_weights(flat, lay):
    """W[K][Cin][Cout] as the ABI reads it out of the flat buffer."""
    return np.asarray(flat, F64)[_windex(lay)]


# --------------------------------------------------------------------------------------------------------------- operators
def _buckets(rb):
    off = rb["offsets"]
    for k in range(rb["K"]):
        if off[k + 1] > off[k]:
            yield k, rb["src"][off[k]: off[k + 1]], rb["dst"][off[k]: off[k + 1]]


def apply(x, flat, lay, rb, n_out):
    """out[dst] += x[src] . W[k] in float64, and the same sum over absolute values."""
    W = get_weights(flat, lay)
    x = np.asarray(x, F64)
    out, a = np.zeros((n_out, lay["Cout"])), np.zeros((n_out, lay["Cout"]))
    for k, s, d in _buckets(rb):
        v, va = x[s] @ W[k], np.abs(x[s]) @ np.abs(W[k])
        if len(np.unique(d)) == len(d):
            out[d] += v
            a[d] += va
        else:
            np.add.at(out, d, v)
            np.add.at(a, d, va)
    return out, a


def dw(x, dout, rb):
    """dW[k][ci][co] = sum over the rules of bucket k of x[src][ci] * dout[dst][co], and its abs_sum."""
    x, dout = np.asarray(x, F64), np.asarray(dout, F64)
    g, a = np.zeros((rb["K"], x.shape[1], dout.shape[1])), np.zeros((rb["K"], x.shape[1], dout.shape[1]))
    for k, s, d in _buckets(rb):
        g[k], a[k] = x[s].T @ dout[d], np.abs(x[s]).T @ np.abs(dout[d])
    return g, a


# ------------------------------------------------------------------------------------------------------------------ inputs
def grid(shape, seed):
    """Multiples of 1/8 in [-1, 1], zeros included: exact in bf16 and fp16, every product a multiple of 1/64."""
    v = np.random.default_rng(seed).integers(-8, 9, shape).astype(F64) / 8
    return v


def assert_grid_exact(abs_sum):
    """Every fp32 sum of the products, in any order, is exact: 64 * abs_sum stays below 2^24."""
    assert 64 * float(np.max(abs_sum, initial=0.0)) < 2 ** 24


def normal_rows(shape, seed, fmt=None):
    v = np.random.default_rng(seed).standard_normal(shape).astype(F32).astype(F64)
    return round16(v, fmt) if fmt else v


def he_weights(K, Cin, Cout, seed, fmt=None):
    v = (np.random.default_rng(seed).standard_normal((K, Cin, Cout)) * np.sqrt(2.0 / (K * Cin))).astype(F32).astype(F64)
    return round16(v, fmt) if fmt else v


TERM_KINDS = ("xb_wf", "xf_wb", "x2_w2", "full")


def term_values(shape, seed, terms):
    """Numbers sign * 2^e * (1 + t2 + t3) whose split into bf16 terms by repeated rounding is EXACTLY (2^e, 2^e t2, 2^e t3):
    t2 = 2^-9 (1 + j / 128) with j >= 64, t3 = 2^-18 (1 + i / 32) with i >= 16.  ``terms`` = 1: exact in bf16 (1 + j / 128 instead);
    2: t3 = 0 (two terms, a 17-bit significand); 3: all 24 bits.  The second term is at least 1.5 * 2^-9 and the third at least
    1.5 * 2^-18 of the number, so a product that loses one of them is wrong by more than 2^-18 of itself."""
    g = np.random.default_rng(seed)
    sign, e = g.choice([-1.0, 1.0], shape), g.integers(-2, 2, shape).astype(F64)
    if terms == 1:
        m = 1 + g.integers(0, 128, shape) / 128
    else:
        m = 1 + 2.0 ** -9 * (1 + g.integers(64, 128, shape) / 128)
        if terms == 3:
            m = m + 2.0 ** -18 * (1 + g.integers(16, 32, shape) / 32)
    v = sign * 2.0 ** e * m
    assert np.array_equal(v.astype(F32).astype(F64), v)
    t = split_bf16(v.astype(F32), 3)
    assert np.array_equal(t[0].astype(F64) + t[1] + t[2], v) and (t[1] != 0).all() == (terms >= 2) and (t[2] != 0).all() == (terms == 3)
    assert (t[1] == 0).all() == (terms == 1) and (t[2] == 0).all() == (terms < 3)
    return v


def make_terms(kind, rb, Cin, Cout, seed):
    """One nonzero channel per input row (row i: channel i mod Cin) and at most one rule per destination row: every output
    element is a single product x * w.  xb_wf: x exact in bf16, w with all 24 bits (x1w2, x1w3); xf_wb the converse (x2w1, x3w1);
    x2_w2: both two terms (x2w2); full: both 24 bits."""
    assert rb["unique"] and kind in TERM_KINDS
    tx, tw = dict(xb_wf=(1, 3), xf_wb=(3, 1), x2_w2=(2, 2), full=(3, 3))[kind]
    x = np.zeros((rb["n_in"], Cin))
    ch = np.arange(rb["n_in"]) % Cin
    x[np.arange(rb["n_in"]), ch] = term_values(rb["n_in"], seed, tx)
    W = term_values((rb["K"], Cin, Cout), seed + 1, tw)
    return x, W


# ------------------------------------------------------------------------------------------------------------ restatements
def split_bf16(v, nt, fmt="bf16"):
    """v (float32) as nt 16-bit terms by repeated round-to-nearest-even, each as float32 (split8 of csrc/spconv.hip)."""
    r = torch.from_numpy(np.ascontiguousarray(v, dtype=F32))
    out = []
    for _ in range(nt):
        h = r.to(FMT[fmt]).float()
        out.append(h.numpy())
        r = r - h
    return out


# the partial products of mfma_split (csrc/spconv.hip), (weight term, row term), in its order
PAIRS3 = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
PAIRS2 = ((1, 0), (0, 1), (0, 0))
PAIRS1 = ((0, 0),)


def _acc32(acc, prod64):
    """One fp32 accumulation step of a product that the matrix unit forms exactly."""
    return (acc.astype(F64) + prod64).astype(F32)


def _row_sums32(tmp, rb, n_out):
    """The rules of a row added in ascending k in fp32 (k_csr_reduce; the partials of k_osconv4)."""
    out = np.zeros((n_out, tmp.shape[1]), F32)
    cnt, off = np.diff(rb["csr_off"]), rb["csr_off"][:-1]
    for j in range(int(cnt.max(initial=0))):
        rows = np.flatnonzero(cnt > j)
        out[rows] = out[rows] + tmp[rb["csr_pos"][off[rows] + j]]
    return out


def apply_fp32(x, flat, lay, rb, n_out):
    """(a) the exact-fp32 engines: an fma chain over the channels of a rule, then the rules of a row in ascending k."""
    W = get_weights(flat, lay).astype(F32)
    x = np.asarray(x, F32)
    tmp = np.zeros((int(rb["offsets"][-1]), lay["Cout"]), F32)
    off = rb["offsets"]
    for k, s, d in _buckets(rb):
        acc = np.zeros((len(s), lay["Cout"]), F32)
        for c in range(lay["Cin"]):
            acc = _acc32(acc, x[s, c].astype(F64)[:, None] * W[k, c].astype(F64)[None, :])
        tmp[off[k]: off[k + 1]] = acc
    return _row_sums32(tmp, rb, n_out).astype(F64)


def apply_split(x, flat, lay, rb, n_out, pairs=PAIRS3, fmt="bf16", out_fmt=None):
    """(b) the split engines: x and w as bf16 terms, the partial products of ``pairs`` per 32-channel chunk in that order, fp32
    accumulation, rows in ascending k.  (d) 16-bit rows: pairs = PAIRS1 with operands that are 16-bit numbers already and
    ``out_fmt``: the result rounded once."""
    nt = 1 + max(max(p) for p in pairs)
    W = get_weights(flat, lay).astype(F32)
    xt = [t.astype(F64) for t in split_bf16(np.asarray(x, F32), nt, fmt)]
    wt = [t.astype(F64) for t in split_bf16(W, nt, fmt)]
    tmp = np.zeros((int(rb["offsets"][-1]), lay["Cout"]), F32)
    off = rb["offsets"]
    for k, s, d in _buckets(rb):
        acc = np.zeros((len(s), lay["Cout"]), F32)
        for q in range(0, lay["Cin"], 32):
            for a, b in pairs:
                acc = _acc32(acc, xt[b][s, q: q + 32] @ wt[a][k, q: q + 32])
        tmp[off[k]: off[k + 1]] = acc
    out = _row_sums32(tmp, rb, n_out).astype(F64)
    return round16(out, out_fmt) if out_fmt else out


def dw_fp32(x, dout, rb, chunk, kind, pairs=PAIRS3, fmt="bf16", prev=None):
    """(c) the weight gradient: slabs of ``chunk`` rules as make_seg cuts every bucket; inside a slab four waves take the MFMA
    steps in turn (kind "direct": 4 rules per step in fp32; "split": 32 rules per step with the partial products of ``pairs``;
    "generic": one fp32 chain over the slab), the four wave sums are added in wave order in fp32, the slabs of a bucket in float64
    (k_dw_reduce) and the total is rounded once; with ``prev`` (accumulate = 1) one more fp32 add."""
    x32, d32 = np.asarray(x, F32), np.asarray(dout, F32)
    Cin, Cout = x32.shape[1], d32.shape[1]
    out = np.zeros((rb["K"], Cin, Cout), F32)
    if kind == "split":
        nt = 1 + max(max(p) for p in pairs)
        xt = [t.astype(F64) for t in split_bf16(x32, nt, fmt)]
        dt = [t.astype(F64) for t in split_bf16(d32, nt, fmt)]
    step = dict(direct=4, split=32, generic=64)[kind]
    for k, s, d in _buckets(rb):
        total = np.zeros((Cin, Cout), F64)
        for b in range(0, len(s), chunk):
            ss, dd = s[b: b + chunk], d[b: b + chunk]
            n_steps = -(-len(ss) // step)
            waves = 1 if kind == "generic" else 4
            acc = np.zeros((waves, Cin, Cout), F32)
            for i in range(n_steps):
                w = i % waves
                r = slice(i * step, (i + 1) * step)
                if kind == "split":
                    for a, bb in pairs:  # the input rows are the MFMA's A operand here
                        acc[w] = _acc32(acc[w], xt[a][ss[r]].T @ dt[bb][dd[r]])
                else:
                    acc[w] = _acc32(acc[w], x32[ss[r]].astype(F64).T @ d32[dd[r]].astype(F64))
            v = acc[0]
            for w in range(1, waves):
                v = v + acc[w]
            total += v.astype(F64)
        out[k] = total.astype(F32)
    if prev is not None:
        out = np.asarray(prev, F32) + out
    return out.astype(F64)


# ---------------------------------------------------------------------------------------------------- host dispatch, restated
def cdiv(a, b):
    return -(-a // b)


def apply_branch(R, Cin, Cout, K, unique, ld_in, ld_out, in_off=0, out_off=0, mode=0):
    """Which kernels mm_spconv_apply_packed selects (csrc/spconv.hip), from the same arithmetic.  in_off / out_off: floats by which
    the row pointers miss 16-byte alignment.  Returns a dict: kernel, EDGE, cout blocks per workgroup (ncbw), grid.y (nch),
    rules per workgroup (tr), reduce, beyond_preload."""
    edge = bool(Cin % 16 or Cout % 16 or ld_in % 4 or ld_out % 4 or in_off % 4 or out_off % 4)
    nq, ncb = cdiv(Cin, 16), cdiv(Cout, 16)
    nchunk = 1
    if ncb > 8:
        nchunk = next((d for d in range(2, ncb + 1) if ncb % d == 0 and ncb // d <= 8), 0)
    lds_ok = bool(nchunk) and nq * 16 * (ncb // (nchunk or 1)) * 64 <= 150 * 1024
    if not lds_ok:
        return dict(kernel="k_generic_rules" if unique else "k_generic_rows", reduce=None)
    if not unique and Cin <= 4 and Cout <= 32 and K * Cin * Cout * 4 <= 48 * 1024:
        return dict(kernel="k_rows_narrow", reduce=None)
    nt = {0: 3, 1: 0, 2: 2}[mode & 3]
    vec_reduce = Cout % 4 == 0 and ld_out % 4 == 0 and out_off % 4 == 0
    reduce = None if unique else ("k_csr_reduce" if vec_reduce else "k_csr_reduce_scalar")
    if nt and not edge and Cin >= 32 and R > 0:
        nq3 = cdiv(Cin, 32)
        nch = 1
        while nch < ncb and (ncb % nch or ncb // nch > 8 or nq3 * (ncb // nch) * 64 * 16 * nt > 80 * 1024):
            nch += 1
        tr = 256
        while tr > 64 and cdiv(R, tr) * nch < 1024:
            tr >>= 1
        return dict(kernel="k_gather_gemm_s3", terms=nt, ncbw=ncb // nch, nch=nch, tr=tr, reduce=None if unique else "k_csr_reduce",
                    beyond_preload=nq3 > 7, edge=False)
    tr = 256
    while tr > 64 and cdiv(R, tr) * nchunk < 1024:
        tr >>= 1
    while cdiv(R, tr) * nchunk < 512 and (ncb // nchunk) % 2 == 0 and ncb // nchunk >= 2:
        nchunk *= 2
    e2 = edge or (not unique and Cout % 4 != 0)
    if not e2 and 0 < R < 200000 and ncb <= 8:
        return dict(kernel="k_gather_gemm_direct", ncbw=ncb, nch=1, tr=64, reduce=reduce, edge=False)
    return dict(kernel="k_gather_gemm" if R > 0 else None, edge=e2, ncbw=ncb // nchunk, nch=nchunk, tr=tr, reduce=reduce)


def _dw_tile(n):
    return cdiv(n, cdiv(n, 4))


DW_WIDE_MIN_RULES = 200000


def dw_tiles(nci, nco, wide_ok):
    ti, tj = _dw_tile(nci), _dw_tile(nco)
    if not wide_ok or (nci <= 4 and nco <= 4):
        return ti, tj
    best, area = cdiv(nci, ti) * cdiv(nco, tj) * (ti + tj), ti * tj
    for a in range(1, nci + 1):
        i = cdiv(nci, a)
        if i > 6:
            continue
        for b in range(1, nco + 1):
            j = cdiv(nco, b)
            if j > 6 or i * j > 25 or (i <= 4 and j <= 4):
                continue
            cost = a * b * (i + j)
            if cost < best or (cost == best and i * j < area):
                best, area, ti, tj = cost, i * j, i, j
    return ti, tj


def dw_chunk(R, Cin, Cout, wide_ok):
    if Cin % 16 or Cout % 16:
        return 1024
    ti, tj = dw_tiles(Cin // 16, Cout // 16, wide_ok)
    ny = cdiv(Cin // 16, ti) * cdiv(Cout // 16, tj)
    c = cdiv(R, max(1024 // ny, 1))
    return int(min(max(cdiv(c, 16) * 16, 64), 8192))


def dw_branch(R, Cin, Cout, rows, mode):
    """Which kernel, channel tile and slab length dw_partial selects.  rows: 0 = fp32, 1 = bf16, 2 = fp16."""
    mfma_ok = Cin % 16 == 0 and Cout % 16 == 0
    nt = -rows if rows else ({0: 3, 1: 0, 2: 2}[mode & 3] if mfma_ok and Cin >= 16 else 0)
    wide_rules = nt > 0 and R >= DW_WIDE_MIN_RULES
    wide_ok = wide_rules and not (mode & 4)
    chunk = dw_chunk(R, Cin, Cout, wide_rules)  # the slabs do not depend on MM_SPCONV_DW_NARROW
    if not mfma_ok:
        return dict(kernel="k_dw_generic", chunk=chunk, tile=None, wide=False)
    ti, tj = dw_tiles(Cin // 16, Cout // 16, wide_ok)
    if nt < 0:
        kernel = "k_dw_direct_s3" if mode & 8 else "k_dw_tr16"
    else:
        kernel = "k_dw_direct_s3" if nt else "k_dw_direct"
    return dict(kernel=kernel, chunk=chunk, tile=(ti, tj), wide=ti > 4 or tj > 4, terms=abs(nt) if nt < 0 else nt)


def os_branch(n_tiles, Cout, K):
    """The launches of os_apply (csrc/osconv.hip): waves per tile and the (width in blocks, count) of every launch."""
    ncb = Cout // 16
    parts = cdiv(ncb, 3)
    while n_tiles * parts < 1024 and parts < ncb and (ncb + parts) // (parts + 1) >= 2:
        parts += 1
    nw = 4
    if n_tiles * parts < 2048:
        while n_tiles * parts < 2048 and parts < ncb:
            parts += 1
        w = cdiv(ncb, parts)
        nw = (16 if K > 8 else 8) if w == 1 else (8 if w == 2 else 4)
    launches, i, cb = [], 0, 0
    while i < parts:
        w = cdiv(ncb - cb, parts - i)
        cnt, cbn = 1, cb + w
        while i + cnt < parts and cdiv(ncb - cbn, parts - i - cnt) == w:
            cnt, cbn = cnt + 1, cbn + w
        # launch_os4: the 8-wave form exists for one and two blocks, the 16-wave form for one
        eff = nw if (nw == 8 and w <= 2) or (nw == 16 and w == 1) else 4
        launches.append((w, cnt, eff))
        cb, i = cbn, i + cnt
    return dict(nw=nw, parts=parts, launches=launches)
