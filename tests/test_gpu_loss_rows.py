"""The row-wise loss and evaluation kernels of csrc/loss.hip, called straight through the C ABI (mm_ce_fwd, mm_ce_bwd, mm_kl_fwd,
mm_kl_bwd, mm_eval_confusion) against the float64 numpy references of tests/_loss_ref.py, and mm_ce_* against mm_ce2_* over one
segment, bit for bit.

Exact, whatever the order of the kernels' sums: the weight sum stats[1] when the class weights are multiples of 1/8 (the makers
assert that the sum is a float32 number), zero gradient rows of rows that are not counted, everything at C = 1, and every count of
the confusion matrices.  The confusion cases decide the ensemble prediction beyond doubt: a float64 margin of 1e-4 (float32
probabilities are within 2.5e-7 of the float64 ones) or a tie that is exact in any precision, which the first class wins.

Pitched operands are views into wider buffers; inputs carry NaN in their padding, outputs a sentinel that must survive.

Loss values and gradients go through expf and logf, so their comparison has a tolerance, and it is not invented.
tests/_loss_ref.py ce_fp32 / kl_fp32 restate the kernels' formulas in numpy float32; their largest error against the float64
reference over ALL the cases of CE_CASES and KL_CASES, in the units of _loss_ref.ce_errors / kl_errors, measured on the CPU
(test_loss_rows_host.py repeats the measurement), is

    quantity       fp32 restatement   bound = 8 x (rounded up)
    ce_loss        6.64e-08           5.4e-07
    ce_grad        4.50e-07           3.6e-06
    kl_loss        1.60e-07           1.3e-06
    kl_grad        5.06e-07           4.1e-06
    kl_same_loss   0                  0
    kl_wide_loss   7.59e-08           6.1e-07
    kl_wide_grad   2.35e-07           1.9e-06

    ce_loss       relative to sum w |nll| / sum w
    ce_grad       per entry, relative to |grad_out| * w_max / sum_w
    kl*_loss      relative to the mean over rows of sum_c q (|log q| + |log p|)
    kl*_grad      per entry, relative to |grad_out| / N

The kernel is allowed 8 x that: another expf and another summation order cost a few ulp each.  Observed on an MI355X: the largest
error of every quantity agrees with the restatement's to the three digits shown, an eighth of its bound.  kl_same is pred == tgt: every term
of the kernel is then (lq - lq) = 0 exactly, so the measured error and the bound are 0.  kl_wide is the case whose logits spread
over 120 within a row, where float32 target probabilities underflow to 0 and their terms contribute 0."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _loss_ref as R
from _gpu_rows import SENTINEL, Ints, Rows, abi as _abi, dev as _dev, vec

pytestmark = pytest.mark.gpu

LOSS_BOUNDS = dict(ce_loss=5.4e-07, ce_grad=3.6e-06, kl_loss=1.3e-06, kl_grad=4.1e-06, kl_same_loss=0.0, kl_wide_loss=6.1e-07, kl_wide_grad=1.9e-06)

LADDER_N = (0, 1, 255, 256, 257, 1024, 1025)  # 1024 rows per block: 1025 is the first row count with two partial sums
LADDER_C = (1, 2, 6, 20, 32)
N_65_PARTIALS = 65537  # 65 partials: the finaliser's 64-stride loop takes a second trip
N_CAPPED = 1048576 + 1025  # 1026 blocks of 1024 rows: past the cap of 1024 partials, the grid-stride loop runs


# --------------------------------------------------------------------------------------------------------------- case tables
def _ce(n, c, **kw):
    d = dict(n=n, c=c, weight=None, labels="mix", ignore=-100, ld=c, ld_d=c, g=1.0, twice=False)
    assert not set(kw) - set(d)
    d.update(kw)
    return d


def _ce_cases():
    t = {}
    for i, (n, c) in enumerate(itertools.product(LADDER_N, LADDER_C)):
        t[f"n{n}_c{c}"] = _ce(n, c, weight="grid" if i % 2 else None)
    t["n65537_c2"] = _ce(N_65_PARTIALS, 2, twice=True)
    t["n65537_c2_weighted_pitched"] = _ce(N_65_PARTIALS, 2, weight="grid", ld=5, ld_d=7, twice=True)
    t["capped_c2"] = _ce(N_CAPPED, 2, weight="grid", twice=True)
    t["capped_c2_unweighted"] = _ce(N_CAPPED, 2)
    for c in LADDER_C:
        t[f"pitched_c{c}"] = _ce(1025, c, weight="grid", ld=c + 3, ld_d=c + 5)
        t[f"pitched_c{c}_unweighted"] = _ce(257, c, ld=c + 3, ld_d=c + 5)
    t["zero_weight_c6"] = _ce(1025, 6, weight="zero")
    t["zero_weight_c2"] = _ce(257, 2, weight="zero", ld=5, ld_d=7)
    t["w6"] = _ce(257, 6, weight="w6")
    for name in ("usa_sing", "day_night", "vkitti_skitti"):  # the three shipped class-weight lists
        t[f"shipped_{name}"] = _ce(1025, 6, weight=name, ld=9, ld_d=11)
    for g in (0.0, -2.5, 65536.0):
        t[f"grad_out_{g:g}"] = _ce(1025, 6, weight="grid", ld=9, ld_d=11, g=g)
        t[f"grad_out_{g:g}_c1"] = _ce(257, 1, g=g)
    t["ignore_is_class_0"] = _ce(1025, 6, weight="grid", ignore=0)
    t["ignore_is_class_1_c2"] = _ce(257, 2, ignore=1, ld=5, ld_d=7)
    t["all_ignored"] = _ce(1025, 6, weight="grid", labels="all_ignored", ld=9, ld_d=11)
    t["all_ignored_n1"] = _ce(1, 6, labels="all_ignored")
    return t


CE_CASES = _ce_cases()


@functools.lru_cache(maxsize=None)
def ce_inputs(name):
    """Inputs of a case (the weight-sum condition asserted by the maker): made once, shared, never modified."""
    c = CE_CASES[name]
    return R.make_ce(c["n"], c["c"], 700 + list(CE_CASES).index(name), c["weight"], c["labels"], c["ignore"])


def _kl(n, c, kind="plain", **kw):
    d = dict(n=n, c=c, kind=kind, ld_p=c, ld_t=c, ld_d=c, g=1.0, twice=False)
    assert not set(kw) - set(d)
    d.update(kw)
    return d


def _kl_cases():
    t = {}
    for n, c in itertools.product(LADDER_N, LADDER_C):
        t[f"n{n}_c{c}"] = _kl(n, c)
    t["n65537_c2"] = _kl(N_65_PARTIALS, 2, twice=True)
    t["capped_c2"] = _kl(N_CAPPED, 2, twice=True)
    for c in LADDER_C:
        t[f"pitched_c{c}"] = _kl(1025, c, ld_p=c + 1, ld_t=c + 3, ld_d=c + 2)
    for g in (0.0, -2.5, 65536.0):
        t[f"grad_out_{g:g}"] = _kl(1025, 6, ld_p=7, ld_t=9, ld_d=8, g=g)
        t[f"grad_out_{g:g}_c1"] = _kl(257, 1, g=g)
    for n, c in ((1, 6), (1025, 2), (1025, 6), (1025, 32), (N_65_PARTIALS, 2)):
        t[f"same_n{n}_c{c}"] = _kl(n, c, "same", ld_p=c + 1, ld_t=c + 3, ld_d=c + 2)
    for n, c in ((1, 6), (1025, 2), (1025, 6), (1025, 20), (1025, 32)):
        t[f"wide_n{n}_c{c}"] = _kl(n, c, "wide", ld_p=c + 1, ld_t=c + 3, ld_d=c + 2, g=-2.5 if c == 20 else 1.0)
    return t


KL_CASES = _kl_cases()


@functools.lru_cache(maxsize=None)
def kl_inputs(name):
    c = KL_CASES[name]
    return R.make_kl(c["n"], c["c"], 900 + list(KL_CASES).index(name), c["kind"])


N_GRID_CAPPED = 2097152 + 2049  # 1026 blocks of 2048 rows: past the grid cap of 1024 blocks


def _cm(n, c, ignore=-100, ld2=None, ld3=None):
    return dict(n=n, c=c, ignore=ignore, ld2=ld2 or c, ld3=ld3 or c)


def _cm_cases():
    t = {}
    for i, (n, c) in enumerate(itertools.product((0, 1, 2047, 2048, 2049), (1, 2, 6, 32))):
        t[f"n{n}_c{c}"] = _cm(n, c, ld2=c + (1 if i % 2 else 0), ld3=c + (2 if i % 2 else 0))
    t["n2049_c6_pitched"] = _cm(2049, 6, ld2=7, ld3=9)
    t["ignore_is_class_1"] = _cm(2049, 6, ignore=1, ld2=7, ld3=9)
    t["ignore_is_class_0_c2"] = _cm(2049, 2, ignore=0)
    t["capped_c2"] = _cm(N_GRID_CAPPED, 2)
    return t


CM_CASES = _cm_cases()


@functools.lru_cache(maxsize=None)
def cm_inputs(name):
    """Two logit matrices and labels of a case; every row's ensemble prediction is decided (asserted by the maker)."""
    c = CM_CASES[name]
    return R.make_confusion(c["n"], c["c"], 1100 + list(CM_CASES).index(name))


# ------------------------------------------------------------------------------------------------------------------ helpers
def _workspace(L):
    return torch.empty(int(L.mm_loss_ws_bytes()), dtype=torch.uint8, device=_dev())


def _check(name, errs):
    print(f"{name}: " + "  ".join(f"{k} {v:.2e} (bound {LOSS_BOUNDS[k]:.1e})" for k, v in errs.items()))
    over = {k: v for k, v in errs.items() if not v <= LOSS_BOUNDS[k]}
    assert not over, f"{name}: {over} exceed {LOSS_BOUNDS}"


def _positive_zero(a):
    return bool((np.ascontiguousarray(a, np.float32).view(np.uint32) == 0).all())


# ------------------------------------------------------------------------------------------------------------ cross entropy
def _run_ce(L, lib, c, x, labels, w, g, ws):
    n, C = c["n"], c["c"]
    stats, dl = vec(None, 2), Rows(None, n, C, c["ld_d"], 4, fill=SENTINEL)
    lib.check(L.mm_ce_fwd(x.ptr, c["ld"], labels.ptr, w.ptr if w else None, n, C, c["ignore"], stats.ptr, ws.data_ptr(), ws.numel(),
                          lib.stream()), "ce_fwd")
    lib.check(L.mm_ce_bwd(x.ptr, c["ld"], labels.ptr, w.ptr if w else None, n, C, c["ignore"], stats.ptr, g.ptr, dl.ptr, c["ld_d"],
                          lib.stream()), "ce_bwd")
    torch.cuda.synchronize()
    return stats, dl


@pytest.mark.parametrize("name", list(CE_CASES))
def test_cross_entropy_forward_and_backward_against_float64(name):
    c, d = CE_CASES[name], ce_inputs(name)
    L, lib = _abi()
    n, C = c["n"], c["c"]
    x, labels = Rows(d["x"], n, C, c["ld"], 4), Ints(d["labels"], dtype=torch.int64)
    w = vec(d["weight"], fill=float("nan")) if d["weight"] is not None else None
    g, ws = vec([c["g"]], fill=float("nan")), _workspace(L)  # grad_out: a scalar on the device
    stats, dl = _run_ce(L, lib, c, x, labels, w, g, ws)
    ref = R.ce(d["x"], d["labels"], d["weight"], c["ignore"], c["g"])
    st, got = stats.get32()[0], dl.get32()
    assert stats.padding_untouched() and dl.padding_untouched()
    # the weight sum: exact on the 1/8 grid, else one conversion of an (all but) exact float64 sum
    if d["on_grid"]:
        assert float(st[1]) == ref["sum_w"], (float(st[1]), ref["sum_w"])
    else:
        assert abs(float(st[1]) - ref["sum_w"]) <= float(np.spacing(np.float32(ref["sum_w"])))
    live = ref["live"]
    if n == 0:
        assert dl.untouched(), "mm_ce_bwd wrote although N = 0"
    assert _positive_zero(got[~live]), "a row that is not counted has a gradient other than 0.f"
    if not live.any():
        assert np.isnan(st[0]) and st[1] == 0 and _positive_zero(got)
    if C == 1:
        assert not got.any(), "C = 1: the gradient is not zero"
        assert not live.any() or st[0] == 0, "C = 1: the loss is not zero"
    _check(name, R.ce_errors(ref, st[0], got.astype(np.float64), c["g"]))
    if c["twice"]:
        stats2, dl2 = _run_ce(L, lib, c, x, labels, w, g, ws)
        assert torch.equal(stats2.flat.view(torch.int32), stats.flat.view(torch.int32)), "two runs differ in the loss bits"
        assert torch.equal(dl2.flat.view(torch.int32), dl.flat.view(torch.int32)), "two runs differ in the gradient bits"


@pytest.mark.parametrize("name", list(CE_CASES))
def test_cross_entropy_is_the_two_segment_entry_with_one_segment_bit_for_bit(name):
    """mm_ce_* against mm_ce2_* with P = N, the tail unlabelled and zero_if_empty = 0: k_ce_*<1> and k_ce_*<2> of csrc/loss.hip are
    one template, so loss, weight sum and every gradient word are the same bits (NaN of the all-ignored cases included: int32
    views), and the tail reports loss 0 over weight 0."""
    c, d = CE_CASES[name], ce_inputs(name)
    L, lib = _abi()
    n, C = c["n"], c["c"]
    x = Rows(d["x"], n, C, c["ld"], 4)
    # N = 0: an address all the same (no address = "unlabelled" to mm_ce2_*), one label that no row reads, as losses._labels
    labels = Ints(d["labels"] if n else np.array([c["ignore"]]), dtype=torch.int64)
    w = vec(d["weight"], fill=float("nan")) if d["weight"] is not None else None
    g, ws = vec([c["g"]], fill=float("nan")), _workspace(L)
    stats, dl = _run_ce(L, lib, c, x, labels, w, g, ws)
    ws2 = torch.empty(int(L.mm_ce2_ws_bytes()), dtype=torch.uint8, device=_dev())
    stats2, dl2 = vec(None, 4), Rows(None, n, C, c["ld_d"], 4, fill=SENTINEL)
    lib.check(L.mm_ce2_fwd(x.ptr, c["ld"], n, n, C, labels.ptr, w.ptr if w else None, None, None, c["ignore"], 0, stats2.ptr,
                           ws2.data_ptr(), ws2.numel(), lib.stream()), "ce2_fwd")
    lib.check(L.mm_ce2_bwd(x.ptr, c["ld"], n, n, C, labels.ptr, w.ptr if w else None, None, None, c["ignore"], stats2.ptr, g.ptr, dl2.ptr,
                           c["ld_d"], lib.stream()), "ce2_bwd")
    torch.cuda.synchronize()
    assert stats2.padding_untouched() and dl2.padding_untouched()
    s1, s2 = stats.bits()[0], stats2.bits()[0]
    assert np.array_equal(s2[:2], s1), f"{name}: (loss, sum_w) bits {s2[:2]} of mm_ce2_fwd, {s1} of mm_ce_fwd"
    tail = stats2.get32()[0, 2:]
    assert (tail == 0.0).all(), f"{name}: the unlabelled tail reports (loss, sum_w) = {tail}, not (0.0, 0.0)"
    assert torch.equal(dl2.flat.view(torch.int32), dl.flat.view(torch.int32)), f"{name}: the gradients of mm_ce2_bwd and mm_ce_bwd differ"


# ----------------------------------------------------------------------------------------------------------------------- KL
def _run_kl(L, lib, c, p, t, g, ws):
    n, C = c["n"], c["c"]
    loss, dp = vec(None, 1), Rows(None, n, C, c["ld_d"], 4, fill=SENTINEL)
    lib.check(L.mm_kl_fwd(p.ptr, c["ld_p"], t.ptr, c["ld_t"], n, C, loss.ptr, ws.data_ptr(), ws.numel(), lib.stream()), "kl_fwd")
    lib.check(L.mm_kl_bwd(p.ptr, c["ld_p"], t.ptr, c["ld_t"], n, C, g.ptr, dp.ptr, c["ld_d"], lib.stream()), "kl_bwd")
    torch.cuda.synchronize()
    return loss, dp


@pytest.mark.parametrize("name", list(KL_CASES))
def test_kl_forward_and_backward_against_float64(name):
    """N = 0: the forward divides the empty sum by N and writes 0 / 0 = NaN, which is what the caller (losses._KLFn, which passes
    an empty batch through) returns and what the batch mean of torch's kl_div gives for an empty batch; the backward returns MM_OK
    and writes nothing.  That is the contract asserted here."""
    c, d = KL_CASES[name], kl_inputs(name)
    L, lib = _abi()
    n, C = c["n"], c["c"]
    p, t = Rows(d["pred"], n, C, c["ld_p"], 4), Rows(d["tgt"], n, C, c["ld_t"], 4)
    g, ws = vec([c["g"]], fill=float("nan")), _workspace(L)
    loss, dp = _run_kl(L, lib, c, p, t, g, ws)
    assert loss.padding_untouched() and dp.padding_untouched()
    v, got = loss.get32()[0, 0], dp.get32()
    if n == 0:
        assert np.isnan(v) and dp.untouched()
    else:
        assert np.isfinite(v) and np.isfinite(got).all()
    if C == 1 and n:
        assert v == 0 and not got.any(), "C = 1: loss or gradient is not zero"
    _check(name, R.kl_errors(R.kl(d["pred"], d["tgt"], c["g"]), v, got.astype(np.float64), c["g"], n, c["kind"]))
    if c["twice"]:
        loss2, dp2 = _run_kl(L, lib, c, p, t, g, ws)
        assert torch.equal(loss2.flat.view(torch.int32), loss.flat.view(torch.int32)), "two runs differ in the loss bits"
        assert torch.equal(dp2.flat.view(torch.int32), dp.flat.view(torch.int32)), "two runs differ in the gradient bits"


# ---------------------------------------------------------------------------------------------------------------- confusion
@pytest.mark.parametrize("name", list(CM_CASES))
def test_confusion_counts_equal_the_reference_and_accumulate(name):
    c, d = CM_CASES[name], cm_inputs(name)
    L, lib = _abi()
    n, C, ld2, ld3 = c["n"], c["c"], c["ld2"], c["ld3"]
    a, b, labels = Rows(d["a"], n, C, ld2, 4), Rows(d["b"], n, C, ld3, 4), Ints(d["labels"], dtype=torch.int64)
    before = (np.arange(3 * C * C, dtype=np.int64) * 7 + 3) % 1000 + (np.int64(1) << 33)  # counts past 32 bits are kept
    want = before + R.confusion(d["pred"], d["labels"], C, c["ignore"]).reshape(-1)
    whole, halves = Ints(before, dtype=torch.int64), Ints(before, dtype=torch.int64)
    lib.check(L.mm_eval_confusion(a.ptr, ld2, b.ptr, ld3, labels.ptr, n, C, c["ignore"], whole.ptr, lib.stream()), "eval_confusion")
    h = n // 2 + 1 if n else 0  # two calls over [0, h) and [h, n) add up to the one call
    for lo, hi in ((0, h), (h, n)):
        lib.check(L.mm_eval_confusion(a.ptr + 4 * lo * ld2, ld2, b.ptr + 4 * lo * ld3, ld3, labels.ptr + 8 * lo, hi - lo, C, c["ignore"],
                                      halves.ptr, lib.stream()), "eval_confusion")
    torch.cuda.synchronize()
    assert whole.padding_untouched() and halves.padding_untouched()
    got = whole.get()
    diff = np.flatnonzero(got != want)
    assert not len(diff), (f"{name}: {len(diff)} of {3 * C * C} counts differ; first at [matrix, target, prediction] = "
                           f"{np.unravel_index(diff[0], (3, C, C))}: {got[diff[0]] - before[diff[0]]} instead of {want[diff[0]] - before[diff[0]]}")
    assert np.array_equal(halves.get(), want), "two calls over the halves differ from one call over the whole"
    counted = int(R.counted(d["labels"], C, c["ignore"]).sum())
    assert (got - before).reshape(3, -1).sum(1).tolist() == [counted] * 3


# ---------------------------------------------------------------------------------------------------------- refused arguments
def test_loss_error_returns_come_before_any_launch():
    """C outside [1, 32], a row pitch below C and a negative N are refused, and a refused call has written nothing.  Every operand
    is 33 columns wide and every label is 0, so a call that was wrongly accepted would still stay inside the buffers.  (The refusal
    of null pointers is not tried: accepted by mistake, such a call would fault.)"""
    L, lib = _abi()
    n, wide = 64, 33
    x, t = Rows(None, n, wide, wide, fill=1.0), Rows(None, n, wide, wide, fill=0.5)
    labels, w = Ints(np.zeros(n, np.int64), dtype=torch.int64), vec(None, wide, fill=1.0)
    stats_in, g, ws = vec([1.0, float(n)], fill=1.0), vec([1.0], fill=1.0), _workspace(L)
    stats, loss, d = vec(None, 2), vec(None, 1), Rows(None, n, wide, wide, fill=SENTINEL)
    cm = Ints(None, 3 * wide * wide, dtype=torch.int64)
    s = lib.stream()

    def ce_fwd(N, C, ld):
        return L.mm_ce_fwd(x.ptr, ld, labels.ptr, w.ptr, N, C, -100, stats.ptr, ws.data_ptr(), ws.numel(), s)

    def ce_bwd(N, C, ld, ld_d):
        return L.mm_ce_bwd(x.ptr, ld, labels.ptr, w.ptr, N, C, -100, stats_in.ptr, g.ptr, d.ptr, ld_d, s)

    def kl_fwd(N, C, ld_p, ld_t):
        return L.mm_kl_fwd(x.ptr, ld_p, t.ptr, ld_t, N, C, loss.ptr, ws.data_ptr(), ws.numel(), s)

    def kl_bwd(N, C, ld_p, ld_t, ld_d):
        return L.mm_kl_bwd(x.ptr, ld_p, t.ptr, ld_t, N, C, g.ptr, d.ptr, ld_d, s)

    def confusion(N, C, ld2, ld3):
        return L.mm_eval_confusion(x.ptr, ld2, t.ptr, ld3, labels.ptr, N, C, -100, cm.ptr, s)

    calls = []
    for C in (0, 33):  # MM_PRED_MAXC = 32
        calls += [("ce_fwd", "bad C", lambda C=C: ce_fwd(n, C, wide)), ("ce_bwd", "bad C", lambda C=C: ce_bwd(n, C, wide, wide)),
                  ("kl_fwd", "bad C", lambda C=C: kl_fwd(n, C, wide, wide)), ("kl_bwd", "bad C", lambda C=C: kl_bwd(n, C, wide, wide, wide)),
                  ("eval_confusion", "bad C", lambda C=C: confusion(n, C, wide, wide))]
    C = 6
    calls += [("ce_fwd ld", "bad C", lambda: ce_fwd(n, C, C - 1)), ("ce_bwd ld", "bad C", lambda: ce_bwd(n, C, C - 1, wide)),
              ("ce_bwd ld_d", "bad C", lambda: ce_bwd(n, C, wide, C - 1)), ("kl_fwd ld_p", "bad C", lambda: kl_fwd(n, C, C - 1, wide)),
              ("kl_fwd ld_t", "bad C", lambda: kl_fwd(n, C, wide, C - 1)), ("kl_bwd ld_p", "bad C", lambda: kl_bwd(n, C, C - 1, wide, wide)),
              ("kl_bwd ld_t", "bad C", lambda: kl_bwd(n, C, wide, C - 1, wide)), ("kl_bwd ld_d", "bad C", lambda: kl_bwd(n, C, wide, wide, C - 1)),
              ("eval_confusion ld2", "bad C", lambda: confusion(n, C, C - 1, wide)),
              ("eval_confusion ld3", "bad C", lambda: confusion(n, C, wide, C - 1))]
    calls += [("ce_fwd N", "negative N", lambda: ce_fwd(-1, C, wide)), ("ce_bwd N", "negative N", lambda: ce_bwd(-1, C, wide, wide)),
              ("kl_fwd N", "negative N", lambda: kl_fwd(-1, C, wide, wide)), ("kl_bwd N", "negative N", lambda: kl_bwd(-1, C, wide, wide, wide)),
              ("eval_confusion N", "negative N", lambda: confusion(-1, C, wide, wide))]
    accepted = []
    for what, msg, call in calls:
        try:
            lib.check(call(), what)
            accepted.append(what)
        except RuntimeError as e:
            assert "rc=-1" in str(e) and msg in str(e), (what, str(e))
    torch.cuda.synchronize()
    assert not accepted, f"accepted: {accepted}"
    assert stats.untouched() and loss.untouched() and d.untouched() and cm.untouched(), "a refused call has written"
