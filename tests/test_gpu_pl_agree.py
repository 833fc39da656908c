"""mm_pl_agree (csrc/pselab.hip k_pl_agree, k_pl_agree_final), called straight through the C ABI, against the float64 numpy
reference of tests/_agree_ref.py, and pselab.agreement_weights on top of it.

Tolerances: w within 1e-5 absolute of float64 - the cross-entropy pair's tolerance; the kernel's formula restated in numpy
float32 (tests/test_pl_agreement_host.py) is within 1.3e-7 of float64 on such logits, so the bound leaves the device's expf / logf
eighty times that (observed on an MI355X over all the cases below: at most 1.3e-7).  stats within 1e-5 * max(1, |ref|) (the restatement's D: within 5.9e-7 * max(1, D)).  ``finite`` is exact.

Inputs: 3 * randn logits, seeded; pitched operands are views into wider buffers whose padding is NaN; ``w`` lies between two runs
of a sentinel that must survive.  Sizes: a tile is 128 rows; 131201 rows are 1026 tiles for the 1024 workgroups, so the tile loop
runs and the finish walks a second trip over the partials."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _agree_ref as R
from _gpu_rows import SENTINEL, Ints, Rows, abi as _abi, dev as _dev, vec

pytestmark = pytest.mark.gpu

LADDER_N = (0, 1, 127, 128, 129)
LADDER_C = (2, 6, 32)
N_CAPPED = 131201
BETA = 2.0


def _case(n, c, ld2=None, ld3=None, bad=(), beta=BETA):
    return dict(n=n, c=c, ld2=ld2 or c, ld3=ld3 or c, bad=tuple(bad), beta=beta)


def _cases():
    t = {f"n{n}_c{c}": _case(n, c) for n, c in itertools.product(LADDER_N, LADDER_C)}
    t["capped_c6"] = _case(N_CAPPED, 6)
    for c in LADDER_C:
        t[f"pitched_c{c}"] = _case(129, c, ld2=c + 3, ld3=c + 1)
    t["capped_pitched_nonfinite_c2"] = _case(N_CAPPED, 2, ld2=3, ld3=5, bad=(0, 63, 64, 127, 128, 70000, N_CAPPED - 1))
    t["nonfinite_c6"] = _case(129, 6, bad=(0, 5, 63, 64, 127, 128))
    t["all_nonfinite_c6"] = _case(3, 6, bad=(0, 1, 2))
    t["beta_small_c6"] = _case(129, 6, beta=0.125)
    t["beta_large_c32"] = _case(129, 32, ld2=40, beta=50.0)
    return t


CASES = _cases()
PLANTS = (("a", np.inf), ("b", np.nan), ("a", -np.inf), ("both", np.nan))  # which matrix, what value; in turn over the bad rows


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(a, b, reference) of a case: made once, shared, never modified."""
    c = CASES[name]
    a, b = R.make_pair(c["n"], c["c"], 900 + list(CASES).index(name))
    if c["n"] >= 2:
        b[1] = a[1]  # an identical pair of rows: weight exactly 1
    for k, r in enumerate(c["bad"]):
        which, v = PLANTS[k % len(PLANTS)]
        col = k % c["c"]
        if which in ("a", "both"):
            a[r, col] = v
        if which in ("b", "both"):
            b[r] = v  # a whole row
    return a, b, R.agreement(a, b, c["beta"])


def _run(L, lib, name):
    c = CASES[name]
    a, b, _ = _inputs(name)
    n, C = c["n"], c["c"]
    ra, rb = Rows(a, n, C, c["ld2"]), Rows(b, n, C, c["ld3"])
    w, stats, fin = vec(None, n), vec(None, 2), Ints(None, 1, dtype=torch.int64)
    ws = torch.empty(int(L.mm_pl_agree_ws_bytes()), dtype=torch.uint8, device=_dev())
    lib.check(L.mm_pl_agree(ra.ptr, c["ld2"], rb.ptr, c["ld3"], n, C, c["beta"], w.ptr, stats.ptr, fin.ptr, ws.data_ptr(), ws.numel(),
                            lib.stream()), "pl_agree")
    torch.cuda.synchronize()
    assert w.padding_untouched() and stats.padding_untouched() and fin.padding_untouched(), name  # nothing beyond N, 2 and 1
    return w.get32().reshape(-1), stats.get32().reshape(-1), int(fin.get()[0])


@pytest.mark.parametrize("name", list(CASES))
def test_weights_statistics_and_count_match_float64(name):
    L, lib = _abi()
    c = CASES[name]
    _, _, ref = _inputs(name)
    w, stats, fin = _run(L, lib, name)
    n = c["n"]
    assert not (w == np.float32(SENTINEL)).any() and np.isfinite(w).all()  # every row written
    ew = float(np.abs(w.astype(np.float64) - ref["weight"]).max(initial=0.0))
    es = [abs(float(stats[k]) - ref[key]) / max(1.0, abs(ref[key])) for k, key in enumerate(("mean_weight", "mean_div"))]
    print(f"{name}: max |w - ref| {ew:.2e}; mean w {stats[0]:.7f} ref {ref['mean_weight']:.7f}; mean D {stats[1]:.7f} ref "
          f"{ref['mean_div']:.7f}; finite {fin} of {n}")
    assert ew <= 1e-5
    assert es[0] <= 1e-5 and es[1] <= 1e-5
    assert fin == ref["finite"] == n - len(c["bad"])
    assert ((w >= 0) & (w <= 1)).all()
    if n >= 2 and 1 not in c["bad"]:
        assert w[1] == 1.0  # identical rows: exactly
    for r in c["bad"]:
        assert w[r] == 0.0  # planted rows: exactly zero, and left out of the mean of D (stats[1] above)
    if n == 0 or fin == 0:
        assert stats[1] == 0.0 and (n > 0 or stats[0] == 0.0)


@pytest.mark.parametrize("name", ["n129_c6", "capped_c6", "capped_pitched_nonfinite_c2"])
def test_two_runs_are_bit_identical(name):
    L, lib = _abi()
    a, b = _run(L, lib, name), _run(L, lib, name)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert a[2] == b[2]


def test_the_finite_count_may_be_left_out():
    L, lib = _abi()
    a, b, ref = _inputs("n129_c6")
    ra, rb, w, stats = Rows(a, 129, 6, 6), Rows(b, 129, 6, 6), vec(None, 129), vec(None, 2)
    ws = torch.empty(int(L.mm_pl_agree_ws_bytes()), dtype=torch.uint8, device=_dev())
    lib.check(L.mm_pl_agree(ra.ptr, 6, rb.ptr, 6, 129, 6, BETA, w.ptr, stats.ptr, None, ws.data_ptr(), ws.numel(), lib.stream()), "pl_agree")
    torch.cuda.synchronize()
    assert np.array_equal(w.get32().reshape(-1), _run(L, lib, "n129_c6")[0])


def test_every_refusal_arrives_before_a_launch():
    """A refused call returns -1 with the error text and leaves every output as it was."""
    L, lib = _abi()
    a, b, _ = _inputs("n129_c6")
    ra, rb = Rows(a, 129, 6, 6), Rows(b, 129, 6, 6)
    w, stats, fin = vec(None, 129), vec(None, 2), Ints(None, 1, dtype=torch.int64)
    need = int(L.mm_pl_agree_ws_bytes())
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())

    def call(a=ra.ptr, ld2=6, b=rb.ptr, ld3=6, N=129, C=6, beta=BETA, w=w.ptr, stats=stats.ptr, ws=ws.data_ptr(), ws_bytes=need):
        return L.mm_pl_agree(a, ld2, b, ld3, N, C, beta, w, stats, fin.ptr, ws, ws_bytes, lib.stream())

    bad = [(dict(C=1), b"C must lie in [2, 32]"), (dict(C=33, ld2=33, ld3=33), b"C must lie in [2, 32]"), (dict(ld2=5), b"row pitch"),
           (dict(ld3=5), b"row pitch"), (dict(beta=0.0), b"beta"), (dict(beta=-2.0), b"beta"), (dict(beta=float("inf")), b"beta"),
           (dict(beta=float("nan")), b"beta"), (dict(N=-1), b"N * C"), (dict(N=(1 << 31) // 6 + 1), b"N * C must stay below 2^31"),
           (dict(a=None), b"null"), (dict(b=None), b"null"), (dict(w=None), b"null"), (dict(stats=None), b"null stats"),
           (dict(ws=None), b"workspace"), (dict(ws_bytes=need - 1), b"workspace")]
    for kw, word in bad:
        assert call(**kw) == -1, kw
        assert b"pl_agree:" in L.mm_last_error() and word in L.mm_last_error(), (kw, L.mm_last_error())
    torch.cuda.synchronize()
    assert w.untouched() and stats.untouched() and fin.untouched()
    assert call() == 0  # and the same operands are fine
    torch.cuda.synchronize()
    assert not w.untouched()


# ---------------------------------------------------------------------------------------------- pselab.agreement_weights
@pytest.mark.parametrize("name", ["n0_c6", "n129_c6", "pitched_c32", "capped_pitched_nonfinite_c2"])
def test_agreement_weights_is_the_abi_call_on_device_tensors(name):
    from mm2d3d_amd import pselab

    L, lib = _abi()
    c = CASES[name]
    a, b, ref = _inputs(name)
    ra, rb = Rows(a, c["n"], c["c"], c["ld2"]), Rows(b, c["n"], c["c"], c["ld3"])
    if c["ld2"] != c["c"] and c["n"] > 1:
        assert ra.view.stride() == (c["ld2"], 1) and not ra.view.is_contiguous()  # read in place through _lib.row_pitched
    out = pselab.agreement_weights(ra.view, rb.view, c["beta"])
    assert set(out) == {"weight", "mean_weight", "mean_div", "finite"}
    assert all(v.is_cuda and not v.requires_grad for v in out.values())
    assert out["weight"].shape == (c["n"],) and out["weight"].dtype == torch.float32
    assert out["mean_weight"].shape == out["mean_div"].shape == out["finite"].shape == () and out["finite"].dtype == torch.int64
    w, stats, fin = _run(L, lib, name)
    assert np.array_equal(out["weight"].cpu().numpy().view(np.int32), w.view(np.int32))
    assert float(out["mean_weight"]) == float(stats[0]) and float(out["mean_div"]) == float(stats[1]) and int(out["finite"]) == fin == ref["finite"]


def test_agreement_weights_takes_half_precision_logits_and_refuses_mismatches():
    from mm2d3d_amd import pselab

    dev = _dev()
    a, b, _ = _inputs("n129_c6")
    ha, hb = torch.from_numpy(a).to(dev).half(), torch.from_numpy(b).to(dev).half()
    got = pselab.agreement_weights(ha, hb, BETA)["weight"].cpu().numpy().astype(np.float64)
    ref = R.agreement(ha.float().cpu().numpy(), hb.float().cpu().numpy(), BETA)["weight"]  # of the rounded logits
    assert np.abs(got - ref).max() <= 1e-5
    with pytest.raises(ValueError, match="same shape"):
        pselab.agreement_weights(ha, hb[:100], BETA)
    with pytest.raises(ValueError, match="classes"):
        pselab.agreement_weights(torch.zeros(4, 1, device=dev), torch.zeros(4, 1, device=dev), BETA)
    with pytest.raises(ValueError, match="classes"):
        pselab.agreement_weights(torch.zeros(4, 33, device=dev), torch.zeros(4, 33, device=dev), BETA)
    with pytest.raises(ValueError, match=r"\[N, C\]"):
        pselab.agreement_weights(torch.zeros(4, device=dev), torch.zeros(4, device=dev), BETA)
