"""mm_teacher_labels on the GPU (csrc/pselab.hip k_teacher_labels, pselab.teacher_labels): the int64 training labels a teacher's
logits give both heads.  Exact parity with pselab.predict (the same device expression: no row may be excluded), the threshold
rule, the kept counts, guard words, and an independent float64 numpy oracle.

Oracle exclusions: a row is compared only if, for both outputs, the float64 gap between the two largest probabilities is
>= 1e-5 and |p - thr| >= 1e-5.  fp32 softmax probabilities of C <= 32 logits of magnitude <= ~15 carry a relative error of a few
2**-24 per exponential and sum (<= 1e-6 absolute on values <= 1), so a gap of 1e-5 cannot be reversed by rounding.  With
3 * randn logits the probabilities are spread over (0, 1): the oracle itself excludes 0-2 rows of 1000, and the test asserts
<= 1 % on the oracle's side before it compares."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 127, 128, 129, 1000]  # the tile is 128 rows
CS = [1, 5, 6, 11, 32]
THRESHOLDS = [None, 0.5, 0.9]
GUARD = 16


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


_CACHE = {}


def _logits(C):
    """(2D, 3D) logits [1000, C] fp32 = 3 * randn, seeded per class count; computed once, never written."""
    if C not in _CACHE:
        rng = np.random.default_rng(1234 + C)
        _CACHE[C] = tuple((3.0 * rng.standard_normal((1000, C))).astype(np.float32) for _ in range(2))
    return _CACHE[C]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_against_predict(a, b, what):
    """Every mode and threshold of teacher_labels against where(p >= thr, label, -100) of predict's outputs, exactly."""
    from mm2d3d_amd import pselab

    ref = pselab.predict(a, b)
    for ens in (False, True):
        keys = (("probs_ensemble", "pseudo_label_ensemble"),) * 2 if ens else (("probs_2d", "pseudo_label_2d"), ("probs_3d", "pseudo_label_3d"))
        for thr in THRESHOLDS:
            got = pselab.teacher_labels(a, b, ensemble=ens, threshold=thr, with_probs=True)
            bare = pselab.teacher_labels(a, b, ensemble=ens, threshold=thr)
            assert set(got) == {"label_2d", "label_3d", "kept", "prob_2d", "prob_3d"} and set(bare) == {"label_2d", "label_3d", "kept"}
            assert got["kept"].dtype == torch.int64 and got["kept"].shape == (2,) and got["label_2d"].dtype == torch.int64
            for j, (out, (pk, yk)) in enumerate(zip(("2d", "3d"), keys)):
                p, y = ref[pk], ref[yk].long()
                want = y if thr is None else torch.where(p >= torch.tensor(thr, dtype=torch.float32, device=p.device), y, torch.full_like(y, -100))
                assert torch.equal(got[f"label_{out}"], want), (what, ens, thr, out)
                assert torch.equal(bare[f"label_{out}"], want), (what, ens, thr, out)
                assert torch.equal(_bits(got[f"prob_{out}"]), _bits(p)), (what, ens, thr, out)
                assert int(got["kept"][j]) == int((want != -100).sum()) == int(bare["kept"][j]), (what, ens, thr, out)
                if thr is None:
                    assert int(got["kept"][j]) == a.shape[0]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", NS)
def test_labels_probabilities_and_counts_equal_predict_exactly(N, C):
    dev = _dev()
    a, b = (torch.from_numpy(x[:N]).to(dev) for x in _logits(C))
    _check_against_predict(a, b, (N, C))


def test_row_pitched_views_are_read_in_place_past_nan_padding():
    dev = _dev()
    N, C = 129, 6
    a0, b0 = (torch.from_numpy(x[:N]).to(dev) for x in _logits(C))
    wide_a = torch.full((N, 8), float("nan"), device=dev)
    wide_b = torch.full((N, 11), float("nan"), device=dev)
    wide_a[:, 1 : 1 + C], wide_b[:, 5 : 5 + C] = a0, b0
    a, b = wide_a[:, 1 : 1 + C], wide_b[:, 5 : 5 + C]
    assert a.stride(0) == 8 and b.stride(0) == 11 and not a.is_contiguous()
    from mm2d3d_amd import pselab

    for ens in (False, True):
        got, want = pselab.teacher_labels(a, b, ensemble=ens, threshold=0.5, with_probs=True), pselab.teacher_labels(a0, b0, ensemble=ens, threshold=0.5, with_probs=True)
        for k in want:
            assert torch.equal(_bits(got[k]), _bits(want[k])), (ens, k)
        assert int(got["kept"].min()) > 0 and int(got["kept"].max()) < N  # the padding was not read: nothing is NaN, the threshold bites
    _check_against_predict(a, b, "pitched")


@pytest.mark.parametrize("N,C", [(129, 5), (1000, 32), (1, 1)])
def test_outputs_stay_inside_guard_padded_buffers(N, C):
    """Through the C ABI: the five outputs as slices of larger buffers whose other words must keep their bits."""
    from mm2d3d_amd import _lib, pselab
    from mm2d3d_amd._lib import check, ptr, stream

    dev = _dev()
    a, b = (torch.from_numpy(x[:N]).to(dev) for x in _logits(C))
    for ens in (0, 1):
        ybuf = torch.full((2, N + 2 * GUARD), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        pbuf = torch.full((2, N + 2 * GUARD), -7.25, dtype=torch.float32, device=dev)
        kbuf = torch.full((2 + 2 * GUARD,), 0x1234567, dtype=torch.int64, device=dev)
        y0, p0, k0 = ybuf.clone(), pbuf.clone(), kbuf.clone()
        ys, ps, ks = ybuf[:, GUARD : GUARD + N], pbuf[:, GUARD : GUARD + N], kbuf[GUARD : GUARD + 2]
        check(_lib.lib().mm_teacher_labels(ptr(a), C, ptr(b), C, N, C, ens, 0.5, -100, ptr(ys[0]), ptr(ys[1]), ptr(ps[0]), ptr(ps[1]), ptr(ks),
                                           stream()), "teacher_labels")
        want = pselab.teacher_labels(a, b, ensemble=bool(ens), threshold=0.5, with_probs=True)
        assert torch.equal(ys[0], want["label_2d"]) and torch.equal(ys[1], want["label_3d"])
        assert torch.equal(_bits(ps[0]), _bits(want["prob_2d"])) and torch.equal(_bits(ps[1]), _bits(want["prob_3d"]))
        assert torch.equal(ks, want["kept"])
        for buf, old, lo, hi in ((ybuf, y0, GUARD, GUARD + N), (pbuf, p0, GUARD, GUARD + N)):
            assert torch.equal(buf[:, :lo], old[:, :lo]) and torch.equal(buf[:, hi:], old[:, hi:])
        assert torch.equal(kbuf[:GUARD], k0[:GUARD]) and torch.equal(kbuf[GUARD + 2 :], k0[GUARD + 2 :])
        # without the optional outputs nothing but the labels is written
        ybuf.copy_(y0)
        check(_lib.lib().mm_teacher_labels(ptr(a), C, ptr(b), C, N, C, ens, 0.5, -100, ptr(ys[0]), ptr(ys[1]), None, None, None, stream()),
              "teacher_labels")
        assert torch.equal(ys[0], want["label_2d"]) and torch.equal(ys[1], want["label_3d"])
        assert torch.equal(ybuf[:, :GUARD], y0[:, :GUARD]) and torch.equal(ybuf[:, GUARD + N :], y0[:, GUARD + N :])
    # another ignore label travels through
    alt = torch.empty((2, N), dtype=torch.int64, device=dev)
    check(_lib.lib().mm_teacher_labels(ptr(a), C, ptr(b), C, N, C, 0, 0.5, 255, ptr(alt[0]), ptr(alt[1]), None, None, None, stream()), "teacher_labels")
    ref = pselab.teacher_labels(a, b, threshold=0.5)
    assert torch.equal(alt[0], torch.where(ref["label_2d"] == -100, torch.full_like(alt[0], 255), ref["label_2d"]))


def _softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _top_and_gap(p):
    """First-maximum argmax, its probability and the gap to the runner-up (inf for one class)."""
    i = p.argmax(1)  # numpy: the first maximum
    top = p[np.arange(len(p)), i]
    if p.shape[1] == 1:
        return i, top, np.full(len(p), np.inf)
    rest = p.copy()
    rest[np.arange(len(p)), i] = -np.inf
    return i, top, top - rest.max(1)


@pytest.mark.parametrize("C", CS)
def test_labels_against_a_float64_oracle(C):
    from mm2d3d_amd import pselab

    dev = _dev()
    a_np, b_np = _logits(C)
    N = a_np.shape[0]
    a, b = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)
    sa, sb = _softmax64(a_np), _softmax64(b_np)
    for ens in (False, True):
        dists = (0.5 * (sa + sb),) * 2 if ens else (sa, sb)
        for thr in THRESHOLDS:
            want, excluded = [], np.zeros(N, bool)
            for p in dists:
                i, top, gap = _top_and_gap(p)
                excluded |= gap < 1e-5
                if thr is not None:
                    excluded |= np.abs(top - thr) < 1e-5
                    i = np.where(top >= thr, i, -100)
                want.append(i)
            print(f"C {C} ensemble {ens} thr {thr}: the oracle excludes {int(excluded.sum())} rows of {N}")
            assert excluded.mean() <= 0.01  # the cap, on the oracle's side, before anything is compared
            got = pselab.teacher_labels(a, b, ensemble=ens, threshold=thr)
            for out, w in zip(("label_2d", "label_3d"), want):
                g = got[out].cpu().numpy()
                assert np.array_equal(g[~excluded], w[~excluded]), (C, ens, thr, out, int((g != w)[~excluded].sum()))


def test_non_finite_logits():
    from mm2d3d_amd import pselab

    dev = _dev()
    a, b = (torch.from_numpy(x[:130]).to(dev).clone() for x in _logits(6))
    a[3], b[3] = float("nan"), float("nan")  # a whole row of both
    a[128] = float("nan")  # of the 2D logits only, in the second tile: the 3D label is judged on its own, the ensemble is NaN
    for ens in (False, True):
        got = pselab.teacher_labels(a, b, ensemble=ens, threshold=0.5, with_probs=True)
        assert int(got["label_2d"][3]) == -100 and int(got["label_3d"][3]) == -100
        assert int(got["label_2d"][128]) == -100
        assert not bool(got["prob_2d"][3] >= 0.5) and not bool(got["prob_2d"][128] >= 0.5)  # NaN, or the ensemble's "no maximum" -1
        if not ens:
            assert torch.isnan(got["prob_2d"][3]) and torch.isnan(got["prob_3d"][3]) and torch.isfinite(got["prob_3d"][128])
        if ens:
            assert int(got["label_3d"][128]) == -100
        kept = torch.stack([(got["label_2d"] != -100).sum(), (got["label_3d"] != -100).sum()])
        assert torch.equal(got["kept"], kept)
    _check_against_predict(a, b, "nan rows")  # threshold=None: what predict gives; thresholds: where(p >= thr) is False on NaN


def test_threshold_zero_refuses_exactly_the_rows_without_a_confidence():
    """What the trainer's "median" mode passes on to mm_pselab_refine, which wants finite probabilities: with threshold 0 a row of
    non-finite logits is -100 (refine passes it through unread) and every other row keeps its label."""
    from mm2d3d_amd import pselab

    dev = _dev()
    a, b = (torch.from_numpy(x[:300]).to(dev).clone() for x in _logits(6))
    bad = [3, 128, 299]
    for i in bad:
        a[i], b[i] = float("nan"), float("inf")
    good = torch.ones(300, dtype=torch.bool, device=dev)
    good[bad] = False
    for ens in (False, True):
        cut, free = pselab.teacher_labels(a, b, ensemble=ens, threshold=0.0, with_probs=True), pselab.teacher_labels(a, b, ensemble=ens)
        for out in ("2d", "3d"):
            y, p = cut[f"label_{out}"], cut[f"prob_{out}"]
            assert bool((y[~good] == -100).all()) and torch.equal(y[good], free[f"label_{out}"][good]) and bool(torch.isfinite(p[good]).all())
            got = pselab.refine_pseudo_labels(p, y, num_classes=6, device=dev)
            want = pselab.refine_pseudo_labels(p[good].contiguous(), y[good].contiguous(), num_classes=6, device=dev)
            assert bool((got[~good] == -100).all()) and torch.equal(got[good], want), (ens, out)
        assert cut["kept"].tolist() == [297, 297]


def test_an_empty_batch_launches_nothing():
    from mm2d3d_amd import pselab

    dev = _dev()
    e = torch.empty((0, 6), device=dev)
    out = pselab.teacher_labels(e, e, threshold=0.9, with_probs=True)
    assert out["label_2d"].shape == (0,) and out["prob_3d"].shape == (0,) and out["kept"].tolist() == [0, 0]
    # shape errors name the function that was called
    with pytest.raises(ValueError, match=r"pselab\.teacher_labels: logits_2d"):
        pselab.teacher_labels(torch.zeros(3, device=dev), e)
    with pytest.raises(ValueError, match=r"pselab\.teacher_labels: .*same shape"):
        pselab.teacher_labels(torch.zeros(2, 6, device=dev), e)


@pytest.mark.parametrize("ens", [False, True], ids=["own", "ensemble"])
def test_a_threshold_tensor_gives_the_labels_of_the_adaptive_object(ens):
    """teacher_labels(threshold=[2, C] tensor) called directly gives what AdaptiveThreshold.labels gives a second object in the same
    state.  Both go through the same wrapper and the same launch, so this is no check against a second implementation (the float64
    oracle of tests/test_gpu_pl_adaptive.py is that): it pins the public argument - the tensor is taken, the per-class entry point
    runs, ``kept`` counts the labels that are not -100, rows without a confidence are refused.  130 rows = one full 128-row tile
    and a ragged one; one row without a confidence in each matrix."""
    from mm2d3d_amd import pselab

    dev = _dev()
    a, b = (torch.from_numpy(x[:130]).to(dev).clone() for x in _logits(6))
    a[3, 2], b[129, 0] = float("nan"), float("inf")
    one, two = (pselab.AdaptiveThreshold(6, momentum=0.5, device=dev) for _ in range(2))
    thr = one.update(a, b, ensemble=ens)
    want = two.labels(a, b, ensemble=ens, with_probs=True)
    got = pselab.teacher_labels(a, b, ensemble=ens, threshold=thr, with_probs=True)
    assert torch.equal(one.state.view(torch.int64), two.state.view(torch.int64)) and torch.equal(_bits(thr), _bits(want["threshold"]))
    assert set(got) == set(want) - {"threshold"}
    for k in ("label_2d", "label_3d", "kept"):
        assert torch.equal(got[k], want[k]), (ens, k)
    kept = [int((got[k] != -100).sum()) for k in ("label_2d", "label_3d")]
    assert got["kept"].tolist() == kept and all(0 < k < 130 for k in kept), kept  # the thresholds bite, and not on every row
    assert int(got["label_2d"][3]) == -100 and int(got["label_3d"][129]) == -100  # no confidence: refused under any threshold
