"""Self-adaptive per-class pseudo-label thresholds on the GPU: pselab.AdaptiveThreshold (csrc/pselab.hip k_pl_stats / k_pl_update
behind mm_pl_adapt, k_teacher_labels behind mm_teacher_labels_cls) and the per-class soft-tail pair (csrc/loss.hip,
mm_ce2s_fwd_cls / mm_ce2s_bwd_cls).  Logits of tests/test_gpu_teacher_labels.py: 3 * randn, seed 1234 + C.

Three kinds of check:
  exact     every row, no exclusions: labels, confidences and counts against pselab.predict (the same device expression) under the
            thresholds the call returned, and those thresholds against float32((pt / pt.max()) * tau) of the state read back.
            Equality was what came out on the MI355X (no contraction: a division, then a multiplication); the assertion allows the
            1 ulp the definition grants.
  oracle    the state and the thresholds against tests/_adaptive_ref.py (float64 numpy).  State within 1e-5 absolute, thresholds
            within 2e-5: fp32 softmax values carry at most 1e-6 absolute error (tests/test_gpu_teacher_labels.py), the means and
            the convex updates do not amplify it, and the ratio times tau at most doubles it.  Counts are exact.  Labels: rows
            whose float64 |p - thr[y]| or top-two gap is below 1e-5 are not decidable in float32 and are excluded, at most 1 % of
            them, asserted on the oracle's side.
  edges     non-finite rows, an all-refused batch, run-to-run bits, row-pitched views, guard words, N == 0."""
import functools
import math

import numpy as np
import pytest
import torch

from _adaptive_ref import AdaptiveRef

pytestmark = pytest.mark.gpu

GUARD = 16


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _logits(C):
    """(2D, 3D) logits [1000, C] fp32 = 3 * randn, seeded per class count; computed once, never written."""
    rng = np.random.default_rng(1234 + C)
    return tuple((3.0 * rng.standard_normal((1000, C))).astype(np.float32) for _ in range(2))


def _pair(C, N, dev, lo=0):
    return tuple(torch.from_numpy(x[lo : lo + N]).to(dev) for x in _logits(C))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _thr_of_state(state):
    """float32((pt / pt.max()) * tau) in float64, in this order, from a state read back."""
    s = state.cpu().numpy()
    pt, tau = s[:, 1:], s[:, :1]
    return ((pt / pt.max(1, keepdims=True)) * tau).astype(np.float32)


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def _check_against_predict(a, b, ens, out, what):
    """labels == where(p >= thr[y], y, -100) from predict's outputs and the thresholds the call returned; confidences bit for bit;
    kept == the count of kept labels."""
    from mm2d3d_amd import pselab

    ref = pselab.predict(a, b)
    thr = out["threshold"]
    keys = (("probs_ensemble", "pseudo_label_ensemble"),) * 2 if ens else (("probs_2d", "pseudo_label_2d"), ("probs_3d", "pseudo_label_3d"))
    for o, (name, (pk, yk)) in enumerate(zip(("2d", "3d"), keys)):
        p, y = ref[pk], ref[yk].long()
        want = torch.where(p >= thr[o][y], y, torch.full_like(y, -100))
        assert torch.equal(out[f"label_{name}"], want), (what, name, int((out[f"label_{name}"] != want).sum()))
        if f"prob_{name}" in out:
            assert torch.equal(_bits(out[f"prob_{name}"]), _bits(p)), (what, name)
        assert int(out["kept"][o]) == int((want != -100).sum()), (what, name)


# ---------------------------------------------------------------------------------------------- exact, every row
@pytest.mark.parametrize("C", [1, 5, 6, 32])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 127, 128, 129, 1000])
def test_labels_confidences_counts_and_thresholds_are_exact(N, C):
    from mm2d3d_amd import pselab

    dev = _dev()
    a, b = _pair(C, N, dev)
    worst = 0
    for ens in (False, True):
        for m in (0.0, 0.5):
            ad = pselab.AdaptiveThreshold(C, momentum=m, device=dev)
            assert ad.state.dtype == torch.float64 and ad.state.shape == (2, 1 + C) and ad.count.dtype == torch.int64
            assert torch.equal(ad.state, torch.full((2, 1 + C), 1.0 / C, dtype=torch.float64, device=dev)) and ad.count.tolist() == [0, 0]
            out = ad.labels(a, b, ensemble=ens, with_probs=True)
            assert set(out) == {"label_2d", "label_3d", "kept", "threshold", "prob_2d", "prob_3d"}
            assert set(ad.labels(a, b, ensemble=ens)) == {"label_2d", "label_3d", "kept", "threshold"}
            thr = out["threshold"]
            assert thr.dtype == torch.float32 and thr.shape == (2, C) and out["kept"].dtype == torch.int64 and out["label_2d"].dtype == torch.int64
            _check_against_predict(a, b, ens, out, (N, C, ens, m))
            # the thresholds of the second call, from the state as it is now
            again = ad.update(a, b, ensemble=ens)
            want = _thr_of_state(ad.state)
            worst = max(worst, _ulps(again.cpu().numpy(), want))
            assert ad.count.tolist() == [3, 3]
    print(f"N {N} C {C}: thr against float32((pt / pt.max()) * tau) of the state read back: {worst} ulp")
    assert worst <= 1


# ---------------------------------------------------------------------------------------------- the state against the oracle
def _state_close(ad, ref, thr, what):
    s = ad.state.cpu().numpy()
    err_s, err_t = float(np.abs(s - ref.state).max()), float(np.abs(thr.cpu().numpy().astype(np.float64) - ref.thresholds().astype(np.float64)).max())
    print(f"{what}: max |state - oracle| {err_s:.2e}, max |thr - oracle| {err_t:.2e}, counts {ad.count.tolist()}")
    assert ad.count.tolist() == ref.count.tolist(), what
    assert err_s <= 1e-5 and err_t <= 2e-5, what


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("C", [5, 6, 32])
def test_state_matches_the_oracle_after_one_and_after_three_updates(C, warmup):
    from mm2d3d_amd import pselab

    dev = _dev()
    x2, x3 = _logits(C)
    slices = [(0, 129), (129, 500), (629, 371)]  # different rows each time; three tiles and a rest, two tiles and a rest
    for ens in (False, True):
        for m in (0.5, 0.999):
            ad, ref = pselab.AdaptiveThreshold(C, momentum=m, warmup=warmup, device=dev), AdaptiveRef(C, momentum=m, warmup=warmup)
            for k, (lo, n) in enumerate(slices):
                thr = ad.update(*_pair(C, n, dev, lo), ensemble=ens)
                ref.update(x2[lo : lo + n], x3[lo : lo + n], ensemble=ens)
                if k in (0, 2):
                    _state_close(ad, ref, thr, f"C {C} ens {ens} m {m} warmup {warmup} after {k + 1}")


# ---------------------------------------------------------------------------------------------- the labels against the oracle
@pytest.mark.parametrize("C", [5, 6, 11, 32])
@pytest.mark.parametrize("N", [64, 129, 1000])
def test_labels_match_the_oracle(N, C):
    from mm2d3d_amd import pselab

    dev = _dev()
    x2, x3 = (x[:N] for x in _logits(C))
    a, b = _pair(C, N, dev)
    for ens in (False, True):
        for m in (0.0, 0.5):
            want = AdaptiveRef(C, momentum=m).labels(x2, x3, ensemble=ens)
            excluded = ((want["margin"] < 1e-5) | (want["gap"] < 1e-5)).any(0)
            print(f"N {N} C {C} ens {ens} m {m}: the oracle excludes {int(excluded.sum())} rows, keeps {want['kept'].tolist()}")
            assert excluded.mean() <= 0.01  # the cap, on the oracle's side, before anything is compared
            if m == 0.0:  # the thresholds bite: neither everything nor nothing is kept
                assert all(0 < int(k) < N for k in want["kept"])
            got = pselab.AdaptiveThreshold(C, momentum=m, device=dev).labels(a, b, ensemble=ens)
            for o, name in enumerate(("label_2d", "label_3d")):
                g = got[name].cpu().numpy()
                assert np.array_equal(g[~excluded], want["label"][o][~excluded]), (N, C, ens, m, name)
            if not excluded.any():
                assert got["kept"].tolist() == want["kept"].tolist()


@pytest.mark.parametrize("C", [5, 6, 32])
def test_the_default_momentum_keeps_every_row_at_the_start(C):
    """The documented start-up behaviour: from tau = pt = 1 / C with momentum 0.999 the thresholds stay near 1 / C, and no
    confidence (the largest of C probabilities that sum to 1) is below 1 / C."""
    from mm2d3d_amd import pselab

    dev = _dev()
    a, b = _pair(C, 1000, dev)
    for ens in (False, True):
        ad = pselab.AdaptiveThreshold(C, device=dev)
        assert ad.momentum == 0.999 and ad.warmup is False
        out = ad.labels(a, b, ensemble=ens)
        assert out["kept"].tolist() == [1000, 1000] and int((out["label_2d"] == -100).sum()) == 0
        assert float(out["threshold"].max()) < 1.0 / C + 1e-3


# ---------------------------------------------------------------------------------------------- edges
def test_non_finite_rows_are_not_counted():
    from mm2d3d_amd import pselab

    dev = _dev()
    C, N = 6, 300
    x2, x3 = (x[:N].copy() for x in _logits(C))
    x2[3], x3[3] = np.nan, np.nan  # a whole row of both
    x2[128, 2], x3[128, 4] = np.inf, np.inf  # one entry each, in the second tile
    x2[299, 1] = np.nan  # of the 2D logits only: the 3D output counts the row, the ensemble does not
    x2[7, 0], x3[7, 5] = -np.inf, -np.inf  # -inf alone stays finite: a probability of exactly 0
    a, b = torch.from_numpy(x2).to(dev), torch.from_numpy(x3).to(dev)
    for ens in (False, True):
        ad, ref = pselab.AdaptiveThreshold(C, momentum=0.5, device=dev), AdaptiveRef(C, momentum=0.5)
        out = ad.labels(a, b, ensemble=ens, with_probs=True)
        want = ref.labels(x2, x3, ensemble=ens)
        _state_close(ad, ref, out["threshold"], f"non-finite rows, ens {ens}")
        assert bool(torch.isfinite(ad.state).all()) and bool(torch.isfinite(out["threshold"]).all())
        refused2 = [3, 128, 299]
        refused3 = [3, 128, 299] if ens else [3, 128]
        assert all(int(out["label_2d"][i]) == -100 for i in refused2) and all(int(out["label_3d"][i]) == -100 for i in refused3)
        assert bool(torch.isfinite(out["prob_2d"][7])) and bool(torch.isfinite(out["prob_3d"][7]))
        if not ens:
            assert bool(torch.isfinite(out["prob_3d"][299]))
        _check_against_predict(a, b, ens, out, f"non-finite rows, ens {ens}")
        # the counted rows, through a momentum-0 update: tau is then the mean confidence over exactly those rows
        z = pselab.AdaptiveThreshold(C, momentum=0.0, device=dev)
        z.update(a, b, ensemble=ens)
        p = out["prob_2d"].double(), out["prob_3d"].double()
        for o, bad in enumerate((refused2, refused3)):
            good = torch.ones(N, dtype=torch.bool, device=dev)
            good[bad] = False
            assert int(good.sum()) == N - len(bad)
            assert abs(float(z.state[o, 0]) - float(p[o][good].mean())) <= 1e-12  # N - len(bad) rows, not one more or fewer
        excluded = ((want["margin"] < 1e-5) | (want["gap"] < 1e-5)).any(0)
        for o, name in enumerate(("label_2d", "label_3d")):
            assert np.array_equal(out[name].cpu().numpy()[~excluded], want["label"][o][~excluded])


def test_a_batch_without_a_counted_row_leaves_the_state_alone():
    from mm2d3d_amd import pselab

    dev = _dev()
    C = 6
    ad = pselab.AdaptiveThreshold(C, momentum=0.5, warmup=True, device=dev)
    ad.update(*_pair(C, 200, dev))
    state, count = ad.state.clone(), ad.count.clone()
    old_thr = _thr_of_state(state)
    bad = torch.full((130, C), float("nan"), device=dev)
    bad[1], bad[129, 3] = float("inf"), float("inf")
    for ens in (False, True):
        out = ad.labels(bad, bad.clone(), ensemble=ens)
        assert torch.equal(_bits(ad.state), _bits(state)) and torch.equal(ad.count, count) and count.tolist() == [1, 1]
        assert _ulps(out["threshold"].cpu().numpy(), old_thr) <= 1
        assert out["kept"].tolist() == [0, 0] and bool((out["label_2d"] == -100).all()) and bool((out["label_3d"] == -100).all())
    # one output alone without a counted row: the other one moves on
    ok = _pair(C, 130, dev)[1]
    ad.update(bad, ok)
    assert torch.equal(_bits(ad.state[0]), _bits(state[0])) and not torch.equal(_bits(ad.state[1]), _bits(state[1]))
    assert ad.count.tolist() == [1, 2]


def test_two_objects_fed_the_same_sequence_end_with_equal_bits():
    from mm2d3d_amd import pselab

    dev = _dev()
    C = 6
    ends = []
    for _ in range(2):
        ad = pselab.AdaptiveThreshold(C, momentum=0.9, warmup=True, device=dev)
        thrs = [ad.update(*_pair(C, n, dev, lo), ensemble=ens) for lo, n, ens in ((0, 1000, False), (100, 333, True), (0, 1, False), (7, 129, True))]
        ends.append((ad.state.view(torch.int64).clone(), ad.count.clone(), torch.stack(thrs).view(torch.int32)))
    assert all(torch.equal(x, y) for x, y in zip(*ends))
    # state_dict / load_state_dict / reset carry exactly these bits
    other = pselab.AdaptiveThreshold(C, momentum=0.9, warmup=True, device=dev)
    sd = ad.state_dict()
    assert set(sd) == {"num_classes", "state", "count"} and sd["state"].data_ptr() != ad.state.data_ptr()
    other.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})
    assert torch.equal(other.state.view(torch.int64), ends[0][0]) and torch.equal(other.count, ends[0][1])
    assert torch.equal(_bits(other.update(*_pair(C, 64, dev))), _bits(ad.update(*_pair(C, 64, dev))))
    other.reset()
    assert torch.equal(other.state, torch.full((2, 1 + C), 1.0 / C, dtype=torch.float64, device=dev)) and other.count.tolist() == [0, 0]
    with pytest.raises(ValueError, match="classes"):
        pselab.AdaptiveThreshold(5, device=dev).load_state_dict(sd)
    with pytest.raises(ValueError, match="momentum"):
        pselab.AdaptiveThreshold(C, momentum=1.0, device=dev)
    with pytest.raises(ValueError, match="classes"):
        pselab.AdaptiveThreshold(33, device=dev)
    with pytest.raises(ValueError, match=r"AdaptiveThreshold\.update"):
        ad.update(*_pair(5, 64, dev))


WALK_N = 1024 * 128 + 129  # 1024 workgroups at most, 128 rows per tile: 1026 tiles


@functools.lru_cache(maxsize=None)
def _walk_logits(C):
    """(2D, 3D) logits [WALK_N, C] fp32 = 3 * randn from a seed of their own, with the non-finite rows of the test below; computed
    once, never written."""
    rng = np.random.default_rng(4321 + C)
    x2, x3 = ((3.0 * rng.standard_normal((WALK_N, C))).astype(np.float32) for _ in range(2))
    x2[131100], x3[131100] = np.nan, np.nan  # a whole row of both, in tile 1024: the second tile of workgroup 0
    x2[131200, 1] = np.inf  # of the 2D logits only, the one row of tile 1025: the second tile of workgroup 1
    return x2, x3


@pytest.mark.parametrize("ens", [False, True], ids=["own", "ensemble"])
@pytest.mark.parametrize("C", [5, 32])
def test_the_walk_over_more_tiles_than_workgroups(C, ens):
    """mm_pl_adapt at N = 1024 * 128 + 129: workgroup 0 takes tiles 0 and 1024 (the second one full), workgroup 1 takes tiles 1 and
    1025 (the second one a single row), every other workgroup one tile - the accumulator carried across a workgroup's tiles and
    the barrier before restaging.  Both second tiles hold rows that are not counted."""
    from mm2d3d_amd import pselab

    dev = _dev()
    x2, x3 = _walk_logits(C)
    a, b = torch.from_numpy(x2).to(dev), torch.from_numpy(x3).to(dev)
    what = f"the walk, C {C} ens {ens}"
    ad, ref = pselab.AdaptiveThreshold(C, momentum=0.5, device=dev), AdaptiveRef(C, momentum=0.5)
    out = ad.labels(a, b, ensemble=ens, with_probs=True)
    ref.update(x2, x3, ensemble=ens)
    _state_close(ad, ref, out["threshold"], what)
    _check_against_predict(a, b, ens, out, what)
    # the counted rows, through a momentum-0 update: tau is then the mean confidence over exactly those rows
    z = pselab.AdaptiveThreshold(C, momentum=0.0, device=dev)
    z.update(a, b, ensemble=ens)
    refused = ([131100, 131200], [131100, 131200] if ens else [131100])
    for o, (name, bad) in enumerate(zip(("2d", "3d"), refused)):
        good = torch.ones(WALK_N, dtype=torch.bool, device=dev)
        good[bad] = False
        assert all(int(out[f"label_{name}"][i]) == -100 for i in bad)
        err = abs(float(z.state[o, 0]) - float(out[f"prob_{name}"].double()[good].mean()))
        print(f"{what}: output {o}: |tau - mean confidence of the {int(good.sum())} counted rows| {err:.2e}")
        assert err <= 1e-12  # WALK_N - len(bad) rows, not one more or fewer
    # two objects fed the same call end with equal bits
    again = pselab.AdaptiveThreshold(C, momentum=0.5, device=dev)
    thr = again.update(a, b, ensemble=ens)
    assert torch.equal(_bits(again.state), _bits(ad.state)) and torch.equal(again.count, ad.count)
    assert torch.equal(_bits(thr), _bits(out["threshold"]))


def test_row_pitched_views_are_read_in_place_past_nan_padding():
    from mm2d3d_amd import pselab

    dev = _dev()
    N, C = 129, 6
    a0, b0 = _pair(C, N, dev)
    wide_a = torch.full((N, 8), float("nan"), device=dev)
    wide_b = torch.full((N, 11), float("nan"), device=dev)
    wide_a[:, 1 : 1 + C], wide_b[:, 5 : 5 + C] = a0, b0
    a, b = wide_a[:, 1 : 1 + C], wide_b[:, 5 : 5 + C]
    assert a.stride(0) == 8 and b.stride(0) == 11 and not a.is_contiguous()
    for ens in (False, True):
        x, y = pselab.AdaptiveThreshold(C, momentum=0.5, device=dev), pselab.AdaptiveThreshold(C, momentum=0.5, device=dev)
        got, want = x.labels(a, b, ensemble=ens, with_probs=True), y.labels(a0, b0, ensemble=ens, with_probs=True)
        for k in want:
            assert torch.equal(_bits(got[k]), _bits(want[k])), (ens, k)
        assert torch.equal(_bits(x.state), _bits(y.state)) and bool(torch.isfinite(x.state).all()) and x.count.tolist() == [1, 1]
        assert 0 < int(got["kept"].min()) and int(got["kept"].max()) < N


@pytest.mark.parametrize("N,C", [(129, 5), (1000, 32), (1, 1), (0, 6)])
def test_state_count_and_thresholds_stay_inside_guard_padded_buffers(N, C):
    """Through the C ABI: the three outputs as slices of larger buffers whose other words must keep their bits."""
    from mm2d3d_amd import _lib, pselab
    from mm2d3d_amd._lib import check, ptr, stream

    dev = _dev()
    a, b = _pair(C, N, dev) if N else (torch.empty((0, C), device=dev),) * 2
    L = _lib.lib()
    ws = torch.empty(int(L.mm_pl_adapt_ws_bytes()), dtype=torch.uint8, device=dev)
    for ens in (0, 1):
        sbuf = torch.full((2 * (1 + C) + 2 * GUARD,), -7.25, dtype=torch.float64, device=dev)
        cbuf = torch.full((2 + 2 * GUARD,), 0x1234567, dtype=torch.int64, device=dev)
        tbuf = torch.full((2 * C + 2 * GUARD,), -3.5, dtype=torch.float32, device=dev)
        ss, cs, ts = sbuf[GUARD : GUARD + 2 * (1 + C)], cbuf[GUARD : GUARD + 2], tbuf[GUARD : GUARD + 2 * C]
        ss.fill_(1.0 / C), cs.zero_()
        s0, c0, t0 = sbuf.clone(), cbuf.clone(), tbuf.clone()
        check(L.mm_pl_adapt(ptr(a), C, ptr(b), C, N, C, ens, 0.5, 0, ptr(ss), ptr(cs), ptr(ts), ptr(ws), ws.numel(), stream()), "pl_adapt")
        want = pselab.AdaptiveThreshold(C, momentum=0.5, device=dev)
        thr = want.update(a, b, ensemble=bool(ens))
        assert torch.equal(_bits(ss), _bits(want.state.reshape(-1))) and torch.equal(cs, want.count) and torch.equal(_bits(ts), _bits(thr.reshape(-1)))
        for buf, old, n in ((sbuf, s0, 2 * (1 + C)), (cbuf, c0, 2), (tbuf, t0, 2 * C)):
            assert torch.equal(_bits(buf[:GUARD]), _bits(old[:GUARD])) and torch.equal(_bits(buf[GUARD + n :]), _bits(old[GUARD + n :]))
        if N == 0:  # only the update runs: it sees no row, the state stays and the thresholds are written
            assert torch.equal(_bits(ss), _bits(s0[GUARD : GUARD + 2 * (1 + C)])) and cs.tolist() == [0, 0]
            assert torch.equal(ts, torch.full((2 * C,), 1.0 / C, dtype=torch.float64).to(torch.float32).to(dev))


def test_an_empty_batch():
    from mm2d3d_amd import pselab

    dev = _dev()
    ad = pselab.AdaptiveThreshold(6, momentum=0.5, device=dev)
    ad.update(*_pair(6, 64, dev))
    state, count = ad.state.clone(), ad.count.clone()
    e = torch.empty((0, 6), device=dev)
    out = ad.labels(e, e, with_probs=True)
    assert out["label_2d"].shape == (0,) and out["prob_3d"].shape == (0,) and out["kept"].tolist() == [0, 0]
    assert torch.equal(_bits(ad.state), _bits(state)) and torch.equal(ad.count, count)
    assert _ulps(out["threshold"].cpu().numpy(), _thr_of_state(state)) <= 1


# ---------------------------------------------------------------------------------------------- the per-class soft-tail pair
def _tail_ref_cls(x64, ta, tb, T, thr):
    """float64, as test_gpu_ce_soft._tail_ref with one threshold per class: (loss, K * d loss / d logits, K, smallest distance of a
    confidence to its threshold)."""
    p = torch.softmax(ta.double(), 1)
    if tb is not None:
        p = 0.5 * (p + torch.softmax(tb.double(), 1))
    finite = torch.isfinite(p).all(1)
    conf, y = torch.where(finite[:, None], p, torch.zeros_like(p)).max(1)
    t = thr.double()[y]
    keep = finite & (conf >= t)
    dist = float((conf - t)[finite].abs().min())
    K = int(keep.sum())
    grad = torch.zeros_like(x64)
    if K == 0:
        return 0.0, grad, 0, dist
    q = torch.softmax(ta[keep].double() / T, 1)
    if tb is not None:
        q = 0.5 * (q + torch.softmax(tb[keep].double() / T, 1))
    x = x64[keep].clone().requires_grad_(True)
    loss = -(q * torch.log_softmax(x, 1)).sum(1).mean()
    loss.backward()
    grad[keep] = x.grad * K
    return loss.item(), grad, K, dist


@pytest.mark.parametrize("name", ["777_300_20", "256_0_6", "129_1_32", "pitched", "nonfinite", "nonfinite_own"])
def test_soft_pair_with_one_value_for_every_class_is_the_scalar_call(name):
    import test_gpu_ce_soft as S

    c, dev = S._case(name), _dev()
    for thr in (0.6, 0.9) if c["thr"] is None else (c["thr"],):
        want = S._run(c, dev, threshold=thr)
        got = S._run(c, dev, threshold=torch.full((c["C"],), thr, dtype=torch.float32, device=dev))
        print(f"{name} thr {thr}: kept {got[3]} of {c['N'] - c['P']}")
        assert got[3] == want[3], (name, thr, got[3], want[3])
        for g, w in zip(got[:3], want[:3]):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (name, thr)


@pytest.mark.parametrize("name", ["777_300_6", "777_300_20", "129_1_32", "pitched", "nonfinite", "nonfinite_own", "300001_150000_6"])
def test_soft_pair_with_distinct_thresholds(name):
    """kept == the count pselab.predict's float32 confidences and classes give, exactly; loss and gradient against float64 at the
    tolerances of tests/test_gpu_ce_soft.py (losses 1e-5 * max(1, |ref|), the gradient times K at 1e-5 absolute)."""
    import test_gpu_ce_soft as S
    from mm2d3d_amd import pselab

    c, dev = S._case(name), _dev()
    C, P, ens = c["C"], c["P"], c["tb"] is not None
    thr = torch.linspace(0.35, 0.8, C, dtype=torch.float32) if C > 1 else torch.tensor([0.5])
    ref = pselab.predict(c["ta"].to(dev), c["tb"].to(dev) if ens else None)
    p, y = (ref["probs_ensemble"], ref["pseudo_label_ensemble"]) if ens else (ref["probs_2d"], ref["pseudo_label_2d"])
    want_kept = int((p >= thr.to(dev)[y.long()]).sum())
    lh, lt, grad, kept = S._run(c, dev, threshold=thr.to(dev))
    print(f"{name}: kept {kept} of {c['N'] - P} tail rows")
    assert kept == want_kept, (name, kept, want_kept)
    if c["N"] > 1000:  # the tile loop at more tiles than workgroups: the exact count is the check (among 150001 confidences one
        return  # may lie within float32 rounding of its threshold, which a float64 gate could decide the other way)
    r1, g1, K, dist = _tail_ref_cls(c["x"][P:].double(), c["ta"], c["tb"], c["T"], thr)
    print(f"{name}: kept {kept} (float64: {K}) of {c['N'] - P}, smallest |confidence - threshold| {dist:.2e}, tail {lt.item():.7f} ref {r1:.7f}")
    assert dist > 1e-6 and kept == K  # (no row this close to its threshold: the float32 gate keeps the reference's rows)
    assert S._close(lt.item(), r1) and S._close(lh.item(), c["ref"][0])
    err = (grad[P:].double() * K - g1).abs().max().item()
    head = (grad[:P].double() * c["sum_w"][0] - c["grad"][:P]).abs().max().item() if P else 0.0
    print(f"{name}: max |K * dgrad| {err:.2e}, head {head:.2e}")
    assert err <= 1e-5 and head <= 1e-5


def test_soft_pair_refuses_a_threshold_tensor_of_the_wrong_kind():
    from mm2d3d_amd.losses import cross_entropy_soft_pair

    dev = _dev()
    x, t = torch.zeros(4, 6, device=dev), torch.zeros(2, 6, device=dev)
    for bad in (torch.zeros(5, device=dev), torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(6), torch.zeros(1, 6, device=dev)):
        with pytest.raises(ValueError, match="threshold"):
            cross_entropy_soft_pair(x, 2, None, t, threshold=bad)
    assert math.isfinite(float(cross_entropy_soft_pair(x, 2, None, t, threshold=torch.zeros(6, device=dev))[1]))
