"""losses.cross_entropy_soft_pair (csrc/loss.hip k_ce2s_*): head rows [0, P) against labels as cross_entropy_pair, tail rows [P, N)
against a teacher's softened distribution, gated by the teacher's confidence - against torch float64 on the CPU, on the same fp32
inputs (x, ta, tb each 3 * randn, seeded).

Tolerances are those of test_gpu_ce_pair.py: losses within 1e-5 * max(1, |ref|); gradients are multiplied by the segment's weight
sum (K, the kept rows, for the tail) and compared at 1e-5 absolute (torch's own fp32 against fp64 on such inputs: at most 2.6e-7
on the loss and 5.2e-7 on the scaled gradient).  The reference gates in float64; every case asserts that no row's float64
confidence lies within 1e-6 of the threshold, so the float32 gate of the kernel must keep exactly the reference's rows."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

W6 = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]  # config.yaml class weights
# name: (N, P, C, T, threshold, ensemble, kind)
CASES = {
    "777_300_6": (777, 300, 6, 1.0, None, False, "plain"),
    "777_300_20": (777, 300, 20, 0.5, 0.9, True, "plain"),
    "256_0_6": (256, 0, 6, 2.0, 0.6, False, "plain"),  # unlabelled head
    "512_512_6": (512, 512, 6, 2.0, 0.6, True, "plain"),  # empty tail
    "1_0_6": (1, 0, 6, 0.5, None, False, "plain"),  # a single row
    "129_1_32": (129, 1, 32, 1.0, 0.6, True, "plain"),  # the largest C; one row past two 64-row tiles (one 128-row tile)
    "128_0_2": (128, 0, 2, 2.0, 0.9, True, "plain"),
    "300001_150000_6": (300001, 150000, 6, 1.0, 0.6, True, "plain"),  # more tiles than workgroups: the tile loop runs
    "pitched": (777, 300, 6, 2.0, 0.6, True, "pitched"),  # all three matrices are views of NaN-padded C + 2 wide tensors
    "nonfinite": (777, 300, 6, 1.0, None, True, "nonfinite"),  # a few teacher rows inf / NaN: never kept, zero gradient rows
    "nonfinite_own": (777, 300, 6, 2.0, None, False, "nonfinite"),
    "out_of_range": (777, 300, 6, 1.0, 0.6, False, "out_of_range"),  # a few head labels >= C: skipped like ignore_index
}
BAD_ROWS = (0, 7, 63, 64, 400)  # tail rows of the "nonfinite" cases
BAD_LABELS = (5, 17, 130)  # head rows of the "out_of_range" case


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def _class_weights(C):
    return [W6[c % 6] for c in range(C)]


def _head_ref(x64, y, w):
    """float64 F.cross_entropy of the head and, per row, sum_w * d loss / d logits (test_gpu_ce_pair._segment_ref)."""
    y = y.clone()
    y[(y < 0) | (y >= x64.shape[1])] = -100
    wt = torch.tensor(w, dtype=torch.float64)
    valid = y != -100
    sum_w = float(wt[y[valid]].sum())
    if x64.shape[0] == 0 or not bool(valid.any()):
        return float("nan"), torch.zeros_like(x64), sum_w
    x = x64.clone().requires_grad_(True)
    v = F.cross_entropy(x, y, weight=wt, ignore_index=-100)
    v.backward()
    return v.item(), x.grad * sum_w, sum_w


def _confidence64(ta, tb):
    p = torch.softmax(ta.double(), 1)
    if tb is not None:
        p = 0.5 * (p + torch.softmax(tb.double(), 1))
    return p.max(1).values  # NaN for a row with non-finite logits


def _tail_ref(x64, ta, tb, T, thr):
    """float64: (loss, K * d loss / d logits, K, smallest distance of a confidence to the threshold)."""
    n = x64.shape[0]
    if n == 0:
        return 0.0, torch.zeros_like(x64), 0, float("inf")
    conf = _confidence64(ta, tb)
    keep = conf >= (0.0 if thr is None else thr)  # a NaN confidence compares false
    dist = float((conf[torch.isfinite(conf)] - thr).abs().min()) if thr is not None else float("inf")
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


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded inputs and the float64 reference of a case: computed once, shared by the tests, never modified."""
    N, P, C, T, thr, ens, kind = CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    x = 3 * torch.randn(N, C, generator=g)
    ta = 3 * torch.randn(N - P, C, generator=g)
    tb = 3 * torch.randn(N - P, C, generator=g) if ens else None
    y0 = torch.randint(0, C, (P,), generator=g)
    y0[torch.rand(P, generator=g) < 0.05] = -100
    if P:
        y0[0] = 1  # never a head with rows and nothing counted
    if kind == "out_of_range":
        y0[BAD_LABELS[0]], y0[BAD_LABELS[1]], y0[BAD_LABELS[2]] = C, C + 7, 1 << 40
    if kind == "nonfinite":
        ta[BAD_ROWS[0], 2] = float("inf")
        ta[BAD_ROWS[1], 0] = float("nan")
        ta[BAD_ROWS[2]] = float("nan")
        if ens:
            tb[BAD_ROWS[3], 1] = float("nan")
            tb[BAD_ROWS[4], 5] = float("inf")
        else:
            ta[BAD_ROWS[3], 1] = float("nan")
            ta[BAD_ROWS[4]] = float("inf")
    w = _class_weights(C)
    r0, g0, sw0 = _head_ref(x[:P].double(), y0, w)
    r1, g1, K, dist = _tail_ref(x[P:].double(), ta, tb, T, thr)
    return dict(name=name, N=N, P=P, C=C, T=T, thr=thr, kind=kind, x=x, ta=ta, tb=tb, y0=y0, w=w, ref=(r0, r1), grad=torch.cat([g0, g1], 0),
                sum_w=(sw0, K), K=K, dist=dist)


def _wide(t, dev, leaf=False):
    """``t`` on the device as a view of a NaN-padded tensor two columns wider."""
    wide = torch.full((t.shape[0], t.shape[1] + 2), float("nan"))
    wide[:, : t.shape[1]] = t
    wide = wide.to(dev)
    if leaf:
        wide.requires_grad_(True)
    return wide, wide[:, : t.shape[1]]


def _run(c, dev, scale=(1.0, 1.0), **kw):
    from mm2d3d_amd.losses import cross_entropy_soft_pair

    pitched = c["kind"] == "pitched"
    if pitched:
        leaf, pred = _wide(c["x"], dev, leaf=True)
        ta = _wide(c["ta"], dev)[1]
        tb = _wide(c["tb"], dev)[1] if c["tb"] is not None else None
        assert pred.stride() == (c["C"] + 2, 1) and ta.stride() == (c["C"] + 2, 1)
    else:
        leaf = pred = c["x"].to(dev).requires_grad_(True)
        ta, tb = c["ta"].to(dev), (c["tb"].to(dev) if c["tb"] is not None else None)
    args = dict(weight_head=c["w"], temperature=c["T"], threshold=c["thr"])
    args.update(kw)
    lh, lt, kept = cross_entropy_soft_pair(pred, c["P"], c["y0"], ta, tb, **args)
    live = [s * v for s, v in zip(scale, (lh, lt)) if math.isfinite(v.item())]  # (an empty head is 0/0: nothing to differentiate)
    sum(live).backward()
    grad = leaf.grad[:, : c["C"]] if pitched else leaf.grad
    assert kept.dtype == torch.int64 and kept.is_cuda and not kept.requires_grad
    return lh.detach().cpu(), lt.detach().cpu(), grad.detach().cpu(), int(kept)


def _close(got, ref):
    if math.isnan(ref):
        return math.isnan(got)
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


@pytest.mark.parametrize("name", list(CASES))
def test_values_gradients_and_kept_rows_match_float64_torch(name):
    c = _case(name)
    print(f"{name}: smallest |confidence - threshold| {c['dist']:.2e}, reference keeps {c['K']} of {c['N'] - c['P']} rows")
    assert c["dist"] > 1e-6  # (choose another seed if a row ever lies this close: the float32 gate could then differ)
    lh, lt, grad, kept = _run(c, _dev())
    P = c["P"]
    scaled = torch.cat([grad[:P].double() * c["sum_w"][0], grad[P:].double() * c["sum_w"][1]], 0)
    err = (scaled - c["grad"]).abs().max().item()
    print(f"{name}: head {lh.item():.7f} ref {c['ref'][0]:.7f}  tail {lt.item():.7f} ref {c['ref'][1]:.7f}  kept {kept} ref {c['K']}  "
          f"max |sum_w * dgrad| {err:.2e}")
    assert kept == c["K"]
    assert _close(lh.item(), c["ref"][0]) and _close(lt.item(), c["ref"][1])
    assert err <= 1e-5
    if c["kind"] == "out_of_range":
        assert torch.equal(grad[list(BAD_LABELS)], torch.zeros(3, c["C"]))
    if c["kind"] == "nonfinite":
        assert kept == c["N"] - P - len(BAD_ROWS)  # every other row is kept: there is no threshold
        assert torch.equal(grad[[P + r for r in BAD_ROWS]], torch.zeros(len(BAD_ROWS), c["C"]))
        assert bool(torch.isfinite(grad).all())
    if c["N"] == P:
        assert lt.item() == 0.0 and kept == 0


@pytest.mark.parametrize("name", ["777_300_6", "777_300_20", "129_1_32", "300001_150000_6", "nonfinite", "nonfinite_own"])
def test_kept_is_the_count_of_teacher_labels(name):
    """Both judge a row by the same float32 expression (csrc/pointpred.h): the counts agree exactly, at any threshold."""
    from mm2d3d_amd import pselab
    from mm2d3d_amd.losses import cross_entropy_soft_pair

    c, dev = _case(name), _dev()
    ens = c["tb"] is not None
    ta = c["ta"].to(dev)
    tb = c["tb"].to(dev) if ens else (3 * torch.randn(c["ta"].shape, generator=torch.Generator().manual_seed(7))).to(dev)
    x = c["x"].to(dev)
    for thr in (None, 0.5, 0.6, 0.9, 0.99):
        want = pselab.teacher_labels(ta, tb, ensemble=ens, threshold=thr)["kept"]
        # "own": kept[0] judges ta alone.  No threshold: teacher_labels keeps the rows without a confidence too, the loss cannot
        finite = int(torch.isfinite(_confidence64(c["ta"], c["tb"])).sum())
        kept = cross_entropy_soft_pair(x, c["P"], None, ta, tb if ens else None, threshold=thr)[2]
        assert int(kept) == (finite if thr is None else int(want[0])), (name, thr)


@pytest.mark.parametrize("name", ["777_300_6", "300001_150000_6"])
def test_the_same_call_twice_is_bit_identical(name):
    c, dev = _case(name), _dev()
    a, b = _run(c, dev), _run(c, dev)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)
    assert a[3] == b[3]


def test_upstream_gradients_reach_their_own_segment():
    """2 * head + 4 * tail: powers of two scale a row's factor exactly, so each segment's rows are the unit rows times its own."""
    c, dev = _case("777_300_6"), _dev()
    P = c["P"]
    unit, scaled = _run(c, dev)[2], _run(c, dev, scale=(2.0, 4.0))[2]
    assert bool((unit[:P] != 0).any()) and bool((unit[P:] != 0).any())
    assert torch.equal(scaled[:P], 2 * unit[:P]) and torch.equal(scaled[P:], 4 * unit[P:])


@pytest.mark.parametrize("name", ["777_300_6", "777_300_20"])
def test_threshold_one_keeps_nothing_and_leaves_the_head_alone(name):
    c, dev = _case(name), _dev()
    P = c["P"]
    assert float(_confidence64(c["ta"], c["tb"]).max()) < 1.0 - 1e-6
    lh0, _, g0, k0 = _run(c, dev, threshold=None)
    lh, lt, g, k = _run(c, dev, threshold=1.0)
    assert k == 0 and k0 == c["N"] - P
    assert lt.item() == 0.0 and torch.equal(g[P:], torch.zeros(c["N"] - P, c["C"]))
    assert lh.item() == lh0.item() and torch.equal(g[:P], g0[:P])  # bit for bit


def test_hard_limit_is_cross_entropy_pair():
    """A teacher of 1000 * one_hot(y): its softmax is exactly one-hot in fp32, so the soft tail is the hard tail."""
    from mm2d3d_amd.losses import cross_entropy_pair, cross_entropy_soft_pair

    c, dev = _case("777_300_6"), _dev()
    N, P, C = c["N"], c["P"], c["C"]
    y = torch.randint(0, C, (N - P,), generator=torch.Generator().manual_seed(5))
    teacher = 1000.0 * F.one_hot(y, C).float()
    assert torch.equal(torch.softmax(teacher, 1), F.one_hot(y, C).float())
    for kw in (dict(), dict(temperature=2.0, threshold=0.99), dict(teacher_other=teacher.to(dev))):
        a = c["x"].to(dev).requires_grad_(True)
        b = c["x"].to(dev).requires_grad_(True)
        hh, ht = cross_entropy_pair(a, P, c["y0"], y, weight_head=c["w"])
        (hh + ht).backward()
        sh, st, kept = cross_entropy_soft_pair(b, P, c["y0"], teacher.to(dev), weight_head=c["w"], **kw)
        (sh + st).backward()
        assert int(kept) == N - P
        assert _close(sh.item(), hh.item()) and _close(st.item(), ht.item())
        ga, gb = a.grad.double().cpu(), b.grad.double().cpu()
        assert ((ga[:P] - gb[:P]).abs().max() * c["sum_w"][0]).item() <= 1e-5
        assert ((ga[P:] - gb[P:]).abs().max() * (N - P)).item() <= 1e-5


def test_soft_limit_is_the_kl_plus_the_entropy_of_the_target():
    """T = 1, no threshold, own target: sum_c q_c (lse - x_c) = KL(q || softmax(x)) + H(q), and H(q) has no gradient."""
    from mm2d3d_amd.losses import cross_entropy_soft_pair, kl_to_detached

    c, dev = _case("777_300_6"), _dev()
    N, P = c["N"], c["P"]
    assert c["T"] == 1.0 and c["thr"] is None and c["tb"] is None
    a = c["x"].to(dev).requires_grad_(True)
    b = c["x"].to(dev).requires_grad_(True)
    kl = kl_to_detached(a[P:], c["ta"].to(dev))
    kl.backward()
    _, st, kept = cross_entropy_soft_pair(b, P, None, c["ta"].to(dev))
    st.backward()
    q = torch.softmax(c["ta"].double(), 1)
    entropy = float(-(q * torch.log_softmax(c["ta"].double(), 1)).sum(1).mean())
    assert int(kept) == N - P
    assert _close(st.item(), kl.item() + entropy)
    assert ((a.grad[P:] - b.grad[P:]).double().abs().max() * (N - P)).item() <= 1e-5
    assert torch.equal(b.grad[:P], torch.zeros_like(b.grad[:P]))


def test_the_gradient_comes_from_a_single_autograd_node():
    """Structure: above ``pred`` the graph of loss_head + loss_tail has ONE node (one backward launch writes the whole gradient)."""
    from mm2d3d_amd.losses import cross_entropy_soft_pair

    c, dev = _case("777_300_6"), _dev()
    x = c["x"].to(dev).requires_grad_(True)
    lh, lt, kept = cross_entropy_soft_pair(x, c["P"], c["y0"], c["ta"].to(dev), weight_head=c["w"])
    total = lh + lt
    above = {fn for fn, _ in total.grad_fn.next_functions if fn is not None}
    assert len(above) == 1 and kept.grad_fn is None
    node = above.pop()
    assert "CrossEntropySoftPair" in type(node).__name__
    below = [fn for fn, _ in node.next_functions if fn is not None]
    assert len(below) == 1 and type(below[0]).__name__ == "AccumulateGrad" and below[0].variable is x


def test_argument_errors():
    from mm2d3d_amd.losses import cross_entropy_soft_pair

    dev = _dev()
    x = torch.zeros(10, 6, device=dev)
    t = torch.zeros(6, 6, device=dev)
    y = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="split"):
        cross_entropy_soft_pair(x, 11, None, t)
    with pytest.raises(ValueError, match="split"):
        cross_entropy_soft_pair(x, -1, None, t)
    with pytest.raises(ValueError, match="teacher"):
        cross_entropy_soft_pair(x, 5, None, t)  # 6 rows for a tail of 5
    with pytest.raises(ValueError, match="teacher"):
        cross_entropy_soft_pair(x, 4, None, torch.zeros(6, 5, device=dev))
    with pytest.raises(ValueError, match="teacher_other"):
        cross_entropy_soft_pair(x, 4, None, t, torch.zeros(5, 6, device=dev))
    with pytest.raises(ValueError, match="teacher"):
        cross_entropy_soft_pair(x, 10, None, t)  # an empty tail takes a [0, C] teacher
    with pytest.raises(ValueError, match="classes"):
        cross_entropy_soft_pair(torch.zeros(10, 33, device=dev), 4, None, torch.zeros(6, 33, device=dev))
    for T in (0.0, -1.0, float("nan"), float("inf"), None, "1"):
        with pytest.raises(ValueError, match="temperature"):
            cross_entropy_soft_pair(x, 4, None, t, temperature=T)
    for thr in (0.0, -0.1, 1.5, float("nan"), "median", True):
        with pytest.raises(ValueError, match="threshold"):
            cross_entropy_soft_pair(x, 4, None, t, threshold=thr)
    with pytest.raises(ValueError, match="gt_head"):
        cross_entropy_soft_pair(x, 5, y, torch.zeros(5, 6, device=dev))
    with pytest.raises(ValueError, match="weight_head"):
        cross_entropy_soft_pair(x, 4, y, t, weight_head=[1.0, 2.0])
    lh, lt, kept = cross_entropy_soft_pair(x, 10, None, torch.zeros(0, 6, device=dev))  # the empty tail itself is legal
    torch.cuda.synchronize()
    assert lh.item() == 0.0 and lt.item() == 0.0 and int(kept) == 0
