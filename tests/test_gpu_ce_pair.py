"""losses.cross_entropy_pair (csrc/loss.hip k_ce_*<2>): two cross entropies over the rows [0, P) and [P, N) of one logits tensor
against torch's float64 ``F.cross_entropy`` on the CPU, per segment, on the same fp32 logits.

Tolerances: losses within 1e-5 * max(1, |ref|) (that of test_cross_entropy_matches_reference_golden).  Gradients are compared
after multiplying both sides by the segment's weight sum, so a row's scale does not depend on N: 1e-5 absolute (fp32 softmax
carries a few ulp: torch's own fp32 against fp64 on these inputs differs by at most 8e-7)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

W6 = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]  # config.yaml class weights
CASES = {
    "777_300_6": (777, 300, 6, "plain"),
    "777_300_20": (777, 300, 20, "plain"),
    "256_0_6": (256, 0, 6, "plain"),
    "512_512_6": (512, 512, 6, "plain"),
    "1_0_6": (1, 0, 6, "plain"),
    "300001_150000_6": (300001, 150000, 6, "plain"),  # more than T * MAX_PART = 262144 rows: the grid-stride loop runs
    "pitched": (777, 300, 6, "pitched"),  # a row-pitched view, ld = C + 2
    "out_of_range": (777, 300, 6, "out_of_range"),  # a few labels >= C: skipped like ignore_index
}


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def _class_weights(C):
    return [W6[c % 6] for c in range(C)]  # the six weights of config.yaml, repeated where a case has more classes


def _segment_ref(x64, y, w):
    """float64 F.cross_entropy of one segment and, per row, sum_w * d loss / d logits.  An empty tail is defined as loss 0."""
    y = y.clone()
    y[(y < 0) | (y >= x64.shape[1])] = -100
    x = x64.clone().requires_grad_(True)
    wt = None if w is None else torch.tensor(w, dtype=torch.float64)
    valid = y != -100
    sum_w = float(valid.sum()) if wt is None else float(wt[y[valid]].sum())
    if x.shape[0] == 0 or not bool(valid.any()):
        return float("nan"), torch.zeros_like(x64), sum_w
    v = F.cross_entropy(x, y, weight=wt, ignore_index=-100)
    v.backward()
    return v.item(), x.grad * sum_w, sum_w


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded inputs and the float64 reference of a case: computed once, shared by the tests, never modified."""
    N, P, C, kind = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    x = 3 * torch.randn(N, C, generator=g)
    y0 = torch.randint(0, C, (P,), generator=g)
    y0[torch.rand(P, generator=g) < 0.05] = -100
    y1 = torch.randint(0, C, (N - P,), generator=g)
    y1[torch.rand(N - P, generator=g) < 0.5] = -100
    for y in (y0, y1):
        if len(y):
            y[0] = 1  # never a segment with rows and nothing counted: those cases are tested on their own below
    if kind == "out_of_range":
        y0[5], y0[17], y1[3], y1[100] = C, C + 7, C, 1 << 40
    w = _class_weights(C)
    r0, g0, sw0 = _segment_ref(x[:P].double(), y0, w)
    r1, g1, sw1 = _segment_ref(x[P:].double(), y1, None)
    if N == P:
        r1 = 0.0  # the rule of zero_if_empty=(False, True): a tail in which nothing counts is loss 0
    return dict(N=N, P=P, C=C, kind=kind, x=x, y0=y0, y1=y1, w=w, ref=(r0, r1), grad=torch.cat([g0, g1], 0), sum_w=(sw0, sw1))


def _pred(c, dev):
    """The case's logits on the device as a leaf (or, pitched, a view of a wider leaf)."""
    if c["kind"] == "pitched":
        wide = torch.full((c["N"], c["C"] + 2), float("nan"))
        wide[:, : c["C"]] = c["x"]
        leaf = wide.to(dev).requires_grad_(True)
        return leaf, leaf[:, : c["C"]]
    leaf = c["x"].to(dev).requires_grad_(True)
    return leaf, leaf


def _run(c, dev, **kw):
    from mm2d3d_amd.losses import cross_entropy_pair

    leaf, pred = _pred(c, dev)
    lh, lt = cross_entropy_pair(pred, c["P"], c["y0"], c["y1"], weight_head=c["w"], **kw)
    live = [v for v in (lh, lt) if math.isfinite(v.item())]  # (an empty head is 0/0, as mm_ce_fwd: nothing to differentiate)
    sum(live).backward()
    grad = leaf.grad[:, : c["C"]] if c["kind"] == "pitched" else leaf.grad
    return lh.detach().cpu(), lt.detach().cpu(), grad.detach().cpu()


def _close(got, ref):
    if math.isnan(ref):
        return math.isnan(got)
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_gradients_match_float64_torch(name):
    c = _case(name)
    lh, lt, grad = _run(c, _dev())
    P = c["P"]
    scaled = torch.cat([grad[:P].double() * c["sum_w"][0], grad[P:].double() * c["sum_w"][1]], 0)
    err = (scaled - c["grad"]).abs().max().item() if c["N"] else 0.0
    print(f"{name}: head {lh.item():.7f} ref {c['ref'][0]:.7f}  tail {lt.item():.7f} ref {c['ref'][1]:.7f}  max |sum_w * dgrad| {err:.2e}")
    assert _close(lh.item(), c["ref"][0]) and _close(lt.item(), c["ref"][1])
    assert err <= 1e-5
    if c["kind"] == "out_of_range":
        bad = torch.tensor([5, 17, P + 3, P + 100])
        assert torch.equal(grad[bad], torch.zeros(4, c["C"]))


@pytest.mark.parametrize("name", ["777_300_6", "300001_150000_6"])
def test_the_same_call_twice_is_bit_identical(name):
    c, dev = _case(name), _dev()
    a, b = _run(c, dev), _run(c, dev)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_upstream_gradients_reach_their_own_segment():
    """2 * head + 4 * tail: powers of two scale a row's factor exactly, so each segment's rows are the unit rows times its own."""
    from mm2d3d_amd.losses import cross_entropy_pair

    c, dev = _case("777_300_6"), _dev()
    _, _, unit = _run(c, dev)
    x = c["x"].to(dev).requires_grad_(True)
    lh, lt = cross_entropy_pair(x, c["P"], c["y0"], c["y1"], weight_head=c["w"])
    (2 * lh + 4 * lt).backward()
    assert torch.equal(x.grad[: c["P"]].cpu(), 2 * unit[: c["P"]]) and torch.equal(x.grad[c["P"]:].cpu(), 4 * unit[c["P"]:])


@pytest.mark.parametrize("name", ["777_300_6", "300001_150000_6"])
def test_one_segment_over_all_rows_agrees_with_cross_entropy(name):
    """Bit for bit: k_ce_*<1> and k_ce_*<2> are one template, and over one labelled segment they run the same arithmetic."""
    from mm2d3d_amd.losses import cross_entropy, cross_entropy_pair

    c, dev = _case(name), _dev()
    N = c["N"]
    y = torch.cat([c["y0"], c["y1"]])
    a = c["x"].to(dev).requires_grad_(True)
    b = c["x"].to(dev).requires_grad_(True)
    one = cross_entropy(a, y, c["w"])
    one.backward()
    lh, lt = cross_entropy_pair(b, N, y, None, weight_head=c["w"])
    (lh + lt).backward()
    assert lt.item() == 0.0
    assert torch.equal(lh.detach(), one.detach())
    assert torch.equal(a.grad, b.grad)


def test_an_unlabelled_segment_has_zero_gradient_rows():
    from mm2d3d_amd.losses import cross_entropy_pair

    c, dev = _case("777_300_6"), _dev()
    P = c["P"]
    _, lt_ref, g_ref = _run(c, dev)
    x = c["x"].to(dev).requires_grad_(True)
    lh, lt = cross_entropy_pair(x, P, None, c["y1"])
    (lh + lt).backward()
    assert lh.item() == 0.0 and lt.item() == lt_ref.item()
    assert torch.equal(x.grad[:P].cpu(), torch.zeros(P, c["C"])) and torch.equal(x.grad[P:].cpu(), g_ref[P:])


def test_a_tail_of_ignored_labels_is_loss_zero_and_leaves_the_head_alone():
    """Deviation from F.cross_entropy (nan): zero_if_empty=(False, True) is the default; (False, False) gives torch's nan."""
    from mm2d3d_amd.losses import cross_entropy_pair

    c, dev = _case("777_300_6"), _dev()
    P = c["P"]
    lh_ref, _, g_ref = _run(c, dev)
    gone = torch.full_like(c["y1"], -100)
    x = c["x"].to(dev).requires_grad_(True)
    lh, lt = cross_entropy_pair(x, P, c["y0"], gone, weight_head=c["w"])
    (lh + lt).backward()
    assert lt.item() == 0.0 and lh.item() == lh_ref.item()
    assert torch.equal(x.grad[P:].cpu(), torch.zeros(c["N"] - P, c["C"])) and torch.equal(x.grad[:P].cpu(), g_ref[:P])
    lh2, lt2 = cross_entropy_pair(c["x"].to(dev), P, c["y0"], gone, weight_head=c["w"], zero_if_empty=(False, False))
    assert math.isnan(lt2.item()) and lh2.item() == lh_ref.item()
    assert math.isnan(F.cross_entropy(c["x"][P:], gone).item())


def test_the_gradient_comes_from_a_single_autograd_node():
    """Structure: above ``pred`` the graph of loss_head + loss_tail has ONE node (one backward launch writes the whole gradient) -
    no slice, zero-fill, copy or add node assembles it."""
    from mm2d3d_amd.losses import cross_entropy_pair

    c, dev = _case("777_300_6"), _dev()
    x = c["x"].to(dev).requires_grad_(True)
    lh, lt = cross_entropy_pair(x, c["P"], c["y0"], c["y1"], weight_head=c["w"])
    total = lh + lt
    above = {fn for fn, _ in total.grad_fn.next_functions if fn is not None}
    assert len(above) == 1
    node = above.pop()
    assert "CrossEntropyPair" in type(node).__name__
    below = [fn for fn, _ in node.next_functions if fn is not None]
    assert len(below) == 1 and type(below[0]).__name__ == "AccumulateGrad" and below[0].variable is x


def test_argument_errors():
    from mm2d3d_amd.losses import cross_entropy_pair

    dev = _dev()
    x = torch.zeros(10, 6, device=dev)
    y = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="split"):
        cross_entropy_pair(x, 11, None, None)
    with pytest.raises(ValueError, match="gt_tail"):
        cross_entropy_pair(x, 5, None, y)
    with pytest.raises(ValueError, match="weight_head"):
        cross_entropy_pair(x, 4, y, None, weight_head=[1.0, 2.0])
    torch.cuda.synchronize()
