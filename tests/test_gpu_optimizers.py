"""GPU parity of the flat SGD / Adam / RMSprop / AdamW updates (csrc/optim.hip) with the reference's own registry entries:
``torch.optim.<Class>`` in fp32 on the CPU.  Envelope: the project's own for AdamW, atol 2e-6 + rtol 1e-6 (torch's fp32
optimisers drift from its fp64 ones by < 8e-7 on these inputs over 12 steps, so the reference alone sits well inside it)."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(6,), (3, 1), (1,), (1037,), (16, 6), (6,), (5000,)]
ATOL, RTOL = 2e-6, 1e-6

# (id, flat class, torch class, hyper-parameters)
CASES = [
    ("sgd", "FlatSGD", "SGD", dict(lr=0.01)),
    ("sgd_momentum_wd", "FlatSGD", "SGD", dict(lr=0.01, momentum=0.9, weight_decay=0.05)),
    ("sgd_nesterov", "FlatSGD", "SGD", dict(lr=0.01, momentum=0.9, weight_decay=0.05, nesterov=True)),
    ("sgd_dampening", "FlatSGD", "SGD", dict(lr=0.01, momentum=0.9, dampening=0.3)),
    ("adam_wd", "FlatAdam", "Adam", dict(lr=0.01, weight_decay=0.05)),
    ("adam_amsgrad", "FlatAdam", "Adam", dict(lr=0.01, weight_decay=0.05, amsgrad=True)),
    ("adamw_amsgrad", "FlatAdamW", "AdamW", dict(lr=0.01, weight_decay=0.05, amsgrad=True)),
    ("rmsprop", "FlatRMSprop", "RMSprop", dict()),
    ("rmsprop_momentum_wd", "FlatRMSprop", "RMSprop", dict(momentum=0.9, weight_decay=0.05)),
    ("rmsprop_centered", "FlatRMSprop", "RMSprop", dict(momentum=0.9, weight_decay=0.05, centered=True)),
]
IDS = [c[0] for c in CASES]
# AdamW without amsgrad keeps the host counter under step(skip_words=): it joins every test but the one on that counter
ADAMW = ("adamw", "FlatAdamW", "AdamW", dict(lr=0.01, weight_decay=0.05))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def _pair(flat, ref, kw, dev, seed=11):
    """The same parameters on the GPU under the flat class and on the CPU under torch's; parameter 0 never receives a gradient."""
    from mm2d3d_amd import optimizers

    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    hp = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    rp = [torch.nn.Parameter(t.clone()) for t in init]
    return g, init, hp, rp, getattr(optimizers, flat)(hp, **kw), getattr(torch.optim, ref)(rp[1:], **kw)


def _backward(g, hp, rp, o, r, dev, scale=None):
    ws = [torch.randn(s, generator=g) for s in SHAPES]
    o.zero_grad(), r.zero_grad()
    lh = sum((p * w.to(dev)).sum() for p, w in zip(hp[1:], ws[1:]))
    (lh if scale is None else scale(lh)).backward()
    sum((p * w).sum() for p, w in zip(rp[1:], ws[1:])).backward()


def _assert_close(hp, rp, init, what):
    assert torch.equal(hp[0].detach().cpu(), init[0]), what
    for i, (a, b) in enumerate(zip(hp[1:], rp[1:])):
        err = float((a.detach().cpu() - b.detach()).abs().max())
        assert torch.allclose(a.detach().cpu(), b.detach(), atol=ATOL, rtol=RTOL), (what, i + 1, err)


def _snapshot(o):
    a = o._arenas[0]
    return {n: a[n].clone() for n in ("p",) + a["state"]}


def _assert_frozen(o, snap, what):
    a = o._arenas[0]
    assert set(snap) == {"p"} | set(a["state"]), what
    for n, t in snap.items():
        assert torch.equal(a[n], t), (what, n)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "loss_scaled"])
@pytest.mark.parametrize("case", CASES + [ADAMW], ids=IDS + [ADAMW[0]])
def test_four_steps_match_torch_on_a_touched_range_that_starts_unaligned(case, scaled):
    """An untouched 6-element parameter ahead of the touched ones: the touched range starts at arena offset 6 (not 16-byte
    aligned), so the scalar instantiations of k_optim run; every element is updated exactly once per step."""
    from mm2d3d_amd.amp import GradScaler

    _, flat, ref, kw = case
    dev = _dev()
    g, init, hp, rp, o, r = _pair(flat, ref, kw, dev)
    scaler = GradScaler(dev, init_scale=1024.0) if scaled else None
    for step in range(4):
        _backward(g, hp, rp, o, r, dev, scaler.scale if scaled else None)
        if scaled:
            scaler.step(o)
            scaler.update()
        else:
            o.step()
        r.step()
        lo = o._touched_ranges(o._arenas[0])[0][0]
        assert lo == 6 and (o._arenas[0]["p"][lo:].data_ptr() & 15) != 0  # the case under test
        _assert_close(hp, rp, init, step)
    if scaled:
        assert scaler.steps_taken(o) == 4
    assert o.state_dict()["step"] == 4


def test_aligned_ranges_and_ragged_tails_take_the_vector_path_and_match_torch():
    """All parameters touched: the range starts at the 16-byte aligned arena base (vector instantiation), 6149 elements = 6 full
    blocks of 1024 + a block whose second thread owns a single element (scalar tail)."""
    dev = _dev()
    for _, flat, ref, kw in (CASES[3], CASES[5], CASES[9], ADAMW):
        from mm2d3d_amd import optimizers

        g = torch.Generator().manual_seed(11)
        init = [torch.randn(s, generator=g) for s in SHAPES]
        hp = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        rp = [torch.nn.Parameter(t.clone()) for t in init]
        o, r = getattr(optimizers, flat)(hp, **kw), getattr(torch.optim, ref)(rp, **kw)
        assert o._arenas[0]["p"].numel() == 6149 and o._arenas[0]["p"].data_ptr() % 16 == 0
        for step in range(3):
            ws = [torch.randn(s, generator=g) for s in SHAPES]
            o.zero_grad(), r.zero_grad()
            sum((p * w.to(dev)).sum() for p, w in zip(hp, ws)).backward()
            sum((p * w).sum() for p, w in zip(rp, ws)).backward()
            o.step(), r.step()
            assert o._touched_ranges(o._arenas[0]) == [[0, 6149]]
            for i, (a, b) in enumerate(zip(hp, rp)):
                assert torch.allclose(a.detach().cpu(), b.detach(), atol=ATOL, rtol=RTOL), (flat, step, i)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_set_skip_word_freezes_everything_and_does_not_use_up_the_first_step(case):
    _, flat, ref, kw = case
    dev = _dev()
    g, init, hp, rp, o, r = _pair(flat, ref, kw, dev)
    word = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    _backward(g, hp, rp, o, r, dev)
    snap = _snapshot(o)
    o.step(skip_words=word)
    _assert_frozen(o, snap, "first step skipped")
    word.zero_()
    o.step(skip_words=word)  # torch's FIRST step: bias corrections of step 1, SGD's buf = g without dampening
    r.step()
    _assert_close(hp, rp, init, "step after the skipped one")
    # a skipped step between taken ones, state arrays now nonzero; then a plain step continues from the device counter
    _backward(g, hp, rp, o, r, dev)
    snap = _snapshot(o)
    word[0] = 7
    o.step(skip_words=word)
    _assert_frozen(o, snap, "second step skipped")
    o.step()
    r.step()
    _assert_close(hp, rp, init, "second step")
    assert o.state_dict()["step"] == 2


def test_skip_words_of_the_plain_entry_points():
    """skip_dev / nskip of mm_sgd_step / mm_adam_step (also as AdamW: decoupled = 1, vmax = NULL) / mm_rmsprop_step themselves: any
    nonzero word makes the launch a no-op."""
    from mm2d3d_amd import _lib
    from mm2d3d_amd._lib import check, ptr, stream

    dev = _dev()
    L = _lib.lib()
    torch.manual_seed(0)
    n = 3001
    p, g, s0, s1, s2 = (torch.randn(n, device=dev).abs() for _ in range(5))
    s1 *= 0.1  # (RMSprop centered: sq - gavg^2 stays positive)
    for words in ([0, 0, 5], [0, 0, 0]):
        w = torch.tensor(words, dtype=torch.int32, device=dev)
        before = [t.clone() for t in (p, s0, s1, s2)]
        check(L.mm_sgd_step(ptr(p), ptr(g), ptr(s0), n, 0.1, 0.9, 0.0, 0.0, 0, 2, 1.0, ptr(w), 3, stream()), "sgd")
        check(L.mm_adam_step(ptr(p), ptr(g), ptr(s0), ptr(s1), ptr(s2), n, 0.1, 0.9, 0.999, 1e-8, 0.0, 0, 1, 1.0, ptr(w), 3, stream()), "adam")
        check(L.mm_rmsprop_step(ptr(p), ptr(g), ptr(s0), ptr(s1), ptr(s2), n, 0.1, 0.99, 1e-8, 0.0, 0.9, 1.0, ptr(w), 3, stream()), "rms")
        check(L.mm_adam_step(ptr(p), ptr(g), ptr(s0), ptr(s1), None, n, 0.1, 0.9, 0.999, 1e-8, 0.01, 1, 1, 1.0, ptr(w), 3, stream()), "adamw")
        same = [torch.equal(a, b) for a, b in zip(before, (p, s0, s1, s2))]
        assert same == [any(words)] * 4, (words, same)


def test_adamw_without_amsgrad_keeps_the_host_counter_under_skip_words():
    """FlatAdamW without amsgrad takes step(skip_words=) as a plain launch: the device skips the update, the HOST counter
    advances all the same, and no device state of the device-counted form is created."""
    _, flat, ref, kw = ADAMW
    dev = _dev()
    g, init, hp, rp, o, r = _pair(flat, ref, kw, dev)
    assert not o._skips_on_device
    word = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    _backward(g, hp, rp, o, r, dev)
    snap = _snapshot(o)
    o.step(skip_words=word)
    _assert_frozen(o, snap, "first step skipped")
    word.zero_()
    o.step(skip_words=word)
    assert not torch.equal(o._arenas[0]["p"], snap["p"])  # the second step is taken
    assert o.state_dict()["step"] == 2
    assert o._own is None


def _adamw_bits_module():
    spec = importlib.util.spec_from_file_location("make_golden_adamw_bits", os.path.join(GOLDEN, "make_golden_adamw_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_adamw_without_amsgrad_is_bit_identical_with_the_retired_kernel():
    """tests/golden/adamw_bits.npz pins the bits of the AdamW update (no amsgrad): p, m, v after steps 1 and 4, recorded on an
    MI355X by tests/golden/make_golden_adamw_bits.py at commit 93edc00, where a kernel of its own in csrc/loss.hip did this update.
    Four runs: plain and loss-scaled, on the whole arena (aligned base, a block of 1024 + a block whose sixth thread owns 3
    elements) and on the range from offset 6 (unaligned: scalar instantiation, 1041 elements, a one-element tail).
    k_optim<ADAM, ADAM_DECOUPLED> must give the same bits.  Measured with the coefficients passed as an OptCoef by value: steps 1
    and every loss-scaled run identical; plain runs after step 4 differ on the scalar path only (range from offset 6: 20 / 461 /
    249 of 1047 elements of p / m / v, p by 1 - 4 ulp; whole arena: 1 / 2 elements of m / v among its last three).  k_optim
    therefore takes the plain step's coefficients as scalar kernel arguments, which gives the old kernel's instruction sequence
    in gfx950 assembly; that build has not yet been run against this fixture on a GPU."""
    mod = _adamw_bits_module()
    gold = np.load(os.path.join(GOLDEN, "adamw_bits.npz"))
    dev = _dev()
    seen_keys = set()
    for key, scaled, first, ranges in mod.RUNS:
        out, seen = mod.run(dev, scaled, first)
        assert len(seen) == 4
        for touched, misalign in seen:  # the case under test
            assert touched == ranges, (key, touched)
            assert (misalign == 0) == (first == 0), (key, misalign)
        assert sorted(out) == sorted(f"step{k}_{n}" for k in (1, 4) for n in ("p", "m", "v")), key
        for name, t in out.items():
            want = torch.from_numpy(gold[f"{key}_{name}"])
            assert want.dtype == torch.float32 and want.shape == (1047,)
            assert torch.equal(t, want), (key, name, int((t != want).sum()))
            seen_keys.add(f"{key}_{name}")
    assert seen_keys == set(gold.files) and len(seen_keys) == 24


def test_an_overflow_skips_sgd_and_adam_together_and_the_next_step_is_step_one():
    from mm2d3d_amd.amp import GradScaler

    dev = _dev()
    gs, init_s, hs, rs, osgd, rsgd = _pair("FlatSGD", "SGD", dict(lr=0.01, momentum=0.9, dampening=0.3), dev)
    ga, init_a, ha, ra, oadam, radam = _pair("FlatAdam", "Adam", dict(lr=0.01, weight_decay=0.05), dev, seed=12)
    sc = GradScaler(dev, init_scale=1024.0)
    _backward(gs, hs, rs, osgd, rsgd, dev, sc.scale)
    _backward(ga, ha, ra, oadam, radam, dev, sc.scale)
    oadam.grad_arenas()[0][1500] = float("inf")
    snaps = _snapshot(osgd), _snapshot(oadam)
    sc.step_all([osgd, oadam])
    sc.update()
    _assert_frozen(osgd, snaps[0], "sgd, overflow in adam's gradients")
    _assert_frozen(oadam, snaps[1], "adam, overflow")
    assert sc.steps_taken(osgd) == 0 and sc.steps_taken(oadam) == 0 and sc.get_scale() == 512.0
    _backward(gs, hs, rs, osgd, rsgd, dev, sc.scale)
    _backward(ga, ha, ra, oadam, radam, dev, sc.scale)
    sc.step_all([osgd, oadam])
    sc.update()
    rsgd.step(), radam.step()
    _assert_close(hs, rs, init_s, "sgd step 1")
    _assert_close(ha, ra, init_a, "adam step 1")
    assert sc.steps_taken(osgd) == 1 and sc.steps_taken(oadam) == 1 and sc.get_scale() == 512.0


def test_sgd_under_one_cycle_follows_torch_lr_momentum_and_parameters():
    from mm2d3d_amd.optimizers import Optimizer

    dev = _dev()
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    hp = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    rp = [torch.nn.Parameter(t.clone()) for t in init]
    o, s = Optimizer("sgd", lr=0.01, momentum=0.9).set_scheduler("one_cycle", max_lr=0.05, total_steps=10).build(hp)
    r = torch.optim.SGD(rp[1:], lr=0.01, momentum=0.9)
    rs = torch.optim.lr_scheduler.OneCycleLR(r, max_lr=0.05, total_steps=10)
    for step in range(8):
        assert abs(o.param_groups[0]["lr"] - r.param_groups[0]["lr"]) < 1e-12
        assert abs(o.param_groups[0]["momentum"] - r.param_groups[0]["momentum"]) < 1e-12
        _backward(g, hp, rp, o, r, dev)
        o.step(), r.step()
        s.step(), rs.step()
        _assert_close(hp, rp, init, step)
    assert o.param_groups[0]["momentum"] != 0.9 and o.param_groups[0]["lr"] != 0.01


def test_trainer_with_sgd_for_2d_and_adam_for_3d_under_the_loss_scale_and_its_checkpoint():
    """``2d_net: sgd``, ``3d_net: adam`` at ``precision: 16`` (fp16 maps + the device-resident loss scale): two steps run, both
    optimisers take both, the 2D parameters carry gradient sinks (the captured-graph path is eligible), and a checkpoint resumed
    in a fresh trainer continues bit for bit.

    "Every parameter that has a gradient moved" after step 1: the first update of a weight w with unscaled gradient g is
    lr*|g| under SGD (buf = g) and lr*|g| / (|g| + eps) under Adam (the bias corrections cancel on step 1); it changes w in
    fp32 whenever it is at least one ulp of w, so every touched parameter with such an element must differ from its initial
    value (a gradient that is zero up to rounding, e.g. of a bias in front of a batch norm, may legitimately leave w as it is)."""
    from mm2d3d_amd import nn2d, scn
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg
    from mm2d3d_amd.optimizers import FlatAdam, FlatSGD, Optimizer
    from mm2d3d_amd.synthetic import make_batch
    from mm2d3d_amd.train import TrainModel

    dev = _dev()
    torch.manual_seed(0)
    kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
    W = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]
    n2, n3 = Net2DSeg(6, pretrained=False).to(dev), Net3DSeg(6, True, kw).to(dev)
    for m in n2.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    n2b, n3b = copy.deepcopy(n2), copy.deepcopy(n3)
    mk = lambda: {"source": make_batch(5, 1, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (48, 64), device=dev)}
    loss = Loss([{"name": "cross_entropy", "target": "segmentation", "args": {"weight": W}}])
    opts = lambda: {"2d_net": Optimizer("sgd", lr=1e-3, momentum=0.9), "3d_net": Optimizer("adam", lr=1e-3)}
    tk = dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, precision=16, gc_freeze=False)
    try:
        tm = TrainModel({"2d_net": n2, "3d_net": n3}, opts(), loss, dict(tk))
        tm.configure_optimizers()
        osgd, oadam = tm.optimizers
        assert type(osgd) is FlatSGD and type(oadam) is FlatAdam
        assert all(hasattr(p, "_mm_sink") for p in n2.parameters())  # what graph2d asks for before it captures the trunk
        init = [a["p"].clone() for o in tm.optimizers for a in o._arenas]
        losses = [float(tm.fit_step(mk()).detach())]
        assert tm.scaler is not None
        scale = tm.scaler.get_scale()
        n_must = n_touched = 0
        for o, p0 in zip(tm.optimizers, init):
            a, lr = o._arenas[0], o.param_groups[0]["lr"]
            gabs = a["g"].abs() / scale
            delta = lr * gabs if o is osgd else lr * gabs / (gabs + o.param_groups[0]["eps"])
            must = delta >= torch.nextafter(p0.abs(), torch.full_like(p0, float("inf"))) - p0.abs()
            for t, (lo, hi) in zip(a["touched"], a["spans"]):
                if t:
                    n_touched += 1
                    if bool(must[lo:hi].any()):
                        n_must += 1
                        assert not torch.equal(a["p"][lo:hi], p0[lo:hi]), (type(o).__name__, lo, hi)
        print(f"touched parameters: {n_touched}, with a representable first update: {n_must}")
        assert n_touched > 300 and n_must >= 0.75 * n_touched
        losses.append(float(tm.fit_step(mk()).detach()))
        assert all(np.isfinite(v) for v in losses), losses
        assert [tm.scaler.steps_taken(o) for o in tm.optimizers] == [2, 2]
        ck = tm.checkpoint()
        assert [sd["step"] for sd in ck["optimizer_states"]] == [2, 2]
        assert set(ck["optimizer_states"][0]["flat"][0]) == {"buf"} and set(ck["optimizer_states"][1]["flat"][0]) == {"m", "v"}
        fresh = TrainModel({"2d_net": n2b, "3d_net": n3b}, opts(), loss, dict(tk))
        fresh.load_checkpoint(ck)
        la, lb = float(tm.fit_step(mk()).detach()), float(fresh.fit_step(mk()).detach())
        assert la == lb, (la, lb)
        torch.cuda.synchronize()
        for x, y in zip(tm.optimizers, fresh.optimizers):
            xa, ya = x._arenas[0], y._arenas[0]
            assert xa["state"] == ya["state"]
            for n in ("p",) + xa["state"]:
                assert torch.equal(xa[n], ya[n]), (type(x).__name__, n)
    finally:
        nn2d.set_precision(nn2d.DEFAULT_PRECISION)
        scn.set_activation_dtype(torch.float32)
