"""Gradient clipping of the flat optimisers (csrc/clip.hip, mm2d3d_amd/clip.py): the norm kernels against float64 numpy, the joint
clip of several optimisers, four clipped steps against ``torch.nn.utils.clip_grad_norm_ / clip_grad_value_`` +
``torch.optim.<Class>`` in fp32 on the CPU, and the interplay with the device-resident loss scale.

Envelope of the comparisons with torch: the project's own for the optimisers, atol 2e-6 + rtol 1e-6 (tests/test_gpu_optimizers.py),
widened only where torch's fp32 run itself leaves it against a float64 run (test_four_clipped_steps_match_torch says where)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(6,), (3, 1), (1,), (1037,), (16, 6), (6,), (5000,)]
ATOL, RTOL = 2e-6, 1e-6

# the ten hyper-parameter cases of tests/test_gpu_optimizers.py: (id, flat class, torch class, hyper-parameters)
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


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def _within_ulps(got, want64, ulps=2):
    want = np.float32(want64)
    return abs(float(np.float32(got)) - float(want)) <= ulps * float(np.spacing(want))


def _sgd_over(sizes, dev, seed, groups=1, fill=None):
    """A FlatSGD (lr = 1) over zero weights of the given sizes, split into ``groups`` parameter groups; every gradient arena holds
    seeded normal numbers (or ``fill``) and every parameter counts as touched."""
    from mm2d3d_amd.optimizers import FlatSGD

    ps = [torch.nn.Parameter(torch.zeros(n, device=dev)) for n in sizes]
    per = (len(ps) + groups - 1) // groups
    o = FlatSGD([{"params": ps[i : i + per]} for i in range(0, len(ps), per)], lr=1.0)
    gen = torch.Generator().manual_seed(seed)
    for g in o.grad_arenas():
        g.copy_(torch.randn(g.numel(), generator=gen) if fill is None else torch.full((g.numel(),), fill))
    o.mark_all_touched()
    return o


def _host_norm(opts):
    return float(np.linalg.norm(np.concatenate([g.cpu().numpy().astype(np.float64) for o in opts for g in o.grad_arenas()])))


@pytest.mark.parametrize("sizes", [[6149], [1], [(1 << 20) + 3]], ids=["6149", "1", "2^20+3"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "loss_scaled"])
def test_total_norm_equals_the_float64_norm_and_is_the_same_bits_twice(sizes, scaled):
    """One workgroup with a ragged tail (6149 = 1537 float4s + 1), a single element (tail only), and 2^20 + 3 elements: 256
    workgroups, both reduction stages, a tail of 3.  The sum is carried in double, so the bound is the final conversions: 2 ulp."""
    from mm2d3d_amd.amp import GradScaler
    from mm2d3d_amd.clip import clip_grad_norm_

    dev = _dev()
    o = _sgd_over(sizes, dev, seed=3)
    scaler, gs = (GradScaler(dev, init_scale=1024.0), 0.25) if scaled else (None, 1.0)
    want = _host_norm([o]) * gs / (1024.0 if scaled else 1.0)
    a = clip_grad_norm_(o, 1.0, scaler=scaler, grad_scale=gs)
    b = clip_grad_norm_([o], 1.0, scaler=scaler, grad_scale=gs)
    assert a.device.type == "cuda" and a.dtype == torch.float32 and a.dim() == 0
    print(f"norm {float(a)!r}, float64 {want!r}")
    assert _within_ulps(float(a), want), (float(a), want)
    assert a.view(torch.int32).item() == b.view(torch.int32).item()


def test_untouched_head_of_the_optimizer_test_layout_and_unaligned_ranges():
    """The layout of tests/test_gpu_optimizers.py: a 6-element parameter that never receives a gradient ahead of 6143 touched
    elements - it holds zeros and contributes nothing (torch's ``grad is None`` rule).  The arena itself is 16-byte aligned, so the
    kernel's scalar head is driven directly: ranges that start 1, 2 and 3 elements (and 6: the touched range) past a boundary, of
    lengths below one float4, ragged and more than one chunk; every element is read exactly once."""
    from mm2d3d_amd import _lib
    from mm2d3d_amd._lib import check, ptr, stream
    from mm2d3d_amd.clip import clip_grad_norm_
    from mm2d3d_amd.optimizers import FlatSGD

    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    hp = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in SHAPES]
    o = FlatSGD(hp, lr=1.0)
    ws = [torch.randn(s, generator=gen) for s in SHAPES]
    sum((p * w.to(dev)).sum() for p, w in zip(hp[1:], ws[1:])).backward()
    g = o.grad_arenas()[0]
    assert g.numel() == 6149 and o._touched_ranges(o._arenas[0]) == [[6, 6149]] and float(g[:6].abs().max()) == 0.0
    want = float(np.linalg.norm(np.concatenate([w.numpy().reshape(-1).astype(np.float64) for w in ws[1:]])))
    assert _within_ulps(float(clip_grad_norm_(o, 1.0)), want)

    L = _lib.lib()
    buf = torch.randn(3 * 4096 * 4 + 64, generator=gen).to(dev)
    assert buf.data_ptr() % 16 == 0
    one = torch.ones(1, device=dev)
    out = torch.zeros(2, device=dev)
    for off in (0, 1, 2, 3, 6):
        for n in (1, 2, 3, 5, 6143, 2 * 4096 * 4 + 7):
            v = buf[off : off + n]
            k = int(L.mm_grad_sqnorm_ws_bytes(n)) // 8
            part = torch.full((k + 1,), -1.0, dtype=torch.float64, device=dev)
            check(L.mm_grad_sqnorm(ptr(v), n, ptr(part), 0, None, stream()), "grad_sqnorm")
            counts = np.array([k], dtype=np.int64)
            check(L.mm_clip_finalize(ptr(part), counts.ctypes.data, 1, ptr(one), 1.0, 1.0, ptr(out[0:1]), ptr(out[1:2]), stream()), "fin")
            assert float(part[k]) == -1.0, "a partial was written past the arena's own"
            want = float(np.linalg.norm(v.cpu().numpy().astype(np.float64)))
            assert _within_ulps(float(out[0]), want), (off, n, float(out[0]), want)


def test_joint_norm_over_two_optimizers_one_of_them_with_two_groups_and_a_finite_norm_of_huge_gradients():
    from mm2d3d_amd.amp import GradScaler
    from mm2d3d_amd.clip import clip_grad_norm_

    dev = _dev()
    a, b = _sgd_over([700, 33, 4100], dev, seed=5, groups=2), _sgd_over([5001], dev, seed=6)
    assert len(a.grad_arenas()) == 2 and len(b.grad_arenas()) == 1
    sc = GradScaler(dev, init_scale=1024.0)
    n1, n2 = clip_grad_norm_([a, b], 1.0, scaler=sc, grad_scale=0.5), clip_grad_norm_([a, b], 1.0, scaler=sc, grad_scale=0.5)
    assert _within_ulps(float(n1), _host_norm([a, b]) * 0.5 / 1024.0)
    assert n1.view(torch.int32).item() == n2.view(torch.int32).item()
    # 1e25 squared leaves fp32's range; the sum of 2^20 + 3 such squares (1e56) is nothing to a double
    huge = _sgd_over([(1 << 20) + 3], dev, seed=0, fill=1e25)
    n = float(clip_grad_norm_(huge, 1.0))
    assert np.isfinite(n) and _within_ulps(n, float(np.float64(np.float32(1e25)) * np.sqrt(float((1 << 20) + 3))))


@pytest.mark.parametrize("max_norm", [0.5, 10.0])
def test_two_sgd_optimizers_are_clipped_by_one_joint_norm(max_norm):
    """lr = 1, no momentum, no decay: the step IS the clipped gradient.  Each optimiser's own norm is 0.4 < 0.5, the joint norm is
    0.4 * sqrt(2) > 0.5 - clipping each on its own would leave both untouched and the step at 0.566."""
    from mm2d3d_amd.clip import clip_grad_norm_

    dev = _dev()
    opts = [_sgd_over([1000], dev, seed=1), _sgd_over([400, 377], dev, seed=2, groups=2)]
    for o in opts:
        own = _host_norm([o])
        for g in o.grad_arenas():
            g.mul_(0.4 / own)
    own, joint = [_host_norm([o]) for o in opts], _host_norm(opts)
    assert all(abs(v - 0.4) < 1e-6 for v in own) and joint > 0.5 and max(own) < 0.5
    w0 = [a["p"].clone() for o in opts for a in o._arenas]
    norm = clip_grad_norm_(opts, max_norm)
    for o in opts:
        o.step()
    dw = float(torch.cat([(a["p"].double() - w.double()) for a, w in zip([a for o in opts for a in o._arenas], w0)]).norm())
    want = min(max_norm, joint)
    print(f"max_norm {max_norm}: |dw| {dw!r}, want {want!r}, norm {float(norm)!r}")
    assert abs(float(norm) - joint) <= 1e-6 * joint
    assert abs(dw - want) <= 1e-5 * want
    for o in opts:
        assert o._clip_scale is None and o.state_dict()["step"] == 1


def test_what_is_not_supported_raises():
    from mm2d3d_amd.clip import clip_grad_norm_, clip_grad_value_

    dev = _dev()
    o = _sgd_over([8], dev, seed=0)
    plain = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3, device=dev))], lr=1.0)
    with pytest.raises(TypeError):
        clip_grad_norm_([o, plain], 1.0)
    with pytest.raises(TypeError):
        clip_grad_value_(plain, 1.0)
    for bad in (1, float("inf"), 2.5):
        with pytest.raises(NotImplementedError):
            clip_grad_norm_(o, 1.0, norm_type=bad)


# ------------------------------------------------------------------------------------------------------ against torch
def _pair(flat, ref, kw, dev, seed=11):
    """The same parameters on the GPU under the flat class and on the CPU under torch's; parameter 0 never receives a gradient."""
    from mm2d3d_amd import optimizers

    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    hp = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    rp = [torch.nn.Parameter(t.clone()) for t in init]
    return g, init, hp, rp, getattr(optimizers, flat)(hp, **kw), getattr(torch.optim, ref)(rp[1:], **kw)


def _backward(g, hp, rp, o, r, dev, scale=None, f64=None):
    """``f64``: (parameters, optimiser) of a float64 CPU run of the same recipe, fed the same numbers."""
    ws = [torch.randn(s, generator=g) for s in SHAPES]
    o.zero_grad(), r.zero_grad()
    lh = sum((p * w.to(dev)).sum() for p, w in zip(hp[1:], ws[1:]))
    (lh if scale is None else scale(lh)).backward()
    sum((p * w).sum() for p, w in zip(rp[1:], ws[1:])).backward()  # the reference's gradients are the unscaled ones
    if f64 is not None:
        f64[1].zero_grad()
        sum((p * w.double()).sum() for p, w in zip(f64[0][1:], ws[1:])).backward()


def _assert_close(hp, rp, init, what, floor=0.0):
    """|w - w_torch| <= max(2e-6 + 1e-6 |w_torch|, floor) element by element; returns the largest difference."""
    assert torch.equal(hp[0].detach().cpu(), init[0]), what
    worst = 0.0
    for i, (a, b) in enumerate(zip(hp[1:], rp[1:])):
        diff = (a.detach().cpu() - b.detach()).abs()
        worst = max(worst, float(diff.max()))
        assert bool((diff <= torch.clamp(ATOL + RTOL * b.detach().abs(), min=floor)).all()), (what, i + 1, float(diff.max()), floor)
    return worst


@pytest.mark.parametrize("algo", ["norm", "value"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "loss_scaled"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_four_clipped_steps_match_torch(case, scaled, algo):
    """unscale -> torch.nn.utils.clip_grad_norm_ / clip_grad_value_ -> torch.optim.<Class>.step in fp32 on the CPU, beside the flat
    optimiser with the clip functions (plain) or GradScaler(init_scale=1024).step(clip=) (loss-scaled).  The gradients are 6143
    standard normal numbers (norm about 78, a quarter of them beyond +-1.15): max_norm = 1 and clip_value = 1.15 clip on
    every step, which the CPU side asserts.

    Envelope: the project's 2e-6 + 1e-6 |w|, except where torch's own fp32 run is further than that from a float64 CPU run of the
    same recipe (same numbers, same calls, parameters and gradients in double), which the test runs beside it: there twice that
    deviation, taken after each step as the largest over all elements.  It is needed for RMSprop with weight decay under the norm
    clip only: clipped to norm 1 the gradients are about 0.013 against 0.05 |w| of decay, their sum passes near zero for some
    elements, and g / (sqrt(sq) + eps) then magnifies the last-bit differences of g.  Measured on the CPU: fp32 against float64
    2.9e-6, 5.5e-6, 7.3e-6, 7.9e-6 after steps 1..4 for rmsprop_momentum_wd (rmsprop_centered: 2.9e-6 .. 8.0e-6), at most 8.3e-7 for
    every other case and for the value clip throughout - those stay inside the plain envelope.  The kernels play no part in the
    figure (on an MI355X they came to 5.9e-6 of torch's fp32 weights after step 4 of the two RMSprop cases, 4.1e-6 after step 2)."""
    from mm2d3d_amd.amp import GradScaler
    from mm2d3d_amd.clip import clip_grad_norm_, clip_grad_value_

    _, flat, ref, kw = case
    dev = _dev()
    g, init, hp, rp, o, r = _pair(flat, ref, kw, dev)
    dp = [torch.nn.Parameter(t.clone().double()) for t in init]
    d = getattr(torch.optim, ref)(dp[1:], **kw)
    scaler = GradScaler(dev, init_scale=1024.0) if scaled else None
    bound, active, worst = (1.0, 0, 0.0) if algo == "norm" else (1.15, 0, 0.0)
    for step in range(4):
        _backward(g, hp, rp, o, r, dev, scaler.scale if scaled else None, f64=(dp, d))
        (torch.nn.utils.clip_grad_norm_ if algo == "norm" else torch.nn.utils.clip_grad_value_)(dp[1:], bound)
        d.step()
        if algo == "norm":
            ref_norm = float(torch.nn.utils.clip_grad_norm_(rp[1:], bound))
            active += ref_norm > bound
        else:
            active += max(float(p.grad.abs().max()) for p in rp[1:]) > bound
            torch.nn.utils.clip_grad_value_(rp[1:], bound)
        if scaled:
            scaler.step(o, clip=(algo, bound))
            scaler.update()
            norm = scaler.last_grad_norm
        else:
            norm = clip_grad_norm_(o, bound) if algo == "norm" else clip_grad_value_(o, bound)
            o.step()
        r.step()
        if algo == "norm":
            assert abs(float(norm) - ref_norm) <= 2e-6 * ref_norm, (float(norm), ref_norm)  # torch's own norm is an fp32 sum
        cpu_dev = max(float((a.detach().double() - b.detach()).abs().max()) for a, b in zip(rp[1:], dp[1:]))
        err = _assert_close(hp, rp, init, step, floor=2.0 * cpu_dev)
        print(f"{case[0]} {algo} {'scaled' if scaled else 'plain'} step {step}: |w - w_torch| {err:.3e}, torch fp32 - float64 {cpu_dev:.3e}")
        worst = max(worst, err)
    assert active >= 3
    if scaled:
        assert scaler.steps_taken(o) == 4 and scaler.get_scale() == 1024.0
    assert o.state_dict()["step"] == 4


def test_clipped_adamw_takes_the_device_coefficient_form_and_matches_torch():
    """FlatAdamW without amsgrad keeps its counter on the host in plain steps; a clipped step runs as mm_adam_prepare +
    mm_adam_step_dev (decoupled decay) with the optimiser's own device counter."""
    from mm2d3d_amd.clip import clip_grad_norm_

    dev = _dev()
    g, init, hp, rp, o, r = _pair("FlatAdamW", "AdamW", dict(lr=0.01, weight_decay=0.05), dev)
    for step in range(3):
        _backward(g, hp, rp, o, r, dev)
        torch.nn.utils.clip_grad_norm_(rp[1:], 1.0)
        clip_grad_norm_(o, 1.0)
        o.step()
        assert o._dev_step is not None
        r.step()
        _assert_close(hp, rp, init, step)
    _backward(g, hp, rp, o, r, dev)  # an unclipped plain step continues from the device counter
    o.step(), r.step()
    _assert_close(hp, rp, init, "plain step after clipped ones")
    assert o.state_dict()["step"] == 4


# ------------------------------------------------------------------------------------------------------ with the loss scale
def _two_under_a_scaler(dev):
    from mm2d3d_amd.amp import GradScaler

    a = _pair("FlatSGD", "SGD", dict(lr=0.01, momentum=0.9, dampening=0.3), dev)
    b = _pair("FlatAdam", "Adam", dict(lr=0.01, weight_decay=0.05), dev, seed=12)
    sc = GradScaler(dev, init_scale=1024.0)
    for t in (a, b):
        _backward(t[0], t[2], t[3], t[4], t[5], dev, sc.scale)
    return a, b, sc


def _snapshot(o):
    a = o._arenas[0]
    return {n: a[n].clone() for n in ("p",) + a["state"]}


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_one_inf_skips_both_clipped_optimizers_and_halves_the_scale(algo):
    dev = _dev()
    a, b, sc = _two_under_a_scaler(dev)
    osgd, oadam = a[4], b[4]
    oadam.grad_arenas()[0][1500] = float("inf")
    snaps = _snapshot(osgd), _snapshot(oadam)
    sc.step_all([osgd, oadam], clip=(algo, 1.0))
    sc.update()
    for o, snap in zip((osgd, oadam), snaps):
        for n, t in snap.items():
            assert torch.equal(o._arenas[0][n], t), (type(o).__name__, n)
    assert sc.steps_taken(osgd) == 0 and sc.steps_taken(oadam) == 0 and sc.get_scale() == 512.0


def test_a_clip_that_does_not_bite_leaves_the_loss_scaled_step_bit_identical():
    """max_norm = 1e30: c = 1 and the effective scale is scale / 1, the scale's own bits."""
    dev = _dev()
    a, b, sc = _two_under_a_scaler(dev)
    a2, b2, sc2 = _two_under_a_scaler(dev)
    for step in range(2):
        if step:
            for t, s in ((a, sc), (b, sc), (a2, sc2), (b2, sc2)):
                _backward(t[0], t[2], t[3], t[4], t[5], dev, s.scale)
        sc.step_all([a[4], b[4]], clip=1e30)
        sc2.step_all([a2[4], b2[4]])
        sc.update(), sc2.update()
        assert float(sc.last_grad_norm) > 1.0 and sc2.last_grad_norm is None
        for x, y in ((a[4], a2[4]), (b[4], b2[4])):
            sx, sy = _snapshot(x), _snapshot(y)
            assert set(sx) == set(sy)
            for n in sx:
                assert torch.equal(sx[n], sy[n]), (type(x).__name__, n, step)
    assert sc.steps_taken(a[4]) == 2 and sc.steps_taken(b[4]) == 2
