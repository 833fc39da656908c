"""GPU parity: HIP sparse operators (through the C-ABI) vs the CPU oracle on identical seeded inputs.

Bar (BASELINE.json north_star): integer voxel / rulebook indices bit-exact under the canonical
order of SURVEY.md A.8; fp32 features / logits / gradients within 1e-3 (stated per test).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scn_ref  # noqa: E402
from oracle.net3d_ref import Net3DSegRef  # noqa: E402

ATOL = 1e-3


def _dev():
    import mm2d3d_amd  # noqa: F401  (fails loudly when libmm2d3d_hip.so is missing)

    return torch.device("cuda:0")


def _random_sparse(seed, S=24, B=3, n=600, C=3, dup=True):
    g = np.random.default_rng(seed)
    coords = np.concatenate([g.integers(0, S, (n, 3)), g.integers(0, B, (n, 1))], 1).astype(np.int64)
    if dup:
        coords = np.concatenate([coords, coords[g.integers(0, n, n // 3)]], 0)
    feats = torch.from_numpy(g.standard_normal((len(coords), C)).astype(np.float32))
    return torch.from_numpy(coords), feats


def _close(a, b, tol=ATOL, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    scale = max(1.0, b.abs().max().item() if b.numel() else 1.0)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


def _lidar_batch(n_scenes=2):
    from mm2d3d_amd.synthetic import make_batch

    return make_batch(1, n_scenes, "nuscenes", img_hw=(32, 48))


@pytest.mark.parametrize("case", ["random", "lidar", "single_point", "empty"])
def test_metadata_bit_exact(case):
    from mm2d3d_amd.scn.metadata import Metadata

    dev = _dev()
    if case == "random":
        coords, _ = _random_sparse(0, S=64, B=3, n=3000)
        S, nlev = 64, 5
    elif case == "lidar":
        coords = _lidar_batch(2)["x"][0]
        S, nlev = 4096, 7
    elif case == "single_point":
        coords, S, nlev = torch.tensor([[5, 6, 7, 0]]), 16, 3
    else:
        coords, S, nlev = torch.zeros((0, 4), dtype=torch.int64), 16, 2
    md = Metadata(dev, S, nlev)
    md.build_levels(coords.to(dev).contiguous())
    md.build_rulebooks()
    # oracle chain
    p2v, first = scn_ref.first_occurrence_ids(scn_ref.pack_keys(coords.numpy()))
    lv = scn_ref.Level(coords.numpy()[first], S)
    assert np.array_equal(md.levels[0].item2vox.cpu().numpy(), p2v)
    for l in range(nlev):
        g = md.levels[l]
        assert g.n == lv.n, (l, g.n, lv.n)
        assert np.array_equal(g.coords.cpu().numpy().astype(np.int64).reshape(-1, 4), lv.coords)
        rb = scn_ref.subm_rulebook(lv)
        assert np.array_equal(g.subm.offsets_host.astype(np.int64), rb.offsets)
        R = rb.n_rules
        assert np.array_equal(g.subm.rin.cpu().numpy()[:R], rb.rin) and np.array_equal(g.subm.rout.cpu().numpy()[:R], rb.rout)
        if l + 1 < nlev:
            rb8, coarse = scn_ref.down_rulebook(lv)
            assert np.array_equal(g.down.offsets_host.astype(np.int64), rb8.offsets)
            assert np.array_equal(g.down.rin.cpu().numpy()[: rb8.n_rules], rb8.rin)
            assert np.array_equal(g.down.rout.cpu().numpy()[: rb8.n_rules], rb8.rout)
            lv = coarse


def test_out_of_range_coordinates_raise():
    from mm2d3d_amd.scn.metadata import Metadata

    dev = _dev()
    md = Metadata(dev, 16, 2)
    with pytest.raises(ValueError):
        md.build_levels(torch.tensor([[1, 2, 3, 0], [-1, 0, 0, 0]], device=dev))


def _pair(mod_ref, mod_hip):
    mod_hip.load_state_dict(mod_ref.state_dict())
    return mod_ref, mod_hip.cuda()


@pytest.fixture(params=["rulebook", "os"])
def engine(request):
    """Both sparse-conv engine families: the k-major rulebook engines (csrc/spconv.hip) and the output-stationary engine
    (csrc/osconv.hip), which the product only picks for levels of >= 200k rows: forced on here at test sizes."""
    from mm2d3d_amd.scn import metadata

    old = (metadata.OS_MIN_ROWS, metadata.OS_BUILD_UP)
    metadata.OS_MIN_ROWS, metadata.OS_BUILD_UP = (0, True) if request.param == "os" else (1 << 60, False)
    yield request.param
    metadata.OS_MIN_ROWS, metadata.OS_BUILD_UP = old


@pytest.mark.parametrize("cin,cout", [(3, 16), (16, 16), (32, 16), (16, 32), (48, 48), (5, 7), (64, 192), (192, 96), (80, 80), (112, 48)])
def test_conv_ops_forward_backward(cin, cout, engine):
    from mm2d3d_amd import scn

    dev = _dev()
    torch.manual_seed(cin * 100 + cout)
    coords, feats = _random_sparse(cin + cout, S=32, B=2, n=1500, C=cin)

    def run(mod, f, cuda):
        inp = mod.InputLayer(3, 32, mode=4)
        sub = mod.SubmanifoldConvolution(3, cin, cout, 3, False)
        down = mod.Convolution(3, cout, cin, 2, 2, False)
        up = mod.Deconvolution(3, cin, cout, 2, 2, False)
        return inp, sub, down, up

    ri, rs, rd, ru = run(scn_ref, feats, False)
    hi, hs, hd, hu = run(scn, feats, True)
    for a, b in ((rs, hs), (rd, hd), (ru, hu)):
        b.load_state_dict(a.state_dict())
        b.cuda()
    fr = feats.clone().requires_grad_(True)
    fh = feats.clone().to(dev).requires_grad_(True)
    xr = ri([coords, fr])
    xh = hi([coords, fh])
    _close(xh.features, xr.features, what="input mean")
    yr1, yh1 = rs(xr), hs(xh)
    _close(yh1.features, yr1.features, what="subm fwd")
    yr2, yh2 = rd(yr1), hd(yh1)
    _close(yh2.features, yr2.features, what="down fwd")
    yr3, yh3 = ru(yr2), hu(yh2)
    _close(yh3.features, yr3.features, what="up fwd")
    g = torch.randn_like(yr3.features)
    (yr3.features * g).sum().backward()
    (yh3.features * g.to(dev)).sum().backward()
    _close(fh.grad, fr.grad, what="d feats")
    for name, a, b in (("subm", rs, hs), ("down", rd, hd), ("up", ru, hu)):
        _close(b.weight.grad, a.weight.grad, what=f"dW {name}")


@pytest.mark.parametrize("momentum", [0.9, 0.99])
@pytest.mark.parametrize("C,leak", [(16, 0.0), (48, 0.333), (7, 0.0), (224, 0.0)])
def test_batchnorm_forward_backward_running_stats(C, leak, momentum):
    from mm2d3d_amd import scn

    dev = _dev()
    torch.manual_seed(C)
    x = torch.randn(3001, C) * 2 + 0.5
    # both readings of the un-vendored dependency's running-statistics constant (scn.DEFAULT_BN_MOMENTUM): keep 0.9 / keep 0.99
    r, h = scn_ref.BatchNormLeakyReLU(C, leakiness=leak, momentum=momentum), scn.BatchNormLeakyReLU(C, leakiness=leak, momentum=momentum)
    with torch.no_grad():
        r.weight.uniform_(0.5, 1.5)
        r.bias.uniform_(-0.5, 0.5)
    h.load_state_dict(r.state_dict())
    h.cuda()
    xr = x.clone().requires_grad_(True)
    xh = x.clone().to(dev).requires_grad_(True)
    tr = scn_ref.SparseConvNetTensor(xr, scn_ref.Level(np.zeros((0, 4), np.int64), 8), 8)
    tr.root = None
    th = scn.SparseConvNetTensor(xh, None, 8, None)
    yr, yh = r(tr).features, h(th).features
    _close(yh, yr, what="bn fwd")
    g = torch.randn_like(yr)
    (yr * g).sum().backward()
    (yh * g.to(dev)).sum().backward()
    _close(xh.grad, xr.grad, what="bn dx")
    _close(h.weight.grad, r.weight.grad, tol=2e-3, what="bn dgamma")
    _close(h.bias.grad, r.bias.grad, tol=2e-3, what="bn dbeta")
    _close(h.running_mean, r.running_mean, what="running_mean")
    _close(h.running_var, r.running_var, what="running_var")
    # the constant is what it says: the old value's share after one training step
    assert abs(float(h.running_var[0]) - (momentum * 1.0 + (1 - momentum) * float(x[:, 0].var(unbiased=True)))) < 1e-3
    r.eval(), h.eval()
    _close(h(th).features, r(tr).features, what="bn eval")

@pytest.mark.parametrize("N,Ns,C,leak,pitch", [
    (3001, 3001, 16, 0.0, 16),          # one statistics group, a few rows per thread
    (558080, 279040, 16, 0.0, 16),      # level 0 of the headline step: 17 rows per thread
    (558080, 300001, 32, 0.333, 32),    # the widest level-0 map (34 rows per thread), leaky, uneven groups
    (120007, 60000, 112, 0.0, 112),     # 28 column groups (18 row slots of the 512 threads)
    (250000, 125000, 48, 0.0, 96),      # rows that are a channel slice of a wider buffer
])
def test_batchnorm_single_launch_kernels_equal_the_three_kernel_path(N, Ns, C, leak, pitch):
    """csrc/bn.hip: the grid-barrier kernels (fp32 rows kept in registers / LDS) against reduce / finalize / apply on the same
    inputs, through the C-ABI.  Same arithmetic per element; only the order in which the per-workgroup partial sums are combined
    differs, so statistics agree to fp32 rounding and outputs to a few ulp of their scale."""
    from mm2d3d_amd import _lib
    from mm2d3d_amd._lib import check, ptr, stream

    dev = _dev()
    L = _lib.lib()
    g = torch.Generator().manual_seed(N % 1000 + C)
    xb = (torch.randn(N, pitch, generator=g) * 1.5 + 0.3).to(dev)
    x = xb[:, pitch - C:]
    dy = torch.randn(N, C, generator=g).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    b = torch.randn(C, generator=g).to(dev)

    def run(mask):
        prev = _lib.bn3d_set_fused(mask)
        h = _lib.handle(dev).h
        try:
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            y, dx = torch.zeros(N, C, device=dev), torch.zeros(N, C, device=dev)
            dw, db = torch.full((C,), 0.5, device=dev), torch.full((C,), -1.0, device=dev)
            stats = torch.zeros((2, 2 if 0 < Ns < N else 1, C), device=dev)
            ws = _lib.workspace.get(int(L.mm_bn_ws_bytes(C)) + 8 * C, dev)
            check(L.mm_bn_fwd_train(h, ptr(x), pitch, N, Ns, C, ptr(w), ptr(b), ptr(rm), ptr(rv), 1e-4, 0.9, leak, ptr(y), C, ptr(stats[0]),
                                    ptr(stats[1]), ptr(ws), ws.numel(), stream()), "fwd")
            check(L.mm_bn_bwd(h, ptr(x), pitch, ptr(dy), C, N, Ns, C, ptr(w), ptr(b), ptr(stats[0]), ptr(stats[1]), leak, ptr(dx), C, ptr(dw),
                              ptr(db), 1, ptr(ws), ws.numel(), stream()), "bwd")
            torch.cuda.synchronize()
        finally:
            _lib.bn3d_set_fused(prev)
        return dict(y=y, dx=dx, dw=dw, db=db, stats=stats, rm=rm, rv=rv)

    a, c = run(3), run(0)
    assert torch.allclose(a["stats"], c["stats"], rtol=2e-6, atol=1e-7)
    assert torch.allclose(a["rm"], c["rm"], rtol=2e-6, atol=1e-8) and torch.allclose(a["rv"], c["rv"], rtol=2e-6, atol=0)
    for k in ("y", "dx"):
        scale = float(c[k].abs().max())
        assert float((a[k] - c[k]).abs().max()) <= 4e-6 * scale, k
    assert float((a["dw"] - c["dw"]).abs().max()) <= 1e-5 * float(c["dw"].abs().max()) + 1e-5
    assert float((a["db"] - c["db"]).abs().max()) <= 1e-5 * float(c["db"].abs().max()) + 1e-5

@pytest.mark.parametrize("leak,split", [(0.0, None), (0.333, 1200)])
def test_join_table_followed_by_batchnorm_builds_no_concat(leak, split):
    """scn_unet.py:81-82: JoinTable -> BatchNormReLU.  Here the join is lazy and the batch norm normalises the parts straight into
    one buffer (ops.BatchNormActJoinFunction); it must equal batch norm over the concatenated rows, forward and backward, in
    training (also with two statistics groups) and in eval mode."""
    import copy
    import types

    from mm2d3d_amd import scn

    dev = _dev()
    torch.manual_seed(7)
    N, ca, cb = 3001, 16, 32
    a0, b0 = (torch.randn(N, ca) * 2 + 0.5).to(dev), (torch.randn(N, cb) - 0.3).to(dev)
    bn1 = (scn.BatchNormLeakyReLU(ca + cb, leakiness=leak) if leak else scn.BatchNormReLU(ca + cb)).to(dev)
    with torch.no_grad():
        bn1.weight.uniform_(0.5, 1.5)
        bn1.bias.uniform_(-0.5, 0.5)
    bn2 = copy.deepcopy(bn1)
    level = types.SimpleNamespace(seg_rows=split)
    a1, b1 = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    a2, b2 = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    joined = scn.JoinTable()([scn.SparseConvNetTensor(a1, None, 8, level), scn.SparseConvNetTensor(b1, None, 8, level)])
    assert joined._features is None and len(joined._parts) == 2
    y1 = bn1(joined).features
    assert joined._features is None  # nobody built the concatenation
    y2 = bn2(scn.SparseConvNetTensor(torch.cat([a2, b2], 1), None, 8, level)).features
    assert torch.allclose(y1, y2, rtol=1e-5, atol=1e-5)
    g = torch.randn_like(y1)
    (y1 * g).sum().backward()
    (y2 * g).sum().backward()
    for u, v, what in ((a1.grad, a2.grad, "dx part 0"), (b1.grad, b2.grad, "dx part 1"), (bn1.weight.grad, bn2.weight.grad, "dgamma"),
                       (bn1.bias.grad, bn2.bias.grad, "dbeta")):
        assert torch.allclose(u, v, rtol=1e-4, atol=1e-4 * float(v.abs().max())), what
    assert torch.allclose(bn1.running_mean, bn2.running_mean, rtol=1e-5, atol=1e-6) and torch.allclose(bn1.running_var, bn2.running_var, rtol=1e-5)
    bn1.eval(), bn2.eval()
    e1 = bn1(scn.JoinTable()([scn.SparseConvNetTensor(a0, None, 8, level), scn.SparseConvNetTensor(b0, None, 8, level)])).features
    e2 = bn2(scn.SparseConvNetTensor(torch.cat([a0, b0], 1), None, 8, level)).features
    assert torch.allclose(e1, e2, rtol=1e-5, atol=1e-5)
    # anything else that reads .features still gets the plain concatenation
    t = scn.JoinTable()([scn.SparseConvNetTensor(a0, None, 8, level), scn.SparseConvNetTensor(b0, None, 8, level)])
    assert torch.equal(t.features, torch.cat([a0, b0], 1))


@pytest.mark.parametrize("residual", [False, True])
def test_net3d_forward_backward_vs_oracle(residual, engine):
    """Forward: logits within 1e-3 of the fp32 oracle (north_star).  Backward: this 50-layer BN network's fp32
    gradients are only conditioned to ~1e-2: the fp32 oracle differs from the fp64 oracle by that much, and a 1-ulp
    perturbation of the input features moves the oracle's own gradients by as much (ReLU masks and BN statistics amplify
    it, most in the residual variant).  Each HIP gradient must therefore be as close to the fp64 oracle as the fp32
    oracle is, or as close as the oracle is to its own 1-ulp-perturbed self (factor 4), floor 1e-3.
    The fp32 oracle's rounding follows its summation order, which torch's CPU thread count sets: for this network the
    gradient of one 3^3 layer of the plain variant lies 1.2e-3 .. 6e-3 from the fp64 oracle with 4-16 threads and 2.4e-2
    with 1-2 threads, while the fp64 oracle moves by 1e-13.  So that the yardstick does not depend on the machine, the fp32
    oracle runs both with the default thread count and with one thread, and the farther of the two from the fp64 oracle is
    the one the HIP gradients are held to."""
    import copy

    from mm2d3d_amd.net3d import Net3DSeg

    dev = _dev()
    torch.manual_seed(0)
    batch = _lidar_batch(2)
    kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7, residual_blocks=residual)
    ref = Net3DSegRef(6, True, kw)
    ref64 = copy.deepcopy(ref).double()
    hip = Net3DSeg(6, True, kw)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.cuda()
    coords, feats = batch["x"]
    bh = {"x": [coords.to(dev), feats.clone().to(dev)]}
    br = {"x": [coords, feats.clone()]}
    pr, fr, ar = ref(br)
    ph, fh, ah = hip(bh)
    p64, _, a64 = ref64({"x": [coords, feats.clone().double()]})
    _close(bh["x"][1], br["x"][1], what="gated feats written back to the batch dict")
    _close(fh, fr, what="3D features")
    _close(ph["seg_logit"], pr["seg_logit"], what="seg_logit")  # north_star: logits within 1e-3
    _close(ah["seg_logit_point"], ar["seg_logit_point"], what="seg_logit_point")
    _close(ph["confidence"], pr["confidence"], what="confidence")
    w = torch.randn_like(pr["seg_logit"])
    (pr["seg_logit"] * w).sum().add((ar["seg_logit_point"] * w).sum()).backward()
    (ph["seg_logit"] * w.to(dev)).sum().add((ah["seg_logit_point"] * w.to(dev)).sum()).backward()
    (p64["seg_logit"] * w.double()).sum().add((a64["seg_logit_point"] * w.double()).sum()).backward()
    g32 = dict(ref.named_parameters())
    g64 = dict(ref64.named_parameters())

    def oracle_again(f):
        """The fp32 oracle's gradients of the same loss once more, with the same weights, on features ``f``."""
        net = copy.deepcopy(ref)
        for q in net.parameters():
            q.grad = None
        pp, _, ap = net({"x": [coords, f.clone()]})
        (pp["seg_logit"] * w).sum().add((ap["seg_logit_point"] * w).sum()).backward()
        return dict(net.named_parameters())

    # conditioning probe: the fp32 oracle on features perturbed by ~1 ulp
    gpert = oracle_again(feats * (1.0 + 2.0 ** -23))
    # the fp32 oracle in a second, fixed summation order: one CPU thread
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        g32_1 = oracle_again(feats)
    finally:
        torch.set_num_threads(threads)
    errs = {}
    for name, p in hip.named_parameters():
        if "linear_global" in name:
            assert p.grad is None
            continue
        assert p.grad is not None, name
        t = g64[name].grad
        scale = max(1.0, t.abs().max().item())
        errs[name] = ((p.grad.detach().cpu().double() - t).abs().max().item() / scale,
                      max((g[name].grad.double() - t).abs().max().item() for g in (g32, g32_1)) / scale,
                      (gpert[name].grad.double() - g32[name].grad.double()).abs().max().item() / scale)
    noise = float(np.median([e[1] for e in errs.values()]))  # typical fp32 rounding noise of this network's gradients
    # A single ReLU-mask flip (pre-activation within a few ulp of 0) moves a weight gradient of this random linear loss by
    # ~1/sqrt(rows) ~ 1e-2 in max-norm (measured: two HIP stem kernels that differ by 3.6e-7 in their outputs, all
    # downstream activations equal to 1e-5, give weight gradients 1.8e-2 apart in the residual variant).
    flip = 3e-2 if residual else 1e-3
    for name, (e_hip, e_ref, e_pert) in errs.items():
        assert e_hip <= max(4.0 * e_ref, 8.0 * noise, 4.0 * e_pert, flip), \
            f"grad {name}: hip-vs-fp64 {e_hip:.3e}, fp32-oracle-vs-fp64 {e_ref:.3e}, oracle 1-ulp sensitivity {e_pert:.3e}"
    # A max-norm envelope alone would let a systematically wrong gradient through as long as it stays small:
    # per tensor also the direction (cosine) and the relative L2 distance to the fp64 oracle, each against what the fp32 oracle
    # itself achieves.  A mask flip moves single elements, not the direction of a whole tensor.
    for name, p in hip.named_parameters():
        if p.grad is None:
            continue
        t = g64[name].grad.double().flatten()
        h = p.grad.detach().cpu().double().flatten()
        rs = [g[name].grad.double().flatten() for g in (g32, g32_1)]
        if float(t.norm()) < 1e-9:
            assert float(h.norm()) < 1e-6, name
            continue
        cos_h = float((h @ t) / (h.norm() * t.norm()).clamp_min(1e-300))
        cos_r = min(float((r @ t) / (r.norm() * t.norm()).clamp_min(1e-300)) for r in rs)
        l2_h, l2_r = float((h - t).norm() / t.norm()), max(float((r - t).norm() / t.norm()) for r in rs)
        assert cos_h >= min(1.0 - 1e-4, 1.0 - 16.0 * (1.0 - cos_r)) - (2e-3 if residual else 0.0), (name, cos_h, cos_r)
        assert l2_h <= max(8.0 * l2_r, 2e-3) + (5e-2 if residual else 0.0), (name, l2_h, l2_r)
    for (n1, b1), (n2, b2) in zip(sorted(hip.named_buffers()), sorted(ref.named_buffers())):
        assert n1 == n2
        _close(b1, b2, what=f"buffer {n1}")


# ----------------------------------------------------------------------------------------------------------------------
# 16-bit activation mode (BASELINE.json configs[4]).  The reference's SparseConvNet has no 16-bit kernels (SURVEY.md
# section 7, last bullet), so there is no reference behaviour to match: the tolerances below are this mode's own, stated
# against the fp32 oracle on the SAME bf16-rounded operands (operator tests: what is left is the bf16 rounding of the
# output rows, 2^-9) and against the fp32 network (network test).
# Both kinds of 16-bit rows: bf16 (no loss scale needed) and IEEE fp16 (BASELINE.json configs[4]'s wording, the reference's
# ``precision: 16``; 2^-11 rounding instead of 2^-8, so every bf16 bound below holds with room).
@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def act16_mode(request):
    from mm2d3d_amd import scn

    scn.set_activation_dtype(request.param)
    yield request.param
    scn.set_activation_dtype(torch.float32)


@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 16), (48, 96), (112, 112), (192, 96)])
def test_act16_conv_ops_forward_backward(cin, cout, act16_mode):
    """SubM / Convolution / Deconvolution with bf16 rows: forward, data gradient and weight gradient against the fp64
    rule-book oracle evaluated on the bf16-rounded operands (inputs, weights and incoming gradients)."""
    from mm2d3d_amd.scn import ops
    from mm2d3d_amd.scn.metadata import Metadata

    dev = _dev()
    torch.manual_seed(cin + cout)
    coords, _ = _random_sparse(cin * 3 + cout, S=32, B=2, n=2500, C=1)
    md = Metadata(dev, 32, 2, act16=True)
    md.build_levels(coords.to(dev).contiguous())
    md.build_rulebooks()
    lv = md.levels[0]
    keys = scn_ref.pack_keys(coords.numpy())
    _, first = scn_ref.first_occurrence_ids(keys)
    rlv = scn_ref.Level(coords.numpy()[first], 32)
    bf = lambda t: t.to(act16_mode)
    for mode in ("subm", "down", "up"):
        if mode == "subm":
            rb, rrb, n_in, n_out, K, tr = lv.subm, scn_ref.subm_rulebook(rlv), lv.n, lv.n, 27, False
        else:
            rrb, rc = scn_ref.down_rulebook(rlv)
            rb, K = lv.down, 8
            n_in, n_out, tr = (lv.n, lv.coarse.n, False) if mode == "down" else (lv.coarse.n, lv.n, True)
            assert rc.n == lv.coarse.n
        x = bf(torch.randn(n_in, cin))
        w = torch.randn(K, 1, cin, cout) * (2.0 / cin / K) ** 0.5
        g = bf(torch.randn(n_out, cout))
        xh = x.to(dev).requires_grad_(True)
        wh = w.to(dev).requires_grad_(True)
        y = ops.SparseConvFunction.apply(xh, wh, rb, mode, n_in, n_out)
        assert y.dtype == act16_mode
        y.backward(g.to(dev))
        assert xh.grad.dtype == act16_mode and wh.grad.dtype == torch.float32
        xr = x.double().requires_grad_(True)
        wr = bf(w).double().reshape(K, cin, cout).requires_grad_(True)  # the kernels use one bf16 term per weight
        yr = scn_ref.rule_conv(xr, wr, rrb, n_out, transpose_roles=tr)
        yr.backward(g.double())
        # outputs are rounded to bf16 (relative 2^-9 = 2e-3 per element): 4e-3 of the largest element
        _close(y.float(), yr, tol=4e-3, what=f"{mode} fwd")
        # the data gradient multiplies by the same bf16 weights
        _close(xh.grad.float(), xr.grad, tol=4e-3, what=f"{mode} dX")
        # weight gradient: fp32 accumulation of exact bf16 products
        _close(wh.grad.reshape(K, cin, cout), wr.grad, tol=1e-4, what=f"{mode} dW")


def test_act16_batchnorm(act16_mode):
    from mm2d3d_amd import scn

    dev = _dev()
    torch.manual_seed(3)
    C, N = 48, 3000
    x = (torch.randn(N, C) * 2 + 0.5).to(act16_mode)
    bn = scn.BatchNormReLU(C).to(dev)
    ref = torch.nn.BatchNorm1d(C, eps=1e-4, momentum=1.0 - bn.momentum).double()  # scn momentum = keep fraction (default 0.99)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.1)
        ref.weight.copy_(bn.weight.cpu().double())
        ref.bias.copy_(bn.bias.cpu().double())
    xh = x.to(dev).requires_grad_(True)
    t = scn.SparseConvNetTensor(xh, None, 32, None)
    y = bn(t).features
    assert y.dtype == act16_mode
    xr = x.double().requires_grad_(True)
    yr = torch.relu(ref(xr))
    g = torch.randn(N, C).to(act16_mode)
    y.backward(g.to(dev))
    yr.backward(g.double())
    _close(y.float(), yr, tol=4e-3, what="bn16 fwd")
    _close(xh.grad.float(), xr.grad, tol=4e-3, what="bn16 dx")
    _close(bn.weight.grad, ref.weight.grad, tol=2e-3, what="bn16 dweight")  # the ReLU mask is decided in fp32 on both sides
    _close(bn.running_mean, ref.running_mean.float(), tol=1e-5, what="bn16 running_mean")


def test_act16_net3d_vs_fp32(act16_mode):
    """The whole 3D net with bf16 rows against itself in fp32 (same weights, same scenes): logits within 3e-2 of the
    largest logit; parameter gradients aligned with the fp32 run (cosine: median > 0.9, every tensor > 0.8; measured 0.95 / 0.88 - the few-row
    batch norms of the coarsest levels are the least conditioned, see test_net3d_forward_backward_vs_oracle)."""
    import copy

    from mm2d3d_amd import scn
    from mm2d3d_amd.net3d import Net3DSeg

    dev = _dev()
    torch.manual_seed(0)
    batch = _lidar_batch(2)
    kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
    net16 = Net3DSeg(6, True, kw).to(dev)
    net32 = copy.deepcopy(net16)
    coords, feats = batch["x"]
    w = torch.randn(coords.shape[0], 6, device=dev)
    S = 256.0 if act16_mode == torch.float16 else 1.0  # fp16 gradient rows: a loss scale (cosines do not depend on it)
    p16, _, a16 = net16({"x": [coords.to(dev), feats.clone().to(dev)]})
    ((p16["seg_logit"] * w).sum() * S).backward()
    scn.set_activation_dtype(torch.float32)
    p32, _, a32 = net32({"x": [coords.to(dev), feats.clone().to(dev)]})
    ((p32["seg_logit"] * w).sum() * S).backward()
    assert p16["seg_logit"].dtype == torch.float32
    _close(p16["seg_logit"], p32["seg_logit"], tol=3e-2, what="act16 logits vs fp32 logits")
    cos = []
    for (n, a), (_, b) in zip(net16.named_parameters(), net32.named_parameters()):
        if b.grad is None:
            assert a.grad is None
            continue
        ga, gb = a.grad.flatten().double(), b.grad.flatten().double()
        c = float((ga @ gb) / (ga.norm() * gb.norm() + 1e-30))
        cos.append((c, n))
    assert min(cos)[0] > 0.8 and float(np.median([c for c, _ in cos])) > 0.9, sorted(cos)[:5]


def test_act16_net3d_vs_16bit_emulating_oracle(act16_mode):
    """The whole 3D net with 16-bit rows against the CPU ORACLE evaluated with the same storage format: oracle.scn_ref
    rounds every sparse row to bf16 exactly where the HIP path stores bf16 (conv outputs, batch-norm outputs, the
    gradients on the way back), multiplies bf16-rounded weights in the 16-channel-multiple convolutions and keeps all sums
    and statistics in fp32 (``EMULATE16``).  What is left between the two is accumulation order and the bf16 rounding
    decisions it flips (one flip = 2^-8 of an element, carried through 50 layers): measured 7.2e-3 of the largest logit
    (about two bf16 ulps; the fp32 oracle is at 1.2e-2), gradient cosines min 0.945 / median 0.983.  Bounds = 2x that."""
    import copy

    from mm2d3d_amd.net3d import Net3DSeg
    from oracle import scn_ref

    dev = _dev()
    torch.manual_seed(0)
    batch = _lidar_batch(2)
    kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
    ref = Net3DSegRef(6, True, kw)
    ref32 = copy.deepcopy(ref)
    hip = Net3DSeg(6, True, kw)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to(dev)
    coords, feats = batch["x"]
    w = torch.randn(coords.shape[0], 6)
    # IEEE fp16 gradient rows need a loss scale (mm2d3d_amd/amp.py in training); the same factor on both sides here
    S = 256.0 if act16_mode == torch.float16 else 1.0
    ph, _, ah = hip({"x": [coords.to(dev), feats.clone().to(dev)]})
    ((ph["seg_logit"] * w.to(dev)).sum().add((ah["seg_logit_point"] * w.to(dev)).sum()) * S).backward()
    scn_ref.EMULATE16[0] = act16_mode
    try:
        pr, _, ar = ref({"x": [coords, feats.clone()]})
        ((pr["seg_logit"] * w).sum().add((ar["seg_logit_point"] * w).sum()) * S).backward()
    finally:
        scn_ref.EMULATE16[0] = None
    p32, _, _ = ref32({"x": [coords, feats.clone()]})
    e16 = (ph["seg_logit"].detach().cpu() - pr["seg_logit"].detach()).abs().max().item()
    e32 = (ph["seg_logit"].detach().cpu() - p32["seg_logit"].detach()).abs().max().item()
    scale = max(1.0, pr["seg_logit"].abs().max().item())
    print(f"act16 logits: vs 16-bit-emulating oracle {e16 / scale:.2e}, vs fp32 oracle {e32 / scale:.2e} (of the largest logit)")
    assert e16 <= 1.5e-2 * scale, (e16, scale)
    _close(ah["seg_logit_point"], ar["seg_logit_point"], tol=1.5e-2, what="act16 aux logits vs emulating oracle")
    cos = []
    gr = dict(ref.named_parameters())
    for n, a in hip.named_parameters():
        if gr[n].grad is None:
            assert a.grad is None, n
            continue
        ga, gb = a.grad.detach().cpu().flatten().double(), gr[n].grad.flatten().double()
        cos.append((float((ga @ gb) / (ga.norm() * gb.norm() + 1e-30)), n))
    print("act16 gradient cosines vs emulating oracle: min %.4f median %.4f" % (min(cos)[0], float(np.median([c for c, _ in cos]))))
    assert min(cos)[0] > 0.9 and float(np.median([c for c, _ in cos])) > 0.965, sorted(cos)[:5]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_metadata_prebuilt_on_a_side_stream_gives_the_same_network_output(mode):
    """scn.prebuild_metadata builds hash, rulebooks and tile tables on a side stream ahead of the forward (TrainModel overlaps
    it with the 2D branch).  Logits and gradients must be bit-identical to the in-line build, in fp32 and in the 16-bit
    activation mode (which needs tables for every level and both directions)."""
    import copy

    from mm2d3d_amd import scn
    from mm2d3d_amd.net3d import Net3DSeg

    dev = _dev()
    torch.manual_seed(0)
    scn.set_activation_dtype(torch.bfloat16 if mode == "bf16" else torch.float32)
    try:
        batch = _lidar_batch(2)
        kw = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
        net_a = Net3DSeg(6, True, kw).to(dev)
        net_b = copy.deepcopy(net_a)
        coords, feats = batch["x"]
        w = torch.randn(coords.shape[0], 6, device=dev)
        pa, _, _ = net_a({"x": [coords.to(dev), feats.clone().to(dev)]})
        (pa["seg_logit"] * w).sum().backward()
        cb = coords.to(dev)
        side = torch.cuda.Stream(dev)
        net_b.prepare({"x": [cb, None]}, side, torch.cuda.current_stream(dev).record_event())
        assert getattr(cb, "_mm_metadata", None) is not None
        pb, _, _ = net_b({"x": [cb, feats.clone().to(dev)]})
        (pb["seg_logit"] * w).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(pa["seg_logit"], pb["seg_logit"])
        for (n, a), (_, b) in zip(net_a.named_parameters(), net_b.named_parameters()):
            assert (a.grad is None) == (b.grad is None), n
            if a.grad is not None:
                assert torch.equal(a.grad, b.grad), n
    finally:
        scn.set_activation_dtype(torch.float32)
