"""Correlation alignment on the GPU (csrc/coral.hip: k_coral_stats / k_coral_final behind mm_coral_fwd, k_coral_bwd behind
mm_coral_bwd; losses.coral) against the float64 reference tests/_coral_ref.py evaluated on the same fp32 rows.

The C ABI is called directly with the operands of tests/_gpu_rows.py: x is a pitched view whose padding is NaN, every output lies
between sentinels that must survive.  count is exact; loss, mean and cov are within 1e-5 * max(1, |ref|), the project's bound for
fp32 outputs of fp64 sums (tests/test_gpu_infomax.py, tests/test_gpu_ce_pair.py).  Every gradient element is within the fp32 bound of
a d-term dot product evaluated from the reference's float64 quantities, (d + 4) * 2^-24 * sum_j |x_ij - m_j| |aux_jk| plus one fp32
ulp of the reference value: d roundings of the products and sums, and a margin of 4 for the fp32 rounding of the centred row (the
backward reads the mean as an fp32 pair, so x - m rounds once), of the stored matrices and of the product with grad_out.  The
largest observed ratio to that bound is printed."""
import functools

import numpy as np
import pytest
import torch

import _coral_ref as R
from _gpu_rows import Ints, Rows, abi, dev, vec

pytestmark = pytest.mark.gpu

MODES = {"plain": 0, "log": 1}
EPS = float(np.float32(1e-4))  # the ridge as the kernel receives it

# (N, P, d)
CASES = {
    "0_0_6": (0, 0, 6),
    "1_0_2": (1, 0, 2),
    "3_1_2": (3, 1, 2),  # n_s < 2
    "64_32_2": (64, 32, 2),
    "300_173_11": (300, 173, 11),  # the split inside a tile and off a wave boundary
    "257_120_32": (257, 120, 32),  # widest rows; the LDS pitch d | 1 = 33 stays odd
    "40_20_32": (40, 20, 32),  # rank-deficient: the repeated ridge eigenvalues must divide cleanly
    "131208_65543_5": (131072 + 129 + 7, 65543, 5),  # 1027 tiles for the 1024 workgroups of the statistics grid: accumulators carried over
    "300_173_11_holes": (300, 173, 11),  # a NaN row and an infinite row in each segment
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded fp32 rows 3 * randn mixed by a seeded d x d matrix (the covariances are not diagonal), the target's scaled so that the
    domains differ, and the float64 reference in both modes: computed once, never modified."""
    N, P, d = CASES[name]
    rng = np.random.default_rng(6000 + sorted(CASES).index(name.replace("_holes", "")))
    x = 3.0 * rng.standard_normal((N, d)) @ (rng.standard_normal((d, d)) / np.sqrt(d)) + rng.standard_normal(d)
    x[P:] = 1.5 * x[P:] + 0.5
    x = x.astype(np.float32)
    if name.endswith("_holes"):
        x[5] = np.nan
        x[127, 3] = np.inf
        x[P + 1, 0] = -np.inf
        x[N - 1, d - 1] = np.nan
    return dict(N=N, P=P, d=d, x=x, ref={m: R.evaluate(x, P, m, EPS) for m in MODES})


class _Call:
    """One mm_coral_fwd and one mm_coral_bwd over pitched, padded operands."""

    def __init__(self, x, N, P, d, mode="log", eps=EPS, gout=1.0, ld=None, ld_dx=None, run=True):
        L, _lib = abi()
        self.L, self.N, self.P, self.d, self.mode, self.eps = L, N, P, d, MODES[mode], eps
        self.ld, self.ld_dx = d + 3 if ld is None else ld, d + 2 if ld_dx is None else ld_dx
        self.x = Rows(x, N, d, max(self.ld, d), off=5)
        self.loss, self.mean, self.cov, self.aux = vec(None, 1), vec(None, 2 * d), vec(None, 2 * d * d), vec(None, 4 * d + 2 * d * d)
        self.count = Ints(None, 2, dtype=torch.int64)
        self.dx = Rows(None, N, d, max(self.ld_dx, d), off=3, fill=-12345.0)
        self.gout = torch.tensor([gout], dtype=torch.float32, device=dev())
        self.ws = torch.empty(int(L.mm_coral_ws_bytes(d)), dtype=torch.uint8, device=dev())
        self.stream = _lib.stream()
        if run:
            assert self.fwd() == 0, L.mm_last_error()
            assert self.bwd() == 0, L.mm_last_error()
            torch.cuda.synchronize()

    def fwd(self, **kw):
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, P=self.P, d=self.d, mode=self.mode, eps=self.eps, loss=self.loss.ptr, count=self.count.ptr,
                 mean=self.mean.ptr, cov=self.cov.ptr, aux=self.aux.ptr, ws=self.ws.data_ptr(), ws_bytes=self.ws.numel())
        a.update(kw)
        return self.L.mm_coral_fwd(a["x"], a["ld"], a["N"], a["P"], a["d"], a["mode"], a["eps"], a["loss"], a["count"], a["mean"], a["cov"],
                                   a["aux"], a["ws"], a["ws_bytes"], self.stream)

    def bwd(self, **kw):
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, P=self.P, d=self.d, aux=self.aux.ptr, g=self.gout.data_ptr(), dx=self.dx.ptr, ld_dx=self.ld_dx)
        a.update(kw)
        return self.L.mm_coral_bwd(a["x"], a["ld"], a["N"], a["P"], a["d"], a["aux"], a["g"], a["dx"], a["ld_dx"], self.stream)

    def outputs(self):
        return (self.loss, self.mean, self.cov, self.aux, self.count, self.dx)

    def outputs_untouched(self):
        return all(o.untouched() for o in self.outputs())

    def padding_untouched(self):
        return all(o.padding_untouched() for o in self.outputs())


def _within(got, ref):
    return bool((np.abs(got - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all())


def _check(call, ref, what, gout=1.0):
    """Loss, counts, means, covariances, padding and the gradient of ``call`` against the reference ``ref``; returns the largest
    ratio of a gradient error to its bound."""
    d = call.d
    loss = float(call.loss.get().reshape(-1)[0])
    mean, cov = call.mean.get().reshape(2, d), call.cov.get().reshape(2, d, d)
    x64 = call.x.get32().astype(np.float64)
    want = gout * ref["grad"]
    bound = abs(gout) * R.gradient_bound(x64, call.P, ref)
    err = np.abs(call.dx.get() - want)
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: loss {loss:.7g} ref {ref['loss']:.7g}  count {call.count.get().tolist()} ref {ref['count']}  "
          f"max |mean - ref| {np.abs(mean - ref['mean']).max():.2e}  max |cov - ref| {np.abs(cov - ref['cov']).max():.2e} of {np.abs(ref['cov']).max():.3g}  "
          f"max |dgrad| {float(err.max()) if err.size else 0.0:.2e} of {float(np.abs(want).max()) if err.size else 0.0:.2e}  ratio to the bound {ratio:.3f}")
    assert call.count.get().tolist() == ref["count"], what
    assert _within(loss, ref["loss"]) and loss >= 0.0, what
    assert _within(mean, ref["mean"]) and _within(cov, ref["cov"]), what
    assert np.isfinite(call.aux.get()).all() and np.isfinite(call.dx.get()).all(), what
    assert ratio <= 1.0, what
    assert call.padding_untouched(), what
    dead = ~R.counted_rows(call.x.get32())
    assert not call.dx.bits()[dead].any(), what  # a row that is not counted: +0 in every bit
    return ratio


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_values_and_gradients_match_the_float64_reference(name, mode):
    c = _case(name)
    ref = c["ref"][mode]
    call = _Call(c["x"], c["N"], c["P"], c["d"], mode)
    _check(call, ref, f"{name} {mode}")
    if min(ref["count"]) < 2:  # a segment without a covariance: zeros, never 0 / 0
        assert float(call.loss.get().reshape(-1)[0]) == 0.0 and not call.dx.bits().any()
        assert not call.aux.get().reshape(-1)[4 * c["d"]:].any()
    else:
        assert ref["loss"] > 0.0 and np.abs(ref["grad"]).max() > 0.0
    if name.endswith("_holes"):
        assert ref["count"] == [c["P"] - 2, c["N"] - c["P"] - 2]
    if name == "40_20_32":  # 13 eigenvalues of each covariance sit on the ridge
        assert [int(np.linalg.matrix_rank(k)) for k in ref["cov"]] == [19, 19]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("gout", [2.0, -0.75])
def test_grad_out_scales_the_gradient(mode, gout):
    c = _case("300_173_11")
    _check(_Call(c["x"], c["N"], c["P"], c["d"], mode, gout=gout), c["ref"][mode], f"grad_out {gout} {mode}", gout)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["300_173_11_holes", "40_20_32", "131208_65543_5"])
def test_the_same_call_twice_is_bit_identical(name, mode):
    c = _case(name)
    a, b = (_Call(c["x"], c["N"], c["P"], c["d"], mode) for _ in range(2))
    for u, v in zip(a.outputs(), b.outputs()):
        if u is a.count:
            assert u.get().tolist() == v.get().tolist()
        else:
            assert np.array_equal(u.bits(), v.bits())


def test_identical_domains_align_exactly():
    """The same rows in both segments: equal sums, equal covariances, loss 0 and an all-zero gradient in both modes."""
    half = _case("300_173_11")["x"][:150]
    x = np.concatenate((half, half))
    for mode in MODES:
        call = _Call(x, 300, 150, 11, mode)
        assert float(call.loss.get().reshape(-1)[0]) == 0.0 and not call.dx.get().any(), mode
        assert np.array_equal(call.cov.bits().reshape(2, -1)[0], call.cov.bits().reshape(2, -1)[1])


def test_every_limit_is_refused_before_a_launch_and_nothing_is_written():
    c = _case("64_32_2")
    d = 6
    x = np.tile(c["x"], (1, 3))
    call = _Call(x, 64, 32, d, run=False)
    shared = (dict(d=1), dict(d=33), dict(d=0), dict(ld=d - 1), dict(P=-1), dict(P=65), dict(N=-1), dict(N=(1 << 31) // d + 1), dict(x=None),
              dict(aux=None))
    for kw in shared + (dict(mode=2), dict(mode=-1), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
                        dict(loss=None), dict(count=None), dict(mean=None), dict(cov=None), dict(ws=None), dict(ws_bytes=call.ws.numel() - 1)):
        assert call.fwd(**kw) == -1, kw
        assert b"coral_fwd:" in call.L.mm_last_error(), kw
    for kw in shared + (dict(ld_dx=d - 1), dict(g=None), dict(dx=None)):
        assert call.bwd(**kw) == -1, kw
        assert b"coral_bwd:" in call.L.mm_last_error(), kw
    torch.cuda.synchronize()
    assert call.outputs_untouched()


# ---------------------------------------------------------------------------------------------- losses.coral
@pytest.mark.parametrize("mode", list(MODES))
def test_coral_under_autograd_on_a_leaf(mode):
    from mm2d3d_amd.losses import coral

    c, d = _case("300_173_11"), dev()
    ref = R.evaluate(c["x"], c["P"], mode, EPS)
    x = torch.from_numpy(c["x"]).to(d).requires_grad_(True)
    out = coral(x, c["P"], mode)
    assert set(out) == {"loss", "count", "mean", "cov"} and all(v.is_cuda for v in out.values())
    assert out["loss"].requires_grad and out["loss"].dim() == 0 and out["loss"].dtype == torch.float32
    assert not any(out[k].requires_grad or out[k].grad_fn is not None for k in ("count", "mean", "cov"))
    assert out["count"].dtype == torch.int64 and out["count"].tolist() == ref["count"]
    assert out["mean"].shape == (2, 11) and out["cov"].shape == (2, 11, 11)
    (0.5 * out["loss"]).backward()
    assert _within(float(out["loss"].detach()), ref["loss"]) and _within(out["cov"].cpu().double().numpy(), ref["cov"])
    err = np.abs(x.grad.cpu().double().numpy() - 0.5 * ref["grad"])
    assert (err <= 0.5 * R.gradient_bound(c["x"], c["P"], ref)).all()


def test_coral_on_a_row_slice_of_a_wider_tensor_and_on_16_bit_rows():
    from mm2d3d_amd.losses import coral

    c, d = _case("300_173_11"), dev()
    N, C, lo, first = c["N"], c["d"], 20, 153
    wide = torch.full((N, C + 5), float("nan"))
    wide[:, 2: 2 + C] = torch.from_numpy(c["x"])
    leaf = wide.to(d).requires_grad_(True)
    view = leaf[lo:, 2: 2 + C]
    assert view.stride(0) == C + 5 and not view.is_contiguous()
    ref = R.evaluate(c["x"][lo:], first, "log", EPS)
    out = coral(view, first)
    out["loss"].backward()
    assert out["count"].tolist() == ref["count"] == [first, N - lo - first] and _within(float(out["loss"].detach()), ref["loss"])
    g = leaf.grad.cpu()
    assert (np.abs(g[lo:, 2: 2 + C].double().numpy() - ref["grad"]) <= R.gradient_bound(c["x"][lo:], first, ref)).all()
    outside = g.clone()
    outside[lo:, 2: 2 + C] = 0
    assert not outside.view(torch.int32).any()  # rows before the slice and the padding columns: +0
    # 16-bit rows: read as the float32 values they are, the gradient rounded once to the input's format
    for dtype, bits in ((torch.float16, 11), (torch.bfloat16, 8)):
        x16 = torch.from_numpy(c["x"]).to(dtype)
        x32 = x16.float().numpy()
        r16 = R.evaluate(x32, c["P"], "log", EPS)
        x = x16.to(d).requires_grad_(True)
        o = coral(x, c["P"])
        o["loss"].backward()
        assert x.grad.dtype == dtype and _within(float(o["loss"].detach()), r16["loss"])
        # ... half an ulp: 2^-11 / 2^-8 relative, and 2^-25 absolute where the value is a float16 subnormal (below 2^-14)
        tol = R.gradient_bound(x32, c["P"], r16) + np.abs(r16["grad"]) * 2.0 ** -bits + (2.0 ** -25 if dtype == torch.float16 else 0.0)
        assert (np.abs(x.grad.cpu().double().numpy() - r16["grad"]) <= tol).all()
