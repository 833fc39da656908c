"""Target-domain entropy and diversity on the GPU (csrc/infomax.hip: k_im_stats / k_im_final behind mm_im_fwd, k_im_bwd behind
mm_im_bwd; losses.target_entropy) against the float64 reference tests/_infomax_ref.py evaluated on the same fp32 logits.

The C ABI is called directly with the operands of tests/_gpu_rows.py: the logits are a pitched view whose padding is NaN, every
output lies between sentinels that must survive.  Tolerances are those of tests/test_gpu_ce_pair.py, the same arithmetic (fp32
expf / logf per row, fp64 sums): losses and mass within 1e-5 * max(1, |ref|), gradients times n within 1e-5 absolute, count exact."""
import functools

import numpy as np
import pytest
import torch

import _infomax_ref as R
from _gpu_rows import Ints, Rows, abi, dev, vec

pytestmark = pytest.mark.gpu

# (N, P, C)
CASES = {
    "1_0_2": (1, 0, 2),
    "129_0_5": (129, 0, 5),  # one full tile plus a row
    "300_173_11": (300, 173, 11),  # the split inside a tile and off a wave boundary
    "257_1_32": (257, 1, 32),  # widest rows; the LDS pitch C | 1 = 33 stays odd
    "128_128_6": (128, 128, 6),  # P == N: no target row
    "0_0_6": (0, 0, 6),
    "131208_7_5": (131072 + 129 + 7, 7, 5),  # 1026 tiles for the 1024 workgroups of the statistics grid: accumulators carried over
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded fp32 logits 3 * randn, a prior, and the float64 reference with and without it: computed once, never modified."""
    N, P, C = CASES[name]
    rng = np.random.default_rng(4000 + sorted(CASES).index(name))
    x = (3.0 * rng.standard_normal((N, C))).astype(np.float32)
    prior = rng.uniform(0.2, 2.0, C)
    prior = (prior / prior.sum()).astype(np.float32)
    return dict(N=N, P=P, C=C, x=x, prior=prior, ref={k: _ref(x, P, p) for k, p in (("uniform", None), ("prior", prior))})


def _ref(x, P, prior):
    f = R.forward(x, P, None if prior is None else prior.astype(np.float64))
    f["de"], f["dd"] = R.gradients(x, P, None if prior is None else prior.astype(np.float64))
    return f


class _Call:
    """One mm_im_fwd and one mm_im_bwd over pitched, padded operands."""

    def __init__(self, x, N, P, C, prior=None, gout=(1.0, 1.0), ld=None, ld_d=None, run=True):
        L, _lib = abi()
        self.L, self.N, self.P, self.C = L, N, P, C
        self.ld, self.ld_d = C + 3 if ld is None else ld, C + 2 if ld_d is None else ld_d
        self.x = Rows(x, N, C, max(self.ld, C), off=5)
        self.stats, self.mass, self.aux = vec(None, 2), vec(None, C), vec(None, C + 1)
        self.count = Ints(None, 1, dtype=torch.int64)
        self.d = Rows(None, N, C, max(self.ld_d, C), off=3, fill=-12345.0)
        self.prior = None if prior is None else torch.from_numpy(np.ascontiguousarray(prior, np.float32)).to(dev())
        self.gout = torch.tensor(gout, dtype=torch.float32, device=dev())
        self.ws = torch.empty(int(L.mm_im_ws_bytes()), dtype=torch.uint8, device=dev())
        self.stream = _lib.stream()
        if run:
            assert self.fwd() == 0, L.mm_last_error()
            assert self.bwd() == 0, L.mm_last_error()
            torch.cuda.synchronize()

    def fwd(self, **kw):
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, P=self.P, C=self.C, prior=None if self.prior is None else self.prior.data_ptr(),
                 stats=self.stats.ptr, mass=self.mass.ptr, count=self.count.ptr, aux=self.aux.ptr, ws=self.ws.data_ptr(),
                 ws_bytes=self.ws.numel())
        a.update(kw)
        return self.L.mm_im_fwd(a["x"], a["ld"], a["N"], a["P"], a["C"], a["prior"], a["stats"], a["mass"], a["count"], a["aux"], a["ws"],
                                a["ws_bytes"], self.stream)

    def bwd(self, **kw):
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, P=self.P, C=self.C, aux=self.aux.ptr, g=self.gout.data_ptr(), d=self.d.ptr, ld_d=self.ld_d)
        a.update(kw)
        return self.L.mm_im_bwd(a["x"], a["ld"], a["N"], a["P"], a["C"], a["aux"], a["g"], a["d"], a["ld_d"], self.stream)

    def outputs_untouched(self):
        return all(o.untouched() for o in (self.stats, self.mass, self.aux, self.count, self.d))

    def padding_untouched(self):
        return all(o.padding_untouched() for o in (self.stats, self.mass, self.aux, self.count, self.d))


def _close(got, ref):
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


def _check(call, ref, what, gout=(1.0, 1.0)):
    """Losses, mass, count, padding and the gradient (times n) of ``call`` against the reference ``ref``."""
    ent, div = call.stats.get().reshape(2)
    mass, n = call.mass.get().reshape(-1), int(call.count.get()[0])
    want = gout[0] * ref["de"] + gout[1] * ref["dd"]
    got = call.d.get()
    err_m = float(np.abs(mass - ref["mass"]).max())
    err_g = float(np.abs(got - want).max() * max(ref["count"], 1)) if got.size else 0.0
    print(f"{what}: ent {ent:.7f} ref {ref['ent']:.7f}  div {div:.7f} ref {ref['div']:.7f}  max |mass - ref| {err_m:.2e}  "
          f"count {n} ref {ref['count']}  max |n * dgrad| {err_g:.2e}")
    assert n == ref["count"], what
    assert _close(ent, ref["ent"]) and _close(div, ref["div"]) and div >= 0.0, what
    assert err_m <= 1e-5, what
    assert err_g <= 1e-5, what
    assert call.padding_untouched(), what
    assert not call.d.bits()[: call.P].any(), what  # head rows: +0 in every bit
    dead = ~R.counted_rows(call.x.get32(), call.P)
    assert not call.d.bits()[dead].any(), what  # and so is every row that is not counted


@pytest.mark.parametrize("kind", ["uniform", "prior"])
@pytest.mark.parametrize("name", list(CASES))
def test_values_and_gradients_match_the_float64_reference(name, kind):
    c = _case(name)
    call = _Call(c["x"], c["N"], c["P"], c["C"], prior=c["prior"] if kind == "prior" else None)
    _check(call, c["ref"][kind], f"{name} {kind}")
    if c["N"] == c["P"]:  # no target row: zeros, never 0 / 0
        assert call.stats.get().tolist() == [[0.0, 0.0]] and not call.mass.get().any() and int(call.count.get()[0]) == 0
        assert not call.d.bits().any()
    else:
        assert abs(float(call.mass.get().sum()) - 1.0) <= 1e-5


@pytest.mark.parametrize("name", ["300_173_11", "257_1_32"])
def test_uniform_prior_as_null_and_as_an_explicit_vector(name):
    """Not required to be bit-equal (ln(1 / C) against ln of the float32 1 / C): both are held to the reference."""
    c = _case(name)
    explicit = np.full(c["C"], 1.0 / c["C"], np.float32)
    for prior in (None, explicit):
        _check(_Call(c["x"], c["N"], c["P"], c["C"], prior=prior), c["ref"]["uniform"], f"{name} prior {'NULL' if prior is None else '1/C'}")


@pytest.mark.parametrize("gout", [(2.0, 0.0), (0.0, 3.0), (1.0, 1.0)])
def test_upstream_gradients_combine_the_two_terms(gout):
    c = _case("300_173_11")
    _check(_Call(c["x"], c["N"], c["P"], c["C"], prior=c["prior"], gout=gout), c["ref"]["prior"], f"grad_out {gout}", gout)


@pytest.mark.parametrize("name", ["300_173_11", "131208_7_5"])
def test_the_same_call_twice_is_bit_identical(name):
    c = _case(name)
    a, b = (_Call(c["x"], c["N"], c["P"], c["C"], prior=c["prior"]) for _ in range(2))
    for u, v in ((a.stats, b.stats), (a.mass, b.mass), (a.aux, b.aux), (a.d, b.d)):
        assert np.array_equal(u.bits(), v.bits())
    assert a.count.get().tolist() == b.count.get().tolist()


def test_non_finite_target_rows_are_not_counted():
    N, P, C = 300, 60, 6
    x = _case("300_173_11")["x"][:, :C].copy()
    x[P + 1] = np.nan  # a NaN row, a +inf row and a -inf row among the target rows, in both tiles and on the tile's last row
    x[127, 2] = np.inf
    x[200, 5] = -np.inf
    x[299, 0] = np.nan
    x[3] = np.inf  # a head row: never read as a row
    for prior in (None, _case("128_128_6")["prior"]):
        ref = _ref(x, P, prior)
        assert ref["count"] == N - P - 4
        call = _Call(x, N, P, C, prior=prior)
        _check(call, ref, f"non-finite rows, prior {prior is not None}")
        assert np.isfinite(call.d.get()).all() and np.isfinite(call.aux.get()).all()


def test_all_target_rows_non_finite():
    N, P, C = 200, 70, 5
    x = _case("129_0_5")["x"][:N // 2].repeat(2, 0).copy()
    x[P:, 1] = np.nan
    x[P + 5] = np.inf
    x[N - 1] = -np.inf
    call = _Call(x, N, P, C, prior=_case("129_0_5")["prior"], gout=(2.0, 3.0))
    assert call.stats.get().tolist() == [[0.0, 0.0]] and not call.mass.get().any() and int(call.count.get()[0]) == 0
    assert not call.d.bits().any() and not call.aux.get().any() and call.padding_untouched()


def test_saturated_rows_stay_finite():
    x = np.array([[90.0, -90.0, 0.0], [-80.0, 80.0, 80.0], [0.0, 0.0, 0.0]], np.float32)
    ref = _ref(x, 0, None)
    assert abs(ref["ent"] - 0.54364) < 5e-6 and abs(ref["div"] - 0.02418) < 5e-6
    call = _Call(x, 3, 0, 3)
    _check(call, ref, "saturated rows")
    assert np.isfinite(call.d.get()).all() and np.isfinite(call.stats.get()).all()
    # logits as far apart as float32 goes: x - max overflows to -inf, a probability of exactly 0
    far = np.array([[3.0e38, -3.0e38, 0.0], [1.0, 2.0, 3.0]], np.float32)
    call = _Call(far, 2, 0, 3)
    _check(call, _ref(far, 0, None), "3e38 apart")
    assert np.isfinite(call.d.get()).all()


def test_all_zero_logits_give_entropy_one_and_divergence_zero():
    for C in (2, 6, 32):
        call = _Call(np.zeros((130, C), np.float32), 130, 1, C)
        ent, div = call.stats.get().reshape(2)
        print(f"C {C}: ent {ent:.8f} div {div:.3e}")
        assert _close(ent, 1.0) and abs(div) <= 1e-5 and int(call.count.get()[0]) == 129
        assert np.abs(call.d.get()).max() * 129 <= 1e-5


def test_every_limit_is_refused_before_a_launch_and_nothing_is_written():
    c = _case("129_0_5")
    call = _Call(c["x"], c["N"], 40, c["C"], run=False)
    C = c["C"]
    for kw in (dict(C=1), dict(C=33), dict(C=0), dict(ld=C - 1), dict(P=-1), dict(P=c["N"] + 1), dict(N=-1), dict(N=(1 << 31) // C + 1),
               dict(x=None), dict(stats=None), dict(mass=None), dict(count=None), dict(aux=None), dict(ws=None), dict(ws_bytes=call.ws.numel() - 1)):
        assert call.fwd(**kw) == -1, kw
        assert b"im_fwd:" in call.L.mm_last_error(), kw
    for kw in (dict(C=1), dict(C=33), dict(ld=C - 1), dict(ld_d=C - 1), dict(P=-1), dict(P=c["N"] + 1), dict(N=-1), dict(N=(1 << 31) // C + 1),
               dict(x=None), dict(aux=None), dict(g=None), dict(d=None)):
        assert call.bwd(**kw) == -1, kw
        assert b"im_bwd:" in call.L.mm_last_error(), kw
    torch.cuda.synchronize()
    assert call.outputs_untouched()


# ---------------------------------------------------------------------------------------------- losses.target_entropy
def _autograd(pred, leaf, first_row, prior, w=(1.0, 1.0)):
    from mm2d3d_amd.losses import target_entropy

    ent, div, mass, count = target_entropy(pred, first_row, prior)
    assert not mass.requires_grad and not count.requires_grad and mass.grad_fn is None and count.grad_fn is None
    assert mass.dtype == torch.float32 and mass.is_cuda and count.dtype == torch.int64 and count.is_cuda and count.dim() == 0
    assert ent.requires_grad and div.requires_grad and ent.grad_fn is div.grad_fn  # one node
    (w[0] * ent + w[1] * div).backward()
    return ent.detach().item(), div.detach().item(), mass.cpu().double().numpy(), int(count), leaf.grad.detach().cpu()


def test_target_entropy_under_autograd_on_a_leaf():
    c, d = _case("300_173_11"), dev()
    ref = c["ref"]["prior"]
    x = torch.from_numpy(c["x"]).to(d).requires_grad_(True)
    ent, div, mass, n, g = _autograd(x, x, c["P"], c["prior"].tolist(), w=(0.5, 2.0))
    assert n == ref["count"] and _close(ent, ref["ent"]) and _close(div, ref["div"]) and np.abs(mass - ref["mass"]).max() <= 1e-5
    err = float(np.abs(g.double().numpy() - (0.5 * ref["de"] + 2.0 * ref["dd"])).max() * n)
    print(f"leaf: max |n * dgrad| {err:.2e}")
    assert err <= 1e-5 and not g[: c["P"]].view(torch.int32).any()
    # a tensor prior and the sequence are one cached device vector; only the entropy in the loss: the other gradient is zeros
    x2 = torch.from_numpy(c["x"]).to(d).requires_grad_(True)
    _, _, _, _, g2 = _autograd(x2, x2, c["P"], torch.from_numpy(c["prior"]), w=(1.0, 0.0))
    assert float(np.abs(g2.double().numpy() - ref["de"]).max() * n) <= 1e-5
    # ... and with the other scalar left out of the graph altogether (its upstream gradient is None): the same launch, the same bits
    from mm2d3d_amd.losses import target_entropy

    x3 = torch.from_numpy(c["x"]).to(d).requires_grad_(True)
    target_entropy(x3, c["P"], c["prior"].tolist())[0].backward()
    assert torch.equal(x3.grad.cpu().view(torch.int32), g2.view(torch.int32))


def test_target_entropy_on_a_row_slice_of_a_wider_tensor():
    c, d = _case("300_173_11"), dev()
    N, C, lo, first = c["N"], c["C"], 20, 153  # rows [20, 300) of the case, of which [153, 280) are target rows
    wide = torch.full((N, C + 5), float("nan"))
    wide[:, 2 : 2 + C] = torch.from_numpy(c["x"])
    leaf = wide.to(d).requires_grad_(True)
    view = leaf[lo:, 2 : 2 + C]
    assert view.stride(0) == C + 5 and not view.is_contiguous()
    ref = _ref(c["x"][lo:], first, None)
    ent, div, mass, n, g = _autograd(view, leaf, first, None)
    assert n == ref["count"] == N - lo - first and _close(ent, ref["ent"]) and _close(div, ref["div"])
    assert np.abs(mass - ref["mass"]).max() <= 1e-5
    inner = g[lo:, 2 : 2 + C].double().numpy()
    assert float(np.abs(inner - (ref["de"] + ref["dd"])).max() * n) <= 1e-5
    outside = g.clone()
    outside[lo + first :, 2 : 2 + C] = 0
    assert not outside.view(torch.int32).any()  # rows before the slice, head rows and the padding columns: +0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_target_entropy_takes_16_bit_logits(dtype):
    c, d = _case("129_0_5"), dev()
    x16 = torch.from_numpy(c["x"]).to(dtype)
    ref = _ref(x16.float().numpy(), 30, None)
    x = x16.to(d).requires_grad_(True)
    ent, div, mass, n, g = _autograd(x, x, 30, None)
    assert g.dtype == dtype and n == ref["count"] and _close(ent, ref["ent"]) and _close(div, ref["div"])
    # the gradient is rounded once to the input's format: half an ulp of the largest entry (8 / 11 significand bits)
    want = ref["de"] + ref["dd"]
    assert float(np.abs(g.double().numpy() - want).max()) <= 1e-5 / n + np.abs(want).max() * 2.0 ** (-8 if dtype == torch.bfloat16 else -11)
