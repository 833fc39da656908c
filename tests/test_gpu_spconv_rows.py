"""The sparse convolution engines of csrc/spconv.hip (mm_spconv_apply / _packed, mm_spconv_dw, _bf16, _f16, mm_spconv_dw_partial +
mm_spconv_dw_reduce_batch), csrc/ostable.hip (mm_os_table_build) and csrc/osconv.hip (mm_spconv_os_pack*, mm_spconv_os_apply, _bf16,
_f16), called straight through the C ABI on synthetic rulebooks against the float64 references of tests/_spconv_ref.py.

Inputs are pitched rows with NaN padding, outputs carry a sentinel in rows and padding, workspaces are NaN before a call and as
large as the library's own *_ws_bytes says, index arrays sit between guard values.  Every call runs twice and the second result
must equal the first bit for bit (the engines promise a fixed order).  The comment of a case names the dispatch branch it is there
for; tests/test_spconv_host.py restates the host dispatch and asserts that the case reaches it.

grid inputs (multiples of 1/8 in [-1, 1]): every product is a multiple of 1/64 and every fp32 sum exact, every value exact in bf16
and fp16, so results are compared bit for bit (16-bit outputs as round16 of the exact sum); rows without a rule are +0 on the CSR
path and on the output-stationary engine, and still hold the sentinel on the unique-destination path.

normal inputs: |got - ref| <= bound(class) * abs_sum per element (abs_sum = the same sum over absolute values); 16-bit outputs in
the interval form got in [round16(ref - e), round16(ref + e)], e = bound * abs_sum.

terms inputs: one nonzero channel per input row and one rule per destination row, so every output element is ONE product x * w of
numbers whose bf16 terms are known; |got - ref| <= bound * |x * w| in the default mode, and the same call with MM_SPCONV_TWO_TERMS
must exceed that bound (the control that shows the assertion sees a lost term).

The bounds are not invented: _spconv_ref restates the kernels' arithmetic in float32 (precision and grouping, not lane order), and
the largest error of the restatement against float64 over all normal (terms) cases of a class, measured on the CPU
(test_spconv_host.py repeats the measurement), is

    class              fp32 restatement   bound = 8 x (rounded up)   observed on an MI355X
    apply_fp32         2.63e-07           2.2e-06                    2.51e-07
    apply_split        1.26e-07           1.1e-06                    2.28e-07
    apply_split_terms  1.14e-07           9.1e-07                    1.71e-07
    dw_fp32            1.15e-07           9.2e-07                    1.93e-07
    dw_split           1.16e-07           9.4e-07                    1.39e-07
    dw_bf16            1.10e-07           8.9e-07                    1.10e-07
    dw_fp16            1.09e-07           8.7e-07                    1.30e-07
    os_split           1.55e-07           1.3e-06                    2.15e-07
    os_split_terms     1.12e-07           9.0e-07                    1.70e-07
    os_bf16            8.20e-08           6.6e-07                    2.87e-08
    os_fp16            8.35e-08           6.7e-07                    4.67e-08

Observed: the largest error over the same cases on the device; for the 16-bit outputs (os_bf16, os_fp16) the smallest bound their
values would pass (_spconv_ref.least_allowance).  No bound is taken from the device figure.  The kernel is allowed 8 x the
restatement's error: another summation order and another fma contraction cost a few ulp each."""
import functools
import zlib

import numpy as np
import pytest
import torch

import _spconv_ref as R
from _gpu_rows import SENTINEL, Ints, Rows, abi as _abi, dev as _dev, vec

pytestmark = pytest.mark.gpu

NAN = float("nan")
MM_OK, MM_ERR_ARG, MM_ERR_WORKSPACE = 0, -1, -3
DEFAULT, FP32, TWO_TERMS, DW_NARROW, DW16_ELEM = 0, 1, 2, 4, 8

BOUNDS = dict(apply_fp32=2.2e-06, apply_split=1.1e-06, apply_split_terms=9.1e-07, dw_fp32=9.2e-07, dw_split=9.4e-07, dw_bf16=8.9e-07,
              dw_fp16=8.7e-07, os_split=1.3e-06, os_split_terms=9.0e-07, os_bf16=6.6e-07, os_fp16=6.7e-07)

# ------------------------------------------------------------------------------------------------------------------ rulebooks
_RAGGED27 = (0, 1, 15, 16, 17, 0, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 0, 511, 513, 1, 33, 1024, 1025, 700, 31, 2, 0)


def _uneven(total, K=27):
    w = [1 + k % 7 for k in range(K)]
    s = [total * v // sum(w) for v in w]
    s[-1] += total - sum(s)
    return tuple(s)


RULEBOOKS = {
    "ragged27": dict(K=27, n_out=1500, n_in=1300, sizes=_RAGGED27, unique=False),  # empty first / middle / last bucket, every tile length +- 1
    "ragged8u": dict(K=8, n_out=3000, n_in=900, sizes=(0, 1, 16, 17, 255, 257, 1000, 64), unique=True),  # direct row writes
    "k1": dict(K=1, n_out=200, n_in=200, sizes=(130,), unique=True),
    "k32": dict(K=32, n_out=200, n_in=200, sizes=tuple(32 * (k % 5) for k in range(32)), unique=False),  # MAXK
    "empty": dict(K=27, n_out=70, n_in=70, sizes=(0,) * 27, unique=True),  # R = 0
    "big_lo": dict(K=27, n_out=16384, n_in=16384, sizes=_uneven(199999), unique=False),  # both sides of the two
    "big_hi": dict(K=27, n_out=16384, n_in=16384, sizes=_uneven(200000), unique=False),  # 200 000 thresholds
    "big_tr256": dict(K=27, n_out=12000, n_in=12000, sizes=tuple(9700 + 20 * (k % 11) for k in range(27)), unique=False),  # tr stays 256
}


@functools.lru_cache(maxsize=None)
def rulebook(name):
    c = RULEBOOKS[name]
    return R.make_rulebook(c["K"], c["n_out"], c["n_in"], c["sizes"], 100 + list(RULEBOOKS).index(name), c["unique"])


@functools.lru_cache(maxsize=None)
def _dev_rulebook(key, maker=None):
    rb = rulebook(key) if maker is None else maker(key)
    return {k: Ints(rb[k]) for k in ("src", "dst", "offsets", "csr_off", "csr_pos")}


def _host_ptr(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data


def _nan_ws(nbytes):
    return torch.full(((int(nbytes) + 3) // 4 + 4,), NAN, dtype=torch.float32, device=_dev())


OBSERVED = {}


def _note(key, v):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), v)
    print(f"{key}: {v:.3e} (bound {BOUNDS[key]:.1e}, largest so far {OBSERVED[key]:.3e})")


def _same_bits(a, b, what):
    bad = np.argwhere(a != b)
    assert not len(bad), f"{what}: {len(bad)} elements differ, first at {bad[0]}"


# ============================================================================================ a. mm_spconv_apply / _packed
def _a(rb, Cin, Cout, want, path="csr", ld_in=None, ld_out=None, in_off=0, tr=False, kflip=0, gap=0, mode=DEFAULT, kinds=("grid", "normal")):
    return dict(rb=rb, Cin=Cin, Cout=Cout, want=want, path=path, ld_in=ld_in or Cin + 4, ld_out=ld_out or Cout, in_off=in_off,
                tr=tr, kflip=kflip, gap=gap, mode=mode, kinds=kinds)


_S3 = "k_gather_gemm_s3"
APPLY_CASES = {
    # k_rows_narrow
    "narrow_3_16": _a("ragged27", 3, 16, "k_rows_narrow"),
    "narrow_4_32": _a("ragged27", 4, 32, "k_rows_narrow", gap=5, ld_out=36),
    "narrow_1_5": _a("ragged27", 1, 5, "k_rows_narrow", tr=True, kflip=1),
    # EDGE k_gather_gemm
    "edge_5_7": _a("ragged27", 5, 7, "k_gather_gemm edge k_csr_reduce_scalar"),
    "edge_20_36": _a("ragged27", 20, 36, "k_gather_gemm edge k_csr_reduce_scalar", ld_out=37, tr=True, kflip=1, gap=3),
    "edge_16_3_csr": _a("ragged8u", 16, 3, "k_gather_gemm edge k_csr_reduce_scalar"),
    "edge_16_3_unique": _a("ragged8u", 16, 3, "k_gather_gemm edge", path="unique", ld_out=5),
    "edge_3_16_unique": _a("ragged8u", 3, 16, "k_gather_gemm edge", path="unique"),  # the narrow kernel needs the CSR
    "edge_5_7_unique": _a("ragged8u", 5, 7, "k_gather_gemm edge", path="unique", ld_out=9),
    "edge_16_16_ld17": _a("ragged27", 16, 16, "k_gather_gemm edge k_csr_reduce", ld_in=17),
    "edge_16_16_misaligned": _a("ragged27", 16, 16, "k_gather_gemm edge k_csr_reduce", in_off=1),
    # k_gather_gemm_direct
    "direct_16_16": _a("ragged27", 16, 16, "k_gather_gemm_direct ncbw=1", kflip=1),
    "direct_16_32": _a("ragged27", 16, 32, "k_gather_gemm_direct ncbw=2", tr=True),
    "direct_16_128": _a("ragged27", 16, 128, "k_gather_gemm_direct ncbw=8", gap=7, ld_out=132),
    "direct_16_16_unique": _a("ragged8u", 16, 16, "k_gather_gemm_direct ncbw=1", path="unique", ld_out=20),
    "direct_16_128_unique": _a("ragged8u", 16, 128, "k_gather_gemm_direct ncbw=8", path="unique", tr=True, kflip=1),
    "direct_16_32_unique": _a("ragged8u", 16, 32, "k_gather_gemm_direct ncbw=2", path="unique", gap=2),
    "direct_64_64_fp32_unique": _a("ragged8u", 64, 64, "k_gather_gemm_direct ncbw=4", path="unique", mode=FP32),
    "direct_64_64_fp32": _a("ragged27", 64, 64, "k_gather_gemm_direct ncbw=4", mode=FP32),
    "direct_16_16_k32": _a("k32", 16, 16, "k_gather_gemm_direct ncbw=1"),
    "direct_16_16_big_lo": _a("big_lo", 16, 16, "k_gather_gemm_direct ncbw=1"),  # R = 199 999
    # staged k_gather_gemm
    "staged_16_16_big_hi": _a("big_hi", 16, 16, "k_gather_gemm ncbw=1 tr=128"),  # R = 200 000
    "staged_16_144": _a("ragged27", 16, 144, "k_gather_gemm ncbw=3 nch=3"),  # nine blocks, chunked over blockIdx.y
    "staged_16_144_strided": _a("ragged27", 16, 144, "k_gather_gemm ncbw=3 nch=3", tr=True, kflip=1, gap=9, ld_out=148),
    "staged_16_144_unique": _a("ragged8u", 16, 144, "k_gather_gemm ncbw=3 nch=3", path="unique", ld_out=148),
    # k_gather_gemm_s3 (split products)
    "s3_32_16": _a("ragged27", 32, 16, _S3 + " ncbw=1"),
    "s3_48_48": _a("ragged27", 48, 48, _S3 + " ncbw=3", tr=True, kflip=1),
    "s3_80_80": _a("ragged27", 80, 80, _S3 + " ncbw=5", gap=11, ld_out=84),
    "s3_112_48": _a("ragged27", 112, 48, _S3 + " ncbw=3"),
    "s3_224_112": _a("ragged27", 224, 112, _S3 + " ncbw=1 nch=7"),
    "s3_64_192": _a("ragged27", 64, 192, _S3 + " ncbw=6 nch=2"),  # twelve blocks
    "s3_256_32": _a("ragged27", 256, 32, _S3 + " ncbw=2 beyond_preload"),
    "s3_32_16_unique": _a("ragged8u", 32, 16, _S3 + " ncbw=1", path="unique", ld_out=20),
    "s3_80_80_unique": _a("ragged8u", 80, 80, _S3 + " ncbw=5", path="unique", tr=True, kflip=1),
    "s3_64_192_unique": _a("ragged8u", 64, 192, _S3 + " ncbw=6 nch=2", path="unique", gap=4, ld_out=196),
    "s3_256_32_unique": _a("ragged8u", 256, 32, _S3 + " ncbw=2 beyond_preload", path="unique"),
    "s3_48_48_unique": _a("ragged8u", 48, 48, _S3 + " ncbw=3", path="unique"),
    "s3_112_48_unique": _a("ragged8u", 112, 48, _S3 + " ncbw=3", path="unique", ld_out=52),
    "s3_224_112_unique": _a("ragged8u", 224, 112, _S3 + " ncbw=1 nch=7", path="unique", tr=True),
    "s3_32_16_k32": _a("k32", 32, 16, _S3 + " ncbw=1", kflip=1),
    "s3_64_64_big_tr256": _a("big_tr256", 64, 64, _S3 + " ncbw=4 tr=256"),
    "s3_64_64_two_terms": _a("ragged27", 64, 64, _S3 + " ncbw=4 terms=2", mode=TWO_TERMS, kinds=("grid",)),
    # generic VALU kernels
    "generic_1216_32_csr": _a("k1", 1216, 32, "k_generic_rows", tr=True, kflip=1),
    "generic_1216_32_unique": _a("k1", 1216, 32, "k_generic_rules", path="unique", gap=6, ld_out=36),
}
APPLY_TERMS = ("s3_32_16_unique", "s3_80_80_unique", "s3_256_32_unique", "terms_48_48_csr")
APPLY_CASES["terms_48_48_csr"] = _a("ragged8u", 48, 48, _S3 + " ncbw=3", kinds=("grid",))  # a unique rulebook through the CSR path


def apply_class(c):
    return "apply_split" if c["want"].startswith(_S3) else "apply_fp32"


def _seed(table, name):
    """Of the name alone: a case added to a table leaves the inputs of the others as they are."""
    return 1000 * (zlib.crc32(name.encode()) % 100000)


@functools.lru_cache(maxsize=None)
def apply_inputs(name, kind):
    """Operands and float64 reference of a case: made once, shared, never modified."""
    c = APPLY_CASES[name]
    rb = rulebook(c["rb"])
    lay = R.layout(rb["K"], c["Cin"], c["Cout"], c["tr"], c["kflip"], c["gap"])
    s = _seed(APPLY_CASES, name)
    if kind == "grid":
        x, W = R.grid((rb["n_in"], c["Cin"]), s), R.grid((rb["K"], c["Cin"], c["Cout"]), s + 1)
    elif kind == "normal":
        x, W = R.normal_rows((rb["n_in"], c["Cin"]), s + 2), R.he_weights(rb["K"], c["Cin"], c["Cout"], s + 3)
    else:
        x, W = R.make_terms(kind, rb, c["Cin"], c["Cout"], s + 4)
    flat = R.put_weights(W, lay)
    ref, a = R.apply(x, flat, lay, rb, rb["n_out"])
    if kind == "grid":
        R.assert_grid_exact(a)
    return dict(x=x, flat=flat, lay=lay, ref=ref, abs=a)


def _call_apply(c, d, out, mode=None, Wpk=None, rb_name=None, **over):
    L, lib = _abi()
    rb, dv = rulebook(rb_name or c["rb"]), _dev_rulebook(rb_name or c["rb"])
    lay = d["lay"]
    x = Rows(d["x"], rb["n_in"], c["Cin"], c["ld_in"], 8 + c["in_off"])
    W = vec(d["flat"], fill=NAN)
    R_ = int(rb["offsets"][-1])
    ws_bytes = int(L.mm_spconv_ws_bytes(R_, c["Cin"], c["Cout"], rb["K"]))
    ws = _nan_ws(ws_bytes)
    unique = c["path"] == "unique"
    a = dict(ld_in=c["ld_in"], K=rb["K"], csr_off=dv["csr_off"].ptr, ws_bytes=ws_bytes)
    a.update(over)
    rc = L.mm_spconv_apply_packed(x.ptr, a["ld_in"], c["Cin"], out.ptr, c["ld_out"], c["Cout"], rb["n_out"], dv["src"].ptr, dv["dst"].ptr,
                                  dv["offsets"].ptr, _host_ptr(rb["offsets"]), a["K"], a["csr_off"], dv["csr_pos"].ptr, int(unique), W.ptr,
                                  lay["w_kstride"], lay["s_ci"], lay["s_co"], lay["kflip"], Wpk, c["mode"] if mode is None else mode,
                                  ws.data_ptr(), a["ws_bytes"], lib.stream())
    torch.cuda.synchronize()
    return int(rc)


def _run_apply(c, d, **kw):
    """Two calls into fresh sentinel rows; the second must repeat the first bit for bit."""
    rb = rulebook(c["rb"])
    outs = []
    for _ in range(2):
        out = Rows(None, rb["n_out"], c["Cout"], c["ld_out"], 8, fill=SENTINEL)
        rc = _call_apply(c, d, out, **kw)
        assert rc == MM_OK, (rc, _abi()[0].mm_last_error())
        assert out.padding_untouched(), "padding of the output rows"
        outs.append(out)
    _same_bits(outs[0].bits(), outs[1].bits(), "second run")
    return outs[0]


def _bare(rb):
    return (rb["nbr"] >= 0).sum(0) == 0


def _check_rows_without_rule(c, out, what):
    rb = rulebook(c["rb"])
    bare = _bare(rb)
    assert bare.sum() >= 5
    b = out.bits()[bare]
    if c["path"] == "unique":
        want = np.float32(SENTINEL).view(np.int32)
        assert (b == want).all(), f"{what}: a row without a rule was written on the unique-destination path"
    else:
        assert not b.any(), f"{what}: a row without a rule is not +0 on the CSR path"


def _f32_bits(a):
    return np.asarray(a, np.float64).astype(np.float32).view(np.int32)


@pytest.mark.parametrize("name", list(APPLY_CASES))
def test_apply_against_float64(name):
    c = APPLY_CASES[name]
    rb = rulebook(c["rb"])
    live = ~_bare(rb) if c["path"] == "unique" else np.ones(rb["n_out"], bool)
    for kind in c["kinds"]:
        d = apply_inputs(name, kind)
        out = _run_apply(c, d)
        what = f"{name} {kind}"
        _check_rows_without_rule(c, out, what)
        got = out.get()[live]
        assert np.isfinite(got).all(), f"{what}: padding, a weight hole or workspace garbage was read"
        if kind == "grid":
            _same_bits(out.bits()[live], _f32_bits(d["ref"][live]), what)
        else:
            key = apply_class(c)
            err = R.rel_error(got, d["ref"][live], d["abs"][live])
            _note(key, err)
            assert err <= BOUNDS[key], f"{what}: {err:.3e} of abs_sum exceeds {BOUNDS[key]:.1e}"


@pytest.mark.parametrize("kind", R.TERM_KINDS)
@pytest.mark.parametrize("name", APPLY_TERMS)
def test_apply_single_products_keep_every_term_and_two_terms_do_not(name, kind):
    c = APPLY_CASES[name]
    rb = rulebook(c["rb"])
    d = apply_inputs(name, kind)
    live = ~_bare(rb)
    assert (d["abs"][live] > 0).all() and np.array_equal(d["abs"], np.abs(d["ref"]))  # single products
    bound = BOUNDS["apply_split_terms"]
    err = R.rel_error(_run_apply(c, d, mode=DEFAULT).get()[live], d["ref"][live], d["abs"][live])
    _note("apply_split_terms", err)
    assert err <= bound, f"{name} {kind}: {err:.3e} of |x * w| exceeds {bound:.1e} in the default mode"
    two = R.rel_error(_run_apply(c, d, mode=TWO_TERMS).get()[live], d["ref"][live], d["abs"][live])
    print(f"{name} {kind}: two terms {two:.3e}")
    assert two > bound, f"{name} {kind}: MM_SPCONV_TWO_TERMS stays within the bound ({two:.3e}): the assertion cannot see a lost term"


def _pack_descs(items):
    """The descriptor table of mm_spconv_os_pack_batch: {W, Wf, K, Cin, Cout, nq, ncb, w_kstride, s_ci, s_co, kflip, blk_end}."""
    L, _ = _abi()
    assert int(L.mm_spconv_os_pack_desc_fields()) == 12
    tab, end = np.zeros((len(items), 12), np.int64), 0
    for i, (W, Wf, lay) in enumerate(items):
        end += int(L.mm_spconv_os_pack_blocks(lay["K"], lay["Cin"], lay["Cout"]))
        tab[i] = (W, Wf, lay["K"], lay["Cin"], lay["Cout"], (lay["Cin"] + 31) // 32, (lay["Cout"] + 15) // 16, lay["w_kstride"],
                  lay["s_ci"], lay["s_co"], lay["kflip"], end)
    return torch.from_numpy(tab.reshape(-1)).to(_dev()), end


def _frag_buffer(L, lay, fn="mm_spconv_os_pack_bytes"):
    return torch.full((int(getattr(L, fn)(lay["K"], lay["Cin"], lay["Cout"])) // 4,), NAN, dtype=torch.float32, device=_dev())


def test_apply_with_packed_fragments_equals_its_own_pack():
    """Wpk from mm_spconv_os_pack (one layer) and from mm_spconv_os_pack_batch (two descriptors): bit-identical to Wpk = NULL."""
    L, lib = _abi()
    names = ("s3_48_48", "s3_80_80", "s3_32_16_unique")
    ds = {n: apply_inputs(n, "normal") for n in names}
    Ws = {n: vec(ds[n]["flat"], fill=NAN) for n in names}
    fr = {n: _frag_buffer(L, ds[n]["lay"]) for n in names}
    lay = ds[names[0]]["lay"]
    lib.check(L.mm_spconv_os_pack(Ws[names[0]].ptr, lay["w_kstride"], lay["s_ci"], lay["s_co"], lay["kflip"], lay["K"], lay["Cin"], lay["Cout"],
                                  fr[names[0]].data_ptr(), lib.stream()), "os_pack")
    descs, total = _pack_descs([(Ws[n].ptr, fr[n].data_ptr(), ds[n]["lay"]) for n in names[1:]])
    lib.check(L.mm_spconv_os_pack_batch(descs.data_ptr(), 2, total, lib.stream()), "os_pack_batch")
    torch.cuda.synchronize()
    for n in names:
        assert not torch.isnan(fr[n]).any(), f"{n}: a fragment was not written"
        c = APPLY_CASES[n]
        own, packed = _run_apply(c, ds[n]), _run_apply(c, ds[n], Wpk=fr[n].data_ptr())
        _same_bits(own.bits(), packed.bits(), f"{n}: packed fragments")


@pytest.mark.parametrize("pair", [(3, 16), (5, 7), (16, 16), (64, 64), (1216, 32)], ids=lambda p: f"{p[0]}_{p[1]}")
def test_apply_on_an_empty_rulebook(pair):
    rb = rulebook("empty")
    for path in ("csr", "unique"):
        c = _a("empty", pair[0], pair[1], "", path=path, ld_out=pair[1] + 4)
        lay = R.layout(rb["K"], *pair)
        d = dict(x=R.grid((rb["n_in"], pair[0]), 5), flat=R.put_weights(R.grid((rb["K"],) + pair, 6), lay), lay=lay)
        out = _run_apply(c, d)
        if path == "unique":
            assert out.untouched(), f"{pair}: written without a rule"
        else:
            assert not out.bits().any(), f"{pair}: not +0 everywhere"


def apply_least_workspace(c, rb):
    """The smallest workspace the call takes (mm_spconv_ws_bytes rounds up): the tmp rows of the CSR path, rounded up to 256 bytes,
    and the weight fragments - fp32 ones, or three bf16 terms per element with Cin padded to 32 on the split path."""
    tmp = 0 if c["path"] == "unique" else (int(rb["offsets"][-1]) * c["Cout"] * 4 + 255) // 256 * 256
    frag = rb["K"] * R.cdiv(c["Cin"], 16) * R.cdiv(c["Cout"], 16) * 1024
    if c["want"].startswith(_S3):
        frag = max(frag, rb["K"] * R.cdiv(c["Cin"], 32) * R.cdiv(c["Cout"], 16) * 3072)
    return tmp + frag


@pytest.mark.parametrize("name", ["s3_48_48", "direct_16_16", "s3_32_16_unique"])
def test_apply_refusals_write_nothing(name):
    c = APPLY_CASES[name]
    d = apply_inputs(name, "grid")
    rb = rulebook(c["rb"])
    out = Rows(None, rb["n_out"], c["Cout"], c["ld_out"], 8, fill=SENTINEL)
    L, _ = _abi()
    exact = apply_least_workspace(c, rb)
    assert exact <= int(L.mm_spconv_ws_bytes(int(rb["offsets"][-1]), c["Cin"], c["Cout"], rb["K"]))
    calls = [("K = 33", dict(K=33), (MM_ERR_ARG,)), ("ld_in < Cin", dict(ld_in=c["Cin"] - 4), (MM_ERR_ARG,)),
             ("workspace one byte short", dict(ws_bytes=exact - 1), (MM_ERR_ARG, MM_ERR_WORKSPACE))]
    if c["path"] != "unique":
        calls.append(("no CSR", dict(csr_off=None), (MM_ERR_ARG,)))
    wrong = {}
    for what, over, want in calls:
        rc = _call_apply(c, d, out, **over)
        if rc not in want or b"spconv_apply" not in (L.mm_last_error() or b""):
            wrong[what] = (rc, L.mm_last_error())
    assert not wrong, wrong
    assert out.untouched(), "a refused call has written"
    assert _call_apply(c, d, out, ws_bytes=exact) == MM_OK
    _same_bits(out.bits(), _run_apply(c, d).bits(), "the least workspace")


# ================================================================================================== b. the weight gradient
def _d(rb, Cin, Cout, want, rows="fp32", mode=DEFAULT, twin=None, kinds=("grid", "normal")):
    return dict(rb=rb, Cin=Cin, Cout=Cout, want=want, rows=rows, mode=mode, twin=twin, kinds=kinds)


DW_CASES = {
    "generic_3_16": _d("ragged27", 3, 16, "k_dw_generic"),
    "generic_5_7": _d("ragged27", 5, 7, "k_dw_generic"),
    "generic_5_7_k32": _d("k32", 5, 7, "k_dw_generic"),
    "direct_32_32_fp32": _d("ragged27", 32, 32, "k_dw_direct tile=2x2", mode=FP32),
    "wide_16_96_lo": _d("big_lo", 16, 96, "k_dw_direct_s3 tile=1x3", twin=DW_NARROW, kinds=("grid",)),
    "wide_96_96_lo": _d("big_lo", 96, 96, "k_dw_direct_s3 tile=3x3", twin=DW_NARROW, kinds=("grid",)),
    "wide_160_80_lo": _d("big_lo", 160, 80, "k_dw_direct_s3 tile=4x3", twin=DW_NARROW, kinds=("grid",)),
    "wide_16_96_hi": _d("big_hi", 16, 96, "k_dw_direct_s3 tile=1x6 wide", twin=DW_NARROW),
    "wide_96_96_hi": _d("big_hi", 96, 96, "k_dw_direct_s3 tile=6x3 wide", twin=DW_NARROW, kinds=("grid",)),
    "wide_160_80_hi": _d("big_hi", 160, 80, "k_dw_direct_s3 tile=5x5 wide", twin=DW_NARROW, kinds=("grid",)),
}
for _rb in ("ragged27", "ragged8u", "k32"):
    for _ci, _co, _t in ((16, 16, "1x1"), (32, 48, "2x3"), (80, 80, "3x3")):
        DW_CASES[f"split_{_ci}_{_co}_{_rb}"] = _d(_rb, _ci, _co, f"k_dw_direct_s3 tile={_t}")
for _fmt in ("bf16", "fp16"):
    for _rb in ("ragged27", "big_hi"):
        for _ci, _co, _t in ((16, 16, "1x1"), (48, 96, "3x3"), (112, 112, "4x4")):
            DW_CASES[f"{_fmt}_{_ci}_{_co}_{_rb}"] = _d(_rb, _ci, _co, f"k_dw_tr16 tile={_t}", rows=_fmt, twin=DW16_ELEM,
                                                       kinds=("grid", "normal") if (_rb, _ci) != ("big_hi", 112) else ("grid",))


def dw_class(c):
    if c["rows"] != "fp32":
        return "dw_" + c["rows"]
    return "dw_split" if "_s3" in c["want"] else "dw_fp32"


@functools.lru_cache(maxsize=None)
def dw_inputs(name, kind):
    c = DW_CASES[name]
    rb = rulebook(c["rb"])
    s = _seed(DW_CASES, name) + 500000
    fmt = None if c["rows"] == "fp32" else c["rows"]
    shape = (rb["K"], c["Cin"], c["Cout"])
    if kind == "grid":
        x, g, prev = R.grid((rb["n_in"], c["Cin"]), s), R.grid((rb["n_out"], c["Cout"]), s + 1), R.grid(shape, s + 2)
    else:
        x, g = R.normal_rows((rb["n_in"], c["Cin"]), s + 3, fmt), R.normal_rows((rb["n_out"], c["Cout"]), s + 4, fmt)
        prev = R.normal_rows(shape, s + 5)
    ref, a = R.dw(x, g, rb)
    if kind == "grid":
        R.assert_grid_exact(a + 1)
    return dict(x=x, g=g, prev=prev, ref=ref, abs=a)


def _dw_operands(c, d):
    rb = rulebook(c["rb"])
    pad = 4 if c["rows"] == "fp32" else 8  # ld a multiple of 4 (fp32 rows) or 8 (16-bit rows), 16-byte aligned
    dt = torch.float32 if c["rows"] == "fp32" else c["rows"]
    x = Rows(d["x"], rb["n_in"], c["Cin"], R.cdiv(c["Cin"], pad) * pad + pad, 8, dtype=dt)
    g = Rows(d["g"], rb["n_out"], c["Cout"], R.cdiv(c["Cout"], pad) * pad + 2 * pad, 8, dtype=dt)
    return x, g


def _call_dw(c, d, dW, accumulate, mode, ops=None):
    L, lib = _abi()
    rb, dv = rulebook(c["rb"]), _dev_rulebook(c["rb"])
    x, g = ops or _dw_operands(c, d)
    ws_bytes = int(L.mm_spconv_dw_ws_bytes(_host_ptr(rb["offsets"]), rb["K"], c["Cin"], c["Cout"]))
    ws = _nan_ws(ws_bytes)
    fn = {"fp32": L.mm_spconv_dw, "bf16": L.mm_spconv_dw_bf16, "fp16": L.mm_spconv_dw_f16}[c["rows"]]
    rc = fn(x.ptr, x.view.stride(0), c["Cin"], g.ptr, g.view.stride(0), c["Cout"], dv["src"].ptr, dv["dst"].ptr, _host_ptr(rb["offsets"]),
            rb["K"], dW.ptr, accumulate, mode, ws.data_ptr(), ws_bytes, lib.stream())
    torch.cuda.synchronize()
    return int(rc)


def _run_dw(c, d, accumulate, mode):
    n = rulebook(c["rb"])["K"] * c["Cin"] * c["Cout"]
    ops, outs = _dw_operands(c, d), []
    for _ in range(2):
        dW = vec(d["prev"], fill=SENTINEL) if accumulate else vec(None, n, fill=NAN)
        assert _call_dw(c, d, dW, accumulate, mode, ops) == MM_OK, _abi()[0].mm_last_error()
        assert dW.padding_untouched()
        outs.append(dW)
    _same_bits(outs[0].bits(), outs[1].bits(), "second run")
    return outs[0]


@pytest.mark.parametrize("name", list(DW_CASES))
def test_dw_against_float64(name):
    c = DW_CASES[name]
    rb = rulebook(c["rb"])
    shape = (rb["K"], c["Cin"], c["Cout"])
    empty = np.diff(rb["offsets"]) == 0
    for kind in c["kinds"]:
        d = dw_inputs(name, kind)
        for acc in (0, 1):
            what = f"{name} {kind} accumulate = {acc}"
            dW = _run_dw(c, d, acc, c["mode"])
            bits, got = dW.bits().reshape(shape), dW.get().reshape(shape)
            assert not np.isnan(got).any(), f"{what}: a NaN survived"
            if acc:
                _same_bits(bits[empty], _f32_bits(d["prev"][empty]), f"{what}: empty buckets")
            else:
                assert not bits[empty].any(), f"{what}: the slab of an empty bucket is not +0"
            want, allow = d["ref"] + (d["prev"] if acc else 0.0), d["abs"] + (np.abs(d["prev"]) if acc else 0.0)
            if kind == "grid":
                _same_bits(bits, _f32_bits(want), what)
            else:
                key = dw_class(c)
                err = R.rel_error(got, want, allow)
                _note(key, err)
                assert err <= BOUNDS[key], f"{what}: {err:.3e} of abs_sum exceeds {BOUNDS[key]:.1e}"
    if c["twin"] is not None:  # narrow tiles / element gathers: the same slab sums, on inputs whose sums round
        d = dw_inputs(name, "normal")
        for acc in (0, 1):
            _same_bits(_run_dw(c, d, acc, c["mode"] | c["twin"]).bits(), _run_dw(c, d, acc, c["mode"]).bits(), f"{name} accumulate = {acc}: mode | {c['twin']}")


@pytest.mark.parametrize("rows", ["fp32", "bf16", "fp16"])
def test_dw_on_an_empty_rulebook(rows):
    c = _d("empty", 16, 32, "", rows=rows)
    rb = rulebook("empty")
    d = dict(x=R.grid((rb["n_in"], 16), 1), g=R.grid((rb["n_out"], 32), 2), prev=R.grid((27, 16, 32), 3))
    assert not _run_dw(c, d, 0, DEFAULT).bits().any(), "accumulate = 0: not +0"
    _same_bits(_run_dw(c, d, 1, DEFAULT).bits().reshape(-1), _f32_bits(d["prev"]).reshape(-1), "accumulate = 1: the prefill")


@pytest.mark.parametrize("rows", ["bf16", "fp16"])
def test_dw_refuses_16_bit_rows_it_cannot_read_16_bytes_at_a_time(rows):
    """MM_ERR_ARG with nothing written; the operands stay inside their buffers and no kernel sees them."""
    L, lib = _abi()
    c = _d("ragged27", 16, 32, "", rows=rows)
    rb, dv = rulebook("ragged27"), _dev_rulebook("ragged27")
    x, g = Rows(None, rb["n_in"], 16, 32, 8, fill=1.0, dtype=rows), Rows(None, rb["n_out"], 32, 48, 8, fill=1.0, dtype=rows)
    dW = vec(None, 27 * 16 * 32)
    ws_bytes = int(L.mm_spconv_dw_ws_bytes(_host_ptr(rb["offsets"]), 27, 16, 32))
    ws = _nan_ws(ws_bytes)
    fn = {"bf16": L.mm_spconv_dw_bf16, "fp16": L.mm_spconv_dw_f16}[rows]

    def call(xp=x.ptr, ld_in=32, gp=g.ptr, ld_do=48, mode=DEFAULT, Cin=16):
        return int(fn(xp, ld_in, Cin, gp, ld_do, 32, dv["src"].ptr, dv["dst"].ptr, _host_ptr(rb["offsets"]), 27, dW.ptr, 0, mode, ws.data_ptr(),
                      ws_bytes, lib.stream()))

    calls = {"in alignment": lambda: call(xp=x.ptr + 2), "dout alignment": lambda: call(gp=g.ptr + 8), "ld_in % 8": lambda: call(ld_in=28),
             "ld_do % 8": lambda: call(ld_do=44), "ld_in < Cin": lambda: call(ld_in=8, mode=DW16_ELEM), "ld_do < Cout": lambda: call(ld_do=24),
             "Cin % 16": lambda: call(Cin=8)}
    wrong = {}
    for what, f in calls.items():
        rc = f()
        if rc != MM_ERR_ARG or b"spconv_dw" not in (L.mm_last_error() or b""):
            wrong[what] = (rc, L.mm_last_error())
    torch.cuda.synchronize()
    assert not wrong, wrong
    assert dW.untouched() and torch.isnan(ws).all(), "a refused call has written"
    assert call(xp=x.ptr + 2, ld_in=30, mode=DW16_ELEM) == MM_OK  # the element gathers take any 2-byte address
    torch.cuda.synchronize()
    assert dW.padding_untouched() and not np.isnan(dW.get()).any()


def test_dw_partial_and_batched_reduce_equal_three_single_calls():
    """Three layers of different (Cin, Cout, K, accumulate), their slabs by mm_spconv_dw_partial, then ONE mm_spconv_dw_reduce_batch
    (descriptor rows as scn/ops.py builds them): bit-identical to three mm_spconv_dw calls."""
    L, lib = _abi()
    layers = (("split_16_16_ragged27", 0), ("split_32_48_ragged8u", 1), ("generic_5_7_k32", 0))
    nr = (int(L.mm_spconv_dw_desc_bytes()) - 32) // 4
    assert nr >= 33  # blk_start[33], and what pads the row to a multiple of 8 bytes
    tab = np.zeros((len(layers), 8 + nr), np.int32)
    ptrs = tab[:, :4].view(np.int64)
    keep, singles, sinks, first = [], [], [], 0
    for i, (name, acc) in enumerate(layers):
        c, d = DW_CASES[name], dw_inputs(name, "normal")
        rb, dv = rulebook(c["rb"]), _dev_rulebook(c["rb"])
        singles.append(_run_dw(c, d, acc, c["mode"]))
        ne, K = c["Cin"] * c["Cout"], rb["K"]
        sink = vec(d["prev"], fill=SENTINEL) if acc else vec(None, K * ne, fill=NAN)
        x, g = _dw_operands(c, d)
        nbytes = int(L.mm_spconv_dw_ws_bytes(_host_ptr(rb["offsets"]), K, c["Cin"], c["Cout"]))
        partial = _nan_ws(nbytes)
        row = np.zeros(nr, np.int32)
        lib.check(L.mm_spconv_dw_partial(0, x.ptr, x.view.stride(0), c["Cin"], g.ptr, g.view.stride(0), c["Cout"], dv["src"].ptr, dv["dst"].ptr,
                                         _host_ptr(rb["offsets"]), K, c["mode"], partial.data_ptr(), nbytes, row.ctypes.data, lib.stream()),
                  "dw_partial")
        ptrs[i, 0], ptrs[i, 1] = partial.data_ptr(), sink.ptr
        tab[i, 4:8] = (ne, K, acc, first)
        tab[i, 8:] = row
        first += int(L.mm_spconv_dw_reduce_blocks(ne, K))
        keep.append((x, g, partial))
        sinks.append(sink)
    descs = torch.from_numpy(tab.reshape(-1)).to(_dev())
    lib.check(L.mm_spconv_dw_reduce_batch(descs.data_ptr(), len(layers), first, lib.stream()), "dw_reduce_batch")
    torch.cuda.synchronize()
    for (name, _), single, sink in zip(layers, singles, sinks):
        assert sink.padding_untouched(), name
        _same_bits(sink.bits(), single.bits(), f"{name}: batched reduce")


# ========================================================================================== c. the output-stationary engine
OS_TABLES = {f"k{K}_n{n}": dict(K=K, n=n, n_in=max(n // 2, 1), up=False) for K in (27, 8) for n in (1, 63, 64, 65, 1000, 65536, 131072)}
OS_TABLES["up_n1000"] = dict(K=8, n=1000, n_in=300, up=True)
OS_TABLES["up_n65"] = dict(K=8, n=65, n_in=20, up=True)
OS_TABLES["k27_n33280"] = dict(K=27, n=33280, n_in=20000, up=False)


@functools.lru_cache(maxsize=None)
def os_rulebook(name):
    c = OS_TABLES[name]
    return R.make_nbr_mixture(c["K"], c["n"], c["n_in"], 7000 + list(OS_TABLES).index(name), c["up"])


@functools.lru_cache(maxsize=None)
def os_table_ref(name):
    return R.os_table(os_rulebook(name)["nbr"])


def _build_table(name, sort_merge):
    L, lib = _abi()
    c, rb, t = OS_TABLES[name], os_rulebook(name), os_table_ref(name)
    nbr = Ints(rb["nbr"])
    dst, nbrp, tmask = Ints(None, t["npad"], fill=-9), Ints(None, c["K"] * t["npad"], fill=-9), Ints(None, t["nt"], fill=-9)
    ws_bytes = int(L.mm_os_table_ws_bytes(c["n"], c["K"]))
    ws = _nan_ws(ws_bytes)
    lib.check(L.mm_os_table_build(nbr.ptr, c["K"], c["n"], R.TILE, sort_merge, dst.ptr, nbrp.ptr, tmask.ptr, ws.data_ptr(), ws_bytes, lib.stream()),
              "os_table_build")
    torch.cuda.synchronize()
    assert nbr.padding_untouched() and dst.padding_untouched() and nbrp.padding_untouched() and tmask.padding_untouched(), name
    return dst, nbrp, tmask


@pytest.mark.parametrize("sort_merge", [0, 1], ids=["onesweep", "merge"])
@pytest.mark.parametrize("name", list(OS_TABLES))
def test_os_table_is_the_stable_sort_by_neighbour_mask(name, sort_merge):
    t = os_table_ref(name)
    dst, nbrp, tmask = _build_table(name, sort_merge)
    _same_bits(dst.get(), t["dst"], f"{name}: dst")
    _same_bits(nbrp.get().reshape(t["nbrp"].shape), t["nbrp"], f"{name}: nbrp")
    _same_bits(tmask.get().view(np.uint32), t["tmask"], f"{name}: tmask")


def _o(table, Cin, Cout, want, tr=False, kflip=0, kinds=("grid", "normal")):
    return dict(table=table, Cin=Cin, Cout=Cout, want=want, tr=tr, kflip=kflip, kinds=kinds)


OS_CASES = {
    # 16-wave one-block form
    "w16_16_16": _o("k27_n1000", 16, 16, "nw=16 1x1"),
    "w16_48_48": _o("k27_n1000", 48, 48, "nw=16 1x3", tr=True, kflip=1),
    "w16_80_80": _o("k27_n1000", 80, 80, "nw=16 1x5"),
    "w16_224_112": _o("k27_n1000", 224, 112, "nw=16 1x7", tr=True, kflip=1),
    # 8-wave form
    "w8_k8_16_32": _o("k8_n1000", 16, 32, "nw=8 1x2"),
    "w8_up_80_80": _o("up_n1000", 80, 80, "nw=8 1x5", tr=True, kflip=1),
    "w8_two_blocks_48_112": _o("k27_n33280", 48, 112, "nw=8 2x3 1x1"),
    # 4-wave form
    "w4_16_16": _o("k27_n131072", 16, 16, "nw=4 1x1"),
    "w4_32_64": _o("k27_n65536", 32, 64, "nw=4 2x2"),
    "w4_32_96": _o("k27_n65536", 32, 96, "nw=4 3x2", tr=True, kflip=1),
    "w4_48_112": _o("k27_n65536", 48, 112, "nw=4 3x1 2x2"),
    "w4_k8_32_64": _o("k8_n65536", 32, 64, "nw=4 2x2", tr=True, kflip=1),
    # the edges of the tile table
    "n1_16_16": _o("k27_n1", 16, 16, "nw=16 1x1"),
    "n65_48_48": _o("k27_n65", 48, 48, "nw=16 1x3"),
}
OS_TERMS = ("w8_up_80_80",)
OS_EQUALS_APPLY = ("w16_80_80", "w8_two_blocks_48_112")
OS_FMTS = ("fp32", "bf16", "fp16")


def os_class(fmt):
    return "os_split" if fmt == "fp32" else "os_" + fmt


@functools.lru_cache(maxsize=None)
def os_inputs(name, kind, fmt):
    c = OS_CASES[name]
    rb = os_rulebook(c["table"])
    f16 = None if fmt == "fp32" else fmt
    lay = R.layout(rb["K"], c["Cin"], c["Cout"], c["tr"], c["kflip"])
    s = _seed(OS_CASES, name) + 900000
    if kind == "grid":
        x, W = R.grid((rb["n_in"], c["Cin"]), s), R.grid((rb["K"], c["Cin"], c["Cout"]), s + 1)
    elif kind == "normal":  # 16-bit rows: weights that are 16-bit numbers already, so the one 16-bit term the engine keeps is exact
        x, W = R.normal_rows((rb["n_in"], c["Cin"]), s + 2, f16), R.he_weights(rb["K"], c["Cin"], c["Cout"], s + 3, f16)
    else:
        x, W = R.make_terms(kind, rb, c["Cin"], c["Cout"], s + 4)
    flat = R.put_weights(W, lay)
    ref, a = R.apply(x, flat, lay, rb, rb["n_out"])
    if kind == "grid":
        R.assert_grid_exact(a)
    return dict(x=x, flat=flat, lay=lay, ref=ref, abs=a)


@functools.lru_cache(maxsize=None)
def _dev_table(name):
    t = os_table_ref(name)
    return Ints(t["dst"]), Ints(t["nbrp"]), Ints(t["tmask"].view(np.int32))


def _run_os(c, d, fmt):
    L, lib = _abi()
    rb, t = os_rulebook(c["table"]), os_table_ref(c["table"])
    dst, nbrp, tmask = _dev_table(c["table"])
    lay = d["lay"]
    sfx = {"fp32": "", "bf16": "_bf16", "fp16": "_f16"}[fmt]
    dt, pad = (torch.float32, 4) if fmt == "fp32" else (fmt, 8)
    W = vec(d["flat"], fill=NAN)
    Wf = _frag_buffer(L, lay, "mm_spconv_os_pack_bytes" if fmt == "fp32" else "mm_spconv_os_pack_bytes_bf16")
    lib.check(getattr(L, "mm_spconv_os_pack" + sfx)(W.ptr, lay["w_kstride"], lay["s_ci"], lay["s_co"], lay["kflip"], lay["K"], lay["Cin"],
                                                    lay["Cout"], Wf.data_ptr(), lib.stream()), "os_pack")
    x = Rows(d["x"], rb["n_in"], c["Cin"], c["Cin"] + pad, 8, dtype=dt)
    outs = []
    for _ in range(2):
        out = Rows(None, rb["n_out"], c["Cout"], c["Cout"] + 4, 8, fill=SENTINEL, dtype=dt)
        lib.check(getattr(L, "mm_spconv_os_apply" + sfx)(x.ptr, c["Cin"] + pad, c["Cin"], out.ptr, c["Cout"] + 4, c["Cout"], Wf.data_ptr(), rb["K"],
                                                         dst.ptr, nbrp.ptr, tmask.ptr, t["nt"], R.TILE, lib.stream()), "os_apply")
        torch.cuda.synchronize()
        assert out.padding_untouched(), "padding of the output rows"
        outs.append(out)
    _same_bits(outs[0].bits(), outs[1].bits(), "second run")
    return outs[0]


@pytest.mark.parametrize("fmt", OS_FMTS)
@pytest.mark.parametrize("name", list(OS_CASES))
def test_os_apply_against_float64(name, fmt):
    c = OS_CASES[name]
    rb = os_rulebook(c["table"])
    bare = (rb["nbr"] >= 0).sum(0) == 0
    for kind in c["kinds"]:
        d = os_inputs(name, kind, fmt)
        out = _run_os(c, d, fmt)
        what = f"{name} {fmt} {kind}"
        assert not out.bits()[bare].any(), f"{what}: a row without a neighbour is not +0"
        got = out.get()
        assert np.isfinite(got).all(), f"{what}: padding or an absent neighbour was read"
        key = os_class(fmt)
        if kind == "grid":
            _same_bits(out.bits(), _f32_bits(d["ref"]) if fmt == "fp32" else R.bits16(d["ref"], fmt), what)
        elif fmt == "fp32":
            err = R.rel_error(got, d["ref"], d["abs"])
            _note(key, err)
            assert err <= BOUNDS[key], f"{what}: {err:.3e} of abs_sum exceeds {BOUNDS[key]:.1e}"
        else:
            ok = R.in_interval(got, d["ref"], BOUNDS[key] * d["abs"], fmt)
            _note(key, R.least_allowance(got, d["ref"], d["abs"], fmt))
            assert ok.all(), f"{what}: {(~ok).sum()} elements outside [round16(ref - e), round16(ref + e)], first at {np.argwhere(~ok)[0]}"


@pytest.mark.parametrize("kind", R.TERM_KINDS)
@pytest.mark.parametrize("name", OS_TERMS)
def test_os_apply_single_products_keep_every_term(name, kind):
    c, d = OS_CASES[name], os_inputs(name, kind, "fp32")
    assert (d["abs"] > 0).all() and np.array_equal(d["abs"], np.abs(d["ref"]))
    err = R.rel_error(_run_os(c, d, "fp32").get(), d["ref"], d["abs"])
    _note("os_split_terms", err)
    assert err <= BOUNDS["os_split_terms"], f"{name} {kind}: {err:.3e} of |x * w| exceeds {BOUNDS['os_split_terms']:.1e}"


@pytest.mark.parametrize("name", OS_EQUALS_APPLY)
def test_os_apply_equals_the_gather_engine_bit_for_bit(name):
    """Cin >= 32: "the same products and order as the split engines of spconv.hip" - mm_spconv_apply on the rulebook of the same nbr."""
    c, d = OS_CASES[name], os_inputs(name, "normal", "fp32")
    rb = os_rulebook(c["table"])
    ca = _a(c["table"], c["Cin"], c["Cout"], "", ld_out=c["Cout"] + 4)
    assert c["Cin"] >= 32 and R.apply_branch(int(rb["offsets"][-1]), c["Cin"], c["Cout"], rb["K"], False, ca["ld_in"], ca["ld_out"])["kernel"] == _S3
    L, lib = _abi()
    dv = {k: Ints(rb[k]) for k in ("src", "dst", "offsets", "csr_off", "csr_pos")}
    x = Rows(d["x"], rb["n_in"], c["Cin"], ca["ld_in"], 8)
    W = vec(d["flat"], fill=NAN)
    out = Rows(None, rb["n_out"], c["Cout"], ca["ld_out"], 8, fill=SENTINEL)
    ws_bytes = int(L.mm_spconv_ws_bytes(int(rb["offsets"][-1]), c["Cin"], c["Cout"], rb["K"]))
    ws, lay = _nan_ws(ws_bytes), d["lay"]
    lib.check(L.mm_spconv_apply(x.ptr, ca["ld_in"], c["Cin"], out.ptr, ca["ld_out"], c["Cout"], rb["n_out"], dv["src"].ptr, dv["dst"].ptr,
                                dv["offsets"].ptr, _host_ptr(rb["offsets"]), rb["K"], dv["csr_off"].ptr, dv["csr_pos"].ptr, 0, W.ptr,
                                lay["w_kstride"], lay["s_ci"], lay["s_co"], lay["kflip"], DEFAULT, ws.data_ptr(), ws_bytes, lib.stream()), "apply")
    torch.cuda.synchronize()
    _same_bits(_run_os(c, d, "fp32").bits(), out.bits(), name)
