"""Host checks of Fourier domain adaptation: the float64 FFT reference (tests/_fda_ref.py) against an independent partial-DFT
evaluation of the same formula, the band of the loaders' image sizes, train_kwargs["fda_beta"] / ["fda_image_norm"] in the
constructor (mm2d3d_amd/fda.py), the refusals of fda_transfer, and the declarations and argument checks of mm_fda_ws_bytes /
mm_fda_transfer (include/mm2d3d.h), every one of which is decided before any device call.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _fda_ref as R

NORM = R.NORM


def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"), dict(gc_freeze=False, **kw))


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("H,W,band,norm", [(9, 14, 1, None), (10, 13, 2, None), (16, 16, 0, None), (16, 16, 3, None), (37, 64, 3, None),
                                           (37, 64, 3, NORM), (9, 14, 4, None)])
def test_fft_reference_matches_the_partial_dft(H, W, band, norm):
    """Both are float64 evaluations of one formula and differ by rounding alone: the FFT's, 2^-53 * log2(HW) * the amplitudes (up
    to HW * max |src|) / HW, some 1e-13 on 0..255 data.  Bound: 1e-10 * max |src|."""
    src, trg = R.inputs(3, 2, 3, H, W, seed=H * W + band, zero_channel=1)
    if norm is not None:
        src, trg = R.normalised(src, norm), R.normalised(trg, norm)
    assert R.assert_phases_defined(src, band, norm) > 0  # the zeroed channel takes the angle(0) = 0 branch
    a, b = R.transfer(src, trg, band, norm), R.transfer_partial(src, trg, band, norm)
    err, top = np.abs(a["img"] - b["img"]).max(), np.abs(src).max()
    moved = np.abs(a["img"] - src).max()
    print(f"{H}x{W} band {band}: max |fft - partial| {err:.2e}, max |src| {top:.4g}, moved by up to {moved:.4g}, mse {a['mse']}")
    assert err <= 1e-10 * top
    assert moved > 0.05 * top  # the transform does something
    np.testing.assert_allclose(b["mse"], a["mse"], rtol=1e-10, atol=0)  # Parseval against the pixels' own mean square
    # source image i takes target image i mod Bt: image 2 pairs with target 0, and differs from what target 1 would give
    alone = R.transfer(src[2:3], trg[0:1], band, norm)["img"]
    assert np.array_equal(alone, a["img"][2:3])
    assert not np.array_equal(R.transfer(src[2:3], trg[1:2], band, norm)["img"], a["img"][2:3])


def test_band_zero_swaps_the_mean_alone_and_equal_images_stay():
    src, trg = R.inputs(1, 1, 2, 10, 13, seed=3, zero_channel=0)
    out = R.transfer(src, trg, 0)["img"]
    for c in (0, 1):  # |mean| of the target with the sign of the source's (a zero mean has angle 0)
        np.testing.assert_allclose(out[0, c] - src[0, c], trg[0, c].astype(np.float64).mean() - src[0, c].astype(np.float64).mean(),
                                   rtol=0, atol=1e-11)
    same = R.transfer(src[:, 1:], src[:, 1:], 3)
    assert np.abs(same["img"] - src[:, 1:]).max() <= 1e-10 * 255 and same["mse"].max() <= 1e-20


def test_band_of_the_loaders_sizes():
    from mm2d3d_amd.fda import band_of

    assert band_of(225, 400, 0.01) == 2 and band_of(225, 400, 0.09) == 20 and band_of(225, 400, 0.05) == 11
    assert band_of(302, 480, 0.01) == 3 and band_of(302, 480, 0.09) == 27
    assert band_of(48, 64, 0.09) == 4 and band_of(48, 64, 0.0) == 0 and band_of(48, 64, 0.02) == 0
    for H, W, beta in ((225, 400, 0.01), (302, 480, 0.09), (9, 14, 0.2)):
        assert band_of(H, W, beta) == R.band_of(H, W, beta)


# ---------------------------------------------------------------------------------------------- the constructor
def test_constructor_defaults_and_values():
    tm = _trainer()
    assert tm.fda_beta is None and tm.fda_image_norm is None and tm.last_fda is None and not tm.input_style.active
    batch = {"img": object()}
    assert tm.input_style.style(batch, None) is batch  # off: nothing is consulted
    tm = _trainer(fda_beta=0.09, fda_image_norm=NORM)
    assert tm.fda_beta == 0.09 and tm.input_style.active
    assert tm.fda_image_norm == (tuple(NORM[0]), tuple(NORM[1]))
    tm.fda_beta = 0.01  # forwarded to the policy object, as the other options are
    assert tm.input_style.fda_beta == 0.01
    assert _trainer(fda_beta=0).fda_beta == 0.0 and _trainer(fda_beta=0).input_style.active  # a band of 0 is an option, not "off"
    # independent of the output-level options: they compose
    tm = _trainer(fda_beta=0.05, lambda_coral=0.1, lambda_minent=0.2, lambda_pl=1.0, pseudo_label_source="teacher", ema_decay=0.9)
    assert tm.fda_beta == 0.05 and tm.lambda_coral == 0.1 and tm.lambda_minent == 0.2 and tm.lambda_pl == 1.0
    plain, on = _trainer(), _trainer(fda_beta=0.09)
    assert set(vars(plain)) == set(vars(on)) and set(vars(plain.input_style)) == set(vars(on.input_style))


def test_constructor_refuses_every_bad_option_by_name():
    for bad in (-0.01, 0.5, 1.0, float("nan"), float("inf"), "0.09", True, [0.09]):
        with pytest.raises(ValueError, match="fda_beta"):
            _trainer(fda_beta=bad)
    for bad in (0.5, ([1.0], [1.0, 2.0]), ([1.0], [0.0]), ([1.0], [-1.0]), ([float("nan")], [1.0]), ([1.0], [float("inf")]), ([], []),
                (["1"], [1.0]), ([1.0],), "ab", ([True], [1.0])):
        for kw in (dict(), dict(fda_beta=0.09)):  # whatever the switch is: an option that cannot run is not hidden
            with pytest.raises(ValueError, match="fda_image_norm"):
                _trainer(fda_image_norm=bad, **kw)


# ---------------------------------------------------------------------------------------------- fda_transfer
def test_fda_transfer_refusals_name_the_argument():
    from mm2d3d_amd.fda import fda_transfer

    m = lambda *shape, **kw: torch.zeros(*shape, device="meta", **kw)  # refused on their values before the device is looked at
    ok = m(2, 3, 48, 64)
    with pytest.raises(ValueError, match="src must live on the GPU"):
        fda_transfer(torch.zeros(2, 3, 48, 64), torch.zeros(2, 3, 48, 64), 0.09)
    for bad in (m(3, 48, 64), [[0.0]], None, m(2, 3, 48, 64, dtype=torch.float16), m(2, 3, 48, 64, dtype=torch.float64),
                m(2, 3, 64, 48).transpose(2, 3), m(2, 3, 48, 128)[..., ::2], m(0, 3, 48, 64)):
        with pytest.raises(ValueError, match="src"):
            fda_transfer(bad, ok, 0.09)
        with pytest.raises(ValueError, match="trg"):
            fda_transfer(ok, bad, 0.09)
    for other in (m(2, 3, 48, 66), m(2, 3, 50, 64), m(2, 1, 48, 64)):  # one C, H, W; the batch sizes are free
        with pytest.raises(ValueError, match="must agree in C, H and W"):
            fda_transfer(ok, other, 0.09)
    with pytest.raises(ValueError, match="channels"):
        fda_transfer(m(2, 5, 48, 64), m(1, 5, 48, 64), 0.09)
    with pytest.raises(ValueError, match="on a side"):
        fda_transfer(m(1, 1, 8, 2049), m(1, 1, 8, 2049), 0.09)
    for bad in (-0.1, 0.5, float("nan"), "0.09", None, True):
        with pytest.raises(ValueError, match="beta"):
            fda_transfer(ok, ok, bad)
    with pytest.raises(ValueError, match="band of 33"):  # 480 * 0.07: beyond the kernels' 32
        fda_transfer(m(1, 3, 480, 640), m(1, 3, 480, 640), 0.07)
    for bad in (([0.0] * 2, [1.0] * 2), ([0.0] * 3, [1.0, 0.0, 1.0]), 1.0):
        with pytest.raises(ValueError, match="image_norm"):
            fda_transfer(ok, ok, 0.09, bad)
    with pytest.raises(ValueError, match="GPU"):  # everything else in order: only the device is left to refuse
        fda_transfer(ok, m(5, 3, 48, 64), 0.09, NORM)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_the_bindings_match():
    import os
    import re

    from mm2d3d_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp, "int": _lib.i32, "size_t": _lib.sz}
    for name, ret, rtype, n in (("mm_fda_transfer", "int", _lib.i32, 15), ("mm_fda_ws_bytes", "size_t", _lib.sz, 6)):
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is rtype and len(args) == len(params) == n, name
        assert args == [ctype[p] for p in params], (name, params)
    assert "2048" in txt[txt.index("Fourier domain adaptation"):txt.index("mm_fda_ws_bytes(")]  # the limit of H and W is stated


def test_argument_errors_come_before_any_launch():
    from mm2d3d_amd import _lib

    L = _lib.lib()
    keep = (ctypes.c_double * 256)()  # never read or written: every call below is refused before a device call
    p = ctypes.addressof(keep)
    need = int(L.mm_fda_ws_bytes(2, 1, 3, 48, 64, 4))
    # fp64 complex: the 9 x 5 in-band terms of the 3 images' channels per tile of 32 rows, those of the 2 source images' channels
    # after the swap, and their shares of mse
    assert need >= 3 * 3 * 2 * (9 * 5) * 16 + 2 * 3 * (9 * 5) * 16 + 2 * 3 * 8
    assert int(L.mm_fda_ws_bytes(8, 8, 3, 302, 480, 27)) >= 16 * 3 * 10 * (55 * 28) * 16 + 8 * 3 * (55 * 28) * 16 + 8 * 3 * 8
    assert int(L.mm_fda_ws_bytes(1, 1, 4, 2048, 2048, 32)) > 0  # the stated limits are inside
    bad_sizes = [dict(Bs=0), dict(Bs=-1), dict(Bt=0), dict(H=0), dict(W=0), dict(W=-3), dict(C=0), dict(C=5), dict(C=-1), dict(band=-1),
                 dict(band=33, H=2048, W=2048), dict(band=24), dict(band=32, W=2048), dict(H=9, W=14, band=5), dict(H=2049), dict(W=2049),
                 dict(H=1 << 20, W=1 << 20), dict(Bs=(1 << 20) + 1), dict(Bt=1 << 30)]
    for kw in bad_sizes:
        a = dict(dict(Bs=2, Bt=1, C=3, H=48, W=64, band=4), **kw)
        assert int(L.mm_fda_ws_bytes(a["Bs"], a["Bt"], a["C"], a["H"], a["W"], a["band"])) == 0, kw

    def call(src=p, Bs=2, trg=p, Bt=1, C=3, H=48, W=64, band=4, mean=None, std=None, out=p, mse=p, ws=p, ws_bytes=need):
        return L.mm_fda_transfer(src, Bs, trg, Bt, C, H, W, band, mean, std, out, mse, ws, ws_bytes, None)

    for kw in bad_sizes + [dict(src=None), dict(trg=None), dict(out=None), dict(mse=None), dict(mean=p), dict(std=p), dict(ws=None),
                           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(Bs=3), dict(band=5), dict(H=65)]:  # the last three: a short workspace
        assert call(**kw) == -1, kw
        assert b"fda_transfer:" in L.mm_last_error(), (kw, L.mm_last_error())
    assert call(mean=p, std=None) == -1 and b"both null or both set" in L.mm_last_error()
    assert call(band=24) == -1 and b"min(H, W)" in L.mm_last_error()
    assert call(H=2049) == -1 and b"2048" in L.mm_last_error()
