"""Fourier domain adaptation on the GPU (csrc/fda.hip: k_fda_rows, k_fda_finish, k_fda_apply behind mm_fda_transfer; fda.fda_transfer)
against the float64 FFT reference tests/_fda_ref.py evaluated on the same fp32 images.

Source pixels are uniform in 0..255, target pixels of another distribution, so that the transform moves pixels by tens of grey
levels; one channel of source image 0 is exact zeros (the angle(0) = 0 branch).  Every output pixel is within
2^-23 * |ref| + 1e-9 * max(|src|, |trg|) of the reference: one fp32 unit for the final rounding, and an absolute term three orders above
the float64 rounding of the two formulations against each other (tests/test_fda_host.py) and four below what an fp32 sum or an
fp32 twiddle factor would show.  mse is within 2^-22 relative.  A second call gives the same bits; src and trg are not written.

Shapes: the smallest at which the kernels can go wrong - odd H, odd W, powers of two, a band of 0, a band wider than half the
height - and, beyond those, every size at which a kernel takes another path: more than one 128-column chunk and more than one
256-column stride with a tail (40x300), more than one row tile of the row pass with a short last one (40 > 32 rows; 66 = 28 + 28 + 10),
more (ky, kx) pairs than the finishing workgroup has threads and 7 instead of 8 row groups per workgroup in the row pass (66x65
at the widest band, 32)."""
import functools

import numpy as np
import pytest
import torch

import _fda_ref as R

pytestmark = pytest.mark.gpu

# (H, W, Bs, Bt, C, band, image_norm)
CASES = {
    "9x14_b1_pairs": (9, 14, 3, 2, 3, 1, None),  # odd H; source image 2 takes target image 0
    "10x13_b2_c1": (10, 13, 2, 3, 1, 2, None),  # odd W, one channel, more target images than source images
    "16x16_b0": (16, 16, 2, 1, 3, 0, None),  # the DC term alone
    "16x16_b3": (16, 16, 2, 1, 3, 3, None),  # powers of two
    "37x64_b3_norm": (37, 64, 2, 2, 3, 3, R.NORM),  # normalised tensors: the DC term in pixel units
    "48x64_b20": (48, 64, 2, 2, 3, 20, None),  # 2 b + 1 = 41 of 48 rows
    "40x300_b4": (40, 300, 1, 1, 2, 4, None),  # column chunks, column strides, two row tiles
    "66x65_b32_c4": (66, 65, 1, 1, 4, 32, None),  # the widest band, 2145 (ky, kx) pairs, four channels
}


def _zero_channel(C):
    return min(R.ZERO_CHANNEL, C - 1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded inputs and their float64 reference: computed once, never modified."""
    H, W, Bs, Bt, C, band, norm = CASES[name]
    src, trg = R.inputs(Bs, Bt, C, H, W, seed=7000 + sorted(CASES).index(name), zero_channel=_zero_channel(C))
    if norm is not None:
        src, trg = R.normalised(src, norm), R.normalised(trg, norm)
    n_zero = R.assert_phases_defined(src, band, norm)  # every in-band source amplitude is exactly 0 or far above rounding
    assert n_zero >= (2 * band + 1) ** 2 - (0 if norm is None else 1) and not src[0, _zero_channel(C)].any()
    beta = (band + 0.25) / min(H, W)
    assert 0.0 <= beta < 0.5 and R.band_of(H, W, beta) == band
    return dict(src=src, trg=trg, band=band, beta=beta, norm=norm, ref=R.transfer(src, trg, band, norm))


def _run(c, src=None):
    from mm2d3d_amd.fda import fda_transfer

    dev = torch.device("cuda:0")
    s, t = torch.from_numpy(c["src"] if src is None else src).to(dev), torch.from_numpy(c["trg"]).to(dev)
    out = fda_transfer(s, t, c["beta"], c["norm"])
    torch.cuda.synchronize()
    return s, t, out


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_float64_reference(name):
    c = _case(name)
    s, t, out = _run(c)
    assert out["band"] == c["band"] and out["img"].dtype == torch.float32 and out["img"].shape == s.shape and out["img"].is_contiguous()
    assert out["img"].data_ptr() != s.data_ptr() and not out["img"].requires_grad
    assert out["mse"].dtype == torch.float32 and out["mse"].shape == (s.shape[0],) and out["mse"].is_cuda
    got, ref = out["img"].cpu().numpy().astype(np.float64), c["ref"]["img"]
    top = max(np.abs(c["src"]).max(), np.abs(c["trg"]).max())
    bound = 2.0 ** -23 * np.abs(ref) + 1e-9 * top
    err = np.abs(got - ref)
    moved = np.abs(ref - c["src"]).max()
    print(f"{name}: max |out - ref| / bound {np.max(err / bound):.3f}, max |out - ref| {err.max():.3e}, moved by up to {moved:.4g} of {top:.4g}")
    assert moved > 0.05 * top
    assert (err <= bound).all(), (np.max(err / bound), np.unravel_index(np.argmax(err / bound), err.shape))
    mse, mref = out["mse"].cpu().numpy().astype(np.float64), c["ref"]["mse"]
    print(f"{name}: mse {mse}, reference {mref}, max relative difference {np.max(np.abs(mse - mref) / mref):.3e}")
    assert (mref > 0).all() and (np.abs(mse - mref) <= 2.0 ** -22 * mref).all()
    # src and trg are read only
    assert np.array_equal(s.cpu().numpy().view(np.int32), c["src"].view(np.int32))
    assert np.array_equal(t.cpu().numpy().view(np.int32), c["trg"].view(np.int32))
    # a second call: the same bits
    _, _, again = _run(c)
    assert torch.equal(again["img"].view(torch.int32), out["img"].view(torch.int32))
    assert torch.equal(again["mse"].view(torch.int32), out["mse"].view(torch.int32))


def test_a_non_finite_pixel_spoils_its_own_image_channel_alone():
    c = _case("9x14_b1_pairs")
    _, _, clean = _run(c)
    src = c["src"].copy()
    src[1, 2, 4, 5] = np.nan
    _, _, out = _run(c, src)
    img, ok = out["img"].cpu().numpy(), clean["img"].cpu().numpy()
    assert np.isnan(img[1, 2]).all()  # as in the FFT formulation: every in-band term of that channel is NaN
    keep = np.ones(img.shape[:2], dtype=bool)
    keep[1, 2] = False
    assert np.array_equal(img[keep].view(np.int32), ok[keep].view(np.int32))
    mse, mok = out["mse"].cpu().numpy(), clean["mse"].cpu().numpy()
    assert np.isnan(mse[1]) and np.array_equal(mse[[0, 2]].view(np.int32), mok[[0, 2]].view(np.int32))
