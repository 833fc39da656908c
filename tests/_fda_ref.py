"""Float64 numpy reference of Fourier domain adaptation (FDA, Yang & Soatto, CVPR 2020) for tests/test_fda_host.py and
tests/test_gpu_fda.py (no tests here).

``transfer`` is the FFT formulation: fft2, fftshift, the amplitudes of the window [c - b, c + b] around c = floor(n / 2) on both axes
taken from the target, ifftshift, ifft2, the real part; ``image_norm`` by de-normalising, transforming and re-normalising.
``transfer_partial`` evaluates the band-limited formula the kernels implement (include/mm2d3d.h) with dense DFT matrices of the
band alone, and treats ``image_norm`` in the DC term alone: it shares nothing with the first but numpy's arithmetic."""
import math

import numpy as np


def band_of(H, W, beta):
    return int(math.floor(min(H, W) * beta))


def _norm(image_norm, C):
    if image_norm is None:
        return np.zeros(C), np.ones(C)
    mean, std = (np.asarray(v, dtype=np.float64) for v in image_norm)
    assert mean.shape == std.shape == (C,)
    return mean, std


def _window(n, b):
    c = n // 2
    assert 0 <= c - b and c + b < n
    return slice(c - b, c + b + 1)


def spectrum_window(img, band):
    """The shifted in-band spectrum [2 b + 1, 2 b + 1] of one float64 image [H, W]."""
    H, W = img.shape
    return np.fft.fftshift(np.fft.fft2(img))[_window(H, band), _window(W, band)]


def _swap_fft(s, t, band):
    H, W = s.shape
    fs, ft = np.fft.fftshift(np.fft.fft2(s)), np.fft.fftshift(np.fft.fft2(t))
    amp, pha = np.abs(fs), np.angle(fs)
    wy, wx = _window(H, band), _window(W, band)
    amp[wy, wx] = np.abs(ft)[wy, wx]
    return np.fft.ifft2(np.fft.ifftshift(amp * np.exp(1j * pha))).real


def transfer(src, trg, band, image_norm=None):
    """``dict(img [Bs, C, H, W], mse [Bs])`` in float64: source image i with the in-band amplitudes of target image i mod Bt."""
    src, trg = np.asarray(src, dtype=np.float64), np.asarray(trg, dtype=np.float64)
    Bs, C, H, W = src.shape
    Bt = trg.shape[0]
    assert trg.shape[1:] == (C, H, W)
    mean, std = _norm(image_norm, C)
    out = np.empty_like(src)
    for i in range(Bs):
        for c in range(C):
            s, t = src[i, c] * std[c] + mean[c], trg[i % Bt, c] * std[c] + mean[c]
            out[i, c] = (_swap_fft(s, t, band) - mean[c]) / std[c]
    return dict(img=out, mse=((out - src) ** 2).mean(axis=(1, 2, 3)))


def _dft_matrix(n, b):
    """E[k + b, r] = e^{-2 pi i k r / n}, k in [-b, b], with the phase reduced in integers first."""
    k, r = np.arange(-b, b + 1)[:, None], np.arange(n)[None, :]
    return np.exp(-2j * np.pi * ((k * r) % n) / n)


def transfer_partial(src, trg, band, image_norm=None):
    """The same result from out = src + 1 / (H W) * Re sum_k dF[k] e^{+...} over the band alone; ``mse`` by Parseval."""
    src, trg = np.asarray(src, dtype=np.float64), np.asarray(trg, dtype=np.float64)
    Bs, C, H, W = src.shape
    Bt = trg.shape[0]
    mean, std = _norm(image_norm, C)
    Ey, Ex = _dft_matrix(H, band), _dft_matrix(W, band)
    out, mse = np.empty_like(src), np.zeros(Bs)
    for i in range(Bs):
        for c in range(C):
            fs, ft = Ey @ src[i, c] @ Ex.T, Ey @ trg[i % Bt, c] @ Ex.T
            scale = np.ones_like(fs, dtype=np.float64)
            if image_norm is not None:  # only the DC term differs between (pixel - mean) / std and pixel / std
                fs[band, band] = std[c] * fs[band, band] + mean[c] * H * W
                ft[band, band] = std[c] * ft[band, band] + mean[c] * H * W
                scale[band, band] = std[c]
            a_s, a_t = np.abs(fs), np.abs(ft)
            zero = fs == 0
            d = np.where(zero, a_t, fs * (a_t / np.where(zero, 1.0, a_s) - 1.0)) / scale
            out[i, c] = src[i, c] + (Ey.conj().T @ d @ Ex.conj()).real / (H * W)
            mse[i] += (np.abs(d) ** 2).sum() / (float(H) * W) ** 2 / C
    return dict(img=out, mse=mse)


def inputs(Bs, Bt, C, H, W, seed, zero_channel=0):
    """Seeded fp32 images: source pixels uniform in 0..255, target pixels darker and of another distribution (a squared uniform
    draw scaled to 0..120 plus a ramp along x), so that the transform moves pixels by tens of grey levels; channel
    ``zero_channel`` of source image 0 is exact zeros."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.0, 255.0, (Bs, C, H, W)).astype(np.float32)
    trg = (120.0 * rng.uniform(0.0, 1.0, (Bt, C, H, W)) ** 2 + 30.0 * np.linspace(0.0, 1.0, W)).astype(np.float32)
    src[0, zero_channel] = 0.0
    return src, trg


# The image_normalizer of the tests.  The mean of channel 1, the channel the tests zero, is 0: its pixels are then exact zeros
# too.  With any other mean the de-normalised channel is a non-zero CONSTANT image, whose non-DC terms an FFT of a length that is
# no power of two (37) returns as rounding noise of some 1e-11 instead of 0 - the FFT formulation then takes that noise's phase, and
# there is nothing to compare with (assert_phases_defined refuses such inputs).
NORM = ([123.675, 0.0, 103.53], [58.395, 57.12, 57.375])
ZERO_CHANNEL = 1


def normalised(pix, image_norm):
    """(pix - mean) / std in fp32, per channel of [B, C, H, W]."""
    m, s = (np.asarray(v, dtype=np.float32)[None, :, None, None] for v in image_norm)
    return ((pix - m) / s).astype(np.float32)


def assert_phases_defined(src, band, image_norm=None):
    """The condition under which a comparison means anything: every in-band |F_src[k]| is exactly 0 or at least
    1e-6 * H W * max |src| - below that the source's phase is rounding noise in the FFT formulation too."""
    src = np.asarray(src, dtype=np.float64)
    Bs, C, H, W = src.shape
    mean, std = _norm(image_norm, C)
    pix = src * std[None, :, None, None] + mean[None, :, None, None]
    floor = 1e-6 * H * W * np.abs(pix).max()
    n_zero = 0
    for i in range(Bs):
        for c in range(C):
            a = np.abs(spectrum_window(pix[i, c], band))
            assert ((a == 0) | (a >= floor)).all(), (i, c, a[(a != 0) & (a < floor)])
            n_zero += int((a == 0).sum())
    return n_zero
