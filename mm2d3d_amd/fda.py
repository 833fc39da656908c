"""Fourier domain adaptation of the source camera images (FDA, Yang & Soatto, CVPR 2020; the 2D input-level baseline of the journal
version of xMUDA): ``fda_transfer`` over the HIP kernels of csrc/fda.hip, and everything ``train_kwargs["fda_beta"]`` and
``["fda_image_norm"]`` switch on in the two-domain step (train.py), in one policy object."""
import math

import torch

from . import _lib
from ._lib import check, ptr, stream
from .stepopts import StepOption, number

MAX_BAND, MAX_CHANNELS, MAX_SIDE = 32, 4, 2048  # csrc/fda.hip

_NORM = {}  # (device index, mean, std) -> fp32 [2, C] on the device: written once, so that a step copies nothing from the host


def _image_norm(image_norm, name):
    """``(mean, std)`` as two tuples of floats of one length, or None."""
    if image_norm is None:
        return None
    try:
        mean, std = image_norm
        mean, std = tuple(mean), tuple(std)
        ok = len(mean) == len(std) >= 1 and not any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in mean + std)
        ok = ok and all(math.isfinite(v) for v in mean) and all(0.0 < v < math.inf for v in std)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be None or (mean, std): two sequences of one length, finite, with std > 0; not {image_norm!r}")
    return tuple(map(float, mean)), tuple(map(float, std))


def band_of(H, W, beta):
    """floor(min(H, W) * beta): the band of the original implementation."""
    return int(math.floor(min(int(H), int(W)) * float(beta)))


def fda_transfer(src, trg, beta, image_norm=None):
    """Source images in the target's style: per channel, the amplitudes of the (2 band + 1)^2 lowest frequencies of ``src[i]`` are
    replaced by those of ``trg[i % Bt]``, the phases stay; ``band = floor(min(H, W) * beta)``; include/mm2d3d.h has the definition.
    ``src`` [Bs, C, H, W] and ``trg`` [Bt, C, H, W]: fp32, contiguous, on the GPU, of one C, H, W.  ``beta``: a number in [0, 0.5)
    (0.01 to 0.09 are usual; a band of 0 swaps the mean brightness alone).  ``image_norm = (mean, std)``: the tensors hold
    ``(pixel - mean) / std`` and the swap is that of the pixels, where FDA is defined.  Returns ``dict(img, band, mse)``: ``img`` a
    new fp32 tensor like ``src``, which is never written; ``band`` an int; ``mse`` fp32 [Bs] on the device, the mean of
    ``(img - src) ** 2`` per source image.  No learnable part and no backward pass: ``img`` carries no graph.  Three launches, no host
    read, bit-stable run to run."""
    who = "fda_transfer"
    for name, t in (("src", src), ("trg", trg)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{who}: {name} must be a tensor [B, C, H, W]")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be float32, not {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
        if t.shape[0] < 1:
            raise ValueError(f"{who}: {name} holds no image")
    Bs, C, H, W = (int(v) for v in src.shape)
    Bt = int(trg.shape[0])
    if tuple(trg.shape[1:]) != (C, H, W):
        raise ValueError(f"{who}: src images are {tuple(src.shape[1:])}, trg images {tuple(trg.shape[1:])}: they must agree in C, H and W")
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{who}: src has {C} channels, the kernels take 1 to {MAX_CHANNELS}")
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{who}: src images of {H} x {W}, the kernels take 1 to {MAX_SIDE} on a side")
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 <= float(beta) < 0.5:
        raise ValueError(f"{who}: beta must be a number in [0, 0.5), not {beta!r}")
    band = band_of(H, W, beta)
    if band > MAX_BAND or 2 * band + 1 > min(H, W):
        raise ValueError(f"{who}: beta {beta!r} gives a band of {band} at {H} x {W}, the kernels take 0 to {MAX_BAND}")
    norm = _image_norm(image_norm, f"{who}: image_norm")
    if norm is not None and len(norm[0]) != C:
        raise ValueError(f"{who}: image_norm has {len(norm[0])} entries, src has C = {C} channels")
    for name, t in (("src", src), ("trg", trg)):
        if not t.is_cuda:
            raise ValueError(f"{who}: {name} must live on the GPU (HIP path only, no CPU fallback)")
    if trg.device != src.device:
        raise ValueError(f"{who}: trg is on {trg.device}, src on {src.device}")
    L = _lib.lib()
    dev = src.device
    ms = None
    if norm is not None:
        key = (dev.index, norm)
        ms = _NORM.get(key)
        if ms is None:
            ms = _NORM[key] = torch.tensor(norm, dtype=torch.float32, device=dev)
    src, trg = src.detach(), trg.detach()
    out = torch.empty_like(src)
    mse = torch.empty(Bs, dtype=torch.float32, device=dev)
    ws = _lib.workspace.get(int(L.mm_fda_ws_bytes(Bs, Bt, C, H, W, band)), dev)
    check(L.mm_fda_transfer(ptr(src), Bs, ptr(trg), Bt, C, H, W, band, ptr(ms[0]) if ms is not None else None,
                            ptr(ms[1]) if ms is not None else None, ptr(out), ptr(mse), ptr(ws), ws.numel(), stream()), "fda_transfer")
    return dict(img=out, band=band, mse=mse)


class InputStyle(StepOption):
    """With ``fda_beta`` set, every TRAIN step styles its source camera images after its target images before the 2D network sees
    them: ``img = fda_transfer(source img, target img, fda_beta, fda_image_norm)["img"]``, in the joined pass and in the two-call
    path alike - source geometry and labels in the target's exposure, colour cast and tone.  ``fda_image_norm``: the loaders'
    ``image_normalizer`` ``(mean, std)`` when the batches hold normalised images, None when they hold pixels.  The caller's batch dicts
    and tensors are not modified (the step works on a shallow copy of the source dict); ``depth``, ``img_indices``, the 3D
    branch's features and the target batch are untouched; the teacher pass, validation, test and ``predict_step`` never style
    anything.  Source and target images of different sizes raise at the step.  ``last_fda``: ``{"img", "band", "mse"}`` of the last
    step (device tensors; ``band`` an int); the mean of ``mse`` is logged as ``{stage}/fda_mse``.  Under data parallelism each rank
    styles its own batch.  Composes with every output-level option.  ``fda_beta`` None (default): nothing is called or
    allocated, no log key appears, the step is launch for launch the step without the option."""

    FORWARDED = ("fda_beta", "fda_image_norm", "last_fda")

    def __init__(self, train_kwargs):
        self.fda_beta = number(train_kwargs, "fda_beta", None, lambda v: 0.0 <= v < 0.5, "a number in [0, 0.5)")
        self.fda_image_norm = _image_norm(train_kwargs.get("fda_image_norm"), "train_kwargs['fda_image_norm']")
        self.last_fda = None

    @property
    def active(self):
        return self.fda_beta is not None

    def style(self, src, trg):
        """The source batch dict the step goes on with: ``src`` itself when the option is off, else a shallow copy whose ``img`` is
        styled after ``trg["img"]``."""
        if not self.active:
            return src
        self.last_fda = fda_transfer(src["img"], trg["img"], self.fda_beta, self.fda_image_norm)
        return dict(src, img=self.last_fda["img"])

    def log(self, logs, stage):
        if self.active:
            logs[f"{stage}/fda_mse"] = self.last_fda["mse"].mean()
