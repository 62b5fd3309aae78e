"""Reconstruction metrics on the device: per-image MSE, PSNR and SSIM in two HIP launches (csrc/metrics.hip).

The reference measures a trained model on the host, one image at a time: R/evaluate.py:69-144 copies both tensors to the
CPU, clips them to [0, 1] and calls skimage's `peak_signal_noise_ratio(data_range=1)` and
`structural_similarity(data_range=1, channel_axis=2)`; P/evaluate_transvae.py:47-77,110-178 applies a sigmoid to the
reconstruction and uses an 11x11 box SSIM built from `F.avg_pool2d(padding=5)`.  Both definitions are here:

    ssim_window="skimage"  7x7 uniform window, scipy 'reflect' border, sample covariance (x 49/48), map cropped by 3 px,
                           mean per channel then over channels (skimage's defaults; H, W >= 7)
    ssim_window="box11"    11x11 uniform window, zero border divided by 121, population covariance, mean over the map
    transform="clip"       clamp both inputs to [0, 1] first (R/evaluate.py:109-110)
    transform="sigmoid"    sigmoid on `recon` only (P/evaluate_transvae.py:131)
    transform="none"

PSNR = 10 log10(data_range^2 / mse), +inf when mse == 0 (as in both references).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from .hip import _lib as L
from .hip import ops

_WINDOWS = {"skimage": L.SSIM_SKIMAGE, "box11": L.SSIM_BOX11}
_TRANSFORMS = {"none": L.METRIC_NONE, "clip": L.METRIC_CLIP, "sigmoid": L.METRIC_SIGMOID}


def _check_args(recon: torch.Tensor, target: torch.Tensor, ssim_window: str, transform: str, data_range: float):
    if ssim_window not in _WINDOWS:
        raise ValueError(f"reconstruction_metrics: unknown ssim_window {ssim_window!r} (expected one of {sorted(_WINDOWS)})")
    if transform not in _TRANSFORMS:
        raise ValueError(f"reconstruction_metrics: unknown transform {transform!r} (expected one of {sorted(_TRANSFORMS)})")
    if recon.dim() != 4 or recon.shape != target.shape:
        raise ValueError(f"reconstruction_metrics: recon and target must both be [B, C, H, W] of one shape, got "
                         f"{tuple(recon.shape)} and {tuple(target.shape)}")
    if recon.numel() == 0:
        raise ValueError("reconstruction_metrics: empty batch")
    H, W = recon.shape[-2:]
    if ssim_window == "skimage" and (H < 7 or W < 7):
        raise ValueError(f"reconstruction_metrics: the skimage SSIM window is 7x7 and needs H, W >= 7 (got {H}x{W}); "
                         "skimage raises here as well")
    if not data_range > 0:
        raise ValueError(f"reconstruction_metrics: data_range must be positive, got {data_range}")


def reconstruction_metrics(recon: torch.Tensor, target: torch.Tensor, *, ssim_window: str = "skimage", transform: str = "clip",
                           data_range: float = 1.0) -> Dict[str, torch.Tensor]:
    """Per-image metrics of a batch of image pairs [B, C, H, W] -> {"mse", "psnr", "ssim"}, each a [B] fp32 device tensor.

    Any element strides are read in place (NCHW-contiguous and channels_last need no copy).  Inputs that are not fp32 are
    cast to fp32 first, which makes a copy.  Runs on the inputs' device with autocast off; CPU tensors raise.
    """
    _check_args(recon, target, ssim_window, transform, data_range)
    ops._need_gpu(recon, target)
    if recon.device != target.device:
        raise RuntimeError(f"reconstruction_metrics: recon on {recon.device}, target on {target.device}")
    with torch.cuda.device(recon.device), torch.autocast("cuda", enabled=False), torch.no_grad():
        x = recon.detach().float()
        y = target.detach().float()
        B, Cn, H, W = x.shape
        kind = _WINDOWS[ssim_window]
        lib = L.load()
        n_part = lib.tv_recon_metrics_partial_count(B, Cn, H, W, kind)
        if n_part <= 0:
            raise RuntimeError(f"reconstruction_metrics: unsupported shape {tuple(x.shape)}")
        partials = torch.empty(n_part, device=x.device, dtype=torch.float32)
        out = torch.empty(3, B, device=x.device, dtype=torch.float32)
        L.check(lib.tv_recon_metrics(ops._p(x), ops._p(y), *x.stride(), *y.stride(), B, Cn, H, W, kind, _TRANSFORMS[transform],
                                     C.c_float(data_range), ops._p(partials), ops._p(out), ops._stream()), "tv_recon_metrics")
    return {"mse": out[0], "psnr": out[1], "ssim": out[2]}


def psnr(recon: torch.Tensor, target: torch.Tensor, *, transform: str = "clip", data_range: float = 1.0) -> torch.Tensor:
    """Per-image PSNR [B] (dB, fp32, +inf for identical images); see :func:`reconstruction_metrics`."""
    # the SSIM half of the pass needs H, W >= 7 only for the skimage window; box11 takes any size
    return reconstruction_metrics(recon, target, ssim_window="box11", transform=transform, data_range=data_range)["psnr"]


def ssim(recon: torch.Tensor, target: torch.Tensor, *, ssim_window: str = "skimage", transform: str = "clip",
         data_range: float = 1.0) -> torch.Tensor:
    """Per-image SSIM [B] (fp32); see :func:`reconstruction_metrics`."""
    return reconstruction_metrics(recon, target, ssim_window=ssim_window, transform=transform, data_range=data_range)["ssim"]
