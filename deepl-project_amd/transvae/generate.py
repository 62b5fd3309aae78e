"""The three modes of the reference's sampling script, P/generate_images.py:75-168, on the HIP path.

`random_samples` and `interpolate_latents` draw their latents exactly as the script does (`torch.manual_seed(seed)`, then
`torch.randn` on the model's device in the script's order), decode them through `model.decoder` and apply the script's sigmoid.
The interpolation's frames are decoded as ONE batch instead of one decoder call per frame.  `reconstruct` takes the already
prepared `[B, 3, H, W]` batch (transvae.image_io.ImagePrep stands in for the script's PIL transform) and returns the script's
`(comparison, original, reconstruction)`.  A DDP-style wrapper is unwrapped through `.module`, as in the script.  Everything
runs in eval mode under no_grad; write the results with transvae.image_io.save_image.
"""
from __future__ import annotations

from typing import Optional

import torch


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def _latent_dim(model, latent_dim: Optional[int]) -> int:
    if latent_dim is not None:
        return int(latent_dim)
    d = getattr(_unwrap(model), "latent_dim", None)
    if d is None:
        raise ValueError("generate: the model has no latent_dim attribute; pass latent_dim")
    return int(d)


def _device(model) -> torch.device:
    return next(_unwrap(model).parameters()).device


@torch.no_grad()
def random_samples(model, num_samples: int, latent_dim: Optional[int] = None, spatial_size: int = 16, seed: Optional[int] = None,
                   sigmoid: bool = True) -> torch.Tensor:
    """P/generate_images.py:75-108: z ~ N(0, 1) of [num_samples, latent_dim, spatial_size, spatial_size] drawn on the device,
    decoded, sigmoid -> [num_samples, 3, H, W] in [0, 1].  sigmoid=False returns the decoder's raw output."""
    m = _unwrap(model)
    m.eval()
    if seed is not None:
        torch.manual_seed(seed)
    z = torch.randn(int(num_samples), _latent_dim(model, latent_dim), spatial_size, spatial_size, device=_device(model))
    samples = m.decoder(z)
    return torch.sigmoid(samples) if sigmoid else samples


@torch.no_grad()
def interpolate_latents(model, num_steps: int, latent_dim: Optional[int] = None, spatial_size: int = 16, seed: Optional[int] = None,
                        sigmoid: bool = True, return_latents: bool = False):
    """P/generate_images.py:111-143: z1 then z2 drawn on the device, alphas = linspace(0, 1, num_steps), frame i decodes
    (1 - a_i) z1 + a_i z2.  The latents are the script's bit for bit; the frames come from one decoder call on the batch of
    latents.  return_latents=True returns (frames, latents)."""
    m = _unwrap(model)
    m.eval()
    if seed is not None:
        torch.manual_seed(seed)
    dev = _device(model)
    d = _latent_dim(model, latent_dim)
    z1 = torch.randn(1, d, spatial_size, spatial_size, device=dev)
    z2 = torch.randn(1, d, spatial_size, spatial_size, device=dev)
    alphas = torch.linspace(0, 1, int(num_steps), device=dev).view(-1, 1, 1, 1)
    latents = (1 - alphas) * z1 + alphas * z2
    frames = m.decoder(latents)
    if sigmoid:
        frames = torch.sigmoid(frames)
    return (frames, latents) if return_latents else frames


@torch.no_grad()
def reconstruct(model, images: torch.Tensor, sigmoid: bool = True):
    """P/generate_images.py:146-168 for a prepared batch: (comparison, original, reconstruction), the comparison being the
    original and the reconstruction side by side along W."""
    _unwrap(model).eval()
    reconstruction = model(images)[0]
    if sigmoid:
        reconstruction = torch.sigmoid(reconstruction)
    return torch.cat([images, reconstruction], dim=3), images, reconstruction
