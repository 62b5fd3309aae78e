"""Closed-form terms of the reference loss on the path's outputs, one HIP pass for value and gradient.

Interface mirror of R/transvae/losses/vae_loss.py (`TransVAELoss(l1_weight, lpips_weight, kl_weight, vf_weight, gan_weight,
use_gan)`, `forward(reconstruction, target, mu, logvar, discriminator=None, dinov2=None) -> dict` with keys 'l1', 'kl', 'total').
The LPIPS term (vae_loss.py:86-91) is computed by a `PerceptualLoss` (transvae/losses/lpips.py, VGG-16 on the HIP path) handed in
as `lpips_net`; its pretrained weights are not part of this package and cannot be fetched by it, so a non-zero lpips_weight
WITHOUT an lpips_net raises.  The VF term (vae_loss.py:99-101) is computed by a `VFLoss` handed in as `vf_loss` when forward() is
given a `DinoV2Features` as `dinov2` (transvae/losses/vf.py: the DINOv2 ViT and the head on the HIP path; weights loaded by the
caller); a `dinov2` without a `vf_loss`, or one that is not a `DinoV2Features`, raises.  The GAN term (vae_loss.py:103-111) takes the caller's discriminator -- `transvae.PatchDiscriminator` on the HIP path,
or any module returning logits -- and `DiscriminatorLoss` (vae_loss.py:199-244) is the discriminator's own objective; both
run through `tv_gan_loss`, value and gradients in one pass.  The two closed-form terms are

    l1 = l1_weight * mean |reconstruction - target|                                   (vae_loss.py:83-84)
    kl = kl_weight * -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) / (B * H_lat * W_lat)  (vae_loss.py:94-96)

with the patched copy's variants as options: `sigmoid_recon=True` (P/.../vae_loss.py:80-84), `kl_mean=True` and
`logvar_clip=(-30, 20)` (P/.../vae_loss.py:96-102; the bf16 trainer clamps before calling the loss, R/train_2.py:316-318).
`tv_vae_loss_l1_kl` reads each tensor once and writes the three gradients in the same pass.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ..hip import _lib as L
from ..hip import ops


class _FusedL1KL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, recon, target, mu, logvar, l1_weight, kl_weight, kl_mean, sigmoid, lo, hi):
        ops._need_gpu(recon, target, mu, logvar)
        recon_c, mu_c, lv_c = recon.float().contiguous(), mu.float().contiguous(), logvar.float().contiguous()
        # the pair (recon, target) is walked flat: both must share one layout
        target_c = target.float().contiguous()
        ops._require(recon_c.shape == target_c.shape and mu_c.shape == lv_c.shape and mu_c.dim() == 4,
                     "loss: reconstruction / target and mu / logvar must have equal shapes ([B, D, H, W] latents)")
        lib = L.load()
        n_img, n_lat = recon_c.numel(), mu_c.numel()
        denom = float(n_lat) if kl_mean else float(mu_c.shape[0] * mu_c.shape[2] * mu_c.shape[3])
        need = ctx.needs_input_grad
        d_recon = torch.empty_like(recon_c) if need[0] else None
        d_mu = torch.empty_like(mu_c) if need[2] else None
        d_lv = torch.empty_like(lv_c) if need[3] else None
        part = torch.empty((lib.tv_vae_loss_partial_count(n_img, n_lat),), dtype=torch.float32, device=recon.device)
        out = torch.empty((3,), dtype=torch.float32, device=recon.device)
        with torch.cuda.device(recon.device):
            L.check(lib.tv_vae_loss_l1_kl(ops._p(recon_c), ops._p(target_c), ops._p(mu_c), ops._p(lv_c), ops._p(d_recon), ops._p(d_mu),
                                          ops._p(d_lv), ops._p(part), ops._p(out), n_img, n_lat, float(l1_weight), float(kl_weight), denom,
                                          int(bool(sigmoid)), float(lo), float(hi), ops._stream()), "tv_vae_loss_l1_kl")
        ctx.save_for_backward(d_recon, d_mu, d_lv)
        ctx.dtypes = (recon.dtype, mu.dtype, logvar.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        d_recon, d_mu, d_lv = ctx.saved_tensors
        # out = (l1, kl, total): the stored gradients are those of `total`; l1 depends on recon only, kl on mu / logvar only
        g_r = g[0] + g[2]
        g_k = g[1] + g[2]
        dr = (d_recon * g_r).to(ctx.dtypes[0]) if d_recon is not None else None
        dm = (d_mu * g_k).to(ctx.dtypes[1]) if d_mu is not None else None
        dl = (d_lv * g_k).to(ctx.dtypes[2]) if d_lv is not None else None
        return dr, None, dm, dl, None, None, None, None, None, None


def fused_l1_kl(reconstruction: torch.Tensor, target: torch.Tensor, mu: torch.Tensor, logvar: torch.Tensor,
                l1_weight: float = 1.0, kl_weight: float = 1e-8, kl_mean: bool = False, sigmoid_recon: bool = False,
                logvar_clip: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    """[l1, kl, total] (weighted) as one fp32 tensor of 3 elements; differentiable w.r.t. reconstruction, mu, logvar."""
    lo, hi = logvar_clip if logvar_clip is not None else (0.0, 0.0)
    return _FusedL1KL.apply(reconstruction, target, mu, logvar, l1_weight, kl_weight, kl_mean, sigmoid_recon, lo, hi)


_GAN_MODES = {"bce": L.GAN_BCE, "hinge": L.GAN_HINGE, "wgan": L.GAN_WGAN}


class _GanLossFn(torch.autograd.Function):
    """tv_gan_loss: the weighted value of one GAN term and, in the same pass, its gradient(s) w.r.t. the logits."""

    @staticmethod
    def forward(ctx, a, b, mode, weight):
        ops._need_gpu(a, b)
        ops._require(a.dtype == torch.float32 and (b is None or b.dtype == torch.float32), "GAN loss: logits must be fp32")
        ops._require(a.numel() > 0 and (b is None or b.numel() > 0), "GAN loss: empty logits")
        a_c = a.contiguous()
        b_c = b.contiguous() if b is not None else None
        lib = L.load()
        n_a, n_b = a_c.numel(), (b_c.numel() if b_c is not None else 0)
        da = torch.empty_like(a_c) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b_c) if (b_c is not None and ctx.needs_input_grad[1]) else None
        part = torch.empty((lib.tv_gan_loss_partial_count(n_a, n_b),), dtype=torch.float32, device=a.device)
        out = torch.empty((1,), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            L.check(lib.tv_gan_loss(ops._p(a_c), ops._p(b_c), ops._p(da), ops._p(db), ops._p(part), ops._p(out), n_a, n_b, int(mode),
                                    float(weight), ops._stream()), "tv_gan_loss")
        ctx.save_for_backward(da, db)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return (da * g if da is not None else None), (db * g if db is not None else None), None, None


def generator_gan_loss(fake_pred: torch.Tensor, weight: float = 1.0) -> torch.Tensor:
    """weight * binary_cross_entropy_with_logits(fake_pred, ones) (vae_loss.py:106-111), fp32 logits of any shape."""
    return _GanLossFn.apply(fake_pred.float(), None, L.GAN_GEN, weight)


class DiscriminatorLoss(nn.Module):
    """R/transvae/losses/vae_loss.py:199-244: 'bce' and 'hinge' are (real + fake) / 2, 'wgan' is -mean(real) + mean(fake).
    Value and both gradients come from one HIP pass over the two logit tensors (fp32, any shape)."""

    def __init__(self, loss_type: str = "bce"):
        super().__init__()
        if loss_type not in _GAN_MODES:
            raise ValueError(f"Unknown loss type: {loss_type}")
        self.loss_type = loss_type

    def forward(self, real_pred: torch.Tensor, fake_pred: torch.Tensor) -> torch.Tensor:
        if self.loss_type not in _GAN_MODES:    # (the attribute is public, as in the reference, which checks here)
            raise ValueError(f"Unknown loss type: {self.loss_type}")
        with torch.autocast("cuda", enabled=False):
            return _GanLossFn.apply(real_pred.float(), fake_pred.float(), _GAN_MODES[self.loss_type], 1.0)


class TransVAELoss(nn.Module):
    def __init__(self, l1_weight: float = 1.0, lpips_weight: float = 1.0, kl_weight: float = 1e-8, vf_weight: float = 0.1,
                 gan_weight: float = 0.05, use_gan: bool = False, sigmoid_recon: bool = False, kl_mean: bool = False,
                 logvar_clip: Optional[Tuple[float, float]] = None, lpips_net: Optional[nn.Module] = None,
                 vf_loss: Optional[nn.Module] = None):
        """Defaults are the reference's (R/transvae/losses/vae_loss.py:31-38: lpips 1.0, vf 0.1, gan 0.05, use_gan False), so
        `TransVAELoss()` cannot silently mean something else here: the LPIPS term (always on in the reference, which fetches
        the VGG weights from the network) needs `lpips_net`, a `transvae.PerceptualLoss` with loaded weights; a non-zero
        lpips_weight without one RAISES -- pass lpips_weight=0 for the closed-form terms alone.  The VF term only exists in
        the reference when its forward() is handed a DINOv2 model (vae_loss.py:99-101); here it needs `vf_loss`, a
        `transvae.VFLoss`, and a `transvae.DinoV2Features` handed to forward() -- any other `dinov2` raises.
        The GAN term exists, as in the reference, when use_gan is set AND forward() is handed a discriminator
        (vae_loss.py:103-111)."""
        super().__init__()
        if lpips_weight != 0.0 and lpips_net is None:
            raise ValueError("TransVAELoss (HIP path): the LPIPS term needs the external VGG network's weights, which this package "
                             "neither ships nor fetches; pass lpips_net=PerceptualLoss.from_file(...), or construct with "
                             "lpips_weight=0 for the closed-form L1 + KL terms")
        self.l1_weight, self.lpips_weight, self.kl_weight = l1_weight, lpips_weight, kl_weight
        self.vf_weight, self.gan_weight, self.use_gan = vf_weight, gan_weight, use_gan
        self.sigmoid_recon, self.kl_mean, self.logvar_clip = sigmoid_recon, kl_mean, logvar_clip
        self.lpips_net = lpips_net if lpips_weight != 0.0 else None   # a submodule: moves with .to(); buffers only, no parameters
        self.vf_loss = vf_loss                                        # a submodule as well; its `proj` is an ordinary parameter

    def forward(self, reconstruction, target, mu, logvar, discriminator=None, dinov2=None) -> dict:
        vf = None
        if dinov2 is not None and self.vf_weight > 0:
            from .vf import DinoV2Features
            if self.vf_loss is None or not isinstance(dinov2, DinoV2Features):
                raise ValueError("TransVAELoss (HIP path): the VF (DINOv2) term needs vf_loss=transvae.VFLoss(...) at construction and a "
                                 "transvae.DinoV2Features as dinov2; call without dinov2, or add that term with the reference's own module")
            vf = self.vf_loss(reconstruction, target, mu, dinov2) * self.vf_weight      # (vae_loss.py:99-101)
        out = fused_l1_kl(reconstruction, target, mu, logvar, self.l1_weight, self.kl_weight, self.kl_mean, self.sigmoid_recon,
                          self.logvar_clip)
        gan = None
        if self.use_gan and discriminator is not None and (self.gan_weight > 0 or not self.sigmoid_recon):
            # gan_weight * BCE_with_logits(D(reconstruction), ones) (vae_loss.py:103-111); the patched copy feeds the
            # discriminator sigmoid(reconstruction) and only when gan_weight > 0 (P/.../vae_loss.py:114-115)
            gan = self._gan_term(reconstruction, discriminator)
        if self.lpips_net is None and vf is None:
            if gan is None:
                return {"l1": out[0], "kl": out[1], "total": out[2]}
            return {"l1": out[0], "kl": out[1], "gan": gan, "total": out[0] + out[1] + gan}
        # the reference's key and sum order: l1, lpips, kl, vf, gan (vae_loss.py:83-114)
        losses = {"l1": out[0]}
        total = out[0]
        if self.lpips_net is not None:
            # lpips_weight * lpips(recon * 2 - 1, target * 2 - 1).mean() (vae_loss.py:86-91); under sigmoid_recon the patched copy's
            # order: sigmoid, 2x - 1, clamp to [-1, 1] on both images (P/.../vae_loss.py:80-91) -- all inside the network's input pass
            d = self.lpips_net.distance(reconstruction, target, normalize=True, sigmoid_input=self.sigmoid_recon, clamp=self.sigmoid_recon)
            losses["lpips"] = d.mean() * self.lpips_weight
            total = total + losses["lpips"]
        losses["kl"] = out[1]
        total = total + out[1]
        if vf is not None:
            losses["vf"] = vf
            total = total + vf
        if gan is not None:
            losses["gan"] = gan
            total = total + gan
        losses["total"] = total
        return losses

    def _gan_term(self, reconstruction, discriminator):
        if getattr(discriminator, "takes_sigmoid_flag", False):     # PatchDiscriminator: the sigmoid rides on its input pass
            fake_pred = discriminator(reconstruction, sigmoid_input=self.sigmoid_recon)
        else:
            fake_pred = discriminator(torch.sigmoid(reconstruction) if self.sigmoid_recon else reconstruction)
        with torch.autocast("cuda", enabled=False):
            return generator_gan_loss(fake_pred, self.gan_weight)
