from .lpips import PerceptualLoss
from .vae_loss import DiscriminatorLoss, TransVAELoss, fused_l1_kl, generator_gan_loss
from .vf import DinoV2Features, VFLoss

__all__ = ["TransVAELoss", "fused_l1_kl", "PerceptualLoss", "DiscriminatorLoss", "generator_gan_loss", "VFLoss", "DinoV2Features"]
