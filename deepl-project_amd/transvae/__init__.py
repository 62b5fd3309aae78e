"""transvae -- MI355X-native TransVAE forward/backward path.

Import surface of the reference package (R/transvae/__init__.py:5-9): `from transvae import
TransVAE, create_transvae, TransVAELoss`.  The loss re-exported here holds the closed-form L1 + KL terms
(one fused HIP pass, transvae/losses/vae_loss.py) and, given a `PerceptualLoss`, the reference's LPIPS term:
`PerceptualLoss` (transvae/losses/lpips.py) is LPIPS-VGG on the HIP path -- thirteen ReLU convolutions through the same
implicit-GEMM kernels as the model, max-pools and the LPIPS head in csrc/lpips.hip.  It ships WITHOUT weights: load the state
dict of `lpips.LPIPS(net='vgg')` with `PerceptualLoss.from_file`.  The adversarial stage (stage 2 of the
reference's configs) is `TransVAELoss(use_gan=True)` handed a discriminator, `DiscriminatorLoss` for the discriminator's own
objective, and `PatchDiscriminator` (transvae/models/discriminator.py), the 70x70 PatchGAN on the HIP path, trained from
scratch.  The VF alignment term (stage 1 of the reference's configs: L1 + LPIPS + KL + VF) is `TransVAELoss(vf_loss=VFLoss(...))`
handed a `DinoV2Features` as `dinov2`: the DINOv2 ViT patch-feature extractor on the HIP path (transvae/losses/vf.py, csrc/vf.hip;
weights loaded with `DinoV2Features.from_file`, none ship) and the cosine head with its gradient into the latent.  The evaluation side (R/evaluate.py) is `evaluate` with per-image
PSNR / SSIM / MSE from `reconstruction_metrics` (transvae/metrics.py), LPIPS from a `PerceptualLoss` and rFID from an
`InceptionFeatures` (the FID Inception-v3 on the HIP path, transvae/metrics_fid.py; weights loaded from the pt_inception file)
with a `FrechetDistance`, computed on the device.  The image pipeline (transvae/image_io.py, csrc/image.hip): `ImagePrep` is the
scripts' `Resize -> CenterCrop -> ToTensor` for a ragged uint8 batch (`collate_uint8` / `UInt8Batch`) in one launch, bit-equal to
PIL; `to_uint8_grid` / `save_image` stand in for torchvision's `make_grid` / `save_image`; transvae/generate.py holds the three
modes of P/generate_images.py.  Latent extraction and latent-space analysis (transvae/latents.py, csrc/latent.hip):
`extract_latents` writes the encoder's latents and their per-channel statistics (`LatentStats`, streaming fp64 moments) for a
downstream generator; `latent_points`, `latent_density_metrics` and `latent_space_metrics` compute the density CV / normalised
entropy / Gini table from a log-domain Gaussian kernel density estimate.  Linear probing of latents (transvae/probe.py,
csrc/probe.hip): `probe_rows` builds the classifier's bf16 operand from stored latents, `softmax_xent` is the cross-entropy with
its gradient and top-1 / top-5 counts in one pass, `LinearProbe` one linear layer; `fit_linear_probe` trains it on
`extract_latents` shards with `FusedAdamW` and `linear_probe_accuracy` runs the extraction first.  The latent diffusion transformer
(transvae/dit.py, csrc/dit.hip): `DiT` / `create_dit` are adaLN-Zero DiT blocks on the stored latents (token GEMMs and attention on
the existing kernels, the conditioning arithmetic and the flow-matching edge in csrc/dit.hip); `flow_matching_loss` is one training
step's loss and backward, `fit_dit` trains on `extract_latents` shards with `FusedAdamW`, `sample_latents` / `sample_images`
integrate the velocity field with Euler steps and classifier-free guidance and decode through the autoencoder; the LightningDiT recipe
is behind keywords whose defaults change nothing (`cosine_weight`; `method="heun"`, `timestep_shift`, `cfg_interval`).  Generator evaluation
(transvae/evaluate_dit.py, transvae/metrics_gen.py, csrc/genmetrics.hip): `evaluate_dit` samples, extracts Inception features and
returns gFID, Inception Score (`InceptionScore`) and the k-NN precision / recall (`knn_radius`, `manifold_hits`,
`precision_recall`) against a `reference_statistics` dict, and on request sFID (the spatial tap of `InceptionFeatures.features(...,
spatial=True)`), KID (`kernel_inception_distance`, `poly_kernel_sums`, `kid_subsets`), density / coverage (`density_coverage`,
`ball_counts`) and the Inception Score as a mean over splits (`InceptionScore(..., split_size=...)`); `ParamEMA` (transvae/optim.py) is the weight average they are measured on,
kept by `fit_dit(..., ema_decay=...)`.  `LightningDiT` / `create_lightning_dit` (transvae/lightning_dit.py, csrc/lightning.hip, csrc/dit.hip)
are the same model with the LightningDiT block: RMSNorm adaLN with a learned weight, per-head qk-norm before the RoPE and a SwiGLU MLP,
each behind a switch; the training, sampling and evaluation entry points above take it unchanged.  `dit_xl` / `lightning_dit_xl` are
the XL configurations (1152 wide, 28 deep, 16 heads of head_dim 72: csrc/attention_hd.hip).  `with transvae.deterministic():`
(transvae/hip/ops.py, csrc/det_reduce.hip) makes every parameter gradient of the HIP kernels bit-reproducible from run to run.
"""
from .dit import DiT, create_dit, dit_xl, fit_dit, flow_matching_loss, sample_images, sample_latents
from .evaluate import evaluate
from .evaluate_dit import ALL_METRICS, evaluate_dit
from .hip.ops import deterministic
from .generate import interpolate_latents, random_samples, reconstruct
from .lightning_dit import LightningDiT, create_lightning_dit, lightning_dit_xl
from .latents import LatentStats, extract_latents, latent_density_metrics, latent_points, latent_space_metrics
from .image_io import ImagePrep, UInt8Batch, collate_uint8, save_image, to_uint8_grid
from .losses.lpips import PerceptualLoss
from .losses.vae_loss import DiscriminatorLoss, TransVAELoss
from .losses.vf import DinoV2Features, VFLoss
from .metrics import reconstruction_metrics
from .probe import LinearProbe, fit_linear_probe, linear_probe_accuracy, probe_rows, softmax_xent
from .metrics_fid import FrechetDistance, InceptionFeatures
from .metrics_gen import (InceptionScore, ball_counts, density_coverage, kernel_inception_distance, kid_subsets, knn_radius, manifold_hits,
                          poly_kernel_sums, precision_recall, reference_statistics)
from .optim import ParamEMA
from .models.discriminator import PatchDiscriminator
from .models.transvae import TransVAE, create_transvae

__version__ = "0.2.0"
__all__ = ["TransVAE", "create_transvae", "TransVAELoss", "reconstruction_metrics", "evaluate", "PerceptualLoss", "DiscriminatorLoss",
           "PatchDiscriminator", "InceptionFeatures", "FrechetDistance", "VFLoss", "DinoV2Features", "ImagePrep", "UInt8Batch",
           "collate_uint8", "to_uint8_grid", "save_image", "random_samples", "interpolate_latents", "reconstruct", "LatentStats",
           "extract_latents", "latent_points", "latent_density_metrics", "latent_space_metrics", "probe_rows", "softmax_xent", "LinearProbe",
           "fit_linear_probe", "linear_probe_accuracy", "DiT", "create_dit", "flow_matching_loss", "sample_latents", "sample_images", "fit_dit",
           "evaluate_dit", "InceptionScore", "knn_radius", "manifold_hits", "precision_recall", "reference_statistics", "ParamEMA",
           "LightningDiT", "create_lightning_dit", "deterministic", "dit_xl", "lightning_dit_xl", "ball_counts", "density_coverage",
           "kernel_inception_distance", "kid_subsets", "poly_kernel_sums", "ALL_METRICS"]
