"""Plain-torch restatement of the adversarial stage: the yardstick of tests/test_gan_host.py and tests/test_gan_gpu.py.

* the 70x70 PatchGAN (pix2pix / taming `NLayerDiscriminator`, n_layers = 3) as an `nn.Sequential` of Conv2d / BatchNorm2d /
  LeakyReLU(0.2) under the name `main`, with SEEDED test weights generated here (He-scaled, so activations are O(1) and errors
  are not hidden behind tiny numbers; the package's own init is N(0, 0.02));
* the three `DiscriminatorLoss` forms and the generator term, restated from R/transvae/losses/vae_loss.py:103-111, 226-241.

`python tests/gan_restatement.py --mint` writes tests/golden/gan_ref_bf16_autocast.json: this restatement's OWN deviation under
`torch.autocast("cpu", dtype=torch.bfloat16)` from its fp32 run, for every whole-network case of the GPU test (logits,
d/d input and every parameter gradient, each as rel-L2).  The HIP path stores activations in bf16, so that is the honest scale.
"""
import json
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_ref_bf16_autocast.json")
SEED = 20261
SHAPES = ((2, 64, 64), (2, 256, 256), (1, 128, 192))     # (B, H, W)
MODES = ("train", "eval")

STATE_KEYS = (["main.0.weight", "main.0.bias", "main.2.weight"]
              + [f"main.{i}.{k}" for i in (3,) for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
              + ["main.5.weight"]
              + [f"main.6.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
              + ["main.8.weight"]
              + [f"main.9.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
              + ["main.11.weight", "main.11.bias"])


class PatchGAN(nn.Module):
    def __init__(self, input_channels=3, ndf=64, n_layers=3):
        super().__init__()
        seq = [nn.Conv2d(input_channels, ndf, 4, 2, 1), nn.LeakyReLU(0.2)]
        c = ndf
        for i in range(1, n_layers + 1):
            stride = 2 if i < n_layers else 1
            seq += [nn.Conv2d(c, 2 * c, 4, stride, 1, bias=False), nn.BatchNorm2d(2 * c), nn.LeakyReLU(0.2)]
            c *= 2
        seq += [nn.Conv2d(c, 1, 4, 1, 1)]
        self.main = nn.Sequential(*seq)

    def forward(self, x):
        return self.main(x)


def seeded_patchgan(ndf=64, seed=SEED):
    """He-scaled conv weights, BatchNorm weight N(1, 0.1) / bias N(0, 0.1), non-trivial running statistics."""
    g = torch.Generator().manual_seed(seed)
    net = PatchGAN(ndf=ndf)
    with torch.no_grad():
        for m in net.main:
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * 16
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_in))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return net


# ---- loss terms (R/transvae/losses/vae_loss.py) ---------------------------------------------------------------------------
def generator_term(fake_pred, gan_weight=1.0):
    """:106-111"""
    return F.binary_cross_entropy_with_logits(fake_pred, torch.ones_like(fake_pred)) * gan_weight


def discriminator_loss(real_pred, fake_pred, loss_type="bce"):
    """:226-241"""
    if loss_type == "bce":
        real_loss = F.binary_cross_entropy_with_logits(real_pred, torch.ones_like(real_pred))
        fake_loss = F.binary_cross_entropy_with_logits(fake_pred, torch.zeros_like(fake_pred))
        return (real_loss + fake_loss) / 2
    if loss_type == "hinge":
        return (torch.mean(F.relu(1.0 - real_pred)) + torch.mean(F.relu(1.0 + fake_pred))) / 2
    if loss_type == "wgan":
        return -torch.mean(real_pred) + torch.mean(fake_pred)
    raise ValueError(f"Unknown loss type: {loss_type}")


# ---- whole-network cases ---------------------------------------------------------------------------------------------------
def case_input(shape):
    """Seeded image in [0, 1]: low-resolution noise upsampled plus fine noise."""
    B, H, W = shape
    g = torch.Generator().manual_seed(SEED + 7 * H + W)
    x = F.interpolate(torch.rand(B, 3, H // 8, W // 8, generator=g), size=(H, W), mode="bilinear", align_corners=False)
    return (0.7 * x + 0.3 * torch.rand(B, 3, H, W, generator=g)).contiguous()


def case_key(shape, mode):
    return "x".join(map(str, shape)) + ":" + mode


def run_case(net, x, mode, autocast=False):
    """logits, d loss / d x and {parameter name: d loss / d parameter} for loss = the generator term of the logits."""
    net = net.train() if mode == "train" else net.eval()
    for p in net.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        logits = net(x)
    generator_term(logits.float()).backward()
    grads = {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}
    return logits.detach().float(), x.grad.detach().float(), grads


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def mint():
    out = {}
    for shape in SHAPES:
        for mode in MODES:
            x = case_input(shape)
            l32, g32, p32 = run_case(seeded_patchgan(), x, mode)
            l16, g16, p16 = run_case(seeded_patchgan(), x, mode, autocast=True)
            out[case_key(shape, mode)] = {"logits": rel_l2(l16, l32), "input_grad": rel_l2(g16, g32),
                                          "param_grads": {k: rel_l2(p16[k], p32[k]) for k in p32}}
            print(case_key(shape, mode), out[case_key(shape, mode)], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "rel-L2 deviation of the plain-torch PatchGAN restatement under torch.autocast('cpu', bfloat16) from its fp32 run "
                           "(loss = generator BCE term of the logits)",
                   "torch": torch.__version__, "cases": out}, f, indent=1)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        mint()
