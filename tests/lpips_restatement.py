"""LPIPS-VGG restated in plain torch ops from its public definition: the yardstick of tests/test_lpips_host.py and
tests/test_lpips_gpu.py.  Neither the `lpips` package nor torchvision is needed.

    scaling layer (x - shift) / scale; VGG-16 features: 13 x [3x3 conv pad 1 + ReLU], F.max_pool2d(2) before conv{2,3,4,5}_1;
    taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; per tap  f = x / (sqrt(sum_c x^2) + 1e-10),  d = sum_c lin_c (f_x - f_t)^2,
    spatial mean; the five taps summed -> [B, 1, 1, 1]

Weights are seeded and generated here, the same on every machine: convolutions He-scaled (std = sqrt(2 / (9 c_in))) with small
biases, so thirteen ReLU layers keep O(1) activations; `lin` weights non-negative, as in LPIPS.

`python tests/lpips_restatement.py --mint` rewrites tests/golden/lpips_ref_bf16_autocast.json: the restatement's OWN deviation
under torch.autocast("cpu", dtype=torch.bfloat16) from its fp32 run, per whole-loss case of the GPU test.
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

LAYERS = (("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128), ("conv3_1", 128, 256),
          ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512),
          ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512))
TAPS = ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")
POOL_BEFORE = ("conv2_1", "conv3_1", "conv4_1", "conv5_1")
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
SEED = 20240
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_ref_bf16_autocast.json")

# whole-loss cases of the GPU test: shapes x pairs
SHAPES = ((2, 64, 64), (2, 256, 256), (1, 128, 192))
PAIRS = ("unrelated", "noise0.05", "noise0.005")


def plain_state_dict(seed=SEED):
    """The documented plain scheme: conv1_1.weight ... conv5_3.bias, lin0 ... lin4 (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, c_in, c_out in LAYERS:
        sd[f"{name}.weight"] = torch.randn(c_out, c_in, 3, 3, generator=g) * math.sqrt(2.0 / (9 * c_in))
        sd[f"{name}.bias"] = torch.randn(c_out, generator=g) * 0.05
    for i, c in enumerate(TAP_CHANNELS):
        sd[f"lin{i}"] = torch.rand(c, generator=g) * (2.0 / c) * 8     # non-negative
    return sd


def lpips_package_state_dict(plain):
    """The same tensors under the key names of lpips.LPIPS(net='vgg').state_dict()."""
    idx = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
    sl = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    for (name, _, _), i, s in zip(LAYERS, idx, sl):
        sd[f"net.slice{s}.{i}.weight"] = plain[f"{name}.weight"]
        sd[f"net.slice{s}.{i}.bias"] = plain[f"{name}.bias"]
    for i in range(5):
        w = plain[f"lin{i}"].view(1, -1, 1, 1)
        sd[f"lin{i}.model.1.weight"] = w
        sd[f"lins.{i}.model.1.weight"] = w
    return sd


def features(x, sd):
    """x in [-1, 1] -> the five tap tensors (NCHW)."""
    dt = x.dtype
    shift = torch.tensor(SHIFT, dtype=dt).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dt).view(1, 3, 1, 1)
    h = (x - shift) / scale
    taps = []
    for name, _, _ in LAYERS:
        if name in POOL_BEFORE:
            h = F.max_pool2d(h, 2)
        h = F.relu(F.conv2d(h, sd[f"{name}.weight"].to(dt), sd[f"{name}.bias"].to(dt), padding=1))
        if name in TAPS:
            taps.append(h)
    return taps


def head(fx, ft, lin):
    """One tap: [B, C, H, W] features, lin [C] -> [B]."""
    nx = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
    nt = ft / (torch.sqrt(torch.sum(ft ** 2, dim=1, keepdim=True)) + 1e-10)
    d = ((nx - nt) ** 2 * lin.to(fx.dtype).view(1, -1, 1, 1)).sum(dim=1)
    return d.mean(dim=(1, 2))


def lpips(x, t, sd, normalize=False):
    """[B, 1, 1, 1]; inputs in [-1, 1], or in [0, 1] with normalize=True."""
    if normalize:
        x, t = 2 * x - 1, 2 * t - 1
    fx, ft = features(x, sd), features(t, sd)
    val = 0
    for k in range(5):
        val = val + head(fx[k].float(), ft[k].float(), sd[f"lin{k}"].float())
    return val.view(-1, 1, 1, 1)


def case_inputs(shape, pair):
    """Seeded images in [0, 1]: (input, target)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(SEED + 7 * H + W + 1000 * PAIRS.index(pair))
    # smooth-ish images: low-resolution noise upsampled, plus fine noise
    t = F.interpolate(torch.rand(B, 3, H // 8, W // 8, generator=g), size=(H, W), mode="bilinear", align_corners=False)
    t = (0.8 * t + 0.2 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    if pair == "unrelated":
        x = F.interpolate(torch.rand(B, 3, H // 8, W // 8, generator=g), size=(H, W), mode="bilinear", align_corners=False)
        x = (0.8 * x + 0.2 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    else:
        x = t + float(pair[5:]) * torch.randn(B, 3, H, W, generator=g)
    return x.contiguous(), t.contiguous()


def value_and_grad(x, t, sd, autocast=False):
    """Per-image values [B] and d sum(values) / d x, fp32 (or the same graph under CPU bf16 autocast)."""
    x = x.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        v = lpips(x, t, sd, normalize=True).view(-1)
    v.float().sum().backward()
    return v.detach().float(), x.grad.detach().float()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def case_key(shape, pair):
    return "x".join(map(str, shape)) + ":" + pair


def mint():
    sd = plain_state_dict()
    out = {}
    for shape in SHAPES:
        for pair in PAIRS:
            x, t = case_inputs(shape, pair)
            v32, g32 = value_and_grad(x, t, sd)
            v16, g16 = value_and_grad(x, t, sd, autocast=True)
            out[case_key(shape, pair)] = {"value": rel_l2(v16, v32), "grad": rel_l2(g16, g32), "values_fp32": [float(u) for u in v32]}
            print(case_key(shape, pair), out[case_key(shape, pair)], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "rel-L2 deviation of the plain-torch LPIPS restatement under torch.autocast('cpu', bfloat16) from its fp32 run",
                   "torch": torch.__version__, "cases": out}, f, indent=1)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        mint()
