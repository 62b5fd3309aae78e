"""The DINOv2 ViT patch-feature extractor and the VF loss restated in plain torch ops: the yardstick of tests/test_vf_host.py
and tests/test_vf_gpu.py.  Neither torch.hub nor any DINOv2 package is needed.

The model is written from the public definition (facebookresearch/dinov2, DinoVisionTransformer): 14 x 14 patch embedding,
class token, position table interpolated bicubically to the patch grid, pre-norm blocks

    x <- x + ls1 * proj(attention(qkv(LayerNorm(x))))        head dimension 64, scale 1/8
    x <- x + ls2 * fc2(gelu(fc1(LayerNorm(x))))              erf GELU, MLP ratio 4

LayerNorm eps 1e-6, a final LayerNorm, and the patch tokens reshaped to [B, C, h, w].  The loss is a functional restatement of
R/transvae/losses/vae_loss.py:136-196 (resize :163-172, projection :175-184, F.normalize :187-188, mean cosine :191, clamp :194).

Weights are seeded and generated here, the same on every machine: projections scaled by 1 / sqrt(fan_in) (sqrt(2 / fan_in) in
front of the GELU), LayerScale gamma drawn AROUND 1 (not the 1e-5 initialisation, so the blocks matter), and one channel of
pos_embed scaled 50x (a residual stream with an outlier channel, as trained ViTs have).

`python tests/vf_restatement.py --mint` rewrites tests/golden/vf_ref_bf16_autocast.json: per whole-network case the rel-L2
deviation of the restatement's feature map from its own fp32 run under
    (a) torch.autocast("cpu", bfloat16)
    (b) the same with the token tensor rounded to bf16 after assembly and after every residual add
(b) is the yardstick of a path that STORES a bf16 residual stream; autocast keeps it in fp32.
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

VARIANTS = {"vits14": (384, 6, 12), "vitb14": (768, 12, 12), "vitl14": (1024, 16, 24)}
PATCH = 14
SEED = 20250
SPIKE_CHANNEL, SPIKE = 5, 50.0
PRETRAIN_GRID = 37
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vf_ref_bf16_autocast.json")

# whole-network cases of the GPU test: name -> (variant, depth, images, source H x W, size)
CASES = {
    "vits14-d12-2x256-to-224": ("vits14", 12, 2, (256, 256), (224, 224)),
    "vitb14-d2-1x150x200-to-112x168": ("vitb14", 2, 1, (150, 200), (112, 168)),
    "vits14-d2-3x96x128-to-224": ("vits14", 2, 3, (96, 128), (224, 224)),
}


def state_dict(variant, depth=None, seed=SEED, grid=PRETRAIN_GRID):
    """The plain scheme (= the hub checkpoint's names): cls_token, pos_embed, patch_embed.proj.*, blocks.{i}.*, norm.* (fp32, CPU)."""
    D, _, full = VARIANTS[variant]
    depth = full if depth is None else depth
    g = torch.Generator().manual_seed(seed + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"cls_token": rn(1, 1, D) * 0.5, "pos_embed": rn(1, 1 + grid * grid, D) * 0.5,
          "patch_embed.proj.weight": rn(D, 3, PATCH, PATCH) / math.sqrt(3 * PATCH * PATCH), "patch_embed.proj.bias": rn(D) * 0.05}
    sd["pos_embed"][..., SPIKE_CHANNEL] *= SPIKE
    for i in range(depth):
        p = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"] = 1 + 0.1 * rn(D)
            sd[p + n + ".bias"] = 0.1 * rn(D)
        sd[p + "attn.qkv.weight"] = rn(3 * D, D) / math.sqrt(D)
        sd[p + "attn.qkv.bias"] = rn(3 * D) * 0.05
        sd[p + "attn.proj.weight"] = rn(D, D) / math.sqrt(D)
        sd[p + "attn.proj.bias"] = rn(D) * 0.05
        sd[p + "mlp.fc1.weight"] = rn(4 * D, D) / math.sqrt(D)
        sd[p + "mlp.fc1.bias"] = rn(4 * D) * 0.05
        sd[p + "mlp.fc2.weight"] = rn(D, 4 * D) * math.sqrt(2.0 / (4 * D))
        sd[p + "mlp.fc2.bias"] = rn(D) * 0.05
        sd[p + "ls1.gamma"] = 1 + 0.1 * rn(D)
        sd[p + "ls2.gamma"] = 1 + 0.1 * rn(D)
    sd["norm.weight"] = 1 + 0.1 * rn(D)
    sd["norm.bias"] = 0.1 * rn(D)
    return sd


def hub_state_dict(plain):
    """The same tensors as a hub checkpoint holds them: the plain names plus the training-only mask_token."""
    sd = dict(plain)
    sd["mask_token"] = torch.zeros(1, plain["cls_token"].shape[-1])
    return sd


def pos_table(pos_embed, h, w, offset=0.1, antialias=False):
    """[1, 1 + M*M, D] -> [1, 1 + h*w, D]: bicubic resampling of the patch table, scale_factor = ((h + offset) / M, (w + offset) / M)
    (size=(h, w) when offset is 0), class row unchanged; unchanged when (h, w) == (M, M)."""
    n = pos_embed.shape[1] - 1
    M = int(round(math.sqrt(n)))
    if (h, w) == (M, M):
        return pos_embed
    D = pos_embed.shape[-1]
    grid = pos_embed[:, 1:].reshape(1, M, M, D).permute(0, 3, 1, 2)
    kw = dict(scale_factor=((h + offset) / M, (w + offset) / M)) if offset else dict(size=(h, w))
    grid = F.interpolate(grid.float(), mode="bicubic", antialias=antialias, **kw).to(pos_embed.dtype)
    assert tuple(grid.shape[-2:]) == (h, w)
    return torch.cat([pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, h * w, D)], dim=1)


def features(img, sd, variant, size=(224, 224), imagenet_norm=True, round_stream=False):
    """img [B, 3, H, W] in [0, 1] -> [B, C, h, w]; round_stream: the token tensor rounded to bf16 after assembly and after
    every residual add (policy (b))."""
    D, heads, _ = VARIANTS[variant]
    depth = sum(1 for k in sd if k.endswith(".ls1.gamma"))
    rs = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if round_stream else (lambda t: t)
    x = F.interpolate(img, size=size, mode="bilinear", align_corners=False)
    if imagenet_norm:
        x = (x - torch.tensor(IMAGENET_MEAN, dtype=x.dtype).view(1, 3, 1, 1)) / torch.tensor(IMAGENET_STD, dtype=x.dtype).view(1, 3, 1, 1)
    B = x.shape[0]
    h, w = size[0] // PATCH, size[1] // PATCH
    dt = img.dtype
    W = lambda k: sd[k].to(dt)
    tok = F.conv2d(x, W("patch_embed.proj.weight"), W("patch_embed.proj.bias"), stride=PATCH).flatten(2).transpose(1, 2)   # [B, h w, D]
    tok = torch.cat([W("cls_token").expand(B, -1, -1), tok.to(dt)], dim=1) + pos_table(W("pos_embed"), h, w)
    tok = rs(tok)
    N = tok.shape[1]
    for i in range(depth):
        p = f"blocks.{i}."
        y = F.layer_norm(tok, (D,), W(p + "norm1.weight"), W(p + "norm1.bias"), 1e-6)
        qkv = F.linear(y, W(p + "attn.qkv.weight"), W(p + "attn.qkv.bias")).reshape(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = torch.softmax((q @ k.transpose(-2, -1)) * (D // heads) ** -0.5, dim=-1)
        o = (att @ v).transpose(1, 2).reshape(B, N, D)
        o = F.linear(o, W(p + "attn.proj.weight"), W(p + "attn.proj.bias"))
        tok = rs(tok + W(p + "ls1.gamma") * o)
        y = F.layer_norm(tok, (D,), W(p + "norm2.weight"), W(p + "norm2.bias"), 1e-6)
        y = F.linear(F.gelu(F.linear(y, W(p + "mlp.fc1.weight"), W(p + "mlp.fc1.bias"))), W(p + "mlp.fc2.weight"), W(p + "mlp.fc2.bias"))
        tok = rs(tok + W(p + "ls2.gamma") * y)
    out = F.layer_norm(tok, (D,), W("norm.weight"), W("norm.bias"), 1e-6)[:, 1:]
    return out.reshape(B, h, w, D).permute(0, 3, 1, 2)


def vf_loss(latent, feats, weight=None, bias=None, margin=0.4):
    """vae_loss.py:163-194 on a precomputed feature map: latent [B, D, Hl, Wl], feats [B, C, h, w]; weight [C, D] / bias [C] of
    the projection (None: D == C)."""
    if latent.shape[-2:] != feats.shape[-2:]:
        latent = F.interpolate(latent, size=feats.shape[-2:], mode="bilinear", align_corners=False)          # :167-172
    if weight is not None:
        B, _, h, w = latent.shape
        latent = F.linear(latent.flatten(2).transpose(1, 2), weight, bias).transpose(1, 2).reshape(B, -1, h, w)   # :175-182
    sim = (F.normalize(latent, dim=1) * F.normalize(feats, dim=1)).sum(dim=1).mean()                          # :187-191
    return torch.clamp(margin - sim, min=0.0)                                                                  # :194


def case_inputs(name):
    variant, depth, B, (H, W), size = CASES[name]
    g = torch.Generator().manual_seed(SEED + 13 * H + W + B)
    img = F.interpolate(torch.rand(B, 3, max(2, H // 8), max(2, W // 8), generator=g), size=(H, W), mode="bilinear", align_corners=False)
    img = (0.8 * img + 0.2 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    return img.contiguous()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def mint():
    out = {}
    for name, (variant, depth, B, hw, size) in CASES.items():
        sd = state_dict(variant, depth)
        img = case_inputs(name)
        with torch.no_grad():
            f32 = features(img, sd, variant, size)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                fa = features(img, sd, variant, size).float()
                fb = features(img, sd, variant, size, round_stream=True).float()
        out[name] = {"autocast": rel_l2(fa, f32), "autocast_bf16_stream": rel_l2(fb, f32), "norm_fp32": float(f32.double().norm())}
        print(name, out[name], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "rel-L2 deviation of the plain-torch DINOv2 ViT restatement's feature map from its fp32 run under (a) "
                           "torch.autocast('cpu', bfloat16) and (b) the same with a bf16-rounded residual stream",
                   "torch": torch.__version__, "cases": out}, f, indent=1)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        mint()
