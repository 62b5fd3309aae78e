"""The VF alignment term on the HIP path: `VFLoss` of R/transvae/losses/vae_loss.py:119-196 and the DINOv2 ViT patch-feature
extractor it is handed.

`DinoV2Features` is the DINOv2 ViT (facebookresearch/dinov2 `DinoVisionTransformer`: patch 14, LayerNorm eps 1e-6, LayerScale,
MLP ratio 4 with erf GELU, head dimension 64), forward only and frozen.  The reference leaves its DINOv2 integration open
(R/PROJECT_STRUCTURE.md:164) and only fixes what the loss expects -- `dinov2(image) -> [B, C, h, w]` --, so this module defines
the extractor: `x_norm_patchtokens` after the final LayerNorm, reshaped.

    image fp32 NCHW in [0, 1], any size
      tv_vf_prep      bilinear resize to `size` (align_corners=False, no antialias), ImageNet normalisation (optional) in fp32,
                      ONE rounding, 14 x 14 patch rows [B h w, 608] bf16 (588 used)
      tv_igemm_nt     patch embedding (K = 608)
      tv_vit_tokens   [B, 1 + h w, D] bf16: cls + pos[0] | patch + pos[1 + p]   (position table interpolated on the host, once per grid)
      per block       tv_rownorm_fwd mode 2 (affine-free LayerNorm; its affine is folded into the next projection)
                      qkv GEMM + bias, tv_attn_fwd (scale 1/8, no table), proj GEMM + bias + residual,
                      LayerNorm, fc1 GEMM + bias + GELU, fc2 GEMM + bias + residual   (LayerScale folded into proj / fc2)
      tv_layernorm_rows   final LayerNorm with its affine on the patch rows only -> [B h w, D] fp32

Weights are BUFFERS, folded in fp32 and packed to bf16 operands once at load time.  No weights ship with the package and none are
downloaded: `DinoV2Features.from_file(path, variant)` / `load_dinov2_state_dict(sd)`.  There is no CPU fallback.

`VFLoss` is the loss arithmetic of the reference: the latent resized bilinearly to the feature grid, `proj = Linear(D, C)` when
D != C, both sides L2-normalised over channels, the cosine averaged over all positions, `clamp(margin - similarity, min=0)`.
Value and gradients come from `tv_vf_head` (+ `tv_bilinear_nchw_bwd`, `tv_vf_head_dproj`), fp32 throughout.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..hip import _lib as L
from ..hip import ops

BF16 = torch.bfloat16
PATCH = 14
K_PATCH, K_PAD = 3 * PATCH * PATCH, 608
LN_EPS = 1e-6
VARIANTS = {"vits14": (384, 6, 12), "vitb14": (768, 12, 12), "vitl14": (1024, 16, 24)}     # width, heads, depth
BLOCK_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ls1.gamma",
              "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma")


def plain_keys(depth: int) -> List[str]:
    """The documented key scheme (the hub checkpoint's own names, without `mask_token`)."""
    keys = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(depth):
        keys += [f"blocks.{i}.{k}" for k in BLOCK_KEYS]
    return keys + ["norm.weight", "norm.bias"]


def to_plain_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Hub checkpoint names -> the plain scheme: a `backbone.` / `module.` prefix is dropped, chunked blocks
    (`blocks.{chunk}.{i}.`) are flattened, `mask_token` (training only) is left out.  Raises on register-token and SwiGLU
    checkpoints."""
    out = {}
    for k, v in sd.items():
        for pre in ("module.", "backbone."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k == "register_tokens" or k.startswith("register_tokens"):
            raise ValueError("DinoV2Features: register-token checkpoints (dinov2_*_reg) are not supported")
        if ".mlp.w12." in k or ".mlp.w3." in k:
            raise ValueError("DinoV2Features: the SwiGLU MLP (vitg14) is not supported")
        if k == "mask_token":
            continue
        parts = k.split(".")
        if parts[0] == "blocks" and len(parts) > 3 and parts[1].isdigit() and parts[2].isdigit():
            k = ".".join(["blocks", parts[2]] + parts[3:])
        out[k] = v
    return out


def interpolate_pos_table(pos_embed: torch.Tensor, h: int, w: int, offset: float = 0.1, antialias: bool = False) -> torch.Tensor:
    """[1, 1 + M*M, D] -> [1 + h*w, D] fp32: the class row unchanged, the M x M patch table resampled bicubically to h x w as
    upstream's `interpolate_pos_encoding` does: with `offset` (0.1 in the hub models) by
    `scale_factor=((h + offset) / M, (w + offset) / M)`, with offset 0 by `size=(h, w)`; unchanged when (h, w) == (M, M).
    (Upstream hands the pair over as (w, h); the two agree on square grids.)"""
    pos = pos_embed.float().reshape(-1, pos_embed.shape[-1])
    n = pos.shape[0] - 1
    M = int(round(math.sqrt(n)))
    if M * M != n:
        raise ValueError(f"pos_embed has {n} patch rows, not a square")
    if (h, w) == (M, M):
        return pos.contiguous()
    D = pos.shape[1]
    grid = pos[1:].reshape(1, M, M, D).permute(0, 3, 1, 2)
    if offset:
        res = F.interpolate(grid, scale_factor=((h + offset) / M, (w + offset) / M), mode="bicubic", antialias=antialias)
    else:
        res = F.interpolate(grid, size=(h, w), mode="bicubic", antialias=antialias)
    if tuple(res.shape[-2:]) != (h, w):
        raise ValueError(f"position table: interpolation gave {tuple(res.shape[-2:])}, wanted {(h, w)}")
    return torch.cat([pos[:1], res.permute(0, 2, 3, 1).reshape(h * w, D)]).contiguous()


def fold_block(sd: Dict[str, torch.Tensor], i: int) -> Dict[str, torch.Tensor]:
    """The four projections of block i with the LayerNorm affine folded into qkv / fc1 (W' = W diag(g), b' = b + W beta) and
    LayerScale into proj / fc2 (W' = diag(gamma) W, b' = gamma b), in the dtype of `sd` (fp32 at pack time, fp64 in the tests)."""
    p = f"blocks.{i}."
    g1, b1, g2, b2 = sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "norm2.weight"], sd[p + "norm2.bias"]
    ls1, ls2 = sd[p + "ls1.gamma"], sd[p + "ls2.gamma"]
    wq, wf = sd[p + "attn.qkv.weight"], sd[p + "mlp.fc1.weight"]
    return {"qkv.w": wq * g1[None, :], "qkv.b": sd[p + "attn.qkv.bias"] + wq @ b1,
            "proj.w": ls1[:, None] * sd[p + "attn.proj.weight"], "proj.b": ls1 * sd[p + "attn.proj.bias"],
            "fc1.w": wf * g2[None, :], "fc1.b": sd[p + "mlp.fc1.bias"] + wf @ b2,
            "fc2.w": ls2[:, None] * sd[p + "mlp.fc2.weight"], "fc2.b": ls2 * sd[p + "mlp.fc2.bias"]}


def _bname(key: str) -> str:
    return key.replace(".", "_")


# ---------------------------------------------------------------------------------------------------------------------
# raw launches
# ---------------------------------------------------------------------------------------------------------------------
def vf_prep(img: torch.Tensor, gh: int, gw: int, imagenet_norm: bool) -> torch.Tensor:
    ops._need_gpu(img)
    ops._require(img.dim() == 4 and img.shape[1] == 3 and img.dtype == torch.float32 and img.is_contiguous(), "vf_prep: contiguous fp32 [B, 3, H, W]")
    B, _, H, W = img.shape
    rows = torch.empty((B * gh * gw, K_PAD), dtype=BF16, device=img.device)
    L.check(L.load().tv_vf_prep(ops._p(img), ops._p(rows), B, H, W, gh, gw, int(bool(imagenet_norm)), ops._stream()), "tv_vf_prep")
    return rows


def vit_tokens(patch: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int) -> torch.Tensor:
    ops._need_gpu(patch, cls, pos)
    T, D = patch.shape
    P = T // B
    ops._require(patch.dtype == BF16 and patch.is_contiguous() and T == B * P and cls.dtype == torch.float32 and cls.numel() == D
                 and cls.is_contiguous() and pos.dtype == torch.float32 and pos.is_contiguous() and tuple(pos.shape) == (P + 1, D),
                 "vit_tokens: operand check failed")
    tok = torch.empty((B, P + 1, D), dtype=BF16, device=patch.device)
    L.check(L.load().tv_vit_tokens(ops._p(patch), ops._p(cls), ops._p(pos), ops._p(tok), B, P, D, ops._stream()), "tv_vit_tokens")
    return tok


def layernorm_hat(x: torch.Tensor, eps: float = LN_EPS) -> torch.Tensor:
    """(x - mean) rsqrt(var + eps) per row, bf16 [T, C] -> bf16 (tv_rownorm_fwd mode 2)."""
    ops._need_gpu(x)
    ops._require(x.dim() == 2 and x.dtype == BF16 and x.is_contiguous(), "layernorm_hat: contiguous bf16 [T, C]")
    y = torch.empty_like(x)
    L.check(L.load().tv_rownorm_fwd(ops._p(x), None, ops._p(y), x.shape[0], x.shape[1], 2, 0.0, eps, ops._stream()), "tv_rownorm_fwd")
    return y


def layernorm_rows(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, skip: int, eps: float = LN_EPS) -> torch.Tensor:
    """LayerNorm with affine on rows skip.. of every image of x [B, N, C] bf16 -> fp32 [B * (N - skip), C]."""
    ops._need_gpu(x, gamma, beta)
    B, N, Cc = x.shape
    ops._require(x.dtype == BF16 and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
                 and gamma.numel() == Cc and beta.numel() == Cc and gamma.is_contiguous() and beta.is_contiguous() and 0 <= skip < N,
                 "layernorm_rows: operand check failed")
    y = torch.empty((B * (N - skip), Cc), dtype=torch.float32, device=x.device)
    L.check(L.load().tv_layernorm_rows(ops._p(x), ops._p(gamma), ops._p(beta), ops._p(y), B, N, skip, Cc, eps, ops._stream()), "tv_layernorm_rows")
    return y


def _linear(x: torch.Tensor, wb: torch.Tensor, bias: torch.Tensor, residual: Optional[torch.Tensor] = None, act: int = L.ACT_NONE) -> torch.Tensor:
    T, K = x.shape
    n = wb.shape[0]
    out = torch.empty((T, n), dtype=BF16, device=x.device)
    d = ops._rows_desc(T, K, n)
    d.act = act
    ops.igemm(d, x, wb, bias, residual, None, out)
    return out


def attention_fwd(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """softmax(q k^T / 8) v on qkv [B, N, 3 * heads * 64] bf16, no position table, forward only."""
    B, N, C3 = qkv.shape
    ops._require(qkv.dtype == BF16 and qkv.is_contiguous() and C3 == 3 * heads * 64, "attention_fwd: operand check failed")
    o = torch.empty((B, N, heads * 64), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
    L.check(L.load().tv_attn_fwd(ops._p(qkv), ops._p(o), ops._p(lse), B, N, heads, 0.125, ops._stream()), "tv_attn_fwd")
    return o


# ---------------------------------------------------------------------------------------------------------------------
# the extractor
# ---------------------------------------------------------------------------------------------------------------------
class DinoV2Features(nn.Module):
    """`forward(image) -> [B, C, h, w]` fp32 patch features (a strided view of the token-major result, which
    :meth:`tokens` returns as [B*h*w, C]).  Frozen: buffers only, no gradient to the image or the weights."""

    def __init__(self, variant: str = "vits14", size: Tuple[int, int] = (224, 224), imagenet_norm: bool = True, depth: Optional[int] = None,
                 interpolate_offset: float = 0.1, interpolate_antialias: bool = False, pretrain_grid: int = 37):
        super().__init__()
        if variant not in VARIANTS:
            raise ValueError(f"DinoV2Features: unknown variant {variant!r} (one of {sorted(VARIANTS)}; vitg14 and the register-token "
                             "models are not supported)")
        if isinstance(size, int):
            size = (size, size)
        if len(size) != 2 or size[0] <= 0 or size[1] <= 0 or size[0] % PATCH or size[1] % PATCH:
            raise ValueError(f"DinoV2Features: size must be two positive multiples of {PATCH}, got {size}")
        self.variant, self.size, self.imagenet_norm = variant, (int(size[0]), int(size[1])), bool(imagenet_norm)
        self.width, self.heads, full = VARIANTS[variant]
        self.depth = full if depth is None else int(depth)
        if not 0 < self.depth <= full:
            raise ValueError(f"DinoV2Features: depth must be in 1..{full}")
        self.interpolate_offset, self.interpolate_antialias = float(interpolate_offset), bool(interpolate_antialias)
        D = self.width
        shapes = {"cls_token": (1, 1, D), "pos_embed": (1, 1 + pretrain_grid * pretrain_grid, D),
                  "patch_embed.proj.weight": (D, 3, PATCH, PATCH), "patch_embed.proj.bias": (D,), "norm.weight": (D,), "norm.bias": (D,)}
        blk = {"norm1.weight": (D,), "norm1.bias": (D,), "attn.qkv.weight": (3 * D, D), "attn.qkv.bias": (3 * D,), "attn.proj.weight": (D, D),
               "attn.proj.bias": (D,), "ls1.gamma": (D,), "norm2.weight": (D,), "norm2.bias": (D,), "mlp.fc1.weight": (4 * D, D),
               "mlp.fc1.bias": (4 * D,), "mlp.fc2.weight": (D, 4 * D), "mlp.fc2.bias": (D,), "ls2.gamma": (D,)}
        for i in range(self.depth):
            for k, s in blk.items():
                shapes[f"blocks.{i}.{k}"] = s
        self._shapes = shapes
        for k in plain_keys(self.depth):
            self.register_buffer(_bname(k), torch.zeros(shapes[k]))
        # operands of the kernels, derived by _pack(): not part of the state dict
        self.register_buffer("_op_pe", torch.zeros(0, dtype=BF16), persistent=False)
        for i in range(self.depth):
            for nm in ("qkv", "proj", "fc1", "fc2"):
                self.register_buffer(f"_op_{i}_{nm}_w", torch.zeros(0, dtype=BF16), persistent=False)
                self.register_buffer(f"_op_{i}_{nm}_b", torch.zeros(0), persistent=False)
        self._pos_cache: Dict[tuple, torch.Tensor] = {}
        self._pack()

    # ---- weights ------------------------------------------------------------------------------------------------------
    def plain_state(self) -> Dict[str, torch.Tensor]:
        return {k: getattr(self, _bname(k)) for k in plain_keys(self.depth)}

    @torch.no_grad()
    def _pack(self):
        """fp32 folds (LayerNorm affine into qkv / fc1, LayerScale into proj / fc2), then one rounding to the bf16 operands; the
        patch embedding as [D, 608] over the (c, ky, kx) patch rows.  Once per load, never per step."""
        D = self.width
        sd = {k: v.float() for k, v in self.plain_state().items()}
        pe = torch.zeros(D, K_PAD, dtype=torch.float32, device=sd["cls_token"].device)
        pe[:, :K_PATCH] = sd["patch_embed.proj.weight"].reshape(D, K_PATCH)
        self._op_pe = pe.to(BF16).contiguous()
        for i in range(self.depth):
            f = fold_block(sd, i)
            for nm in ("qkv", "proj", "fc1", "fc2"):
                setattr(self, f"_op_{i}_{nm}_w", f[nm + ".w"].to(BF16).contiguous())
                setattr(self, f"_op_{i}_{nm}_b", f[nm + ".b"].float().contiguous())
        self._pos_cache = {}

    def load_dinov2_state_dict(self, sd: Dict[str, torch.Tensor]) -> "DinoV2Features":
        """Accepts the hub checkpoint's names (see :func:`to_plain_keys`) or the plain scheme of :func:`plain_keys`; `depth=`
        smaller than the checkpoint's takes the first blocks.  Any other mismatch raises with the lists of missing / unexpected
        keys and wrong shapes.  `pos_embed` may have any square pretraining grid."""
        got = to_plain_keys(sd)
        want = plain_keys(self.depth)
        deeper = {k for k in got if k.startswith("blocks.") and k.split(".")[1].isdigit() and int(k.split(".")[1]) >= self.depth}
        missing = [k for k in want if k not in got]
        unexpected = [k for k in got if k not in want and k not in deeper]
        bad = []
        for k in want:
            if k in got and k != "pos_embed" and tuple(got[k].shape) != tuple(self._shapes[k]):
                bad.append(f"{k} {tuple(got[k].shape)} (want {tuple(self._shapes[k])})")
        if "pos_embed" in got:
            pe = got["pos_embed"]
            n = pe.shape[1] - 1 if pe.dim() == 3 else -1
            if pe.dim() != 3 or pe.shape[0] != 1 or pe.shape[2] != self.width or n < 1 or int(round(math.sqrt(n))) ** 2 != n:
                bad.append(f"pos_embed {tuple(pe.shape)} (want [1, 1 + M*M, {self.width}])")
        if missing or unexpected or bad:
            raise KeyError(f"DinoV2Features.load_dinov2_state_dict: the state dict does not match DINOv2 {self.variant} (depth {self.depth}).\n"
                           f"  missing ({len(missing)}): {missing}\n  unexpected ({len(unexpected)}): {unexpected}\n"
                           f"  wrong shape ({len(bad)}): {bad}")
        with torch.no_grad():
            for k in want:
                if k == "pos_embed":
                    self.pos_embed = got[k].detach().to(self.cls_token.device, torch.float32).clone()
                else:
                    getattr(self, _bname(k)).copy_(got[k])
        self._pack()
        return self

    @classmethod
    def from_file(cls, path: str, variant: str, **kwargs) -> "DinoV2Features":
        """A DinoV2Features from a file written with torch.save(torch.hub.load('facebookresearch/dinov2', 'dinov2_<variant>')
        .state_dict(), path) (or the plain scheme)."""
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        return cls(variant, **kwargs).load_dinov2_state_dict(sd)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        pe = state_dict.get(prefix + "pos_embed")
        if pe is not None and pe.dim() == 3 and pe.shape[2] == self.width and tuple(pe.shape) != tuple(self.pos_embed.shape):
            self.pos_embed = torch.zeros(pe.shape, dtype=torch.float32, device=self.pos_embed.device)   # another pretraining grid
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._pack()

    def _pos_table(self, h: int, w: int) -> torch.Tensor:
        key = (h, w, str(self.pos_embed.device))
        tab = self._pos_cache.get(key)
        if tab is None:
            with torch.no_grad():
                tab = interpolate_pos_table(self.pos_embed.detach().cpu(), h, w, self.interpolate_offset, self.interpolate_antialias)
            tab = self._pos_cache[key] = tab.to(self.pos_embed.device)
        return tab

    # ---- forward ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def tokens(self, image: torch.Tensor) -> Tuple[torch.Tensor, Tuple[int, int, int]]:
        """([B*h*w, C] fp32 patch features, token-major; (B, h, w))."""
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[0] == 0:
            raise ValueError(f"DinoV2Features: image must be [B, 3, H, W], got {tuple(image.shape)}")
        ops._need_gpu(image)
        if image.device != self.cls_token.device:
            raise RuntimeError(f"DinoV2Features: image on {image.device}, weights on {self.cls_token.device}")
        with torch.cuda.device(image.device), torch.autocast("cuda", enabled=False):
            B = image.shape[0]
            h, w = self.size[0] // PATCH, self.size[1] // PATCH
            D, heads = self.width, self.heads
            rows = vf_prep(image.detach().float().contiguous(), h, w, self.imagenet_norm)
            pe = _linear(rows, self._op_pe, self.patch_embed_proj_bias)
            x = vit_tokens(pe, self.cls_token.reshape(-1), self._pos_table(h, w), B).view(B * (1 + h * w), D)
            N = 1 + h * w
            for i in range(self.depth):
                op = lambda nm: (getattr(self, f"_op_{i}_{nm}_w"), getattr(self, f"_op_{i}_{nm}_b"))
                qkv = _linear(layernorm_hat(x), *op("qkv"))
                o = attention_fwd(qkv.view(B, N, 3 * D), heads)
                x = _linear(o.view(B * N, D), *op("proj"), residual=x)
                hid = _linear(layernorm_hat(x), *op("fc1"), act=L.ACT_GELU)
                x = _linear(hid, *op("fc2"), residual=x)
            return layernorm_rows(x.view(B, N, D), self.norm_weight, self.norm_bias, 1), (B, h, w)

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        feat, (B, h, w) = self.tokens(image)
        return feat.view(B, h, w, self.width).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------
class _VFHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latent, feat, weight, bias, margin, grid):
        ops._need_gpu(latent, feat, weight, bias)
        B, h, w = grid
        lat = latent.detach().float().contiguous()
        _, D, Hl, Wl = lat.shape
        T, Cc = feat.shape
        ops._require(feat.dtype == torch.float32 and feat.is_contiguous() and T == B * h * w and lat.shape[0] == B, "VF head: feature / latent shapes")
        lib = L.load()
        dev = lat.device
        need_lat = ctx.needs_input_grad[0]
        need_w = weight is not None and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        wc = weight.detach().float().contiguous() if weight is not None else None
        bc = bias.detach().float().contiguous() if bias is not None else None
        part = torch.empty((lib.tv_vf_head_partial_count(T),), dtype=torch.float64, device=dev)
        out = torch.empty((3,), dtype=torch.float32, device=dev)
        dzr = torch.empty((T, D), dtype=torch.float32, device=dev)
        zr = torch.empty((T, D), dtype=torch.float32, device=dev) if need_w else None
        ab = torch.empty((T, 2), dtype=torch.float32, device=dev) if need_w else None
        import ctypes as C
        with torch.cuda.device(dev):
            L.check(lib.tv_vf_head(ops._p(lat), ops._p(feat), ops._p(wc), ops._p(bc), ops._p(part), ops._p(out), ops._p(dzr), ops._p(zr), ops._p(ab),
                                   B, D, Hl, Wl, h, w, Cc, float(margin), ops._stream()), "tv_vf_head")
            gate = C.c_void_p(out.data_ptr() + 4)
            dlat = dw = db = None
            if need_lat:
                dlat = torch.empty_like(lat)
                L.check(lib.tv_bilinear_nchw_bwd(ops._p(dzr), gate, ops._p(dlat), B, D, Hl, Wl, h, w, ops._stream()), "tv_bilinear_nchw_bwd")
            if need_w:
                n = lib.tv_vf_head_dproj_partial_count(T, Cc, D)
                wpart = torch.empty((n,), dtype=torch.float32, device=dev)
                dw = torch.empty_like(wc)
                db = torch.empty_like(bc)
                L.check(lib.tv_vf_head_dproj(ops._p(feat), ops._p(zr), ops._p(ab), ops._p(wc), ops._p(bc), gate, ops._p(wpart), ops._p(dw), ops._p(db),
                                             T, Cc, D, ops._stream()), "tv_vf_head_dproj")
        ctx.save_for_backward(dlat, dw, db)
        ctx.in_dtype = latent.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        dlat, dw, db = ctx.saved_tensors
        return ((dlat * g).to(ctx.in_dtype) if dlat is not None else None, None, dw * g if dw is not None else None,
                db * g if db is not None else None, None, None)


class VFLoss(nn.Module):
    """R/transvae/losses/vae_loss.py:119-196 with the projection created at construction (`proj.weight`, `proj.bias`, when
    latent_dim != feature_dim): an ordinary parameter -- the reference creates it lazily after its optimizer exists and so never
    trains it; here the caller decides.  `temperature` is stored and unused, as in the reference.

        forward(latent, features)                          features: [B, C, h, w] fp32 (a DinoV2Features output)
        forward(reconstruction, target, latent, dinov2)    the reference's signature; dinov2: a DinoV2Features
    """

    def __init__(self, latent_dim: int, feature_dim: int, margin: float = 0.4, temperature: float = 0.07):
        super().__init__()
        self.latent_dim, self.feature_dim = int(latent_dim), int(feature_dim)
        self.margin, self.temperature = margin, temperature
        self.proj = nn.Linear(self.latent_dim, self.feature_dim) if self.latent_dim != self.feature_dim else None

    def forward(self, *args):
        if len(args) == 2:
            latent, features = args
        elif len(args) == 4:
            _, target, latent, dinov2 = args
            if not isinstance(dinov2, DinoV2Features):
                raise ValueError("VFLoss (HIP path): the VF term runs with a transvae.DinoV2Features extractor")
            features = dinov2(target)
        else:
            raise TypeError("VFLoss.forward(latent, features) or VFLoss.forward(reconstruction, target, latent, dinov2)")
        if latent.dim() != 4 or features.dim() != 4 or latent.shape[0] != features.shape[0]:
            raise ValueError(f"VFLoss: latent [B, D, Hl, Wl] and features [B, C, h, w] expected, got {tuple(latent.shape)} and {tuple(features.shape)}")
        if latent.shape[1] != self.latent_dim or features.shape[1] != self.feature_dim:
            raise ValueError(f"VFLoss: built for latent_dim={self.latent_dim}, feature_dim={self.feature_dim}; got {latent.shape[1]} and "
                             f"{features.shape[1]} channels")
        if features.requires_grad:
            raise ValueError("VFLoss: differentiable w.r.t. the latent (and proj) only; pass features.detach()")
        ops._need_gpu(latent, features)
        B, Cc, h, w = features.shape
        tok = features.detach().permute(0, 2, 3, 1)          # the extractor's own token-major layout: no copy
        tok = tok.float().contiguous().view(B * h * w, Cc)
        with torch.autocast("cuda", enabled=False):
            if self.proj is None:
                return _VFHeadFn.apply(latent, tok, None, None, self.margin, (B, h, w))
            return _VFHeadFn.apply(latent, tok, self.proj.weight, self.proj.bias, self.margin, (B, h, w))
