"""Latent diffusion transformer on the HIP path: adaLN-Zero DiT blocks trained by flow matching on `extract_latents` shards.

The reference names the stage only (`train_dit.py` / `evaluate_dit.py`, both TODO); the protocol here is this package's own
(DESIGN.md section 3.4).  What runs where:

    token GEMMs        patch embedding, qkv, proj, fc1 + GELU, fc2, final linear     `ops.linear` (tv_igemm_nt / tv_wgrad_tn)
    attention          2-D RoPE in place, flash attention, head_dim 64 or 72         `ops.attention`
    conditioning rows  adaLN (LayerNorm-hat, 1 + scale, shift), gate + residual      `adaln` / `gate_residual` (csrc/dit.hip)
    flow-matching edge x_t rows from latents, loss + gradient, Euler step            `flow_rows` / `flow_loss` / `flow_euler`
    the recipe         loss with the cosine term, Heun corrector     `flow_loss_cos` / `flow_heun`
    conditioning path  timestep sinusoid + MLP, label embedding, SiLU, the adaLN_modulation linears: B rows, 1/N of the token
                       work, plain fp32 torch under autograd

`DiT` keeps fp32 master weights under the public DiT state-dict names; `flow_matching_loss` computes the loss and runs the backward;
`sample_latents` / `sample_images` integrate the velocity field with Euler or Heun steps on an optionally shifted time grid, with
classifier-free guidance inside an interval of t; `fit_dit` streams the
shards with `FusedAdamW`.  There is no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .hip import _lib as L
from .hip import ops
from .modules.attention import RoPE2D
from .optim import FusedAdamW, ParamEMA
from .probe import _Shards, _round_up, _stat_vectors

LN_EPS = 1e-6
TIME_SCALE = 1000.0          # t in [0, 1] enters the sinusoid as 1000 t (the public embedder's range)
PRESETS = {"DiT-S": (384, 12), "DiT-B": (768, 12), "DiT-L": (1024, 24)}
Stats = Union[Dict[str, torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]


# ---------------------------------------------------------------------------------------------------------------------------
# kernels 1-4 under autograd
# ---------------------------------------------------------------------------------------------------------------------------
class ModGrad:
    """The [B, ld] gradient of one modulation matrix, filled range by range by the backwards of the functions that read it.

    The function called with `owner=True` must be the FIRST reader in forward order, so that its backward runs last: it hands the
    buffer to autograd as the gradient of `mod` after checking that all `expected` column ranges were written."""

    def __init__(self, expected: int):
        self.expected, self.filled, self.buf = int(expected), 0, None

    def buffer(self, mod: torch.Tensor) -> torch.Tensor:
        if self.buf is None:
            self.buf = torch.empty_like(mod)
        return self.buf

    def take(self) -> torch.Tensor:
        if self.filled != self.expected:
            raise RuntimeError(f"transvae.dit: {self.filled} of {self.expected} column ranges of the modulation gradient were written")
        buf, self.buf, self.filled = self.buf, None, 0
        return buf


def _check_rows(x: torch.Tensor, mod: torch.Tensor, N: int, what: str):
    ops._need_gpu(x, mod)
    ops._require(x.dtype == torch.bfloat16 and x.dim() == 2 and x.is_contiguous(), f"{what}: contiguous bf16 rows [B N, C]")
    ops._require(mod.dtype == torch.float32 and mod.dim() == 2 and mod.is_contiguous() and mod.device == x.device,
                 f"{what}: contiguous fp32 modulation [B, ld] on the rows' device")
    ops._require(N > 0 and x.shape[0] == mod.shape[0] * N, f"{what}: {x.shape[0]} rows are not {mod.shape[0]} samples of {N}")


class _AdaLNFn(torch.autograd.Function):
    """`adaln` (w = None: the LayerNorm entry points, no weight gradient) and `lightning_dit.adaln_rms` (the RMSNorm's fp32 weight)."""

    @staticmethod
    def forward(ctx, x, w, mod, shift_off, scale_off, N, eps, sink, owner):
        B, ld = mod.shape
        lib = L.load()
        y = torch.empty_like(x)
        tail = (ops._p(mod), shift_off, scale_off, ld, ops._p(y), B, N, x.shape[1], eps, ops._stream())
        if w is None:
            L.check(lib.tv_adaln_fwd(ops._p(x), *tail), "tv_adaln_fwd")
        else:
            L.check(lib.tv_adaln_rms_fwd(ops._p(x), ops._p(w), *tail), "tv_adaln_rms_fwd")
        ctx.args = (shift_off, scale_off, N, eps, sink, owner)
        ctx.save_for_backward(x, w, mod)
        return y, x            # the second output is the residual stream itself: its gradient comes back as `dres`

    @staticmethod
    def backward(ctx, gy, gres):
        x, w, mod = ctx.saved_tensors
        shift_off, scale_off, N, eps, sink, owner = ctx.args
        what = "adaln" if w is None else "adaln_rms"
        B, ld = mod.shape
        C = x.shape[1]
        lib = L.load()
        gy = gy.contiguous()
        if gres is not None:
            gres = gres.contiguous()
            ops._require(gres.dtype == torch.bfloat16, f"{what}: the residual stream's gradient must be bf16")
        ops._require(gy.dtype == torch.bfloat16, f"{what}: bf16 gradient rows")
        dx = torch.empty_like(x)
        dw = None if w is None else torch.empty_like(w)
        dmod = sink.buffer(mod) if sink is not None else torch.zeros_like(mod)
        count = lib.tv_adaln_bwd_partial_count if w is None else lib.tv_adaln_rms_bwd_partial_count
        part = torch.empty(count(B, N, C), dtype=torch.float32, device=x.device)
        head = (ops._p(mod), shift_off, scale_off, ld, ops._p(gy), ops._p(gres), ops._p(dx), ops._p(dmod))
        tail = (ops._p(part), B, N, C, eps, ops._stream())
        if w is None:
            L.check(lib.tv_adaln_bwd(ops._p(x), *head, *tail), "tv_adaln_bwd")
        else:
            L.check(lib.tv_adaln_rms_bwd(ops._p(x), ops._p(w), *head, ops._p(dw), *tail), "tv_adaln_rms_bwd")
        if sink is not None:
            sink.filled += 2
            dmod = sink.take() if owner else None
        return dx, dw, dmod, None, None, None, None, None, None


class _GateResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mod, gate_off, N, sink):
        _check_rows(x, mod, N, "gate_residual")
        ops._require(y.shape == x.shape and y.dtype == torch.bfloat16 and y.is_contiguous(), "gate_residual: y must match x")
        B, ld = mod.shape
        out = torch.empty_like(x)
        L.check(L.load().tv_gate_residual_fwd(ops._p(x), ops._p(y), ops._p(mod), gate_off, ld, ops._p(out), B, N, x.shape[1], ops._stream()),
                "tv_gate_residual_fwd")
        ctx.args = (gate_off, N, sink)
        ctx.save_for_backward(y, mod)
        return out

    @staticmethod
    def backward(ctx, gout):
        y, mod = ctx.saved_tensors
        gate_off, N, sink = ctx.args
        B, ld = mod.shape
        C = y.shape[1]
        lib = L.load()
        gout = gout.contiguous()
        ops._require(gout.dtype == torch.bfloat16, "gate_residual: bf16 gradient rows")
        dy = torch.empty_like(y)
        dmod = sink.buffer(mod) if sink is not None else torch.zeros_like(mod)
        part = torch.empty(lib.tv_gate_residual_bwd_partial_count(B, N, C), dtype=torch.float32, device=y.device)
        L.check(lib.tv_gate_residual_bwd(ops._p(gout), ops._p(y), ops._p(mod), gate_off, ld, ops._p(dy), ops._p(dmod), ops._p(part), B, N, C,
                                         ops._stream()), "tv_gate_residual_bwd")
        if sink is not None:
            sink.filled += 1
            dmod = None
        return gout, dy, dmod, None, None, None


def adaln(x: torch.Tensor, mod: torch.Tensor, shift_off: int, scale_off: int, tokens: int, eps: float = LN_EPS,
          sink: Optional[ModGrad] = None, owner: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(LN-hat(x) (1 + scale) + shift, x): bf16 rows [B tokens, C]; shift / scale are C columns of the fp32 `mod` [B, ld] from the
    given offsets.  The second result IS x; feed it to `gate_residual` so that the residual stream's gradient joins the LayerNorm
    backward in fp32 inside the kernel.  Without a `sink` the backward returns a full gradient of `mod` with its two ranges filled."""
    _check_rows(x, mod, int(tokens), "adaln")
    return _AdaLNFn.apply(x, None, mod, int(shift_off), int(scale_off), int(tokens), float(eps), sink, bool(owner))


def gate_residual(x: torch.Tensor, y: torch.Tensor, mod: torch.Tensor, gate_off: int, tokens: int, sink: Optional[ModGrad] = None) -> torch.Tensor:
    """x + gate y on bf16 rows, gate = C columns of `mod` from `gate_off`.  The gradient of x is the incoming gradient itself."""
    return _GateResidualFn.apply(x, y, mod, int(gate_off), int(tokens), sink)


# ---------------------------------------------------------------------------------------------------------------------------
# kernels 5-7
# ---------------------------------------------------------------------------------------------------------------------------
def _latent_view(latents: torch.Tensor, what: str) -> torch.Tensor:
    ops._need_gpu(latents)
    ops._require(latents.dim() == 4 and latents.dtype == torch.float32, f"{what}: fp32 latents [B, D, h, w]")
    B, D, h, w = latents.shape
    x = latents
    if not (x.stride(3) == 1 and x.stride(2) == w and x.stride(1) >= h * w and x.stride(0) >= (D - 1) * x.stride(1) + h * w):
        x = x.contiguous()
    return x


def _dense(t: torch.Tensor, like: torch.Tensor, what: str) -> torch.Tensor:
    ops._need_gpu(t)
    ops._require(t.dtype == torch.float32 and tuple(t.shape) == tuple(like.shape) and t.device == like.device, f"{what}: fp32 of the latents' shape")
    return t.contiguous()


def flow_rows(latents: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, patch_size: int, noise: Optional[torch.Tensor] = None,
              t: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 patch rows [B N, ld] of x_t = t x + (1 - t) e with x = (latents - mean) rstd; without noise, of x itself.  Columns
    (py, px, c), ld = p p D rounded up to a multiple of 32, pad columns 0.  `mean` / `rstd` are fp32 [D] on the device."""
    x = _latent_view(latents, "flow_rows")
    B, D, h, w = x.shape
    p = int(patch_size)
    ld = _round_up(p * p * D, 32)
    rows_n = B * (h // p) * (w // p)
    with torch.cuda.device(x.device):
        if noise is not None:
            noise = _dense(noise, x, "flow_rows: noise")
            ops._require(t is not None and t.dtype == torch.float32 and t.numel() == B and t.is_contiguous() and t.device == x.device,
                         "flow_rows: t must be contiguous fp32 [B] on the latents' device")
        if out is None:
            out = torch.empty((rows_n, ld), dtype=torch.bfloat16, device=x.device)
        ops._require(out.dtype == torch.bfloat16 and tuple(out.shape) == (rows_n, ld) and out.is_contiguous(), "flow_rows: out must be bf16 [B N, ld]")
        L.check(L.load().tv_flow_rows(ops._p(x), x.stride(0), x.stride(1), ops._p(mean), ops._p(rstd), ops._p(noise), ops._p(t), ops._p(out),
                                      B, D, h, w, p, ld, ops._stream()), "tv_flow_rows")
    return out


def flow_loss(pred: torch.Tensor, latents: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, noise: torch.Tensor, patch_size: int,
              grad_scale: float = 1.0, want_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(fp64 [2] = {sum, mean} of (pred - (x - e))^2 over the real columns, bf16 gradient of the mean times `grad_scale` | None)."""
    x = _latent_view(latents, "flow_loss")
    B, D, h, w = x.shape
    p = int(patch_size)
    ld = _round_up(p * p * D, 32)
    ops._need_gpu(pred)
    ops._require(pred.dtype == torch.bfloat16 and tuple(pred.shape) == (B * (h // p) * (w // p), ld) and pred.is_contiguous(),
                 "flow_loss: pred must be contiguous bf16 [B N, ld]")
    noise = _dense(noise, x, "flow_loss: noise")
    lib = L.load()
    with torch.cuda.device(x.device):
        out = torch.empty(2, dtype=torch.float64, device=x.device)
        part = torch.empty(lib.tv_flow_loss_partial_count(B, D, h, w, p, ld), dtype=torch.float64, device=x.device)
        dpred = torch.empty_like(pred) if want_grad else None
        L.check(lib.tv_flow_loss(ops._p(pred), ops._p(x), x.stride(0), x.stride(1), ops._p(mean), ops._p(rstd), ops._p(noise), ops._p(dpred),
                                 ops._p(out), ops._p(part), B, D, h, w, p, ld, float(grad_scale), ops._stream()), "tv_flow_loss")
    return out, dpred


def flow_euler(x: torch.Tensor, v: torch.Tensor, patch_size: int, dt: float, cfg_scale: Optional[float] = None) -> torch.Tensor:
    """In place on dense fp32 x [B, D, h, w]: x += dt v, v bf16 rows [B N, ld]; with `cfg_scale` s, v has 2 B N rows (conditional
    half first) and the step uses v_u + s (v_c - v_u)."""
    ops._need_gpu(x, v)
    ops._require(x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(), "flow_euler: dense fp32 x [B, D, h, w]")
    B, D, h, w = x.shape
    p = int(patch_size)
    ld = _round_up(p * p * D, 32)
    guided = cfg_scale is not None
    ops._require(v.dtype == torch.bfloat16 and v.is_contiguous() and v.device == x.device and
                 tuple(v.shape) == ((2 if guided else 1) * B * (h // p) * (w // p), ld), "flow_euler: v must be contiguous bf16 [(2) B N, ld]")
    with torch.cuda.device(x.device):
        L.check(L.load().tv_flow_euler(ops._p(x), ops._p(v), B, D, h, w, p, ld, float(dt), float(cfg_scale or 0.0), int(guided), ops._stream()),
                "tv_flow_euler")
    return x


def flow_loss_cos(pred: torch.Tensor, latents: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, noise: torch.Tensor, patch_size: int,
                  cos_weight: float, grad_scale: float = 1.0, want_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """`flow_loss` with the per-position cosine term: (fp64 [5] = {mse sum, mse mean, sum and mean over the
    B h w latent pixels of 1 - cos(pred, x - e), mse mean + cos_weight cos mean}, bf16 gradient of the last times `grad_scale` | None)."""
    if not (math.isfinite(float(cos_weight)) and float(cos_weight) >= 0.0):
        raise ValueError(f"flow_loss_cos: cos_weight={cos_weight!r} must be finite and not negative")
    x = _latent_view(latents, "flow_loss_cos")
    B, D, h, w = x.shape
    p = int(patch_size)
    ld = _round_up(p * p * D, 32)
    ops._need_gpu(pred)
    ops._require(pred.dtype == torch.bfloat16 and tuple(pred.shape) == (B * (h // p) * (w // p), ld) and pred.is_contiguous(),
                 "flow_loss_cos: pred must be contiguous bf16 [B N, ld]")
    noise = _dense(noise, x, "flow_loss_cos: noise")
    lib = L.load()
    with torch.cuda.device(x.device):
        out = torch.empty(5, dtype=torch.float64, device=x.device)
        part = torch.empty(lib.tv_flow_loss_cos_partial_count(B, D, h, w, p, ld), dtype=torch.float64, device=x.device)
        dpred = torch.empty_like(pred) if want_grad else None
        L.check(lib.tv_flow_loss_cos(ops._p(pred), ops._p(x), x.stride(0), x.stride(1), ops._p(mean), ops._p(rstd), ops._p(noise), ops._p(dpred),
                                     ops._p(out), ops._p(part), B, D, h, w, p, ld, float(cos_weight), float(grad_scale), ops._stream()),
                "tv_flow_loss_cos")
    return out, dpred


def flow_heun(x: torch.Tensor, v1: torch.Tensor, v2: torch.Tensor, patch_size: int, dt: float, cfg_scale: float = 1.0, guided1: bool = False,
              guided2: bool = False) -> torch.Tensor:
    """The corrector of a Heun step, in place on dense fp32 x [B, D, h, w] that holds the predictor's x + dt g1: x += dt / 2 (g2 - g1).
    g_k is read from bf16 rows v_k [B N, ld]; with `guided_k`, v_k has 2 B N rows (conditional half first) and
    g_k = v_u + cfg_scale (v_c - v_u), as in `flow_euler`."""
    ops._need_gpu(x, v1, v2)
    ops._require(x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(), "flow_heun: dense fp32 x [B, D, h, w]")
    B, D, h, w = x.shape
    p = int(patch_size)
    ld = _round_up(p * p * D, 32)
    for v, guided, what in ((v1, guided1, "v1"), (v2, guided2, "v2")):
        ops._require(v.dtype == torch.bfloat16 and v.is_contiguous() and v.device == x.device and
                     tuple(v.shape) == ((2 if guided else 1) * B * (h // p) * (w // p), ld), f"flow_heun: {what} must be contiguous bf16 [(2) B N, ld]")
    with torch.cuda.device(x.device):
        L.check(L.load().tv_flow_heun(ops._p(x), ops._p(v1), ops._p(v2), B, D, h, w, p, ld, float(dt), float(cfg_scale), int(bool(guided1)),
                                      int(bool(guided2)), ops._stream()), "tv_flow_heun")
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def timestep_embedding(t: torch.Tensor, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    """The public sinusoid: cat(cos(t f), sin(t f)), f_i = max_period^(-i / half), fp32 [B, dim]."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
    args = t.float()[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


class _Embedder(nn.Module):
    def __init__(self, hidden: int, freq: int):
        super().__init__()
        self.frequency_embedding_size = freq
        self.mlp = nn.Sequential(nn.Linear(freq, hidden), nn.SiLU(), nn.Linear(hidden, hidden))

    def forward(self, t):
        return self.mlp(timestep_embedding(t * TIME_SCALE, self.frequency_embedding_size))


class _Labels(nn.Module):
    def __init__(self, num_classes: int, hidden: int):
        super().__init__()
        self.embedding_table = nn.Embedding(num_classes + 1, hidden)      # the last row is the null class


class _Patches(nn.Module):
    def __init__(self, in_channels: int, hidden: int, patch: int):
        super().__init__()
        self.proj = nn.Conv2d(in_channels, hidden, patch, patch)          # parameters only; applied as a GEMM on patch rows


class _Attn(nn.Module):
    def __init__(self, hidden: int):
        super().__init__()
        self.qkv = nn.Linear(hidden, 3 * hidden)
        self.proj = nn.Linear(hidden, hidden)


class _Mlp(nn.Module):
    def __init__(self, hidden: int, inner: int):
        super().__init__()
        self.fc1 = nn.Linear(hidden, inner)
        self.fc2 = nn.Linear(inner, hidden)


class DiTBlock(nn.Module):
    def __init__(self, hidden: int, mlp_ratio: float):
        super().__init__()
        self.attn = _Attn(hidden)
        self.mlp = _Mlp(hidden, int(hidden * mlp_ratio))
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden, 6 * hidden))


class _Final(nn.Module):
    def __init__(self, hidden: int, out_cols: int):
        super().__init__()
        self.linear = nn.Linear(hidden, out_cols)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden, 2 * hidden))


def _grid_of(input_size) -> Tuple[int, int]:
    if isinstance(input_size, int):
        return int(input_size), int(input_size)
    if isinstance(input_size, Sequence) and len(input_size) == 2:
        return int(input_size[0]), int(input_size[1])
    raise ValueError(f"DiT: input_size={input_size!r} must be an int or (h, w)")


class DiT(nn.Module):
    """adaLN-Zero diffusion transformer on latents [B, in_channels, h, w].

    forward(x, t, y): x bf16 patch rows [B N, ld] (what `flow_rows` returns) or fp32 latents [B, D, h, w], already normalised;
    t fp32 [B] in [0, 1]; y int64 [B] in [0, num_classes], num_classes being the null class.  Returns bf16 velocity rows [B N, ld]
    with the columns of `flow_rows`; the pad columns are exactly 0."""

    def __init__(self, input_size=16, patch_size: int = 1, in_channels: int = 32, hidden_size: int = 768, depth: int = 12,
                 num_classes: int = 1000, mlp_ratio: float = 4.0, class_dropout_prob: float = 0.1, use_rope: bool = True,
                 frequency_embedding_size: int = 256, generator: Optional[torch.Generator] = None, head_dim: int = 64):
        super().__init__()
        h, w = _grid_of(input_size)
        if patch_size not in (1, 2):
            raise ValueError(f"DiT: patch_size={patch_size} must be 1 or 2")
        if h < 1 or w < 1 or h % patch_size or w % patch_size:
            raise ValueError(f"DiT: input_size={(h, w)} is not divisible by patch_size={patch_size}")
        if head_dim not in (64, 72):
            raise ValueError(f"DiT: head_dim={head_dim} must be 64 or 72, the head dimensions of the attention kernels")
        if hidden_size < head_dim or hidden_size % head_dim:
            raise ValueError(f"DiT: hidden_size={hidden_size} must be a multiple of head_dim = {head_dim}")
        if not use_rope:
            raise ValueError("DiT: use_rope=False is not supported: positions are 2-D RoPE only, there is no absolute position table")
        if in_channels < 1 or depth < 1 or num_classes < 1:
            raise ValueError(f"DiT: in_channels={in_channels}, depth={depth} and num_classes={num_classes} must be positive")
        if not 0.0 <= class_dropout_prob < 1.0:
            raise ValueError(f"DiT: class_dropout_prob={class_dropout_prob} must be in [0, 1)")
        inner = int(hidden_size * mlp_ratio)
        if inner < 32 or inner % 32:
            raise ValueError(f"DiT: mlp_ratio={mlp_ratio} gives an inner width {inner} that is no multiple of 32")
        self.input_size, self.patch_size, self.in_channels = (h, w), int(patch_size), int(in_channels)
        self.hidden_size, self.depth, self.num_classes = int(hidden_size), int(depth), int(num_classes)
        self.head_dim, self.attn_scale = int(head_dim), float(head_dim) ** -0.5          # (0.125 exactly at 64)
        self.num_heads, self.class_dropout_prob, self.use_rope = hidden_size // head_dim, float(class_dropout_prob), True
        self.grid = (h // patch_size, w // patch_size)
        self.tokens = self.grid[0] * self.grid[1]
        self.patch_cols = patch_size * patch_size * in_channels
        self.ld = _round_up(self.patch_cols, 32)
        self.x_embedder = _Patches(in_channels, hidden_size, patch_size)
        self.t_embedder = _Embedder(hidden_size, frequency_embedding_size)
        self.y_embedder = _Labels(num_classes, hidden_size)
        self.blocks = nn.ModuleList([DiTBlock(hidden_size, mlp_ratio) for _ in range(depth)])
        self.final_layer = _Final(hidden_size, self.patch_cols)
        object.__setattr__(self, "_rope", RoPE2D(head_dim))          # a table builder, kept out of the state dict
        self.initialize_weights(generator)

    def _apply(self, fn, *a, **k):
        self._rope._apply(fn)
        return super()._apply(fn, *a, **k)

    @torch.no_grad()
    def initialize_weights(self, generator: Optional[torch.Generator] = None):
        """The public initialisation: Xavier-uniform linears with zero bias, N(0, 0.02^2) embedders, zeros for every
        adaLN_modulation.1 and for final_layer.linear."""
        gen = generator if generator is not None else torch.Generator().manual_seed(0)

        def xavier(w: torch.Tensor):
            fan_out, fan_in = w.shape[0], w[0].numel()
            a = math.sqrt(6.0 / (fan_in + fan_out))
            w.copy_((torch.rand(w.shape, generator=gen) * 2 - 1) * a)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                xavier(m.weight)
                m.bias.zero_()
        xavier(self.x_embedder.proj.weight)
        self.x_embedder.proj.bias.zero_()
        self.y_embedder.embedding_table.weight.copy_(torch.randn(self.y_embedder.embedding_table.weight.shape, generator=gen) * 0.02)
        for lin in (self.t_embedder.mlp[0], self.t_embedder.mlp[2]):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * 0.02)
        for blk in self.blocks:
            blk.adaLN_modulation[1].weight.zero_()
            blk.adaLN_modulation[1].bias.zero_()
        self.final_layer.adaLN_modulation[1].weight.zero_()
        self.final_layer.adaLN_modulation[1].bias.zero_()
        self.final_layer.linear.weight.zero_()
        self.final_layer.linear.bias.zero_()

    def check_labels(self, y: torch.Tensor, what: str = "labels"):
        if y.dim() != 1 or y.dtype != torch.int64:
            raise ValueError(f"DiT: {what} must be int64 [B], got {tuple(y.shape)} {y.dtype}")
        if y.numel() and (int(y.min()) < 0 or int(y.max()) > self.num_classes):
            raise ValueError(f"DiT: {what} must lie in [0, {self.num_classes}] ({self.num_classes} is the null class): "
                             f"min {int(y.min())}, max {int(y.max())}")

    def check_latents(self, shape, what: str = "latents"):
        if len(shape) != 4 or shape[1] != self.in_channels or tuple(shape[2:]) != self.input_size:
            raise ValueError(f"DiT: {what} must be [B, {self.in_channels}, {self.input_size[0]}, {self.input_size[1]}], got {tuple(shape)}")

    def conditioning(self, t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """t_emb + y_emb, fp32 [B, C] (every adaLN_modulation applies its own SiLU)"""
        return self.t_embedder(t) + self.y_embedder.embedding_table(y)

    @ops.hip_entry
    def forward(self, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        ops._need_gpu(x, t, y)
        C, N, p = self.hidden_size, self.tokens, self.patch_size
        if x.dim() == 4:
            self.check_latents(x.shape, "x")
            zero = torch.zeros(self.in_channels, dtype=torch.float32, device=x.device)
            x = flow_rows(x, zero, torch.ones_like(zero), p)
        if x.dim() != 2 or x.shape[1] != self.ld or x.shape[0] % N or x.dtype != torch.bfloat16:
            raise ValueError(f"DiT: x must be bf16 rows [B {N}, {self.ld}] or fp32 latents, got {tuple(x.shape)} {x.dtype}")
        B = x.shape[0] // N
        if t.shape != (B,) or y.shape != (B,):
            raise ValueError(f"DiT: t and y must be [{B}], got {tuple(t.shape)} and {tuple(y.shape)}")
        c = self.conditioning(t.float(), y)
        we = self.x_embedder.proj.weight.permute(0, 2, 3, 1).reshape(C, self.patch_cols)
        wf, bf = self.final_layer.linear.weight, self.final_layer.linear.bias
        if self.ld != self.patch_cols:                       # zero pad: no input mass, pad outputs exactly 0, no gradient kept
            we = F.pad(we, (0, self.ld - self.patch_cols))
            wf = F.pad(wf, (0, 0, 0, self.ld - self.patch_cols))
            bf = F.pad(bf, (0, self.ld - self.patch_cols))
        h = ops.linear(x.contiguous(), we.contiguous(), self.x_embedder.proj.bias)
        tab = self._rope.table(*self.grid)
        for blk in self.blocks:
            mod = blk.adaLN_modulation(c).contiguous()
            sink = ModGrad(6) if mod.requires_grad else None
            a, hs = adaln(h, mod, 0, C, N, LN_EPS, sink, True)
            qkv = ops.linear(a, blk.attn.qkv.weight, blk.attn.qkv.bias)
            o = ops.attention(qkv.view(B, N, 3 * C), tab, self.num_heads, self.attn_scale, self.head_dim)
            a = ops.linear(o.view(B * N, C), blk.attn.proj.weight, blk.attn.proj.bias)
            h = gate_residual(hs, a, mod, 2 * C, N, sink)
            a, hs = adaln(h, mod, 3 * C, 4 * C, N, LN_EPS, sink, False)
            a = ops.linear(a, blk.mlp.fc1.weight, blk.mlp.fc1.bias, act="gelu")
            a = ops.linear(a, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
            h = gate_residual(hs, a, mod, 5 * C, N, sink)
        mod = self.final_layer.adaLN_modulation(c).contiguous()
        a, _ = adaln(h, mod, 0, C, N, LN_EPS, ModGrad(2) if mod.requires_grad else None, True)
        return ops.linear(a, wf.contiguous(), bf.contiguous())


def state_dict_keys(depth: int) -> list:
    """The state-dict names of a `DiT` of `depth` blocks: the public DiT definition's, without its `pos_embed` buffer."""
    keys = ["x_embedder.proj", "t_embedder.mlp.0", "t_embedder.mlp.2"]
    for i in range(depth):
        keys += [f"blocks.{i}.attn.qkv", f"blocks.{i}.attn.proj", f"blocks.{i}.mlp.fc1", f"blocks.{i}.mlp.fc2", f"blocks.{i}.adaLN_modulation.1"]
    keys += ["final_layer.linear", "final_layer.adaLN_modulation.1"]
    out = [k + s for k in keys for s in (".weight", ".bias")]
    out.insert(6, "y_embedder.embedding_table.weight")
    return out


def create_dit(name: str = "DiT-B", input_size=16, patch_size: int = 1, in_channels: int = 32, num_classes: int = 1000, **kwargs) -> DiT:
    """`DiT-S` (384 wide, 12 deep), `DiT-B` (768, 12) or `DiT-L` (1024, 24), all at head_dim 64.  DiT-XL (1152 wide, 28 deep, 16 heads
    of 72) is `dit_xl`."""
    if name not in PRESETS:
        raise ValueError(f"create_dit: name={name!r} is not one of {sorted(PRESETS)}")
    hidden, depth = PRESETS[name]
    return DiT(input_size, patch_size, in_channels, hidden, depth, num_classes, **kwargs)


def dit_xl(input_size=16, patch_size: int = 1, in_channels: int = 32, num_classes: int = 1000, **kwargs) -> DiT:
    """DiT-XL: 1152 wide, 28 deep, 16 heads of head_dim 72 (the attention kernels of csrc/attention_hd.hip)."""
    return DiT(input_size, patch_size, in_channels, 1152, 28, num_classes, head_dim=72, **kwargs)


# ---------------------------------------------------------------------------------------------------------------------------
# training and sampling
# ---------------------------------------------------------------------------------------------------------------------------
def _check_stats(stats: Stats, D: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, std) of `stats` (the latents_stats.pt dict or a pair), checked on the host side of the call"""
    if isinstance(stats, dict) and "mean" in stats and "std" in stats:
        mean, std = stats["mean"], stats["std"]
    elif isinstance(stats, (tuple, list)) and len(stats) == 2:
        mean, std = stats
    else:
        raise ValueError("stats must be the latents_stats.pt dict or a (mean, std) pair")
    if mean.numel() != D or std.numel() != D:
        raise ValueError(f"stats of {mean.numel()} channels for latents of {D}")
    return mean, std


def _stats_of(stats: Stats, D: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(mean [D], rstd [D], mean, std) fp32 on `device`"""
    mean, std = _check_stats(stats, D)
    m, r = _stat_vectors(mean, std, device)
    return m, r, m, std.detach().reshape(-1).to(device=device, dtype=torch.float32)


def _take_mu(dit: DiT, latents: torch.Tensor) -> torch.Tensor:
    if latents.dim() == 4 and latents.shape[1] == 2 * dit.in_channels:        # a moments shard: the mu half, in place
        latents = latents[:, :dit.in_channels]
    dit.check_latents(latents.shape)
    return latents


def draw_t(B: int, t_sampling: str, generator: Optional[torch.Generator], device) -> torch.Tensor:
    if t_sampling == "uniform":
        return torch.rand(B, generator=generator, device=device)
    if t_sampling == "lognorm":
        return torch.sigmoid(torch.randn(B, generator=generator, device=device))
    raise ValueError(f"t_sampling={t_sampling!r} must be 'uniform' or 'lognorm'")


def _check_cosine_weight(cosine_weight: float):
    if not (math.isfinite(float(cosine_weight)) and float(cosine_weight) >= 0.0):
        raise ValueError(f"cosine_weight={cosine_weight!r} must be finite and not negative")


def flow_matching_loss(dit: DiT, latents: torch.Tensor, labels: torch.Tensor, stats: Stats, *, t: Optional[torch.Tensor] = None,
                       noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, t_sampling: str = "lognorm",
                       grad_scale: float = 1.0, check_labels: bool = True, cosine_weight: float = 0.0) -> torch.Tensor:
    """One flow-matching step's loss, and its backward when gradients are enabled.

    x = (latents - mean) / std with `stats`, e = `noise` or N(0, I), t = `t` or drawn by `t_sampling`; the model sees the rows of
    t x + (1 - t) e and the loss is the mean of (v_pred - (x - e))^2 over the real columns.  In training mode each label is
    replaced by the null class with `dit.class_dropout_prob`.  Everything random is drawn with `generator` on the latents' device.
    With `cosine_weight` > 0 the loss is that mean plus `cosine_weight` times the mean over the latent pixels of
    1 - cos(v_pred, x - e) across the channels (`flow_loss_cos`); at 0.0 the term does not exist.
    Returns the loss as an fp64 device scalar (no synchronisation); the parameters' `.grad` hold `grad_scale` times its gradient."""
    if t_sampling not in ("uniform", "lognorm"):
        raise ValueError(f"t_sampling={t_sampling!r} must be 'uniform' or 'lognorm'")
    _check_cosine_weight(cosine_weight)
    latents = _take_mu(dit, latents)
    if check_labels:
        dit.check_labels(labels)
    _check_stats(stats, dit.in_channels)
    ops._need_gpu(latents, labels)
    dev = latents.device
    B = latents.shape[0]
    with torch.cuda.device(dev), torch.autocast("cuda", enabled=False):
        mean, rstd, _, _ = _stats_of(stats, dit.in_channels, dev)
        if t is None:
            t = draw_t(B, t_sampling, generator, dev)
        if noise is None:
            noise = torch.randn((B, dit.in_channels) + dit.input_size, generator=generator, device=dev)
        t = t.to(device=dev, dtype=torch.float32).contiguous()
        y = labels
        if dit.training and dit.class_dropout_prob > 0:
            drop = torch.rand(B, generator=generator, device=dev) < dit.class_dropout_prob
            y = torch.where(drop, torch.full_like(y, dit.num_classes), y)
        rows = flow_rows(latents, mean, rstd, dit.patch_size, noise, t)
        train = torch.is_grad_enabled()
        pred = dit(rows, t, y)
        if float(cosine_weight) > 0.0:
            out, dpred = flow_loss_cos(pred.detach(), latents, mean, rstd, noise, dit.patch_size, cosine_weight, grad_scale, train)
        else:
            out, dpred = flow_loss(pred.detach(), latents, mean, rstd, noise, dit.patch_size, grad_scale, train)
        if train:
            pred.backward(dpred)
    return out[4] if float(cosine_weight) > 0.0 else out[1]


SAMPLE_METHODS = ("euler", "heun")


def time_grid(steps: int, timestep_shift: float = 1.0) -> list:
    """The `steps + 1` times of the sampler, t = 0 (noise) to t = 1, as Python floats (float64): u_i = i / steps and
    t_i = s u_i / (1 + (s - 1) u_i); s < 1 spends more steps near the noise, s = 1 is the equal grid i (1 / steps) that ends at 1.0."""
    steps, s = int(steps), float(timestep_shift)
    if steps < 1:
        raise ValueError(f"sample_latents: steps={steps} must be positive")
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"sample_latents: timestep_shift={timestep_shift!r} must be positive")
    if s == 1.0:
        dt = 1.0 / steps
        return [i * dt for i in range(steps)] + [1.0]
    grid = [s * (i / steps) / (1.0 + (s - 1.0) * (i / steps)) for i in range(steps)]
    return grid + [1.0]


def _check_sampler(method: str, timestep_shift: float, cfg_interval) -> Tuple[float, float]:
    if method not in SAMPLE_METHODS:
        raise ValueError(f"sample_latents: method={method!r} must be one of {SAMPLE_METHODS}")
    if not (math.isfinite(float(timestep_shift)) and float(timestep_shift) > 0.0):
        raise ValueError(f"sample_latents: timestep_shift={timestep_shift!r} must be positive")
    if not (isinstance(cfg_interval, (tuple, list)) and len(cfg_interval) == 2):
        raise ValueError(f"sample_latents: cfg_interval={cfg_interval!r} must be a (lo, hi) pair")
    lo, hi = float(cfg_interval[0]), float(cfg_interval[1])
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"sample_latents: cfg_interval={cfg_interval!r} must satisfy 0 <= lo <= hi <= 1")
    return lo, hi


@torch.no_grad()
def sample_latents(dit: DiT, labels: torch.Tensor, *, steps: int, cfg_scale: float = 1.0, generator: Optional[torch.Generator] = None,
                   stats: Stats, noise: Optional[torch.Tensor] = None, method: str = "euler", timestep_shift: float = 1.0,
                   cfg_interval: Tuple[float, float] = (0.0, 1.0)) -> torch.Tensor:
    """Integration of the velocity field from t = 0 (noise) to t = 1 in `steps` steps on `time_grid(steps, timestep_shift)`, then
    de-normalisation with `stats`: fp32 latents [B, D, h, w] for `vae.decode`.  An evaluation at time t is guided iff cfg_scale != 1
    and cfg_interval[0] <= t <= cfg_interval[1]: it runs as one batch of 2B (labels, then the null class) and gives
    v_null + cfg_scale (v_label - v_null); an unguided one runs the B labelled rows alone.  method="euler": one evaluation per step;
    "heun": the Euler predictor, a second evaluation at the step's end on its result, and `flow_heun`."""
    if int(steps) < 1:
        raise ValueError(f"sample_latents: steps={steps} must be positive")
    lo, hi = _check_sampler(method, timestep_shift, cfg_interval)
    dit.check_labels(labels)
    _check_stats(stats, dit.in_channels)
    ops._need_gpu(labels)
    dev = labels.device
    B, D, p = labels.shape[0], dit.in_channels, dit.patch_size
    was_training = dit.training
    dit.eval()
    with torch.cuda.device(dev), torch.autocast("cuda", enabled=False):
        _, _, mean, std = _stats_of(stats, D, dev)
        if noise is None:
            noise = torch.randn((B, D) + dit.input_size, generator=generator, device=dev)
        dit.check_latents(noise.shape, "noise")
        x = noise.to(device=dev, dtype=torch.float32).clone().contiguous()
        guided = float(cfg_scale) != 1.0
        zero, one = torch.zeros(D, device=dev), torch.ones(D, device=dev)
        T = B * dit.tokens
        rows = torch.empty(((2 if guided else 1) * T, dit.ld), dtype=torch.bfloat16, device=dev)
        y = torch.cat([labels, torch.full_like(labels, dit.num_classes)]) if guided else labels
        grid = time_grid(steps, timestep_shift)

        def velocity(tv: float):
            """(bf16 velocity rows of the model at x and time tv, whether they hold the null-class half)"""
            g = guided and lo <= tv <= hi
            flow_rows(x, zero, one, p, out=rows[:T])
            if g:
                flow_rows(x, zero, one, p, out=rows[T:])
            n = (2 if g else 1) * B
            t = torch.full((n,), tv, dtype=torch.float32, device=dev)
            return dit(rows[:n * dit.tokens], t, y[:n]), g

        equal_dt = 1.0 / int(steps) if float(timestep_shift) == 1.0 else None
        for i in range(int(steps)):
            dt = equal_dt if equal_dt is not None else grid[i + 1] - grid[i]
            v1, g1 = velocity(grid[i])
            flow_euler(x, v1, p, dt, float(cfg_scale) if g1 else None)
            if method == "heun":
                v2, g2 = velocity(grid[i + 1])
                flow_heun(x, v1, v2, p, dt, float(cfg_scale), g1, g2)
        x = x * std.view(1, D, 1, 1) + mean.view(1, D, 1, 1)
    dit.train(was_training)
    return x


@torch.no_grad()
def sample_images(vae: nn.Module, dit: DiT, labels: torch.Tensor, *, steps: int, cfg_scale: float = 1.0,
                  generator: Optional[torch.Generator] = None, stats: Stats, noise: Optional[torch.Tensor] = None, grid: bool = False,
                  nrow: int = 8, method: str = "euler", timestep_shift: float = 1.0,
                  cfg_interval: Tuple[float, float] = (0.0, 1.0)) -> torch.Tensor:
    """`sample_latents`, then `vae.decode`: the decoder's raw output [B, 3, H, W]; grid=True: the uint8 sheet of
    `to_uint8_grid(..., transform="sigmoid")`."""
    lat = sample_latents(dit, labels, steps=steps, cfg_scale=cfg_scale, generator=generator, stats=stats, noise=noise, method=method,
                         timestep_shift=timestep_shift, cfg_interval=cfg_interval)
    img = vae.decode(lat)
    if grid:
        from .image_io import to_uint8_grid
        return to_uint8_grid(img.float(), nrow=nrow, transform="sigmoid")
    return img


def fit_dit(train_dir, dit: DiT, *, epochs: int, batch_size: int, lr: float, weight_decay: float = 0.0, t_sampling: str = "lognorm",
            use_flip: bool = True, seed: int = 0, log_every: int = 50, device="cuda", ema_decay: Optional[float] = None,
            cosine_weight: float = 0.0) -> Dict:
    """Train `dit` by flow matching on an `extract_latents` directory (or a `(latents, labels)` pair with `stats` as a third item).

    Shards stream one at a time in an order drawn per epoch from a host generator seeded with `seed + 1`, with a permutation inside
    each shard; with `use_flip` and `latents_flip` in the shard every sample is its mirrored latent with probability 1/2, drawn by
    the same generator.  t, the noise and the label dropout come from a device generator seeded with `seed`.  `FusedAdamW`,
    constant learning rate; the loss is read back once per `log_every` steps (one host synchronisation each).
    With `ema_decay` a `ParamEMA` of the weights (equal to them at the start) is updated after every optimizer step and returned
    under "ema"; with None nothing is kept and there is no such key.  `cosine_weight` is `flow_matching_loss`'s.
    Returns {"loss" (mean of the last logging interval), "history" [{"step", "loss"}], "shard_orders", "steps", "optimizer"}."""
    if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
        raise ValueError(f"fit_dit: ema_decay={ema_decay!r} must be in [0, 1] or None")
    if epochs < 1 or batch_size < 1 or not lr > 0 or log_every < 1:
        raise ValueError("fit_dit: epochs, batch_size, lr and log_every must be positive")
    _check_cosine_weight(cosine_weight)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("transvae.hip: this op only runs on a HIP device (MI355X); there is no CPU fallback")
    stats = None
    if isinstance(train_dir, (tuple, list)) and len(train_dir) == 3:
        train_dir, stats = tuple(train_dir[:2]), train_dir[2]
    sh = _Shards(train_dir, dit.num_classes + 1, "train")          # the null class is a legal stored label
    if stats is None:
        stats = sh.stats
    if stats is None:
        raise ValueError(f"fit_dit: {train_dir} has no latents_stats.pt")
    _take_mu(dit, sh.load(0)["latents"])
    with torch.cuda.device(device):
        _stats_of(stats, dit.in_channels, device)
        dit.to(device).train()
        opt = FusedAdamW(dit.parameters(), lr=lr, weight_decay=weight_decay)
        ema = ParamEMA(dit.parameters(), decay=float(ema_decay), optimizer=opt) if ema_decay is not None else None
        order_gen = torch.Generator().manual_seed(int(seed) + 1)
        dev_gen = torch.Generator(device=device).manual_seed(int(seed))
        acc = torch.zeros((), dtype=torch.float64, device=device)
        step, pending, history, orders = 0, 0, [], []
        for _ in range(int(epochs)):
            order = torch.randperm(len(sh), generator=order_gen).tolist()
            orders.append(order)
            for k in order:
                shard = sh.load(k)
                n = shard["labels"].shape[0]
                perm = torch.randperm(n, generator=order_gen)
                flip = shard.get("latents_flip") if use_flip else None
                mirrored = (torch.rand(n, generator=order_gen) < 0.5) if flip is not None else None
                lat, lab = shard["latents"].to(device), shard["labels"].to(device)
                flip = flip.to(device) if flip is not None else None
                for i in range(0, n, batch_size):
                    idx = perm[i:i + batch_size].to(device)
                    x = lat[idx]
                    if flip is not None:
                        x = torch.where(mirrored[perm[i:i + batch_size]].to(device).view(-1, 1, 1, 1), flip[idx], x)
                    opt.zero_grad(set_to_none=True)
                    acc += flow_matching_loss(dit, x, lab[idx], stats, generator=dev_gen, t_sampling=t_sampling, check_labels=False,
                                              cosine_weight=cosine_weight)
                    opt.step()
                    if ema is not None:
                        ema.update()
                    step += 1
                    pending += 1
                    if pending == log_every:
                        history.append({"step": step, "loss": float(acc) / pending})       # the one synchronisation of the interval
                        acc.zero_()
                        pending = 0
                del lat, lab, flip
        if pending:
            history.append({"step": step, "loss": float(acc) / pending})
    out = {"loss": history[-1]["loss"], "history": history, "shard_orders": orders, "steps": step, "optimizer": opt}
    if ema is not None:
        out["ema"] = ema
    return out
