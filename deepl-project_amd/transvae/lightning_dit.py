"""The LightningDiT block on the HIP path: RMSNorm adaLN, per-head qk-norm and a SwiGLU MLP on top of `transvae.dit.DiT`.

The reference's downstream step trains a LightningDiT on the stored latents (`train_dit.py --dit_config configs/lightningdit_xl.yaml`,
a TODO there).  `LightningDiT` is `DiT` with three switches, each of which replaces one part of the block:

    use_rmsnorm   adaLN on an RMSNorm with a learned weight instead of the affine-free LayerNorm    `adaln_rms`
    use_qknorm    per-head RMSNorm of q and k before the 2-D RoPE                                   `qk_norm_rope_attention`
    use_swiglu    w3(silu(x1) x2), [x1 | x2] = w12(x), inner width (2 int(C mlp_ratio)) // 3         `swiglu`

`adaln_rms` is the RMS form of the adaLN kernel pair in csrc/dit.hip, the qk-norm pair is csrc/qk_norm.hip (one kernel family for
head_dim 64 and 72, `LightningDiT(..., head_dim=72)` / `lightning_dit_xl`), the SwiGLU pair csrc/lightning.hip; everything else
(embedders, conditioning path, padding, RoPE table, token GEMMs, attention at head_dim 64 or 72, gate + residual, the flow-matching edge,
`flow_matching_loss` / `sample_latents` / `fit_dit` / `evaluate_dit`) is what `DiT` uses, unchanged.  With a switch off that part of the
block is the DiT path.  There is no CPU fallback: host tensors raise.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .dit import LN_EPS, DiT, ModGrad, _AdaLNFn, _check_rows, adaln, flow_rows, gate_residual
from .hip import _lib as L
from .hip import ops
from .probe import _round_up

LIGHTNING_PRESETS = {"LightningDiT-B": (768, 12), "LightningDiT-L": (1024, 24)}


# ---------------------------------------------------------------------------------------------------------------------------
# the three kernel pairs under autograd
# ---------------------------------------------------------------------------------------------------------------------------
def _check_weight(w: torch.Tensor, n: int, like: torch.Tensor, what: str):
    ops._need_gpu(w)
    ops._require(w.dtype == torch.float32 and tuple(w.shape) == (n,) and w.is_contiguous() and w.device == like.device,
                 f"{what}: contiguous fp32 weight [{n}] on the rows' device")


class _QkNormRopeAttnFn(torch.autograd.Function):
    """Per-head RMSNorm of q and k, RoPE and attention at head_dim 64 or 72: weights [head_dim], table [N, 4, head_dim // 2]."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, rope_tab, heads, scale, eps, keep_raw, hd):
        ops.check_qkv(qkv, rope_tab, heads, hd, "qk_norm_rope_attention")
        B, N, _ = qkv.shape
        _check_weight(wq, hd, qkv, "qk_norm_rope_attention: q_norm")
        _check_weight(wk, hd, qkv, "qk_norm_rope_attention: k_norm")
        qn = torch.empty_like(qkv) if keep_raw else qkv          # in place when no backward will ask for the raw projections
        ops.hd_call("tv_qknorm_rope_fwd", hd, (ops._p(qkv), ops._p(wq), ops._p(wk), ops._p(rope_tab), ops._p(qn)), B, N, heads, eps)
        o = torch.empty((B, N, heads * hd), dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
        ops.hd_call("tv_attn_fwd", hd, (ops._p(qn), ops._p(o), ops._p(lse)), B, N, heads, scale)
        ctx.args = (heads, scale, eps, hd)
        if keep_raw:
            ctx.save_for_backward(qkv, qn, o, lse, wq, wk, rope_tab)
        return o

    @staticmethod
    def backward(ctx, go):
        qkv, qn, o, lse, wq, wk, rope_tab = ctx.saved_tensors
        heads, scale, eps, hd = ctx.args
        B, N, _ = qkv.shape
        lib = L.load()
        go = go.contiguous()
        ops._require(go.dtype == torch.bfloat16, "qk_norm_rope_attention: bf16 gradient rows")
        delta = torch.empty((2, B, heads, N), dtype=torch.float32, device=qkv.device)   # scratch: -delta, -lse log2(e)
        dqkv = torch.empty_like(qkv)
        # with the table tv_attn_bwd stores dq / dk with respect to the un-rotated operands: the norm's backward has no rotation in it
        ops.hd_call("tv_attn_bwd", hd, (ops._p(qn), ops._p(o), ops._p(go), ops._p(lse), ops._p(delta), ops._p(rope_tab), ops._p(dqkv)),
                    B, N, heads, scale)
        dwq, dwk = torch.empty_like(wq), torch.empty_like(wk)
        count = lib.tv_qknorm_rope_bwd_partial_count(B, N, heads) if hd == 64 else lib.tv_qknorm_rope_bwd_hd_partial_count(B, N, heads, hd)
        part = torch.empty(count, dtype=torch.float32, device=qkv.device)
        ops.hd_call("tv_qknorm_rope_bwd", hd, (ops._p(qkv), ops._p(wq), ops._p(wk), ops._p(dqkv), ops._p(dwq), ops._p(dwk), ops._p(part)),
                    B, N, heads, eps)
        return dqkv, dwq, dwk, None, None, None, None, None, None


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        ops._need_gpu(u)
        ops._require(u.dtype == torch.bfloat16 and u.dim() == 2 and u.is_contiguous() and u.shape[1] % 64 == 0,
                     "swiglu: contiguous bf16 rows [T, 2 Hp], Hp a multiple of 32")
        T, Hp = u.shape[0], u.shape[1] // 2
        h = torch.empty((T, Hp), dtype=torch.bfloat16, device=u.device)
        L.check(L.load().tv_swiglu_fwd(ops._p(u), ops._p(h), T, Hp, ops._stream()), "tv_swiglu_fwd")
        ctx.save_for_backward(u)
        return h

    @staticmethod
    def backward(ctx, gh):
        u, = ctx.saved_tensors
        gh = gh.contiguous()
        ops._require(gh.dtype == torch.bfloat16, "swiglu: bf16 gradient rows")
        du = torch.empty_like(u)
        L.check(L.load().tv_swiglu_bwd(ops._p(u), ops._p(gh), ops._p(du), u.shape[0], u.shape[1] // 2, ops._stream()), "tv_swiglu_bwd")
        return du


def adaln_rms(x: torch.Tensor, weight: torch.Tensor, mod: torch.Tensor, shift_off: int, scale_off: int, tokens: int, eps: float = LN_EPS,
              sink: Optional[ModGrad] = None, owner: bool = False):
    """(RMSNorm(x; weight) (1 + scale) + shift, x): `dit.adaln` on an RMSNorm with a learned fp32 weight [C].  bf16 rows
    [B tokens, C]; shift / scale are C columns of the fp32 `mod` [B, ld] from the given offsets; the second result IS x, and the `sink`
    / `owner` protocol is `dit.adaln`'s.  The weight's gradient is written by the same backward launch sequence, bit-reproducibly."""
    _check_rows(x, mod, int(tokens), "adaln_rms")
    _check_weight(weight, x.shape[1], x, "adaln_rms")
    return _AdaLNFn.apply(x, weight, mod, int(shift_off), int(scale_off), int(tokens), float(eps), sink, bool(owner))


def qk_norm_rope_attention(qkv: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, rope_tab: Optional[torch.Tensor], heads: int,
                           scale: float, eps: float = LN_EPS, head_dim: int = 64) -> torch.Tensor:
    """Attention on qkv [B, N, 3 C] bf16 (q | k | v, each [heads, head_dim]) with a per-head RMSNorm of q and k (fp32 weights
    [head_dim]) before the 2-D RoPE; returns o [B, N, C].  When no gradient is wanted (`torch.no_grad()`, or nothing that requires
    one) the norm and the rotation run IN PLACE on `qkv`, which the caller must not reuse; otherwise the raw projections are kept
    for the backward.  `head_dim` is 64 or 72 (never inferred from the shapes); 72 takes a table [N, 4, 36]."""
    keep_raw = torch.is_grad_enabled() and (qkv.requires_grad or q_weight.requires_grad or k_weight.requires_grad)
    return _QkNormRopeAttnFn.apply(qkv, q_weight, k_weight, rope_tab, int(heads), float(scale), float(eps), bool(keep_raw), int(head_dim))


def swiglu(u: torch.Tensor) -> torch.Tensor:
    """silu(x1) x2 on bf16 rows u = [x1 | x2] of width 2 Hp (Hp a multiple of 32): bf16 [T, Hp]."""
    return _SwiGLUFn.apply(u)


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
class _RmsWeight(nn.Module):
    """The learned weight of an RMSNorm; the arithmetic is in the kernels."""

    def __init__(self, n: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))


class _LightningAttn(nn.Module):
    def __init__(self, hidden: int, use_qknorm: bool, head_dim: int = 64):
        super().__init__()
        self.qkv = nn.Linear(hidden, 3 * hidden)
        if use_qknorm:
            self.q_norm = _RmsWeight(head_dim)
            self.k_norm = _RmsWeight(head_dim)
        self.proj = nn.Linear(hidden, hidden)


class _SwiGLUMlp(nn.Module):
    def __init__(self, hidden: int, inner: int):
        super().__init__()
        self.w12 = nn.Linear(hidden, 2 * inner)          # rows [x1 (the gated half) | x2]
        self.w3 = nn.Linear(inner, hidden)


class _GeluMlp(nn.Module):
    def __init__(self, hidden: int, inner: int):
        super().__init__()
        self.fc1 = nn.Linear(hidden, inner)
        self.fc2 = nn.Linear(inner, hidden)


def swiglu_inner(hidden: int, mlp_ratio: float) -> int:
    """The public `int(2 / 3 * int(hidden * mlp_ratio))` in integers: 341 at width 128, 2048 at 768, 2730 at 1024."""
    return (2 * int(hidden * mlp_ratio)) // 3


class LightningDiTBlock(nn.Module):
    def __init__(self, hidden: int, mlp_ratio: float, use_rmsnorm: bool, use_qknorm: bool, use_swiglu: bool, head_dim: int = 64):
        super().__init__()
        if use_rmsnorm:
            self.norm1 = _RmsWeight(hidden)
        self.attn = _LightningAttn(hidden, use_qknorm, head_dim)
        if use_rmsnorm:
            self.norm2 = _RmsWeight(hidden)
        self.mlp = _SwiGLUMlp(hidden, swiglu_inner(hidden, mlp_ratio)) if use_swiglu else _GeluMlp(hidden, int(hidden * mlp_ratio))
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden, 6 * hidden))


class _LightningFinal(nn.Module):
    def __init__(self, hidden: int, out_cols: int, use_rmsnorm: bool):
        super().__init__()
        if use_rmsnorm:
            self.norm_final = _RmsWeight(hidden)
        self.linear = nn.Linear(hidden, out_cols)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden, 2 * hidden))


class LightningDiT(DiT):
    """`DiT` with the LightningDiT block: `use_rmsnorm`, `use_qknorm`, `use_swiglu`, all on by default; with
    a switch off that part of the block is `DiT`'s.  Inputs, outputs, embedders, conditioning, checks and the RoPE table are `DiT`'s.
    The SwiGLU inner width H = (2 int(hidden mlp_ratio)) // 3 is kept in the state dict; when it is no multiple of 32 the operands
    are zero-padded to the next one inside `forward` (pad columns of the hidden rows exactly 0, no gradient kept)."""

    _built = False          # DiT.__init__ initialises before the blocks below exist: `initialize_weights` waits for them

    def __init__(self, input_size=16, patch_size: int = 1, in_channels: int = 32, hidden_size: int = 768, depth: int = 12,
                 num_classes: int = 1000, mlp_ratio: float = 4.0, class_dropout_prob: float = 0.1, use_rope: bool = True,
                 frequency_embedding_size: int = 256, generator: Optional[torch.Generator] = None, use_rmsnorm: bool = True,
                 use_qknorm: bool = True, use_swiglu: bool = True, head_dim: int = 64):
        if hidden_size > 1536:
            raise ValueError(f"LightningDiT: hidden_size={hidden_size} is above 1536, the widest row of the adaLN kernels")
        super().__init__(input_size, patch_size, in_channels, hidden_size, depth, num_classes, mlp_ratio, class_dropout_prob, use_rope,
                         frequency_embedding_size, generator, head_dim)
        self.use_rmsnorm, self.use_qknorm, self.use_swiglu = bool(use_rmsnorm), bool(use_qknorm), bool(use_swiglu)
        self.mlp_inner = swiglu_inner(hidden_size, mlp_ratio)
        if self.use_swiglu and self.mlp_inner < 1:
            raise ValueError(f"LightningDiT: mlp_ratio={mlp_ratio} gives no SwiGLU inner width")
        self.mlp_inner_padded = _round_up(self.mlp_inner, 32)
        self.blocks = nn.ModuleList([LightningDiTBlock(hidden_size, mlp_ratio, self.use_rmsnorm, self.use_qknorm, self.use_swiglu, self.head_dim)
                                     for _ in range(depth)])
        self.final_layer = _LightningFinal(hidden_size, self.patch_cols, self.use_rmsnorm)
        self._built = True
        self.initialize_weights(generator)

    @torch.no_grad()
    def initialize_weights(self, generator: Optional[torch.Generator] = None):
        """DiT's initialisation (the linears of the SwiGLU MLP are Xavier-uniform with zero bias like every other), and ones for
        every norm weight."""
        if not self._built:
            return
        super().initialize_weights(generator)
        for m in self.modules():
            if isinstance(m, _RmsWeight):
                m.weight.fill_(1.0)

    def _norm(self, h, norm, mod, shift_off, scale_off, sink, owner):
        if norm is None:
            return adaln(h, mod, shift_off, scale_off, self.tokens, LN_EPS, sink, owner)
        return adaln_rms(h, norm.weight, mod, shift_off, scale_off, self.tokens, LN_EPS, sink, owner)

    def _swiglu_operands(self, mlp: _SwiGLUMlp):
        H, Hp = self.mlp_inner, self.mlp_inner_padded
        w12, b12, w3 = mlp.w12.weight, mlp.w12.bias, mlp.w3.weight
        if Hp != H:                     # zero pad, rows [x1 | 0 | x2 | 0]: the pad columns of h are silu(0) 0 = 0 and meet zero columns of w3
            w12 = torch.cat([F.pad(w12[:H], (0, 0, 0, Hp - H)), F.pad(w12[H:], (0, 0, 0, Hp - H))])
            b12 = torch.cat([F.pad(b12[:H], (0, Hp - H)), F.pad(b12[H:], (0, Hp - H))])
            w3 = F.pad(w3, (0, Hp - H))
        return w12.contiguous(), b12.contiguous(), w3.contiguous()

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
        rms = self.use_rmsnorm
        for blk in self.blocks:
            mod = blk.adaLN_modulation(c).contiguous()
            sink = ModGrad(6) if mod.requires_grad else None
            a, hs = self._norm(h, blk.norm1 if rms else None, mod, 0, C, sink, True)
            qkv = ops.linear(a, blk.attn.qkv.weight, blk.attn.qkv.bias).view(B, N, 3 * C)
            if self.use_qknorm:
                o = qk_norm_rope_attention(qkv, blk.attn.q_norm.weight, blk.attn.k_norm.weight, tab, self.num_heads, self.attn_scale, LN_EPS, self.head_dim)
            else:
                o = ops.attention(qkv, tab, self.num_heads, self.attn_scale, self.head_dim)
            a = ops.linear(o.view(B * N, C), blk.attn.proj.weight, blk.attn.proj.bias)
            h = gate_residual(hs, a, mod, 2 * C, N, sink)
            a, hs = self._norm(h, blk.norm2 if rms else None, mod, 3 * C, 4 * C, sink, False)
            if self.use_swiglu:
                w12, b12, w3 = self._swiglu_operands(blk.mlp)
                a = ops.linear(swiglu(ops.linear(a, w12, b12)), w3, blk.mlp.w3.bias)
            else:
                a = ops.linear(a, blk.mlp.fc1.weight, blk.mlp.fc1.bias, act="gelu")
                a = ops.linear(a, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
            h = gate_residual(hs, a, mod, 5 * C, N, sink)
        mod = self.final_layer.adaLN_modulation(c).contiguous()
        a, _ = self._norm(h, self.final_layer.norm_final if rms else None, mod, 0, C, ModGrad(2) if mod.requires_grad else None, True)
        return ops.linear(a, wf.contiguous(), bf.contiguous())


def state_dict_keys(depth: int, use_rmsnorm: bool = True, use_qknorm: bool = True, use_swiglu: bool = True) -> list:
    """The state-dict names of a `LightningDiT` of `depth` blocks: the public LightningDiT definition's, without its `pos_embed`
    buffer (written from the public source, unchecked against a public checkpoint)."""
    wb = lambda k: [k + ".weight", k + ".bias"]
    keys = wb("x_embedder.proj") + wb("t_embedder.mlp.0") + wb("t_embedder.mlp.2") + ["y_embedder.embedding_table.weight"]
    for i in range(depth):
        b = f"blocks.{i}."
        keys += ([b + "norm1.weight"] if use_rmsnorm else []) + wb(b + "attn.qkv")
        keys += [b + "attn.q_norm.weight", b + "attn.k_norm.weight"] if use_qknorm else []
        keys += wb(b + "attn.proj") + ([b + "norm2.weight"] if use_rmsnorm else [])
        keys += (wb(b + "mlp.w12") + wb(b + "mlp.w3")) if use_swiglu else (wb(b + "mlp.fc1") + wb(b + "mlp.fc2"))
        keys += wb(b + "adaLN_modulation.1")
    keys += (["final_layer.norm_final.weight"] if use_rmsnorm else []) + wb("final_layer.linear") + wb("final_layer.adaLN_modulation.1")
    return keys


def create_lightning_dit(name: str = "LightningDiT-B", input_size=16, patch_size: int = 1, in_channels: int = 32, num_classes: int = 1000,
                         **kwargs) -> LightningDiT:
    """`LightningDiT-B` (768 wide, 12 deep) or `LightningDiT-L` (1024, 24), both at head_dim 64.  LightningDiT-XL (1152 wide, 28 deep,
    16 heads of 72) is `lightning_dit_xl`."""
    if name not in LIGHTNING_PRESETS:
        raise ValueError(f"create_lightning_dit: name={name!r} is not one of {sorted(LIGHTNING_PRESETS)}")
    hidden, depth = LIGHTNING_PRESETS[name]
    return LightningDiT(input_size, patch_size, in_channels, hidden, depth, num_classes, **kwargs)


def lightning_dit_xl(input_size=16, patch_size: int = 1, in_channels: int = 32, num_classes: int = 1000, **kwargs) -> LightningDiT:
    """LightningDiT-XL, the configuration the reference's downstream step names: 1152 wide, 28 deep, 16 heads of head_dim 72."""
    return LightningDiT(input_size, patch_size, in_channels, 1152, 28, num_classes, head_dim=72, **kwargs)
