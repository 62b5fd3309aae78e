"""The 70x70 PatchGAN discriminator of the adversarial stage, on the HIP path.

The reference's loss accepts "any nn.Module" as `discriminator` (R/transvae/losses/vae_loss.py:103-111) and ships none; this is
the network the VAE trainers around it use (pix2pix / taming-transformers `NLayerDiscriminator`, n_layers = 3):

    Conv(3, ndf, 4, s2, p1) + LeakyReLU(0.2)
    Conv(ndf, 2ndf, 4, s2, p1, no bias) + BatchNorm + LeakyReLU(0.2)
    Conv(2ndf, 4ndf, 4, s2, p1, no bias) + BatchNorm + LeakyReLU(0.2)
    Conv(4ndf, 8ndf, 4, s1, p1, no bias) + BatchNorm + LeakyReLU(0.2)
    Conv(8ndf, 1, 4, s1, p1)                                              -> logits [B, 1, H/8 - 2, W/8 - 2]

Parameters and buffers live in a plain `nn.Sequential` named `main`, so the state dict has exactly the keys and shapes of that
Sequential (main.0.weight ... main.11.bias) and checkpoints move both ways; the Sequential itself is never called.  The forward
runs on the package's kernels: `tv_patch4x4s2` turns the fp32 image into the first layer's bf16 operand (a K = 64 GEMM with the
LeakyReLU epilogue), the other convolutions are `tv_igemm_nt` with 4x4 taps ('c4s2' / 'c4s1' of transvae.hip.ops), BatchNorm +
LeakyReLU is the `tv_bn_*` family of csrc/gan.hip.  Activations are bf16 NHWC, statistics and parameter gradients fp32.
One call is one BatchNorm batch, as in torch: real and fake batches passed separately get separate statistics.
There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..hip import _lib as L
from ..hip import ops

BF16 = torch.bfloat16
_LAST_PAD = 32     # the single output channel of the last layer as 32 GEMM columns (zero rows): its data gradient is a GEMM
                   # over those columns, and tv_igemm_nt needs the reduction dimension to be a multiple of 32


def _strides4(t: torch.Tensor):
    return tuple(int(s) for s in t.stride())


class _PatchRowsFn(torch.autograd.Function):
    """fp32 image [B, 3, H, W] (any strides) -> bf16 [B, H/2, W/2, 64]: the 4x4 / stride-2 / pad-1 patches, (ky, kx, c) order."""

    @staticmethod
    def forward(ctx, x, sigmoid: bool):
        ops._need_gpu(x)
        B, _, H, W = x.shape
        rows = torch.empty((B, H // 2, W // 2, 64), dtype=BF16, device=x.device)
        L.check(L.load().tv_patch4x4s2(ops._p(x), *_strides4(x), ops._p(rows), B, H, W, int(bool(sigmoid)), ops._stream()), "tv_patch4x4s2")
        ctx.sigmoid = bool(sigmoid)
        ctx.save_for_backward(x if sigmoid else None)
        ctx.x_shape = tuple(x.shape)
        return rows

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, _, H, W = ctx.x_shape
        g = g.contiguous()
        dx = torch.empty(ctx.x_shape, dtype=torch.float32, device=g.device)
        st = _strides4(x) if x is not None else (0, 0, 0, 0)
        L.check(L.load().tv_patch4x4s2_bwd(ops._p(g), ops._p(x), *st, ops._p(dx), B, H, W, int(ctx.sigmoid), ops._stream()), "tv_patch4x4s2_bwd")
        return dx, None


class _StemFn(torch.autograd.Function):
    """x1 = conv4x4s2(lrelu(rows w0^T + b0), w1): layers 0 and 1 up to the first BatchNorm.  Only the bf16 output y0 of the
    LeakyReLU layer is saved (its sign is its own backward mask), and the mask rides in the epilogue of layer 1's data gradient."""

    @staticmethod
    def forward(ctx, rows, w0, b0, w1):
        ops._need_gpu(rows, w0, b0, w1)
        ops._require(rows.dtype == BF16 and rows.is_contiguous() and rows.dim() == 4 and rows.shape[-1] == 64, "stem: bf16 patch rows [B, H, W, 64]")
        B, H, W, _ = rows.shape
        ndf = w0.shape[0]
        w0c, w1c = w0.contiguous(), w1.contiguous()
        wb0, _ = ops.pack_weight(w0c.view(ndf, 1, 64), True, False, False)
        y0 = torch.empty((B, H, W, ndf), dtype=BF16, device=rows.device)
        d = ops._rows_desc(B * H * W, 64, ndf)
        d.act = L.ACTX_LRELU
        ops.igemm(d, rows, wb0, b0.contiguous(), None, None, y0)
        x1, _, g1, _ = ops.conv_forward(y0, w1c, None, None, "c4s2", L.ACT_NONE, False)
        ctx.geo1 = g1
        ctx.save_for_backward(rows, w0c, y0, w1c)
        return x1

    @staticmethod
    def backward(ctx, gx1):
        rows, w0, y0, w1 = ctx.saved_tensors
        g1 = ctx.geo1
        gx1 = gx1.contiguous()
        B, H, W, _ = rows.shape
        ndf = w0.shape[0]
        need_rows, need_w0, need_b0, need_w1 = ctx.needs_input_grad
        dw1 = ops.conv_wgrad(g1, w1, y0, gx1, False)[0] if need_w1 else None
        drows = dw0 = db0 = None
        if need_rows or need_w0 or need_b0:
            gz0 = ops.conv_dgrad(g1, w1, gx1, y0.shape, aux=y0, aux_act=L.ACTX_LRELU)     # gradient w.r.t. layer 0's pre-activation
            g0 = ops._Geo("linear", rows.view(-1, 64), w0)
            if need_w0 or need_b0:
                dw0, db0 = ops.conv_wgrad(g0, w0, rows.view(-1, 64), gz0.view(-1, ndf), True)
            if need_rows:
                drows = ops.conv_dgrad(g0, w0, gz0.view(-1, ndf), (B * H * W, 64)).view(B, H, W, 64)
        return drows, dw0, db0, dw1


class _BnLReluFn(torch.autograd.Function):
    """y = lrelu(batchnorm(x)) on bf16 NHWC x.  training: batch statistics (and the running buffers updated on the device);
    otherwise the running statistics, whose backward is the plain affine one."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training: bool, eps: float, momentum: float):
        ops._need_gpu(x, gamma, beta)
        ops._require(x.dtype == BF16 and x.is_contiguous() and x.dim() == 4, "batch norm: contiguous bf16 NHWC")
        Cc = x.shape[-1]
        M = x.numel() // Cc
        lib = L.load()
        dev = x.device
        gamma_c, beta_c = gamma.contiguous(), beta.contiguous()
        mr = torch.empty((2, Cc), dtype=torch.float32, device=dev)
        ss = torch.empty((2, Cc), dtype=torch.float32, device=dev)
        if training:
            n_part = lib.tv_bn_partial_count(M, Cc)
            ops._require(n_part > 0, f"batch norm: unsupported channel count {Cc}")
            part = torch.empty((n_part,), dtype=torch.float32, device=dev)
            L.check(lib.tv_bn_stats(ops._p(x), ops._p(gamma_c), ops._p(beta_c), ops._p(part), ops._p(mr), ops._p(ss), ops._p(running_mean),
                                    ops._p(running_var), M, Cc, C.c_float(eps), C.c_float(momentum), ops._stream()), "tv_bn_stats")
        else:
            rstd = torch.rsqrt(running_var.float() + eps)
            mr[0], mr[1] = running_mean.float(), rstd
            ss[0] = gamma_c * rstd
            ss[1] = beta_c - mr[0] * ss[0]
        y = torch.empty_like(x)
        L.check(lib.tv_bn_lrelu_apply(ops._p(x), ops._p(ss), ops._p(y), M, Cc, ops._stream()), "tv_bn_lrelu_apply")
        ctx.training = bool(training)
        ctx.save_for_backward(x, mr, ss)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mr, ss = ctx.saved_tensors
        gy = gy.contiguous()
        Cc = x.shape[-1]
        M = x.numel() // Cc
        lib = L.load()
        dev = x.device
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        red = dg = db = dx = None
        if need_g or need_b or (need_x and ctx.training):
            part = torch.empty((lib.tv_bn_partial_count(M, Cc),), dtype=torch.float32, device=dev)
            red = torch.empty((2, Cc), dtype=torch.float32, device=dev)
            dg = torch.empty((Cc,), dtype=torch.float32, device=dev) if need_g else None
            db = torch.empty((Cc,), dtype=torch.float32, device=dev) if need_b else None
            L.check(lib.tv_bn_lrelu_bwd_reduce(ops._p(x), ops._p(gy), ops._p(mr), ops._p(ss), ops._p(part), ops._p(red), ops._p(dg), ops._p(db),
                                               M, Cc, 0, ops._stream()), "tv_bn_lrelu_bwd_reduce")
        if need_x:
            dx = torch.empty_like(x)
            L.check(lib.tv_bn_lrelu_bwd_apply(ops._p(x), ops._p(gy), ops._p(mr), ops._p(ss), ops._p(red), ops._p(dx), M, Cc,
                                              int(not ctx.training), ops._stream()), "tv_bn_lrelu_bwd_apply")
        return dx, dg, db, None, None, None, None, None


def batch_norm_lrelu(x, bn: nn.BatchNorm2d, training: bool):
    if training and bn.track_running_stats:
        with torch.no_grad():
            bn.num_batches_tracked += 1
        return _BnLReluFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, bn.eps, bn.momentum)
    return _BnLReluFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, False, bn.eps, bn.momentum)


class PatchDiscriminator(nn.Module):
    """`forward(x [B, 3, H, W] fp32) -> logits [B, 1, H/8 - 2, W/8 - 2] fp32`; H, W multiples of 8, at least 32.
    Differentiable w.r.t. x and the parameters; `train()` / `eval()` switch BatchNorm between batch and running statistics."""

    takes_sigmoid_flag = True    # forward(x, sigmoid_input=True) applies a sigmoid inside the input pass (TransVAELoss uses it)

    def __init__(self, input_channels: int = 3, ndf: int = 64, n_layers: int = 3):
        super().__init__()
        if input_channels != 3:
            raise ValueError(f"PatchDiscriminator (HIP path): input_channels must be 3, got {input_channels}")
        if n_layers != 3:
            raise ValueError(f"PatchDiscriminator (HIP path): only the 70x70 network (n_layers=3) is built, got n_layers={n_layers}")
        if ndf <= 0 or ndf % 32:
            raise ValueError(f"PatchDiscriminator (HIP path): ndf must be a positive multiple of 32, got {ndf}")
        self.ndf = ndf
        seq = [nn.Conv2d(3, ndf, 4, 2, 1), nn.LeakyReLU(0.2, True)]
        c = ndf
        for i in range(1, 4):
            seq += [nn.Conv2d(c, 2 * c, 4, 2 if i < 3 else 1, 1, bias=False), nn.BatchNorm2d(2 * c), nn.LeakyReLU(0.2, True)]
            c *= 2
        seq += [nn.Conv2d(c, 1, 4, 1, 1)]
        self.main = nn.Sequential(*seq)
        for m in self.main:
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0.0, 0.02)
                # channels_last memory = the [Cout, KH, KW, Cin] layout the kernels repack from
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight, 1.0, 0.02)
                nn.init.constant_(m.bias, 0.0)

    def _check(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"PatchDiscriminator: input must be [B, 3, H, W], got {tuple(x.shape)}")
        H, W = x.shape[-2:]
        if x.shape[0] == 0 or H % 8 or W % 8 or H < 32 or W < 32:
            raise ValueError(f"PatchDiscriminator: a non-empty batch with H and W multiples of 8, at least 32; got {tuple(x.shape)}")

    @ops.hip_entry
    def forward(self, x: torch.Tensor, sigmoid_input: bool = False) -> torch.Tensor:
        self._check(x)
        ops._need_gpu(x)
        m = self.main
        if m[0].weight.device != x.device:
            raise RuntimeError(f"PatchDiscriminator: input on {x.device}, weights on {m[0].weight.device}")
        x = x.float()
        rows = _PatchRowsFn.apply(x, bool(sigmoid_input))
        ndf = self.ndf
        w0 = F.pad(m[0].weight.permute(0, 2, 3, 1).reshape(ndf, 48), (0, 16))
        h = _StemFn.apply(rows, w0, m[0].bias, m[2].weight.permute(0, 2, 3, 1))
        h = batch_norm_lrelu(h, m[3], self.training)
        h = ops.conv(h, m[5].weight.permute(0, 2, 3, 1), None, None, "c4s2")
        h = batch_norm_lrelu(h, m[6], self.training)
        h = ops.conv(h, m[8].weight.permute(0, 2, 3, 1), None, None, "c4s1")
        h = batch_norm_lrelu(h, m[9], self.training)
        w4 = F.pad(m[11].weight.permute(0, 2, 3, 1), (0, 0, 0, 0, 0, 0, 0, _LAST_PAD - 1))
        b4 = F.pad(m[11].bias, (0, _LAST_PAD - 1))
        h = ops.conv(h, w4, b4, None, "c4s1")
        return ops.to_nchw(h, 0, 1)
