"""LPIPS (VGG-16) perceptual distance on the HIP path: `lpips.LPIPS(net='vgg')` of R/transvae/losses/vae_loss.py:52,88-91.

    scaling layer (x - shift) / scale  ->  VGG-16 features up to relu5_3 (13 x [3x3 conv + ReLU], four 2x2 max-pools)
    taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64 / 128 / 256 / 512 / 512 channels); per tap and pixel
        f = x / (sqrt(sum_c x_c^2) + 1e-10),  g likewise from the target,  d = sum_c lin_c (f_c - g_c)^2
    spatial mean per tap, summed over the taps  ->  [B, 1, 1, 1]

Reconstruction and target run through the network as ONE batch of 2B (one launch per layer): `tv_lpips_prep` writes the first
layer's bf16 operand straight from the fp32 NCHW images, the convolutions are `tv_igemm_nt` with the ReLU epilogue, the pools
`tv_maxpool2x2_fwd`, the head `tv_lpips_head` (csrc/lpips.hip).  The weights are frozen: they are BUFFERS (no optimizer
state, invisible to DDP), packed to bf16 operands once at load time, and no weight gradient is ever computed.

Gradient.  Only `input` is differentiable.  When it requires grad, forward() also runs the data-gradient chain of the
reconstruction half -- head gradient per tap (written by the head's own launch), ReLU masks from the layers' bf16 outputs
(nothing else is saved), `tv_maxpool2x2_bwd` joining a tap's head gradient with the one coming down from the pool -- and keeps
d value[b] / d input; backward() scales it by the incoming per-image gradient.  (The same trade as the fused L1 + KL loss: no
activation of the 2B-image VGG pass outlives forward().)

No pretrained weights ship with the package and none are downloaded: load the state dict of `lpips.LPIPS(net='vgg')` with
:meth:`PerceptualLoss.load_lpips_state_dict` / :meth:`PerceptualLoss.from_file`.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from ..hip import _lib as L
from ..hip import ops

BF16 = torch.bfloat16

# (name, c_in, c_out); a max-pool precedes the first convolution of blocks 2-5; a tap follows the last one of each block
VGG_LAYERS: Tuple[Tuple[str, int, int], ...] = (
    ("conv1_1", 3, 64), ("conv1_2", 64, 64),
    ("conv2_1", 64, 128), ("conv2_2", 128, 128),
    ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256),
    ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512),
    ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512))
TAP_LAYERS = ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")
TAP_CHANNELS = (64, 128, 256, 512, 512)
POOL_BEFORE = ("conv2_1", "conv3_1", "conv4_1", "conv5_1")
LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)

# lpips.LPIPS(net='vgg').state_dict(): torchvision's vgg16().features indices of the 13 convolutions, grouped into the
# package's five slices.  (Written from the public definition of that module; the plain scheme below is the documented one.)
_TV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_TV_SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)


def plain_keys() -> List[str]:
    """The documented key scheme: conv1_1.weight ... conv5_3.bias, lin0 ... lin4 (and optionally shift / scale)."""
    keys = []
    for name, _, _ in VGG_LAYERS:
        keys += [f"{name}.weight", f"{name}.bias"]
    return keys + [f"lin{i}" for i in range(5)]


def _lpips_key_map() -> Dict[str, str]:
    """lpips-package key -> plain key."""
    m = {}
    for (name, _, _), idx, sl in zip(VGG_LAYERS, _TV_INDEX, _TV_SLICE):
        for part in ("weight", "bias"):
            m[f"net.slice{sl}.{idx}.{part}"] = f"{name}.{part}"
    for i in range(5):
        m[f"lin{i}.model.1.weight"] = f"lin{i}"
        m[f"lins.{i}.model.1.weight"] = f"lin{i}"
    m["scaling_layer.shift"] = "shift"
    m["scaling_layer.scale"] = "scale"
    return m


# ---------------------------------------------------------------------------------------------------------------------
# raw launches (bf16 NHWC device tensors; no autograd)
# ---------------------------------------------------------------------------------------------------------------------
def max_pool2x2(x: torch.Tensor) -> torch.Tensor:
    """F.max_pool2d(x, 2) on a contiguous bf16 NHWC tensor [B, H, W, C] -> [B, H // 2, W // 2, C]."""
    ops._need_gpu(x)
    ops._require(x.dim() == 4 and x.dtype == BF16 and x.is_contiguous(), "max_pool2x2: contiguous bf16 NHWC")
    B, H, W, Cc = x.shape
    y = torch.empty((B, H // 2, W // 2, Cc), dtype=BF16, device=x.device)
    L.check(L.load().tv_maxpool2x2_fwd(ops._p(x), ops._p(y), B, H, W, Cc, ops._stream()), "tv_maxpool2x2_fwd")
    return y


def max_pool2x2_backward(x: torch.Tensor, gy: torch.Tensor, add: Optional[torch.Tensor] = None, relu_mask: bool = False) -> torch.Tensor:
    """Gradient of max_pool2x2 w.r.t. x (argmax recomputed from x, torch's tie rule) [+ add] [masked by x > 0]."""
    ops._need_gpu(x, gy, add)
    B, H, W, Cc = x.shape
    ops._require(x.dtype == BF16 and x.is_contiguous() and gy.dtype == BF16 and gy.is_contiguous()
                 and tuple(gy.shape) == (B, H // 2, W // 2, Cc), "max_pool2x2_backward: x / gy must be contiguous bf16 NHWC of matching shapes")
    if add is not None:
        ops._require(add.shape == x.shape and add.dtype == BF16 and add.is_contiguous(), "max_pool2x2_backward: add must look like x")
    gx = torch.empty_like(x)
    L.check(L.load().tv_maxpool2x2_bwd(ops._p(x), ops._p(gy), ops._p(add), ops._p(gx), B, H, W, Cc, int(bool(relu_mask)), ops._stream()),
            "tv_maxpool2x2_bwd")
    return gx


def relu_backward(y: torch.Tensor, gy: torch.Tensor) -> torch.Tensor:
    """gy where the ReLU layer's own output y is > 0, else 0."""
    ops._need_gpu(y, gy)
    ops._require(y.shape == gy.shape and y.dtype == BF16 and gy.dtype == BF16 and y.is_contiguous() and gy.is_contiguous(),
                 "relu_backward: contiguous bf16 tensors of one shape")
    return ops.act_backward(y, gy, L.ACTX_RELU)


def conv3x3_relu(x: torch.Tensor, wb: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """relu(conv3x3(x) + bias), one rounding to bf16; x [B, H, W, Cin] bf16, wb the packed operand [Cout, 3, 3, Cin] bf16."""
    ops._need_gpu(x, wb, bias)
    B, H, W, Cin = x.shape
    Cout = wb.shape[0]
    ops._require(x.dtype == BF16 and x.is_contiguous() and wb.dtype == BF16 and wb.is_contiguous() and tuple(wb.shape) == (Cout, 3, 3, Cin),
                 "conv3x3_relu: operand check failed")
    out = torch.empty((B, H, W, Cout), dtype=BF16, device=x.device)
    d = ops._desc(batch=B, h_in=H, w_in=W, c_in=Cin, ldx=Cin, h_out=H, w_out=W, c_out=Cout, ldo=Cout, kh=3, kw=3, stride=1, pad=1,
                  act=L.ACTX_RELU)
    ops.igemm(d, x, wb, bias, None, None, out)
    return out


def conv3x3_relu_dgrad(gz: torch.Tensor, wt: torch.Tensor, y_prev: Optional[torch.Tensor]) -> torch.Tensor:
    """Data gradient of a 3x3 convolution; with y_prev (the producing ReLU layer's output) masked by y_prev > 0 in the same launch.
    gz [B, H, W, Cout] bf16, wt the packed transposed operand [Cin, 3, 3 (reversed), Cout] bf16."""
    B, H, W, Cout = gz.shape
    Cin = wt.shape[0]
    ops._require(gz.dtype == BF16 and gz.is_contiguous() and tuple(wt.shape) == (Cin, 3, 3, Cout), "conv3x3_relu_dgrad: operand check failed")
    dx = torch.empty((B, H, W, Cin), dtype=BF16, device=gz.device)
    d = ops._desc(batch=B, h_in=H, w_in=W, c_in=Cout, ldx=Cout, h_out=H, w_out=W, c_out=Cin, ldo=Cin, kh=3, kw=3, stride=1, pad=1)
    ops._igemm_bwd(d, gz, wt, None, y_prev, L.ACTX_RELU, dx)
    return dx


def lpips_head(feat: torch.Tensor, lin: torch.Tensor, out: torch.Tensor, want_grad: bool, accumulate: bool, upstream: float = 1.0):
    """One tap: feat [2B, H, W, C] bf16 (x images first, then t), lin [C] fp32; out [B] fp32 is written (or added to).
    Returns the bf16 gradient w.r.t. the x half [B, H, W, C] (times upstream) when want_grad."""
    ops._need_gpu(feat, lin, out)
    B2, H, W, Cc = feat.shape
    B = B2 // 2
    ops._require(B2 == 2 * B and feat.dtype == BF16 and feat.is_contiguous() and lin.dtype == torch.float32 and lin.numel() == Cc
                 and lin.is_contiguous() and out.dtype == torch.float32 and out.numel() == B and out.is_contiguous(),
                 "lpips_head: operand check failed")
    lib = L.load()
    n_part = lib.tv_lpips_head_partial_count(B, H * W, Cc)
    ops._require(n_part > 0, f"lpips_head: unsupported channel count {Cc}")
    part = torch.empty(n_part, dtype=torch.float32, device=feat.device)
    grad = torch.empty((B, H, W, Cc), dtype=BF16, device=feat.device) if want_grad else None
    L.check(lib.tv_lpips_head(ops._p(feat), ops._p(lin), ops._p(part), ops._p(out), ops._p(grad), B, H * W, Cc, C.c_float(upstream),
                              int(bool(accumulate)), ops._stream()), "tv_lpips_head")
    return grad


def _prep_flags(normalize: bool, sigmoid: bool, clamp: bool) -> int:
    return (L.LPIPS_MAP if normalize else 0) | (L.LPIPS_SIGMOID if sigmoid else 0) | (L.LPIPS_CLAMP if clamp else 0)


class _LpipsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, target, net, flags_in, flags_tg, want_grad):
        ops._need_gpu(inp, target)
        x = inp.detach().float().contiguous()
        t = target.detach().float().contiguous()
        B, _, H, W = x.shape
        need = bool(want_grad) and ctx.needs_input_grad[0]   # (grad mode is off inside forward(): the caller says whether it was on)
        lib = L.load()
        st = ops._stream
        cols = torch.empty((2 * B, H, W, 32), dtype=BF16, device=x.device)
        L.check(lib.tv_lpips_prep(ops._p(x), ops._p(t), ops._p(cols), B, B, H, W, flags_in, flags_tg, ops._p(net.shift_scale), st()), "tv_lpips_prep")
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        ys: List[torch.Tensor] = []       # ReLU outputs of the 13 layers (2B images)
        head_grads: List[Optional[torch.Tensor]] = []
        h = cols
        for i, (name, _, c_out) in enumerate(VGG_LAYERS):
            if name in POOL_BEFORE:
                h = max_pool2x2(h)
            wb = getattr(net, f"_op_{name}")
            bias = getattr(net, f"{name}_bias")
            if i == 0:   # K = 32 GEMM on the patch rows
                y = torch.empty((2 * B, H, W, c_out), dtype=BF16, device=x.device)
                d = ops._rows_desc(2 * B * H * W, 32, c_out)
                d.act = L.ACTX_RELU
                ops.igemm(d, h, wb, bias, None, None, y)
            else:
                y = conv3x3_relu(h, wb, bias)
            h = y
            if need:
                ys.append(y)
            if name in TAP_LAYERS:
                k = TAP_LAYERS.index(name)
                head_grads.append(lpips_head(y, getattr(net, f"lin{k}"), out, need, accumulate=k > 0))
        del cols
        if need:
            # the reconstruction half (images 0 .. B-1 of every tensor) backwards; gz = gradient w.r.t. a layer's pre-activation
            gz = relu_backward(ys[12][:B], head_grads[4])
            for i in range(12, 0, -1):
                name = VGG_LAYERS[i][0]
                wt = getattr(net, f"_opt_{name}")
                y_prev = ys[i - 1][:B]
                if name in POOL_BEFORE:    # this layer read pool(y_prev), and y_prev is a tap
                    gp = conv3x3_relu_dgrad(gz, wt, None)
                    gz = max_pool2x2_backward(y_prev, gp, add=head_grads[TAP_LAYERS.index(VGG_LAYERS[i - 1][0])], relu_mask=True)
                else:
                    gz = conv3x3_relu_dgrad(gz, wt, y_prev)
                ys[i] = None
            dcols = ops.gemm_rows(gz.view(B * H * W, 64), net._opt_conv1_1, 32)
            d_in = torch.empty_like(x)
            L.check(lib.tv_lpips_prep_bwd(ops._p(dcols), ops._p(x), ops._p(d_in), B, H, W, flags_in, ops._p(net.shift_scale), st()), "tv_lpips_prep_bwd")
            ctx.save_for_backward(d_in)
            ctx.in_dtype = inp.dtype
        return out.view(B, 1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        (d_in,) = ctx.saved_tensors
        return (d_in * g.reshape(-1, 1, 1, 1).to(d_in.dtype)).to(ctx.in_dtype), None, None, None, None, None


class PerceptualLoss(nn.Module):
    """LPIPS-VGG with frozen weights held as buffers.  `forward(input, target, normalize=False) -> [B, 1, 1, 1]` fp32, the
    `lpips.LPIPS.forward` convention: images in [-1, 1], or in [0, 1] with normalize=True.  Differentiable w.r.t. `input` only."""

    def __init__(self):
        super().__init__()
        for name, c_in, c_out in VGG_LAYERS:
            self.register_buffer(f"{name}_weight", torch.zeros(c_out, c_in, 3, 3))
            self.register_buffer(f"{name}_bias", torch.zeros(c_out))
            # bf16 operands of the kernels, derived from the weights by _pack(): not part of the state dict
            self.register_buffer(f"_op_{name}", torch.zeros(0, dtype=BF16), persistent=False)
            self.register_buffer(f"_opt_{name}", torch.zeros(0, dtype=BF16), persistent=False)
        for i, c in enumerate(TAP_CHANNELS):
            self.register_buffer(f"lin{i}", torch.zeros(c))
        self.register_buffer("shift_scale", torch.tensor(LPIPS_SHIFT + LPIPS_SCALE, dtype=torch.float32))
        self._pack()

    # ---- weights ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _pack(self):
        """fp32 [O, I, 3, 3] -> the forward operand [O, 3, 3, I] and the data-gradient operand [I, 3, 3 (taps reversed), O] in bf16
        (conv1_1: [64, 32] / [32, 64] over the (ky, kx, c) patch rows, 27 of 32 columns used).  Once per load, never per step."""
        for name, c_in, c_out in VGG_LAYERS:
            w = getattr(self, f"{name}_weight").float()
            krsc = w.permute(0, 2, 3, 1).contiguous()                       # [O, ky, kx, I]
            if c_in == 3:
                op = torch.zeros(c_out, 32, dtype=torch.float32, device=w.device)
                op[:, :27] = krsc.reshape(c_out, 27)
                opt = op.t().contiguous()
            else:
                op = krsc
                opt = krsc.flip(1, 2).permute(3, 1, 2, 0).contiguous()      # [I, 2-ky, 2-kx, O]
            setattr(self, f"_op_{name}", op.to(BF16).contiguous())
            setattr(self, f"_opt_{name}", opt.to(BF16).contiguous())

    def load_lpips_state_dict(self, sd: Dict[str, torch.Tensor]) -> "PerceptualLoss":
        """Accepts the state dict of `lpips.LPIPS(net='vgg')` (net.slice{1..5}.{idx}.{weight,bias}, lin{i}.model.1.weight -- also
        under lins.{i} --, scaling_layer.{shift,scale}) or the plain scheme of :func:`plain_keys` (conv1_1.weight ... conv5_3.bias,
        lin0 ... lin4, optional shift / scale).  Any mismatch raises with the full lists of missing and unexpected keys."""
        kmap = _lpips_key_map()
        plain = set(plain_keys()) | {"shift", "scale"}
        got: Dict[str, torch.Tensor] = {}
        unexpected = []
        for k, v in sd.items():
            pk = kmap.get(k, k if k in plain else None)
            if pk is None:
                unexpected.append(k)
            elif pk in got and not torch.equal(got[pk].reshape(-1).float().cpu(), v.reshape(-1).float().cpu()):
                unexpected.append(k + " (conflicts with another key of the same tensor)")
            else:
                got[pk] = v
        missing = [k for k in plain_keys() if k not in got]
        bad_shape = []
        for k, v in got.items():
            if k in ("shift", "scale"):
                ok = v.numel() == 3
            elif k.startswith("lin"):
                ok = v.numel() == TAP_CHANNELS[int(k[3:])]
            else:
                ok = tuple(v.shape) == tuple(getattr(self, k.replace(".", "_")).shape)
            if not ok:
                bad_shape.append(f"{k} {tuple(v.shape)}")
        if missing or unexpected or bad_shape:
            raise KeyError("PerceptualLoss.load_lpips_state_dict: the state dict does not match LPIPS-VGG.\n"
                           f"  missing ({len(missing)}): {missing}\n  unexpected ({len(unexpected)}): {unexpected}\n"
                           f"  wrong shape ({len(bad_shape)}): {bad_shape}\n"
                           "  accepted schemes: lpips.LPIPS(net='vgg').state_dict(), or " + ", ".join(plain_keys()[:2]) + " ... lin0 ... lin4")
        with torch.no_grad():
            for k, v in got.items():
                if k == "shift":
                    self.shift_scale[:3].copy_(v.reshape(3))
                elif k == "scale":
                    self.shift_scale[3:].copy_(v.reshape(3))
                elif k.startswith("lin"):
                    getattr(self, k).copy_(v.reshape(-1))
                else:
                    getattr(self, k.replace(".", "_")).copy_(v)
        self._pack()
        return self

    @classmethod
    def from_file(cls, path: str) -> "PerceptualLoss":
        """A PerceptualLoss from a file written with torch.save(lpips.LPIPS(net='vgg').state_dict(), path) (or the plain scheme)."""
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        return cls().load_lpips_state_dict(sd)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._pack()

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _check(self, inp: torch.Tensor, target: torch.Tensor):
        if inp.dim() != 4 or inp.shape != target.shape or inp.shape[1] != 3:
            raise ValueError(f"PerceptualLoss: input and target must both be [B, 3, H, W] of one shape, got {tuple(inp.shape)} and "
                             f"{tuple(target.shape)}")
        if inp.shape[0] == 0:
            raise ValueError("PerceptualLoss: empty batch")
        H, W = inp.shape[-2:]
        if H % 16 or W % 16:
            raise ValueError(f"PerceptualLoss: H and W must be multiples of 16 (four 2x2 pools, as the model requires), got {H}x{W}")
        if target.requires_grad:
            raise ValueError("PerceptualLoss: differentiable w.r.t. `input` only; pass target.detach()")

    def distance(self, inp: torch.Tensor, target: torch.Tensor, normalize: bool = False, sigmoid_input: bool = False,
                 clamp: bool = False) -> torch.Tensor:
        """forward() with the patched loss's options folded into the input pass (P/transvae/losses/vae_loss.py:80-91):
        sigmoid_input applies a sigmoid to `input` first, clamp clamps both images to [-1, 1] after the optional 2x - 1."""
        self._check(inp, target)
        ops._need_gpu(inp, target)
        if inp.device != target.device or inp.device != self.shift_scale.device:
            raise RuntimeError(f"PerceptualLoss: input on {inp.device}, target on {target.device}, weights on {self.shift_scale.device}")
        with torch.cuda.device(inp.device), torch.autocast("cuda", enabled=False):
            return _LpipsFn.apply(inp, target, self, _prep_flags(normalize, sigmoid_input, clamp), _prep_flags(normalize, False, clamp),
                                  torch.is_grad_enabled() and inp.requires_grad)

    def forward(self, input: torch.Tensor, target: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        return self.distance(input, target, normalize=normalize)
