"""rFID on the HIP path: the FID Inception-v3 pool3 feature extractor and the Frechet distance between feature statistics.

    images in [0, 1]  ->  bilinear resize to 299 x 299 (align_corners=False)  ->  2x - 1
    stem: 3->32 3x3 s2, 32->32 3x3, 32->64 3x3 p1, max-pool 3x3 s2, 64->80 1x1, 80->192 3x3, max-pool 3x3 s2
    Mixed_5b/5c/5d (InceptionA, pool branch 32 / 64 / 64), Mixed_6a (InceptionB), Mixed_6b..6e (InceptionC, c7 = 128 / 160 / 160 /
    192), Mixed_7a (InceptionD), Mixed_7b / 7c (InceptionE)  ->  global average pool  ->  [B, 2048] fp32

in the form the FID literature uses (pt_inception / pytorch-fid `FIDInceptionV3`): every convolution bias-free with eval-mode
BatchNorm (eps 1e-3) and ReLU; the branch average pools 3x3 / stride 1 / pad 1 with count_include_pad=False; the pool branch of
the second InceptionE a 3x3 / stride 1 / pad 1 MAX pool.  Written from that public definition.

Execution.  `tv_fid_prep` writes the first convolution's bf16 operand (resize, 2x - 1 and the 3x3 / stride-2 patch rows in one
pass over the fp32 NCHW images); every convolution is one `tv_igemm_nt` launch with the ReLU epilogue, BatchNorm folded into its
bf16 weight and fp32 bias when the weights are packed; a block's branches store straight into their column range of the block's
output (row stride `ldo`, offset pointer), so no concatenation kernel exists; the 1x7 / 7x1 / 1x3 / 3x1 convolutions are a row
gather (`tv_gather_line`) followed by a GEMM with K = taps * C, because the convolution descriptor has one pad for both axes;
widths that are no multiple of 32 (80, 48) are produced padded (96, 64) with zero weights.  Pools: `tv_pool3x3`; the last step is
`tv_global_avgpool`.  Forward only, no gradient.  `features(..., spatial=True)` also returns the sFID tap: the first 7 channels of
`Mixed_6d.branch1x1` over the 17 x 17 grid as fp32 rows (`tv_spatial_rows`; DESIGN.md section 3.5 on which activation that is).

`FrechetDistance` keeps count, mean and centred scatter matrix of both feature streams in fp64 on the device
(`tv_fid_accumulate`: the pairwise (Chan) merge applied one sample at a time, so the statistics do not depend on the batch
split) and computes  |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2)  on the host with numpy.linalg.eigh.

No weights ship with the package and none are downloaded: `InceptionFeatures.from_file("pt_inception.pth")`.  There is no CPU
fallback.  The key names of the pt_inception file are written from the public definition and have NOT been checked against the
real file.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .hip import _lib as L
from .hip import ops

BF16 = torch.bfloat16
BN_EPS = 1e-3
FEATURE_DIM = 2048
SPATIAL_BLOCK, SPATIAL_CHANNELS = "Mixed_6d", 7      # the sFID tap: the first 7 channels of this block's 1x1 branch
SPATIAL_DIM = 17 * 17 * SPATIAL_CHANNELS             # 2023 values per image, (h, w, c) order
SPATIAL_LD = 2048                                    # the row width: the next multiple of 64 (tv_fid_accumulate), zero-filled
_BN_PARTS = (("bn.weight", "gamma"), ("bn.bias", "beta"), ("bn.running_mean", "mean"), ("bn.running_var", "var"))


def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def _layers() -> Tuple[Tuple[str, int, int, int, int, int, int, int], ...]:
    """(name, c_in, c_out, kh, kw, stride, pad_h, pad_w) of the 94 convolutions, in execution order."""
    out: List[Tuple[str, int, int, int, int, int, int, int]] = []

    def add(name, c_in, c_out, k=1, stride=1, pad=0):
        kh, kw = (k, k) if isinstance(k, int) else k
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        out.append((name, c_in, c_out, kh, kw, stride, ph, pw))

    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, 3)
    for blk, c_in, pool in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(f"{blk}.branch1x1", c_in, 64)
        add(f"{blk}.branch5x5_1", c_in, 48)
        add(f"{blk}.branch5x5_2", 48, 64, 5, 1, 2)
        add(f"{blk}.branch3x3dbl_1", c_in, 64)
        add(f"{blk}.branch3x3dbl_2", 64, 96, 3, 1, 1)
        add(f"{blk}.branch3x3dbl_3", 96, 96, 3, 1, 1)
        add(f"{blk}.branch_pool", c_in, pool)
    add("Mixed_6a.branch3x3", 288, 384, 3, 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(f"{blk}.branch1x1", 768, 192)
        add(f"{blk}.branch7x7_1", 768, c7)
        add(f"{blk}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(f"{blk}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(f"{blk}.branch7x7dbl_1", 768, c7)
        add(f"{blk}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(f"{blk}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(f"{blk}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(f"{blk}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(f"{blk}.branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for blk, c_in in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(f"{blk}.branch1x1", c_in, 320)
        add(f"{blk}.branch3x3_1", c_in, 384)
        add(f"{blk}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{blk}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{blk}.branch3x3dbl_1", c_in, 448)
        add(f"{blk}.branch3x3dbl_2", 448, 384, 3, 1, 1)
        add(f"{blk}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{blk}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{blk}.branch_pool", c_in, 192)
    return tuple(out)


FID_LAYERS = _layers()
_SPEC = {l[0]: l for l in FID_LAYERS}


def plain_keys() -> List[str]:
    """The documented plain scheme: per layer `<name>.weight` [c_out, c_in, kh, kw] and `<name>.gamma / .beta / .mean / .var`
    [c_out] (BatchNorm weight, bias, running mean, running variance), `<name>` as in FID_LAYERS."""
    keys = []
    for l in FID_LAYERS:
        keys += [f"{l[0]}.weight"] + [f"{l[0]}.{p}" for _, p in _BN_PARTS]
    return keys


def _pt_key_map() -> Dict[str, str]:
    """pt_inception / torchvision key -> plain key."""
    m = {}
    for l in FID_LAYERS:
        m[f"{l[0]}.conv.weight"] = f"{l[0]}.weight"
        for src, dst in _BN_PARTS:
            m[f"{l[0]}.{src}"] = f"{l[0]}.{dst}"
    return m


def _buf(key: str) -> str:
    return "w_" + key.replace(".", "_")


# ---------------------------------------------------------------------------------------------------------------------
# raw launches (bf16 NHWC device tensors)
# ---------------------------------------------------------------------------------------------------------------------
def fid_prep(a: torch.Tensor, b: Optional[torch.Tensor] = None, clip: bool = False) -> torch.Tensor:
    """fp32 NCHW images in [0, 1] (a, then b) -> the first convolution's operand [Ba + Bb, 149, 149, 32] bf16."""
    ops._need_gpu(a, b)
    ops._require(a.dim() == 4 and a.shape[1] == 3 and a.dtype == torch.float32 and a.is_contiguous(), "fid_prep: contiguous fp32 [B, 3, H, W]")
    Ba, _, H, W = a.shape
    Bb = 0
    if b is not None:
        ops._require(b.dtype == torch.float32 and b.is_contiguous() and tuple(b.shape[1:]) == (3, H, W), "fid_prep: b must look like a")
        Bb = b.shape[0]
    cols = torch.empty((Ba + Bb, 149, 149, 32), dtype=BF16, device=a.device)
    L.check(L.load().tv_fid_prep(ops._p(a), ops._p(b), ops._p(cols), Ba, Bb, H, W, int(bool(clip)), ops._stream()), "tv_fid_prep")
    return cols


def _out_view(shape, out, off, width, device):
    """(tensor the caller reads, first-column view the kernel writes, row stride)"""
    if out is None:
        y = torch.empty(tuple(shape) + (width,), dtype=BF16, device=device)
        return y, y, width
    ops._require(tuple(out.shape[:-1]) == tuple(shape) and out.dtype == BF16 and out.is_contiguous() and off % 8 == 0
                 and off + width <= out.shape[-1], "output column range does not fit")
    return out, out[..., off:off + width], out.shape[-1]


def pool3x3(x: torch.Tensor, mode: int, out: Optional[torch.Tensor] = None, off: int = 0) -> torch.Tensor:
    """3x3 pool of a contiguous bf16 NHWC tensor (L.POOL3_*); with `out`, into columns [off, off + C) of it."""
    ops._need_gpu(x, out)
    ops._require(x.dim() == 4 and x.dtype == BF16 and x.is_contiguous(), "pool3x3: contiguous bf16 NHWC")
    B, H, W, Cc = x.shape
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == L.POOL3_MAX_S2 else (H, W)
    y, view, ldo = _out_view((B, Ho, Wo), out, off, Cc, x.device)
    L.check(L.load().tv_pool3x3(ops._p(x), ops._p(view), B, H, W, Cc, ldo, int(mode), ops._stream()), "tv_pool3x3")
    return y


def gather_line(x: torch.Tensor, taps: int, axis: int) -> torch.Tensor:
    """[B, H, W, C] bf16 -> [B * H * W, taps * C]: the rows of a taps x 1 (axis 0) or 1 x taps (axis 1) "same" convolution."""
    ops._need_gpu(x)
    ops._require(x.dim() == 4 and x.dtype == BF16 and x.is_contiguous(), "gather_line: contiguous bf16 NHWC")
    B, H, W, Cc = x.shape
    y = torch.empty((B * H * W, taps * Cc), dtype=BF16, device=x.device)
    L.check(L.load().tv_gather_line(ops._p(x), ops._p(y), B, H, W, Cc, int(taps), int(axis), ops._stream()), "tv_gather_line")
    return y


def global_avgpool(x: torch.Tensor) -> torch.Tensor:
    """[B, H, W, C] bf16 -> [B, C] fp32."""
    ops._need_gpu(x)
    ops._require(x.dim() == 4 and x.dtype == BF16 and x.is_contiguous(), "global_avgpool: contiguous bf16 NHWC")
    B, H, W, Cc = x.shape
    y = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    L.check(L.load().tv_global_avgpool(ops._p(x), ops._p(y), B, H * W, Cc, ops._stream()), "tv_global_avgpool")
    return y


def spatial_rows(x: torch.Tensor, c0: int, nc: int, ldo: int) -> torch.Tensor:
    """[B, H, W, C] bf16 -> [B, ldo] fp32: channels [c0, c0 + nc) of every position in (h, w, c) order, zeros from H * W * nc on."""
    ops._need_gpu(x)
    ops._require(x.dim() == 4 and x.dtype == BF16 and x.is_contiguous(), "spatial_rows: contiguous bf16 NHWC")
    B, H, W, Cc = x.shape
    ops._require(0 <= c0 and nc >= 1 and c0 + nc <= Cc and H * W * nc <= ldo, "spatial_rows: channel range or row width does not fit")
    y = torch.empty((B, ldo), dtype=torch.float32, device=x.device)
    L.check(L.load().tv_spatial_rows(ops._p(x), B, H * W, Cc, Cc, int(c0), int(nc), ops._p(y), int(ldo), ops._stream()), "tv_spatial_rows")
    return y


def _mode_of(kh: int, kw: int, stride: int, ph: int, pw: int) -> str:
    return {(1, 1, 1, 0, 0): "c1", (3, 3, 1, 1, 1): "c3s1", (3, 3, 1, 0, 0): "c3v1", (3, 3, 2, 0, 0): "c3v2", (5, 5, 1, 2, 2): "c5s1"}[
        (kh, kw, stride, ph, pw)]


def conv_relu(x: torch.Tensor, wb: torch.Tensor, bias: torch.Tensor, mode: str, out: Optional[torch.Tensor] = None, off: int = 0) -> torch.Tensor:
    """relu(conv(x) + bias), one rounding to bf16: one tv_igemm_nt launch.  x [B, H, W, Cin] bf16, wb the packed operand
    [Cout, KH, KW, Cin] bf16, mode an ops conv mode; with `out`, stored into columns [off, off + Cout) of it."""
    ops._need_gpu(x, wb, bias, out)
    ops._require(x.dtype == BF16 and x.is_contiguous() and wb.dtype == BF16 and wb.is_contiguous() and bias.dtype == torch.float32
                 and bias.numel() == wb.shape[0], "conv_relu: operand check failed")
    g = ops._Geo(mode, x, wb)
    y, view, ldo = _out_view((g.B, g.Ho, g.Wo), out, off, g.Cout, x.device)
    d = g.fwd_desc(L.ACTX_RELU)
    d.ldo = ldo
    ops.igemm(d, x, wb, bias, None, None, view)
    return y


def line_conv_relu(x: torch.Tensor, wb: torch.Tensor, bias: torch.Tensor, taps: int, axis: int, out: Optional[torch.Tensor] = None,
                   off: int = 0) -> torch.Tensor:
    """A taps x 1 (axis 0) / 1 x taps (axis 1) "same" convolution + bias + ReLU: row gather, then a GEMM with K = taps * Cin.
    wb [Cout, taps * Cin] bf16 (tap-major)."""
    B, H, W, Cin = x.shape
    Cout = wb.shape[0]
    ops._require(wb.dtype == BF16 and wb.is_contiguous() and tuple(wb.shape) == (Cout, taps * Cin) and bias.numel() == Cout,
                 "line_conv_relu: operand check failed")
    rows = gather_line(x, taps, axis)
    y, view, ldo = _out_view((B, H, W), out, off, Cout, x.device)
    d = ops._rows_desc(B * H * W, taps * Cin, Cout)
    d.act = L.ACTX_RELU
    d.ldo = ldo
    ops.igemm(d, rows, wb, bias, None, None, view)
    return y


# ---------------------------------------------------------------------------------------------------------------------
class InceptionFeatures(nn.Module):
    """The FID Inception-v3 pool3 extractor with frozen weights held as buffers.  `forward(images) -> [B, 2048]` fp32 for
    images [B, 3, H, W] in [0, 1] (H, W >= 8); `features(a, b)` runs two image sets as one batch."""

    MAX_BATCH = 256      # images per pass (a 147 x 147 x 64 activation of 256 images is 0.7 GB)

    def __init__(self):
        super().__init__()
        for name, c_in, c_out, kh, kw, _, _, _ in FID_LAYERS:
            self.register_buffer(_buf(f"{name}.weight"), torch.zeros(c_out, c_in, kh, kw))
            for _, part in _BN_PARTS:
                self.register_buffer(_buf(f"{name}.{part}"), torch.ones(c_out) if part in ("gamma", "var") else torch.zeros(c_out))
        self._ops: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

    # ---- weights ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def packed(self, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(bf16 operand, fp32 bias) of one layer: BatchNorm folded (w * gamma / sqrt(var + eps), beta - mean * gamma / sqrt(var +
        eps)), [c_out', kh, kw, c_in'] with c' the widths padded to multiples of 32 by zeros; the line convolutions as
        [c_out, taps * c_in], the first layer as [32, 32] over the (ky, kx, c) patch rows.  Packed once per load / device."""
        hit = self._ops.get(name)
        w = getattr(self, _buf(f"{name}.weight"))
        if hit is not None and hit[0].device == w.device:
            return hit
        _, c_in, c_out, kh, kw, _, _, _ = _SPEC[name]
        gamma, beta, mean, var = (getattr(self, _buf(f"{name}.{p}")).float() for _, p in _BN_PARTS)
        scale = gamma / torch.sqrt(var + BN_EPS)
        krsc = (w.float() * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1)            # [O, kh, kw, I]
        o_pad = _pad32(c_out)
        bias = torch.zeros(o_pad, dtype=torch.float32, device=w.device)
        bias[:c_out] = beta - mean * scale
        if c_in == 3:
            op = torch.zeros(o_pad, 32, dtype=torch.float32, device=w.device)
            op[:c_out, :27] = krsc.reshape(c_out, 27)
        else:
            op = torch.zeros(o_pad, kh, kw, _pad32(c_in), dtype=torch.float32, device=w.device)
            op[:c_out, :, :, :c_in] = krsc
            if kh != kw:
                op = op.reshape(o_pad, kh * kw * _pad32(c_in))
        hit = (op.to(BF16).contiguous(), bias)
        self._ops[name] = hit
        return hit

    def _apply(self, fn, *args, **kwargs):
        self._ops = {}
        return super()._apply(fn, *args, **kwargs)

    def load_fid_state_dict(self, sd: Dict[str, torch.Tensor]) -> "InceptionFeatures":
        """Accepts the pt_inception / pytorch-fid FIDInceptionV3 scheme (`<layer>.conv.weight`, `<layer>.bn.{weight, bias,
        running_mean, running_var}`; `fc.*`, `AuxLogits.*` and `num_batches_tracked` are ignored) or the plain scheme of
        :func:`plain_keys`.  A missing, unexpected or mis-shaped key raises KeyError naming it."""
        kmap = _pt_key_map()
        plain = set(plain_keys())
        got: Dict[str, torch.Tensor] = {}
        unexpected = []
        for k, v in sd.items():
            if k.startswith("fc.") or k.startswith("AuxLogits.") or k.endswith("num_batches_tracked"):
                continue
            pk = kmap.get(k, k if k in plain else None)
            if pk is None:
                unexpected.append(k)
            else:
                got[pk] = v
        missing = [k for k in plain_keys() if k not in got]
        bad_shape = [f"{k} {tuple(v.shape)} (expected {tuple(getattr(self, _buf(k)).shape)})" for k, v in got.items()
                     if tuple(v.shape) != tuple(getattr(self, _buf(k)).shape)]
        if missing or unexpected or bad_shape:
            raise KeyError("InceptionFeatures.load_fid_state_dict: the state dict does not match the FID Inception-v3.\n"
                           f"  missing ({len(missing)}): {missing}\n  unexpected ({len(unexpected)}): {unexpected}\n"
                           f"  wrong shape ({len(bad_shape)}): {bad_shape}\n"
                           "  accepted schemes: pt_inception (Conv2d_1a_3x3.conv.weight, Conv2d_1a_3x3.bn.weight ...), or "
                           + ", ".join(plain_keys()[:5]) + " ...")
        with torch.no_grad():
            for k, v in got.items():
                getattr(self, _buf(k)).copy_(v)
        self._ops = {}
        return self

    @classmethod
    def from_file(cls, path: str) -> "InceptionFeatures":
        """An InceptionFeatures from a file holding the pt_inception state dict (or the plain scheme)."""
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        return cls().load_fid_state_dict(sd)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._ops = {}

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _conv(self, x, name, out=None, off=0):
        _, _, _, kh, kw, stride, ph, pw = _SPEC[name]
        wb, bias = self.packed(name)
        if kh == kw:
            return conv_relu(x, wb, bias, _mode_of(kh, kw, stride, ph, pw), out, off)
        return line_conv_relu(x, wb, bias, max(kh, kw), 0 if kh > kw else 1, out, off)

    def _chain(self, x, blk, names, out=None, off=0):
        for i, n in enumerate(names):
            last = i == len(names) - 1
            x = self._conv(x, f"{blk}.{n}", out if last else None, off if last else 0)
        return x

    def _block_out(self, x, width, h=None, w=None):
        return torch.empty((x.shape[0], h or x.shape[1], w or x.shape[2], width), dtype=BF16, device=x.device)

    def _inception_a(self, x, blk, pool):
        y = self._block_out(x, 224 + pool)
        self._conv(x, f"{blk}.branch1x1", y, 0)
        self._chain(x, blk, ("branch5x5_1", "branch5x5_2"), y, 64)
        self._chain(x, blk, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), y, 128)
        self._conv(pool3x3(x, L.POOL3_AVG_S1P1), f"{blk}.branch_pool", y, 224)
        return y

    def _inception_b(self, x, blk):
        ho, wo = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
        y = self._block_out(x, 768, ho, wo)
        self._conv(x, f"{blk}.branch3x3", y, 0)
        self._chain(x, blk, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), y, 384)
        pool3x3(x, L.POOL3_MAX_S2, y, 480)
        return y

    def _inception_c(self, x, blk):
        y = self._block_out(x, 768)
        self._conv(x, f"{blk}.branch1x1", y, 0)
        self._chain(x, blk, ("branch7x7_1", "branch7x7_2", "branch7x7_3"), y, 192)
        self._chain(x, blk, ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"), y, 384)
        self._conv(pool3x3(x, L.POOL3_AVG_S1P1), f"{blk}.branch_pool", y, 576)
        return y

    def _inception_d(self, x, blk):
        ho, wo = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
        y = self._block_out(x, 1280, ho, wo)
        self._chain(x, blk, ("branch3x3_1", "branch3x3_2"), y, 0)
        self._chain(x, blk, ("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"), y, 320)
        pool3x3(x, L.POOL3_MAX_S2, y, 512)
        return y

    def _inception_e(self, x, blk, pool_mode):
        y = self._block_out(x, 2048)
        self._conv(x, f"{blk}.branch1x1", y, 0)
        t = self._conv(x, f"{blk}.branch3x3_1")
        self._conv(t, f"{blk}.branch3x3_2a", y, 320)
        self._conv(t, f"{blk}.branch3x3_2b", y, 704)
        t = self._chain(x, blk, ("branch3x3dbl_1", "branch3x3dbl_2"))
        self._conv(t, f"{blk}.branch3x3dbl_3a", y, 1088)
        self._conv(t, f"{blk}.branch3x3dbl_3b", y, 1472)
        self._conv(pool3x3(x, pool_mode), f"{blk}.branch_pool", y, 1856)
        return y

    def _run(self, a, b, clip, spatial=False):
        cols = fid_prep(a, b, clip)                                          # [B, 149, 149, 32]
        B = cols.shape[0]
        wb, bias = self.packed("Conv2d_1a_3x3")
        h = torch.empty((B, 149, 149, 32), dtype=BF16, device=cols.device)
        d = ops._rows_desc(B * 149 * 149, 32, 32)
        d.act = L.ACTX_RELU
        ops.igemm(d, cols, wb, bias, None, None, h)
        del cols
        h = self._conv(h, "Conv2d_2a_3x3")                                   # 147
        h = self._conv(h, "Conv2d_2b_3x3")
        h = pool3x3(h, L.POOL3_MAX_S2)                                       # 73
        h = self._conv(h, "Conv2d_3b_1x1")                                   # 80 channels in 96 columns
        h = self._conv(h, "Conv2d_4a_3x3")                                   # 71
        h = pool3x3(h, L.POOL3_MAX_S2)                                       # 35
        h = self._inception_a(h, "Mixed_5b", 32)
        h = self._inception_a(h, "Mixed_5c", 64)
        h = self._inception_a(h, "Mixed_5d", 64)
        h = self._inception_b(h, "Mixed_6a")                                 # 17
        sp = None
        for blk in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            h = self._inception_c(h, blk)
            if spatial and blk == SPATIAL_BLOCK:                             # branch1x1 sits at column 0 of the block's output
                sp = spatial_rows(h, 0, SPATIAL_CHANNELS, SPATIAL_LD)
        h = self._inception_d(h, "Mixed_7a")                                 # 8
        h = self._inception_e(h, "Mixed_7b", L.POOL3_AVG_S1P1)
        h = self._inception_e(h, "Mixed_7c", L.POOL3_MAX_S1P1)
        return (global_avgpool(h), sp) if spatial else global_avgpool(h)

    @torch.no_grad()
    def features(self, a: torch.Tensor, b: Optional[torch.Tensor] = None, clip: bool = False, spatial: bool = False):
        """[Ba (+ Bb), 2048] fp32 features of the images `a` (then `b`) as ONE batch; clip=True clamps the pixels to [0, 1].
        spatial=True returns (pool3 [n, 2048], spatial [n, SPATIAL_LD]): the second holds the sFID tap, the first SPATIAL_CHANNELS
        channels of `SPATIAL_BLOCK.branch1x1` over the 17 x 17 grid in (h, w, c) order (SPATIAL_DIM values) and zeros after them."""
        for t in (a,) if b is None else (a, b):
            if t.dim() != 4 or t.shape[1] != 3 or t.shape[0] == 0 or t.shape[2] < 8 or t.shape[3] < 8:
                raise ValueError(f"InceptionFeatures: images must be a non-empty [B, 3, H, W] with H, W >= 8, got {tuple(t.shape)}")
        if b is not None and b.shape[2:] != a.shape[2:]:
            raise ValueError(f"InceptionFeatures: the two image sets differ in size: {tuple(a.shape)} and {tuple(b.shape)}")
        ops._need_gpu(a, b)
        dev = getattr(self, _buf("Conv2d_1a_3x3.weight")).device
        if a.device != dev or (b is not None and b.device != dev):
            raise RuntimeError(f"InceptionFeatures: images on {a.device}, weights on {dev}")
        a = a.detach().float().contiguous()
        b = None if b is None else b.detach().float().contiguous()
        with torch.cuda.device(a.device), torch.autocast("cuda", enabled=False):
            n = a.shape[0] + (0 if b is None else b.shape[0])
            if n <= self.MAX_BATCH:
                return self._run(a, b, clip, spatial)
            parts = [self._run(t[i:i + self.MAX_BATCH], None, clip, spatial) for t in ((a,) if b is None else (a, b))
                     for i in range(0, t.shape[0], self.MAX_BATCH)]
            if spatial:
                return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            return torch.cat(parts)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        return self.features(images)


# ---------------------------------------------------------------------------------------------------------------------
# Frechet distance
# ---------------------------------------------------------------------------------------------------------------------
def _sym_eigh(m: np.ndarray):
    return np.linalg.eigh((m + m.T) * 0.5)


def frechet_from_statistics(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) in fp64, numpy.linalg.eigh only.

    tr (S1 S2)^(1/2) is the sum of the square roots of the eigenvalues of the symmetric matrix S1^(1/2) S2 S1^(1/2), clipped at
    zero.  S1 = V diag(w) V^T; the matrix is formed in S1's eigenbasis and restricted to the eigenvectors with w > d eps max(w):
    diag(sqrt w) V^T S2 V diag(sqrt w).  The dropped directions carry only zero eigenvalues of the product, and leaving them out
    keeps their rounding noise (of order eps max(w)^2, whose square root is 1e-8 max(w) per direction) out of the sum when the
    covariances are rank-deficient (n <= d)."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(-1), np.asarray(mu2, dtype=np.float64).reshape(-1)
    s1, s2 = np.asarray(sigma1, dtype=np.float64), np.asarray(sigma2, dtype=np.float64)
    d = mu1.shape[0]
    if mu2.shape[0] != d or s1.shape != (d, d) or s2.shape != (d, d):
        raise ValueError(f"frechet_from_statistics: shapes {mu1.shape} {s1.shape} {mu2.shape} {s2.shape}")
    w, v = _sym_eigh(s1)
    keep = w > d * np.finfo(np.float64).eps * max(float(w.max()), 0.0)
    tr_sqrt = 0.0
    if keep.any():
        q = v[:, keep] * np.sqrt(w[keep])                     # S1^(1/2) on its range, in the eigenbasis
        ev = np.linalg.eigh(_half_sym(q.T @ ((s2 + s2.T) * 0.5) @ q))[0]
        tr_sqrt = float(np.sqrt(np.clip(ev, 0.0, None)).sum())
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * tr_sqrt)


def _half_sym(m: np.ndarray) -> np.ndarray:
    return (m + m.T) * 0.5


class FrechetDistance:
    """Streaming Frechet distance between two feature sets.  update(real, fake) merges fp32 feature rows [B, >= dims] (device
    tensors; the first `dims` columns are used) into fp64 statistics on the device; compute() returns the distance."""

    def __init__(self, dims: int = FEATURE_DIM):
        if L.load().tv_fid_state_doubles(int(dims)) < 0:
            raise ValueError(f"FrechetDistance: dims={dims} must be a multiple of 64 up to 8192")
        self.dims = int(dims)
        self._state = [None, None]
        self._n = [0, 0]

    def _merge(self, side: int, feats: torch.Tensor):
        ops._need_gpu(feats)
        ops._require(feats.dim() == 2 and feats.dtype == torch.float32 and feats.shape[1] >= self.dims and feats.stride(1) == 1
                     and feats.stride(0) >= self.dims, "FrechetDistance.update: fp32 [B, >= dims] rows")
        if feats.shape[0] == 0:
            return
        lib = L.load()
        with torch.cuda.device(feats.device):
            if self._state[side] is None:
                self._state[side] = torch.zeros(lib.tv_fid_state_doubles(self.dims), dtype=torch.float64, device=feats.device)
            st = self._state[side]
            ops._require(st.device == feats.device, "FrechetDistance.update: features moved to another device")
            B = feats.shape[0]
            scratch = torch.empty((B, self.dims), dtype=torch.float64, device=feats.device)
            L.check(lib.tv_fid_accumulate(ops._p(feats), B, self.dims, feats.stride(0), self._n[side], ops._p(st), ops._p(scratch),
                                          ops._stream()), "tv_fid_accumulate")
        self._n[side] += B

    def update(self, real_features: Optional[torch.Tensor], fake_features: Optional[torch.Tensor]) -> None:
        if real_features is not None:
            self._merge(0, real_features)
        if fake_features is not None:
            self._merge(1, fake_features)

    @property
    def n(self) -> Tuple[int, int]:
        return tuple(self._n)

    def state(self, side: int) -> torch.Tensor:
        """The device state {count, unused, mean[dims], M2[dims, dims]} of one side (fp64)."""
        return self._state[side]

    def statistics(self, side: int):
        """(n, mean [dims], covariance [dims, dims] = scatter / (n - 1), as np.cov gives) of one side, fp64 on the host."""
        n = self._n[side]
        if n < 2:
            raise ValueError(f"FrechetDistance: {n} sample(s) on side {side}; the covariance needs at least 2")
        st = self._state[side].cpu().numpy()
        d = self.dims
        assert int(st[0]) == n
        return n, st[2:2 + d].copy(), st[2 + d:].reshape(d, d) / (n - 1)

    def compute(self) -> float:
        _, mu1, s1 = self.statistics(0)
        _, mu2, s2 = self.statistics(1)
        return frechet_from_statistics(mu1, s1, mu2, s2)
