"""NumPy / torch restatement of the image pipeline's definitions (test infrastructure, not product).

Inbound: PIL's 8-bit bilinear `Image.resize` as integer arithmetic on coefficient tables built in float64, torchvision's
`Resize(int)` size rule, `CenterCrop`'s offsets and `ToTensor`'s value.  Checked bit for bit against Pillow 12.2.0 (the fixture
tests/golden/image_prep_pil.npz holds PIL's own outputs; tests/test_image_host.py compares against PIL directly where it is
importable).  Outbound: torchvision's `make_grid` layout and `save_image`'s quantisation, written from torchvision's public source.

Everything here is written independently of transvae.image_io: the product builds its tables with its own code.
"""
import math

import numpy as np
import torch

PB = 22


def coeffs(in_size, out_size):
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]   # float64
        ww = 0.0
        for v in w:
            ww += v                                                                    # PIL's summation order
        k = [int(0.5 + (v / ww) * (1 << PB)) for v in w]                               # truncation
        yield xmin, n, k


def resample_axis(img, out_size, axis):
    """One pass of PIL's resample along `axis` (0 = vertical, 1 = horizontal) of a uint8 [H, W, C] array."""
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for i, (xmin, n, k) in enumerate(coeffs(a.shape[0], out_size)):
        acc = (1 << (PB - 1)) + np.tensordot(np.asarray(k, np.int64), a[xmin:xmin + n], axes=(0, 0))
        assert acc.max() < 2 ** 31
        out[i] = np.clip(acc >> PB, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_resize(img, out_h, out_w):
    """Image.fromarray(img).resize((out_w, out_h), BILINEAR): horizontal pass if the width changes, then the vertical pass on
    the uint8 result if the height changes."""
    if out_w != img.shape[1]:
        img = resample_axis(img, out_w, 1)
    if out_h != img.shape[0]:
        img = resample_axis(img, out_h, 0)
    return img


def resize_size(h, w, res):
    """torchvision Resize(int)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == res:
        return h, w
    new_long = int(res * long / short)
    return (new_long, res) if w <= h else (res, new_long)


def center_crop(img, res_h, res_w):
    h, w = img.shape[:2]
    top = int(round((h - res_h) / 2.0))       # Python's round: half to even
    left = int(round((w - res_w) / 2.0))
    return img[top:top + res_h, left:left + res_w]


def prep_uint8(img, res=None, resize=None):
    """The uint8 [res_h, res_w, 3] result of Resize(res) -> CenterCrop(res), or of an explicit resize=(h, w) with no crop."""
    if resize is not None:
        return pil_resize(img, resize[0], resize[1])
    oh, ow = resize_size(img.shape[0], img.shape[1], res)
    return center_crop(pil_resize(img, oh, ow), res, res)


def to_tensor(u8, signed=False):
    """ToTensor: [H, W, 3] uint8 -> fp32 [3, H, W], float(v) / 255.0f; signed: x*2-1 in fp32 after the division."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return x * 2 - 1 if signed else x


def grid_shape(B, H, W, nrow, padding):
    if B == 1:
        return H, W
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding


def make_grid(x, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid of a [B, 3, H, W] tensor (no normalisation) -> [3, Hg, Wg], same dtype."""
    B, Cn, H, W = x.shape
    if B == 1:
        return x[0]
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    ch, cw = H + padding, W + padding
    grid = x.new_full((Cn, ch * ymaps + padding, cw * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for xx in range(xmaps):
            if k >= B:
                break
            grid[:, y * ch + padding:y * ch + padding + H, xx * cw + padding:xx * cw + padding + W] = x[k]
            k += 1
    return grid


def quantise(x):
    """save_image: mul(255).add_(0.5).clamp_(0, 255) in fp32, each step rounded, then truncation; NaN -> 0.  [3, H, W] fp32 -> uint8 [H, W, 3]."""
    t = x.to(torch.float32).mul(255).add_(0.5)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t).clamp_(0, 255)
    return t.permute(1, 2, 0).to(torch.uint8).contiguous().numpy()


def grid_u8(x, nrow=8, padding=2, pad_value=0.0):
    return quantise(make_grid(x.float().cpu(), nrow, padding, pad_value))


def grid_u8_sigmoid_fp64(x, nrow=8, padding=2, pad_value=0.0, tie_eps=1e-3):
    """The sigmoid grid with the sigmoid in fp64: (uint8 grid, near-tie mask [Hg, Wg, 3], share of near-tie input elements).
    A pixel is near a tie when its fp64 255 s + 0.5 lies within tie_eps of an integer."""
    xd = x.double().cpu()
    s = 1.0 / (1.0 + torch.exp(-xd))
    q = 255.0 * s + 0.5
    near = (q - torch.round(q)).abs() < tie_eps
    qg = make_grid(q, nrow, padding, 255.0 * float(pad_value) + 0.5)
    ng = make_grid(near.to(torch.float64), nrow, padding, 0.0) > 0
    u8 = qg.clamp(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous().numpy()
    return u8, ng.permute(1, 2, 0).contiguous().numpy(), float(near.double().mean())


def decode_png(data):
    """Inverse of an 8-bit RGB, non-interlaced PNG whose rows all use filter 0: -> uint8 [H, W, 3]."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour, comp, filt, interlace = hdr
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3).copy()
