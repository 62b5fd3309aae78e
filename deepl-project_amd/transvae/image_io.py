"""The edge between decoded images and tensors, on the device (csrc/image.hip).

Inbound, every script of the reference that touches pixels builds `Resize(res) -> CenterCrop(res) -> ToTensor()` and runs it per
image on the host through PIL (R/train.py:141-144,396-399, R/evaluate.py:39-42, R/inference_example.py:13-16,
P/generate_images.py:152-155; R/train_2.py:166-170 adds `x*2-1`).  :class:`ImagePrep` is that transform for a whole ragged
batch of uint8 images in one launch, bit-equal to PIL's 8-bit bilinear resample: the loader ships the decoded bytes
(:func:`collate_uint8` -> :class:`UInt8Batch`, one pinned buffer) and the fp32 `[B, 3, res, res]` tensor is made on the device.

Outbound, the patched scripts write decoded samples with torchvision's `make_grid` / `save_image`
(P/generate_images.py:181-235, P/evaluate_transvae.py:227-249): :func:`to_uint8_grid` lays out and quantises the grid in one
launch and :func:`save_image` writes it as a PNG with the standard library.

There is no CPU fallback: host tensors raise.  The coefficient tables (O(res * taps) integers) are host glue, built once per
size pair and cached.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .hip import _lib as L
from .hip import ops

PRECISION_BITS = 22      # PIL's fixed point for 8-bit resampling
MAX_RATIO = 16           # largest supported down-scale per axis (tv_image_prep)
_RANGES = ("unit", "signed")
_TRANSFORMS = {"none": L.IMAGE_NONE, "sigmoid": L.IMAGE_SIGMOID}


# ------------------------------------------------------------------------------------------------------------------
# geometry and tables (host)
# ------------------------------------------------------------------------------------------------------------------
def resize_size(h: int, w: int, res: int) -> Tuple[int, int]:
    """torchvision's Resize(int): the short side becomes `res`, the long side int(res * long / short); an image whose short
    side already equals `res` keeps its size (and is not resampled)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == res:
        return h, w
    new_long = int(res * long / short)
    return (new_long, res) if w <= h else (res, new_long)


def center_crop_offsets(h: int, w: int, crop_h: int, crop_w: int) -> Tuple[int, int]:
    """torchvision's CenterCrop: Python's round (half to even) of half the excess."""
    return int(round((h - crop_h) / 2.0)), int(round((w - crop_w) / 2.0))


def bilinear_table(in_size: int, out_size: int, lo: int = 0, n: Optional[int] = None):
    """PIL's bilinear coefficients for output indices lo .. lo+n-1 of an in_size -> out_size resample:
    (first_tap[n], tap_count[n], k[n][ksize]) as int32, k in 22-bit fixed point (`0.5 + w * 2^22` truncated)."""
    n = out_size - lo if n is None else n
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    first = np.zeros(n, np.int32)
    count = np.zeros(n, np.int32)
    k = np.zeros((n, ksize), np.int32)
    for i in range(n):
        center = (lo + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(cnt)]
        ww = 0.0
        for v in w:                 # PIL's summation order
            ww += v
        first[i], count[i] = xmin, cnt
        for x, v in enumerate(w):
            k[i, x] = int(0.5 + (v / ww) * (1 << PRECISION_BITS))
    return first, count, k


# ------------------------------------------------------------------------------------------------------------------
# the uint8 batch
# ------------------------------------------------------------------------------------------------------------------
def _as_hwc_uint8(img, index: int) -> np.ndarray:
    """One decoded image as a uint8 numpy view [H, W, C] (no copy where the source allows)."""
    if isinstance(img, torch.Tensor):
        if img.is_cuda:
            raise ValueError(f"collate_uint8: image {index} is a device tensor; the collate packs host images")
        if img.dtype != torch.uint8:
            raise ValueError(f"collate_uint8: image {index} has dtype {img.dtype}, expected uint8")
        a = img.numpy()
    elif isinstance(img, np.ndarray):
        a = img
    else:
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None and isinstance(img, Image.Image):
            a = np.asarray(img)
        else:
            raise ValueError(f"collate_uint8: image {index} is a {type(img).__name__}; expected a PIL image, an array or a uint8 tensor")
    if a.dtype != np.uint8:
        raise ValueError(f"collate_uint8: image {index} has dtype {a.dtype}, expected uint8")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError(f"collate_uint8: image {index} has shape {a.shape}, expected [H, W, 3]")
    return a


class UInt8Batch:
    """A ragged batch of decoded RGB images in ONE byte buffer.

    data    uint8 1-D tensor (host, pinned when possible, or device)
    table   int64 [B, 5] host tensor: byte offset, height, width, row stride in bytes, channels
    labels  whatever the dataset returned next to each image (a tensor when they stack), or None
    """

    def __init__(self, data: torch.Tensor, table: torch.Tensor, labels=None):
        self.data, self.table, self.labels = data, table, labels

    def __len__(self):
        return int(self.table.shape[0])

    @property
    def device(self):
        return self.data.device

    def to(self, device, non_blocking: bool = False) -> "UInt8Batch":
        labels = self.labels.to(device, non_blocking=non_blocking) if isinstance(self.labels, torch.Tensor) else self.labels
        return UInt8Batch(self.data.to(device, non_blocking=non_blocking), self.table, labels)

    def cuda(self, device=None, non_blocking: bool = False) -> "UInt8Batch":
        return self.to("cuda" if device is None else device, non_blocking=non_blocking)

    def pin_memory(self) -> "UInt8Batch":       # DataLoader(pin_memory=True) calls this in its pinning thread
        return UInt8Batch(self.data.pin_memory(), self.table, self.labels)

    def image(self, i: int) -> torch.Tensor:
        """Image i as a uint8 [H, W, C] view of the buffer."""
        off, h, w, stride, c = (int(v) for v in self.table[i])
        return torch.as_strided(self.data, (h, w, c), (stride, c, 1), off)


def pack_uint8(images: Sequence, labels=None, pin: Optional[bool] = None, align: int = 1, row_pad: int = 0) -> UInt8Batch:
    """Pack host images into one buffer.  `align` (bytes) places every image start on a multiple of it and `row_pad` adds
    that many bytes to every row stride; the defaults pack tightly, so most starts are odd addresses."""
    arrs = [_as_hwc_uint8(im, i) for i, im in enumerate(images)]
    table = torch.zeros(len(arrs), 5, dtype=torch.int64)
    pos = 0
    for i, a in enumerate(arrs):
        h, w, c = a.shape
        pos = (pos + align - 1) // align * align
        stride = w * c + row_pad
        table[i] = torch.tensor([pos, h, w, stride, c])
        pos += h * stride
    if pin is None:
        from torch.utils.data import get_worker_info
        pin = get_worker_info() is None and torch.cuda.is_available()
    data = torch.zeros(max(pos, 1), dtype=torch.uint8)
    if pin:
        data = data.pin_memory()
    buf = data.numpy()
    for i, a in enumerate(arrs):
        off, h, w, stride, c = (int(v) for v in table[i])
        if h and w:
            np.lib.stride_tricks.as_strided(buf[off:], (h, w * c), (stride, 1))[...] = a.reshape(h, w * c)
    return UInt8Batch(data, table, labels)


def collate_uint8(batch, pin: Optional[bool] = None) -> UInt8Batch:
    """`collate_fn` for a DataLoader whose dataset returns decoded images (PIL images when PIL is importable, uint8 HWC
    arrays or tensors) or `(image, label)` pairs: the images of mixed sizes go into one byte buffer, the labels are kept
    (stacked into a tensor when they are numbers or tensors of one shape).  In a worker process the buffer is left unpinned --
    `DataLoader(pin_memory=True)` pins it through :meth:`UInt8Batch.pin_memory`."""
    batch = list(batch)
    if batch and isinstance(batch[0], (tuple, list)):
        images = [b[0] for b in batch]
        labels = [b[1] if len(b) > 1 else None for b in batch]
        try:
            labels = torch.as_tensor(labels) if not isinstance(labels[0], torch.Tensor) else torch.stack(labels)
        except Exception:
            pass
    else:
        images, labels = batch, None
    return pack_uint8(images, labels, pin=pin)


# ------------------------------------------------------------------------------------------------------------------
# inbound
# ------------------------------------------------------------------------------------------------------------------
class ImagePrep:
    """`Resize(resolution) -> CenterCrop(resolution) -> ToTensor()` on the device, bit-equal to PIL + torchvision.

    resolution  int (square crop) -- torchvision's Resize(int) size rule and CenterCrop's offsets
    range       "unit": [0, 1] (ToTensor);  "signed": x*2-1 in fp32 after the division (R/train_2.py:170)
    resize      (h, w): resize every image to exactly this size, no crop (`resolution` is then ignored)

    Calling it on a :class:`UInt8Batch` (on the device), a list of uint8 HWC device tensors / host arrays of mixed sizes, or a
    dense uint8 `[B, H, W, 3]` device tensor returns the fp32 `[B, 3, res, res]` device tensor in one launch on the current stream.
    """

    def __init__(self, resolution: Optional[int] = None, range: str = "unit", resize: Optional[Tuple[int, int]] = None):
        if range not in _RANGES:
            raise ValueError(f"ImagePrep: unknown range {range!r} (expected one of {list(_RANGES)})")
        if resize is not None:
            resize = (int(resize[0]), int(resize[1]))
            if resize[0] <= 0 or resize[1] <= 0:
                raise ValueError(f"ImagePrep: resize must be a positive (h, w), got {resize}")
        elif resolution is None or int(resolution) <= 0:
            raise ValueError(f"ImagePrep: resolution must be a positive int, got {resolution!r}")
        self.resolution = None if resolution is None else int(resolution)
        self.range, self.resize = range, resize
        lut = torch.arange(256, dtype=torch.float32) / 255.0           # IEEE float(v) / 255.0f, ToTensor's value
        self._lut_host = lut * 2 - 1 if range == "signed" else lut
        self._coef = np.zeros(0, np.int32)      # every table built so far, back to back
        self._tables = {}                        # (in, out, lo, n) -> (offset, ksize)
        self._dev = {}                           # device -> (lut, coef tensor, coef length)

    # -- geometry --------------------------------------------------------------------------------------------------
    def output_size(self) -> Tuple[int, int]:
        return self.resize if self.resize is not None else (self.resolution, self.resolution)

    def geometry(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """(out_h, out_w, crop_top, crop_left) of an h x w source."""
        if self.resize is not None:
            return self.resize[0], self.resize[1], 0, 0
        oh, ow = resize_size(h, w, self.resolution)
        top, left = center_crop_offsets(oh, ow, self.resolution, self.resolution)
        return oh, ow, top, left

    def _table(self, in_size: int, out_size: int, lo: int, n: int) -> Tuple[int, int]:
        key = (in_size, out_size, lo, n)
        hit = self._tables.get(key)
        if hit is None:
            first, count, k = bilinear_table(in_size, out_size, lo, n)
            hit = (int(self._coef.size), int(k.shape[1]))
            self._coef = np.concatenate([self._coef, first, count, k.reshape(-1)]).astype(np.int32)
            self._tables[key] = hit
        return hit

    def describe(self, table: torch.Tensor):
        """The tv_image_desc array for the rows (offset, h, w, row stride, channels) of `table`; raises ValueError naming the
        first image outside the supported set."""
        rh, rw = self.output_size()
        descs = (L.ImageDesc * len(table))()
        for i, row in enumerate(table.tolist()):
            off, h, w, stride, c = row
            if c != 3:
                raise ValueError(f"ImagePrep: image {i} has {c} channels; only 3-channel (RGB) images are supported")
            if h <= 0 or w <= 0:
                raise ValueError(f"ImagePrep: image {i} is empty ({h}x{w})")
            oh, ow, top, left = self.geometry(h, w)
            if h > MAX_RATIO * oh or w > MAX_RATIO * ow:
                raise ValueError(f"ImagePrep: image {i}: {h}x{w} -> {oh}x{ow} is a down-scale by more than {MAX_RATIO}, which is not supported")
            if oh < rh or ow < rw:
                raise ValueError(f"ImagePrep: image {i}: resized {oh}x{ow} is smaller than the {rh}x{rw} crop")
            xtab, xk = self._table(w, ow, left, rw) if ow != w else (-1, 0)
            ytab, yk = self._table(h, oh, top, rh) if oh != h else (-1, 0)
            descs[i] = L.ImageDesc(off, h, w, stride, c, oh, ow, top, left, xtab, xk, ytab, yk)
        return descs

    # -- input forms -----------------------------------------------------------------------------------------------
    def _gather(self, images) -> Tuple[torch.Tensor, torch.Tensor]:
        """(byte buffer, host table) of any accepted input; the buffer is on the device except for packed host arrays."""
        if isinstance(images, UInt8Batch):
            ops._need_gpu(images.data)
            return images.data, images.table
        if isinstance(images, torch.Tensor):
            ops._need_gpu(images)
            if images.dtype != torch.uint8 or images.dim() != 4:
                raise ValueError(f"ImagePrep: a dense batch must be uint8 [B, H, W, 3], got {images.dtype} {tuple(images.shape)}")
            B, H, W, Cn = images.shape
            if not (images.stride(3) == 1 and images.stride(2) == Cn and images.stride(1) >= W * Cn and images.stride(0) >= 0):
                images = images.contiguous()
            table = torch.tensor([[b * images.stride(0), H, W, images.stride(1), Cn] for b in range(B)], dtype=torch.int64).reshape(B, 5)
            span = (B - 1) * images.stride(0) + (H - 1) * images.stride(1) + W * Cn if B and H and W else 0
            return torch.as_strided(images, (max(span, 1),), (1,)) if span else images.reshape(-1), table
        if isinstance(images, (list, tuple)):
            if not images:
                raise ValueError("ImagePrep: empty batch")
            if all(isinstance(im, torch.Tensor) for im in images):
                ops._need_gpu(*images)
                rows, parts, pos = [], [], 0
                for i, im in enumerate(images):
                    if im.dtype != torch.uint8 or im.dim() != 3:
                        raise ValueError(f"ImagePrep: image {i} must be uint8 [H, W, 3], got {im.dtype} {tuple(im.shape)}")
                    h, w, c = im.shape
                    rows.append([pos, h, w, w * c, c])
                    parts.append(im.reshape(-1) if im.is_contiguous() else im.contiguous().reshape(-1))
                    pos += h * w * c
                return torch.cat(parts), torch.tensor(rows, dtype=torch.int64)
            if any(isinstance(im, torch.Tensor) for im in images):
                raise ValueError("ImagePrep: a list must hold either device tensors or host arrays, not both")
            batch = pack_uint8(images)       # host arrays / PIL images: one buffer, uploaded once by __call__
            return batch.data, batch.table
        raise ValueError(f"ImagePrep: cannot take a {type(images).__name__}")

    def _device_state(self, dev: torch.device):
        st = self._dev.get(dev)
        if st is None or st[2] != self._coef.size:
            lut = st[0] if st is not None else self._lut_host.to(dev)
            coef = torch.from_numpy(self._coef.copy()).to(dev) if self._coef.size else torch.zeros(1, dtype=torch.int32, device=dev)
            st = (lut, coef, int(self._coef.size))
            self._dev[dev] = st
        return st

    def __call__(self, images) -> torch.Tensor:
        data, table = self._gather(images)
        if len(table) == 0:
            raise ValueError("ImagePrep: empty batch")
        descs = self.describe(table)
        if not data.is_cuda:                 # only the packed host arrays get here: tensors were checked in _gather
            if not torch.cuda.is_available():
                raise RuntimeError("transvae.hip: this op only runs on a HIP device (MI355X); there is no CPU fallback")
            data = data.to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
        B = len(table)
        rh, rw = self.output_size()
        dev = data.device
        with torch.cuda.device(dev), torch.no_grad():
            lut, coef_dev, coef_len = self._device_state(dev)
            host = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
            if torch.cuda.is_available():
                host = host.pin_memory()
            desc_dev = host.to(dev, non_blocking=True)
            out = torch.empty(B, 3, rh, rw, device=dev, dtype=torch.float32)
            coef_host = self._coef.ctypes.data_as(C.c_void_p) if coef_len else None
            rc = L.load().tv_image_prep(ops._p(data), data.numel(), C.cast(descs, C.c_void_p), ops._p(desc_dev), B, coef_host,
                                        ops._p(coef_dev), coef_len, ops._p(lut), ops._p(out), rh, rw, ops._stream())
            if rc == L.ERR_UNSUPPORTED:
                raise ValueError("ImagePrep: " + L.load().tv_last_error().decode(errors="replace"))
            L.check(rc, "tv_image_prep")
        return out


# ------------------------------------------------------------------------------------------------------------------
# outbound
# ------------------------------------------------------------------------------------------------------------------
def grid_geometry(B: int, H: int, W: int, nrow: int = 8, padding: int = 2) -> Tuple[int, int, int, int]:
    """torchvision's make_grid layout: (grid height, grid width, xmaps, ymaps); a batch of one has no border."""
    if B == 1:
        return H, W, 1, 1
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding, xmaps, ymaps


def to_uint8_grid(images: torch.Tensor, nrow: int = 8, padding: int = 2, pad_value: float = 0, transform: str = "none") -> torch.Tensor:
    """`make_grid(images, nrow, padding, pad_value)` followed by `save_image`'s quantisation (x*255, +0.5, clamp, truncate; NaN
    gives 0), one launch: fp32 `[B, 3, H, W]` (or `[3, H, W]`) of any strides -> uint8 `[Hg, Wg, 3]` on the same device.
    transform="sigmoid" applies a sigmoid first, as the patched scripts do before writing."""
    if transform not in _TRANSFORMS:
        raise ValueError(f"to_uint8_grid: unknown transform {transform!r} (expected one of {sorted(_TRANSFORMS)})")
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[1] != 3 or images.numel() == 0:
        raise ValueError(f"to_uint8_grid: images must be a non-empty [B, 3, H, W], got {tuple(images.shape)}")
    if int(nrow) <= 0 or int(padding) < 0:
        raise ValueError(f"to_uint8_grid: nrow must be positive and padding non-negative, got {nrow} and {padding}")
    ops._need_gpu(images)
    with torch.cuda.device(images.device), torch.autocast("cuda", enabled=False), torch.no_grad():
        x = images.detach().float()
        B, _, H, W = x.shape
        Hg, Wg, _, _ = grid_geometry(B, H, W, int(nrow), int(padding))
        out = torch.empty(Hg, Wg, 3, device=x.device, dtype=torch.uint8)
        L.check(L.load().tv_image_grid_u8(ops._p(x), *x.stride(), ops._p(out), B, H, W, int(nrow), int(padding), C.c_float(pad_value),
                                          _TRANSFORMS[transform], ops._stream()), "tv_image_grid_u8")
    return out


def encode_png(rgb: np.ndarray) -> bytes:
    """An 8-bit RGB PNG of a uint8 [H, W, 3] array: zlib + struct only, filter 0 on every row."""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.size == 0:
        raise ValueError(f"encode_png: expected a non-empty uint8 [H, W, 3] array, got {rgb.dtype} {rgb.shape}")
    h, w, _ = rgb.shape
    raw = np.zeros((h, 1 + 3 * w), np.uint8)       # a filter-type byte (0 = none) in front of every row
    raw[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(tag: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def save_image(images_or_grid: torch.Tensor, path, **grid_kw) -> None:
    """Write a PNG: a uint8 `[Hg, Wg, 3]` grid as it is, or fp32 images through :func:`to_uint8_grid` with `grid_kw`
    (torchvision's `save_image(tensor, path, nrow=..., padding=...)`)."""
    t = images_or_grid
    if not (t.dtype == torch.uint8 and t.dim() == 3 and t.shape[-1] == 3):
        t = to_uint8_grid(t, **grid_kw)
    elif grid_kw:
        raise ValueError(f"save_image: a uint8 grid is written as it is; unexpected arguments {sorted(grid_kw)}")
    data = encode_png(t.detach().cpu().numpy())
    with open(path, "wb") as f:
        f.write(data)
