"""Drop-in for the reference's evaluation loop, R/evaluate.py:69-144 (`evaluate(model, dataloader, metrics, device)`).

The reference copies every batch to the host and runs skimage one image at a time; here the per-image values come from
:func:`transvae.metrics.reconstruction_metrics` on the device (the reference's definitions: inputs clipped to [0, 1],
skimage's 7x7 SSIM, data_range 1), stay there while the loop runs and reach the host once, at the end.  LPIPS follows
R/evaluate.py:126-133: `lpips(images * 2 - 1, reconstruction * 2 - 1)` on the UNCLIPPED tensors, original first, from the
`PerceptualLoss` handed in as `lpips_net`.  rFID (the `rfid` of the reference's configs) is the Frechet distance between the
FID Inception-v3 features of the originals and of the reconstructions, both clipped to [0, 1], from the `InceptionFeatures`
handed in as `fid_net`; the feature statistics stream through a `FrechetDistance` on the device (transvae/metrics_fid.py).
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from .metrics import reconstruction_metrics

_KNOWN = ("psnr", "ssim", "mse")


def _uint8_images(batch, device):
    """The images of one batch of a uint8 loader, on the device: a tuple is (images, labels); a list of two whose first entry
    is itself a batch (UInt8Batch, list or 4-D tensor) is the default collate's form of such a tuple; any other list is the
    images themselves."""
    from .image_io import UInt8Batch
    if isinstance(batch, tuple):
        batch = batch[0]
    elif isinstance(batch, list) and len(batch) == 2 and (isinstance(batch[0], (UInt8Batch, list))
                                                          or (isinstance(batch[0], torch.Tensor) and batch[0].dim() == 4)):
        batch = batch[0]
    if isinstance(batch, (UInt8Batch, torch.Tensor)):
        return batch.to(device, non_blocking=True)
    if isinstance(batch, list):
        return [im.to(device, non_blocking=True) if isinstance(im, torch.Tensor) else im for im in batch]
    return batch


def evaluate(model: torch.nn.Module, dataloader: Iterable, metrics: Sequence[str] = ("psnr", "ssim"),
             device="cuda", per_image: bool = False, lpips_net: Optional[torch.nn.Module] = None,
             fid_net: Optional[torch.nn.Module] = None, prep=None) -> Dict[str, Dict]:
    """{metric: {"mean", "std", "median"}} over every image of `dataloader`, like R/evaluate.py.

    `dataloader` yields `(images, labels)` pairs as in the reference (a bare image tensor is accepted too).  The model runs
    in eval mode under no_grad as `model(images)`, so z is sampled as in the reference.  Metrics: "psnr", "ssim" and "mse"
    (P/evaluate_transvae.py:134).  The statistics are NumPy's over the per-image values taken as float64 (`np.std` is the
    population standard deviation).  "lpips" needs `lpips_net`, a `transvae.PerceptualLoss` with loaded weights on `device`
    (the package ships none); without one it raises ValueError.  per_image=True (not in the reference) adds each metric's
    per-image values, in loader order, as a float64 array under "values".  "rfid" needs `fid_net`, a
    `transvae.InceptionFeatures` with loaded weights on `device`; it is a property of the whole set, so its entry is
    {"value", "n"} (n images per side) and per_image adds nothing to it.

    `prep` (a `transvae.image_io.ImagePrep`): the loader yields decoded uint8 images -- a `UInt8Batch` (from `collate_uint8`), a
    list of uint8 HWC images of mixed sizes or a dense uint8 [B, H, W, 3] tensor, bare or as the first element of an
    `(images, labels)` tuple -- and each batch goes through `prep` on the device before the model, replacing the reference's
    per-image `Resize -> CenterCrop -> ToTensor` on the host (R/evaluate.py:39-42).  The reference's 256 / 512 / 1024 benchmark is
    then three calls over one uint8 loader.  Without `prep` nothing changes.
    """
    metrics = tuple(metrics)
    if "lpips" in metrics and lpips_net is None:
        raise ValueError("evaluate (HIP path): the LPIPS term needs the external VGG network's weights, which this package neither "
                         "ships nor fetches; pass lpips_net=PerceptualLoss.from_file(...) or drop 'lpips' from metrics")
    if "rfid" in metrics and fid_net is None:
        raise ValueError("evaluate (HIP path): rFID needs the FID Inception-v3 weights, which this package neither ships nor "
                         "fetches; pass fid_net=InceptionFeatures.from_file(...) or drop 'rfid' from metrics")
    unknown = [m for m in metrics if m not in _KNOWN and m not in ("lpips", "rfid")]
    if unknown or not metrics:
        raise ValueError(f"evaluate: unknown metrics {unknown} (expected a non-empty subset of {list(_KNOWN) + ['lpips', 'rfid']})")
    model.eval()
    frechet = None
    if "rfid" in metrics:
        from .metrics_fid import FrechetDistance
        frechet = FrechetDistance()
    metrics_all, metrics = metrics, tuple(m for m in metrics if m != "rfid")
    values = {m: [] for m in metrics}
    with torch.no_grad():
        for batch in dataloader:
            if prep is not None:
                images = prep(_uint8_images(batch, device))
            else:
                images = batch[0] if isinstance(batch, (tuple, list)) else batch
                images = images.to(device)
            reconstruction = model(images)[0]
            batch_values = {}
            if any(m in _KNOWN for m in metrics):
                batch_values = reconstruction_metrics(reconstruction, images, ssim_window="skimage", transform="clip", data_range=1.0)
            if "lpips" in metrics:
                batch_values["lpips"] = lpips_net(images, reconstruction, normalize=True).reshape(-1)
            if frechet is not None:      # originals and reconstructions as one batch of 2B
                nb = images.shape[0]
                feats = fid_net.features(images, reconstruction, clip=True)
                frechet.update(feats[:nb], feats[nb:])
            for m in metrics:
                values[m].append(batch_values[m])
    results = {}
    for m in metrics:
        v = torch.cat(values[m]).cpu().numpy().astype(np.float64) if values[m] else np.zeros(0)
        results[m] = {"mean": float(np.mean(v)), "std": float(np.std(v)), "median": float(np.median(v))}
        if per_image:
            results[m]["values"] = v
    if frechet is not None:
        results["rfid"] = {"value": frechet.compute(), "n": frechet.n[0]}
        results = {m: results[m] for m in metrics_all}
    return results
