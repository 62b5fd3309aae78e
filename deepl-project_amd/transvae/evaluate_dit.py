"""gFID, Inception Score and precision / recall of a latent DiT: the last step of the reference's latent-generator pipeline
(`evaluate_dit.py --num_samples 10000 --batch_size 128`, "Evaluate FID"), which the reference leaves as a TODO.

The loop: labels -> `sample_images` (Euler steps with classifier-free guidance, decode through the autoencoder) ->
`InceptionFeatures.features(clip=True)` -> streaming statistics on the device.  The real side comes from
`transvae.metrics_gen.reference_statistics`, computed once per data set.  Protocol: DESIGN.md section 3.5."""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from .dit import DiT, sample_images
from .hip import ops
from .metrics_fid import SPATIAL_DIM, SPATIAL_LD, FrechetDistance, frechet_from_statistics
from .metrics_gen import (MAX_K, InceptionScore, _density_coverage_device, _kid_device, _precision_recall_device, score_from_state,
                          scores_from_states)
from .metrics_gen import kid_subsets as _kid_subsets

METRICS = ("gfid", "is", "precision", "recall")
ALL_METRICS = ("gfid", "sfid", "is", "precision", "recall", "kid", "density", "coverage")


def _load_reference(reference) -> Dict:
    if isinstance(reference, (str, bytes)) or hasattr(reference, "__fspath__"):
        reference = torch.load(reference, map_location="cpu")
    if not isinstance(reference, dict) or not all(k in reference for k in ("n", "mean", "cov")):
        raise ValueError("evaluate_dit: reference must be a reference_statistics dict (keys n, mean, cov, features) or a path to one")
    return reference


@torch.no_grad()
def evaluate_dit(vae, dit: DiT, reference: Union[Dict, str], *, fid_net, num_samples: int = 10000, batch_size: int = 128, steps: int = 50,
                 cfg_scale: float = 1.0, metrics: Sequence[str] = METRICS, is_head: Optional[InceptionScore] = None, k: int = 3,
                 seed: int = 0, labels: Optional[torch.Tensor] = None, ema=None, transform: str = "clip", max_features: int = 10000,
                 return_features: bool = False, stats=None, method: str = "euler", timestep_shift: float = 1.0,
                 cfg_interval=(0.0, 1.0), is_split_size: Optional[int] = None, prdc_k: int = 5, kid_subsets: int = 100,
                 kid_subset_size: int = 1000, kid_seed: int = 0) -> Dict:
    """{"gfid", "is", "precision", "recall", "n"} (restricted to `metrics`) of `num_samples` images sampled from `dit`.
    `metrics` may also name "sfid", "kid" (which adds "kid_std"), "density" and "coverage"; ALL_METRICS lists every name.

    Sample i has label i % dit.num_classes unless `labels` [num_samples] is given; the noise comes batch by batch from a device
    generator seeded with `seed`; sampling is `sample_images(vae, dit, ..., steps, cfg_scale)` (with `method`, `timestep_shift` and
    `cfg_interval` handed to `sample_latents`, which validates them before the first launch) with the model in eval mode, under
    `ema.applied(dit)` when a `ParamEMA` is handed in.  `stats` is the `latents_stats.pt` dict (or a (mean, std) pair) that
    de-normalises the sampled latents; None: mean 0, std 1.  transform="clip" feeds the decoder's output to
    `fid_net.features(img, clip=True)` as `evaluate` does for rFID; "sigmoid" applies a sigmoid first, as generate.py does.
    gFID is the Frechet distance between the reference's (mean, cov) and the streamed statistics of all fake features; "is" needs
    `is_head` and covers all of them; precision / recall use the reference's stored features against the first `max_features`
    fake ones with k-NN radius `k`.  The loop adds no host synchronisation of its own: the statistics, the score state, the hit
    counts and a per-batch finiteness flag of the features stay on the device and are read back after the last batch (four small
    copies).  `sample_latents` checks its labels on the host, which synchronises once per batch.  `is_head` is an accumulator:
    it is reset at the start and holds this run's state afterwards.  return_features adds "features" (fp32 [num_samples, d],
    device).

    "sfid" is the Frechet distance on the spatial rows of `fid_net.features(..., spatial=True)` (2023 values per image) against the
    reference's "spatial_mean" / "spatial_cov" (`reference_statistics(..., spatial=True)`); with return_features it adds "spatial"
    (fp32 [num_samples, 2048], the last 25 columns zero).  "kid" is `kernel_inception_distance` between the reference's stored
    features and the first `max_features` fake ones with `kid_subsets`, `kid_subset_size` and `kid_seed` (both sides must hold `kid_subset_size` rows: the subsets are not clamped
    here, as they are in the stand-alone function); "density" / "coverage" are
    `density_coverage` on the same rows with `prdc_k`.  `is_split_size` cuts the samples into consecutive splits of that many for
    "is", which then is the mean of the per-split scores, with "is_std" beside it (`is_head` keeps the split size afterwards)."""
    metrics = tuple(metrics)
    unknown = [m for m in metrics if m not in ALL_METRICS]
    if unknown or not metrics:
        raise ValueError(f"evaluate_dit: metrics has unknown names {unknown} (expected a non-empty subset of {list(ALL_METRICS)})")
    if "is" in metrics and is_head is None:
        raise ValueError("evaluate_dit: metrics asks for 'is', which needs is_head=InceptionScore.from_file(...): the classifier "
                         "head of the FID Inception-v3, which this package neither ships nor fetches")
    if transform not in ("clip", "sigmoid"):
        raise ValueError(f"evaluate_dit: transform={transform!r} must be 'clip' or 'sigmoid'")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"evaluate_dit: k={k} must be in [1, {MAX_K}]")
    if not 1 <= int(prdc_k) <= MAX_K:
        raise ValueError(f"evaluate_dit: prdc_k={prdc_k} must be in [1, {MAX_K}]")
    if is_split_size is not None and int(is_split_size) < 1:
        raise ValueError(f"evaluate_dit: is_split_size={is_split_size} must be positive (or None: one score over the whole set)")
    num_samples, batch_size, k, prdc_k = int(num_samples), int(batch_size), int(k), int(prdc_k)
    want_pr = "precision" in metrics or "recall" in metrics
    want_dc = "density" in metrics or "coverage" in metrics
    want_kid, want_sfid = "kid" in metrics, "sfid" in metrics
    want_rows = want_pr or want_dc or want_kid                  # metrics on the stored feature rows of both sides
    if num_samples < 2 or (want_pr and num_samples < k + 1):
        raise ValueError(f"evaluate_dit: num_samples={num_samples} must be at least 2, and at least k + 1 = {k + 1} for precision / recall")
    if batch_size < 1 or int(steps) < 1 or int(max_features) < 1:
        raise ValueError("evaluate_dit: batch_size, steps and max_features must be positive")
    reference = _load_reference(reference)
    ref_mean = np.asarray(torch.as_tensor(reference["mean"]).double().cpu().numpy()).reshape(-1)
    ref_cov = np.asarray(torch.as_tensor(reference["cov"]).double().cpu().numpy())
    ref_feats = reference.get("features")
    if ref_feats is not None:
        ref_feats = torch.as_tensor(ref_feats)
    if want_sfid:
        if not all(key in reference for key in ("spatial_mean", "spatial_cov")):
            raise ValueError("evaluate_dit: metrics asks for 'sfid', but the reference holds no spatial statistics; build it with "
                             "reference_statistics(..., spatial=True)")
        sp_mean = np.asarray(torch.as_tensor(reference["spatial_mean"]).double().cpu().numpy()).reshape(-1)
        sp_cov = np.asarray(torch.as_tensor(reference["spatial_cov"]).double().cpu().numpy())
        if sp_mean.shape[0] != SPATIAL_DIM or sp_cov.shape != (SPATIAL_DIM, SPATIAL_DIM):
            raise ValueError(f"evaluate_dit: the reference's spatial statistics must be {SPATIAL_DIM} wide, got {sp_mean.shape[0]}")
    if want_dc or want_kid:
        need = prdc_k + 1 if want_dc else 2
        if ref_feats is None or ref_feats.dim() != 2 or ref_feats.shape[0] < need:
            raise ValueError(f"evaluate_dit: reference holds no features (at least {need} rows), which kid / density / coverage need; "
                             "build it with reference_statistics(..., max_features > 0)")
        if want_kid:                                             # the draw's own argument checks, before the first launch
            # a KID over clamped subsets is another statistic than the one asked for; the stand-alone
            # kernel_inception_distance clamps, a whole evaluation does not do so silently
            have = min(ref_feats.shape[0], num_samples, int(max_features))
            if have < int(kid_subset_size):
                raise ValueError(f"evaluate_dit: metrics has names ['kid'] that need kid_subset_size={int(kid_subset_size)} rows on either "
                                 f"side, but the reference holds {ref_feats.shape[0]} features and {min(num_samples, int(max_features))} fake "
                                 "ones are kept; lower kid_subset_size, or raise num_samples / max_features")
            kid_draw = _kid_subsets(ref_feats.shape[0], min(num_samples, int(max_features)), kid_subsets, kid_subset_size, kid_seed)
    if want_pr:
        if ref_feats is None or ref_feats.dim() != 2 or ref_feats.shape[0] < k + 1:
            raise ValueError(f"evaluate_dit: reference holds no features (at least k + 1 = {k + 1} rows), which precision / recall need; "
                             "build it with reference_statistics(..., max_features > 0)")
    dev = next(dit.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("transvae.hip: this op only runs on a HIP device (MI355X); there is no CPU fallback")
    if labels is None:
        labels = torch.arange(num_samples, device=dev) % dit.num_classes
    else:
        ops._need_gpu(labels)
        if tuple(labels.shape) != (num_samples,):
            raise ValueError(f"evaluate_dit: labels must be [{num_samples}], got {tuple(labels.shape)}")
    if stats is None:
        stats = (torch.zeros(dit.in_channels, device=dev), torch.ones(dit.in_channels, device=dev))
    width = None
    with torch.cuda.device(dev), (ema.applied(dit) if ema is not None else contextlib.nullcontext()):
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        frechet, feats_all, bad = None, [], []
        sfrechet, rows_all = (FrechetDistance(SPATIAL_LD) if want_sfid else None), []
        if is_head is not None and "is" in metrics:
            if is_split_size is not None:
                is_head.split_size = int(is_split_size)
            is_head.reset()
        for i0 in range(0, num_samples, batch_size):
            img = sample_images(vae, dit, labels[i0:i0 + batch_size], steps=int(steps), cfg_scale=float(cfg_scale), generator=gen, stats=stats,
                                method=method, timestep_shift=timestep_shift, cfg_interval=cfg_interval)
            img = img.float()
            if transform == "sigmoid":
                img = torch.sigmoid(img)
            if want_sfid:
                feats, rows = fid_net.features(img, clip=True, spatial=True)
                sfrechet.update(None, rows)
                if return_features:
                    rows_all.append(rows)
            else:
                feats = fid_net.features(img, clip=True)
            if width is None:
                width = feats.shape[1]
                if width != ref_mean.shape[0] or ref_cov.shape != (width, width) or (want_rows and ref_feats.shape[1] != width):
                    raise ValueError(f"evaluate_dit: reference has feature width {ref_mean.shape[0]}, fid_net gives {width}")
                if "is" in metrics and is_head.dims != width:
                    raise ValueError(f"evaluate_dit: is_head takes feature width {is_head.dims}, fid_net gives {width}")
                frechet = FrechetDistance(width)
            bad.append(~torch.isfinite(feats).all())
            frechet.update(None, feats)
            if "is" in metrics:
                is_head.update(feats)
            if want_rows or return_features:
                feats_all.append(feats)
        fake = torch.cat(feats_all) if feats_all else None
        pr = dc = kid = None
        if want_rows:
            real_dev = ref_feats.to(device=dev, dtype=torch.float32)
        if want_pr:
            pr = torch.stack(_precision_recall_device(real_dev, fake[:int(max_features)], k))
        if want_dc:
            dc = torch.stack(_density_coverage_device(real_dev, fake[:int(max_features)], prdc_k))
        if want_kid:
            kid = _kid_device(real_dev, fake[:int(max_features)], kid_draw)
        # the first read-back of this loop; the statistics, the score state and the hit counts follow below
        bad = torch.stack(bad).cpu().tolist()
    if any(bad):
        b = bad.index(True)
        raise RuntimeError(f"evaluate_dit: non-finite Inception features in samples {b * batch_size} .. "
                           f"{min(num_samples, (b + 1) * batch_size) - 1} (batch {b})")
    out = {}
    if "gfid" in metrics:
        _, mu, cov = frechet.statistics(1)
        out["gfid"] = frechet_from_statistics(ref_mean, ref_cov, mu, cov)
    if want_sfid:
        _, mu, cov = sfrechet.statistics(1)
        out["sfid"] = frechet_from_statistics(sp_mean, sp_cov, mu[:SPATIAL_DIM], cov[:SPATIAL_DIM, :SPATIAL_DIM])
    if "is" in metrics and is_head.split_size is not None:
        scores = scores_from_states(is_head.state().cpu().numpy())
        out["is"], out["is_std"] = float(scores.mean()), float(scores.std())
    elif "is" in metrics:
        out["is"] = score_from_state(is_head.state().cpu().numpy())
    if pr is not None:
        p, r = pr.cpu().tolist()
        if "precision" in metrics:
            out["precision"] = p
        if "recall" in metrics:
            out["recall"] = r
    if dc is not None:
        dens, cover = dc.cpu().tolist()
        if "density" in metrics:
            out["density"] = dens
        if "coverage" in metrics:
            out["coverage"] = cover
    if kid is not None:
        out["kid"], out["kid_std"] = kid.cpu().tolist()
    out["n"] = num_samples
    if return_features:
        out["features"] = fake
        if want_sfid:
            out["spatial"] = torch.cat(rows_all)
    return out
