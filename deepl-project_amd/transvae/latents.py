"""Latent extraction for a downstream generator and latent-space density metrics, on the device.

`LatentStats` streams count, mean and centred scatter of every (image, position) sample of the encoder's latents in fp64
(`tv_latent_stats`, csrc/latent.hip).  `extract_latents` runs `model.encode` over a loader, writes `torch.save` shards of the
latents (and of the latents of the mirrored images) and `latents_stats.pt` with the per-channel mean / std a LightningDiT-style
trainer normalises by.  `latent_density_metrics` is the "Density CV, Normalized Entropy, Gini" table of the reference's
documentation (names only there; the definitions are ours): a Gaussian kernel density estimate over the
latent points in the log domain (`tv_kde_logdensity`), then three scale-free dispersion measures of the per-point densities.
There is no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, Optional, Union

import torch

from .hip import _lib as L
from .hip import ops

MAX_DIM = 64                      # tv_latent_stats / tv_kde_logdensity: channels / coordinates at most
_LS_HDR, _LS_MAXG, _LS_CHUNK = 192, 256, 512
_KDE_SPLIT_BELOW, _KDE_SPLIT_MAX = 2048, 64


class LatentStats:
    """Streaming per-channel statistics of latents [B, dim, h, w] over all (image, position) samples, fp64 on the device."""

    def __init__(self, dim: int):
        if not 1 <= int(dim) <= MAX_DIM:
            raise ValueError(f"LatentStats: dim={dim} must be in [1, {MAX_DIM}]")
        self.dim = int(dim)
        self._state: Optional[torch.Tensor] = None
        self._n = 0

    def update(self, latents: torch.Tensor) -> None:
        """Merge fp32 latents [B, dim, h, w] (or [B, dim, P]); a channel slice of a wider tensor is read in place."""
        if latents.dim() not in (3, 4) or latents.shape[1] != self.dim:
            raise ValueError(f"LatentStats.update: expected [B, {self.dim}, h, w], got {tuple(latents.shape)}")
        ops._need_gpu(latents)
        ops._require(latents.dtype == torch.float32, "LatentStats.update: fp32 latents")
        B, P = latents.shape[0], int(math.prod(latents.shape[2:]))
        if B == 0 or P == 0:
            return
        x = latents
        inner_ok = x.stride(-1) == 1 and (x.dim() == 3 or x.stride(2) == x.shape[3])
        if not (inner_ok and x.stride(1) >= P and x.stride(0) >= (self.dim - 1) * x.stride(1) + P):
            x = x.contiguous()
        lib = L.load()
        with torch.cuda.device(x.device):
            if self._state is None:
                self._state = torch.zeros(1 + self.dim + self.dim * self.dim, dtype=torch.float64, device=x.device)
            ops._require(self._state.device == x.device, "LatentStats.update: latents moved to another device")
            groups = min(_LS_MAXG, -(-(B * P) // _LS_CHUNK))
            scratch = torch.empty(_LS_HDR + groups * self.dim * self.dim, dtype=torch.float64, device=x.device)
            L.check(lib.tv_latent_stats(ops._p(x), x.stride(0), x.stride(1), B, self.dim, P, ops._p(self._state), ops._p(scratch),
                                        ops._stream()), "tv_latent_stats")
        self._n += B * P

    @property
    def n(self) -> int:
        return self._n

    def _need(self, k: int):
        if self._n < k:
            raise ValueError(f"LatentStats: {self._n} sample(s); this statistic needs at least {k}")

    @property
    def mean(self) -> torch.Tensor:
        """[dim] fp64, on the device."""
        self._need(1)
        return self._state[1:1 + self.dim].clone()

    @property
    def cov(self) -> torch.Tensor:
        """[dim, dim] fp64 population covariance (scatter / n), on the device."""
        self._need(1)
        return self._state[1 + self.dim:].reshape(self.dim, self.dim) / self._n

    @property
    def std(self) -> torch.Tensor:
        """[dim] fp64 population standard deviation, on the device."""
        return self.cov.diagonal().clamp_min(0).sqrt()

    def state_dict(self) -> Dict:
        return {"dim": self.dim, "n": self._n, "state": None if self._state is None else self._state.detach().cpu().clone()}

    def load_state_dict(self, sd: Dict, device="cuda") -> None:
        if int(sd["dim"]) != self.dim:
            raise ValueError(f"LatentStats.load_state_dict: dim {sd['dim']} != {self.dim}")
        self._n = int(sd["n"])
        self._state = None if sd["state"] is None else sd["state"].to(device=device, dtype=torch.float64).clone()


def _unpack(batch, device, prep):
    """(images on the device, labels or None) of one loader batch: the batch conventions of `evaluate()`."""
    from .evaluate import _uint8_images
    labels = batch[1] if isinstance(batch, (tuple, list)) and len(batch) == 2 and isinstance(batch[1], torch.Tensor) \
        and batch[1].dim() <= 1 else None
    if prep is not None:
        return prep(_uint8_images(batch, device)), labels
    images = batch[0] if isinstance(batch, (tuple, list)) else batch
    return images.to(device), labels


def extract_latents(model: torch.nn.Module, dataloader: Iterable, out_dir: str, *, flip: bool = True, what: str = "mean", prep=None,
                    shard_size: int = 8192, device="cuda") -> LatentStats:
    """Encode every image of `dataloader` and write `out_dir/latents_shard{k:03d}.pt` + `out_dir/latents_stats.pt`.

    A shard is a `torch.save` dict: "latents" fp32 [n, C, h, w], "latents_flip" (flip=True: the latents of the horizontally
    mirrored IMAGES; a batch and its mirror go through the encoder as one batch of 2B), "labels" int64 [n] when the loader
    yields them.  what="mean": C = latent_dim, the posterior mean; what="moments": C = 2 latent_dim, cat([mu, logvar], 1).
    `latents_stats.pt`: "mean", "std" fp32 [1, D, 1, 1] and "cov" fp64 [D, D] over every position of the unflipped mu
    (population statistics), plus "n".  `prep` and uint8 batches as in `evaluate()`.  Returns the `LatentStats`."""
    if what not in ("mean", "moments"):
        raise ValueError(f"extract_latents: what={what!r} (expected 'mean' or 'moments')")
    if shard_size < 1:
        raise ValueError("extract_latents: shard_size must be positive")
    os.makedirs(out_dir, exist_ok=True)
    model.eval()
    stats = None
    pend = {"latents": [], "latents_flip": [], "labels": []}
    count, shard = 0, 0

    def flush(n_take):
        nonlocal count, shard
        out = {}
        for key, lst in pend.items():
            if not lst:
                continue
            full = torch.cat(lst)
            out[key], rest = full[:n_take].clone(), full[n_take:]
            pend[key] = [rest] if rest.shape[0] else []
        torch.save(out, os.path.join(out_dir, f"latents_shard{shard:03d}.pt"))
        shard += 1
        count -= n_take

    with torch.no_grad():
        for batch in dataloader:
            images, labels = _unpack(batch, device, prep)
            nb = images.shape[0]
            both = torch.cat([images, torch.flip(images, dims=[3])]) if flip else images
            mu, logvar = model.encode(both)
            if stats is None:
                stats = LatentStats(mu.shape[1])
            stats.update(mu[:nb])
            lat = mu if what == "mean" else torch.cat([mu, logvar], 1)
            pend["latents"].append(lat[:nb].float().cpu())
            if flip:
                pend["latents_flip"].append(lat[nb:].float().cpu())
            if labels is not None:
                pend["labels"].append(labels.reshape(-1).to(torch.int64).cpu())
            count += nb
            while count >= shard_size:
                flush(shard_size)
    if count:
        flush(count)
    if stats is None:
        raise ValueError("extract_latents: the loader yielded no batch")
    d = stats.dim
    torch.save({"mean": stats.mean.float().reshape(1, d, 1, 1).cpu(), "std": stats.std.float().reshape(1, d, 1, 1).cpu(),
                "cov": stats.cov.cpu(), "n": stats.n}, os.path.join(out_dir, "latents_stats.pt"))
    return stats


def latent_points(latents: torch.Tensor, per: str = "token", max_points: Optional[int] = None,
                  generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """[B, D, h, w] -> points [n, D]: every spatial position of every image (per="token") or each image's spatial mean
    (per="image").  With max_points < n a subset is drawn by a permutation from `generator` (a CPU generator; seed 0 if None)."""
    if per not in ("token", "image"):
        raise ValueError(f"latent_points: per={per!r} (expected 'token' or 'image')")
    if latents.dim() != 4:
        raise ValueError(f"latent_points: expected [B, D, h, w], got {tuple(latents.shape)}")
    x = latents.float()
    pts = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) if per == "token" else x.mean(dim=(2, 3))
    if max_points is not None and pts.shape[0] > max_points:
        if generator is None:
            generator = torch.Generator().manual_seed(0)
        idx = torch.randperm(pts.shape[0], generator=generator)[:max_points]
        pts = pts[idx.to(pts.device)]
    return pts.contiguous()


def kde_logdensity(data: torch.Tensor, queries: Optional[torch.Tensor], bandwidth: float, exclude_self: bool = False) -> torch.Tensor:
    """log sum_j exp(-|q_i - x_j|^2 / (2 h^2)) per query, fp32 [M] (`tv_kde_logdensity`; no normaliser).  queries=None: the data
    points themselves; with exclude_self the term j == i is dropped."""
    q = data if queries is None else queries
    if data.dim() != 2 or q.dim() != 2 or q.shape[1] != data.shape[1]:
        raise ValueError(f"kde_logdensity: data [N, d] and queries [M, d], got {tuple(data.shape)} and {tuple(q.shape)}")
    N, d = data.shape
    M = q.shape[0]
    if d > MAX_DIM or d < 1:
        raise ValueError(f"kde_logdensity: d={d} must be in [1, {MAX_DIM}] (project with pca= first)")
    if N < 1 or M < 1 or (exclude_self and (queries is not None or N < 2)):
        raise ValueError("kde_logdensity: needs at least one point (two with exclude_self, which takes queries=None)")
    if not (bandwidth > 0 and math.isfinite(bandwidth)):
        raise ValueError(f"kde_logdensity: bandwidth {bandwidth!r} must be positive and finite")
    ops._need_gpu(data, q)
    ops._require(data.dtype == torch.float32 and q.dtype == torch.float32, "kde_logdensity: fp32 points")

    def rows(t):
        return t if t.stride(1) == 1 and t.stride(0) >= d else t.contiguous()
    data = rows(data)
    q = data if queries is None else rows(q)
    lib = L.load()
    with torch.cuda.device(data.device):
        out = torch.empty(M, dtype=torch.float32, device=data.device)
        scratch = torch.empty(2 * _KDE_SPLIT_MAX * M, dtype=torch.float64, device=data.device) if M < _KDE_SPLIT_BELOW else None
        L.check(lib.tv_kde_logdensity(ops._p(data), N, ops._p(q), M, d, data.stride(0), q.stride(0), 1.0 / (2.0 * bandwidth * bandwidth),
                                      1 if exclude_self else 0, ops._p(out), ops._p(scratch), ops._stream()), "tv_kde_logdensity")
    return out


def density_metrics_from_logdensity(logdens: torch.Tensor) -> Dict[str, float]:
    """CV, normalised entropy and Gini of f_i = exp(l_i - max l), fp64 on the tensor's device (all three are scale-free)."""
    ld = logdens.double()
    n = ld.shape[0]
    f = torch.exp(ld - ld.max())
    tot = f.sum()
    cv = f.std(unbiased=False) / f.mean()
    p = f / tot
    ent = -(torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))).sum() / math.log(n)
    fs = torch.sort(f).values
    w = 2.0 * torch.arange(1, n + 1, dtype=torch.float64, device=ld.device) - n - 1
    gini = (w * fs).sum() / (n * tot)
    return {"density_cv": float(cv), "normalized_entropy": float(ent), "gini": float(gini)}


def latent_density_metrics(points: torch.Tensor, bandwidth: Union[str, float] = "scott", standardize: bool = True,
                           pca: Optional[int] = None, leave_one_out: bool = True) -> Dict[str, float]:
    """{"density_cv", "normalized_entropy", "gini", "bandwidth", "n", "d"} of a Gaussian KDE over points [n, D].

    standardize: every dimension to population mean 0 / std 1 first.  pca=k: project (after the standardisation) onto the top k
    principal axes (fp64 `eigh` of the covariance on the host, one fp32 matmul).  bandwidth: "scott" = n^(-1/(d + 4)) with d the
    dimension the estimate runs in, or a float.  leave_one_out: a point does not count towards its own density."""
    if points.dim() != 2:
        raise ValueError(f"latent_density_metrics: points must be [n, D], got {tuple(points.shape)}")
    n, D = points.shape
    if n < 2:
        raise ValueError(f"latent_density_metrics: {n} point(s); at least 2 are needed")
    if pca is not None and not 1 <= int(pca) <= D:
        raise ValueError(f"latent_density_metrics: pca={pca} must be in [1, D={D}]")
    d = D if pca is None else int(pca)
    if d > MAX_DIM:
        raise ValueError(f"latent_density_metrics: d={d} > {MAX_DIM}; pass pca= to project first")
    if isinstance(bandwidth, str):
        if bandwidth != "scott":
            raise ValueError(f"latent_density_metrics: bandwidth={bandwidth!r} (expected 'scott' or a float)")
        h = float(n) ** (-1.0 / (d + 4))
    else:
        h = float(bandwidth)
        if not (h > 0 and math.isfinite(h)):
            raise ValueError(f"latent_density_metrics: bandwidth {bandwidth!r} must be positive and finite")
    ops._need_gpu(points)
    x = points.float()
    if standardize:
        x64 = x.double()
        mu, sd = x64.mean(0), x64.std(0, unbiased=False)
        x = ((x64 - mu) / torch.where(sd > 0, sd, torch.ones_like(sd))).float()
    if pca is not None:
        x64 = x.double()
        xc = x64 - x64.mean(0)
        cov = (xc.T @ xc / n).cpu()
        _, vec = torch.linalg.eigh(cov)                                  # ascending eigenvalues
        axes = vec[:, -d:].flip(1).float().to(x.device)
        x = (x - x64.mean(0).float()) @ axes
    ld = kde_logdensity(x.contiguous(), None, h, exclude_self=leave_one_out)
    res = density_metrics_from_logdensity(ld)
    res.update({"bandwidth": h, "n": int(n), "d": int(d)})
    return res


def latent_space_metrics(model: torch.nn.Module, dataloader: Iterable, *, per: str = "token", max_points: int = 65536, prep=None,
                         device="cuda", generator: Optional[torch.Generator] = None, **metric_args) -> Dict[str, float]:
    """Encode the loader's images (posterior means), take `latent_points(per, max_points)` and return
    `latent_density_metrics(points, **metric_args)`."""
    model.eval()
    mus = []
    with torch.no_grad():
        for batch in dataloader:
            images, _ = _unpack(batch, device, prep)
            mus.append(model.encode(images)[0].float())
    if not mus:
        raise ValueError("latent_space_metrics: the loader yielded no batch")
    pts = latent_points(torch.cat(mus), per=per, max_points=max_points, generator=generator)
    return latent_density_metrics(pts, **metric_args)
