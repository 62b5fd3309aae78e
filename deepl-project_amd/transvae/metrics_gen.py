"""Generation metrics on Inception pool3 features (csrc/genmetrics.hip; protocol: DESIGN.md section 3.5).

* `knn_radius`, `manifold_hits`, `precision_recall`: the improved precision / recall of Kynkaanniemi et al. (2019) with
  k-nearest-neighbour manifolds, k = 3 as in the ADM evaluation suite.  Two all-pairs passes over the features per side; no
  N x N matrix is formed.  Squared distances are direct differences in one fp32 chain, never the Gram form.
* `InceptionScore`: exp(mean_i KL(p_i || mean_j p_j)) over the whole set, the softmax statistics streamed in fp64 on the device
  (`tv_softmax_stats`), the logits from the classifier head of the FID Inception-v3 file.
* `reference_statistics`: everything `transvae.evaluate_dit` needs from the real images, computed once.

There is no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from .hip import _lib as L
from .hip import ops

MAX_K = 8                  # tv_knn_radius keeps the 8 smallest distances
MAX_DIM = 8192
QUERIES_PER_LAUNCH = 8192  # no launch runs long: 8192 x 50 000 x 2048 is a sixth of a second of arithmetic at a third of peak
_FULL_BLOCKS = 512         # csrc/genmetrics.hip: from this many 64-query blocks on the data range is not cut
_SLICES = 32


def _rows(t: torch.Tensor, d: int) -> torch.Tensor:
    return t if t.stride(1) == 1 and t.stride(0) >= d else t.contiguous()


def _check_points(what: str, name: str, t: torch.Tensor):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= MAX_DIM:
        raise ValueError(f"{what}: {name} must be [n, d] with n >= 1 and 1 <= d <= {MAX_DIM}, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")


def _scratch(step: int, per_query: int, dtype, device):
    """slice partials for launches of up to `step` queries (only launches of fewer than 64 * 512 queries cut the data range)"""
    return torch.empty(per_query * min(step, 64 * _FULL_BLOCKS), dtype=dtype, device=device)


def knn_radius(x: torch.Tensor, k: int = 3, queries_per_launch: int = QUERIES_PER_LAUNCH) -> torch.Tensor:
    """fp32 [N]: the squared distance from every row of x [N, d] to its k-th nearest other row (`tv_knn_radius`; self is excluded
    by index, duplicates count).  The query range is cut into launches of at most `queries_per_launch`; the values do not
    depend on the cut.  The rows must be finite (not checked here: a NaN distance is dropped from the k-list, include/transvae_hip.h)."""
    _check_points("knn_radius", "x", x)
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"knn_radius: k={k} must be in [1, {MAX_K}]")
    N, d = x.shape
    if N < int(k) + 1:
        raise ValueError(f"knn_radius: x has {N} row(s); k={k} needs at least {int(k) + 1}")
    if int(queries_per_launch) < 1:
        raise ValueError(f"knn_radius: queries_per_launch={queries_per_launch} must be positive")
    ops._need_gpu(x)
    ops._require(x.dtype == torch.float32, "knn_radius: fp32 points")
    x = _rows(x, d)
    lib = L.load()
    with torch.cuda.device(x.device):
        r2 = torch.empty(N, dtype=torch.float32, device=x.device)
        step = min(int(queries_per_launch), N)
        scratch = _scratch(step, 8 * _SLICES, torch.float32, x.device)
        for i0 in range(0, N, step):
            M = min(step, N - i0)
            L.check(lib.tv_knn_radius(ops._p(x), N, d, x.stride(0), i0, M, int(k), ops._p(r2[i0:]), ops._p(scratch), ops._stream()),
                    "tv_knn_radius")
    return r2


def manifold_hits(q: torch.Tensor, x: torch.Tensor, r2: torch.Tensor, queries_per_launch: int = QUERIES_PER_LAUNCH) -> torch.Tensor:
    """int32 [M]: 1 where the query q_i lies within squared distance r2[j] of some x_j (`tv_manifold_hits`, `<=` on fp32).
    q, x and r2 must be finite (not checked here)."""
    _check_points("manifold_hits", "q", q)
    _check_points("manifold_hits", "x", x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"manifold_hits: q has {q.shape[1]} columns and x {x.shape[1]}")
    if not isinstance(r2, torch.Tensor) or tuple(r2.shape) != (x.shape[0],):
        raise ValueError(f"manifold_hits: r2 must be [{x.shape[0]}], one squared radius per row of x")
    if int(queries_per_launch) < 1:
        raise ValueError(f"manifold_hits: queries_per_launch={queries_per_launch} must be positive")
    ops._need_gpu(q, x, r2)
    ops._require(q.dtype == torch.float32 and x.dtype == torch.float32 and r2.dtype == torch.float32, "manifold_hits: fp32 points and radii")
    ops._require(q.device == x.device == r2.device, "manifold_hits: q, x and r2 on one device")
    (M, d), N = q.shape, x.shape[0]
    q, x, r2 = _rows(q, d), _rows(x, d), r2.contiguous()
    lib = L.load()
    with torch.cuda.device(x.device):
        hit = torch.empty(M, dtype=torch.int32, device=x.device)
        step = min(int(queries_per_launch), M)
        scratch = _scratch(step, _SLICES, torch.int32, x.device)
        for i0 in range(0, M, step):
            m = min(step, M - i0)
            L.check(lib.tv_manifold_hits(ops._p(q[i0:]), m, q.stride(0), ops._p(x), N, x.stride(0), ops._p(r2), d, ops._p(hit[i0:]),
                                         ops._p(scratch), ops._stream()), "tv_manifold_hits")
    return hit


def _precision_recall_device(real: torch.Tensor, fake: torch.Tensor, k: int):
    """(precision, recall) as fp64 device scalars: no synchronisation"""
    _check_points("precision_recall", "real", real)
    _check_points("precision_recall", "fake", fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"precision_recall: real has {real.shape[1]} columns and fake {fake.shape[1]}")
    r_real, r_fake = knn_radius(real, k), knn_radius(fake, k)
    precision = manifold_hits(fake, real, r_real).double().mean()
    recall = manifold_hits(real, fake, r_fake).double().mean()
    return precision, recall


def precision_recall(real: torch.Tensor, fake: torch.Tensor, k: int = 3) -> Dict[str, float]:
    """{"precision": share of fake rows inside the real manifold, "recall": share of real rows inside the fake manifold}; a
    manifold is the union of the balls around each row reaching to its k-th nearest other row."""
    p, r = _precision_recall_device(real, fake, k)
    return {"precision": float(p), "recall": float(r)}


class InceptionScore:
    """Streaming Inception Score.  weight [K, d] (and bias [K]) are the classifier head on top of the pool3 features; `update`
    takes fp32 feature rows [B, d] on the head's device, `compute` returns exp(S / n - sum_k pbar_k log pbar_k) over the whole
    set (no splits), with S = sum_i sum_k p_ik log p_ik and pbar = mean_i p_i, in fp64."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
        if weight.dim() != 2 or not 1 <= weight.shape[0] <= 4096:
            raise ValueError(f"InceptionScore: weight must be [K, d] with 1 <= K <= 4096, got {tuple(weight.shape)}")
        if bias is not None and tuple(bias.shape) != (weight.shape[0],):
            raise ValueError(f"InceptionScore: bias must be [{weight.shape[0]}], got {tuple(bias.shape)}")
        self.weight = weight.detach().float().contiguous()
        self.bias = torch.zeros(weight.shape[0]) if bias is None else bias.detach().float().contiguous()
        self.bias = self.bias.to(self.weight.device)
        self.classes, self.dims = self.weight.shape
        self._state = None
        self._n = 0

    @classmethod
    def from_file(cls, path: str) -> "InceptionScore":
        """The head of the pt_inception file `InceptionFeatures.from_file` reads: `fc.weight` and, if present, `fc.bias`."""
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        if "fc.weight" not in sd:
            raise KeyError(f"InceptionScore.from_file: {path} has no 'fc.weight'")
        return cls(sd["fc.weight"], sd.get("fc.bias"))

    def to(self, device) -> "InceptionScore":
        self.weight, self.bias = self.weight.to(device), self.bias.to(device)
        return self

    def reset(self) -> None:
        self._state, self._n = None, 0

    @property
    def n(self) -> int:
        return self._n

    @torch.no_grad()
    def update(self, features: torch.Tensor) -> None:
        if features.dim() != 2 or features.shape[1] != self.dims:
            raise ValueError(f"InceptionScore.update: features must be [B, {self.dims}], got {tuple(features.shape)}")
        ops._need_gpu(features, self.weight)
        ops._require(features.dtype == torch.float32 and features.device == self.weight.device,
                     "InceptionScore.update: fp32 features on the head's device")
        B, K = features.shape[0], self.classes
        if B == 0:
            return
        lib = L.load()
        with torch.cuda.device(features.device), torch.autocast("cuda", enabled=False):
            logits = torch.addmm(self.bias, features, self.weight.t())
            if self._state is None:
                self._state = torch.zeros(2 + K, dtype=torch.float64, device=features.device)
            scratch = torch.empty(B * (K + 1), dtype=torch.float64, device=features.device)
            L.check(lib.tv_softmax_stats(ops._p(logits), B, K, logits.stride(0), ops._p(self._state), ops._p(scratch), ops._stream()),
                    "tv_softmax_stats")
        self._n += B

    def state(self) -> torch.Tensor:
        """The device state {rows, S, psum[K]} (fp64)."""
        return self._state

    def compute(self) -> float:
        if self._n < 1:
            raise ValueError("InceptionScore: no features yet")
        return score_from_state(self._state.cpu().numpy())


def score_from_state(st: np.ndarray) -> float:
    """exp(S / n - sum_k pbar_k log pbar_k) from a `tv_softmax_stats` state, fp64 on the host"""
    n = float(st[0])
    pbar = st[2:] / n
    nz = pbar > 0
    return float(math.exp(st[1] / n - float((pbar[nz] * np.log(pbar[nz])).sum())))


def reference_statistics(loader: Iterable, fid_net, *, prep=None, is_head: Optional[InceptionScore] = None,
                         max_features: int = 10000) -> Dict:
    """The real side of `evaluate_dit`, once per data set: {"n", "mean" [d], "cov" [d, d] (fp64, as np.cov gives), "features" (the
    first `max_features` feature rows, fp32, host) and, with `is_head`, "is" (the real set's Inception Score)}.  The loader yields
    images in [0, 1] (or uint8 batches for `prep`) as `evaluate` takes them; the features are `fid_net.features(images, clip=True)`.
    The dict goes to disk with `torch.save` and comes back with `torch.load`."""
    from .evaluate import _uint8_images
    from .metrics_fid import FrechetDistance
    if int(max_features) < 0:
        raise ValueError(f"reference_statistics: max_features={max_features} must not be negative")
    frechet, kept, have = None, [], 0
    dev = next(fid_net.buffers()).device
    if is_head is not None:
        is_head.reset()
    for batch in loader:
        if prep is not None:
            images = prep(_uint8_images(batch, dev))
        else:
            images = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(dev)
        feats = fid_net.features(images, clip=True)
        if frechet is None:
            frechet = FrechetDistance(feats.shape[1])
        frechet.update(feats, None)
        if is_head is not None:
            is_head.update(feats)
        if have < max_features:
            kept.append(feats[:max_features - have])
            have += kept[-1].shape[0]
    if frechet is None:
        raise ValueError("reference_statistics: the loader yielded no batch")
    n, mean, cov = frechet.statistics(0)
    out = {"n": int(n), "mean": torch.from_numpy(mean), "cov": torch.from_numpy(cov),
           "features": torch.cat(kept).cpu() if kept else torch.zeros(0, frechet.dims)}
    if is_head is not None:
        out["is"] = is_head.compute()
    return out
