"""Generation metrics on Inception pool3 features (csrc/genmetrics.hip; protocol: DESIGN.md section 3.5).

* `knn_radius`, `manifold_hits`, `precision_recall`: the improved precision / recall of Kynkaanniemi et al. (2019) with
  k-nearest-neighbour manifolds, k = 3 as in the ADM evaluation suite.  Two all-pairs passes over the features per side; no
  N x N matrix is formed.  Squared distances are direct differences in one fp32 chain, never the Gram form.
* `InceptionScore`: exp(mean_i KL(p_i || mean_j p_j)) over the whole set, the softmax statistics streamed in fp64 on the device
  (`tv_softmax_stats`), the logits from the classifier head of the FID Inception-v3 file.
  `InceptionScore(..., split_size=s)` keeps one state per split of s rows: the mean (and standard deviation) over splits.
* `ball_counts`, `density_coverage`: density / coverage of Naeem et al. (2020), k = 5, on the same distances (`tv_ball_counts`).
* `kid_subsets`, `poly_kernel_sums`, `kernel_inception_distance`: KID, the unbiased MMD^2 with the kernel (x . y / d + 1)^3 over
  subsets; the kernel sums of all subsets in one launch, in a fixed order, without an m x m matrix (`tv_poly_kernel_sums`).
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


_RADIUS_OF = {"data": 0, "query": 1}


def ball_counts(q: torch.Tensor, x: torch.Tensor, r2: torch.Tensor, radius_of: str = "data",
                queries_per_launch: int = QUERIES_PER_LAUNCH) -> torch.Tensor:
    """int32 [M] (`tv_ball_counts`, `<=` on fp32, the distance chain of `manifold_hits`): with radius_of="data" the number of rows
    x_j whose ball of squared radius r2[j] holds the query q_i (r2 [N]); with radius_of="query" the number of rows x_j inside the
    query's own ball of squared radius r2[i] (r2 [M]).  q, x and r2 must be finite (not checked here)."""
    _check_points("ball_counts", "q", q)
    _check_points("ball_counts", "x", x)
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"ball_counts: q has {q.shape[1]} columns and x {x.shape[1]}")
    if radius_of not in _RADIUS_OF:
        raise ValueError(f"ball_counts: radius_of={radius_of!r} must be 'data' or 'query'")
    rows = x.shape[0] if radius_of == "data" else q.shape[0]
    if not isinstance(r2, torch.Tensor) or tuple(r2.shape) != (rows,):
        raise ValueError(f"ball_counts: r2 must be [{rows}], one squared radius per row of {'x' if radius_of == 'data' else 'q'}")
    if int(queries_per_launch) < 1:
        raise ValueError(f"ball_counts: queries_per_launch={queries_per_launch} must be positive")
    ops._need_gpu(q, x, r2)
    ops._require(q.dtype == torch.float32 and x.dtype == torch.float32 and r2.dtype == torch.float32, "ball_counts: fp32 points and radii")
    ops._require(q.device == x.device == r2.device, "ball_counts: q, x and r2 on one device")
    (M, d), N = q.shape, x.shape[0]
    q, x, r2 = _rows(q, d), _rows(x, d), r2.contiguous()
    per_query = _RADIUS_OF[radius_of]
    lib = L.load()
    with torch.cuda.device(x.device):
        count = torch.empty(M, dtype=torch.int32, device=x.device)
        step = min(int(queries_per_launch), M)
        scratch = _scratch(step, _SLICES, torch.int32, x.device)
        for i0 in range(0, M, step):
            m = min(step, M - i0)
            L.check(lib.tv_ball_counts(ops._p(q[i0:]), m, q.stride(0), ops._p(x), N, x.stride(0), ops._p(r2[i0:] if per_query else r2), d,
                                       per_query, ops._p(count[i0:]), ops._p(scratch), ops._stream()), "tv_ball_counts")
    return count


def _density_coverage_device(real: torch.Tensor, fake: torch.Tensor, k: int):
    """(density, coverage) as fp64 device scalars: no synchronisation"""
    _check_points("density_coverage", "real", real)
    _check_points("density_coverage", "fake", fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"density_coverage: real has {real.shape[1]} columns and fake {fake.shape[1]}")
    r_real = knn_radius(real, k)
    density = ball_counts(fake, real, r_real, "data").double().sum() / float(int(k) * fake.shape[0])
    coverage = (ball_counts(real, fake, r_real, "query") > 0).double().mean()
    return density, coverage


def density_coverage(real: torch.Tensor, fake: torch.Tensor, k: int = 5) -> Dict[str, float]:
    """Naeem et al. (2020), with the balls around the REAL rows reaching to their k-th nearest other real row:
    {"density": sum over the fake rows of the number of real balls holding them, over k * (number of fake rows);
     "coverage": share of real rows whose own ball holds at least one fake row}."""
    d, c = _density_coverage_device(real, fake, k)
    return {"density": float(d), "coverage": float(c)}


# ---------------------------------------------------------------------------------------------------------------------
# KID
# ---------------------------------------------------------------------------------------------------------------------
def kid_subsets(n_real: int, n_fake: int, subsets: int = 100, subset_size: int = 1000, seed: int = 0):
    """(ia, ib, m): int32 [subsets, m] row indices into the real and the fake set, m = min(subset_size, n_real, n_fake).  The
    package's own draw: one numpy.random.default_rng(seed); subset after subset, first `choice(n_real, m, replace=False)`, then
    `choice(n_fake, m, replace=False)`."""
    n_real, n_fake, subsets, subset_size = int(n_real), int(n_fake), int(subsets), int(subset_size)
    if subsets < 1 or subsets > 65535:
        raise ValueError(f"kid_subsets: subsets={subsets} must be in [1, 65535]")
    m = min(subset_size, n_real, n_fake)
    if m < 2:
        raise ValueError(f"kid_subsets: subset_size={subset_size} with {n_real} real and {n_fake} fake rows leaves m={m}; the unbiased "
                         "estimate needs at least 2")
    if m > 1 << 16:
        raise ValueError(f"kid_subsets: m={m} rows per subset; at most {1 << 16}")
    g = np.random.default_rng(int(seed))
    ia, ib = np.empty((subsets, m), dtype=np.int32), np.empty((subsets, m), dtype=np.int32)
    for s in range(subsets):
        ia[s] = g.choice(n_real, m, replace=False)
        ib[s] = g.choice(n_fake, m, replace=False)
    return ia, ib, m


def poly_kernel_sums(a: torch.Tensor, ia: torch.Tensor, b: torch.Tensor, ib: torch.Tensor, gamma: float, coef0: float = 1.0,
                     skip_equal_position: bool = False) -> torch.Tensor:
    """fp64 [S]: for every subset s, the sum over positions i, j < m of (gamma a[ia[s, i]] . b[ib[s, j]] + coef0)^3, without the
    pairs i == j when `skip_equal_position` (`tv_poly_kernel_sums`; fixed summation order, no m x m matrix).  ia, ib: int32
    [S, m] device tensors with entries inside a and b (not checked here: they stay on the device)."""
    _check_points("poly_kernel_sums", "a", a)
    _check_points("poly_kernel_sums", "b", b)
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"poly_kernel_sums: a has {a.shape[1]} columns and b {b.shape[1]}")
    if not (isinstance(ia, torch.Tensor) and isinstance(ib, torch.Tensor) and ia.dim() == 2 and ia.shape == ib.shape and ia.shape[1] >= 1
            and ia.shape[0] >= 1):
        raise ValueError("poly_kernel_sums: ia and ib must be [S, m] index tensors of one shape")
    ops._need_gpu(a, b, ia, ib)
    ops._require(a.dtype == torch.float32 and b.dtype == torch.float32 and ia.dtype == torch.int32 and ib.dtype == torch.int32,
                 "poly_kernel_sums: fp32 rows and int32 indices")
    ops._require(a.device == b.device == ia.device == ib.device, "poly_kernel_sums: a, b, ia and ib on one device")
    d = a.shape[1]
    S, m = ia.shape
    a, b, ia, ib = _rows(a, d), _rows(b, d), ia.contiguous(), ib.contiguous()
    lib = L.load()
    need = lib.tv_poly_kernel_scratch_doubles(m, S)
    if need < 0:
        raise ValueError(f"poly_kernel_sums: m={m} must be in [1, {1 << 16}] and S={S} in [1, 65535]")
    with torch.cuda.device(a.device):
        sums = torch.empty(S, dtype=torch.float64, device=a.device)
        scratch = torch.empty(need, dtype=torch.float64, device=a.device)
        L.check(lib.tv_poly_kernel_sums(ops._p(a), a.stride(0), ops._p(ia), ops._p(b), b.stride(0), ops._p(ib), m, S, d, float(gamma),
                                        float(coef0), int(bool(skip_equal_position)), ops._p(sums), ops._p(scratch), ops._stream()),
                "tv_poly_kernel_sums")
    return sums


def _kid_device(real: torch.Tensor, fake: torch.Tensor, draw) -> torch.Tensor:
    """fp64 [2] on the device: (mean, standard deviation) of the per-subset unbiased MMD^2 over the subsets `draw` = (ia, ib, m)
    of `kid_subsets`; no synchronisation"""
    _check_points("kernel_inception_distance", "real", real)
    _check_points("kernel_inception_distance", "fake", fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"kernel_inception_distance: real has {real.shape[1]} columns and fake {fake.shape[1]}")
    ia, ib, m = draw
    if int(ia.max()) >= real.shape[0] or int(ib.max()) >= fake.shape[0] or int(ia.min()) < 0 or int(ib.min()) < 0:
        raise ValueError("kernel_inception_distance: the subsets index rows outside the feature sets")
    ops._need_gpu(real, fake)
    ia, ib = torch.from_numpy(ia).to(real.device), torch.from_numpy(ib).to(real.device)
    gamma = 1.0 / real.shape[1]
    sxx = poly_kernel_sums(real, ia, real, ia, gamma, 1.0, True)
    syy = poly_kernel_sums(fake, ib, fake, ib, gamma, 1.0, True)
    sxy = poly_kernel_sums(real, ia, fake, ib, gamma, 1.0, False)
    vals = sxx / float(m * (m - 1)) + syy / float(m * (m - 1)) - 2.0 * sxy / float(m * m)
    return torch.stack([vals.mean(), vals.std(unbiased=False)])


def kernel_inception_distance(real: torch.Tensor, fake: torch.Tensor, subsets: int = 100, subset_size: int = 1000,
                              seed: int = 0) -> Dict[str, float]:
    """{"kid", "kid_std"}: mean and (population) standard deviation over `subsets` subsets of the unbiased MMD^2 with the kernel
    k(x, y) = (x . y / d + 1)^3 (Binkowski et al. 2018): Sxx / (m (m - 1)) + Syy / (m (m - 1)) - 2 Sxy / m^2 per subset, Sxx and Syy
    without the pairs at equal position.  The subsets are `kid_subsets(len(real), len(fake), subsets, subset_size, seed)`."""
    _check_points("kernel_inception_distance", "real", real)
    _check_points("kernel_inception_distance", "fake", fake)
    mean, std = _kid_device(real, fake, kid_subsets(real.shape[0], fake.shape[0], subsets, subset_size, seed)).cpu().tolist()
    return {"kid": mean, "kid_std": std}


class InceptionScore:
    """Streaming Inception Score.  weight [K, d] (and bias [K]) are the classifier head on top of the pool3 features; `update`
    takes fp32 feature rows [B, d] on the head's device, `compute` returns exp(S / n - sum_k pbar_k log pbar_k) over the whole
    set (no splits), with S = sum_i sum_k p_ik log p_ik and pbar = mean_i p_i, in fp64.

    With `split_size` the rows are cut, in the order they arrive, into consecutive splits of that many rows (the last may be
    short); every split keeps its own state, `compute` returns the mean of the per-split scores (what the ADM evaluation suite
    reports) and `compute_std` their population standard deviation.  A split's state does not depend on how the rows were cut
    into `update` calls."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, split_size: Optional[int] = None):
        if weight.dim() != 2 or not 1 <= weight.shape[0] <= 4096:
            raise ValueError(f"InceptionScore: weight must be [K, d] with 1 <= K <= 4096, got {tuple(weight.shape)}")
        if bias is not None and tuple(bias.shape) != (weight.shape[0],):
            raise ValueError(f"InceptionScore: bias must be [{weight.shape[0]}], got {tuple(bias.shape)}")
        if split_size is not None and int(split_size) < 1:
            raise ValueError(f"InceptionScore: split_size={split_size} must be positive (or None: one score over the whole set)")
        self.split_size = None if split_size is None else int(split_size)
        self._splits = []
        self.weight = weight.detach().float().contiguous()
        self.bias = torch.zeros(weight.shape[0]) if bias is None else bias.detach().float().contiguous()
        self.bias = self.bias.to(self.weight.device)
        self.classes, self.dims = self.weight.shape
        self._state = None
        self._n = 0

    @classmethod
    def from_file(cls, path: str, split_size: Optional[int] = None) -> "InceptionScore":
        """The head of the pt_inception file `InceptionFeatures.from_file` reads: `fc.weight` and, if present, `fc.bias`."""
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        if "fc.weight" not in sd:
            raise KeyError(f"InceptionScore.from_file: {path} has no 'fc.weight'")
        return cls(sd["fc.weight"], sd.get("fc.bias"), split_size)

    def to(self, device) -> "InceptionScore":
        self.weight, self.bias = self.weight.to(device), self.bias.to(device)
        return self

    def reset(self) -> None:
        self._state, self._n, self._splits = None, 0, []

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
            scratch = torch.empty(B * (K + 1), dtype=torch.float64, device=features.device)
            if self.split_size is None:
                if self._state is None:
                    self._state = torch.zeros(2 + K, dtype=torch.float64, device=features.device)
                L.check(lib.tv_softmax_stats(ops._p(logits), B, K, logits.stride(0), ops._p(self._state), ops._p(scratch), ops._stream()),
                        "tv_softmax_stats")
            else:
                for split, b0, nb in split_pieces(self._n, B, self.split_size):
                    if split == len(self._splits):
                        self._splits.append(torch.zeros(2 + K, dtype=torch.float64, device=features.device))
                    L.check(lib.tv_softmax_stats(ops._p(logits[b0:]), nb, K, logits.stride(0), ops._p(self._splits[split]), ops._p(scratch),
                                                 ops._stream()), "tv_softmax_stats")
        self._n += B

    def state(self) -> torch.Tensor:
        """The device state {rows, S, psum[K]} (fp64); with a split size the states of the splits so far, [splits, 2 + K]."""
        return self._state if self.split_size is None else (torch.stack(self._splits) if self._splits else None)

    def scores(self) -> np.ndarray:
        """The per-split scores (fp64, host); one entry without a split size."""
        if self._n < 1:
            raise ValueError("InceptionScore: no features yet")
        return scores_from_states(self.state().cpu().numpy())

    def compute(self) -> float:
        """The score of the whole set, or with a split size the mean of the per-split scores."""
        return float(self.scores().mean())

    def compute_std(self) -> float:
        """The population standard deviation of the per-split scores (0 without a split size)."""
        return float(self.scores().std())


def split_pieces(n0: int, B: int, split_size: int):
    """[(split, first row, rows)]: how a batch of B rows arriving after n0 rows is cut at the boundaries of splits of `split_size`"""
    out, b0 = [], 0
    while b0 < B:
        split, used = divmod(n0 + b0, split_size)
        nb = min(B - b0, split_size - used)
        out.append((split, b0, nb))
        b0 += nb
    return out


def scores_from_states(st: np.ndarray) -> np.ndarray:
    """fp64 [splits]: `score_from_state` of every row of a stack of states (a single state counts as one split)"""
    st = np.asarray(st, dtype=np.float64)
    return np.array([score_from_state(row) for row in st.reshape(-1, st.shape[-1])])


def score_from_state(st: np.ndarray) -> float:
    """exp(S / n - sum_k pbar_k log pbar_k) from a `tv_softmax_stats` state, fp64 on the host"""
    n = float(st[0])
    pbar = st[2:] / n
    nz = pbar > 0
    return float(math.exp(st[1] / n - float((pbar[nz] * np.log(pbar[nz])).sum())))


def reference_statistics(loader: Iterable, fid_net, *, prep=None, is_head: Optional[InceptionScore] = None,
                         max_features: int = 10000, spatial: bool = False) -> Dict:
    """The real side of `evaluate_dit`, once per data set: {"n", "mean" [d], "cov" [d, d] (fp64, as np.cov gives), "features" (the
    first `max_features` feature rows, fp32, host) and, with `is_head`, "is" (the real set's Inception Score)}.  The loader yields
    images in [0, 1] (or uint8 batches for `prep`) as `evaluate` takes them; the features are `fid_net.features(images, clip=True)`.
    spatial=True adds what sFID needs, "spatial_n", "spatial_mean" [2023] and "spatial_cov" [2023, 2023]: the same statistics of the
    spatial rows of `fid_net.features(images, clip=True, spatial=True)`.
    The dict goes to disk with `torch.save` and comes back with `torch.load`."""
    from .evaluate import _uint8_images
    from .metrics_fid import SPATIAL_DIM, SPATIAL_LD, FrechetDistance
    if int(max_features) < 0:
        raise ValueError(f"reference_statistics: max_features={max_features} must not be negative")
    frechet, kept, have = None, [], 0
    sfrechet = FrechetDistance(SPATIAL_LD) if spatial else None
    dev = next(fid_net.buffers()).device
    if is_head is not None:
        is_head.reset()
    for batch in loader:
        if prep is not None:
            images = prep(_uint8_images(batch, dev))
        else:
            images = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(dev)
        if spatial:
            feats, rows = fid_net.features(images, clip=True, spatial=True)
            sfrechet.update(rows, None)
        else:
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
    if spatial:
        sn, smean, scov = sfrechet.statistics(0)
        out["spatial_n"] = int(sn)
        out["spatial_mean"] = torch.from_numpy(smean[:SPATIAL_DIM].copy())
        out["spatial_cov"] = torch.from_numpy(np.ascontiguousarray(scov[:SPATIAL_DIM, :SPATIAL_DIM]))
    return out
