"""Linear probing of latents: the "linear probing accuracy" part of the reference's VF-loss analysis table, on the device.

`probe_rows` turns stored latents into the classifier's bf16 operand (`tv_probe_rows`: average pooling to a grid, per-channel
standardisation, one rounding), `LinearProbe` is one `ops.linear` layer, `softmax_xent` the cross-entropy with label smoothing,
its gradient and top-1 / top-5 counts in one pass (`tv_softmax_xent`, csrc/probe.hip).  `fit_linear_probe` trains the layer with
`FusedAdamW` on the shards `extract_latents` writes and reports validation accuracy; `linear_probe_accuracy` runs the extraction
first.  The reference names the measurement only; the protocol here is this package's own.
There is no CPU fallback: host tensors raise.
"""
from __future__ import annotations

import glob
import math
import os
from typing import Dict, Iterable, Optional, Tuple, Union

import torch
import torch.nn.functional as F

from .hip import _lib as L
from .hip import ops
from .latents import LatentStats, extract_latents
from .optim import FusedAdamW

Source = Union[str, Tuple[torch.Tensor, torch.Tensor]]


def _round_up(n: int, k: int) -> int:
    return -(-n // k) * k


def _grid(h: int, w: int, pool: Optional[int]) -> Tuple[int, int]:
    if pool is None:
        return h, w
    g = int(pool)
    if g < 1 or h % g or w % g:
        raise ValueError(f"probe_rows: pool={pool} must divide the latent grid {h} x {w}")
    return g, g


def _probe_rows(latents: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    B, D, h, w = latents.shape
    x = latents
    if not (x.stride(3) == 1 and x.stride(2) == w and x.stride(1) >= h * w and x.stride(0) >= (D - 1) * x.stride(1) + h * w):
        x = x.contiguous()
    ld = _round_up(gh * gw * D, 32)
    with torch.cuda.device(x.device):
        rows = torch.empty((B, ld), dtype=torch.bfloat16, device=x.device)
        L.check(L.load().tv_probe_rows(ops._p(x), x.stride(0), x.stride(1), ops._p(mean), ops._p(rstd), ops._p(rows), B, D, h, w, gh, gw, ld,
                                       ops._stream()), "tv_probe_rows")
    return rows


def _stat_vectors(mean: torch.Tensor, std: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 mean [D] and rstd [D] on `device`; the reciprocal is taken in fp64 and rounded once"""
    m, s = mean.detach().reshape(-1), std.detach().reshape(-1)
    if m.numel() != s.numel() or m.numel() < 1:
        raise ValueError(f"probe_rows: mean and std must hold one value per channel, got {tuple(mean.shape)} and {tuple(std.shape)}")
    if not bool(((s > 0) & torch.isfinite(s)).all()):
        raise ValueError("probe_rows: every channel's std must be positive and finite")
    return m.to(device=device, dtype=torch.float32).contiguous(), (1.0 / s.double()).to(device=device, dtype=torch.float32).contiguous()


def probe_rows(latents: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, pool: Optional[int] = None) -> torch.Tensor:
    """fp32 latents [B, D, h, w] -> bf16 rows [B, ld], ld = g * g * D rounded up to a multiple of 32, pad columns 0.

    Every channel is average-pooled to a `pool` x `pool` grid (None: the grid as it is), standardised with `mean` / `std`
    ([D] or [1, D, 1, 1], as `latents_stats.pt` holds them) and rounded once.  Column order (py, px, c).  A channel slice of a wider
    tensor (`moments[:, :D]`) is read in place."""
    if latents.dim() != 4:
        raise ValueError(f"probe_rows: expected [B, D, h, w], got {tuple(latents.shape)}")
    B, D, h, w = latents.shape
    gh, gw = _grid(h, w, pool)
    if mean.numel() != D:
        raise ValueError(f"probe_rows: {D} channels but statistics of {mean.numel()}")
    ops._need_gpu(latents)
    ops._require(latents.dtype == torch.float32, "probe_rows: fp32 latents")
    if B == 0:
        return torch.empty((0, _round_up(gh * gw * D, 32)), dtype=torch.bfloat16, device=latents.device)
    m, r = _stat_vectors(mean, std, latents.device)
    return _probe_rows(latents, m, r, gh, gw)


class _SoftmaxXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, n_classes, eps, state, count):
        B, ld = logits.shape
        lib = L.load()
        with torch.cuda.device(logits.device):
            dl = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
            local = torch.zeros(4, dtype=torch.float64, device=logits.device)
            partials = torch.empty(lib.tv_softmax_xent_partial_count(B), dtype=torch.float64, device=logits.device)
            L.check(lib.tv_softmax_xent(ops._p(logits), ops._p(labels), ops._p(dl), ops._p(local), ops._p(partials), B, n_classes, ld, eps,
                                        1.0 / count, ops._stream()), "tv_softmax_xent")
            if state is not None:
                state.add_(local)
        ctx.dl = dl
        return (local[0] / count).float()

    @staticmethod
    def backward(ctx, gy):
        dl, ctx.dl = ctx.dl, None
        return dl.mul_(gy), None, None, None, None, None


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor, n_classes: int, label_smoothing: float = 0.0,
                 state: Optional[torch.Tensor] = None, count: Optional[int] = None) -> torch.Tensor:
    """Cross-entropy of bf16 logits [B, ld] (the first `n_classes` columns valid, ld % 8 == 0) against int64 labels [B]: the sum
    over the counted rows divided by `count` (default B), an fp32 scalar.  Backward hands out the gradient the forward pass stored.

    A label outside [0, n_classes) marks a row to ignore: zero gradient, not counted.  `state` (4 doubles on the device, see
    `new_xent_state`) is added to: {loss sum, rows counted, top-1 hits, top-5 hits}.  The pad columns never receive probability or
    smoothing mass."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError(f"softmax_xent: logits [B, ld] and labels [B], got {tuple(logits.shape)} and {tuple(labels.shape)}")
    B, ld = logits.shape
    if int(n_classes) < 2 or ld % 8 or ld < n_classes:
        raise ValueError(f"softmax_xent: n_classes={n_classes} must be at least 2 and ld={ld} a multiple of 8 that covers it")
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"softmax_xent: label_smoothing={label_smoothing} must be in [0, 1)")
    if B == 0 or (count is not None and count < 1):
        raise ValueError("softmax_xent: needs at least one row and a positive count")
    ops._need_gpu(logits, labels)
    ops._require(logits.dtype == torch.bfloat16 and logits.is_contiguous(), "softmax_xent: contiguous bf16 logits")
    ops._require(labels.dtype == torch.int64 and labels.is_contiguous() and labels.device == logits.device, "softmax_xent: contiguous int64 labels")
    if state is not None:
        ops._require(state.dtype == torch.float64 and state.numel() == 4 and state.is_contiguous() and state.device == logits.device,
                     "softmax_xent: state is 4 contiguous doubles on the logits' device")
    return _SoftmaxXentFn.apply(logits, labels, int(n_classes), float(label_smoothing), state, int(count or B))


def new_xent_state(device) -> torch.Tensor:
    """{loss sum, rows counted, top-1 hits, top-5 hits} as zeros: what `softmax_xent(state=...)` adds to"""
    return torch.zeros(4, dtype=torch.float64, device=device)


def read_xent_state(state: torch.Tensor) -> Dict[str, float]:
    """One synchronisation: {"loss", "top1", "top5", "n"} of the rows counted so far"""
    s, n, t1, t5 = state.tolist()
    if n == 0:
        raise ValueError("read_xent_state: no row was counted")
    return {"loss": s / n, "top1": t1 / n, "top5": t5 / n, "n": int(n)}


class LinearProbe(torch.nn.Module):
    """One linear layer on bf16 rows: `weight` [num_classes, in_features], `bias` [num_classes], fp32.

    forward(rows): rows bf16 [B, in_features rounded up to 32] (what `probe_rows` returns) -> bf16 logits
    [B, num_classes rounded up to 8]; the pad logits are exactly 0 and `softmax_xent(..., n_classes=num_classes)` never reads them.
    The input needs no gradient, so backward is the weight and bias gradient alone."""

    def __init__(self, in_features: int, num_classes: int, generator: Optional[torch.Generator] = None):
        super().__init__()
        if int(num_classes) < 2:
            raise ValueError(f"LinearProbe: num_classes={num_classes} must be at least 2")
        if int(in_features) < 1:
            raise ValueError(f"LinearProbe: in_features={in_features} must be positive")
        self.in_features, self.num_classes = int(in_features), int(num_classes)
        self.ld_in, self.ld_out = _round_up(self.in_features, 32), _round_up(self.num_classes, 8)
        gen = generator if generator is not None else torch.Generator().manual_seed(0)
        self.weight = torch.nn.Parameter(torch.randn(self.num_classes, self.in_features, generator=gen) * 0.01)
        self.bias = torch.nn.Parameter(torch.zeros(self.num_classes))

    @ops.hip_entry
    def forward(self, rows: torch.Tensor) -> torch.Tensor:
        ops._need_gpu(rows)
        if rows.dim() != 2 or rows.shape[1] != self.ld_in:
            raise ValueError(f"LinearProbe: expected rows [B, {self.ld_in}], got {tuple(rows.shape)}")
        w, b = self.weight, self.bias
        if self.ld_in != self.in_features or self.ld_out != self.num_classes:      # zero pad: no logit mass, no gradient kept
            w = F.pad(w, (0, self.ld_in - self.in_features, 0, self.ld_out - self.num_classes))
            b = F.pad(b, (0, self.ld_out - self.num_classes))
        return ops.linear(rows, w, b)


# ---------------------------------------------------------------------------------------------------------------------------
# data: an extract_latents directory or a (latents, labels) pair, one shard at a time
# ---------------------------------------------------------------------------------------------------------------------------
class _Shards:
    def __init__(self, src: Source, num_classes: int, what: str):
        self.num_classes, self.what = num_classes, what
        self.stats = None
        if isinstance(src, (str, os.PathLike)):
            self.dir = os.fspath(src)
            self.names = sorted(glob.glob(os.path.join(self.dir, "latents_shard*.pt")))
            if not self.names:
                raise ValueError(f"fit_linear_probe: no latents_shard*.pt in {self.dir}")
            sp = os.path.join(self.dir, "latents_stats.pt")
            if os.path.exists(sp):
                self.stats = torch.load(sp)
            self.pair = None
        elif isinstance(src, (tuple, list)) and len(src) == 2:
            self.dir, self.names = None, [f"the {what} pair"]
            self.pair = {"latents": src[0], "labels": src[1]}
        else:
            raise ValueError(f"fit_linear_probe: {what} must be an extract_latents directory or a (latents, labels) pair")
        self._cache = None
        self.sizes = [self.load(k)["labels"].shape[0] for k in range(len(self.names))]
        if sum(self.sizes) == 0:
            raise ValueError(f"fit_linear_probe: the {what} side is empty")

    def __len__(self):
        return len(self.names)

    def load(self, k: int) -> Dict[str, torch.Tensor]:
        """Shard k on the host, labels validated.  A single shard stays loaded."""
        if self._cache is not None and self._cache[0] == k:
            return self._cache[1]
        sh = self.pair if self.pair is not None else torch.load(self.names[k])
        name = self.names[k]
        if "labels" not in sh or sh["labels"] is None:
            raise ValueError(f"fit_linear_probe: {name} holds no labels (extract_latents writes them when the loader yields them)")
        lat, lab = sh["latents"], sh["labels"]
        if lat.dim() != 4 or lab.dim() != 1 or lab.shape[0] != lat.shape[0] or lat.dtype != torch.float32:
            raise ValueError(f"fit_linear_probe: {name}: latents fp32 [n, C, h, w] and labels [n], got {tuple(lat.shape)} {lat.dtype} and "
                             f"{tuple(lab.shape)}")
        lab = lab.to(torch.int64)
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= self.num_classes):
            raise ValueError(f"fit_linear_probe: {name} has a label outside [0, {self.num_classes}): "
                             f"min {int(lab.min())}, max {int(lab.max())}")
        out = {"latents": lat, "labels": lab}
        if sh.get("latents_flip") is not None:
            out["latents_flip"] = sh["latents_flip"]
        if len(self.names) == 1:
            self._cache = (k, out)
        return out


def _train_stats(train: _Shards, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """per-channel mean / std of the train side: `latents_stats.pt`, or `LatentStats` over the pair"""
    if train.stats is not None:
        return train.stats["mean"], train.stats["std"]
    if train.dir is not None:
        raise ValueError(f"fit_linear_probe: {train.dir} has no latents_stats.pt")
    lat = train.load(0)["latents"]
    st = LatentStats(lat.shape[1])
    for i in range(0, lat.shape[0], 4096):
        st.update(lat[i:i + 4096].to(device))
    return st.mean.float(), st.std.float()


def _evaluate(probe, val: _Shards, mean, rstd, D, pool, batch_size, device) -> Dict[str, float]:
    state = new_xent_state(device)
    with torch.no_grad():
        for k in range(len(val)):
            sh = val.load(k)
            lat, lab = sh["latents"].to(device), sh["labels"].to(device)
            gh, gw = _grid(lat.shape[2], lat.shape[3], pool)
            for i in range(0, lat.shape[0], batch_size):
                rows = _probe_rows(lat[i:i + batch_size, :D], mean, rstd, gh, gw)
                softmax_xent(probe(rows), lab[i:i + batch_size], probe.num_classes, 0.0, state)
    return read_xent_state(state)


def fit_linear_probe(train: Source, val: Source, num_classes: int, *, pool: Optional[int] = None, epochs: int, batch_size: int, lr: float,
                     weight_decay: float = 0.0, label_smoothing: float = 0.0, use_flip: bool = True, seed: int = 0,
                     device="cuda") -> Dict:
    """Train a `LinearProbe` on the train side's latents and report accuracy on the val side.

    `train` / `val`: an `extract_latents` output directory (its shards and `latents_stats.pt`; with what="moments" shards the mu
    half is used) or a `(latents fp32 [n, D, h, w], labels [n])` pair.  Features: `probe_rows(latents, mean, std, pool)` with the
    TRAIN side's per-channel statistics on both sides.  Shards stream one at a time, in an order drawn per epoch from a generator
    seeded with `seed + 1`, with a permutation within each shard; with `use_flip` and `latents_flip` in the shard, each sample is
    its mirrored version with probability 1/2, drawn by the same generator.  The weights start as N(0, 0.01^2) from a generator
    seeded with `seed`, the bias as 0.  `FusedAdamW`, learning rate `lr * (1 + cos(pi t / T)) / 2` at step t of T, set per step.
    Returns {"top1", "top5", "loss" (validation, after the last epoch), "history" (per epoch: train loss / top-1 with smoothing and
    augmentation on, validation loss / top-1 / top-5, the shard order), "n_train", "n_val", "probe"}."""
    if int(num_classes) < 2:
        raise ValueError(f"fit_linear_probe: num_classes={num_classes} must be at least 2")
    if epochs < 1 or batch_size < 1 or not lr > 0:
        raise ValueError("fit_linear_probe: epochs, batch_size and lr must be positive")
    tr, va = _Shards(train, int(num_classes), "train"), _Shards(val, int(num_classes), "val")
    first = tr.load(0)["latents"]
    gh, gw = _grid(first.shape[2], first.shape[3], pool)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("transvae.hip: this op only runs on a HIP device (MI355X); there is no CPU fallback")
    with torch.cuda.device(device):
        mean_t, std_t = _train_stats(tr, device)
        mean, rstd = _stat_vectors(mean_t, std_t, device)
        D = mean.numel()
        if first.shape[1] not in (D, 2 * D):
            raise ValueError(f"fit_linear_probe: shards of {first.shape[1]} channels but statistics of {D}")
        probe = LinearProbe(gh * gw * D, int(num_classes), generator=torch.Generator().manual_seed(int(seed))).to(device)
        opt = FusedAdamW(probe.parameters(), lr=lr, weight_decay=weight_decay)
        order_gen = torch.Generator().manual_seed(int(seed) + 1)
        total_steps = int(epochs) * sum(-(-n // batch_size) for n in tr.sizes)
        step, history = 0, []
        for epoch in range(int(epochs)):
            state = new_xent_state(device)
            order = torch.randperm(len(tr), generator=order_gen).tolist()
            for k in order:
                sh = tr.load(k)
                n = sh["labels"].shape[0]
                perm = torch.randperm(n, generator=order_gen)
                flip = sh.get("latents_flip") if use_flip else None
                mirrored = (torch.rand(n, generator=order_gen) < 0.5) if flip is not None else None
                lat, lab = sh["latents"].to(device), sh["labels"].to(device)
                flip = flip.to(device) if flip is not None else None
                for i in range(0, n, batch_size):
                    idx = perm[i:i + batch_size].to(device)
                    x = lat[idx]
                    if flip is not None:
                        x = torch.where(mirrored[perm[i:i + batch_size]].to(device).view(-1, 1, 1, 1), flip[idx], x)
                    for g in opt.param_groups:
                        g["lr"] = lr * 0.5 * (1.0 + math.cos(math.pi * step / total_steps))
                    opt.zero_grad(set_to_none=True)
                    logits = probe(_probe_rows(x[:, :D], mean, rstd, gh, gw))
                    softmax_xent(logits, lab[idx], probe.num_classes, label_smoothing, state).backward()
                    opt.step()
                    step += 1
                del lat, lab, flip
            tm = read_xent_state(state)
            vm = _evaluate(probe, va, mean, rstd, D, pool, batch_size, device)
            history.append({"epoch": epoch, "train_loss": tm["loss"], "train_top1": tm["top1"], "val_loss": vm["loss"], "val_top1": vm["top1"],
                            "val_top5": vm["top5"], "shard_order": order})
    last = history[-1]
    return {"top1": last["val_top1"], "top5": last["val_top5"], "loss": last["val_loss"], "history": history, "n_train": sum(tr.sizes),
            "n_val": sum(va.sizes), "probe": probe}


def linear_probe_accuracy(model: torch.nn.Module, train_loader: Iterable, val_loader: Iterable, num_classes: int, work_dir: str, *,
                          prep=None, **fit_args) -> Dict:
    """`extract_latents` of both loaders (posterior means; the mirrored latents of the train side when `use_flip` is on) into
    `work_dir/train` and `work_dir/val`, then `fit_linear_probe` on the two directories."""
    device = fit_args.get("device", "cuda")
    tdir, vdir = os.path.join(work_dir, "train"), os.path.join(work_dir, "val")
    extract_latents(model, train_loader, tdir, flip=bool(fit_args.get("use_flip", True)), prep=prep, device=device)
    extract_latents(model, val_loader, vdir, flip=False, prep=prep, device=device)
    return fit_linear_probe(tdir, vdir, num_classes, **fit_args)
