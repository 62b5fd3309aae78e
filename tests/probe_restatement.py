"""Restatements of transvae/probe.py and csrc/probe.hip: the yardsticks of tests/test_probe_host.py and tests/test_probe_gpu.py.

* float64 restatements of `tv_softmax_xent` (the tie rule as a stable descending sort) and `tv_probe_rows`, with the bounds of
  DESIGN.md section 3.1 row C;
* fp32 emulations of both kernels in the kernels' own order of operations, with switchable defects (the mutation tests);
* a plain-torch fp32 probe trainer with the init, batches and schedule of `fit_linear_probe`, and the synthetic problem it is
  checked on: 4 Gaussian blobs (sigma 1) in latent space [8, 4, 4] whose means are 16 sigma apart.

`python tests/probe_restatement.py --mint` writes tests/golden/probe_ref_bf16_autocast.json: the trainer's OWN deviation under
`torch.autocast("cpu", dtype=torch.bfloat16)` from its fp32 run (first-step gradients as rel-L2, the per-epoch loss relative).
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_ref_bf16_autocast.json")
U = 2.0 ** -24
F64 = torch.float64
LOG2E = 1.44269504088896340736


# ---------------------------------------------------------------------------------------------------------------------------
# tv_softmax_xent
# ---------------------------------------------------------------------------------------------------------------------------
def xent64(logits, labels, n, eps=0.0, scale=1.0):
    """float64 from the bf16 logits [B, ld] as given.  {"loss": sum over counted rows, "n", "top1", "top5", "d": scale (p - t) [B, ld]
    with pad columns and ignored rows 0, "slack": the fp32 allowance of row C on d, "valid": counted rows}"""
    B, ld = logits.shape
    x = logits[:, :n].to(F64)
    labels = labels.to(torch.int64)
    valid = (labels >= 0) & (labels < n)
    y = torch.where(valid, labels, torch.zeros_like(labels))
    m = x.max(1, keepdim=True).values
    lse = torch.logsumexp(x, 1)
    xy = x.gather(1, y[:, None])[:, 0]
    rows = lse - (1.0 - eps) * xy - (eps / n) * x.sum(1)
    p = torch.exp(x - lse[:, None])
    t = torch.full_like(p, eps / n)
    t.scatter_(1, y[:, None], 1.0 - eps + eps / n)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices        # ties keep the lower index first
    rank = (order == y[:, None]).to(torch.int64).argmax(1)
    d = torch.zeros(B, ld, dtype=F64)
    d[:, :n] = scale * (p - t) * valid[:, None]
    # s: a chain of 8 ceil(nvec / 64) adds per lane and 6 butterfly levels, each exponential 1 ulp (counted 2), the division
    # and the product by it; the exponent m - x is rounded once and multiplied by log2 e once: 2 |m - x| u relative
    k = 8 * math.ceil(math.ceil(n / 8) / 64) + 6 + 4
    slack = torch.zeros(B, ld, dtype=F64)
    slack[:, :n] = (abs(scale) * U * ((k + 2.0 * (m - x)) * p + 3.0 * t + 2.0 * (p - t).abs())
                    + 2.0 ** -126 * (1.0 + abs(scale))) * valid[:, None]       # fp32 results below the smallest normal may flush
    return {"loss": float(rows[valid].sum()), "n": int(valid.sum()), "top1": int((rank[valid] == 0).sum()), "top5": int((rank[valid] < 5).sum()),
            "d": d, "slack": slack, "valid": valid}


def _lane_layout(x, fill):
    """[B, n] -> [B, iters, 64, 8]: vector v = lane + 64 k holds columns 8 v .. 8 v + 7"""
    B, n = x.shape
    nvec = -(-n // 8)
    iters = -(-nvec // 64)
    full = torch.full((B, iters * 64 * 8), fill, dtype=x.dtype)
    full[:, :n] = x
    return full.view(B, iters, 64, 8)


def _wave_sum(v):
    """butterfly with the kernel's pairing: lane l adds lane l ^ o, o = 32 .. 1"""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def _chain(a):
    """per lane, over k then e in order, fp32: [B, iters, 64, 8] -> [B, 64]"""
    s = torch.zeros(a.shape[0], 64, dtype=a.dtype)
    for k in range(a.shape[1]):
        for e in range(8):
            s = s + a[:, k, :, e]
    return s


def xent_emulate(logits, labels, n, eps=0.0, scale=1.0, defect=None):
    """fp32 emulation of tv_softmax_xent in its own order -> {"loss", "n", "top1", "top5", "d" bf16 [B, ld]}.
    defect: None | "no_max" | "pad_in_sum" | "smooth_over_ld" | "round_before_scale" | "tie_ge"."""
    B, ld = logits.shape
    f32 = torch.float32
    cols = ld if defect == "pad_in_sum" else n
    x = logits[:, :cols].to(f32)
    labels = labels.to(torch.int64)
    valid = (labels >= 0) & (labels < n)
    y = torch.where(valid, labels, torch.zeros_like(labels))
    xy = x.gather(1, y[:, None])
    m = torch.zeros(B, 1) if defect == "no_max" else x.max(1, keepdim=True).values
    j = torch.arange(cols)[None, :]
    if defect == "tie_ge":
        rank = ((x >= xy) & (j != y[:, None])).sum(1)
    else:
        rank = (x > xy).sum(1) + ((x == xy) & (j < y[:, None])).sum(1)
    dd = m - x
    e = torch.exp2(dd * torch.tensor(-LOG2E, dtype=f32))
    s = _wave_sum(_chain(_lane_layout(e, 0.0)))
    q = _wave_sum(_chain(_lane_layout(dd, 0.0)))
    nn = ld if defect == "smooth_over_ld" else n
    eps32 = torch.tensor(eps, dtype=f32)
    rows = torch.log(s).to(F64) + (1.0 - eps32.to(F64)) * (m - xy)[:, 0].to(F64) + (eps32.to(F64) / nn) * q.to(F64)
    t_miss = eps32 / torch.tensor(float(nn), dtype=f32)
    t_hit = (torch.tensor(1.0, dtype=f32) - eps32) + t_miss
    t = t_miss.expand(B, cols).clone()
    t.scatter_(1, y[:, None], t_hit.expand(B, 1))
    p = e * (torch.tensor(1.0, dtype=f32) / s)[:, None]
    sc = torch.tensor(scale, dtype=f32)
    if defect == "round_before_scale":
        g = (sc * (p - t).bfloat16().to(f32)).bfloat16()
    else:
        g = (sc * (p - t)).bfloat16()
    d = torch.zeros(B, ld, dtype=torch.bfloat16)
    d[:, :n] = torch.where(valid[:, None], g[:, :n], torch.zeros((), dtype=torch.bfloat16))
    return {"loss": float(rows[valid].sum()), "n": int(valid.sum()), "top1": int((rank[valid] == 0).sum()), "top5": int((rank[valid] < 5).sum()),
            "d": d}


def xent_inputs(B, n, ld, scale, seed, tied=False, bad_labels=True):
    """bf16 logits [B, ld] (pad columns hold a sentinel: a kernel that reads them shows), int64 labels with about a quarter out of
    range.  tied: the logits take 8 distinct bf16 values."""
    g = torch.Generator().manual_seed(seed)
    if tied:
        levels = torch.tensor([-2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0]) * scale
        x = levels[torch.randint(0, 8, (B, ld), generator=g)]
    else:
        x = torch.randn(B, ld, generator=g) * scale
    x[:, n:] = 60.0
    labels = torch.randint(0, n, (B,), generator=g)
    if bad_labels:
        bad = torch.rand(B, generator=g) < 0.25
        bad[0] = False
        labels = torch.where(bad, torch.where(torch.rand(B, generator=g) < 0.5, torch.full_like(labels, -1), torch.full_like(labels, n)), labels)
    return x.bfloat16(), labels


# ---------------------------------------------------------------------------------------------------------------------------
# tv_probe_rows
# ---------------------------------------------------------------------------------------------------------------------------
def grid_of(h, w, pool):
    return (h, w) if pool is None else (int(pool), int(pool))


def rows64(lat, mean, rstd, gh, gw):
    """float64 from the fp32 inputs as given -> (rows [B, ld] with zero pad, slack [B, ld]): the fp32 window sum carries
    (win - 1) u sum|x|, the reciprocal of a window that is no power of two and its product 2 u |v|, the difference and the product
    by rstd u each"""
    B, D, h, w = lat.shape
    wh, ww = h // gh, w // gw
    win = wh * ww
    x = lat.to(F64).view(B, D, gh, wh, gw, ww)
    v = x.mean((3, 5))
    absmean = x.abs().mean((3, 5))
    mu, rs = mean.to(F64).view(1, D, 1, 1), rstd.to(F64).view(1, D, 1, 1)
    y = (v - mu) * rs
    pow2 = (win & (win - 1)) == 0
    sl = rs * U * ((win - 1) * absmean + (0.0 if pow2 else 2.0) * v.abs()) + 2.0 * U * y.abs()
    Fc = gh * gw * D
    ld = -(-Fc // 32) * 32
    out, slack = torch.zeros(B, ld, dtype=F64), torch.zeros(B, ld, dtype=F64)
    out[:, :Fc] = y.permute(0, 2, 3, 1).reshape(B, Fc)
    slack[:, :Fc] = sl.permute(0, 2, 3, 1).reshape(B, Fc)
    return out, slack


def rows_emulate(lat, mean, rstd, gh, gw, defect=None):
    """fp32 emulation of tv_probe_rows: the window summed in scan order, one product by 1 / window, (v - mean) * rstd, one rounding.
    defect: None | "pool_after_round" | "order_cpp" (columns (c, py, px))."""
    B, D, h, w = lat.shape
    wh, ww = h // gh, w // gw
    mu, rs = mean.float().view(1, D, 1, 1), rstd.float().view(1, D, 1, 1)
    x = lat.float().view(B, D, gh, wh, gw, ww)
    inv = torch.tensor(1.0 / (wh * ww), dtype=torch.float32)
    if defect == "pool_after_round":
        x = ((lat.float() - mu) * rs).bfloat16().float().view(B, D, gh, wh, gw, ww)
    s = torch.zeros(B, D, gh, gw)
    for i in range(wh):
        for j in range(ww):
            s = s + x[:, :, :, i, :, j]
    v = s * inv
    y = v.bfloat16() if defect == "pool_after_round" else ((v - mu) * rs).bfloat16()
    Fc = gh * gw * D
    out = torch.zeros(B, -(-Fc // 32) * 32, dtype=torch.bfloat16)
    out[:, :Fc] = (y if defect == "order_cpp" else y.permute(0, 2, 3, 1)).reshape(B, Fc)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the synthetic problem and the plain-torch trainer
# ---------------------------------------------------------------------------------------------------------------------------
NUM_CLASSES = 4
SIGNS = torch.tensor([[1, 1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, -1, -1, -1, -1], [1, 1, -1, -1, 1, 1, -1, -1], [1, -1, 1, -1, 1, -1, 1, -1]],
                     dtype=torch.float32)          # class means: +-1 per channel, constant over the 4 x 4 grid; any two classes differ in
#                                                    4 channels x 16 positions by 2: 16 sigma apart (4 / 0.25 = 16 sigma after pool=1)
FIT_ARGS = dict(epochs=3, batch_size=64, lr=0.01, weight_decay=0.01, label_smoothing=0.1, use_flip=True)
TRAIN_SHARDS, VAL_SHARDS = (300, 212), (128, 128)


def blob_split(sizes, seed):
    """[{"latents" [n, 8, 4, 4], "latents_flip", "labels"}] per shard"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        labels = torch.randint(0, NUM_CLASSES, (n,), generator=g)
        lat = SIGNS[labels].view(n, 8, 1, 1) + torch.randn(n, 8, 4, 4, generator=g)
        out.append({"latents": lat.contiguous(), "latents_flip": torch.flip(lat, dims=[3]).contiguous(), "labels": labels})
    return out


def split_stats(shards):
    """per-channel population mean / std over every position, fp32 [1, D, 1, 1] as latents_stats.pt holds them"""
    x = torch.cat([s["latents"] for s in shards]).double()
    D = x.shape[1]
    return {"mean": x.mean((0, 2, 3)).float().view(1, D, 1, 1), "std": x.std((0, 2, 3), unbiased=False).float().view(1, D, 1, 1)}


def decoy_stats(stats):
    """what the VAL directory's latents_stats.pt holds in the GPU test: statistics fit_linear_probe must not read.  Features built
    with them move class 0 (channels 4 .. 7 at +1) onto class 1 (-1)"""
    mean = stats["mean"].clone()
    mean[0, 4:] += 2.0 * stats["std"][0, 4:].mean()
    return {"mean": mean, "std": stats["std"].clone()}


def write_split(path, shards, stats):
    os.makedirs(path, exist_ok=True)
    for k, s in enumerate(shards):
        torch.save(s, os.path.join(path, f"latents_shard{k:03d}.pt"))
    torch.save(stats, os.path.join(path, "latents_stats.pt"))


def epoch_plan(gen, sizes, batch_size, has_flip):
    """one epoch of fit_linear_probe's draws from `gen`: (shard order, [(shard, sample indices, mirrored flags | None)])"""
    order = torch.randperm(len(sizes), generator=gen).tolist()
    batches = []
    for k in order:
        perm = torch.randperm(sizes[k], generator=gen)
        mirrored = (torch.rand(sizes[k], generator=gen) < 0.5) if has_flip else None
        for i in range(0, sizes[k], batch_size):
            idx = perm[i:i + batch_size]
            batches.append((k, idx, None if mirrored is None else mirrored[idx]))
    return order, batches


def features32(lat, stats, pool):
    """plain fp32: average pooling, (v - mean) / std, columns (py, px, c)"""
    B, D, h, w = lat.shape
    gh, gw = grid_of(h, w, pool)
    v = F.avg_pool2d(lat, (h // gh, w // gw))
    return ((v - stats["mean"]) / stats["std"]).permute(0, 2, 3, 1).reshape(B, gh * gw * D)


def train_probe(train, val, stats, num_classes, *, pool=None, epochs, batch_size, lr, weight_decay=0.0, label_smoothing=0.0, use_flip=True,
                seed=0, autocast=False, grad_sign=1.0):
    """The probe in plain torch on shard lists -> {"history": [{"train_loss", "val_loss", "val_top1", "shard_order"}], "first_wgrad",
    "first_bgrad"}.  autocast: the linear layer under torch.autocast("cpu", bfloat16), the loss in fp32.  grad_sign = -1: the defect."""
    sizes = [s["labels"].shape[0] for s in train]
    has_flip = use_flip and all("latents_flip" in s for s in train)
    feat = features32(train[0]["latents"][:1], stats, pool).shape[1]
    W = (torch.randn(num_classes, feat, generator=torch.Generator().manual_seed(seed)) * 0.01).requires_grad_(True)
    b = torch.zeros(num_classes, requires_grad=True)
    opt = torch.optim.AdamW([W, b], lr=lr, weight_decay=weight_decay)
    gen = torch.Generator().manual_seed(seed + 1)
    total = epochs * sum(-(-n // batch_size) for n in sizes)

    def logits_of(x):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            return F.linear(x, W, b).float()
    step, history, first = 0, [], None
    for _ in range(epochs):
        order, batches = epoch_plan(gen, sizes, batch_size, has_flip)
        tot = 0.0
        for k, idx, mirrored in batches:
            lat = train[k]["latents"][idx]
            if mirrored is not None:
                lat = torch.where(mirrored.view(-1, 1, 1, 1), train[k]["latents_flip"][idx], lat)
            for g in opt.param_groups:
                g["lr"] = lr * 0.5 * (1.0 + math.cos(math.pi * step / total))
            opt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(logits_of(features32(lat, stats, pool)), train[k]["labels"][idx], label_smoothing=label_smoothing)
            loss.backward()
            if first is None:
                first = (W.grad.detach().clone(), b.grad.detach().clone())
            if grad_sign != 1.0:
                W.grad.mul_(grad_sign)
                b.grad.mul_(grad_sign)
            opt.step()
            tot += float(loss.detach()) * idx.numel()
            step += 1
        with torch.no_grad():
            vl = torch.cat([logits_of(features32(s["latents"], stats, pool)) for s in val])
            vy = torch.cat([s["labels"] for s in val])
            history.append({"train_loss": tot / sum(sizes), "val_loss": float(F.cross_entropy(vl, vy)),
                            "val_top1": float((vl.argmax(1) == vy).float().mean()), "shard_order": order})
    return {"history": history, "first_wgrad": first[0], "first_bgrad": first[1], "W": W.detach(), "b": b.detach()}


def step_case():
    """the single training step of the GPU test: bf16 rows [96, 64], 10 classes"""
    g = torch.Generator().manual_seed(77)
    rows = torch.randn(96, 64, generator=g).bfloat16()
    labels = torch.randint(0, 10, (96,), generator=g)
    W = torch.randn(10, 64, generator=g) * 0.1
    b = torch.randn(10, generator=g) * 0.1
    return rows, labels, W, b


def step_grads(rows, labels, W, b, label_smoothing=0.1, autocast=False):
    W, b = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        logits = F.linear(rows.float(), W, b).float()
    loss = F.cross_entropy(logits, labels, label_smoothing=label_smoothing)
    loss.backward()
    return float(loss.detach()), W.grad.detach(), b.grad.detach()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def mint():
    out = {}
    l32, w32, b32 = step_grads(*step_case())
    l16, w16, b16 = step_grads(*step_case(), autocast=True)
    out["step"] = {"weight_grad": rel_l2(w16, w32), "bias_grad": rel_l2(b16, b32), "loss": abs(l16 - l32) / l32}
    train, val = blob_split(TRAIN_SHARDS, 1), blob_split(VAL_SHARDS, 2)
    stats = split_stats(train)
    for pool in (None, 1):
        r32 = train_probe(train, val, stats, NUM_CLASSES, pool=pool, **FIT_ARGS)
        r16 = train_probe(train, val, stats, NUM_CLASSES, pool=pool, autocast=True, **FIT_ARGS)
        out[f"fit:pool={pool}"] = {
            "first_weight_grad": rel_l2(r16["first_wgrad"], r32["first_wgrad"]),
            "train_loss": [abs(a["train_loss"] - c["train_loss"]) / c["train_loss"] for a, c in zip(r16["history"], r32["history"])],
            "val_loss": [abs(a["val_loss"] - c["val_loss"]) / c["val_loss"] for a, c in zip(r16["history"], r32["history"])],
            "val_top1_fp32": [c["val_top1"] for c in r32["history"]]}
    for k, v in out.items():
        print(k, v, flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "deviation of the plain-torch probe trainer under torch.autocast('cpu', bfloat16) from its fp32 run: first-step "
                           "gradients as rel-L2, per-epoch losses relative", "torch": torch.__version__, "cases": out}, f, indent=1)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        mint()
