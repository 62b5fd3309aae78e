"""The latent DiT of transvae/dit.py and csrc/dit.hip restated in plain torch (the project's own definition):

  * `DiTRef`: the module with the same state-dict keys, runnable in fp32 / fp64 and under bf16 autocast with a bf16-rounded
    residual stream; `flow_step` (loss + gradients), `sample` (Euler + classifier-free guidance), `train_steps` (AdamW on one batch);
  * fp64 references of the seven kernels with the slack of their DESIGN.md section 3.1 row E;
  * fp32 emulations of each kernel in its own order of operations, and the same emulations with named defects.

`python tests/dit_restatement.py --mint` writes tests/golden/dit_ref_bf16_autocast.json: the restatement's OWN relL2 deviation of
the bf16-autocast form from fp32 for the whole-model cases of tests/test_dit_gpu.py, per output and gradient tensor, the sampler
case, and the two losses of the training case, with the seeds they were minted with.
"""
import json
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
LN_EPS = 1e-6
TIME_SCALE = 1000.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_ref_bf16_autocast.json")

# whole-model cases of the GPU test: width 128, depth 2, 10 classes, B = 3 (one label is the null class)
MODEL_CASES = {"f16d32_p1": dict(in_channels=32, input_size=(8, 8), patch_size=1),
               "f8d16_p2": dict(in_channels=16, input_size=(16, 16), patch_size=2)}
MODEL_ARGS = dict(hidden_size=128, depth=2, num_classes=10)
MODEL_B = 3
SAMPLER = dict(case="f16d32_p1", steps=4, cfg_scale=1.5)
TRAIN = dict(case="f16d32_p1", steps=30, lr=2e-3)       # lr chosen on the CPU so that the fp32 restatement ends below a quarter


def rel_l2(a, b):
    a, b = a.detach().to(F64).cpu(), b.detach().to(F64).cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def r16(t):
    return t.to(F32).to(BF)


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def patchify(x, p):
    """[B, D, h, w] -> [B, N, p p D], token (ty, tx) row ty (w / p) + tx, column (py p + px) D + c"""
    B, D, h, w = x.shape
    return x.reshape(B, D, h // p, p, w // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, (h // p) * (w // p), p * p * D)


def unpatchify(rows, D, h, w, p):
    B = rows.shape[0]
    return rows.reshape(B, h // p, w // p, p, p, D).permute(0, 5, 1, 3, 2, 4).reshape(B, D, h, w)


def rope_tables(gh, gw, dtype):
    """the model's 2-D RoPE (transvae/modules/attention.py): angle vector [y f, y f, x f, x f], f = 10000^(-2 i / 32), i < 16;
    pair q uses angle[2 q] for its first output and angle[2 q + 1] for its second"""
    f = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    ys = torch.arange(gh, dtype=F32).repeat_interleave(gw)
    xs = torch.arange(gw, dtype=F32).repeat(gh)
    yf, xf = torch.outer(ys, f), torch.outer(xs, f)
    ang = torch.cat([yf, yf, xf, xf], dim=-1)
    t1, t2 = ang[:, 0::2], ang[:, 1::2]
    return tuple(t.to(dtype) for t in (t1.cos(), t1.sin(), t2.cos(), t2.sin()))      # (fp32 angles, as the model's table builder)


def rope_apply(t, tabs):
    c1, s1, c2, s2 = tabs
    a, b = t[..., 0::2], t[..., 1::2]
    return torch.stack([a * c1 - b * s1, a * s2 + b * c2], dim=-1).flatten(-2)


def timestep_embedding(t, dim):
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32, device=t.device) / half).to(t.dtype)
    args = t[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


class _Seq(nn.Module):
    pass


class DiTRef(nn.Module):
    def __init__(self, input_size, patch_size, in_channels, hidden_size, depth, num_classes, mlp_ratio=4.0, freq=256):
        super().__init__()
        C = hidden_size
        self.input_size, self.p, self.D, self.C, self.depth, self.num_classes, self.freq = tuple(input_size), patch_size, in_channels, C, depth, num_classes, freq
        self.x_embedder = _Seq()
        self.x_embedder.proj = nn.Conv2d(in_channels, C, patch_size, patch_size)
        self.t_embedder = _Seq()
        self.t_embedder.mlp = nn.Sequential(nn.Linear(freq, C), nn.SiLU(), nn.Linear(C, C))
        self.y_embedder = _Seq()
        self.y_embedder.embedding_table = nn.Embedding(num_classes + 1, C)
        self.blocks = nn.ModuleList()
        for _ in range(depth):
            b = _Seq()
            b.attn = _Seq()
            b.attn.qkv, b.attn.proj = nn.Linear(C, 3 * C), nn.Linear(C, C)
            b.mlp = _Seq()
            b.mlp.fc1, b.mlp.fc2 = nn.Linear(C, int(C * mlp_ratio)), nn.Linear(int(C * mlp_ratio), C)
            b.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(C, 6 * C))
            self.blocks.append(b)
        self.final_layer = _Seq()
        self.final_layer.linear = nn.Linear(C, patch_size * patch_size * in_channels)
        self.final_layer.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(C, 2 * C))

    def forward(self, x, t, y, bf16_stream=False):
        """x [B, D, h, w] normalised (x_t), t [B], y [B] -> velocity [B, D, h, w].  bf16_stream: the residual stream and every
        branch operand are rounded to bf16 where the HIP path stores bf16 (call it under torch.autocast(bf16))."""
        rnd = (lambda v: v.to(BF).to(v.dtype) if v.dtype != BF else v) if bf16_stream else (lambda v: v)
        dt = self.x_embedder.proj.weight.dtype
        B, D, h, w = x.shape
        p, C = self.p, self.C
        gh, gw = h // p, w // p
        N, heads = gh * gw, C // 64
        dev = x.device.type
        with torch.autocast(dev, enabled=False):         # the conditioning path is fp32 on the HIP path as well
            c = self.t_embedder.mlp(timestep_embedding(t.to(dt) * TIME_SCALE, self.freq)) + self.y_embedder.embedding_table(y)
            mods = [b.adaLN_modulation(c) for b in self.blocks]
            modf = self.final_layer.adaLN_modulation(c)
        we = self.x_embedder.proj.weight.permute(0, 2, 3, 1).reshape(C, p * p * D)
        hcur = rnd(F.linear(rnd(patchify(x, p)), we, self.x_embedder.proj.bias).to(dt))
        tabs = tuple(tb.to(x.device) for tb in rope_tables(gh, gw, dt))

        def ln_mod(v, shift, scale):
            with torch.autocast(dev, enabled=False):
                return rnd(F.layer_norm(v.to(dt), (C,), eps=LN_EPS) * (1 + scale[:, None]) + shift[:, None])
        for b, mod in zip(self.blocks, mods):
            s1, k1, g1, s2, k2, g2 = mod.chunk(6, dim=1)
            qkv = rnd(F.linear(ln_mod(hcur, s1, k1), b.attn.qkv.weight, b.attn.qkv.bias).to(dt))
            q, k, v = [u.reshape(B, N, heads, 64).transpose(1, 2) for u in qkv.chunk(3, dim=-1)]
            q, k = rnd(rope_apply(q, tabs)), rnd(rope_apply(k, tabs))
            o = F.scaled_dot_product_attention(q, k, v).to(dt)
            a = rnd(F.linear(rnd(o.transpose(1, 2).reshape(B, N, C)), b.attn.proj.weight, b.attn.proj.bias).to(dt))
            hcur = rnd(hcur + g1[:, None] * a)
            m = rnd(F.gelu(F.linear(ln_mod(hcur, s2, k2), b.mlp.fc1.weight, b.mlp.fc1.bias)).to(dt))
            m = rnd(F.linear(m, b.mlp.fc2.weight, b.mlp.fc2.bias).to(dt))
            hcur = rnd(hcur + g2[:, None] * m)
        sf, kf = modf.chunk(2, dim=1)
        out = rnd(F.linear(ln_mod(hcur, sf, kf), self.final_layer.linear.weight, self.final_layer.linear.bias).to(dt))
        return unpatchify(out, D, h, w, p)


def state_dict_keys(depth):
    keys = ["x_embedder.proj", "t_embedder.mlp.0", "t_embedder.mlp.2"]
    for i in range(depth):
        keys += [f"blocks.{i}.attn.qkv", f"blocks.{i}.attn.proj", f"blocks.{i}.mlp.fc1", f"blocks.{i}.mlp.fc2", f"blocks.{i}.adaLN_modulation.1"]
    keys += ["final_layer.linear", "final_layer.adaLN_modulation.1"]
    out = [k + s for k in keys for s in (".weight", ".bias")]
    out.insert(6, "y_embedder.embedding_table.weight")
    return out


ZERO_INIT = ("adaLN_modulation.1", "final_layer.linear")


def make_state(case, seed, randomize_zero_init):
    """A seeded state dict for a whole-model case: the public initialisation (Xavier-uniform linears, zero biases, N(0, 0.02^2)
    embedders, zeros for every adaLN_modulation.1 and final_layer.linear); randomize_zero_init draws the zero-initialised
    tensors as N(0, 0.05^2) instead (weights) / N(0, 0.1^2) (biases), which opens every gate."""
    g = torch.Generator().manual_seed(seed)
    m = DiTRef(**MODEL_CASES[case], **MODEL_ARGS)
    sd = {}
    for k, v in m.state_dict().items():
        zero = any(z in k for z in ZERO_INIT)
        if zero:
            sd[k] = (torch.randn(v.shape, generator=g) * (0.05 if k.endswith("weight") else 0.1)) if randomize_zero_init else torch.zeros_like(v)
        elif k.endswith("bias"):
            sd[k] = torch.zeros_like(v)
        elif "embedding_table" in k or "t_embedder" in k:
            sd[k] = torch.randn(v.shape, generator=g) * 0.02
        else:
            a = math.sqrt(6.0 / (v.shape[0] + v[0].numel()))
            sd[k] = (torch.rand(v.shape, generator=g) * 2 - 1) * a
    return sd


def make_batch(case, seed, B=MODEL_B):
    """latents (the mu half of a moments tensor), statistics, labels (the last one the null class), t and noise of a case"""
    cfg = MODEL_CASES[case]
    g = torch.Generator().manual_seed(seed)
    D, (h, w) = cfg["in_channels"], cfg["input_size"]
    moments = torch.randn(B, 2 * D, h, w, generator=g) * 1.5 + 0.3
    stats = {"mean": torch.full((1, D, 1, 1), 0.3) + 0.1 * torch.randn(1, D, 1, 1, generator=g),
             "std": 1.5 + 0.2 * torch.rand(1, D, 1, 1, generator=g)}
    labels = torch.randint(0, MODEL_ARGS["num_classes"], (B,), generator=g)
    labels[-1] = MODEL_ARGS["num_classes"]
    t = torch.rand(B, generator=g)
    noise = torch.randn(B, D, h, w, generator=g)
    return {"moments": moments, "latents": moments[:, :D], "stats": stats, "labels": labels, "t": t, "noise": noise}


def build(case, sd, dtype=F32):
    m = DiTRef(**MODEL_CASES[case], **MODEL_ARGS)
    m.load_state_dict(sd)
    return m.to(dtype)


def flow_step(model, batch, autocast=False):
    """loss and gradients of one flow-matching step -> (velocity [B, D, h, w], loss, {name: grad})"""
    dt = next(model.parameters()).dtype
    mean, std = batch["stats"]["mean"].to(dt), batch["stats"]["std"].to(dt)
    x = (batch["latents"].to(dt) - mean) / std
    e, t = batch["noise"].to(dt), batch["t"].to(dt)
    tt = t.view(-1, 1, 1, 1)
    xt = tt * x + (1 - tt) * e
    model.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        v = model(xt, t, batch["labels"], bf16_stream=autocast)
    loss = ((v.to(dt) - (x - e)) ** 2).mean()
    loss.backward()
    return v.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@torch.no_grad()
def sample(model, labels, noise, stats, steps, cfg_scale, autocast=False):
    dt = next(model.parameters()).dtype
    x = noise.to(dt).clone()
    null = torch.full_like(labels, model.num_classes)
    for i in range(steps):
        t = torch.full((labels.shape[0],), i / steps, dtype=dt)
        with torch.autocast("cpu", dtype=BF, enabled=autocast):
            vc = model(x, t, labels, bf16_stream=autocast).to(dt)
            if cfg_scale != 1.0:
                vu = model(x, t, null, bf16_stream=autocast).to(dt)
                vc = vu + cfg_scale * (vc - vu)
        x = x + vc / steps
    return x * stats["std"].to(dt) + stats["mean"].to(dt)


def train_steps(model, batch, steps, lr):
    """`steps` AdamW updates (weight decay 0) on one fixed batch with fixed t and noise -> the list of losses"""
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    losses = []
    for _ in range(steps + 1):
        _, loss, _ = flow_step(model, batch)
        losses.append(float(loss))
        opt.step()
    return losses


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references of the kernels with the slack of DESIGN.md section 3.1 row E
# ---------------------------------------------------------------------------------------------------------------------------
def k_s(C):
    """adds behind one row sum: the lane's chain of 8 ceil(C / 512) terms and the six butterfly steps"""
    return 8 * math.ceil(C / 512) + 6


def k_rows_adaln(N):
    """adds behind a column sum of tv_adaln_bwd: 16 rows per wave in a slab of 64, four waves, the slabs"""
    return 16 + 4 + math.ceil(N / 64)


def gate_lanes(C):
    return 256 // (C // 8)


def k_rows_gate(N, C):
    L = gate_lanes(C)
    return math.ceil(64 / L) + L + math.ceil(N / 64)


def _stats64(x, eps=LN_EPS):
    x = x.to(F64)
    mu = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    return (x - mu) * rstd, mu, rstd


def _xhat_err(xh, mu, rstd, C):
    """|xhat32 - xhat64| of the two-pass fp32 statistics: A u cond (1 + |xhat|), A = 1.5 k_s + 5, cond = 1 + |mu| rstd"""
    return U * (1.5 * k_s(C) + 5) * (1 + mu.abs() * rstd) * (1 + xh.abs())


def _per_row(v, N):
    return v.repeat_interleave(N, dim=0)


def adaln_fwd64(x, shift, scale, N):
    """x bf16 [B N, C], shift / scale fp32 [B, C] -> (y64, slack)"""
    C = x.shape[1]
    xh, mu, rstd = _stats64(x)
    k1 = 1 + _per_row(scale.to(F64), N)
    sh = _per_row(shift.to(F64), N)
    y = xh * k1 + sh
    slack = k1.abs() * _xhat_err(xh, mu, rstd, C) + 2 * U * ((xh * k1).abs() + y.abs())
    return y, slack


def adaln_bwd64(x, scale, dy, dres, N):
    """-> {"dx", "dx_slack", "dshift", "dshift_terms", "dscale", "dscale_bound"}: dx one rounding; the sums fp32"""
    T, C = x.shape
    B = T // N
    xh, mu, rstd = _stats64(x)
    k1 = 1 + _per_row(scale.to(F64), N)
    d = dy.to(F64)
    g = d * k1
    mean = lambda t: t.mean(1, keepdim=True)
    a1, a2 = mean(g), mean(g * xh)
    inner = g - a1 - xh * a2
    dx = rstd * inner
    exh = _xhat_err(xh, mu, rstd, C)
    ks = k_s(C)
    cond = 1 + mu.abs() * rstd
    d_a1 = (ks + 3) * U * mean(g.abs())
    d_a2 = (ks + 3) * U * mean((g * xh).abs()) + mean(g.abs() * exh)
    d_inner = 2 * U * g.abs() + d_a1 + xh.abs() * d_a2 + a2.abs() * exh + 3 * U * (g.abs() + a1.abs() + (xh * a2).abs())
    d_rstd = U * (ks * cond + ks / 2 + 2)
    slack = rstd * d_inner + dx.abs() * (d_rstd + 2 * U)
    if dres is not None:
        dx = dx + dres.to(F64)
        slack = slack + U * dres.to(F64).abs()
    slack = slack + U * dx.abs()
    kr = k_rows_adaln(N)
    dshift = d.view(B, N, C).sum(1)
    dscale = (d * xh).view(B, N, C).sum(1)
    dscale_bound = U * (kr + 1) * (d * xh).abs().view(B, N, C).sum(1) + (d.abs() * exh).view(B, N, C).sum(1)
    return {"dx": dx, "dx_slack": slack, "dshift": dshift, "dshift_terms": d.abs().view(B, N, C).sum(1), "k_rows": kr,
            "dscale": dscale, "dscale_bound": dscale_bound}


def gate_fwd64(x, y, gate, N):
    out = _per_row(gate.to(F64), N) * y.to(F64) + x.to(F64)
    return out, U * out.abs()


def gate_bwd64(dout, y, gate, N):
    T, C = y.shape
    B = T // N
    dy = _per_row(gate.to(F64), N) * dout.to(F64)
    prod = dout.to(F64) * y.to(F64)
    return {"dy": dy, "dy_slack": U * dy.abs(), "dgate": prod.view(B, N, C).sum(1), "dgate_terms": prod.abs().view(B, N, C).sum(1),
            "k_rows": k_rows_gate(N, C)}


def _pad_cols(rows, ld):
    return F.pad(rows, (0, ld - rows.shape[-1]))


def round_up(n, k):
    return -(-n // k) * k


def flow_rows64(lat, mean, rstd, noise, t, p):
    """-> (rows64 [B N, ld] with zero pad columns, slack); noise None: the rows of x"""
    B, D, h, w = lat.shape
    ld = round_up(p * p * D, 32)
    x = (lat.to(F64) - mean.to(F64).view(1, D, 1, 1)) * rstd.to(F64).view(1, D, 1, 1)
    if noise is None:
        y, slack = x, 2 * U * x.abs()
    else:
        tt = t.to(F64).view(B, 1, 1, 1)
        e = noise.to(F64)
        y = tt * x + (1 - tt) * e
        slack = U * (2 * (tt * x).abs() + 2 * ((1 - tt) * e).abs() + y.abs())
    flat = lambda v: _pad_cols(patchify(v, p).reshape(-1, p * p * D), ld)
    return flat(y), flat(slack)


def flow_loss64(pred, lat, mean, rstd, noise, p, grad_scale=1.0):
    """-> {"loss", "sum", "dpred", "slack"}: the mean over the real columns, and bf16-once gradient rows (pad columns exactly 0)"""
    B, D, h, w = lat.shape
    F_ = p * p * D
    ld = round_up(F_, 32)
    x = (lat.to(F64) - mean.to(F64).view(1, D, 1, 1)) * rstd.to(F64).view(1, D, 1, 1)
    v = patchify(x - noise.to(F64), p).reshape(-1, F_)
    xa = patchify(x.abs(), p).reshape(-1, F_)
    d = pred.to(F64)[:, :F_] - v
    count = d.numel()
    coef = 2.0 * grad_scale / count
    dpred = coef * d
    slack = abs(coef) * U * (2 * xa + v.abs() + 3 * d.abs()) + U * dpred.abs()
    return {"loss": float((d * d).sum() / count), "sum": float((d * d).sum()), "dpred": _pad_cols(dpred, ld), "slack": _pad_cols(slack, ld)}


def flow_euler64(x, v, p, dt, cfg_scale=None):
    """-> (x' 64 [B, D, h, w], absterms for check_fp32 with c = 1)"""
    B, D, h, w = x.shape
    F_ = p * p * D
    N = (h // p) * (w // p)
    v = v.to(F64)[:, :F_]
    if cfg_scale is None:
        vel, inner = v, torch.zeros_like(v)
    else:
        vc, vu = v[:B * N], v[B * N:]
        inner = cfg_scale * (vc - vu)
        vel = vu + inner
    un = lambda r: unpatchify(r.reshape(B, N, F_), D, h, w, p)
    return x.to(F64) + dt * un(vel), abs(dt) * (un(inner.abs()) + un(vel.abs()))


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' own order (defect=...: the same with a named defect)
# ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fma: the product is exact in fp64"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _lanes(x):
    """[T, C] -> [T, KCH, 64, 8]: chunk ch = lane + 64 k holds columns 8 ch .. 8 ch + 7 (zeros past the row), and the mask"""
    T, C = x.shape
    kch = math.ceil(C / 512)
    full = torch.zeros(T, kch * 512, dtype=x.dtype)
    full[:, :C] = x
    mask = torch.zeros(kch * 512, dtype=torch.bool)
    mask[:C] = True
    return full.view(T, kch, 64, 8), mask.view(1, kch, 64, 8)


def _unlanes(v, C):
    return v.reshape(v.shape[0], -1)[:, :C]


def _wave_sum(v):
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, :1]


def _chain(a, b=None):
    """per lane over k then e: s += a (b None) or s = fma(a, b, s) -> [T, 64]"""
    s = torch.zeros(a.shape[0], 64, dtype=F32)
    for k in range(a.shape[1]):
        for e in range(8):
            s = s + a[:, k, :, e] if b is None else fma32(a[:, k, :, e], b[:, k, :, e], s)
    return s


def _row_stats(x, C, eps=LN_EPS, defect=None):
    """(v = x - mean in lane layout, rstd [T, 1], mask): the two-pass statistics of ad_load_row"""
    xl, mask = _lanes(x.to(F32))
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    if defect == "one_pass_bf16":      # E[x^2] - mean^2 from sums kept in bf16
        xs = x.to(F32)
        s, q = torch.zeros(x.shape[0], dtype=BF), torch.zeros(x.shape[0], dtype=BF)
        for j in range(C):
            s, q = (s.to(F32) + xs[:, j]).to(BF), (q.to(F32) + xs[:, j] * xs[:, j]).to(BF)
        mu = (s.to(F32) * inv_c).view(-1, 1)
        var = (q.to(F32) * inv_c).view(-1, 1) - mu * mu
        v = torch.where(mask, xl - mu.view(-1, 1, 1, 1), torch.zeros((), dtype=F32))
        return v, torch.rsqrt(var.clamp_min(0) + eps), mask
    mu = _wave_sum(_chain(xl)) * inv_c
    v = torch.where(mask, xl - mu.view(-1, 1, 1, 1), torch.zeros((), dtype=F32))
    sv = _wave_sum(_chain(v, v)) * inv_c
    return v, torch.rsqrt(sv + torch.tensor(eps, dtype=F32)), mask


def _sample_of_rows(T, N, defect):
    b = torch.arange(T) // N
    if defect == "neighbour_sample":      # the first row of every sample but the first reads the previous sample's modulation
        first = (torch.arange(T) % N == 0) & (b > 0)
        b = torch.where(first, b - 1, b)
    return b


def adaln_fwd_emulate(x, shift, scale, N, defect=None):
    T, C = x.shape
    v, rstd, _ = _row_stats(x, C, defect=defect)
    b = _sample_of_rows(T, N, defect)
    sc = scale.to(F32)[b] if defect == "no_one_plus" else 1.0 + scale.to(F32)[b]
    xh = _unlanes(v * rstd.view(-1, 1, 1, 1), C)
    return fma32(xh, sc, shift.to(F32)[b]).to(BF)


def _slab_sum(a, b, B, N, C):
    """column sums of tv_adaln_bwd: per wave its rows of a slab in order (s += a, or fma(a, b, s)), waves in order, slabs in order"""
    J = math.ceil(N / 64)
    pad = lambda t: F.pad(t.view(B, N, C), (0, 0, 0, J * 64 - N)).view(B, J, 16, 4, C)
    a = pad(a)
    b = pad(b) if b is not None else None
    s = torch.zeros(B, J, 4, C, dtype=F32)
    for i in range(16):
        s = s + a[:, :, i] if b is None else fma32(a[:, :, i], b[:, :, i], s)
    blk = torch.zeros(B, J, C, dtype=F32)
    for wv in range(4):
        blk = blk + s[:, :, wv]
    out = torch.zeros(B, C, dtype=F32)
    for j in range(J):
        out = out + blk[:, j]
    return out


def adaln_bwd_emulate(x, scale, dy, dres, N, defect=None):
    """-> (dx bf16, dshift fp32 [B, C], dscale fp32 [B, C])"""
    T, C = x.shape
    B = T // N
    v, rstd, mask = _row_stats(x, C)
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    b = _sample_of_rows(T, N, defect)
    sc1, _ = _lanes(1.0 + scale.to(F32)[b])
    d, _ = _lanes(dy.to(F32))
    xh = v * rstd.view(-1, 1, 1, 1)
    g = d * sc1
    if defect == "round_g":
        g = g.to(BF).to(F32)
    a1 = _wave_sum(_chain(g)) * inv_c
    a2 = _wave_sum(_chain(g, xh)) * inv_c
    inner = fma32(-xh, a2.view(-1, 1, 1, 1).expand_as(xh), g - a1.view(-1, 1, 1, 1))
    dx = rstd.view(-1, 1, 1, 1) * inner
    dx = _unlanes(dx, C)
    if dres is not None:
        dx = dx + dres.to(F32)
    dflat, xflat = dy.to(F32), _unlanes(xh, C)
    if defect == "dscale_with_x":
        xflat = x.to(F32)
    return dx.to(BF), _slab_sum(dflat, None, B, N, C), _slab_sum(dflat, xflat, B, N, C)


def gate_fwd_emulate(x, y, gate, N):
    b = torch.arange(x.shape[0]) // N
    return fma32(gate.to(F32)[b], y.to(F32), x.to(F32)).to(BF)


def gate_bwd_emulate(dout, y, gate, N):
    """-> (dy bf16, dgate fp32 [B, C]): per thread its rows of a slab (stride = the row lanes), row lanes in order, slabs in order"""
    T, C = y.shape
    B = T // N
    b = torch.arange(T) // N
    dy = (gate.to(F32)[b] * dout.to(F32)).to(BF)
    L = gate_lanes(C)
    I, J = math.ceil(64 / L), math.ceil(N / 64)

    def lay(t):
        t = F.pad(t.to(F32).view(B, N, C), (0, 0, 0, J * 64 - N)).view(B, J, 64, C)
        return F.pad(t, (0, 0, 0, I * L - 64)).view(B, J, I, L, C)
    d, yy = lay(dout), lay(y)
    s = torch.zeros(B, J, L, C, dtype=F32)
    for i in range(I):
        s = fma32(d[:, :, i], yy[:, :, i], s)
    blk = torch.zeros(B, J, C, dtype=F32)
    for r in range(L):
        blk = blk + s[:, :, r]
    out = torch.zeros(B, C, dtype=F32)
    for j in range(J):
        out = out + blk[:, j]
    return dy, out


def _x32(lat, mean, rstd):
    D = lat.shape[1]
    return (lat.to(F32) - mean.to(F32).view(1, D, 1, 1)) * rstd.to(F32).view(1, D, 1, 1)


def flow_rows_emulate(lat, mean, rstd, noise, t, p, defect=None):
    B, D, h, w = lat.shape
    ld = round_up(p * p * D, 32)
    x = _x32(lat, mean, rstd)
    if noise is None:
        y = x
    else:
        tb = t.to(F32).view(B, 1, 1, 1)
        ub = 1.0 - tb
        if defect == "swap_t":
            tb, ub = ub, tb
        y = fma32(tb.expand_as(x), x, ub * noise.to(F32))
    return _pad_cols(patchify(y, p).reshape(-1, p * p * D), ld).to(BF)


def flow_loss_emulate(pred, lat, mean, rstd, noise, p, grad_scale=1.0, defect=None):
    """-> (loss, dpred bf16 [B N, ld])"""
    B, D, h, w = lat.shape
    F_ = p * p * D
    ld = round_up(F_, 32)
    x = _x32(lat, mean, rstd)
    v = x - noise.to(F32)
    if defect == "target_sign":
        v = noise.to(F32) - x
    d = pred.to(F32)[:, :F_] - patchify(v, p).reshape(-1, F_)
    count = d.numel() if defect != "pad_in_mean" else d.shape[0] * ld
    coef = torch.tensor(2.0 * grad_scale / count, dtype=F64).to(F32)
    total = (d.to(F64) * d.to(F64)).sum()
    return float(total / count), _pad_cols((coef * d).to(BF), ld)


def flow_euler_emulate(x, v, p, dt, cfg_scale=None, defect=None):
    B, D, h, w = x.shape
    F_ = p * p * D
    N = (h // p) * (w // p)
    v = v.to(F32)[:, :F_]
    dt32 = torch.tensor(dt, dtype=F32)
    if cfg_scale is None:
        vel = v
    else:
        s = torch.tensor(cfg_scale, dtype=F32)
        vc, vu = v[:B * N], v[B * N:]
        vel = fma32(s.expand_as(vc), vc - vu, vc if defect == "cfg_from_cond" else vu)
    return fma32(dt32.expand_as(x), unpatchify(vel.reshape(B, N, F_), D, h, w, p), x.to(F32))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
ROW_SHAPES = ((3, 65, 128), (2, 1, 384), (3, 256, 768), (2, 64, 1024))
FLOW_SHAPES = ((3, 32, 8, 8, 1), (2, 16, 16, 16, 2), (2, 4, 6, 10, 2))


def row_inputs(B, N, C, seed):
    """bf16 rows (offset rows, one constant row), bf16 gradients, an fp32 [B, 6 C] modulation with sample 0's scale = -1 and
    the last sample's gate = 0; slices at offsets C (shift), 2 C (scale), 4 C (gate)"""
    g = torch.Generator().manual_seed(seed)
    T = B * N
    x = (torch.randn(T, C, generator=g) * (0.5 + torch.rand(T, 1, generator=g) * 2) + torch.randn(T, 1, generator=g) * 3).to(BF)
    x[T - 1] = 1.75                                            # a constant row: variance 0
    y = torch.randn(T, C, generator=g).to(BF)
    dy = (torch.randn(T, C, generator=g) * 0.1).to(BF)
    dres = (torch.randn(T, C, generator=g) * 0.1).to(BF)
    mod = torch.randn(B, 6 * C, generator=g) * 0.5
    mod[0, 2 * C:3 * C] = -1.0
    mod[B - 1, 4 * C:5 * C] = 0.0
    return {"x": x, "y": y, "dy": dy, "dres": dres, "mod": mod, "shift_off": C, "scale_off": 2 * C, "gate_off": 4 * C}


def flow_inputs(B, D, h, w, p, seed):
    """the mu half of a [B, 2 D, h, w] tensor, per-channel statistics, noise, t with 0 and 1 among its values, bf16 prediction rows"""
    g = torch.Generator().manual_seed(seed)
    moments = torch.randn(B, 2 * D, h, w, generator=g) * 2 + 0.5
    mean = 0.5 + 0.1 * torch.randn(D, generator=g)
    rstd = (1.0 / (2 + 0.2 * torch.rand(D, generator=g, dtype=F64))).to(F32)
    noise = torch.randn(B, D, h, w, generator=g)
    t = torch.rand(B, generator=g)
    t[0], t[-1] = 0.0, 1.0
    ld = round_up(p * p * D, 32)
    N = (h // p) * (w // p)
    pred = torch.randn(B * N, ld, generator=g).to(BF)
    v2 = torch.randn(2 * B * N, ld, generator=g).to(BF)
    return {"moments": moments, "lat": moments[:, :D], "mean": mean, "rstd": rstd, "noise": noise, "t": t, "pred": pred, "v2": v2, "ld": ld, "N": N}


# ---------------------------------------------------------------------------------------------------------------------------
def mint():
    out = {"model_args": MODEL_ARGS, "batch": MODEL_B, "cases": {}}
    for i, case in enumerate(MODEL_CASES):
        seeds = {"state": 100 + i, "batch": 200 + i}
        sd, batch = make_state(case, seeds["state"], True), make_batch(case, seeds["batch"])
        v32, l32, g32 = flow_step(build(case, sd), batch)
        v16, l16, g16 = flow_step(build(case, sd), batch, autocast=True)
        out["cases"][case] = {"seeds": seeds, "loss_fp32": float(l32), "loss": abs(float(l16) - float(l32)) / float(l32),
                              "velocity": rel_l2(v16, v32), "grads": {k: rel_l2(g16[k], g32[k]) for k in g32}}
    case = SAMPLER["case"]
    seeds = {"state": 300, "batch": 301}
    sd, batch = make_state(case, seeds["state"], True), make_batch(case, seeds["batch"])
    args = (batch["labels"], batch["noise"], batch["stats"], SAMPLER["steps"], SAMPLER["cfg_scale"])
    out["sampler"] = dict(SAMPLER, seeds=seeds, latents=rel_l2(sample(build(case, sd), *args, autocast=True), sample(build(case, sd), *args)))
    case = TRAIN["case"]
    seeds = {"state": 400, "batch": 401}
    sd, batch = make_state(case, seeds["state"], False), make_batch(case, seeds["batch"])
    losses = train_steps(build(case, sd), batch, TRAIN["steps"], TRAIN["lr"])
    out["train"] = dict(TRAIN, seeds=seeds, first_loss=losses[0], final_loss=losses[-1])
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("sampler", "train")}, indent=1))
    for case, c in out["cases"].items():
        print(case, "velocity", c["velocity"], "loss", c["loss"], "max grad dev", max(c["grads"].values()))


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.manual_seed(0)
        mint()
