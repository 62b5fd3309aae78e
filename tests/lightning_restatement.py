"""The LightningDiT of transvae/lightning_dit.py and csrc/lightning.hip restated in plain torch:

  * `LightningDiTRef`: the module with the same state-dict keys and the three switches, runnable in fp32 / fp64 and under bf16
    autocast with a `bf16_stream` switch that rounds where the HIP path stores bf16; the step, sampler and training helpers are
    those of tests/dit_restatement.py;
  * fp64 references of the six kernels with the slack of their DESIGN.md section 3.1 row J;
  * fp32 emulations of each kernel in its own order of operations, and the same emulations with named defects.

`python tests/lightning_restatement.py --mint` writes tests/golden/lightning_dit_ref_bf16_autocast.json: the restatement's OWN relL2
deviation of the bf16-autocast form from fp32 for the whole-model cases of tests/test_lightning_gpu.py, per output and gradient
tensor, the sampler case, and the two losses of the training case, with the seeds they were minted with.
"""
import json
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

import dit_restatement as R
from dit_restatement import BF, F32, F64, LN_EPS, TIME_SCALE, U, fma32, k_rows_adaln, k_s, rel_l2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lightning_dit_ref_bf16_autocast.json")
TINY = 2.0 ** -126        # the sigmoid's absolute floor: below it fp32 is subnormal, and expf(-x1) overflows at x1 < -88.7 (s = 0)

ALL_ON = dict(use_rmsnorm=True, use_qknorm=True, use_swiglu=True)
_P1 = dict(in_channels=32, input_size=(8, 8), patch_size=1)
# whole-model cases of the GPU test: width 128 (two heads; H = 341, padded to 352), depth 2, 10 classes, B = 3 (one null label)
MODEL_CASES = {"f16d32_p1": dict(_P1, **ALL_ON),
               "f8d16_p2": dict(in_channels=16, input_size=(16, 16), patch_size=2, **ALL_ON),
               "f16d32_p1_rms_only": dict(_P1, use_rmsnorm=True, use_qknorm=False, use_swiglu=False),
               "f16d32_p1_no_rms": dict(_P1, use_rmsnorm=False, use_qknorm=True, use_swiglu=True)}
MODEL_ARGS = dict(hidden_size=128, depth=2, num_classes=10)
MODEL_B = 3
SAMPLER = dict(case="f16d32_p1", steps=4, cfg_scale=1.5)
TRAIN = dict(case="f16d32_p1", steps=30, lr=2e-3)       # lr chosen on the CPU so that the fp32 restatement ends below a quarter
FLAG_SETS = [dict(use_rmsnorm=a, use_qknorm=b, use_swiglu=c) for a, b, c in ((True, True, True), (True, False, False), (False, True, True))]


def swiglu_inner(hidden, mlp_ratio=4.0):
    """the public definition's width, in floating point as it writes it"""
    return int(2 / 3 * int(hidden * mlp_ratio))


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
class _W(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))


def rms_norm(v, w, eps=LN_EPS):
    return v * torch.rsqrt((v * v).mean(-1, keepdim=True) + eps) * w


class LightningDiTRef(nn.Module):
    def __init__(self, input_size, patch_size, in_channels, hidden_size, depth, num_classes, mlp_ratio=4.0, freq=256, use_rmsnorm=True,
                 use_qknorm=True, use_swiglu=True):
        super().__init__()
        C = hidden_size
        self.input_size, self.p, self.D, self.C, self.depth, self.num_classes, self.freq = tuple(input_size), patch_size, in_channels, C, depth, num_classes, freq
        self.flags = (use_rmsnorm, use_qknorm, use_swiglu)
        H = swiglu_inner(C, mlp_ratio)
        self.x_embedder = R._Seq()
        self.x_embedder.proj = nn.Conv2d(in_channels, C, patch_size, patch_size)
        self.t_embedder = R._Seq()
        self.t_embedder.mlp = nn.Sequential(nn.Linear(freq, C), nn.SiLU(), nn.Linear(C, C))
        self.y_embedder = R._Seq()
        self.y_embedder.embedding_table = nn.Embedding(num_classes + 1, C)
        self.blocks = nn.ModuleList()
        for _ in range(depth):
            b = R._Seq()
            if use_rmsnorm:
                b.norm1 = _W(C)
            b.attn = R._Seq()
            b.attn.qkv = nn.Linear(C, 3 * C)
            if use_qknorm:
                b.attn.q_norm, b.attn.k_norm = _W(64), _W(64)
            b.attn.proj = nn.Linear(C, C)
            if use_rmsnorm:
                b.norm2 = _W(C)
            b.mlp = R._Seq()
            if use_swiglu:
                b.mlp.w12, b.mlp.w3 = nn.Linear(C, 2 * H), nn.Linear(H, C)
            else:
                b.mlp.fc1, b.mlp.fc2 = nn.Linear(C, int(C * mlp_ratio)), nn.Linear(int(C * mlp_ratio), C)
            b.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(C, 6 * C))
            self.blocks.append(b)
        self.final_layer = R._Seq()
        if use_rmsnorm:
            self.final_layer.norm_final = _W(C)
        self.final_layer.linear = nn.Linear(C, patch_size * patch_size * in_channels)
        self.final_layer.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(C, 2 * C))

    def forward(self, x, t, y, bf16_stream=False):
        """x [B, D, h, w] normalised (x_t), t [B], y [B] -> velocity [B, D, h, w].  bf16_stream: the residual stream and every
        branch operand are rounded to bf16 where the HIP path stores bf16 (call it under torch.autocast(bf16))."""
        rnd = (lambda v: v.to(BF).to(v.dtype) if v.dtype != BF else v) if bf16_stream else (lambda v: v)
        use_rms, use_qk, use_sw = self.flags
        dt = self.x_embedder.proj.weight.dtype
        B, D, h, w = x.shape
        p, C = self.p, self.C
        gh, gw = h // p, w // p
        N, heads = gh * gw, C // 64
        dev = x.device.type
        with torch.autocast(dev, enabled=False):         # the conditioning path is fp32 on the HIP path as well
            c = self.t_embedder.mlp(R.timestep_embedding(t.to(dt) * TIME_SCALE, self.freq)) + self.y_embedder.embedding_table(y)
            mods = [b.adaLN_modulation(c) for b in self.blocks]
            modf = self.final_layer.adaLN_modulation(c)
        we = self.x_embedder.proj.weight.permute(0, 2, 3, 1).reshape(C, p * p * D)
        hcur = rnd(F.linear(rnd(R.patchify(x, p)), we, self.x_embedder.proj.bias).to(dt))
        tabs = tuple(tb.to(x.device) for tb in R.rope_tables(gh, gw, dt))

        def norm_mod(v, norm, shift, scale):
            with torch.autocast(dev, enabled=False):
                v = v.to(dt)
                z = rms_norm(v, norm.weight) if norm is not None else F.layer_norm(v, (C,), eps=LN_EPS)
                return rnd(z * (1 + scale[:, None]) + shift[:, None])
        for b, mod in zip(self.blocks, mods):
            s1, k1, g1, s2, k2, g2 = mod.chunk(6, dim=1)
            qkv = rnd(F.linear(norm_mod(hcur, b.norm1 if use_rms else None, s1, k1), b.attn.qkv.weight, b.attn.qkv.bias).to(dt))
            q, k, v = [u.reshape(B, N, heads, 64).transpose(1, 2) for u in qkv.chunk(3, dim=-1)]
            if use_qk:
                with torch.autocast(dev, enabled=False):
                    q, k = rms_norm(q, b.attn.q_norm.weight), rms_norm(k, b.attn.k_norm.weight)
            q, k = rnd(R.rope_apply(q, tabs)), rnd(R.rope_apply(k, tabs))
            o = F.scaled_dot_product_attention(q, k, v).to(dt)
            a = rnd(F.linear(rnd(o.transpose(1, 2).reshape(B, N, C)), b.attn.proj.weight, b.attn.proj.bias).to(dt))
            hcur = rnd(hcur + g1[:, None] * a)
            a = norm_mod(hcur, b.norm2 if use_rms else None, s2, k2)
            if use_sw:
                u = rnd(F.linear(a, b.mlp.w12.weight, b.mlp.w12.bias).to(dt))
                x1, x2 = u.chunk(2, dim=-1)
                m = rnd(F.silu(x1) * x2)
                m = rnd(F.linear(m, b.mlp.w3.weight, b.mlp.w3.bias).to(dt))
            else:
                m = rnd(F.gelu(F.linear(a, b.mlp.fc1.weight, b.mlp.fc1.bias)).to(dt))
                m = rnd(F.linear(m, b.mlp.fc2.weight, b.mlp.fc2.bias).to(dt))
            hcur = rnd(hcur + g2[:, None] * m)
        sf, kf = modf.chunk(2, dim=1)
        a = norm_mod(hcur, self.final_layer.norm_final if use_rms else None, sf, kf)
        out = rnd(F.linear(a, self.final_layer.linear.weight, self.final_layer.linear.bias).to(dt))
        return R.unpatchify(out, D, h, w, p)


def state_dict_keys(depth, use_rmsnorm=True, use_qknorm=True, use_swiglu=True):
    m = LightningDiTRef((8, 8), 1, 4, 64, depth, 3, use_rmsnorm=use_rmsnorm, use_qknorm=use_qknorm, use_swiglu=use_swiglu)
    return list(m.state_dict())


def _geometry(case):
    return {k: v for k, v in MODEL_CASES[case].items() if not k.startswith("use_")}


def _flags(case):
    return {k: v for k, v in MODEL_CASES[case].items() if k.startswith("use_")}


def build(case, sd, dtype=F32):
    m = LightningDiTRef(**MODEL_CASES[case], **MODEL_ARGS)
    m.load_state_dict(sd)
    return m.to(dtype)


def make_state(case, seed, randomize_zero_init):
    """R.make_state's rules; the norm weights are ones, or 1 + N(0, 0.2^2) with randomize_zero_init, so that their gradients matter"""
    g = torch.Generator().manual_seed(seed)
    m = LightningDiTRef(**MODEL_CASES[case], **MODEL_ARGS)
    sd = {}
    for k, v in m.state_dict().items():
        if "norm" in k:
            sd[k] = 1 + 0.2 * torch.randn(v.shape, generator=g) if randomize_zero_init else torch.ones_like(v)
        elif any(z in k for z in R.ZERO_INIT):
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
    cfg = _geometry(case)
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


flow_step, sample, train_steps = R.flow_step, R.sample, R.train_steps


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references of the kernels with the slack of DESIGN.md section 3.1 row J
# ---------------------------------------------------------------------------------------------------------------------------
K_HEAD = 8 + 3          # adds behind a 64-term head sum: the lane's chain of 8, three butterfly steps
QK_GROUPS, QK_MAX_BLOCKS, QK_FIN_LANES, DW_LANES = 32, 1024, 64, 16


def e_rel(k):
    """relative error of xhat = x rsqrt(mean(x^2) + eps) with a k-add fp32 chain behind the (all-positive) sum of squares:
    k / 2 from the sum, 3 / 2 for 1 / n, the product with it and the add of eps (halved by the square root), 2 for rsqrtf, 1 for
    the product with x, rounded up: u (k / 2 + 5)"""
    return U * (0.5 * k + 5)


def k_dw(B):
    """adds behind dw: the sample lane's chain, sixteen lanes, and the roundings of 1 + scale and of the fma"""
    return math.ceil(B / DW_LANES) + DW_LANES + 2


def qk_geometry(units):
    nblk = min(math.ceil(units / QK_GROUPS), QK_MAX_BLOCKS)
    return nblk, math.ceil(units / (QK_GROUPS * nblk))


def k_dwqk(units):
    """adds behind dwq / dwk: the group's passes, 32 groups, the block lane's chain, 64 lanes, and the product's own rounding"""
    nblk, passes = qk_geometry(units)
    return passes + QK_GROUPS + math.ceil(nblk / QK_FIN_LANES) + QK_FIN_LANES + 1


def _rms64(x, eps=LN_EPS):
    x = x.to(F64)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return x * rstd, rstd


def adaln_rms_fwd64(x, w, shift, scale, N):
    """x bf16 [B N, C], w fp32 [C], shift / scale fp32 [B, C] -> (y64, slack)"""
    C = x.shape[1]
    xh, _ = _rms64(x)
    k1 = 1 + R._per_row(scale.to(F64), N)
    z = xh * w.to(F64)
    y = z * k1 + R._per_row(shift.to(F64), N)
    slack = (k1 * z).abs() * e_rel(k_s(C)) + 2 * U * ((z * k1).abs() + y.abs())
    return y, slack


def adaln_rms_bwd64(x, w, scale, dy, dres, N):
    """-> dx (one rounding) with its slack; dshift, dscale, dw (fp32 sums) with their bounds"""
    T, C = x.shape
    B = T // N
    ks = k_s(C)
    xh, rstd = _rms64(x)
    exh = e_rel(ks) * xh.abs()
    k1 = 1 + R._per_row(scale.to(F64), N)
    w64 = w.to(F64)
    d = dy.to(F64)
    g = d * (k1 * w64)
    mean = lambda t: t.mean(1, keepdim=True)
    a2 = mean(g * xh)
    inner = g - xh * a2
    dx = rstd * inner
    d_g = 3 * U * g.abs()                                    # 1 + scale, its product with w, the product with dy
    d_a2 = (ks + 6) * U * mean((g * xh).abs()) + mean(g.abs() * exh)
    d_inner = d_g + xh.abs() * d_a2 + a2.abs() * exh + 2 * U * (g.abs() + (xh * a2).abs())
    slack = rstd * d_inner + dx.abs() * (U * (0.5 * ks + 3.5) + 2 * U)
    if dres is not None:
        dx = dx + dres.to(F64)
        slack = slack + U * dres.to(F64).abs()
    slack = slack + U * dx.abs()
    kr = k_rows_adaln(N)
    per = lambda t: t.view(B, N, C).sum(1)
    S = per(d * xh)
    S_bound = U * (kr + 1) * per((d * xh).abs()) + per(d.abs() * exh)
    k1b = 1 + scale.to(F64)
    return {"dx": dx, "dx_slack": slack, "dshift": per(d), "dshift_terms": per(d.abs()), "k_rows": kr,
            "dscale": w64 * S, "dscale_bound": w64.abs() * S_bound,
            "dw": (k1b * S).sum(0), "dw_bound": (k1b.abs() * S_bound).sum(0) + k_dw(B) * U * (k1b * S).abs().sum(0)}


def rope_table(gh, gw):
    """the kernels' table [N, 4, 32] fp32 = cos1, sin1, cos2, sin2"""
    return torch.stack(R.rope_tables(gh, gw, F32), dim=1).contiguous()


def _rope64(z, tab, N):
    """z [T, ..., 64] fp64, tab [N, 4, 32] -> (rotated, the absolute terms of each output)"""
    T = z.shape[0]
    tb = tab.to(F64)[torch.arange(T) % N]
    shape = (T,) + (1,) * (z.dim() - 2) + (32,)
    c1, s1, c2, s2 = (tb[:, i].view(shape) for i in range(4))
    a, b = z[..., 0::2], z[..., 1::2]
    out = torch.stack([a * c1 - b * s1, a * s2 + b * c2], dim=-1).flatten(-2)
    terms = torch.stack([(a * c1).abs() + (b * s1).abs(), (a * s2).abs() + (b * c2).abs()], dim=-1).flatten(-2)
    return out, terms


def qknorm_fwd64(qkv, wq, wk, tab, N):
    """qkv bf16 [T, 3, heads, 64] -> (out64 of the same shape, slack); the v third is the input itself with slack 0"""
    x = qkv.to(F64)
    out, slack = x.clone(), torch.zeros_like(x)
    for i, w in ((0, wq), (1, wk)):
        qh, _ = _rms64(x[:, i])
        z = qh * w.to(F64)
        e_z = z.abs() * (e_rel(K_HEAD) + U)
        if tab is None:
            out[:, i], slack[:, i] = z, e_z
        else:
            o, terms = _rope64(z, tab, N)
            _, e_terms = _rope64(e_z, tab, N)
            out[:, i], slack[:, i] = o, e_terms + U * terms + U * o.abs()
    return out, slack


def qknorm_bwd64(qkv, wq, wk, dqkv):
    """qkv raw bf16 [T, 3, heads, 64], dqkv bf16 of the same shape (gradient of the un-rotated z; the v third passes through)"""
    x, d = qkv.to(F64), dqkv.to(F64)
    T, _, heads, _ = x.shape
    out, slack = d.clone(), torch.zeros_like(d)
    res = {}
    for i, w, name in ((0, wq, "dwq"), (1, wk, "dwk")):
        qh, r = _rms64(x[:, i])
        eqh = e_rel(K_HEAD) * qh.abs()
        g = d[:, i] * w.to(F64)
        mean = lambda t: t.mean(-1, keepdim=True)
        m = mean(g * qh)
        inner = g - qh * m
        dq = r * inner
        d_m = (K_HEAD + 4) * U * mean((g * qh).abs()) + mean(g.abs() * eqh)
        d_inner = U * g.abs() + qh.abs() * d_m + m.abs() * eqh + 2 * U * (g.abs() + (qh * m).abs())
        out[:, i] = dq
        slack[:, i] = r * d_inner + dq.abs() * (U * (0.5 * K_HEAD + 3.5) + 2 * U) + U * dq.abs()
        prod = d[:, i] * qh
        res[name] = prod.sum((0, 1))
        res[name + "_bound"] = k_dwqk(T * 2 * heads) * U * prod.abs().sum((0, 1)) + (d[:, i].abs() * eqh).sum((0, 1))
    res.update(dqkv=out, slack=slack)
    return res


def _sig64(x1):
    s = torch.sigmoid(x1)
    return s, 4 * U * s + TINY          # expf within one ulp (2 u), the add and the IEEE division; the subnormal / overflow floor


def swiglu_fwd64(u):
    """u bf16 [T, 2 Hp] -> (h64 [T, Hp], slack)"""
    x1, x2 = u.to(F64).chunk(2, dim=1)
    s, e_s = _sig64(x1)
    h = x1 * s * x2
    return h, (x1 * x2).abs() * e_s + 2 * U * h.abs()


def swiglu_bwd64(u, dh):
    """-> (du64 [T, 2 Hp], slack)"""
    x1, x2 = u.to(F64).chunk(2, dim=1)
    d = dh.to(F64)
    s, e_s = _sig64(x1)
    t = 1 + x1 * (1 - s)
    du1 = d * x2 * (s * t)
    e_t = x1.abs() * (e_s + U * (1 - s)) + U * t.abs()
    sl1 = (d * x2).abs() * (e_s * t.abs() + s * e_t) + 3 * U * du1.abs()
    du2 = d * (x1 * s)
    sl2 = (d * x1).abs() * e_s + 2 * U * du2.abs()
    return torch.cat([du1, du2], dim=1), torch.cat([sl1, sl2], dim=1)


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' own order (defect=...: the same with a named defect)
# ---------------------------------------------------------------------------------------------------------------------------
def _rms_stats(x, C, eps=LN_EPS, defect=None):
    """(xhat in lane layout, rstd [T, 1]): the one-chain statistic of ad_load_xhat<KCH, true>"""
    xl, mask = R._lanes(x.to(F32))
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    if defect == "stat_bf16":                       # the sum of squares kept in bf16
        xs = x.to(F32)
        q = torch.zeros(x.shape[0], dtype=BF)
        for j in range(C):
            q = (q.to(F32) + xs[:, j] * xs[:, j]).to(BF)
        ss = (q.to(F32) * inv_c).view(-1, 1)
    elif defect == "mean_subtracted":               # LayerNorm's statistic where the RMS one belongs
        v, rstd, _ = R._row_stats(x, C, eps)
        return v * rstd.view(-1, 1, 1, 1), rstd
    else:
        ss = R._wave_sum(R._chain(xl, xl)) * inv_c
    rstd = torch.rsqrt(ss + torch.tensor(eps, dtype=F32))
    return xl * rstd.view(-1, 1, 1, 1), rstd


def adaln_rms_fwd_emulate(x, w, shift, scale, N, defect=None):
    T, C = x.shape
    xh, _ = _rms_stats(x, C, defect=defect)
    xh = R._unlanes(xh, C)
    b = R._sample_of_rows(T, N, defect)
    sc, sh, w = 1.0 + scale.to(F32)[b], shift.to(F32)[b], w.to(F32)
    if defect == "weight_after_mod":
        return (fma32(xh, sc, sh) * w).to(BF)
    return fma32(xh * w, sc, sh).to(BF)


def adaln_rms_bwd_emulate(x, w, scale, dy, dres, N, defect=None):
    """-> (dx bf16, dshift, dscale fp32 [B, C], dw fp32 [C])"""
    T, C = x.shape
    B = T // N
    xhl, rstd = _rms_stats(x, C)
    inv_c = torch.tensor(1.0 / C, dtype=F32)
    b = R._sample_of_rows(T, N, defect)
    w = w.to(F32)
    gw, _ = R._lanes((1.0 + scale.to(F32)[b]) * w)
    d, _ = R._lanes(dy.to(F32))
    g = d * gw
    a2 = R._wave_sum(R._chain(g, xhl)) * inv_c
    inner = fma32(-xhl, a2.view(-1, 1, 1, 1).expand_as(xhl), g)
    dx = R._unlanes(rstd.view(-1, 1, 1, 1) * inner, C)
    if dres is not None:
        dx = dx + dres.to(F32)
    dflat, xflat = dy.to(F32), R._unlanes(xhl, C)
    S = R._slab_sum(dflat, xflat, B, N, C)
    k1 = torch.ones(B, C) if defect == "dw_no_one_plus" else 1.0 + scale.to(F32)
    lanes = torch.zeros(DW_LANES, C, dtype=F32)
    for bb in range(B):
        lanes[bb % DW_LANES] = fma32(k1[bb], S[bb], lanes[bb % DW_LANES])
    dw = torch.zeros(C, dtype=F32)
    for i in range(DW_LANES):
        dw = dw + lanes[i]
    return dx.to(BF), R._slab_sum(dflat, None, B, N, C), w * S, dw


def _group_sum(v):
    """[..., 8 lanes] -> [..., 1]: the three-step butterfly of a lane group"""
    lanes = torch.arange(8)
    for o in (1, 2, 4):
        v = v + v[..., lanes ^ o]
    return v[..., :1]


def _head_chain(a, b):
    """[..., 8 lanes, 8] -> [..., 8 lanes]: s = fma(a, b, s) over the lane's eight elements"""
    s = torch.zeros(a.shape[:-1], dtype=F32)
    for e in range(8):
        s = fma32(a[..., e], b[..., e], s)
    return s


def _head_stats(x, eps=LN_EPS):
    """x fp32 [..., 64] -> (x in [..., 8, 8] lane layout, r [..., 1, 1])"""
    xl = x.reshape(x.shape[:-1] + (8, 8))
    ss = _group_sum(_head_chain(xl, xl)) * torch.tensor(1.0 / 64.0, dtype=F32)
    return xl, torch.rsqrt(ss + torch.tensor(eps, dtype=F32)).unsqueeze(-1)


def _rope32(z, tab, N):
    T = z.shape[0]
    tb = tab.to(F32)[torch.arange(T) % N]
    shape = (T,) + (1,) * (z.dim() - 2) + (32,)
    c1, s1, c2, s2 = (tb[:, i].view(shape) for i in range(4))
    a, b = z[..., 0::2], z[..., 1::2]
    return torch.stack([a * c1 - b * s1, a * s2 + b * c2], dim=-1).flatten(-2)


def qknorm_fwd_emulate(qkv, wq, wk, tab, N, defect=None):
    """qkv bf16 [T, 3, heads, 64] -> bf16 of the same shape"""
    out = qkv.clone()
    for i, w in ((0, wq), (1, wk)):
        x = qkv[:, i].to(F32)
        w = w.to(F32)
        if defect == "norm_after_rope" and tab is not None:     # rotate the raw vector, then normalise and weigh
            x = _rope32(x, tab, N)
        xl, r = _head_stats(x)
        if defect == "all_heads":                               # one statistic per token over every head
            r = torch.rsqrt((x * x).mean((-2, -1), keepdim=True) + LN_EPS).unsqueeze(-1)
        z = ((xl * r).reshape(x.shape)) * w
        if tab is not None and defect != "norm_after_rope":
            z = _rope32(z, tab, N)
        out[:, i] = z.to(BF)
    return out


def _ordered_head_sum(terms):
    """terms fp32 [units, 64] (zero rows for the other operand's units) -> [64] in the order of tv_qknorm_rope_bwd"""
    units = terms.shape[0]
    nblk, passes = qk_geometry(units)
    t = F.pad(terms, (0, 0, 0, passes * nblk * QK_GROUPS - units)).view(passes, nblk, QK_GROUPS, 64)
    acc = torch.zeros(nblk, QK_GROUPS, 64, dtype=F32)
    for p in range(passes):
        acc = acc + t[p]
    blk = torch.zeros(nblk, 64, dtype=F32)
    for gI in range(QK_GROUPS):
        blk = blk + acc[:, gI]
    lanes = torch.zeros(QK_FIN_LANES, 64, dtype=F32)
    rows = F.pad(blk, (0, 0, 0, math.ceil(nblk / QK_FIN_LANES) * QK_FIN_LANES - nblk)).view(-1, QK_FIN_LANES, 64)
    for k in range(rows.shape[0]):
        lanes = lanes + rows[k]
    out = torch.zeros(64, dtype=F32)
    for i in range(QK_FIN_LANES):
        out = out + lanes[i]
    return out


def qknorm_bwd_emulate(qkv, wq, wk, dqkv):
    """-> (dqkv bf16 in place of the q and k thirds, dwq, dwk fp32 [64])"""
    T, _, heads, _ = qkv.shape
    out = dqkv.clone()
    terms = torch.zeros(2, T, 2, heads, 64, dtype=F32)
    for i, w in ((0, wq), (1, wk)):
        xl, r = _head_stats(qkv[:, i].to(F32))
        qh = xl * r
        d = dqkv[:, i].to(F32).reshape(qh.shape)
        g = d * w.to(F32).view(8, 8)
        m = _group_sum(_head_chain(g, qh)) * torch.tensor(1.0 / 64.0, dtype=F32)
        inner = fma32(-qh, m.unsqueeze(-1).expand_as(qh), g)
        out[:, i] = (r * inner).reshape(T, heads, 64).to(BF)
        terms[i, :, i] = (d * qh).reshape(T, heads, 64)
    return out, _ordered_head_sum(terms[0].reshape(-1, 64)), _ordered_head_sum(terms[1].reshape(-1, 64))


def _sig32(x1):
    return 1.0 / (1.0 + torch.exp(-x1))


def swiglu_fwd_emulate(u, defect=None):
    x1, x2 = u.to(F32).chunk(2, dim=1)
    if defect == "halves_swapped":
        x1, x2 = x2, x1
    return ((x1 * _sig32(x1)) * x2).to(BF)


def swiglu_bwd_emulate(u, dh, defect=None):
    x1, x2 = u.to(F32).chunk(2, dim=1)
    if defect == "halves_swapped":
        x1, x2 = x2, x1
    d = dh.to(F32)
    s = _sig32(x1)
    deriv = s if defect == "no_x_term" else s * fma32(x1, 1.0 - s, torch.ones_like(s))
    return torch.cat([((d * x2) * deriv).to(BF), (d * (x1 * s)).to(BF)], dim=1)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
ROW_SHAPES = ((3, 65, 128), (2, 1, 384), (3, 256, 768), (2, 64, 1024), (2, 3, 1152))
QK_SHAPES = ((3, 65, 2), (2, 1, 6), (1, 5, 3), (1, 256, 12), (2, 64, 16))          # (B, N, heads); (1, 5, 3): 15 head vectors per third
SWIGLU_SHAPES = ((2, 32), (195, 352), (130, 2752), (1024, 2048))                    # (T, Hp)
SWIGLU_EDGE = (0.0, 3e38, -3e38, -100.0)          # x1 of row 0, columns 0 .. 3 (x2 = 0.5, dh = 0.25 there)
QK_GRIDS = {65: (5, 13), 1: (1, 1), 5: (1, 5), 256: (16, 16), 64: (8, 8)}         # token grid of each N


def row_inputs(B, N, C, seed):
    """R.row_inputs without the offset rows' meaning (an RMS statistic has no mean), a norm weight about 1 with a zero at channel 3,
    an all-zero row, sample 0's scale = -1; slices at offsets C (shift) and 2 C (scale) of an fp32 [B, 4 C] modulation"""
    inp = R.row_inputs(B, N, C, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    w = 1 + 0.3 * torch.randn(C, generator=g)
    w[3] = 0.0
    inp["x"][B * N - 1] = 0.0
    inp["mod"] = inp["mod"][:, :4 * C].contiguous()
    inp["w"] = w
    return inp


def qk_inputs(B, N, heads, seed):
    """bf16 qkv and gradient [B N, 3, heads, 64], weights about 1, the table of the token grid; head vector (0, q, 0) is all zero"""
    g = torch.Generator().manual_seed(seed)
    T = B * N
    qkv = (torch.randn(T, 3, heads, 64, generator=g) * (0.3 + 2 * torch.rand(T, 3, heads, 1, generator=g))).to(BF)
    qkv[0, 0, 0] = 0.0
    dqkv = (torch.randn(T, 3, heads, 64, generator=g) * 0.1).to(BF)
    wq, wk = 1 + 0.3 * torch.randn(64, generator=g), 1 + 0.3 * torch.randn(64, generator=g)
    return {"qkv": qkv, "dqkv": dqkv, "wq": wq, "wk": wk, "tab": rope_table(*QK_GRIDS[N])}


def swiglu_inputs(T, Hp, seed, pad=11):
    """bf16 u [T, 2 Hp] and dh [T, Hp]; the edge values of SWIGLU_EDGE at the head of row 0; the last `pad` columns of each half are
    zero, as the padded operands of a LightningDiT whose inner width is no multiple of 32 give them"""
    g = torch.Generator().manual_seed(seed)
    u = (torch.randn(T, 2 * Hp, generator=g) * 3).to(BF)
    dh = (torch.randn(T, Hp, generator=g) * 0.1).to(BF)
    for j, v in enumerate(SWIGLU_EDGE):
        u[0, j], u[0, Hp + j], dh[0, j] = v, 0.5, 0.25
    u[:, Hp - pad:Hp] = 0.0
    u[:, 2 * Hp - pad:] = 0.0
    return {"u": u, "dh": dh, "pad": pad}


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
