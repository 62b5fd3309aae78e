"""The head_dim 72 family of csrc/attention_hd.hip and the XL models restated in plain torch:

  * `HdRef`: `DiT` / `LightningDiT` with a `head_dim` argument (the state-dict keys of tests/lightning_restatement.py; every switch
    off is the DiT block), runnable in fp32 / fp64 and under bf16 autocast like `DiTRef`;
  * the 36-pair RoPE (`rope_pairs`, `rope_table`), the attention backward's exact form and emulation with a [N, 4, 36] table (the
    forward emulation and the table-free backward are `attn_fwd_emul` / `attn_bwd_emul` of tests/test_error_budget_host.py as they
    are: the kernels keep row A's policies and parameters);
  * fp64 references with slack for tv_rope_qk_hd and the qk-norm pair: row J's formulas with K_HEAD = 8 + 4 (the lane's chain of
    8 FMAs, four butterfly steps of the 16-lane group), and fp32 emulations in the kernels' order, with named defects.

`python tests/hd72_restatement.py --mint` writes tests/golden/dit_hd72_ref_bf16_autocast.json: the restatement's OWN relL2 deviation
of its bf16-autocast form from fp32 for the whole-model cases of tests/test_hd72_gpu.py, the sampler case and the training case.
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

import dit_restatement as R
import lightning_restatement as LR
from dit_restatement import BF, F32, F64, LN_EPS, TIME_SCALE, U, fma32, rel_l2
from test_error_budget_host import LOG2E, f32, r16, split3

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_hd72_ref_bf16_autocast.json")
HD, PAIRS, PIECES = 72, 36, 9
SCALE = 72 ** -0.5
K_HEAD = 8 + 4            # adds behind a 72-term head sum: the lane's chain of 8, four butterfly steps (lanes 9..15 add zeros)
K_DELTA = 8 + 8           # delta: a chain of 8 per piece, the nine piece sums in order
QK_LANES, QK_GROUPS, QK_MAX_BLOCKS, QK_FIN_LANES = 16, 16, 1024, 64
INV_HD = torch.tensor(1.0 / 72.0, dtype=F32)

_P1 = dict(in_channels=32, input_size=(8, 8), patch_size=1)
_OFF = dict(use_rmsnorm=False, use_qknorm=False, use_swiglu=False)
# width 288 = 4 heads of 72 (the smallest multiple of 72 and of the GEMM's 32), depth 2, 10 classes, B = 3 (one null label)
MODEL_CASES = {"dit": dict(_P1, **_OFF),
               "lightning": dict(_P1, **LR.ALL_ON),
               "lightning_rms_only": dict(_P1, use_rmsnorm=True, use_qknorm=False, use_swiglu=False),
               "lightning_no_rms": dict(_P1, use_rmsnorm=False, use_qknorm=True, use_swiglu=True)}
MODEL_ARGS = dict(hidden_size=288, depth=2, num_classes=10, head_dim=72)
MODEL_B = 3
SAMPLER = dict(steps=8, cfg_scale=1.5)
TRAIN = dict(steps=30, lr=2e-3)
SAMPLER_CASES = ("dit", "lightning")


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def rope_tables(gh, gw, dtype, hd=HD):
    """the model's 2-D RoPE at head_dim hd: angle vector [y f, y f, x f, x f], f = 10000^(-2 i / (hd / 2)), i < hd / 4"""
    half = hd // 2
    f = 1.0 / (10000 ** (torch.arange(0, half, 2).float() / half))
    ys = torch.arange(gh, dtype=F32).repeat_interleave(gw)
    xs = torch.arange(gw, dtype=F32).repeat(gh)
    yf, xf = torch.outer(ys, f), torch.outer(xs, f)
    ang = torch.cat([yf, yf, xf, xf], dim=-1)
    t1, t2 = ang[:, 0::2], ang[:, 1::2]
    return tuple(t.to(dtype) for t in (t1.cos(), t1.sin(), t2.cos(), t2.sin()))


def rope_table(gh, gw, hd=HD):
    """the kernels' table [N, 4, hd / 2] fp32 = cos1, sin1, cos2, sin2"""
    return torch.stack(rope_tables(gh, gw, F32, hd), dim=1).contiguous()


class HdRef(LR.LightningDiTRef):
    """`LightningDiTRef` with a head dimension; with the three switches off it is `DiTRef` (the same keys and arithmetic)."""

    def __init__(self, input_size, patch_size, in_channels, hidden_size, depth, num_classes, head_dim=72, **kw):
        super().__init__(input_size, patch_size, in_channels, hidden_size, depth, num_classes, **kw)
        assert hidden_size % head_dim == 0
        self.head_dim = head_dim
        if self.flags[1]:
            for b in self.blocks:
                b.attn.q_norm, b.attn.k_norm = LR._W(head_dim), LR._W(head_dim)

    def forward(self, x, t, y, bf16_stream=False):
        rnd = (lambda v: v.to(BF).to(v.dtype) if v.dtype != BF else v) if bf16_stream else (lambda v: v)
        use_rms, use_qk, use_sw = self.flags
        dt = self.x_embedder.proj.weight.dtype
        B, D, h, w = x.shape
        p, C, hd = self.p, self.C, self.head_dim
        gh, gw = h // p, w // p
        N, heads = gh * gw, C // hd
        dev = x.device.type
        with torch.autocast(dev, enabled=False):         # the conditioning path is fp32 on the HIP path as well
            c = self.t_embedder.mlp(R.timestep_embedding(t.to(dt) * TIME_SCALE, self.freq)) + self.y_embedder.embedding_table(y)
            mods = [b.adaLN_modulation(c) for b in self.blocks]
            modf = self.final_layer.adaLN_modulation(c)
        we = self.x_embedder.proj.weight.permute(0, 2, 3, 1).reshape(C, p * p * D)
        hcur = rnd(F.linear(rnd(R.patchify(x, p)), we, self.x_embedder.proj.bias).to(dt))
        tabs = tuple(tb.to(x.device) for tb in rope_tables(gh, gw, dt, hd))

        def norm_mod(v, norm, shift, scale):
            with torch.autocast(dev, enabled=False):
                v = v.to(dt)
                z = LR.rms_norm(v, norm.weight) if norm is not None else F.layer_norm(v, (C,), eps=LN_EPS)
                return rnd(z * (1 + scale[:, None]) + shift[:, None])
        for b, mod in zip(self.blocks, mods):
            s1, k1, g1, s2, k2, g2 = mod.chunk(6, dim=1)
            qkv = rnd(F.linear(norm_mod(hcur, b.norm1 if use_rms else None, s1, k1), b.attn.qkv.weight, b.attn.qkv.bias).to(dt))
            q, k, v = [u.reshape(B, N, heads, hd).transpose(1, 2) for u in qkv.chunk(3, dim=-1)]
            if use_qk:
                with torch.autocast(dev, enabled=False):
                    q, k = LR.rms_norm(q, b.attn.q_norm.weight), LR.rms_norm(k, b.attn.k_norm.weight)
            q, k = rnd(R.rope_apply(q, tabs)), rnd(R.rope_apply(k, tabs))
            o = F.scaled_dot_product_attention(q, k, v).to(dt)          # (scale 1 / sqrt(head_dim))
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


def flags(case):
    return {k: v for k, v in MODEL_CASES[case].items() if k.startswith("use_")}


def build(case, sd, dtype=F32):
    m = HdRef(**MODEL_CASES[case], **MODEL_ARGS)
    m.load_state_dict(sd)
    return m.to(dtype)


def make_state(case, seed, randomize_zero_init):
    """LR.make_state's rules on this file's cases"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in HdRef(**MODEL_CASES[case], **MODEL_ARGS).state_dict().items():
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


flow_step, sample, train_steps = R.flow_step, R.sample, R.train_steps


# ---------------------------------------------------------------------------------------------------------------------------
# the 36-pair RoPE and the attention backward with it (row A's forms of tests/test_error_budget_host.py at [N, 4, 36])
# ---------------------------------------------------------------------------------------------------------------------------
def table_rows(tab, rows, stride32=False):
    """(c1, s1, c2, s2) [M, 1, 36] fp64 of the given rows.  stride32 (a defect): the flat table read with the head_dim 64 layout,
    row pitch 128 and planes 32 apart"""
    if not stride32:
        return tuple(tab.to(F64)[rows, i][:, None, :] for i in range(4))
    flat = tab.to(F64).reshape(-1)
    idx = (rows[:, None] * 128 + torch.arange(PAIRS)[None]) % flat.numel()
    return tuple(flat[(idx + 32 * i) % flat.numel()][:, None, :] for i in range(4))


def rope_pairs(t, tab, rows, kind="forward", fp32=False, stride32=False):
    """The reference's (non-orthogonal) RoPE 2x2 on the 72-wide heads of t [M, n 72] with rows `rows` of tab [tokens, 4, 36]:
      forward  y[2p] = a c1 - b s1,   y[2p+1] = a s2 + b c2
      adjoint  a'    = a c1 + b s2,   b'      = -a s1 + b c2
    fp32: each product and the sum rounded to fp32 (the kernels' arithmetic, fp contraction off)."""
    rd = f32 if fp32 else (lambda v: v)
    M = t.shape[0]
    tp = t.to(F64).reshape(M, -1, PAIRS, 2)
    a, b = tp[..., 0], tp[..., 1]
    c1, s1, c2, s2 = table_rows(tab, rows, stride32)
    if kind == "forward":
        ya, yb = rd(rd(a * c1) - rd(b * s1)), rd(rd(a * s2) + rd(b * c2))
    else:
        ya, yb = rd(rd(a * c1) + rd(b * s2)), rd(rd(b * c2) - rd(a * s1))
    return torch.stack([ya, yb], -1).reshape(t.shape)


def rope_terms(t, tab, rows, kind="forward"):
    """sum of the absolute values of the two products behind each output of rope_pairs"""
    M = t.shape[0]
    tp = t.to(F64).reshape(M, -1, PAIRS, 2).abs()
    a, b = tp[..., 0], tp[..., 1]
    c1, s1, c2, s2 = (v.abs() for v in table_rows(tab, rows))
    if kind == "forward":
        ya, yb = a * c1 + b * s1, a * s2 + b * c2
    else:
        ya, yb = a * c1 + b * s2, b * c2 + a * s1
    return torch.stack([ya, yb], -1).reshape(t.shape)


def rope_qk64(qkv, tab, N, kind="forward"):
    """tv_rope_qk_hd: qkv bf16 [T, 3, heads, 72] -> (out64, slack); two products and their sum in fp32, the v third untouched"""
    T, _, heads, _ = qkv.shape
    rows = torch.arange(T) % N
    out, slack = qkv.to(F64).clone(), torch.zeros(qkv.shape, dtype=F64)
    for i in (0, 1):
        x = qkv[:, i].reshape(T, heads * HD)
        o = rope_pairs(x, tab, rows, kind)
        out[:, i] = o.reshape(T, heads, HD)
        slack[:, i] = (U * rope_terms(x, tab, rows, kind) + U * o.abs()).reshape(T, heads, HD)
    return out, slack


def rope_qk_emulate(qkv, tab, N, kind="forward", defect=None):
    T, _, heads, _ = qkv.shape
    rows = torch.arange(T) % N
    out = qkv.clone()
    for i in (0, 1):
        o = rope_pairs(qkv[:, i].reshape(T, heads * HD), tab, rows, kind, fp32=True, stride32=defect == "stride32")
        out[:, i] = o.reshape(T, heads, HD).to(BF)
    return out


def attn_bwd_exact(q, k, v, o, do, lse, scale, tab=None):
    """test_error_budget_host.attn_bwd_exact with the 36-pair adjoint"""
    q, k, v, o, do, lse = (t.to(F64) for t in (q, k, v, o, do, lse))
    delta = (do * o).sum(1)
    p = torch.exp(q @ k.t() * scale - lse[:, None])
    ds = p * (do @ v.t() - delta[:, None])
    dq, dk = scale * ds @ k, scale * ds.t() @ q
    if tab is not None:
        rows = torch.arange(q.shape[0])
        dq, dk = rope_pairs(dq, tab, rows, "adjoint"), rope_pairs(dk, tab, rows, "adjoint")
    return dq, dk, p.t() @ do, delta


def delta_emul(o, do):
    """the delta kernel's order: per 16-byte piece a chain of 8 FMAs from 0, the nine piece sums added in order"""
    a, g = o.to(F32).reshape(-1, PIECES, 8), do.to(F32).reshape(-1, PIECES, 8)
    part = torch.zeros(a.shape[:2], dtype=F32)
    for e in range(8):
        part = fma32(a[..., e], g[..., e], part)
    acc = part[:, 0]
    for pc in range(1, PIECES):
        acc = acc + part[:, pc]
    return acc.to(F64)


def attn_bwd_emul(q, k, v, o, do, lse, scale, mutate=None, tab=None, sums=False):
    """test_error_budget_host.attn_bwd_emul (row A's backward policy) at head_dim 72: delta in the kernel's order and joined in fp32
    (it never leaves fp32 here, which the three-piece form of the 64 kernels equals to 2^-24); the 36-pair adjoint on the scaled
    fp32 sums before the one rounding.  mutate: 'rope_after' (adjoint applied to the rounded dq / dk, rounded again), 'rope_stride32'
    (the table read with the head_dim 64 layout), 'rope_fwd'.  sums: also return the scaled fp32 sums (dq, dk) the store starts from."""
    q, k, v, o, do = (t.to(F64) for t in (q, k, v, o, do))
    c2 = float(torch.tensor(scale * LOG2E, dtype=F32))
    delta = delta_emul(o, do)
    nl = f32(-f32(lse.to(F64)) * LOG2E)
    s = f32(q @ k.t())
    p = f32(torch.exp2(f32(s * c2 + nl[:, None])))
    dpm = f32(f32(do @ v.t()) - delta[:, None])
    ds = r16(f32(p * dpm))
    dq = f32(f32(ds @ k) * scale)
    dk = f32(f32(ds.t() @ q) * scale)
    raw = (dq, dk)
    if tab is not None:
        rows = torch.arange(q.shape[0])
        kind = "forward" if mutate == "rope_fwd" else "adjoint"
        if mutate == "rope_after":
            dq, dk = r16(dq), r16(dk)
        dq, dk = (rope_pairs(t, tab, rows, kind, fp32=True, stride32=mutate == "rope_stride32") for t in (dq, dk))
    dv = r16(f32(r16(p).t() @ do))
    res = (r16(dq), r16(dk), dv, delta)
    return res + raw if sums else res


# ---------------------------------------------------------------------------------------------------------------------------
# qk-norm + RoPE at 72: fp64 with row J's slack, and the kernels' order in fp32
# ---------------------------------------------------------------------------------------------------------------------------
e_rel = LR.e_rel


def qk_geometry(units):
    nblk = min(math.ceil(units / QK_GROUPS), QK_MAX_BLOCKS)
    return nblk, math.ceil(units / (QK_GROUPS * nblk))


def k_dwqk(units):
    """adds behind dwq / dwk: the group's passes, 16 groups, the block lane's chain, 64 lanes, and the product's own rounding"""
    nblk, passes = qk_geometry(units)
    return passes + QK_GROUPS + math.ceil(nblk / QK_FIN_LANES) + QK_FIN_LANES + 1


def qknorm_fwd64(qkv, wq, wk, tab, N):
    """qkv bf16 [T, 3, heads, 72] -> (out64, slack): LR.qknorm_fwd64 with mean_72 and K_HEAD = 12"""
    x = qkv.to(F64)
    T, _, heads, _ = x.shape
    rows = torch.arange(T) % N
    out, slack = x.clone(), torch.zeros_like(x)
    for i, w in ((0, wq), (1, wk)):
        qh, _ = LR._rms64(x[:, i])
        z = qh * w.to(F64)
        e_z = z.abs() * (e_rel(K_HEAD) + U)
        if tab is None:
            out[:, i], slack[:, i] = z, e_z
        else:
            flat = lambda t: t.reshape(T, heads * HD)
            o = rope_pairs(flat(z), tab, rows)
            terms, e_terms = rope_terms(flat(z), tab, rows), rope_terms(flat(e_z), tab, rows)
            out[:, i], slack[:, i] = o.reshape(z.shape), (e_terms + U * terms + U * o.abs()).reshape(z.shape)
    return out, slack


def qknorm_bwd64(qkv, wq, wk, dqkv):
    """LR.qknorm_bwd64 with mean_72, K_HEAD = 12 and this file's dw geometry"""
    x, d = qkv.to(F64), dqkv.to(F64)
    T, _, heads, _ = x.shape
    out, slack = d.clone(), torch.zeros_like(d)
    res = {}
    for i, w, name in ((0, wq, "dwq"), (1, wk, "dwk")):
        qh, r = LR._rms64(x[:, i])
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


def _lanes(x):
    """fp32 [..., 72] -> [..., 16 lanes, 8]: lanes 0..8 one piece each, lanes 9..15 zeros"""
    return F.pad(x.reshape(x.shape[:-1] + (PIECES, 8)), (0, 0, 0, QK_LANES - PIECES))


def _group_sum(v):
    """[..., 16 lanes] -> [..., 1]: the four-step xor butterfly of a lane group"""
    lanes = torch.arange(QK_LANES)
    for o in (1, 2, 4, 8):
        v = v + v[..., lanes ^ o]
    return v[..., :1]


def _head_stats(x, eps=LN_EPS, n_mean=72):
    """x fp32 [..., 72] -> (x in [..., 16, 8] lane layout, r [..., 1, 1]).  n_mean: the divisor (a defect when not 72)"""
    xl = _lanes(x)
    inv = INV_HD if n_mean == 72 else torch.tensor(1.0 / n_mean, dtype=F32)
    ss = _group_sum(LR._head_chain(xl, xl)) * inv
    return xl, torch.rsqrt(ss + torch.tensor(eps, dtype=F32)).unsqueeze(-1)


def _unlanes(xl):
    return xl[..., :PIECES, :].reshape(xl.shape[:-2] + (HD,))


def qknorm_fwd_emulate(qkv, wq, wk, tab, N, defect=None):
    """qkv bf16 [T, 3, heads, 72] -> bf16 of the same shape.  defect: 'mean64' / 'mean80' (the divisor of another head dimension)"""
    T, _, heads, _ = qkv.shape
    rows = torch.arange(T) % N
    out = qkv.clone()
    n_mean = {"mean64": 64, "mean80": 80}.get(defect, 72)
    for i, w in ((0, wq), (1, wk)):
        x = qkv[:, i].to(F32)
        xl, r = _head_stats(x, n_mean=n_mean)
        z = _unlanes(xl * r) * w.to(F32)
        if tab is not None:
            z = rope_pairs(z.reshape(T, heads * HD), tab, rows, fp32=True).reshape(z.shape)
        out[:, i] = z.to(BF)
    return out


def _ordered_head_sum(terms):
    """terms fp32 [units, 72] (zero rows for the other operand's units) -> [72] in the order of tv_qknorm_rope_bwd_hd"""
    units = terms.shape[0]
    nblk, passes = qk_geometry(units)
    t = F.pad(terms, (0, 0, 0, passes * nblk * QK_GROUPS - units)).view(passes, nblk, QK_GROUPS, HD)
    acc = torch.zeros(nblk, QK_GROUPS, HD, dtype=F32)
    for p in range(passes):
        acc = acc + t[p]
    blk = torch.zeros(nblk, HD, dtype=F32)
    for gI in range(QK_GROUPS):
        blk = blk + acc[:, gI]
    lanes = torch.zeros(QK_FIN_LANES, HD, dtype=F32)
    rows = F.pad(blk, (0, 0, 0, math.ceil(nblk / QK_FIN_LANES) * QK_FIN_LANES - nblk)).view(-1, QK_FIN_LANES, HD)
    for k in range(rows.shape[0]):
        lanes = lanes + rows[k]
    out = torch.zeros(HD, dtype=F32)
    for i in range(QK_FIN_LANES):
        out = out + lanes[i]
    return out


def qknorm_bwd_emulate(qkv, wq, wk, dqkv, defect=None):
    """-> (dqkv bf16 in place of the q and k thirds, dwq, dwk fp32 [72])"""
    T, _, heads, _ = qkv.shape
    out = dqkv.clone()
    n_mean = {"mean64": 64, "mean80": 80}.get(defect, 72)
    inv = INV_HD if n_mean == 72 else torch.tensor(1.0 / n_mean, dtype=F32)
    terms = torch.zeros(2, T, 2, heads, HD, dtype=F32)
    for i, w in ((0, wq), (1, wk)):
        xl, r = _head_stats(qkv[:, i].to(F32), n_mean=n_mean)
        qh = xl * r
        d = _lanes(dqkv[:, i].to(F32))
        g = d * _lanes(w.to(F32))
        m = _group_sum(LR._head_chain(g, qh)) * inv
        inner = fma32(-qh, m.unsqueeze(-1).expand_as(qh), g)
        out[:, i] = _unlanes(r * inner).to(BF)
        terms[i, :, i] = _unlanes(d * qh)
    return out, _ordered_head_sum(terms[0].reshape(-1, HD)), _ordered_head_sum(terms[1].reshape(-1, HD))


# ---------------------------------------------------------------------------------------------------------------------------
# shapes and inputs
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = ((2, 1, 1), (1, 5, 3), (3, 65, 2), (1, 257, 2), (1, 256, 16), (1, 1024, 1))       # (B, N, heads) at head_dim 72
GRIDS = {1: (1, 1), 5: (1, 5), 65: (5, 13), 257: None, 256: (16, 16), 1024: (32, 32)}      # token grid of each N (257: no table)
SPIKES = {1024: ((70, 3, 30.0), (500, 40, 30.0), (1000, 77, 30.0))}                         # (key, query, score gain) of the long case


def table_of(N):
    return None if GRIDS[N] is None else rope_table(*GRIDS[N])


def qk_inputs(B, N, heads, seed):
    """bf16 qkv and gradient [B N, 3, heads, 72], weights about 1, the table of the token grid; head vector (0, q, 0) is all zero"""
    g = torch.Generator().manual_seed(seed)
    T = B * N
    qkv = (torch.randn(T, 3, heads, HD, generator=g) * (0.3 + 2 * torch.rand(T, 3, heads, 1, generator=g))).to(BF)
    qkv[0, 0, 0] = 0.0
    dqkv = (torch.randn(T, 3, heads, HD, generator=g) * 0.1).to(BF)
    wq, wk = 1 + 0.3 * torch.randn(HD, generator=g), 1 + 0.3 * torch.randn(HD, generator=g)
    return {"qkv": qkv, "dqkv": dqkv, "wq": wq, "wk": wk, "tab": table_of(N)}


def attn_inputs(B, N, heads, seed, qk_scale=1.5):
    """bf16 qkv [B, N, 3, heads, 72] and do [B, N, heads, 72].  SPIKES: key kj of every slice is aligned with query qi so that its
    score stands `gain` (natural-log units of the scaled score) above a typical one: many key blocks with a moving maximum"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3, heads, HD, generator=g, dtype=F64)
    qkv[:, :, :2] *= qk_scale
    for kj, qi, gain in SPIKES.get(N, ()):
        qv = qkv[:, qi, 0]
        qkv[:, kj, 1] = qv * (gain / SCALE) / (qv * qv).sum(-1, keepdim=True)
    do = torch.randn(B, N, heads, HD, generator=g, dtype=F64)
    return qkv.to(BF), do.to(BF)


# ---------------------------------------------------------------------------------------------------------------------------
def mint():
    out = {"model_args": MODEL_ARGS, "batch": MODEL_B, "cases": {}, "sampler": {}, "train": {}}
    for i, case in enumerate(MODEL_CASES):
        seeds = {"state": 500 + i, "batch": 600 + i}
        sd, batch = make_state(case, seeds["state"], True), make_batch(case, seeds["batch"])
        v32, l32, g32 = flow_step(build(case, sd), batch)
        v16, l16, g16 = flow_step(build(case, sd), batch, autocast=True)
        out["cases"][case] = {"seeds": seeds, "loss_fp32": float(l32), "loss": abs(float(l16) - float(l32)) / float(l32),
                              "velocity": rel_l2(v16, v32), "grads": {k: rel_l2(g16[k], g32[k]) for k in g32}}
    for i, case in enumerate(SAMPLER_CASES):
        seeds = {"state": 700 + i, "batch": 710 + i}
        sd, batch = make_state(case, seeds["state"], True), make_batch(case, seeds["batch"])
        args = (batch["labels"], batch["noise"], batch["stats"], SAMPLER["steps"], SAMPLER["cfg_scale"])
        out["sampler"][case] = dict(SAMPLER, seeds=seeds, latents=rel_l2(sample(build(case, sd), *args, autocast=True), sample(build(case, sd), *args)))
        seeds = {"state": 800 + i, "batch": 810 + i}
        sd, batch = make_state(case, seeds["state"], False), make_batch(case, seeds["batch"])
        losses = train_steps(build(case, sd), batch, TRAIN["steps"], TRAIN["lr"])
        out["train"][case] = dict(TRAIN, seeds=seeds, first_loss=losses[0], final_loss=losses[-1])
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
