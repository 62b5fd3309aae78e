"""Error budget, host side: fp64 references of every kernel family, the checks that hold a kernel to its rounding contract
("Rounding contract"), and mutation tests proving on the CPU that those checks reject specific, realistic
defects at the tolerance and in the shape class the GPU tests use.

tests/test_error_budget_gpu.py imports the references and the checks from here.  Every bound names its contract row:

  [G] GEMM / convolution forward, one rounding      [D] data gradient, one rounding
  [W] weight gradient, fp32 output                 [A] attention (o, lse, delta, dq, dk, dv)
  [N] GroupNorm + SiLU and the row norms

Checks
  one-rounding bf16 output y of an exact value y64 (check_one_rounding):
      |y - y64| <= ulp_bf16(y64) + slack,
      slack = L' (2^-20 sum_k |x_k w_k| + 2^-24 |bias|) + 2^-20 |z| + 2^-24 |residual|          ([G], [D], [N])
  where L' = max |act'| (1 without an activation, 1.13 GELU, 1.1 SiLU) carries the fp32 accumulation error of the
  pre-activation z through the activation and 2^-20 |z| covers the A&S erf (1.5e-7 absolute, common.h) and the
  __expf / rcp SiLU.  2^-20 sum|x w| is the statistical fp32 bound of a sum of K products (error ~ sqrt(K / 32) 2^-25
  sum|x w| for K / 32 MFMA roundings, well below it up to K = 13 824), not the worst case gamma_K.  Bias: over the elements
  whose slack is below ulp/16 (one per distinct y64), mean(sign(y64) (y - y64) / ulp(y64)) within +-0.02 (RNE: 0 +- 1e-3 at 1e5 elements).
  fp32 output (check_fp32): |y - y64| <= c 2^-24 sum|terms| + 2^-24 |y64|, c stated at each use.
  attention outputs (check_vs_emulation): per (image, head) slice,
      relL2(hip - exact) <= TAU relL2(emul - exact)   and   max|hip - exact| <= 2 max|emul - exact| + ulp_bf16(max|exact|)
  with `emul` the host model of the ideal kernel (attn_fwd_emul / attn_bwd_emul).

The production attention branch (fused.AttnBranchFn) has its own references here: rms_ln_hat64 / rownorm_bwd64 ([N], mode 1
and the fused residual gradient), rope_epilogue64 ([G], RoPE on the accumulator of the QKV projection) and the `tab` argument
of attn_bwd_exact / attn_bwd_emul ([A], the RoPE adjoint in the dq / dk stores), each with its fp32 emulation and mutations.

The production GroupNorm + SiLU path (fused.gn_silu_fwd / gn_silu_apply / gn_silu_bwd, the calls of fused.ResBlockFn):
gn_stats64 (the mean / rstd bounds about the kernels' pivot, k_s), gn_silu64, gn_bwd64 (the fp64 backward with dres, k_g),
gn_kernel_emul_ordered (fp32 in the kernels' own order of operations) and its eleven mutations.
"""
import functools
import math
import re

import numpy as np
import pytest
import torch

BF = torch.bfloat16
F64 = torch.float64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LAZY = 8.0            # attention.hip TV_ATTN_LAZY (log2 units)
TAU = 1.2             # [A] relL2 ratio; calibrated by test_tau_calibration_from_two_orderings (measured <= 1.04)
BIAS_TOL = 0.02


# ---------------------------------------------------------------------------------------------------------------------------
# rounding helpers
# ---------------------------------------------------------------------------------------------------------------------------
def r16(t):
    """round to bf16 (nearest even), returned as float64"""
    return t.to(torch.float32).to(BF).to(F64)


def rtz16(t):
    """round toward zero to bf16 (the defect of mutation 2), as float64"""
    b = t.to(torch.float32).contiguous().view(torch.int32)
    return (b & ~0xFFFF).view(torch.float32).to(F64)


def f32(t):
    return t.to(torch.float32).to(F64)


def ulp16(y64):
    """one bf16 ulp at |y64| (8 significant bits): 2^(floor(log2|y|) - 7), floored at the smallest normal's ulp"""
    _, e = torch.frexp(y64.abs().to(F64))
    e = torch.clamp(e, min=-125)
    return torch.ldexp(torch.ones_like(y64, dtype=F64), (e - 8).to(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# activations in fp64
# ---------------------------------------------------------------------------------------------------------------------------
def act64(z, act):
    if act == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == "silu":
        return z * torch.sigmoid(z)
    return z


def act_grad64(z, act):
    if act == "gelu":
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act == "silu":
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    return torch.ones_like(z)


LIP = {None: 1.0, "gelu": 1.13, "silu": 1.1}         # max |act'|
LIP2 = {None: 0.0, "gelu": 0.8, "silu": 0.5}         # max |act''|


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references  (inputs: the bf16-rounded values the kernel consumes, any float dtype)
# ---------------------------------------------------------------------------------------------------------------------------
def conv64(x, w, mode):
    """exact conv / linear of NHWC x and [Cout, KH, KW, Cin] (or [Cout, Cin]) w -> (y64 NHWC, sum |x w| NHWC)"""
    import torch.nn.functional as F
    x, w = x.to(F64), w.to(F64)

    def one(xx, ww):
        if mode == "linear":
            return xx @ ww.t()
        xn, wn = xx.permute(0, 3, 1, 2), ww.permute(0, 3, 1, 2)
        if mode == "c3s1":
            y = F.conv2d(xn, wn, padding=1)
        elif mode == "c3s2":
            y = F.conv2d(xn, wn, stride=2, padding=1)
        elif mode == "c3up":
            y = F.conv2d(F.interpolate(xn, scale_factor=2, mode="nearest"), wn, padding=1)
        elif mode == "unshuf":
            y = F.conv2d(xn, wn, stride=2)
        elif mode == "shuf":
            y = F.conv2d(xn, wn)
            B, C4, H, W = y.shape
            cq = C4 // 4
            y = y.view(B, 2, 2, cq, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, cq, 2 * H, 2 * W)
        else:
            raise ValueError(mode)
        return y.permute(0, 2, 3, 1).contiguous()
    return one(x, w), one(x.abs(), w.abs())


def epilogue64(acc, absdot, bias=None, residual=None, act=None):
    """[G] out = act(acc + bias) + residual in fp64 -> (y64, slack, z64)"""
    z = acc + (0 if bias is None else bias.to(F64))
    y = act64(z, act)
    zerr = 2.0 ** -20 * absdot + (0 if bias is None else 2.0 ** -24 * bias.to(F64).abs())
    slack = LIP[act] * zerr + (2.0 ** -20 * z.abs() if act else 0)
    if residual is not None:
        y = y + residual.to(F64)
        slack = slack + 2.0 ** -24 * residual.to(F64).abs()
    return y, slack, z


def deriv64(z, absdot, bias, act):
    """[G] saved derivative act'(z) of the fp32 z -> (d64, slack): the A&S / __expf error 2^-20 (1 + |z|) plus act'' times
    the accumulation error of z"""
    zerr = 2.0 ** -20 * absdot + (0 if bias is None else 2.0 ** -24 * bias.to(F64).abs())
    return act_grad64(z, act), LIP2[act] * zerr + 2.0 ** -20 * (1.0 + z.abs())


def wgrad64(x, g):
    """[W] dw[o, i] = sum_t g[t, o] x[t, i] for row-major token matrices -> (dw64, sum |g x|)"""
    x, g = x.to(F64).reshape(-1, x.shape[-1]), g.to(F64).reshape(-1, g.shape[-1])
    return g.t() @ x, g.abs().t() @ x.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------
def one_rounding_report(y, y64, slack):
    """(max of |y - y64| / (ulp + slack), max ulps, sign-aware mean ulps over well-conditioned elements, their count)"""
    y, y64 = y.to(F64), y64.to(F64)
    slack = torch.as_tensor(slack, dtype=F64).expand_as(y64)
    u = ulp16(y64)
    err = y - y64
    ratio = (err.abs() / (u + slack)).max().item() if err.numel() else 0.0
    ulps = (err.abs() / u).max().item() if err.numel() else 0.0
    good = (slack < u / 16) & (y64 != 0)
    # one sample per distinct exact value: inputs with few distinct values (a bf16 x at |mean| / std = 100 takes ~20 levels per
    # channel) repeat the same rounding many times, which is no bias of the kernel
    yv, idx = torch.unique(y64[good], return_inverse=True)
    first = torch.full((yv.numel(),), -1, dtype=torch.long).scatter_reduce(
        0, idx, torch.arange(idx.numel()), reduce="amin", include_self=False)
    n = yv.numel()
    e, uu = err[good][first], u[good][first]
    mean = (torch.sign(yv) * e / uu).mean().item() if n else 0.0
    return ratio, ulps, mean, n


def check_one_rounding(y, y64, slack, what, min_bias_n=2000):
    """[G]/[D]/[N]: |y - y64| <= ulp_bf16(y64) + slack element by element, and no rounding bias (|mean| <= BIAS_TOL over the
    distinct exact values whose slack is below ulp / 16, when there are at least `min_bias_n` of them)."""
    ratio, ulps, mean, n = one_rounding_report(y, y64, slack)
    if ratio > 1.0:
        y64d, yd = y64.to(F64).flatten(), y.to(F64).flatten()
        sl = torch.as_tensor(slack, dtype=F64).expand_as(y64.to(F64)).flatten()
        i = int(((yd - y64d).abs() / (ulp16(y64d) + sl)).argmax())
        raise AssertionError(f"{what}: |y - y64| = {ratio:.3g} x (ulp + slack) at flat index {i}: y={yd[i].item():.8g} "
                             f"y64={y64d[i].item():.8g} slack={sl[i].item():.3g}")
    if n >= min_bias_n:
        assert abs(mean) <= BIAS_TOL, f"{what}: rounding bias {mean:+.4f} ulp over {n} elements"
    return ratio, ulps, mean


def check_fp32(y, y64, absterms, c, what):
    """[W]/[A]/[N] fp32 outputs: |y - y64| <= c 2^-24 absterms + 2^-24 |y64| element by element; returns the max ratio"""
    y, y64 = y.to(F64), y64.to(F64)
    bound = c * 2.0 ** -24 * torch.as_tensor(absterms, dtype=F64) + 2.0 ** -24 * y64.abs() + 1e-300
    r = ((y - y64).abs() / bound).max().item()
    assert r <= 1.0, f"{what}: |y - y64| = {r:.3g} x the bound c={c} 2^-24 sum|terms|"
    return r


def rel_l2(a, b):
    a, b = a.to(F64), b.to(F64)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def check_vs_emulation(hip, emul, exact, what, tau=TAU):
    """[A]: one (image, head) slice -- relL2(hip - exact) <= tau relL2(emul - exact) and
    max|hip - exact| <= 2 max|emul - exact| + ulp_bf16(max|exact|).  Returns (relL2 ratio, max ratio)."""
    e_h, e_e = rel_l2(hip, exact), rel_l2(emul, exact)
    hip, emul, exact = hip.to(F64), emul.to(F64), exact.to(F64)
    m_h, m_e = (hip - exact).abs().max().item(), (emul - exact).abs().max().item()
    one = ulp16(exact.abs().max().reshape(1)).item()
    assert e_h <= tau * e_e, f"{what}: relL2 {e_h:.4g} > {tau} x emulation {e_e:.4g}"
    assert m_h <= 2 * m_e + one, f"{what}: max err {m_h:.4g} > 2 x emulation {m_e:.4g} + ulp {one:.3g}"
    return e_h / max(e_e, 1e-300), m_h / max(2 * m_e + one, 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------
# attention: exact fp64 and the ideal-kernel emulation (one (image, head) slice: q, k, v [N, 64])
# ---------------------------------------------------------------------------------------------------------------------------
def attn_exact(q, k, v, scale):
    """fp64 softmax(q k^T scale) v and lse (natural log)"""
    s = (q.to(F64) @ k.to(F64).t()) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[:, None])
    return p @ v.to(F64), lse


def attn_fwd_emul(q, k, v, scale, kblock=64, group=32, order=None, mutate=None):
    """[A] the forward kernel's documented policy for the queries q (one or more whole waves) against all keys k: fp32 scores; rows in waves of `group` queries; key blocks of `kblock`;
    a wave rescales its running (m, l, O) only when some row's block max exceeds m by more than LAZY / c2
    (TV_ATTN_LAZY, attention.hip:467-489); p = exp2(s c2 - m c2) in fp32, l sums fp32 p, P enters PV as bf16
    (attention.hip:469,498), O in fp32; o = bf16(O / l) and lse = (m c2 + log2 l) ln2.
    order: permutation of the key blocks (the calibration's reordered emulation).  mutate: 'p2' (P rounded twice) or
    'lazy_quarter' (at a rescale that moves a row's max by LAZY..LAZY+1, a quarter of its O stays unscaled)."""
    N, Nk = q.shape[0], k.shape[0]
    c2 = float(np.float32(scale * LOG2E))
    s_all = f32(q.to(F64) @ k.to(F64).t())
    v64 = v.to(F64)
    nb = -(-Nk // kblock)
    blocks = list(range(nb)) if order is None else list(order)
    o = torch.empty(N, v.shape[1], dtype=F64)
    lse = torch.empty(N, dtype=F64)
    for g0 in range(0, N, group):
        rows = slice(g0, min(N, g0 + group))
        m = torch.full((rows.stop - rows.start,), -math.inf, dtype=F64)
        l = torch.zeros_like(m)
        O = torch.zeros(rows.stop - rows.start, v.shape[1], dtype=F64)
        for t in blocks:
            s = s_all[rows, t * kblock:min(Nk, (t + 1) * kblock)]
            vb = v64[t * kblock:min(Nk, (t + 1) * kblock)]
            mloc = s.max(1).values
            grow = (mloc - m) * c2
            if bool((grow > LAZY).any()):
                mnew = torch.maximum(m, mloc)
                alpha = f32(torch.exp2(f32((m - mnew) * c2)))
                alpha = torch.where(torch.isfinite(m), alpha, torch.zeros_like(alpha))
                if mutate == "lazy_quarter":
                    hit = ((grow > LAZY) & (grow < LAZY + 1) & torch.isfinite(m))[:, None]
                    O = torch.where(hit, f32(0.75 * alpha[:, None] * O + 0.25 * O), f32(alpha[:, None] * O))
                else:
                    O = f32(alpha[:, None] * O)
                l = f32(alpha * l)
                m = mnew
            p = f32(torch.exp2(f32(s * c2 - f32(m * c2)[:, None])))
            l = f32(l + f32(p.sum(1)))
            pb = r16(p)
            if mutate == "p2":
                pb = r16(pb * 0.75) / 0.75
            O = f32(O + pb @ vb)
        o[rows] = r16(f32(O / l[:, None]))
        lse[rows] = f32(f32(f32(m * c2) + f32(torch.log2(l))) * LN2)
    return o, lse


def rope_pairs(t, tab, rows, kind="forward", fp32=False):
    """The reference's (non-orthogonal) RoPE 2x2 on the 64-wide heads of t [M, n 64], pair p = (t[2p], t[2p+1]) = (a, b), with
    row rows[m] of tab [tokens, 4, 32] = (c1, s1, c2, s2):
      forward  y[2p] = a c1 - b s1,   y[2p+1] = a s2 + b c2        (igemm_common.h:302-310)
      adjoint  a'    = a c1 + b s2,   b'      = -a s1 + b c2       (attention.hip:309-317)
    fp32: each product and the sum rounded to fp32 (the kernels' arithmetic on their fp32 accumulators)."""
    rd = f32 if fp32 else (lambda v: v)
    M = t.shape[0]
    tp = t.to(F64).reshape(M, -1, 32, 2)
    a, b = tp[..., 0], tp[..., 1]
    c1, s1, c2, s2 = (tab.to(F64)[rows, i][:, None, :] for i in range(4))
    if kind == "forward":
        ya, yb = rd(rd(a * c1) - rd(b * s1)), rd(rd(a * s2) + rd(b * c2))
    else:
        ya, yb = rd(rd(a * c1) + rd(b * s2)), rd(rd(b * c2) - rd(a * s1))
    return torch.stack([ya, yb], -1).reshape(t.shape)


def attn_bwd_exact(q, k, v, o, do, lse, scale, tab=None):
    """fp64 backward of the forward the kernel saved (its bf16 o and fp32 lse): delta = sum(do o), P = exp(s - lse),
    dS = P (do v^T - delta), dq = scale dS k, dk = scale dS^T q, dv = P^T do.  tab [N, 4, 32]: q, k are the rotated values
    and dq, dk the gradients of the un-rotated projections (the RoPE adjoint of the query's / the key's token)."""
    q, k, v, o, do, lse = (t.to(F64) for t in (q, k, v, o, do, lse))
    delta = (do * o).sum(1)
    p = torch.exp(q @ k.t() * scale - lse[:, None])
    ds = p * (do @ v.t() - delta[:, None])
    dq, dk = scale * ds @ k, scale * ds.t() @ q
    if tab is not None:
        rows = torch.arange(q.shape[0])
        dq, dk = rope_pairs(dq, tab, rows, "adjoint"), rope_pairs(dk, tab, rows, "adjoint")
    return dq, dk, p.t() @ do, delta


def split3(x):
    """fp32 x as three bf16 pieces hi + mid + lo (attention.hip:867-877)"""
    d0 = r16(x)
    r1 = f32(x - d0)
    d1 = r16(r1)
    d2 = r16(f32(r1 - d1))
    return d0, d1, d2


def attn_bwd_emul(q, k, v, o, do, lse, scale, mutate=None, tab=None):
    """[A] the backward kernels' documented policy: delta = fp32 sum of do o; P = exp2(s c2 - lse log2e) in fp32;
    dP - delta accumulated in fp32 from -delta as three bf16 pieces; dS = P (dP - delta) rounded to bf16 for dq and dk,
    P rounded to bf16 for dv; fp32 sums; scale applied to the fp32 sum; one rounding of each output.
    tab [N, 4, 32]: the RoPE adjoint of the query's (dq) / the key's (dk) token applied in fp32 to the scaled fp32 sums
    before that one rounding (attention.hip:960-962, 1145-1147).
    mutate 'delta1': -delta enters as one bf16 piece.  With a table: 'rope_fwd' (the forward rotation in place of the
    adjoint), 'rope_row32' (table row of token + 32), 'rope_after' (adjoint applied to the rounded dq / dk, rounded again)."""
    q, k, v, o, do = (t.to(F64) for t in (q, k, v, o, do))
    c2 = float(np.float32(scale * LOG2E))
    delta = f32((do * o).sum(1))
    nl = f32(-f32(lse.to(F64)) * LOG2E)
    s = f32(q @ k.t())
    p = f32(torch.exp2(f32(s * c2 + nl[:, None])))
    nd = sum(split3(-delta)) if mutate != "delta1" else r16(-delta)
    dpm = f32(do @ v.t() + nd[:, None])
    ds = r16(f32(p * dpm))
    dq = f32(f32(ds @ k) * scale)
    dk = f32(f32(ds.t() @ q) * scale)
    if tab is not None:
        rows = torch.arange(q.shape[0])
        if mutate == "rope_row32":
            rows = (rows + 32) % tab.shape[0]
        kind = "forward" if mutate == "rope_fwd" else "adjoint"
        if mutate == "rope_after":
            dq, dk = r16(dq), r16(dk)
        dq, dk = rope_pairs(dq, tab, rows, kind, fp32=True), rope_pairs(dk, tab, rows, kind, fp32=True)
    dv = r16(f32(r16(p).t() @ do))
    return r16(dq), r16(dk), dv, delta


# ---------------------------------------------------------------------------------------------------------------------------
# norms in fp64
# ---------------------------------------------------------------------------------------------------------------------------
GN_THREADS, GN_SLAB = 256, 512      # norm.hip: GN_THREADS, GN_PIX_PER_BLOCK
U32 = 2.0 ** -24                     # unit roundoff of fp32


def gn_rows(C):
    """pixel lanes of a GroupNorm block: nch = C / 8 threads cover one pixel, rows = 256 / nch pixels per sweep"""
    return GN_THREADS // (C // 8)


def gn_chain(hw, C):
    """additions behind one per-channel sum of the GroupNorm kernels: a lane's chain over its pixels of a slab, the lanes in
    order through LDS, the slabs in order (gn_finalize_kernel)"""
    rows = gn_rows(C)
    return -(-min(hw, GN_SLAB) // rows) + rows + -(-hw // GN_SLAB)


def gn_k_s(hw, C, G):
    """[N] additions behind a GROUP sum of the forward: the channel chain, the cpg channels merged by gn_prepare, and 4 for
    x - piv, the product by 1 / hw, piv + S / hw and the division by cpg"""
    return gn_chain(hw, C) + C // G + 4


def gn_k_g(hw, C, B):
    """[N] additions behind dgamma / dbeta: the channel chain, the B images (atomics) and 4 for xhat, h, silu' and dh"""
    return gn_chain(hw, C) + B + 4


def gn_stats64(x, G, eps=1e-5):
    """[N] two-pass fp64 statistics of x [B, HW, C] per (image, group) and the bounds of row N, stated about the kernel's
    pivot piv[b, c] = x[b, 0, c] (row B's form) -> (mean [B, G], var, rstd, bound on |mean - mean64|, bound on
    |rstd / rstd64 - 1|).  With dm_c = mean_c - piv_c and k_s = gn_k_s:
        |mean - mean64|      <= k_s u mean|x - piv| + (cpg + 1) u mean_c|mean_c|
        |rstd / rstd64 - 1|  <= k_s u (1 + mean_c(dm_c^2) / (var + eps)) + 2 u
    (the sums S = sum(x - piv) and Q = sum (x - piv)^2 carry k_s u of sum|x - piv| and of hw (var_c + dm_c^2); var + eps is
    what rstd is taken of, so the ratio is finite at var = 0; 2 u: the division and rsqrtf; (cpg + 1) u: each mean_c = piv + S / hw
    is rounded at its own magnitude, the cpg - 1 additions of gn_prepare's chain at up to cpg mean|mean_c|, then the division
    -- a single u |mean| is exceeded 3 x by the fp32 emulation at cpg = 48, |mean| = 100 std).  Plain torch on x's device."""
    x = x.to(F64)
    B, HW, C = x.shape
    xg = x.view(B, HW, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, G, 1)) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    piv = x[:, :1, :]
    absdev = (x - piv).abs().mean(1).view(B, G, C // G).mean(2)
    mc = x.mean(1, keepdim=True)
    dm2 = ((mc - piv) ** 2).view(B, G, C // G).mean(2)
    k = gn_k_s(HW, C, G) * U32
    bm = k * absdev + (C // G + 1) * U32 * mc.abs().view(B, G, C // G).mean(2)
    return mean, var, rstd, bm, k * (1.0 + dm2 / (var + eps)) + 2 * U32


def check_gn_stats(x, G, mr, what, eps=1e-5):
    """[N] mr [B, G, 2] = the (mean, rstd) a forward wrote, against gn_stats64's bounds -> (mean ratio, rstd ratio)"""
    mean64, _, rstd64, bm, br = gn_stats64(x, G, eps)
    mr = mr.to(F64).to(mean64.device)
    rm = ((mr[..., 0] - mean64).abs() / (bm + 1e-300)).max().item()
    rr = ((mr[..., 1] / rstd64 - 1).abs() / br).max().item()
    assert rm <= 1.0, f"{what}: mean off by {rm:.3g} x its bound"
    assert rr <= 1.0, f"{what}: rstd off by {rr:.3g} x its bound"
    return rm, rr


def _per_channel(t, C):
    """[B, G] -> [B, 1, C]"""
    B, G = t.shape
    return t.view(B, G, 1).expand(B, G, C // G).reshape(B, 1, C)


def gn_silu64(x, gamma, beta, G, eps=1e-5):
    """[N] y = silu(gamma (x - mean) rstd + beta) per (image, group), two-pass fp64 statistics; x [B, HW, C] ->
    (y64, slack, z64, xhat64, rstd64[B, G])"""
    x = x.to(F64)
    B, HW, C = x.shape
    xg = x.view(B, HW, G, C // G)
    mu = xg.mean((1, 3), keepdim=True)
    var = ((xg - mu) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = ((xg - mu) * rstd).view(B, HW, C)
    z = xh * gamma.to(F64) + beta.to(F64)
    sc = (gamma.to(F64).view(1, G, C // G) * rstd.view(B, G, 1)).reshape(B, 1, C)
    # z = x sc + sh in fp32 (norm.hip:184): 2^-22 (|x sc| + |sh|) before the activation, then [G]'s 2^-20 |z|
    sh = beta.to(F64) - (mu.view(B, G, 1) * gamma.to(F64).view(1, G, C // G) * rstd.view(B, G, 1)).reshape(B, 1, C)
    slack = LIP["silu"] * 2.0 ** -22 * ((x * sc).abs() + sh.abs() + z.abs()) + 2.0 ** -20 * z.abs()
    # the statistics' own error, stated about the pivot (gn_stats64): rstd scales z - beta, the mean shifts z by sc
    _, _, _, bm, br = gn_stats64(x, G, eps)
    slack = slack + LIP["silu"] * ((z - beta.to(F64)).abs() * _per_channel(br, C) + sc.abs() * _per_channel(bm, C))
    return act64(z, "silu"), slack, z, xh, rstd.view(B, G)


def gn_bwd64(x, gamma, beta, gy, dres, G, eps=1e-5):
    """[N] backward of silu(groupnorm(x)) in fp64 [+ dres] -> (dx64, dx slack, dgamma64, dbeta64, terms of dgamma / dbeta).
    g' = gy silu'(z);  dx = rstd (gamma g' - mean(gamma g') - xhat mean(gamma g' xhat)) per (image, group).
    dx slack: 2^-19 terms (1 + |mu| rstd) + 2^-20 |dx64| [+ 2^-24 |dres|]  (terms = the formula on absolute values; fp32 z
    carries 2^-22 (|x sc| + |sh|) into silu', hence the conditioning factor: the row-norm form), plus the rstd bound of
    gn_stats64 times terms (3 + |z - beta|): rstd is a factor of dx, enters xhat twice in xhat mean(g' xhat) and moves silu'
    by |silu''| |z - beta| <= |z - beta| / 2 of its relative error.
    dgamma = sum g' xhat, dbeta = sum g' (over images and pixels); their terms: sum |g'| (|mu| rstd + |xhat| + 1), xhat being
    good to 2^-22 of |x| rstd."""
    x, gamma, beta, gy = x.to(F64), gamma.to(F64), beta.to(F64), gy.to(F64)
    B, HW, C = x.shape
    cpg = C // G
    _, _, z, xh, rstd = gn_silu64(x, gamma, beta, G, eps)
    gp = gy * act_grad64(z, "silu")
    gpg = (gp * gamma).view(B, HW, G, cpg)
    xhg = xh.view(B, HW, G, cpg)
    r = rstd.view(B, 1, G, 1)
    m1 = gpg.mean((1, 3), keepdim=True)
    m2 = (gpg * xhg).mean((1, 3), keepdim=True)
    dx64 = (r * (gpg - m1 - xhg * m2)).view(B, HW, C)
    mu_r = (x.view(B, HW, G, cpg).mean((1, 3), keepdim=True) * r).abs().expand(B, HW, G, cpg).reshape(B, HW, C)
    terms = (r * (gpg.abs() + gpg.abs().mean((1, 3), keepdim=True) + xhg.abs() * (gpg * xhg).abs().mean((1, 3), keepdim=True))).view(B, HW, C)
    br = _per_channel(gn_stats64(x, G, eps)[4], C)
    dsl = 2.0 ** -19 * terms * (1 + mu_r) + 2.0 ** -20 * dx64.abs() + br * terms * (3 + (z - beta).abs())
    if dres is not None:
        dx64 = dx64 + dres.to(F64)
        dsl = dsl + 2.0 ** -24 * dres.to(F64).abs()
    pterms = (gp.abs() * (mu_r + xh.abs() + 1)).sum((0, 1))
    return dx64, dsl, (gp * xh).sum((0, 1)), gp.sum((0, 1)), pterms


EPS_RMS, EPS_LN = 1e-6, 1e-5


def rms_hat64(x, eps=EPS_RMS):
    """[N] mode 0: y = x r, r = rsqrt(mean x^2 + eps) -> (y64, r)"""
    x = x.to(F64)
    r = torch.rsqrt((x * x).mean(1, keepdim=True) + eps)
    return x * r, r


def rms_ln_hat64(x, w, eps_rms=EPS_RMS, eps_ln=EPS_LN):
    """[N] mode 1: RMSNorm x weight, then the affine-free LayerNorm.  r = rsqrt(mean x^2 + eps_rms), u = x r w, mu = mean u,
    s = rsqrt(var u + eps_ln), y = (u - mu) s -> (y64, u, mu, s, r); differentiable (the backward reference is its autograd)"""
    x, w = x.to(F64), w.to(F64)
    r = torch.rsqrt((x * x).mean(1, keepdim=True) + eps_rms)
    u = x * r * w
    mu = u.mean(1, keepdim=True)
    s = torch.rsqrt(((u - mu) ** 2).mean(1, keepdim=True) + eps_ln)
    return (u - mu) * s, u, mu, s, r


def rms_ln_slack(y64, u, mu, s):
    """[N] y of mode 1: u carries three fp32 roundings and the rsqrt, mu an fp32 sum, both enter (u - mu) s; |y64| is s's own
    relative error"""
    return 2.0 ** -20 * (s * (u.abs() + mu.abs()) + y64.abs())


def rownorm_bwd64(x, w, gy, dres, mode):
    """[N] backward of rms_hat (mode 0, w ignored) / rms_ln_hat (mode 1) by fp64 autograd, + dres ->
    (dx64, dx slack, dw64 | None, dw terms | None).
    terms = the backward formula on absolute values:  du = s (g - mean g - y mean(g y)),  dw = sum_t du xhat,  gx = du w,
    dx = r (gx - xhat mean(gx xhat)).
    dx slack: mode 0  2^-19 terms + 2^-24 |dres|;  mode 1  2^-19 terms (1 + |mu| s) + 2^-20 |dx64| + 2^-24 |dres|  (the
    conditioning factor: y = (u - mu) s is recomputed in fp32, its error is 2^-24 (|u| + |mu|) s).
    dw terms: sum_t |du xhat| (1 + |mu| s)."""
    x64 = x.to(F64).clone().requires_grad_(True)
    w64 = w.to(F64).clone().requires_grad_(True) if mode == 1 else None
    y = rms_ln_hat64(x64, w64)[0] if mode == 1 else rms_hat64(x64)[0]
    y.backward(gy.to(F64))
    dx64 = x64.grad if dres is None else x64.grad + dres.to(F64)
    x, gy = x.to(F64), gy.to(F64)
    xh, r = rms_hat64(x)
    mean = lambda t: t.mean(1, keepdim=True)
    if mode == 1:
        y, _, mu, s, _ = rms_ln_hat64(x, w)
        cond = 1 + mu.abs() * s
        du = s * (gy - mean(gy) - y * mean(gy * y))
        g_abs = s * (gy.abs() + mean(gy.abs()) + y.abs() * mean((gy * y).abs())) * w.to(F64).abs()
        dw_terms = ((du * xh).abs() * cond).sum(0)
    else:
        cond, g_abs, dw_terms = 1.0, gy.abs(), None
    terms = r * (g_abs + xh.abs() * mean(g_abs * xh.abs()))
    slack = 2.0 ** -19 * terms * cond + (2.0 ** -20 * dx64.abs() if mode == 1 else 0)
    if dres is not None:
        slack = slack + 2.0 ** -24 * dres.to(F64).abs()
    return dx64, slack, (w64.grad if mode == 1 else None), dw_terms


def rope_epilogue64(acc, absdot, bias, tab, tokens, rope_cols):
    """[G] the QKV projection with RoPE on its fp32 accumulator: z = acc + bias; columns < rope_cols (whole 64-wide heads) are
    rotated pair by pair with table row m % tokens (rope_pairs), the others are the plain projection -> (y64, slack).
    Slack of a rotated element a c - b s:  2^-20 (absdot_a |c| + absdot_b |s|)  (accumulation)  + 2^-24 (|bias_a c| +
    |bias_b s|)  (bias add)  + 2^-23 (|a c| + |b s|)  (the two products and their sum); epilogue64's on the others."""
    z, slack, _ = epilogue64(acc, absdot, bias)
    M = z.shape[0]
    rows = torch.arange(M) % tokens
    y = z.clone()
    y[:, :rope_cols] = rope_pairs(z[:, :rope_cols], tab, rows)
    atab = tab.to(F64).abs()

    def fwd_mag(t):          # (|a| |c1| + |b| |s1|, |a| |s2| + |b| |c2|) of the pairs of t
        tp = t[:, :rope_cols].abs().reshape(M, -1, 32, 2)
        c1, s1, c2, s2 = (atab[rows, i][:, None, :] for i in range(4))
        return torch.stack([tp[..., 0] * c1 + tp[..., 1] * s1, tp[..., 0] * s2 + tp[..., 1] * c2], -1).reshape(M, rope_cols)
    bterm = fwd_mag(bias.to(F64).expand_as(z)) if bias is not None else 0
    slack = slack.clone()
    slack[:, :rope_cols] = 2.0 ** -20 * fwd_mag(absdot) + 2.0 ** -24 * bterm + 2.0 ** -23 * fwd_mag(z)
    return y, slack


# ---------------------------------------------------------------------------------------------------------------------------
# CPU "kernels" for the mutation tests: the ideal emulation and its deliberately broken variants
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_inputs(M, K, N, seed=0):
    """[G] input design of the GPU tests: per-row scales of x over 2^-6..2^6, per-column scales of w, bias and residual
    that match the accumulator in some columns and dominate it in others"""
    g = torch.Generator().manual_seed(seed)
    rs = torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).to(F64))
    cs = torch.exp2(torch.randint(-2, 3, (N, 1), generator=g).to(F64))
    x = r16(torch.randn(M, K, generator=g, dtype=F64) * rs)
    w = r16(torch.randn(N, K, generator=g, dtype=F64) * cs * K ** -0.5)
    colf = torch.where(torch.arange(N) % 3 == 0, 16.0, 1.0).to(F64)
    b = f32(torch.randn(N, generator=g, dtype=F64) * cs[:, 0] * colf)
    res = r16(torch.randn(M, N, generator=g, dtype=F64) * rs * cs[:, 0] * colf)
    return x, w, b, res


def gemm_kernel_emul(x, w, b, res, act=None, mutate=None, reverse=False):
    """fp32 accumulation (torch fp32 matmul; `reverse` sums K in the opposite order), + bias, act, + residual in fp32, one
    rounding.  Mutations 1-5 of the issue."""
    xs, ws = (x.flip(1), w.flip(1)) if reverse else (x, w)
    if mutate == "drop_kstep":        # 4: one K-step (64 of K) dropped in the ragged last row band only
        M, K = x.shape
        tail = (M // 256) * 256
        acc = (xs.float() @ ws.float().t()).to(F64)
        xk = xs.clone()
        xk[:, 64:128] = 0
        acc[tail:] = (xk[tail:].float() @ ws.float().t()).to(F64)
    else:
        acc = (xs.float() @ ws.float().t()).to(F64)
    if mutate == "round_acc":         # 1: extra bf16 rounding of the accumulator before bias / residual
        acc = r16(acc)
    bb = b.clone()
    if mutate == "bias_col":          # 5: bias read from the neighbouring column in one column tile
        bb[128:256] = b[129:257]
    z = f32(acc + bb)
    y = z if act is None else f32(act64(z, act))
    y = f32(y + res) if res is not None else y
    if mutate == "rtz":               # 2
        return rtz16(y), z
    if mutate == "scale":             # 3: output x (1 + 2^-8)
        return r16(y * (1 + 2.0 ** -8)), z
    return r16(y), z


# ---------------------------------------------------------------------------------------------------------------------------
# tests: the helpers themselves
# ---------------------------------------------------------------------------------------------------------------------------
def test_ulp_and_rounding_helpers():
    y = torch.tensor([1.0, 1.5, -3.0, 0.25, 1e-3], dtype=F64)
    assert ulp16(y).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9, 2.0 ** -17]
    t = torch.tensor([1.0 + 2.0 ** -7 * 0.75, -(1.0 + 2.0 ** -7 * 0.75)], dtype=F64)
    assert r16(t).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    assert rtz16(t).tolist() == [1.0, -1.0]
    d0, d1, d2 = split3(torch.tensor([math.pi * 1e3], dtype=F64).float().to(F64))
    assert abs((d0 + d1 + d2).item() - float(np.float32(math.pi * 1e3))) <= 2.0 ** -24 * math.pi * 1e3


def test_gemm_rows2_rejects_bad_operands():
    """ops.gemm_rows2's operand check (the contiguity / dtype / row checks used to be bypassed by `... and shape_ok or
    wb.numel() == ...`): a non-contiguous or fp32 x2, a short x2 or an fp32 / non-contiguous wb raise before any launch."""
    from transvae.hip import ops
    T, K1, K2, N = 256, 64, 64, 128
    x1 = torch.zeros(T, K1, dtype=BF)
    x2 = torch.zeros(T, K2, dtype=BF)
    wb = torch.zeros(N, K1 + K2, dtype=BF)
    bad = [
        (x1, torch.zeros(K2, T, dtype=BF).t(), wb),               # non-contiguous x2
        (x1, torch.zeros(T, K2), wb),                             # fp32 x2
        (x1, torch.zeros(T // 2, K2, dtype=BF), wb),              # x2 with other rows
        (torch.zeros(T, K1), x2, wb),                             # fp32 x1
        (x1, x2, torch.zeros(N, K1 + K2)),                        # fp32 wb
        (x1, x2, torch.zeros(K1 + K2, N, dtype=BF).t()),          # non-contiguous wb
        (x1, x2, torch.zeros(N, K1 + K2 + 64, dtype=BF)),         # wrong K
    ]
    for a, b, c in bad:
        with pytest.raises(RuntimeError, match="gemm_rows2"):
            ops.gemm_rows2(a, b, c, N)


# ---------------------------------------------------------------------------------------------------------------------------
# mutation tests: [G] / [D] one-rounding outputs (shape class of the GPU tests: ragged M, N over two 128-column tiles)
# ---------------------------------------------------------------------------------------------------------------------------
M_MUT, K_MUT, N_MUT = 512 + 40, 192, 384


@pytest.fixture(scope="module")
def gemm_case():
    x, w, b, res = gemm_inputs(M_MUT, K_MUT, N_MUT, seed=3)
    acc, absdot = conv64(x, w, "linear")
    return x, w, b, res, acc, absdot


@pytest.mark.parametrize("act,with_res", [(None, True), ("gelu", False), ("silu", True)])
def test_clean_emulation_passes_in_both_summation_orders(gemm_case, act, with_res):
    x, w, b, res, acc, absdot = gemm_case
    r = res if with_res else None
    y64, slack, _ = epilogue64(acc, absdot, b, r, act)
    for rev in (False, True):
        y, _ = gemm_kernel_emul(x, w, b, r, act, reverse=rev)
        check_one_rounding(y, y64, slack, f"clean act={act} reverse={rev}")


@pytest.mark.parametrize("mutation", ["round_acc", "rtz", "scale", "drop_kstep", "bias_col"])
def test_gemm_mutations_are_rejected(gemm_case, mutation):
    """mutations 1-5: extra accumulator rounding before the bias / residual, round-toward-zero, x (1 + 2^-8), one K-step
    dropped in the ragged last row band, bias of the neighbouring column in one column tile"""
    x, w, b, res, acc, absdot = gemm_case
    y64, slack, _ = epilogue64(acc, absdot, b, res, None)
    y, _ = gemm_kernel_emul(x, w, b, res, None, mutate=mutation)
    with pytest.raises(AssertionError):
        check_one_rounding(y, y64, slack, mutation)


def test_save_deriv_from_rounded_z_is_rejected(gemm_case):
    """mutation 6: TV_ACT_SAVE_DERIV taking GELU' of bf16(z) instead of the fp32 z"""
    x, w, b, _, acc, absdot = gemm_case
    _, z32 = gemm_kernel_emul(x, w, b, None, "gelu")
    d64, dslack = deriv64(acc + b, absdot, b, "gelu")
    check_one_rounding(r16(act_grad64(z32, "gelu")), d64, dslack, "clean saved derivative")
    with pytest.raises(AssertionError):
        check_one_rounding(r16(act_grad64(r16(z32), "gelu")), d64, dslack, "derivative of bf16(z)")


# ---------------------------------------------------------------------------------------------------------------------------
# [W] weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
WGRAD_C = 16.0      # [W] |dw - dw64| <= 16 2^-24 sum|g x| + 2^-24 |dw64|  (= 2^-20 sum|g x|)


def test_wgrad_missing_pixel_is_rejected():
    """mutation 12: the weight gradient of 4 images x 16 x 16 pixels without one pixel of one image; clean fp32 sums in two
    orders (split-K chunks added in either order) pass"""
    g = torch.Generator().manual_seed(4)
    x = r16(torch.randn(4, 16, 16, 64, generator=g, dtype=F64))
    gy = r16(torch.randn(4, 16, 16, 96, generator=g, dtype=F64))
    dw64, absd = wgrad64(x, gy)
    xt, gt = x.reshape(-1, 64).float(), gy.reshape(-1, 96).float()
    clean = (gt.t() @ xt).to(F64)
    chunks = f32(sum((gt[i::4].t() @ xt[i::4]).to(F64) for i in (3, 1, 2, 0)))
    check_fp32(clean, dw64, absd, WGRAD_C, "clean dw")
    check_fp32(chunks, dw64, absd, WGRAD_C, "clean dw, split-K reordered")
    keep = torch.ones(xt.shape[0], dtype=torch.bool)
    keep[2 * 256 + 7 * 16 + 3] = False
    bad = (gt[keep].t() @ xt[keep]).to(F64)
    with pytest.raises(AssertionError):
        check_fp32(bad, dw64, absd, WGRAD_C, "dw missing a pixel")


# ---------------------------------------------------------------------------------------------------------------------------
# [A] attention
# ---------------------------------------------------------------------------------------------------------------------------
def attn_inputs(N, seed=0, v_offset=0.0, spikes=(), lazy_rows=(), qk_scale=1.5):
    """q, k, v [N, 64] bf16 values.  v_offset: a large common offset (delta >> |dP - delta|).  spikes: (key, query, gain)
    as in test_hip_kernels.py's spiked-key test.  lazy_rows: (query, key, grow) -- key aligned with query so that the
    query's score there exceeds its row max by `grow` in log2 units of scale 0.125"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(N, 64, generator=g, dtype=F64) * qk_scale
    k = torch.randn(N, 64, generator=g, dtype=F64) * qk_scale
    v = v_offset + (0.25 if v_offset else 1.0) * torch.randn(N, 64, generator=g, dtype=F64)
    for kj, qi, gain in spikes:
        k[kj] = q[qi] * gain / 2.0
    q, k, v = r16(q), r16(k), r16(v)
    c2 = 0.125 * LOG2E
    for qi, kj, grow in lazy_rows:
        # the maximum the kernel holds for row qi when key block kj // 64 opens (the lazy policy over its wave of 32)
        g0 = qi // 32 * 32
        s = q[g0:g0 + 32] @ k.t()
        m = torch.full((s.shape[0],), -math.inf, dtype=F64)
        for t in range(kj // 64):
            mloc = s[:, t * 64:(t + 1) * 64].max(1).values
            if bool(((mloc - m) * c2 > LAZY).any()):
                m = torch.maximum(m, mloc)
        # k[kj] along q[qi]: q.k = held max + grow / c2 (a growth of `grow` in log2 units)
        k[kj] = r16(q[qi] * ((m[qi - g0] + grow / c2) / (q[qi] @ q[qi])))
    return q, k, v


def _attn_slice_errors(q, k, v, kblock, mutate=None):
    o_ex, lse_ex = attn_exact(q, k, v, 0.125)
    o_e, lse_e = attn_fwd_emul(q, k, v, 0.125, kblock=kblock)
    o_h, lse_h = attn_fwd_emul(q, k, v, 0.125, kblock=kblock, mutate=mutate)
    return o_h, o_e, o_ex, lse_h, lse_ex


def test_tau_calibration_from_two_orderings():
    """TAU: two ideal emulations that differ only in key-block order (and so in the order of every fp32 sum and in which
    blocks trigger a lazy rescale) are within relL2 ratio 1.04 of each other on these slices (asserted <= 1.08); TAU = 1.2
    leaves room for the kernel's own summation order inside a block and its MFMA accumulation, and still rejects P rounded
    twice (ratio 1.25-1.34 on flat score rows)."""
    worst = 0.0
    for N, kb, seed, vo in ((256, 64, 1, 0.0), (300, 64, 2, 4.0), (512, 32, 3, 0.0)):
        q, k, v = attn_inputs(N, seed=seed, v_offset=vo, spikes=((N // 2 + 3, 5, 6.0),))
        o_ex, _ = attn_exact(q, k, v, 0.125)
        nb = -(-N // kb)
        o_a, _ = attn_fwd_emul(q, k, v, 0.125, kblock=kb)
        o_b, _ = attn_fwd_emul(q, k, v, 0.125, kblock=kb, order=list(reversed(range(nb))))
        ea, eb = rel_l2(o_a, o_ex), rel_l2(o_b, o_ex)
        worst = max(worst, ea / eb, eb / ea)
        check_vs_emulation(o_b, o_a, o_ex, f"reordered N={N}")
    assert worst <= 1.08, worst


def test_attention_p_rounded_twice_is_rejected():
    """mutation 9: P rounded to bf16 twice (once more after a non-power-of-two scale, as a normalised-P variant would);
    flat score rows (q, k of std 0.5), where P's rounding is a visible part of the output error"""
    q, k, v = attn_inputs(256, seed=5, qk_scale=0.5)
    o_h, o_e, o_ex, _, _ = _attn_slice_errors(q, k, v, 64, mutate="p2")
    with pytest.raises(AssertionError):
        check_vs_emulation(o_h, o_e, o_ex, "P rounded twice")


def test_attention_lazy_rescale_defect_is_rejected():
    """mutation 10 (guide T13 hazard a): at a lazy rescale a quarter of the pending O enters unscaled, on rows whose max
    grows just past the threshold; the rows are built to grow by 8.5 (log2) at key block 3, others by 7.5 (no rescale)"""
    N = 512
    lazy = [(qi, 3 * 64 + 10 + qi % 20, 8.5) for qi in range(0, 32, 3)] + [(qi, 4 * 64 + 5, 7.5) for qi in (64 + 3,)]
    q, k, v = attn_inputs(N, seed=6, lazy_rows=lazy)
    o_h, o_e, o_ex, _, _ = _attn_slice_errors(q, k, v, 64, mutate="lazy_quarter")
    o_r, _ = attn_fwd_emul(q, k, v, 0.125, kblock=64, order=list(reversed(range(N // 64))))
    check_vs_emulation(o_r, o_e, o_ex, "clean, reordered")
    with pytest.raises(AssertionError):
        check_vs_emulation(o_h, o_e, o_ex, "quarter unscaled at a lazy rescale")


LSE_C = 16.0     # [A] lse: |lse - lse64| <= 16 2^-24 (1 + |lse64| + scale max_j sum_d |q_d k_jd|) + 2^-24 |lse64|


def lse_terms(q, k, lse64, scale):
    return 1.0 + lse64.abs() + scale * (q.to(F64).abs() @ k.to(F64).abs().t()).max(1).values


def test_lse_offset_is_rejected():
    """mutation 8: lse off by 2^-12; the ideal emulation's lse passes"""
    q, k, v = attn_inputs(300, seed=7)
    _, lse_ex = attn_exact(q, k, v, 0.125)
    _, lse_e = attn_fwd_emul(q, k, v, 0.125)
    terms = lse_terms(q, k, lse_ex, 0.125)
    check_fp32(lse_e, lse_ex, terms, LSE_C, "emulated lse")
    with pytest.raises(AssertionError):
        check_fp32(lse_e + 2.0 ** -12, lse_ex, terms, LSE_C, "lse + 2^-12")


def test_single_piece_delta_is_rejected():
    """mutation 7: -delta entering dq / dk as one bf16 piece, with v = 4 + 0.25 randn (delta >> |dP - delta|)"""
    q, k, v = attn_inputs(256, seed=8, v_offset=4.0)
    g = torch.Generator().manual_seed(9)
    do = r16(torch.randn(256, 64, generator=g, dtype=F64))
    o, lse = attn_fwd_emul(q, k, v, 0.125)
    ex = attn_bwd_exact(q, k, v, o, do, lse, 0.125)
    clean = attn_bwd_emul(q, k, v, o, do, lse, 0.125)
    bad = attn_bwd_emul(q, k, v, o, do, lse, 0.125, mutate="delta1")
    for i, nm in enumerate(("dq", "dk", "dv")):
        check_vs_emulation(clean[i], clean[i], ex[i], nm)
    with pytest.raises(AssertionError):
        check_vs_emulation(bad[0], clean[0], ex[0], "dq with a one-piece delta")


# ---------------------------------------------------------------------------------------------------------------------------
# [N] GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------
def gn_inputs(B, HW, C, G, seed=0):
    """per-(image, group) means up to 100x the std, stds 1e-2 .. 1e2"""
    g = torch.Generator().manual_seed(seed)
    std = 10.0 ** (torch.rand(B, 1, G, 1, generator=g, dtype=F64) * 4 - 2)
    mean = std * (torch.rand(B, 1, G, 1, generator=g, dtype=F64) * 200 - 100)
    x = mean + std * torch.randn(B, HW, G, C // G, generator=g, dtype=F64)
    gamma = f32(1 + 0.2 * torch.randn(C, generator=g, dtype=F64))
    beta = f32(0.2 * torch.randn(C, generator=g, dtype=F64))
    return r16(x.view(B, HW, C)), gamma, beta


def gn_kernel_emul(x, gamma, beta, G, eps=1e-5, one_pass=False):
    """fp32 statistics (two-pass / pivot, or the one-pass E[x^2] - E[x]^2 in sequential fp32 sums: mutation 11),
    z = x sc + sh in fp32, silu, one rounding"""
    B, HW, C = x.shape
    xg = x.view(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    if one_pass:
        xf = xg.float().numpy()
        s1 = np.cumsum(xf, axis=-1, dtype=np.float32)[..., -1]
        s2 = np.cumsum(xf * xf, axis=-1, dtype=np.float32)[..., -1]
        n = np.float32(xg.shape[-1])
        mu = torch.from_numpy(s1 / n).to(F64)
        var = torch.from_numpy(np.maximum(s2 / n - (s1 / n) ** 2, 0).astype(np.float32)).to(F64)
    else:
        mu = f32(xg.mean(-1))
        var = f32(((xg - xg.mean(-1, keepdim=True)) ** 2).mean(-1))
    rstd = f32(1.0 / torch.sqrt(var + eps))
    sc = f32(gamma.view(1, G, C // G) * rstd[:, :, None]).reshape(B, 1, C)
    sh = f32(beta.view(1, G, C // G) - mu[:, :, None] * sc.view(B, G, C // G)).reshape(B, 1, C)
    z = f32(x * sc + sh)
    return r16(act64(z, "silu"))


def gn_pivot_inputs(B, HW, C, G, k, seed=0):
    """gn_inputs with pixel 0 of every channel -- the kernels' pivot -- set k group-sigma above the group mean"""
    x, gamma, beta = gn_inputs(B, HW, C, G, seed)
    xg = x.view(B, HW, G, C // G)
    piv = xg.mean((1, 3)) + k * xg.std((1, 3), unbiased=False)
    x = x.clone()
    x[:, 0, :] = r16(piv.view(B, G, 1).expand(B, G, C // G).reshape(B, C))
    return x, gamma, beta


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two fp32 is exact in fp64 (48 bits); one fp64 sum, rounded to fp32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _silu32(z):
    with np.errstate(over="ignore"):
        return z * (np.float32(1) / (np.float32(1) + np.exp(-z)))


def _silu_grad32(z):
    with np.errstate(over="ignore"):
        s = np.float32(1) / (np.float32(1) + np.exp(-z))
    return s * _fma32(z, np.float32(1) - s, np.float32(1))


def _gn_slab_sums(a, b1, b2, tail=True):
    """the reduction of gn_stats_kernel / gn_silu_bwd_reduce_kernel + gn_finalize_kernel on [B, hw, C] float32 terms:
    s += a and q = fmaf(b1, b2, q) per pixel lane (pixels prow, prow + rows, ... of a 512-pixel slab), the lanes added in
    order, the slabs added in order -> (s, q) [B, C].  Pixels a lane does not have contribute an exact + 0.  tail = False
    leaves the ragged last slab out (a mutation)."""
    B, hw, C = a.shape
    rows = gn_rows(C)
    steps = -(-GN_SLAB // rows)
    nslab = -(-hw // GN_SLAB) if tail else hw // GN_SLAB
    if nslab == 0:
        return np.zeros((B, C), np.float32), np.zeros((B, C), np.float32)

    def slabs(t):
        buf = np.zeros((B, nslab, steps * rows, C), np.float32)
        for s in range(nslab):
            n = min(GN_SLAB, hw - s * GN_SLAB)
            buf[:, s, :n] = t[:, s * GN_SLAB:s * GN_SLAB + n]
        return buf.reshape(B, nslab, steps, rows, C)
    a, b1, b2 = slabs(a), slabs(b1), slabs(b2)
    s = np.zeros((B, nslab, rows, C), np.float32)
    q = np.zeros((B, nslab, rows, C), np.float32)
    for t in range(steps):
        s = s + a[:, :, t]
        q = _fma32(b1[:, :, t], b2[:, :, t], q)
    fold = lambda v: np.cumsum(np.cumsum(v, axis=2, dtype=np.float32)[:, :, -1], axis=1, dtype=np.float32)[:, -1]
    return fold(s), fold(q)


GN_MUTATIONS = ("no_spread", "n_minus_1", "group_of_chunk", "image0_stats", "no_tail", "dres_after", "sums_no_gamma",
                "inv_hw_for_n", "silu_grad_bf16_h", "dgamma_first_image", "sign_s2")


def gn_kernel_emul_ordered(x, gamma, beta, G, gy=None, dres=None, eps=1e-5, mutate=None):
    """fp32 in the order of operations of norm.hip's GroupNorm kernels -> dict(mr [B, G, 2], y, and with gy: dx, dgamma,
    dbeta), float64 tensors of the values the kernels would store.
    Forward: S = sum(x - piv), Q = sum (x - piv)^2 about piv = x[b, 0, c] (_gn_slab_sums); gn_prepare: mean_c = piv + S / hw,
    M2_c = max(Q - S^2 / hw, 0), mean = sum_c mean_c / cpg, var = (sum_c M2_c + hw sum_c (mean_c - mean)^2) / (cpg hw),
    rstd = 1 / sqrt(var + eps); sc = rstd gamma, sh = beta - mean sc, y = bf16(silu(fma(x, sc, sh))).
    Backward: xhat = (x - mean) rstd, h = fma(xhat, gamma, beta), dh = gy silu'(h), red = (sum dh, sum dh xhat) in the same
    order; S1 = sum_c gamma red_0 / n, S2 likewise, n = cpg hw; A = rstd gamma, B = beta - mean A, Cc = rstd^2 S2,
    D = mean Cc - rstd S1; dx = bf16(fma(dh, A, fma(-x, Cc, D)) + dres); dgamma = sum_b red_1, dbeta = sum_b red_0.
    Every fmaf of the source is one rounding; an a * b + c written without it is two (the compiler may contract it, which
    only removes a rounding).  rsqrtf and __expf / rcp are numpy's correctly rounded ones.
    mutate: one of GN_MUTATIONS (test_groupnorm_mutations_are_rejected)."""
    f = np.float32
    B, HW, C = x.shape
    cpg = C // G
    xf, ga, be = x.numpy().astype(f), gamma.numpy().astype(f), beta.numpy().astype(f)
    piv = xf[:, :1, :]
    d = xf - piv
    S, Q = _gn_slab_sums(d, d, d, tail=mutate != "no_tail")
    inv_hw = f(1) / f(HW)
    mc = piv[:, 0] + S * inv_hw
    m2c = np.maximum(Q - S * S * inv_hw, f(0))
    chain = lambda v: np.cumsum(v.reshape(B, G, cpg), axis=2, dtype=f)[:, :, -1]
    mean = chain(mc) / f(cpg)
    dc = (mc.reshape(B, G, cpg) - mean[:, :, None]).astype(f)
    spread = np.zeros((B, G), f)
    for j in range(cpg):
        spread = _fma32(dc[:, :, j], dc[:, :, j], spread)
    n = f(cpg) * f(HW)
    if mutate == "no_spread":
        var = chain(m2c) / n
    else:
        var = (chain(m2c) + f(HW) * spread) / (n - f(1) if mutate == "n_minus_1" else n)
    rstd = f(1) / np.sqrt(var + f(eps))
    if mutate == "image0_stats":
        mean, rstd = np.repeat(mean[:1], B, 0), np.repeat(rstd[:1], B, 0)
    gidx = np.arange(C) // cpg
    if mutate == "group_of_chunk":
        gidx = (np.arange(C) // 8 * 8) // cpg
    mu_c, rs_c = mean[:, gidx][:, None, :], rstd[:, gidx][:, None, :]
    sc = rs_c * ga
    sh = be - mu_c * sc
    y = torch.from_numpy(_silu32(_fma32(xf, sc, sh)).astype(np.float64))
    out = {"mr": torch.from_numpy(np.stack([mean, rstd], -1).astype(np.float64)), "y": r16(y)}
    if gy is None:
        return out
    gf = gy.numpy().astype(f)
    rbf = lambda h: torch.from_numpy(h).to(BF).float().numpy() if mutate == "silu_grad_bf16_h" else h
    xh = (xf - mu_c) * rs_c
    dh = gf * _silu_grad32(rbf(_fma32(xh, ga, be)))
    red0, red1 = _gn_slab_sums(dh, dh, xh)
    gsum = np.ones_like(ga) if mutate == "sums_no_gamma" else ga
    a1, a2 = np.zeros((B, G), f), np.zeros((B, G), f)
    for j in range(cpg):
        a1 = _fma32(gsum[j::cpg][None], red0[:, j::cpg], a1)
        a2 = _fma32(gsum[j::cpg][None], red1[:, j::cpg], a2)
    inv_n = f(1) / (f(HW) if mutate == "inv_hw_for_n" else n)
    m1c, m2g = (a1 * inv_n)[:, gidx][:, None, :], (a2 * inv_n)[:, gidx][:, None, :]
    cA = rs_c * ga
    cB = be - mu_c * cA
    cC = rs_c * rs_c * m2g
    if mutate == "sign_s2":
        cC = -cC
    cD = mu_c * cC - rs_c * m1c
    dh = gf * _silu_grad32(rbf(_fma32(xf, cA, cB)))
    dxf = _fma32(dh, cA, _fma32(-xf, cC, cD))
    if dres is None:
        dx = r16(torch.from_numpy(dxf))
    elif mutate == "dres_after":
        dx = r16(r16(torch.from_numpy(dxf)) + dres.to(F64))
    else:
        dx = r16(torch.from_numpy(dxf + dres.numpy().astype(f)))
    bsum = lambda v: torch.from_numpy((v[0] if mutate == "dgamma_first_image" else np.cumsum(v, axis=0, dtype=f)[-1]).astype(np.float64))
    out.update(dx=dx, dgamma=bsum(red1), dbeta=bsum(red0))
    return out


GN_HOST_SHAPES = [(2, 1030, 192, 32), (2, 513, 64, 32), (1, 3, 1536, 32), (2, 700, 32, 32)]


@functools.lru_cache(maxsize=None)
def gn_case(shape, k):
    """inputs at pivot offset k, gy, the fp64 references without and with dres: computed once, shared, never modified"""
    B, HW, C, G = shape
    x, gamma, beta = gn_pivot_inputs(B, HW, C, G, k, seed=HW + C) if k else gn_inputs(B, HW, C, G, seed=HW + C)
    gy = r16(torch.randn(B, HW, C, generator=torch.Generator().manual_seed(2), dtype=F64))
    y64, ysl, *_ = gn_silu64(x, gamma, beta, G)
    ref0 = gn_bwd64(x, gamma, beta, gy, None, G)
    dres = rownorm_dres(ref0[0].view(B * HW, C), seed=HW).view(B, HW, C)
    ref1 = gn_bwd64(x, gamma, beta, gy, dres, G)
    return x, gamma, beta, gy, dres, (y64, ysl), ref0, ref1


def gn_check_all(case, shape, out0, out1, what, bias=True):
    """every bound of row N on an emulation's (or a kernel's) outputs without (out0) and with dres (out1) -> ratios.
    bias = False: the rounding-bias check of check_one_rounding is reported, not asserted (a kernel at an outlier pivot: the
    error of rstd is one signed factor on every z - beta of a group, up to the slack, which that check reads as a bias of up
    to 1/16 ulp on the elements it samples)."""
    B, HW, C, G = shape
    x, gamma, beta, gy, dres, (y64, ysl), ref0, ref1 = case
    c = max(64.0, gn_k_g(HW, C, B))
    nb = 2000 if bias else 1 << 62
    res = {"mean,rstd": check_gn_stats(x, G, out0["mr"], what + " statistics"),
           "y": check_one_rounding(out0["y"], y64, ysl, what + " y", min_bias_n=nb),
           "dx": check_one_rounding(out0["dx"], ref0[0], ref0[1], what + " dx", min_bias_n=nb),
           "dx+dres": check_one_rounding(out1["dx"], ref1[0], ref1[1], what + " dx + dres", min_bias_n=nb),
           "dgamma": (check_fp32(out0["dgamma"], ref0[2], ref0[4], c, what + " dgamma"),),
           "dbeta": (check_fp32(out0["dbeta"], ref0[3], ref0[4], c, what + " dbeta"),)}
    return {k: tuple(round(v, 4) for v in t) for k, t in res.items()}


@pytest.mark.parametrize("k", [0, 8, 64])
@pytest.mark.parametrize("shape", GN_HOST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_ordered_emulation_sits_inside_every_bound(shape, k):
    """[N] the fp32 emulation in the kernels' order: mean / rstd, y, dx without and with dres, dgamma, dbeta, at pivot
    offsets of 0 / 8 / 64 group-sigma.  The bounds were never fitted to a kernel."""
    B, HW, C, G = shape
    case = gn_case(shape, k)
    x, gamma, beta, gy, dres = case[:5]
    out0 = gn_kernel_emul_ordered(x, gamma, beta, G, gy, None)
    out1 = gn_kernel_emul_ordered(x, gamma, beta, G, gy, dres)
    assert torch.equal(out0["y"], out1["y"]) and torch.equal(out0["mr"], out1["mr"])
    print(f"[error-budget-host] GroupNorm {shape} pivot +{k} sigma: {gn_check_all(case, shape, out0, out1, 'clean emulation')}")


def gn_spread_inputs(shape, seed=0):
    """gn_inputs at |mean| <= 3 std whose channels sit -2 .. 2 group-std apart inside a group: the between-channel term"""
    B, HW, C, G = shape
    g = torch.Generator().manual_seed(seed)
    cpg = C // G
    std = 10.0 ** (torch.rand(B, 1, G, 1, generator=g, dtype=F64) * 4 - 2)
    mean = std * (torch.rand(B, 1, G, 1, generator=g, dtype=F64) * 6 - 3 + torch.linspace(-2, 2, cpg, dtype=F64).view(1, 1, 1, cpg))
    x = mean + std * torch.randn(B, HW, G, cpg, generator=g, dtype=F64)
    _, gamma, beta = gn_inputs(1, 1, C, G, seed)
    return r16(x.view(B, HW, C)), gamma, beta


# mutation -> (host shape, the check that must reject it)
GN_MUTATION_CASES = {
    "no_spread": ((2, 513, 64, 32), "statistics"),
    "n_minus_1": ((1, 3, 1536, 32), "statistics"),
    "group_of_chunk": ((2, 1030, 192, 32), "y"),
    "image0_stats": ((2, 513, 64, 32), "statistics"),
    "no_tail": ((2, 513, 64, 32), "statistics"),
    "dres_after": ((1, 3, 1536, 32), "dx + dres"),
    "sums_no_gamma": ((2, 513, 64, 32), "dx"),
    "inv_hw_for_n": ((2, 513, 64, 32), "dx"),
    "silu_grad_bf16_h": ((2, 513, 64, 32), "dx"),
    "dgamma_first_image": ((2, 513, 64, 32), "dgamma"),
    "sign_s2": ((2, 513, 64, 32), "dx"),
}


@pytest.mark.parametrize("mutation", GN_MUTATIONS)
def test_groupnorm_mutations_are_rejected(mutation):
    """[N] each defect of GN_MUTATIONS in the ordered emulation is rejected by the bound named in GN_MUTATION_CASES, at the
    smallest host shape that can show it, while the clean emulation passes on the same inputs.  no_spread runs on
    gn_spread_inputs (in gn_inputs the channels of a group share their mean and the term is noise).  All eleven are
    rejected: none of them is invisible in the outputs."""
    shape, which = GN_MUTATION_CASES[mutation]
    B, HW, C, G = shape
    if mutation == "no_spread":
        x, gamma, beta = gn_spread_inputs(shape, seed=3)
        check_gn_stats(x, G, gn_kernel_emul_ordered(x, gamma, beta, G)["mr"], "clean emulation, spread inputs")
        with pytest.raises(AssertionError, match="rstd"):
            check_gn_stats(x, G, gn_kernel_emul_ordered(x, gamma, beta, G, mutate=mutation)["mr"], mutation)
        return
    case = gn_case(shape, 0)
    x, gamma, beta, gy, dres = case[:5]
    bad0 = gn_kernel_emul_ordered(x, gamma, beta, G, gy, None, mutate=mutation)
    bad1 = gn_kernel_emul_ordered(x, gamma, beta, G, gy, dres, mutate=mutation)
    with pytest.raises(AssertionError, match=re.escape(f"{mutation} {which}")):
        gn_check_all(case, shape, bad0, bad1, mutation)


def test_groupnorm_one_pass_variance_is_rejected():
    """mutation 11: one-pass E[x^2] - E[x]^2 in fp32 at |mean| / std = 100"""
    B, HW, C, G = 2, 1024, 64, 8
    x, gamma, beta = gn_inputs(B, HW, C, G, seed=10)
    xg = x.view(B, HW, G, C // G)
    m = xg.mean((1, 3), keepdim=True)
    s = xg.std((1, 3), keepdim=True)
    x = r16((m + (xg - m) / s * (m.abs() / 100)).view(B, HW, C))      # every group at |mean| / std = 100
    y64, slack, *_ = gn_silu64(x, gamma, beta, G)
    check_one_rounding(gn_kernel_emul(x, gamma, beta, G), y64, slack, "clean GroupNorm + SiLU")
    with pytest.raises(AssertionError):
        check_one_rounding(gn_kernel_emul(x, gamma, beta, G, one_pass=True), y64, slack, "one-pass variance")


# ---------------------------------------------------------------------------------------------------------------------------
# [N] row norms: rms_hat (mode 0) and rms_ln_hat (mode 1), forward and backward with the fused residual gradient
# ---------------------------------------------------------------------------------------------------------------------------
def rms_ln_inputs(T, C, seed=0):
    """x [T, C] bf16 values, w [C] fp32 values, gy [T, C] bf16 values.  Per-row scales 2^-6 .. 2^6; a per-row common offset
    (along 1 / w, so that it survives the weight) that puts |mean u| / std u around 0 (rows 0 mod 3), 4-8 (1 mod 3) and
    32-100 (2 mod 3): the LayerNorm's cancellation.  Row 1 is all zero and row 2 constant."""
    g = torch.Generator().manual_seed(seed)
    w = f32(1 + 0.1 * torch.randn(C, generator=g, dtype=F64))
    rs = torch.exp2(torch.randint(-6, 7, (T, 1), generator=g).to(F64))
    u01 = torch.rand(T, 1, generator=g, dtype=F64)
    kind = (torch.arange(T) % 3)[:, None]
    off = torch.where(kind == 0, torch.zeros_like(u01), torch.where(kind == 1, 4 + 4 * u01, 32 * (100 / 32) ** u01))
    off = off * torch.where(torch.rand(T, 1, generator=g) < 0.5, -1.0, 1.0)
    x = (torch.randn(T, C, generator=g, dtype=F64) + off / w) * rs
    x[1] = 0
    x[2] = rs[2] * 3
    gy = r16(torch.randn(T, C, generator=g, dtype=F64))
    return r16(x), w, gy


def rownorm_dres(dx64, seed=0):
    """the fused residual gradient of the tests: on even rows of the magnitude of dx and partly cancelling it, on odd rows
    unrelated unit noise"""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(dx64.shape, generator=g, dtype=F64)
    even = (torch.arange(dx64.shape[0]) % 2 == 0)[:, None]
    return r16(torch.where(even, dx64 * (0.5 * n - 1), n))


def rownorm_fwd_emul(x, w, mode, mutate=None):
    """fp32 in the kernel's order of operations (norm.hip:345-376): ss = sum x^2, r = rsqrt(ss / C + eps); mode 1:
    u = (x r) w, mu = sum u / C, s = rsqrt(sum (u - mu)^2 / C + eps), y = bf16((u - mu) s); mode 0: y = bf16(x r).
    mutate 'u_bf16': u rounded to bf16 between the two norms."""
    xf = x.float()
    inv_c = torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    r = torch.rsqrt((xf * xf).sum(1, keepdim=True) * inv_c + EPS_RMS)
    if mode == 0:
        return r16(xf * r)
    u = xf * r * w.float()
    if mutate == "u_bf16":
        u = u.to(BF).float()
    mu = u.sum(1, keepdim=True) * inv_c
    d = u - mu
    s = torch.rsqrt((d * d).sum(1, keepdim=True) * inv_c + EPS_LN)
    return r16(d * s)


def rownorm_bwd_emul(x, w, gy, dres, mode, mutate=None, reorder=False):
    """fp32 in the kernel's order of operations (norm.hip:405-481) -> (dx, dw | None).  xhat = x r; mode 1: u = xhat w, mu, s
    as in the forward, y = (u - mu) s, du = s (g - mean g - y mean(g y)), dw += du xhat, g := du w; then
    dx = bf16(r (g - xhat mean(g xhat)) + dres).  The row sum of dw is in no fixed order in the kernel (per-lane chains over a
    block's rows, LDS atomics over its waves, global atomics over the blocks): `reorder` sums 37 interleaved row classes as
    sequential fp32 chains and adds them last to first, instead of torch's one fp32 sum.
    mutate 'dres_after': dres added after the rounding of dx (a second rounding); 'dw_drop_row': one row missing from dw."""
    xf, g = x.float(), gy.float()
    inv_c = torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    sum_ = lambda t: t.sum(1, keepdim=True)
    r = torch.rsqrt(sum_(xf * xf) * inv_c + EPS_RMS)
    xh = xf * r
    dw = None
    if mode == 1:
        wf = w.float()
        mu = sum_(xh * wf) * inv_c
        d = xh * wf - mu
        s = torch.rsqrt(sum_(d * d) * inv_c + EPS_LN)
        yv = d * s
        a1, a2 = sum_(g) * inv_c, sum_(g * yv) * inv_c
        du = s * (g - a1 - yv * a2)
        c = du * xh
        if mutate == "dw_drop_row":
            c = torch.cat([c[:5], c[6:]])
        if reorder:
            parts = [torch.from_numpy(np.cumsum(c[i::37].numpy(), axis=0, dtype=np.float32)[-1]) for i in range(min(37, c.shape[0]))]
            dw = torch.zeros_like(parts[0])
            for p in reversed(parts):
                dw = dw + p
        else:
            dw = c.sum(0)
        g = du * wf
    a3 = sum_(g * xh) * inv_c
    dx = r * (g - xh * a3)
    if dres is None:
        return r16(dx), dw
    if mutate == "dres_after":
        return r16(r16(dx) + dres.to(F64)), dw
    return r16(dx + dres.float()), dw


ROWNORM_C_DW = 64.0     # [N] fp32 dw by atomics: the constant of dgamma / dbeta
ROWNORM_HOST_SHAPES = [(520, 384), (300, 1536), (64, 2048)]


def test_rms_ln_inputs_reach_the_cancellation_classes():
    """the input design does what its docstring says: |mean u| / std u below 0.5, in 3-10 and in 25-130 on the three row
    classes (rows 1 and 2, the zero and the constant row, aside)"""
    x, w, _ = rms_ln_inputs(300, 384, seed=1)
    _, u, mu, s, _ = rms_ln_hat64(x, w)
    ratio = (mu.abs() * s)[3:, 0]
    kind = torch.arange(3, 300) % 3
    assert ratio[kind == 0].max() < 0.5
    assert 3 < ratio[kind == 1].min() and ratio[kind == 1].max() < 10
    assert 25 < ratio[kind == 2].min() and ratio[kind == 2].max() < 130
    assert float(x[1].abs().max()) == 0 and float(x[2].min()) == float(x[2].max()) != 0


@pytest.mark.parametrize("T,C", ROWNORM_HOST_SHAPES)
def test_rms_ln_hat_forward_clean_passes_and_bf16_u_is_rejected(T, C):
    """[N] mode 1 forward.  Measured here: the clean fp32 emulation at ratio 0.500-0.501 of the bound, rounding bias within
    +-0.002 ulp; u rounded to bf16 between the two norms lands at 10^3 x the bound (rows at |mean u| / std u of 32-100)."""
    x, w, _ = rms_ln_inputs(T, C, seed=T + C)
    y64, u, mu, s, _ = rms_ln_hat64(x, w)
    slack = rms_ln_slack(y64, u, mu, s)
    y = rownorm_fwd_emul(x, w, 1)
    assert bool(torch.isfinite(y).all())
    rep = check_one_rounding(y, y64, slack, "clean rms_ln_hat")
    print(f"[error-budget-host] rms_ln_hat {T}x{C} clean (ratio, ulps, bias): {tuple(round(v, 4) for v in rep)}")
    with pytest.raises(AssertionError):
        check_one_rounding(rownorm_fwd_emul(x, w, 1, mutate="u_bf16"), y64, slack, "u rounded to bf16")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T,C", ROWNORM_HOST_SHAPES)
def test_rownorm_backward_clean_passes_and_defects_are_rejected(T, C, mode):
    """[N] backward of both modes, with and without dres; dw (mode 1) in two summation orders and on top of a running sum.
    Measured here for the clean fp32 emulation (never the kernel): dx at ratio 0.500-0.52 of its bound in both modes with and
    without dres; dw at most 0.02 of its bound in either order.  Rejected: dres added after the rounding of dx; dw without
    one row's contribution."""
    x, w, gy = rms_ln_inputs(T, C, seed=T + C + mode)
    dx0, _, _, _ = rownorm_bwd64(x, w, gy, None, mode)
    dres = rownorm_dres(dx0, seed=T)
    for dr in (None, dres):
        dx64, slack, dw64, dw_terms = rownorm_bwd64(x, w, gy, dr, mode)
        dx, dw = rownorm_bwd_emul(x, w, gy, dr, mode)
        assert bool(torch.isfinite(dx).all())
        rep = check_one_rounding(dx, dx64, slack, f"clean rownorm dx mode {mode}")
        print(f"[error-budget-host] rownorm bwd {T}x{C} mode {mode} dres={dr is not None} dx (ratio, ulps, bias): "
              f"{tuple(round(v, 4) for v in rep)}")
    with pytest.raises(AssertionError):
        check_one_rounding(rownorm_bwd_emul(x, w, gy, dres, mode, mutate="dres_after")[0], dx64, slack, "dres after the rounding")
    if mode == 1:
        _, dw2 = rownorm_bwd_emul(x, w, gy, dres, mode, reorder=True)
        r1 = check_fp32(dw, dw64, dw_terms, ROWNORM_C_DW, "clean dw")
        r2 = check_fp32(dw2, dw64, dw_terms, ROWNORM_C_DW, "clean dw, reordered")
        base = f32(torch.randn(C, generator=torch.Generator().manual_seed(5), dtype=F64) * dw64.abs().mean())
        r3 = check_fp32(f32(base + dw2.to(F64)), base + dw64, dw_terms + base.abs(), ROWNORM_C_DW, "clean dw on a running sum")
        print(f"[error-budget-host] rownorm dw {T}x{C} ratios: {r1:.4f} {r2:.4f} {r3:.4f}")
        _, bad = rownorm_bwd_emul(x, w, gy, dres, mode, mutate="dw_drop_row")
        with pytest.raises(AssertionError):
            check_fp32(bad, dw64, dw_terms, ROWNORM_C_DW, "dw missing a row")


# ---------------------------------------------------------------------------------------------------------------------------
# [G] RoPE in the epilogue of the QKV projection
# ---------------------------------------------------------------------------------------------------------------------------
def rope_table(N, seed):
    """[N, 4, 32] fp32 values with four independent planes (cos / sin of two unrelated angles): the reference's rotation is
    not orthogonal, so nothing may rely on c2 = c1, s2 = s1"""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(N, 32, generator=g) * 6.28
    return torch.stack([torch.cos(ang), torch.sin(ang), torch.cos(ang * 0.5), torch.sin(ang * 0.5)], 1).contiguous()


def rope_kernel_emul(x, w, b, tab, tokens, rope_cols, mutate=None, reverse=False):
    """fp32 accumulation, + bias, the rotation in fp32 (each product and the sum rounded), one rounding.  Mutations:
    'after_rounding' (z rounded to bf16, rotated, rounded again), 'plane1' (s2, c2 taken from s1, c1), 'row_m' (table row m
    instead of m % tokens: `tab` then holds a row for every m), 'v_rot32' (the first 32 columns of the v third rotated too)."""
    xs, ws = (x.flip(1), w.flip(1)) if reverse else (x, w)
    z = f32((xs.float() @ ws.float().t()).to(F64) + b)
    M = z.shape[0]
    rows = torch.arange(M) if mutate == "row_m" else torch.arange(M) % tokens
    t = tab.to(F64)
    if mutate == "plane1":
        t = torch.stack([t[:, 0], t[:, 1], t[:, 0], t[:, 1]], 1)
    if mutate == "after_rounding":
        z = r16(z)
    y = z.clone()
    y[:, :rope_cols] = rope_pairs(z[:, :rope_cols], t, rows, fp32=True)
    if mutate == "v_rot32":
        full = rope_pairs(z[:, rope_cols:rope_cols + 64], t, rows, fp32=True)
        y[:, rope_cols:rope_cols + 32] = full[:, :32]
    return r16(y)


@pytest.fixture(scope="module")
def rope_case():
    """300 x 192 x 384 (two heads each of q, k and v; columns 0..255 rotated), 60 tokens per image: five images"""
    M, K, N, tokens, cols = 300, 192, 384, 60, 256
    x, w, b, _ = gemm_inputs(M, K, N, seed=21)
    tab_m = rope_table(M, 4).to(F64)            # a row for every m; the clean table is its first `tokens` rows
    acc, absdot = conv64(x, w, "linear")
    y64, slack = rope_epilogue64(acc, absdot, b, tab_m[:tokens], tokens, cols)
    return x, w, b, tab_m, tokens, cols, y64, slack


def test_rope_epilogue_clean_emulation_passes_in_both_summation_orders(rope_case):
    """Measured here: ratio 0.500, rounding bias within +-0.002 ulp; the v third equals the plain projection's reference"""
    x, w, b, tab_m, tokens, cols, y64, slack = rope_case
    acc, absdot = conv64(x, w, "linear")
    plain, _, _ = epilogue64(acc, absdot, b)
    assert torch.equal(plain[:, cols:], y64[:, cols:]) and not torch.equal(plain[:, :cols], y64[:, :cols])
    for rev in (False, True):
        rep = check_one_rounding(rope_kernel_emul(x, w, b, tab_m[:tokens], tokens, cols, reverse=rev), y64, slack, f"clean rope reverse={rev}")
        print(f"[error-budget-host] rope epilogue clean reverse={rev} (ratio, ulps, bias): {tuple(round(v, 4) for v in rep)}")


@pytest.mark.parametrize("mutation", ["after_rounding", "plane1", "row_m", "v_rot32"])
def test_rope_epilogue_mutations_are_rejected(rope_case, mutation):
    """rotation after the rounding; s2 / c2 taken from s1 / c1; table row m instead of m % tokens (wrong from the second image
    on); rotation applied to the first 32 columns of the v third"""
    x, w, b, tab_m, tokens, cols, y64, slack = rope_case
    tab = tab_m if mutation == "row_m" else tab_m[:tokens]
    y = rope_kernel_emul(x, w, b, tab, tokens, cols, mutate=mutation)
    if mutation == "row_m":       # the first image is right: the defect is only visible behind an image boundary
        check_one_rounding(y[:tokens], y64[:tokens], slack[:tokens], "first image", min_bias_n=10 ** 9)
    with pytest.raises(AssertionError):
        check_one_rounding(y, y64, slack, mutation)


# ---------------------------------------------------------------------------------------------------------------------------
# [A] attention backward with the RoPE adjoint in its stores
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_rope_case():
    N = 256
    q, k, v = attn_inputs(N, seed=8, v_offset=4.0)
    g = torch.Generator().manual_seed(9)
    do = r16(torch.randn(N, 64, generator=g, dtype=F64))
    tab = rope_table(N, 6).to(F64)
    o, lse = attn_fwd_emul(q, k, v, 0.125)
    ex = attn_bwd_exact(q, k, v, o, do, lse, 0.125, tab=tab)
    clean = attn_bwd_emul(q, k, v, o, do, lse, 0.125, tab=tab)
    return (q, k, v, o, do, lse, tab), ex, clean


def test_attention_backward_rope_adjoint_reference_is_the_adjoint(attn_rope_case):
    """<R x, g> == <x, R^T g> in fp64 for rope_pairs; without a table the extended functions return what they did; dv does
    not depend on the table"""
    (q, k, v, o, do, lse, tab), ex, clean = attn_rope_case
    g = torch.Generator().manual_seed(2)
    xx, gg = torch.randn(256, 128, generator=g, dtype=F64), torch.randn(256, 128, generator=g, dtype=F64)
    rows = torch.arange(256)
    lhs = (rope_pairs(xx, tab, rows) * gg).sum()
    rhs = (xx * rope_pairs(gg, tab, rows, "adjoint")).sum()
    assert abs(lhs - rhs) <= 1e-12 * (xx.abs() * gg.abs()).sum()
    ex0 = attn_bwd_exact(q, k, v, o, do, lse, 0.125)
    em0 = attn_bwd_emul(q, k, v, o, do, lse, 0.125)
    assert torch.equal(ex0[2], ex[2]) and torch.equal(em0[2], clean[2])
    assert torch.equal(rope_pairs(ex0[0], tab, rows, "adjoint"), ex[0])
    for i, nm in enumerate(("dq", "dk", "dv")):
        check_vs_emulation(clean[i], clean[i], ex[i], nm)


@pytest.mark.parametrize("mutation", ["rope_fwd", "rope_row32"])
def test_attention_backward_rope_adjoint_mutations_are_rejected(attn_rope_case, mutation):
    """the forward rotation in place of the adjoint; the table row of token + 32 (a tile-local index): relL2 400-540 x the
    emulation's.  Not rejected, and so not listed: the adjoint applied after the rounding of dq / dk and rounded again
    (mutate 'rope_after').  It adds a second rounding of the same size; measured on three slices (N = 256 with and without
    the offset on v, N = 300) its relL2 is 1.16-1.23 x the emulation's and its max error 0.25-0.42 of that rule, which
    straddles TAU = 1.2.  TAU is calibrated by test_tau_calibration_from_two_orderings and stays; what holds the adjoint
    store to a single rounding is the element-by-element one-rounding contract of rows G / D, which row A does not have."""
    args, ex, clean = attn_rope_case
    bad = attn_bwd_emul(*args[:6], 0.125, mutate=mutation, tab=args[6])
    for i, nm in ((0, "dq"), (1, "dk")):
        with pytest.raises(AssertionError):
            check_vs_emulation(bad[i], clean[i], ex[i], f"{nm} {mutation}")
