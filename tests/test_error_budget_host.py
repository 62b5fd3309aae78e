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
"""
import math

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


def attn_bwd_exact(q, k, v, o, do, lse, scale):
    """fp64 backward of the forward the kernel saved (its bf16 o and fp32 lse): delta = sum(do o), P = exp(s - lse),
    dS = P (do v^T - delta), dq = scale dS k, dk = scale dS^T q, dv = P^T do"""
    q, k, v, o, do, lse = (t.to(F64) for t in (q, k, v, o, do, lse))
    delta = (do * o).sum(1)
    p = torch.exp(q @ k.t() * scale - lse[:, None])
    ds = p * (do @ v.t() - delta[:, None])
    return scale * ds @ k, scale * ds.t() @ q, p.t() @ do, delta


def split3(x):
    """fp32 x as three bf16 pieces hi + mid + lo (attention.hip:867-877)"""
    d0 = r16(x)
    r1 = f32(x - d0)
    d1 = r16(r1)
    d2 = r16(f32(r1 - d1))
    return d0, d1, d2


def attn_bwd_emul(q, k, v, o, do, lse, scale, mutate=None):
    """[A] the backward kernels' documented policy: delta = fp32 sum of do o; P = exp2(s c2 - lse log2e) in fp32;
    dP - delta accumulated in fp32 from -delta as three bf16 pieces; dS = P (dP - delta) rounded to bf16 for dq and dk,
    P rounded to bf16 for dv; fp32 sums; scale applied to the fp32 sum; one rounding of each output.
    mutate 'delta1': -delta enters as one bf16 piece."""
    q, k, v, o, do = (t.to(F64) for t in (q, k, v, o, do))
    c2 = float(np.float32(scale * LOG2E))
    delta = f32((do * o).sum(1))
    nl = f32(-f32(lse.to(F64)) * LOG2E)
    s = f32(q @ k.t())
    p = f32(torch.exp2(f32(s * c2 + nl[:, None])))
    nd = sum(split3(-delta)) if mutate != "delta1" else r16(-delta)
    dpm = f32(do @ v.t() + nd[:, None])
    ds = r16(f32(p * dpm))
    dq = r16(f32(f32(ds @ k) * scale))
    dk = r16(f32(f32(ds.t() @ q) * scale))
    dv = r16(f32(r16(p).t() @ do))
    return dq, dk, dv, delta


# ---------------------------------------------------------------------------------------------------------------------------
# norms in fp64
# ---------------------------------------------------------------------------------------------------------------------------
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
    return act64(z, "silu"), slack, z, xh, rstd.view(B, G)


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
