"""Train-step glue under the rounding contract, host side: the fp64 references and per-element
bounds of `csrc/optim.hip`, `csrc/loss.hip` and `csrc/fold.hip`, float32 emulations of each kernel's documented arithmetic
(contracted to fma or not, sums in two orders), and mutation tests showing on the CPU that the bounds reject specific defects.
tests/test_glue_gpu.py imports the references and the bounds from here.

u = 2^-24 is the unit roundoff of fp32 round-to-nearest.  Every bound below is a count of the fp32 roundings on the way to the
output, each weighted by the magnitude of the value that was rounded; a contracted (fma) evaluation has fewer roundings and
is inside the same bound.  TINY = 2^-149 (the fp32 subnormal spacing) covers results that underflow.

[O] tv_opt_grad_norm + tv_opt_adamw, one step from fp32 (p, g, m, v), step t (adamw_ref64):
      g' = g coef                                       coef == 1: exact.  Clipping: coef carries COEF_C u (the norm NORM_C, the
                                                        add of 1e-6 and the division), the product 1 more: eg = (COEF_C + 1) u |g'|
      m' = m + (g' - m)(1 - beta1)                      |dm'| <= u (3 (1 - beta1) |g' - m| + |m'|) + (1 - beta1) eg
                                                        (the difference, 1 - beta1, the product; the sum)
      v' = beta2 v + (1 - beta2) g' g'                  |dv'| <= u (2 beta2 v + 4 (1 - beta2) g'^2) + 2 (1 - beta2) |g'| eg
                                                        (the product and the sum; 1 - beta2, two products and the sum)
      denom = sqrt(v') bc2s_inv + eps                   |d denom| <= sqrt(v') bc2s_inv (dv' / 2 v' + 3 u) + u denom
      U  = step_size m' / denom                         |dU| <= |U| (d denom / denom + 3 u) + step_size |dm'| / denom
      p' = (p - lr wd p) - U                            |dp'| <= u (2 lr wd |p| + |p - lr wd p| + |p'|) + |dU|
    i.e. the constants 3 / 1 (m'), 2 / 4 (v'), 3 over |p| and 10 over |U| (p') plus the propagated bound of m'.
    The norm: per thread an fma chain of 256 squares, a wave butterfly and 4 wave sums in fp32, the chunks in fp64, one
    rounding of the root: worst case (256 / 2 + 10) / 2 + 1 = 70 u relative (a chain of positive terms loses at most half its
    length), statistically sqrt(256 / 3) / 4 = 2.3 u; NORM_C = 16 is the project's constant for an fp32 sum (rows W, A).
[K] tv_pack_weight_multi / tv_opt_cast_shadows: bit-equal to permute (+ tap flip) / to `.to(bfloat16)`.
[L] tv_vae_loss_l1_kl: values 1e-6 relative of fp64 (row X); d_recon exactly +-l1_scale / 0 without the sigmoid, with it
    c = 16 over the true l1_scale s (1 - s) (row Q); d_mu one product; d_logvar with the project's figure for the
    exponential, 2^-20 (1 + |lv|) relative on e, carried as an absolute slack on 1 - e, plus two roundings.
[Z] tv_fold_cols / _bwd: Wf the IEEE product; bf c = 16 over sum|W beta| (at most 2 x 5 roundings per lane up to C = 384 and 6
    butterfly levels); dW two roundings; dgamma, dbeta k(R) = 8 + 16 + ceil(R / 64) (a thread's chain of 4 products and adds,
    16 row lanes, the row chunks).
"""
import math

import numpy as np
import pytest
import torch

from test_error_budget_host import F64, check_fp32

U = 2.0 ** -24
TINY = 2.0 ** -149
F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------------
# [O] optimizer
# ---------------------------------------------------------------------------------------------------------------------------
OPT_CHUNK = 65536
OPT_SIZES = [1, 3, 5, 255, 65535, 65536, 65537, 2 * 65536 + 3]
OPT_SCALES = [-20, -15, -10, -6, -2, 2, 6, 10]        # per-tensor gradient scale 2^k
NORM_C = 16.0
COEF_C = NORM_C + 2.0
VALUE_RTOL = 1e-6


def opt_hyper(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05):
    """the hyper-parameters as the fp32 values the C ABI receives"""
    return {k: float(F32(v)) for k, v in dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd).items()}


def opt_bias_corrections(hp, t):
    """ctrl[5], ctrl[6]: 1 - beta1^t and sqrt(1 - beta2^t) in fp64, rounded to fp32 (opt_ctrl_kernel)"""
    return float(F32(1.0 - hp["beta1"] ** float(t))), float(F32(math.sqrt(1.0 - hp["beta2"] ** float(t))))


def opt_inputs(seed=0, sizes=OPT_SIZES, scales=OPT_SCALES, zero_grad=False):
    """per tensor (p, g, m, v) as float32 arrays: g ~ 2^k randn, m of g's scale, v of its square, p over 2^-8 .. 2^2 so that
    the update matches p in some elements and dominates it in others.  Element 0: g = m = v = 0; element 1: v subnormal;
    element 2: m = -g."""
    rng = np.random.default_rng(seed)
    out = []
    for n, k in zip(sizes, scales):
        s = 2.0 ** k
        p = (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 3, n)).astype(F32)
        g = (rng.standard_normal(n) * s).astype(F32)
        m = (rng.standard_normal(n) * s * 0.5).astype(F32)
        v = ((rng.standard_normal(n) * s) ** 2 * rng.uniform(0.1, 2.0, n)).astype(F32)
        g[0] = m[0] = v[0] = 0
        if n > 1:
            v[1] = F32(1e-40)
        if n > 2:
            m[2] = -g[2]
        if zero_grad:
            g[:] = 0
        out.append((p, g, m, v))
    return out


def opt_norm64(tensors):
    return math.sqrt(sum(float((t[1].astype(np.float64) ** 2).sum()) for t in tensors))


def opt_coef64(norm64, max_norm):
    """(clip coefficient from the fp64 norm, whether its rounding error enters the bounds)"""
    if not max_norm or max_norm <= 0:
        return 1.0, False
    q = float(F32(max_norm)) / (norm64 + float(F32(1e-6)))
    return min(1.0, q), q < 2.0


def adamw_ref64(p, g, m, v, coef, clip, hp, t):
    """-> dict of fp64 m', v', p' and their per-element bounds bm, bv, bp (module docstring, row O)"""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"]
    bc1, bc2s = opt_bias_corrections(hp, t)
    ss, inv = lr / bc1, 1.0 / bc2s
    g1 = g * coef
    eg = (COEF_C + 1.0) * U * np.abs(g1) if clip else 0.0
    d = g1 - m
    m2 = m + d * (1.0 - b1)
    bm = U * (3.0 * (1.0 - b1) * np.abs(d) + np.abs(m2)) + (1.0 - b1) * eg + TINY
    v2 = b2 * v + (1.0 - b2) * g1 * g1
    bv = U * (2.0 * b2 * v + 4.0 * (1.0 - b2) * g1 * g1) + 2.0 * (1.0 - b2) * np.abs(g1) * eg + TINY
    root = np.sqrt(v2)
    denom = root * inv + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        droot = np.where(v2 > 0, bv / (2.0 * root), 0.0)
    bden = inv * (droot + 3.0 * U * root) + U * denom
    upd = ss * m2 / denom
    bu = np.abs(upd) * (bden / denom + 3.0 * U) + ss * bm / denom
    p1 = p - lr * wd * p
    p2 = p1 - upd
    bp = U * (2.0 * lr * wd * np.abs(p) + np.abs(p1) + np.abs(p2)) + bu + TINY
    return dict(m=m2, v=v2, p=p2, bm=bm, bv=bv, bp=bp, upd=upd)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def adamw_emul32(p, g, m, v, coef, hp, t, fma=False, mutate=None):
    """adamw_elem (optim.hip) in float32, uncontracted or with every a * b + c contracted.  Mutations: 'wd_after' (weight decay
    applied to the updated parameter), 't_minus_1' (bias corrections of step t - 1), 'eps_in_sqrt', 'clip_m_only' (v sees the
    unclipped gradient), 'bc2_no_sqrt' (1 - beta2^t without its root)."""
    one = F32(1)
    lr, b1, b2, eps, wd = (F32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    bc1, bc2s = opt_bias_corrections(hp, t - 1 if mutate == "t_minus_1" else t)
    if mutate == "bc2_no_sqrt":
        bc2s = float(F32(bc2s * bc2s))
    ss, inv = lr / F32(bc1), one / F32(bc2s)
    coef = F32(coef)
    g1 = g * coef
    gv = g if mutate == "clip_m_only" else g1
    lw = lr * wd
    if fma:
        p1 = p if mutate == "wd_after" else _fma32(-lw, p, p)
        m2 = _fma32(g1 - m, one - b1, m)
        v2 = _fma32((one - b2) * gv, gv, b2 * v)
        den = np.sqrt(v2 * inv * inv + eps) if mutate == "eps_in_sqrt" else _fma32(np.sqrt(v2), inv, eps)
        p2 = _fma32(-ss, m2 / den, p1)
        if mutate == "wd_after":
            p2 = _fma32(-lw, p2, p2)
    else:
        p1 = p if mutate == "wd_after" else p - lw * p
        m2 = m + (g1 - m) * (one - b1)
        v2 = b2 * v + (one - b2) * gv * gv
        den = np.sqrt(v2 * inv * inv + eps) if mutate == "eps_in_sqrt" else np.sqrt(v2) * inv + eps
        p2 = p1 - ss * (m2 / den)
        if mutate == "wd_after":
            p2 = p2 - lw * p2
    return m2.astype(F32), v2.astype(F32), p2.astype(F32)


def norm_emul32(tensors, vector=True):
    """opt_sqnorm_kernel + opt_ctrl_kernel: per chunk of 65 536, thread j's fma chain (vector: float4 j, j + 256, ...; scalar:
    element j, j + 256, ...), the 256 threads in fp32, the chunks in fp64, the root rounded to fp32"""
    tot = 0.0
    for _, g, _, _ in tensors:
        for s in range(0, g.size, OPT_CHUNK):
            c = np.zeros(OPT_CHUNK, F32)
            c[:min(OPT_CHUNK, g.size - s)] = g[s:s + OPT_CHUNK]
            steps = c.reshape(64, 256, 4).transpose(0, 2, 1).reshape(256, 256) if vector else c.reshape(256, 256)
            acc = np.zeros(256, F32)
            for row in steps:
                acc = _fma32(row, row, acc)
            tot += float(acc.reshape(4, 64).sum(1, dtype=F32).sum(dtype=F32)) if vector else float(np.cumsum(acc, dtype=F32)[-1])
    return float(F32(math.sqrt(tot)))


def coef_emul32(norm32, max_norm):
    if not max_norm or max_norm <= 0:
        return F32(1)
    return min(F32(1), F32(max_norm) / (F32(norm32) + F32(1e-6)))


def check_bound(y, y64, bound, what):
    """|y - y64| <= bound element by element, nothing masked; returns the worst ratio"""
    y, y64, bound = np.asarray(y, np.float64), np.asarray(y64, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(y).all(), f"{what}: non-finite output"
    r = np.abs(y - y64) / bound
    i = int(np.argmax(r))
    assert r.flat[i] <= 1.0, f"{what}: |y - y64| = {r.flat[i]:.4g} x its bound at flat index {i}: y={y.flat[i]:.9g} y64={y64.flat[i]:.9g}"
    return float(r.flat[i])


def check_adamw(got, ref, what):
    """got = (m', v', p') fp32 arrays -> worst ratios (m, v, p)"""
    return tuple(check_bound(got[i], ref[k], ref["b" + k], f"{what} {k}'") for i, k in enumerate(("m", "v", "p")))


def check_norm(norm, norm64, what):
    r = abs(float(norm) - norm64) / (NORM_C * U * norm64 + TINY)
    assert math.isfinite(float(norm)) and r <= 1.0, f"{what}: norm {float(norm)!r} vs {norm64!r}: {r:.3g} x the bound"
    return r


def err_stats(y, y64):
    """(max error in fp32 ulps of y64, mean signed error in ulps): the report's figures"""
    y, y64 = np.asarray(y, np.float64).ravel(), np.asarray(y64, np.float64).ravel()
    ulp = np.spacing(np.maximum(np.abs(y64), 2.0 ** -126).astype(F32)).astype(np.float64)
    e = (y - y64) / ulp
    return float(np.abs(e).max()), float((np.sign(y64) * e).mean())


OPT_CASES = [          # (lr, beta2, wd, t, clip) -- clip: None, 'far' (coefficient exactly 1), 'below', 'zero' (all-zero gradients)
    (3e-3, 0.999, 0.05, 1, None), (3e-3, 0.999, 0.0, 2, "below"), (3e-3, 0.95, 0.05, 10, "far"), (3e-3, 0.95, 0.0, 1000, "below"),
    (3e-3, 0.999, 0.05, 100000, "below"), (0.0, 0.999, 0.05, 10, "below"), (0.0, 0.95, 0.0, 1, None), (3e-3, 0.999, 0.05, 2, "zero"),
    (3e-3, 0.95, 0.05, 100000, None), (3e-3, 0.999, 0.0, 1000, "far"),
]


def opt_case(case, seed=0):
    """-> (tensors, hp, t, max_norm | None, norm64, coef64, clip)"""
    lr, b2, wd, t, clip = case
    tensors = opt_inputs(seed, zero_grad=clip == "zero")
    hp = opt_hyper(lr=lr, beta2=b2, wd=wd)
    n64 = opt_norm64(tensors)
    max_norm = {None: None, "far": 2.0 ** 40, "below": n64 / 3.7, "zero": 1.0}[clip]
    coef, active = opt_coef64(n64, max_norm)
    return tensors, hp, t, max_norm, n64, coef, active


@pytest.mark.parametrize("case", OPT_CASES, ids=str)
def test_adamw_clean_emulation_is_inside_the_bounds(case):
    """both emulations (contracted or not), with the clip coefficient from either emulated norm, pass rows O's bounds"""
    tensors, hp, t, max_norm, n64, coef, active = opt_case(case)
    for vector in (True, False):
        n32 = norm_emul32(tensors, vector)
        check_norm(n32, n64, f"norm emulation vector={vector}")
        c32 = coef_emul32(n32, max_norm)
        if case[4] in ("far", "zero", None):
            assert c32 == 1.0 and coef == 1.0
        for fma in (False, True):
            for p, g, m, v in tensors:
                check_adamw(adamw_emul32(p, g, m, v, c32, hp, t, fma=fma), adamw_ref64(p, g, m, v, coef, active, hp, t),
                            f"emulation fma={fma} n={p.size}")


def test_adamw_zero_element_is_exact():
    """g = m = v = 0: the update is exactly 0 apart from the weight decay"""
    tensors, hp, t, *_ = opt_case((3e-3, 0.999, 0.0, 10, None))
    for p, g, m, v in tensors:
        m2, v2, p2 = adamw_emul32(p, g, m, v, 1.0, hp, t)
        assert m2[0] == 0 and v2[0] == 0 and p2[0] == p[0]
        ref = adamw_ref64(p, g, m, v, 1.0, False, hp, t)
        assert ref["p"][0] == float(p[0])


@pytest.mark.parametrize("mutation,case", [
    ("wd_after", (3e-3, 0.999, 0.05, 1000, None)), ("t_minus_1", (3e-3, 0.999, 0.05, 10, None)), ("eps_in_sqrt", (3e-3, 0.999, 0.05, 10, None)),
    ("clip_m_only", (3e-3, 0.999, 0.05, 10, "below")), ("bc2_no_sqrt", (3e-3, 0.999, 0.05, 10, None))])
def test_adamw_mutations_are_rejected(mutation, case):
    tensors, hp, t, max_norm, n64, coef, active = opt_case(case)
    c32 = coef_emul32(norm_emul32(tensors), max_norm)
    for fma in (False, True):
        bad = 0
        for p, g, m, v in tensors:
            ref = adamw_ref64(p, g, m, v, coef, active, hp, t)
            try:
                check_adamw(adamw_emul32(p, g, m, v, c32, hp, t, fma=fma, mutate=mutation), ref, mutation)
            except AssertionError:
                bad += 1
        # the GPU test checks every tensor, so one rejection is enough; eps inside the root is invisible where sqrt(v) >> 1e-4
        # (the gradient scales 2^2 and up), every other defect shows in all but the one- and three-element tensors
        assert bad >= (4 if mutation == "eps_in_sqrt" else len(tensors) - 2), (mutation, fma, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# [K] packed operands
# ---------------------------------------------------------------------------------------------------------------------------
PACK_FORMS = [      # (O, T, I, flip): every O, I in {1, 63, 64, 65, 130}, every T in {1, 9, 16}, both flips
    (1, 1, 1, 0), (63, 9, 65, 1), (64, 16, 64, 0), (65, 1, 130, 1), (130, 9, 1, 0), (130, 16, 63, 1), (1, 16, 130, 1),
    (64, 9, 64, 1), (63, 1, 63, 0), (65, 16, 65, 0)]


def pack_ref(src, flip):
    """bf16 [O, T, I] -> [I, T', O]"""
    return (src.flip(1) if flip else src).permute(2, 1, 0).contiguous()


def pack_tiles(O, T, I):
    return ((O + 63) // 64) * ((I + 63) // 64) * T


def test_pack_forms_cover_the_issue_sizes():
    assert {f[0] for f in PACK_FORMS} == {f[2] for f in PACK_FORMS} == {1, 63, 64, 65, 130}
    assert {f[1] for f in PACK_FORMS} == {1, 9, 16} and {f[3] for f in PACK_FORMS} == {0, 1} and len(PACK_FORMS) >= 5
    src = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4).to(torch.bfloat16)
    assert pack_ref(src, 1)[3, 0, 1] == src[1, 2, 3] and pack_ref(src, 0)[3, 0, 1] == src[1, 0, 3]


# ---------------------------------------------------------------------------------------------------------------------------
# [L] tv_vae_loss_l1_kl
# ---------------------------------------------------------------------------------------------------------------------------
LOSS_N_IMG = [1, 255, 4096, 4097, 3 * 4096 + 17]
LOSS_N_LAT = [1, 100, 4097]
LOSS_LOGITS = [0.0, 1e-3, 1.0, 8.0, 12.0, 17.0, 30.0, 90.0, 104.0]
LOSS_CLIP = (-30.0, 20.0)
SIG_C = 16.0          # row Q


def loss_scales(n_img, l1_weight, kl_weight, kl_denom):
    """l1_scale, kl_scale as the host wrapper of the kernel computes them: fp32 divisions"""
    return float(F32(l1_weight) / F32(n_img)), float(F32(kl_weight) / F32(kl_denom))


def loss_inputs(n_img, n_lat, seed=0, edges=False, clip=None):
    """recon, target, mu, logvar as float32 arrays.  recon ~ 2 randn (logits when the sigmoid is on), target in [0, 1), exact
    ties recon == target at every 7th element.  edges: the saturation logits +-LOSS_LOGITS in recon (n_img >= 32) and, in
    logvar (n_lat >= 16), lo, hi, one ulp outside and inside each, +-1000 (with a clamp) or +-20 (without)."""
    rng = np.random.default_rng(seed)
    recon = (2.0 * rng.standard_normal(n_img)).astype(F32)
    target = rng.uniform(0, 1, n_img).astype(F32)
    recon[6::7] = target[6::7]
    mu = rng.standard_normal(n_lat).astype(F32)
    lv = (1.5 * rng.standard_normal(n_lat)).astype(F32)
    if edges:
        assert n_img >= 32 and n_lat >= 16
        lg = np.array([s * x for x in LOSS_LOGITS for s in (1.0, -1.0)], F32)
        recon[8:8 + lg.size] = lg
        target[8:8 + lg.size] = rng.uniform(0.25, 0.75, lg.size).astype(F32)
        if clip is not None:
            lo, hi = F32(clip[0]), F32(clip[1])
            ninf, pinf = F32(-np.inf), F32(np.inf)
            lv[:10] = [lo, hi, np.nextafter(lo, ninf), np.nextafter(hi, pinf), np.nextafter(lo, pinf), np.nextafter(hi, ninf),
                       1000.0, -1000.0, 0.0, -0.0]
        else:
            lv[:4] = [20.0, -20.0, 0.0, -0.0]
    return recon, target, mu, lv


def loss_ref64(recon, target, mu, lv, l1_scale, kl_scale, sigmoid, clip):
    """the reference's formulation in fp64 torch (sigmoid, L1 mean, torch.clamp, KL sum) and its autograd ->
    dict(out[3], d_recon, d_mu, d_logvar, and the per-element bounds b_recon, b_logvar)"""
    r = torch.from_numpy(recon.astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy(target.astype(np.float64))
    m = torch.from_numpy(mu.astype(np.float64)).requires_grad_(True)
    l = torch.from_numpy(lv.astype(np.float64)).requires_grad_(True)
    rr = torch.sigmoid(r) if sigmoid else r
    l1 = (rr - t).abs().sum() * l1_scale
    lc = torch.clamp(l, clip[0], clip[1]) if clip is not None else l
    kl = (-0.5 * (1.0 + lc - m * m - torch.exp(lc))).sum() * kl_scale
    (l1 + kl).backward()
    e = torch.exp(lc.detach())
    inside = torch.ones_like(e) if clip is None else ((l.detach() >= clip[0]) & (l.detach() <= clip[1])).to(F64)
    b_lv = inside * abs(kl_scale) * 0.5 * (2.0 ** -20 * (1.0 + lc.detach().abs()) * e + 2.0 * U * (1.0 - e).abs()) + TINY
    d_r = r.grad
    if sigmoid:       # autograd's s (1 - s) cancels in fp64 as well (0 from logit +37 on): the derivative as e / (1 + e)^2
        ea = torch.exp(-r.detach().abs())
        d_r = torch.sign(rr.detach() - t) * l1_scale * ea / ((1.0 + ea) * (1.0 + ea))
    b_r = (SIG_C + 1.0) * U * d_r.abs() + TINY if sigmoid else torch.zeros_like(d_r)
    return dict(out=np.array([l1.item(), kl.item(), (l1 + kl).item()]), d_recon=d_r.numpy(), d_mu=m.grad.numpy(),
                d_logvar=l.grad.numpy(), b_recon=b_r.numpy(), b_logvar=b_lv.numpy())


def _block_sum32(terms, seq):
    """vae_loss_kernel's sum: blocks of 4096, thread j's chain over j, j + 256, ..., each wave of 64 as a butterfly in fp32 (far
    lanes first as the kernel's, or `seq`: neighbours first), the 4 waves in order, the blocks in fp64"""
    n = terms.size
    nb = -(-n // 4096)
    c = np.zeros(nb * 4096, F32)
    c[:n] = terms
    c = c.reshape(nb, 16, 256)
    acc = np.zeros((nb, 256), F32)
    for i in range(16):
        acc = acc + c[:, i]
    w = acc.reshape(nb, 4, 64)
    while w.shape[2] > 1:
        h = w.shape[2] // 2
        w = w[:, :, 0::2] + w[:, :, 1::2] if seq else w[:, :, :h] + w[:, :, h:]
    part = np.zeros(nb, F32)
    for i in range(4):
        part = part + w[:, i, 0]
    return part


def loss_emul32(recon, target, mu, lv, l1_scale, kl_scale, sigmoid, clip, seq=False, mutate=None):
    """the kernel's documented arithmetic in float32 (np.exp for the exponential).  Mutations: 'kl_batch_only' (KL scale x 256:
    divided by the batch, not batch x H x W), 'grad_outside_clamp', 'r_one_minus_r' (the sigmoid derivative as r (1 - r)),
    'nan_clamp' (fminf / fmaxf: a NaN logvar becomes lo)."""
    one = F32(1)
    l1s, kls = F32(l1_scale), F32(kl_scale * 256 if mutate == "kl_batch_only" else kl_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        if sigmoid:
            e = np.exp(-np.abs(recon)).astype(F32)
            r = np.where(recon >= 0, one / (one + e), e / (one + e)).astype(F32)
            dr = r * (one - r) if mutate == "r_one_minus_r" else e / ((one + e) * (one + e))
        else:
            r, dr = recon, np.ones_like(recon)
        d = r - target
        d_recon = (np.where(d > 0, l1s, np.where(d < 0, -l1s, F32(0))) * dr).astype(F32)
        d_recon = np.where(np.isnan(d), F32(np.nan), d_recon)
        lc, outside = lv, np.zeros(lv.shape, bool)
        if clip is not None:
            lo, hi = F32(clip[0]), F32(clip[1])
            outside = (lv < lo) | (lv > hi)
            lc = np.fmin(np.fmax(lv, lo), hi) if mutate == "nan_clamp" else np.where(lv < lo, lo, np.where(lv > hi, hi, lv))
            if mutate == "nan_clamp":
                outside = ~((lv >= lo) & (lv <= hi))
            if mutate == "grad_outside_clamp":
                outside[:] = False
        e = np.exp(lc).astype(F32)
        term = F32(-0.5) * (one + lc - mu * mu - e)
        d_mu = kls * mu
        d_lv = np.where(outside, F32(0), kls * F32(-0.5) * (one - e)).astype(F32)
        pa = (_block_sum32(np.abs(d), seq) * l1s).astype(np.float64).sum()
        pb = (_block_sum32(term, seq) * kls).astype(np.float64).sum()
    return np.array([F32(pa), F32(pb), F32(pa + pb)]), d_recon, d_mu.astype(F32), d_lv


def check_loss(got, ref, sigmoid, l1_scale, recon, target, what, have=(True, True, True)):
    """got = (out, d_recon, d_mu, d_logvar) -> figures.  Values 1e-6 relative; d_recon exact without the sigmoid, c = 16 with;
    d_mu within one rounding; d_logvar within its slack.  `have`: which gradients were asked for."""
    out, d_recon, d_mu, d_lv = got
    fig = {}
    for i, nm in enumerate(("l1", "kl", "total")):
        assert math.isfinite(float(out[i])), (what, nm, out)
        fig[nm] = abs(float(out[i]) - ref["out"][i]) / abs(ref["out"][i])
        assert fig[nm] <= VALUE_RTOL, f"{what}: {nm} = {float(out[i])!r} vs {ref['out'][i]!r}: {fig[nm]:.3g} relative"
    if have[0]:
        if sigmoid:
            fig["d_recon"] = check_bound(d_recon, ref["d_recon"], ref["b_recon"], what + " d_recon")
        else:
            d = recon.astype(np.float64) - target.astype(np.float64)
            exact = np.where(d > 0, F32(l1_scale), np.where(d < 0, -F32(l1_scale), F32(0))).astype(F32)
            assert np.array_equal(np.asarray(d_recon, F32), exact), what + ": d_recon is not exactly +-l1_scale / 0"
            fig["d_recon"] = 0.0
    if have[1]:
        fig["d_mu"] = check_bound(d_mu, ref["d_mu"], U * np.abs(ref["d_mu"]) + TINY, what + " d_mu")
    if have[2]:
        fig["d_logvar"] = check_bound(d_lv, ref["d_logvar"], ref["b_logvar"], what + " d_logvar")
        assert np.all(np.asarray(d_lv)[ref["d_logvar"] == 0] == 0), what + ": a gradient flows outside the clamp"
    return fig


def check_nonfinite(out, d_lv, which, what):
    """a NaN in logvar / mu poisons out[1] and out[2]; in recon / target out[0] and out[2] -- as the torch formulation"""
    bad = (1, 2) if which in ("logvar", "mu") else (0, 2)
    for i in bad:
        assert math.isnan(float(out[i])), f"{what}: NaN in {which} but out[{i}] = {float(out[i])!r}"
    if which == "logvar":
        assert math.isnan(float(d_lv)), f"{what}: NaN in logvar but its gradient is {float(d_lv)!r}"


LOSS_W = dict(l1_weight=1.0, kl_weight=1e-3, kl_denom=64.0)


@pytest.mark.parametrize("sigmoid,clip", [(0, None), (1, None), (0, LOSS_CLIP), (1, LOSS_CLIP)])
def test_loss_clean_emulation_is_inside_the_bounds(sigmoid, clip):
    for n_img, n_lat, edges in ((1, 1, False), (255, 100, True), (3 * 4096 + 17, 4097, True)):
        l1s, kls = loss_scales(n_img, **LOSS_W)
        x = loss_inputs(n_img, n_lat, seed=n_img, edges=edges, clip=clip)
        ref = loss_ref64(*x, l1s, kls, sigmoid, clip)
        for seq in (False, True):
            check_loss(loss_emul32(*x, l1s, kls, sigmoid, clip, seq=seq), ref, sigmoid, l1s, x[0], x[1], f"emulation seq={seq}")


@pytest.mark.parametrize("mutation", ["kl_batch_only", "grad_outside_clamp", "r_one_minus_r"])
def test_loss_mutations_are_rejected(mutation):
    n_img, n_lat = 255, 100
    l1s, kls = loss_scales(n_img, **LOSS_W)
    x = loss_inputs(n_img, n_lat, seed=3, edges=True, clip=LOSS_CLIP)
    ref = loss_ref64(*x, l1s, kls, 1, LOSS_CLIP)
    with pytest.raises(AssertionError):
        check_loss(loss_emul32(*x, l1s, kls, 1, LOSS_CLIP, mutate=mutation), ref, 1, l1s, x[0], x[1], mutation)


def test_r_one_minus_r_is_rejected_at_logit_12_alone():
    """the saturated-sigmoid defect at one logit: r (1 - r) at +12 is about 1e-2 relative off e / (1 + e)^2"""
    recon, target = np.array([12.0], F32), np.array([0.5], F32)
    mu, lv = np.zeros(1, F32), np.ones(1, F32)
    ref = loss_ref64(recon, target, mu, lv, 1.0, 1.0, 1, None)
    check_loss(loss_emul32(recon, target, mu, lv, 1.0, 1.0, 1, None), ref, 1, 1.0, recon, target, "clean")
    bad = loss_emul32(recon, target, mu, lv, 1.0, 1.0, 1, None, mutate="r_one_minus_r")
    assert abs(bad[1][0] / ref["d_recon"][0] - 1) > 1e-3
    with pytest.raises(AssertionError):
        check_loss(bad, ref, 1, 1.0, recon, target, "r (1 - r)")


def test_nan_swallowing_clamp_is_rejected():
    l1s, kls = loss_scales(255, **LOSS_W)
    x = loss_inputs(255, 100, seed=4)
    x[3][17] = np.nan
    ref = loss_ref64(*x, l1s, kls, 0, LOSS_CLIP)
    assert math.isnan(ref["out"][1]) and math.isnan(ref["out"][2]) and math.isfinite(ref["out"][0])       # torch.clamp propagates
    out, _, _, d_lv = loss_emul32(*x, l1s, kls, 0, LOSS_CLIP)
    check_nonfinite(out, d_lv[17], "logvar", "clean")
    out, _, _, d_lv = loss_emul32(*x, l1s, kls, 0, LOSS_CLIP, mutate="nan_clamp")
    with pytest.raises(AssertionError):
        check_nonfinite(out, d_lv[17], "logvar", "fminf / fmaxf clamp")
    x[3][17] = np.inf                                                                                      # +inf clamps to hi
    ref = loss_ref64(*x, l1s, kls, 0, LOSS_CLIP)
    out, _, _, d_lv = loss_emul32(*x, l1s, kls, 0, LOSS_CLIP)
    assert np.isfinite(ref["out"]).all() and np.isfinite(out).all() and d_lv[17] == 0 and ref["d_logvar"][17] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# [Z] folds
# ---------------------------------------------------------------------------------------------------------------------------
FOLD_R = [1, 3, 63, 64, 65, 200]
FOLD_C = [4, 60, 64, 68, 72, 384, 1, 7, 66, 130]          # the last four: the scalar branches (C % 4 != 0)
FOLD_BF_C = 16.0
FOLD_ROWS = 64


def fold_k(R):
    """roundings of a column sum: a thread's chain of 4 products and 4 adds, 16 row lanes, ceil(R / 64) chunks"""
    return 8.0 + 16.0 + -(-R // FOLD_ROWS)


def fold_inputs(R, Cc, seed=0):
    """W, gamma, beta, dWf [R, C] / [C], dbf [R] as float32 arrays: gamma with per-column scales 2^-6 .. 2^6; dbf 64x dWf's
    scale in every third row; from three rows on the last row of dWf is set so that each column of dWf * W sums to 2^-10 of
    its sum of magnitudes."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((R, Cc)) * Cc ** -0.5).astype(F32)
    gamma = (rng.standard_normal(Cc) * 2.0 ** rng.integers(-6, 7, Cc)).astype(F32)
    beta = (0.2 * rng.standard_normal(Cc)).astype(F32)
    dWf = rng.standard_normal((R, Cc)).astype(F32)
    dbf = (rng.standard_normal(R) * np.where(np.arange(R) % 3 == 0, 64.0, 1.0)).astype(F32)
    if R >= 3:
        t = dWf[:-1].astype(np.float64) * W[:-1]
        want = 2.0 ** -10 * 2.0 * np.abs(t).sum(0) - t.sum(0)
        dWf[-1] = (want / W[-1].astype(np.float64)).astype(F32)
    return W, gamma, beta, dWf, dbf


def fold_ref64(W, gamma, beta, dWf, dbf):
    """-> dict of fp64 values and |terms|; beta / dbf None: no bias term"""
    W64, g64, d64 = W.astype(np.float64), gamma.astype(np.float64), dWf.astype(np.float64)
    out = dict(Wf=(W * gamma).astype(F32), dgamma=(d64 * W64).sum(0), t_dgamma=np.abs(d64 * W64).sum(0), dW=d64 * g64,
               t_dW=np.abs(d64 * g64))
    if beta is not None:
        b64, db64 = beta.astype(np.float64), dbf.astype(np.float64)
        out.update(bf=W64 @ b64, t_bf=np.abs(W64) @ np.abs(b64), dbeta=db64 @ W64, t_dbeta=np.abs(db64) @ np.abs(W64))
        out["dW"] = out["dW"] + db64[:, None] * b64
        out["t_dW"] = out["t_dW"] + np.abs(db64[:, None] * b64)
    return out


def fold_emul32(W, gamma, beta, dWf, dbf, kernel_order=True, mutate=None):
    """float32 model of both kernels.  kernel_order: the column sums as fold_bwd_kernel takes them (rows r0 + ry, + 16, ... per
    thread, 16 row lanes in order, chunks in order); otherwise numpy's pairwise fp32 sums.  Mutations: 'drop_last_chunk'
    (dgamma without the last row chunk), 'dbeta_from_dWf', 'drop_col_tail' (the last C % 64 columns never written)."""
    R, Cc = W.shape
    has_b = beta is not None
    Wf = W * gamma
    bf = (W * beta).sum(1, dtype=F32) if has_b else None
    dW = dWf * gamma + (dbf[:, None] * beta if has_b else F32(0))
    tg = dWf * W
    tb = None
    if has_b:
        tb = (dWf if mutate == "dbeta_from_dWf" else dbf[:, None] * np.ones_like(W)) * W
    nchunk = -(-R // FOLD_ROWS)

    def colsum(t):
        if not kernel_order:
            last = (nchunk - 1) * FOLD_ROWS if mutate == "drop_last_chunk" else R
            return t[:last].sum(0, dtype=F32) if last else np.zeros(Cc, F32)
        tot = np.zeros(Cc, F32)
        for k in range(nchunk - 1 if mutate == "drop_last_chunk" else nchunk):
            c = np.zeros((FOLD_ROWS, Cc), F32)
            rows = t[k * FOLD_ROWS:(k + 1) * FOLD_ROWS]
            c[:rows.shape[0]] = rows
            lanes = np.zeros((16, Cc), F32)
            for i in range(4):
                lanes = lanes + c[i * 16:(i + 1) * 16]
            blk = np.zeros(Cc, F32)
            for i in range(16):
                blk = blk + lanes[i]
            tot = tot + blk
        return tot
    dgamma = colsum(tg)
    dbeta = colsum(tb) if has_b else None
    if mutate == "drop_col_tail" and Cc % 64:
        keep = Cc - Cc % 64
        for a in (Wf, dW):
            a[:, keep:] = 0
        dgamma[keep:] = 0
    return dict(Wf=Wf.astype(F32), bf=bf, dW=dW.astype(F32), dgamma=dgamma, dbeta=dbeta)


def check_fold(got, ref, R, what):
    """got: dict of Wf, bf, dW, dgamma, dbeta (None where absent) -> worst ratios"""
    fig = {}
    assert np.array_equal(np.asarray(got["Wf"], F32).view(np.uint32), ref["Wf"].view(np.uint32)), what + ": Wf is not the IEEE fp32 product"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    fig["dW"] = check_fp32(t(got["dW"]), t(ref["dW"]), t(ref["t_dW"]), 2.0, what + " dW")
    fig["dgamma"] = check_fp32(t(got["dgamma"]), t(ref["dgamma"]), t(ref["t_dgamma"]), fold_k(R), what + " dgamma")
    if "bf" in ref:
        fig["bf"] = check_fp32(t(got["bf"]), t(ref["bf"]), t(ref["t_bf"]), FOLD_BF_C, what + " bf")
        fig["dbeta"] = check_fp32(t(got["dbeta"]), t(ref["dbeta"]), t(ref["t_dbeta"]), fold_k(R), what + " dbeta")
    for k in ("dW", "dgamma", "bf", "dbeta"):
        if got.get(k) is not None:
            assert np.isfinite(np.asarray(got[k])).all(), (what, k)
    return fig


@pytest.mark.parametrize("R", FOLD_R)
def test_fold_clean_emulation_is_inside_the_bounds(R):
    for Cc in FOLD_C:
        W, gamma, beta, dWf, dbf = fold_inputs(R, Cc, seed=R * 1000 + Cc)
        for has_b in (True, False):
            b, db = (beta, dbf) if has_b else (None, None)
            ref = fold_ref64(W, gamma, b, dWf, db)
            if R >= 3:
                assert np.all(np.abs(ref["dgamma"]) <= 2.0 ** -8 * ref["t_dgamma"])          # the columns do cancel
            for order in (True, False):
                check_fold(fold_emul32(W, gamma, b, dWf, db, kernel_order=order), ref, R, f"emulation {R}x{Cc} order={order}")


@pytest.mark.parametrize("mutation,R,Cc", [("drop_last_chunk", 65, 68), ("drop_last_chunk", 200, 7), ("dbeta_from_dWf", 63, 64),
                                           ("drop_col_tail", 64, 68), ("drop_col_tail", 3, 130)])
def test_fold_mutations_are_rejected(mutation, R, Cc):
    W, gamma, beta, dWf, dbf = fold_inputs(R, Cc, seed=R * 1000 + Cc)
    ref = fold_ref64(W, gamma, beta, dWf, dbf)
    for order in (True, False):
        with pytest.raises(AssertionError):
            check_fold(fold_emul32(W, gamma, beta, dWf, dbf, kernel_order=order, mutate=mutation), ref, R, mutation)
