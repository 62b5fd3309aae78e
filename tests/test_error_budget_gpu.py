"""Error budget, GPU side: every kernel family against an fp64 reference of the same bf16 inputs, with the bound its row of
the rounding contract implies (checks and references in tests/test_error_budget_host.py, whose mutation
tests show that these bounds reject specific defects).  Inputs are built to reach where kernels go wrong: per-row scales
of x over 2^-6..2^6, bias / residual that match or dominate the accumulator, ragged row tails, N edges, forced tiles;
attention with a large common offset on v, spiked keys and rows whose max grows across the lazy-rescale threshold;
GroupNorm with |mean| up to 100 std; the production attention branch (fused.AttnBranchFn): rms_ln_hat with |mean u| up to
100 std u and the fused residual gradient, RoPE in the QKV projection's epilogue across image boundaries, the RoPE adjoint
in the attention-backward stores; the production GroupNorm + SiLU path (fused.gn_silu_fwd / gn_silu_apply / gn_silu_bwd with
the fused skip-connection gradient) over its thread geometries, at outlier pivots and on its non-temporal instantiations.
Every tuning hook a test sets is restored in a `finally`.
"""
import pytest
import torch

import functools

from test_error_budget_host import (
    BF, EPS_LN, EPS_RMS, F64, LSE_C, ROWNORM_C_DW, WGRAD_C, act_grad64, attn_bwd_emul, attn_bwd_exact, attn_exact,
    attn_fwd_emul, attn_inputs, check_fp32, check_one_rounding, check_vs_emulation, conv64, deriv64, epilogue64, f32,
    gemm_inputs, gn_bwd64, gn_case, gn_check_all, gn_inputs, gn_k_g, gn_silu64, check_gn_stats, lse_terms, r16,
    rms_ln_hat64, rms_ln_inputs, rms_ln_slack, rope_epilogue64, rownorm_bwd64, rownorm_dres, ulp16, wgrad64)

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


# ---------------------------------------------------------------------------------------------------------------------------
# [W] hardware: does the bf16 MFMA's fp32 accumulation round to nearest?
# ---------------------------------------------------------------------------------------------------------------------------
def test_mfma_fp32_accumulation_rounds_to_nearest():
    """Exact-input probe through the weight gradient (fp32 output): positive bf16 x, g, so every fp32 rounding of a growing
    partial sum is a one-sided coin if the accumulation truncates (a bias of about -0.5 ulp per rounding, -40 in units of
    2^-24 sum|g x| over these 8192 tokens) and unbiased if it rounds to nearest.  The fp64 reference is exact (products of
    bf16 have 16 bits; 8192 of them fit in 53).  Asserts the mean signed error within +-2 units of 2^-24 sum|g x|."""
    from transvae.hip import ops
    g = torch.Generator().manual_seed(1)
    T, K, N = 8192, 128, 128
    x = r16(0.5 + 0.5 * torch.rand(T, K, generator=g, dtype=F64))
    gy = r16(0.5 + 0.5 * torch.rand(T, N, generator=g, dtype=F64))
    w = r16(torch.randn(N, K, generator=g, dtype=F64) * K ** -0.5)
    xd = x.to(dev(), BF).requires_grad_(True)
    wd = w.float().to(dev()).requires_grad_(True)
    y = ops.linear(xd, wd)
    y.backward(gy.to(dev(), BF))
    torch.cuda.synchronize()
    dw64, absd = wgrad64(x, gy)
    e = (wd.grad.cpu().to(F64) - dw64) / (2.0 ** -24 * absd)
    report("MFMA accumulation bias (units of 2^-24 sum|gx|)", f"mean {e.mean().item():+.3f} max {e.abs().max().item():.3f}")
    assert abs(e.mean().item()) <= 2.0, e.mean().item()
    check_fp32(wd.grad.cpu(), dw64, absd, WGRAD_C, "probe dw")


# ---------------------------------------------------------------------------------------------------------------------------
# [G] GEMM forward (linear) with every epilogue form, on the heuristic tile and on forced tiles
# ---------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(2048 + 40, 64, 384), (2048 + 40, 192, 160), (2048 + 40, 1536, 384), (300, 192, 384)]
TILE_CFGS = {"default": None, "256x256-8phase": (256, 256), "256x192-8phase": (256, 192), "nt-stores": "nt"}


def _set_cfg(lib, cfg):
    if cfg == "nt":
        lib.tv_set_igemm_nt_threshold(0)
    elif cfg is not None:
        lib.tv_set_igemm_config(cfg[0], cfg[1], 0, 0)
        lib.tv_set_igemm_persist(-2)


def _reset_cfg(lib):
    lib.tv_set_igemm_nt_threshold(64)
    lib.tv_set_igemm_config(0, 0, 0, 0)
    lib.tv_set_igemm_persist(-2)
    lib.tv_set_igemm_persist(0)


@pytest.mark.parametrize("cfg", list(TILE_CFGS))
@pytest.mark.parametrize("M,K,N", GEMM_SHAPES)
def test_gemm_forward_one_rounding(M, K, N, cfg):
    """[G]: plain + bias, + residual, GELU with the saved derivative (TV_ACT_SAVE_DERIV), SiLU, and TV_ACT_ADD
    (acc + residual + aux in one fp32 sum)"""
    from transvae.hip import _lib as L, ops
    lib = L.load()
    x, w, b, res = gemm_inputs(M, K, N, seed=M + K + N)
    aux = r16(res.flip(0))
    acc, absdot = conv64(x, w, "linear")
    xd, wd, bd, rd, ad = x.to(dev(), BF), w.float().to(dev()), b.float().to(dev()), res.to(dev(), BF), aux.to(dev(), BF)
    wb = w.to(dev(), BF).contiguous()
    try:
        _set_cfg(lib, TILE_CFGS[cfg])
        out = {
            "plain": ops.conv_forward(xd, wd, bd, None, "linear", L.ACT_NONE, False)[0],
            "residual": ops.conv_forward(xd, wd, bd, rd, "linear", L.ACT_NONE, False)[0],
            "gelu+deriv": ops.conv_forward(xd, wd, bd, None, "linear", L.ACT_GELU, "deriv")[:2],
            "silu": ops.conv_forward(xd, wd, bd, None, "linear", L.ACT_SILU, False)[0],
            "act_add": ops.gemm_rows(xd, wb, N, residual=rd, aux=ad, aux_act=L.ACT_ADD),
        }
        torch.cuda.synchronize()
    finally:
        _reset_cfg(lib)
    worst = {}
    y64, sl, _ = epilogue64(acc, absdot, b)
    worst["plain"] = check_one_rounding(out["plain"].cpu(), y64, sl, "plain")
    y64, sl, _ = epilogue64(acc, absdot, b, res)
    worst["residual"] = check_one_rounding(out["residual"].cpu(), y64, sl, "residual")
    y64, sl, z = epilogue64(acc, absdot, b, None, "gelu")
    worst["gelu"] = check_one_rounding(out["gelu+deriv"][0].cpu(), y64, sl, "gelu")
    d64, dsl = deriv64(z, absdot, b, "gelu")
    worst["gelu'"] = check_one_rounding(out["gelu+deriv"][1].cpu(), d64, dsl, "saved gelu'")
    y64, sl, _ = epilogue64(acc, absdot, b, None, "silu")
    worst["silu"] = check_one_rounding(out["silu"].cpu(), y64, sl, "silu")
    y64, sl, _ = epilogue64(acc, absdot, None, res + aux)
    sl = sl + 2.0 ** -24 * aux.abs()
    worst["act_add"] = check_one_rounding(out["act_add"].cpu(), y64, sl, "acc + residual + aux")
    report(f"[G] linear {M}x{K}x{N} {cfg} (ratio, max ulps, bias)",
           {k: tuple(round(v, 3) for v in t) for k, t in worst.items()})


def test_gemm_rows2_against_fp64_of_the_concatenation():
    """[G]/[D]: the two-source loop against fp64 of [x1 | x2] w^T, forward (bias + residual) and data-gradient
    (saved-derivative multiply) forms, 256-row tiles, ragged rows"""
    from transvae.hip import _lib as L, ops
    lib = L.load()
    T, K1, K2, N = 2048 + 72, 1536, 384, 768
    x, w, b, res = gemm_inputs(T, K1 + K2, N, seed=77)
    der = r16(torch.rand(T, N, generator=torch.Generator().manual_seed(3), dtype=F64))
    x1, x2 = x[:, :K1].contiguous(), x[:, K1:].contiguous()
    acc, absdot = conv64(x, w, "linear")
    d = lambda t: t.to(dev(), BF).contiguous()
    try:
        for bn in (256, 192):
            lib.tv_set_igemm_config(256, bn, 0, 0)
            y = ops.gemm_rows2(d(x1), d(x2), d(w), N, bias=b.float().to(dev()), residual=d(res))
            dx = ops.gemm_rows2(d(x1), d(x2), d(w), N, aux=d(der), aux_act=L.ACT_DERIV)
            assert y is not None and dx is not None
            y64, sl, _ = epilogue64(acc, absdot, b, res)
            r1 = check_one_rounding(y.cpu(), y64, sl, f"rows2 bias+residual bn={bn}")
            r2 = check_one_rounding(dx.cpu(), acc * der, 2.0 ** -20 * absdot * der, f"rows2 x deriv bn={bn}")
            report(f"[G] rows2 bn={bn}", (tuple(round(v, 3) for v in r1), tuple(round(v, 3) for v in r2)))
    finally:
        lib.tv_set_igemm_config(0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# [G] the QKV projection with RoPE in its epilogue (tv_igemm_nt_rope), as fused.AttnBranchFn launches it
# ---------------------------------------------------------------------------------------------------------------------------
ROPE_CASES = [
    # heads (K = 64 heads, N = 3 K, rope_cols = 2 K), tokens per image, images, table.  rope_cols = 128 (heads 1) and 384
    # (heads 3) fall inside a 256-wide tile, 128 inside a 192-wide one; M = 420, 900, 300, 600, 360, 1200, 180, 1500 leave a
    # ragged last row tile and every 128- / 256-row tile of the 60- and 300-token cases straddles an image boundary
    (1, 60, 7, "indep"), (1, 300, 3, "indep"), (1, 1024, 2, "indep"),
    (2, 60, 5, "indep"), (2, 300, 2, "indep"), (2, 1024, 3, "real"),
    (3, 60, 6, "indep"), (3, 300, 4, "indep"), (3, 1024, 2, "indep"),
    (6, 60, 3, "real"), (6, 300, 5, "indep"), (6, 1024, 2, "indep"),
]
_GRID = {60: (5, 12), 300: (15, 20), 1024: (32, 32)}


@functools.lru_cache(maxsize=1)
def _rope_reference(case):
    heads, tokens, images, table = case
    M, K = tokens * images, heads * 64
    x, w, b, _ = gemm_inputs(M, K, 3 * K, seed=M + K)
    if table == "real":
        from oracle import filler, transvae_oracle as O
        tab = torch.stack(O.rope_tables(*_GRID[tokens], filler.inv_freq(64)), 1).float().contiguous()
    else:
        tab = _rope_table(tokens, heads)
    acc, absdot = conv64(x, w, "linear")
    y64, slack = rope_epilogue64(acc, absdot, b, tab.to(F64), tokens, 2 * K)
    return x, w, b, tab, y64, slack


@pytest.mark.parametrize("cfg", list(TILE_CFGS))
@pytest.mark.parametrize("case", ROPE_CASES, ids=[f"h{c[0]}-{c[1]}tok-x{c[2]}-{c[3]}" for c in ROPE_CASES])
def test_rope_epilogue_one_rounding(case, cfg):
    """[G]: q and k thirds rotated on the fp32 accumulator with the table row of token m % tokens, v third plain, one rounding;
    tables with four independent planes and the reference's own"""
    from transvae.hip import _lib as L, ops
    lib = L.load()
    heads, tokens, images, _ = case
    K = heads * 64
    x, w, b, tab, y64, slack = _rope_reference(case)
    try:
        _set_cfg(lib, TILE_CFGS[cfg])
        y = ops.conv_forward(x.to(dev(), BF), w.float().to(dev()), b.float().to(dev()), None, "linear", L.ACT_NONE, False,
                             rope=(tab.to(dev()), tokens, 2 * K))[0]
        torch.cuda.synchronize()
    finally:
        _reset_cfg(lib)
    y = y.cpu()
    out = {"q,k": check_one_rounding(y[:, :2 * K], y64[:, :2 * K], slack[:, :2 * K], "rotated q, k"),
           "v": check_one_rounding(y[:, 2 * K:], y64[:, 2 * K:], slack[:, 2 * K:], "v third")}
    report(f"[G] rope epilogue {case} {cfg} (ratio, max ulps, bias)", {k: tuple(round(v, 3) for v in t) for k, t in out.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# [G] / [D] / [W] convolutions: forward, data gradient, weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def conv_inputs(mode, B, H, W, Cin, Cout, seed, exact_taps=False):
    """x with per-image / per-channel scales; w with per-output-channel scales.  exact_taps: w = (integer in [-8, 8]) 2^-s,
    so the polyphase / adjoint operands (sums of up to four taps, ops._up_fwd_weight / _up_dgrad_weight) are exact in
    bf16 and the operand the kernel consumes equals w"""
    g = torch.Generator().manual_seed(seed)
    kh = {"c3s1": 3, "c3s2": 3, "c3up": 3, "unshuf": 2, "shuf": 1}[mode]
    co = 4 * Cout if mode == "shuf" else Cout
    xs = torch.exp2(torch.randint(-4, 5, (B, 1, 1, Cin), generator=g).to(F64))
    x = r16(torch.randn(B, H, W, Cin, generator=g, dtype=F64) * xs)
    cs = torch.exp2(torch.randint(-2, 3, (co, 1, 1, 1), generator=g).to(F64))
    if exact_taps:
        w = torch.randint(-8, 9, (co, kh, kh, Cin), generator=g).to(F64) * 2.0 ** -7 * cs
    else:
        w = r16(torch.randn(co, kh, kh, Cin, generator=g, dtype=F64) * cs * (kh * kh * Cin) ** -0.5)
    b = f32(torch.randn(co if mode != "shuf" else co, generator=g, dtype=F64) * cs.flatten() * 0.5)
    return x, w, b


def conv_grads64(x, w, gy, mode):
    """fp64 (dx, sum|w gy| per dx element, dw, sum|x gy| per dw element) through autograd of conv64"""
    def vjp(xx, ww, gg):
        xx = xx.clone().requires_grad_(True)
        ww = ww.clone().requires_grad_(True)
        y, _ = conv64(xx, ww, mode)
        y.backward(gg)
        return xx.grad, ww.grad
    dx, dw = vjp(x.to(F64), w.to(F64), gy.to(F64))
    adx, adw = vjp(x.to(F64).abs(), w.to(F64).abs(), gy.to(F64).abs())
    return dx, adx, dw, adw


CONV_CASES = [
    # mode, B, H, W, Cin, Cout, halo
    ("c3s1", 2, 32, 40, 64, 192, 1),
    ("c3s1", 2, 32, 40, 64, 192, 0),
    ("c3s1", 3, 16, 16, 192, 160, 1),
    ("c3s2", 2, 32, 24, 96, 128, 1),
    ("c3up", 2, 16, 12, 128, 64, 1),
    ("unshuf", 2, 16, 24, 64, 128, 1),
    ("shuf", 2, 12, 10, 128, 64, 1),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}x{c[4]}-{c[5]}-halo{c[6]}" for c in CONV_CASES])
def test_conv_forward_dgrad_wgrad(case):
    """[G] forward with SiLU + residual and with the saved SiLU derivative; [D] data gradient plain, x saved derivative
    (TV_ACT_DERIV), x act' of a saved pre-activation (its bf16 copy) and (acc + residual) x derivative; [W] weight and
    bias gradient (fp32, run twice: split-K atomics reorder the sums)"""
    from transvae.hip import _lib as L, ops
    mode, B, H, W, Cin, Cout, halo = case
    lib = L.load()
    x, w, b = conv_inputs(mode, B, H, W, Cin, Cout, seed=B * H + Cin, exact_taps=(mode == "c3up"))
    acc, absdot = conv64(x, w, mode)
    bb = b if mode != "shuf" else None
    g = torch.Generator().manual_seed(9)
    res = r16(acc * (torch.randn(acc.shape, generator=g, dtype=F64) * 0.5 - 1))     # same magnitude, partly cancelling
    gz = r16(torch.randn(acc.shape, generator=g, dtype=F64) * torch.exp2(torch.randint(-3, 4, (1, 1, 1, acc.shape[-1]), generator=g).to(F64)))
    der = r16(torch.rand(x.shape, generator=g, dtype=F64))
    pre = r16(torch.randn(x.shape, generator=g, dtype=F64) * 2)
    gres = r16(torch.randn(x.shape, generator=g, dtype=F64))
    xd, wd = x.to(dev(), BF), w.float().to(dev())
    bd = bb.float().to(dev()) if bb is not None else None
    try:
        lib.tv_set_igemm_halo(halo)
        y_res = ops.conv_forward(xd, wd, bd, res.to(dev(), BF), mode, L.ACT_SILU, False)[0]
        y_d, sd = ops.conv_forward(xd, wd, bd, None, mode, L.ACT_SILU, "deriv")[:2]
        geo = ops._Geo(mode, xd, wd)
        gzd = gz.to(dev(), BF)
        dx = ops.conv_dgrad(geo, wd, gzd, x.shape)
        dx_der = ops.conv_dgrad(geo, wd, gzd, x.shape, aux=der.to(dev(), BF), aux_act=L.ACT_DERIV)
        dx_pre = ops.conv_dgrad(geo, wd, gzd, x.shape, aux=pre.to(dev(), BF), aux_act=L.ACT_GELU)
        dx_res = ops.conv_dgrad(geo, wd, gzd, x.shape, residual=gres.to(dev(), BF), aux=der.to(dev(), BF), aux_act=L.ACT_DERIV)
        dws = []
        for _ in range(2):
            xr = xd.clone().requires_grad_(True)
            wr = wd.clone().requires_grad_(True)
            br = bd.clone().requires_grad_(True) if bd is not None else None
            ops.conv(xr, wr, br, None, mode=mode).backward(gzd)
            dws.append((wr.grad.cpu(), None if br is None else br.grad.cpu()))
        torch.cuda.synchronize()
    finally:
        lib.tv_set_igemm_halo(1)
    out = {}
    y64, sl, z = epilogue64(acc, absdot, bb, res, "silu")
    out["silu+res"] = check_one_rounding(y_res.cpu(), y64, sl, "forward silu + residual")
    y64, sl, z = epilogue64(acc, absdot, bb, None, "silu")
    out["silu(saved)"] = check_one_rounding(y_d.cpu(), y64, sl, "forward silu, derivative saved")
    d64, dsl = deriv64(z, absdot, bb, "silu")
    out["silu'"] = check_one_rounding(sd.cpu(), d64, dsl, "saved silu'")
    dx64, adx, dw64, adw = conv_grads64(x, w, gz, mode)
    e = 2.0 ** -20 * adx
    out["dgrad"] = check_one_rounding(dx.cpu(), dx64, e, "dgrad")
    out["dgrad*deriv"] = check_one_rounding(dx_der.cpu(), dx64 * der, e * der, "dgrad x deriv")
    gp = act_grad64(pre, "gelu")
    out["dgrad*gelu'(pre)"] = check_one_rounding(dx_pre.cpu(), dx64 * gp, e * gp.abs() + 2.0 ** -20 * (1 + pre.abs()) * dx64.abs(),
                                                 "dgrad x gelu'(saved pre-activation)")
    out["(dgrad+res)*deriv"] = check_one_rounding(dx_res.cpu(), (dx64 + gres) * der, (e + 2.0 ** -24 * gres.abs()) * der,
                                                  "(dgrad + residual) x deriv")
    dwk, adwk = dw64, adw          # (autograd of conv64 returns the gradient in w's own [Cout, KH, KW, Cin] layout)
    db64, adb = gz.to(F64).sum((0, 1, 2)), gz.to(F64).abs().sum((0, 1, 2))
    for i, (dw, db) in enumerate(dws):
        out[f"dw#{i}"] = (check_fp32(dw, dwk, adwk, WGRAD_C, f"wgrad run {i}"),)
        if db is not None:
            out[f"db#{i}"] = (check_fp32(db, db64, adb, WGRAD_C, f"bias grad run {i}"),)
    report(f"[G/D/W] {case}", {k: tuple(round(v, 3) for v in t) for k, t in out.items()})


@pytest.mark.parametrize("W", [8, 16, 32, 64, 128])
def test_wgrad_widths(W):
    """[W] the weight gradient of a 3x3 layer and of a linear layer over the same pixels, image widths 8 .. 128 (split-K; each run
    twice: atomics reorder the sums).  Which kernel each shape runs, as ops.wgrad_which reports it (asserted on the host by
    test_wgrad_matrix_host.test_wgrad_widths_shapes_run_the_single_tap_kernel):
      128 -> 192   tn<192,128> bkp=64 waves=8 fast=1 at every width, 3x3 and linear alike (neither kx3 tile divides the layer);
      192 -> 192   3x3: kx3<192,96> taps=3, seg = min(W, 64), from W = 16 on (W = 8: tn<192,192>); linear: kx3<192,192> taps=1;
      128 -> 128   3x3: kx3<128,128> taps=3, seg = min(W, 64), from W = 16 on (W = 8: tn<128,128>); linear: tn<128,128>."""
    worst = [_wgrad_widths_layer(W, C, Co) for C, Co in ((128, 192), (192, 192), (128, 128))]
    report(f"[W] W={W} max ratio (128->192, 192->192, 128->128)", tuple(round(v, 3) for v in worst))


def _wgrad_widths_layer(W, C, Co):
    from transvae.hip import ops
    g = torch.Generator().manual_seed(W)
    B, H = 4, 64 if W <= 32 else 16
    x = r16(torch.randn(B, H, W, C, generator=g, dtype=F64))
    w = r16(torch.randn(Co, 3, 3, C, generator=g, dtype=F64) * (9 * C) ** -0.5)
    gz = r16(torch.randn(B, H, W, Co, generator=g, dtype=F64))
    _, _, dw64, adw = conv_grads64(x, w, gz, "c3s1")
    w1 = r16(torch.randn(Co, C, generator=g, dtype=F64) * C ** -0.5)
    dl64, adl = wgrad64(x, gz)
    worst = []
    for _ in range(2):
        wr = w.float().to(dev()).requires_grad_(True)
        ops.conv(x.to(dev(), BF), wr, None, None, mode="c3s1").backward(gz.to(dev(), BF))
        wl = w1.float().to(dev()).requires_grad_(True)
        ops.linear(x.reshape(-1, C).to(dev(), BF), wl).backward(gz.reshape(-1, Co).to(dev(), BF))
        torch.cuda.synchronize()
        worst.append(check_fp32(wr.grad.cpu(), dw64, adw, WGRAD_C, f"3x3 dw W={W} {C}->{Co}"))
        worst.append(check_fp32(wl.grad.cpu(), dl64, adl, WGRAD_C, f"linear dw W={W} {C}->{Co}"))
    return max(worst)


# ---------------------------------------------------------------------------------------------------------------------------
# [A] attention
# ---------------------------------------------------------------------------------------------------------------------------
def _rope_table(N, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(N, 32, generator=g) * 6.28
    tab = torch.stack([torch.cos(ang), torch.sin(ang), torch.cos(ang * 0.5), torch.sin(ang * 0.5)], 1)
    return tab.contiguous()


def _sample_groups(N, n):
    """32-row waves to emulate: all of them up to n, else the first, the last (ragged) and evenly spread others"""
    G = -(-N // 32)
    if G <= n:
        return list(range(G))
    return sorted(set([0, G - 1] + [int(i * (G - 1) / (n - 1)) for i in range(n)]))


ATTN_CASES = [
    # N, heads, rope, design
    (16, 2, False, "plain"),
    (300, 2, True, "offset-v"),
    (300, 2, False, "spiked"),
    (512, 1, False, "lazy-rows"),
    (2160, 1, False, "spiked"),
    (4096, 1, True, "plain"),
    (4096, 1, False, "offset-v"),
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=[f"N{c[0]}-h{c[1]}-{'rope' if c[2] else 'norope'}-{c[3]}" for c in ATTN_CASES])
def test_attention_against_emulation(case):
    """[A] o and lse of the forward (32-query kernel below 2048 tokens, 64-query kernel from there: key blocks of 64 / 32 in
    the lazy policy), delta, and dq / dk / dv, per (image, head) slice.  RoPE cases (ragged N = 300, N = 4096): tv_attn_bwd a
    second time with the table, as the model calls it -- dq, dk against the emulation that applies the adjoint to the fp32
    sums before the one rounding, dv and delta bit-identical to the run without the table"""
    from transvae.hip import _lib as L
    import ctypes as C
    N, heads, rope, design = case
    lib = L.load()
    Cc = heads * 64
    sl = []
    for h in range(heads):
        kw = dict(seed=N + h)
        if design == "offset-v":
            kw["v_offset"] = 4.0
        if design == "spiked":
            kw["spikes"] = ((N // 2 + 3, 5, 6.0), (N - 70, 40, 9.0), (N - 1, 130, 12.0), (200, 131, 4.0))
        if design == "lazy-rows":
            kw["lazy_rows"] = [(qi, 5 * 64 + 7 + qi % 30, 8.4 if qi % 2 else 7.6) for qi in range(64, 96, 5)]
        sl.append(attn_inputs(N, **kw))
    qkv = torch.cat([torch.cat([s[i] for s in sl], 1) for i in range(3)], 1)[None].float()       # [1, N, 3C]
    qkv_d = qkv.to(dev(), BF).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    if rope:
        tab = _rope_table(N, 3).to(dev())
        L.check(lib.tv_rope_qk(p(qkv_d), p(tab), 1, N, heads, 0, stream), "tv_rope_qk")
    o = torch.empty(1, N, Cc, dtype=BF, device=dev())
    lse = torch.empty(1, heads, N, dtype=torch.float32, device=dev())
    L.check(lib.tv_attn_fwd(p(qkv_d), p(o), p(lse), 1, N, heads, 0.125, stream), "tv_attn_fwd")
    g = torch.Generator().manual_seed(N)
    do = r16(torch.randn(1, N, Cc, generator=g, dtype=F64))
    do_d = do.to(dev(), BF)
    delta = torch.empty(2, 1, heads, N, dtype=torch.float32, device=dev())
    dqkv = torch.empty_like(qkv_d)
    L.check(lib.tv_attn_bwd(p(qkv_d), p(o), p(do_d), p(lse), p(delta), None, p(dqkv), 1, N, heads, 0.125, stream), "tv_attn_bwd")
    if rope:      # the production form (fused.AttnBranchFn): same rotated q, k; the RoPE adjoint applied in the dq / dk stores
        delta_t = torch.empty_like(delta)
        dqkv_t = torch.empty_like(qkv_d)
        L.check(lib.tv_attn_bwd(p(qkv_d), p(o), p(do_d), p(lse), p(delta_t), p(tab), p(dqkv_t), 1, N, heads, 0.125, stream), "tv_attn_bwd")
    torch.cuda.synchronize()
    qkv_h, o_h, lse_h, dl_h, dqkv_h = qkv_d.cpu().to(F64)[0], o.cpu().to(F64)[0], lse.cpu().to(F64)[0], delta.cpu().to(F64), dqkv.cpu().to(F64)[0]
    kb = 32 if N >= 2048 else 64
    res = {}
    for h in range(heads):
        cs = slice(h * 64, h * 64 + 64)
        q, k, v = qkv_h[:, cs], qkv_h[:, Cc + h * 64:Cc + h * 64 + 64], qkv_h[:, 2 * Cc + h * 64:2 * Cc + h * 64 + 64]
        o_ex, lse_ex = attn_exact(q, k, v, 0.125)
        grp = _sample_groups(N, 12)
        rows = torch.cat([torch.arange(g0 * 32, min(N, g0 * 32 + 32)) for g0 in grp])
        o_e = torch.empty(0, 64, dtype=F64)
        for g0 in grp:
            r0, r1 = g0 * 32, min(N, g0 * 32 + 32)
            # a wave's rows are independent of the other waves: emulate it on its own (keys: all of them)
            oo, _ = attn_fwd_emul(q[r0:r1], k, v, 0.125, kblock=kb, group=32)
            o_e = torch.cat([o_e, oo])
        res[f"o h{h}"] = check_vs_emulation(o_h[rows, cs], o_e, o_ex[rows], f"o head {h}")
        res[f"lse h{h}"] = (check_fp32(lse_h[h], lse_ex, lse_terms(q, k, lse_ex, 0.125), LSE_C, f"lse head {h}"),)
        dox = do[0, :, cs].to(F64)
        d64 = (dox * o_h[:, cs]).sum(1)
        res[f"delta h{h}"] = (check_fp32(-dl_h[0, 0, h], d64, (dox * o_h[:, cs]).abs().sum(1), 16.0, f"delta head {h}"),)
        ex = attn_bwd_exact(q, k, v, o_h[:, cs], dox, lse_h[h], 0.125)
        em = attn_bwd_emul(q, k, v, o_h[:, cs], dox, lse_h[h], 0.125)
        got = (dqkv_h[:, cs], dqkv_h[:, Cc + h * 64:Cc + h * 64 + 64], dqkv_h[:, 2 * Cc + h * 64:2 * Cc + h * 64 + 64])
        # (with RoPE: q, k are the rotated bf16 values the kernels read back from qkv; dq, dk are in that frame -- ops applies
        # the adjoint rotation after tv_attn_bwd)
        for i, nm in enumerate(("dq", "dk", "dv")):
            res[f"{nm} h{h}"] = check_vs_emulation(got[i], em[i], ex[i], f"{nm} head {h}")
        if rope:
            tab64, dt = tab.cpu().to(F64), dqkv_t.cpu().to(F64)[0]
            ex_t = attn_bwd_exact(q, k, v, o_h[:, cs], dox, lse_h[h], 0.125, tab=tab64)
            em_t = attn_bwd_emul(q, k, v, o_h[:, cs], dox, lse_h[h], 0.125, tab=tab64)
            got_t = (dt[:, cs], dt[:, Cc + h * 64:Cc + h * 64 + 64], dt[:, 2 * Cc + h * 64:2 * Cc + h * 64 + 64])
            for i, nm in enumerate(("dq", "dk")):
                res[f"{nm}+adjoint h{h}"] = check_vs_emulation(got_t[i], em_t[i], ex_t[i], f"{nm} with the adjoint in the store, head {h}")
            assert torch.equal(got_t[2], got[2]), f"dv head {h} changes with the table"
            assert torch.equal(delta_t.cpu(), delta.cpu()), "delta changes with the table"
    report(f"[A] {case} (relL2 ratio, max ratio)", {k: tuple(round(v, 3) for v in t) for k, t in res.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# [N] GroupNorm + SiLU and the row norms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,G", [(2, 1024, 128, 32), (3, 640, 192, 32)])
def test_groupnorm_silu(B, HW, C, G):
    """[N] forward: one rounding of silu(x sc + sh) (z in fp32 from x and the fp32 scale / shift); backward: dx one
    rounding, dgamma / dbeta fp32 sums; means up to 100 std, stds 1e-2 .. 1e2"""
    from transvae.hip import ops
    x, gamma, beta = gn_inputs(B, HW, C, G, seed=B * C)
    H = 32
    gy = r16(torch.randn(B, HW, C, generator=torch.Generator().manual_seed(2), dtype=F64))
    xd = x.view(B, H, HW // H, C).to(dev(), BF).contiguous().requires_grad_(True)
    gd = gamma.float().to(dev()).requires_grad_(True)
    bd = beta.float().to(dev()).requires_grad_(True)
    y = ops.group_norm_silu(xd, gd, bd, G)
    y.backward(gy.view(B, H, HW // H, C).to(dev(), BF))
    torch.cuda.synchronize()
    y64, slack, *_ = gn_silu64(x, gamma, beta, G)
    out = {"y": check_one_rounding(y.cpu().view(B, HW, C), y64, slack, "GroupNorm + SiLU forward")}
    dx64, dsl, dg64, db64, pterms = gn_bwd64(x, gamma, beta, gy, None, G)      # the fp64 backward and its slacks
    out["dx"] = check_one_rounding(xd.grad.cpu().view(B, HW, C), dx64, dsl, "GroupNorm + SiLU dx")
    out["dgamma"] = (check_fp32(gd.grad.cpu(), dg64, pterms, 64.0, "dgamma"),)
    out["dbeta"] = (check_fp32(bd.grad.cpu(), db64, pterms, 64.0, "dbeta"),)
    report(f"[N] GroupNorm {B}x{HW}x{C}/{G}", {k: tuple(round(v, 3) for v in t) for k, t in out.items()})


# the production path: fused.gn_silu_fwd / gn_silu_apply / gn_silu_bwd, the calls of fused.ResBlockFn.
# What the inputs make visible (norm.hip): dres added after the bf16 rounding -- rownorm_dres cancels dx on even pixels, so the
# second rounding is taken at dx's magnitude and read at the sum's (the host mutation `dres_after`); a FROM_MR kernel whose sc
# is not gn_prepare's expression -- the bit-equality of gn_silu_apply, plain and NT; a pixel loop without its `min(hw, ...)` --
# every B > 1 case with hw % 512 != 0 pulls the next image's pixels into the statistics / the backward sums, and the guarded
# buffers of test_groupnorm_stays_inside_a_ragged_last_slab show the stray stores; `(chunk * 8) / cpg` as a channel's group --
# wrong statistics for part of every 8-vector unless cpg is a multiple of 8 (cpg = 1, 2, 6, 10, 12, 24 here).
GN_PROD_CASES = [
    # B, HW, C, G                thread geometry: nch = C / 8 threads per pixel, rows = 256 / nch pixel lanes, slabs of 512 pixels
    (1, 1, 32, 32),            # cpg 1 (Chan's merge of one channel), a single pixel, var 0, 63 of 64 lanes without a pixel
    (2, 3, 1536, 32),          # rows 1, 64 idle threads, hw < 512
    (3, 513, 2048, 32),        # the C limit, a second slab of one pixel
    (2, 512, 768, 32),         # exactly one slab
    (3, 511, 320, 32),         # cpg 10, 16 idle threads
    (2, 1537, 384, 32),        # a ragged fourth slab
    (2, 4103, 192, 32),        # cpg 6: 8-vectors straddle groups; 9 slabs, 16 idle threads
    (1, 65536, 64, 32),        # 128 partials through gn_finalize_kernel
    (2, 700, 64, 1),           # one group for all channels
    (2, 700, 64, 8),           # C / 8 groups: one per vector
]


def _gn_prod_run(x, gamma, beta, gy, dres_list, G, eps=1e-5):
    """fused.gn_silu_fwd, gn_silu_apply and gn_silu_bwd once per entry of dres_list (None or a [B, HW, C] tensor) ->
    (mr, y, y of the apply, [(dx, dgamma, dbeta), ...]) on the host"""
    from transvae.hip import fused
    B, HW, C = x.shape
    up = lambda t: t.view(B, 1, HW, C).to(dev(), BF).contiguous()
    xd, gyd = up(x), up(gy)
    gd, bd = gamma.float().to(dev()), beta.float().to(dev())
    y, mr = fused.gn_silu_fwd(xd, gd, bd, G, eps)
    y2 = fused.gn_silu_apply(xd, mr, gd, bd, G)
    outs = [fused.gn_silu_bwd(xd, gyd, None if dr is None else up(dr), mr, gd, bd, G) for dr in dres_list]
    torch.cuda.synchronize()
    return mr.cpu(), y.cpu().view(B, HW, C), y2.cpu().view(B, HW, C), [(a.cpu().view(B, HW, C), b.cpu(), c.cpu()) for a, b, c in outs]


def _gn_prod_check(shape, k, tag):
    """one production-path case at pivot offset k: every assertion of test_groupnorm_production_path -> the y error in ulps"""
    B, HW, C, G = shape
    case = gn_case(shape, k)
    x, gamma, beta, gy, dres = case[:5]
    mr, y, y2, runs = _gn_prod_run(x, gamma, beta, gy, [None, dres, torch.zeros_like(dres)], G)
    mr_b, y_b, y2_b, runs_b = _gn_prod_run(x, gamma, beta, gy, [None], G)
    assert bool(torch.isfinite(y.float()).all()) and all(bool(torch.isfinite(r[0].float()).all()) for r in runs)
    out = gn_check_all(case, shape, dict(mr=mr, y=y, dx=runs[0][0], dgamma=runs[0][1], dbeta=runs[0][2]), dict(dx=runs[1][0]), tag, bias=(k == 0))
    report(f"[N] production GroupNorm {tag} (ratio, max ulps, bias)", out)
    assert torch.equal(y2, y), f"{tag}: gn_silu_apply differs from gn_silu_fwd in {int((y2 != y).sum())} elements"
    assert torch.equal(runs[2][0], runs[0][0]), f"{tag}: an all-zero dres changes dx"
    assert torch.equal(mr_b, mr) and torch.equal(y_b, y) and torch.equal(y2_b, y), f"{tag}: the forward is not bit-reproducible"
    assert torch.equal(runs_b[0][0], runs[0][0]), f"{tag}: dx is not bit-reproducible"
    y64 = case[5][0]
    return ((y.to(F64) - y64).abs() / ulp16(y64)).max().item()


@pytest.mark.parametrize("shape", GN_PROD_CASES, ids=lambda s: "x".join(map(str, s[:3])) + f"-G{s[3]}")
def test_groupnorm_production_path(shape):
    """[N] the three calls fused.ResBlockFn makes, over the thread geometries of GN_PROD_CASES: mean / rstd inside the bound
    about the pivot; y one rounding; gn_silu_apply (the FROM_MR recompute) bit-equal to the forward's y; dx one rounding
    without dres, with a dres of dx's own magnitude that partly cancels it (rownorm_dres) and bit-equal under an all-zero
    dres; dgamma / dbeta fp32 sums at c = max(64, k_g); forward and dx bit-identical over two runs."""
    _gn_prod_check(shape, 0, "x".join(map(str, shape)))


@pytest.mark.parametrize("shape", [(2, 4096, 192, 32), (1, 65536, 64, 32)], ids=lambda s: "x".join(map(str, s[:3])))
def test_groupnorm_pivot_outlier(shape):
    """[N] pixel 0 of every channel -- the pivot of gn_stats_kernel -- 0, 8 and 64 group-sigma from the group mean: the sums
    about it lose accuracy as dm^2 / var grows, which the bounds carry (gn_stats64).  Same assertions as the production-path
    test (the rounding-bias figure is asserted at offset 0 only, see gn_check_all); the absolute y error in bf16 ulps is
    printed per offset."""
    for k in (0, 8, 64):
        ulps = _gn_prod_check(shape, k, "x".join(map(str, shape)) + f" pivot +{k} sigma")
        report(f"[N] GroupNorm {shape} pivot +{k} sigma, max |y - y64| in bf16 ulps", round(ulps, 3))


def test_groupnorm_accumulates_parameter_gradients():
    """[N] tv_gn_silu_bwd_apply ADDS into dgamma / dbeta (atomics): on top of a running sum N(0, 4) the result is the sum plus
    the fp64 gradient within the fp32 bound, terms + |base| (the third run of test_rms_ln_hat)"""
    import ctypes as C
    from transvae.hip import _lib as L, fused
    lib = L.load()
    shape = (3, 511, 320, 32)
    B, HW, Cc, G = shape
    case = gn_case(shape, 0)
    x, gamma, beta, gy, dres = case[:5]
    dx64, dsl, dg64, db64, pterms = case[7]
    g = torch.Generator().manual_seed(5)
    base_g, base_b = f32(torch.randn(Cc, generator=g, dtype=F64) * 2), f32(torch.randn(Cc, generator=g, dtype=F64) * 2)
    up = lambda t: t.view(B, 1, HW, Cc).to(dev(), BF).contiguous()
    xd, gyd, rd = up(x), up(gy), up(dres)
    gd, bd = gamma.float().to(dev()), beta.float().to(dev())
    _, mr = fused.gn_silu_fwd(xd, gd, bd, G, 1e-5)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    red = torch.empty((B, Cc, 2), dtype=torch.float32, device=dev())
    part = torch.empty((lib.tv_gn_partial_count(B, HW, Cc),), dtype=torch.float32, device=dev())
    dx = torch.empty_like(xd)
    dg, db = base_g.float().to(dev()).contiguous(), base_b.float().to(dev()).contiguous()
    L.check(lib.tv_gn_silu_bwd_reduce(p(xd), p(gyd), p(mr), p(gd), p(bd), p(red), p(part), B, HW, Cc, G, stream), "tv_gn_silu_bwd_reduce")
    L.check(lib.tv_gn_silu_bwd_apply(p(xd), p(gyd), p(rd), p(mr), p(red), p(gd), p(bd), p(dx), p(dg), p(db), B, HW, Cc, G, stream),
            "tv_gn_silu_bwd_apply")
    torch.cuda.synchronize()
    c = max(64.0, gn_k_g(HW, Cc, B))
    out = {"dx+dres": check_one_rounding(dx.cpu().view(B, HW, Cc), dx64, dsl, "dx + dres"),
           "dgamma": (check_fp32(dg.cpu(), base_g + dg64, pterms + base_g.abs(), c, "dgamma on a running sum"),),
           "dbeta": (check_fp32(db.cpu(), base_b + db64, pterms + base_b.abs(), c, "dbeta on a running sum"),)}
    report(f"[N] GroupNorm {shape} parameter gradients on a running sum", {k: tuple(round(v, 4) for v in t) for k, t in out.items()})


def test_groupnorm_nontemporal_instantiations_equal_the_plain_ones():
    """[N] B = 2, HW = 65 536, C = 512 is exactly 128 MiB: every launch takes the NT = true kernels (norm.hip gn_nt), while each
    image alone (64 MiB) takes the plain ones.  Images are independent and every reduction has a fixed order, so mr, y, the
    apply's y and dx (+ dres) of the pair are bit-equal to the two single-image runs, and dgamma / dbeta of the pair to the sum
    of the singles' (two addends from zero; addition commutes).  Everything stays on the device; the singles' mr is checked
    against fp64 statistics in plain torch there."""
    from transvae.hip import fused
    B, HW, C, G = 2, 65536, 512, 32
    assert B * HW * C * 2 == 128 << 20
    g = torch.Generator(device=dev()).manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev(), dtype=torch.float32)
    std = torch.exp2(4 * rnd(B, 1, G, 1))
    x = ((rnd(B, HW, G, C // G) + 10 * rnd(B, 1, G, 1)) * std).view(B, 1, HW, C).to(BF).contiguous()
    gy = rnd(B, 1, HW, C).to(BF)
    dres = (rnd(B, 1, HW, C) / std.expand(B, HW, G, C // G).reshape(B, 1, HW, C)).to(BF)      # the magnitude of dx ~ gy rstd
    gamma, beta = 1 + 0.2 * rnd(C), 0.2 * rnd(C)

    def run(xs, gs, ds):
        y, mr = fused.gn_silu_fwd(xs, gamma, beta, G, 1e-5)
        y2 = fused.gn_silu_apply(xs, mr, gamma, beta, G)
        dx, dg, db = fused.gn_silu_bwd(xs, gs, ds, mr, gamma, beta, G)
        return mr, y, y2, dx, dg, db
    pair = run(x, gy, dres)
    singles = [run(x[b:b + 1], gy[b:b + 1], dres[b:b + 1]) for b in range(B)]
    torch.cuda.synchronize()
    assert torch.equal(pair[2], pair[1]), "NT apply differs from the NT forward"
    for i, nm in enumerate(("mr", "y", "apply y", "dx + dres")):
        for b in range(B):
            assert x[b:b + 1].is_contiguous() and torch.equal(pair[i][b:b + 1], singles[b][i]), f"{nm} of image {b}: NT and plain kernels differ"
    for i, nm in ((4, "dgamma"), (5, "dbeta")):
        assert torch.equal(pair[i], singles[0][i] + singles[1][i]), f"{nm}: the pair is not the sum of the single images"
    assert bool(torch.isfinite(pair[3].float()).all()) and float(pair[3].float().abs().max()) > 0
    rat = [check_gn_stats(x[b].view(1, HW, C), G, singles[b][0], f"plain kernels, image {b}") for b in range(B)]
    report(f"[N] NT = plain at {B}x{HW}x{C}; single-image (mean, rstd) ratios", [tuple(round(v, 4) for v in r) for r in rat])


def test_groupnorm_stays_inside_a_ragged_last_slab():
    """[N] hw = 513: the second slab holds one pixel.  The five entry points run through ctypes on buffers that continue for
    511 more pixels -- inputs there hold large finite values, outputs a sentinel -- so a pixel loop that ran to the end of its
    slab instead of to hw would stay inside the allocations, change the statistics and overwrite the sentinel.  The results
    are bit-equal to the fused.* calls on the exact-size tensors and every sentinel is intact."""
    import ctypes as C
    from transvae.hip import _lib as L, fused
    lib = L.load()
    shape = (1, 513, 64, 32)
    B, HW, Cc, G = shape
    PAD = 1024
    x, gamma, beta, gy, dres = gn_case(shape, 0)[:5]

    def padded(t, fill):
        buf = torch.full((PAD, Cc), fill, dtype=BF, device=dev())
        if t is not None:
            buf[:HW] = t.view(HW, Cc).to(dev(), BF)
        return buf
    xd, gyd, rd = padded(x, 3e4), padded(gy, 3e4), padded(dres, 3e4)
    y, y2, dx = padded(None, 768.0), padded(None, 768.0), padded(None, 768.0)
    gd, bd = gamma.float().to(dev()), beta.float().to(dev())
    f32buf = lambda *s: torch.empty(s, dtype=torch.float32, device=dev())
    stats, red, mr = f32buf(B, Cc, 2), f32buf(B, Cc, 2), f32buf(B, G, 2)
    part = f32buf(lib.tv_gn_partial_count(B, HW, Cc))
    dg, db = torch.zeros(Cc, device=dev()), torch.zeros(Cc, device=dev())
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.tv_gn_stats(p(xd), p(stats), p(part), B, HW, Cc, stream), "tv_gn_stats")
    L.check(lib.tv_gn_silu_fwd(p(xd), p(stats), p(gd), p(bd), p(mr), p(y), B, HW, Cc, G, 1e-5, stream), "tv_gn_silu_fwd")
    L.check(lib.tv_gn_silu_apply(p(xd), p(mr), p(gd), p(bd), p(y2), B, HW, Cc, G, stream), "tv_gn_silu_apply")
    L.check(lib.tv_gn_silu_bwd_reduce(p(xd), p(gyd), p(mr), p(gd), p(bd), p(red), p(part), B, HW, Cc, G, stream), "tv_gn_silu_bwd_reduce")
    L.check(lib.tv_gn_silu_bwd_apply(p(xd), p(gyd), p(rd), p(mr), p(red), p(gd), p(bd), p(dx), p(dg), p(db), B, HW, Cc, G, stream),
            "tv_gn_silu_bwd_apply")
    xe, gye, re_ = (t[:HW].clone().view(B, 1, HW, Cc) for t in (xd, gyd, rd))
    ye, mre = fused.gn_silu_fwd(xe, gd, bd, G, 1e-5)
    dxe, dge, dbe = fused.gn_silu_bwd(xe, gye, re_, mre, gd, bd, G)
    torch.cuda.synchronize()
    for nm, buf in (("y", y), ("apply y", y2), ("dx", dx)):
        assert bool((buf[HW:] == 768.0).all()), f"{nm}: stores past pixel hw - 1"
    assert torch.equal(mr, mre), "statistics read pixels past hw - 1"
    assert torch.equal(y[:HW], ye.view(HW, Cc)) and torch.equal(y2[:HW], ye.view(HW, Cc))
    assert torch.equal(dx[:HW], dxe.view(HW, Cc)) and torch.equal(dg, dge) and torch.equal(db, dbe), "backward sums read pixels past hw - 1"


@pytest.mark.parametrize("C,G", [(2056, 32), (36, 4), (64, 5)])
def test_groupnorm_rejects_bad_shapes(C, G):
    """[N] argument validation only: C > 2048 (more 8-vectors than threads), C % 8 != 0 and C % G != 0 raise through L.check
    with gn_check's message from every entry point, before any launch"""
    from transvae.hip import fused
    x = torch.zeros(1, 2, 2, C, dtype=BF, device=dev())
    w = torch.ones(C, dtype=torch.float32, device=dev())
    mr = torch.zeros(1, G, 2, dtype=torch.float32, device=dev())
    for call in (lambda: fused.gn_silu_fwd(x, w, w, G, 1e-5), lambda: fused.gn_silu_apply(x, mr, w, w, G),
                 lambda: fused.gn_silu_bwd(x, x, None, mr, w, w, G)):
        with pytest.raises(RuntimeError, match=rf"bad shape batch=1 hw=4 C={C} G=\d+ \(C % 8 == 0, C % G == 0, C <= 2048 required\)"):
            call()
    torch.cuda.synchronize()


ROWNORM_LOOP = 8192 + 4 * 2048 + 13     # rows: the forward's 2048 blocks x 4 waves twice and a ragged third pass, the backward's
                                        # 1024 x 4 four times and a ragged fifth (norm.hip:345,405)


def _rownorm_run(x, w, gy, dres, mode, dw0=None):
    """tv_rownorm_fwd and tv_rownorm_bwd as fused.rownorm_fwd / rownorm_bwd launch them -> (y, dx, dw) on the host; dw starts
    from dw0 (zeros when None)"""
    import ctypes as C
    from transvae.hip import _lib as L
    lib = L.load()
    T, Cc = x.shape
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xd, gd = x.to(dev(), BF).contiguous(), gy.to(dev(), BF).contiguous()
    wd = w.float().to(dev()).contiguous() if mode == 1 else None
    rd = dres.to(dev(), BF).contiguous() if dres is not None else None
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    dw = None
    if mode == 1:
        dw = torch.zeros(Cc, dtype=torch.float32, device=dev()) if dw0 is None else dw0.float().to(dev()).contiguous()
    L.check(lib.tv_rownorm_fwd(p(xd), p(wd), p(y), T, Cc, mode, EPS_RMS, EPS_LN, stream), "tv_rownorm_fwd")
    L.check(lib.tv_rownorm_bwd(p(xd), p(wd), p(gd), p(rd), p(dx), p(dw), T, Cc, mode, EPS_RMS, EPS_LN, stream), "tv_rownorm_bwd")
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu(), None if dw is None else dw.cpu()


@pytest.mark.parametrize("T,Cc", [(300, 384), (2048 + 40, 768), (40, 1536), (64, 2048), (9, 2560), (ROWNORM_LOOP, 384)])
def test_rms_ln_hat(T, Cc):
    """[N] mode 1 (RMSNorm x weight, then the affine-free LayerNorm), the norm of fused.AttnBranchFn: y one rounding; dx one
    rounding without and with the fused residual gradient; dw fp32 by atomics, three runs (from zero twice, once on top of
    a running sum).  |mean u| / std u up to 100, an all-zero and a constant row; every per-lane chunk count (C = 384 .. 2560)
    and the row loop of both kernels taken more than once with a ragged last pass."""
    x, w, gy = rms_ln_inputs(T, Cc, seed=T + Cc)
    y64, u, mu, s, _ = rms_ln_hat64(x, w)
    dres = rownorm_dres(rownorm_bwd64(x, w, gy, None, 1)[0], seed=T)
    base = f32(torch.randn(Cc, generator=torch.Generator().manual_seed(5), dtype=F64) * 4)
    out = {}
    for tag, dr, dw0 in (("", None, None), ("+dres", dres, None), ("+dres, running dw", dres, base)):
        y, dx, dw = _rownorm_run(x, w, gy, dr, 1, dw0)
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
        dx64, dsl, dw64, dwt = rownorm_bwd64(x, w, gy, dr, 1)
        if not tag:
            out["y"] = check_one_rounding(y, y64, rms_ln_slack(y64, u, mu, s), "rms_ln_hat")
        out["dx" + tag] = check_one_rounding(dx, dx64, dsl, "rms_ln_hat dx" + tag)
        if dw0 is None:
            out["dw" + tag] = (check_fp32(dw, dw64, dwt, ROWNORM_C_DW, "rms_ln_hat dw" + tag),)
        else:
            out["dw" + tag] = (check_fp32(dw, dw0 + dw64, dwt + dw0.abs(), ROWNORM_C_DW, "rms_ln_hat dw" + tag),)
    report(f"[N] rms_ln_hat {T}x{Cc} (ratio, max ulps, bias)", {k: tuple(round(v, 3) for v in t) for k, t in out.items()})


@pytest.mark.parametrize("T,Cc", [(300, 384), (2048 + 40, 768), (40, 1536), (ROWNORM_LOOP, 384)])
def test_rms_hat(T, Cc):
    """[N] rms_hat: y = x rsqrt(mean x^2 + eps) one rounding (2^-20 |y| for the fp32 sum and rsqrt); dx = r (g - xhat
    mean(g xhat)) one rounding (2^-19 of the terms), and the same with the fused residual gradient as fused.ConvFFNBranchFn
    passes it (+ 2^-24 |dres|)"""
    from transvae.hip import ops
    g = torch.Generator().manual_seed(T)
    rs = torch.exp2(torch.randint(-6, 7, (T, 1), generator=g).to(F64))
    x = r16(torch.randn(T, Cc, generator=g, dtype=F64) * rs)
    gy = r16(torch.randn(T, Cc, generator=g, dtype=F64))
    xd = x.to(dev(), BF).requires_grad_(True)
    y = ops.rms_hat(xd)
    y.backward(gy.to(dev(), BF))
    torch.cuda.synchronize()
    r = 1.0 / torch.sqrt((x * x).mean(1, keepdim=True) + 1e-6)
    y64 = x * r
    out = {"y": check_one_rounding(y.cpu(), y64, 2.0 ** -20 * y64.abs(), "rms_hat")}
    m = (gy * y64).mean(1, keepdim=True)
    dx64 = r * (gy - y64 * m)
    terms = r * (gy.abs() + y64.abs() * (gy * y64).abs().mean(1, keepdim=True))
    out["dx"] = check_one_rounding(xd.grad.cpu(), dx64, 2.0 ** -19 * terms, "rms_hat dx")
    dres = rownorm_dres(dx64, seed=T)
    y2, dx2, _ = _rownorm_run(x, None, gy, dres, 0)
    assert torch.equal(y2, y.detach().cpu())
    out["dx+dres"] = check_one_rounding(dx2, dx64 + dres, 2.0 ** -19 * terms + 2.0 ** -24 * dres.abs(), "rms_hat dx + dres")
    report(f"[N] rms_hat {T}x{Cc}", {k: tuple(round(v, 3) for v in t) for k, t in out.items()})
