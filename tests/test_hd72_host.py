"""DESIGN.md section 3.1 row Y on the host: the emulations of the head_dim 72 kernels (tests/hd72_restatement.py) sit inside the
bounds the GPU tests hold the kernels to, the named defects are rejected by the same checks, tau is calibrated at D = 72, and the
XL constructors build what they say."""
import math

import pytest
import torch

import hd72_restatement as H
from test_dit_host import U, check_report, fp32_ratio
from test_error_budget_host import (LSE_C, TAU, attn_bwd_emul, attn_exact, attn_fwd_emul, check_fp32, check_one_rounding, check_vs_emulation,
                                    lse_terms, one_rounding_report, r16, rel_l2)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HD = H.HD
HOST_SHAPES = [s for s in H.SHAPES if s != (1, 1024, 1)] + [(1, 320, 1)]      # (the long spiked case runs on the device; 320 = five key blocks here)


def slice_of(B, N, heads, seed, b=0, h=0, **kw):
    """(q, k, v, do, table | None) of one (image, head) slice"""
    qkv, do = H.attn_inputs(B, N, heads, seed, **kw)
    return tuple(qkv[b, :, i, h] for i in range(3)) + (do[b, :, h], H.table_of(N) if N in H.GRIDS else None)


# ---------------------------------------------------------------------------------------------------------------------------
# emulations inside the bounds
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,heads", HOST_SHAPES)
def test_attention_emulations_sit_inside_the_bounds(B, N, heads):
    q, k, v, do, tab = slice_of(B, N, heads, seed=B + N + heads, b=B - 1, h=heads - 1)
    o_ex, lse_ex = attn_exact(q, k, v, H.SCALE)
    o_e, lse_e = attn_fwd_emul(q, k, v, H.SCALE)
    check_vs_emulation(o_e, o_e, o_ex, "o")
    check_fp32(lse_e, lse_ex, lse_terms(q, k, lse_ex, H.SCALE), LSE_C, "lse")
    if N >= 128:        # the reordered emulation is inside the rule as well
        nb = -(-N // 64)
        o_r, _ = attn_fwd_emul(q, k, v, H.SCALE, order=list(reversed(range(nb))))
        check_vs_emulation(o_r, o_e, o_ex, "o, key blocks reversed")
    for tb in (None, tab):
        ex = H.attn_bwd_exact(q, k, v, o_e, do, lse_e, H.SCALE, tab=tb)
        em = H.attn_bwd_emul(q, k, v, o_e, do, lse_e, H.SCALE, tab=tb)
        for i, nm in enumerate(("dq", "dk", "dv")):
            check_vs_emulation(em[i], em[i], ex[i], nm)
        check_fp32(em[3], ex[3], (do.to(F64) * o_e).abs().sum(1), float(H.K_DELTA), "delta")
        if tb is None:      # the project's D-generic emulation (delta as three bf16 pieces) is the same policy: inside the rule against this one
            old = attn_bwd_emul(q, k, v, o_e, do, lse_e, H.SCALE)
            for i, nm in enumerate(("dq", "dk", "dv")):
                if N >= 64:
                    check_vs_emulation(old[i], em[i], ex[i], nm + ", row A's emulation")


@pytest.mark.parametrize("B,N,heads", [s for s in HOST_SHAPES if s[1] in H.GRIDS and H.GRIDS[s[1]] is not None])
def test_rope_and_qknorm_emulations_sit_inside_the_bounds(B, N, heads):
    q = H.qk_inputs(B, N, heads, seed=B + N + heads)
    for kind in ("forward", "adjoint"):
        y64, slack = H.rope_qk64(q["qkv"], q["tab"], N, kind)
        check_report(one_rounding_report(H.rope_qk_emulate(q["qkv"], q["tab"], N, kind)[:, :2], y64[:, :2], slack[:, :2]), f"rope {kind}")
    for tab in (q["tab"], None):
        y64, slack = H.qknorm_fwd64(q["qkv"], q["wq"], q["wk"], tab, N)
        out = H.qknorm_fwd_emulate(q["qkv"], q["wq"], q["wk"], tab, N)
        check_report(one_rounding_report(out[:, :2], y64[:, :2], slack[:, :2]), "qknorm fwd")
        assert not bool(out[0, 0, 0].any()) and torch.equal(out[:, 2], q["qkv"][:, 2])
    ref = H.qknorm_bwd64(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    d, dwq, dwk = H.qknorm_bwd_emulate(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    check_report(one_rounding_report(d[:, :2], ref["dqkv"][:, :2], ref["slack"][:, :2]), "qknorm bwd")
    assert fp32_ratio(dwq, ref["dwq"], ref["dwq_bound"]) <= 1.0 and fp32_ratio(dwk, ref["dwk"], ref["dwk_bound"]) <= 1.0
    assert bool(torch.isfinite(d).all())


def test_head_sum_orders():
    """the addition counts written into row Y: 8 + 4 behind a qk-norm head sum (dead lanes add exact zeros), 8 + 8 behind delta"""
    assert H.K_HEAD == 12 and H.K_DELTA == 16
    x = torch.randn(5, 72, generator=torch.Generator().manual_seed(0))
    xl = H._lanes(x)
    assert xl.shape == (5, 16, 8) and not bool(xl[:, 9:].any()) and torch.equal(H._unlanes(xl), x)
    s = H._group_sum(H.LR._head_chain(xl, xl))
    assert float((s[:, 0].double() - (x.double() ** 2).sum(1)).abs().max()) <= 12 * U * float((x.double() ** 2).sum(1).max())


# ---------------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["mean64", "mean80"])
def test_qknorm_with_another_head_dimensions_mean_is_rejected(defect):
    B, N, heads = 3, 65, 2
    q = H.qk_inputs(B, N, heads, seed=1)
    y64, slack = H.qknorm_fwd64(q["qkv"], q["wq"], q["wk"], q["tab"], N)
    rep = one_rounding_report(H.qknorm_fwd_emulate(q["qkv"], q["wq"], q["wk"], q["tab"], N, defect=defect)[:, :2], y64[:, :2], slack[:, :2])
    assert rep[0] > 1.0, rep
    ref = H.qknorm_bwd64(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    d, _, _ = H.qknorm_bwd_emulate(q["qkv"], q["wq"], q["wk"], q["dqkv"], defect=defect)
    assert one_rounding_report(d[:, :2], ref["dqkv"][:, :2], ref["slack"][:, :2])[0] > 1.0


def test_pad_columns_from_the_next_head_are_rejected():
    """q.k summed over 80 with columns 72..79 taken from the next head's first piece (a pad loaded, not made)"""
    B, N, heads = 1, 256, 2
    qkv, _ = H.attn_inputs(B, N, heads, seed=2)
    q, k, v = (qkv[0, :, i, 0] for i in range(3))
    q80, k80 = torch.cat([q, qkv[0, :, 0, 1, :8]], 1), torch.cat([k, qkv[0, :, 1, 1, :8]], 1)
    o_ex, lse_ex = attn_exact(q, k, v, H.SCALE)
    o_e, _ = attn_fwd_emul(q, k, v, H.SCALE)
    o_bad, lse_bad = attn_fwd_emul(q80, k80, v, H.SCALE)
    with pytest.raises(AssertionError):
        check_vs_emulation(o_bad, o_e, o_ex, "pad from the next head")
    with pytest.raises(AssertionError):
        check_fp32(lse_bad, lse_ex, lse_terms(q, k, lse_ex, H.SCALE), LSE_C, "lse, pad from the next head")


def test_table_read_with_the_64_layout_is_rejected():
    B, N, heads = 3, 65, 2
    q = H.qk_inputs(B, N, heads, seed=3)
    y64, slack = H.rope_qk64(q["qkv"], q["tab"], N)
    assert one_rounding_report(H.rope_qk_emulate(q["qkv"], q["tab"], N, defect="stride32")[:, :2], y64[:, :2], slack[:, :2])[0] > 1.0
    qv, k, v, do, tab = slice_of(1, 256, 1, seed=4)
    o, lse = attn_fwd_emul(qv, k, v, H.SCALE)
    ex = H.attn_bwd_exact(qv, k, v, o, do, lse, H.SCALE, tab=tab)
    clean = H.attn_bwd_emul(qv, k, v, o, do, lse, H.SCALE, tab=tab)
    bad = H.attn_bwd_emul(qv, k, v, o, do, lse, H.SCALE, tab=tab, mutate="rope_stride32")
    for i, nm in ((0, "dq"), (1, "dk")):
        with pytest.raises(AssertionError):
            check_vs_emulation(bad[i], clean[i], ex[i], nm)


def test_adjoint_after_the_rounding_is_rejected():
    """dq / dk rounded to bf16, rotated, rounded again.  Row A's relL2 rule straddles tau for this defect at head_dim 64
    (tests/test_error_budget_host.py says why); what rejects it is the one-rounding rule on the store itself: the stored value
    against the fp64 adjoint of the scaled fp32 sums the store starts from, slack = the fp32 arithmetic of the 2x2."""
    q, k, v, do, tab = slice_of(1, 256, 1, seed=5)
    o, lse = attn_fwd_emul(q, k, v, H.SCALE)
    rows = torch.arange(256)
    clean = H.attn_bwd_emul(q, k, v, o, do, lse, H.SCALE, tab=tab, sums=True)
    bad = H.attn_bwd_emul(q, k, v, o, do, lse, H.SCALE, tab=tab, mutate="rope_after", sums=True)
    for i, nm in ((0, "dq"), (1, "dk")):
        y64 = H.rope_pairs(clean[4 + i], tab, rows, "adjoint")
        slack = U * H.rope_terms(clean[4 + i], tab, rows, "adjoint") + U * y64.abs()
        check_one_rounding(clean[i], y64, slack, nm)
        with pytest.raises(AssertionError):
            check_one_rounding(bad[i], y64, slack, nm + ", adjoint after the rounding")


def test_p_rounded_twice_is_rejected():
    qkv, _ = H.attn_inputs(1, 256, 1, seed=6, qk_scale=0.5)         # flat score rows: P's rounding is a visible part of the error
    q, k, v = (qkv[0, :, i, 0] for i in range(3))
    o_ex, _ = attn_exact(q, k, v, H.SCALE)
    o_e, _ = attn_fwd_emul(q, k, v, H.SCALE)
    o_bad, _ = attn_fwd_emul(q, k, v, H.SCALE, mutate="p2")
    with pytest.raises(AssertionError):
        check_vs_emulation(o_bad, o_e, o_ex, "P rounded twice")


def test_tau_calibration_from_two_orderings_at_72():
    """The project's calibration repeated at D = 72: two ideal emulations that differ only in key-block order stay within the relL2
    ratio that TAU = 1.2 leaves room for (the D = 64 calibration measured at most 1.04 and asserts 1.08)."""
    worst = 0.0
    for N, kb, seed in ((256, 64, 1), (300, 64, 2), (512, 32, 3)):
        g = torch.Generator().manual_seed(seed)
        q, k = (r16(torch.randn(N, HD, generator=g, dtype=F64) * 1.5) for _ in range(2))
        v = r16((4.0 if seed == 2 else 0.0) + (0.25 if seed == 2 else 1.0) * torch.randn(N, HD, generator=g, dtype=F64))
        k[N // 2 + 3] = r16(q[5] * 3.0)
        o_ex, _ = attn_exact(q, k, v, H.SCALE)
        nb = -(-N // kb)
        o_a, _ = attn_fwd_emul(q, k, v, H.SCALE, kblock=kb)
        o_b, _ = attn_fwd_emul(q, k, v, H.SCALE, kblock=kb, order=list(reversed(range(nb))))
        ea, eb = rel_l2(o_a, o_ex), rel_l2(o_b, o_ex)
        worst = max(worst, ea / eb, eb / ea)
        check_vs_emulation(o_b, o_a, o_ex, f"reordered N={N}")
    print(f"[error-budget] tau calibration at D = 72: worst ratio {worst:.4f}")
    assert worst <= 1.08 < TAU, worst


# ---------------------------------------------------------------------------------------------------------------------------
# constructors
# ---------------------------------------------------------------------------------------------------------------------------
def dit_params(C, depth, cols, classes, freq=256):
    lin = lambda i, o: i * o + o
    block = lin(C, 3 * C) + lin(C, C) + lin(C, 4 * C) + lin(4 * C, C) + lin(C, 6 * C)
    return lin(cols, C) + lin(freq, C) + lin(C, C) + (classes + 1) * C + depth * block + lin(C, cols) + lin(C, 2 * C)


def lightning_params(C, depth, cols, classes, hd, freq=256):
    lin = lambda i, o: i * o + o
    H_ = (2 * 4 * C) // 3
    block = C + lin(C, 3 * C) + 2 * hd + lin(C, C) + C + lin(C, 2 * H_) + lin(H_, C) + lin(C, 6 * C)
    return lin(cols, C) + lin(freq, C) + lin(C, C) + (classes + 1) * C + depth * block + C + lin(C, cols) + lin(C, 2 * C)


def test_xl_constructors():
    import transvae
    from transvae import dit as D, lightning_dit as LD
    with torch.device("meta"):
        a, b = transvae.dit_xl(), transvae.lightning_dit_xl()
    for m in (a, b):
        assert (m.hidden_size, m.depth, m.num_heads, m.head_dim) == (1152, 28, 16, 72) and m.attn_scale == 72 ** -0.5
    assert list(a.state_dict()) == D.state_dict_keys(28) and list(b.state_dict()) == LD.state_dict_keys(28)
    assert tuple(b.blocks[0].attn.q_norm.weight.shape) == (72,) and tuple(b.blocks[27].attn.k_norm.weight.shape) == (72,)
    assert sum(p.numel() for p in a.parameters()) == dit_params(1152, 28, 32, 1000)
    assert sum(p.numel() for p in b.parameters()) == lightning_params(1152, 28, 32, 1000, 72)
    assert LD.swiglu_inner(1152, 4.0) == 3072
    for name in ("dit_xl", "lightning_dit_xl"):
        assert name in transvae.__all__


def test_head_dim_keyword():
    import transvae
    from transvae.modules.attention import RoPE2D
    assert transvae.DiT(8, 1, 32, 288, 2, 10, head_dim=72).num_heads == 4
    assert transvae.LightningDiT(8, 1, 32, 288, 1, 10, head_dim=72).blocks[0].attn.q_norm.weight.shape == (72,)
    for cls in (transvae.DiT, transvae.LightningDiT):
        with pytest.raises(ValueError, match="head_dim"):
            cls(8, 1, 32, 320, 1, 10, head_dim=80)
        with pytest.raises(ValueError, match="head_dim"):
            cls(8, 1, 32, 1184, 1, 10, head_dim=72)
    m = transvae.DiT(hidden_size=1152, depth=1)
    assert m.num_heads == 18 and m.head_dim == 64 and m.attn_scale == 0.125
    assert tuple(RoPE2D(72).table(2, 3).shape) == (6, 4, 36)
    assert torch.equal(RoPE2D(72).table(5, 13), H.rope_table(5, 13))


def test_wrappers_take_head_dim_explicitly():
    from transvae.hip import ops
    from transvae import lightning_dit as LD
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention(torch.zeros(1, 4, 216, dtype=BF), None, 1, 0.1, head_dim=72)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LD.qk_norm_rope_attention(torch.zeros(1, 4, 216, dtype=BF), torch.ones(72), torch.ones(72), None, 1, 0.1, head_dim=72)
    with pytest.raises(RuntimeError, match="head_dim"):
        LD.qk_norm_rope_attention(torch.zeros(1, 4, 240, dtype=BF), torch.ones(80), torch.ones(80), None, 1, 0.1, head_dim=80)
