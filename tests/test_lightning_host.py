"""transvae/lightning_dit.py and csrc/lightning.hip without a GPU: the bounds of DESIGN.md section 3.1 row J validated against fp32
emulations in the kernels' own order of operations (never against a kernel), the mutations those bounds must reject, the exact
cases, the host logic (state-dict keys, presets, the SwiGLU width, argument validation) and the golden file of the restatement's
own bf16-autocast deviation."""
import json

import pytest
import torch

import lightning_restatement as LR
from test_dit_host import U, check_report, fp32_ratio, sl
from test_error_budget_host import F64, one_rounding_report

BF = torch.bfloat16


def rms_fwd_report(inp, N, defect=None):
    y64, slack = LR.adaln_rms_fwd64(inp["x"], inp["w"], sl(inp, "shift_off"), sl(inp, "scale_off"), N)
    return one_rounding_report(LR.adaln_rms_fwd_emulate(inp["x"], inp["w"], sl(inp, "shift_off"), sl(inp, "scale_off"), N, defect), y64, slack)


def rms_bwd_ratios(inp, N, with_dres, defect=None):
    dres = inp["dres"] if with_dres else None
    ref = LR.adaln_rms_bwd64(inp["x"], inp["w"], sl(inp, "scale_off"), inp["dy"], dres, N)
    dx, dshift, dscale, dw = LR.adaln_rms_bwd_emulate(inp["x"], inp["w"], sl(inp, "scale_off"), inp["dy"], dres, N, defect)
    return {"dx": one_rounding_report(dx, ref["dx"], ref["dx_slack"]),
            "dshift": fp32_ratio(dshift, ref["dshift"], ref["k_rows"] * U * ref["dshift_terms"]),
            "dscale": fp32_ratio(dscale, ref["dscale"], ref["dscale_bound"]),
            "dw": fp32_ratio(dw, ref["dw"], ref["dw_bound"])}


def qk_fwd_report(q, N, with_tab, defect=None):
    tab = q["tab"] if with_tab else None
    y64, slack = LR.qknorm_fwd64(q["qkv"], q["wq"], q["wk"], tab, N)
    y = LR.qknorm_fwd_emulate(q["qkv"], q["wq"], q["wk"], tab, N, defect)
    return one_rounding_report(y[:, :2], y64[:, :2], slack[:, :2]), y


def qk_bwd_ratios(q):
    ref = LR.qknorm_bwd64(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    d, dwq, dwk = LR.qknorm_bwd_emulate(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    return {"dqk": one_rounding_report(d[:, :2], ref["dqkv"][:, :2], ref["slack"][:, :2]), "dv_equal": torch.equal(d[:, 2], q["dqkv"][:, 2]),
            "dwq": fp32_ratio(dwq, ref["dwq"], ref["dwq_bound"]), "dwk": fp32_ratio(dwk, ref["dwk"], ref["dwk_bound"])}


def swiglu_reports(s, defect=None):
    h64, hs = LR.swiglu_fwd64(s["u"])
    d64, ds = LR.swiglu_bwd64(s["u"], s["dh"])
    h, du = LR.swiglu_fwd_emulate(s["u"], defect), LR.swiglu_bwd_emulate(s["u"], s["dh"], defect)
    return one_rounding_report(h, h64, hs), one_rounding_report(du, d64, ds), h, du


def check_swiglu_exact(s, h, du):
    """row 0, columns 0 .. 3 hold x1 = 0, 3e38, -3e38, -100 with x2 = 0.5 and dh = 0.25; the last `pad` columns are zero operands"""
    Hp = h.shape[1]
    hf, d1, d2 = h[0, :4].float(), du[0, :4].float(), du[0, Hp:Hp + 4].float()
    x = torch.tensor(LR.SWIGLU_EDGE).to(BF).float()
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(du).all())
    assert hf[0] == 0 and d2[0] == 0 and d1[0] == torch.tensor(0.25 * 0.5 * 0.5).to(BF).float(), "x1 = 0: silu = 0, silu' = 1 / 2"
    assert hf[1] == (x[1] * 0.5).to(BF).float() and d1[1] == 0.125 and d2[1] == (0.25 * x[1]).to(BF).float(), "x1 = 3e38: silu = x1, silu' = 1"
    for j in (2, 3):
        assert hf[j] == 0 and d1[j] == 0 and d2[j] == 0, "x1 = -3e38, -100: silu = -0, silu' = -0"
    assert not bool(h[:, Hp - s["pad"]:].any()), "zero operands give exactly 0"
    assert not bool(du[:, Hp - s["pad"]:Hp].any()) and not bool(du[:, 2 * Hp - s["pad"]:].any())


# ---------------------------------------------------------------------------------------------------------------------------
# emulations inside the bounds
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", LR.ROW_SHAPES)
def test_rms_adaln_emulations_sit_inside_the_bounds(B, N, C):
    inp = LR.row_inputs(B, N, C, seed=B + N + C)
    check_report(rms_fwd_report(inp, N), "adaln_rms_fwd")
    for with_dres in (False, True):
        r = rms_bwd_ratios(inp, N, with_dres)
        check_report(r["dx"], f"adaln_rms_bwd dx (dres={with_dres})")
        assert r["dshift"] <= 1.0 and r["dscale"] <= 1.0 and r["dw"] <= 1.0, r


@pytest.mark.parametrize("B,N,heads", LR.QK_SHAPES)
def test_qknorm_emulations_sit_inside_the_bounds(B, N, heads):
    q = LR.qk_inputs(B, N, heads, seed=B + N + heads)
    for with_tab in (True, False):
        rep, y = qk_fwd_report(q, N, with_tab)
        check_report(rep, f"qknorm_rope_fwd (table={with_tab})")
        assert torch.equal(y[:, 2], q["qkv"][:, 2]), "the v third"
    r = qk_bwd_ratios(q)
    check_report(r["dqk"], "qknorm_rope_bwd")
    assert r["dv_equal"] and r["dwq"] <= 1.0 and r["dwk"] <= 1.0, r


@pytest.mark.parametrize("T,Hp", LR.SWIGLU_SHAPES)
def test_swiglu_emulations_sit_inside_the_bounds(T, Hp):
    s = LR.swiglu_inputs(T, Hp, seed=T + Hp)
    rh, rd, h, du = swiglu_reports(s)
    check_report(rh, "swiglu_fwd")
    check_report(rd, "swiglu_bwd")
    check_swiglu_exact(s, h, du)


# ---------------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["stat_bf16", "mean_subtracted", "weight_after_mod", "neighbour_sample"])
def test_rms_adaln_fwd_bounds_reject(defect):
    B, N, C = 3, 65, 128
    inp = LR.row_inputs(B, N, C, seed=7)
    assert rms_fwd_report(inp, N)[0] <= 1.0
    ratio = rms_fwd_report(inp, N, defect)[0]
    print(f"[error-budget] adaln_rms_fwd mutation {defect}: {ratio:.3g} x the bound")
    assert ratio > 1.0


@pytest.mark.parametrize("defect,key", [("dw_no_one_plus", "dw"), ("neighbour_sample", "dx")])
def test_rms_adaln_bwd_bounds_reject(defect, key):
    B, N, C = 3, 65, 128
    inp = LR.row_inputs(B, N, C, seed=8)
    sound, bad = rms_bwd_ratios(inp, N, True), rms_bwd_ratios(inp, N, True, defect)
    first = lambda v: v[0] if isinstance(v, tuple) else v
    assert first(sound[key]) <= 1.0
    print(f"[error-budget] adaln_rms_bwd mutation {defect}: {key} {first(bad[key]):.3g} x the bound")
    assert first(bad[key]) > 1.0


@pytest.mark.parametrize("defect", ["all_heads", "norm_after_rope"])
def test_qknorm_bounds_reject(defect):
    B, N, heads = 3, 65, 2
    q = LR.qk_inputs(B, N, heads, seed=9)
    assert qk_fwd_report(q, N, True)[0][0] <= 1.0
    ratio = qk_fwd_report(q, N, True, defect)[0][0]
    print(f"[error-budget] qknorm_rope_fwd mutation {defect}: {ratio:.3g} x the bound")
    assert ratio > 1.0


@pytest.mark.parametrize("defect,which", [("halves_swapped", 0), ("halves_swapped", 1), ("no_x_term", 1)])
def test_swiglu_bounds_reject(defect, which):
    s = LR.swiglu_inputs(195, 352, seed=10)
    assert max(swiglu_reports(s)[i][0] for i in (0, 1)) <= 1.0
    ratio = swiglu_reports(s, defect)[which][0]
    print(f"[error-budget] swiglu mutation {defect} ({'bwd' if which else 'fwd'}): {ratio:.3g} x the bound")
    assert ratio > 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    B, N, C = 3, 65, 128
    inp = LR.row_inputs(B, N, C, seed=12)
    shift, scale = sl(inp, "shift_off"), sl(inp, "scale_off")
    y = LR.adaln_rms_fwd_emulate(inp["x"], inp["w"], shift, scale, N)
    y64, _ = LR.adaln_rms_fwd64(inp["x"], inp["w"], shift, scale, N)
    assert torch.equal(y[:N], shift[0].to(BF).expand(N, C)) and torch.equal(y64[:N], shift[0].to(F64).expand(N, C))      # scale = -1
    assert torch.equal(y[:, 3], LR.R._per_row(shift, N)[:, 3].to(BF))                                                    # w = 0
    assert torch.equal(y[-1], shift[-1].to(BF)) and bool(torch.isfinite(y).all())                                         # the all-zero row
    dx, _, dscale, dw = LR.adaln_rms_bwd_emulate(inp["x"], inp["w"], scale, inp["dy"], None, N)
    assert bool(torch.isfinite(dx).all()) and not bool(dscale[:, 3].any()) and bool(dw.abs().min() >= 0)
    q = LR.qk_inputs(3, 65, 2, seed=13)
    one = torch.ones(64)
    with_tab = LR.qknorm_fwd_emulate(q["qkv"], one, one, q["tab"], 65)
    plain = LR.qknorm_fwd_emulate(q["qkv"], one, one, None, 65)
    assert torch.equal(with_tab[0::65], plain[0::65]), "position 0 with weight 1 is bf16(q r)"
    assert not bool(with_tab[0, 0, 0].any()) and not bool(LR.qknorm_fwd64(q["qkv"], one, one, q["tab"], 65)[0][0, 0, 0].any()), "a zero head"
    d, _, _ = LR.qknorm_bwd_emulate(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    assert bool(torch.isfinite(d).all())


# ---------------------------------------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names_presets_and_state_dict_keys():
    import transvae
    from transvae import dit, lightning_dit as LD
    for name in ("LightningDiT", "create_lightning_dit"):
        assert name in transvae.__all__ and hasattr(transvae, name)
    assert LD.LIGHTNING_PRESETS == {"LightningDiT-B": (768, 12), "LightningDiT-L": (1024, 24)}
    assert dit.PRESETS == {"DiT-S": (384, 12), "DiT-B": (768, 12), "DiT-L": (1024, 24)}
    assert issubclass(transvae.LightningDiT, transvae.DiT)
    for flags in LR.FLAG_SETS:
        m = transvae.LightningDiT((8, 8), 1, 32, 128, 2, 10, **flags)
        ref = LR.LightningDiTRef((8, 8), 1, 32, 128, 2, 10, **flags)
        assert list(m.state_dict()) == LD.state_dict_keys(2, **flags) == LR.state_dict_keys(2, **flags) == list(ref.state_dict())
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        ref.load_state_dict(m.state_dict())
        for k, v in m.state_dict().items():                      # DiT's initialisation, and ones for every norm weight
            if "norm" in k:
                assert bool((v == 1).all()), k
            elif "adaLN_modulation.1" in k or "final_layer.linear" in k or k.endswith(".bias"):
                assert not bool(v.any()), k
            else:
                assert bool(v.any()), k
    full = transvae.LightningDiT((8, 8), 1, 32, 128, 2, 10)
    assert (full.mlp_inner, full.mlp_inner_padded) == (341, 352)
    assert tuple(full.state_dict()["blocks.0.mlp.w12.weight"].shape) == (682, 128), "the state dict keeps H"
    assert tuple(full.state_dict()["blocks.1.attn.q_norm.weight"].shape) == (64,)
    plain = LD.state_dict_keys(3, use_rmsnorm=False, use_qknorm=False, use_swiglu=False)
    assert plain == dit.state_dict_keys(3), "with every switch off the names are DiT's"
    m = transvae.create_lightning_dit("LightningDiT-B", input_size=8, patch_size=2, in_channels=16, num_classes=10)
    assert (m.hidden_size, m.depth, m.num_heads, m.tokens, m.ld, m.mlp_inner, m.mlp_inner_padded) == (768, 12, 12, 16, 64, 2048, 2048)
    assert list(m.state_dict()) == LD.state_dict_keys(12)


def test_swiglu_width_is_the_public_one():
    from transvae import dit, lightning_dit as LD
    widths = {w for w, _ in list(LD.LIGHTNING_PRESETS.values()) + list(dit.PRESETS.values())} | {64, 128, 1152, 1536}
    for w in sorted(widths):
        m = int(w * 4.0)
        assert (2 * m) // 3 == int(2 / 3 * m) == LD.swiglu_inner(w, 4.0) == LR.swiglu_inner(w), w
    assert (LD.swiglu_inner(128, 4.0), LD.swiglu_inner(768, 4.0), LD.swiglu_inner(1024, 4.0)) == (341, 2048, 2730)


def test_argument_validation():
    import transvae
    with pytest.raises(ValueError, match="name"):
        transvae.create_lightning_dit("LightningDiT-XL")
    with pytest.raises(ValueError, match="head_dim"):
        transvae.LightningDiT(8, 1, 32, 96, 2, 10)
    with pytest.raises(ValueError, match="1536"):
        transvae.LightningDiT(8, 1, 32, 1600, 1, 10)
    with pytest.raises(ValueError, match="patch_size"):
        transvae.LightningDiT(8, 3, 32, 128, 2, 10)
    with pytest.raises(ValueError, match="use_rope"):
        transvae.LightningDiT(8, 1, 32, 128, 2, 10, use_rope=False)
    m = transvae.LightningDiT(8, 1, 4, 64, 1, 10)
    with pytest.raises(ValueError, match="labels"):
        transvae.sample_latents(m, torch.tensor([0, 11]), steps=2, stats=(torch.zeros(4), torch.ones(4)))


def test_cpu_tensors_raise():
    import transvae
    from transvae import lightning_dit as LD
    m = transvae.LightningDiT(8, 1, 4, 64, 1, 10)
    lat, stats, y = torch.zeros(2, 4, 8, 8), (torch.zeros(4), torch.ones(4)), torch.tensor([0, 10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(lat, torch.zeros(2), y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.flow_matching_loss(m, lat, y, stats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LD.adaln_rms(torch.zeros(4, 64, dtype=BF), torch.ones(64), torch.zeros(2, 128), 0, 64, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LD.qk_norm_rope_attention(torch.zeros(1, 4, 192, dtype=BF), torch.ones(64), torch.ones(64), None, 1, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LD.swiglu(torch.zeros(4, 64, dtype=BF))


def test_abi_symbols_are_declared_and_bound():
    import os
    from transvae.hip import _lib
    names = ["tv_adaln_rms_fwd", "tv_adaln_rms_bwd", "tv_adaln_rms_bwd_partial_count", "tv_qknorm_rope_fwd", "tv_qknorm_rope_bwd",
             "tv_qknorm_rope_bwd_partial_count", "tv_swiglu_fwd", "tv_swiglu_bwd"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "transvae_hip.h")).read()
    _lib.build()
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and n + "(" in header and hasattr(lib, n), n
    assert lib.tv_abi_version() == 1
    assert lib.tv_adaln_rms_bwd_partial_count(3, 65, 128) == 3 * 2 * 2 * 128 + 3 * 128
    assert lib.tv_qknorm_rope_bwd_partial_count(1, 5, 3) == 128 and lib.tv_qknorm_rope_bwd_partial_count(256, 256, 12) == 1024 * 128


# ---------------------------------------------------------------------------------------------------------------------------
# the golden file
# ---------------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_restatement_gives():
    with open(LR.GOLDEN) as f:
        gold = json.load(f)
    assert set(gold["cases"]) == set(LR.MODEL_CASES) and gold["model_args"] == LR.MODEL_ARGS and gold["batch"] == LR.MODEL_B
    for case, c in gold["cases"].items():
        assert set(c["grads"]) == set(LR.state_dict_keys(LR.MODEL_ARGS["depth"], **LR._flags(case)))
        assert 0 < c["velocity"] < 2e-2 and all(0 < v < 5e-2 for v in c["grads"].values()), case
    case = "f16d32_p1"
    c = gold["cases"][case]
    sd, batch = LR.make_state(case, c["seeds"]["state"], True), LR.make_batch(case, c["seeds"]["batch"])
    v32, l32, g32 = LR.flow_step(LR.build(case, sd), batch)
    v16, l16, g16 = LR.flow_step(LR.build(case, sd), batch, autocast=True)
    assert float(l32) == pytest.approx(c["loss_fp32"], rel=1e-4)
    assert LR.rel_l2(v16, v32) == pytest.approx(c["velocity"], rel=0.5)
    for key in ("blocks.0.norm1.weight", "blocks.0.attn.q_norm.weight", "blocks.1.mlp.w12.weight"):
        assert LR.rel_l2(g16[key], g32[key]) == pytest.approx(c["grads"][key], rel=0.5), key
    assert all(float(g.abs().max()) > 0 for g in g32.values()), "a gate is shut: the comparison would prove nothing"
    sd0 = LR.make_state(case, 1, False)
    v0, l0, _ = LR.flow_step(LR.build(case, sd0), batch)
    x = (batch["latents"] - batch["stats"]["mean"]) / batch["stats"]["std"]
    assert not bool(v0.any()) and float(l0) == pytest.approx(float(((x - batch["noise"]) ** 2).mean()), rel=1e-6)
    assert gold["sampler"]["steps"] == 4 and gold["sampler"]["cfg_scale"] == 1.5 and 0 < gold["sampler"]["latents"] < 2e-2
    assert gold["train"]["steps"] == 30 and gold["train"]["final_loss"] < 0.25 * gold["train"]["first_loss"]
