"""transvae/dit.py and csrc/dit.hip without a GPU: the bounds of DESIGN.md section 3.1 row E validated against fp32 emulations in
the kernels' own order of operations (never against a kernel), the mutations those bounds must reject, the exact cases, the host
logic (state-dict keys, presets, argument validation) and the golden file of the restatement's own bf16-autocast deviation."""
import json

import pytest
import torch

import dit_restatement as R
from test_error_budget_host import BIAS_TOL, F64, one_rounding_report

U = 2.0 ** -24


def fp32_ratio(y, y64, bound):
    """max of |y - y64| / (bound + u |y64|): the fp32 criterion of section 3.1 with the row's own first term"""
    y, y64 = y.to(F64), y64.to(F64)
    return ((y - y64).abs() / (bound + U * y64.abs() + 1e-300)).max().item()


def sl(inp, key):
    C = inp["x"].shape[1]
    return inp["mod"][:, inp[key]:inp[key] + C]


def adaln_fwd_ratio(inp, N, defect=None):
    y64, slack = R.adaln_fwd64(inp["x"], sl(inp, "shift_off"), sl(inp, "scale_off"), N)
    y = R.adaln_fwd_emulate(inp["x"], sl(inp, "shift_off"), sl(inp, "scale_off"), N, defect=defect)
    return one_rounding_report(y, y64, slack)


def adaln_bwd_ratios(inp, N, with_dres, defect=None):
    dres = inp["dres"] if with_dres else None
    ref = R.adaln_bwd64(inp["x"], sl(inp, "scale_off"), inp["dy"], dres, N)
    dx, dshift, dscale = R.adaln_bwd_emulate(inp["x"], sl(inp, "scale_off"), inp["dy"], dres, N, defect=defect)
    return {"dx": one_rounding_report(dx, ref["dx"], ref["dx_slack"]),
            "dshift": fp32_ratio(dshift, ref["dshift"], ref["k_rows"] * U * ref["dshift_terms"]),
            "dscale": fp32_ratio(dscale, ref["dscale"], ref["dscale_bound"])}


def gate_ratios(inp, N):
    g = sl(inp, "gate_off")
    o64, oslack = R.gate_fwd64(inp["x"], inp["y"], g, N)
    ref = R.gate_bwd64(inp["dy"], inp["y"], g, N)
    dy, dgate = R.gate_bwd_emulate(inp["dy"], inp["y"], g, N)
    return {"out": one_rounding_report(R.gate_fwd_emulate(inp["x"], inp["y"], g, N), o64, oslack),
            "dy": one_rounding_report(dy, ref["dy"], ref["dy_slack"]),
            "dgate": fp32_ratio(dgate, ref["dgate"], ref["k_rows"] * U * ref["dgate_terms"])}


def check_report(rep, what, min_bias_n=2000):
    ratio, ulps, mean, n = rep
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x (ulp + slack)"
    if n >= min_bias_n:
        assert abs(mean) <= BIAS_TOL, f"{what}: rounding bias {mean:+.4f} ulp over {n} elements"


# ---------------------------------------------------------------------------------------------------------------------------
# emulations inside the bounds
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", R.ROW_SHAPES)
def test_row_kernel_emulations_sit_inside_the_bounds(B, N, C):
    inp = R.row_inputs(B, N, C, seed=B + N + C)
    check_report(adaln_fwd_ratio(inp, N), "adaln_fwd")
    for with_dres in (False, True):
        r = adaln_bwd_ratios(inp, N, with_dres)
        check_report(r["dx"], f"adaln_bwd dx (dres={with_dres})")
        assert r["dshift"] <= 1.0 and r["dscale"] <= 1.0, r
    g = gate_ratios(inp, N)
    check_report(g["out"], "gate_residual_fwd")
    check_report(g["dy"], "gate_residual_bwd dy")
    assert g["dgate"] <= 1.0, g


@pytest.mark.parametrize("B,D,h,w,p", R.FLOW_SHAPES)
def test_flow_kernel_emulations_sit_inside_the_bounds(B, D, h, w, p):
    f = R.flow_inputs(B, D, h, w, p, seed=B + D + h)
    for noise in (f["noise"], None):
        y64, slack = R.flow_rows64(f["lat"], f["mean"], f["rstd"], noise, f["t"], p)
        rows = R.flow_rows_emulate(f["lat"], f["mean"], f["rstd"], noise, f["t"], p)
        check_report(one_rounding_report(rows, y64, slack), "flow_rows")
        assert bool((rows[:, p * p * D:] == 0).all())
    ref = R.flow_loss64(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, grad_scale=0.5)
    loss, dpred = R.flow_loss_emulate(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, grad_scale=0.5)
    assert abs(loss - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    check_report(one_rounding_report(dpred, ref["dpred"], ref["slack"]), "flow_loss dpred")
    assert bool((dpred[:, p * p * D:] == 0).all())
    x0 = f["noise"].clone()
    for s, v in ((None, f["v2"][:B * f["N"]]), (1.5, f["v2"])):
        x64, terms = R.flow_euler64(x0, v, p, 0.25, s)
        assert fp32_ratio(R.flow_euler_emulate(x0, v, p, 0.25, s), x64, U * terms) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["no_one_plus", "one_pass_bf16", "neighbour_sample"])
def test_adaln_fwd_bounds_reject(defect):
    B, N, C = 3, 65, 128
    inp = R.row_inputs(B, N, C, seed=7)
    assert adaln_fwd_ratio(inp, N)[0] <= 1.0
    ratio = adaln_fwd_ratio(inp, N, defect)[0]
    print(f"[error-budget] adaln_fwd mutation {defect}: {ratio:.3g} x the bound")
    assert ratio > 1.0


@pytest.mark.parametrize("defect,key", [("round_g", "dx"), ("neighbour_sample", "dx"), ("dscale_with_x", "dscale")])
def test_adaln_bwd_bounds_reject(defect, key):
    B, N, C = 3, 65, 128
    inp = R.row_inputs(B, N, C, seed=8)
    sound, bad = adaln_bwd_ratios(inp, N, True), adaln_bwd_ratios(inp, N, True, defect)
    first = lambda v: v[0] if isinstance(v, tuple) else v
    assert first(sound[key]) <= 1.0
    print(f"[error-budget] adaln_bwd mutation {defect}: {key} {first(bad[key]):.3g} x the bound")
    assert first(bad[key]) > 1.0


@pytest.mark.parametrize("defect", ["swap_t", "target_sign", "pad_in_mean", "cfg_from_cond"])
def test_flow_bounds_reject(defect):
    B, D, h, w, p = 2, 4, 6, 10, 2                      # 16 columns padded to 32: the pad columns matter
    f = R.flow_inputs(B, D, h, w, p, seed=9)
    f["t"][0], f["t"][1] = 0.25, 0.6
    if defect == "swap_t":
        y64, slack = R.flow_rows64(f["lat"], f["mean"], f["rstd"], f["noise"], f["t"], p)
        ratio = one_rounding_report(R.flow_rows_emulate(f["lat"], f["mean"], f["rstd"], f["noise"], f["t"], p, defect), y64, slack)[0]
    elif defect == "cfg_from_cond":
        x64, terms = R.flow_euler64(f["noise"], f["v2"], p, 0.25, 1.5)
        ratio = fp32_ratio(R.flow_euler_emulate(f["noise"], f["v2"], p, 0.25, 1.5, defect), x64, U * terms)
    else:
        ref = R.flow_loss64(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p)
        loss, dpred = R.flow_loss_emulate(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, defect=defect)
        ratio = max(abs(loss - ref["loss"]) / (1e-6 * abs(ref["loss"])), one_rounding_report(dpred, ref["dpred"], ref["slack"])[0])
    print(f"[error-budget] flow mutation {defect}: {ratio:.3g} x the bound")
    assert ratio > 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    f = R.flow_inputs(3, 32, 8, 8, 1, seed=11)
    rows = R.flow_rows_emulate(f["lat"], f["mean"], f["rstd"], f["noise"], f["t"], 1)
    rows64, _ = R.flow_rows64(f["lat"], f["mean"], f["rstd"], f["noise"], f["t"], 1)
    N = f["N"]
    e_rows = R.patchify(f["noise"], 1).reshape(-1, 32)
    x_rows = R.patchify(R._x32(f["lat"], f["mean"], f["rstd"]), 1).reshape(-1, 32)
    assert torch.equal(rows[:N], e_rows[:N].to(R.BF)) and torch.equal(R.r16(rows64[:N]), e_rows[:N].to(R.BF))      # t = 0
    assert torch.equal(rows[-N:], x_rows[-N:].to(R.BF))                                                              # t = 1
    B, N, C = 3, 65, 128
    inp = R.row_inputs(B, N, C, seed=12)
    shift = sl(inp, "shift_off")
    y = R.adaln_fwd_emulate(inp["x"], shift, sl(inp, "scale_off"), N)
    y64, _ = R.adaln_fwd64(inp["x"], shift, sl(inp, "scale_off"), N)
    assert torch.equal(y[:N], shift[0].to(R.BF).expand(N, C)) and torch.equal(y64[:N], shift[0].to(F64).expand(N, C))  # scale = -1
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(y64).all())                                             # the constant row
    assert torch.equal(y[-1], R.fma32(torch.zeros(C), torch.zeros(C), shift[-1]).to(R.BF))
    dx, _, _ = R.adaln_bwd_emulate(inp["x"], sl(inp, "scale_off"), inp["dy"], None, N)
    assert bool(torch.isfinite(dx).all())
    g = sl(inp, "gate_off")
    out = R.gate_fwd_emulate(inp["x"], inp["y"], g, N)
    dy, _ = R.gate_bwd_emulate(inp["dy"], inp["y"], g, N)
    assert torch.equal(out[-N:], inp["x"][-N:]) and bool((dy[-N:] == 0).all())                                          # gate = 0
    o64, _ = R.gate_fwd64(inp["x"], inp["y"], g, N)
    assert torch.equal(o64[-N:], inp["x"][-N:].to(F64))


# ---------------------------------------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_names_presets_and_state_dict_keys():
    import transvae
    from transvae import dit
    for name in ("DiT", "create_dit", "flow_matching_loss", "sample_latents", "sample_images", "fit_dit"):
        assert name in transvae.__all__ and hasattr(transvae, name)
    assert dit.PRESETS == {"DiT-S": (384, 12), "DiT-B": (768, 12), "DiT-L": (1024, 24)}
    m = transvae.create_dit("DiT-S", input_size=8, patch_size=2, in_channels=16, num_classes=10)
    assert (m.hidden_size, m.depth, m.num_heads, m.tokens, m.ld) == (384, 12, 6, 16, 64)
    assert list(m.state_dict()) == dit.state_dict_keys(12) == R.state_dict_keys(12)
    small = transvae.DiT((8, 8), 1, 32, 128, 2, 10)
    ref = R.DiTRef((8, 8), 1, 32, 128, 2, 10)
    assert {k: tuple(v.shape) for k, v in small.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    ref.load_state_dict(small.state_dict())
    sd = small.state_dict()
    for k, v in sd.items():                                   # the public initialisation
        if "adaLN_modulation.1" in k or "final_layer.linear" in k or k.endswith(".bias"):
            assert not bool(v.any()), k
        else:
            assert bool(v.any()), k
    assert abs(float(sd["y_embedder.embedding_table.weight"].std()) - 0.02) < 0.003
    assert float(sd["blocks.0.attn.qkv.weight"].abs().max()) <= (6.0 / (128 + 384)) ** 0.5


def test_argument_validation(tmp_path):
    import transvae
    with pytest.raises(ValueError, match="patch_size"):
        transvae.DiT(8, 3, 32, 128, 2, 10)
    with pytest.raises(ValueError, match="input_size"):
        transvae.DiT((8, 7), 2, 32, 128, 2, 10)
    with pytest.raises(ValueError, match="head_dim"):
        transvae.DiT(8, 1, 32, 96, 2, 10)
    with pytest.raises(ValueError, match="head_dim"):
        transvae.DiT(8, 1, 32, 1184, 2, 10)
    with pytest.raises(ValueError, match="use_rope"):
        transvae.DiT(8, 1, 32, 128, 2, 10, use_rope=False)
    with pytest.raises(ValueError, match="name"):
        transvae.create_dit("DiT-XL")
    m = transvae.DiT(8, 1, 4, 64, 1, 10)
    lat, stats = torch.zeros(2, 4, 8, 8), (torch.zeros(4), torch.ones(4))
    for bad in (torch.tensor([0, 11]), torch.tensor([-1, 3])):
        with pytest.raises(ValueError, match="labels"):
            transvae.flow_matching_loss(m, lat, bad, stats)
        with pytest.raises(ValueError, match="labels"):
            transvae.sample_latents(m, bad, steps=2, stats=stats)
    with pytest.raises(ValueError, match="stats"):
        transvae.flow_matching_loss(m, lat, torch.tensor([0, 10]), (torch.zeros(5), torch.ones(5)))
    with pytest.raises(ValueError, match="stats"):
        transvae.sample_latents(m, torch.tensor([0, 10]), steps=2, stats=(torch.zeros(5), torch.ones(5)))
    with pytest.raises(ValueError, match="latents"):
        transvae.flow_matching_loss(m, torch.zeros(2, 4, 8, 6), torch.tensor([0, 1]), stats)
    with pytest.raises(ValueError, match="t_sampling"):
        transvae.flow_matching_loss(m, lat, torch.tensor([0, 1]), stats, t_sampling="cosine")
    with pytest.raises(ValueError, match="steps"):
        transvae.sample_latents(m, torch.tensor([0, 1]), steps=0, stats=stats)
    with pytest.raises(ValueError, match="positive"):
        transvae.fit_dit((lat, torch.tensor([0, 1]), stats), m, epochs=0, batch_size=2, lr=1e-3)


def test_cpu_tensors_raise():
    import transvae
    from transvae import dit
    m = transvae.DiT(8, 1, 4, 64, 1, 10)
    lat, stats, y = torch.zeros(2, 4, 8, 8), (torch.zeros(4), torch.ones(4)), torch.tensor([0, 10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(lat, torch.zeros(2), y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.flow_matching_loss(m, lat, y, stats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.sample_latents(m, y, steps=2, stats=stats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dit.adaln(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(2, 128), 0, 64, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dit.gate_residual(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(2, 64), 0, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.fit_dit((lat, y, stats), m, epochs=1, batch_size=2, lr=1e-3, device="cpu")


# ---------------------------------------------------------------------------------------------------------------------------
# the golden file
# ---------------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_restatement_gives():
    """The structure of the committed file, one whole-model case re-derived (the deviations are those of this restatement on the
    seeds recorded), the adaLN-Zero property of the fp32 restatement, and the training case's margin."""
    with open(R.GOLDEN) as f:
        gold = json.load(f)
    assert set(gold["cases"]) == set(R.MODEL_CASES) and gold["model_args"] == R.MODEL_ARGS and gold["batch"] == R.MODEL_B
    for case, c in gold["cases"].items():
        assert set(c["grads"]) == set(R.state_dict_keys(R.MODEL_ARGS["depth"]))
        assert 0 < c["velocity"] < 2e-2 and all(0 < v < 5e-2 for v in c["grads"].values()), case
    case = "f16d32_p1"
    c = gold["cases"][case]
    sd, batch = R.make_state(case, c["seeds"]["state"], True), R.make_batch(case, c["seeds"]["batch"])
    v32, l32, g32 = R.flow_step(R.build(case, sd), batch)
    v16, l16, g16 = R.flow_step(R.build(case, sd), batch, autocast=True)
    assert float(l32) == pytest.approx(c["loss_fp32"], rel=1e-4)
    assert R.rel_l2(v16, v32) == pytest.approx(c["velocity"], rel=0.5)
    key = "blocks.0.adaLN_modulation.1.weight"
    assert R.rel_l2(g16[key], g32[key]) == pytest.approx(c["grads"][key], rel=0.5)
    assert all(float(g.abs().max()) > 0 for g in g32.values()), "a gate is shut: the comparison would prove nothing"
    # the public initialisation: the output is exactly 0 and the loss the mean of v^2
    sd0 = R.make_state(case, 1, False)
    v0, l0, _ = R.flow_step(R.build(case, sd0), batch)
    x = (batch["latents"] - batch["stats"]["mean"]) / batch["stats"]["std"]
    assert not bool(v0.any()) and float(l0) == pytest.approx(float(((x - batch["noise"]) ** 2).mean()), rel=1e-6)
    assert gold["sampler"]["steps"] == 4 and gold["sampler"]["cfg_scale"] == 1.5 and 0 < gold["sampler"]["latents"] < 2e-2
    assert gold["train"]["steps"] == 30 and gold["train"]["final_loss"] < 0.25 * gold["train"]["first_loss"]
