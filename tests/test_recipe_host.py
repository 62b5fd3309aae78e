"""The LightningDiT recipe (cosine loss, time shift, guidance interval, Heun steps) without a GPU: the bounds of its line of DESIGN.md
section 3.1 row E validated against fp32 emulations in the kernels' own order (never against a kernel), the defects those bounds
must reject, the closed-form gradient against autograd, the time grid, argument validation, the golden file and the ABI names."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import recipe_restatement as RR
from dit_restatement import BF, F64
from test_dit_host import U, check_report, fp32_ratio
from test_error_budget_host import one_rounding_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW, GS = 0.75, 0.5


def cos_ratios(f, p, defect=None):
    ref = RR.flow_loss_cos64(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, CW, GS)
    vals, dpred = RR.flow_loss_cos_emulate(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, CW, GS, defect=defect)
    return one_rounding_report(dpred, ref["dpred"], ref["slack"]), RR.values_ratio(vals, ref), dpred, ref


HEUN_FLAGS = ((False, False), (True, False), (False, True), (True, True))


def heun_ratio(f, p, g1, g2, defect=None, s=1.5, dt=0.25):
    x64, terms = RR.flow_heun64(f["noise"], f["v2"], f["v2b"], p, dt, s, g1, g2)
    return fp32_ratio(RR.flow_heun_emulate(f["noise"], f["v2"], f["v2b"], p, dt, s, g1, g2, defect=defect), x64, U * terms)


@pytest.mark.parametrize("B,D,h,w,p", RR.FLOW_SHAPES)
def test_emulations_sit_inside_the_bounds(B, D, h, w, p):
    f = RR.recipe_inputs(B, D, h, w, p, seed=B + D + h)
    rep, rv, dpred, ref = cos_ratios(f, p)
    print(f"[error-budget] flow_loss_cos emulation {B}x{D}x{h}x{w} p={p}: dpred {rep}, values {rv:.3g} x the bound")
    check_report(rep, "flow_loss_cos dpred")
    assert rv <= 1.0
    assert bool((dpred[:, p * p * D:] == 0).all()), "pad columns"
    assert not bool(ref["live"][1, 0]) and bool(ref["live"].sum() == ref["live"].numel() - 1), "one zero-prediction position"
    for g1, g2 in HEUN_FLAGS:
        assert heun_ratio(f, p, g1, g2) <= 1.0, (g1, g2)


@pytest.mark.parametrize("defect", ["neighbour_norm", "count_mse"])
def test_cosine_bounds_reject(defect):
    B, D, h, w, p = 2, 4, 6, 10, 2
    f = RR.recipe_inputs(B, D, h, w, p, seed=9)
    sound, bad = cos_ratios(f, p), cos_ratios(f, p, defect)
    assert sound[0][0] <= 1.0 and sound[1] <= 1.0
    print(f"[error-budget] flow_loss_cos mutation {defect}: dpred {bad[0][0]:.3g}, values {bad[1]:.3g} x the bound")
    assert bad[0][0] > 1.0
    if defect == "count_mse":
        assert bad[1] > 1.0


@pytest.mark.parametrize("defect", ["swap_guided", "full_dt"])
def test_heun_bounds_reject(defect):
    B, D, h, w, p = 2, 4, 6, 10, 2
    f = RR.recipe_inputs(B, D, h, w, p, seed=9)
    assert heun_ratio(f, p, True, False) <= 1.0
    ratio = heun_ratio(f, p, True, False, defect)
    print(f"[error-budget] flow_heun mutation {defect}: {ratio:.3g} x the bound")
    assert ratio > 1.0


def test_exact_cases_of_the_emulations():
    B, D, h, w, p = 2, 4, 6, 10, 2
    f = RR.recipe_inputs(B, D, h, w, p, seed=11)
    zero = torch.zeros_like(f["pred"])
    vals, dpred = RR.flow_loss_cos_emulate(zero, f["lat"], f["mean"], f["rstd"], f["noise"], p, CW, GS)
    from dit_restatement import flow_loss_emulate
    _, plain = flow_loss_emulate(zero, f["lat"], f["mean"], f["rstd"], f["noise"], p, GS)
    assert vals["cos"] == 1.0 and torch.equal(dpred, plain), "a zero prediction: cos = 0 everywhere, the squared-error gradient alone"
    x = f["noise"]
    assert torch.equal(RR.flow_heun_emulate(x, f["v2"], f["v2"], p, 0.25, 1.5, True, True), x), "g2 == g1 leaves x"
    half = f["v2"][:B * f["N"]]
    assert torch.equal(RR.flow_heun_emulate(x, half, half, p, 0.25), x)


def test_closed_form_gradient_equals_autograd():
    g = torch.Generator().manual_seed(3)
    T, pp, D = 40, 4, 5
    p_ = torch.randn(T, pp, D, generator=g, dtype=F64).requires_grad_(True)
    v = torch.randn(T, pp, D, generator=g, dtype=F64)
    (1 - F.cosine_similarity(p_, v, dim=-1, eps=RR.COS_EPS)).sum().backward()
    n_p, n_v = p_.detach().norm(dim=-1, keepdim=True), v.norm(dim=-1, keepdim=True)
    cos = (p_.detach() * v).sum(-1, keepdim=True) / (n_p * n_v)
    closed = -(v / n_v - cos * p_.detach() / n_p) / n_p
    assert float((closed - p_.grad).abs().max()) <= 1e-12 * float(p_.grad.abs().max())
    # the fp64 reference is that closed form: lat = x (mean 0, rstd 1), no noise, p = 1, so the rows are the positions
    B, D, h = 2, 6, 4
    lat = torch.randn(B, D, h, h, generator=g)
    pred = torch.zeros(B * h * h, 32, dtype=BF)
    pred[:, :D] = torch.randn(B * h * h, D, generator=g).to(BF)
    ref = RR.flow_loss_cos64(pred, lat, torch.zeros(D), torch.ones(D), torch.zeros_like(lat), 1, cos_weight=2.0, grad_scale=3.0)
    pa = pred[:, :D].to(F64).clone().requires_grad_(True)
    tgt = lat.to(F64).permute(0, 2, 3, 1).reshape(-1, D)
    loss = ((pa - tgt) ** 2).mean() + 2.0 * (1 - F.cosine_similarity(pa, tgt, dim=-1, eps=RR.COS_EPS)).mean()
    (3.0 * loss).backward()
    assert float(loss.detach()) == pytest.approx(ref["total"], rel=1e-12)
    assert float((ref["dpred"][:, :D] - pa.grad).abs().max()) <= 1e-12 * float(pa.grad.abs().max())
    # and the autograd form of the restatement's training step agrees with it on live positions
    pb = pred[:, :D].to(F64).clone().requires_grad_(True)
    RR.cosine_term(pb, tgt).backward()
    pc = pred[:, :D].to(F64).clone().requires_grad_(True)
    (1 - F.cosine_similarity(pc, tgt, dim=-1, eps=RR.COS_EPS)).mean().backward()
    assert float((pb.grad - pc.grad).abs().max()) <= 1e-12 * float(pc.grad.abs().max())
    pz = torch.zeros(3, D, dtype=F64, requires_grad=True)
    term = RR.cosine_term(pz, tgt[:3])
    term.backward()
    assert float(term) == 1.0 and not bool(pz.grad.any()), "a zero prediction: the term is 1 and passes no gradient"


def test_time_grid():
    from transvae import dit
    for steps in (1, 4, 7, 50):
        for s in (0.3, 1.0, 3.0):
            grid = dit.time_grid(steps, s)
            assert len(grid) == steps + 1 and grid[0] == 0.0 and grid[-1] == 1.0
            assert all(b > a for a, b in zip(grid, grid[1:])), "monotone"
            assert grid == pytest.approx(RR.time_grid(steps, s), abs=1e-15)
        dt = 1.0 / steps
        assert dit.time_grid(steps, 1.0)[:-1] == [i * dt for i in range(steps)], "shift 1 is today's grid, bit for bit"
    grid = dit.time_grid(4, 0.3)
    assert grid == pytest.approx([0.0, 1 / 11, 3 / 13, 9 / 19, 1.0], abs=1e-15)
    assert [round(t, 4) for t in grid] == [0.0, 0.0909, 0.2308, 0.4737, 1.0]
    assert grid[1] - grid[0] < grid[4] - grid[3], "s < 1 spends more steps near the noise"
    s = RR.SAMPLER
    assert (s["steps"], s["timestep_shift"], tuple(s["cfg_interval"]), s["cfg_scale"]) == (4, 0.3, (0.2, 1.0), 1.5)
    ev = RR.evaluations(4, "heun", 0.3, 1.5, (0.2, 1.0))
    assert [(i, g) for i, _, g in ev] == [(0, False), (0, False), (1, False), (1, True), (2, True), (2, True), (3, True), (3, True)], \
        "Heun step 1 has an unguided first and a guided second evaluation"
    assert [g for _, _, g in RR.evaluations(4, "euler", 0.3, 1.5, (0.2, 1.0))] == [False, False, True, True]
    assert not any(g for _, _, g in RR.evaluations(4, "heun", 0.3, 1.0, (0.0, 1.0))), "cfg_scale = 1 never guides"
    assert not any(g for _, _, g in RR.evaluations(4, "euler", 1.0, 1.5, (1.0, 1.0))), "Euler never evaluates at t = 1"


def test_argument_validation():
    import transvae
    from transvae import dit
    m = transvae.DiT(8, 1, 4, 64, 1, 10)
    y, stats = torch.tensor([0, 10]), (torch.zeros(4), torch.ones(4))
    lat = torch.zeros(2, 4, 8, 8)
    for kw, match in ((dict(method="rk4"), "method"), (dict(timestep_shift=0.0), "timestep_shift"), (dict(timestep_shift=-1.0), "timestep_shift"),
                      (dict(timestep_shift=float("nan")), "timestep_shift"), (dict(cfg_interval=(0.5, 0.2)), "cfg_interval"),
                      (dict(cfg_interval=(-0.1, 1.0)), "cfg_interval"), (dict(cfg_interval=(0.0, 1.5)), "cfg_interval"),
                      (dict(cfg_interval=(0.5,)), "cfg_interval")):
        with pytest.raises(ValueError, match=match):                 # (on the host, before the device is looked at)
            transvae.sample_latents(m, y, steps=2, stats=stats, **kw)
        with pytest.raises(ValueError, match=match):
            transvae.sample_images(None, m, y, steps=2, stats=stats, **kw)
    with pytest.raises(ValueError, match="cosine_weight"):
        transvae.flow_matching_loss(m, lat, y, stats, cosine_weight=-1.0)
    with pytest.raises(ValueError, match="cosine_weight"):
        transvae.fit_dit((lat, y, stats), m, epochs=1, batch_size=2, lr=1e-3, cosine_weight=float("inf"))
    with pytest.raises(ValueError, match="cos_weight"):
        dit.flow_loss_cos(torch.zeros(128, 32, dtype=torch.bfloat16), lat, stats[0], stats[1], lat, 1, -0.5)
    # valid new arguments reach the device check like the old ones
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.sample_latents(m, y, steps=2, stats=stats, method="heun", timestep_shift=0.3, cfg_interval=(0.2, 1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.flow_matching_loss(m, lat, y, stats, cosine_weight=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dit.flow_loss_cos(torch.zeros(128, 32, dtype=torch.bfloat16), lat, stats[0], stats[1], lat, 1, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dit.flow_heun(lat, torch.zeros(128, 32, dtype=torch.bfloat16), torch.zeros(128, 32, dtype=torch.bfloat16), 1, 0.25)


def test_golden_file_is_a_re_mint():
    with open(RR.GOLDEN) as f:
        gold = json.load(f)
    again = RR.mint(write=False)
    assert set(gold) == set(again) and set(gold["cases"]) == set(RR.CASES) and gold["cosine_weight"] == RR.COSINE_WEIGHT
    for name, c in gold["cases"].items():
        a = again["cases"][name]
        assert c["seeds"] == a["seeds"] and set(c["grads"]) == set(a["grads"])
        assert a["loss_fp32"] == pytest.approx(c["loss_fp32"], rel=1e-4) and a["mse_fp32"] == pytest.approx(c["mse_fp32"], rel=1e-4)
        assert c["loss_fp32"] > c["mse_fp32"] > 0, "the cosine term is in the loss"
        assert 0 < c["loss"] < 2e-2 and all(0 < v < 5e-2 for v in c["grads"].values()), name
        key = max(c["grads"], key=c["grads"].get)
        assert a["grads"][key] == pytest.approx(c["grads"][key], rel=0.5), (name, key)
    gs, as_ = gold["sampler"], again["sampler"]
    assert {k: v for k, v in gs.items() if k != "latents"} == {k: v for k, v in as_.items() if k != "latents"}
    assert set(gs["latents"]) == set(RR.METHODS)
    for method in RR.METHODS:
        assert 0 < gs["latents"][method] < 2e-2 and as_["latents"][method] == pytest.approx(gs["latents"][method], rel=0.5)


def test_abi_names_in_header_and_signatures():
    from transvae.hip import _lib
    txt = open(os.path.join(ROOT, "include", "transvae_hip.h")).read()
    declared = set(re.findall(r"\b(tv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    for name in ("tv_flow_loss_cos", "tv_flow_loss_cos_partial_count", "tv_flow_heun"):
        assert name in declared and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["tv_flow_loss_cos"][1]) == len(_lib.SIGNATURES["tv_flow_loss"][1]) + 1
    assert len(_lib.SIGNATURES["tv_flow_heun"][1]) == len(_lib.SIGNATURES["tv_flow_euler"][1]) + 2
