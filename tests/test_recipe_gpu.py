"""The LightningDiT recipe on the device: tv_flow_loss_cos and tv_flow_heun through the C ABI against fp64
under their line of section 3.1 row E, their exact cases and bit-reproducibility; one training step with the cosine term and the
sampler with a shifted grid, a guidance interval and both methods against the plain-torch restatement (tests/recipe_restatement.py)
under the bf16 tier's yardstick; `fit_dit` with the cosine term end to end."""
import ctypes as C
import json

import pytest
import torch

import dit_restatement as R
import lightning_restatement as LR
import recipe_restatement as RR
from test_dit_gpu import FLOOR, MARGIN, SENTINEL, _p, _stream, dev, guarded, report, take
from test_dit_host import U, check_report, fp32_ratio
from test_error_budget_host import one_rounding_report

pytestmark = pytest.mark.gpu

CW, GS = 0.75, 0.5
HEUN_FLAGS = ((False, False), (True, False), (False, True), (True, True))


def golden():
    with open(RR.GOLDEN) as f:
        return json.load(f)


def run_cos(lat, mean, rstd, noise, pred, p, cw=CW, gs=GS, want_grad=True):
    """tv_flow_loss_cos through the C ABI on strided latents, every output followed by a sentinel -> (out [5] fp64, dpred | None), on the host"""
    from transvae.hip import _lib as L
    lib = L.load()
    B, D, h, w = lat.shape
    T, ld = pred.shape
    out = torch.full((6,), SENTINEL, dtype=torch.float64, device=dev())
    n = lib.tv_flow_loss_cos_partial_count(B, D, h, w, p, ld)
    assert n == 2 * lib.tv_flow_loss_partial_count(B, D, h, w, p, ld)
    part = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=dev())
    dpred = guarded(T, ld) if want_grad else None
    L.check(lib.tv_flow_loss_cos(_p(pred), _p(lat), lat.stride(0), lat.stride(1), _p(mean), _p(rstd), _p(noise), _p(dpred), _p(out), _p(part),
                                 B, D, h, w, p, ld, cw, gs, _stream()), "tv_flow_loss_cos")
    torch.cuda.synchronize()
    assert float(out[5]) == SENTINEL and float(part[n]) == SENTINEL, "wrote past out / partials"
    return out[:5].cpu(), (take(dpred) if want_grad else None)


def run_heun(x, v1, v2, p, dt, s, g1, g2):
    """tv_flow_heun through the C ABI on a copy of x followed by a sentinel sample -> x' on the host"""
    from transvae.hip import _lib as L
    B, D, h, w = x.shape
    buf = torch.full((B + 1, D, h, w), SENTINEL, dtype=torch.float32, device=dev())
    buf[:B] = x
    a = v1 if g1 else v1[:v1.shape[0] // 2].contiguous()
    b = v2 if g2 else v2[:v2.shape[0] // 2].contiguous()
    L.check(L.load().tv_flow_heun(_p(buf), _p(a), _p(b), B, D, h, w, p, v1.shape[1], dt, s, int(g1), int(g2), _stream()), "tv_flow_heun")
    torch.cuda.synchronize()
    assert bool((buf[B] == SENTINEL).all()), "wrote past x"
    return buf[:B].cpu()


def on_device(f, D):
    d = {k: v.to(dev()) for k, v in f.items() if torch.is_tensor(v)}
    lat = d["moments"][:, :D]                                     # the mu half in place: a non-contiguous batch stride
    return d, lat


@pytest.mark.parametrize("B,D,h,w,p", RR.FLOW_SHAPES)
def test_kernels_against_fp64(B, D, h, w, p):
    from transvae import dit
    f = RR.recipe_inputs(B, D, h, w, p, seed=B + D + h)
    d, lat = on_device(f, D)
    F_ = p * p * D
    out, dpred = run_cos(lat, d["mean"], d["rstd"], d["noise"], d["pred"], p)
    ref = RR.flow_loss_cos64(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, CW, GS)
    rep = one_rounding_report(dpred, ref["dpred"], ref["slack"])
    rv = RR.values_ratio(out.tolist(), ref)
    report(f"flow_loss_cos {B}x{D}x{h}x{w} p={p}: dpred, values / bound", (rep, rv))
    check_report(rep, "flow_loss_cos dpred")
    assert rv <= 1.0, (out.tolist(), {k: ref[k] for k in RR.VALUE_KEYS}, ref["bounds"])
    assert bool((dpred[:, F_:] == 0).all()), "pad columns of the gradient"
    plain, _ = dit.flow_loss(d["pred"], lat, d["mean"], d["rstd"], d["noise"], p, grad_scale=GS)
    assert torch.equal(out[:2], plain.cpu()), "the squared-error half has tv_flow_loss's bits"
    value_only, none = run_cos(lat, d["mean"], d["rstd"], d["noise"], d["pred"], p, want_grad=False)
    assert none is None and torch.equal(value_only, out), "dpred = NULL: the values alone"
    out2, dpred2 = dit.flow_loss_cos(d["pred"], lat, d["mean"], d["rstd"], d["noise"], p, CW, GS)
    assert torch.equal(out2.cpu(), out) and torch.equal(dpred2.cpu(), dpred), "the wrapper is the same call"
    for g1, g2 in HEUN_FLAGS:
        got = run_heun(d["noise"], d["v2"], d["v2b"], p, 0.25, 1.5, g1, g2)
        x64, terms = RR.flow_heun64(f["noise"], f["v2"], f["v2b"], p, 0.25, 1.5, g1, g2)
        r = fp32_ratio(got, x64, U * terms)
        report(f"flow_heun guided=({g1}, {g2})", r)
        assert r <= 1.0, (g1, g2)
        N = f["N"]
        a = d["v2"] if g1 else d["v2"][:B * N].contiguous()
        b = d["v2b"] if g2 else d["v2b"][:B * N].contiguous()
        assert torch.equal(dit.flow_heun(d["noise"].clone(), a, b, p, 0.25, 1.5, g1, g2).cpu(), got), "the wrapper is the same call"


@pytest.mark.parametrize("B,D,h,w,p", RR.FLOW_SHAPES)
def test_exact_cases(B, D, h, w, p):
    from transvae import dit
    f = RR.recipe_inputs(B, D, h, w, p, seed=B + D + h)
    d, lat = on_device(f, D)
    N = f["N"]
    # prediction rows all zero: every cos is 0 by the rule, so the mean of 1 - cos is exactly 1 and the gradient is tv_flow_loss's
    zero_pred = torch.zeros_like(d["pred"])
    out, dpred = run_cos(lat, d["mean"], d["rstd"], d["noise"], zero_pred, p)
    plain, dplain = dit.flow_loss(zero_pred, lat, d["mean"], d["rstd"], d["noise"], p, grad_scale=GS)
    assert float(out[3]) == 1.0 and float(out[2]) == float(B * h * w)
    assert torch.equal(dpred, dplain.cpu()) and torch.equal(out[:2], plain.cpu())
    assert float(out[4]) == float(out[1]) + CW
    # a prediction equal to the target (latents and noise on a 1/8 grid: x - e is exact in bf16): all sums 0, an all-zero gradient
    g = torch.Generator().manual_seed(5)
    lat8 = (torch.randint(-32, 33, (B, D, h, w), generator=g) / 8).to(dev())
    e8 = (torch.randint(-32, 33, (B, D, h, w), generator=g) / 8).to(dev())
    assert float((lat8 - e8).abs().sum(1).min()) > 0, "a position with a zero target would have cos = 0 by the rule"
    zero, one = torch.zeros(D, device=dev()), torch.ones(D, device=dev())
    target = dit.flow_rows(lat8 - e8, zero, one, p)
    out0, d0 = run_cos(lat8, zero, one, e8, target, p, cw=1.0, gs=1.0)
    assert out0.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0] and not bool(d0.any())
    # Heun: a second evaluation equal to the first leaves every bit of x
    x0 = d["noise"]
    for guided in (False, True):
        assert torch.equal(run_heun(x0, d["v2"], d["v2"], p, 0.25, 1.5, guided, guided), f["noise"]), guided
    # the two guidance scales that select one half
    cond = lambda v: torch.cat([v[:B * N], v[:B * N]])
    unco = lambda v: torch.cat([v[B * N:], v[B * N:]])
    got0 = run_heun(x0, d["v2"], d["v2b"], p, 0.25, 0.0, True, True)
    assert torch.equal(got0, run_heun(x0, unco(d["v2"]), unco(d["v2b"]), p, 0.25, 0.0, False, False)), "cfg_scale = 0: the unconditional halves alone"
    got1 = run_heun(x0, d["v2"], d["v2b"], p, 0.25, 1.0, True, True)
    _, terms = RR.flow_heun64(f["noise"], f["v2"], f["v2b"], p, 0.25, 1.0, True, True)
    x64, _ = RR.flow_heun64(f["noise"], cond(f["v2"]), cond(f["v2b"]), p, 0.25)
    assert fp32_ratio(got1, x64, U * terms) <= 1.0, "cfg_scale = 1: the conditional halves alone, within the bound"


def test_bit_reproducible():
    B, D, h, w, p = 2, 16, 16, 16, 2
    f = RR.recipe_inputs(B, D, h, w, p, seed=4)
    d, lat = on_device(f, D)
    runs = [run_cos(lat, d["mean"], d["rstd"], d["noise"], d["pred"], p) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    xs = [run_heun(d["noise"], d["v2"], d["v2b"], p, 0.25, 1.5, True, False) for _ in range(2)]
    assert torch.equal(xs[0], xs[1])


# ---------------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------------
def hip_model(name, sd):
    import transvae
    mod, case = RR.case_parts(name)
    cls = transvae.LightningDiT if mod is LR else transvae.DiT
    m = cls(**mod.MODEL_CASES[case], **mod.MODEL_ARGS)
    m.load_state_dict(sd)
    return m.to(dev()).eval()


def hip_step(m, batch, cosine_weight):
    import transvae
    m.zero_grad(set_to_none=True)
    stats = {k: v.to(dev()) for k, v in batch["stats"].items()}
    D = m.in_channels
    loss = transvae.flow_matching_loss(m, batch["moments"].to(dev())[:, :D], batch["labels"].to(dev()), stats, t=batch["t"].to(dev()),
                                       noise=batch["noise"].to(dev()), cosine_weight=cosine_weight)
    return float(loss)


@pytest.mark.parametrize("name", list(RR.CASES))
def test_training_step_against_the_restatement(name):
    gold = golden()["cases"][name]
    mod, case = RR.case_parts(name)
    sd, batch = mod.make_state(case, gold["seeds"]["state"], True), mod.make_batch(case, gold["seeds"]["batch"])
    _, l32, _, g32 = RR.flow_step(mod.build(case, sd), batch, RR.COSINE_WEIGHT)
    m = hip_model(name, sd)
    loss = hip_step(m, batch, RR.COSINE_WEIGHT)
    dl = abs(loss - float(l32)) / float(l32)
    report(f"{name} loss relative (bound {max(FLOOR, MARGIN * gold['loss']):.3g})", dl)
    worst = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        worst[k] = (R.rel_l2(p.grad, g32[k]), max(FLOOR, MARGIN * gold["grads"][k]))
    for k, (e, bound) in sorted(worst.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:6]:
        report(f"{name} d({k}) relL2 (bound {bound:.3g})", e)
    assert dl <= max(FLOOR, MARGIN * gold["loss"])
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("name", list(RR.CASES))
def test_public_initialisation_with_the_cosine_term(name):
    """adaLN-Zero's zero final layer predicts exactly 0: the term is 1 at every position and gives no gradient"""
    import transvae
    mod, case = RR.case_parts(name)
    batch = mod.make_batch(case, 21)
    m = hip_model(name, mod.make_state(case, 20, False))
    x = (batch["latents"].double() - batch["stats"]["mean"].double()) / batch["stats"]["std"].double()
    mse = float(((x - batch["noise"].double()) ** 2).mean())
    with transvae.deterministic():
        loss1 = hip_step(m, batch, 1.0)
        g1 = {k: p.grad.clone() for k, p in m.final_layer.linear.named_parameters()}
        loss0 = hip_step(m, batch, 0.0)
        g0 = {k: p.grad.clone() for k, p in m.final_layer.linear.named_parameters()}
    assert loss1 == pytest.approx(mse + 1.0, rel=1e-5) and loss0 == pytest.approx(mse, rel=1e-5)
    for k in g0:
        assert float(g0[k].abs().max()) > 0 and torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize("method", RR.METHODS)
def test_sampler_against_the_restatement(method):
    import transvae
    gold = golden()["sampler"]
    mod, case = RR.case_parts(gold["case"])
    sd, batch = mod.make_state(case, gold["seeds"]["state"], True), mod.make_batch(case, gold["seeds"]["batch"])
    kw = dict(steps=gold["steps"], cfg_scale=gold["cfg_scale"])
    ref = RR.sample(mod.build(case, sd), batch["labels"], batch["noise"], batch["stats"], kw["steps"], kw["cfg_scale"], method,
                    gold["timestep_shift"], tuple(gold["cfg_interval"]))
    m = hip_model(gold["case"], sd)
    y, noise = batch["labels"].to(dev()), batch["noise"].to(dev())
    got = transvae.sample_latents(m, y, stats=batch["stats"], noise=noise, method=method, timestep_shift=gold["timestep_shift"],
                                  cfg_interval=tuple(gold["cfg_interval"]), **kw)
    assert got.dtype == torch.float32 and got.shape == batch["noise"].shape
    e = R.rel_l2(got, ref)
    bound = max(FLOOR, MARGIN * gold["latents"][method])
    report(f"sampler {method} relL2 (bound {bound:.3g})", e)
    assert e <= bound
    plain = transvae.sample_latents(m, y, stats=batch["stats"], noise=noise, method=method, **kw)
    assert not torch.equal(plain, got), "the shift and the interval change the result"


def test_sampler_defaults_and_an_empty_interval():
    import transvae
    gold = golden()["sampler"]
    mod, case = RR.case_parts(gold["case"])
    sd, batch = mod.make_state(case, gold["seeds"]["state"], True), mod.make_batch(case, gold["seeds"]["batch"])
    m = hip_model(gold["case"], sd)
    y, noise = batch["labels"].to(dev()), batch["noise"].to(dev())
    kw = dict(steps=gold["steps"], stats=batch["stats"], noise=noise)
    base = transvae.sample_latents(m, y, cfg_scale=1.5, **kw)
    explicit = transvae.sample_latents(m, y, cfg_scale=1.5, method="euler", timestep_shift=1.0, cfg_interval=(0.0, 1.0), **kw)
    assert torch.equal(base, explicit), "explicit defaults are the call without them"
    unguided = transvae.sample_latents(m, y, cfg_scale=1.0, **kw)
    empty = transvae.sample_latents(m, y, cfg_scale=1.5, cfg_interval=(1.0, 1.0), **kw)
    assert torch.equal(empty, unguided) and not torch.equal(base, unguided), "Euler never evaluates at t = 1: no step is guided"


def test_fit_dit_with_the_cosine_term(tmp_path):
    import transvae
    from probe_restatement import write_split
    g = torch.Generator().manual_seed(0)
    D, h = 4, 8
    shards = []
    for n in (10, 6):
        lat = torch.randn(n, 2 * D, h, h, generator=g)
        shards.append({"latents": lat, "latents_flip": lat.flip(-1), "labels": torch.randint(0, 5, (n,), generator=g)})
    write_split(str(tmp_path), shards, {"mean": torch.zeros(1, D, 1, 1), "std": torch.ones(1, D, 1, 1)})
    runs = {}
    for cw in (0.0, 1.0):
        m = transvae.DiT(h, 2, D, 64, 1, 5, generator=torch.Generator().manual_seed(1))
        runs[cw] = transvae.fit_dit(str(tmp_path), m, epochs=2, batch_size=4, lr=1e-3, seed=0, log_every=3, device=dev(), cosine_weight=cw)
    r = runs[1.0]
    assert r["steps"] == 2 * (3 + 2) and [hh["step"] for hh in r["history"]] == [3, 6, 9, 10] and r["shard_orders"] == runs[0.0]["shard_orders"]
    # ten steps from the zero-initialised final layer: the prediction is still small against x - e, so the term stays near its
    # initial value 1 (it lies in [0, 2]) on top of a squared error that both runs share to first order
    first = r["history"][0]["loss"] - runs[0.0]["history"][0]["loss"]
    report("fit_dit first-interval loss with / without the cosine term", (r["history"][0]["loss"], runs[0.0]["history"][0]["loss"]))
    assert isinstance(r["loss"], float) and 0.5 < first < 1.5
