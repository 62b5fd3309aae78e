"""csrc/dit.hip and transvae/dit.py on the device: the seven kernels against fp64 under DESIGN.md section 3.1 row E, their exact
cases and bit-reproducibility, the whole model, the sampler and a short training run against the plain-torch restatement
(tests/dit_restatement.py) under the bf16 tier's yardstick, and `fit_dit` end to end on a two-shard directory."""
import ctypes as C
import json

import pytest
import torch

import dit_restatement as R
from test_dit_host import U, check_report, fp32_ratio, sl
from test_error_budget_host import F64, one_rounding_report

pytestmark = pytest.mark.gpu

FLOOR, MARGIN = 1e-2, 1.25        # the VF bullet's yardstick: relL2 within max(1e-2, 1.25 x the restatement's own bf16 deviation)
SENTINEL = 7.5


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def golden():
    with open(R.GOLDEN) as f:
        return json.load(f)


def guarded(rows, cols, dtype=torch.bfloat16):
    """an output with one sentinel row past what the kernel may write"""
    return torch.full((rows + 1, cols), SENTINEL, dtype=dtype, device=dev())


def take(buf):
    assert bool((buf[-1] == SENTINEL).all()), "wrote past the output"
    return buf[:-1].cpu()


def run_rows(inp, B, N, with_dres):
    """kernels 1-4 through the C ABI on slices at non-zero offsets of one [B, 6 C] matrix"""
    from transvae.hip import _lib as L
    lib = L.load()
    C_ = inp["x"].shape[1]
    T, ld = B * N, 6 * C_
    d = {k: v.to(dev()) for k, v in inp.items() if torch.is_tensor(v)}
    so, ko, go = inp["shift_off"], inp["scale_off"], inp["gate_off"]
    y, dx, out, dyg = guarded(T, C_), guarded(T, C_), guarded(T, C_), guarded(T, C_)
    dmod = torch.full((B + 1, ld), SENTINEL, dtype=torch.float32, device=dev())
    L.check(lib.tv_adaln_fwd(_p(d["x"]), _p(d["mod"]), so, ko, ld, _p(y), B, N, C_, R.LN_EPS, _stream()), "tv_adaln_fwd")
    part = torch.empty(lib.tv_adaln_bwd_partial_count(B, N, C_), dtype=torch.float32, device=dev())
    L.check(lib.tv_adaln_bwd(_p(d["x"]), _p(d["mod"]), so, ko, ld, _p(d["dy"]), _p(d["dres"]) if with_dres else None, _p(dx), _p(dmod), _p(part),
                             B, N, C_, R.LN_EPS, _stream()), "tv_adaln_bwd")
    L.check(lib.tv_gate_residual_fwd(_p(d["x"]), _p(d["y"]), _p(d["mod"]), go, ld, _p(out), B, N, C_, _stream()), "tv_gate_residual_fwd")
    part2 = torch.empty(lib.tv_gate_residual_bwd_partial_count(B, N, C_), dtype=torch.float32, device=dev())
    L.check(lib.tv_gate_residual_bwd(_p(d["dy"]), _p(d["y"]), _p(d["mod"]), go, ld, _p(dyg), _p(dmod), _p(part2), B, N, C_, _stream()),
            "tv_gate_residual_bwd")
    torch.cuda.synchronize()
    dm = take(dmod)
    written = torch.zeros(ld, dtype=torch.bool)
    for o in (so, ko, go):
        written[o:o + C_] = True
    assert bool((dm[:, ~written] == SENTINEL).all()), "the backward wrote outside its column ranges"
    return {"y": take(y), "dx": take(dx), "out": take(out), "dy": take(dyg), "dshift": dm[:, so:so + C_], "dscale": dm[:, ko:ko + C_],
            "dgate": dm[:, go:go + C_]}


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("B,N,C_", R.ROW_SHAPES)
def test_row_kernels_against_fp64(B, N, C_, with_dres):
    inp = R.row_inputs(B, N, C_, seed=B + N + C_)
    got = run_rows(inp, B, N, with_dres)
    shift, scale, gate = sl(inp, "shift_off"), sl(inp, "scale_off"), sl(inp, "gate_off")
    y64, slack = R.adaln_fwd64(inp["x"], shift, scale, N)
    rep = one_rounding_report(got["y"], y64, slack)
    report(f"adaln_fwd {B}x{N}x{C_}", rep)
    check_report(rep, "adaln_fwd")
    assert torch.equal(got["y"][:N], shift[0].to(R.BF).expand(N, C_)), "scale = -1 must give y = shift"
    assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["dx"]).all()), "the constant row"
    ref = R.adaln_bwd64(inp["x"], scale, inp["dy"], inp["dres"] if with_dres else None, N)
    rep = one_rounding_report(got["dx"], ref["dx"], ref["dx_slack"])
    rs = fp32_ratio(got["dshift"], ref["dshift"], ref["k_rows"] * U * ref["dshift_terms"])
    rq = fp32_ratio(got["dscale"], ref["dscale"], ref["dscale_bound"])
    report(f"adaln_bwd {B}x{N}x{C_} dres={with_dres}", (rep, rs, rq))
    check_report(rep, "adaln_bwd dx")
    assert rs <= 1.0 and rq <= 1.0, (rs, rq)
    o64, oslack = R.gate_fwd64(inp["x"], inp["y"], gate, N)
    rep = one_rounding_report(got["out"], o64, oslack)
    check_report(rep, "gate_residual_fwd")
    gref = R.gate_bwd64(inp["dy"], inp["y"], gate, N)
    rep2 = one_rounding_report(got["dy"], gref["dy"], gref["dy_slack"])
    rg = fp32_ratio(got["dgate"], gref["dgate"], gref["k_rows"] * U * gref["dgate_terms"])
    report(f"gate_residual {B}x{N}x{C_}", (rep, rep2, rg))
    check_report(rep2, "gate_residual_bwd dy")
    assert rg <= 1.0, rg
    assert torch.equal(got["out"][-N:], inp["x"][-N:]) and bool((got["dy"][-N:] == 0).all()), "gate = 0"


def run_flow(f, B, D, h, w, p):
    from transvae import dit
    d = {k: v.to(dev()) for k, v in f.items() if torch.is_tensor(v)}
    lat = d["moments"][:, :D]                                     # the mu half in place: a non-contiguous batch stride
    assert not lat.is_contiguous() or B == 1
    buf = guarded(B * f["N"], f["ld"])
    rows = dit.flow_rows(lat, d["mean"], d["rstd"], p, d["noise"], d["t"], out=buf[:-1])
    plain = dit.flow_rows(lat, d["mean"], d["rstd"], p)
    out, dpred = dit.flow_loss(d["pred"], lat, d["mean"], d["rstd"], d["noise"], p, grad_scale=0.5)
    torch.cuda.synchronize()
    assert bool((buf[-1] == SENTINEL).all()), "wrote past the rows"
    return d, lat, rows, plain, out, dpred


@pytest.mark.parametrize("B,D,h,w,p", R.FLOW_SHAPES)
def test_flow_kernels_against_fp64(B, D, h, w, p):
    from transvae import dit
    f = R.flow_inputs(B, D, h, w, p, seed=B + D + h)
    d, lat, rows, plain, out, dpred = run_flow(f, B, D, h, w, p)
    torch.cuda.synchronize()
    F_, N = p * p * D, f["N"]
    for got, noise in ((rows.cpu(), f["noise"]), (plain.cpu(), None)):
        y64, slack = R.flow_rows64(f["lat"], f["mean"], f["rstd"], noise, f["t"], p)
        rep = one_rounding_report(got, y64, slack)
        report(f"flow_rows {B}x{D}x{h}x{w} p={p} noise={noise is not None}", rep)
        check_report(rep, "flow_rows")
        assert bool((got[:, F_:] == 0).all()), "pad columns"
    e_rows = R.patchify(f["noise"], p).reshape(-1, F_)
    x_rows = R.patchify(R._x32(f["lat"], f["mean"], f["rstd"]), p).reshape(-1, F_)
    assert torch.equal(rows.cpu()[:N, :F_], e_rows[:N].to(R.BF)), "t = 0 must give bf16(e)"
    assert torch.equal(rows.cpu()[-N:, :F_], x_rows[-N:].to(R.BF)), "t = 1 must give bf16(x)"
    assert torch.equal(plain.cpu()[:, :F_], x_rows.to(R.BF)), "the null-noise mode is the plain patchify"
    ref = R.flow_loss64(f["pred"], f["lat"], f["mean"], f["rstd"], f["noise"], p, grad_scale=0.5)
    total, loss = out.cpu().tolist()
    report(f"flow_loss {B}x{D}x{h}x{w} p={p} relative error", abs(loss - ref["loss"]) / ref["loss"])
    assert abs(loss - ref["loss"]) <= 1e-6 * ref["loss"] and abs(total - ref["sum"]) <= 1e-6 * ref["sum"]
    rep = one_rounding_report(dpred.cpu(), ref["dpred"], ref["slack"])
    check_report(rep, "flow_loss dpred")
    assert bool((dpred.cpu()[:, F_:] == 0).all()), "pad columns of the gradient"
    # a prediction equal to the target: loss 0 and an all-zero gradient (latents and noise on a 1/8 grid: x - e is exact in bf16)
    g = torch.Generator().manual_seed(5)
    lat8 = (torch.randint(-32, 33, (B, D, h, w), generator=g) / 8).to(dev())
    e8 = (torch.randint(-32, 33, (B, D, h, w), generator=g) / 8).to(dev())
    zero, one = torch.zeros(D, device=dev()), torch.ones(D, device=dev())
    target = dit.flow_rows(lat8 - e8, zero, one, p)
    out0, d0 = dit.flow_loss(target, lat8, zero, one, e8, p)
    assert out0.cpu().tolist() == [0.0, 0.0] and not bool(d0.any())
    # Euler steps: plain, guided, and the two guidance scales that select one half
    x0 = d["noise"].clone()
    v2, v1 = d["v2"], d["v2"][:B * N].contiguous()
    vu = d["v2"][B * N:].contiguous()
    for s, v in ((None, v1), (1.5, v2), (1.0, v2), (0.0, v2)):
        got = dit.flow_euler(x0.clone(), v, p, 0.25, s).cpu()
        x64, terms = R.flow_euler64(f["noise"], v.cpu(), p, 0.25, s)
        r = fp32_ratio(got, x64, U * terms)
        report(f"flow_euler cfg={s}", r)
        assert r <= 1.0
        if s == 0.0:
            assert torch.equal(got, dit.flow_euler(x0.clone(), vu, p, 0.25).cpu()), "cfg_scale = 0 is the unconditional half alone"
        if s == 1.0:
            cond, terms1 = R.flow_euler64(f["noise"], v1.cpu(), p, 0.25)
            assert fp32_ratio(got, cond, U * terms) <= 1.0, "cfg_scale = 1 is the conditional half alone"


def test_reductions_are_bit_reproducible():
    from transvae import dit
    B, N, C_ = 3, 65, 128
    inp = R.row_inputs(B, N, C_, seed=3)
    a, b = run_rows(inp, B, N, True), run_rows(inp, B, N, True)
    for k in ("dx", "dshift", "dscale", "dy", "dgate"):
        assert torch.equal(a[k], b[k]), k
    f = R.flow_inputs(2, 16, 16, 16, 2, seed=4)
    r1, r2 = run_flow(f, 2, 16, 16, 16, 2), run_flow(f, 2, 16, 16, 16, 2)
    assert torch.equal(r1[4], r2[4]) and torch.equal(r1[5], r2[5])


# ---------------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------------
def hip_model(case, sd):
    import transvae
    m = transvae.DiT(**R.MODEL_CASES[case], **R.MODEL_ARGS)
    m.load_state_dict(sd)
    return m.to(dev()).eval()


def hip_step(m, batch):
    import transvae
    m.zero_grad(set_to_none=True)
    stats = {k: v.to(dev()) for k, v in batch["stats"].items()}
    D = m.in_channels
    loss = transvae.flow_matching_loss(m, batch["moments"].to(dev())[:, :D], batch["labels"].to(dev()), stats, t=batch["t"].to(dev()),
                                       noise=batch["noise"].to(dev()))
    return float(loss)


def hip_velocity(m, batch):
    from transvae import dit
    mean, rstd, _, _ = dit._stats_of(batch["stats"], m.in_channels, dev())
    rows = dit.flow_rows(batch["moments"].to(dev())[:, :m.in_channels], mean, rstd, m.patch_size, batch["noise"].to(dev()), batch["t"].to(dev()))
    with torch.no_grad():
        v = m(rows, batch["t"].to(dev()), batch["labels"].to(dev()))
    assert bool((v[:, m.patch_cols:] == 0).all()), "pad columns of the velocity"
    h, w = m.input_size
    return R.unpatchify(v[:, :m.patch_cols].float().cpu().reshape(batch["t"].shape[0], m.tokens, m.patch_cols), m.in_channels, h, w, m.patch_size)


@pytest.mark.parametrize("case", list(R.MODEL_CASES))
def test_public_initialisation_is_adaln_zero(case):
    batch = R.make_batch(case, 21)
    m = hip_model(case, R.make_state(case, 20, False))
    v = hip_velocity(m, batch)
    assert not bool(v.any()), "the zero-initialised final layer must give exactly 0"
    loss = hip_step(m, batch)
    x = (batch["latents"].double() - batch["stats"]["mean"].double()) / batch["stats"]["std"].double()
    assert loss == pytest.approx(float(((x - batch["noise"].double()) ** 2).mean()), rel=1e-5)
    assert float(m.final_layer.linear.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("case", list(R.MODEL_CASES))
def test_whole_model_against_the_restatement(case):
    gold = golden()["cases"][case]
    sd, batch = R.make_state(case, gold["seeds"]["state"], True), R.make_batch(case, gold["seeds"]["batch"])
    v32, l32, g32 = R.flow_step(R.build(case, sd), batch)
    m = hip_model(case, sd)
    dv = R.rel_l2(hip_velocity(m, batch), v32)
    loss = hip_step(m, batch)
    dl = abs(loss - float(l32)) / float(l32)
    report(f"{case} velocity relL2 (bound {max(FLOOR, MARGIN * gold['velocity']):.3g})", dv)
    report(f"{case} loss relative (bound {max(FLOOR, MARGIN * gold['loss']):.3g})", dl)
    worst = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        worst[k] = (R.rel_l2(p.grad, g32[k]), max(FLOOR, MARGIN * gold["grads"][k]))
    for k, (e, bound) in sorted(worst.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:6]:
        report(f"{case} d({k}) relL2 (bound {bound:.3g})", e)
    assert dv <= max(FLOOR, MARGIN * gold["velocity"]) and dl <= max(FLOOR, MARGIN * gold["loss"])
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_sampler_against_the_restatement():
    import transvae
    gold = golden()["sampler"]
    case = gold["case"]
    sd, batch = R.make_state(case, gold["seeds"]["state"], True), R.make_batch(case, gold["seeds"]["batch"])
    ref = R.sample(R.build(case, sd), batch["labels"], batch["noise"], batch["stats"], gold["steps"], gold["cfg_scale"])
    m = hip_model(case, sd)
    got = transvae.sample_latents(m, batch["labels"].to(dev()), steps=gold["steps"], cfg_scale=gold["cfg_scale"], stats=batch["stats"],
                                  noise=batch["noise"].to(dev()))
    assert got.dtype == torch.float32 and got.shape == batch["noise"].shape
    e = R.rel_l2(got, ref)
    report(f"sampler relL2 (bound {max(FLOOR, MARGIN * gold['latents']):.3g})", e)
    assert e <= max(FLOOR, MARGIN * gold["latents"])
    again = transvae.sample_latents(m, batch["labels"].to(dev()), steps=gold["steps"], cfg_scale=gold["cfg_scale"], stats=batch["stats"],
                                    generator=torch.Generator(device=dev()).manual_seed(3))
    assert bool(torch.isfinite(again).all()) and not torch.equal(again, got)


def test_thirty_training_steps_halve_the_loss():
    from transvae.optim import FusedAdamW
    gold = golden()["train"]
    assert gold["final_loss"] < 0.25 * gold["first_loss"]
    case = gold["case"]
    sd, batch = R.make_state(case, gold["seeds"]["state"], False), R.make_batch(case, gold["seeds"]["batch"])
    m = hip_model(case, sd)
    opt = FusedAdamW(m.parameters(), lr=gold["lr"], weight_decay=0.0)
    losses = []
    for _ in range(gold["steps"]):
        losses.append(hip_step(m, batch))
        opt.step()
    losses.append(hip_step(m, batch))
    report("training losses first / last (restatement: %.4g / %.4g)" % (gold["first_loss"], gold["final_loss"]), (losses[0], losses[-1]))
    assert losses[0] == pytest.approx(gold["first_loss"], rel=1e-3)
    assert losses[-1] < 0.5 * losses[0]


def test_fit_dit_end_to_end(tmp_path):
    import transvae
    from probe_restatement import write_split
    g = torch.Generator().manual_seed(0)
    D, h = 4, 8
    shards = []
    for n in (10, 6):
        lat = torch.randn(n, 2 * D, h, h, generator=g)          # what="moments" shards: the mu half is used
        shards.append({"latents": lat, "latents_flip": lat.flip(-1), "labels": torch.randint(0, 5, (n,), generator=g)})
    stats = {"mean": torch.zeros(1, D, 1, 1), "std": torch.ones(1, D, 1, 1)}
    write_split(str(tmp_path), shards, stats)
    runs = []
    for seed in (0, 0, 1, 2, 3):
        m = transvae.DiT(h, 2, D, 64, 1, 5, generator=torch.Generator().manual_seed(1))
        runs.append(transvae.fit_dit(str(tmp_path), m, epochs=2, batch_size=4, lr=1e-3, seed=seed, log_every=3, device=dev()))
    r = runs[0]
    assert r["steps"] == 2 * (3 + 2) and len(r["shard_orders"]) == 2 and all(sorted(o) == [0, 1] for o in r["shard_orders"])
    assert isinstance(r["loss"], float) and 0 < r["loss"] < 10 and [hh["step"] for hh in r["history"]] == [3, 6, 9, 10]
    assert runs[1]["shard_orders"] == r["shard_orders"], "the shard order is reproducible from the seed"
    assert runs[1]["loss"] == pytest.approx(r["loss"], rel=1e-2)          # (the weight gradients' split-K sums vary run to run, row W)
    assert len({json.dumps(x["shard_orders"]) for x in runs}) > 1, "the shard order does not depend on the seed"
