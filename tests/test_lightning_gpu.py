"""csrc/lightning.hip and transvae/lightning_dit.py on the device: the six kernels through the C ABI against fp64 under DESIGN.md
section 3.1 row J, their exact cases and bit-reproducibility, the whole model under each switch, the sampler and a short training
run against the plain-torch restatement (tests/lightning_restatement.py) under the bf16 tier's yardstick, and `fit_dit` with a weight
EMA end to end on a two-shard directory."""
import ctypes as C
import json

import pytest
import torch

import lightning_restatement as LR
from test_dit_host import U, check_report, fp32_ratio, sl
from test_error_budget_host import one_rounding_report
from test_lightning_host import check_swiglu_exact

pytestmark = pytest.mark.gpu

FLOOR, MARGIN = 1e-2, 1.25        # the DiT yardstick: relL2 within max(1e-2, 1.25 x the restatement's own bf16 deviation)
SENTINEL = 7.5
BF = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def golden():
    with open(LR.GOLDEN) as f:
        return json.load(f)


def guarded(rows, cols, dtype=BF):
    """an output with one sentinel row past what the kernel may write"""
    return torch.full((rows + 1, cols), SENTINEL, dtype=dtype, device=dev())


def guarded_copy(t):
    """`t` as rows of 64 with one sentinel row behind it"""
    buf = guarded(t.numel() // 64, 64, t.dtype)
    buf[:-1] = t.reshape(-1, 64).to(dev())
    return buf


def take(buf):
    assert bool((buf[-1] == SENTINEL).all()), "wrote past the output"
    return buf[:-1].cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# RMSNorm adaLN
# ---------------------------------------------------------------------------------------------------------------------------
def run_rms(inp, B, N, with_dres):
    """the pair through the C ABI on slices at non-zero offsets of one [B, 4 C] matrix"""
    from transvae.hip import _lib as L
    lib = L.load()
    C_ = inp["x"].shape[1]
    T, ld = B * N, 4 * C_
    d = {k: v.to(dev()) for k, v in inp.items() if torch.is_tensor(v)}
    so, ko = inp["shift_off"], inp["scale_off"]
    y, dx = guarded(T, C_), guarded(T, C_)
    dmod = torch.full((B + 1, ld), SENTINEL, dtype=torch.float32, device=dev())
    dw = guarded(1, C_, torch.float32)
    L.check(lib.tv_adaln_rms_fwd(_p(d["x"]), _p(d["w"]), _p(d["mod"]), so, ko, ld, _p(y), B, N, C_, LR.LN_EPS, _stream()), "tv_adaln_rms_fwd")
    part = torch.empty(lib.tv_adaln_rms_bwd_partial_count(B, N, C_), dtype=torch.float32, device=dev())
    L.check(lib.tv_adaln_rms_bwd(_p(d["x"]), _p(d["w"]), _p(d["mod"]), so, ko, ld, _p(d["dy"]), _p(d["dres"]) if with_dres else None, _p(dx),
                                 _p(dmod), _p(dw), _p(part), B, N, C_, LR.LN_EPS, _stream()), "tv_adaln_rms_bwd")
    torch.cuda.synchronize()
    dm = take(dmod)
    written = torch.zeros(ld, dtype=torch.bool)
    for o in (so, ko):
        written[o:o + C_] = True
    assert bool((dm[:, ~written] == SENTINEL).all()), "the backward wrote outside its column ranges"
    return {"y": take(y), "dx": take(dx), "dshift": dm[:, so:so + C_], "dscale": dm[:, ko:ko + C_], "dw": take(dw)[0]}


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("B,N,C_", LR.ROW_SHAPES)
def test_rms_adaln_against_fp64(B, N, C_, with_dres):
    inp = LR.row_inputs(B, N, C_, seed=B + N + C_)
    got = run_rms(inp, B, N, with_dres)
    shift, scale = sl(inp, "shift_off"), sl(inp, "scale_off")
    y64, slack = LR.adaln_rms_fwd64(inp["x"], inp["w"], shift, scale, N)
    rep = one_rounding_report(got["y"], y64, slack)
    report(f"adaln_rms_fwd {B}x{N}x{C_}", rep)
    check_report(rep, "adaln_rms_fwd")
    assert torch.equal(got["y"][:N], shift[0].to(BF).expand(N, C_)), "scale = -1 must give bf16(shift)"
    assert torch.equal(got["y"][:, 3], LR.R._per_row(shift, N)[:, 3].to(BF)), "w = 0 must give bf16(shift)"
    assert torch.equal(got["y"][-1], shift[-1].to(BF)), "the all-zero row"
    assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["dx"]).all()), "the all-zero row"
    ref = LR.adaln_rms_bwd64(inp["x"], inp["w"], scale, inp["dy"], inp["dres"] if with_dres else None, N)
    rep = one_rounding_report(got["dx"], ref["dx"], ref["dx_slack"])
    rs = fp32_ratio(got["dshift"], ref["dshift"], ref["k_rows"] * U * ref["dshift_terms"])
    rq = fp32_ratio(got["dscale"], ref["dscale"], ref["dscale_bound"])
    rw = fp32_ratio(got["dw"], ref["dw"], ref["dw_bound"])
    report(f"adaln_rms_bwd {B}x{N}x{C_} dres={with_dres}", (rep, rs, rq, rw))
    check_report(rep, "adaln_rms_bwd dx")
    assert rs <= 1.0 and rq <= 1.0 and rw <= 1.0, (rs, rq, rw)
    assert not bool(got["dscale"][:, 3].any()), "w = 0 shuts that column's dscale"


# ---------------------------------------------------------------------------------------------------------------------------
# qk-norm + RoPE
# ---------------------------------------------------------------------------------------------------------------------------
def run_qk(q, B, N, heads, with_tab=True, one_weight=False):
    """forward out of place and in place, then the backward, through the C ABI"""
    from transvae.hip import _lib as L
    lib = L.load()
    ones = torch.ones(64, device=dev())
    wq, wk = (ones, ones) if one_weight else (q["wq"].to(dev()), q["wk"].to(dev()))
    tab = q["tab"].to(dev()) if with_tab else None
    src, out, inplace = guarded_copy(q["qkv"]), guarded(B * N * 3 * heads, 64), guarded_copy(q["qkv"])
    L.check(lib.tv_qknorm_rope_fwd(_p(src), _p(wq), _p(wk), _p(tab), _p(out), B, N, heads, LR.LN_EPS, _stream()), "tv_qknorm_rope_fwd")
    L.check(lib.tv_qknorm_rope_fwd(_p(inplace), _p(wq), _p(wk), _p(tab), _p(inplace), B, N, heads, LR.LN_EPS, _stream()), "tv_qknorm_rope_fwd")
    dqkv = guarded_copy(q["dqkv"])
    dw = guarded(2, 64, torch.float32)
    part = torch.empty(lib.tv_qknorm_rope_bwd_partial_count(B, N, heads), dtype=torch.float32, device=dev())
    L.check(lib.tv_qknorm_rope_bwd(_p(src), _p(wq), _p(wk), _p(dqkv), _p(dw[0]), _p(dw[1]), _p(part), B, N, heads, LR.LN_EPS, _stream()),
            "tv_qknorm_rope_bwd")
    torch.cuda.synchronize()
    shape = q["qkv"].shape
    assert torch.equal(take(src).reshape(shape), q["qkv"]), "the out-of-place forward and the backward leave qkv alone"
    dwv = take(dw)
    return {"out": take(out).reshape(shape), "inplace": take(inplace).reshape(shape), "dqkv": take(dqkv).reshape(shape), "dwq": dwv[0], "dwk": dwv[1]}


@pytest.mark.parametrize("B,N,heads", LR.QK_SHAPES)
def test_qknorm_rope_against_fp64(B, N, heads):
    q = LR.qk_inputs(B, N, heads, seed=B + N + heads)
    for with_tab in (True, False):
        got = run_qk(q, B, N, heads, with_tab)
        y64, slack = LR.qknorm_fwd64(q["qkv"], q["wq"], q["wk"], q["tab"] if with_tab else None, N)
        rep = one_rounding_report(got["out"][:, :2], y64[:, :2], slack[:, :2])
        report(f"qknorm_rope_fwd {B}x{N}x{heads} table={with_tab}", rep)
        check_report(rep, "qknorm_rope_fwd")
        assert torch.equal(got["out"], got["inplace"]), "in place and out of place give the same bits"
        assert torch.equal(got["out"][:, 2], q["qkv"][:, 2]), "the v third is copied bit for bit"
        assert not bool(got["out"][0, 0, 0].any()), "a zero head vector gives exactly 0"
    ref = LR.qknorm_bwd64(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    rep = one_rounding_report(got["dqkv"][:, :2], ref["dqkv"][:, :2], ref["slack"][:, :2])
    rq, rk = fp32_ratio(got["dwq"], ref["dwq"], ref["dwq_bound"]), fp32_ratio(got["dwk"], ref["dwk"], ref["dwk_bound"])
    report(f"qknorm_rope_bwd {B}x{N}x{heads}", (rep, rq, rk))
    check_report(rep, "qknorm_rope_bwd")
    assert rq <= 1.0 and rk <= 1.0, (rq, rk)
    assert torch.equal(got["dqkv"][:, 2], q["dqkv"][:, 2]), "dv is untouched"
    assert bool(torch.isfinite(got["dqkv"]).all()), "the zero head vector's gradient"
    a, b = run_qk(q, B, N, heads, True, one_weight=True), run_qk(q, B, N, heads, False, one_weight=True)
    assert torch.equal(a["out"][0::N], b["out"][0::N]), "at position 0 with weight 1 the output is bf16(q r)"


# ---------------------------------------------------------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------------------------------------------------------
def run_swiglu(s, T, Hp):
    from transvae.hip import _lib as L
    lib = L.load()
    u, dh = s["u"].to(dev()), s["dh"].to(dev())
    h, du = guarded(T, Hp), guarded(T, 2 * Hp)
    L.check(lib.tv_swiglu_fwd(_p(u), _p(h), T, Hp, _stream()), "tv_swiglu_fwd")
    L.check(lib.tv_swiglu_bwd(_p(u), _p(dh), _p(du), T, Hp, _stream()), "tv_swiglu_bwd")
    torch.cuda.synchronize()
    return take(h), take(du)


@pytest.mark.parametrize("T,Hp", LR.SWIGLU_SHAPES)
def test_swiglu_against_fp64(T, Hp):
    s = LR.swiglu_inputs(T, Hp, seed=T + Hp)
    h, du = run_swiglu(s, T, Hp)
    h64, hs = LR.swiglu_fwd64(s["u"])
    d64, ds = LR.swiglu_bwd64(s["u"], s["dh"])
    rh, rd = one_rounding_report(h, h64, hs), one_rounding_report(du, d64, ds)
    report(f"swiglu {T}x{Hp}", (rh, rd))
    check_report(rh, "swiglu_fwd")
    check_report(rd, "swiglu_bwd")
    check_swiglu_exact(s, h, du)


def test_reductions_are_bit_reproducible():
    B, N, C_ = 3, 65, 128
    inp = LR.row_inputs(B, N, C_, seed=3)
    a, b = run_rms(inp, B, N, True), run_rms(inp, B, N, True)
    for k in ("dx", "dshift", "dscale", "dw"):
        assert torch.equal(a[k], b[k]), k
    q = LR.qk_inputs(2, 64, 16, seed=4)
    a, b = run_qk(q, 2, 64, 16), run_qk(q, 2, 64, 16)
    for k in ("dqkv", "dwq", "dwk"):
        assert torch.equal(a[k], b[k]), k
    s = LR.swiglu_inputs(195, 352, seed=5)
    assert torch.equal(run_swiglu(s, 195, 352)[1], run_swiglu(s, 195, 352)[1])


# ---------------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------------
def hip_model(case, sd):
    import transvae
    m = transvae.LightningDiT(**LR.MODEL_CASES[case], **LR.MODEL_ARGS)
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
    return LR.R.unpatchify(v[:, :m.patch_cols].float().cpu().reshape(batch["t"].shape[0], m.tokens, m.patch_cols), m.in_channels, h, w, m.patch_size)


@pytest.mark.parametrize("case", ["f16d32_p1", "f8d16_p2"])
def test_public_initialisation_is_adaln_zero(case):
    batch = LR.make_batch(case, 21)
    m = hip_model(case, LR.make_state(case, 20, False))
    v = hip_velocity(m, batch)
    assert not bool(v.any()), "the zero-initialised final layer must give exactly 0"
    loss = hip_step(m, batch)
    x = (batch["latents"].double() - batch["stats"]["mean"].double()) / batch["stats"]["std"].double()
    assert loss == pytest.approx(float(((x - batch["noise"].double()) ** 2).mean()), rel=1e-5)
    assert float(m.final_layer.linear.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("case", list(LR.MODEL_CASES))
def test_whole_model_against_the_restatement(case):
    gold = golden()["cases"][case]
    sd, batch = LR.make_state(case, gold["seeds"]["state"], True), LR.make_batch(case, gold["seeds"]["batch"])
    v32, l32, g32 = LR.flow_step(LR.build(case, sd), batch)
    m = hip_model(case, sd)
    dv = LR.rel_l2(hip_velocity(m, batch), v32)
    loss = hip_step(m, batch)
    dl = abs(loss - float(l32)) / float(l32)
    report(f"{case} velocity relL2 (bound {max(FLOOR, MARGIN * gold['velocity']):.3g})", dv)
    report(f"{case} loss relative (bound {max(FLOOR, MARGIN * gold['loss']):.3g})", dl)
    worst = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        worst[k] = (LR.rel_l2(p.grad, g32[k]), max(FLOOR, MARGIN * gold["grads"][k]))
    for k, (e, bound) in sorted(worst.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:6]:
        report(f"{case} d({k}) relL2 (bound {bound:.3g})", e)
    assert dv <= max(FLOOR, MARGIN * gold["velocity"]) and dl <= max(FLOOR, MARGIN * gold["loss"])
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_sampler_against_the_restatement():
    import transvae
    gold = golden()["sampler"]
    case = gold["case"]
    sd, batch = LR.make_state(case, gold["seeds"]["state"], True), LR.make_batch(case, gold["seeds"]["batch"])
    ref = LR.sample(LR.build(case, sd), batch["labels"], batch["noise"], batch["stats"], gold["steps"], gold["cfg_scale"])
    m = hip_model(case, sd)
    got = transvae.sample_latents(m, batch["labels"].to(dev()), steps=gold["steps"], cfg_scale=gold["cfg_scale"], stats=batch["stats"],
                                  noise=batch["noise"].to(dev()))
    assert got.dtype == torch.float32 and got.shape == batch["noise"].shape
    e = LR.rel_l2(got, ref)
    report(f"sampler relL2 (bound {max(FLOOR, MARGIN * gold['latents']):.3g})", e)
    assert e <= max(FLOOR, MARGIN * gold["latents"])


def test_thirty_training_steps_halve_the_loss():
    from transvae.optim import FusedAdamW
    gold = golden()["train"]
    assert gold["final_loss"] < 0.25 * gold["first_loss"]
    case = gold["case"]
    sd, batch = LR.make_state(case, gold["seeds"]["state"], False), LR.make_batch(case, gold["seeds"]["batch"])
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


def test_fit_dit_with_ema_end_to_end(tmp_path):
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
        m = transvae.LightningDiT(h, 2, D, 64, 1, 5, generator=torch.Generator().manual_seed(1))
        runs.append((m, transvae.fit_dit(str(tmp_path), m, epochs=2, batch_size=4, lr=1e-3, seed=seed, log_every=3, device=dev(), ema_decay=0.9)))
    m, r = runs[0]
    assert r["steps"] == 2 * (3 + 2) and len(r["shard_orders"]) == 2 and all(sorted(o) == [0, 1] for o in r["shard_orders"])
    assert isinstance(r["loss"], float) and 0 < r["loss"] < 10 and [hh["step"] for hh in r["history"]] == [3, 6, 9, 10]
    assert runs[1][1]["shard_orders"] == r["shard_orders"], "the shard order is reproducible from the seed"
    assert len({json.dumps(x["shard_orders"]) for _, x in runs}) > 1, "the shard order does not depend on the seed"
    assert r["ema"].num_updates == r["steps"]
    labels = torch.tensor([0, 4, 5], device=dev())
    noise = torch.randn(3, D, h, h, generator=torch.Generator().manual_seed(2)).to(dev())
    own = transvae.sample_latents(m, labels, steps=3, cfg_scale=1.5, stats=stats, noise=noise)
    with r["ema"].applied(m):
        avg = transvae.sample_latents(m, labels, steps=3, cfg_scale=1.5, stats=stats, noise=noise)
    assert avg.shape == noise.shape and bool(torch.isfinite(avg).all()) and not torch.equal(avg, own)
    assert torch.equal(transvae.sample_latents(m, labels, steps=3, cfg_scale=1.5, stats=stats, noise=noise), own), "the weights come back"
