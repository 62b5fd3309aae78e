"""csrc/attention_hd.hip (the head_dim 72 family) and the XL constructors on the device: attention forward and backward per (image,
head) slice against the ideal-kernel emulation under DESIGN.md section 3.1 row Y (row A's criteria), tv_rope_qk_hd and the qk-norm
pair against fp64 with slack (row J's), head isolation inside NaN-filled memory (the padding rule), bit-reproducibility, and the
whole models at width 288 = 4 heads of 72 against the plain-torch restatement (tests/hd72_restatement.py) under the bf16 tier's
yardstick, with the sampler, a short training run and one fit_dit -> evaluate_dit round trip."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

import hd72_restatement as H
from test_dit_host import U, check_report, fp32_ratio
from test_error_budget_host import LSE_C, attn_exact, attn_fwd_emul, check_fp32, check_vs_emulation, lse_terms, one_rounding_report

pytestmark = pytest.mark.gpu

FLOOR, MARGIN = 1e-2, 1.25        # the DiT yardstick: relL2 within max(1e-2, 1.25 x the restatement's own bf16 deviation)
SENTINEL = 7.5
GUARD = 4096                      # elements in front of and behind every tensor handed to a kernel (a multiple of 16 bytes)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
HD = H.HD


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from transvae.hip import _lib as L
    return L, L.load()


def golden():
    with open(H.GOLDEN) as f:
        return json.load(f)


class Guarded:
    """a tensor of `shape` in the middle of a larger allocation filled with `fill` (NaN around inputs, a sentinel around outputs)"""

    def __init__(self, shape, dtype, fill, src=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.n, self.fill = n, fill
        if src is not None:
            self.t.copy_(src.to(dev()))

    def take(self):
        edge = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        same = torch.isnan(edge) if self.fill != self.fill else edge == self.fill
        assert bool(same.all()), "wrote outside the tensor"
        return self.t.cpu()


def nan_in(t):
    return Guarded(t.shape, t.dtype, float("nan"), t)


def out_of(shape, dtype=BF):
    return Guarded(shape, dtype, SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def run_attn(qkv, do, tab=None, backward=True):
    """tv_attn_fwd_hd and tv_attn_bwd_hd through the C ABI: every input a view inside NaN-filled memory, every output a view inside
    sentinel-filled memory -> dict of host tensors (delta: the scratch's first plane, -delta)"""
    L, lib = _lib()
    B, N, _, heads, _ = qkv.shape
    q_in = nan_in(qkv)
    o, lse = out_of((B, N, heads, HD)), out_of((B, heads, N), F32)
    L.check(lib.tv_attn_fwd_hd(_p(q_in.t), _p(o.t), _p(lse.t), B, N, heads, HD, H.SCALE, _stream()), "tv_attn_fwd_hd")
    res = {}
    if backward:
        g_in, dqkv, delta = nan_in(do), out_of(qkv.shape), out_of((2, B, heads, N), F32)
        tb = None if tab is None else nan_in(tab)
        L.check(lib.tv_attn_bwd_hd(_p(q_in.t), _p(o.t), _p(g_in.t), _p(lse.t), _p(delta.t), None if tb is None else _p(tb.t), _p(dqkv.t), B, N, heads,
                                   HD, H.SCALE, _stream()), "tv_attn_bwd_hd")
        torch.cuda.synchronize()
        res.update(dqkv=dqkv.take(), delta=delta.take()[0])
    torch.cuda.synchronize()
    res.update(o=o.take(), lse=lse.take())
    assert torch.equal(q_in.take().view(torch.int16), qkv.view(torch.int16)), "the kernels leave qkv alone"
    return res


_attn_cache = {}


def attn_case(B, N, heads):
    """inputs, the device results without and with the table, and per slice the exact forward and its emulation (computed once)"""
    key = (B, N, heads)
    if key not in _attn_cache:
        qkv, do = H.attn_inputs(B, N, heads, seed=B + N + heads)
        tab = H.table_of(N)
        plain = run_attn(qkv, do)
        roped = run_attn(qkv, do, tab) if tab is not None else None
        fwd = {}
        for b in range(B):
            for h in range(heads):
                q, k, v = (qkv[b, :, i, h] for i in range(3))
                fwd[b, h] = (attn_exact(q, k, v, H.SCALE), attn_fwd_emul(q, k, v, H.SCALE))
        _attn_cache[key] = (qkv, do, tab, plain, roped, fwd)
    return _attn_cache[key]


@pytest.mark.parametrize("B,N,heads", H.SHAPES)
def test_attention_forward_against_the_emulation(B, N, heads):
    qkv, do, tab, plain, roped, fwd = attn_case(B, N, heads)
    worst = [0.0, 0.0, 0.0]
    for (b, h), ((o_ex, lse_ex), (o_e, _)) in fwd.items():
        q, k = qkv[b, :, 0, h], qkv[b, :, 1, h]
        r = check_vs_emulation(plain["o"][b, :, h], o_e, o_ex, f"o[{b}, {h}]")
        rl = check_fp32(plain["lse"][b, h], lse_ex, lse_terms(q, k, lse_ex, H.SCALE), LSE_C, f"lse[{b}, {h}]")
        worst = [max(a, c) for a, c in zip(worst, (*r, rl))]
    report(f"attn72 fwd {B}x{N}x{heads} (relL2 ratio, max ratio, lse ratio)", worst)
    if roped is not None:
        assert torch.equal(roped["o"], plain["o"]) and torch.equal(roped["lse"], plain["lse"])


@pytest.mark.parametrize("B,N,heads", H.SHAPES)
def test_attention_backward_against_the_emulation(B, N, heads):
    qkv, do, tab, plain, roped, _ = attn_case(B, N, heads)
    for name, got, tb in (("no table", plain, None), ("table", roped, tab)):
        if got is None:
            continue
        worst = [0.0] * 4
        for b in range(B):
            for h in range(heads):
                q, k, v = (qkv[b, :, i, h] for i in range(3))
                args = (q, k, v, got["o"][b, :, h], do[b, :, h], got["lse"][b, h], H.SCALE)
                ex, em = H.attn_bwd_exact(*args, tab=tb), H.attn_bwd_emul(*args, tab=tb)
                for i, nm in enumerate(("dq", "dk", "dv")):
                    r = check_vs_emulation(got["dqkv"][b, :, i, h], em[i], ex[i], f"{nm}[{b}, {h}] {name}")
                    worst[i] = max(worst[i], r[0])
                terms = (do[b, :, h].to(F64) * got["o"][b, :, h].to(F64)).abs().sum(1)
                worst[3] = max(worst[3], check_fp32(-got["delta"][b, h], ex[3], terms, 16.0, f"delta[{b}, {h}]"))
        report(f"attn72 bwd {B}x{N}x{heads} {name} (relL2 ratios dq, dk, dv; delta ratio)", worst)
    if roped is not None:
        assert torch.equal(roped["dqkv"][:, :, 2], plain["dqkv"][:, :, 2]) and torch.equal(roped["delta"], plain["delta"]), "dv and delta do not see the table"


def test_head_isolation_inside_nan_memory():
    """The padding rule.  One (image, head) of qkv and do is NaN, everything around every tensor is NaN: every other slice is finite and
    bit-equal to the same slice computed alone as B = 1, heads = 1 -- a pad obtained by loading the neighbour turns into NaN here."""
    B, N, heads = 2, 65, 3
    qkv, do = H.attn_inputs(B, N, heads, seed=11)
    tab = H.table_of(N)
    qkv[1, :, :, 1], do[1, :, 1] = float("nan"), float("nan")
    for tb in (None, tab):
        got = run_attn(qkv, do, tb)
        for b in range(B):
            for h in range(heads):
                if (b, h) == (1, 1):
                    continue
                alone = run_attn(qkv[b:b + 1, :, :, h:h + 1].contiguous(), do[b:b + 1, :, h:h + 1].contiguous(), tb)
                for k, a, w in (("o", got["o"][b, :, h], alone["o"][0, :, 0]), ("lse", got["lse"][b, h], alone["lse"][0, 0]),
                                ("dqkv", got["dqkv"][b, :, :, h], alone["dqkv"][0, :, :, 0])):
                    assert bool(torch.isfinite(a).all()), (k, b, h)
                    assert torch.equal(a, w), (k, b, h)


def test_last_head_vector_is_the_last_thing_read():
    """(2, 1, 1): one token, one head; the v third of the last token ends the tensor, and NaN follows it"""
    qkv, do = H.attn_inputs(2, 1, 1, seed=3)
    got = run_attn(qkv, do, H.table_of(1))
    assert torch.equal(got["o"].view(torch.int16), qkv[:, :, 2].view(torch.int16)), "one key: o is v"
    assert bool(torch.isfinite(got["dqkv"]).all())
    assert float(got["dqkv"][:, :, :2].float().abs().max()) <= 2.0 ** -14, "one key: dP = delta up to the order of two fp32 sums, so dq, dk ~ 0"
    assert torch.equal(got["dqkv"][:, :, 2].view(torch.int16), do.view(torch.int16)), "one key: dv is do"


def test_argument_checks():
    L, lib = _lib()
    x = torch.zeros(3 * 64, dtype=BF, device=dev())
    f = torch.zeros(64, dtype=F32, device=dev())
    for hd in (64, 80, 0):
        assert lib.tv_attn_fwd_hd(_p(x), _p(x), _p(f), 1, 1, 1, hd, 0.125, None) != 0 and "head_dim" in lib.tv_last_error().decode()
        assert lib.tv_attn_bwd_hd(_p(x), _p(x), _p(x), _p(f), _p(f), None, _p(x), 1, 1, 1, hd, 0.125, None) != 0 and "head_dim" in lib.tv_last_error().decode()
        assert lib.tv_rope_qk_hd(_p(x), _p(f), 1, 1, 1, hd, 0, None) != 0 and "head_dim" in lib.tv_last_error().decode()
        assert lib.tv_qknorm_rope_fwd_hd(_p(x), _p(f), _p(f), None, _p(x), 1, 1, 1, hd, 1e-6, None) != 0 and "head_dim" in lib.tv_last_error().decode()
        assert lib.tv_qknorm_rope_bwd_hd(_p(x), _p(f), _p(f), _p(x), _p(f), _p(f), _p(f), 1, 1, 1, hd, 1e-6, None) != 0
        assert "head_dim" in lib.tv_last_error().decode()
        assert lib.tv_qknorm_rope_bwd_hd_partial_count(1, 1, 1, hd) == -1
    assert lib.tv_attn_fwd_hd(_p(x), _p(x), _p(f), 1, 0, 1, 72, 0.125, None) != 0
    assert lib.tv_attn_fwd_hd(_p(x), None, _p(f), 1, 1, 1, 72, 0.125, None) != 0
    from transvae.hip import ops
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attention(torch.zeros(1, 1, 240, dtype=BF, device=dev()), None, 1, 0.1, head_dim=80)


# ---------------------------------------------------------------------------------------------------------------------------
# tv_rope_qk_hd and the qk-norm pair
# ---------------------------------------------------------------------------------------------------------------------------
QK_SHAPES = [s for s in H.SHAPES if H.GRIDS[s[1]] is not None]


@pytest.mark.parametrize("B,N,heads", QK_SHAPES)
def test_rope_qk_against_fp64(B, N, heads):
    L, lib = _lib()
    q = H.qk_inputs(B, N, heads, seed=B + N + heads)
    tab = nan_in(q["tab"])
    for kind, tr in (("forward", 0), ("adjoint", 1)):
        x = nan_in(q["qkv"])
        L.check(lib.tv_rope_qk_hd(_p(x.t), _p(tab.t), B, N, heads, HD, tr, _stream()), "tv_rope_qk_hd")
        torch.cuda.synchronize()
        got = x.take()
        y64, slack = H.rope_qk64(q["qkv"], q["tab"], N, kind)
        rep = one_rounding_report(got[:, :2], y64[:, :2], slack[:, :2])
        report(f"rope_qk72 {kind} {B}x{N}x{heads}", rep)
        check_report(rep, f"rope_qk72 {kind}")
        assert torch.equal(got[:, 2], q["qkv"][:, 2]), "the v third is untouched"
        assert torch.equal(got, H.rope_qk_emulate(q["qkv"], q["tab"], N, kind)), "two products and their sum in fp32, rounded once"


def run_qk(q, B, N, heads, with_tab=True, one_weight=False):
    """forward out of place and in place, then the backward, through the C ABI"""
    L, lib = _lib()
    ones = torch.ones(HD, device=dev())
    wq, wk = (ones, ones) if one_weight else (q["wq"].to(dev()), q["wk"].to(dev()))
    tab = nan_in(q["tab"]).t if with_tab else None
    src, out, inplace = nan_in(q["qkv"]), out_of(q["qkv"].shape), nan_in(q["qkv"])
    L.check(lib.tv_qknorm_rope_fwd_hd(_p(src.t), _p(wq), _p(wk), _p(tab), _p(out.t), B, N, heads, HD, H.LN_EPS, _stream()), "tv_qknorm_rope_fwd_hd")
    L.check(lib.tv_qknorm_rope_fwd_hd(_p(inplace.t), _p(wq), _p(wk), _p(tab), _p(inplace.t), B, N, heads, HD, H.LN_EPS, _stream()), "tv_qknorm_rope_fwd_hd")
    dqkv = nan_in(q["dqkv"])
    dw = out_of((2, HD), F32)
    part = torch.empty(lib.tv_qknorm_rope_bwd_hd_partial_count(B, N, heads, HD), dtype=F32, device=dev())
    L.check(lib.tv_qknorm_rope_bwd_hd(_p(src.t), _p(wq), _p(wk), _p(dqkv.t), _p(dw.t[0]), _p(dw.t[1]), _p(part), B, N, heads, HD, H.LN_EPS, _stream()),
            "tv_qknorm_rope_bwd_hd")
    torch.cuda.synchronize()
    assert torch.equal(src.take(), q["qkv"]), "the out-of-place forward and the backward leave qkv alone"
    dwv = dw.take()
    return {"out": out.take(), "inplace": inplace.take(), "dqkv": dqkv.take(), "dwq": dwv[0], "dwk": dwv[1]}


@pytest.mark.parametrize("B,N,heads", QK_SHAPES)
def test_qknorm_rope_against_fp64(B, N, heads):
    q = H.qk_inputs(B, N, heads, seed=B + N + heads)
    for with_tab in (True, False):
        got = run_qk(q, B, N, heads, with_tab)
        y64, slack = H.qknorm_fwd64(q["qkv"], q["wq"], q["wk"], q["tab"] if with_tab else None, N)
        rep = one_rounding_report(got["out"][:, :2], y64[:, :2], slack[:, :2])
        report(f"qknorm72_rope_fwd {B}x{N}x{heads} table={with_tab}", rep)
        check_report(rep, "qknorm72_rope_fwd")
        assert torch.equal(got["out"], got["inplace"]), "in place and out of place give the same bits"
        assert torch.equal(got["out"][:, 2], q["qkv"][:, 2]), "the v third is copied bit for bit"
        assert not bool(got["out"][0, 0, 0].any()), "a zero head vector gives exactly 0"
    ref = H.qknorm_bwd64(q["qkv"], q["wq"], q["wk"], q["dqkv"])
    rep = one_rounding_report(got["dqkv"][:, :2], ref["dqkv"][:, :2], ref["slack"][:, :2])
    rq, rk = fp32_ratio(got["dwq"], ref["dwq"], ref["dwq_bound"]), fp32_ratio(got["dwk"], ref["dwk"], ref["dwk_bound"])
    report(f"qknorm72_rope_bwd {B}x{N}x{heads}", (rep, rq, rk))
    check_report(rep, "qknorm72_rope_bwd")
    assert rq <= 1.0 and rk <= 1.0, (rq, rk)
    assert torch.equal(got["dqkv"][:, 2], q["dqkv"][:, 2]), "dv is untouched"
    assert bool(torch.isfinite(got["dqkv"]).all()), "the zero head vector's gradient"
    a, b = run_qk(q, B, N, heads, True, one_weight=True), run_qk(q, B, N, heads, False, one_weight=True)
    assert torch.equal(a["out"][0::N], b["out"][0::N]), "at position 0 with weight 1 the output is bf16(q r)"


def test_bit_reproducibility():
    import transvae
    from transvae.hip import ops
    from transvae.lightning_dit import qk_norm_rope_attention
    B, N, heads = 3, 65, 2
    qkv, do = H.attn_inputs(B, N, heads, seed=5)
    tab = H.table_of(N)
    a, b = run_attn(qkv, do, tab), run_attn(qkv, do, tab)
    for k in ("o", "lse", "dqkv", "delta"):
        assert torch.equal(a[k], b[k]), k
    q = H.qk_inputs(B, N, heads, seed=6)
    a, b = run_qk(q, B, N, heads), run_qk(q, B, N, heads)
    for k in ("out", "dqkv", "dwq", "dwk"):
        assert torch.equal(a[k], b[k]), k

    def wrapped():
        x = qkv.reshape(B, N, 3 * heads * HD).to(dev()).requires_grad_(True)
        wq, wk = (q[n].to(dev()).requires_grad_(True) for n in ("wq", "wk"))
        o = qk_norm_rope_attention(x, wq, wk, tab.to(dev()), heads, H.SCALE, H.LN_EPS, head_dim=72)
        o.backward(do.reshape(B, N, heads * HD).to(dev()))
        x2 = qkv.reshape(B, N, 3 * heads * HD).to(dev()).requires_grad_(True)
        o2 = ops.attention(x2.clone(), tab.to(dev()), heads, H.SCALE, head_dim=72)
        o2.backward(do.reshape(B, N, heads * HD).to(dev()))
        return [t.detach().cpu() for t in (o, x.grad, wq.grad, wk.grad, o2, x2.grad)]
    first = wrapped()
    with transvae.deterministic():
        det = [wrapped(), wrapped()]
    for i, (u, v, w) in enumerate(zip(first, *det)):
        assert torch.equal(u, v) and torch.equal(v, w), i


# ---------------------------------------------------------------------------------------------------------------------------
# the whole models at width 288 = 4 heads of 72
# ---------------------------------------------------------------------------------------------------------------------------
def hip_model(case, sd):
    import transvae
    cfg = H.MODEL_CASES[case]
    if case == "dit":
        m = transvae.DiT(**{k: v for k, v in cfg.items() if not k.startswith("use_")}, **H.MODEL_ARGS)
    else:
        m = transvae.LightningDiT(**cfg, **H.MODEL_ARGS)
    assert m.num_heads == 4 and m.head_dim == 72
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
    return H.R.unpatchify(v[:, :m.patch_cols].float().cpu().reshape(batch["t"].shape[0], m.tokens, m.patch_cols), m.in_channels, h, w, m.patch_size)


@pytest.mark.parametrize("case", list(H.MODEL_CASES))
def test_whole_model_against_the_restatement(case):
    gold = golden()["cases"][case]
    sd, batch = H.make_state(case, gold["seeds"]["state"], True), H.make_batch(case, gold["seeds"]["batch"])
    v32, l32, g32 = H.flow_step(H.build(case, sd), batch)
    m = hip_model(case, sd)
    dv = H.rel_l2(hip_velocity(m, batch), v32)
    loss = hip_step(m, batch)
    dl = abs(loss - float(l32)) / float(l32)
    report(f"hd72 {case} velocity relL2 (bound {max(FLOOR, MARGIN * gold['velocity']):.3g})", dv)
    report(f"hd72 {case} loss relative (bound {max(FLOOR, MARGIN * gold['loss']):.3g})", dl)
    worst = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        worst[k] = (H.rel_l2(p.grad, g32[k]), max(FLOOR, MARGIN * gold["grads"][k]))
    for k, (e, bound) in sorted(worst.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:6]:
        report(f"hd72 {case} d({k}) relL2 (bound {bound:.3g})", e)
    assert dv <= max(FLOOR, MARGIN * gold["velocity"]) and dl <= max(FLOOR, MARGIN * gold["loss"])
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("case", H.SAMPLER_CASES)
def test_sampler_against_the_restatement(case):
    import transvae
    gold = golden()["sampler"][case]
    sd, batch = H.make_state(case, gold["seeds"]["state"], True), H.make_batch(case, gold["seeds"]["batch"])
    ref = H.sample(H.build(case, sd), batch["labels"], batch["noise"], batch["stats"], gold["steps"], gold["cfg_scale"])
    m = hip_model(case, sd)
    got = transvae.sample_latents(m, batch["labels"].to(dev()), steps=gold["steps"], cfg_scale=gold["cfg_scale"], stats=batch["stats"],
                                  noise=batch["noise"].to(dev()))
    assert got.dtype == torch.float32 and got.shape == batch["noise"].shape
    e = H.rel_l2(got, ref)
    report(f"hd72 {case} sampler relL2 (bound {max(FLOOR, MARGIN * gold['latents']):.3g})", e)
    assert e <= max(FLOOR, MARGIN * gold["latents"])


@pytest.mark.parametrize("case", H.SAMPLER_CASES)
def test_thirty_training_steps_halve_the_loss(case):
    from transvae.optim import FusedAdamW
    gold = golden()["train"][case]
    assert gold["final_loss"] < 0.5 * gold["first_loss"]
    sd, batch = H.make_state(case, gold["seeds"]["state"], False), H.make_batch(case, gold["seeds"]["batch"])
    m = hip_model(case, sd)
    opt = FusedAdamW(m.parameters(), lr=gold["lr"], weight_decay=0.0)
    losses = []
    for _ in range(gold["steps"]):
        losses.append(hip_step(m, batch))
        opt.step()
    losses.append(hip_step(m, batch))
    report(f"hd72 {case} training losses first / last (restatement: %.4g / %.4g)" % (gold["first_loss"], gold["final_loss"]), (losses[0], losses[-1]))
    assert losses[0] == pytest.approx(gold["first_loss"], rel=1e-3)
    assert losses[-1] < 0.5 * losses[0]


class StubVAE:
    """decode: the first three latent channels, up-sampled 4x: [B, 4, 8, 8] -> [B, 3, 32, 32]"""

    def decode(self, lat):
        return F.interpolate(0.25 * lat[:, :3].float() + 0.5, scale_factor=4, mode="nearest")


@pytest.mark.parametrize("kind", ["DiT", "LightningDiT"])
def test_fit_dit_and_evaluate_dit_round_trip(tmp_path, kind):
    import transvae
    import fid_restatement as FR
    from probe_restatement import write_split
    g = torch.Generator().manual_seed(0)
    D, h = 4, 8
    shards = []
    for n in (10, 6):
        lat = torch.randn(n, 2 * D, h, h, generator=g)          # what="moments" shards: the mu half is used
        shards.append({"latents": lat, "latents_flip": lat.flip(-1), "labels": torch.randint(0, 5, (n,), generator=g)})
    stats = {"mean": torch.zeros(1, D, 1, 1), "std": torch.ones(1, D, 1, 1)}
    write_split(str(tmp_path), shards, stats)
    m = getattr(transvae, kind)(h, 2, D, 288, 1, 5, generator=torch.Generator().manual_seed(1), head_dim=72)
    assert m.num_heads == 4
    r = transvae.fit_dit(str(tmp_path), m, epochs=2, batch_size=4, lr=1e-3, seed=0, log_every=3, device=dev(), ema_decay=0.9)
    assert r["steps"] == 2 * (3 + 2) and isinstance(r["loss"], float) and 0 < r["loss"] < 10 and r["ema"].num_updates == r["steps"]
    net = transvae.InceptionFeatures().load_fid_state_dict(FR.plain_state_dict()).to(dev())
    imgs = FR.smooth_images(48, 32, 32, 123)
    reference = transvae.reference_statistics([(imgs[:24], None), (imgs[24:], None)], net)
    kw = dict(fid_net=net, num_samples=48, batch_size=16, steps=2, cfg_scale=1.5, metrics=("gfid",), stats=stats)
    own = transvae.evaluate_dit(StubVAE(), m, reference, **kw)
    avg = transvae.evaluate_dit(StubVAE(), m, reference, ema=r["ema"], **kw)
    assert own["n"] == 48 and all(0 <= float(x["gfid"]) < float("inf") for x in (own, avg))
    assert own["gfid"] != avg["gfid"], "the weight average is another model"
