"""Train-step glue under the rounding contract, GPU side: `csrc/optim.hip`, `csrc/loss.hip` and
`csrc/fold.hip` against fp64 references of the same fp32 inputs, with the per-element bounds of tests/test_glue_host.py (whose
emulations and mutation tests settle those bounds on the CPU).  Shapes and pointer alignment go through the C ABI; the host
wrappers (FusedAdamW, TransVAELoss, fused.fold) are driven where they are the thing under test.  Every buffer a kernel writes
is a view into a larger allocation whose remainder holds a sentinel that is checked afterwards.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_error_budget_host import check_fp32, check_one_rounding, f32, r16, rel_l2  # noqa: F401  (the contract's shared checks)
from test_glue_host import (
    F32, FOLD_C, FOLD_R, LOSS_CLIP, LOSS_N_IMG, LOSS_N_LAT, LOSS_W, OPT_CASES, OPT_CHUNK, PACK_FORMS, adamw_ref64, check_adamw,
    check_fold, check_loss, check_nonfinite, check_norm, err_stats, fold_inputs, fold_ref64, loss_inputs, loss_ref64, loss_scales,
    opt_bias_corrections, opt_case, opt_coef64, opt_hyper, opt_norm64, pack_ref, pack_tiles)

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -7.25          # exactly representable in fp32 and bf16


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def _lib():
    from transvae.hip import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Guarded:
    """`n` elements at element offset `off` of a sentinel-filled allocation with GUARD elements after them"""

    def __init__(self, n, off=0, dtype=torch.float32, init=None):
        self.buf = torch.full((off + n + GUARD,), SENT, dtype=dtype, device=dev())
        self.view = self.buf[off:off + n]
        self.off, self.n = off, n
        if init is not None:
            self.view.copy_(torch.as_tensor(init).reshape(-1).to(dtype))

    def intact(self):
        b = self.buf.cpu().float()
        return bool((b[:self.off] == SENT).all()) and bool((b[self.off + self.n:] == SENT).all())

    def np(self):
        return self.view.cpu().numpy() if self.view.dtype != torch.bfloat16 else self.view.cpu().view(torch.int16).numpy()


def bf16_bits(a):
    """fp32 array -> the bits of torch's round-to-nearest-even bf16"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# [O] tv_opt_grad_norm + tv_opt_adamw through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _chunks(sizes):
    rows = [(i, c) for i, n in enumerate(sizes) for c in range(-(-n // OPT_CHUNK))]
    return torch.tensor(rows, dtype=torch.int32, device=dev()), len(rows)


class OptState:
    """the tensors of one optimizer call on the device.  offs = element offsets of (param, grad, exp_avg, exp_avg_sq);
    shadow: None (absent) or its element offset (bf16: 4 elements = 8 bytes)"""

    def __init__(self, tensors, offs=(0, 0, 0, 0), shadow=0):
        self.t = [[Guarded(a.size, o, init=a) for a, o in zip(tt, offs)] for tt in tensors]
        self.sh = [Guarded(tt[0].size, shadow, torch.bfloat16) for tt in tensors] if shadow is not None else None
        sizes = [tt[0].size for tt in tensors]
        self.table = torch.tensor([[g.view.data_ptr() for g in row] + [self.sh[i].view.data_ptr() if self.sh else 0, sizes[i]]
                                   for i, row in enumerate(self.t)], dtype=torch.int64, device=dev())
        self.chunks, self.n = _chunks(sizes)
        self.partials = torch.zeros(self.n, dtype=torch.float32, device=dev())
        self.ctrl = torch.zeros(8, dtype=torch.float32, device=dev())

    def step(self, hp, max_norm):
        L, lib = _lib()
        L.check(lib.tv_opt_grad_norm(_p(self.table), _p(self.chunks), self.n, _p(self.partials), _p(self.ctrl), float(max_norm or 0.0),
                                     hp["beta1"], hp["beta2"], 1, _stream()), "tv_opt_grad_norm")
        L.check(lib.tv_opt_adamw(_p(self.table), _p(self.chunks), self.n, _p(self.ctrl), hp["lr"], hp["beta1"], hp["beta2"], hp["eps"],
                                 hp["wd"], _stream()), "tv_opt_adamw")
        torch.cuda.synchronize()
        return self.ctrl.cpu().numpy()

    def results(self):
        """per tensor (m', v', p') -- the order of check_adamw -- and the shadows' bits"""
        assert all(g.intact() for row in self.t for g in row), "a write outside a tensor"
        assert self.sh is None or all(g.intact() for g in self.sh), "a write outside a shadow"
        return [(row[2].np(), row[3].np(), row[0].np()) for row in self.t], ([g.np() for g in self.sh] if self.sh else None)


@pytest.mark.parametrize("case", OPT_CASES, ids=str)
def test_adamw_one_step_against_fp64(case):
    """[O] one step over the size table (vector loop only, tail only, both, an exact chunk, a one-element last chunk), gradient
    scales 2^-20 .. 2^10, zero / subnormal-v / opposite-sign elements: the norm within NORM_C, ctrl[5..6] the fp64 bias
    corrections rounded once, m', v', p' inside their per-element bounds, every shadow the bf16 rounding of the new parameter"""
    tensors, hp, t, max_norm, n64, coef, active = opt_case(case)
    st = OptState(tensors)
    st.ctrl[0] = t - 1
    ctrl = st.step(hp, max_norm)
    res, sh = st.results()
    assert ctrl[0] == t and ctrl[3] == 0 and ctrl[4] == 0
    assert (float(ctrl[5]), float(ctrl[6])) == opt_bias_corrections(hp, t)
    fig = {"norm": check_norm(ctrl[1], n64, "norm") if n64 > 0 else float(ctrl[1])}
    if not active:
        assert ctrl[2] == 1.0, ctrl[2]
    worst, ulps = np.zeros(3), np.zeros(3)
    bias = []
    for (p, g, m, v), got, s in zip(tensors, res, sh):
        ref = adamw_ref64(p, g, m, v, coef, active, hp, t)
        stats = [err_stats(got[i], ref[k]) for i, k in enumerate(("m", "v", "p"))]
        report(f"[O] {case} n={p.size} (max ulps, bias) of m', v', p'", [tuple(round(x, 3) for x in s_) for s_ in stats])
        worst = np.maximum(worst, check_adamw(got, ref, f"n={p.size}"))
        ulps = np.maximum(ulps, [s_[0] for s_ in stats])
        bias.append(stats[2][1])
        assert np.array_equal(s, bf16_bits(got[2])), f"n={p.size}: shadow is not bf16(p')"
        if hp["wd"] == 0 or hp["lr"] == 0:
            assert got[2][0] == p[0]                       # g = m = v = 0: no update at all
        assert got[0][0] == 0 and got[1][0] == 0
        if hp["lr"] == 0:
            assert np.array_equal(got[2], p)
    fig.update(ratio_m_v_p=tuple(worst.round(3)), max_ulps=tuple(ulps.round(2)), bias_p=round(float(np.mean(bias)), 4), coef=float(ctrl[2]))
    report(f"[O] adamw {case}", fig)


OPT_ALIGN = [((1, 0, 0, 0), 0), ((0, 1, 0, 0), 0), ((0, 0, 1, 0), 0), ((0, 0, 0, 1), 0), ((0, 0, 0, 0), None), ((0, 0, 0, 0), 1),
             ((2, 3, 1, 2), 3), ((3, 2, 2, 1), None), ((0, 0, 0, 0), 4)]


@pytest.mark.parametrize("case", [OPT_CASES[1], OPT_CASES[8]], ids=str)
def test_adamw_bits_do_not_depend_on_alignment(case):
    """[O] the 16-byte vector loop and the scalar loop give the same bits: each fp32 pointer unaligned by 4 bytes in turn, the
    shadow absent / off its 8-byte alignment, mixed offsets -- the norm, the clip coefficient, m', v', p' and the shadows equal
    the aligned run's"""
    tensors, hp, t, max_norm, *_ = opt_case(case)
    base = OptState(tensors)
    base.ctrl[0] = t - 1
    c0 = base.step(hp, max_norm)
    r0, s0 = base.results()
    diff = 0
    for offs, shadow in OPT_ALIGN:
        st = OptState(tensors, offs, shadow)
        st.ctrl[0] = t - 1
        c1 = st.step(hp, max_norm)
        r1, s1 = st.results()
        assert np.array_equal(c0, c1), f"offsets {offs}: ctrl {c1} differs from the aligned run's {c0}"
        for i, (a, b) in enumerate(zip(r0, r1)):
            for k in range(3):
                d = int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum())
                diff += d
                assert d == 0, f"offsets {offs} shadow {shadow}: tensor {i} output {'mvp'[k]} differs in {d} elements from the aligned run"
            if s1 is not None:
                assert np.array_equal(s0[i], s1[i]), (offs, shadow, i)
    report(f"[O] alignment cases {case}", f"{len(OPT_ALIGN)} cases, {diff} differing elements")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_adamw_skips_a_non_finite_step(bad):
    """[O] one NaN / +inf in the last tail element of an unaligned tensor in the last chunk: parameters, both moments, shadows and
    ctrl[0] bit-unchanged, ctrl[3] = 1, ctrl[4] counts it; the next clean step uses t, not t + 1"""
    tensors, hp, t, max_norm, *_ = opt_case(OPT_CASES[1])
    offs, shadow = (1, 1, 1, 1), 1
    clean = OptState(tensors, offs, shadow)
    clean.ctrl[0] = t - 1
    c_ref = clean.step(hp, max_norm)
    r_ref, s_ref = clean.results()

    st = OptState(tensors, offs, shadow)
    st.ctrl[0] = t - 1
    good = st.t[-1][1].view[-1].clone()
    st.t[-1][1].view[-1] = bad
    before = [[g.buf.clone() for g in row] for row in st.t], [g.buf.clone() for g in st.sh]
    c1 = st.step(hp, max_norm)
    assert c1[0] == t - 1 and c1[3] == 1 and c1[4] == 1, c1
    for row, brow in zip(st.t, before[0]):
        for k in (0, 2, 3):
            assert torch.equal(row[k].buf.view(torch.int32), brow[k].view(torch.int32))
    for g, b in zip(st.sh, before[1]):
        assert torch.equal(g.buf.view(torch.int16), b.view(torch.int16))
    st.t[-1][1].view[-1] = good
    c2 = st.step(hp, max_norm)
    assert c2[0] == t and c2[3] == 0 and c2[4] == 1, c2
    assert np.array_equal(c2[[0, 1, 2, 5, 6]], c_ref[[0, 1, 2, 5, 6]])
    r2, s2 = st.results()
    for a, b, sa, sb in zip(r_ref, r2, s_ref, s2):
        assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in range(3)) and np.array_equal(sa, sb)
    report(f"[O] skip on {bad}", "state bit-unchanged, step counter held, next step equals the clean run's")


def test_cast_shadows_is_the_bf16_rounding():
    """[K] tv_opt_cast_shadows at every size of the table, shadows on and off their alignment"""
    L, lib = _lib()
    tensors, *_ = opt_case(OPT_CASES[0])
    for offs, shadow in (((0, 0, 0, 0), 0), ((1, 0, 0, 0), 1), ((3, 0, 0, 0), 2)):
        st = OptState(tensors, offs, shadow)
        L.check(lib.tv_opt_cast_shadows(_p(st.table), _p(st.chunks), st.n, _stream()), "tv_opt_cast_shadows")
        torch.cuda.synchronize()
        res, sh = st.results()
        for (p, *_), s in zip(tensors, sh):
            assert np.array_equal(s, bf16_bits(p)), (offs, shadow, p.size)
    report("[K] tv_opt_cast_shadows", "bit-equal to .to(bfloat16) at every size")


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_fused_adamw_wrapper_against_fp64(t):
    """[O] through FusedAdamW: two parameter groups (lr / weight_decay / eps), the step counter set through load_state_dict, a
    second step on which one parameter has no gradient (a new chunk table) and one gradient has other strides than its
    parameter (the re-lay path); each step against fp64 from the device state before it, the same per-element bounds"""
    from transvae.optim import FusedAdamW
    rng = np.random.default_rng(t)
    shapes = [(65537,), (64, 33), (7,), (300, 17), (2, 3, 5, 5)]
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(F32)).to(dev())) for s in shapes]
    groups = [dict(params=ps[:2], lr=3e-3, weight_decay=0.05, eps=1e-8), dict(params=ps[2:], lr=1e-3, weight_decay=0.0, eps=1e-6)]
    opt = FusedAdamW(groups, betas=(0.9, 0.95))
    hps = [opt_hyper(lr=3e-3, beta2=0.95, wd=0.05, eps=1e-8)] * 2 + [opt_hyper(lr=1e-3, beta2=0.95, wd=0.0, eps=1e-6)] * 3

    def set_grads(skip=(), strided=()):
        gs = []
        for i, p in enumerate(ps):
            if i in skip:
                p.grad = None
                gs.append(None)
                continue
            g = torch.from_numpy((rng.standard_normal(p.shape) * 2.0 ** (i - 3)).astype(F32)).to(dev())
            if i in strided:
                g = g.t().contiguous().t()
                assert g.stride() != p.stride()
            p.grad = g
            gs.append(g.cpu().numpy())
        return gs

    # state at step t - 1 through load_state_dict
    set_grads()
    opt.fused_clip_step(1.0)
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(float(t - 1))
    opt.load_state_dict(sd)
    worst = np.zeros(3)
    for step, (skip, strided) in enumerate((((), ()), ((2,), (1, 3)))):
        gs = set_grads(skip, strided)
        before = [(p.detach().cpu().numpy().copy(), opt.state[p]["exp_avg"].cpu().numpy().copy(), opt.state[p]["exp_avg_sq"].cpu().numpy().copy())
                  for p in ps]
        norm, skipped = opt.fused_clip_step(1.0)
        torch.cuda.synchronize()
        tt = t + step
        assert float(skipped) == 0 and float(opt._ctrl[0]) == tt
        n64 = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in gs if g is not None))
        check_norm(float(norm), n64, "wrapper norm")
        coef, active = opt_coef64(n64, 1.0)
        for i, p in enumerate(ps):
            got = (opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy(), p.detach().cpu().numpy())
            if gs[i] is None:
                assert all(np.array_equal(got[k], before[i][(1, 2, 0)[k]]) for k in range(3))
                continue
            ref = adamw_ref64(before[i][0].ravel(), gs[i].ravel(), before[i][1].ravel(), before[i][2].ravel(), coef, active, hps[i], tt)
            worst = np.maximum(worst, check_adamw([a.ravel() for a in got], ref, f"step {tt} param {i}"))
            if p.dim() >= 2:
                assert torch.equal(opt._shadow[id(p)].view(torch.int16), p.detach().to(torch.bfloat16).view(torch.int16))
    report(f"[O] FusedAdamW t={t} ratio (m', v', p')", tuple(worst.round(3)))


# ---------------------------------------------------------------------------------------------------------------------------
# [K] tv_pack_weight_multi
# ---------------------------------------------------------------------------------------------------------------------------
def test_pack_weight_multi_is_a_bit_exact_permute():
    """[K] ten forms in one launch (O, I in {1, 63, 64, 65, 130}, T in {1, 9, 16}, both flips, tile_start the exclusive prefix sum):
    every destination bit-equal to permute (+ tap flip), nothing written outside [I][T][O]"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(0)
    srcs, dsts, rows, total = [], [], [], 0
    for O, T, I, flip in PACK_FORMS:
        s = torch.randn(O, T, I, generator=g).to(torch.bfloat16).to(dev())
        d = Guarded(I * T * O, off=1, dtype=torch.bfloat16)
        srcs.append(s)
        dsts.append(d)
        rows.append((s.data_ptr(), d.view.data_ptr(), O | (T << 32), I | (flip << 32), total))
        total += pack_tiles(O, T, I)
    tab = torch.tensor(rows, dtype=torch.int64, device=dev())
    L.check(lib.tv_pack_weight_multi(_p(tab), len(rows), total, _stream()), "tv_pack_weight_multi")
    torch.cuda.synchronize()
    for (O, T, I, flip), s, d in zip(PACK_FORMS, srcs, dsts):
        assert d.intact(), (O, T, I, flip)
        assert torch.equal(d.view.view(I, T, O).view(torch.int16), pack_ref(s, flip).view(torch.int16)), (O, T, I, flip)
    report("[K] tv_pack_weight_multi", f"{len(rows)} forms, {total} tiles, bit-equal")


# ---------------------------------------------------------------------------------------------------------------------------
# [L] tv_vae_loss_l1_kl
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_run(x, n_img, n_lat, sigmoid, clip, have=(True, True, True)):
    L, lib = _lib()
    ins = [torch.from_numpy(a).to(dev()) for a in x]
    outs = [Guarded(n, off=1) if h else None for n, h in zip((n_img, n_lat, n_lat), have)]
    part = Guarded(int(lib.tv_vae_loss_partial_count(n_img, n_lat)))
    out = Guarded(3)
    lo, hi = clip if clip is not None else (0.0, 0.0)
    L.check(lib.tv_vae_loss_l1_kl(*[_p(t) for t in ins], *[_p(o.view) if o else None for o in outs], _p(part.view), _p(out.view), n_img, n_lat,
                                  LOSS_W["l1_weight"], LOSS_W["kl_weight"], LOSS_W["kl_denom"], int(sigmoid), lo, hi, _stream()),
            "tv_vae_loss_l1_kl")
    torch.cuda.synchronize()
    assert part.intact() and out.intact() and all(o.intact() for o in outs if o)
    return (out.np(),) + tuple(o.np() if o else None for o in outs)


@pytest.mark.parametrize("sigmoid,clip", [(0, None), (1, None), (0, LOSS_CLIP), (1, LOSS_CLIP)])
def test_vae_loss_against_fp64(sigmoid, clip):
    """[L] every n_img x n_lat of the table (one element, one ragged block, an exact block, one element more, several blocks):
    values 1e-6 relative, gradients per element; saturation logits and the clamp's edges where the size admits them; each
    gradient pointer absent in turn; two runs bit-identical"""
    worst = {}
    for n_img in LOSS_N_IMG:
        for n_lat in LOSS_N_LAT:
            edges = n_img >= 32 and n_lat >= 16
            l1s, kls = loss_scales(n_img, **LOSS_W)
            x = loss_inputs(n_img, n_lat, seed=n_img + n_lat, edges=edges, clip=clip)
            ref = loss_ref64(*x, l1s, kls, sigmoid, clip)
            got = _loss_run(x, n_img, n_lat, sigmoid, clip)
            for i, nm in enumerate(("l1", "kl", "total")):
                report(f"[L] sigmoid={sigmoid} clip={clip} {n_img}x{n_lat} {nm}", f"{float(got[0][i])!r} vs {ref['out'][i]!r}")
            if sigmoid:
                assert np.isfinite(got[1]).all()
            fig = check_loss(got, ref, sigmoid, l1s, x[0], x[1], f"{n_img}x{n_lat}")
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
            again = _loss_run(x, n_img, n_lat, sigmoid, clip)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again)), "not bit-reproducible"
            if (n_img, n_lat) == (4097, 100):
                for drop in range(3):
                    have = tuple(i != drop for i in range(3))
                    part = _loss_run(x, n_img, n_lat, sigmoid, clip, have)
                    assert all(b is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, part))
    report(f"[L] tv_vae_loss_l1_kl sigmoid={sigmoid} clip={clip} (value rel. errors, gradient ratios)", {k: float(f"{v:.3g}") for k, v in worst.items()})


@pytest.mark.parametrize("which", ["logvar", "mu", "recon", "target"])
def test_vae_loss_propagates_non_finite_inputs(which):
    """[L] one NaN with the clamp on reaches the value the non-finite guard reads, as the torch formulation's; +inf in logvar
    clamps to hi and stays finite"""
    n_img, n_lat = 4097, 100
    l1s, kls = loss_scales(n_img, **LOSS_W)
    x = loss_inputs(n_img, n_lat, seed=5)
    idx = {"logvar": 3, "mu": 2, "recon": 0, "target": 1}[which]
    x[idx][17] = np.nan
    ref = loss_ref64(*x, l1s, kls, 0, LOSS_CLIP)
    out, _, _, d_lv = _loss_run(x, n_img, n_lat, 0, LOSS_CLIP)
    report(f"[L] NaN in {which}", f"out = {out.tolist()} (fp64 torch: {ref['out'].tolist()})")
    assert [math.isnan(v) for v in ref["out"]] == [math.isnan(float(v)) for v in out]
    check_nonfinite(out, d_lv[17], which, f"NaN in {which}")
    if which == "logvar":
        x[3][17] = np.inf
        ref = loss_ref64(*x, l1s, kls, 0, LOSS_CLIP)
        got = _loss_run(x, n_img, n_lat, 0, LOSS_CLIP)
        check_loss(got, ref, 0, l1s, x[0], x[1], "+inf in logvar")
        assert got[3][17] == 0


def test_vae_loss_through_the_module():
    """[L] TransVAELoss (sigmoid, clamp, the reference's KL denominator batch x H x W) and its autograd against the same fp64"""
    from transvae.losses.vae_loss import TransVAELoss
    B, H = 2, 8
    n_img, n_lat = B * 3 * 32 * 32, B * 4 * H * H
    x = loss_inputs(n_img, n_lat, seed=9, edges=True, clip=LOSS_CLIP)
    l1s, kls = loss_scales(n_img, 1.0, 1e-3, float(B * H * H))
    recon = torch.from_numpy(x[0]).view(B, 3, 32, 32).to(dev()).requires_grad_(True)
    mu = torch.from_numpy(x[2]).view(B, 4, H, H).to(dev()).requires_grad_(True)
    lv = torch.from_numpy(x[3]).view(B, 4, H, H).to(dev()).requires_grad_(True)
    crit = TransVAELoss(l1_weight=1.0, lpips_weight=0.0, kl_weight=1e-3, sigmoid_recon=True, logvar_clip=LOSS_CLIP)
    out = crit(recon, torch.from_numpy(x[1]).view(B, 3, 32, 32).to(dev()), mu, lv)
    out["total"].backward()
    torch.cuda.synchronize()
    ref = loss_ref64(*x, l1s, kls, 1, LOSS_CLIP)
    got = (np.array([float(out["l1"]), float(out["kl"]), float(out["total"])], F32), recon.grad.cpu().numpy().ravel(),
           mu.grad.cpu().numpy().ravel(), lv.grad.cpu().numpy().ravel())
    fig = check_loss(got, ref, 1, l1s, x[0], x[1], "TransVAELoss")
    report("[L] TransVAELoss", {k: float(f"{v:.3g}") for k, v in fig.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# [Z] tv_fold_cols / tv_fold_cols_bwd
# ---------------------------------------------------------------------------------------------------------------------------
def _fold_run(W, gamma, beta, dWf, dbf):
    L, lib = _lib()
    R, Cc = W.shape
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev()).contiguous()
    Wd, gd, bd, dWfd, dbfd = up(W), up(gamma), up(beta), up(dWf), up(dbf)
    has_b = beta is not None
    Wf, dW = Guarded(R * Cc), Guarded(R * Cc)
    bf = Guarded(R) if has_b else None
    dg = Guarded(Cc)
    db = Guarded(Cc) if has_b else None
    part = Guarded(int(lib.tv_fold_partial_count(R, Cc)))
    L.check(lib.tv_fold_cols(_p(Wd), _p(gd), _p(bd), _p(Wf.view), _p(bf.view) if has_b else None, R, Cc, _stream()), "tv_fold_cols")
    L.check(lib.tv_fold_cols_bwd(_p(dWfd), _p(dbfd) if has_b else None, _p(Wd), _p(gd), _p(bd), _p(dW.view), _p(dg.view),
                                 _p(db.view) if has_b else None, _p(part.view), R, Cc, _stream()), "tv_fold_cols_bwd")
    torch.cuda.synchronize()
    assert all(g.intact() for g in (Wf, dW, bf, dg, db, part) if g is not None), f"{R}x{Cc}: a write outside an output"
    return dict(Wf=Wf.np().reshape(R, Cc), dW=dW.np().reshape(R, Cc), bf=bf.np() if has_b else None, dgamma=dg.np(),
                dbeta=db.np() if has_b else None)


@pytest.mark.parametrize("R", FOLD_R)
def test_fold_against_fp64(R):
    """[Z] R x every C (float4 and scalar branches, one and several column blocks, a ragged last one), with and without beta: Wf the
    IEEE product, bf / dW / dgamma / dbeta inside their bounds with cancelling columns and a dominating dbf, partials sized by
    tv_fold_partial_count with a guard behind them, two runs bit-identical"""
    worst = {}
    for Cc in FOLD_C:
        W, gamma, beta, dWf, dbf = fold_inputs(R, Cc, seed=R * 1000 + Cc)
        for has_b in (True, False):
            b, db = (beta, dbf) if has_b else (None, None)
            ref = fold_ref64(W, gamma, b, dWf, db)
            got = _fold_run(W, gamma, b, dWf, db)
            fig = check_fold(got, ref, R, f"{R}x{Cc} beta={has_b}")
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
            again = _fold_run(W, gamma, b, dWf, db)
            assert all(got[k] is None or np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got), "not bit-reproducible"
    report(f"[Z] fold R={R} worst ratios", {k: round(v, 3) for k, v in worst.items()})


def test_fold_through_fused_fold():
    """[Z] fused.fold (three stacked triples, as the QKV fold) and its autograd inside the same bounds"""
    from transvae.hip import fused
    R, Cc, n = 65, 72, 3
    data = [fold_inputs(R, Cc, seed=50 + s) for s in range(n)]
    mk = lambda a: torch.from_numpy(a).to(dev()).requires_grad_(True)
    Ws, gs, bs = [mk(d[0]) for d in data], [mk(d[1]) for d in data], [mk(d[2]) for d in data]
    Wf, bf = fused.fold(Ws, gs, bs)
    dWf = torch.from_numpy(np.concatenate([d[3] for d in data])).to(dev())
    dbf = torch.from_numpy(np.concatenate([d[4] for d in data])).to(dev())
    torch.autograd.backward([Wf, bf], [dWf, dbf])
    torch.cuda.synchronize()
    worst = {}
    for s, d in enumerate(data):
        ref = fold_ref64(*d)
        got = dict(Wf=Wf[s * R:(s + 1) * R].detach().cpu().numpy(), bf=bf[s * R:(s + 1) * R].detach().cpu().numpy(), dW=Ws[s].grad.cpu().numpy(),
                   dgamma=gs[s].grad.cpu().numpy(), dbeta=bs[s].grad.cpu().numpy())
        for k, v in check_fold(got, ref, R, f"fused.fold triple {s}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    report("[Z] fused.fold worst ratios", {k: round(v, 3) for k, v in worst.items()})
