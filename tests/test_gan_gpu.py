"""The adversarial stage on the GPU: every new kernel against fp64 of the same bf16 inputs under its DESIGN.md §3.1 row (bounds
and references from tests/test_gan_host.py), the 4x4 convolutions under rows G / D / W, bit-reproducibility, the whole
discriminator against the plain-torch restatement (tests/gan_restatement.py) within max(floor, 1.25 x the restatement's own
bf16-autocast deviation), the GAN terms of the loss, a stage-2 loop, and the frozen-encoder train step."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gan_restatement as GR
import test_gan_host as H
from oracle import filler
from oracle import transvae_oracle as O
from test_error_budget_host import F64, check_fp32, check_one_rounding, conv64, epilogue64, rel_l2, wgrad64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _lib():
    from transvae.hip import _lib as L
    return L, L.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def micro_model(**kw):
    from transvae import TransVAE
    m = TransVAE(config=dict(O.MICRO), variant="micro", compression_ratio=16, latent_dim=4, **kw)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(O.MICRO, latent_dim=4)))
    return m.to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# [L] LeakyReLU epilogue and its gradient mask
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(1234, 64, 72), (4096, 64, 64)])
def test_lrelu_epilogue_and_mask(M, K, N):
    from transvae.hip import ops
    L, lib = _lib()
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(BF).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    y = torch.empty(M, N, dtype=BF, device=DEV)
    d = ops._rows_desc(M, K, N)
    d.act = L.ACTX_LRELU
    ops.igemm(d, x, w, b, None, None, y)
    acc, absdot = conv64(x.cpu(), w.cpu(), "linear")
    y64, slack = H.lrelu_epilogue64(acc, absdot, b.cpu())
    r = check_one_rounding(y.cpu(), y64, slack, "lrelu epilogue")
    print("lrelu epilogue ratio/ulps/bias", r)
    # data gradient through the layer: dx = (gz wt^T) masked by y
    gz = torch.randn(M, 96, generator=g).to(BF).to(DEV)
    wt = (torch.randn(N, 96, generator=g) / 10).to(BF).to(DEV)
    dx = ops.gemm_rows(gz, wt, N, aux=y, aux_act=L.ACTX_LRELU)
    acc2, abs2 = conv64(gz.cpu(), wt.cpu(), "linear")
    pos = y.cpu().to(F64) > 0
    d64 = torch.where(pos, acc2, H.SLOPE * acc2)
    check_one_rounding(dx.cpu(), d64, 2.0 ** -20 * abs2 + 2.0 ** -24 * acc2.abs(), "lrelu data gradient")
    # tv_act_bwd: kept elements bit-exact
    gy = torch.randn(M, N, generator=g).to(BF).to(DEV)
    dz = ops.act_backward(y, gy, L.ACTX_LRELU)
    dz64, ms = H.lrelu_mask64(y.cpu(), gy.cpu())
    check_one_rounding(dz.cpu(), dz64, ms, "lrelu mask", min_bias_n=10 ** 9)
    assert torch.equal(dz[y.float() > 0], gy[y.float() > 0])


# ---------------------------------------------------------------------------------------------------------------------------
# [Q] patch gather and adjoint
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
def test_patch4x4s2_and_adjoint(sigmoid, channels_last):
    L, lib = _lib()
    g = torch.Generator().manual_seed(5)
    B, Hh, W = 2, 40, 24
    img = (torch.randn(B, 3, Hh, W, generator=g) * 1.5).to(DEV)
    if channels_last:
        img = img.contiguous(memory_format=torch.channels_last)
    rows = torch.empty(B, Hh // 2, W // 2, 64, dtype=BF, device=DEV)
    L.check(lib.tv_patch4x4s2(_p(img), *img.stride(), _p(rows), B, Hh, W, int(sigmoid), _st()))
    r64 = H.patch_rows64(img.cpu(), sigmoid)
    check_one_rounding(rows.cpu(), r64, 2.0 ** -20 if sigmoid else 0.0, "patch rows", min_bias_n=10 ** 9)
    assert float(rows[..., 48:].float().abs().max()) == 0.0
    drows = torch.randn(B, Hh // 2, W // 2, 64, generator=g).to(BF).to(DEV)
    dimg = torch.empty(B, 3, Hh, W, dtype=torch.float32, device=DEV)
    L.check(lib.tv_patch4x4s2_bwd(_p(drows), _p(img), *img.stride(), _p(dimg), B, Hh, W, int(sigmoid), _st()))
    d64, dabs = H.patch_rows_adjoint64(drows.cpu(), img.cpu(), sigmoid)
    print("patch adjoint ratio", check_fp32(dimg.cpu(), d64, dabs, 16 if sigmoid else 4, "patch adjoint"))


# ---------------------------------------------------------------------------------------------------------------------------
# [B] BatchNorm + LeakyReLU
# ---------------------------------------------------------------------------------------------------------------------------
def _bn_run(x, dy, gamma, beta, rm, rv, eval_mode=False, eps=1e-5):
    L, lib = _lib()
    M, Cc = x.shape
    part = torch.empty(lib.tv_bn_partial_count(M, Cc), dtype=torch.float32, device=DEV)
    mr = torch.empty(2, Cc, dtype=torch.float32, device=DEV)
    ss = torch.empty(2, Cc, dtype=torch.float32, device=DEV)
    if eval_mode:
        rstd = torch.rsqrt(rv + eps)
        mr[0], mr[1] = rm, rstd
        ss[0] = gamma * rstd
        ss[1] = beta - rm * ss[0]
    else:
        L.check(lib.tv_bn_stats(_p(x), _p(gamma), _p(beta), _p(part), _p(mr), _p(ss), _p(rm), _p(rv), M, Cc, C.c_float(eps), C.c_float(0.1), _st()))
    y = torch.empty_like(x)
    L.check(lib.tv_bn_lrelu_apply(_p(x), _p(ss), _p(y), M, Cc, _st()))
    red = torch.empty(2, Cc, dtype=torch.float32, device=DEV)
    dg = torch.empty(Cc, dtype=torch.float32, device=DEV)
    db = torch.empty(Cc, dtype=torch.float32, device=DEV)
    L.check(lib.tv_bn_lrelu_bwd_reduce(_p(x), _p(dy), _p(mr), _p(ss), _p(part), _p(red), _p(dg), _p(db), M, Cc, 0, _st()))
    dx = torch.empty_like(x)
    L.check(lib.tv_bn_lrelu_bwd_apply(_p(x), _p(dy), _p(mr), _p(ss), _p(red), _p(dx), M, Cc, int(eval_mode), _st()))
    return mr, ss, y, red, dg, db, dx


@pytest.mark.parametrize("M,Cc", [(2 * 31 * 31, 128), (2 * 31 * 31, 512), (70000, 256)])
def test_batchnorm_lrelu_family(M, Cc):
    x, dy, gamma, beta = (t.to(DEV) for t in H.bn_inputs(M, Cc, seed=Cc))
    rm = torch.zeros(Cc, device=DEV)
    rv = torch.ones(Cc, device=DEV)
    mr, ss, y, red, dg, db, dx = _bn_run(x, dy, gamma, beta, rm, rv)
    xc = x.cpu()
    print("bn stats ratios (mean, rstd)", H.check_bn_stats(xc, mr[0].cpu(), mr[1].cpu(), "tv_bn_stats"))
    mean64, var64, rstd64, unb64 = H.bn_stats64(xc)
    sc64 = gamma.cpu().to(F64) * rstd64
    assert float(((ss[0].cpu().to(F64) / sc64 - 1).abs() / (H.bn_stats_bounds(xc, mean64, var64)[1] + 2.0 ** -23)).max()) <= 1.0
    y64, slack = H.bn_apply64(xc, ss.cpu())
    check_one_rounding(y.cpu(), y64, slack, "tv_bn_lrelu_apply")
    ref = H.bn_bwd64(xc, dy.cpu(), mr.cpu(), ss.cpu())
    print("dbeta ratio", check_fp32(db.cpu(), ref["dbeta"], ref["abs_dbeta"], H.BN_CHAIN + 4, "dbeta"))
    print("dgamma ratio", check_fp32(dg.cpu(), ref["dgamma"], ref["abs_dgamma"], H.BN_CHAIN + 4, "dgamma"))
    assert torch.equal(red[0], db) and torch.equal(red[1], dg)
    ref2 = H.bn_bwd64(xc, dy.cpu(), mr.cpu(), ss.cpu())
    # dx from the kernel's own fp32 reductions (the inputs of that launch)
    M_ = xc.shape[0]
    h = xc.to(F64) * ss[0].cpu().to(F64) + ss[1].cpu().to(F64)
    dh = torch.where(h > 0, dy.cpu().to(F64), H.SLOPE * dy.cpu().to(F64))
    xh = (xc.to(F64) - mr[0].cpu().to(F64)) * mr[1].cpu().to(F64)
    dx64 = ss[0].cpu().to(F64) * (dh - (red[0].cpu().to(F64) + xh * red[1].cpu().to(F64)) / M_)
    check_one_rounding(dx.cpu(), dx64, ref2["dx_slack"], "tv_bn_lrelu_bwd_apply")
    # running statistics after two calls (momentum 0.1, unbiased variance)
    _bn_run(x, dy, gamma, beta, rm, rv)
    rm64 = 0.9 * (0.1 * mean64) + 0.1 * mean64
    rv64 = 0.9 * (0.9 + 0.1 * unb64) + 0.1 * unb64
    bm, br = H.bn_stats_bounds(xc, mean64, var64)
    assert float(((rm.cpu().to(F64) - rm64).abs() / (bm + 2.0 ** -22 * rm64.abs())).max()) <= 1.0
    assert float(((rv.cpu().to(F64) / rv64 - 1).abs() / (2 * br + 2.0 ** -22)).max()) <= 1.0
    # eval mode: running statistics, plain affine backward
    mr_e, ss_e, y_e, red_e, dg_e, db_e, dx_e = _bn_run(x, dy, gamma, beta, rm, rv, eval_mode=True)
    y64e, slack_e = H.bn_apply64(xc, ss_e.cpu())
    check_one_rounding(y_e.cpu(), y64e, slack_e, "eval apply")
    ref_e = H.bn_bwd64(xc, dy.cpu(), mr_e.cpu(), ss_e.cpu(), eval_mode=True)
    check_one_rounding(dx_e.cpu(), ref_e["dx"], ref_e["dx_slack"], "eval dx")
    check_fp32(dg_e.cpu(), ref_e["dgamma"], ref_e["abs_dgamma"], H.BN_CHAIN + 4, "eval dgamma")
    check_fp32(db_e.cpu(), ref_e["dbeta"], ref_e["abs_dbeta"], H.BN_CHAIN + 4, "eval dbeta")


def test_bn_statistics_and_gan_loss_are_bit_reproducible():
    from transvae import DiscriminatorLoss
    x, dy, gamma, beta = (t.to(DEV) for t in H.bn_inputs(70001, 128, seed=9))
    runs = []
    for _ in range(2):
        rm, rv = torch.zeros(128, device=DEV), torch.ones(128, device=DEV)
        mr, ss, y, red, dg, db, dx = _bn_run(x, dy, gamma, beta, rm, rv)
        runs.append([t.clone() for t in (mr, ss, red, rm, rv)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    g = torch.Generator().manual_seed(1)
    a, b = (torch.randn(128, 1, 30, 30, generator=g) * 3).to(DEV), (torch.randn(128, 1, 30, 30, generator=g) * 3).to(DEV)
    for t in ("bce", "hinge", "wgan"):
        v = [DiscriminatorLoss(t)(a, b) for _ in range(2)]
        assert torch.equal(v[0], v[1])


# ---------------------------------------------------------------------------------------------------------------------------
# [X] GAN loss
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gen", "bce", "hinge", "wgan"])
def test_gan_loss_value_and_gradients(mode):
    from transvae import DiscriminatorLoss
    from transvae.losses import generator_gan_loss
    g = torch.Generator().manual_seed(11)
    a = torch.randn(3, 1, 30, 30, generator=g) * 2.5
    b = torch.randn(2, 1, 31, 29, generator=g) * 2.5            # a different count, not a multiple of 4
    a.view(-1)[:6] = torch.tensor([40.0, -40.0, 0.0, 1.0, -1.0, 88.0])
    b.view(-1)[:4] = torch.tensor([40.0, -40.0, 0.0, -1.0])
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = H.gan_loss64(a64, b64 if mode != "gen" else None, mode, 0.05 if mode == "gen" else 1.0)
    ref.backward()
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    got = generator_gan_loss(ad, 0.05) if mode == "gen" else DiscriminatorLoss(mode)(ad, bd)
    got.backward()
    print(mode, "value", float(got), "ref", float(ref))
    assert math.isfinite(float(got)) and abs(float(got) - float(ref)) <= 1e-6 * abs(float(ref))
    assert torch.isfinite(ad.grad).all()
    assert rel_l2(ad.grad.cpu(), a64.grad) <= 1e-5
    if mode != "gen":
        assert torch.isfinite(bd.grad).all() and rel_l2(bd.grad.cpu(), b64.grad) <= 1e-5
    if mode in ("gen", "bce"):     # saturation at +-40: d bce(x, 1) = sigmoid(x) - 1
        n = a.numel()
        scale = (0.05 if mode == "gen" else 0.5) / n
        assert float(ad.grad.view(-1)[0]) == 0.0 and abs(float(ad.grad.view(-1)[1]) + scale) <= 1e-6 * scale
    # restated torch forms agree as well
    if mode != "gen":
        assert abs(float(got) - float(GR.discriminator_loss(a.double(), b.double(), mode))) <= 1e-6 * abs(float(ref))


# ---------------------------------------------------------------------------------------------------------------------------
# 4x4 convolutions under rows G / D / W
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,Hh,W,Cin,Cout,form", [("c4s2", 62, 62, 64, 128, "polyphase"), ("c4s2", 62, 62, 64, 128, "dilated"),
                                                     ("c4s2", 16, 24, 128, 256, "polyphase"), ("c4s1", 31, 31, 256, 64, None),
                                                     ("c4s1", 8, 12, 64, 32, None)])
def test_conv4x4_forward_dgrad_wgrad(mode, Hh, W, Cin, Cout, form):
    from transvae.hip import ops
    g = torch.Generator().manual_seed(Hh * W + Cin)
    B = 2
    x = torch.randn(B, Hh, W, Cin, generator=g).to(BF).to(DEV)
    w = (torch.randn(Cout, 4, 4, Cin, generator=g) / math.sqrt(16 * Cin)).to(BF).float().to(DEV)
    bias = (torch.randn(Cout, generator=g) * 0.1).to(DEV)
    old = ops.C4S2_DGRAD_FORM
    if form:
        ops.C4S2_DGRAD_FORM = form
    try:
        out, _, geo, wc = ops.conv_forward(x, w, bias, None, mode, 0, False)
        stride = 2 if mode == "c4s2" else 1
        xn, wn = x.cpu().to(F64).permute(0, 3, 1, 2), w.cpu().to(F64).permute(0, 3, 1, 2)
        acc = F.conv2d(xn, wn, stride=stride, padding=1).permute(0, 2, 3, 1)
        absdot = F.conv2d(xn.abs(), wn.abs(), stride=stride, padding=1).permute(0, 2, 3, 1)
        assert tuple(out.shape) == tuple(acc.shape)
        y64, slack, _ = epilogue64(acc, absdot, bias.cpu())
        check_one_rounding(out.cpu(), y64, slack, f"{mode} forward [G]")
        gz = torch.randn(out.shape, generator=g).to(BF).to(DEV)
        dx = ops.conv_dgrad(geo, wc, gz, x.shape)
        gzn = gz.cpu().to(F64).permute(0, 3, 1, 2)
        d64 = F.conv_transpose2d(gzn, wn, stride=stride, padding=1).permute(0, 2, 3, 1)
        dabs = F.conv_transpose2d(gzn.abs(), wn.abs(), stride=stride, padding=1).permute(0, 2, 3, 1)
        assert tuple(d64.shape) == tuple(x.shape)
        check_one_rounding(dx.cpu(), d64, 2.0 ** -20 * dabs, f"{mode} data gradient [D]")
        dw, dbias = ops.conv_wgrad(geo, wc, x, gz, True)
        xr = xn.detach().clone().requires_grad_(True)
        wr = wn.detach().clone().requires_grad_(True)
        (F.conv2d(xr, wr, stride=stride, padding=1) * gzn).sum().backward()
        wa = wn.detach().abs().clone().requires_grad_(True)
        (F.conv2d(xn.abs(), wa, stride=stride, padding=1) * gzn.abs()).sum().backward()
        check_fp32(dw.cpu(), wr.grad.permute(0, 2, 3, 1), wa.grad.permute(0, 2, 3, 1), 16, f"{mode} weight gradient [W]")
        check_fp32(dbias.cpu(), gzn.sum((0, 2, 3)), gzn.abs().sum((0, 2, 3)), 16, f"{mode} bias gradient [W]")
    finally:
        ops.C4S2_DGRAD_FORM = old


# ---------------------------------------------------------------------------------------------------------------------------
# the whole discriminator against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
WHOLE = {}


@pytest.mark.parametrize("mode", GR.MODES)
@pytest.mark.parametrize("shape", GR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_discriminator_against_restatement(shape, mode):
    from transvae import PatchDiscriminator
    from transvae.losses import generator_gan_loss
    with open(GR.GOLDEN) as f:
        gold = json.load(f)["cases"][GR.case_key(shape, mode)]
    ref = GR.seeded_patchgan()
    x = GR.case_input(shape)
    l32, g32, p32 = GR.run_case(ref, x, mode)
    d = PatchDiscriminator()
    d.load_state_dict(GR.seeded_patchgan().state_dict())
    d = d.to(DEV)
    d.train() if mode == "train" else d.eval()
    xd = x.to(DEV).requires_grad_(True)
    logits = d(xd)
    assert tuple(logits.shape) == tuple(l32.shape) and logits.dtype == torch.float32
    generator_gan_loss(logits, 1.0).backward()
    rep = {"logits": (rel_l2(logits.detach().cpu(), l32), max(1e-2, 1.25 * gold["logits"])),
           "input_grad": (rel_l2(xd.grad.cpu(), g32), max(3e-2, 1.25 * gold["input_grad"]))}
    for k, p in d.named_parameters():
        rep[k] = (rel_l2(p.grad.cpu(), p32[k]), max(3e-2, 1.25 * gold["param_grads"][k]))
    print(GR.case_key(shape, mode), {k: (round(e, 5), round(e / b, 3)) for k, (e, b) in rep.items()})
    for k, (e, b) in rep.items():
        assert e < b, (k, e, b)
    if mode == "train":     # the running statistics moved exactly as torch's
        for i in (3, 6, 9):
            assert rel_l2(d.main[i].running_mean.cpu(), ref.main[i].running_mean) < 1e-2
            assert rel_l2(d.main[i].running_var.cpu(), ref.main[i].running_var) < 1e-2
            assert int(d.main[i].num_batches_tracked) == int(ref.main[i].num_batches_tracked)
    # channels_last input: the same bits
    with torch.no_grad():
        d.eval()
        a = d(x.to(DEV))
        b = d(x.to(DEV).contiguous(memory_format=torch.channels_last))
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# the loss terms
# ---------------------------------------------------------------------------------------------------------------------------
class _TinyD(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.net = nn.Sequential(nn.Conv2d(3, 8, 4, 2, 1), nn.LeakyReLU(0.2), nn.Conv2d(8, 1, 4, 2, 1))

    def forward(self, x):
        return self.net(x)


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("which", ["patch", "torch"])
def test_transvae_loss_gan_term(which, sigmoid):
    from transvae import PatchDiscriminator, TransVAELoss
    m = micro_model()
    D = (PatchDiscriminator(ndf=32) if which == "patch" else _TinyD()).to(DEV)
    x = filler.rand_input("micro.x", (2, 3, 64, 64)).to(DEV)
    eps = filler.randn_input("micro.eps", (2, 4, 4, 4)).to(DEV)
    recon, mu, logvar = m(x, eps=eps)
    recon.retain_grad()
    loss_fn = TransVAELoss(lpips_weight=0.0, use_gan=True, gan_weight=0.05, sigmoid_recon=sigmoid)
    out = loss_fn(recon, x, mu, logvar, discriminator=D)
    assert list(out) == ["l1", "kl", "gan", "total"]
    # the same logits through the restated term (BatchNorm in train mode: the statistics of this very batch)
    with torch.no_grad():
        if which == "patch":
            logits = D(recon.detach(), sigmoid_input=sigmoid)
        else:
            logits = D(torch.sigmoid(recon.detach()) if sigmoid else recon.detach())
    ref = float(GR.generator_term(logits.double().cpu(), 0.05))
    assert abs(float(out["gan"]) - ref) <= 1e-6 * abs(ref), (float(out["gan"]), ref)
    assert float(out["total"]) == float(out["l1"] + out["kl"] + out["gan"])
    base = TransVAELoss(lpips_weight=0.0, sigmoid_recon=sigmoid)(recon, x, mu, logvar)
    out["gan"].backward(retain_graph=True)
    assert recon.grad is not None and float(recon.grad.abs().max()) > 0
    # use_gan=False with a discriminator passed: exactly today's dict and values
    off = TransVAELoss(lpips_weight=0.0, use_gan=False, sigmoid_recon=sigmoid)(recon, x, mu, logvar, discriminator=D)
    assert list(off) == ["l1", "kl", "total"] and all(torch.equal(off[k], base[k]) for k in base)
    none = TransVAELoss(lpips_weight=0.0, use_gan=True, sigmoid_recon=sigmoid)(recon, x, mu, logvar, discriminator=None)
    assert list(none) == ["l1", "kl", "total"] and all(torch.equal(none[k], base[k]) for k in base)
    with pytest.raises(ValueError, match="VF"):
        loss_fn(recon, x, mu, logvar, discriminator=D, dinov2=nn.Identity())


def test_stage2_loop_on_the_micro_model():
    """Alternating generator / discriminator updates with two FusedAdamW instances, the reference's stage 2 in miniature."""
    from transvae import DiscriminatorLoss, PatchDiscriminator, TransVAELoss
    from transvae.optim import FusedAdamW
    from transvae.parallel import clip_and_step
    torch.manual_seed(0)
    m = micro_model(clamp_latent=True)
    D = PatchDiscriminator(ndf=32).to(DEV)
    with torch.no_grad():      # a livelier start than N(0, 0.02) for a six-step test
        for mod in D.main:
            if isinstance(mod, nn.Conv2d):
                mod.weight.mul_(3.0)
    opt_g = FusedAdamW(m.parameters(), lr=1e-4, betas=(0.5, 0.9), weight_decay=0.0)
    opt_d = FusedAdamW(D.parameters(), lr=2e-3, betas=(0.5, 0.9), weight_decay=0.0)
    loss_fn, d_loss = TransVAELoss(lpips_weight=0.0, use_gan=True, gan_weight=0.05), DiscriminatorLoss("bce")
    g = torch.Generator().manual_seed(3)
    x = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    rm0 = D.main[3].running_mean.clone()

    def fixed_d_loss():
        with torch.no_grad():
            fake = m(x, eps=torch.zeros(4, 4, 4, 4, device=DEV))[0]
            return float(d_loss(D(x), D(fake)))
    first = fixed_d_loss()
    hist = []
    for step in range(6):
        opt_g.zero_grad(set_to_none=True)
        recon, mu, logvar = m(x)
        out = loss_fn(recon, x, mu, logvar, discriminator=D)
        out["total"].backward()
        clip_and_step(list(m.parameters()), opt_g, 1.0)
        opt_d.zero_grad(set_to_none=True)       # (the generator step left gradients on D's parameters, as in any GAN loop)
        ld = d_loss(D(x), D(recon.detach()))
        ld.backward()
        clip_and_step(list(D.parameters()), opt_d, 1.0)
        hist.append((float(out["total"]), float(out["gan"]), float(ld)))
    last = fixed_d_loss()
    print("stage-2 loop (total, gan, d):", np.round(hist, 4), "fixed-batch d loss", first, "->", last)
    assert all(math.isfinite(v) for row in hist for v in row)
    assert last < first
    assert float((D.main[3].running_mean - rm0).abs().max()) > 0
    assert all(torch.isfinite(p).all() for p in list(m.parameters()) + list(D.parameters()))


# ---------------------------------------------------------------------------------------------------------------------------
# encoder frozen
# ---------------------------------------------------------------------------------------------------------------------------
def _freeze_encoder(m):
    m.encoder.requires_grad_(False)
    m.conv_mu.requires_grad_(False)
    m.conv_logvar.requires_grad_(False)


def test_frozen_encoder_train_step(golden_dir):
    from transvae.optim import FusedAdamW
    from transvae.parallel import clip_and_step, train_step, vae_bench_loss
    x = filler.rand_input("micro.x", (2, 3, 64, 64)).to(DEV)
    eps = filler.randn_input("micro.eps", (2, 4, 4, 4)).to(DEV)
    peaks = {}
    for frozen in (False, True):
        m = micro_model()
        m.train()
        if frozen:
            _freeze_encoder(m)
        recon, mu, logvar = m(x, eps=eps)           # warm-up: operand caches, workspaces
        O.bench_loss(recon, x, mu, logvar).backward()
        m.zero_grad(set_to_none=True)
        del recon, mu, logvar
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        recon, mu, logvar = m(x, eps=eps)
        O.bench_loss(recon, x, mu, logvar).backward()
        torch.cuda.synchronize()
        peaks[frozen] = torch.cuda.max_memory_allocated() - base
        if frozen:
            frozen_model = m
        del recon, mu, logvar
    print("peak step memory unfrozen / frozen: %.2f / %.2f MiB" % (peaks[False] / 2 ** 20, peaks[True] / 2 ** 20))
    assert peaks[True] < peaks[False], peaks
    m = frozen_model
    fz = [(k, p) for k, p in m.named_parameters() if k.startswith(("encoder.", "conv_mu.", "conv_logvar."))]
    assert fz and all(p.grad is None for _, p in fz)
    # decoder gradients against the oracle at the micro-model gradient test's own bound
    g = dict(np.load(os.path.join(golden_dir, "micro_model.npz")))
    with open(os.path.join(golden_dir, "micro_grads_ref_bf16_autocast.json")) as f:
        ref16 = json.load(f)
    params = dict(m.named_parameters())
    checked = 0
    for k in g:
        if k.startswith("g:decoder."):
            err = rel_l2(params[k[2:]].grad.cpu(), torch.from_numpy(g[k]))
            assert err < max(3e-2, 1.5 * ref16[k[2:]]["l2rel"]), (k, err)
            checked += 1
    assert checked > 0
    # an optimizer over the trainable parameters only: the frozen ones are bit-unchanged after a step
    before = {k: p.detach().clone() for k, p in fz}
    dec0 = m.decoder.conv_out.weight.detach().clone()
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0)
    clip_and_step([p for p in m.parameters() if p.requires_grad], opt, 1.0)
    assert all(torch.equal(before[k], p) for k, p in fz) and all(p.grad is None for _, p in fz)
    assert not torch.equal(dec0, m.decoder.conv_out.weight)

    # two micro-batches through train_step == one batch of both (the tolerance of the existing accumulation test)
    gen = torch.Generator().manual_seed(9)
    x4 = torch.rand(4, 3, 64, 64, generator=gen).to(DEV)
    eps4 = torch.randn(4, 4, 4, 4, generator=gen).to(DEV)
    res = {}
    for micro in (4, 2):
        mm = micro_model(clamp_latent=True)
        mm.train()
        _freeze_encoder(mm)
        opt = torch.optim.SGD([p for p in mm.parameters() if p.requires_grad], lr=0.0)
        cursor = [0]

        def forward_loss(model, xb):
            e = eps4[cursor[0]:cursor[0] + xb.shape[0]]
            cursor[0] += xb.shape[0]
            recon, mu, logvar = model(xb, eps=e)
            return vae_bench_loss(recon, xb, mu, logvar)
        out = []
        for _ in range(2):
            cursor[0] = 0
            loss = train_step(mm, opt, x4, micro, forward_loss, None, 4, {})
            assert all(p.grad is None for k, p in mm.named_parameters() if not p.requires_grad)
            out.append((float(loss), {k: p.grad.detach().double().cpu() for k, p in mm.named_parameters() if p.requires_grad}))
        res[micro] = out
    for step in range(2):
        assert abs(res[2][step][0] - res[4][step][0]) < 1e-6 * abs(res[4][step][0])
        for k, a in res[4][step][1].items():
            b = res[2][step][1][k]
            assert float((a - b).norm()) <= 2e-5 * float(a.norm()) + 1e-9, (step, k, float((a - b).norm()), float(a.norm()))
