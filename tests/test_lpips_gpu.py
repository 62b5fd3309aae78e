"""LPIPS (VGG-16) perceptual term on the MI355X: each kernel against fp64 of the same bf16 inputs under its rounding contract
(DESIGN.md section 3.1), the whole loss against the plain-torch fp32 restatement (tests/lpips_restatement.py) under the
project's bf16-tier rule, and the TransVAELoss / evaluate() integration.

Whole-loss figures measured on MI355X (rel-L2 against the fp32 restatement; value / gradient, worst image set per pair; the
bound is max(floor, 1.25 x the restatement's own bf16-autocast deviation), floors 1e-2 / 3e-2): see DESIGN.md section 3.
"""
import json

import pytest
import torch
import torch.nn.functional as F

import lpips_restatement as R
from test_error_budget_host import BF, F64, check_one_rounding, conv64, epilogue64, r16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bf(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(BF)


@pytest.fixture(scope="module")
def net():
    from transvae import PerceptualLoss
    return PerceptualLoss().load_lpips_state_dict(R.plain_state_dict()).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# ReLU epilogue and mask
# ---------------------------------------------------------------------------------------------------------------------
def test_relu_epilogue_rounds_once_and_mask_is_exact():
    from transvae.hip import ops
    from transvae.losses import lpips as LP
    g = torch.Generator().manual_seed(3)
    B, H, W, Cin, Cout = 2, 13, 19, 96, 72          # ragged: no tile divides it
    x = bf((B, H, W, Cin), g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.3
    wb = w.to(BF)
    y = LP.conv3x3_relu(x.to(DEV), wb.to(DEV), bias.to(DEV)).cpu()
    acc, absdot = conv64(x, wb, "c3s1")
    z = acc + bias.to(F64)
    y64 = torch.clamp(z, min=0)
    slack = 2.0 ** -20 * absdot + 2.0 ** -24 * bias.to(F64).abs()    # relu is 1-Lipschitz: the accumulation error of z
    ratio, ulps, mean = check_one_rounding(y, y64, slack, "relu epilogue")
    print(f"relu epilogue: {ratio:.3f} x (ulp + slack), {ulps:.3f} ulp, bias {mean:+.4f}")
    assert bool((y.float() >= 0).all())
    assert float((y == 0).float().mean()) > 0.2           # the mask below has something to mask

    # data gradient through the ReLU layer that produced `y`: conv_T(gz) where y > 0, exactly 0 elsewhere
    gz = bf((B, H, W, 64), g)
    w2 = torch.randn(64, 3, 3, Cout, generator=g) * 0.1            # the next layer: Cout -> 64
    wt = w2.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(BF)     # [Cout, 3, 3, 64]
    plain = LP.conv3x3_relu_dgrad(gz.to(DEV), wt.to(DEV), None).cpu()
    masked = LP.conv3x3_relu_dgrad(gz.to(DEV), wt.to(DEV), y.to(DEV)).cpu()
    assert torch.equal(masked, torch.where(y.float() > 0, plain, torch.zeros_like(plain)))
    acc2, absdot2 = conv64(gz, wt, "c3s1")
    check_one_rounding(plain, acc2, 2.0 ** -20 * absdot2, "relu-layer data gradient")
    # the standalone mask
    gy = bf(y.shape, g)
    assert torch.equal(LP.relu_backward(y.to(DEV), gy.to(DEV)).cpu(), torch.where(y.float() > 0, gy, torch.zeros_like(gy)))
    # a multiple-of-tile shape takes the register epilogue form; same contract
    x2 = bf((1, 32, 32, 64), g)
    w3 = (torch.randn(128, 3, 3, 64, generator=g) * (2.0 / (9 * 64)) ** 0.5).to(BF)
    y2 = LP.conv3x3_relu(x2.to(DEV), w3.to(DEV), None).cpu()
    acc3, absdot3 = conv64(x2, w3, "c3s1")
    check_one_rounding(y2, torch.clamp(acc3, min=0), 2.0 ** -20 * absdot3, "relu epilogue (register form)")
    y_prev = bf((1, 32, 32, 64), g)
    m2 = LP.conv3x3_relu_dgrad(y2.to(DEV), w3.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(DEV), y_prev.to(DEV)).cpu()
    p2 = LP.conv3x3_relu_dgrad(y2.to(DEV), w3.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(DEV), None).cpu()
    assert torch.equal(m2, torch.where(y_prev.float() > 0, p2, torch.zeros_like(p2)))


@pytest.mark.parametrize("act", ["gelu", "silu", None])
def test_other_activations_unchanged(act):
    """GELU / SiLU / no activation through the raw entry point equal the unchanged ops.conv path bit for bit, and still meet
    the one-rounding contract (the ReLU forms are additional switch cases, not a change to these)."""
    from transvae.hip import _lib as L, ops
    g = torch.Generator().manual_seed(5)
    x = bf((2, 16, 16, 64), g)
    w = torch.randn(128, 3, 3, 64, generator=g) * (2.0 / (9 * 64)) ** 0.5
    bias = torch.randn(128, generator=g) * 0.3
    y_ops = ops.conv(x.to(DEV), w.to(DEV), bias.to(DEV), None, "c3s1", act).cpu()
    out = torch.empty(2, 16, 16, 128, dtype=BF, device=DEV)
    d = ops._desc(batch=2, h_in=16, w_in=16, c_in=64, ldx=64, h_out=16, w_out=16, c_out=128, ldo=128, kh=3, kw=3, stride=1, pad=1,
                  act=ops._act_id(act))
    ops.igemm(d, x.to(DEV), w.to(BF).to(DEV), bias.to(DEV), None, None, out)
    assert torch.equal(out.cpu(), y_ops)
    acc, absdot = conv64(x, w.to(BF), "c3s1")
    y64, slack, _ = epilogue64(acc, absdot, bias, None, act)
    check_one_rounding(y_ops, y64, slack, f"conv + {act}")


# ---------------------------------------------------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 16, 24, 64), (1, 7, 9, 8), (3, 6, 5, 136)])
@pytest.mark.parametrize("kind", ["random", "half_zero"])
def test_maxpool_is_bit_equal_to_torch(shape, kind):
    from transvae.losses import lpips as LP
    g = torch.Generator().manual_seed(11)
    x = bf(shape, g)
    if kind == "half_zero":          # ReLU outputs tie at 0: the gradient must go to the first maximum in torch's scan order
        x = torch.clamp(x.float(), min=0).to(BF)
    xn = x.permute(0, 3, 1, 2).float().requires_grad_(True)
    yn = F.max_pool2d(xn, 2)
    gy = bf(tuple(yn.permute(0, 2, 3, 1).shape), g)
    yn.backward(gy.permute(0, 3, 1, 2).float())
    y = LP.max_pool2x2(x.to(DEV)).cpu()
    assert torch.equal(y.float(), yn.detach().permute(0, 2, 3, 1))
    gx = LP.max_pool2x2_backward(x.to(DEV), gy.to(DEV)).cpu()
    assert torch.equal(gx.float(), xn.grad.permute(0, 2, 3, 1))
    # with the second gradient and the ReLU mask: (route + add) rounded once, zero where x <= 0
    add = bf(shape, g)
    gx2 = LP.max_pool2x2_backward(x.to(DEV), gy.to(DEV), add=add.to(DEV), relu_mask=True).cpu()
    want = (xn.grad.permute(0, 2, 3, 1) + add.float()).to(BF)
    assert torch.equal(gx2, torch.where(x.float() > 0, want, torch.zeros_like(want)))


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
def head64(x, t, lin):
    """fp64 of the head on [B, H, W, C] tensors -> (values [B], magnitude D [B] of the DESIGN 3.1 bound)"""
    nx = x / (torch.sqrt((x ** 2).sum(-1, keepdim=True)) + 1e-10)
    nt = t / (torch.sqrt((t ** 2).sum(-1, keepdim=True)) + 1e-10)
    d = ((nx - nt) ** 2 * lin).sum(-1).mean(dim=(1, 2))
    mag = ((nx.abs() + nt.abs()) ** 2 * lin).sum(-1).mean(dim=(1, 2))
    return d, mag


def head_bound_factor(C, HW):
    """DESIGN.md 3.1 row 'LPIPS head': k(C, HW) fp32 roundings in front of D, from the kernel's documented summation shape."""
    import math
    depth = 8 + int(math.log2(C // 8))                     # adds in a channel sum: 8 per lane + the butterfly
    ppb = 4 * (512 // C) * 16                              # pixels per block
    n_sum = 16 + 6 + 4 + -(-HW // ppb)                     # adds in a pixel sum: per lane, wave butterfly, waves, partials
    return 2 * (depth + 4) + (depth + 2) + n_sum + 2


@pytest.mark.parametrize("C,H,W", [(64, 24, 40), (512, 8, 12)])
def test_head_value_and_gradient(C, H, W):
    from transvae.losses import lpips as LP
    g = torch.Generator().manual_seed(17)
    B = 3
    x = torch.clamp(bf((B, H, W, C), g).float(), min=0).to(BF)
    t = torch.clamp(bf((B, H, W, C), g).float(), min=0).to(BF)
    x[1, 2, 3] = 0                                            # a pixel whose vector is all zero (x only) ...
    x[0, 0, 0] = 0
    t[0, 0, 0] = 0                                            # ... and one where both are
    lin = torch.rand(C, generator=g) * 16 / C
    feat = torch.cat([x, t]).to(DEV)
    out = torch.full((B,), 7.0, device=DEV)
    up = 0.37
    grad = LP.lpips_head(feat, lin.to(DEV), out, want_grad=True, accumulate=False, upstream=up).cpu()
    x64 = x.to(F64).requires_grad_(True)
    d64, mag = head64(x64, t.to(F64), lin.to(F64))
    err = (out.cpu().to(F64) - d64.detach()).abs()
    bound = head_bound_factor(C, H * W) * 2.0 ** -24 * mag.detach()
    print("head value: err / bound =", (err / bound).tolist(), "k =", head_bound_factor(C, H * W))
    assert bool((err <= bound).all()), (err, bound)
    # accumulate adds onto what is there, in call order
    out2 = out.clone()
    assert LP.lpips_head(feat, lin.to(DEV), out2, want_grad=False, accumulate=True) is None
    assert torch.equal(out2, out + out)
    # gradient against fp64 autograd; autograd's own value at an all-zero vector is 0 / 0, the kernel's is defined as 0
    (d64.sum() * up).backward()
    g64 = x64.grad.clone()
    zero_pix = (x.float().abs().sum(-1) == 0)
    assert int(zero_pix.sum()) == 2
    assert bool((grad[zero_pix].float() == 0).all()) and bool(torch.isfinite(grad.float()).all())
    g64[zero_pix] = 0
    assert bool(torch.isfinite(g64).all())
    # one bf16 rounding of an fp32 value whose own error is k 2^-24 of its terms' magnitude
    rel = float((grad.to(F64) - g64).norm() / g64.norm())
    print("head gradient rel-L2 vs fp64:", rel)
    assert rel < 2.0 ** -8                                    # half an ulp per element is 2^-9 relative at worst, ~2^-9.8 rms
    # identical inputs: exactly zero value and gradient
    same = torch.cat([x, x]).to(DEV)
    gs = LP.lpips_head(same, lin.to(DEV), out, want_grad=True, accumulate=False)
    assert bool((out == 0).all()) and bool((gs.float() == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# input preparation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(False, False, False), (True, False, False), (True, True, True)])
def test_prep_and_its_adjoint(net, flags):
    import ctypes as C
    from transvae.hip import _lib as L, ops
    from transvae.losses import lpips as LP
    normalize, sigmoid, clamp = flags
    g = torch.Generator().manual_seed(23)
    B, H, W = 2, 16, 32
    a = torch.randn(B, 3, H, W, generator=g) * (2.0 if sigmoid else 0.6) + (0.0 if sigmoid else 0.5)
    b = torch.rand(B, 3, H, W, generator=g) * 1.4 - 0.2
    fa, fb = LP._prep_flags(normalize, sigmoid, clamp), LP._prep_flags(normalize, False, clamp)
    cols = torch.empty(2 * B, H, W, 32, dtype=BF, device=DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    L.check(L.load().tv_lpips_prep(ops._p(ad), ops._p(bd), ops._p(cols), B, B, H, W, fa, fb, ops._p(net.shift_scale), ops._stream()), "prep")

    def ref(v, sig):
        v = v.to(F64)
        if sig:
            v = torch.sigmoid(v)
        if normalize:
            v = 2 * v - 1
        if clamp:
            v = v.clamp(-1, 1)
        return (v - torch.tensor(R.SHIFT, dtype=F64).view(1, 3, 1, 1)) / torch.tensor(R.SCALE, dtype=F64).view(1, 3, 1, 1)
    a64 = a.to(F64).requires_grad_(True)
    s64 = torch.cat([ref(a64, sigmoid), ref(b, False)])
    patches = F.unfold(s64, 3, padding=1).view(2 * B, 3, 9, H, W).permute(0, 3, 4, 2, 1).reshape(2 * B, H, W, 27)   # (ky, kx, c)
    got = cols.cpu()
    assert float(got[..., 27:].abs().max()) == 0.0
    # one rounding of an fp32 value a few fp32 ulps (sigmoid: 2^-20 relative) from exact
    check_one_rounding(got[..., :27], patches.detach(), 2.0 ** -20 * (patches.detach().abs() + 1.0), "lpips prep")
    dcols = torch.zeros(B, H, W, 32, dtype=BF)
    dcols[..., :27] = bf((B, H, W, 27), g)
    da = torch.empty(B, 3, H, W, device=DEV)
    dc = dcols.to(DEV)
    L.check(L.load().tv_lpips_prep_bwd(ops._p(dc), ops._p(ad), ops._p(da), B, H, W, fa, ops._p(net.shift_scale), ops._stream()), "prep_bwd")
    (patches[:B] * dcols[..., :27].to(F64)).sum().backward()
    rel = float((da.cpu().to(F64) - a64.grad).norm() / a64.grad.norm())
    print("prep adjoint rel-L2 vs fp64:", rel)
    assert rel < 1e-5                                          # fp32 sums of 9 exact bf16 terms, fp32 scalings


@pytest.mark.parametrize("sigmoid", [False, True])
def test_prep_clamp_passes_a_nan_on(net, sigmoid):
    """torch.clamp propagates a NaN: with the clamp flag a NaN pixel of the reconstruction is NaN in exactly the patch columns
    that hold it in the torch restatement (sigmoid, 2x - 1, clamp, scale, unfold), and every other element keeps its bits"""
    from transvae.hip import _lib as L, ops
    from transvae.losses import lpips as LP
    g = torch.Generator().manual_seed(29)
    B, H, W = 2, 16, 32
    a = torch.randn(B, 3, H, W, generator=g) * 2.0
    b = torch.rand(B, 3, H, W, generator=g) * 1.4 - 0.2
    fa, fb = LP._prep_flags(True, sigmoid, True), LP._prep_flags(True, False, True)

    def run(a):
        cols = torch.empty(2 * B, H, W, 32, dtype=BF, device=DEV)
        ad, bd = a.to(DEV), b.to(DEV)
        L.check(L.load().tv_lpips_prep(ops._p(ad), ops._p(bd), ops._p(cols), B, B, H, W, fa, fb, ops._p(net.shift_scale), ops._stream()), "prep")
        return cols.cpu()

    clean = run(a)
    bad = a.clone()
    bad[1, 2, 7, 13] = float("nan")
    bad[0, 0, 0, 0] = float("nan")                         # a corner: its patches are partly padding
    got = run(bad)
    v = torch.sigmoid(bad.to(F64)) if sigmoid else bad.to(F64)
    v = ((2 * v - 1).clamp(-1, 1) - torch.tensor(R.SHIFT, dtype=F64).view(1, 3, 1, 1)) / torch.tensor(R.SCALE, dtype=F64).view(1, 3, 1, 1)
    want = torch.zeros(2 * B, H, W, 32, dtype=torch.bool)
    want[:B, ..., :27] = F.unfold(v, 3, padding=1).view(B, 3, 9, H, W).permute(0, 3, 4, 2, 1).reshape(B, H, W, 27).isnan()
    assert int(want.sum()) == 9 + 4
    assert torch.equal(got.isnan(), want)
    assert torch.equal(got.view(torch.int16)[~want], clean.view(torch.int16)[~want])


# ---------------------------------------------------------------------------------------------------------------------
# whole loss
# ---------------------------------------------------------------------------------------------------------------------
VALUE_FLOOR, GRAD_FLOOR, MARGIN = 1e-2, 3e-2, 1.25      # the floors of the model's bf16 tier (tests/test_model_gpu.py, smoke())


def hip_value_and_grad(net, x, t):
    xd = x.to(DEV).requires_grad_(True)
    v = net(xd, t.to(DEV), normalize=True)
    assert v.shape == (x.shape[0], 1, 1, 1) and v.dtype == torch.float32
    v.sum().backward()
    return v.detach().view(-1).cpu(), xd.grad.detach().cpu()


@pytest.mark.parametrize("pair", R.PAIRS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whole_loss_against_fp32_restatement(net, shape, pair):
    with open(R.GOLDEN) as f:
        dev16 = json.load(f)["cases"][R.case_key(shape, pair)]
    sd = R.plain_state_dict()
    x, t = R.case_inputs(shape, pair)
    v32, g32 = R.value_and_grad(x, t, sd)
    assert torch.allclose(v32, torch.tensor(dev16["values_fp32"]), rtol=1e-3)          # the golden was minted on these inputs
    v, gr = hip_value_and_grad(net, x, t)
    ev, eg = R.rel_l2(v, v32), R.rel_l2(gr, g32)
    bv, bg = max(VALUE_FLOOR, MARGIN * dev16["value"]), max(GRAD_FLOOR, MARGIN * dev16["grad"])
    print(f"lpips {R.case_key(shape, pair)}: value rel-L2 {ev:.3e} (bound {bv:.3e}, autocast {dev16['value']:.3e}); "
          f"grad rel-L2 {eg:.3e} (bound {bg:.3e}, autocast {dev16['grad']:.3e}); values {v.tolist()} vs {v32.tolist()}")
    assert bool(torch.isfinite(gr).all())
    assert ev < bv, (ev, bv)
    assert eg < bg, (eg, bg)


def test_identical_images_give_exact_zero(net):
    x, _ = R.case_inputs((2, 64, 64), "unrelated")
    v, g = hip_value_and_grad(net, x, x.clone())
    assert bool((v == 0).all()), v
    assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


def test_values_do_not_depend_on_the_batch(net):
    x, t = R.case_inputs((2, 64, 64), "noise0.05")
    x2, t2 = R.case_inputs((2, 64, 64), "unrelated")
    X, T = torch.cat([x, x2]).to(DEV), torch.cat([t, t2]).to(DEV)
    with torch.no_grad():
        full = net(X, T, normalize=True).view(-1)
        single = torch.cat([net(X[i:i + 1], T[i:i + 1], normalize=True).view(-1) for i in range(4)])
        again = net(X, T, normalize=True).view(-1)
    assert torch.equal(full, again)
    assert torch.equal(full, single), (full, single)


def test_normalize_and_patched_variant(net):
    """normalize=True equals the explicit 2x - 1 bit for bit; the patched loss's order (sigmoid, 2x - 1, clamp) equals the same
    transforms applied with torch first (up to the sigmoid's own 2^-20)."""
    g = torch.Generator().manual_seed(29)
    x, t = torch.rand(1, 3, 32, 32, generator=g).to(DEV), torch.rand(1, 3, 32, 32, generator=g).to(DEV)
    with torch.no_grad():
        assert torch.equal(net(x, t, normalize=True), net(2 * x - 1, 2 * t - 1))
        logits = torch.randn(1, 3, 32, 32, generator=g).to(DEV) * 2
        tt = t * 1.3 - 0.1
        a = net.distance(logits, tt, normalize=True, sigmoid_input=True, clamp=True)
        b = net((torch.sigmoid(logits) * 2 - 1).clamp(-1, 1), (tt * 2 - 1).clamp(-1, 1))
    assert abs(float(a) - float(b)) < 2e-2 * abs(float(b))


# ---------------------------------------------------------------------------------------------------------------------
# integration
# ---------------------------------------------------------------------------------------------------------------------
def micro_model():
    from oracle import filler
    from oracle import transvae_oracle as O
    from transvae import TransVAE
    cfg = dict(O.MICRO)
    sd = filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4))
    m = TransVAE(config=cfg, variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(sd)
    return m.to(DEV), filler


def test_loss_integration(net):
    from transvae import TransVAELoss
    m, filler = micro_model()
    x = filler.rand_input("micro.x", (2, 3, 64, 64)).to(DEV)
    eps = filler.randn_input("micro.eps", (2, 4, 4, 4)).to(DEV)
    loss_fn = TransVAELoss(l1_weight=1.0, lpips_weight=1.0, kl_weight=1e-3, lpips_net=net)
    recon, mu, logvar = m(x, eps=eps)
    out = loss_fn(recon, x, mu, logvar)
    assert set(out) == {"l1", "lpips", "kl", "total"}
    total = out["l1"] + out["lpips"] + out["kl"]
    assert torch.equal(out["total"], total)
    with torch.no_grad():
        direct = net(recon.detach() * 2 - 1, x * 2 - 1).mean()
    assert abs(float(out["lpips"]) - float(direct)) <= 1e-6 * abs(float(direct)) and float(direct) > 0
    # against the closed-form-only loss: the other terms are untouched
    base = TransVAELoss(l1_weight=1.0, lpips_weight=0.0, kl_weight=1e-3)(recon, x, mu, logvar)
    assert torch.equal(base["l1"], out["l1"]) and torch.equal(base["kl"], out["kl"])
    out["total"].backward()
    missing = [n for n, p in m.named_parameters() if p.requires_grad and (p.grad is None or not bool(torch.isfinite(p.grad).all()))]
    assert not missing, missing
    zero = [n for n, p in m.named_parameters() if p.requires_grad and float(p.grad.abs().max()) == 0.0]
    assert not zero, zero
    assert all(b.grad is None for b in net.buffers())
    # the patched variant runs and differs
    outp = TransVAELoss(l1_weight=1.0, lpips_weight=0.5, kl_weight=1e-3, sigmoid_recon=True, lpips_net=net)(recon.detach(), x, mu.detach(), logvar.detach())
    with torch.no_grad():
        dp = 0.5 * net((torch.sigmoid(recon.detach()) * 2 - 1).clamp(-1, 1), (x * 2 - 1).clamp(-1, 1)).mean()
    assert abs(float(outp["lpips"]) - float(dp)) < 2e-2 * abs(float(dp))


def test_evaluate_integration(net):
    from transvae import evaluate, reconstruction_metrics
    m, filler = micro_model()
    imgs = filler.rand_input("micro.x", (4, 3, 64, 64))
    loader = [(imgs[:3], None), (imgs[3:], None)]

    class Fixed(torch.nn.Module):            # deterministic "model": evaluate()'s model(images) samples z otherwise
        def forward(self, x):
            return (m.decode(m.encode(x)[0]),)
    model = Fixed()
    res = evaluate(model, loader, metrics=("psnr", "ssim", "lpips"), device=DEV, per_image=True, lpips_net=net)
    assert set(res) == {"psnr", "ssim", "lpips"}
    with torch.no_grad():
        x = imgs.to(DEV)
        rec = torch.cat([model(x[:3])[0], model(x[3:])[0]])
        direct = torch.cat([net(x[:3], rec[:3], normalize=True), net(x[3:], rec[3:], normalize=True)]).view(-1)
        rm = reconstruction_metrics(rec, x)
    assert res["lpips"]["values"].shape == (4,)
    assert (res["lpips"]["values"] == direct.cpu().double().numpy()).all()
    assert (res["psnr"]["values"] == rm["psnr"].cpu().double().numpy()).all()
    assert (res["ssim"]["values"] == rm["ssim"].cpu().double().numpy()).all()
    assert abs(res["lpips"]["mean"] - float(direct.double().mean())) < 1e-12
