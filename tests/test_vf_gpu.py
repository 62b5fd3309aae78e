"""VF alignment term on the MI355X: every new kernel against fp64 of the same inputs under its row V of the rounding contract
(references, bounds and their mutation checks in tests/test_vf_host.py), the existing GEMM and attention
kernels at the ViT's shapes under their rows G and A, the whole extractor against the plain-torch fp32 restatement
(tests/vf_restatement.py) under the project's bf16-tier rule with the bf16-residual-stream yardstick, the head against fp64
autograd under row X, and the TransVAELoss integration."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

import vf_restatement as R
import test_vf_host as H
from test_error_budget_gpu import _sample_groups, report
from test_error_budget_host import (BF, F64, attn_exact, attn_fwd_emul, attn_inputs, check_one_rounding, check_vs_emulation, conv64,
                                    epilogue64, gemm_inputs, r16, rel_l2)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# the new kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("shape,size", H.PREP_CASES)
def test_prep_is_one_rounding_of_fp64(shape, size, norm):
    from transvae.losses import vf as V
    img = H.prep_image(shape)
    rows = V.vf_prep(img.to(DEV), size[0] // 14, size[1] // 14, norm).cpu()
    v64 = H.prep64(img, size, norm)
    assert rows.shape == (v64.shape[0], H.K_PAD) and float(rows[:, H.K_PATCH:].abs().max()) == 0.0
    rep = check_one_rounding(rows[:, :H.K_PATCH], v64, H.prep_slack(v64), "tv_vf_prep")
    report(f"[V] tv_vf_prep {shape} -> {size} norm={norm} (ratio, max ulps, bias)", tuple(round(v, 3) for v in rep))


def test_tokens_are_one_rounding_of_patch_plus_pos():
    from transvae.losses import vf as V
    B, P, D = 3, 23, 384
    patch, cls, pos = H.token_inputs(B, P, D)
    tok = V.vit_tokens(patch.to(DEV), cls.to(DEV), pos.to(DEV), B).cpu()
    t64, slack = H.tokens64(patch, cls, pos, B)
    rep = check_one_rounding(tok, t64, slack, "tv_vit_tokens")
    check_one_rounding(tok[:, 0], t64[:, 0], slack[:, 0], "tv_vit_tokens class row", min_bias_n=10 ** 9)
    report("[V] tv_vit_tokens (ratio, max ulps, bias)", tuple(round(v, 3) for v in rep))


@pytest.mark.parametrize("Cc", [384, 768, 1024])
def test_layernorm_mode2_and_final_norm(Cc):
    """T = 771 rows (3 x 257), both chunk counts; rows with |mean| / std up to ~350, spiked channels, a zero and a constant row"""
    from transvae.losses import vf as V
    T, B = 771, 3
    x = H.ln_inputs(T, Cc, seed=T + Cc)
    xd = x.to(DEV, BF).contiguous()
    y = V.layernorm_hat(xd).cpu()
    y64, mu, s = H.ln64(x)
    rep = check_one_rounding(y, y64, H.ln_slack(y64, x, mu, s), "tv_rownorm_fwd mode 2")
    assert abs(rep[2]) <= 0.02, rep
    g = torch.Generator().manual_seed(Cc)
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    out = V.layernorm_rows(xd.view(B, T // B, Cc), gamma.to(DEV), beta.to(DEV), 1).cpu()
    y64f, bound = H.final_norm64(x, gamma, beta)
    keep = lambda t: t.view(B, T // B, Cc)[:, 1:].reshape(-1, Cc)
    assert out.shape == (B * (T // B - 1), Cc) and out.dtype == torch.float32
    ratio = ((out.to(F64) - keep(y64f)).abs() / keep(bound)).max().item()
    report(f"[V] LayerNorm {T}x{Cc}: mode 2 (ratio, max ulps, bias), final norm |err| / bound", (tuple(round(v, 3) for v in rep), round(ratio, 3)))
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the existing kernels at the ViT's shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,form", [(771, 384, 1152, "bias"), (194, 1536, 384, "residual"), (514, 608, 384, "bias"), (771, 384, 1536, "gelu")])
def test_block_gemms_at_vit_shapes(M, K, N, form):
    """[G] ragged M; K = 608 is the patch embedding's padded K"""
    from transvae.hip import _lib as L, ops
    from transvae.losses import vf as V
    x, w, b, res = gemm_inputs(M, K, N, seed=M + K + N)
    acc, absdot = conv64(x, w, "linear")
    xd, wb, bd = x.to(DEV, BF), w.to(DEV, BF).contiguous(), b.float().to(DEV)
    rd = res.to(DEV, BF) if form == "residual" else None
    y = V._linear(xd, wb, bd, residual=rd, act=L.ACT_GELU if form == "gelu" else L.ACT_NONE).cpu()
    y64, sl, _ = epilogue64(acc, absdot, b, res if form == "residual" else None, "gelu" if form == "gelu" else None)
    rep = check_one_rounding(y, y64, sl, f"linear {M}x{K}x{N} {form}")
    report(f"[G] linear {M}x{K}x{N} {form} (ratio, max ulps, bias)", tuple(round(v, 3) for v in rep))


@pytest.mark.parametrize("N", [257, 97])
def test_attention_at_vit_token_counts(N):
    """[A] heads 6, no table, the ragged token counts of a 224 x 224 and a 112 x 168 image"""
    from transvae.losses import vf as V
    heads = 6
    sl = [attn_inputs(N, seed=N + h) for h in range(heads)]
    qkv = torch.cat([torch.cat([s[i] for s in sl], 1) for i in range(3)], 1)[None].float()
    o = V.attention_fwd(qkv.to(DEV, BF).contiguous(), heads).cpu().to(F64)[0]
    res = {}
    for h in range(heads):
        q, k, v = sl[h]
        o_ex, _ = attn_exact(q, k, v, 0.125)
        grp = _sample_groups(N, 12)
        rows = torch.cat([torch.arange(g0 * 32, min(N, g0 * 32 + 32)) for g0 in grp])
        o_e = torch.cat([attn_fwd_emul(q[g0 * 32:min(N, g0 * 32 + 32)], k, v, 0.125, kblock=64, group=32)[0] for g0 in grp])
        res[f"o h{h}"] = check_vs_emulation(o[rows, h * 64:h * 64 + 64], o_e, o_ex[rows], f"o head {h}")
    report(f"[A] N={N} heads=6 (relL2 ratio, max ratio)", {k: tuple(round(v, 3) for v in t) for k, t in res.items()})


# ---------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------
FLOOR, MARGIN = 1e-2, 1.25


def build_net(name):
    from transvae import DinoV2Features
    variant, depth, _, _, size = R.CASES[name]
    sd = R.state_dict(variant, depth)
    return DinoV2Features(variant, size=size, depth=depth).load_dinov2_state_dict(R.hub_state_dict(sd)).to(DEV), sd


@pytest.mark.parametrize("name", list(R.CASES))
def test_whole_network_against_fp32_restatement(name):
    with open(R.GOLDEN) as f:
        gold = json.load(f)["cases"][name]
    variant, depth, B, _, size = R.CASES[name]
    net, sd = build_net(name)
    img = R.case_inputs(name)
    with torch.no_grad():
        f32 = R.features(img, sd, variant, size)
    assert abs(float(f32.double().norm()) - gold["norm_fp32"]) < 1e-3 * gold["norm_fp32"]      # the golden was minted on these inputs
    got = net(img.to(DEV))
    assert got.shape == f32.shape and got.dtype == torch.float32 and not got.requires_grad
    err = rel_l2(got.cpu(), f32)
    bound = max(FLOOR, MARGIN * gold["autocast_bf16_stream"])
    report(f"[V] {name}: rel-L2 {err:.3e} (bound {bound:.3e}); ratio to (a) autocast {err / gold['autocast']:.3f}, to (b) bf16 stream "
           f"{err / gold['autocast_bf16_stream']:.3f}", "")
    assert bool(torch.isfinite(got).all())
    assert err < bound, (err, bound)
    # the token-major result is the same memory, and the raw-image form differs
    tok, (b_, h, w) = net.tokens(img.to(DEV))
    assert (b_, h, w) == (B, size[0] // 14, size[1] // 14) and torch.equal(tok.view(B, h, w, -1).permute(0, 3, 1, 2), got)
    if B == 3:        # a batch equals the same images run one at a time, bit for bit
        single = torch.cat([net(img[i:i + 1].to(DEV)) for i in range(B)])
        assert torch.equal(single, got)
        assert torch.equal(net(img.to(DEV)), got)


def test_raw_image_form_matches_the_restatement():
    from transvae import DinoV2Features
    name = "vits14-d2-3x96x128-to-224"
    variant, depth, _, _, size = R.CASES[name]
    sd = R.state_dict(variant, depth)
    net = DinoV2Features(variant, size=size, depth=depth, imagenet_norm=False).load_dinov2_state_dict(sd).to(DEV)
    img = R.case_inputs(name)[:1]
    with torch.no_grad():
        f32 = R.features(img, sd, variant, size, imagenet_norm=False)
    assert rel_l2(net(img.to(DEV)).cpu(), f32) < FLOOR


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
def run_head(lat, feats, weight, bias, train_proj=True):
    from transvae import VFLoss
    D, Cc = lat.shape[1], feats.shape[1]
    vf = VFLoss(D, Cc).to(DEV)
    if weight is not None:
        with torch.no_grad():
            vf.proj.weight.copy_(weight)
            vf.proj.bias.copy_(bias)
        vf.proj.requires_grad_(train_proj)
    else:
        assert vf.proj is None
    ld = lat.to(DEV).requires_grad_(True)
    v = vf(ld, feats.to(DEV))
    v.backward()
    dw = vf.proj.weight.grad.cpu() if weight is not None and train_proj else None
    db = vf.proj.bias.grad.cpu() if weight is not None and train_proj else None
    return v.detach().cpu(), ld.grad.cpu(), dw, db


@pytest.mark.parametrize("name", list(H.HEAD_CASES))
def test_head_against_fp64_autograd(name):
    lat, feats, weight, bias = H.head_inputs(name)
    want = H.head64(lat, feats, weight, bias)
    got = run_head(lat, feats, weight, bias)
    out = H.check_head(got, want, f"tv_vf_head {name}")
    report(f"[V] tv_vf_head {name}", {k: f"{v:.2e}" for k, v in out.items()})
    again = run_head(lat, feats, weight, bias)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    if weight is not None:       # a frozen projection: same value and latent gradient, no projection gradient
        frozen = run_head(lat, feats, weight, bias, train_proj=False)
        assert torch.equal(frozen[0], got[0]) and torch.equal(frozen[1], got[1]) and frozen[2] is None
    # gate shut: features = the projected latent, similarity 1
    (B, D, Hl, Wl), (h, w), Cc, proj = H.HEAD_CASES[name]
    z = F.interpolate(lat, size=(h, w), mode="bilinear", align_corners=False)
    same = F.linear(z.flatten(2).transpose(1, 2), weight, bias).transpose(1, 2).reshape(B, Cc, h, w) if proj else z
    shut = run_head(lat, same.contiguous(), weight, bias)
    assert float(shut[0]) == 0.0
    assert all(float(t.abs().max()) == 0.0 and bool(torch.isfinite(t).all()) for t in shut[1:] if t is not None)


# ---------------------------------------------------------------------------------------------------------------------
# integration
# ---------------------------------------------------------------------------------------------------------------------
def test_loss_integration():
    from oracle import filler
    from oracle import transvae_oracle as O
    from transvae import DinoV2Features, TransVAE, TransVAELoss, VFLoss
    cfg = dict(O.MICRO)
    m = TransVAE(config=cfg, variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4)))
    m = m.to(DEV)
    x = filler.rand_input("micro.x", (2, 3, 64, 64)).to(DEV)
    eps = filler.randn_input("micro.eps", (2, 4, 4, 4)).to(DEV)
    net = DinoV2Features("vits14", depth=2).load_dinov2_state_dict(R.state_dict("vits14", 2)).to(DEV)
    vf = VFLoss(4, 384).to(DEV)
    loss_fn = TransVAELoss(l1_weight=1.0, lpips_weight=0.0, kl_weight=1e-3, vf_weight=0.1, vf_loss=vf)
    recon, mu, logvar = m(x, eps=eps)
    mu.retain_grad()
    out = loss_fn(recon, x, mu, logvar, dinov2=net)
    assert list(out) == ["l1", "kl", "vf", "total"]
    assert torch.equal(out["total"], out["l1"] + out["kl"] + out["vf"])
    base = TransVAELoss(l1_weight=1.0, lpips_weight=0.0, kl_weight=1e-3, vf_weight=0.1, vf_loss=vf)(recon, x, mu, logvar)
    assert list(base) == ["l1", "kl", "total"] and torch.equal(base["l1"], out["l1"]) and torch.equal(base["kl"], out["kl"])
    out["total"].backward(retain_graph=True)
    g_total = mu.grad.clone()
    mu.grad = None
    base["total"].backward(retain_graph=True)
    g_base = mu.grad.clone()
    mu2 = mu.detach().clone().requires_grad_(True)
    direct = vf(mu2, net(x))
    assert abs(float(out["vf"].detach()) - 0.1 * float(direct.detach())) <= 1e-6 * abs(float(direct.detach())) and float(direct.detach()) > 0
    direct.backward()
    want = g_base.double() + 0.1 * mu2.grad.double()
    assert float(mu2.grad.abs().max()) > 0
    err = float((g_total.double() - want).norm() / want.norm())
    report("[V] TransVAELoss mu gradient: rel-L2 against L1 + KL + 0.1 x head", f"{err:.2e}")
    assert err <= 1e-6
    assert all(b.grad is None and not b.requires_grad for b in net.buffers())
    assert vf.proj.weight.grad is not None and float(vf.proj.weight.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="VF"):
        loss_fn(recon.detach(), x, mu.detach(), logvar.detach(), dinov2=torch.nn.Identity())
