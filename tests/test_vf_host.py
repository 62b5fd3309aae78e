"""VF alignment term, host side: the restatement's loss against an independent fp64 formula, the loader, the position-table
interpolation, the pack-time folds, and fp32 emulations of the new kernels (csrc/vf.hip, the plain LayerNorm of csrc/norm.hip) in
the kernels' order of operations, held to the bounds of DESIGN.md section 3.1 rows V -- with mutation checks showing that those
bounds reject specific defects.  tests/test_vf_gpu.py imports the references and bounds from here."""
import math

import pytest
import torch
import torch.nn.functional as F

import vf_restatement as R
from test_error_budget_host import BF, F64, check_one_rounding, r16, rel_l2, rms_ln_inputs

K_PATCH, K_PAD = 588, 608


# ---------------------------------------------------------------------------------------------------------------------
# references (fp64) and bounds
# ---------------------------------------------------------------------------------------------------------------------
def prep64(img, size, imagenet_norm):
    """fp64 patch rows [B*h*w, 588] in (c, ky, kx) order of the resized (and normalised) image"""
    x = F.interpolate(img.to(F64), size=size, mode="bilinear", align_corners=False)
    if imagenet_norm:
        x = (x - torch.tensor(R.IMAGENET_MEAN, dtype=F64).view(1, 3, 1, 1)) / torch.tensor(R.IMAGENET_STD, dtype=F64).view(1, 3, 1, 1)
    return F.unfold(x, 14, stride=14).transpose(1, 2).reshape(-1, K_PATCH)


def prep_slack(v64):
    return 2.0 ** -20 * (1.0 + v64.abs())                       # the tv_lpips_prep row: a few fp32 roundings of O(1) terms


def tokens64(patch, cls, pos, B):
    """patch [B*P, D] (bf16 values), cls [D], pos [1 + P, D] -> ([B, 1 + P, D] fp64, slack)"""
    P, D = patch.shape[0] // B, patch.shape[1]
    body = patch.to(F64).view(B, P, D)
    head = cls.to(F64).view(1, 1, D).expand(B, 1, D)
    raw = torch.cat([head, body], 1)
    return raw + pos.to(F64)[None], 2.0 ** -24 * (raw.abs() + pos.to(F64).abs()[None])


def ln64(x, eps=1e-6):
    """-> (xhat64, mu, s) of rows x [T, C]"""
    x = x.to(F64)
    mu = x.mean(1, keepdim=True)
    s = torch.rsqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    return (x - mu) * s, mu, s


def ln_slack(y64, x, mu, s):
    """row V (LayerNorm mode 2), the mode-1 form: mu is an fp32 sum, x - mu one rounding, s carries the fp32 variance and rsqrt"""
    return 2.0 ** -20 * (s * (x.to(F64).abs() + mu.abs()) + y64.abs())


def final_norm64(x, gamma, beta, eps=1e-6):
    """-> (y64, bound): y = xhat gamma + beta in fp32 from an xhat with ln_slack's error, one fma (2^-24 of its terms, doubled)"""
    xh, mu, s = ln64(x, eps)
    g, b = gamma.to(F64), beta.to(F64)
    y = xh * g + b
    return y, ln_slack(xh, x, mu, s) * g.abs() + 2.0 ** -23 * (y.abs() + b.abs())


def head64(lat, feats, weight, bias, margin=0.4):
    """fp64 autograd of the restatement -> (value, dlat, dw | None, db | None)"""
    lat = lat.to(F64).clone().requires_grad_(True)
    w = weight.to(F64).clone().requires_grad_(True) if weight is not None else None
    b = bias.to(F64).clone().requires_grad_(True) if bias is not None else None
    v = R.vf_loss(lat, feats.to(F64), w, b, margin)
    v.backward()
    zero = torch.zeros_like
    return (v.detach(), lat.grad if lat.grad is not None else zero(lat), None if w is None else (w.grad if w.grad is not None else zero(w)),
            None if b is None else (b.grad if b.grad is not None else zero(b)))


HEAD_VALUE_RTOL, HEAD_GRAD_RTOL = 1e-6, 1e-5                    # row X (tv_gan_loss)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' order of operations
# ---------------------------------------------------------------------------------------------------------------------
def taps(n_in, n_out, align_corners=False):
    """(i0, i1, l fp32) per output index: src = ((2 o + 1) n_in - n_out) / (2 n_out) in integers, one rounding of l"""
    o = torch.arange(n_out, dtype=torch.int64)
    if align_corners:
        src = o.to(F64) * (n_in - 1) / max(n_out - 1, 1)
        i0 = src.floor().to(torch.int64)
        l = (src - i0).float()
    else:
        num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
        pos = num > 0
        i0 = torch.where(pos, num // den, torch.zeros_like(num))
        l = torch.where(pos, (num - i0 * den).float() / float(den), torch.zeros(n_out))
    return i0, torch.clamp(i0 + 1, max=n_in - 1), l


def bilinear_emul(img, size, align_corners=False):
    """fp32: top = (1 - lx) p00 + lx p01, bot likewise, (1 - ly) top + ly bot"""
    y0, y1, ly = taps(img.shape[2], size[0], align_corners)
    x0, x1, lx = taps(img.shape[3], size[1], align_corners)
    img = img.float()
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    r0, r1 = img[:, :, y0], img[:, :, y1]
    top = (1 - lx) * r0[..., x0] + lx * r0[..., x1]
    bot = (1 - lx) * r1[..., x0] + lx * r1[..., x1]
    return (1 - ly) * top + ly * bot


def prep_emul(img, size, imagenet_norm, mutate=None):
    x = bilinear_emul(img, size, align_corners=(mutate == "align_corners"))
    mean = torch.tensor(R.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(R.IMAGENET_STD).view(1, 3, 1, 1)
    if mutate == "norm_after_rounding":
        x = x.to(BF).float()
    if imagenet_norm:
        x = (x - mean) / std
    rows = torch.zeros(x.shape[0] * (size[0] // 14) * (size[1] // 14), K_PAD, dtype=BF)
    rows[:, :K_PATCH] = F.unfold(x, 14, stride=14).transpose(1, 2).reshape(-1, K_PATCH).to(BF)
    return rows


def tokens_emul(patch, cls, pos, B, mutate=None):
    P, D = patch.shape[0] // B, patch.shape[1]
    raw = torch.cat([cls.float().view(1, 1, D).expand(B, 1, D), patch.float().view(B, P, D)], 1)
    p = pos.float()
    if mutate == "pos_row_p":
        p = torch.cat([p[:1], p[:-1]])                        # patch p gets pos[p] instead of pos[1 + p]
    return (raw + p[None]).to(BF)


def ln_emul(x, eps=1e-6, mutate=None):
    """fp32, two passes: mu = sum x / C, d = x - mu, s = rsqrt(sum d^2 / C + eps) -> fp32 d s (the caller rounds)"""
    xf = x.float()
    inv_c = torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    mu = xf.sum(1, keepdim=True) * inv_c
    d = xf - mu
    if mutate == "one_pass":
        var = (xf * xf).sum(1, keepdim=True) * inv_c - mu * mu
        s = torch.rsqrt(torch.clamp(var, min=0) + eps)
    else:
        s = torch.rsqrt((d * d).sum(1, keepdim=True) * inv_c + eps)
    return d * s


def final_norm_emul(x, gamma, beta, B, skip=1, mutate=None):
    N = x.shape[0] // B
    y = (ln_emul(x) * gamma.float() + beta.float()).view(B, N, -1)
    if mutate == "cls_included":
        return y[:, :N - skip].reshape(B * (N - skip), -1)
    return y[:, skip:].reshape(B * (N - skip), -1)


def head_emul(lat, feats, weight, bias, margin=0.4, mutate=None):
    """fp32 per-position terms, fp64 mean, the kernel's alpha / beta form of the gradient -> (value, dlat, dw, db)"""
    B, C, h, w = feats.shape
    D = lat.shape[1]
    lat32 = lat.float().clone().requires_grad_(True)
    z = bilinear_emul(lat32, (h, w)).permute(0, 2, 3, 1).reshape(-1, D)
    f = feats.float().permute(0, 2, 3, 1).reshape(-1, C)
    zd = z.detach()
    y = zd @ weight.float().t() + bias.float() if weight is not None else zd
    yf, yy, ff = (y * f).sum(1), (y * y).sum(1), (f * f).sum(1)
    ny, nf = yy.sqrt(), ff.sqrt()
    cy, cf = ny.clamp_min(1e-12), nf.clamp_min(1e-12)
    cos = yf / (cy * cf)
    T = cos.numel()
    sim = cos.double().sum() / T
    if mutate == "mean_over_channels":
        sim = ((y / cy[:, None]) * (f / cf[:, None])).double().mean()
    m = margin - sim
    gate = 1.0 if (m >= 0 or mutate == "gate_open") else 0.0
    value = torch.clamp(m, min=0.0)
    g = torch.tensor(-1.0 / T, dtype=torch.float32)
    alpha = g / (cy * cf)
    beta = torch.where(ny > 1e-12, g * yf / (cy * cy * cy * cf), torch.zeros_like(yf))
    gy = alpha[:, None] * f - beta[:, None] * y
    gz = gy @ weight.float() if weight is not None else gy
    z.backward(gz * gate)
    dw = (gy.t() @ zd) * gate if weight is not None else None
    db = gy.sum(0) * gate if weight is not None else None
    return value, lat32.grad, dw, db


# ---------------------------------------------------------------------------------------------------------------------
# the restatement's loss, the loader, the position table, the folds
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_loss_equals_an_independent_formula():
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(2, 16, 8, 8, generator=g, dtype=F64)
    feats = torch.randn(2, 48, 8, 8, generator=g, dtype=F64)
    w, b = torch.randn(48, 16, generator=g, dtype=F64), torch.randn(48, generator=g, dtype=F64)
    v = R.vf_loss(lat, feats, w, b, 0.4)
    tot = 0.0
    for bi in range(2):
        for y in range(8):
            for x in range(8):
                yv = w @ lat[bi, :, y, x] + b
                fv = feats[bi, :, y, x]
                tot += float(yv @ fv) / (float(yv.norm()) * float(fv.norm()))
    assert abs(float(v) - max(0.4 - tot / 128, 0.0)) < 1e-12
    # a resized latent: the same with F.interpolate's bilinear samples; and the gate
    lat2 = torch.randn(2, 16, 4, 6, generator=g, dtype=F64)
    up = F.interpolate(lat2, size=(8, 8), mode="bilinear", align_corners=False)
    assert abs(float(R.vf_loss(lat2, feats, w, b)) - float(R.vf_loss(up, feats, w, b))) < 1e-15
    same = F.linear(lat.flatten(2).transpose(1, 2), w, b).transpose(1, 2).reshape(2, 48, 8, 8)
    assert float(R.vf_loss(lat, same, w, b)) == 0.0


def test_loader_round_trip_and_refusals():
    from transvae.losses import vf as V
    plain = R.state_dict("vits14", depth=2)
    hub = R.hub_state_dict(plain)
    hub = {("backbone." + k if i % 2 else k): v for i, (k, v) in enumerate(hub.items())}
    back = V.to_plain_keys(hub)
    assert sorted(back) == sorted(V.plain_keys(2)) == sorted(plain)
    assert all(torch.equal(back[k], plain[k]) for k in plain)
    chunked = {k.replace("blocks.", "blocks.0."): v for k, v in plain.items()}
    assert sorted(V.to_plain_keys(chunked)) == sorted(plain)
    net = V.DinoV2Features("vits14", depth=2).load_dinov2_state_dict(hub)
    assert torch.equal(net.pos_embed, plain["pos_embed"]) and torch.equal(net.blocks_1_ls2_gamma, plain["blocks.1.ls2.gamma"])
    assert net._op_pe.shape == (384, K_PAD) and net._op_pe.dtype == BF and float(net._op_pe[:, K_PATCH:].abs().max()) == 0.0
    again = V.DinoV2Features("vits14", depth=2)
    again.load_state_dict(net.state_dict())
    assert torch.equal(again._op_1_fc2_w, net._op_1_fc2_w) and torch.equal(again._op_0_qkv_b, net._op_0_qkv_b)
    with pytest.raises(ValueError, match="register"):
        V.to_plain_keys({**plain, "register_tokens": torch.zeros(1, 4, 384)})
    with pytest.raises(ValueError, match="SwiGLU"):
        V.to_plain_keys({**plain, "blocks.0.mlp.w12.weight": torch.zeros(8, 384)})
    with pytest.raises(KeyError, match="missing"):
        V.DinoV2Features("vits14", depth=2).load_dinov2_state_dict({k: v for k, v in plain.items() if k != "norm.bias"})
    with pytest.raises(KeyError, match="wrong shape"):
        V.DinoV2Features("vitb14", depth=2).load_dinov2_state_dict(plain)
    with pytest.raises(ValueError):
        V.DinoV2Features("vitg14")
    with pytest.raises(ValueError):
        V.DinoV2Features("vits14", size=(224, 225))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 3, 32, 32))


@pytest.mark.parametrize("hw", [(16, 16), (8, 12), (37, 37)])
def test_position_table_interpolation(hw):
    from transvae.losses import vf as V
    g = torch.Generator().manual_seed(2)
    pos = torch.randn(1, 1 + 37 * 37, 24, generator=g)
    h, w = hw
    tab = V.interpolate_pos_table(pos, h, w, offset=0.1, antialias=False)
    assert tab.shape == (1 + h * w, 24) and torch.equal(tab[0], pos[0, 0])
    if hw == (37, 37):
        assert torch.equal(tab, pos[0])
        return
    grid = pos[:, 1:].reshape(1, 37, 37, 24).permute(0, 3, 1, 2)
    want = F.interpolate(grid, scale_factor=((h + 0.1) / 37, (w + 0.1) / 37), mode="bicubic", antialias=False)
    assert torch.equal(tab[1:], want.permute(0, 2, 3, 1).reshape(h * w, 24))
    assert torch.equal(tab, R.pos_table(pos, h, w)[0])
    plain_size = V.interpolate_pos_table(pos, h, w, offset=0.0)
    assert torch.equal(plain_size[1:], F.interpolate(grid, size=(h, w), mode="bicubic").permute(0, 2, 3, 1).reshape(h * w, 24))


def test_folds_are_exact_in_fp64():
    from transvae.losses import vf as V
    sd = {k: v.to(F64) for k, v in R.state_dict("vits14", depth=1).items()}
    f = V.fold_block(sd, 0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 384, generator=g, dtype=F64) * 3 + 2
    p = "blocks.0."
    xh = ln64(x)[0]
    for nm, norm in (("attn.qkv", "norm1"), ("mlp.fc1", "norm2")):
        want = F.linear(F.layer_norm(x, (384,), sd[p + norm + ".weight"], sd[p + norm + ".bias"], 1e-6), sd[p + nm + ".weight"], sd[p + nm + ".bias"])
        got = F.linear(xh, f[nm.split(".")[1] + ".w"], f[nm.split(".")[1] + ".b"])
        assert rel_l2(got, want) < 1e-14
    o = torch.randn(7, 384, generator=g, dtype=F64)
    assert rel_l2(F.linear(o, f["proj.w"], f["proj.b"]), sd[p + "ls1.gamma"] * F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])) < 1e-14
    hdn = torch.randn(7, 1536, generator=g, dtype=F64)
    assert rel_l2(F.linear(hdn, f["fc2.w"], f["fc2.b"]), sd[p + "ls2.gamma"] * F.linear(hdn, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])) < 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# emulations inside the bounds, mutations outside
# ---------------------------------------------------------------------------------------------------------------------
PREP_CASES = [((2, 64, 96), (224, 224)), ((1, 256, 256), (224, 224)), ((1, 300, 260), (224, 224)), ((1, 300, 260), (112, 168))]


def prep_image(shape, seed=5):
    B, H, W = shape
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed + H))


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("shape,size", PREP_CASES)
def test_prep_emulation_and_mutations(shape, size, norm):
    img = prep_image(shape)
    v64 = prep64(img, size, norm)
    rows = prep_emul(img, size, norm)
    assert float(rows[:, K_PATCH:].abs().max()) == 0.0
    check_one_rounding(rows[:, :K_PATCH], v64, prep_slack(v64), "vf prep")
    with pytest.raises(AssertionError):
        check_one_rounding(prep_emul(img, size, norm, "align_corners")[:, :K_PATCH], v64, prep_slack(v64), "align_corners=True")
    if norm:
        with pytest.raises(AssertionError):
            check_one_rounding(prep_emul(img, size, norm, "norm_after_rounding")[:, :K_PATCH], v64, prep_slack(v64), "normalised after rounding")


def token_inputs(B=2, P=9, D=384, seed=7):
    g = torch.Generator().manual_seed(seed)
    patch = (torch.randn(B * P, D, generator=g) * 2).to(BF)
    cls = torch.randn(D, generator=g)
    pos = torch.randn(1 + P, D, generator=g)
    pos[:, R.SPIKE_CHANNEL] *= R.SPIKE
    return patch, cls, pos


def test_tokens_emulation_and_mutation():
    patch, cls, pos = token_inputs()
    t64, slack = tokens64(patch, cls, pos, 2)
    check_one_rounding(tokens_emul(patch, cls, pos, 2), t64, slack, "vit tokens", min_bias_n=10 ** 9)
    with pytest.raises(AssertionError):
        check_one_rounding(tokens_emul(patch, cls, pos, 2, "pos_row_p"), t64, slack, "pos row p", min_bias_n=10 ** 9)


def ln_inputs(T, C, seed=0):
    """rows of rms_ln_inputs (|mean| / std around 0, 4-8 and 32-100; a zero and a constant row) with, on every fifth row, one
    channel spiked to 50 x the row's scale (the outlier channel of the restatement's position table), and on rows 7 mod 10 a
    common offset of ~350 std -- as far as bf16 inputs can sit from 0 (three or four levels per row).  There fp32's
    E[x^2] - mean^2 is off by percents of the variance: the 1-ulp bound cannot see a one-pass variance at |mean| / std = 100
    (0.1 ulp), it does see it on these rows."""
    x, _, _ = rms_ln_inputs(T, C, seed=seed)
    x = x.clone()
    rows = torch.arange(5, T, 5)
    x[rows, R.SPIKE_CHANNEL] = x[rows].abs().mean(1) * R.SPIKE
    g = torch.Generator().manual_seed(seed + 1)
    far = torch.arange(7, T, 10)
    sc = torch.exp2(torch.randint(-3, 4, (far.numel(), 1), generator=g).to(F64))
    sign = torch.where(torch.rand(far.numel(), 1, generator=g) < 0.5, -1.0, 1.0).to(F64)
    x[far] = (1000.0 * sign + 3.0 * torch.randn(far.numel(), C, generator=g, dtype=F64)) * sc
    return r16(x)


@pytest.mark.parametrize("T,C", [(771, 384), (771, 768), (771, 1024)])
def test_layernorm_emulation_and_one_pass_variance(T, C):
    x = ln_inputs(T, C, seed=T + C)
    y64, mu, s = ln64(x)
    slack = ln_slack(y64, x, mu, s)
    rep = check_one_rounding(r16(ln_emul(x)), y64, slack, "LayerNorm mode 2")
    assert abs(rep[2]) <= 0.02
    with pytest.raises(AssertionError):
        check_one_rounding(r16(ln_emul(x, mutate="one_pass")), y64, slack, "one-pass variance")
    # final norm: fp32 output inside its derived bound; the class row in the output is far outside
    g = torch.Generator().manual_seed(C)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    B = 3
    N = T // B
    xb = x[:B * N]
    y64f, bound = final_norm64(xb, gamma, beta)
    keep = lambda t: t.view(B, N, C)[:, 1:].reshape(-1, C)
    got = final_norm_emul(xb, gamma, beta, B).to(F64)
    ratio = ((got - keep(y64f)).abs() / keep(bound)).max().item()
    print(f"[vf-host] final norm {T}x{C}: max |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    bad = final_norm_emul(xb, gamma, beta, B, mutate="cls_included").to(F64)
    assert ((bad - keep(y64f)).abs() / keep(bound)).max().item() > 1.0


HEAD_CASES = {                       # latent [B, D, Hl, Wl], feature grid, C, projection
    "proj-same-grid": ((2, 32, 16, 16), (16, 16), 384, True),
    "down-D16": ((2, 16, 32, 32), (16, 16), 384, True),
    "up-nonsquare": ((2, 32, 8, 12), (16, 16), 384, True),
    "no-projection": ((2, 32, 16, 16), (16, 16), 32, False),
}


def head_inputs(name, seed=11):
    (B, D, Hl, Wl), (h, w), C, proj = HEAD_CASES[name]
    g = torch.Generator().manual_seed(seed + D + Hl)
    lat = torch.randn(B, D, Hl, Wl, generator=g)
    feats = torch.randn(B, C, h, w, generator=g) * 1.7
    weight = torch.randn(C, D, generator=g) / math.sqrt(D) if proj else None
    bias = torch.randn(C, generator=g) * 0.1 if proj else None
    return lat, feats, weight, bias


def check_head(got, want, what):
    """row X: value within 1e-6 relative, gradients within 1e-5 rel-L2 -> the measured figures"""
    v, dlat, dw, db = got
    v64, dlat64, dw64, db64 = want
    out = {"value": abs(float(v) - float(v64)) / abs(float(v64)), "dlat": rel_l2(dlat, dlat64)}
    if dw64 is not None:
        out["dw"], out["db"] = rel_l2(dw, dw64), rel_l2(db, db64)
    print(f"[vf-head] {what}: {out}")
    assert out["value"] <= HEAD_VALUE_RTOL, (what, out)
    assert all(out[k] <= HEAD_GRAD_RTOL for k in out if k != "value"), (what, out)
    return out


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_emulation_and_mutations(name):
    lat, feats, weight, bias = head_inputs(name)
    want = head64(lat, feats, weight, bias)
    assert float(want[0]) > 0.2                                   # random inputs: |cos| small, the gate open
    check_head(head_emul(lat, feats, weight, bias), want, name)
    with pytest.raises(AssertionError):
        check_head(head_emul(lat, feats, weight, bias, mutate="mean_over_channels"), want, "mean over channels")
    # gate shut: features = the projected latent (similarity 1) -> value and every gradient exactly 0; a gate left open is caught
    (B, D, Hl, Wl), (h, w), C, proj = HEAD_CASES[name]
    z = F.interpolate(lat, size=(h, w), mode="bilinear", align_corners=False)
    same = F.linear(z.flatten(2).transpose(1, 2), weight, bias).transpose(1, 2).reshape(B, C, h, w) if proj else z
    shut = head_emul(lat, same, weight, bias)
    assert float(shut[0]) == 0.0 and all(float(t.abs().max()) == 0.0 for t in shut[1:] if t is not None)
    want0 = head64(lat, same, weight, bias)
    assert float(want0[0]) == 0.0 and float(want0[1].abs().max()) == 0.0
    opened = head_emul(lat, same, weight, bias, mutate="gate_open")
    assert float(opened[1].abs().max()) > 0.0                      # (what "exactly 0" rejects)


# ---------------------------------------------------------------------------------------------------------------------
# TransVAELoss host logic and the public surface
# ---------------------------------------------------------------------------------------------------------------------
def test_public_surface():
    import transvae
    assert transvae.VFLoss is not None and transvae.DinoV2Features is not None
    assert "VFLoss" in transvae.__all__ and "DinoV2Features" in transvae.__all__
    vf = transvae.VFLoss(32, 384)
    assert sorted(vf.state_dict()) == ["proj.bias", "proj.weight"] and vf.proj.weight.shape == (384, 32)
    assert transvae.VFLoss(32, 32).proj is None and vf.temperature == 0.07 and vf.margin == 0.4


def test_transvae_loss_host_logic():
    import inspect
    import torch.nn as nn
    from transvae import TransVAELoss, VFLoss
    assert "vf_loss" in inspect.signature(TransVAELoss.__init__).parameters
    x = torch.zeros(1, 3, 16, 16)
    mu = torch.zeros(1, 4, 1, 1)
    for kw in ({}, {"vf_loss": VFLoss(4, 384)}):
        loss = TransVAELoss(lpips_weight=0.0, vf_weight=0.1, **kw)
        with pytest.raises(ValueError, match="VF"):
            loss(x, x, mu, mu, dinov2=nn.Identity())
    loss = TransVAELoss(lpips_weight=0.0, vf_weight=0.1, vf_loss=VFLoss(4, 384))
    assert "vf_loss.proj.weight" in dict(loss.named_parameters())
    # without dinov2 (and with vf_weight 0) nothing of the VF term is touched: the call reaches the fused L1 + KL pass, which has no CPU path
    for l2 in (loss, TransVAELoss(lpips_weight=0.0, vf_weight=0.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            l2(x, x, mu, mu, dinov2=None if l2 is loss else nn.Identity())
