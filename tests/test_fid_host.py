"""rFID, host side: weight loading of `InceptionFeatures` under both key schemes, the Frechet distance of `FrechetDistance` on
host-supplied statistics against closed forms (and scipy's sqrtm form where scipy imports), the restatement's sanity, the
argument checks of `evaluate`, and the fp64 references the GPU test (tests/test_fid_gpu.py) holds the new kernels to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_restatement as FR

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references of the kernels (inputs: the bf16 / fp32 values the kernel consumes)
# ---------------------------------------------------------------------------------------------------------------------------
def pool64(x, mode):
    """x NHWC -> fp64 NHWC of the three tv_pool3x3 forms; the average also returns mean |x| over the in-bounds taps"""
    xn = x.to(F64).permute(0, 3, 1, 2)
    if mode == "max_s2":
        return F.max_pool2d(xn, 3, stride=2).permute(0, 2, 3, 1), None
    if mode == "max_s1p1":
        return F.max_pool2d(xn, 3, stride=1, padding=1).permute(0, 2, 3, 1), None
    y = F.avg_pool2d(xn, 3, stride=1, padding=1, count_include_pad=False).permute(0, 2, 3, 1)
    ya = F.avg_pool2d(xn.abs(), 3, stride=1, padding=1, count_include_pad=False).permute(0, 2, 3, 1)
    return y, ya


def gather_line_ref(x, taps, axis):
    """[B, H, W, C] -> [B * H * W, taps * C] by pad + unfold"""
    B, H, W, C = x.shape
    h = taps // 2
    pad = (0, 0, 0, 0, h, h) if axis == 0 else (0, 0, h, h)
    xp = F.pad(x, pad)
    u = xp.unfold(1 if axis == 0 else 2, taps, 1)            # [B, H, W, C, taps]
    return u.permute(0, 1, 2, 4, 3).reshape(B * H * W, taps * C)


def fid_prep64(x):
    """fp32 NCHW in [0, 1] -> ([B, 149, 149, 27] fp64 patch rows of 2 * resize(x) - 1 in (ky, kx, c) order)"""
    r = 2 * F.interpolate(x.to(F64), size=(299, 299), mode="bilinear", align_corners=False) - 1
    p = F.unfold(r, 3, stride=2)                                 # [B, 3 * 9, 149 * 149], rows (c, ky, kx)
    B = x.shape[0]
    return p.view(B, 3, 9, 149, 149).permute(0, 3, 4, 2, 1).reshape(B, 149, 149, 27)


def conv64_mode(x, w, mode):
    """exact conv of NHWC x and [Cout, KH, KW, Cin] w for the forward-only modes -> (y64 NHWC, sum |x w| NHWC)"""
    stride, pad = {"c3v1": (1, 0), "c3v2": (2, 0), "c5s1": (1, 2), "c1": (1, 0)}[mode]
    xn, wn = x.to(F64).permute(0, 3, 1, 2), w.to(F64).permute(0, 3, 1, 2)
    return (F.conv2d(xn, wn, stride=stride, padding=pad).permute(0, 2, 3, 1),
            F.conv2d(xn.abs(), wn.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1))


def test_references_agree_with_direct_definitions():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 6, 8, generator=g)
    r = gather_line_ref(x, 3, 1).view(2, 5, 6, 3, 8)
    assert torch.equal(r[:, :, 1:5, 0], x[:, :, 0:4]) and torch.equal(r[:, :, :, 1], x) and r[:, :, 0, 0].abs().max() == 0
    r = gather_line_ref(x, 7, 0).view(2, 5, 6, 7, 8)
    assert torch.equal(r[:, 3:, :, 0], x[:, :2]) and torch.equal(r[:, :, :, 3], x) and r[:, 0, :, :3].abs().max() == 0
    y, ya = pool64(x, "avg_s1p1")
    assert abs(float(y[0, 0, 0, 0]) - float(x[0, :2, :2, 0].double().mean())) < 1e-15
    img = torch.rand(1, 3, 20, 30, generator=g)
    p = fid_prep64(img)
    res = 2 * F.interpolate(img.double(), size=(299, 299), mode="bilinear", align_corners=False) - 1
    assert float((p[0, 5, 7, 4 * 3 + 1] - res[0, 1, 11, 15]).abs()) == 0      # tap (1, 1) of patch (5, 7), channel 1


# ---------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_sd():
    return FR.plain_state_dict()


def test_layer_table_matches_the_restatement():
    from transvae.metrics_fid import FID_LAYERS, plain_keys
    assert len(FID_LAYERS) == 94 == len(FR.LAYERS)
    for a, b in zip(FID_LAYERS, FR.LAYERS):
        pad = b[6] if isinstance(b[6], tuple) else (b[6], b[6])
        assert a[:6] == b[:6] and a[6:] == pad, (a, b)
    assert len(plain_keys()) == 94 * 5


def test_both_key_schemes_load_to_identical_packed_weights(plain_sd):
    from transvae import InceptionFeatures
    from transvae.metrics_fid import FID_LAYERS
    a = InceptionFeatures().load_fid_state_dict(plain_sd)
    b = InceptionFeatures().load_fid_state_dict(FR.pt_inception_state_dict(plain_sd))
    for l in FID_LAYERS:
        (wa, ba), (wb, bb) = a.packed(l[0]), b.packed(l[0])
        assert wa.dtype == torch.bfloat16 and ba.dtype == torch.float32
        assert torch.equal(wa, wb) and torch.equal(ba, bb), l[0]
        assert wa.shape[0] % 32 == 0 and wa.shape[-1] % 32 == 0
    # BatchNorm folded: operand = w * gamma / sqrt(var + eps) in the kernels' [O, kh, kw, I] order, bias = beta - mean * scale
    n = "Mixed_6b.branch7x7_2"
    s = plain_sd[f"{n}.gamma"] / torch.sqrt(plain_sd[f"{n}.var"] + 1e-3)
    w, bias = a.packed(n)
    ref = (plain_sd[f"{n}.weight"] * s.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(128, 7 * 128).to(torch.bfloat16)
    assert torch.equal(w, ref)
    assert torch.allclose(bias, plain_sd[f"{n}.beta"] - plain_sd[f"{n}.mean"] * s, rtol=1e-6, atol=1e-7)
    # padded widths: 80 -> 96 output rows and input columns of zeros
    w3b, b3b = a.packed("Conv2d_3b_1x1")
    w4a, _ = a.packed("Conv2d_4a_3x3")
    assert tuple(w3b.shape) == (96, 1, 1, 64) and w3b[80:].abs().max() == 0 and b3b[80:].abs().max() == 0
    assert tuple(w4a.shape) == (192, 3, 3, 96) and w4a[..., 80:].abs().max() == 0
    assert tuple(a.packed("Conv2d_1a_3x3")[0].shape) == (32, 32)


def test_missing_or_misshaped_keys_raise_and_name_the_key(plain_sd):
    from transvae import InceptionFeatures
    sd = dict(plain_sd)
    del sd["Mixed_7c.branch3x3dbl_3b.var"]
    with pytest.raises(KeyError, match="Mixed_7c.branch3x3dbl_3b.var"):
        InceptionFeatures().load_fid_state_dict(sd)
    sd = FR.pt_inception_state_dict(plain_sd)
    del sd["Mixed_5b.branch1x1.conv.weight"]
    with pytest.raises(KeyError, match="Mixed_5b.branch1x1.weight"):
        InceptionFeatures().load_fid_state_dict(sd)
    sd = dict(plain_sd)
    sd["Conv2d_2a_3x3.weight"] = torch.zeros(32, 32, 1, 1)
    with pytest.raises(KeyError, match=r"Conv2d_2a_3x3.weight \(32, 32, 1, 1\)"):
        InceptionFeatures().load_fid_state_dict(sd)
    sd = dict(plain_sd)
    sd["Mixed_9z.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="Mixed_9z.weight"):
        InceptionFeatures().load_fid_state_dict(sd)


def test_from_file_round_trip(plain_sd, tmp_path):
    from transvae import InceptionFeatures
    p = tmp_path / "pt_inception.pth"
    torch.save(FR.pt_inception_state_dict(plain_sd), str(p))
    m = InceptionFeatures.from_file(str(p))
    assert torch.equal(m.packed("Mixed_7a.branch3x3_2")[0], InceptionFeatures().load_fid_state_dict(plain_sd).packed("Mixed_7a.branch3x3_2")[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 3, 32, 32))


def test_restatement_features_are_finite_and_not_degenerate(plain_sd):
    x = FR.smooth_images(2, 64, 64, 5)
    f = FR.run(x, plain_sd)
    assert tuple(f.shape) == (2, 2048) and torch.isfinite(f).all()
    assert 1e-3 < float(f.abs().mean()) < 1e3 and float((f > 0).float().mean()) > 0.5
    assert float((f[0] - f[1]).abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# Frechet distance on host-supplied statistics
# ---------------------------------------------------------------------------------------------------------------------------
def _spd(d, seed, rank=None):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((d, rank or 2 * d))
    return a @ a.T / a.shape[1]


def test_frechet_identical_statistics_give_zero():
    from transvae.metrics_fid import frechet_from_statistics
    for d, rank in ((64, None), (2048, None), (256, 40)):
        s = _spd(d, d, rank)
        mu = np.random.default_rng(1).standard_normal(d)
        v = frechet_from_statistics(mu, s, mu, s)
        print(d, rank, v)
        assert abs(v) <= 1e-9, (d, rank, v)


def test_frechet_commuting_covariances_closed_form():
    from transvae.metrics_fid import frechet_from_statistics
    rng = np.random.default_rng(3)
    d = 300
    a, b = rng.uniform(0.1, 4.0, d), rng.uniform(0.1, 4.0, d)
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    ref = ((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    v = frechet_from_statistics(mu1, np.diag(a), mu2, np.diag(b))
    assert abs(v - ref) <= 1e-10 * ref, (v, ref)
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]           # the same in a rotated basis
    v = frechet_from_statistics(q @ mu1, q @ np.diag(a) @ q.T, q @ mu2, q @ np.diag(b) @ q.T)
    assert abs(v - ref) <= 1e-10 * ref, (v, ref)


@pytest.mark.parametrize("d", [64, 2048])
def test_frechet_equals_the_sqrtm_form(d):
    linalg = pytest.importorskip("scipy.linalg")
    from transvae.metrics_fid import frechet_from_statistics
    s1, s2 = _spd(d, 10 + d), _spd(d, 20 + d)
    rng = np.random.default_rng(d)
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    covmean = linalg.sqrtm(s1 @ s2)
    ref = ((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean.real)
    v = frechet_from_statistics(mu1, s1, mu2, s2)
    assert abs(v - ref) <= 1e-8 * abs(ref), (v, ref)


def test_frechet_needs_two_samples():
    from transvae import FrechetDistance
    with pytest.raises(ValueError, match="at least 2"):
        FrechetDistance().compute()
    with pytest.raises(ValueError, match="multiple of 64"):
        FrechetDistance(dims=100)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluate()
# ---------------------------------------------------------------------------------------------------------------------------
def test_evaluate_argument_checks():
    from transvae import evaluate
    m = torch.nn.Identity()
    with pytest.raises(ValueError, match="fid_net"):
        evaluate(m, [], metrics=("psnr", "rfid"))
    with pytest.raises(ValueError, match="unknown metrics"):
        evaluate(m, [], metrics=("psnr", "fid"))
    with pytest.raises(ValueError, match="unknown metrics"):
        evaluate(m, [], metrics=("fid",), fid_net=torch.nn.Identity())
