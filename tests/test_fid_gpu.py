"""rFID on the GPU: every new kernel against fp64 of the same bf16 inputs under the rounding contract (references in
tests/test_fid_host.py, checks from tests/test_error_budget_host.py), the added convolution modes under row [G], the streaming
moments against NumPy in fp64 and bit-identical across batch splits, the whole Inception-v3 against the plain-torch restatement
(tests/fid_restatement.py) within max(1e-2, 1.25 x the restatement's own bf16-autocast deviation), the rFID floor of the bf16
path against the same yardstick, and evaluate(..., "rfid").

Every test prints its measured figure before it asserts; DESIGN.md section 3.1 is where the MI355X figures are recorded."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_restatement as FR
import test_fid_host as H
from oracle import filler
from oracle import transvae_oracle as O
from test_error_budget_host import F64, check_fp32, check_one_rounding, epilogue64, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _L():
    from transvae.hip import _lib as L
    return L


@pytest.fixture(scope="module")
def net():
    from transvae import InceptionFeatures
    return InceptionFeatures().load_fid_state_dict(FR.plain_state_dict()).to(DEV)


@pytest.fixture(scope="module")
def golden():
    with open(FR.GOLDEN) as f:
        return json.load(f)


def _acts(shape, seed):
    """bf16 activations like a ReLU layer's output: half of them zero, the rest |N(0, 1)|"""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(shape, generator=g)).to(BF)


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 35, 35, 288), (3, 17, 19, 96)], ids=["35x35x288", "17x19x96"])
def test_pool3x3(shape):
    from transvae import metrics_fid as MF
    L = _L()
    x = (_acts(shape, 1) - 0.25).to(BF)            # signed values: the padded maximum must ignore the border, not read zeros
    xd = x.to(DEV)
    for mode, name in ((L.POOL3_MAX_S2, "max_s2"), (L.POOL3_MAX_S1P1, "max_s1p1")):
        y = MF.pool3x3(xd, mode).cpu()
        ref, _ = H.pool64(x, name)
        assert tuple(y.shape) == tuple(ref.shape)
        assert torch.equal(y.to(F64), ref), name
    y = MF.pool3x3(xd, L.POOL3_AVG_S1P1).cpu()
    ref, refabs = H.pool64(x, "avg_s1p1")
    r = check_one_rounding(y, ref, 2.0 ** -20 * refabs, "avg pool 3x3")       # fp32 sum of <= 9 terms and a division
    print("avg pool ratio/ulps/bias", r)
    # into a column range of a wider tensor: the other columns stay untouched
    wide = torch.full(shape[:3] + (shape[3] + 64,), 7.0, dtype=BF, device=DEV)
    MF.pool3x3(xd, L.POOL3_MAX_S1P1, wide, 32)
    assert torch.equal(wide[..., 32:32 + shape[3]].cpu().to(F64), H.pool64(x, "max_s1p1")[0])
    assert bool((wide[..., :32] == 7).all()) and bool((wide[..., 32 + shape[3]:] == 7).all())


@pytest.mark.parametrize("taps", [3, 7])
@pytest.mark.parametrize("axis", [0, 1])
def test_gather_line(taps, axis):
    from transvae import metrics_fid as MF
    x = _acts((2, 17, 13, 160), taps + axis) + 1
    y = MF.gather_line(x.to(DEV), taps, axis).cpu()
    assert torch.equal(y, H.gather_line_ref(x, taps, axis))


@pytest.mark.parametrize("B,Hh,W", [(2, 256, 256), (3, 64, 96), (1, 512, 384)], ids=["256", "64x96-up", "512x384-down"])
def test_fid_prep(B, Hh, W):
    from transvae import metrics_fid as MF
    g = torch.Generator().manual_seed(Hh + W)
    x = torch.rand(B, 3, Hh, W, generator=g)
    cols = MF.fid_prep(x[:1].to(DEV), x[1:].to(DEV) if B > 1 else None).cpu()
    assert tuple(cols.shape) == (B, 149, 149, 32) and cols[..., 27:].abs().max() == 0
    ref = H.fid_prep64(x)
    # fp32 interpolation: the two weights are exact fractions rounded once (2^-24 relative), three fused lerps and the 2x - 1
    # map round once each on values in [0, 1] / [-1, 1]: below 8 roundings of 2^-24 -> 2^-21; stated as 2^-20
    r = check_one_rounding(cols[..., :27], ref, 2.0 ** -20, f"fid_prep {Hh}x{W}")
    print("fid_prep ratio/ulps/bias", r)
    # clip: pixels outside [0, 1] are clamped before the resize
    z = (x[:1] * 1.5 - 0.25)
    c1 = MF.fid_prep(z.to(DEV), None, clip=True).cpu()
    c2 = MF.fid_prep(z.clamp(0, 1).to(DEV), None).cpu()
    assert torch.equal(c1, c2)


def test_fid_prep_clip_passes_a_nan_on():
    """torch.clamp propagates a NaN: under clip a NaN pixel is NaN in exactly the patch columns where the restatement
    (`clamp(0, 1)`, then the same resize) has NaN, and every other element keeps its bits"""
    from transvae import metrics_fid as MF
    g = torch.Generator().manual_seed(41)
    z = torch.rand(2, 3, 64, 96, generator=g) * 1.5 - 0.25
    clean = MF.fid_prep(z[:1].to(DEV), z[1:].to(DEV), clip=True).cpu()
    bad = z.clone()
    bad[1, 1, 30, 50] = float("nan")
    got = MF.fid_prep(bad[:1].to(DEV), bad[1:].to(DEV), clip=True).cpu()
    want = torch.zeros(got.shape, dtype=torch.bool)
    want[..., :27] = H.fid_prep64(bad.clamp(0, 1)).isnan()
    assert 0 < int(want.sum()) and not bool(want[0].any())
    assert torch.equal(got.isnan(), want)
    assert torch.equal(got.view(torch.int16)[~want], clean.view(torch.int16)[~want])


def test_global_avgpool():
    from transvae import metrics_fid as MF
    x = _acts((5, 8, 8, 2048), 3)
    y = MF.global_avgpool(x.to(DEV)).cpu()
    x64 = x.to(F64).view(5, 64, 2048)
    r = check_fp32(y, x64.mean(1), x64.abs().sum(1) / 64, 1, "global average pool")     # fp32 accumulation slack 2^-24 sum |x| (of the mean)
    print("global avgpool ratio", r)
    x2 = _acts((2, 5, 7, 96), 4)
    assert rel_l2(MF.global_avgpool(x2.to(DEV)).cpu(), x2.to(F64).view(2, 35, 96).mean(1)) < 1e-7


@pytest.mark.parametrize("mode,Hh,W,Cin,Cout", [("c3v1", 21, 19, 32, 64), ("c3v2", 35, 35, 288, 384), ("c3v2", 18, 21, 96, 96),
                                                  ("c5s1", 35, 35, 64, 64), ("c1", 17, 19, 768, 192)])
def test_added_conv_modes_forward(mode, Hh, W, Cin, Cout):
    """Row [G] for the forward-only modes, stored into a column range of a wider tensor as the Inception blocks do."""
    from transvae import metrics_fid as MF
    L = _L()
    g = torch.Generator().manual_seed(Hh * W + Cin)
    k = {"c3v1": 3, "c3v2": 3, "c5s1": 5, "c1": 1}[mode]
    x = torch.randn(2, Hh, W, Cin, generator=g).to(BF)
    w = (torch.randn(Cout, k, k, Cin, generator=g) / math.sqrt(k * k * Cin)).to(BF)
    bias = torch.randn(Cout, generator=g) * 0.1
    acc, absdot = H.conv64_mode(x, w, mode)
    z = acc + bias.to(F64)
    y64 = torch.relu(z)
    slack = 2.0 ** -20 * absdot + 2.0 ** -24 * bias.to(F64).abs()                 # ReLU: Lipschitz 1, exact
    out = MF.conv_relu(x.to(DEV), w.to(DEV), bias.to(DEV), mode)
    assert tuple(out.shape) == tuple(y64.shape)
    r = check_one_rounding(out.cpu(), y64, slack, f"{mode} forward [G]")
    print(mode, "ratio/ulps/bias", r)
    wide = torch.full(tuple(y64.shape[:3]) + (Cout + 96,), 3.0, dtype=BF, device=DEV)
    MF.conv_relu(x.to(DEV), w.to(DEV), bias.to(DEV), mode, wide, 64)
    assert torch.equal(wide[..., 64:64 + Cout], out) and bool((wide[..., :64] == 3).all()) and bool((wide[..., 64 + Cout:] == 3).all())
    # forward only
    from transvae.hip import ops
    with pytest.raises(ValueError):
        ops.conv_dgrad(ops._Geo(mode, x.to(DEV), w.to(DEV)), w.float().to(DEV), out, x.shape)


@pytest.mark.parametrize("taps,axis,C,Cout", [(7, 1, 160, 160), (7, 0, 128, 192), (3, 0, 384, 384)])
def test_line_conv_against_fp64(taps, axis, C, Cout):
    from transvae import metrics_fid as MF
    g = torch.Generator().manual_seed(taps * C + axis)
    x = torch.randn(2, 17, 17, C, generator=g).to(BF)
    kh, kw = (taps, 1) if axis == 0 else (1, taps)
    w = (torch.randn(Cout, kh, kw, C, generator=g) / math.sqrt(taps * C)).to(BF)
    bias = torch.randn(Cout, generator=g) * 0.1
    xn, wn = x.to(F64).permute(0, 3, 1, 2), w.to(F64).permute(0, 3, 1, 2)
    pad = (taps // 2, 0) if axis == 0 else (0, taps // 2)
    acc = F.conv2d(xn, wn, padding=pad).permute(0, 2, 3, 1)
    absdot = F.conv2d(xn.abs(), wn.abs(), padding=pad).permute(0, 2, 3, 1)
    y64 = torch.relu(acc + bias.to(F64))
    out = MF.line_conv_relu(x.to(DEV), w.reshape(Cout, taps * C).to(DEV), bias.to(DEV), taps, axis)
    check_one_rounding(out.cpu(), y64, 2.0 ** -20 * absdot + 2.0 ** -24 * bias.to(F64).abs(), f"{kh}x{kw} line convolution [G]")


# ---------------------------------------------------------------------------------------------------------------------------
# streaming moments
# ---------------------------------------------------------------------------------------------------------------------------
def _feed(fd, side, x, splits):
    i = 0
    k = 0
    while i < x.shape[0]:
        b = splits[k % len(splits)]
        fd.update(*((x[i:i + b], None) if side == 0 else (None, x[i:i + b])))
        i += b
        k += 1


def test_fid_accumulate_matches_numpy_and_is_split_invariant():
    from transvae import FrechetDistance
    g = torch.Generator().manual_seed(11)
    n, d = 4096, 2048
    std = 0.5 + torch.rand(d, generator=g)
    mean = 3.0 * std * (2 * torch.rand(d, generator=g) - 1)       # |mean| up to 3 standard deviations
    mix = torch.randn(d, 64, generator=g) * 0.2
    x = (torch.randn(n, d, generator=g) + torch.randn(n, 64, generator=g) @ mix.t()) * std + mean
    xd = x.to(DEV)
    fd = FrechetDistance()
    _feed(fd, 0, xd, (1, 7, 64, 100, 33, 128))
    _feed(fd, 1, xd, (256, 3, 1000))
    assert fd.n == (n, n)
    cnt, mu, cov = fd.statistics(0)
    x64 = x.numpy().astype(np.float64)
    mu_ref, cov_ref = x64.mean(0), np.cov(x64, rowvar=False)
    e_mu = np.linalg.norm(mu - mu_ref) / np.linalg.norm(mu_ref)
    e_cov = np.linalg.norm(cov - cov_ref) / np.linalg.norm(cov_ref)
    print("accumulate: mean rel", e_mu, "cov rel Frobenius", e_cov)
    assert e_mu <= 1e-10 and e_cov <= 1e-10
    assert torch.equal(fd.state(0), fd.state(1)), "the state depends on the batch split"
    assert np.array_equal(cov, cov.T)
    assert abs(fd.compute()) <= 1e-9 * np.trace(cov_ref)
    # a strided view (a feature subspace) reads the same rows
    fs = FrechetDistance(dims=256)
    fs.update(xd[:300], xd[:300, :256].contiguous())
    assert torch.equal(fs.state(0), fs.state(1))


# ---------------------------------------------------------------------------------------------------------------------------
# the whole network
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.case_key)
def test_network_against_restatement(net, golden, shape):
    x = FR.case_inputs(shape)
    ref = FR.run(x, FR.plain_state_dict())
    got = net(x.to(DEV))
    assert tuple(got.shape) == (shape[0], 2048) and got.dtype == torch.float32
    err = rel_l2(got.cpu(), ref)
    dev16 = golden["cases"][FR.case_key(shape)]["features"]
    print(f"network {FR.case_key(shape)}: rel-L2 {err:.4g}, restatement's own autocast deviation {dev16:.4g}, ratio {err / dev16:.3f}")
    assert err <= max(1e-2, 1.25 * dev16), (err, dev16)
    # an image's features do not depend on the batch around it
    xd = x.to(DEV)
    alone = net(xd[1:2])
    both = net.features(xd, xd.flip(0))                       # a batch of 2B
    assert torch.equal(alone[0], got[1]) and torch.equal(both[1], got[1]) and torch.equal(both[shape[0]], got[shape[0] - 1])


def test_rfid_floor_of_the_bf16_path(net, golden):
    """The Frechet distance (first 256 feature dimensions, n = 512 > d) between the HIP features and the restatement's fp32
    features of the SAME images, against the same quantity for the restatement's own bf16-autocast features."""
    from transvae import FrechetDistance
    fl = golden["floor"]
    ref = torch.from_numpy(np.load(FR.GOLDEN_FLOOR)["features"])
    assert tuple(ref.shape) == (FR.FLOOR_N, FR.FLOOR_DIMS) == (fl["n"], fl["dims"])
    x = FR.floor_images()
    feats = torch.cat([net(x[i:i + 128].to(DEV)) for i in range(0, FR.FLOOR_N, 128)])
    fd = FrechetDistance(dims=FR.FLOOR_DIMS)
    fd.update(ref.to(DEV), feats)
    val = fd.compute()
    check = FR.frechet_numpy(ref.numpy(), feats[:, :FR.FLOOR_DIMS].cpu().numpy())
    yard = fl["frechet_autocast_vs_fp32"]
    print(f"rFID floor of the bf16 path: HIP {val:.6g} (numpy {check:.6g}), restatement autocast {yard:.6g}, ratio {val / yard:.3f}; "
          f"trace of the fp32 covariance {fl['trace_cov_fp32']:.6g}; feature rel-L2 {rel_l2(feats[:, :FR.FLOOR_DIMS].cpu(), ref):.4g}")
    assert abs(val - check) <= 1e-8 * max(1.0, fl["trace_cov_fp32"])
    assert val <= 1.25 * yard, (val, yard)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluate()
# ---------------------------------------------------------------------------------------------------------------------------
class _Identity(torch.nn.Module):
    def forward(self, x):
        return (x,)


def test_evaluate_rfid(net):
    from transvae import FrechetDistance, TransVAE, evaluate
    m = TransVAE(config=dict(O.MICRO), variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(O.MICRO, latent_dim=4)))
    m = m.to(DEV)
    imgs = FR.smooth_images(6, 64, 64, 77)
    loader = [(imgs[:4], None), (imgs[4:], None)]
    torch.manual_seed(5)
    out = evaluate(m, loader, metrics=("psnr", "rfid"), device=DEV, fid_net=net, per_image=True)
    assert list(out) == ["psnr", "rfid"] and set(out["rfid"]) == {"value", "n"} and out["rfid"]["n"] == 6
    torch.manual_seed(5)
    base = evaluate(m, loader, metrics=("psnr",), device=DEV, per_image=True)
    assert np.array_equal(base["psnr"]["values"], out["psnr"]["values"]) and base["psnr"]["mean"] == out["psnr"]["mean"]
    # the hand loop
    torch.manual_seed(5)
    fd = FrechetDistance()
    m.eval()
    with torch.no_grad():
        for b, _ in loader:
            b = b.to(DEV)
            r = m(b)[0]
            f = net.features(b.clamp(0, 1), r.float().clamp(0, 1))
            fd.update(f[:b.shape[0]], f[b.shape[0]:])
    assert out["rfid"]["value"] == fd.compute()
    assert math.isfinite(out["rfid"]["value"]) and out["rfid"]["value"] > 0
    ident = evaluate(_Identity(), loader, metrics=("rfid",), device=DEV, fid_net=net)
    print("rFID micro model", out["rfid"]["value"], "identity", ident["rfid"]["value"])
    assert abs(ident["rfid"]["value"]) <= 1e-6 and ident["rfid"]["n"] == 6
