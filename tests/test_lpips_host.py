"""LPIPS (VGG-16) perceptual term, host side: the plain-torch restatement is sane, and PerceptualLoss / its loader / the
TransVAELoss and evaluate() plumbing behave as specified without a GPU (tests/lpips_restatement.py holds the yardstick)."""
import os
import re

import pytest
import torch

import lpips_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plain_sd():
    return R.plain_state_dict()


def test_restatement_is_sane(plain_sd):
    g = torch.Generator().manual_seed(1)
    x, t = torch.rand(2, 3, 32, 48, generator=g), torch.rand(2, 3, 32, 48, generator=g)
    # no tap is all zero for the chosen seed (thirteen He-scaled ReLU layers keep O(1) activations)
    for k, f in enumerate(R.features(2 * x - 1, plain_sd)):
        assert float(f.abs().max()) > 1e-2 and float((f > 0).float().mean()) > 0.05, (k, float(f.abs().max()))
        assert float(f.std()) < 50.0
    d = R.lpips(x, t, plain_sd, normalize=True)
    assert d.shape == (2, 1, 1, 1) and bool((d > 0).all())
    assert torch.equal(R.lpips(x, x, plain_sd, normalize=True), torch.zeros(2, 1, 1, 1))
    assert torch.equal(d, R.lpips(2 * x - 1, 2 * t - 1, plain_sd))
    for i in range(5):
        assert bool((plain_sd[f"lin{i}"] >= 0).all())


def test_perceptual_loss_builds_without_gpu_and_has_no_parameters():
    from transvae import PerceptualLoss
    net = PerceptualLoss()
    assert list(net.parameters()) == []
    names = dict(net.named_buffers())
    assert tuple(names["conv1_1_weight"].shape) == (64, 3, 3, 3) and tuple(names["conv5_3_weight"].shape) == (512, 512, 3, 3)
    assert tuple(names["lin3"].shape) == (512,)
    assert torch.allclose(names["shift_scale"], torch.tensor(R.SHIFT + R.SCALE))
    # the packed operands are derived, not state
    assert not any(k.startswith("_op") for k in net.state_dict())
    assert len(net.state_dict()) == 13 * 2 + 5 + 1


def test_loader_maps_both_key_schemes_onto_the_same_buffers(plain_sd):
    from transvae import PerceptualLoss
    a = PerceptualLoss().load_lpips_state_dict(plain_sd)
    b = PerceptualLoss().load_lpips_state_dict(R.lpips_package_state_dict(plain_sd))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(sa["conv3_2_weight"], plain_sd["conv3_2.weight"]) and torch.equal(sa["lin4"], plain_sd["lin4"])
    # packed operands: [O, ky, kx, I] forward, [I, 2-ky, 2-kx, O] for the data gradient, conv1_1 as a K = 32 GEMM
    w = plain_sd["conv2_1.weight"]
    assert torch.equal(a._op_conv2_1.float(), w.permute(0, 2, 3, 1).to(torch.bfloat16).float())
    assert torch.equal(a._opt_conv2_1[5, 0, 2, 7].float(), w[7, 5, 2, 0].to(torch.bfloat16).float())
    assert tuple(a._op_conv1_1.shape) == (64, 32) and tuple(a._opt_conv1_1.shape) == (32, 64)
    assert float(a._op_conv1_1[:, 27:].abs().max()) == 0.0
    assert torch.equal(a._op_conv1_1[3, (1 * 3 + 2) * 3 + 1].float(), plain_sd["conv1_1.weight"][3, 1, 1, 2].to(torch.bfloat16).float())
    # a state-dict round trip re-derives the operands
    c = PerceptualLoss()
    c.load_state_dict(sa)
    assert torch.equal(c._opt_conv4_2, a._opt_conv4_2)


def test_loader_lists_missing_and_unexpected_keys(plain_sd):
    from transvae import PerceptualLoss
    sd = dict(plain_sd)
    del sd["conv4_2.bias"], sd["lin2"]
    sd["net.slice9.99.weight"] = torch.zeros(1)
    sd["classifier.weight"] = torch.zeros(1)
    with pytest.raises(KeyError) as e:
        PerceptualLoss().load_lpips_state_dict(sd)
    msg = str(e.value)
    for k in ("conv4_2.bias", "lin2", "net.slice9.99.weight", "classifier.weight"):
        assert k in msg, k
    bad = dict(plain_sd)
    bad["conv1_2.weight"] = torch.zeros(64, 3, 3, 3)
    with pytest.raises(KeyError, match="conv1_2.weight"):
        PerceptualLoss().load_lpips_state_dict(bad)


def test_from_file(tmp_path, plain_sd):
    from transvae import PerceptualLoss
    p = str(tmp_path / "lpips_vgg.pth")
    torch.save(R.lpips_package_state_dict(plain_sd), p)
    net = PerceptualLoss.from_file(p)
    assert torch.equal(net.conv5_1_bias, plain_sd["conv5_1.bias"])


def test_validation():
    from transvae import PerceptualLoss
    net = PerceptualLoss()
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(ValueError, match="multiples of 16"):
        net(torch.zeros(1, 3, 24, 32), torch.zeros(1, 3, 24, 32))
    with pytest.raises(ValueError, match="one shape"):
        net(x, torch.zeros(1, 3, 32, 48))
    with pytest.raises(ValueError, match="one shape"):
        net(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError, match="`input` only"):
        net(x, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x, x)


def test_loss_and_evaluate_take_an_lpips_net():
    from transvae import PerceptualLoss, TransVAELoss, evaluate
    net = PerceptualLoss()
    loss = TransVAELoss(lpips_weight=1.0, lpips_net=net)
    assert loss.lpips_net is net and list(loss.parameters()) == []
    assert TransVAELoss(lpips_weight=0.0, lpips_net=net).lpips_net is None
    with pytest.raises(ValueError, match="LPIPS"):
        TransVAELoss()
    with pytest.raises(ValueError, match="LPIPS"):
        TransVAELoss(lpips_weight=0.5)
    # an empty loader: the argument is accepted and every metric is reported
    with pytest.warns(RuntimeWarning):
        out = evaluate(torch.nn.Identity(), [], metrics=("psnr", "ssim", "lpips"), device="cpu", lpips_net=net)
    assert set(out) == {"psnr", "ssim", "lpips"}
    with pytest.raises(ValueError, match="LPIPS term needs the external VGG network"):
        evaluate(torch.nn.Identity(), [], metrics=("lpips",))


def test_new_symbols_are_declared_and_bound():
    from transvae.hip import _lib
    hdr = open(os.path.join(ROOT, "include", "transvae_hip.h")).read()
    dev = open(os.path.join(ROOT, "deepl-project_amd", "csrc", "common.h")).read()
    for name in ("tv_maxpool2x2_fwd", "tv_maxpool2x2_bwd", "tv_lpips_prep", "tv_lpips_prep_bwd", "tv_lpips_head",
                 "tv_lpips_head_partial_count"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", hdr), name
    # the ReLU id: one name, one number, in the header, the kernels and the binding -- and outside the pinned TV_ACT_ family
    ids = [int(re.search(r"#define\s+TV_ACTX_RELU\s+(\d+)", s).group(1)) for s in (hdr, dev)]
    assert ids == [_lib.ACTX_RELU, _lib.ACTX_RELU]
    assert _lib.ACTX_RELU not in (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_SILU, _lib.ACT_DERIV, _lib.ACT_ADD) and _lib.ACTX_RELU < _lib.ACT_SAVE_DERIV
    flags = {k: int(v) for k, v in re.findall(r"#define\s+(TV_LPIPS_[A-Z]+)\s+(\d+)", hdr)}
    assert flags == {"TV_LPIPS_MAP": _lib.LPIPS_MAP, "TV_LPIPS_SIGMOID": _lib.LPIPS_SIGMOID, "TV_LPIPS_CLAMP": _lib.LPIPS_CLAMP}


def test_golden_covers_every_whole_loss_case():
    import json
    with open(R.GOLDEN) as f:
        cases = json.load(f)["cases"]
    for shape in R.SHAPES:
        for pair in R.PAIRS:
            c = cases[R.case_key(shape, pair)]
            assert 0 < c["value"] < 0.5 and 0 < c["grad"] < 0.5 and len(c["values_fp32"]) == shape[0]
