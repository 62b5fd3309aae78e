"""Reconstruction metrics on the MI355X (`-m gpu`): transvae.metrics against the float64 restatement of
tests/test_metrics_host.py, reproducibility, and transvae.evaluate on the micro model.

Tolerances per image: |d ssim| <= 1e-4, |d psnr| <= 1e-3 dB, mse to 2e-5 relative (the kernel stages fp32 and sums in
fp32 within a tile, fp64 across tiles).
"""
import numpy as np
import pytest
import torch

from test_metrics_host import reference_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(64, 3, 256, 256), (4, 3, 512, 512), (2, 3, 1024, 1024), (1, 3, 37, 53), (1, 3, 7, 7)]
COMBOS = [(w, t) for w in ("skimage", "box11") for t in ("clip", "sigmoid", "none")]


def make_pair(shape, kind, seed):
    """target in [0, 1]; recon = target + error (smooth: low-frequency images and error; noisy: white noise), spilling
    outside [0, 1] so that the clip transform has work to do."""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    if kind == "smooth":
        lo = torch.rand(B, C, max(2, H // 32), max(2, W // 32), generator=g)
        target = torch.nn.functional.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
        err = torch.nn.functional.interpolate(torch.randn(B, C, max(2, H // 16), max(2, W // 16), generator=g), size=(H, W),
                                              mode="bilinear", align_corners=False)
        recon = target + 0.05 * err
    else:
        target = torch.rand(shape, generator=g)
        recon = target + 0.2 * torch.randn(shape, generator=g)
    return recon.float(), target.float()


def check(out, ref, label):
    mse, psnr, ssim = (out[k].double().cpu().numpy() for k in ("mse", "psnr", "ssim"))
    assert np.all(np.abs(ssim - ref["ssim"]) <= 1e-4), (label, np.abs(ssim - ref["ssim"]).max())
    assert np.all(np.abs(psnr - ref["psnr"]) <= 1e-3), (label, np.abs(psnr - ref["psnr"]).max())
    np.testing.assert_allclose(mse, ref["mse"], rtol=2e-5, atol=0, err_msg=label)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["smooth", "noisy"])
def test_matches_float64_restatement(shape, kind):
    from transvae.metrics import reconstruction_metrics
    recon, target = make_pair(shape, kind, seed=2 * SHAPES.index(shape) + (kind == "noisy"))
    r_dev, t_dev = recon.to(DEV), target.to(DEV)
    for window, transform in COMBOS:
        x = recon * 2.0 if transform == "sigmoid" else recon   # logits of a sigmoid head
        out = reconstruction_metrics(x.to(DEV) if transform == "sigmoid" else r_dev, t_dev, ssim_window=window, transform=transform)
        assert all(v.shape == (shape[0],) and v.dtype == torch.float32 and v.is_cuda for v in out.values())
        check(out, reference_metrics(x.numpy(), target.numpy(), window, transform), f"{window}/{transform}")


def test_clip_sees_values_outside_unit_range():
    from transvae.metrics import reconstruction_metrics
    recon, target = make_pair((2, 3, 64, 96), "noisy", seed=5)
    recon, target = recon * 1.6 - 0.3, target * 1.4 - 0.2
    assert recon.min() < 0 and recon.max() > 1 and target.min() < 0 and target.max() > 1
    for window in ("skimage", "box11"):
        out = reconstruction_metrics(recon.to(DEV), target.to(DEV), ssim_window=window, transform="clip")
        check(out, reference_metrics(recon.numpy(), target.numpy(), window, "clip"), window)
        raw = reference_metrics(recon.numpy(), target.numpy(), window, "none")
        assert np.all(np.abs(out["mse"].cpu().numpy() - raw["mse"]) > 1e-3)   # the clamp took effect


def test_strided_inputs_read_in_place():
    """channels_last and a non-contiguous NCHW view give the contiguous result; fp16 inputs are cast."""
    from transvae.metrics import reconstruction_metrics
    recon, target = make_pair((3, 3, 80, 144), "smooth", seed=7)
    base = {w: reconstruction_metrics(recon.to(DEV), target.to(DEV), ssim_window=w) for w in ("skimage", "box11")}
    cl_r = recon.to(DEV).contiguous(memory_format=torch.channels_last)
    cl_t = target.to(DEV).contiguous(memory_format=torch.channels_last)
    assert not cl_r.is_contiguous()
    wide = torch.zeros(3, 3, 80, 160, device=DEV)
    wide[..., :144] = target.to(DEV)
    view = wide[..., :144]
    for w in ("skimage", "box11"):
        for r, t in ((cl_r, cl_t), (recon.to(DEV), view), (cl_r, target.to(DEV))):
            out = reconstruction_metrics(r, t, ssim_window=w)
            for k in ("mse", "psnr", "ssim"):
                assert torch.equal(out[k], base[w][k]), (w, k)
        check(reconstruction_metrics(cl_r.half(), cl_t.half(), ssim_window=w),
              reference_metrics(recon.half().numpy(), target.half().numpy(), w, "clip"), "fp16")


def test_identical_images():
    from transvae.metrics import psnr, reconstruction_metrics, ssim
    recon, _ = make_pair((4, 3, 40, 72), "smooth", seed=9)
    x = recon.to(DEV)
    for w in ("skimage", "box11"):
        for t in ("clip", "none"):
            out = reconstruction_metrics(x, x.clone(), ssim_window=w, transform=t)
            assert torch.all(out["mse"] == 0)
            assert torch.all(torch.isinf(out["psnr"]) & (out["psnr"] > 0))
            assert torch.all((out["ssim"] - 1).abs() <= 1e-6), out["ssim"]
    assert torch.all(torch.isinf(psnr(x, x)))
    assert torch.all((ssim(x, x) - 1).abs() <= 1e-6)


def test_batch_independent_and_reproducible():
    from transvae.metrics import reconstruction_metrics
    recon, target = make_pair((64, 3, 256, 256), "noisy", seed=11)
    r, t = recon.to(DEV), target.to(DEV)
    for w in ("skimage", "box11"):
        a = reconstruction_metrics(r, t, ssim_window=w)
        b = reconstruction_metrics(r, t, ssim_window=w)
        for k in a:
            assert torch.equal(a[k], b[k]), (w, k)
        for i in (0, 17, 63):
            one = reconstruction_metrics(r[i:i + 1], t[i:i + 1], ssim_window=w)
            for k in a:
                assert torch.equal(one[k], a[k][i:i + 1]), (w, k, i)


def test_evaluate_on_micro_model():
    from oracle import filler
    from oracle import transvae_oracle as O
    from transvae import TransVAE, evaluate
    from transvae.metrics import reconstruction_metrics
    cfg = dict(O.MICRO)
    m = TransVAE(config=cfg, variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4)))
    m = m.to(DEV)
    g = torch.Generator().manual_seed(3)
    batches = [(torch.rand(n, 3, 64, 64, generator=g), torch.zeros(n)) for n in (2, 3, 2)]
    names = ("psnr", "ssim", "mse")

    torch.manual_seed(1234)
    res = evaluate(m, batches, metrics=names, device=DEV, per_image=True)
    assert not m.training

    torch.manual_seed(1234)
    want = {k: [] for k in names}
    with torch.no_grad():
        for images, _ in batches:
            out = reconstruction_metrics(m(images.to(DEV))[0], images.to(DEV))
            for k in names:
                want[k].append(out[k])
    for k in names:
        v = torch.cat(want[k]).cpu().numpy().astype(np.float64)
        assert np.array_equal(res[k]["values"], v), k
        assert res[k]["mean"] == np.mean(v) and res[k]["std"] == np.std(v) and res[k]["median"] == np.median(v), k
    assert set(evaluate(m, batches[:1], device=DEV)) == {"psnr", "ssim"}
