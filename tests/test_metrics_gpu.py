"""Reconstruction metrics on the MI355X (`-m gpu`): transvae.metrics against the float64 restatement of
tests/test_metrics_host.py, reproducibility, and transvae.evaluate on the micro model.

Tolerances per image of the first tests: |d ssim| <= 1e-4, |d psnr| <= 1e-3 dB, mse to 2e-5 relative (the kernel stages fp32
and sums in fp32 within a tile, fp64 across tiles).  The rounding-contract tests below hold the kernel to
the bound derived from its order of operations instead (`metrics_bound` of tests/test_metrics_host.py, computed in fp64 from
the inputs, validated there against an fp32 emulation and against mutations): tile geometry, more than 256 tiles, value
patterns that lean on the per-tile pivot, data ranges, strides, non-finite inputs and the batch limit.
"""
import numpy as np
import pytest
import torch

from test_metrics_host import (ALL_TRANSFORMS, EDGE_SHAPES, MANY_TILES_SHAPE, VALUE_CASES, bound_ratios, logits_of, metrics_bound,
                               noisy_pair, reference_metrics, report, value_case)

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


# ---------------------------------------------------------------------------------------------------------------------------
# rounding contract
# ---------------------------------------------------------------------------------------------------------------------------
def run_np(recon, target, window, transform, R=1.0):
    from transvae.metrics import reconstruction_metrics
    out = reconstruction_metrics(torch.from_numpy(recon).to(DEV), torch.from_numpy(target).to(DEV), ssim_window=window,
                                 transform=transform, data_range=R)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_bound(recon, target, window, transform, R, label):
    ref, bound = metrics_bound(recon, target, window, transform, R)
    out = run_np(recon, target, window, transform, R)
    rat = bound_ratios(out, ref, bound)
    report(f"metrics {label} {window}/{transform} ratio", {k: round(v, 4) for k, v in rat.items()})
    assert all(v <= 1.0 for v in rat.values()), (label, window, transform, rat)
    return out, ref, bound


@pytest.mark.parametrize("window,shape", [(w, s) for w in ("skimage", "box11") for s in EDGE_SHAPES[w]],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_tile_edges_inside_bound(window, shape):
    recon, target = noisy_pair((2, 2) + shape, seed=200 + EDGE_SHAPES[window].index(shape))
    for transform in ALL_TRANSFORMS:
        check_bound(logits_of(recon, transform), target, window, transform, 1.0, "x".join(map(str, shape)))


@pytest.mark.parametrize("window", ["skimage", "box11"])
@pytest.mark.parametrize("transform", ALL_TRANSFORMS)
def test_many_tiles_inside_bound(window, transform):
    """306 / 342 tiles: the finalise kernel's strided loop takes a second pass"""
    recon, target = noisy_pair(MANY_TILES_SHAPE, seed=300)
    check_bound(logits_of(recon, transform), target, window, transform, 1.0, "2113x1025")


@pytest.mark.parametrize("window", ["skimage", "box11"])
@pytest.mark.parametrize("name", VALUE_CASES)
def test_values_inside_bound(name, window):
    """For the pivot cases (the tile-centre pixel an outlier, a step edge through it) the absolute SSIM error is printed too:
    a CPU emulation puts it near 2.5e-5 when the outlier is the pivot of a flat tile."""
    recon, target, transforms, R = value_case(name, window)
    for transform in transforms:
        out, ref, bound = check_bound(recon, target, window, transform, R, name)
        if name in ("outlier_in_0", "outlier_in_1", "step"):
            report(f"metrics {name} {window}/{transform} |d ssim|, bound",
                   (float(np.abs(out["ssim"] - ref["ssim"]).max()), float(bound["ssim"].max())))
        if name == "const_identical":
            assert out["mse"][0] == 0 and np.isposinf(out["psnr"][0])


def test_expanded_target_equals_materialised():
    """a target broadcast over the batch (stride 0) is read in place and gives the bits of its materialised copy"""
    from transvae.metrics import reconstruction_metrics
    recon, target = noisy_pair((3, 2, 70, 134), seed=31)
    r = torch.from_numpy(recon).to(DEV)
    t = torch.from_numpy(target[:1]).to(DEV).expand(3, -1, -1, -1)
    assert t.stride(0) == 0
    for w in ("skimage", "box11"):
        a = reconstruction_metrics(r, t, ssim_window=w)
        b = reconstruction_metrics(r, t.contiguous(), ssim_window=w)
        for k in a:
            assert torch.equal(a[k], b[k]), (w, k)
    one = torch.from_numpy(recon[:1, :1]).to(DEV).expand(3, 2, -1, -1)       # both inputs, batch and channel stride 0
    a = reconstruction_metrics(one, t, ssim_window="skimage")
    b = reconstruction_metrics(one.contiguous(), t.contiguous(), ssim_window="skimage")
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _pattern(v):
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 2.0, np.where(np.isinf(v), np.sign(v), 0.0))


@pytest.mark.parametrize("window", ["skimage", "box11"])
def test_non_finite_inputs(window):
    """One NaN pixel in image 1 of 3 (interior, then row 0): that image's three values follow the fp64 restatement's NaN / inf
    pattern (np.clip and the sigmoid pass a NaN on), the other images keep their bits.  +inf under `none` likewise."""
    recon, target = noisy_pair((3, 2, 70, 134), seed=32)
    cases = [(t, pos, np.nan) for t in ALL_TRANSFORMS for pos in ((33, 70), (0, 70))] + [("none", (33, 70), np.inf)]
    for transform, (py, px), bad in cases:
        x = logits_of(recon, transform)
        clean = run_np(x, target, window, transform)
        x = x.copy()
        x[1, 1, py, px] = bad
        out = run_np(x, target, window, transform)
        with np.errstate(all="ignore"):
            ref = reference_metrics(x, target, window, transform)
        for k in ("mse", "psnr", "ssim"):
            assert _pattern(out[k][1]) == _pattern(ref[k][1]) != 0, (transform, py, bad, k, out[k][1], ref[k][1])
            assert np.array_equal(out[k][[0, 2]], clean[k][[0, 2]]), (transform, py, bad, k)


def test_batch_limit_raises_and_launches_nothing():
    """B C = 65 538 planes exceed the grid's y dimension: the argument error, and neither buffer is written"""
    import ctypes as C
    from transvae.hip import _lib as L, ops
    from transvae.metrics import reconstruction_metrics
    B, Cn = 21846, 3
    x = torch.zeros(B, Cn, 7, 7, device=DEV)
    with pytest.raises(RuntimeError, match="B \\* C > 65535"):
        reconstruction_metrics(x, x)
    lib = L.load()
    partials = torch.full((lib.tv_recon_metrics_partial_count(B, Cn, 7, 7, L.SSIM_SKIMAGE),), -7.25, device=DEV)
    out = torch.full((3, B), -7.25, device=DEV)
    rc = lib.tv_recon_metrics(ops._p(x), ops._p(x), *x.stride(), *x.stride(), B, Cn, 7, 7, L.SSIM_SKIMAGE, L.METRIC_CLIP,
                              C.c_float(1.0), ops._p(partials), ops._p(out), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == -7.25).all()) and bool((partials == -7.25).all())


def test_evaluate_reports_nan_for_a_diverged_image():
    """evaluate() with its default clip transform: a NaN in one reconstruction gives NaN for that image's PSNR and SSIM and
    leaves every other image's values bit-unchanged"""
    from transvae import evaluate

    class Recon(torch.nn.Module):
        def __init__(self, poison):
            super().__init__()
            self.poison = poison

        def forward(self, x):
            r = x * 0.9 + 0.03
            if self.poison:
                r[1, 2, 11, 40] = float("nan")
            return (r,)

    g = torch.Generator().manual_seed(5)
    batches = [(torch.rand(3, 3, 32, 48, generator=g), torch.zeros(3))]
    good = evaluate(Recon(False), batches, metrics=("psnr", "ssim"), device=DEV, per_image=True)
    bad = evaluate(Recon(True), batches, metrics=("psnr", "ssim"), device=DEV, per_image=True)
    for k in ("psnr", "ssim"):
        assert np.isnan(bad[k]["values"][1]) and np.isnan(bad[k]["mean"]), k
        assert np.isfinite(good[k]["values"]).all()
        assert np.array_equal(bad[k]["values"][[0, 2]], good[k]["values"][[0, 2]]), k
