"""Reconstruction metrics, host side: a float64 NumPy restatement of both SSIM definitions and both PSNR forms, checked
against the library filters they are built from, and argument validation of transvae.metrics / transvae.evaluate.

The restatement is the yardstick of tests/test_metrics_gpu.py.

  skimage (R/evaluate.py:105-124: `peak_signal_noise_ratio(data_range=1)`, `structural_similarity(data_range=1,
  channel_axis=2)` on images clipped to [0, 1]).  skimage.metrics.structural_similarity with its defaults
  (win_size=7, gaussian_weights=False, use_sample_covariance=True, K1=0.01, K2=0.03):
      ux, uy, uxx, uyy, uxy = uniform_filter(X, 7), ... (scipy.ndimage, mode 'reflect' = d c b a | a b c d)
      cov_norm = 49 / 48;  vx = cov_norm (uxx - ux^2), vy = ..., vxy = cov_norm (uxy - ux uy)
      S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = (K1 R)^2, C2 = (K2 R)^2
      mssim = mean of S cropped by (7 - 1) // 2 = 3 px on each side; with channel_axis: the mean over channels of that
  peak_signal_noise_ratio: 10 log10(R^2 / mean((x - y)^2)).
  box11 (P/evaluate_transvae.py:47-77, on sigmoid(recon) vs images, P/...:131): F.avg_pool2d(k=11, stride=1, padding=5)
  (zero border, count_include_pad: always / 121), population variance, S.mean() over the whole [1, C, H, W] map;
  calculate_psnr: 20 log10(R / sqrt(F.mse_loss)).
"""
import numpy as np
import pytest
import torch

K1, K2 = 0.01, 0.03


def box_filter(a, k, mode):
    """Direct k x k window mean over the last two axes of a float64 array (each window a sum of k row sums of k terms, no
    running sums); mode 'reflect' (scipy) or 'zero' (avg_pool2d: zero border, / k^2 everywhere)."""
    h = k // 2
    pad = [(0, 0)] * (a.ndim - 2) + [(h, h), (h, h)]
    p = np.pad(a, pad, mode="symmetric" if mode == "reflect" else "constant")
    H, W = a.shape[-2:]
    rows = np.zeros(p.shape[:-1] + (W,))
    for dx in range(k):
        rows += p[..., dx:dx + W]
    s = np.zeros(a.shape)
    for dy in range(k):
        s += rows[..., dy:dy + H, :]
    return s / (k * k)


def transform_pair(recon, target, transform):
    x, y = np.asarray(recon, np.float64), np.asarray(target, np.float64)
    if transform == "clip":
        return np.clip(x, 0, 1), np.clip(y, 0, 1)
    if transform == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x)), y
    assert transform == "none"
    return x, y


def ssim_map_mean(x, y, window, R):
    """[..., H, W] -> [...] mean SSIM of each plane."""
    k, mode, cov = (7, "reflect", 49 / 48) if window == "skimage" else (11, "zero", 1.0)
    ux, uy = box_filter(x, k, mode), box_filter(y, k, mode)
    uxx, uyy, uxy = box_filter(x * x, k, mode), box_filter(y * y, k, mode), box_filter(x * y, k, mode)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    if window == "skimage":
        p = (k - 1) // 2
        S = S[..., p:-p, p:-p]
    return S.mean(axis=(-2, -1))


def reference_metrics(recon, target, window="skimage", transform="clip", R=1.0):
    """[B, C, H, W] arrays -> dict of [B] float64 arrays: mse, psnr (skimage form), psnr_p (P's form), ssim."""
    x, y = transform_pair(recon, target, transform)
    B = x.shape[0]
    mse = ((x - y) ** 2).reshape(B, -1).mean(1)
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(R * R / mse)
        psnr_p = np.where(mse == 0, np.inf, 20 * np.log10(R / np.sqrt(np.maximum(mse, 1e-300))))
    ssim = ssim_map_mean(x, y, window, R).mean(axis=1)   # per channel, then over channels (skimage channel_axis)
    return {"mse": mse, "psnr": psnr, "psnr_p": psnr_p, "ssim": ssim}


def test_reflect_filter_is_scipy_uniform_filter():
    nd = pytest.importorskip("scipy.ndimage")
    a = np.random.default_rng(0).standard_normal((13, 29))
    for k in (7, 11):
        np.testing.assert_allclose(box_filter(a, k, "reflect"), nd.uniform_filter(a, size=k, mode="reflect"), rtol=0, atol=1e-13)


def test_box11_filter_is_avg_pool2d():
    a = np.random.default_rng(1).random((23, 17))
    ref = torch.nn.functional.avg_pool2d(torch.from_numpy(a)[None, None], 11, stride=1, padding=5)[0, 0].numpy()
    np.testing.assert_allclose(box_filter(a, 11, "zero"), ref, rtol=0, atol=1e-13)


def test_box11_ssim_is_the_patched_torch_formula():
    """P/evaluate_transvae.py:56-77 written out in torch (float64) on one [1, C, H, W] image: its whole-map mean equals the
    restatement's mean of per-channel means."""
    F = torch.nn.functional
    rng = np.random.default_rng(2)
    x, y = rng.random((1, 3, 20, 24)), rng.random((1, 3, 20, 24))
    a, b = torch.from_numpy(x), torch.from_numpy(y)
    mu1, mu2 = F.avg_pool2d(a, 11, 1, 5), F.avg_pool2d(b, 11, 1, 5)
    s1 = F.avg_pool2d(a * a, 11, 1, 5) - mu1 ** 2
    s2 = F.avg_pool2d(b * b, 11, 1, 5) - mu2 ** 2
    s12 = F.avg_pool2d(a * b, 11, 1, 5) - mu1 * mu2
    m = ((2 * mu1 * mu2 + K1 ** 2) * (2 * s12 + K2 ** 2)) / ((mu1 ** 2 + mu2 ** 2 + K1 ** 2) * (s1 + s2 + K2 ** 2))
    ref = reference_metrics(x, y, window="box11", transform="none")
    assert abs(float(m.mean()) - ref["ssim"][0]) < 1e-12
    assert abs(float(F.mse_loss(a, b)) - ref["mse"][0]) < 1e-15


def test_psnr_forms_agree_and_identical_images():
    rng = np.random.default_rng(3)
    x = rng.random((2, 3, 9, 11))
    y = np.clip(x + 0.05 * rng.standard_normal(x.shape), 0, 1)
    r = reference_metrics(x, y, transform="none")
    np.testing.assert_allclose(r["psnr"], r["psnr_p"], rtol=1e-12)
    r = reference_metrics(x, x, transform="none")
    assert np.all(r["mse"] == 0) and np.all(np.isinf(r["psnr"])) and np.all(np.isinf(r["psnr_p"]))
    np.testing.assert_allclose(r["ssim"], 1.0, atol=1e-12)


def test_skimage_window_rejects_small_images():
    from transvae.metrics import reconstruction_metrics
    for shape in ((1, 3, 6, 32), (1, 3, 32, 6)):
        with pytest.raises(ValueError, match="H, W >= 7"):
            reconstruction_metrics(torch.zeros(shape), torch.zeros(shape))


def test_unknown_window_and_transform():
    from transvae.metrics import reconstruction_metrics
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="ssim_window"):
        reconstruction_metrics(x, x, ssim_window="gaussian")
    with pytest.raises(ValueError, match="transform"):
        reconstruction_metrics(x, x, transform="tanh")
    with pytest.raises(ValueError, match="shape"):
        reconstruction_metrics(x, x[:, :2])


def test_cpu_tensors_raise():
    from transvae.metrics import psnr, reconstruction_metrics, ssim
    x = torch.rand(2, 3, 16, 16)
    for fn in (reconstruction_metrics, psnr, ssim):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x)


def test_evaluate_rejects_lpips_and_unknown_metrics():
    from transvae import evaluate
    with pytest.raises(ValueError, match="LPIPS term needs the external VGG network"):
        evaluate(torch.nn.Identity(), [], metrics=("psnr", "lpips"))
    with pytest.raises(ValueError, match="unknown metrics"):
        evaluate(torch.nn.Identity(), [], metrics=("psnr", "fid"))


def test_public_names():
    import transvae
    assert {"reconstruction_metrics", "evaluate", "TransVAE", "create_transvae", "TransVAELoss"} <= set(transvae.__all__)
    assert callable(transvae.reconstruction_metrics) and callable(transvae.evaluate)
