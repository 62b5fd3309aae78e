"""Reconstruction metrics, host side: a float64 NumPy restatement of both SSIM definitions and both PSNR forms, checked
against the library filters they are built from, and argument validation of transvae.metrics / transvae.evaluate.

The restatement is the yardstick of tests/test_metrics_gpu.py.  The second half of the file is the kernel's row of the rounding
contract: an fp32 emulation of csrc/metrics.hip, the derived bound, the shared cases and the mutations.

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


# ---------------------------------------------------------------------------------------------------------------------------
# Rounding contract of `tv_recon_metrics`: an fp32 emulation of csrc/metrics.hip in the kernel's order
# of operations, the bound derived from that order, the case list shared with tests/test_metrics_gpu.py, and mutation tests.
# The bound is a function of the inputs alone (fp64); it was written from the kernel's source and is never fitted to an output.
# ---------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
TW = 128
THREADS = 256
GEOM = {"skimage": dict(K=7, TH=64, reflect=True, cov=49.0 / 48.0, lo=3),
        "box11": dict(K=11, TH=56, reflect=False, cov=1.0, lo=0)}
SIGMOID_U = 4          # fp32 sigmoid: expf at 1 ulp (2 u), the rounding of 1 + e, the division
CONST_U = 6            # C1, C2 = (k R)(k R) in fp32: k rounded, two products, twice, one more product: within 6 u
F32 = np.float32


def _gamma(n):
    return n * U / (1.0 - n * U)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64 (the fp64 sum is rounded again, which can differ from a true
    fma in a half-ulp tie only)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _transform32(v, transform, is_recon):
    v = np.asarray(v, F32)
    if transform == "clip":
        return np.clip(v, F32(0), F32(1))          # propagates a NaN, as the kernel's compare-and-select does
    if transform == "sigmoid" and is_recon:
        with np.errstate(over="ignore"):
            return (F32(1) / (F32(1) + np.exp(-v))).astype(F32)
    return v


def _reflect_index(i, n, border):
    """met_reflect: scipy 'reflect' (d c b a | a b c d) for one overhang, clamped into the image ('mirror': d c b | a b c d)"""
    if border == "reflect":
        j = np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    else:
        j = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return np.clip(j, 0, n - 1)


def _butterfly(v):
    """tv_wave_sum on [..., 64]: v += shfl_xor(v, o) for o = 32 .. 1; every lane ends with the same sum"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(v.dtype)
    return v[..., 0]


def _block_sum(per_thread):
    """[P, 256] per-thread fp32 values -> [P]: wave butterflies, then the four wave sums in wave order"""
    w = _butterfly(per_thread.reshape(per_thread.shape[0], THREADS // 64, 64))
    acc = np.zeros(per_thread.shape[0], F32)
    for k in range(THREADS // 64):
        acc = (acc + w[:, k]).astype(F32)
    return acc


def emulate_metrics(recon, target, window="skimage", transform="clip", R=1.0, *, contract=True, pivot="centre", cov=None,
                    border="reflect", crop=True, box_div="window", pad_after_transform=False, scale_c=True, mse_ragged=False,
                    finalize_limit=None):
    """csrc/metrics.hip on the CPU: fp32 wherever the kernel is fp32, in its order: staging about the tile's pivot, the
    horizontal K-term sums (adds for the first moments, fma chains for the second), the K-row ring summed in slot order, the
    product by 1 / K^2, the covariance normalisation, the map, the per-thread row chain, the wave butterfly, four waves, and fp64
    across tiles.  `contract`: the compiler's fma contraction of `v2 - mx mx`, `2 ux uy + c1`, `ux ux + uy uy + c1` (either form
    is the kernel's; the bound covers both).  The remaining keywords are the mutations of the tests below; their defaults
    are the kernel.  [B, C, H, W] -> dict of [B] float32 arrays."""
    g = GEOM[window]
    K, TH, refl, lo = g["K"], g["TH"], g["reflect"], (g["lo"] if crop else 0)
    covn = F32(g["cov"] if cov is None else cov)
    h, NR, NC, ROWS = K // 2, TH + K - 1, TW + K - 1, TH // 2
    x = np.asarray(recon, F32)
    B, C, H, W = x.shape
    x = x.reshape(B * C, H, W)
    y = np.asarray(target, F32).reshape(B * C, H, W)
    P = B * C
    with np.errstate(all="ignore"):
        tx, ty = _transform32(x, transform, True), _transform32(y, transform, False)
        pad_x = _transform32(np.zeros((), F32), transform, True) if pad_after_transform else F32(0)
        pad_y = _transform32(np.zeros((), F32), transform, False) if pad_after_transform else F32(0)
        Rf = F32(R) if scale_c else F32(1)
        c1 = (F32(0.01) * Rf) * (F32(0.01) * Rf)
        c2 = (F32(0.03) * Rf) * (F32(0.03) * Rf)
        inv_np = F32(1.0 / (K * K))
        NE = NR * NC
        NL = -(-NE // THREADS)
        tiles_y, tiles_x = -(-H // TH), -(-W // TW)
        part_s, part_q = [], []
        for tile in range(tiles_y * tiles_x):
            ty0, tx0 = (tile // tiles_x) * TH, (tile % tiles_x) * TW
            r, c = ty0 - h + np.arange(NR), tx0 - h + np.arange(NC)
            in_r, in_c = (r >= 0) & (r < H), (c >= 0) & (c < W)
            inside = in_r[:, None] & in_c[None, :]
            if refl:
                gr, gc = _reflect_index(r, H, border), _reflect_index(c, W, border)
                X, Y = tx[:, gr][:, :, gc], ty[:, gr][:, :, gc]
            else:
                gr, gc = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
                X = np.where(inside, tx[:, gr][:, :, gc], pad_x)
                Y = np.where(inside, ty[:, gr][:, :, gc], pad_y)
            pr, pc = min(ty0 + TH // 2, H - 1), min(tx0 + TW // 2, W - 1)
            px, py = tx[:, pr, pc][:, None, None], ty[:, pr, pc][:, None, None]
            if pivot == "none":
                px, py = np.zeros_like(px), np.zeros_like(py)

            # sum (x - y)^2: element e = tid + 256 k of the staged block, an fma chain over k
            lr, lc = np.arange(NR), np.arange(NC)
            own = ((lr >= h) & (lr < h + TH))[:, None] & ((lc >= h) & (lc < h + TW))[None, :]
            if not mse_ragged:
                own = own & (r < H)[:, None] & (c < W)[None, :]
            d = np.zeros((P, NL * THREADS), F32)
            d[:, :NE] = (X - Y).reshape(P, NE)
            o = np.zeros(NL * THREADS, bool)
            o[:NE] = own.reshape(NE)
            d, o = d.reshape(P, NL, THREADS), o.reshape(NL, THREADS)
            sq = np.zeros((P, THREADS), F32)
            for k in range(NL):
                sq = np.where(o[k], _fma32(d[:, k], d[:, k], sq), sq)
            part_q.append(_block_sum(sq))

            sx, sy = (X - px).astype(F32), (Y - py).astype(F32)
            rx, ry = (X, Y) if pivot == "raw_second" else (sx, sy)     # operands of the second moments
            m = [np.zeros((P, NR, TW), F32) for _ in range(5)]
            for j in range(K):
                a, b = sx[:, :, j:j + TW], sy[:, :, j:j + TW]
                a2, b2 = rx[:, :, j:j + TW], ry[:, :, j:j + TW]
                m[0] = (m[0] + a).astype(F32)
                m[1] = (m[1] + b).astype(F32)
                m[2] = _fma32(a2, a2, m[2])
                m[3] = _fma32(b2, b2, m[3])
                m[4] = _fma32(a2, b2, m[4])
            S = np.zeros((P, TH, TW), F32)
            for half in range(2):
                row0 = half * ROWS
                i = np.arange(ROWS) + K - 1                       # LDS row (relative to row0) that completes the window
                v = []
                for mm in m:
                    s = np.zeros((P, ROWS, TW), F32)
                    for q in range(K):                            # ring slot q holds the row with index = q (mod K)
                        s = (s + mm[:, row0 + i - ((i - q) % K)]).astype(F32)
                    v.append(s)
                if box_div == "count":                            # mutation: divide by the number of in-bounds taps
                    rows = ty0 + row0 + np.arange(ROWS)
                    cols = tx0 + np.arange(TW)
                    nr = np.minimum(rows + h, H - 1) - np.maximum(rows - h, 0) + 1
                    nc = np.minimum(cols + h, W - 1) - np.maximum(cols - h, 0) + 1
                    cnt = np.maximum(nr[:, None] * nc[None, :], 1).astype(F32)
                    v = [(s / cnt).astype(F32) for s in v]
                else:
                    v = [(s * inv_np).astype(F32) for s in v]
                mx, my = v[0], v[1]
                ux, uy = (mx + px).astype(F32), (my + py).astype(F32)
                ex, ey = (ux, uy) if pivot == "raw_second" else (mx, my)   # the mean that the second moments are about
                if contract:
                    vx, vy = covn * _fma32(-ex, ex, v[2]), covn * _fma32(-ey, ey, v[3])
                    vxy = covn * _fma32(-ex, ey, v[4])
                    a1 = _fma32(F32(2) * ux, uy, c1)
                    b1 = _fma32(ux, ux, uy * uy) + c1
                else:
                    vx, vy = covn * (v[2] - ex * ex), covn * (v[3] - ey * ey)
                    vxy = covn * (v[4] - ex * ey)
                    a1 = F32(2) * ux * uy + c1
                    b1 = ux * ux + uy * uy + c1
                num = a1 * (F32(2) * vxy + c2)
                den = b1 * (vx + vy + c2)
                S[:, row0:row0 + ROWS] = num / den
            rows, cols = ty0 + np.arange(TH), tx0 + np.arange(TW)
            counted = ((rows >= lo) & (rows < H - lo))[:, None] & ((cols >= lo) & (cols < W - lo))[None, :]
            S = np.where(counted, S, F32(0))                      # a select: a NaN outside the region does not leak
            acc = np.zeros((P, 2, TW), F32)                       # thread (half, col): a chain down its ROWS rows
            for half in range(2):
                for rr in range(ROWS):
                    acc[:, half] = acc[:, half] + S[:, half * ROWS + rr]
            part_s.append(_block_sum(acc.reshape(P, THREADS)))

        ps = np.stack(part_s, 1).astype(np.float64)[:, :finalize_limit]   # [P, tiles]
        pq = np.stack(part_q, 1).astype(np.float64)[:, :finalize_limit]
        count = float((H - 2 * lo) * (W - 2 * lo))
        ssim = (ps.sum(1) / count).reshape(B, C).sum(1) / C
        mse = pq.sum(1).reshape(B, C).sum(1) / float(C * H * W)
        Rd = float(F32(R))
        psnr = np.where(mse == 0, np.inf, 10.0 * np.log10(Rd * Rd / np.where(mse == 0, 1.0, mse)))
        return {"mse": mse.astype(F32), "psnr": psnr.astype(F32), "ssim": ssim.astype(F32)}


def _win_mean(a, K):
    """valid K x K window mean over the last two axes (fp64, direct sums)"""
    Hh, Ww = a.shape[-2] - K + 1, a.shape[-1] - K + 1
    rows = np.zeros(a.shape[:-1] + (Ww,))
    for j in range(K):
        rows += a[..., j:j + Ww]
    s = np.zeros(a.shape[:-2] + (Hh, Ww))
    for i in range(K):
        s += rows[..., i:i + Hh, :]
    return s / (K * K)


def metrics_bound(recon, target, window="skimage", transform="clip", R=1.0):
    """DESIGN.md §3.1 row M.  [B, C, H, W] fp32 inputs -> (ref, bound): the fp64 values {"mse", "psnr", "ssim"} and the absolute
    bound on each of the kernel's outputs, computed in fp64 from the inputs, u = 2^-24.

    MSE (all terms >= 0, so relative): d = fl(x - y) one rounding (2 u on d^2), the per-thread fma chain of at most NL =
    ceil(NR NC / 256) terms, 6 butterfly steps, 4 waves, fp64 across tiles, one final rounding: (NL + 13) u mse; with the
    sigmoid also mean(2 |d| e + e^2), e = 4 u sigmoid(x).  PSNR: (10 / ln 10) rel / (1 - rel) + u |psnr|, rel = bound(mse) / mse.

    SSIM per pixel, with a = x - px, b = y - py the values about the tile's pivots (the padded zeros of box11 are -px, -py):
      first moments   |d mx|  <= g(2K + 1) mean|a| + mean e     (the staging rounding, K - 1 and K - 1 adds, 1 / K^2 and its product)
      second moments  |d qx|  <= g(2K + 3) mean a^2 + mean(2 |a| e + e^2), |d qxy| <= g(2K + 3) mean|a b| + mean|b| e
      variances       |d vx|  <= cov (|d qx| + 2 |mx| |d mx| + u mx^2 + u |qx - mx^2|) + 2 u vx, likewise vy, vxy
      means           |d ux|  <= |d mx| + u |ux|
      A1 = 2 ux uy + C1, A2 = 2 vxy + C2, B1 = ux^2 + uy^2 + C1, B2 = vx + vy + C2 by first-order propagation plus their own
      roundings (C1, C2 within 6 u), and
      |d S| <= [(dA1 |A2| + |A1| dA2 + dA1 dA2) / (B1 B2) + |S| (rho + 3 u)] / (1 - rho),  rho = dB1 / B1 + dB2 / B2
    (A2 may be zero or negative: nothing divides by it; rho >= 1/2 gives no bound at all: inf).
    SSIM per image: the mean of |d S| over the counted region + g(ROWS + 10) (mean|S| + mean|d S|) for the per-thread chain of
    ROWS rows, the butterfly and the four waves, + u |ssim| for the final rounding.
    """
    g = GEOM[window]
    K, TH, refl, lo, covn = g["K"], g["TH"], g["reflect"], g["lo"], g["cov"]
    h, ROWS = K // 2, TH // 2
    NL = -(-(TH + K - 1) * (TW + K - 1) // THREADS)
    x32 = np.asarray(recon, F32)
    B, C, H, W = x32.shape
    R = float(F32(R))
    with np.errstate(all="ignore"):
        x, y = transform_pair(x32.astype(np.float64), np.asarray(target, F32).astype(np.float64), transform)
        e = SIGMOID_U * U * np.abs(x) + 2.0 ** -126 if transform == "sigmoid" else np.zeros_like(x)
        d = x - y
        mse = (d * d).reshape(B, -1).mean(1)
        gm = _gamma(NL + 13)
        mse_b = gm * mse + (1 + gm) * ((2 * np.abs(d) + U * np.abs(d) + e) * e).reshape(B, -1).mean(1)
        psnr = np.where(mse == 0, np.inf, 10 * np.log10(R * R / np.where(mse == 0, 1.0, mse)))
        rel = np.where(mse == 0, 0.0, mse_b / np.where(mse == 0, 1.0, mse))
        psnr_b = np.where(mse == 0, 0.0, np.where(rel < 0.5, (10 / np.log(10)) * rel / (1 - rel) + 2 * U * np.abs(psnr), np.inf))

        pad = [(0, 0), (0, 0), (h, h), (h, h)]
        mode = dict(mode="symmetric") if refl else dict(mode="constant")
        Xp, Yp, Ep = np.pad(x, pad, **mode), np.pad(y, pad, **mode), np.pad(e, pad, **mode)
        C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
        g1, g2, gs = _gamma(2 * K + 1), _gamma(2 * K + 3), _gamma(ROWS + 10)
        sum_S, sum_absS, sum_dS = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
        for ty0 in range(0, H, TH):
            for tx0 in range(0, W, TW):
                th, tw = min(TH, H - ty0), min(TW, W - tx0)
                blk = (Ellipsis, slice(ty0, ty0 + th + K - 1), slice(tx0, tx0 + tw + K - 1))
                pr, pc = min(ty0 + TH // 2, H - 1), min(tx0 + TW // 2, W - 1)
                px, py = x[:, :, pr, pc][..., None, None], y[:, :, pr, pc][..., None, None]
                a, b, ee = Xp[blk] - px, Yp[blk] - py, Ep[blk]
                mx, my = _win_mean(a, K), _win_mean(b, K)
                qx, qy, qxy = _win_mean(a * a, K), _win_mean(b * b, K), _win_mean(a * b, K)
                dmx = g1 * _win_mean(np.abs(a), K) + (1 + g1) * _win_mean(ee, K)
                dmy = g1 * _win_mean(np.abs(b), K)
                dqx = g2 * qx + (1 + g2) * _win_mean((2 * np.abs(a) + ee) * ee, K)
                dqy = g2 * qy
                dqxy = g2 * _win_mean(np.abs(a * b), K) + (1 + g2) * _win_mean(np.abs(b) * ee, K)

                def var_err(q, dq, m1, dm1, m2, dm2):
                    raw = q - m1 * m2
                    t = dq + np.abs(m1) * dm2 + np.abs(m2) * dm1 + dm1 * dm2
                    t = (t + U * (np.abs(m1) + dm1) * (np.abs(m2) + dm2)) * (1 + U) + U * np.abs(raw)
                    return covn * raw, covn * t * (1 + 3 * U) + 2 * U * covn * np.abs(raw)

                vx, dvx = var_err(qx, dqx, mx, dmx, mx, dmx)
                vy, dvy = var_err(qy, dqy, my, dmy, my, dmy)
                vxy, dvxy = var_err(qxy, dqxy, mx, dmx, my, dmy)
                ux, uy = mx + px, my + py
                dux, duy = dmx + U * (np.abs(ux) + dmx), dmy + U * (np.abs(uy) + dmy)
                A1, B1 = 2 * ux * uy + C1, ux * ux + uy * uy + C1
                A2, B2 = 2 * vxy + C2, vx + vy + C2
                dA1 = 2 * (np.abs(ux) * duy + np.abs(uy) * dux + dux * duy) + 2 * U * np.abs(2 * ux * uy) + CONST_U * U * C1 + U * np.abs(A1)
                dB1 = (2 * np.abs(ux) + dux) * dux + (2 * np.abs(uy) + duy) * duy + 3 * U * (ux * ux + uy * uy) + CONST_U * U * C1 + U * B1
                dA2 = 2 * dvxy + CONST_U * U * C2 + U * np.abs(A2)
                dB2 = dvx + dvy + U * np.abs(vx + vy) + CONST_U * U * C2 + U * B2
                S = (A1 * A2) / (B1 * B2)
                rho = dB1 / B1 + dB2 / B2
                dS = ((dA1 * np.abs(A2) + np.abs(A1) * dA2 + dA1 * dA2) / (B1 * B2) + np.abs(S) * (rho + 3 * U)) / (1 - rho)
                dS = np.where(rho < 0.5, dS * (1 + 2.0 ** -20), np.inf)
                rows, cols = ty0 + np.arange(th), tx0 + np.arange(tw)
                cnt = ((rows >= lo) & (rows < H - lo))[:, None] & ((cols >= lo) & (cols < W - lo))[None, :]
                sum_S += np.where(cnt, S, 0).sum((-2, -1))
                sum_absS += np.where(cnt, np.abs(S), 0).sum((-2, -1))
                sum_dS += np.where(cnt, dS, 0).sum((-2, -1))
        n = float((H - 2 * lo) * (W - 2 * lo))
        ssim = (sum_S / n).mean(1)
        ssim_b = ((sum_dS + gs * (sum_absS + sum_dS)) / n).mean(1) + 2 * U * np.abs(ssim)
    return {"mse": mse, "psnr": psnr, "ssim": ssim}, {"mse": mse_b, "psnr": psnr_b, "ssim": ssim_b}


def bound_ratios(out, ref, bound):
    """worst error / bound per output over the batch; a non-finite reference value must be matched exactly (ratio 0 or inf)"""
    res = {}
    for k in ("mse", "psnr", "ssim"):
        o, r, b = np.asarray(out[k], np.float64), ref[k], bound[k]
        fin = np.isfinite(r)
        same = np.where(fin, False, (o == r) | (np.isnan(o) & np.isnan(r)))
        with np.errstate(all="ignore"):
            q = np.where(fin, np.where(np.abs(o - r) == 0, 0.0, np.abs(o - r) / b), np.where(same, 0.0, np.inf))
        res[k] = float(np.max(np.where(np.isnan(q), np.inf, q)))
    return res


# --- the cases, shared with tests/test_metrics_gpu.py ----------------------------------------------------------------------
ALL_TRANSFORMS = ("clip", "sigmoid", "none")
EDGE_SHAPES = {"skimage": [(7, 129), (8, 8), (13, 13), (63, 127), (64, 128), (65, 129), (70, 134), (129, 257)],
               "box11": [(1, 1), (3, 5), (10, 10), (56, 128), (57, 129), (112, 256), (113, 257)]}
MANY_TILES_SHAPE = (1, 1, 2113, 1025)        # 34 x 9 tiles (skimage), 38 x 9 (box11): the finalise loop runs a second pass
VALUE_SHAPE = (1, 2, 70, 134)                # 2 x 2 tiles for both windows, ragged in both directions
VALUE_CASES = ("const", "const_identical", "flat_noise", "step", "outlier_in_0", "outlier_in_1", "offset64", "u8_range255",
               "pm1_range2", "logits100", "tiny_mse")


def noisy_pair(shape, seed):
    """target in [0, 1], recon = target + 0.2 N(0, 1): spills outside [0, 1], so the clip has work to do"""
    rng = np.random.default_rng(seed)
    target = rng.random(shape).astype(F32)
    return (target + 0.2 * rng.standard_normal(shape)).astype(F32), target


def logits_of(recon, transform):
    return (recon * F32(2)).astype(F32) if transform == "sigmoid" else recon     # logits of a sigmoid head


def value_case(name, window):
    """-> recon, target [1, 2, 70, 134] fp32, the transforms the case runs under, data_range"""
    rng = np.random.default_rng(100 + VALUE_CASES.index(name))
    shape = VALUE_SHAPE
    cr, cc = GEOM[window]["TH"] // 2, TW // 2              # the first tile's pivot pixel
    noise = lambda s: (s * rng.standard_normal(shape)).astype(F32)
    if name == "const":
        return np.full(shape, 0.3, F32), np.full(shape, 0.6, F32), ALL_TRANSFORMS, 1.0
    if name == "const_identical":
        return np.full(shape, 0.37, F32), np.full(shape, 0.37, F32), ("clip", "none"), 1.0
    if name == "flat_noise":
        t = (F32(0.5) + noise(1e-3)).astype(F32)
        return (t + noise(1e-3)).astype(F32), t, ALL_TRANSFORMS, 1.0
    if name == "step":
        t = np.zeros(shape, F32)
        t[..., cc:] = 1
        return (t + noise(1e-3)).astype(F32), t, ("clip", "none"), 1.0
    if name in ("outlier_in_0", "outlier_in_1"):
        flat = F32(0) if name == "outlier_in_0" else F32(1)
        t = (flat + noise(1e-3)).astype(F32)
        r = (t + noise(1e-3)).astype(F32)
        t[..., cr, cc] = r[..., cr, cc] = 1 - flat
        return r, t, ("none",), 1.0
    if name == "offset64":       # every value a multiple of 2^-10: exact in fp32; variances near 1e-4, below C2 = 9e-4
        t = (64 + rng.integers(0, 32, shape) / 1024.0).astype(F32)
        r = (t.astype(np.float64) + rng.integers(-8, 9, shape) / 1024.0).astype(F32)
        return r, t, ("none",), 1.0
    if name == "u8_range255":
        t = rng.integers(0, 256, shape).astype(F32)
        return np.clip(t + np.rint(8 * rng.standard_normal(shape)), 0, 255).astype(F32), t, ("none",), 255.0
    if name == "pm1_range2":
        t = (2 * rng.random(shape) - 1).astype(F32)
        return np.clip(t + noise(0.1), -1, 1).astype(F32), t, ("none",), 2.0
    if name == "logits100":
        t = (rng.random(shape) < 0.5).astype(F32)
        flip = rng.random(shape) < 0.05
        return np.where((t > 0) ^ flip, F32(100), F32(-100)).astype(F32), t, ("sigmoid",), 1.0
    assert name == "tiny_mse"                               # differences of an ulp or two: mse near 1e-14
    t = rng.random(shape).astype(F32)
    r = (t + noise(1e-7)).astype(F32)
    return r, t, ("clip", "none"), 1.0


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def _emulation_inside(recon, target, window, transform, R, label, contracts=(True, False)):
    ref, bound = metrics_bound(recon, target, window, transform, R)
    worst = {}
    for contract in contracts:
        out = emulate_metrics(recon, target, window, transform, R, contract=contract)
        rat = bound_ratios(out, ref, bound)
        worst = {k: max(worst.get(k, 0.0), rat[k]) for k in rat}
    report(f"metrics emulation {label} {window}/{transform}", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (label, window, transform, worst)
    return ref, bound


@pytest.mark.parametrize("window", ["skimage", "box11"])
def test_emulation_inside_bound_tile_edges(window):
    for i, (H, W) in enumerate(EDGE_SHAPES[window]):
        recon, target = noisy_pair((2, 2, H, W), seed=200 + i)
        for transform in ALL_TRANSFORMS:
            _emulation_inside(logits_of(recon, transform), target, window, transform, 1.0, f"{H}x{W}")


@pytest.mark.parametrize("window", ["skimage", "box11"])
@pytest.mark.parametrize("name", VALUE_CASES)
def test_emulation_inside_bound_values(name, window):
    recon, target, transforms, R = value_case(name, window)
    for transform in transforms:
        ref, _ = _emulation_inside(recon, target, window, transform, R, name)
        if name == "const_identical":
            assert ref["mse"][0] == 0 and np.isinf(ref["psnr"][0]) and abs(ref["ssim"][0] - 1) < 1e-15
        if name == "const" and window == "skimage":   # a flat pair has no structure term: S is the luminance term alone (box11's
                                                      # zero border puts an edge around the image)
            x, y = transform_pair(recon[0, 0, 0, 0], target[0, 0, 0, 0], transform)
            assert abs(ref["ssim"][0] - (2 * x * y + K1 ** 2) / (x * x + y * y + K1 ** 2)) < 1e-13


@pytest.mark.parametrize("window", ["skimage", "box11"])
@pytest.mark.parametrize("transform", ALL_TRANSFORMS)
def test_emulation_inside_bound_many_tiles(window, transform):
    recon, target = noisy_pair(MANY_TILES_SHAPE, seed=300)
    _emulation_inside(logits_of(recon, transform), target, window, transform, 1.0, "2113x1025", contracts=(True,))


def test_bound_agrees_with_the_restatement():
    """the bound's own fp64 values (moments about the pivots, tile by tile) are the restatement's"""
    for window in ("skimage", "box11"):
        recon, target = noisy_pair((2, 2, 70, 134), seed=7)
        ref, _ = metrics_bound(recon, target, window, "clip", 1.0)
        want = reference_metrics(recon, target, window, "clip", 1.0)
        for k in ("mse", "psnr", "ssim"):
            np.testing.assert_allclose(ref[k], want[k], rtol=1e-12, atol=0)


# --- mutations: what the bound rejects --------------------------------------------------------------------------------------
def _mutation_ratio(recon, target, window, transform, R, **mutation):
    ref, bound = metrics_bound(recon, target, window, transform, R)
    base = bound_ratios(emulate_metrics(recon, target, window, transform, R), ref, bound)
    assert all(v <= 1.0 for v in base.values()), base                 # the kernel's own order passes on these inputs
    return bound_ratios(emulate_metrics(recon, target, window, transform, R, **mutation), ref, bound)


@pytest.mark.parametrize("window", ["skimage", "box11"])
def test_mutation_no_pivot(window):
    """moments about 0 on images offset by 64: E[x^2] - E[x]^2 cancels 4096 against variances near 1e-4 and C2 = 9e-4.  Misses
    the SSIM bound by 1.7e5 x (skimage) / 4.2e4 x (box11); this is the kernel with `s_x[e] = x`."""
    recon, target, _, R = value_case("offset64", window)
    rat = _mutation_ratio(recon, target, window, "none", R, pivot="none")
    report(f"metrics mutation no pivot {window}", rat)
    assert rat["ssim"] > 1


@pytest.mark.parametrize("window", ["skimage", "box11"])
def test_mutation_variance_from_pivot_free_second_moments(window):
    """the pivot kept for the means, the variance formed as E[x^2] - (mx + px)^2 from raw second moments: the same cancellation.
    Misses by 5.3e5 x / 4.6e5 x."""
    recon, target, _, R = value_case("offset64", window)
    rat = _mutation_ratio(recon, target, window, "none", R, pivot="raw_second")
    report(f"metrics mutation raw second moments {window}", rat)
    assert rat["ssim"] > 1


def test_mutation_population_covariance_in_skimage():
    """cov_norm = 1 instead of 49 / 48 (a definition, caught by the restatement): misses by 2.2e2 x"""
    rng = np.random.default_rng(21)                  # variances near C2: where they dwarf it, S hardly moves with cov_norm
    target = (0.5 + 0.03 * rng.standard_normal((1, 2, 37, 53))).astype(F32)
    recon = (target + 0.03 * rng.standard_normal(target.shape)).astype(F32)
    rat = _mutation_ratio(recon, target, "skimage", "clip", 1.0, cov=1.0)
    report("metrics mutation population covariance", rat)
    assert rat["ssim"] > 1


def test_mutation_mirror_border_is_invisible_under_the_crop():
    """`mirror` (d c b | a b c d) instead of `reflect`: with the 3-pixel crop every counted 7x7 window lies inside the image, so
    the border rule reaches no output and no test of the outputs can tell the two apart (asserted: bit-equal).  The rule
    matters as soon as the crop goes: then mirror moves the SSIM by 76 x the bound."""
    recon, target = noisy_pair((1, 2, 13, 13), seed=22)
    a = emulate_metrics(recon, target, "skimage", "clip", 1.0)
    b = emulate_metrics(recon, target, "skimage", "clip", 1.0, border="mirror")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    _, bound = metrics_bound(recon, target, "skimage", "clip", 1.0)
    a = emulate_metrics(recon, target, "skimage", "clip", 1.0, crop=False)
    b = emulate_metrics(recon, target, "skimage", "clip", 1.0, crop=False, border="mirror")
    factor = float(np.abs(a["ssim"].astype(np.float64) - b["ssim"]).max() / bound["ssim"].max())
    report("metrics mutation mirror border, crop omitted", factor)
    assert factor > 1


def test_mutation_crop_omitted():
    """the mean taken over the whole map, reflect border included: misses by 35 x"""
    recon, target = noisy_pair((1, 2, 13, 13), seed=22)
    rat = _mutation_ratio(recon, target, "skimage", "clip", 1.0, crop=False)
    report("metrics mutation crop omitted", rat)
    assert rat["ssim"] > 1


def test_mutation_box11_border_by_in_bounds_count():
    """count_include_pad=False (divide by the in-bounds taps) instead of / 121: misses by 2.2e2 x"""
    recon, target = noisy_pair((1, 2, 10, 10), seed=23)
    rat = _mutation_ratio(recon, target, "box11", "clip", 1.0, box_div="count")
    report("metrics mutation box11 in-bounds count", rat)
    assert rat["ssim"] > 1


def test_mutation_transform_after_the_padding():
    """the sigmoid applied to the padded zeros (0.5 instead of 0 around the reconstruction): misses by 1.4e4 x"""
    recon, target = noisy_pair((1, 2, 10, 10), seed=24)
    rat = _mutation_ratio(logits_of(recon, "sigmoid"), target, "box11", "sigmoid", 1.0, pad_after_transform=True)
    report("metrics mutation transform after padding", rat)
    assert rat["ssim"] > 1


@pytest.mark.parametrize("window", ["skimage", "box11"])
def test_mutation_constants_not_scaled_by_data_range(window):
    """C1, C2 of data_range = 1 on 8-bit values with data_range = 255: misses by 3.1e4 x / 1.9e4 x"""
    rng = np.random.default_rng(28)                  # a low-contrast 8-bit pair: variances below C2 = 58.5
    target = (100 + rng.integers(-3, 4, VALUE_SHAPE)).astype(F32)
    recon = (target + rng.integers(-2, 3, VALUE_SHAPE)).astype(F32)
    rat = _mutation_ratio(recon, target, window, "none", 255.0, scale_c=False)
    report(f"metrics mutation unscaled constants {window}", rat)
    assert rat["ssim"] > 1


def test_mutation_ragged_tile_counted_in_mse():
    """the staged pixels beyond the image (reflected copies of the last rows and columns) added to sum (x - y)^2 at 65 x 129:
    misses the MSE bound by 9.8e5 x.  (box11 stages zeros there, which add nothing.)"""
    recon, target = noisy_pair((1, 2, 65, 129), seed=25)
    rat = _mutation_ratio(recon, target, "skimage", "clip", 1.0, mse_ragged=True)
    report("metrics mutation ragged tile in mse", rat)
    assert rat["mse"] > 1 and rat["psnr"] > 1


def test_mutation_finalize_reads_256_partials():
    """7 x 32 897: 258 tiles in one row; a finalise without its strided loop drops the last two.  Misses by 1.3e3 x (mse) and
    2.4e2 x (ssim)."""
    recon, target = noisy_pair((1, 1, 7, 257 * TW + 1), seed=26)
    rat = _mutation_ratio(recon, target, "skimage", "clip", 1.0, finalize_limit=256)
    report("metrics mutation finalise 256", rat)
    assert rat["mse"] > 1 and rat["ssim"] > 1


def test_nan_pattern_of_the_restatement():
    """np.clip and the sigmoid pass a NaN on: one NaN pixel makes all three values of its image NaN and touches no other image;
    +inf under `none` gives mse = inf, psnr = -inf, ssim = NaN"""
    recon, target = noisy_pair((3, 2, 16, 20), seed=27)
    for transform in ALL_TRANSFORMS:
        r = recon.copy()
        r[1, 0, 5, 9] = np.nan
        for window in ("skimage", "box11"):
            with np.errstate(all="ignore"):
                ref = reference_metrics(r, target, window, transform)
                emu = emulate_metrics(r, target, window, transform)
            clean = emulate_metrics(recon, target, window, transform)
            for k in ("mse", "psnr", "ssim"):
                assert np.isnan(ref[k][1]) and np.isnan(emu[k][1]) and np.isfinite(ref[k][[0, 2]]).all()
                assert np.array_equal(emu[k][[0, 2]], clean[k][[0, 2]])
    r = recon.copy()
    r[1, 0, 5, 9] = np.inf
    with np.errstate(all="ignore"):
        ref = reference_metrics(r, target, "skimage", "none")
        emu = emulate_metrics(r, target, "skimage", "none")
    assert ref["mse"][1] == np.inf and ref["psnr"][1] == -np.inf and np.isnan(ref["ssim"][1])
    assert emu["mse"][1] == np.inf and emu["psnr"][1] == -np.inf and np.isnan(emu["ssim"][1])
