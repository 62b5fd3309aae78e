"""csrc/latent.hip and transvae/latents.py on the device: `tv_kde_logdensity` under the contract of DESIGN.md section 3.1 row T
against the float64 restatement, `tv_latent_stats` under row F's criterion against NumPy float64, `extract_latents` on the micro
model and `latent_density_metrics` against the restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import latent_restatement as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def kde(x, q, h, loo, pad=3):
    """the C ABI with ldx = d + pad: the points are column slices of wider buffers filled with a sentinel"""
    from transvae.hip import _lib as L
    lib = L.load()
    N, d = x.shape
    xb = torch.full((N, d + pad), 7.5e8, dtype=torch.float32, device=dev())
    xb[:, :d] = x.to(dev())
    if q is None:
        qb, M = xb, N
    else:
        M = q.shape[0]
        qb = torch.full((M, d + pad + 1), -7.5e8, dtype=torch.float32, device=dev())
        qb[:, :d] = q.to(dev())
    out = torch.full((M + 8,), -7.25, dtype=torch.float32, device=dev())
    scratch = torch.empty(128 * M, dtype=torch.float64, device=dev()) if M < 2048 else None
    L.check(lib.tv_kde_logdensity(_p(xb), N, _p(qb), M, d, xb.stride(0), qb.stride(0), 1.0 / (2.0 * h * h), 1 if loo else 0, _p(out),
                                  _p(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tv_kde_logdensity")
    torch.cuda.synchronize()
    assert bool((out[M:] == -7.25).all()), "wrote past out[M]"
    return out[:M].cpu()


def points(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    if n >= 63:
        x[7] = x[3]              # a duplicated point
        x[11] = 1e3              # a point far from everything: its log density must be finite
    return x


@pytest.mark.parametrize("d", [1, 2, 3, 16, 32, 33, 64])
def test_kde_against_fp64(d):
    worst = 0.0
    for n in (2, 63, 64, 65, 257, 1000):
        x = points(n, d, 100 * d + n)
        h = R.scott(n, d)
        for loo in (False, True):
            out = kde(x, None, h, loo)
            assert bool(torch.isfinite(out).all()), (d, n, loo)
            ratio = R.kde_ratio(out, x, None, h, loo)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (d, n, loo, ratio)
            assert torch.equal(out, kde(x, None, h, loo)), "two runs differ"
    report(f"kde d={d}: worst |out - l64| / bound", round(worst, 3))


@pytest.mark.parametrize("d", [2, 3, 16])
def test_kde_small_bandwidth(d):
    x = points(257, d, 5)
    for loo in (False, True):
        ratio = R.kde_ratio(kde(x, None, 0.01, loo), x, None, 0.01, loo)
        report(f"kde d={d} h=0.01 loo={loo}", round(ratio, 3))
        assert ratio <= 1.0


def test_kde_split_and_unsplit():
    """M = 7 queries over N = 5000 takes the sliced path (5 slices + merge); M = N = 5000 the unsliced one"""
    x = points(5000, 3, 9)
    q = torch.cat([x[:5], torch.tensor([[0.1, -0.2, 0.3], [5.0, 5.0, 5.0]])])
    h = R.scott(5000, 3)
    out = kde(x, q, h, False)
    ratio = R.kde_ratio(out, x, q, h, False)
    report("kde N=5000 M=7 (sliced)", round(ratio, 3))
    assert ratio <= 1.0 and torch.equal(out, kde(x, q, h, False))
    full = kde(x, None, h, False)
    ratio = R.kde_ratio(full, x, None, h, False)
    report("kde N=M=5000 (unsliced)", round(ratio, 3))
    assert ratio <= 1.0
    loo = kde(x, None, h, True)
    ratio = R.kde_ratio(loo, x, None, h, True)
    report("kde N=M=5000 leave-one-out", round(ratio, 3))
    assert ratio <= 1.0 and bool(torch.isfinite(loo).all())


# ---------------------------------------------------------------------------------------------------------------------------
def _stats(lat, dim=None):
    import transvae
    st = transvae.LatentStats(dim or lat.shape[1])
    st.update(lat)
    return st


@pytest.mark.parametrize("D", [4, 16, 32, 64])
def test_latent_stats_against_numpy(D):
    import transvae
    g = torch.Generator().manual_seed(D)
    worst = 0.0
    for B in (1, 3):
        for P in (1, 35, 256):
            x = (1e3 + torch.randn(B, D, P, generator=g)).to(dev())
            st = _stats(x)
            n, mean, cov = R.moments64(x.cpu().numpy())
            assert st.n == n
            em = R.rel_fro(st.mean.cpu().numpy(), mean)
            worst = max(worst, em)
            assert em <= 1e-10
            if n > 1:
                ec = R.rel_fro(st.cov.cpu().numpy(), cov)
                worst = max(worst, ec)
                assert ec <= 1e-10, (B, P, ec)
            c = st.cov
            assert torch.equal(c, c.T), "the scatter is not bit-symmetric"
            st2 = _stats(x)
            assert torch.equal(st2._state, st._state), "two runs differ"
    report(f"latent stats D={D}: worst relative Frobenius error", f"{worst:.2e}")
    # batches 1 + 2 against 3 at once, a strided channel slice of a [B, 2 D, h, w] moments tensor, and the state round trip
    mom = (1e3 + torch.randn(3, 2 * D, 5, 7, generator=g)).to(dev())
    whole = _stats(mom[:, :D])
    parts = transvae.LatentStats(D)
    parts.update(mom[:1, :D])
    saved = parts.state_dict()
    parts = transvae.LatentStats(D)
    parts.load_state_dict(saved, device=dev())
    parts.update(mom[1:, :D])
    n, mean, cov = R.moments64(mom[:, :D].cpu().numpy())
    assert parts.n == whole.n == n
    assert R.rel_fro(whole.cov.cpu().numpy(), cov) <= 1e-10 and R.rel_fro(whole.mean.cpu().numpy(), mean) <= 1e-10
    assert R.rel_fro(parts.cov.cpu().numpy(), whole.cov.cpu().numpy()) <= 1e-12
    assert R.rel_fro(parts.mean.cpu().numpy(), whole.mean.cpu().numpy()) <= 1e-12
    assert R.rel_fro(parts.std.cpu().numpy(), np.sqrt(np.diag(cov))) <= 1e-10


# ---------------------------------------------------------------------------------------------------------------------------
def micro_model():
    from oracle import filler
    from oracle import transvae_oracle as O
    from transvae import TransVAE
    cfg = dict(O.MICRO)
    assert cfg["depths"] == [1, 1, 1, 1, 1] and cfg["base_dims"] == [32, 32, 64, 64, 128]
    m = TransVAE(config=cfg, variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4)))
    return m.to(dev()).eval()


@pytest.mark.parametrize("what", ["mean", "moments"])
def test_extract_latents_micro(tmp_path, what):
    import transvae
    from oracle import filler
    model = micro_model()
    x = filler.rand_input("latents.x", (5, 3, 64, 64))
    labels = torch.tensor([3, 1, 4, 1, 5])
    loader = [(x[0:2], labels[0:2]), (x[2:4], labels[2:4]), (x[4:5], labels[4:5])]
    stats = transvae.extract_latents(model, loader, str(tmp_path), flip=True, what=what, shard_size=3, device=dev())
    shards = [torch.load(os.path.join(tmp_path, f"latents_shard{k:03d}.pt")) for k in range(2)]
    assert not os.path.exists(os.path.join(tmp_path, "latents_shard002.pt"))
    assert [s["latents"].shape[0] for s in shards] == [3, 2]
    lat = torch.cat([s["latents"] for s in shards])
    flp = torch.cat([s["latents_flip"] for s in shards])
    assert torch.equal(torch.cat([s["labels"] for s in shards]), labels) and shards[0]["labels"].dtype == torch.int64
    assert lat.dtype == torch.float32 and flp.dtype == torch.float32
    with torch.no_grad():
        want = torch.cat([torch.cat(model.encode(b.to(dev())), 1) for b, _ in loader]).cpu()
        want_f = torch.cat([torch.cat(model.encode(torch.flip(b, dims=[3]).to(dev())), 1) for b, _ in loader]).cpu()
    C4 = 4 if what == "mean" else 8
    assert lat.shape == (5, C4, 4, 4)
    assert torch.equal(lat, want[:, :C4]), "saved latents differ from model.encode(x)"
    assert torch.equal(flp, want_f[:, :C4]), "saved flipped latents differ from model.encode(flip(x))"
    sf = torch.load(os.path.join(tmp_path, "latents_stats.pt"))
    assert sf["mean"].shape == (1, 4, 1, 1) and sf["std"].shape == (1, 4, 1, 1) and sf["mean"].dtype == torch.float32
    assert sf["cov"].dtype == torch.float64 and sf["n"] == 5 * 16 == stats.n
    n, mean, cov = R.moments64(lat[:, :4].numpy())
    assert R.rel_fro(sf["cov"].numpy(), cov) <= 1e-10
    assert R.rel_fro(stats.mean.cpu().numpy(), mean) <= 1e-10
    assert torch.equal(sf["mean"].reshape(-1), stats.mean.float().cpu()) and torch.equal(sf["std"].reshape(-1), stats.std.float().cpu())
    assert np.allclose(sf["std"].reshape(-1).numpy(), np.sqrt(np.diag(cov)), rtol=1e-6)


@pytest.mark.parametrize("pca", [None, 2])
def test_density_metrics_against_restatement(pca):
    import transvae
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(1000, 4, generator=g) * torch.tensor([1.0, 2.0, 0.5, 3.0]) + torch.tensor([0.0, 5.0, -1.0, 2.0])
    pts[:300] += torch.tensor([4.0, 0.0, 0.0, 6.0])          # two clusters: the densities are far from uniform
    got = transvae.latent_density_metrics(pts.to(dev()), pca=pca)
    want = R.density_metrics64(pts, pca=pca)
    assert got["n"] == 1000 and got["d"] == (pca or 4) and abs(got["bandwidth"] - want["bandwidth"]) < 1e-12
    for key in ("density_cv", "normalized_entropy", "gini"):
        rel = abs(got[key] - want[key]) / abs(want[key])
        report(f"density metrics pca={pca} {key}", f"{got[key]:.6f} (relative error {rel:.1e})")
        assert rel <= 1e-5, (key, got[key], want[key])


def test_latent_space_metrics_glue():
    import transvae
    from oracle import filler
    model = micro_model()
    x = filler.rand_input("latents.x", (5, 3, 64, 64))
    res = transvae.latent_space_metrics(model, [(x[:3], None), (x[3:], None)], device=dev(), max_points=64, pca=2)
    with torch.no_grad():
        mu = torch.cat([model.encode(x[:3].to(dev()))[0], model.encode(x[3:].to(dev()))[0]])
    pts = transvae.latent_points(mu, max_points=64)
    assert pts.shape == (64, 4)
    want = transvae.latent_density_metrics(pts, pca=2)
    assert res == want and res["n"] == 64 and res["d"] == 2 and 0 < res["normalized_entropy"] <= 1
