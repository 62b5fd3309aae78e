"""Latent-space metrics, host side: the float64 restatement (tests/latent_restatement.py) against closed forms, the contract
bound of DESIGN.md section 3.1 row T against an fp32 emulation and against four defects it has to reject, and the argument
errors of transvae/latents.py.  Nothing here needs a GPU."""
import ctypes as C
import math

import pytest
import torch

import latent_restatement as R


def test_circle_is_uniform():
    """n equally spaced points on a circle all see the same neighbourhood: CV 0, entropy 1, Gini 0"""
    n = 48
    a = torch.arange(n, dtype=torch.float64) * (2 * math.pi / n)
    pts = torch.stack([torch.cos(a), torch.sin(a)], 1)
    for loo in (False, True):
        l64, _ = R.log_density64(pts, None, 0.3, loo)
        m = R.metrics64(l64)
        assert abs(m["density_cv"]) < 1e-12 and abs(m["normalized_entropy"] - 1) < 1e-12 and abs(m["gini"]) < 1e-12, m


def test_gini_of_one_to_four():
    m = R.metrics64(torch.log(torch.tensor([3.0, 1.0, 4.0, 2.0], dtype=torch.float64)))
    assert abs(m["gini"] - 0.25) < 1e-14
    assert abs(m["density_cv"] - math.sqrt(1.25) / 2.5) < 1e-14
    p = torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64)
    assert abs(m["normalized_entropy"] - float(-(p * p.log()).sum() / math.log(4))) < 1e-14


@pytest.mark.parametrize("loo", [False, True])
def test_two_clusters_closed_form(loo):
    """a copies of one point and b copies of another at distance r: density ratio (a' + b e) / (b' + a e), e = exp(-r^2 / 2h^2)"""
    a, b, r, h = 5, 3, 1.5, 0.7
    pts = torch.zeros(a + b, 2, dtype=torch.float64)
    pts[a:, 0] = r
    l64, _ = R.log_density64(pts, None, h, loo)
    e = math.exp(-r * r / (2 * h * h))
    own = 1 if loo else 0
    want = math.log((a - own + b * e) / (b - own + a * e))
    assert abs(float(l64[0] - l64[a]) - want) < 1e-13
    assert float((l64[:a] - l64[0]).abs().max()) == 0 and float((l64[a:] - l64[a]).abs().max()) == 0


def mutation_points(n=400, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    x[7] = x[3]              # a duplicated point
    x[11] = 1e3              # a point far from everything
    return x


CASES = [(1, None), (2, None), (3, None), (16, None), (32, None), (64, None), (3, 0.01), (16, 0.05)]


@pytest.mark.parametrize("d,h", CASES)
def test_emulation_inside_the_bound(d, h):
    """an fp32 computation in the kernel's order of operations sits inside row T's bound, with the derived k(N)"""
    x = mutation_points(d=d)
    hh = h or R.scott(x.shape[0], d)
    for loo in (False, True):
        ratio = R.kde_ratio(R.emulate_fp32(x, None, hh, loo), x, None, hh, loo)
        print(f"[error-budget] kde emulation d={d} h={hh:.3g} loo={loo}: {ratio:.3f} of the bound")
        assert ratio <= 1.0


def test_emulation_split_queries():
    g = torch.Generator().manual_seed(1)
    x, q = torch.randn(5000, 3, generator=g), torch.randn(7, 3, generator=g)
    h = R.scott(5000, 3)
    assert R.kde_ratio(R.emulate_fp32(x, q, h), x, q, h) <= 1.0


@pytest.mark.parametrize("defect,d,h,loo", [("bf16_inputs", 16, None, True), ("bf16_inputs", 2, None, False), ("gram", 3, 0.01, True),
                                            ("gram", 2, 0.01, True), ("keep_self", 16, None, True), ("keep_self", 2, None, True),
                                            ("no_max", 16, None, True), ("no_max", 2, None, True)])
def test_bound_rejects_defect(defect, d, h, loo):
    """Gram distances: at a small bandwidth in few dimensions, where |x|^2 / h^2 dwarfs the scores' own size (in 16 dimensions
    at h = 0.05 the nearest neighbour is so far that the form's error stays inside the bound: 0.58).  No running maximum: under
    leave-one-out, where the outlier has no self term to hold its sum above the underflow."""
    x = mutation_points(d=d)
    hh = h or R.scott(x.shape[0], d)
    ratio = R.kde_ratio(R.emulate_fp32(x, None, hh, loo, defect=defect), x, None, hh, loo)
    print(f"[error-budget] kde defect {defect} d={d}: {ratio:.3g} x the bound")
    assert ratio > 1.0


def test_moments_restatement():
    import numpy as np
    a = np.random.default_rng(0).normal(size=(3, 4, 5, 2))
    n, mean, cov = R.moments64(a)
    rows = a.transpose(0, 2, 3, 1).reshape(-1, 4)
    assert n == 30 and np.allclose(mean, rows.mean(0)) and np.allclose(cov, np.cov(rows.T, bias=True))


def test_argument_errors():
    import transvae
    from transvae import latents as T
    with pytest.raises(ValueError, match="64"):
        transvae.latent_density_metrics(torch.zeros(10, 65))
    with pytest.raises(ValueError, match="at least 2"):
        transvae.latent_density_metrics(torch.zeros(1, 4))
    with pytest.raises(ValueError, match="pca"):
        transvae.latent_density_metrics(torch.zeros(10, 4), pca=5)
    with pytest.raises(ValueError, match="bandwidth"):
        transvae.latent_density_metrics(torch.zeros(10, 4), bandwidth="silverman")
    with pytest.raises(ValueError, match="bandwidth"):
        transvae.latent_density_metrics(torch.zeros(10, 4), bandwidth=0.0)
    with pytest.raises(ValueError):
        transvae.LatentStats(65)
    with pytest.raises(ValueError):
        transvae.LatentStats(4).update(torch.zeros(2, 5, 3, 3))
    with pytest.raises(ValueError, match="per"):
        transvae.latent_points(torch.zeros(2, 4, 3, 3), per="pixel")
    with pytest.raises(ValueError, match="what"):
        transvae.extract_latents(torch.nn.Identity(), [], "unused", what="z")
    with pytest.raises(ValueError):
        T.kde_logdensity(torch.zeros(1, 2), None, 1.0, exclude_self=True)


def test_cpu_tensors_are_refused():
    import transvae
    from transvae import latents as T
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.latent_density_metrics(torch.randn(10, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.LatentStats(4).update(torch.zeros(2, 4, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.kde_logdensity(torch.zeros(5, 2), None, 1.0)


def test_latent_points_shapes():
    import transvae
    x = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2)
    tok = transvae.latent_points(x)
    assert tok.shape == (8, 3) and torch.equal(tok[1], x[0, :, 0, 1])
    img = transvae.latent_points(x, per="image")
    assert img.shape == (2, 3) and torch.equal(img, x.mean(dim=(2, 3)))
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    a, b = transvae.latent_points(x, max_points=5, generator=g1), transvae.latent_points(x, max_points=5, generator=g2)
    assert a.shape == (5, 3) and torch.equal(a, b)
    assert {tuple(r.tolist()) for r in a} <= {tuple(r.tolist()) for r in tok}


def test_c_abi_rejects_bad_arguments():
    """TV_CHECK_ARG fires before anything touches a device"""
    from transvae.hip import _lib as L
    L.build()
    lib = L.load()
    p = C.c_void_p(64)
    assert lib.tv_kde_logdensity(p, 1, p, 1, 2, 2, 2, 1.0, 1, p, p, None) != 0          # N == 1 with exclude_self
    assert b"exclude_self" in lib.tv_last_error()
    assert lib.tv_kde_logdensity(p, 8, p, 8, 65, 65, 65, 1.0, 0, p, p, None) != 0       # d > 64
    assert lib.tv_kde_logdensity(p, 8, p, 8, 4, 3, 4, 1.0, 0, p, p, None) != 0          # ldx < d
    assert lib.tv_kde_logdensity(p, 8, p, 8, 4, 4, 4, 0.0, 0, p, p, None) != 0          # no bandwidth
    assert lib.tv_latent_stats(p, 65 * 4, 4, 1, 65, 4, p, p, None) != 0                 # D > 64
    assert lib.tv_latent_stats(p, 4, 4, 2, 2, 4, p, p, None) != 0                       # overlapping strides
