"""sFID, KID, density / coverage and the Inception Score over splits without a GPU: the fp64 restatement
(tests/gen_suite_restatement.py) on toys with known answers, the conditions the GPU tests' inputs have to meet, the clean fp32
emulations under the bounds of DESIGN.md section 3.1 row S, every planted defect rejected, the subset draw, the split arithmetic and
the host-side argument checks."""
import inspect

import numpy as np
import pytest
import torch

import gen_restatement as G
import gen_suite_restatement as GS


@pytest.fixture(scope="module", params=[(s, sh) for s in G.SHAPES for sh in (0.0, 1000.0)], ids=lambda p: f"{G.shape_id(p[0])}-{p[1]:g}")
def case(request):
    (N, M, d, k, seed), shift = request.param
    x, q = G.make_inputs(N, M, d, seed, shift=shift)
    return dict(x=x, q=q, k=k, r2=G.knn_radius64(x, k).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# ball counts, density and coverage
# ---------------------------------------------------------------------------------------------------------------------------
def test_count_toys():
    x = np.array([[0.0], [1.0], [5.0]], dtype=np.float32)
    q = np.array([[0.5], [4.0], [100.0]], dtype=np.float32)
    assert GS.counts64(q, x, [1.0, 0.25, 1.0], "data").tolist() == [2, 1, 0]          # 0.25 from x_0 and x_1; exactly 1 from x_2
    assert GS.counts64(q, x, [0.25, 9.0, 1.0], "query").tolist() == [2, 2, 0]
    same = GS.density_coverage64(x, x.copy(), 1)
    assert same == {"density": 2.0, "coverage": 1.0}      # radii 1, 1, 16: the points fall into 2, 3 (a tie at 16 counts) and 1 balls
    far = GS.density_coverage64(x, x + np.float32(1000.0), 1)
    assert far == {"density": 0.0, "coverage": 0.0}


def test_reference_decides_the_counts(case):
    x, q, r2 = case["x"], case["q"], case["r2"]
    pairs = 0.0
    for qq, xx, of in ((q, x, "data"), (x, q, "query")):
        inside, undecided = GS.classify_pairs(qq, xx, r2, of)
        print(f"{of}: decided inside {int(inside.sum())}, undecided {int(undecided.sum())} of {undecided.size} pairs")
        assert undecided.mean() <= GS.UNDECIDED_PAIRS_MAX
        pairs = max(pairs, undecided.mean())
    cov = GS.undecided_coverage(x, q, r2)
    dc = GS.density_coverage64(x, q, case["k"])
    print(f"density {dc['density']:.4g}, coverage {dc['coverage']:.4g}, undecided coverage decisions {cov:.3g}")
    assert cov <= GS.UNDECIDED_COVERAGE_MAX
    assert 0.0 < dc["density"] and 0.0 < dc["coverage"] <= 1.0


def test_inputs_give_both_coverage_outcomes():
    cov = [GS.density_coverage64(*G.make_inputs(N, M, d, seed), k)["coverage"] for N, M, d, k, seed in G.SHAPES]
    assert min(cov) < 1.0 and max(cov) > 0.0 and any(0.0 < c < 1.0 for c in cov), cov


def test_clean_count_chain_passes(case):
    x, q, r2 = case["x"], case["q"], case["r2"]
    for qq, xx, of in ((q, x, "data"), (x, q, "query")):
        msg, _ = GS.check_counts(GS.counts32(qq, xx, r2, of), qq, xx, r2, of)
        assert msg is None, msg


def test_strict_comparison_is_rejected_on_a_tie():
    x = np.array([[0, 0], [3, 4], [40, 0]], dtype=np.float32)           # r2 at k = 1: 25, 25, 37^2 + 16
    r2 = G.knn_radius64(x, 1).astype(np.float32)
    q = np.array([[-3, 4], [-30, -30]], dtype=np.float32)               # exactly 25 from x_0 (and 52 from x_1); far from all
    # a tie is undecided under (d + 2) u, so the range check lets it pass either way: the exact (integer) case is what catches it
    assert GS.counts64(q, x, r2, "data").tolist() == [1, 0]
    assert GS.counts32(q, x, r2, "data").tolist() == [1, 0]
    assert GS.counts32(q, x, r2, "data", strict=True).tolist() == [0, 0]
    rq = np.float32([25.0, 1.0])
    assert GS.counts64(q, x, rq, "query").tolist() == [1, 0]
    assert GS.counts32(q, x, rq, "query").tolist() == [1, 0]
    assert GS.counts32(q, x, rq, "query", strict=True).tolist() == [0, 0]


def test_swapped_radius_is_rejected():
    N, M, d, k, seed = G.SHAPES[2]                                       # M == N: the swapped index stays in range
    x, q = G.make_inputs(N, M, d, seed)
    r2 = G.knn_radius64(x, k).astype(np.float32)
    for of in ("data", "query"):
        assert GS.check_counts(GS.counts32(q, x, r2, of), q, x, r2, of)[0] is None
        assert GS.check_counts(GS.counts32(q, x, r2, of, swapped=True), q, x, r2, of)[0] is not None, of


# ---------------------------------------------------------------------------------------------------------------------------
# KID
# ---------------------------------------------------------------------------------------------------------------------------
def _subsets(n_a, n_b, S, m, seed, repeat=True):
    g = np.random.default_rng(seed)
    ia = np.stack([g.choice(n_a, m, replace=False) for _ in range(S)]).astype(np.int32)
    ib = np.stack([g.choice(n_b, m, replace=False) for _ in range(S)]).astype(np.int32)
    if repeat and m > 1:
        ib[1, 1] = ib[1, 0]                                              # a row met twice on the cross side
    return ia, ib


def test_poly_sum_toys():
    a = np.array([[1.0, 2.0], [0.0, 1.0]], dtype=np.float32)
    idx = np.array([[0, 1]], dtype=np.int32)
    # gamma = 1, coef0 = 1: k = (x.y + 1)^3 = [[216, 27], [27, 8]]
    assert GS.poly_sums64(a, idx, a, idx, 1.0, 1.0, False).tolist() == [278.0]
    assert GS.poly_sums64(a, idx, a, idx, 1.0, 1.0, True).tolist() == [54.0]
    assert GS.poly_sums32(a, idx, a, idx, 1.0, 1.0, True).tolist() == [54.0]
    assert GS.mmd2_from_sums([54.0], [54.0], [278.0], 2).tolist() == [54.0 - 139.0]
    assert GS.self_kid64(a, idx)[0] == pytest.approx(GS.kid64(a, a, idx, idx)[0], rel=1e-12) and GS.self_kid64(a, idx)[0] < 0


@pytest.mark.parametrize("shape", [(130, 70, 2048), (65, 9, 37), (257, 257, 64)], ids=lambda s: "x".join(map(str, s)))
def test_clean_product_chain_passes_and_defects_do_not(shape):
    N, M, d = shape
    a, b = GS.poly_inputs(N, M, d, 5)
    m = min(N, M, 70)
    ia, ib = _subsets(N, M, 3, m, 7)
    gamma = 1.0 / d
    for x, ix, y, iy, skip in ((a, ia, a, ia, True), (b, ib, b, ib, True), (a, ia, b, ib, False)):
        ref, bound = GS.poly_sums64(x, ix, y, iy, gamma, 1.0, skip), GS.poly_sums_bound(x, ix, y, iy, gamma, 1.0, skip)
        err = np.abs(GS.poly_sums32(x, ix, y, iy, gamma, 1.0, skip) - ref)
        print(f"{shape} skip {skip}: worst error / bound {np.max(err / bound):.3g}")
        assert (err <= bound).all()
        if skip:
            assert (np.abs(GS.poly_sums32(x, ix, y, iy, gamma, 1.0, skip, keep_diagonal=True) - ref) > bound).all(), "diagonal kept"
    mean, std, _ = GS.kid64(a, b, ia, ib)
    bm, bs = GS.kid_bound(a, b, ia, ib)
    got = GS.kid64(a, b, ia, ib, sums=GS.poly_sums32)
    assert abs(got[0] - mean) <= bm and abs(got[1] - std) <= bs
    assert abs(GS.kid64(a, b, ia, ib, keep_diagonal=True)[0] - mean) > bm, "diagonal kept"
    assert abs(GS.kid64(a, b, ia, ib, biased=True)[0] - mean) > bm, "biased normaliser"


def test_integer_kernel_sums_are_exact():
    g = np.random.default_rng(13)
    x = g.integers(-3, 4, size=(150, 37)).astype(np.float32)
    y = g.integers(-3, 4, size=(150, 37)).astype(np.float32)
    for m in (1, 63, 65):
        ia, ib = _subsets(150, 150, 3, m, m)
        for args in ((x, ia, x, ia, 1.0, 1.0, True), (x, ia, y, ib, 1.0, 1.0, False)):
            ref = GS.poly_sums64(*args)
            assert ref.max() < 150 * 150 * 2.0 ** 26 and np.array_equal(ref, np.round(ref))
            assert np.array_equal(GS.poly_sums32(*args), ref)


def test_subset_draw_is_deterministic_and_clamped():
    import transvae
    ia, ib, m = transvae.kid_subsets(50, 37, subsets=4, subset_size=20, seed=3)
    assert m == 20 and ia.shape == ib.shape == (4, 20) and ia.dtype == ib.dtype == np.int32
    ra, rb = GS.draw_subsets(50, 37, 4, 20, 3)
    assert np.array_equal(ia, ra) and np.array_equal(ib, rb), "the draw is not the documented one"
    again = transvae.kid_subsets(50, 37, subsets=4, subset_size=20, seed=3)
    assert np.array_equal(again[0], ia) and np.array_equal(again[1], ib)
    other = transvae.kid_subsets(50, 37, subsets=4, subset_size=20, seed=4)
    assert not np.array_equal(other[0], ia)
    assert 0 <= ia.min() and ia.max() < 50 and 0 <= ib.min() and ib.max() < 37
    assert all(len(set(r.tolist())) == 20 for r in ia) and all(len(set(r.tolist())) == 20 for r in ib), "drawn with replacement"
    ia, ib, m = transvae.kid_subsets(50, 12, subsets=2, subset_size=1000, seed=0)          # clamped to the smaller side
    assert m == 12 and ia.shape == (2, 12) and sorted(ib[0].tolist()) == list(range(12))
    with pytest.raises(ValueError, match="m=1"):
        transvae.kid_subsets(50, 1, subsets=2, subset_size=10)
    with pytest.raises(ValueError, match="subsets=0"):
        transvae.kid_subsets(50, 50, subsets=0)


# ---------------------------------------------------------------------------------------------------------------------------
# Inception Score over splits
# ---------------------------------------------------------------------------------------------------------------------------
def test_split_arithmetic():
    from transvae.metrics_gen import scores_from_states, split_pieces
    assert split_pieces(0, 37, 10) == [(0, 0, 10), (1, 10, 10), (2, 20, 10), (3, 30, 7)]
    assert split_pieces(5, 32, 10) == [(0, 0, 5), (1, 5, 10), (2, 15, 10), (3, 25, 7)]
    assert split_pieces(30, 7, 10) == [(3, 0, 7)] and split_pieces(10, 0, 10) == [] and split_pieces(9, 1, 10) == [(0, 0, 1)]
    for cuts in ((37,), (5, 32), (10, 10, 10, 7), (1,) * 37):
        rows, n0 = {}, 0
        for B in cuts:
            for split, b0, nb in split_pieces(n0, B, 10):
                rows.setdefault(split, []).extend(range(n0 + b0, n0 + b0 + nb))
            n0 += B
        assert [(r[0], r[-1] + 1) for _, r in sorted(rows.items())] == GS.split_bounds(37, 10), cuts
    z = (np.random.default_rng(2).standard_normal((37, 11)) * 3).astype(np.float32)
    states = GS.split_states64(z, 10)
    assert states.shape == (4, 13) and states[:, 0].tolist() == [10, 10, 10, 7]
    got, want = scores_from_states(states), GS.split_scores64(z, 10)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert scores_from_states(G.softmax_stats64(z)).shape == (1,)
    whole = G.score64(z.astype(np.float64))
    assert got.mean() != pytest.approx(whole, rel=1e-6), "the mean over splits is another statistic than the whole-set score"


# ---------------------------------------------------------------------------------------------------------------------------
# the host interface
# ---------------------------------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    import transvae
    from transvae import evaluate_dit as _  # noqa: F401
    from transvae.evaluate_dit import ALL_METRICS, METRICS
    from transvae.metrics_fid import SPATIAL_DIM, SPATIAL_LD
    for name in ("ball_counts", "density_coverage", "kernel_inception_distance", "kid_subsets", "poly_kernel_sums", "ALL_METRICS"):
        assert name in transvae.__all__ and hasattr(transvae, name), name
    assert METRICS == ("gfid", "is", "precision", "recall") and set(METRICS) < set(ALL_METRICS)
    assert set(ALL_METRICS) - set(METRICS) == {"sfid", "kid", "density", "coverage"}
    assert (SPATIAL_DIM, SPATIAL_LD) == (2023, 2048) and SPATIAL_LD % 64 == 0
    sig = inspect.signature(transvae.evaluate_dit).parameters
    for name, default in dict(metrics=METRICS, is_split_size=None, prdc_k=5, kid_subsets=100, kid_subset_size=1000, kid_seed=0).items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    assert inspect.signature(transvae.reference_statistics).parameters["spatial"].default is False
    assert inspect.signature(transvae.InceptionFeatures.features).parameters["spatial"].default is False
    assert inspect.signature(transvae.InceptionScore).parameters["split_size"].default is None
    assert inspect.signature(transvae.density_coverage).parameters["k"].default == 5
    kid = inspect.signature(transvae.kernel_inception_distance).parameters
    assert (kid["subsets"].default, kid["subset_size"].default, kid["seed"].default) == (100, 1000, 0)


def test_no_cpu_fallback():
    import transvae
    x = torch.rand(12, 8)
    idx = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.ball_counts(x, x, torch.ones(12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.density_coverage(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.kernel_inception_distance(x, x, subsets=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.poly_kernel_sums(x, idx, x, idx, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.InceptionScore(torch.rand(5, 8), split_size=4).update(x)


def test_argument_errors():
    import transvae
    x = torch.rand(6, 8)
    with pytest.raises(ValueError, match="radius_of='point'"):
        transvae.ball_counts(x, x, torch.ones(6), radius_of="point")
    with pytest.raises(ValueError, match=r"r2 must be \[4\]"):
        transvae.ball_counts(torch.rand(4, 8), x, torch.ones(6), radius_of="query")
    with pytest.raises(ValueError, match=r"r2 must be \[6\]"):
        transvae.ball_counts(torch.rand(4, 8), x, torch.ones(4), radius_of="data")
    with pytest.raises(ValueError, match="columns"):
        transvae.ball_counts(torch.rand(4, 7), x, torch.ones(6))
    with pytest.raises(ValueError, match="columns"):
        transvae.density_coverage(x, torch.rand(6, 7))
    with pytest.raises(ValueError, match="k=9"):
        transvae.density_coverage(x, x, k=9)
    with pytest.raises(ValueError, match="columns"):
        transvae.kernel_inception_distance(x, torch.rand(6, 7))
    with pytest.raises(ValueError, match="m=1"):
        transvae.kernel_inception_distance(x, torch.rand(1, 8))
    with pytest.raises(ValueError, match="one shape"):
        transvae.poly_kernel_sums(x, torch.zeros(2, 3, dtype=torch.int32), x, torch.zeros(2, 4, dtype=torch.int32), 1.0)
    with pytest.raises(ValueError, match="split_size=0"):
        transvae.InceptionScore(torch.rand(5, 8), split_size=0)
    dit = transvae.DiT(8, 2, 4, 64, 1, 5)
    ref = {"n": 4, "mean": torch.zeros(8), "cov": torch.eye(8), "features": torch.rand(6, 8)}
    ev = lambda **kw: transvae.evaluate_dit(None, dit, kw.pop("reference", ref), fid_net=None, **kw)
    with pytest.raises(ValueError, match=r"metrics.*\['fvd'\]"):
        ev(metrics=("gfid", "fvd"))
    with pytest.raises(ValueError, match=r"'sfid'.*spatial=True"):
        ev(metrics=("sfid",), num_samples=8)
    with pytest.raises(ValueError, match="2023 wide"):
        ev(metrics=("sfid",), num_samples=8, reference=dict(ref, spatial_mean=torch.zeros(8), spatial_cov=torch.eye(8)))
    with pytest.raises(ValueError, match="prdc_k=0"):
        ev(metrics=("density",), prdc_k=0)
    with pytest.raises(ValueError, match="is_split_size=0"):
        ev(metrics=("gfid",), is_split_size=0)
    with pytest.raises(ValueError, match="reference holds no features"):
        ev(metrics=("coverage",), num_samples=8, reference={"n": 4, "mean": torch.zeros(8), "cov": torch.eye(8)})
    with pytest.raises(ValueError, match="reference holds no features"):
        ev(metrics=("density",), num_samples=8, prdc_k=6)                                    # 6 rows, k + 1 = 7 needed
    with pytest.raises(ValueError, match="subsets=0"):
        ev(metrics=("kid",), num_samples=8, kid_subsets=0, kid_subset_size=6)
    with pytest.raises(ValueError, match=r"\['kid'\].*kid_subset_size=1000.*holds 6 features and 8 fake"):  # no silent clamp in a whole evaluation
        ev(metrics=("kid",), num_samples=8)
    with pytest.raises(ValueError, match=r"kid_subset_size=6.*4 fake"):
        ev(metrics=("kid",), num_samples=8, max_features=4, kid_subset_size=6)
    for m in ("kid", "density", "coverage"):                                                 # well-formed: as far as the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev(metrics=(m,), num_samples=8, kid_subset_size=6)
