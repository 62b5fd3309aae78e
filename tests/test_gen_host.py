"""The generation metrics without a GPU: the fp64 restatement (tests/gen_restatement.py) on toys with known answers, the clean fp32
chain emulation under the bounds of DESIGN.md section 3.1 row S, every planted defect rejected, and the host-side argument checks of
transvae/metrics_gen.py, transvae/evaluate_dit.py and ParamEMA."""
import inspect

import numpy as np
import pytest
import torch

import gen_restatement as G


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement on toys
# ---------------------------------------------------------------------------------------------------------------------------
def test_identical_sets_give_one():
    x, _ = G.make_inputs(40, 4, 16, 5)
    assert G.precision_recall64(x, x.copy(), 3) == {"precision": 1.0, "recall": 1.0}


def test_far_clusters_give_zero():
    g = np.random.default_rng(0)
    a = g.standard_normal((30, 8)).astype(np.float32)
    b = (g.standard_normal((30, 8)) + 100.0).astype(np.float32)
    assert G.precision_recall64(a, b, 3) == {"precision": 0.0, "recall": 0.0}


def test_radius_counts_duplicates_and_excludes_self():
    x = np.array([[0.0], [0.0], [3.0], [10.0]], dtype=np.float32)
    assert G.knn_radius64(x, 1).tolist() == [0.0, 0.0, 9.0, 49.0]
    assert G.knn_radius64(x, 2).tolist() == [9.0, 9.0, 9.0, 100.0]
    assert G.knn_radius64(x, 2, i0=2, M=2).tolist() == [9.0, 100.0]


def test_inception_score_toys():
    K = 7
    assert G.score64(np.zeros((5, K))) == pytest.approx(1.0, abs=1e-12)              # uniform rows: IS = 1
    z = np.full((3 * K, K), -40.0)
    z[np.arange(3 * K), np.arange(3 * K) % K] = 40.0                                # balanced, confident rows: IS -> K
    assert G.score64(z) == pytest.approx(K, rel=1e-9)
    st = G.softmax_stats64(z.astype(np.float32))
    assert st[0] == 3 * K and st[2:].sum() == pytest.approx(3 * K, rel=1e-12)
    w = np.random.default_rng(1).standard_normal((K, 4))
    f = np.random.default_rng(2).standard_normal((9, 4))
    assert G.inception_score64(f, w, np.zeros(K)) == pytest.approx(G.inception_score64(f, w), rel=1e-15)


def test_softmax_state_is_independent_of_the_cut():
    z = np.random.default_rng(3).standard_normal((5, 11)).astype(np.float32) * 9
    whole = G.softmax_stats64(z)
    cut = G.softmax_stats64(z[2:], G.softmax_stats64(z[:2]))
    assert np.array_equal(whole, cut)


def test_ema_restatement():
    e, w = np.float32([1.0, -2.0, 0.5]), np.float32([3.0, -2.0, 0.25])
    a = np.float32(1.0 - 0.9)
    got = G.ema64(e, w, a)
    assert got[1] == -2.0 and got[0] == pytest.approx(1.2, rel=1e-7) and got[2] == pytest.approx(0.475, rel=1e-7)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference alone meets the test's conditions; the clean emulation passes; the defects do not
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=G.SHAPES, ids=G.shape_id)
def case(request):
    N, M, d, k, seed = request.param
    x, q = G.make_inputs(N, M, d, seed)
    r2 = G.knn_radius64(x, k).astype(np.float32)
    return dict(x=x, q=q, k=k, r2=r2)


def test_reference_decides_and_has_both_outcomes(case):
    cls = G.classify_hits(case["q"], case["x"], case["r2"])
    print(f"hits {int((cls == 1).sum())}, misses {int((cls == 0).sum())}, undecided {int((cls < 0).sum())}")
    assert (cls < 0).mean() <= G.UNDECIDED_MAX
    assert (cls == 1).any() and (cls == 0).any()


@pytest.mark.parametrize("shift", [0.0, 1000.0])
def test_clean_chain_passes(case, shift):
    N, M = case["x"].shape[0], case["q"].shape[0]
    x, q = case["x"], case["q"]
    if shift:
        x, q = (x + np.float32(shift)).astype(np.float32), (q + np.float32(shift)).astype(np.float32)
    got = G.knn_radius32(x, case["k"])
    assert G.check_radii(got, x, case["k"]) is None
    ref = G.knn_radius64(x, case["k"])
    print(f"worst relative error of the unfused chain: {np.max(np.abs(got - ref) / ref):.3g} (bound {G.radius_bound(x.shape[1]):.3g})")
    msg, undecided = G.check_hits(G.hits32(q, x, got), q, x, got)
    assert msg is None and undecided <= G.UNDECIDED_MAX


def test_gram_form_is_rejected():
    N, M, d, k, seed = G.SHAPES[0]
    x, q = G.make_inputs(N, M, d, seed, shift=1000.0)
    bad = G.knn_radius32(x, k, gram=True)
    assert G.check_radii(bad, x, k) is not None
    ref = G.knn_radius64(x, k)
    print(f"Gram form at +1000: relative error {np.min(np.abs(bad - ref) / ref):.3g} .. {np.max(np.abs(bad - ref) / ref):.3g}")
    r2 = ref.astype(np.float32)
    msg, _ = G.check_hits(G.hits32(q, x, r2, gram=True), q, x, r2)
    assert msg is not None


def test_self_not_excluded_is_rejected(case):
    assert G.check_radii(G.knn_radius32(case["x"], case["k"], keep_self=True), case["x"], case["k"]) is not None


def test_off_by_one_is_rejected(case):
    assert G.check_radii(G.knn_radius32(case["x"], case["k"], off_by_one=True), case["x"], case["k"]) is not None


def test_strict_comparison_is_rejected_on_a_tie():
    x = np.array([[0, 0], [3, 4], [40, 0]], dtype=np.float32)           # r2 at k = 1: 25, 25, 37^2 + 16
    r2 = G.knn_radius64(x, 1).astype(np.float32)
    q = np.array([[-3, 4], [-30, -30]], dtype=np.float32)               # exactly 25 from x_0; far from all
    assert G.hits64(q, x, r2).tolist() == [1, 0]
    assert G.classify_hits(q, x, r2).tolist()[1] == 0
    assert G.hits32(q, x, r2).tolist() == [1, 0]
    assert G.hits32(q, x, r2, strict=True).tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the host interface
# ---------------------------------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    import transvae
    for name in ("evaluate_dit", "InceptionScore", "knn_radius", "manifold_hits", "precision_recall", "reference_statistics", "ParamEMA"):
        assert name in transvae.__all__ and hasattr(transvae, name), name
    assert inspect.signature(transvae.fit_dit).parameters["ema_decay"].default is None
    sig = inspect.signature(transvae.evaluate_dit).parameters
    want = dict(num_samples=10000, batch_size=128, steps=50, cfg_scale=1.0, metrics=("gfid", "is", "precision", "recall"), is_head=None, k=3,
                seed=0, labels=None, ema=None, transform="clip", max_features=10000, return_features=False)
    for name, default in want.items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    assert sig["fid_net"].kind is inspect.Parameter.KEYWORD_ONLY and sig["fid_net"].default is inspect.Parameter.empty
    assert list(sig)[:3] == ["vae", "dit", "reference"]
    assert inspect.signature(transvae.ParamEMA).parameters["decay"].default == 0.9999
    assert inspect.signature(transvae.knn_radius).parameters["k"].default == 3


def test_no_cpu_fallback():
    import transvae
    x = torch.rand(6, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.knn_radius(x, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.manifold_hits(x, x, torch.ones(6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.precision_recall(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.InceptionScore(torch.rand(5, 8)).update(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        transvae.ParamEMA([torch.nn.Parameter(torch.zeros(3))])
    dit = transvae.DiT(8, 2, 4, 64, 1, 5)
    ref = {"n": 4, "mean": torch.zeros(8), "cov": torch.eye(8), "features": torch.rand(6, 8)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transvae.evaluate_dit(None, dit, ref, fid_net=None, num_samples=8, metrics=("gfid",))


def test_argument_errors():
    import transvae
    x = torch.rand(6, 8)
    with pytest.raises(ValueError, match="k=9"):
        transvae.knn_radius(x, 9)
    with pytest.raises(ValueError, match="k=0"):
        transvae.knn_radius(x, 0)
    with pytest.raises(ValueError, match="at least 7"):
        transvae.knn_radius(x, 6)
    with pytest.raises(ValueError, match=r"x must be \[n, d\]"):
        transvae.knn_radius(torch.rand(6), 3)
    with pytest.raises(ValueError, match="columns"):
        transvae.manifold_hits(torch.rand(3, 7), x, torch.ones(6))
    with pytest.raises(ValueError, match="r2 must be"):
        transvae.manifold_hits(x, x, torch.ones(5))
    with pytest.raises(ValueError, match="weight must be"):
        transvae.InceptionScore(torch.rand(5))
    with pytest.raises(ValueError, match="bias must be"):
        transvae.InceptionScore(torch.rand(5, 8), torch.rand(4))
    with pytest.raises(ValueError, match="decay"):
        transvae.ParamEMA([torch.nn.Parameter(torch.zeros(3))], decay=1.5)
    dit = transvae.DiT(8, 2, 4, 64, 1, 5)
    with pytest.raises(ValueError, match="ema_decay"):
        transvae.fit_dit("nowhere", dit, epochs=1, batch_size=1, lr=1e-3, ema_decay=2.0)
    ref = {"n": 4, "mean": torch.zeros(8), "cov": torch.eye(8), "features": torch.rand(6, 8)}
    head = transvae.InceptionScore(torch.rand(5, 8))
    ev = lambda **kw: transvae.evaluate_dit(None, dit, kw.pop("reference", ref), fid_net=None, **kw)
    with pytest.raises(ValueError, match=r"metrics.*\['kid'\]"):
        ev(metrics=("gfid", "kid"))
    with pytest.raises(ValueError, match="metrics"):
        ev(metrics=())
    with pytest.raises(ValueError, match="is_head"):
        ev(metrics=("is",))
    with pytest.raises(ValueError, match="num_samples=1 "):
        ev(num_samples=1, metrics=("gfid",))
    with pytest.raises(ValueError, match="num_samples=3 "):
        ev(num_samples=3, metrics=("precision",), k=3)
    with pytest.raises(ValueError, match="transform"):
        ev(transform="tanh", metrics=("gfid",))
    with pytest.raises(ValueError, match="k=0"):
        ev(k=0, metrics=("gfid",))
    with pytest.raises(ValueError, match="reference holds no features"):
        ev(reference={"n": 4, "mean": torch.zeros(8), "cov": torch.eye(8)}, metrics=("recall",), num_samples=8)
    with pytest.raises(ValueError, match="reference must be"):
        ev(reference={"mean": torch.zeros(8)}, metrics=("gfid",), is_head=head)
    with pytest.raises(ValueError, match="reference holds no features"):                    # a numpy array, too few rows / not a matrix
        ev(reference=dict(ref, features=np.zeros((2, 8), dtype=np.float32)), metrics=("recall",), num_samples=8)
    with pytest.raises(ValueError, match="reference holds no features"):
        ev(reference=dict(ref, features=np.zeros(8, dtype=np.float32)), metrics=("precision",), num_samples=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                              # a well-formed numpy reference gets as far as the device check
        ev(reference=dict(ref, features=np.zeros((6, 8), dtype=np.float32)), metrics=("recall",), num_samples=8)


def test_reference_dict_round_trips_through_torch_save(tmp_path):
    from transvae.evaluate_dit import _load_reference
    ref = {"n": 4, "mean": torch.zeros(8, dtype=torch.float64), "cov": torch.eye(8, dtype=torch.float64), "features": torch.rand(6, 8), "is": 1.5}
    path = str(tmp_path / "ref.pt")
    torch.save(ref, path)
    back = _load_reference(path)
    assert back["n"] == 4 and back["is"] == 1.5 and torch.equal(back["features"], ref["features"]) and torch.equal(back["cov"], ref["cov"])


def test_frechet_row_form_is_an_independent_reference():
    """gen_restatement.frechet_rows64 (the nuclear-norm form, numpy alone) equals fid_restatement.frechet_numpy where that is defined
    (n > d) within its 1e-8 x trace, gives 0 for a set against itself at n <= d, and there frechet_numpy's own deviation stays inside
    frechet_null_space_noise while the package's frechet_from_statistics stays at 1e-8 x trace"""
    import fid_restatement as FR
    from transvae.metrics_fid import frechet_from_statistics
    g = np.random.default_rng(5)
    a, b = g.standard_normal((200, 16)) * 2.0 + 1.0, g.standard_normal((150, 16)) * g.uniform(0.5, 3.0, 16)
    trace = np.trace(np.cov(a, rowvar=False))
    assert abs(G.frechet_rows64(a, b) - FR.frechet_numpy(a, b)) <= 1e-8 * trace
    x, q = G.make_inputs(48, 48, 2048, 0)
    trace = np.trace(np.cov(x.astype(np.float64), rowvar=False))
    assert abs(G.frechet_rows64(q, q)) <= 1e-12 * trace
    rows, eig = G.frechet_rows64(x, q), FR.frechet_numpy(x, q)
    f1, f2 = x.astype(np.float64), q.astype(np.float64)
    pkg = frechet_from_statistics(f1.mean(0), np.cov(f1, rowvar=False), f2.mean(0), np.cov(f2, rowvar=False))
    print(f"48 x 2048: row form {rows!r}, frechet_numpy off {eig - rows:.3g} (allowed {G.frechet_null_space_noise(x, q):.3g}), "
          f"frechet_from_statistics off {pkg - rows:.3g} (allowed {1e-8 * trace:.3g})")
    assert abs(eig - rows) <= G.frechet_null_space_noise(x, q)
    assert abs(pkg - rows) <= 1e-8 * trace
