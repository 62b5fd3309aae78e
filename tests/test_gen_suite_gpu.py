"""sFID, KID, density / coverage and the Inception Score over splits on the device: tv_ball_counts, tv_poly_kernel_sums and
tv_spatial_rows through the C ABI against fp64 under DESIGN.md section 3.1 row S, their exact cases, bit-reproducibility and both
load paths; the spatial tap of InceptionFeatures against the fp32 restatement; InceptionScore(split_size=...); evaluate_dit with
ALL_METRICS end to end."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_restatement as FR
import gen_restatement as G
import gen_suite_restatement as GS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 1.0e30           # in the columns past d of a strided input: read by mistake, it wrecks every distance and every product


def _L():
    from transvae.hip import _lib as L
    return L


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def strided(a, ld):
    """the rows of `a` in a device buffer of row stride ld"""
    n, d = a.shape
    buf = torch.full((n, ld), PAD, dtype=torch.float32, device=DEV)
    buf[:, :d] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return buf


def counts_abi(q, ldq, x, ldx, r2, radius_of):
    """tv_ball_counts through the C ABI, one sentinel past the output"""
    L = _L()
    (M, d), N = q.shape, x.shape[0]
    qb, xb = strided(q, ldq), strided(x, ldx)
    rb = torch.from_numpy(np.asarray(r2, dtype=np.float32)).to(DEV)
    assert rb.shape[0] == (N if radius_of == "data" else M)
    out = torch.full((M + 1,), 77, dtype=torch.int32, device=DEV)
    scratch = torch.empty(32 * M, dtype=torch.int32, device=DEV)
    L.check(L.load().tv_ball_counts(_p(qb), M, ldq, _p(xb), N, ldx, _p(rb), d, 0 if radius_of == "data" else 1, _p(out), _p(scratch),
                                    _stream()), "tv_ball_counts")
    assert int(out[-1]) == 77, "wrote past count"
    return out[:-1].cpu().numpy()


def hits_abi(q, ldq, x, ldx, r2):
    L = _L()
    (M, d), N = q.shape, x.shape[0]
    qb, xb = strided(q, ldq), strided(x, ldx)
    rb = torch.from_numpy(np.asarray(r2, dtype=np.float32)).to(DEV)
    out = torch.empty(M, dtype=torch.int32, device=DEV)
    scratch = torch.empty(32 * M, dtype=torch.int32, device=DEV)
    L.check(L.load().tv_manifold_hits(_p(qb), M, ldq, _p(xb), N, ldx, _p(rb), d, _p(out), _p(scratch), _stream()), "tv_manifold_hits")
    return out.cpu().numpy()


def poly_abi(a, lda, ia, b, ldb, ib, gamma, coef0, skip):
    """tv_poly_kernel_sums through the C ABI, one sentinel past the sums"""
    L = _L()
    lib = L.load()
    d = a.shape[1]
    S, m = ia.shape
    ab, bb = strided(a, lda), strided(b, ldb)
    iad, ibd = torch.from_numpy(np.ascontiguousarray(ia, dtype=np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(ib, dtype=np.int32)).to(DEV)
    out = torch.full((S + 1,), 7.5, dtype=torch.float64, device=DEV)
    need = lib.tv_poly_kernel_scratch_doubles(m, S)
    assert need == ((m + 63) // 64) ** 2 * S
    scratch = torch.empty(need, dtype=torch.float64, device=DEV)
    L.check(lib.tv_poly_kernel_sums(_p(ab), lda, _p(iad), _p(bb), ldb, _p(ibd), m, S, d, float(gamma), float(coef0), int(skip), _p(out),
                                    _p(scratch), _stream()), "tv_poly_kernel_sums")
    assert float(out[-1]) == 7.5, "wrote past the sums"
    return out[:-1].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# tv_ball_counts
# ---------------------------------------------------------------------------------------------------------------------------
# per shape: the row stride of the first run (odd at d = 2048: the scalar path; 40 at d = 37: float4 loads with a ragged last group),
# the stride of the other load path, and a sub-range of queries
LAYOUT = {G.SHAPES[0]: (2048 + 3, 2048, (64, 6)), G.SHAPES[1]: (37 + 3, 37, (3, 5)), G.SHAPES[2]: (64, 67, (70, 150)), G.SHAPES[3]: (2048, 2049, (1, 3))}


@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["plain", "plus1000"])
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.shape_id)
def test_ball_counts_against_fp64(shape, shift):
    import transvae
    N, M, d, k, seed = shape
    ld, ld_other, (i0, m) = LAYOUT[shape]
    x, q = G.make_inputs(N, M, d, seed, shift=shift)
    r2 = G.knn_radius64(x, k).astype(np.float32)
    for qq, xx, of in ((q, x, "data"), (x, q, "query")):
        got = counts_abi(qq, ld, xx, ld, r2, of)
        msg, undecided = GS.check_counts(got, qq, xx, r2, of)
        print(f"counts {G.shape_id(shape)} shift {shift} radius per {of}: total {int(got.sum())}, fp64 {int(GS.counts64(qq, xx, r2, of).sum())}, "
              f"undecided share of pairs {undecided:.3g}")
        assert undecided <= GS.UNDECIDED_PAIRS_MAX
        assert msg is None, msg
        assert np.array_equal(counts_abi(qq, ld_other, xx, ld_other, r2, of), got), "float4 and scalar loads give other counts"
        lo = min(i0, qq.shape[0] - 1)
        n = min(m, qq.shape[0] - lo)
        part = counts_abi(qq[lo:lo + n], ld, xx, ld, r2 if of == "data" else r2[lo:lo + n], of)
        assert np.array_equal(part, got[lo:lo + n]), "a sub-range of queries gives other counts than the whole range"
        if of == "data":
            assert np.array_equal((got > 0).astype(np.int32), hits_abi(qq, ld, xx, ld, r2)), "count > 0 is not tv_manifold_hits"
    # density / coverage with the device's own radii: the decided pairs fix both up to the undecided ones
    xd, qd = torch.from_numpy(x).to(DEV), torch.from_numpy(q).to(DEV)
    rdev = transvae.knn_radius(xd, k).cpu().numpy()
    dc = transvae.density_coverage(xd, qd, k)
    assert sorted(dc) == ["coverage", "density"]
    inside, und = GS.classify_pairs(q, x, rdev, "data")
    lo, hi = inside.sum() / (k * M), (inside.sum() + und.sum()) / (k * M)
    cin, cund = GS.classify_pairs(x, q, rdev, "query")
    covered, open_ = cin.any(1), ~cin.any(1) & cund.any(1)
    print(f"density {dc['density']!r} in [{lo!r}, {hi!r}]; coverage {dc['coverage']!r}, decided {covered.mean()!r}, undecided points {int(open_.sum())}; "
          f"fp64 {GS.density_coverage64(x, q, k)}")
    assert open_.mean() <= GS.UNDECIDED_COVERAGE_MAX
    assert lo * (1 - 1e-12) <= dc["density"] <= hi * (1 + 1e-12)
    assert covered.sum() <= round(dc["coverage"] * N) <= covered.sum() + open_.sum()
    assert dc["density"] > 0 and 0 < dc["coverage"] <= 1


def test_ball_counts_exact_cases():
    g = np.random.default_rng(11)
    d = 37
    x = g.integers(-63, 64, size=(150, d)).astype(np.float32)        # |v| < 64: every D < 37 * 127^2 < 2^24 is exact in fp32
    x[17] = x[3]                                                      # a duplicated point
    q = np.concatenate([x[:5] + np.float32(1), g.integers(-63, 64, size=(40, d)).astype(np.float32)], 0)
    for k in (1, 3, 8):
        r2 = G.knn_radius64(x, k).astype(np.float32)
        assert np.array_equal(r2.astype(np.float64), G.knn_radius64(x, k))
        assert np.array_equal(counts_abi(q, d, x, d + 1, r2, "data"), GS.counts64(q, x, r2, "data")), k
        assert np.array_equal(counts_abi(x, d + 3, q, d, r2, "query"), GS.counts64(x, q, r2, "query")), k
        assert np.array_equal(counts_abi(x, d, x, d, r2, "query"), GS.counts64(x, x, r2, "query")), k       # itself and k others at least
    # a tie D == r2 counts; just outside does not
    t = np.zeros((3, d), dtype=np.float32)
    t[1, :2], t[2, 0] = (3, 4), 40
    r2 = np.float32([25.0, 25.0, 37.0 ** 2 + 16.0])
    qq = np.zeros((3, d), dtype=np.float32)
    qq[0, :2], qq[1, :2], qq[2, :3] = (-3, 4), (-30, -30), (-3, 4, 1)
    assert counts_abi(qq, d, t, d, r2, "data").tolist() == [1, 0, 0]
    assert counts_abi(qq, d, t, d, np.float32([25.0, 1.0e6, 25.0]), "query").tolist() == [1, 3, 0]


def test_argument_errors():
    L = _L()
    lib = L.load()
    x = torch.zeros(8, 8, device=DEV)
    r = torch.zeros(8, device=DEV)
    h = torch.zeros(8, dtype=torch.int32, device=DEV)
    s = torch.zeros(64, dtype=torch.float64, device=DEV)
    for args, word in (((_p(x), 8, 8, _p(x), 8, 8, _p(r), 8, 2, _p(h), None, None), "radius_of=2"),
                       ((_p(x), 8, 8, _p(x), 8, 8, _p(r), 0, 0, _p(h), None, None), "d=0"),
                       ((_p(x), 8, 4, _p(x), 8, 8, _p(r), 8, 1, _p(h), None, None), "ldq=4"),
                       ((_p(x), 0, 8, _p(x), 8, 8, _p(r), 8, 1, _p(h), None, None), "M=0")):
        assert lib.tv_ball_counts(*args) != 0 and word in lib.tv_last_error().decode(), word
    for args, word in (((_p(x), 8, _p(h), _p(x), 8, _p(h), 0, 1, 8, 1.0, 1.0, 0, _p(s), _p(s), None), "m=0"),
                       ((_p(x), 8, _p(h), _p(x), 8, _p(h), 4, 0, 8, 1.0, 1.0, 0, _p(s), _p(s), None), "S=0"),
                       ((_p(x), 8, _p(h), _p(x), 8, _p(h), 4, 1, 9000, 1.0, 1.0, 0, _p(s), _p(s), None), "d=9000"),
                       ((_p(x), 8, _p(h), _p(x), 4, _p(h), 4, 1, 8, 1.0, 1.0, 0, _p(s), _p(s), None), "ldb=4"),
                       ((_p(x), 8, _p(h), _p(x), 8, _p(h), 4, 1, 8, 1.0, 1.0, 0, _p(s), None, None), "scratch")):
        assert lib.tv_poly_kernel_sums(*args) != 0 and word in lib.tv_last_error().decode(), word
    assert lib.tv_poly_kernel_scratch_doubles(0, 1) == -1 and lib.tv_poly_kernel_scratch_doubles(65, 3) == 12
    xb = torch.zeros(2, 4, 16, dtype=torch.bfloat16, device=DEV)
    for args, word in (((_p(xb), 2, 4, 16, 16, 12, 7, _p(x), 32, None), "c0=12"), ((_p(xb), 2, 4, 16, 16, 0, 7, _p(x), 27, None), "ldo=27"),
                       ((_p(xb), 2, 4, 16, 8, 0, 7, _p(x), 32, None), "ldc=8")):
        assert lib.tv_spatial_rows(*args) != 0 and word in lib.tv_last_error().decode(), word


# ---------------------------------------------------------------------------------------------------------------------------
# tv_poly_kernel_sums and KID
# ---------------------------------------------------------------------------------------------------------------------------
def _subsets(n_a, n_b, S, m, seed, repeat=True):
    g = np.random.default_rng(seed)
    ia = np.stack([g.choice(n_a, m, replace=False) for _ in range(S)]).astype(np.int32)
    ib = np.stack([g.choice(n_b, m, replace=False) for _ in range(S)]).astype(np.int32)
    if repeat and m > 1:
        ib[1, 1] = ib[1, 0]                                              # a row met twice on the cross side
    return ia, ib


# (rows of a, rows of b, d), the row stride (39: odd, the scalar path) and m (none a multiple of 64; 257 is four tiles and one row)
POLY_CASES = (((130, 70, 2048), 2048, 70), ((65, 9, 37), 39, 9), ((257, 257, 64), 64, 257))


@pytest.mark.parametrize("case", POLY_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_poly_kernel_sums_against_fp64(case):
    (N, M, d), ld, m = case
    a, b = GS.poly_inputs(N, M, d, 5)
    ia, ib = _subsets(N, M, 3, m, 7)
    gamma = 1.0 / d
    for x, ix, y, iy, skip, name in ((a, ia, a, ia, True, "Sxx"), (b, ib, b, ib, True, "Syy"), (a, ia, b, ib, False, "Sxy")):
        got = poly_abi(x, ld, ix, y, ld, iy, gamma, 1.0, skip)
        ref, bound = GS.poly_sums64(x, ix, y, iy, gamma, 1.0, skip), GS.poly_sums_bound(x, ix, y, iy, gamma, 1.0, skip)
        err = np.abs(got - ref)
        print(f"{name} {N}x{M}x{d} m {m}: worst relative error {np.max(err / np.abs(ref)):.3g}, worst error / bound {np.max(err / bound):.3g}")
        assert (err <= bound).all(), (name, err, bound)
        kept = GS.poly_sums64(x, ix, y, iy, gamma, 1.0, False)
        if skip:
            assert (np.abs(got - kept) > bound).all(), "the pairs at equal position were kept"
        assert np.array_equal(poly_abi(x, ld, ix, y, ld, iy, gamma, 1.0, skip), got), "two runs differ"
        other = ld + 1 if ld % 4 == 0 else (d + 3) // 4 * 4
        assert np.array_equal(poly_abi(x, other, ix, y, other, iy, gamma, 1.0, skip), got), "float4 and scalar loads give other bits"


@pytest.mark.parametrize("m", [1, 63, 64, 65, 150])
def test_poly_kernel_sums_exact_cases(m):
    g = np.random.default_rng(13)
    d = 37
    x = g.integers(-3, 4, size=(150, d)).astype(np.float32)          # |dot| <= 333, t <= 334, k <= 334^3 < 2^26: every step exact
    y = g.integers(-3, 4, size=(150, d)).astype(np.float32)
    ia, ib = _subsets(150, 150, 3, m, 100 + m)
    for ld in (d, 40):
        for args, name in (((x, ia, x, ia), "Sxx"), ((y, ib, y, ib), "Syy"), ((x, ia, y, ib), "Sxy")):
            skip = name != "Sxy"
            ref = GS.poly_sums64(*args, 1.0, 1.0, skip)
            got = poly_abi(args[0], ld, args[1], args[2], ld, args[3], 1.0, 1.0, skip)
            assert np.array_equal(got, ref), (name, m, ld, got, ref)
    if m == 1:
        assert poly_abi(x, d, ia, x, d, ia, 1.0, 1.0, True).tolist() == [0.0, 0.0, 0.0]


def test_kernel_inception_distance():
    """against the fp64 restatement on the same drawn subsets within the propagated bound; and a set against itself.

    The unbiased estimate of a subset against itself is not 0: with Sxx = Syy the off-diagonal sum and Sxy that plus the diagonal it
    is (2 / m) (mean off-diagonal k - mean diagonal k), of order 1 / m (gen_suite_restatement.self_kid64).  What rounding allows is
    checked against that closed form at the same bound, and the two skipped sums of equal operands must be the same bits."""
    import transvae
    N, M, d = 130, 70, 2048
    real, fake = GS.poly_inputs(N, M, d, 5)
    rd, fd = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV)
    got = transvae.kernel_inception_distance(rd, fd, subsets=5, subset_size=50, seed=2)
    assert sorted(got) == ["kid", "kid_std"]
    ia, ib = GS.draw_subsets(N, M, 5, 50, 2)
    mean, std, _ = GS.kid64(real, fake, ia, ib)
    bm, bs = GS.kid_bound(real, fake, ia, ib)
    print(f"KID {got['kid']!r} (fp64 {mean!r}, off {got['kid'] - mean:.3g}, allowed {bm:.3g}); std {got['kid_std']!r} (fp64 {std!r}, "
          f"off {got['kid_std'] - std:.3g}, allowed {bs:.3g})")
    assert abs(got["kid"] - mean) <= bm and abs(got["kid_std"] - std) <= bs
    assert abs(GS.kid64(real, fake, ia, ib, biased=True)[0] - got["kid"]) > bm and abs(GS.kid64(real, fake, ia, ib, keep_diagonal=True)[0] - got["kid"]) > bm
    assert transvae.kernel_inception_distance(rd, fd, subsets=5, subset_size=50, seed=2) == got
    clamped = transvae.kernel_inception_distance(rd, fd, subsets=2, subset_size=1000, seed=0)      # m = 70, every fake row in each subset
    ia, ib = GS.draw_subsets(N, M, 2, 1000, 0)
    assert ia.shape == (2, 70) and abs(clamped["kid"] - GS.kid64(real, fake, ia, ib)[0]) <= GS.kid_bound(real, fake, ia, ib)[0]
    # a set against itself
    own = transvae.kernel_inception_distance(rd, rd, subsets=4, subset_size=60, seed=1)
    ia, ib = GS.draw_subsets(N, N, 4, 60, 1)
    assert abs(own["kid"] - GS.kid64(real, real, ia, ib)[0]) <= GS.kid_bound(real, real, ia, ib)[0]
    idx = torch.from_numpy(ia).to(DEV)
    sxx = transvae.poly_kernel_sums(rd, idx, rd, idx, 1.0 / d, 1.0, True)
    syy = transvae.poly_kernel_sums(rd.clone(), idx.clone(), rd, idx, 1.0 / d, 1.0, True)
    sxy = transvae.poly_kernel_sums(rd, idx, rd, idx, 1.0 / d, 1.0, False)
    assert torch.equal(sxx, syy) and sxx.dtype == torch.float64
    vals = GS.mmd2_from_sums(sxx.cpu().numpy(), syy.cpu().numpy(), sxy.cpu().numpy(), 60)
    want = GS.self_kid64(real, ia)
    bound = GS.kid_bound(real, real, ia, ia)[1]
    print(f"a subset against itself: {vals}, closed form {want}, allowed {bound:.3g}")
    assert (np.abs(vals - want) <= bound).all() and (want < 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the spatial tap
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,ldc,c0,nc,ldo", [(3, 5, 4, 20, 24, 3, 7, 149), (2, 17, 17, 768, 768, 0, 7, 2048), (1, 3, 3, 8, 8, 7, 1, 9)])
def test_spatial_rows(B, H, W, C, ldc, c0, nc, ldo):
    L = _L()
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, H, W, ldc, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.full((B * ldo + 1,), 7.5, dtype=torch.float32, device=DEV)
    L.check(L.load().tv_spatial_rows(_p(x), B, H * W, C, ldc, c0, nc, _p(out), ldo, _stream()), "tv_spatial_rows")
    assert float(out[-1]) == 7.5, "wrote past the rows"
    got = out[:-1].view(B, ldo)
    want = x[..., c0:c0 + nc].float().reshape(B, H * W * nc)
    assert torch.equal(got[:, :H * W * nc], want)
    assert bool((got[:, H * W * nc:] == 0).all()) and not bool(torch.signbit(got[:, H * W * nc:]).any())


@pytest.fixture(scope="module")
def net():
    from transvae import InceptionFeatures
    return InceptionFeatures().load_fid_state_dict(FR.plain_state_dict()).to(DEV)


def test_spatial_features_against_restatement(net):
    from transvae.metrics_fid import SPATIAL_DIM, SPATIAL_LD
    x = GS.spatial_case_images()
    ref = GS.run_spatial(x, FR.plain_state_dict())
    with open(GS.GOLDEN_SPATIAL) as f:
        dev16 = json.load(f)["spatial"]
    xd = x.to(DEV)
    pool, rows = net.features(xd, spatial=True)
    assert tuple(pool.shape) == (4, 2048) and tuple(rows.shape) == (4, SPATIAL_LD) and rows.dtype == torch.float32
    assert tuple(ref.shape) == (4, SPATIAL_DIM)
    err = FR.rel_l2(rows[:, :SPATIAL_DIM].cpu(), ref)
    print(f"spatial tap: rel-L2 {err:.4g}, restatement's own autocast deviation {dev16:.4g}, ratio {err / dev16:.3f}")
    assert err <= max(1e-2, 1.25 * dev16), (err, dev16)
    assert bool((rows[:, SPATIAL_DIM:] == 0).all())
    assert torch.equal(pool, net.features(xd)), "asking for the spatial rows changed the pool3 features"
    both_pool, both_rows = net.features(xd[:1], xd[1:], clip=True, spatial=True)
    assert torch.equal(both_rows, rows) and torch.equal(both_pool, pool)                  # (the images lie in [0, 1]: clip changes nothing)
    net.MAX_BATCH = 3                                                                      # the chunked path: passes of 3 and 1 images
    try:
        cp, cr = net.features(xd, spatial=True)
        c2 = net.features(xd[:2], xd[2:], spatial=True)
    finally:
        del net.MAX_BATCH
    assert torch.equal(cp, pool) and torch.equal(cr, rows) and torch.equal(c2[0], pool) and torch.equal(c2[1], rows)


def test_sfid_statistics_match_numpy_on_2023_columns():
    from transvae import FrechetDistance
    from transvae.metrics_fid import SPATIAL_DIM, SPATIAL_LD, frechet_from_statistics
    g = torch.Generator().manual_seed(12)
    n = 64
    rows = [torch.zeros(n, SPATIAL_LD) for _ in range(2)]
    rows[0][:, :SPATIAL_DIM] = torch.relu(torch.randn(n, SPATIAL_DIM, generator=g) + 0.3)
    rows[1][:, :SPATIAL_DIM] = torch.relu(1.2 * torch.randn(n, SPATIAL_DIM, generator=g) + 0.5)
    fd = FrechetDistance(SPATIAL_LD)
    fd.update(rows[0][:40].to(DEV), rows[1][:7].to(DEV))
    fd.update(rows[0][40:].to(DEV), rows[1][7:].to(DEV))
    stats = []
    for side in (0, 1):
        cnt, mu, cov = fd.statistics(side)
        x64 = rows[side][:, :SPATIAL_DIM].numpy().astype(np.float64)
        mu_ref, cov_ref = x64.mean(0), np.cov(x64, rowvar=False)
        assert cnt == n and not mu[SPATIAL_DIM:].any() and not cov[SPATIAL_DIM:].any() and not cov[:, SPATIAL_DIM:].any()
        mu, cov = mu[:SPATIAL_DIM], cov[:SPATIAL_DIM, :SPATIAL_DIM]
        e_mu, e_cov = np.linalg.norm(mu - mu_ref) / np.linalg.norm(mu_ref), np.linalg.norm(cov - cov_ref) / np.linalg.norm(cov_ref)
        print(f"side {side}: mean rel {e_mu:.3g}, cov rel Frobenius {e_cov:.3g}")
        assert e_mu <= 1e-10 and e_cov <= 1e-10
        stats += [mu, cov]
    trace = float(np.trace(stats[1]))
    want = G.frechet_rows64(rows[0][:, :SPATIAL_DIM].numpy(), rows[1][:, :SPATIAL_DIM].numpy())
    got = frechet_from_statistics(*stats)
    print(f"sFID of 64 rows: {got!r}, row form {want!r}, allowed {1e-8 * max(1.0, trace):.3g}")
    assert abs(got - want) <= 1e-8 * max(1.0, trace)
    assert abs(got - fd.compute()) <= 1e-8 * max(1.0, trace), "the zero columns add to the distance"


# ---------------------------------------------------------------------------------------------------------------------------
# Inception Score over splits
# ---------------------------------------------------------------------------------------------------------------------------
def test_inception_score_over_splits():
    import transvae
    L = _L()
    K = 16
    z = (np.random.default_rng(21).standard_normal((37, K)) * 3).astype(np.float32)
    zd = torch.from_numpy(z).to(DEV)
    w = torch.eye(K)                    # an identity head: the logits are the rows themselves, whatever GEMM computes them
    runs = []
    for cuts in ((37,), (5, 32), (10, 10, 10, 7)):
        head = transvae.InceptionScore(w, split_size=10).to(DEV)
        b0 = 0
        for nb in cuts:
            head.update(zd[b0:b0 + nb])
            b0 += nb
        assert head.n == 37 and tuple(head.state().shape) == (4, 2 + K)
        runs.append(head)
    assert all(torch.equal(r.state(), runs[0].state()) for r in runs[1:]), "the per-split states depend on the batching"
    direct = []
    for a, b in GS.split_bounds(37, 10):
        st = torch.zeros(2 + K, dtype=torch.float64, device=DEV)
        scratch = torch.empty((b - a) * (K + 1), dtype=torch.float64, device=DEV)
        L.check(L.load().tv_softmax_stats(_p(zd[a:]), b - a, K, K, _p(st), _p(scratch), _stream()), "tv_softmax_stats")
        direct.append(st)
    assert torch.equal(torch.stack(direct), runs[0].state()), "a split's state is not tv_softmax_stats of its rows"
    got = runs[0].scores()
    want = GS.split_scores64(z, 10)
    slack = np.array([GS.score_bound_from_state(z[a:b]) for a, b in GS.split_bounds(37, 10)]) + 4 * G.U64
    print(f"per-split scores {got}, fp64 {want}, allowed on the log {slack}")
    assert (np.abs(np.log(got) - np.log(want)) <= slack).all()
    assert abs(runs[0].compute() - want.mean()) <= float((want * np.expm1(slack)).mean())
    assert abs(runs[0].compute_std() - want.std()) <= float((want * np.expm1(slack)).max())
    assert runs[0].compute_std() > 0
    # without a split size: today's single state, bit for bit
    plain = transvae.InceptionScore(w).to(DEV)
    plain.update(zd[:5])
    plain.update(zd[5:])
    st = torch.zeros(2 + K, dtype=torch.float64, device=DEV)
    scratch = torch.empty(37 * (K + 1), dtype=torch.float64, device=DEV)
    L.check(L.load().tv_softmax_stats(_p(zd), 37, K, K, _p(st), _p(scratch), _stream()), "tv_softmax_stats")
    assert tuple(plain.state().shape) == (2 + K,) and torch.equal(plain.state(), st)
    assert plain.compute() == transvae.metrics_gen.score_from_state(st.cpu().numpy()) and plain.compute_std() == 0.0
    assert plain.compute() != pytest.approx(runs[0].compute(), rel=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluate_dit end to end (the tiny fixtures of tests/test_gen_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
class StubVAE:
    """decode: the first three latent channels, up-sampled 4x: [B, 4, 8, 8] -> [B, 3, 32, 32]"""

    def decode(self, lat):
        return F.interpolate(0.25 * lat[:, :3].float() + 0.5, scale_factor=4, mode="nearest")


@pytest.fixture(scope="module")
def dit():
    import transvae
    g = torch.Generator().manual_seed(1)
    m = transvae.DiT(8, 2, 4, 64, 1, 5, generator=g)
    with torch.no_grad():       # adaLN-Zero starts the final layer and every modulation at zero, which hides t and the label: fill them
        for p in m.parameters():
            if not bool(p.any()):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def head():
    import transvae
    g = torch.Generator().manual_seed(6)
    return transvae.InceptionScore(torch.randn(16, 2048, generator=g) * 0.02, torch.randn(16, generator=g) * 0.1).to(DEV)


@pytest.fixture(scope="module")
def real_images():
    return FR.smooth_images(48, 32, 32, 123)


@pytest.fixture(scope="module")
def reference(net, head, real_images):
    import transvae
    return transvae.reference_statistics([(real_images[:24], None), (real_images[24:], None)], net, is_head=head, spatial=True)


KW = dict(num_samples=48, batch_size=16, steps=2, cfg_scale=1.5, return_features=True)
KID = dict(kid_subsets=4, kid_subset_size=20, kid_seed=3)


@pytest.fixture(scope="module")
def default_run(dit, net, head, reference):
    import transvae
    return transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, is_head=head, **KW)


@pytest.fixture(scope="module")
def full_run(dit, net, head, reference, default_run):
    import transvae
    from transvae.evaluate_dit import ALL_METRICS
    return transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, is_head=head, metrics=ALL_METRICS, **KID, **KW)


def test_reference_statistics_spatial(reference, net, head, real_images):
    import transvae
    from transvae.metrics_fid import SPATIAL_DIM
    assert reference["spatial_n"] == 48 and tuple(reference["spatial_mean"].shape) == (SPATIAL_DIM,)
    assert tuple(reference["spatial_cov"].shape) == (SPATIAL_DIM, SPATIAL_DIM) and reference["spatial_cov"].dtype == torch.float64
    _, rows = net.features(real_images.to(DEV), clip=True, spatial=True)
    r64 = rows[:, :SPATIAL_DIM].cpu().numpy().astype(np.float64)
    assert np.allclose(reference["spatial_mean"].numpy(), r64.mean(0), rtol=1e-12, atol=1e-14)
    assert np.allclose(reference["spatial_cov"].numpy(), np.cov(r64, rowvar=False), rtol=1e-9, atol=1e-13)
    plain = transvae.reference_statistics([(real_images[:24], None), (real_images[24:], None)], net, is_head=head)
    assert sorted(plain) == ["cov", "features", "is", "mean", "n"] and sorted(set(reference) - set(plain)) == ["spatial_cov", "spatial_mean", "spatial_n"]
    for key in plain:
        same = plain[key] == reference[key] if not torch.is_tensor(plain[key]) else torch.equal(plain[key], reference[key])
        assert same, f"asking for the spatial statistics changed {key!r}"


def test_default_call_is_unchanged(default_run, full_run, reference, head):
    out = default_run
    assert sorted(out) == ["features", "gfid", "is", "n", "precision", "recall"] and out["n"] == 48
    f = out["features"].cpu().numpy()
    want = {"gfid": G.frechet_rows64(reference["features"].numpy(), f),
            "is": G.inception_score64(f.astype(np.float64), head.weight.cpu().numpy(), head.bias.cpu().numpy())}
    want.update(G.precision_recall64(reference["features"].numpy(), f, 3))
    for m, v in want.items():
        assert out[m] == pytest.approx(v, rel=1e-6), m
    # the same seed with every metric switched on: the four default values come out again (to the tolerance
    # tests/test_gen_gpu.py holds a second run to)
    for m in ("gfid", "is", "precision", "recall"):
        assert full_run[m] == pytest.approx(out[m], rel=1e-6), m


def test_evaluate_dit_all_metrics_against_the_restatement(full_run, reference, net, real_images):
    from transvae.metrics_fid import SPATIAL_DIM, SPATIAL_LD
    out = full_run
    assert sorted(out) == ["coverage", "density", "features", "gfid", "is", "kid", "kid_std", "n", "precision", "recall", "sfid", "spatial"]
    rows = out["spatial"]
    assert tuple(rows.shape) == (48, SPATIAL_LD) and rows.is_cuda and rows.dtype == torch.float32 and bool((rows[:, SPATIAL_DIM:] == 0).all())
    assert all(np.isfinite(out[m]) for m in ("sfid", "kid", "kid_std", "density", "coverage"))
    real, fake = reference["features"].numpy(), out["features"].cpu().numpy()
    # sFID: numpy alone, from the rows of both sides
    _, real_rows = net.features(real_images.to(DEV), clip=True, spatial=True)
    a, b = real_rows[:, :SPATIAL_DIM].cpu().numpy(), rows[:, :SPATIAL_DIM].cpu().numpy()
    trace = float(np.trace(reference["spatial_cov"].numpy()))
    want = G.frechet_rows64(a, b)
    print(f"sfid {out['sfid']!r}: row form {want!r} (off {out['sfid'] - want:.3g}, allowed {1e-8 * max(1.0, trace):.3g}), trace {trace:.6g}")
    assert abs(out["sfid"] - want) <= 1e-8 * max(1.0, trace) and out["sfid"] > 0
    # KID on the package's draw
    ia, ib = GS.draw_subsets(48, 48, KID["kid_subsets"], KID["kid_subset_size"], KID["kid_seed"])
    mean, std, _ = GS.kid64(real, fake, ia, ib)
    bm, bs = GS.kid_bound(real, fake, ia, ib)
    print(f"kid {out['kid']!r} (fp64 {mean!r}, allowed {bm:.3g}), kid_std {out['kid_std']!r} (fp64 {std!r}, allowed {bs:.3g})")
    assert abs(out["kid"] - mean) <= bm and abs(out["kid_std"] - std) <= bs
    # density / coverage, k = 5: the decided pairs fix both up to the undecided ones (radii: fp64 within (d + 2) u of the device's)
    import transvae
    rdev = transvae.knn_radius(torch.from_numpy(real).to(DEV), 5).cpu().numpy()
    assert G.check_radii(rdev, real, 5) is None
    inside, und = GS.classify_pairs(fake, real, rdev, "data")
    cin, cund = GS.classify_pairs(real, fake, rdev, "query")
    lo, hi = inside.sum() / (5 * 48), (inside.sum() + und.sum()) / (5 * 48)
    covered, open_ = cin.any(1), ~cin.any(1) & cund.any(1)
    print(f"density {out['density']!r} in [{lo!r}, {hi!r}], coverage {out['coverage']!r} with {int(covered.sum())} decided and {int(open_.sum())} "
          f"undecided of 48; fp64 {GS.density_coverage64(real, fake, 5)}")
    assert lo * (1 - 1e-12) <= out["density"] <= hi * (1 + 1e-12)
    assert covered.sum() <= round(out["coverage"] * 48) <= covered.sum() + open_.sum()
    if not und.any() and not open_.any():
        assert (out["density"], out["coverage"]) == (pytest.approx(lo, rel=1e-12), covered.mean())


def test_evaluate_dit_against_its_own_features(default_run, dit, net):
    """the reference's stored rows are the run's own features: every reference ball holds its own centre again, so coverage is 1 and
    the density is that of the set in its own balls (in the run above the samples lie far from the reference and both are 0)"""
    import transvae
    own = default_run["features"].cpu()
    f64 = own.numpy().astype(np.float64)
    ref = {"n": 48, "mean": torch.from_numpy(f64.mean(0)), "cov": torch.from_numpy(np.cov(f64, rowvar=False)), "features": own}
    out = transvae.evaluate_dit(StubVAE(), dit, ref, fid_net=net, metrics=("kid", "density", "coverage"), **KID, **KW)
    assert sorted(out) == ["coverage", "density", "features", "kid", "kid_std", "n"]
    real, fake = own.numpy(), out["features"].cpu().numpy()
    rdev = transvae.knn_radius(own.to(DEV), 5).cpu().numpy()
    inside, und = GS.classify_pairs(fake, real, rdev, "data")
    lo, hi = inside.sum() / (5 * 48), (inside.sum() + und.sum()) / (5 * 48)
    print(f"own features: density {out['density']!r} in [{lo!r}, {hi!r}], coverage {out['coverage']!r}, kid {out['kid']!r} +- {out['kid_std']!r}; "
          f"fp64 {GS.density_coverage64(real, fake, 5)}")
    assert out["coverage"] == 1.0 and lo * (1 - 1e-12) <= out["density"] <= hi * (1 + 1e-12) and out["density"] >= 1.0 / 5
    ia, ib = GS.draw_subsets(48, 48, KID["kid_subsets"], KID["kid_subset_size"], KID["kid_seed"])
    mean, std, _ = GS.kid64(real, fake, ia, ib)
    bm, bs = GS.kid_bound(real, fake, ia, ib)
    assert abs(out["kid"] - mean) <= bm and abs(out["kid_std"] - std) <= bs


def test_evaluate_dit_split_scores_and_errors(default_run, dit, net, head, reference):
    import transvae
    kw = dict(KW, return_features=False)
    out = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, is_head=head, metrics=("is",), is_split_size=20, **kw)
    assert sorted(out) == ["is", "is_std", "n"]
    f = default_run["features"].cpu().numpy().astype(np.float64)
    w, b = head.weight.cpu().numpy(), head.bias.cpu().numpy()
    scores = np.array([G.inception_score64(f[a:e], w, b) for a, e in GS.split_bounds(48, 20)])
    assert len(scores) == 3
    print(f"is over splits {out['is']!r} +- {out['is_std']!r}; restated {scores.mean()!r} +- {scores.std()!r}; whole set {default_run['is']!r}")
    assert out["is"] == pytest.approx(scores.mean(), rel=1e-6) and out["is_std"] == pytest.approx(scores.std(), rel=1e-4, abs=1e-7)
    head.split_size = None                                     # the shared accumulator as the other tests expect it
    bare = {key: v for key, v in reference.items() if not key.startswith("spatial")}
    with pytest.raises(ValueError, match=r"'sfid'.*spatial=True"):
        transvae.evaluate_dit(StubVAE(), dit, bare, fid_net=net, metrics=("gfid", "sfid"), **kw)
