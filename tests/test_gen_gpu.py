"""csrc/genmetrics.hip, tv_opt_ema and their host interface on the device: the pairwise kernels through the C ABI against fp64 under
DESIGN.md section 3.1 row S (also shifted by +1000, where a Gram form fails), their exact cases, symmetry and bit-reproducibility;
tv_softmax_stats and its independence of the cut into calls; tv_opt_ema; ParamEMA; fit_dit's EMA; evaluate_dit end to end."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_restatement as FR
import gen_restatement as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.5
PAD = 1.0e30           # in the columns past d of a strided input: read by mistake, it wrecks every distance


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


def knn_abi(x, ld, k, i0=0, M=None):
    """tv_knn_radius through the C ABI, one sentinel past the output"""
    L = _L()
    N, d = x.shape
    M = N - i0 if M is None else M
    xb = strided(x, ld)
    out = torch.full((M + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    scratch = torch.empty(256 * M, dtype=torch.float32, device=DEV)
    L.check(L.load().tv_knn_radius(_p(xb), N, d, ld, i0, M, k, _p(out), _p(scratch), _stream()), "tv_knn_radius")
    assert float(out[-1]) == SENTINEL, "wrote past r2"
    return out[:-1].cpu().numpy()


def hits_abi(q, ldq, x, ldx, r2):
    L = _L()
    (M, d), N = q.shape, x.shape[0]
    qb, xb = strided(q, ldq), strided(x, ldx)
    rb = torch.from_numpy(np.asarray(r2, dtype=np.float32)).to(DEV)
    out = torch.full((M + 1,), 77, dtype=torch.int32, device=DEV)
    scratch = torch.empty(32 * M, dtype=torch.int32, device=DEV)
    L.check(L.load().tv_manifold_hits(_p(qb), M, ldq, _p(xb), N, ldx, _p(rb), d, _p(out), _p(scratch), _stream()), "tv_manifold_hits")
    assert int(out[-1]) == 77, "wrote past hit"
    return out[:-1].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# the pairwise kernels against fp64
# ---------------------------------------------------------------------------------------------------------------------------
# per shape: the row stride (d + 3 is odd at d = 2048: the scalar path; 40 at d = 37: float4 loads with a ragged last group) and a
# sub-range of queries (i0 > 0, M < N) for one of them
LAYOUT = {G.SHAPES[0]: (2048 + 3, None), G.SHAPES[1]: (37 + 3, None), G.SHAPES[2]: (64, (70, 150)), G.SHAPES[3]: (2048, None)}


@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["plain", "plus1000"])
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.shape_id)
def test_pairwise_against_fp64(shape, shift):
    N, M, d, k, seed = shape
    ld, sub = LAYOUT[shape]
    x, q = G.make_inputs(N, M, d, seed, shift=shift)
    r2 = knn_abi(x, ld, k)
    ref = G.knn_radius64(x, k)
    print(f"radii {G.shape_id(shape)} shift {shift}: worst relative error {np.max(np.abs(r2 - ref) / ref):.3g}, bound {G.radius_bound(d):.3g}")
    assert G.check_radii(r2, x, k) is None, G.check_radii(r2, x, k)
    if sub is not None:
        i0, m = sub
        part = knn_abi(x, ld, k, i0, m)
        assert np.array_equal(part, r2[i0:i0 + m]), "a sub-range of queries gives other bits than the whole range"
    hit = hits_abi(q, ld, x, ld, r2)
    msg, undecided = G.check_hits(hit, q, x, r2)
    print(f"hits {G.shape_id(shape)} shift {shift}: {int(hit.sum())} of {M}, undecided share {undecided:.3g}")
    assert undecided <= G.UNDECIDED_MAX
    assert msg is None, msg
    assert 0 < hit.sum() < M, "the inputs are meant to give both outcomes"


def test_exact_cases_are_bit_equal_to_fp64():
    g = np.random.default_rng(11)
    d = 37
    x = g.integers(-63, 64, size=(150, d)).astype(np.float32)        # |v| < 64: every D < 37 * 127^2 < 2^24 is exact in fp32
    x[17] = x[3]                                                      # a duplicated point
    q = np.concatenate([x[:5] + np.float32(1), g.integers(-63, 64, size=(40, d)).astype(np.float32)], 0)
    for k in (1, 3, 8):
        r2 = knn_abi(x, d, k)
        assert np.array_equal(r2.astype(np.float64), G.knn_radius64(x, k)), k
        if k == 1:
            assert r2[3] == 0.0 and r2[17] == 0.0, "a duplicate is a neighbour at distance 0"
        assert np.array_equal(hits_abi(q, d, x, d + 1, r2), G.hits64(q, x, r2)), k
    # a tie D == r2 hits; just outside does not
    t = np.zeros((3, d), dtype=np.float32)
    t[1, :2], t[2, 0] = (3, 4), 40
    r2 = knn_abi(t, d, 1)
    assert r2.tolist() == [25.0, 25.0, 37.0 ** 2 + 16.0]
    qq = np.zeros((3, d), dtype=np.float32)
    qq[0, :2], qq[1, :2], qq[2, :3] = (-3, 4), (-30, -30), (-3, 4, 1)
    assert hits_abi(qq, d, t, d, r2).tolist() == [1, 0, 0]
    # N = k + 1: every other point is a neighbour, the radius is the farthest
    s = g.integers(-63, 64, size=(4, d)).astype(np.float32)
    assert np.array_equal(knn_abi(s, d, 3).astype(np.float64), G.sqdist64(s, s).max(1))


def test_symmetry_permutation_and_reproducibility():
    import transvae
    N, M, d, k, seed = G.SHAPES[2]
    x, q = G.make_inputs(N, M, d, seed)
    xd, qd = torch.from_numpy(x).to(DEV), torch.from_numpy(q).to(DEV)
    r = transvae.knn_radius(xd, k)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4)).to(DEV)
    rp = transvae.knn_radius(xd[perm].contiguous(), k)
    assert torch.equal(rp, r[perm]), "the radii depend on the order of the rows: D(a, b) != D(b, a), or on the tile a pair falls in"
    assert torch.equal(transvae.knn_radius(xd, k), r)
    h = transvae.manifold_hits(qd, xd, r)
    assert torch.equal(transvae.manifold_hits(qd, xd, r), h) and h.dtype == torch.int32
    assert torch.equal(transvae.manifold_hits(qd, xd[perm].contiguous(), rp), h)
    assert torch.equal(transvae.knn_radius(xd, k, queries_per_launch=64), r)
    assert torch.equal(transvae.manifold_hits(qd, xd, r, queries_per_launch=100), h)
    pr, want = transvae.precision_recall(xd, qd, k), G.precision_recall64(x, q, k)
    assert sorted(pr) == ["precision", "recall"]
    # real = x, fake = q.  The decided queries fix the count up to the undecided ones; with none undecided it is the fp64 value
    for name, cls, n in (("precision", G.classify_hits(q, x, r.cpu().numpy()), M), ("recall", G.classify_hits(x, q, transvae.knn_radius(qd, k).cpu().numpy()), N)):
        inside, undecided = int((cls == 1).sum()), int((cls < 0).sum())
        print(f"{name}: {pr[name]!r}, fp64 {want[name]!r}, decided inside {inside}, undecided {undecided} of {n}")
        assert undecided <= G.UNDECIDED_MAX * n
        assert inside <= round(pr[name] * n) <= inside + undecided, (name, pr[name], inside, undecided)
        if not undecided:
            assert pr[name] == want[name], name


def test_wrapper_cuts_at_8192_queries():
    """N > 8192: the default wrapper runs two launches (8192 queries in 8 data slices, then the rest); one launch of all N gives
    the same bits, and a sample of the radii is within the bound of fp64"""
    import transvae
    from transvae import metrics_gen
    assert metrics_gen.QUERIES_PER_LAUNCH == 8192
    N, d, k = 8200, 8, 3
    x, _ = G.make_inputs(N, 2, d, 9)
    xd = torch.from_numpy(x).to(DEV)
    r = transvae.knn_radius(xd, k)
    assert torch.equal(transvae.knn_radius(xd, k, queries_per_launch=N), r)
    got = r.cpu().numpy()
    for i0 in (0, 8150):
        assert G.check_radii(got[i0:i0 + 50], x, k, i0, 50) is None


def test_pairwise_argument_errors():
    L = _L()
    lib = L.load()
    x = torch.zeros(8, 8, device=DEV)
    r = torch.zeros(8, device=DEV)
    h = torch.zeros(8, dtype=torch.int32, device=DEV)
    for args, word in (((_p(x), 8, 8, 8, 0, 8, 9, _p(r), None, None), "k=9"), ((_p(x), 3, 8, 8, 0, 3, 3, _p(r), None, None), "N=3"),
                       ((_p(x), 8, 9000, 9000, 0, 8, 3, _p(r), None, None), "d=9000"), ((_p(x), 8, 8, 4, 0, 8, 3, _p(r), None, None), "ldx=4"),
                       ((_p(x), 8, 8, 8, 4, 8, 3, _p(r), None, None), "i0=4")):
        assert lib.tv_knn_radius(*args) != 0 and word in lib.tv_last_error().decode(), word
    assert lib.tv_manifold_hits(_p(x), 8, 8, _p(x), 8, 8, _p(r), 0, _p(h), None, None) != 0 and "d=0" in lib.tv_last_error().decode()
    assert lib.tv_manifold_hits(_p(x), 8, 4, _p(x), 8, 8, _p(r), 8, _p(h), None, None) != 0 and "ldq=4" in lib.tv_last_error().decode()
    assert lib.tv_softmax_stats(_p(x), 8, 5000, 5000, _p(x), _p(x), None) != 0 and "K=5000" in lib.tv_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------------
# tv_softmax_stats and InceptionScore
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_abi(z, ld, cuts):
    L = _L()
    B, K = z.shape
    zb = strided(z, ld)
    state = torch.zeros(2 + K + 1, dtype=torch.float64, device=DEV)
    state[-1] = SENTINEL
    b0 = 0
    for nb in cuts:
        scratch = torch.empty(nb * (K + 1), dtype=torch.float64, device=DEV)
        L.check(L.load().tv_softmax_stats(_p(zb[b0:]), nb, K, ld, _p(state), _p(scratch), _stream()), "tv_softmax_stats")
        b0 += nb
    assert b0 == B and float(state[-1]) == SENTINEL, "wrote past the state"
    return state[:-1].cpu().numpy()


@pytest.mark.parametrize("B,K", [(5, 1008), (3, 1), (2, 4096)])
def test_softmax_stats(B, K):
    g = np.random.default_rng(B * 10000 + K)
    z = (g.standard_normal((B, K)) * 4).astype(np.float32)
    z[0, 0], z[0, K - 1] = 80.0, -80.0
    z[B - 1] = z[B - 2]                                       # equal rows
    got = softmax_abi(z, K + 5, (B,))
    ref, bound = G.softmax_stats64(z), G.softmax_stats_bound(z)
    assert got[0] == B
    err = np.abs(got - ref)
    print(f"softmax_stats {B}x{K}: worst error / bound {np.max(err[1:] / np.where(bound[1:] > 0, bound[1:], 1.0)):.3g}")
    assert (err[1:] <= bound[1:]).all()
    if B == 5:
        for cuts in ((2, 3), (1, 1, 1, 1, 1)):
            assert np.array_equal(softmax_abi(z, K + 5, cuts), got), cuts


def test_inception_score():
    import transvae
    g = torch.Generator().manual_seed(3)
    d, K, n = 2048, 16, 40
    f = torch.rand(n, d, generator=g)
    w = torch.randn(K, d, generator=g) * (3.0 / d ** 0.5)
    b = torch.randn(K, generator=g)
    head = transvae.InceptionScore(w, b).to(DEV)
    for i in (0, 16, 32):
        head.update(f[i:i + 16].to(DEV))
    got = head.compute()
    ref = G.inception_score64(f.numpy(), w.numpy(), b.numpy())
    # fp32 logits: |dz| <= d u (|f| |w|^T + |b|) each; log IS = mean_i sum_k p (log p - log pbar) moves by at most 4 max |dz|
    dz = d * G.U * float((f.abs().double() @ w.abs().double().T + b.abs().double()).max())
    print(f"InceptionScore {got!r}, fp64 {ref!r}, bound on the log {4 * dz:.3g}")
    assert head.n == n and 1.0 < got < K
    assert abs(np.log(got) - np.log(ref)) <= 4 * dz
    whole = transvae.InceptionScore(w, b).to(DEV)
    whole.update(f.to(DEV))
    assert torch.equal(whole.state(), head.state()), "the state depends on the cut into updates"


# ---------------------------------------------------------------------------------------------------------------------------
# tv_opt_ema and ParamEMA
# ---------------------------------------------------------------------------------------------------------------------------
def test_opt_ema_kernel():
    L = _L()
    lib = L.load()
    chunk = lib.tv_opt_chunk_elems()
    sizes = (1, chunk - 1, chunk + 1)
    g = torch.Generator().manual_seed(8)
    ema0 = [torch.randn(n, generator=g) for n in sizes]
    w = [torch.randn(n, generator=g) for n in sizes]
    for e, v in zip(ema0, w):
        v[::3] = e[::3]                                       # w == ema: those bits must not move
    a = float(1.0 - 0.999)
    a32 = np.float32(a)
    wd = [v.to(DEV) for v in w]
    rows = [[i, c] for i, n in enumerate(sizes) for c in range((n + chunk - 1) // chunk)]
    chunks = torch.tensor(rows, dtype=torch.int32, device=DEV)

    def run(ctrl):
        # each EMA tensor sits inside a buffer with a sentinel on either side (the first at an address that is not 16-byte aligned)
        bufs = [torch.full((n + 8,), SENTINEL, device=DEV) for n in sizes]
        views = [b[(1 if i == 0 else 4):(1 if i == 0 else 4) + n] for i, (b, n) in enumerate(zip(bufs, sizes))]
        for v, e in zip(views, ema0):
            v.copy_(e)
        tab = torch.tensor([[v.data_ptr(), s.data_ptr(), 0, 0, 0, n] for v, s, n in zip(views, wd, sizes)], dtype=torch.int64, device=DEV)
        L.check(lib.tv_opt_ema(_p(tab), _p(chunks), len(rows), _p(ctrl), a, _stream()), "tv_opt_ema")
        torch.cuda.synchronize()
        for i, (b, n) in enumerate(zip(bufs, sizes)):
            o = 1 if i == 0 else 4
            assert bool((b[:o] == SENTINEL).all()) and bool((b[o + n:] == SENTINEL).all()), "wrote outside the tensor"
        return [v.cpu() for v in views]

    ctrl = torch.zeros(8, device=DEV)
    got = run(None)
    for e, v, o in zip(ema0, w, got):
        ref = G.ema64(e.numpy(), v.numpy(), a32)
        assert (np.abs(o.numpy().astype(np.float64) - ref) <= G.ema_bound(e.numpy(), v.numpy())).all()
        assert torch.equal(o[::3], e[::3]), "w == ema changed bits"
        if o.numel() > 3:
            assert not torch.equal(o, e)
    assert all(torch.equal(x, y) for x, y in zip(run(ctrl), got)), "ctrl[3] == 0 must update as a NULL ctrl does"
    ctrl[3] = 1.0
    assert all(torch.equal(x, y) for x, y in zip(run(ctrl), ema0)), "a skipped step must leave every bit"


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


def test_param_ema(dit):
    import transvae
    ema = transvae.ParamEMA(dit.parameters(), decay=0.5)
    assert all(torch.equal(e, p) for e, p in zip(ema.shadow, dit.parameters())) and ema.num_updates == 0
    before = [p.detach().clone() for p in dit.parameters()]
    g = torch.Generator(device=DEV).manual_seed(2)
    with torch.no_grad():
        for p in dit.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g, device=DEV))
    moved = [p.detach().clone() for p in dit.parameters()]
    ema.update()
    a32 = np.float32(0.5)
    for e, b, m in zip(ema.shadow, before, moved):
        ref = G.ema64(b.cpu().numpy(), m.cpu().numpy(), a32)
        assert (np.abs(e.cpu().numpy().astype(np.float64) - ref) <= G.ema_bound(b.cpu().numpy(), m.cpu().numpy())).all()
    assert ema.num_updates == 1
    x = torch.randn(3, 4, 8, 8, generator=g, device=DEV)
    t = torch.tensor([0.1, 0.5, 0.9], device=DEV)
    y = torch.tensor([0, 4, 5], device=DEV)
    with torch.no_grad():
        v_own = dit(x, t, y)
        with ema.applied(dit):
            v_ema = dit(x, t, y)
        assert all(torch.equal(p, m) for p, m in zip(dit.parameters(), moved)), "applied() did not restore the bits"
        assert torch.equal(dit(x, t, y), v_own)
        twin = transvae.DiT(8, 2, 4, 64, 1, 5).to(DEV).eval()
        ema.copy_to(twin.parameters())
        assert torch.equal(twin(x, t, y), v_ema) and not torch.equal(v_ema, v_own)
    other = transvae.ParamEMA(twin.parameters(), decay=0.9)
    with torch.no_grad():
        for e in other.shadow:
            e.zero_()
    other.load_state_dict(ema.state_dict())
    assert other.decay == 0.5 and other.num_updates == 1 and all(torch.equal(a, b) for a, b in zip(other.shadow, ema.shadow))
    assert sorted(ema.state_dict()) == ["decay", "num_updates", "shadow"]
    with torch.no_grad():                                      # leave the shared model as it was handed in
        for p, b in zip(dit.parameters(), before):
            p.copy_(b)


def test_param_ema_follows_a_skipped_optimizer_step():
    import transvae
    p = torch.nn.Parameter(torch.ones(10, device=DEV))
    opt = transvae.optim.FusedAdamW([p], lr=0.1, weight_decay=0.0, bf16_operands=False)
    ema = transvae.ParamEMA([p], decay=0.5, optimizer=opt)
    p.grad = torch.full((10,), float("nan"), device=DEV)
    opt.step()
    with torch.no_grad():
        p.add_(1.0)
    ema.update()
    assert torch.equal(ema.shadow[0], torch.ones(10, device=DEV)), "the optimizer skipped the step: the average must not move"
    p.grad = torch.ones(10, device=DEV)
    opt.step()
    ema.update()
    assert bool((ema.shadow[0] > 1.0).all())


def test_fit_dit_keeps_an_ema(tmp_path):
    import transvae
    from probe_restatement import write_split
    g = torch.Generator().manual_seed(0)
    D, h = 4, 8
    shards = []
    for n in (10, 6):
        lat = torch.randn(n, 2 * D, h, h, generator=g)
        shards.append({"latents": lat, "latents_flip": lat.flip(-1), "labels": torch.randint(0, 5, (n,), generator=g)})
    write_split(str(tmp_path), shards, {"mean": torch.zeros(1, D, 1, 1), "std": torch.ones(1, D, 1, 1)})

    def run(**kw):
        m = transvae.DiT(h, 2, D, 64, 1, 5, generator=torch.Generator().manual_seed(1))
        init = [p.detach().clone() for p in m.parameters()]
        return m, init, transvae.fit_dit(str(tmp_path), m, epochs=2, batch_size=4, lr=1e-3, seed=0, log_every=3, device=DEV, **kw)

    m, init, r = run(ema_decay=0.9)
    ema = r["ema"]
    assert isinstance(ema, transvae.ParamEMA) and ema.decay == 0.9 and ema.num_updates == r["steps"] == 10
    trained = [(e, p, i) for e, p, i in zip(ema.shadow, m.parameters(), init) if not torch.equal(p.cpu(), i)]
    assert trained, "no parameter moved"
    for e, p, i in trained:
        assert not torch.equal(e, p) and not torch.equal(e.cpu(), i)
    _, _, r0 = run(ema_decay=None)
    assert "ema" not in r0


# ---------------------------------------------------------------------------------------------------------------------------
# evaluate_dit end to end
# ---------------------------------------------------------------------------------------------------------------------------
class StubVAE:
    """decode: the first three latent channels, up-sampled 4x: [B, 4, 8, 8] -> [B, 3, 32, 32]"""

    def decode(self, lat):
        return F.interpolate(0.25 * lat[:, :3].float() + 0.5, scale_factor=4, mode="nearest")


class NaNFeatures:
    """the feature network, with one non-finite entry in the features of the batch `bad_call`"""

    def __init__(self, net, bad_call):
        self.net, self.calls, self.bad_call = net, 0, bad_call

    def features(self, img, clip=False):
        f = self.net.features(img, clip=clip)
        self.calls += 1
        if self.calls - 1 == self.bad_call:
            f[0, 5] = float("inf")
        return f


@pytest.fixture(scope="module")
def net():
    from transvae import InceptionFeatures
    return InceptionFeatures().load_fid_state_dict(FR.plain_state_dict()).to(DEV)


@pytest.fixture(scope="module")
def head():
    import transvae
    g = torch.Generator().manual_seed(6)
    return transvae.InceptionScore(torch.randn(16, 2048, generator=g) * 0.02, torch.randn(16, generator=g) * 0.1).to(DEV)


@pytest.fixture(scope="module")
def reference(net, head):
    import transvae
    imgs = FR.smooth_images(48, 32, 32, 123)
    return transvae.reference_statistics([(imgs[:24], None), (imgs[24:], None)], net, is_head=head)


KW = dict(num_samples=48, batch_size=16, steps=2, cfg_scale=1.5, return_features=True)


@pytest.fixture(scope="module")
def first_run(dit, net, head, reference):
    import transvae
    return transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, is_head=head, **KW)


def restated(reference, feats, head):
    f = feats.cpu().numpy().astype(np.float64)
    out = {"gfid": G.frechet_rows64(reference["features"].numpy(), f),            # numpy alone, from the rows: none of the package's code
           "is": G.inception_score64(f, head.weight.cpu().numpy(), head.bias.cpu().numpy())}
    out.update(G.precision_recall64(reference["features"].numpy(), feats.cpu().numpy(), 3))
    return out


def test_reference_statistics(reference, net, head):
    assert reference["n"] == 48 and tuple(reference["mean"].shape) == (2048,) and tuple(reference["cov"].shape) == (2048, 2048)
    assert reference["mean"].dtype == torch.float64 and reference["cov"].dtype == torch.float64
    f = reference["features"]
    assert tuple(f.shape) == (48, 2048) and f.dtype == torch.float32 and f.device.type == "cpu"
    f64 = f.numpy().astype(np.float64)
    assert np.allclose(reference["mean"].numpy(), f64.mean(0), rtol=1e-12, atol=1e-14)
    assert np.allclose(reference["cov"].numpy(), np.cov(f64, rowvar=False), rtol=1e-9, atol=1e-13)
    w, b = head.weight.cpu().double(), head.bias.cpu().double()
    dz = 2048 * G.U * float((f.abs().double() @ w.abs().T + b.abs()).max())      # fp32 logits; the log of the score moves by <= 4 max |dz|
    assert abs(np.log(reference["is"]) - np.log(G.inception_score64(f64, w.numpy(), b.numpy()))) <= 4 * dz


def test_evaluate_dit_against_the_restatement(first_run, reference, head):
    out = first_run
    assert sorted(out) == ["features", "gfid", "is", "n", "precision", "recall"] and out["n"] == 48
    feats = out["features"]
    assert tuple(feats.shape) == (48, 2048) and feats.is_cuda and feats.dtype == torch.float32
    assert all(np.isfinite(out[m]) for m in ("gfid", "is", "precision", "recall"))
    want = restated(reference, feats, head)
    print("evaluate_dit", {m: out[m] for m in want}, "restated", want)
    for m, v in want.items():
        assert out[m] == pytest.approx(v, rel=1e-6), m
    # the returned gFID against two numpy references on the full rows (48 x 2048: both covariances have rank 47).  The row form
    # is exact at any rank and is held to the tolerance of tests/test_fid_gpu.py, 1e-8 x trace.  fid_restatement.frechet_numpy is
    # written for n > d: at n <= d it takes square roots of rounding noise in ~2000 null directions (measured on 48 restatement
    # features per side on the host: 1.9e-4 from the row form at a trace of 130, the package's value 9e-9 from it), so it is held
    # to the bound of its own arithmetic, gen_restatement.frechet_null_space_noise.
    a, b = reference["features"].numpy(), feats.cpu().numpy()
    trace = float(np.trace(reference["cov"].numpy()))
    rows, eig, noise = G.frechet_rows64(a, b), FR.frechet_numpy(a, b), G.frechet_null_space_noise(a, b)
    print(f"gfid {out['gfid']!r}: row form {rows!r} (off {out['gfid'] - rows:.3g}, allowed {1e-8 * max(1.0, trace):.3g}), "
          f"frechet_numpy {eig!r} (off {out['gfid'] - eig:.3g}, allowed {noise:.3g}), trace {trace:.6g}")
    assert abs(out["gfid"] - rows) <= 1e-8 * max(1.0, trace)
    assert abs(out["gfid"] - eig) <= 1e-8 * max(1.0, trace) + noise


def test_evaluate_dit_seeds_and_subsets(first_run, dit, net, head, reference):
    import transvae
    again = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, is_head=head, **KW)
    for m in ("gfid", "is", "precision", "recall"):
        assert again[m] == pytest.approx(first_run[m], rel=1e-6), m
    other = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, metrics=("gfid",), seed=1, **KW)
    assert sorted(other) == ["features", "gfid", "n"]
    assert other["gfid"] != pytest.approx(first_run["gfid"], rel=1e-6) and not torch.equal(other["features"], first_run["features"])


def test_evaluate_dit_against_its_own_features(first_run, dit, net, tmp_path):
    import transvae
    f = first_run["features"].cpu()
    f64 = f.numpy().astype(np.float64)
    cov = np.cov(f64, rowvar=False)
    path = str(tmp_path / "own.pt")
    torch.save({"n": 48, "mean": torch.from_numpy(f64.mean(0)), "cov": torch.from_numpy(cov), "features": f}, path)
    kw = dict(KW, return_features=False)
    out = transvae.evaluate_dit(StubVAE(), dit, path, fid_net=net, metrics=("gfid", "precision", "recall"), **kw)
    assert sorted(out) == ["gfid", "n", "precision", "recall"]
    assert out["precision"] == 1.0 and out["recall"] == 1.0
    assert abs(out["gfid"]) < 1e-6 * np.trace(cov)


def test_evaluate_dit_ema_labels_and_errors(dit, net, reference):
    import transvae
    kw = dict(num_samples=16, batch_size=8, steps=1, metrics=("gfid",), return_features=True)
    plain = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, **kw)
    ema = transvae.ParamEMA(dit.parameters(), decay=0.0)
    same = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, ema=ema, **kw)
    assert torch.equal(same["features"], plain["features"]), "an EMA equal to the weights must give the same samples"
    with torch.no_grad():
        for e in ema.shadow:
            e.mul_(0.5)
    kept = [p.detach().clone() for p in dit.parameters()]
    halved = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, ema=ema, **kw)
    assert not torch.equal(halved["features"], plain["features"])
    assert all(torch.equal(p, q) for p, q in zip(dit.parameters(), kept))
    labels = (torch.arange(16, device=DEV) % dit.num_classes).flip(0)
    flipped = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, labels=labels.contiguous(), **kw)
    assert not torch.equal(flipped["features"], plain["features"])
    sig = transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, transform="sigmoid", **kw)
    assert not torch.equal(sig["features"], plain["features"])
    narrow = {"n": 48, "mean": torch.zeros(64, dtype=torch.float64), "cov": torch.eye(64, dtype=torch.float64)}
    with pytest.raises(ValueError, match="feature width 64"):
        transvae.evaluate_dit(StubVAE(), dit, narrow, fid_net=net, **kw)
    with pytest.raises(ValueError, match=r"labels must be \[16\]"):
        transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=net, labels=labels[:5], **kw)
    with pytest.raises(RuntimeError, match=r"samples 8 \.\. 15 \(batch 1\)"):
        transvae.evaluate_dit(StubVAE(), dit, reference, fid_net=NaNFeatures(net, 1), **kw)
