"""Plain fp64 restatement of the rest of the generator-evaluation suite (sFID tap, KID, density / coverage, Inception Score over
splits; csrc/genmetrics.hip, csrc/fid.hip, transvae/metrics_gen.py): references, the bounds of DESIGN.md section 3.1 row S, the fp32
chain emulations with planted defects, and the seeded inputs.  Builds on gen_restatement (distances, radii, softmax statistics) and
fid_restatement (the network, its weights and images)."""
import json
import os
import sys

import numpy as np

import gen_restatement as G

U = G.U
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_SPATIAL = os.path.join(HERE, "golden", "gen_suite_spatial_ref_bf16_autocast.json")
SPATIAL_CASE = (4, 64, 64, 321)        # images, H, W, seed of fid_restatement.smooth_images
SPATIAL_CHANNELS, SPATIAL_GRID = 7, 17
UNDECIDED_PAIRS_MAX = 1e-3
UNDECIDED_COVERAGE_MAX = 1e-2


# ---------------------------------------------------------------------------------------------------------------------------
# ball counts, density and coverage
# ---------------------------------------------------------------------------------------------------------------------------
def _radii(r2, radius_of, M, N):
    """the radius of pair (i, j) as an [M, N]-broadcastable fp64 array"""
    r = np.asarray(r2, dtype=np.float64)
    assert radius_of in ("data", "query") and r.shape == ((N,) if radius_of == "data" else (M,))
    return r[None, :] if radius_of == "data" else r[:, None]


def counts64(q, x, r2, radius_of="data"):
    D = G.sqdist64(q, x)
    return (D <= _radii(r2, radius_of, *D.shape)).sum(1).astype(np.int64)


def classify_pairs(q, x, r2, radius_of="data"):
    """(inside [M, N], undecided [M, N]): a pair is decided when fp64 puts D outside r (1 +- (d + 2) u)"""
    tau = G.radius_bound(x.shape[1])
    D = G.sqdist64(q, x)
    r = _radii(r2, radius_of, *D.shape)
    inside = D <= r * (1 - tau)
    outside = D > r * (1 + tau)
    return inside, ~(inside | outside)


def check_counts(got, q, x, r2, radius_of="data"):
    """(message or None, undecided share of all pairs): every count within [decided inside, decided inside + undecided]"""
    inside, undecided = classify_pairs(q, x, r2, radius_of)
    lo, hi = inside.sum(1), inside.sum(1) + undecided.sum(1)
    got = np.asarray(got).astype(np.int64)
    bad = (got < lo) | (got > hi)
    msg = None
    if bad.any():
        i = int(np.argmax(bad))
        msg = f"{int(bad.sum())} of {got.shape[0]} counts outside their range, first at {i}: got {int(got[i])}, allowed [{int(lo[i])}, {int(hi[i])}]"
    return msg, float(undecided.mean())


def undecided_coverage(real, fake, r2_real):
    """share of real rows whose coverage decision hangs on an undecided pair: no decided fake row inside, at least one undecided"""
    inside, undecided = classify_pairs(real, fake, r2_real, "query")
    return float((~inside.any(1) & undecided.any(1)).mean())


def density_coverage64(real, fake, k):
    r2 = G.knn_radius64(real, k)
    density = counts64(fake, real, r2, "data").sum() / float(k * fake.shape[0])
    coverage = float((counts64(real, fake, r2, "query") > 0).mean())
    return {"density": float(density), "coverage": coverage}


def counts32(q, x, r2, radius_of="data", strict=False, swapped=False):
    """the fp32 chain emulated on the host; defects: strict = `<` for `<=`; swapped = the radius of the other side's index
    (data for query and query for data; needs M == N)"""
    D = G.sqdist32(q, x)
    side = {"data": "query", "query": "data"}[radius_of] if swapped else radius_of
    r = np.asarray(r2, dtype=np.float32)
    r = r[None, :] if side == "data" else r[:, None]
    return ((D < r) if strict else (D <= r)).sum(1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# KID: polynomial-kernel sums and the unbiased MMD^2
# ---------------------------------------------------------------------------------------------------------------------------
def poly_inputs(N, M, d, seed):
    """(a [N, d], b [M, d]) fp32, the rows of gen_restatement.make_inputs (non-negative, like pool3 features)"""
    return G.make_inputs(N, M, d, seed)


def poly_sums64(a, ia, b, ib, gamma, coef0=1.0, skip=False, keep_diagonal=False):
    """[S] fp64: sum over positions i, j of (gamma a[ia[s, i]] . b[ib[s, j]] + coef0)^3, the pairs i == j left out with `skip`.
    defect: keep_diagonal ignores `skip`."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty(len(ia))
    for s, (ra, rb) in enumerate(zip(ia, ib)):
        k = (gamma * (a[ra] @ b[rb].T) + coef0) ** 3
        out[s] = k.sum() - (np.trace(k) if skip and not keep_diagonal else 0.0)
    return out


def poly_sums_bound(a, ia, b, ib, gamma, coef0=1.0, skip=False):
    """[S]: sum over the pairs of 3 t^2 gamma (d + 2) u sum_c |a_c b_c|.  The fp32 chain of d products is off by at most
    (d + 2) u sum_c |a_c b_c| (d fused multiply-adds, the conversion is exact), t = gamma dot + coef0 moves by gamma times that,
    and d(t^3) = 3 t^2 dt to first order; the fp64 steps after it add 2^-53-sized terms that the bound swallows."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = a.shape[1]
    out = np.empty(len(ia))
    for s, (ra, rb) in enumerate(zip(ia, ib)):
        t = gamma * (a[ra] @ b[rb].T) + coef0
        e = 3.0 * t * t * gamma * (d + 2) * U * (np.abs(a[ra]) @ np.abs(b[rb]).T)
        out[s] = e.sum() - (np.trace(e) if skip else 0.0)
    return out


def poly_sums32(a, ia, b, ib, gamma, coef0=1.0, skip=False, keep_diagonal=False):
    """the kernel's arithmetic emulated on the host: the dot product as one unfused fp32 chain over c in order, then fp64"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    out = np.empty(len(ia))
    for s, (ra, rb) in enumerate(zip(ia, ib)):
        x, y = a[ra], b[rb]
        dot = np.zeros((x.shape[0], y.shape[0]), dtype=np.float32)
        for c in range(x.shape[1]):
            dot = dot + x[:, c, None] * y[None, :, c]
        t = dot.astype(np.float64) * gamma + coef0
        k = (t * t) * t
        out[s] = k.sum() - (np.trace(k) if skip and not keep_diagonal else 0.0)
    return out


def mmd2_from_sums(sxx, syy, sxy, m, biased=False):
    """per subset: Sxx / (m (m - 1)) + Syy / (m (m - 1)) - 2 Sxy / m^2; defect: biased divides all three by m^2"""
    nn = float(m * m) if biased else float(m * (m - 1))
    return np.asarray(sxx) / nn + np.asarray(syy) / nn - 2.0 * np.asarray(sxy) / float(m * m)


def kid64(real, fake, ia, ib, sums=poly_sums64, biased=False, keep_diagonal=False):
    """(mean, population standard deviation, per-subset values) of the unbiased MMD^2 with k = (x . y / d + 1)^3 over the subsets"""
    m, gamma = ia.shape[1], 1.0 / real.shape[1]
    kw = dict(keep_diagonal=True) if keep_diagonal else {}
    vals = mmd2_from_sums(sums(real, ia, real, ia, gamma, 1.0, True, **kw), sums(fake, ib, fake, ib, gamma, 1.0, True, **kw),
                          sums(real, ia, fake, ib, gamma, 1.0, False), m, biased=biased)
    return float(vals.mean()), float(vals.std()), vals


def kid_bound(real, fake, ia, ib):
    """(bound on the mean, bound on the standard deviation): per subset Bxx / (m (m - 1)) + Byy / (m (m - 1)) + 2 Bxy / m^2; the mean
    moves by at most the mean of these, and a standard deviation is 1-Lipschitz in the root-mean-square of the changes, which the
    largest change bounds.  One part in 10^12 of the terms' size is added for the fp64 steps themselves."""
    m, gamma = ia.shape[1], 1.0 / real.shape[1]
    bxx, byy = poly_sums_bound(real, ia, real, ia, gamma, 1.0, True), poly_sums_bound(fake, ib, fake, ib, gamma, 1.0, True)
    bxy = poly_sums_bound(real, ia, fake, ib, gamma, 1.0, False)
    per = bxx / float(m * (m - 1)) + byy / float(m * (m - 1)) + 2.0 * bxy / float(m * m)
    size = (poly_sums64(real, ia, real, ia, gamma, 1.0, True) + poly_sums64(fake, ib, fake, ib, gamma, 1.0, True)) / float(m * (m - 1))
    per = per + 1e-12 * size
    return float(per.mean()), float(per.max())


def self_kid64(x, idx):
    """The unbiased MMD^2 of a subset against ITSELF (the same rows at the same positions) in closed form.  Sxx = Syy = the
    off-diagonal sum, Sxy = that plus the diagonal, so the value is 2 Soff / (m (m - 1)) - 2 (Soff + Sdiag) / m^2
    = (2 / m) (mean off-diagonal k - mean diagonal k): of order 1 / m and negative for features (k(x, x) >= k(x, y)), not 0."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(len(idx))
    for s, r in enumerate(idx):
        k = (x[r] @ x[r].T / x.shape[1] + 1.0) ** 3
        m = len(r)
        out[s] = 2.0 / m * ((k.sum() - np.trace(k)) / (m * (m - 1)) - np.trace(k) / m)
    return out


def draw_subsets(n_real, n_fake, subsets, subset_size, seed):
    """the package's draw, restated: one default_rng(seed); per subset choice(n_real, m) then choice(n_fake, m), without replacement,
    m clamped to the smaller set"""
    m = min(subset_size, n_real, n_fake)
    g = np.random.default_rng(seed)
    ia, ib = np.empty((subsets, m), dtype=np.int32), np.empty((subsets, m), dtype=np.int32)
    for s in range(subsets):
        ia[s] = g.choice(n_real, m, replace=False)
        ib[s] = g.choice(n_fake, m, replace=False)
    return ia, ib


# ---------------------------------------------------------------------------------------------------------------------------
# Inception Score over splits
# ---------------------------------------------------------------------------------------------------------------------------
def split_bounds(n, split_size):
    """[(first row, end row)] of the consecutive splits; the last may be short"""
    return [(i, min(n, i + split_size)) for i in range(0, n, split_size)]


def split_states64(logits, split_size):
    return np.stack([G.softmax_stats64(logits[a:b]) for a, b in split_bounds(len(logits), split_size)])


def split_scores64(logits, split_size):
    z = np.asarray(logits, dtype=np.float64)
    return np.array([G.score64(z[a:b]) for a, b in split_bounds(len(z), split_size)])


def score_bound_from_state(logits):
    """what `softmax_stats_bound` allows the LOG of the score of these rows to move by: the score is exp(S / n - sum_k pbar_k log
    pbar_k) with pbar = psum / n; dS / n moves it directly and each psum_k by |log pbar_k + 1| dpsum_k / n"""
    z = np.asarray(logits, dtype=np.float64)
    b = G.softmax_stats_bound(z)
    st = G.softmax_stats64(z)
    n = st[0]
    pbar = st[2:] / n
    nz = pbar > 0
    return float(b[1] / n + (np.abs(np.log(pbar[nz]) + 1.0) * b[2:][nz]).sum() / n)


# ---------------------------------------------------------------------------------------------------------------------------
# the spatial tap: relu(bn(conv)) of Mixed_6d.branch1x1, channels 0 .. 6, flattened (h, w, c)
# ---------------------------------------------------------------------------------------------------------------------------
def spatial_tap(x, sd):
    """x [B, 3, H, W] in [0, 1] -> [B, 17 * 17 * 7]: fid_restatement's network up to Mixed_6c, then the 1x1 branch of Mixed_6d"""
    import torch
    import torch.nn.functional as F
    import fid_restatement as FR

    def c(h, name):
        stride, pad = FR.GEOMETRY[name]
        dt = h.dtype
        h = F.conv2d(h, sd[f"{name}.weight"].to(dt), None, stride=stride, padding=pad)
        h = F.batch_norm(h, sd[f"{name}.mean"].to(dt), sd[f"{name}.var"].to(dt), sd[f"{name}.gamma"].to(dt), sd[f"{name}.beta"].to(dt),
                         False, 0.0, FR.EPS)
        return F.relu(h)

    def chain(h, blk, names):
        for n in names:
            h = c(h, f"{blk}.{n}")
        return h

    def avg(h):
        return F.avg_pool2d(h, 3, stride=1, padding=1, count_include_pad=False)

    h = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    h = 2 * h - 1
    for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        h = c(h, n)
    h = F.max_pool2d(h, 3, stride=2)
    h = c(c(h, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
    h = F.max_pool2d(h, 3, stride=2)
    for blk in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        h = torch.cat([c(h, f"{blk}.branch1x1"), chain(h, blk, ("branch5x5_1", "branch5x5_2")),
                       chain(h, blk, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3")), c(avg(h), f"{blk}.branch_pool")], 1)
    h = torch.cat([c(h, "Mixed_6a.branch3x3"), chain(h, "Mixed_6a", ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3")),
                   F.max_pool2d(h, 3, stride=2)], 1)
    for blk in ("Mixed_6b", "Mixed_6c"):
        h = torch.cat([c(h, f"{blk}.branch1x1"), chain(h, blk, ("branch7x7_1", "branch7x7_2", "branch7x7_3")),
                       chain(h, blk, ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5")),
                       c(avg(h), f"{blk}.branch_pool")], 1)
    t = c(h, "Mixed_6d.branch1x1")[:, :SPATIAL_CHANNELS]                    # [B, 7, 17, 17]
    assert tuple(t.shape[1:]) == (SPATIAL_CHANNELS, SPATIAL_GRID, SPATIAL_GRID)
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)


def spatial_case_images():
    import fid_restatement as FR
    n, H, W, seed = SPATIAL_CASE
    return FR.smooth_images(n, H, W, seed)


def run_spatial(x, sd, autocast=False):
    import torch
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        return spatial_tap(x, sd).float()


def mint():
    import torch
    import fid_restatement as FR
    sd = FR.plain_state_dict()
    x = spatial_case_images()
    f32, f16 = run_spatial(x, sd), run_spatial(x, sd, autocast=True)
    assert torch.isfinite(f32).all() and float(f32.abs().max()) > 0
    out = {"what": "deviation of the restatement's spatial tap (Mixed_6d.branch1x1, channels 0..6) under torch.autocast('cpu', bfloat16) "
                   "from its fp32 run, rel-L2, on spatial_case_images()",
           "torch": torch.__version__, "case": list(SPATIAL_CASE), "spatial": FR.rel_l2(f16, f32),
           "mean_abs_fp32": float(f32.abs().mean()), "max_abs_fp32": float(f32.abs().max()), "nonzero_share_fp32": float((f32 > 0).float().mean())}
    print(out, flush=True)
    with open(GOLDEN_SPATIAL, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        import torch
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        mint()
