"""Plain fp64 restatement of the generation metrics (csrc/genmetrics.hip, transvae/metrics_gen.py, tv_opt_ema): references, the
fp32 chain emulation with optional planted defects, the bounds of DESIGN.md section 3.1 row S and the seeded input recipe."""
import math

import numpy as np

U = 2.0 ** -24            # fp32 unit roundoff
U64 = 2.0 ** -53

# (N, M, d, k, seed): the pairwise cases; hits / misses / undecided of the fp64 reference alone with make_inputs below: 49/21/0, 7/2/0,
# 189/68/0, 3/2/0.  These counts are this recipe's own (numpy's default_rng, the draws in the order of make_inputs); another
# generator or draw order gives other counts.  What the cases have to meet is asserted in tests/test_gen_host.py: an undecided
# share of at most 1 % and both outcomes present.
SHAPES = ((130, 70, 2048, 3, 0), (65, 9, 37, 1, 1), (257, 257, 64, 8, 2), (4, 5, 2048, 3, 3))
UNDECIDED_MAX = 0.01


def shape_id(s):
    return "x".join(map(str, s))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: non-negative, low-intrinsic-dimension rows, like pool3 features; the queries are half inside, half a wider, shifted draw
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(N, M, d, seed, shift=0.0):
    """(x [N, d], q [M, d]) fp32; `shift` is added to every coordinate of both (rounded once)"""
    g = np.random.default_rng(seed)
    A = g.standard_normal((8, d))

    def draw(n, scale, loc):
        z = (g.standard_normal((n, 8)) * scale + loc) @ A / math.sqrt(8.0) + 0.1 * g.standard_normal((n, d)) + 0.5
        return np.maximum(z, 0.0).astype(np.float32)

    x = draw(N, 1.0, 0.0)
    q = np.concatenate([draw(M - M // 2, 1.0, 0.0), draw(M // 2, 1.6, 0.7)], 0)
    if shift:
        x, q = (x + np.float32(shift)).astype(np.float32), (q + np.float32(shift)).astype(np.float32)
    return x, q


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------
def sqdist64(a, b):
    """[len(a), len(b)] squared distances by direct differences in fp64 (row blocks keep the temporary small)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(0, a.shape[0], 16):
        out[i:i + 16] = ((a[i:i + 16, None, :] - b[None, :, :]) ** 2).sum(-1)
    return out


def kth_excluding_self(D, k, i0=0):
    """row r of D [M, N] belongs to point i0 + r: the k-th smallest entry of the row with column i0 + r left out"""
    D = np.array(D, copy=True)
    D[np.arange(D.shape[0]), i0 + np.arange(D.shape[0])] = np.inf
    return np.sort(D, axis=1)[:, k - 1]


def knn_radius64(x, k, i0=0, M=None):
    M = x.shape[0] - i0 if M is None else M
    return kth_excluding_self(sqdist64(x[i0:i0 + M], x), k, i0)


def hits64(q, x, r2):
    return (sqdist64(q, x) <= np.asarray(r2, dtype=np.float64)[None, :]).any(1).astype(np.int32)


def precision_recall64(real, fake, k):
    r_real, r_fake = knn_radius64(real, k), knn_radius64(fake, k)
    return {"precision": float(hits64(fake, real, r_real).mean()), "recall": float(hits64(real, fake, r_fake).mean())}


def classify_hits(q, x, r2):
    """per query: 1 decided inside, 0 decided outside, -1 undecided, with tau = (d + 2) u around every radius"""
    tau = radius_bound(x.shape[1])
    D = sqdist64(q, x)
    r = np.asarray(r2, dtype=np.float64)[None, :]
    inside = (D <= r * (1 - tau)).any(1)
    outside = (D > r * (1 + tau)).all(1)
    return np.where(inside, 1, np.where(outside, 0, -1))


def frechet_rows64(f1, f2):
    """Frechet distance between two feature sets [n1, d], [n2, d] from the rows alone, fp64, for any rank (n <= d included).
    With the centred rows C_i, S_i = C_i^T C_i / (n_i - 1), so the non-zero eigenvalues of S1 S2 are those of (C1 C2^T)(C1 C2^T)^T
    / ((n1 - 1)(n2 - 1)): tr (S1 S2)^(1/2) is the sum of the singular values of the n1 x n2 matrix C1 C2^T over
    sqrt((n1 - 1)(n2 - 1)), and tr S_i = |C_i|_F^2 / (n_i - 1).  No d x d matrix, no square root of rounding noise in a null space."""
    f1, f2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    mu1, mu2 = f1.mean(0), f2.mean(0)
    c1, c2 = f1 - mu1, f2 - mu2
    n1, n2 = f1.shape[0] - 1, f2.shape[0] - 1
    tr_sqrt = np.linalg.svd(c1 @ c2.T, compute_uv=False).sum() / math.sqrt(n1 * n2)
    return float(((mu1 - mu2) ** 2).sum() + (c1 ** 2).sum() / n1 + (c2 ** 2).sum() / n2 - 2.0 * tr_sqrt)


def frechet_null_space_noise(f1, f2):
    """What fid_restatement.frechet_numpy may be off by on rank-deficient sets (n <= d; its docstring asks for n > d).  eigh returns
    the zero eigenvalues of S1 as values up to d eps l1 in size (l_i = the largest eigenvalue of S_i); the positive ones survive the
    clip, so S1^(1/2) carries up to sqrt(d eps l1) in each null direction and m = S1^(1/2) S2 S1^(1/2) spurious eigenvalues up to
    d eps l1 l2, the size of eigvalsh's own error on m as well.  Each of up to d such values adds its square root, sqrt(d eps l1 l2),
    to tr sqrt, which enters the distance twice: 2 d sqrt(d eps l1 l2).  On full-rank sets the true eigenvalues dwarf these and the
    function's 1e-8 trace tolerance holds; here the bound is what its own arithmetic allows."""
    def top(f):
        f = np.asarray(f, dtype=np.float64)
        return float(np.linalg.norm(f - f.mean(0), 2) ** 2 / (f.shape[0] - 1))
    d = np.asarray(f1).shape[1]
    return 2.0 * d * math.sqrt(d * np.finfo(np.float64).eps * top(f1) * top(f2))


def softmax_stats64(logits, state=None):
    """the state {rows, sum_rows sum_k p log p, sum_rows p_k} after adding the fp32 logits' rows one at a time, fp64"""
    z = np.asarray(logits, dtype=np.float64)
    K = z.shape[1]
    st = np.zeros(2 + K) if state is None else np.array(state, dtype=np.float64, copy=True)
    for row in z:
        t = row - row.max()
        e = np.exp(t)
        s = 0.0
        for v in e:
            s += v
        p, lp = e / s, t - math.log(s)
        a = 0.0
        for v in p * lp:
            a += v
        st[0] += 1.0
        st[1] += a
        st[2:] += p
    return st


def softmax_stats_bound(logits):
    """per state entry: 16 K 2^-53 times the sum of the absolute terms of that entry"""
    z = np.asarray(logits, dtype=np.float64)
    K = z.shape[1]
    t = z - z.max(1, keepdims=True)
    p = np.exp(t) / np.exp(t).sum(1, keepdims=True)
    lp = t - np.log(np.exp(t).sum(1, keepdims=True))
    mag = np.concatenate([[0.0, np.abs(p * lp).sum()], p.sum(0)])
    return 16 * K * U64 * mag


def inception_score64(features, weight, bias=None):
    """exp(mean_i KL(p_i || pbar)) with p = softmax(features W^T + b), fp64, the whole set"""
    z = np.asarray(features, dtype=np.float64) @ np.asarray(weight, dtype=np.float64).T
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)
    return score64(z)


def score64(z):
    t = z - z.max(1, keepdims=True)
    lp = t - np.log(np.exp(t).sum(1, keepdims=True))
    p = np.exp(lp)
    pbar = p.mean(0)
    nz = pbar > 0
    return float(math.exp((p * lp).sum() / z.shape[0] - (pbar[nz] * np.log(pbar[nz])).sum()))


def ema64(ema, w, a32):
    """ema + a (w - ema) in fp64 with the fp32 factor the kernel is given"""
    e, w = np.asarray(ema, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return e + float(np.float32(a32)) * (w - e)


# ---------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------
def radius_bound(d):
    """relative: a chain of d non-negative terms, each (a - b)^2 carrying two roundings before it is added"""
    return (d + 2) * U


def ema_bound(ema, w):
    return 2 * U * (np.abs(np.asarray(w, dtype=np.float64)) + np.abs(np.asarray(ema, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 chain, emulated on the host (unfused: the square is rounded before it is added), with planted defects
# ---------------------------------------------------------------------------------------------------------------------------
def sqdist32(a, b, gram=False):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if gram:                                              # |a|^2 + |b|^2 - 2 a.b, every step fp32
        na = np.zeros(a.shape[0], dtype=np.float32)
        nb = np.zeros(b.shape[0], dtype=np.float32)
        ab = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
        for c in range(a.shape[1]):
            na = na + a[:, c] * a[:, c]
            nb = nb + b[:, c] * b[:, c]
            ab = ab + a[:, c, None] * b[None, :, c]
        return (na[:, None] + nb[None, :]) - np.float32(2) * ab
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for c in range(a.shape[1]):
        df = a[:, c, None] - b[None, :, c]
        acc = acc + df * df
    return acc


def knn_radius32(x, k, i0=0, M=None, gram=False, keep_self=False, off_by_one=False):
    """defects: gram = the Gram form; keep_self = self is not excluded; off_by_one = the (k + 1)-th instead of the k-th"""
    M = x.shape[0] - i0 if M is None else M
    D = sqdist32(x[i0:i0 + M], x, gram=gram).astype(np.float64)
    kk = k + 1 if off_by_one else k
    if keep_self:
        return np.sort(D, axis=1)[:, kk - 1].astype(np.float32)
    return kth_excluding_self(D, kk, i0).astype(np.float32)


def hits32(q, x, r2, gram=False, strict=False):
    """defects: gram; strict = `<` instead of `<=`"""
    D = sqdist32(q, x, gram=gram)
    r = np.asarray(r2, dtype=np.float32)[None, :]
    return ((D < r) if strict else (D <= r)).any(1).astype(np.int32)


def check_radii(got, x, k, i0=0, M=None):
    """None, or a message: every radius within (d + 2) u of fp64"""
    ref = knn_radius64(x, k, i0, M)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bad = ~(err <= radius_bound(x.shape[1]) * ref)
    if bad.any():
        i = int(np.argmax(np.where(ref > 0, err / np.where(ref > 0, ref, 1), np.where(err > 0, np.inf, 0))))
        return f"{int(bad.sum())} of {ref.shape[0]} radii outside (d + 2) u; worst at {i}: got {float(got[i])!r}, fp64 {ref[i]!r}"
    return None


def check_hits(got, q, x, r2):
    """(message or None, undecided share): the kernel agrees on every decided query"""
    cls = classify_hits(q, x, r2)
    got = np.asarray(got)
    decided = cls >= 0
    wrong = decided & (got != cls)
    if ((got != 0) & (got != 1)).any():
        return "hit values other than 0 / 1", float((~decided).mean())
    msg = f"{int(wrong.sum())} decided queries disagree, first {int(np.argmax(wrong))}" if wrong.any() else None
    return msg, float((~decided).mean())
