"""Plain-torch float64 restatement of transvae/latents.py: the log-domain Gaussian kernel density estimate, the three density
metrics and the streaming moments, plus the contract bound of DESIGN.md section 3.1 row T and an fp32 emulation of the kernel's
order of operations (with switchable defects, for the mutation tests of tests/test_latents_host.py)."""
import math

import numpy as np
import torch

U = 2.0 ** -24


def kde_k(n: int) -> float:
    """k(N) of row T: 4 ln N (exponent a_j = -inv (dist_j - dmin): the rounding of the difference, of the product, of a_j log2 e,
    and the constant's own error, each |a_j| u, weighted sum_j p_j |a_j| <= ln N) + 2 (v_exp_f32, 1 ulp) + 3 (the fp32 tree over 8
    terms) + ln N (final rounding of |out| <= |m| + ln N; the |m| part sits in the first term) + 1 (everything done in fp64: running
    sum, rescales, log)."""
    return 5.0 * math.log(max(n, 2)) + 6.0


def sqdist64(q: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    q, x = q.double(), x.double()
    dist = torch.zeros(q.shape[0], x.shape[0], dtype=torch.float64)
    for k in range(x.shape[1]):
        dist += (q[:, k:k + 1] - x[None, :, k]) ** 2
    return dist


def log_density64(x: torch.Tensor, q=None, h: float = 1.0, exclude_self: bool = False):
    """(l64 [M], sum_j p_ij |s_ij| [M]) in float64 from the fp32 inputs as given."""
    qq = x if q is None else q
    s = -sqdist64(qq, x) / (2.0 * h * h)
    if exclude_self:
        s.fill_diagonal_(-math.inf)
    l64 = torch.logsumexp(s, dim=1)
    p = torch.exp(s - l64[:, None])
    spread = (p * torch.where(torch.isinf(s), torch.zeros_like(s), s.abs())).sum(1)
    return l64, spread


def kde_bound(x, q=None, h: float = 1.0, exclude_self: bool = False):
    """(l64, bound): |out_i - l64_i| <= u (d + 3) sum_j p_ij |s_ij| + k(N) u"""
    l64, spread = log_density64(x, q, h, exclude_self)
    d, n = x.shape[1], x.shape[0]
    return l64, U * (d + 3) * spread + kde_k(n) * U


def kde_ratio(out: torch.Tensor, x, q=None, h: float = 1.0, exclude_self: bool = False) -> float:
    """worst |out - l64| / bound; inf when an output is not finite"""
    l64, bound = kde_bound(x, q, h, exclude_self)
    out = out.double().cpu()
    if not bool(torch.isfinite(out).all()):
        return math.inf
    return float(((out - l64).abs() / bound).max())


def scott(n: int, d: int) -> float:
    return float(n) ** (-1.0 / (d + 4))


def emulate_fp32(x: torch.Tensor, q=None, h: float = 1.0, exclude_self: bool = False, defect=None) -> torch.Tensor:
    """fp32 emulation: sequential chain over k of direct differences, score = -inv * dist, torch.logsumexp in fp32.
    defect: None | "bf16_inputs" | "gram" | "keep_self" | "no_max"."""
    x = x.float()
    qq = x if q is None else q.float()
    if defect == "bf16_inputs":
        x, qq = x.bfloat16().float(), qq.bfloat16().float()
    inv = torch.tensor(1.0 / (2.0 * h * h), dtype=torch.float32)
    if defect == "gram":
        dist = (qq * qq).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * (qq @ x.T)
    else:
        dist = torch.zeros(qq.shape[0], x.shape[0], dtype=torch.float32)
        for k in range(x.shape[1]):
            t = qq[:, k:k + 1] - x[None, :, k]
            dist = torch.addcmul(dist, t, t)
    s = -inv * dist
    if exclude_self and defect != "keep_self":
        s.fill_diagonal_(-math.inf)
    if defect == "no_max":
        return torch.log(torch.exp(s).sum(1))
    return torch.logsumexp(s, dim=1)


def metrics64(logdens: torch.Tensor):
    """{"density_cv", "normalized_entropy", "gini"} of f = exp(l - max l) in float64"""
    ld = logdens.double().cpu()
    n = ld.shape[0]
    f = torch.exp(ld - ld.max())
    cv = float(torch.sqrt(((f - f.mean()) ** 2).mean()) / f.mean())
    p = f / f.sum()
    nz = p > 0
    ent = float(-(p[nz] * torch.log(p[nz])).sum() / math.log(n))
    fs = torch.sort(f).values
    i = torch.arange(1, n + 1, dtype=torch.float64)
    gini = float(((2 * i - n - 1) * fs).sum() / (n * fs.sum()))
    return {"density_cv": cv, "normalized_entropy": ent, "gini": gini}


def prepare_points64(points: torch.Tensor, standardize=True, pca=None) -> torch.Tensor:
    """the standardisation and the PCA projection of latent_density_metrics, rounded to fp32 where the package rounds"""
    x = points.float().cpu()
    n = x.shape[0]
    if standardize:
        x64 = x.double()
        sd = x64.std(0, unbiased=False)
        x = ((x64 - x64.mean(0)) / torch.where(sd > 0, sd, torch.ones_like(sd))).float()
    if pca is not None:
        x64 = x.double()
        xc = x64 - x64.mean(0)
        _, vec = torch.linalg.eigh(xc.T @ xc / n)
        x = (x - x64.mean(0).float()) @ vec[:, -pca:].flip(1).float()
    return x


def density_metrics64(points, bandwidth="scott", standardize=True, pca=None, leave_one_out=True):
    x = prepare_points64(points, standardize, pca)
    n, d = x.shape
    h = scott(n, d) if bandwidth == "scott" else float(bandwidth)
    l64, _ = log_density64(x, None, h, leave_one_out)
    res = metrics64(l64)
    res.update({"bandwidth": h, "n": n, "d": d})
    return res


def moments64(latents: np.ndarray):
    """(n, mean [D], population covariance [D, D]) of latents [B, D, ...] over every (image, position) sample, NumPy float64"""
    a = np.asarray(latents, dtype=np.float64)
    D = a.shape[1]
    rows = np.moveaxis(a.reshape(a.shape[0], D, -1), 1, 2).reshape(-1, D)
    mean = rows.mean(0)
    c = rows - mean
    return rows.shape[0], mean, c.T @ c / rows.shape[0]


def rel_fro(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
