"""The LightningDiT recipe around the latent DiT restated in plain torch: the cosine term of the loss, the
shifted time grid, the guidance interval and Heun steps.

  * `flow_loss_cos64` / `flow_heun64`: fp64 references of tv_flow_loss_cos and tv_flow_heun with the slack / absolute terms of
    their line of DESIGN.md section 3.1 row E, and the bounds of the loss values;
  * `flow_loss_cos_emulate` / `flow_heun_emulate`: fp32 emulations in the kernels' own order of operations, and the same with named
    defects;
  * `time_grid`, `evaluations`, `sample`: the sampler with method / shift / interval; `flow_step`: one training step with the cosine
    term under autograd.

`python tests/recipe_restatement.py --mint` writes tests/golden/dit_recipe_ref_bf16_autocast.json: the restatement's OWN deviation
of the bf16-autocast form from fp32 for the whole-model and sampler cases of tests/test_recipe_gpu.py, with the seeds used.
"""
import json
import os
import sys

import torch

import dit_restatement as R
import lightning_restatement as LR
from dit_restatement import BF, F32, F64, U, fma32, patchify, rel_l2, round_up, unpatchify

COS_EPS = 1e-8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_recipe_ref_bf16_autocast.json")

# whole-model cases: the two of dit_restatement.MODEL_CASES and a LightningDiT (all three block features) of the first one's size
CASES = {"dit_f16d32_p1": (R, "f16d32_p1"), "dit_f8d16_p2": (R, "f8d16_p2"), "lightning_f16d32_p1": (LR, "f16d32_p1")}
COSINE_WEIGHT = 1.0
# steps = 4 at shift 0.3 puts the grid at 0, 1/11, 3/13, 9/19, 1: the interval's lower end 0.2 falls inside step 1
SAMPLER = dict(case="dit_f16d32_p1", steps=4, cfg_scale=1.5, timestep_shift=0.3, cfg_interval=(0.2, 1.0))
METHODS = ("euler", "heun")
FLOW_SHAPES = R.FLOW_SHAPES


# ---------------------------------------------------------------------------------------------------------------------------
# the sampler's schedule
# ---------------------------------------------------------------------------------------------------------------------------
def time_grid(steps, shift=1.0):
    """steps + 1 times in float64: u = i / steps, t = s u / (1 + (s - 1) u); t = 0 is noise"""
    out = []
    for i in range(steps + 1):
        u = i / steps
        out.append(shift * u / (1.0 + (shift - 1.0) * u))
    return out


def guided_at(t, cfg_scale, cfg_interval):
    return cfg_scale != 1.0 and cfg_interval[0] <= t <= cfg_interval[1]


def evaluations(steps, method="euler", shift=1.0, cfg_scale=1.0, cfg_interval=(0.0, 1.0)):
    """[(step, t, guided)] of every model evaluation of a sampling run, in order"""
    grid = time_grid(steps, shift)
    out = []
    for i in range(steps):
        out.append((i, grid[i], guided_at(grid[i], cfg_scale, cfg_interval)))
        if method == "heun":
            out.append((i, grid[i + 1], guided_at(grid[i + 1], cfg_scale, cfg_interval)))
    return out


@torch.no_grad()
def sample(model, labels, noise, stats, steps, cfg_scale, method="euler", shift=1.0, cfg_interval=(0.0, 1.0), autocast=False):
    dt_ = next(model.parameters()).dtype
    x = noise.to(dt_).clone()
    null = torch.full_like(labels, model.num_classes)
    grid = time_grid(steps, shift)

    def velocity(xx, tv):
        t = torch.full((labels.shape[0],), tv, dtype=dt_)
        with torch.autocast("cpu", dtype=BF, enabled=autocast):
            vc = model(xx, t, labels, bf16_stream=autocast).to(dt_)
            if guided_at(tv, cfg_scale, cfg_interval):
                vu = model(xx, t, null, bf16_stream=autocast).to(dt_)
                vc = vu + cfg_scale * (vc - vu)
        return vc
    for i in range(steps):
        dt = grid[i + 1] - grid[i]
        g1 = velocity(x, grid[i])
        if method == "heun":
            g2 = velocity(x + dt * g1, grid[i + 1])
            x = x + (dt / 2) * (g1 + g2)
        else:
            x = x + dt * g1
    return x * stats["std"].to(dt_) + stats["mean"].to(dt_)


# ---------------------------------------------------------------------------------------------------------------------------
# one training step with the cosine term
# ---------------------------------------------------------------------------------------------------------------------------
def cosine_term(v, target, eps=COS_EPS):
    """mean over the positions of 1 - cos across dim 1; a position with |v| <= eps has cos = 0 and passes no gradient (the
    project's rule: F.cosine_similarity under autograd would return target / (|target| eps) there)"""
    np2 = (v * v).sum(1)
    live = np2 > eps * eps
    n_p = torch.sqrt(torch.where(live, np2, torch.ones_like(np2)))
    n_v = target.norm(dim=1).clamp_min(eps)
    cos = torch.where(live, (v * target).sum(1) / (n_p * n_v), torch.zeros_like(np2))
    return (1 - cos).mean()


def flow_step(model, batch, cosine_weight=COSINE_WEIGHT, autocast=False):
    """dit_restatement.flow_step with `cosine_weight` times the cosine term -> (velocity, loss, mse, {name: grad})"""
    dt = next(model.parameters()).dtype
    mean, std = batch["stats"]["mean"].to(dt), batch["stats"]["std"].to(dt)
    x = (batch["latents"].to(dt) - mean) / std
    e, t = batch["noise"].to(dt), batch["t"].to(dt)
    tt = t.view(-1, 1, 1, 1)
    xt = tt * x + (1 - tt) * e
    model.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        v = model(xt, t, batch["labels"], bf16_stream=autocast)
    mse = ((v.to(dt) - (x - e)) ** 2).mean()
    loss = mse + cosine_weight * cosine_term(v.to(dt), x - e)
    loss.backward()
    return v.detach(), loss.detach(), mse.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------
def _pad(rows, ld):
    return torch.nn.functional.pad(rows, (0, ld - rows.shape[-1]))


def flow_loss_cos64(pred, lat, mean, rstd, noise, p, cos_weight, grad_scale=1.0, eps=COS_EPS):
    """-> {"mse_sum", "mse", "cos_sum", "cos", "total", "dpred", "slack", "bounds"}.

    Slack of dpred (bf16 once) and bounds of the values, u = 2^-24, from the kernel's operation count.  v carries
    dv = u (2 |x| + |v|) (the flow_loss row).  The three sums are fma chains of D terms: d(np2) = D u np2 (the prediction is exact),
    d(nv2) = sum 2 |v| dv + D u nv2, d(dot) = sum |p| dv + D u sum |p v|.  A reciprocal norm is formed in fp64 and rounded once:
    rel_p = d(np2) / (2 np2) + 2 u, rel_v likewise; d(cos) = d(dot) / (n_p n_v) + |cos| (rel_p + rel_v + u).
    gc = (v rv - (cos p) rp) rp: d(a) = dv rv + |a| (rel_v + u), d(b) = |p| rp d(cos) + |b| (rel_p + 2 u),
    d(gc) = (d(a) + d(b) + u |a - b|) rp + |gc| (rel_p + u).  The gradient is fma(-cc, gc, cm d) with both coefficients rounded once:
    slack = |cm| u (2 |x| + |v| + 3 |d|) + |cc| (d(gc) + 2 u |gc|) + u |dpred|.
    Values: the squared-error half as tv_flow_loss (1e-6 relative); the fp64 sum of 1 - cos adds nothing visible, so the cosine sum
    is within sum d(cos), its mean within that over the positions, and the total within the two joined."""
    B, D, h, w = lat.shape
    F_, pp = p * p * D, p * p
    ld = round_up(F_, 32)
    x = (lat.to(F64) - mean.to(F64).view(1, D, 1, 1)) * rstd.to(F64).view(1, D, 1, 1)
    v = patchify(x - noise.to(F64), p).reshape(-1, F_)
    xa = patchify(x.abs(), p).reshape(-1, F_)
    P = pred.to(F64)[:, :F_]
    d = P - v
    T = P.shape[0]
    count, npos = d.numel(), T * pp
    q = lambda a: a.reshape(T, pp, D)
    Pq, Vq = q(P), q(v)
    dv = q(U * (2 * xa + v.abs()))
    np2, nv2, dot = (Pq * Pq).sum(-1, keepdim=True), (Vq * Vq).sum(-1, keepdim=True), (Pq * Vq).sum(-1, keepdim=True)
    n_p, n_v = np2.sqrt(), nv2.sqrt().clamp_min(eps)
    live = n_p > eps
    n_ps = torch.where(live, n_p, torch.ones_like(n_p))
    cos = torch.where(live, dot / (n_ps * n_v), torch.zeros_like(dot))
    a, b = Vq / n_v, cos * Pq / n_ps
    gc = torch.where(live, (a - b) / n_ps, torch.zeros_like(Pq))
    cm, cc = 2.0 * grad_scale / count, grad_scale * cos_weight / npos
    dpred = cm * d - cc * gc.reshape(T, F_)
    d_np2 = D * U * np2
    d_nv2 = (2 * Vq.abs() * dv).sum(-1, keepdim=True) + D * U * nv2
    d_dot = (Pq.abs() * dv).sum(-1, keepdim=True) + D * U * (Pq * Vq).abs().sum(-1, keepdim=True)
    rel_p = d_np2 / (2 * n_ps * n_ps) + 2 * U
    rel_v = d_nv2 / (2 * n_v * n_v) + 2 * U
    d_cos = torch.where(live, d_dot / (n_ps * n_v) + cos.abs() * (rel_p + rel_v + U), torch.zeros_like(dot))
    d_a = dv / n_v + a.abs() * (rel_v + U)
    d_b = Pq.abs() / n_ps * d_cos + b.abs() * (rel_p + 2 * U)
    d_gc = torch.where(live, (d_a + d_b + U * (a - b).abs()) / n_ps + gc.abs() * (rel_p + U), torch.zeros_like(Pq))
    slack = abs(cm) * U * (2 * xa + v.abs() + 3 * d.abs()) + abs(cc) * (d_gc + 2 * U * gc.abs()).reshape(T, F_) + U * dpred.abs()
    mse_sum, cos_sum = float((d * d).sum()), float((1 - cos).sum())
    b_cos = float(d_cos.sum()) + 1e-13 * npos
    bounds = {"mse_sum": 1e-6 * mse_sum, "mse": 1e-6 * mse_sum / count, "cos_sum": b_cos, "cos": b_cos / npos,
              "total": 1e-6 * mse_sum / count + cos_weight * b_cos / npos}
    return {"mse_sum": mse_sum, "mse": mse_sum / count, "cos_sum": cos_sum, "cos": cos_sum / npos,
            "total": mse_sum / count + cos_weight * cos_sum / npos, "dpred": _pad(dpred, ld), "slack": _pad(slack, ld), "bounds": bounds,
            "live": live}


VALUE_KEYS = ("mse_sum", "mse", "cos_sum", "cos", "total")


def values_ratio(got, ref):
    """max over the five values of |got - ref| / bound (`got`: the kernel's out vector or an emulation's dict)"""
    if not isinstance(got, dict):
        got = dict(zip(VALUE_KEYS, [float(g) for g in got]))
    return max(abs(got[k] - ref[k]) / (ref["bounds"][k] + 1e-300) for k in VALUE_KEYS)


def _velocity64(v, BN, F_, s, guided):
    v = v.to(F64)[:, :F_]
    vc = v[:BN]
    if not guided:
        return vc, torch.zeros_like(vc)
    vu = v[BN:2 * BN]
    inner = s * (vc - vu)
    return vu + inner, inner


def flow_heun64(x, v1, v2, p, dt, cfg_scale=1.0, guided1=False, guided2=False):
    """x holds the predictor's result -> (x' 64, absterms for fp32_ratio with c = 1): one rounding each for the inner difference and the
    fma of a guided velocity, one for g2 - g1; the last fma's is the criterion's own u |x'|"""
    B, D, h, w = x.shape
    F_ = p * p * D
    N = (h // p) * (w // p)
    g1, i1 = _velocity64(v1, B * N, F_, cfg_scale, guided1)
    g2, i2 = _velocity64(v2, B * N, F_, cfg_scale, guided2)
    un = lambda r: unpatchify(r.reshape(B, N, F_), D, h, w, p)
    return x.to(F64) + (dt / 2) * un(g2 - g1), abs(dt / 2) * un(i1.abs() + g1.abs() * bool(guided1) + i2.abs() + g2.abs() * bool(guided2) + (g2 - g1).abs())


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' own order (defect=...: the same with a named defect)
# ---------------------------------------------------------------------------------------------------------------------------
def flow_loss_cos_emulate(pred, lat, mean, rstd, noise, p, cos_weight, grad_scale=1.0, defect=None):
    """-> ({the five values}, dpred bf16 [B N, ld]).  defects: "neighbour_norm" (a position reads the next position's |p|^2),
    "count_mse" (the cosine term divided by the element count instead of the position count)"""
    B, D, h, w = lat.shape
    F_, pp = p * p * D, p * p
    ld = round_up(F_, 32)
    v = patchify(R._x32(lat, mean, rstd) - noise.to(F32), p).reshape(-1, F_)
    P = pred.to(F32)[:, :F_]
    d = P - v
    T = P.shape[0]
    count, npos = d.numel(), T * pp
    Pq, Vq = P.reshape(T, pp, D), v.reshape(T, pp, D)
    np2, nv2, dot = (torch.zeros(T, pp, dtype=F32) for _ in range(3))
    for c in range(D):
        np2, nv2, dot = fma32(Pq[..., c], Pq[..., c], np2), fma32(Vq[..., c], Vq[..., c], nv2), fma32(Pq[..., c], Vq[..., c], dot)
    if defect == "neighbour_norm":
        np2 = np2.reshape(-1).roll(-1).reshape(T, pp)
    np2_, nvc, dot_ = np2.to(F64), nv2.to(F64).clamp_min(COS_EPS * COS_EPS), dot.to(F64)
    live = np2_ > COS_EPS * COS_EPS
    safe = torch.where(live, np2_, torch.ones_like(np2_))
    cos = torch.where(live, dot_ / torch.sqrt(safe * nvc), torch.zeros_like(dot_)).to(F32)
    rp, rv = (1.0 / torch.sqrt(safe)).to(F32), (1.0 / torch.sqrt(nvc)).to(F32)
    gc = (Vq * rv[..., None] - (cos[..., None] * Pq) * rp[..., None]) * rp[..., None]
    if defect == "count_mse":
        npos = count
    cm = torch.tensor(2.0 * grad_scale / count, dtype=F64).to(F32)
    cc = torch.tensor(grad_scale * cos_weight / npos, dtype=F64).to(F32)
    gr = (cm * d).reshape(T, pp, D)
    gr = torch.where(live[..., None], fma32((-cc).expand_as(gc), gc, gr), gr).reshape(T, F_)
    mse_sum, cos_sum = float((d.to(F64) * d.to(F64)).sum()), float((1.0 - cos.to(F64)).sum())
    vals = {"mse_sum": mse_sum, "mse": mse_sum / count, "cos_sum": cos_sum, "cos": cos_sum / npos,
            "total": mse_sum / count + cos_weight * (cos_sum / npos)}
    return vals, _pad(gr.to(BF), ld)


def _velocity32(v, BN, F_, s, guided):
    v = v.to(F32)[:, :F_]
    vc = v[:BN]
    if not guided:
        return vc
    vu = v[BN:2 * BN]
    return fma32(torch.tensor(s, dtype=F32).expand_as(vc), vc - vu, vu)


def flow_heun_emulate(x, v1, v2, p, dt, cfg_scale=1.0, guided1=False, guided2=False, defect=None):
    """defects: "swap_guided" (each evaluation combined by the other's flag; hand both buffers 2 B N rows), "full_dt" (dt for dt / 2)"""
    B, D, h, w = x.shape
    F_ = p * p * D
    N = (h // p) * (w // p)
    if defect == "swap_guided":
        guided1, guided2 = guided2, guided1
    g1, g2 = _velocity32(v1, B * N, F_, cfg_scale, guided1), _velocity32(v2, B * N, F_, cfg_scale, guided2)
    hdt = torch.tensor(dt, dtype=F32) * (1.0 if defect == "full_dt" else 0.5)
    return fma32(hdt.expand_as(x), unpatchify((g2 - g1).reshape(B, N, F_), D, h, w, p), x.to(F32))


def recipe_inputs(B, D, h, w, p, seed):
    """dit_restatement.flow_inputs plus a second pair of velocity rows, and one prediction position and one target position zeroed"""
    f = R.flow_inputs(B, D, h, w, p, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    f["v2b"] = torch.randn(2 * B * f["N"], f["ld"], generator=g).to(BF)
    f["pred"] = f["pred"].clone()
    f["pred"][1, :D] = 0                     # a zero prediction at one position: cos = 0 there, the squared-error gradient alone
    return f


# ---------------------------------------------------------------------------------------------------------------------------
def case_parts(name):
    mod, case = CASES[name]
    return mod, case


def mint(write=True):
    """the golden file's content; write=False: computed only (the host test compares it with the committed file)"""
    out ={"cosine_weight": COSINE_WEIGHT, "cases": {}, "sampler": {}}
    for i, name in enumerate(CASES):
        mod, case = case_parts(name)
        seeds = {"state": 500 + i, "batch": 600 + i}
        sd, batch = mod.make_state(case, seeds["state"], True), mod.make_batch(case, seeds["batch"])
        v32, l32, m32, g32 = flow_step(mod.build(case, sd), batch)
        v16, l16, m16, g16 = flow_step(mod.build(case, sd), batch, autocast=True)
        out["cases"][name] = {"seeds": seeds, "loss_fp32": float(l32), "mse_fp32": float(m32), "loss": abs(float(l16) - float(l32)) / float(l32),
                              "grads": {k: rel_l2(g16[k], g32[k]) for k in g32}}
    mod, case = case_parts(SAMPLER["case"])
    seeds = {"state": 700, "batch": 701}
    sd, batch = mod.make_state(case, seeds["state"], True), mod.make_batch(case, seeds["batch"])
    out["sampler"] = dict(SAMPLER, seeds=seeds, latents={})
    for method in METHODS:
        args = (batch["labels"], batch["noise"], batch["stats"], SAMPLER["steps"], SAMPLER["cfg_scale"], method, SAMPLER["timestep_shift"],
                SAMPLER["cfg_interval"])
        out["sampler"]["latents"][method] = rel_l2(sample(mod.build(case, sd), *args, autocast=True), sample(mod.build(case, sd), *args))
    out = json.loads(json.dumps(out))
    if write:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    return out


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.manual_seed(0)
        res = mint()
        print(json.dumps(res["sampler"], indent=1))
        for name, c in res["cases"].items():
            print(name, "loss", c["loss"], "max grad dev", max(c["grads"].values()))
