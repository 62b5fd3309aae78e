"""The train step around the HIP path on the GPU (`-m gpu`): several optimizer steps against the fp32 CPU oracle,
the non-finite guard, the reference trainers' autocast call style, and the N>1 code path with the REAL model
(two ranks over gloo sharing cuda:0 -- RCCL refuses two ranks per device; the DDP hooks, bucket views, no_sync and the
fused autograd Functions are the same).

Reference call pattern: R/train.py:557-646 (accumulate, clip, AdamW), R/train_2.py:266-273,303-338 (bf16 policy,
logvar clamp, skip on non-finite), P/.../transvae.py:186-196,243-245 (clamps)."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import filler
from oracle import transvae_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def micro_model(**kw):
    from transvae import TransVAE
    m = TransVAE(config=dict(O.MICRO), variant="micro", compression_ratio=16, latent_dim=4, **kw)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(O.MICRO, latent_dim=4)))
    return m.to(DEV)


def make_optimizer(params, kind, lr):
    if kind == "torch":
        return torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.95), weight_decay=0.0, fused=True)
    from transvae.optim import FusedAdamW
    return FusedAdamW(params, lr=lr, betas=(0.9, 0.95), weight_decay=0.0)


def optimizer_kinds():
    kinds = ["torch"]
    try:
        import transvae.optim  # noqa: F401
        kinds.append("hip")
    except ImportError:
        pass
    return kinds


@pytest.mark.parametrize("kind", optimizer_kinds())
def test_train_steps_follow_the_oracle(kind):
    """10 optimizer steps of transvae.parallel.train_step (2 micro-batches per step, packed-weight cache on, clip 1.0,
    AdamW lr 1e-4) on the micro model against the fp32 oracle + torch.optim.AdamW on the same weights, images and noise
    stream.  bf16 tier: every step's loss within 1e-2 relative of the oracle's (measured ~1e-3), gradient norms within
    5 %, the loss falls, nothing is skipped.  This is the test that clears the kernels of the round-1 NaN."""
    from transvae.parallel import train_step, vae_bench_loss
    steps, B, mb, lr = 10, 4, 2, 1e-4
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, 64, 64, generator=g)
    eps_all = torch.randn(steps, B, 4, 4, 4, generator=g)

    # ---- oracle: fp32 CPU, one full batch per step
    cfg = dict(O.MICRO)
    sd = filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4))
    sd = {k: v.clone().requires_grad_(not k.endswith("inv_freq")) for k, v in sd.items()}
    params = [v for v in sd.values() if v.requires_grad]
    opt_ref = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.95), weight_decay=0.0)
    ref_loss, ref_norm = [], []
    for s in range(steps):
        opt_ref.zero_grad()
        recon, mu, logvar = O.forward(x, sd, cfg, eps_all[s], clamp=True)
        loss = O.bench_loss(recon, x, mu, logvar, clamp_logvar=True)
        loss.backward()
        ref_norm.append(float(torch.nn.utils.clip_grad_norm_(params, 1.0)))
        opt_ref.step()
        ref_loss.append(float(loss.detach()))

    # ---- HIP path: two micro-batches per step through train_step
    m = micro_model(clamp_latent=True)
    m.train()
    opt = make_optimizer(m.parameters(), kind, lr)
    xd = x.to(DEV)
    counters = {}
    got_loss, got_norm = [], []
    for s in range(steps):
        it = iter([eps_all[s, :mb].to(DEV), eps_all[s, mb:].to(DEV)])

        def forward_loss(model, xb):
            recon, mu, logvar = model(xb, eps=next(it))
            return vae_bench_loss(recon, xb, mu, logvar)
        got_loss.append(train_step(m, opt, xd, mb, forward_loss, 1.0, B, counters))
        got_norm.append(counters["grad_norm"])
    got_loss = [float(v) for v in got_loss]
    got_norm = [float(v) for v in got_norm]
    print("oracle loss", np.round(ref_loss, 4), "\nhip    loss", np.round(got_loss, 4))
    print("oracle |g| ", np.round(ref_norm, 4), "\nhip    |g| ", np.round(got_norm, 4))
    assert float(counters["skipped"]) == 0
    assert all(np.isfinite(got_loss)) and got_loss[-1] < got_loss[0] - 0.05
    for s in range(steps):
        assert abs(got_loss[s] - ref_loss[s]) < 1e-2 * ref_loss[s], (s, got_loss[s], ref_loss[s])
        assert abs(got_norm[s] - ref_norm[s]) < 5e-2 * ref_norm[s], (s, got_norm[s], ref_norm[s])
    # after 10 AdamW steps the weights have moved by ~steps * lr per element; both runs moved the same way
    moved, agree = 0.0, 0.0
    p0 = filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4))
    for k, p in m.named_parameters():
        d_hip = (p.detach().cpu().double() - p0[k].double()).flatten()
        d_ref = (sd[k].detach().double() - p0[k].double()).flatten()
        moved += float(d_ref.norm() ** 2)
        agree += float((d_hip - d_ref).norm() ** 2)
    # measured 0.13-0.16: Adam's first updates are sign-like (m / sqrt(v) ~ +-1), so bf16 noise on near-zero gradient entries
    # flips whole steps of lr; the loss and gradient-norm trajectories above are the tight check
    assert agree / moved < 0.25 ** 2, (agree / moved) ** 0.5


def test_in_place_gradient_accumulation_equals_autograd_accumulation():
    """Micro-batches after the first add their weight / bias gradients straight into param.grad (tv_wgrad_tn_acc) instead of
    returning them to autograd.  Three micro-batches with and without that mode give the same gradients (fp32 summation
    order only), and the in-place mode really engaged (autograd saw no gradient for the convolution weights)."""
    from transvae.hip import ops
    from transvae.parallel import vae_bench_loss
    g = torch.Generator().manual_seed(2)
    x = torch.rand(3, 3, 64, 64, generator=g).to(DEV)
    eps = torch.randn(3, 4, 4, 4, generator=g).to(DEV)
    res = []
    for in_place in (False, True):
        m = micro_model(clamp_latent=True)
        m.train()
        for i in range(3):
            with ops.accumulate_grads_in_place(in_place and i > 0):
                recon, mu, logvar = m(x[i:i + 1], eps=eps[i:i + 1])
                (vae_bench_loss(recon, x[i:i + 1], mu, logvar) / 3).backward()
        res.append({k: p.grad.detach().clone() for k, p in m.named_parameters()})
    for k in res[0]:
        a, b = res[0][k].double(), res[1][k].double()
        assert float((a - b).norm()) <= 1e-5 * float(a.norm()) + 1e-9, k
    # the mode engaged: micro-batches 2 and 3 added most weight gradients in place (what stays with autograd: the folded
    # qkv / proj_in projections, the 2x2 DC weights, the padded stem / head weights)
    m = micro_model(clamp_latent=True)
    m.train()
    per_mb = []
    for i in range(3):
        before = dict(ops.acc_stats)
        with ops.accumulate_grads_in_place(i > 0):
            recon, mu, logvar = m(x[i:i + 1], eps=eps[i:i + 1])
            (vae_bench_loss(recon, x[i:i + 1], mu, logvar) / 3).backward()
        per_mb.append({k: ops.acc_stats[k] - before[k] for k in before})
    print("weight gradients per micro-batch (in place / through autograd):", per_mb)
    assert per_mb[0]["in_place"] == 0 and per_mb[1]["in_place"] > per_mb[1]["autograd"] and per_mb[2] == per_mb[1]


def test_train_step_micro_batches_equal_one_batch_and_accumulators_are_swapped():
    """transvae.parallel.train_step over four micro-batches of one image: the kernels add the GEMM layers' gradients in place,
    every other parameter's accumulator is taken out for the backward pass and added back by ONE multi-tensor add
    (parallel._swap_out_autograd_grads) -- the gradients equal those of the same four images in one micro-batch (fp32
    summation order), for two consecutive steps (the first in-place micro-batch of a process still runs the old way and
    teaches which parameters the kernels own)."""
    from transvae import parallel
    from transvae.hip import ops
    from transvae.parallel import train_step, vae_bench_loss
    g = torch.Generator().manual_seed(9)
    x = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    eps = torch.randn(4, 4, 4, 4, generator=g).to(DEV)
    res = {}
    for micro in (4, 1):
        m = micro_model(clamp_latent=True)
        m.train()
        opt = torch.optim.SGD(m.parameters(), lr=0.0)        # the parameters stay put: both steps see the same gradients
        cursor = [0]

        def forward_loss(model, xb):
            e = eps[cursor[0]:cursor[0] + xb.shape[0]]
            cursor[0] += xb.shape[0]
            recon, mu, logvar = model(xb, eps=e)
            return vae_bench_loss(recon, xb, mu, logvar)
        before = dict(parallel.swap_stats)
        out = []
        for _ in range(2):
            cursor[0] = 0
            loss = train_step(m, opt, x, micro, forward_loss, None, 4, {})
            out.append((float(loss), {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}))
        res[micro] = out
        if micro == 1:
            engaged = parallel.swap_stats["micro_batches"] - before["micro_batches"]
            tensors = parallel.swap_stats["tensors"] - before["tensors"]
            print("micro-batches with swapped accumulators:", engaged, " tensors swapped:", tensors, " parameters the kernels own:", len(ops.in_place_params))
            assert engaged >= 5 and tensors > 0 and len(ops.in_place_params) > 20       # (6 in-place micro-batches; the very first may teach)
    for step in range(2):
        assert abs(res[1][step][0] - res[4][step][0]) < 1e-6 * abs(res[4][step][0])
        for k, a in res[4][step][1].items():
            b = res[1][step][1][k]
            assert float((a - b).norm()) <= 2e-5 * float(a.norm()) + 1e-9, (step, k, float((a - b).norm()), float(a.norm()))


def test_large_two_train_steps_against_the_reference(golden_dir):
    """The metric's unit of work pinned to the reference at the headline configuration: TWO optimizer steps of TransVAE-Large
    f16d32 (one 256 x 256 image per step) through transvae.parallel.train_step + transvae.optim.FusedAdamW -- the patched
    model's clamps, L1 + 1e-8 KL with the logvar clamp, clip-norm 1.0, AdamW lr 1e-4 betas (0.9, 0.95) wd 0, no warm-up --
    against what the REFERENCE model + torch.optim.AdamW did on the CPU in fp32 from the same weights, images and noise
    (tests/golden/large_two_steps.npz, `oracle/make_goldens.py --large-steps`, R/train.py:577-620,681-687): per step the
    loss, the gradient norm before the clip, 256 sampled values of 14 named (clipped) gradients and the parameter deltas at
    the same indices.  Yardstick: the reference's own bf16-autocast run of the same two steps
    (large_two_steps_ref_bf16_autocast.json).

    Step 0 is asserted directly against the reference.  Adam's first update is -lr * sign(g), so a parameter delta differs
    by 2 lr wherever bf16 noise flips the sign of a near-zero gradient element (the reference's own bf16 run: 0.01-37 % rel-L2
    per tensor over 256 samples, 15 % over all): deltas are bounded loosely per tensor and tightly in aggregate.
    Step 1 starts from parameters that differ from the reference's by those flips, after an update that moved EVERY parameter
    by lr (the reference's own loss RISES 0.595 -> 0.631), and the path is chaotic there (tools/probes/bwd_repeat_probe.py:
    moving 5 % of the micro model's parameters by ONE fp32 ulp moves its gradients by 2 %): the deviation from the
    reference's step 1 is split exactly -- (a) the HIP path against the fp32 ORACLE evaluated AT THE HIP PATH'S OWN
    PARAMETERS after step 0 (same image, same noise): the bf16 tier, asserted; (b) what is left is the trajectory's
    sensitivity to step 0's sign flips: reported, and bounded loosely against the reference's step 1."""
    from transvae import TransVAE
    from transvae.optim import FusedAdamW
    from transvae.parallel import train_step, vae_bench_loss
    g = dict(np.load(os.path.join(golden_dir, "large_two_steps.npz")))
    with open(os.path.join(golden_dir, "large_two_steps_ref_bf16_autocast.json")) as f:
        ref16 = json.load(f)
    keys = [k[4:] for k in g if k.startswith("idx:")]
    assert len(keys) == 14
    cfg = O.variant_config("large", 16, 32)
    m = TransVAE(variant="large", compression_ratio=16, latent_dim=32, clamp_latent=True)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(cfg, 32), gains=filler.LARGE_GAINS))
    m = m.to(DEV)
    m.train()
    params = dict(m.named_parameters())
    idx = {k: torch.from_numpy(g["idx:" + k]).to(DEV) for k in keys}
    opt = FusedAdamW(m.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.0)
    counters = {}
    report, scal = [], []
    agg = {0: [0.0, 0.0], 1: [0.0, 0.0]}
    raw_grads, sd_after0 = {}, None
    for step in range(2):
        x = filler.rand_input(f"largesteps.x{step}", (1, 3, 256, 256)).to(DEV)
        eps = filler.randn_input(f"largesteps.eps{step}", (1, 32, 16, 16)).to(DEV)
        before = {k: params[k].detach().flatten()[idx[k]].clone() for k in keys}
        if step == 1:
            sd_after0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

        def forward_loss(model, xb):
            recon, mu, logvar = model(xb, eps=eps)
            return vae_bench_loss(recon, xb, mu, logvar)
        loss = float(train_step(m, opt, x, 1, forward_loss, 1.0, 1, counters))
        norm = float(counters["grad_norm"])
        assert float(counters["skipped"]) == 0
        ref_loss, ref_norm = float(g[f"loss{step}"]), float(g[f"gnorm{step}"])
        print(f"step {step}: loss {loss:.6f} (reference {ref_loss:.6f}, its bf16 run {ref16['loss_bf16'][step]:.6f})  "
              f"grad-norm {norm:.4f} (reference {ref_norm:.4f}, its bf16 run {ref16['gnorm_bf16'][step]:.4f})")
        scal.append((step, loss, ref_loss, norm, ref_norm))
        coef = min(1.0, 1.0 / (norm + 1e-6))        # FusedAdamW clips inside the update: .grad holds the un-clipped gradient
        for k in keys:
            raw = params[k].grad.detach().flatten()[idx[k]].double().cpu().numpy()
            raw_grads[(step, k)] = raw
            gv = raw * coef
            rg = g[f"s{step}.g:{k}"].astype(np.float64)
            eg = float(np.linalg.norm(gv - rg) / np.linalg.norm(rg))
            dv = (params[k].detach().flatten()[idx[k]] - before[k]).double().cpu().numpy()
            rd = g[f"s{step}.d:{k}"].astype(np.float64)
            ed = float(np.linalg.norm(dv - rd) / np.linalg.norm(rd))
            agg[step][0] += float(np.linalg.norm(dv - rd) ** 2)
            agg[step][1] += float(np.linalg.norm(rd) ** 2)
            report.append((step, k, eg, ref16[f"s{step}.g:{k}"], ed, ref16[f"s{step}.d:{k}"], float(np.abs(dv).max())))
    for row in report:
        print("   step %d %-46s grad %.4f (ref bf16 %.4f)   delta %.4f (ref bf16 %.4f)  max |delta| %.3e" % row)
    aggs = []
    for step in range(2):
        ours = (agg[step][0] / agg[step][1]) ** 0.5
        theirs = (sum(ref16[f"s{step}.d:{k}"] ** 2 for k in keys) / len(keys)) ** 0.5
        aggs.append((ours, theirs))
        print(f"step {step}: parameter deltas over all {len(keys) * 256} samples: rel-L2 {ours:.4f}; the reference's own bf16 run {theirs:.4f}")
    del m, opt, params
    torch.cuda.empty_cache()
    # ---- step 0: directly against the reference, at its own bf16 deviation
    step, loss, ref_loss, norm, ref_norm = scal[0]
    assert abs(loss - ref_loss) < max(3e-3, 3 * ref16["loss0"]) * ref_loss, (loss, ref_loss)
    assert abs(norm - ref_norm) < max(2e-2, 2 * ref16["gnorm0"]) * ref_norm, (norm, ref_norm)
    for step, k, eg, rg16, ed, rd16, dmax in report:
        assert dmax <= 1.002e-4, (step, k, dmax)      # an AdamW step never exceeds lr per element (+ fp32 rounding of the difference)
        if step == 0:
            assert eg < max(3e-2, 1.5 * rg16), (k, eg, rg16)       # 256 samples estimate a tensor's rel-L2 to about +-10 %
            assert ed < max(0.30, 2.0 * rd16), (k, ed, rd16)
    assert aggs[0][0] < max(0.12, 1.5 * aggs[0][1]), aggs[0]
    # ---- step 1 (a): the fp32 oracle at the HIP path's own parameters after step 0
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd = {k: v.requires_grad_(not k.endswith("inv_freq")) for k, v in sd_after0.items()}
    x1 = filler.rand_input("largesteps.x1", (1, 3, 256, 256))
    eps1 = filler.randn_input("largesteps.eps1", (1, 32, 16, 16))
    r_ref, mu_ref, lv_ref = O.forward(x1, sd, cfg, eps1, clamp=True)
    o_loss = O.bench_loss(r_ref, x1, mu_ref, lv_ref, clamp_logvar=True)
    o_loss.backward()
    o_norm = float(torch.sqrt(sum(v.grad.double().pow(2).sum() for v in sd.values() if v.grad is not None)))
    _, loss1, ref_loss1, norm1, ref_norm1 = scal[1]
    print(f"step 1, same parameters: loss {loss1:.6f} vs the oracle's {float(o_loss):.6f}; grad-norm {norm1:.4f} vs {o_norm:.4f} "
          f"(the reference's own trajectory: {ref_loss1:.6f}, {ref_norm1:.4f})")
    assert abs(loss1 - float(o_loss)) < 3e-3 * float(o_loss), (loss1, float(o_loss))
    assert abs(norm1 - o_norm) < 2e-2 * o_norm, (norm1, o_norm)
    for k in keys:
        og = sd[k].grad.flatten()[torch.from_numpy(g["idx:" + k])].double().numpy()
        e = float(np.linalg.norm(raw_grads[(1, k)] - og) / np.linalg.norm(og))
        print("   step 1 %-46s gradient vs the oracle at the same parameters %.4f (reference's bf16 tier on this tensor %.4f)" % (k, e, ref16[f"s0.g:{k}"]))
        assert e < max(3e-2, 1.5 * ref16[f"s0.g:{k}"]), (k, e, ref16[f"s0.g:{k}"])
    # ---- step 1 (b): the trajectory against the reference's (its own bf16 run: loss 1.3e-3, norm 0.9 %, gradients 2-6 %)
    assert abs(loss1 - ref_loss1) < 1e-2 * ref_loss1, (loss1, ref_loss1)
    assert abs(norm1 - ref_norm1) < 0.12 * ref_norm1, (norm1, ref_norm1)
    for step, k, eg, rg16, ed, rd16, dmax in report:
        if step == 1:
            assert eg < 0.35 and ed < max(0.35, 2.0 * rd16), (k, eg, ed)
    assert aggs[1][0] < max(0.2, 2.0 * aggs[1][1]), aggs[1]


@pytest.mark.parametrize("kind", optimizer_kinds())
def test_non_finite_step_is_skipped_on_the_device(kind):
    """R/train_2.py:328-338.  Without the P/ clamps a logvar of +1000 overflows exp(): loss and gradients are not finite;
    the step must leave parameters and optimizer state untouched and count one skip -- and the same weights WITH the
    clamps (the bench's configuration) step normally."""
    from transvae.parallel import train_step, vae_bench_loss
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 64, 64, generator=g).to(DEV)
    eps = torch.randn(2, 4, 4, 4, generator=g).to(DEV)

    def forward_loss(model, xb):
        recon, mu, logvar = model(xb, eps=eps)
        return vae_bench_loss(recon, xb, mu, logvar)
    for clamp in (False, True):
        m = micro_model(clamp_latent=clamp)
        m.train()
        opt = make_optimizer(m.parameters(), kind, 1e-3)
        counters = {}
        train_step(m, opt, x, 2, forward_loss, 1.0, 2, counters)          # a normal step first (creates the Adam state)
        assert float(counters["skipped"]) == 0
        with torch.no_grad():
            m.conv_logvar.bias.add_(1000.0)
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        loss = train_step(m, opt, x, 2, forward_loss, 1.0, 2, counters)
        if clamp:
            assert torch.isfinite(loss) and float(counters["skipped"]) == 0
            assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())
        else:
            assert not torch.isfinite(loss)
            assert float(counters["skipped"]) == 1
            for k, v in m.state_dict().items():
                assert torch.equal(v, before[k]), k
            with torch.no_grad():
                m.conv_logvar.bias.sub_(1000.0)
            loss = train_step(m, opt, x, 2, forward_loss, 1.0, 2, counters)   # and training resumes
            assert torch.isfinite(loss) and float(counters["skipped"]) == 1
            assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_forward_backward_under_autocast_equals_plain_call():
    """The reference trainers wrap model(images) in torch.cuda.amp.autocast (R/train.py:589-593, R/train_2.py:303-312).
    The path has its own precision policy, so the result must be bit-identical with and without autocast (the parameter
    folds W @ b / W * g would otherwise turn bf16 and the fp32-bias check would fire)."""
    x = filler.rand_input("micro.x", (2, 3, 64, 64)).to(DEV)
    eps = filler.randn_input("micro.eps", (2, 4, 4, 4)).to(DEV)
    outs = []
    for amp in (False, True):
        m = micro_model()
        m.train()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            recon, mu, logvar = m(x, eps=eps)
            mu2, _ = m.encode(x)
            dec = m.decode(eps)
        assert recon.dtype == torch.float32 and mu.dtype == torch.float32
        (recon.float() - x).abs().mean().backward()
        outs.append((recon.detach(), mu.detach(), mu2.detach(), dec.detach(),
                     {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for k in a[4]:
        ga, gb = a[4][k].double(), b[4][k].double()
        # weight gradients are summed with fp32 atomics (order noise; biases that feed a GroupNorm have an exactly-zero
        # gradient in exact arithmetic, so what they hold IS that noise)
        assert float((ga - gb).norm()) <= 1e-4 * float(ga.norm()) + 1e-8, k


def test_wrong_dtype_operands_raise_runtime_error():
    from transvae.hip import ops
    x = torch.randn(64, 64, device=DEV).to(torch.bfloat16)
    w = torch.randn(64, 64, device=DEV)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.linear(x, w, torch.zeros(64, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="fp32 master"):
        ops.linear(x, w.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="bf16"):
        ops.linear(x.float(), w)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_model_on_a_non_current_device():
    """model.to('cuda:1') without torch.cuda.set_device(1): the entry points switch device themselves."""
    from transvae import TransVAE
    m = TransVAE(config=dict(O.MICRO), variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(O.MICRO, latent_dim=4)))
    x = filler.rand_input("micro.x", (2, 3, 64, 64))
    eps = filler.randn_input("micro.eps", (2, 4, 4, 4))
    assert torch.cuda.current_device() == 0
    r0 = m.to("cuda:0")(x.to("cuda:0"), eps=eps.to("cuda:0"))[0].cpu()
    r1 = m.to("cuda:1")(x.to("cuda:1"), eps=eps.to("cuda:1"))[0].cpu()
    assert torch.equal(r0, r1)


# ---- N > 1 with the real model ------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, q, grad_exchange="fp32"):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "deepl-project_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from transvae.parallel import shard_range, train_step, vae_bench_loss, wrap_ddp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = micro_model(clamp_latent=True)
    m.train()
    ddp = wrap_ddp(m, torch.device(DEV), grad_exchange=grad_exchange)
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.0, fused=True)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    eps = torch.randn(4, 4, 4, 4, generator=g).to(DEV)
    s, c = shard_range(4, world, rank)
    cursor = [s]

    def forward_loss(model, xb):
        e = eps[cursor[0]:cursor[0] + xb.shape[0]]
        cursor[0] += xb.shape[0]
        recon, mu, logvar = model(xb, eps=e)
        return vae_bench_loss(recon, xb, mu, logvar)
    counters = {}
    loss = train_step(ddp, opt, x[s:s + c], 1, forward_loss, None, 4, counters)     # 2 micro-batches: no_sync + sync
    t = loss.detach().clone()      # each rank's value is weighted by world_size (DDP averages): the mean over ranks is the loss
    dist.all_reduce(t)
    t /= world
    grads = {k: p.grad.detach().float().cpu().numpy().copy() for k, p in m.named_parameters()}
    if rank == 0:
        q.put((float(t), float(counters["grad_norm"]), grads))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_ddp_gradients_equal_the_single_process_step():
    """World size 2 over gloo, both ranks on cuda:0, the real HIP micro model under DDP (bucket views, no_sync on the first
    micro-batch): the averaged gradients equal those of one process running the whole batch (fp32 summation order only)."""
    from transvae.parallel import train_step, vae_bench_loss
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    loss2, norm2, grads2 = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    # single process, same batch in one micro-batch
    m = micro_model(clamp_latent=True)
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.0, fused=True)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    eps = torch.randn(4, 4, 4, 4, generator=g).to(DEV)

    def forward_loss(model, xb):
        recon, mu, logvar = model(xb, eps=eps)
        return vae_bench_loss(recon, xb, mu, logvar)
    counters = {}
    loss1 = train_step(m, opt, x, 4, forward_loss, None, 4, counters)
    assert abs(float(loss1) - loss2) < 1e-5 * abs(float(loss1))
    assert abs(float(counters["grad_norm"]) - norm2) < 1e-4 * norm2
    # Biases directly in front of a GroupNorm with ONE channel per group (the micro model's 32-channel ResBlocks: conv1.bias,
    # the last convolution of a Down/Upsample ...) have an exact gradient of ZERO; what both runs hold there is the same bf16
    # residue (norm ~1e-6, three to four orders below the other bias gradients) plus fp32 summation-order noise of the split
    # sums, so a RELATIVE deviation says nothing: they are held to 1e-4 of the median bias-gradient norm instead.
    import statistics
    bias_scale = statistics.median(float(p.grad.norm()) for k, p in m.named_parameters() if k.endswith(".bias"))
    errs = []
    for k, p in m.named_parameters():
        a, b = p.grad.detach().double().cpu(), torch.from_numpy(grads2[k]).double()
        n = float(a.norm())
        if n > 1e-12:
            errs.append((float((a - b).norm()) / max(n, 1e-2 * bias_scale if k.endswith(".bias") else 0.0), k, n))
    errs.sort(reverse=True)
    print("median bias-gradient norm", bias_scale, " largest deviations (rel-L2, key, norm):", errs[:6])
    assert errs[0][0] < 1e-4, errs[:6]


def test_two_rank_bf16_gradient_exchange_against_the_fp32_exchange():
    """wrap_ddp(grad_exchange="bf16") with the real HIP micro model (two ranks over gloo on cuda:0): the averaged gradients
    equal those of the fp32 exchange to one bf16 rounding of each rank's bucket (rel-L2 <= 2^-8 per parameter tensor; the
    structurally cancelled bias gradients are held to the median bias-gradient norm as in the test above), loss identical."""
    import statistics
    ctx = mp.get_context("spawn")
    res = {}
    for mode in ("fp32", "bf16"):
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q, mode)) for r in range(2)]
        for p in procs:
            p.start()
        res[mode] = q.get(timeout=600)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    (l32, n32, g32), (l16, n16, g16) = res["fp32"], res["bf16"]
    assert abs(l32 - l16) < 1e-6 * abs(l32)
    assert abs(n32 - n16) < 2.0 ** -8 * n32
    bias_scale = statistics.median(float(np.linalg.norm(v)) for k, v in g32.items() if k.endswith(".bias"))
    worst, moved = 0.0, 0
    for k in g32:
        a, b = g32[k].astype(np.float64), g16[k].astype(np.float64)
        n = float(np.linalg.norm(a))
        if n > 1e-12:
            worst = max(worst, float(np.linalg.norm(a - b)) / max(n, 1e-2 * bias_scale if k.endswith(".bias") else 0.0))
            moved += int(not np.array_equal(a, b))
    print("bf16 exchange: largest rel-L2 deviation of a gradient tensor from the fp32 exchange", worst)
    assert worst < 2.0 ** -8 and moved > 0


def _rccl_rank_main(port, q, grad_exchange):
    """Child process: RCCL first, before any other GPU call of this process."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "deepl-project_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    try:
        dev = torch.device(DEV)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        backend = dist.get_backend()
        loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "librccl" in ln or "libnccl" in ln]
        from transvae.optim import FusedAdamW
        from transvae.parallel import train_step, vae_bench_loss, wrap_ddp
        g = torch.Generator().manual_seed(5)
        x = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
        eps = torch.randn(4, 4, 4, 4, generator=g).to(DEV)

        def run(wrapped):
            m = micro_model(clamp_latent=True)
            m.train()
            mod = wrap_ddp(m, dev, bucket_mb=1, grad_exchange=grad_exchange, force=True) if wrapped else m
            assert isinstance(mod, torch.nn.parallel.DistributedDataParallel) == wrapped
            opt = FusedAdamW(m.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.0)
            cursor = [0]

            def forward_loss(model, xb):
                e = eps[cursor[0]:cursor[0] + xb.shape[0]]
                cursor[0] += xb.shape[0]
                recon, mu, logvar = model(xb, eps=e)
                return vae_bench_loss(recon, xb, mu, logvar)
            counters = {}
            losses, norms, grads, pars = [], [], [], []
            for _ in range(2):          # DDP re-buckets after its first backward pass: two steps cover both bucket layouts
                cursor[0] = 0
                # 4 micro-batches: autograd / in place under no_sync (x2: the Conv-FFN composite gradients are deferred) / sync
                losses.append(float(train_step(mod, opt, x, 1, forward_loss, 1.0, 4, counters)))
                torch.cuda.synchronize()
                norms.append(float(counters["grad_norm"]))
                grads.append({k: p.grad.detach().float().cpu().numpy().copy() for k, p in m.named_parameters()})
                pars.append({k: p.detach().float().cpu().numpy().copy() for k, p in m.named_parameters()})
            return losses, norms, grads, pars
        res_ddp = run(True)
        t = torch.ones(1024, device=DEV)
        dist.all_reduce(t)             # one explicit collective on RCCL's stream beside DDP's
        torch.cuda.synchronize()
        assert float(t.sum()) == 1024.0
        res_plain = run(False)
        dist.barrier()
        dist.destroy_process_group()
        q.put(("ok", backend, loaded, res_ddp, res_plain))
    except Exception as e:      # noqa: BLE001 -- hand the failure to the parent instead of a bare exit code
        import traceback
        q.put(("error", repr(e), traceback.format_exc()))


@pytest.mark.parametrize("grad_exchange", ["fp32", "bf16"])
def test_rccl_world_size_one_ddp_step_equals_the_unwrapped_step(grad_exchange):
    """RCCL itself (backend "nccl" on ROCm, R/train.py:90,672-674) on the one GPU of the box: a FRESH child process
    initialises the process group on cuda:0 before any other GPU call, wraps the real HIP micro model with
    wrap_ddp(force=True) -- DDP's bucket views over channels_last parameters, its all-reduce (and the bf16 compress hook)
    on RCCL's stream, no_sync on the first micro-batch -- runs two train steps with FusedAdamW and must land where the
    un-wrapped model lands.  With one rank the all-reduce is the identity, so fp32 gradients agree to summation order and
    the bf16 exchange to one bf16 rounding of the bucket."""
    import statistics
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_rank_main, args=(_free_port(), q, grad_exchange))
    p.start()
    res = q.get(timeout=900)
    p.join(timeout=120)
    assert res[0] == "ok", res[1:]
    assert p.exitcode == 0
    _, backend, loaded, (l_d, n_d, g_d, p_d), (l_p, n_p, g_p, p_p) = res
    assert backend == "nccl"
    print("RCCL library mapped in the child:", sorted(set(loaded)))
    assert any("rccl" in s or "nccl" in s for s in loaded) or True      # (torch may link RCCL statically: the backend name is the test)
    tol = 2.0 ** -8 if grad_exchange == "bf16" else 1e-4
    # step 0: one forward / backward from identical parameters -- the DDP path against the un-wrapped one
    assert abs(l_d[0] - l_p[0]) < 1e-6 * abs(l_p[0]), (l_d, l_p)
    assert abs(n_d[0] - n_p[0]) < 2 * tol * n_p[0], (n_d, n_p)
    bias_scale = statistics.median(float(np.linalg.norm(v)) for k, v in g_p[0].items() if k.endswith(".bias"))
    errs = []
    for k in g_p[0]:
        a, b = g_d[0][k].astype(np.float64), g_p[0][k].astype(np.float64)
        n = float(np.linalg.norm(b))
        if n > 1e-12:
            errs.append((float(np.linalg.norm(a - b)) / max(n, 1e-2 * bias_scale if k.endswith(".bias") else 0.0), k, n))
    errs.sort(reverse=True)
    print(f"{grad_exchange} exchange over RCCL, one rank: losses {l_d} vs {l_p}, norms {n_d} vs {n_p}; median bias-gradient norm {bias_scale:.3e}; "
          f"step 0: largest rel-L2 gradient deviations from the un-wrapped step (rel, key, norm): {errs[:6]}")
    assert errs[0][0] < tol, errs[:6]
    for k in p_p[0]:     # one Adam step of lr = 1e-4: the bf16 exchange keeps every sign, so the parameters agree to rounding
        d = np.abs(p_d[0][k].astype(np.float64) - p_p[0][k].astype(np.float64))
        assert float(d.max()) <= 2.1e-4 and float(d.mean()) < 1e-7, (k, float(d.max()), float(d.mean()))
    # step 1 (DDP has re-bucketed by the observed gradient order): the micro model is chaotic after an Adam step -- two
    # un-wrapped runs in one process differ by up to 1.5 % in their step-1 gradients from 1-ulp parameter differences
    # (tools/probes/step_repro_probe.py) -- so the second step is held to that band
    assert abs(l_d[1] - l_p[1]) < 1e-4 * abs(l_p[1]), (l_d, l_p)
    assert abs(n_d[1] - n_p[1]) < 1e-2 * n_p[1], (n_d, n_p)
    num = sum(float(np.linalg.norm(g_d[1][k].astype(np.float64) - g_p[1][k].astype(np.float64)) ** 2) for k in g_p[1]) ** 0.5
    den = sum(float(np.linalg.norm(g_p[1][k].astype(np.float64)) ** 2) for k in g_p[1]) ** 0.5
    print(f"   step 1: rel-L2 of all gradients against the un-wrapped run {num / den:.3e}")
    assert num / den < 5e-2


def test_bucket_timeline_records_every_bucket_once():
    """transvae.parallel.BucketTimeline (tools/ddp_bucket_timeline.py): world size 1, the real HIP micro model under DDP with
    small buckets: every parameter appears in exactly one bucket, ready times are monotone and inside the backward pass,
    and the gradients are the un-wrapped model's (the hook hands the bucket back unchanged)."""
    from transvae.parallel import BucketTimeline, vae_bench_loss, wrap_ddp
    if not dist.is_initialized():
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        m = micro_model(clamp_latent=True)
        m.train()
        g = torch.Generator().manual_seed(5)
        x = torch.rand(2, 3, 64, 64, generator=g).to(DEV)
        eps = torch.randn(2, 4, 4, 4, generator=g).to(DEV)
        recon, mu, logvar = m(x, eps=eps)
        vae_bench_loss(recon, x, mu, logvar).backward()
        ref = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        m.zero_grad(set_to_none=True)
        ddp = wrap_ddp(m, torch.device(DEV), bucket_mb=1, force=True)
        tl = BucketTimeline(ddp)
        for it in range(2):        # (DDP re-buckets by the observed gradient order after its first backward pass: report the second)
            ddp.zero_grad(set_to_none=True)
            recon, mu, logvar = ddp(x, eps=eps)
            loss = vae_bench_loss(recon, x, mu, logvar)
            tl.start()
            loss.backward()
            rep = tl.report()
        names = [n for r in tl.records for n in r[2]]
        assert sorted(names) == sorted(k for k, _ in m.named_parameters()) and len(rep["buckets"]) >= 3
        t = [b["ready_ms"] for b in rep["buckets"]]
        assert all(t[i] <= t[i + 1] + 1e-3 for i in range(len(t) - 1)) and 0 <= t[0] and t[-1] <= rep["backward_ms"] + 1e-3
        assert abs(rep["buckets"][-1]["cum_bytes_frac"] - 1.0) < 1e-6
        for k, p in m.named_parameters():
            assert torch.allclose(p.grad, ref[k], rtol=1e-4, atol=1e-9), k
    finally:
        dist.destroy_process_group()


# ---- transvae.optim.FusedAdamW against torch.optim.AdamW ------------------------------------------------
def test_fused_adamw_matches_torch_adamw_and_clip():
    """Five steps on tensors of awkward sizes (a 70 001-element vector spanning two chunks, channels_last 4-D weights, a
    gradient that is a 4-byte-aligned view into a flat bucket like DDP's), weight decay on, clip active: parameters and
    moments equal torch.optim.AdamW + clip_grad_norm_ to fp32 rounding; the returned norm equals torch's."""
    from transvae.optim import FusedAdamW
    g = torch.Generator().manual_seed(0)
    shapes = [(70001,), (33,), (64, 32, 3, 3), (96, 64), (7, 5, 1, 1)]

    def make():
        ps = []
        for s in shapes:
            t = torch.randn(s, generator=torch.Generator().manual_seed(len(s) * 100 + s[0])).to(DEV)
            if len(s) == 4:
                t = t.contiguous(memory_format=torch.channels_last)
            ps.append(torch.nn.Parameter(t))
        return ps
    pa, pb = make(), make()
    oa = FusedAdamW(pa, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    ob = torch.optim.AdamW(pb, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    for step in range(5):
        bucket = torch.randn(sum(p.numel() for p in pa) + 1, generator=g).to(DEV) * (5.0 if step % 2 == 0 else 0.01)
        off = 1                                      # odd element offset: 4-byte aligned views
        for a, b in zip(pa, pb):
            gv = bucket[off:off + a.numel()]
            off += a.numel()
            a.grad = gv.as_strided(a.shape, a.stride()) if a.dim() == 4 else gv.view(a.shape)
            b.grad = a.grad.clone()
        norm, skipped = oa.fused_clip_step(1.0)
        ref_norm = torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()
        assert float(skipped) == 0 and abs(float(norm) - float(ref_norm)) < 1e-5 * float(ref_norm)
        for a, b in zip(pa, pb):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (step, tuple(a.shape), float((a - b).abs().max()))
            assert torch.allclose(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"], rtol=1e-5, atol=1e-9)
            assert torch.allclose(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"], rtol=1e-5, atol=1e-12)
    # state_dict interchange (the reference checkpoint's optimizer_state_dict, R/train.py:753-769)
    sd = oa.state_dict()
    assert float(sd["state"][0]["step"]) == 5 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ob2 = torch.optim.AdamW(pb, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    ob2.load_state_dict(sd)
    oa2 = FusedAdamW(pa, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    oa2.load_state_dict(ob.state_dict())
    for a, b in zip(pa, pb):
        a.grad = torch.ones_like(a)
        b.grad = torch.ones_like(b)
    oa2.fused_clip_step(None)
    ob2.step()
    for a, b in zip(pa, pb):
        assert torch.allclose(a, b, rtol=2e-6, atol=1e-7)


def test_fused_adamw_keeps_the_bf16_operands_current():
    """After a step the operands served by ops.pack_weight (forward = the optimizer's bf16 copy, transposed = refreshed by
    tv_pack_weight_multi) equal a fresh tv_pack_weight of the updated fp32 weight, without any per-call pack kernel; an
    outside in-place update invalidates them."""
    from transvae.hip import ops
    from transvae.optim import FusedAdamW
    w = torch.nn.Parameter(torch.randn(96, 64, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last))
    lin = torch.nn.Parameter(torch.randn(130, 72, device=DEV))
    opt = FusedAdamW([w, lin], lr=1e-2, betas=(0.9, 0.95), weight_decay=0.0)

    def views():
        return w.permute(0, 2, 3, 1).view(96, 9, 64), lin.view(130, 1, 72)

    def fresh(v, flip):
        d = torch.empty(v.shape, dtype=torch.bfloat16, device=DEV)
        dt = torch.empty((v.shape[2], v.shape[1], v.shape[0]), dtype=torch.bfloat16, device=DEV)
        from transvae.hip import _lib as L
        L.check(L.load().tv_pack_weight(ops._p(v.contiguous()), ops._p(d), ops._p(dt), v.shape[0], v.shape[1], v.shape[2], int(flip),
                                        ops._stream()), "tv_pack_weight")
        return d, dt
    for it in range(3):
        vw, vl = views()
        d1, t1 = ops.pack_weight(vw, True, True, True)
        d2, t2 = ops.pack_weight(vl, True, True, False)
        for (d, t), (v, flip) in (((d1, t1), (vw, True)), ((d2, t2), (vl, False))):
            rd, rt = fresh(v.detach(), flip)
            assert torch.equal(d, rd) and torch.equal(t, rt), it
        assert d1.data_ptr() == opt._shadow[id(w)].data_ptr()          # served from the optimizer's copy
        w.grad = torch.randn_like(w)
        lin.grad = torch.randn_like(lin)
        opt.fused_clip_step(1.0)
    with torch.no_grad():
        w.mul_(2.0)                                                      # someone else touches the weight
    d, t = ops.pack_weight(views()[0], True, True, True)
    rd, rt = fresh(views()[0].detach(), True)
    assert torch.equal(d, rd) and torch.equal(t, rt) and d.data_ptr() != opt._shadow[id(w)].data_ptr()


# ---- the closed-form loss in one HIP pass --------------------------------------------------------------
@pytest.mark.parametrize("variant", ["reference", "patched"])
def test_fused_l1_kl_loss_matches_the_reference_formulas(variant):
    """R/transvae/losses/vae_loss.py:83-84,94-96 (variant 'reference') and P/.../vae_loss.py:80-84,96-102 ('patched': sigmoid
    on the reconstruction, mean-KL, logvar clamp) written out with torch ops on the CPU in float64, against
    transvae.TransVAELoss: values to 1e-6 relative, the three gradients to 1e-5 (fp32 elementwise)."""
    from transvae import TransVAELoss
    g = torch.Generator().manual_seed(3)
    recon = (torch.randn(3, 3, 40, 24, generator=g) * 0.7 + 0.4)
    target = torch.rand(3, 3, 40, 24, generator=g)
    mu = torch.randn(3, 8, 5, 3, generator=g) * 2
    logvar = torch.randn(3, 8, 5, 3, generator=g) * 12          # some values outside [-30, 20]
    patched = variant == "patched"
    r64, m64, l64 = (t.double().requires_grad_(True) for t in (recon, mu, logvar))
    if patched:
        l1 = torch.nn.functional.l1_loss(r64.sigmoid(), target.double())
        lv = l64.clamp(-30.0, 20.0)
        kl = (-0.5 * (1.0 + lv - m64.pow(2) - lv.exp())).mean()
    else:
        l1 = torch.nn.functional.l1_loss(r64, target.double())
        lv = l64.clamp(-30.0, 20.0)       # (train_2.py:316-318 clamps before the call; exp(240) is not a number worth comparing)
        kl = -0.5 * torch.sum(1 + lv - m64.pow(2) - lv.exp()) / (mu.shape[0] * mu.shape[2] * mu.shape[3])
    total = 1.0 * l1 + 1e-3 * kl
    total.backward()
    loss_fn = TransVAELoss(l1_weight=1.0, lpips_weight=0.0, kl_weight=1e-3, sigmoid_recon=patched, kl_mean=patched, logvar_clip=(-30.0, 20.0))
    rd, md, ld = (t.to(DEV).requires_grad_(True) for t in (recon, mu, logvar))
    out = loss_fn(rd, target.to(DEV), md, ld)
    assert set(out) == {"l1", "kl", "total"}
    assert abs(float(out["l1"]) - float(l1)) < 1e-6 * float(l1)
    assert abs(float(out["kl"]) - 1e-3 * float(kl)) < 1e-5 * abs(1e-3 * float(kl))
    assert abs(float(out["total"]) - float(total)) < 1e-5 * abs(float(total))
    out["total"].backward()
    for got, ref in ((rd.grad, r64.grad), (md.grad, m64.grad), (ld.grad, l64.grad)):
        assert float((got.cpu().double() - ref).norm()) < 1e-5 * float(ref.norm()) + 1e-12
    # the reference's defaults (vae_loss.py:31-38: lpips 1.0, vf 0.1, gan 0.05) are kept: what cannot be computed here raises
    with pytest.raises(ValueError, match="LPIPS"):
        TransVAELoss()
    with pytest.raises(ValueError, match="LPIPS"):
        TransVAELoss(lpips_weight=1.0)
    with pytest.raises(ValueError, match="VF"):
        loss_fn(rd, target.to(DEV), md, ld, dinov2=torch.nn.Identity())
    import inspect
    sig = inspect.signature(TransVAELoss.__init__).parameters
    assert (sig["lpips_weight"].default, sig["vf_weight"].default, sig["gan_weight"].default, sig["use_gan"].default) == (1.0, 0.1, 0.05, False)


def test_resume_from_a_reference_written_checkpoint(golden_dir):
    """SURVEY 8f-4 on the GPU: tests/golden/ref_checkpoint_nano.pth (written by the reference model + torch AdamW after ITS
    first step, R/train.py:753-769) is loaded into the HIP model and transvae.optim.FusedAdamW; the next step, on the
    reference's own second batch, must land where the reference landed: loss within the bf16 tier, Adam moments and
    parameters at the sampled positions within the update's own size."""
    import json
    from transvae import TransVAE
    from transvae.checkpoint import load_checkpoint, save_checkpoint
    from transvae.optim import FusedAdamW
    from transvae.parallel import clip_and_step
    cfg = dict(depths=[1, 1, 1], base_dims=[32, 32, 64], mlp_ratio=1.0, head_dim=64)
    m = TransVAE(config=dict(cfg), variant="nano", compression_ratio=4, latent_dim=4).to(DEV)
    opt = FusedAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01)
    path = os.path.join(golden_dir, "ref_checkpoint_nano.pth")
    meta = load_checkpoint(path, m, opt, map_location=DEV)
    assert meta["global_step"] == 1
    raw = torch.load(path, weights_only=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), raw["model_state_dict"][k]), k
    assert float(opt._ctrl[0]) == 1.0
    with open(os.path.join(golden_dir, "ref_checkpoint_nano_expect.json")) as f:
        exp = json.load(f)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    x = filler.rand_input("nano.x1", (2, 3, 32, 32)).to(DEV)
    eps = filler.randn_input("nano.eps1", (2, 4, 8, 8)).to(DEV)
    m.train()
    recon, mu, logvar = m(x, eps=eps)
    loss = O.bench_loss(recon, x, mu, logvar)
    loss.backward()
    clip_and_step(list(m.parameters()), opt, 1.0)
    assert abs(float(loss) - exp["loss_step1"]) < 1e-2 * exp["loss_step1"], (float(loss), exp["loss_step1"])
    params = dict(m.named_parameters())
    num = den = 0.0
    for k, e in exp["params"].items():
        idx = torch.tensor(e["idx"], device=DEV)
        got = params[k].detach().flatten()[idx].double().cpu()
        ref = torch.tensor(e["val"], dtype=torch.float64)
        start = before[k].flatten()[idx].double().cpu()
        num += float((got - ref).norm() ** 2)
        den += float((ref - start).norm() ** 2)
        m_got = opt.state[params[k]]["exp_avg"].flatten()[idx].double().cpu()
        m_ref = torch.tensor(exp["exp_avg"][k]["val"], dtype=torch.float64)
        assert float((m_got - m_ref).norm()) < 0.25 * float(m_ref.norm()) + 1e-9, k      # (16 samples of a bf16-noisy gradient)
    assert (num / den) ** 0.5 < 0.25, (num / den) ** 0.5      # the step taken agrees with the reference's step
    assert float(opt._ctrl[0]) == 2.0
    # written back in the reference's format: step counters are plain scalars again
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "back.pth")
        save_checkpoint(m, opt, epoch=0, global_step=2, path=out, args=meta["args"])
        back = torch.load(out, weights_only=True)
        assert float(back["optimizer_state_dict"]["state"][0]["step"]) == 2.0
        assert set(back["optimizer_state_dict"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.gpu
def test_bench_two_rank_launch_as_the_driver_does_it():
    """The N > 1 contract of bench.py end to end, launched the way the driver launches it
    (python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 ... bench.py --gpus 2 ...):
    rendezvous, one rank per process, DDP over the fused autograd Functions with the HIP optimizer, barrier + max-over-ranks
    timing, ONE JSON line from rank 0.  On a one-GPU box both ranks share cuda:0 over gloo (TV_BENCH_REHEARSE=1: RCCL refuses
    two ranks on one device); everything else is the code path of the 8-GPU run.  Small model, 2 steps."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, TV_BENCH_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--variant", "tiny", "--res", "64", "--global-batch", "8", "--micro-batch", "2", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # rank 0 only, one line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["scaling"] == "strong" and out["unit"] == "images/sec" and out["value"] > 0
    assert out["skipped_steps"] == 0 and math.isfinite(out["final_loss"])
    assert out["config"]["global_batch"] == 8


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs_and_full_adds_the_kernel_figures(tmp_path):
    """A plain bench.py run times its steps and prints the result line without the roofline or the CPU baseline;
    --dump-outputs DIR writes the last timed step's loss, gradient norm and sampled parameters / gradients (float npy,
    finite, the loss equal to the line's final_loss); --full adds the roofline entries.  Tiny model at 64 x 64."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TV_")}
    common = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
              "--variant", "tiny", "--res", "64", "--global-batch", "4", "--micro-batch", "2"]

    def run(*extra):
        r = subprocess.run(common + list(extra), cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])

    dump = str(tmp_path / "out")
    out = run("--dump-outputs", dump)
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and len(out["losses"]) == 4
    assert "roofline" not in out and "cpu_baseline" not in out
    files = sorted(os.listdir(dump))
    assert files == ["grad_norm.npy", "grad_sample.npy", "loss.npy", "param_sample.npy"]
    arrs = {f[:-4]: np.load(os.path.join(dump, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["param_sample"].shape == arrs["grad_sample"].shape and arrs["grad_sample"].size > 0
    assert abs(float(arrs["loss"][0]) - out["final_loss"]) <= 1e-5 * max(1.0, abs(out["final_loss"]))
    assert float(arrs["grad_norm"][0]) > 0 and np.abs(arrs["grad_sample"]).max() > 0

    full = run("--full", "--no-cpu-baseline")
    assert full["roofline"]["achieved"] > 0 and len(full["roofline"]["also"]) == 2
