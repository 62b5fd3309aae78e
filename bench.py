#!/usr/bin/env python3
"""Train-step throughput of the TransVAE path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 3 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one optimizer step over the GLOBAL batch (256 images, 256x256, TransVAE-Large
f16d32): forward + backward of every micro-batch, gradient all-reduce (N>1, last micro-batch
only), clip-norm 1.0, AdamW(lr 1e-4, betas (0.9, 0.95), wd 0) -- R/train.py:557-646,681-687.
Loss = L1 + 1e-8 KL (the closed-form terms of R/transvae/losses/vae_loss.py:83-84,94-96; LPIPS/VF need external
networks and are out of scope).  The global batch is FIXED as N grows ("strong" scaling).
Synthetic data (torch.rand images) and random fan-in-scaled weights of the exact architecture: the
reference init overflows to NaN in forward, and no checkpoint exists.  The numerical policy is
the reference's bf16 trainer's ("with the P/ clamps enabled"): the model clamps mu / logvar
(P/.../transvae.py:186-196,243-245), the loss clamps logvar (R/train_2.py:316-318), the learning rate follows
the linear warm-up of R/train_2.py:266-273 (--lr-warmup-steps, default 1000 like the reference), and a step
with non-finite gradients is skipped on the device (R/train_2.py:328-338).  A run in which ANY step's loss is
non-finite or any step was skipped prints no metric line and exits non-zero.

--resolutions 256 512 alternates the resolution step by step (BASELINE config 4, /root/reference README.md:192-203:
documented, never implemented there); every rank runs the same resolution in a given step.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the --steps steps and prints it; what else the
benchmark measures runs only with --full: `roofline` times the dominant kernel (the 192->192 3x3 implicit-GEMM
convolution of the 256x256 stages, tv_igemm_nt; one launch = 64 images) live with HIP events on the launch
stream, `roofline.also` its weight gradient and the largest linear layer; `traffic` comes from the committed PMC
summaries under profiles/ (labelled: not measured inside the run).  `cpu_baseline` times the fp32 CPU oracle (a
port of the reference path, pinned to it by golden vectors) on a bounded sample: a micro-batch of 2
images through the same train step, one untimed warm-up step + two timed steps, thread and core counts stated.

--dump-outputs DIR writes what the last timed step computed, for output-for-output comparisons of two builds (same
arguments, same seeded inputs): loss.npy and grad_norm.npy (float64, the step's loss and its gradient norm before clipping),
param_sample.npy and grad_sample.npy (float32, the updated parameters and the step's gradients at up to 4096 seeded
positions per parameter tensor, in named_parameters() order).

Micro-batch: 128 images on a 288 GB device (peak 245 GiB; falls back to 64 if the first step runs out of memory),
64 otherwise; `config.micro_batch` says which ran.  Started by torch.distributed.run (also with ONE rank) the step
goes through DistributedDataParallel over RCCL (`config.dist_backend`).  TV_* tuning variables of the library
are refused unless --allow-tuning-env (then listed in `config.tuning_env`).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

TRAIN_GFLOP_PER_IMAGE = {"large": 6187.8, "tiny": 1965.6, "base": 2483.7, "huge": 12883.5, "giant": 22221.6}
PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def init_scaled_(model, seed: int = 0):
    """Fan-in scaled random weights (the rule of oracle/filler.py, drawn on the device)."""
    g = torch.Generator(device=next(model.parameters()).device)
    g.manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 4:
                fan = p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(torch.randn(p.shape, generator=g, device=p.device) * fan ** -0.5)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g, device=p.device) * p.shape[1] ** -0.5)
            elif name.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g, device=p.device) * 0.1)
            else:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g, device=p.device))


def _pmc_traffic(files, family: str, mb: int):
    """HBM bytes per launch of one kernel family from the newest committed PMC summary that holds it (profiles/: separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950 corrections applied by tools/probes/pmc_derive.py), scaled by the
    image count.  NOT measured inside a bench run -- labelled so."""
    for name in files:
        path = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            j = json.load(f).get(family)
        if j and "hbm_bytes_per_launch" in j:
            src = ("profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes in their own runs, gfx950 corrections applied; "
                   "not measured inside this run)" % name)
            return round(j["hbm_bytes_per_launch"] * mb / j["images"]), src
    return None, None


def time_dominant_kernel(mb: int, res: int, dev):
    """HIP-event timing of tv_igemm_nt on the stage-0 ResBlock conv (192->192, 3x3, res x res)."""
    from transvae.hip import ops
    C = 192
    x = torch.randn(mb, res, res, C, device=dev).to(torch.bfloat16)
    w = (torch.randn(C, 9, C, device=dev) * (9 * C) ** -0.5)
    wb, _ = ops.pack_weight(w, True, False, False)
    out = torch.empty_like(x)
    d = ops._desc(batch=mb, h_in=res, w_in=res, c_in=C, ldx=C, h_out=res, w_out=res, c_out=C, ldo=C, kh=3, kw=3, stride=1, pad=1)
    for _ in range(10):      # steady state: the first launches run cold (function attribute, clocks ramping, L2 empty)
        ops.igemm(d, x, wb, None, None, None, out)
    n = 30
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.igemm(d, x, wb, None, None, None, out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    flop = 2.0 * mb * res * res * C * 9 * C
    # HBM bytes per launch: NOT measured in this run (PMC counters need their own rocprofv3 passes) -- read from the committed
    # summary of those passes over exactly this kernel and shape, scaled by the image count
    traffic, traffic_src = _pmc_traffic(("r04_dominant_kernel_pmc_all.json", "r03_dominant_kernel_pmc_all.json"), "conv3x3_halo", mb) if res == 256 else (None, None)
    return {"bound": "mfma", "kernel": "conv3x3_halo_kernel (the instantiation tv_igemm_nt selects) via tv_igemm_nt (conv3x3 192->192 @%dx%d, %d images)" % (res, res, mb),
            "achieved": round(flop / ms / 1e9, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(flop / ms / 1e9 / PEAK_BF16_TFLOPS, 4), "flop_per_launch": flop, "ms_per_launch": round(ms, 4),
            "traffic": traffic, "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": 2 * mb * res * res * C * 2 + 9 * C * C * 2}


def time_linear_kernel(mb: int, dev):
    """HIP-event timing of the largest linear layer of the deepest stage (Conv-FFN proj_in, 1536 -> 6144 on 16 x 16 tokens per
    image) through tv_igemm_nt: igemm_nt_kernel<256,256,...> on its eight-phase ping-pong loop, the second largest GEMM
    kernel family of the step by time (profiles/r04_rocprof_kernel_stats.csv)."""
    from transvae.hip import ops
    from transvae.hip import _lib as L
    M, K, N = mb * 256, 1536, 6144
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    w = torch.randn(N, K, device=dev) * K ** -0.5
    b = torch.randn(N, device=dev) * 0.1
    fn = lambda: ops.conv_forward(x, w, b, None, "linear", L.ACT_NONE, False)[0]
    for _ in range(10):
        fn()
    n = 30
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    flop = 2.0 * M * K * N
    traffic, traffic_src = _pmc_traffic(("r04_p8_gemm_pmc.json",), "igemm_nt", mb)
    return {"bound": "mfma", "kernel": "igemm_nt_kernel (the instantiation tv_igemm_nt selects) via tv_igemm_nt (linear 1536->6144, %d rows = %d images x 256 tokens)" % (M, mb),
            "achieved": round(flop / ms / 1e9, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(flop / ms / 1e9 / PEAK_BF16_TFLOPS, 4), "flop_per_launch": flop, "ms_per_launch": round(ms, 4),
            "traffic": traffic, "traffic_source": traffic_src, "algorithmic_bytes_per_launch": (M * K + M * N + N * K) * 2}


def time_wgrad_kernel(mb: int, res: int, dev):
    """HIP-event timing of the weight gradient (+ bias gradient) of the same stage-0 ResBlock convolution (tv_wgrad_tn ->
    wgrad_kx3_kernel): the largest weight-gradient kernel of the step (profiles/r04_rocprof_kernel_stats.csv)."""
    from transvae.hip import ops
    C = 192
    x = torch.randn(mb, res, res, C, device=dev).to(torch.bfloat16)
    gy = torch.randn(mb, res, res, C, device=dev).to(torch.bfloat16)
    w = torch.zeros(C, 3, 3, C, device=dev)
    geo = ops._Geo("c3s1", x, w)
    dw, db = ops.conv_wgrad_alloc(geo, w, True, x, gy)
    dw.zero_()          # wgrad_acc ADDS: never accumulate into uninitialised memory (NaN / Inf operands would perturb the timing)
    db.zero_()
    d = geo.fwd_desc(0)
    for _ in range(10):
        ops.wgrad_acc(d, x, gy, dw, db)
    n = 30
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.wgrad_acc(d, x, gy, dw, db)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    flop = 2.0 * mb * res * res * C * 9 * C
    traffic, traffic_src = _pmc_traffic(("r04_dominant_kernel_pmc_all.json", "r03_dominant_kernel_pmc_all.json"), "wgrad_kx3", mb) if res == 256 else (None, None)
    return {"bound": "mfma", "kernel": "wgrad_kx3_kernel (the instantiation tv_wgrad_tn_acc selects) via tv_wgrad_tn_acc (weight + bias gradient of conv3x3 192->192 @%dx%d, %d images)" % (res, res, mb),
            "achieved": round(flop / ms / 1e9, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(flop / ms / 1e9 / PEAK_BF16_TFLOPS, 4), "flop_per_launch": flop, "ms_per_launch": round(ms, 4),
            "traffic": traffic, "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": 2 * mb * res * res * C * 2 + 9 * C * C * 4}


DUMP_PER_TENSOR = 4096      # sampled positions per parameter tensor: Large 1.7 M, giant 3.1 M per array (<= 26 MB in all)


def dump_outputs(model, loss: float, grad_norm: float, out_dir: str):
    """The last timed step's results as DIR/<name>.npy: the loss and gradient norm in full, the updated parameters and the
    step's gradients at fixed seeded positions (the same for every run with the same arguments)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(0)
    ps, gs = [], []
    with torch.no_grad():
        for _, p in model.named_parameters():
            n = p.numel()
            idx = (torch.arange(n) if n <= DUMP_PER_TENSOR else
                   torch.randint(n, (DUMP_PER_TENSOR,), generator=g).sort().values).to(p.device)
            ps.append(p.detach().reshape(-1).index_select(0, idx).float())
            gs.append(p.grad.reshape(-1).index_select(0, idx).float() if p.grad is not None
                      else torch.full((idx.numel(),), float("nan"), device=p.device))
    np.save(os.path.join(out_dir, "loss.npy"), np.array([loss], dtype=np.float64))
    np.save(os.path.join(out_dir, "grad_norm.npy"), np.array([grad_norm], dtype=np.float64))
    np.save(os.path.join(out_dir, "param_sample.npy"), torch.cat(ps).cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "grad_sample.npy"), torch.cat(gs).cpu().numpy().astype(np.float32))


def cpu_baseline(variant: str, res: int, threads: int, lr: float, batch: int = 2, timed_steps: int = 2):
    """The oracle (CPU restatement of the reference path) on a bounded sample of the same workload, SURVEY 8d: a micro-batch
    of `batch` images through the SAME step as the GPU leg -- forward with the P/ clamps, L1 + 1e-8 KL with the logvar
    clamp, backward, clip-norm 1.0, AdamW at the warm-up learning rate -- ONE untimed warm-up step (first-touch allocation,
    thread-pool start) and then `timed_steps` timed steps; images/s = batch * timed_steps / time."""
    from oracle import transvae_oracle as O
    torch.set_num_threads(threads)
    cfg = O.variant_config(variant, 16, 32)
    schema = O.state_dict_schema(cfg, 32)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, s in schema.items():
        if k.endswith("inv_freq"):
            sd[k] = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
            continue
        if len(s) == 4:
            t = torch.randn(s, generator=g) * (s[1] * s[2] * s[3]) ** -0.5
        elif len(s) == 2:
            t = torch.randn(s, generator=g) * s[1] ** -0.5
        elif k.endswith(".bias"):
            t = torch.randn(s, generator=g) * 0.1
        else:
            t = 1.0 + 0.1 * torch.randn(s, generator=g)
        sd[k] = t.requires_grad_(True)
    params = [v for v in sd.values() if v.requires_grad]
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.95), weight_decay=0.0)
    x = torch.rand(batch, 3, res, res, generator=g)
    eps = torch.randn(batch, 32, res // 16, res // 16, generator=g)

    def step():
        opt.zero_grad(set_to_none=True)
        recon, mu, logvar = O.forward(x, sd, cfg, eps, clamp=True)
        loss = O.bench_loss(recon, x, mu, logvar, clamp_logvar=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        return float(loss)
    t0 = time.time()
    step()
    warm = time.time() - t0
    times = []
    for _ in range(timed_steps):
        t0 = time.time()
        step()
        times.append(time.time() - t0)
    dt = sum(times)
    return {"value": round(batch * timed_steps / dt, 5), "unit": "images/sec", "cores": threads, "host_cores": os.cpu_count(),
            "kind": "port",
            "sample": f"micro-batch of {batch} images, TransVAE-{variant} f16d32 {res}x{res}, fp32 oracle fwd+bwd+clip+AdamW "
                      f"(same clamps / loss / optimizer as the GPU leg): 1 warm-up step ({warm:.1f} s) + {timed_steps} timed steps "
                      f"({', '.join('%.1f' % t for t in times)} s), {threads} torch threads on a host of {os.cpu_count()} logical cores",
            # the reference's OWN fp32 CPU path cannot travel to the GPU box; timed in the build container
            "reference_cpu_path": {"value": 0.019, "unit": "images/sec", "cores": 8, "where": "build container (8 cores)",
                                   "sample": "TransVAE-large f16d32 256x256, batch 2, fwd+bwd+clip+AdamW, 104.7 s/step"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variant", default="large")
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--resolutions", type=int, nargs="+", default=None,
                    help="alternate these resolutions step by step (BASELINE config 4: --resolutions 256 512 --global-batch 128)")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--lr-warmup-steps", type=int, default=1000, help="linear warm-up of R/train_2.py:266-273 (0 = constant lr)")
    ap.add_argument("--optimizer", choices=["hip", "torch"], default="hip",
                    help="hip: transvae.optim.FusedAdamW (norm + clip + guard + AdamW + operand refresh in 4 launches); "
                         "torch: torch.optim.AdamW(fused=True) behind the same guard")
    ap.add_argument("--no-clamp", action="store_true", help="model without the P/ clamps (for the guard's A/B only)")
    ap.add_argument("--global-batch", type=int, default=256)
    ap.add_argument("--micro-batch", type=int, default=0,
                    help="images per micro-batch (at 256 x 256; other resolutions: the same pixels).  0 = 128 when the device holds "
                         ">= 260 GiB (peak 245 GiB for Large: 159 images/s against 155 at 64 on one box, "
                         "profiles/r04_kernel_experiments.txt item 8), else 64")
    ap.add_argument("--checkpointing", choices=["off", "resblocks", "all"], default="off",
                    help="activation recompute (R/transvae/models/encoder.py:97-99,117-118): resblocks = the fused-op recompute of the "
                         "CNN stages only (2 instead of 4 saved full-resolution tensors per ResBlock), all = every block like the reference")
    ap.add_argument("--grad-exchange", choices=["fp32", "bf16"], default="fp32",
                    help="N > 1: gradient all-reduce in fp32 (4.2 GB per step, the reference's DDP) or with bf16 buckets (2.1 GB)")
    ap.add_argument("--full", action="store_true",
                    help="also time the dominant kernels (roofline) and the fp32 CPU baseline after the timed steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (loss, gradient norm, sampled parameters "
                         "and gradients)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-batch", type=int, default=2, help="images per step of the CPU baseline (SURVEY 8d: 2-4)")
    ap.add_argument("--dist-backend", choices=["auto", "nccl", "gloo", "none"], default="auto",
                    help="auto: nccl (= RCCL) whenever the process was started by torch.distributed.run (RANK / WORLD_SIZE in the "
                         "environment), also with ONE rank -- DDP, its bucket views and the all-reduce then run exactly as at N > 1; "
                         "none with a plain `python bench.py`")
    ap.add_argument("--mem-fraction", type=float, default=0.0,
                    help="cap this process's share of the device memory (torch.cuda.set_per_process_memory_fraction): rehearses the "
                         "fallback of the automatic micro-batch on a smaller device")
    ap.add_argument("--allow-tuning-env", action="store_true",
                    help="run although TV_* tuning variables are set (they are printed into config.tuning_env either way)")
    ap.add_argument("--kernel-only", action="store_true", help="only time the dominant kernel (for rocprofv3 --pmc passes)")
    args = ap.parse_args()
    # read at HSA initialisation: must be in the environment BEFORE the first torch.cuda call of this process (the image exports
    # it already; this is the default for a bare shell).  dmabuf IPC is the only mode the host driver supports.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # process-global tuning hooks of the library (transvae/hip/_lib.py) change the timed path: refuse them unless asked for
    tuning_env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("TV_") and k not in ("TV_BENCH_REHEARSE",)}
    if tuning_env and not args.allow_tuning_env:
        raise SystemExit(f"bench.py: tuning variables are set ({tuning_env}); unset them or pass --allow-tuning-env "
                         "(they are then reported in config.tuning_env)")
    if args.kernel_only:
        torch.cuda.set_device(0)
        kmb = args.micro_batch if args.micro_batch > 0 else 64
        r = time_dominant_kernel(kmb, args.res, torch.device("cuda", 0))
        r["also"] = [time_wgrad_kernel(kmb, args.res, torch.device("cuda", 0)), time_linear_kernel(kmb, torch.device("cuda", 0))]
        print(json.dumps(r), flush=True)
        return

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the TransVAE path has no CPU fallback")
    # rehearsal hook: TV_BENCH_REHEARSE=1 runs all ranks on GPU 0 over gloo (RCCL refuses two ranks per device);
    # it exists to exercise the N>1 code path on a one-GPU box and is never used for reported numbers
    rehearse = os.environ.get("TV_BENCH_REHEARSE") == "1"
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if args.mem_fraction > 0:
        torch.cuda.set_per_process_memory_fraction(args.mem_fraction, dev)
    auto_mb = args.micro_batch <= 0
    if auto_mb:
        total_gib = torch.cuda.mem_get_info(dev)[1] / 2 ** 30
        if args.variant in ("giant", "huge"):       # (giant: 4.6 GiB of activations per image beside 88 GiB of state)
            args.micro_batch = 32
        else:
            args.micro_batch = 128 if total_gib >= 260 else 64
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ and "MASTER_ADDR" in os.environ
    backend = args.dist_backend
    if backend == "auto":
        backend = "gloo" if rehearse else ("nccl" if (world > 1 or launched) else "none")
    if world > 1 and backend == "none":
        raise SystemExit("--dist-backend none with more than one rank")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)      # RCCL on ROCm
    elif backend == "gloo":
        dist.init_process_group("gloo")

    from transvae import TransVAE
    from transvae.hip import _lib
    from transvae.parallel import shard_range, train_step, vae_bench_loss, warmup_lr, wrap_ddp
    _lib.load()  # fails loudly if the HIP library is missing

    torch.manual_seed(0)
    with torch.device(dev):
        model = TransVAE(variant=args.variant, compression_ratio=16, latent_dim=32, clamp_latent=not args.no_clamp)
    init_scaled_(model, seed=0)
    if args.checkpointing != "off":
        model.enable_gradient_checkpointing(args.checkpointing)
    model.train()
    ddp = wrap_ddp(model, dev, grad_exchange=args.grad_exchange, force=backend != "none")
    if args.optimizer == "hip":
        from transvae.optim import FusedAdamW
        opt = FusedAdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0, fused=True)

    start, count = shard_range(args.global_batch, world, rank)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + rank)
    resolutions = args.resolutions or [args.res]
    xs = {r: torch.rand(count, 3, r, r, device=dev, generator=gen) for r in resolutions}
    micro = {r: max(1, args.micro_batch * 256 * 256 // (r * r)) for r in resolutions}   # same pixels per micro-batch

    def forward_loss(m, xb):
        lat = xb.shape[-1] // 16
        eps = torch.randn(xb.shape[0], 32, lat, lat, device=dev, generator=gen)
        recon, mu, logvar = m(xb, eps=eps)
        return vae_bench_loss(recon, xb, mu, logvar)

    def sync():
        torch.cuda.synchronize()
        if backend != "none":
            dist.barrier()
        torch.cuda.synchronize()

    counters = {}
    opt_step = [0]

    def one_step():
        r = resolutions[opt_step[0] % len(resolutions)]
        lr = warmup_lr(args.lr, opt_step[0], args.lr_warmup_steps)     # a python float: no device sync
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt_step[0] += 1
        return train_step(ddp, opt, xs[r], micro[r], forward_loss, 1.0, args.global_batch, counters)

    if rank == 0:
        log(f"{args.variant} f16d32 {'/'.join(map(str, resolutions))}px global batch {args.global_batch} on {world} GPU(s), "
            f"{count} img/rank in micro-batches of {', '.join(str(micro[r]) for r in resolutions)}")
    losses = []
    for i in range(args.warmup):
        retry = False
        try:
            loss = one_step()
        except torch.OutOfMemoryError:
            # the automatic micro-batch (128 on a 288 GB device: peak 245 GiB) did not fit on this box: fall back to 64 once --
            # only with ONE rank (a lone rank's fallback would desynchronise DDP's collectives)
            if not (auto_mb and i == 0 and world == 1 and args.micro_batch > 64):
                raise
            retry = True
        if retry:       # (outside the handler: the traceback kept the failed pass's tensors alive)
            import gc
            log(f"micro-batch {args.micro_batch} ran out of memory: falling back to 64")
            args.micro_batch = 64
            micro = {r: max(1, 64 * 256 * 256 // (r * r)) for r in resolutions}
            opt.zero_grad(set_to_none=True)
            opt_step[0] = 0
            gc.collect()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            loss = one_step()
        losses.append(loss)
        if rank == 0:
            torch.cuda.synchronize()
            log(f"warmup {i}: loss {float(loss):.4f}  grad-norm {float(counters['grad_norm']):.3e}  "
                f"mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        losses.append(one_step())       # device scalars; read after the timed region
        if rank == 0 and args.steps > 1:
            log(f"step {i} queued")
    sync()
    dt = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
    if backend != "none":
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    dt = float(dt)
    # every step's loss (all ranks' shares summed) and the number of skipped steps
    lt = torch.stack([l.float() for l in losses])
    if backend != "none":      # train_step weights a rank's loss by world_size (DDP averages gradients): the mean over ranks is the loss
        lt = lt.to(dev)
        dist.all_reduce(lt)
        lt /= world
    lt = lt.cpu()
    skipped = float(counters.get("skipped", torch.zeros(()))) if counters else 0.0
    final_loss = float(lt[-1])
    bad = (not bool(torch.isfinite(lt).all())) or skipped > 0
    if bad:
        if rank == 0:
            log(f"FAILED: non-finite loss or skipped steps (skipped {skipped:.0f}); per-step losses: "
                + " ".join(f"{float(v):.4g}" for v in lt))
        if backend != "none":
            dist.barrier()
            dist.destroy_process_group()
        sys.exit(3)

    if rank == 0 and args.dump_outputs:
        dump_outputs(model, final_loss, float(counters["grad_norm"]), args.dump_outputs)
    if rank == 0:
        ips = args.global_batch * args.steps / dt
        def gflop(r):
            return TRAIN_GFLOP_PER_IMAGE.get(args.variant) if r == 256 else (31419.3 if (args.variant, r) == ("large", 512) else None)
        per_res = [gflop(resolutions[(args.warmup + i) % len(resolutions)]) for i in range(args.steps)]
        gf = None if any(v is None for v in per_res) else sum(per_res) / len(per_res)
        res_name = "+".join(f"{r}x{r}" for r in resolutions)
        out = {
            # BASELINE.json's metric string for its own configuration; any other variant / resolution / batch says so
            "metric": f"images/sec train step, TransVAE-{args.variant.capitalize()} f16d32 {'+'.join(map(str, resolutions))}px bs{args.global_batch}",
            "value": round(ips, 3), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"TransVAE-{args.variant} f16d32 {res_name} train step "
                                   f"(fwd+bwd+grad all-reduce+clip+AdamW), global batch {args.global_batch}",
                       "global_batch": args.global_batch, "micro_batch": [micro[r] for r in resolutions] if len(resolutions) > 1 else args.micro_batch,
                       "parallelism": f"dp{world}", "gradient_exchange": args.grad_exchange if backend != "none" else None,
                       "dist_backend": {"nccl": "nccl (RCCL), DistributedDataParallel", "gloo": "gloo (one-GPU rehearsal), DistributedDataParallel",
                                        "none": "none (single process, no process group)"}[backend],
                       "tuning_env": tuning_env,
                       "weights": "random fan-in scaled", "loss": "L1 + 1e-8 KL (vae_loss.py:83-84,94-96)",
                       "numerics": "P/ clamps on mu/logvar, skip-on-non-finite guard",
                       "checkpointing": args.checkpointing,
                       "lr": args.lr, "lr_warmup_steps": args.lr_warmup_steps,
                       "optimizer": "transvae.optim.FusedAdamW (HIP multi-tensor)" if args.optimizer == "hip" else "torch.optim.AdamW(fused)"},
            "final_loss": round(final_loss, 5),
            "losses": [round(float(v), 5) for v in lt],
            "skipped_steps": int(skipped),
            "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2**30, 1),
        }
        if gf:
            out["model_tflops_per_gpu"] = round(ips * gf / 1e3 / world, 1)
            out["mfma_roofline_frac"] = round(ips * gf / 1e3 / world / PEAK_BF16_TFLOPS, 4)
            out["flop_accounting"] = ("model_tflops = images/s x the REFERENCE's algorithmic FLOPs per image (SURVEY 8d: 2 MAC, 3x forward); the path "
                                      "executes fewer: exact reformulations (Conv-FFN tail on the composite W_out W3: -283 GF per Large image; "
                                      "polyphase up-convolutions: 4 taps for 9, ~-180 GF) -- DESIGN 4, 4.6")
        if args.full:
            log("timing the dominant kernel")
            kmb = min(args.micro_batch, count, 64)     # ONE launch: 64 images (a 128-image micro-batch's 3.2 GB tensors go out as two launches of 64)
            out["roofline"] = time_dominant_kernel(kmb, 256, dev)
            # the dominant kernel BY TIME is the 3x3 convolution above (profiles/r04_rocprof_kernel_stats.csv: 17 % of the step);
            # the largest weight-gradient kernel (9 %) is reported beside it
            out["roofline"]["also"] = [time_wgrad_kernel(kmb, 256, dev), time_linear_kernel(kmb, dev)]
        if args.full and world == 1 and not args.no_cpu_baseline:
            log("cpu baseline (oracle: 1 warm-up + 2 timed steps) ...")
            del model, ddp, opt
            torch.cuda.empty_cache()
            out["cpu_baseline"] = cpu_baseline(args.variant, resolutions[0], max(1, min(args.cpu_threads, os.cpu_count() or 1)),
                                               warmup_lr(args.lr, 1, args.lr_warmup_steps), batch=args.cpu_batch)
        print(json.dumps(out), flush=True)
    if backend != "none":
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
