"""Cost of the adversarial stage (transvae.PatchDiscriminator, csrc/gan.hip, the frozen-encoder train step).  GPU box.

    python tools/gan_bench.py [--batch 128] [--res 256] [--iters 10] [--step-ms MS] [--skip-model] [--out profiles/gan_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `disc`:   (a) discriminator forward, (b) forward + backward to input and parameters at batch x 3 x res^2, device events around
             warmed-up loops; then every convolution layer on its own (forward, data gradient in both 'c4s2' forms, weight
             gradient) -> TFLOP/s from 2 * 16 * Cin * Cout * output pixels.
2. `model`:  (c) one stage-2 generator step of Large at micro-batch `batch` with the encoder frozen (model forward, L1 + KL + GAN
             term through the discriminator, backward, FusedAdamW over the trainable parameters) and (d) the same step unfrozen.
3. `trace`:  the discriminator forward + backward under `rocprofv3 --kernel-trace --stats`, a run of its own; the row kernels'
             effective TB/s on their algorithmic bytes (header comment of csrc/gan.hip) -> profiles/gan_kernel_stats.csv.
--step-ms: train-step time of `bench.py --steps 20 --warmup 5` on the same box (run separately, untouched), recorded next to it.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))

LAYERS = (("main.2", "c4s2", 64, 128, 2), ("main.5", "c4s2", 128, 256, 4), ("main.8", "c4s1", 256, 512, 8), ("main.11", "c4s1", 512, 32, 8))


def timed(fn, iters, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def make_disc(dev):
    import torch
    from transvae import PatchDiscriminator
    torch.manual_seed(0)
    return PatchDiscriminator().to(dev)


def disc_fwd_bwd(D, x):
    from transvae.losses import generator_gan_loss
    x.grad = None
    for p in D.parameters():
        p.grad = None
    generator_gan_loss(D(x), 1.0).backward()


def algorithmic_bytes(B, H, W, ndf=64):
    """{kernel: bytes per discriminator forward + backward} (csrc/gan.hip header); BatchNorm layers at H/4, H/8, H/8 - 1."""
    P = B * H * W
    bn = [(B * (H // 4) * (W // 4), 2 * ndf), (B * (H // 8) * (W // 8), 4 * ndf), (B * (H // 8 - 1) * (W // 8 - 1), 8 * ndf)]
    mc = sum(m * c for m, c in bn)
    return {"patch4x4s2_kernel": 44 * P, "patch4x4s2_bwd_kernel": 44 * P, "bn_reduce_kernel<0>": 2 * mc, "bn_reduce_kernel<1>": 4 * mc,
            "bn_lrelu_apply_kernel": 4 * mc, "bn_lrelu_bwd_apply_kernel": 6 * mc}


def child_disc(a):
    import torch
    from transvae.hip import ops
    dev = torch.device("cuda:0")
    D = make_disc(dev)
    torch.manual_seed(0)
    x = torch.rand(a.batch, 3, a.res, a.res, device=dev).requires_grad_(True)
    with torch.no_grad():
        ms_f = [timed(lambda: D(x), a.iters) for _ in range(3)]
    ms_fb = [timed(lambda: disc_fwd_bwd(D, x), a.iters) for _ in range(3)]
    print(json.dumps({"what": "discriminator", "batch": a.batch, "res": a.res, "fwd_ms": [round(m, 3) for m in ms_f],
                      "fwd_bwd_ms": [round(m, 3) for m in ms_fb]}), flush=True)
    for name, mode, c_in, c_out, down in LAYERS:
        h_in = a.res // down - (1 if name == "main.11" else 0)
        xin = torch.randn(a.batch, h_in, h_in, c_in, device=dev).to(torch.bfloat16)
        w = torch.randn(c_out, 4, 4, c_in, device=dev) * 0.02
        out, _, geo, wc = ops.conv_forward(xin, w, None, None, mode, 0, False)
        gz = torch.randn_like(out)
        flop = 2.0 * 16 * c_in * c_out * out.shape[0] * out.shape[1] * out.shape[2]
        row = {"what": "conv", "layer": name, "mode": mode, "h_in": h_in, "c_in": c_in, "c_out": c_out}
        m = timed(lambda: ops.conv_forward(xin, w, None, None, mode, 0, False), a.iters)
        row["fwd_ms"], row["fwd_TFLOPs"] = round(m, 4), round(flop / m / 1e9, 1)
        forms = ("polyphase", "dilated") if mode == "c4s2" else ("plain",)
        for form in forms:
            old = ops.C4S2_DGRAD_FORM
            if mode == "c4s2":
                ops.C4S2_DGRAD_FORM = form
            m = timed(lambda: ops.conv_dgrad(geo, wc, gz, xin.shape), a.iters)
            ops.C4S2_DGRAD_FORM = old
            row[f"dgrad_{form}_ms"], row[f"dgrad_{form}_TFLOPs"] = round(m, 4), round(flop / m / 1e9, 1)
        m = timed(lambda: ops.conv_wgrad(geo, wc, xin, gz, False), a.iters)
        row["wgrad_ms"], row["wgrad_TFLOPs"] = round(m, 4), round(flop / m / 1e9, 1)
        print(json.dumps(row), flush=True)
        del xin, out, gz


def child_model(a):
    import torch
    from transvae import TransVAE, TransVAELoss
    from transvae.optim import FusedAdamW
    from transvae.parallel import clip_and_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.rand(a.batch, 3, a.res, a.res, device=dev)
    loss_fn = TransVAELoss(lpips_weight=0.0, use_gan=True, gan_weight=0.05)
    for frozen in (True, False):
        m = TransVAE(variant="large", compression_ratio=16, latent_dim=32).to(dev).train()
        D = make_disc(dev)
        if frozen:
            m.encoder.requires_grad_(False)
            m.conv_mu.requires_grad_(False)
            m.conv_logvar.requires_grad_(False)
        params = [p for p in m.parameters() if p.requires_grad]
        opt = FusedAdamW(params, lr=1e-5, betas=(0.9, 0.95), weight_decay=0.0)

        def step():
            opt.zero_grad(set_to_none=True)
            recon, mu, logvar = m(x)
            loss_fn(recon, x, mu, logvar, discriminator=D)["total"].backward()
            clip_and_step(params, opt, 1.0)
        ms = [timed(step, max(2, a.iters // 3), warmup=2) for _ in range(2)]
        print(json.dumps({"what": "stage-2 generator step", "model": "large_f16d32", "batch": a.batch, "res": a.res, "encoder_frozen": frozen,
                          "ms": [round(v, 2) for v in ms], "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}), flush=True)
        del m, D, opt, params
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


def child_trace(a):
    import torch
    dev = torch.device("cuda:0")
    D = make_disc(dev)
    torch.manual_seed(0)
    x = torch.rand(a.batch, 3, a.res, a.res, device=dev).requires_grad_(True)
    for _ in range(a.iters):
        disc_fwd_bwd(D, x)
    torch.cuda.synchronize()


def run(cmd, limit):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"step failed with status {r.returncode}: nothing more is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-ms", type=float, default=None, help="train-step time of bench.py on the same box")
    ap.add_argument("--bench-images-per-s", type=float, default=None, help="bench.py --steps 20 --warmup 5 figure of the same box")
    ap.add_argument("--skip-model", action="store_true", help="leave out the Large stage-2 steps (c), (d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gan_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "gan_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--child", choices=("disc", "model", "trace"))
    a = ap.parse_args()
    if a.child:
        return {"disc": child_disc, "model": child_model, "trace": child_trace}[a.child](a)
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--res", str(a.res), "--iters", str(a.iters)]
    rows = [json.loads(l) for l in run(me + ["--child", "disc"], 300).splitlines() if l.startswith("{")]
    if not a.skip_model:
        rows += [json.loads(l) for l in run(me + ["--child", "model"], 500).splitlines() if l.startswith("{")]
    for r in rows:
        print(json.dumps(r))
    if a.trace_dir is None:
        import tempfile
        a.trace_dir = tempfile.mkdtemp(prefix="gan_trace_")
    os.makedirs(a.trace_dir, exist_ok=True)
    run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace_dir, "-o", "gan", "--output-format", "csv", "--"] + me + ["--child", "trace"], 300)
    stats = sorted(glob.glob(os.path.join(a.trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    kernels = []
    if stats:
        os.makedirs(os.path.dirname(a.stats_out), exist_ok=True)
        shutil.copyfile(stats[-1], a.stats_out)
        nbytes = algorithmic_bytes(a.batch, a.res, a.res)
        with open(stats[-1]) as f:
            for r in csv.DictReader(f):
                name, calls, total_ns = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
                row = {"kernel": name[:80], "calls": calls, "ms_per_iter": round(total_ns / 1e6 / a.iters, 4), "percent": float(r["Percentage"])}
                for fam, nb in nbytes.items():
                    if fam in name.replace(" ", "") and "finalize" not in name:
                        row["effective_TBps"] = round(nb / (total_ns / a.iters) / 1e3, 3)
                kernels.append(row)
                print(json.dumps(row))
    out = {"batch": a.batch, "res": a.res, "iters": a.iters, "rows": rows, "kernels": kernels}
    steps = {r["encoder_frozen"]: min(r["ms"]) for r in rows if r["what"] == "stage-2 generator step"}
    if len(steps) == 2:
        out["frozen_over_unfrozen"] = round(steps[True] / steps[False], 4)
    if a.step_ms:
        out["train_step_ms"] = a.step_ms
    if a.bench_images_per_s:
        out["bench_images_per_s"] = a.bench_images_per_s
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
