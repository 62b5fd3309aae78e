"""Cost of the reconstruction metrics (transvae.metrics, csrc/metrics.hip) and of evaluate() against model() alone.  GPU box.

    python tools/eval_bench.py [--iters 20] [--variant large]

1. The metrics launches alone (stencil + finalise), both SSIM windows, on fp32 NCHW pairs at batch 64 x 3 x 256^2 and
   batch 8 x 3 x 1024^2.  Effective GB/s counts the algorithmic bytes, 8 B per element pair read once (B*C*H*W * 8).
2. model(images) alone vs evaluate(model, loader) on the same batches (Large f16d32, 256^2, batch 64): the metrics'
   share of an evaluation step.
Device events around warmed-up loops; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))
from transvae import TransVAE, evaluate  # noqa: E402
from transvae.metrics import reconstruction_metrics  # noqa: E402


def timed(fn, iters, warmup=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--variant", default="large")
    ap.add_argument("--model-batches", type=int, default=4, help="batches of 64 in the evaluate() loader")
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    for B, H in ((64, 256), (8, 1024)):
        t = torch.rand(B, 3, H, H, device=dev)
        r = (t + 0.1 * torch.randn_like(t)).contiguous()
        nbytes = 8 * r.numel()
        for window in ("skimage", "box11"):
            ms = timed(lambda: reconstruction_metrics(r, t, ssim_window=window), a.iters)
            rows.append({"what": "metrics", "batch": B, "res": H, "window": window, "ms": round(ms, 4),
                         "effective_GBps": round(nbytes / ms / 1e6, 1)})
            print(json.dumps(rows[-1]), flush=True)
    if not a.skip_model:
        model = TransVAE(variant=a.variant, compression_ratio=16, latent_dim=32).to(dev).eval()
        loader = [(torch.rand(64, 3, 256, 256, device=dev), None) for _ in range(a.model_batches)]

        def forward_only():
            with torch.no_grad():
                for images, _ in loader:
                    model(images)
        t_model = timed(forward_only, max(1, a.iters // 4), warmup=1)
        t_eval = timed(lambda: evaluate(model, loader, metrics=("psnr", "ssim", "mse"), device=dev), max(1, a.iters // 4), warmup=1)
        rows.append({"what": "evaluate", "variant": a.variant, "batch": 64, "res": 256, "batches": a.model_batches,
                     "model_ms": round(t_model, 3), "evaluate_ms": round(t_eval, 3),
                     "overhead_pct": round(100 * (t_eval - t_model) / t_model, 2)})
        print(json.dumps(rows[-1]), flush=True)


if __name__ == "__main__":
    main()
