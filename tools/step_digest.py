#!/usr/bin/env python3
"""Step digests: SHA-256 of every parameter, every gradient and the loss after N deterministic train steps.

`bench.py --dump-outputs` compares two builds output for output, but with the default kernels two runs of the SAME build
already differ in every split-K weight gradient (fp32 atomics).  Inside `transvae.deterministic()` they do not, so a digest
per tensor is a build-against-build comparison at step level: run this on two builds and diff the JSON.

    python tools/step_digest.py --steps 3 --out digests.json                        # micro model, seconds
    python tools/step_digest.py --variant large --res 256 --batch 256 --micro-batch 128 --time

Everything random is drawn on the CPU from --seed (weights: the fan-in rule of bench.py; images; the encoder's noise), so the
digests depend on the build and the split heuristics only.  --time also measures what the mode costs: train steps with the
mode off and on in alternating windows of one process, timed with device events, written to profiles/deterministic_mode.json
together with the largest workspace the steps asked for.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "deepl-project_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

MICRO = dict(depths=[1, 1, 1, 1, 1], base_dims=[32, 32, 64, 64, 128], mlp_ratio=1.0, head_dim=64)   # the micro model of the tests


def build_model(variant: str, seed: int, device):
    """A TransVAE variant with seeded fan-in scaled weights (drawn on the CPU: the same numbers on every build)."""
    from transvae import TransVAE
    if variant == "micro":
        m = TransVAE(config=dict(MICRO), variant="micro", compression_ratio=16, latent_dim=4, clamp_latent=True)
    else:
        m = TransVAE(variant=variant, compression_ratio=16, latent_dim=32, clamp_latent=True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (p.shape[1] * p.shape[2] * p.shape[3]) ** -0.5)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            elif name.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            else:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    return m.to(device).train()


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _stepper(variant, batch, res, micro, seed, device):
    """(model, one_step() -> loss tensor): train_step + FusedAdamW + clip 1.0 on seeded images and noise"""
    from transvae.optim import FusedAdamW
    from transvae.parallel import train_step, vae_bench_loss
    m = build_model(variant, seed, device)
    opt = FusedAdamW(m.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(batch, 3, res, res, generator=g).to(device)
    lat_c = 4 if variant == "micro" else 32
    counters = {}

    def forward_loss(model, xb):
        eps = torch.randn(xb.shape[0], lat_c, xb.shape[-1] // 16, xb.shape[-1] // 16, generator=g).to(device)
        recon, mu, logvar = model(xb, eps=eps)
        return vae_bench_loss(recon, xb, mu, logvar)

    def one_step():
        return train_step(m, opt, x, micro, forward_loss, 1.0, batch, counters)
    return m, one_step


def step_digest(steps: int = 3, variant: str = "micro", batch: int = 4, res: int = 64, micro: int = 2, seed: int = 0,
                device="cuda:0") -> dict:
    """`steps` train steps inside transvae.deterministic() from seeded weights and inputs ->
    {"config": ..., "loss": [hex of every step's loss], "params": {name: sha256}, "grads": {name: sha256 of the last step's}}"""
    import transvae
    device = torch.device(device)
    with torch.cuda.device(device), transvae.deterministic():
        m, one_step = _stepper(variant, batch, res, micro, seed, device)
        losses = [one_step() for _ in range(steps)]
        torch.cuda.synchronize()
    return {
        "config": dict(steps=steps, variant=variant, batch=batch, res=res, micro=micro, seed=seed),
        "loss": [float(v).hex() for v in losses],
        "loss_sha256": _sha(torch.stack([v.detach().double().reshape(()) for v in losses])),
        "params": {n: _sha(p) for n, p in m.named_parameters()},
        "grads": {n: _sha(p.grad) for n, p in m.named_parameters() if p.grad is not None},
    }


def time_modes(variant: str = "large", batch: int = 256, res: int = 256, micro: int = 128, seed: int = 0, windows: int = 3,
               steps_per_window: int = 2, device="cuda:0") -> dict:
    """Step time with the mode off and on: after a warm-up step of each, `windows` alternating windows of `steps_per_window` steps
    per mode in one process (same model, same allocator state, same clocks), device events around each window."""
    from transvae.hip import ops
    device = torch.device(device)
    with torch.cuda.device(device):
        m, one_step = _stepper(variant, batch, res, micro, seed, device)
        ms = {False: [], True: []}
        for on in (False, True):                 # warm-up: allocator, workspaces, function attributes
            with ops.deterministic(on):
                one_step()
        torch.cuda.synchronize()
        for _ in range(windows):
            for on in (False, True):
                with ops.deterministic(on):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(steps_per_window):
                        one_step()
                    b.record()
                    b.synchronize()
                    ms[on].append(a.elapsed_time(b) / steps_per_window)
        off, on_ = min(ms[False]), min(ms[True])
        return {
            "config": dict(variant=variant, batch=batch, res=res, micro=micro, windows=windows, steps_per_window=steps_per_window),
            "device": torch.cuda.get_device_name(device),
            "step_ms_off": ms[False], "step_ms_on": ms[True],
            "best_step_ms_off": off, "best_step_ms_on": on_, "on_over_off": on_ / off,
            "peak_workspace_bytes": ops.det_stats["peak_bytes"],
            "peak_memory_gib": torch.cuda.max_memory_allocated(device) / 2 ** 30,
        }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--variant", default="micro")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--micro-batch", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the digests here as JSON")
    ap.add_argument("--time", action="store_true", help="time the steps with the mode off and on instead of digesting them")
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "deterministic_mode.json"))
    args = ap.parse_args()
    if args.time:
        r = time_modes(args.variant, args.batch, args.res, args.micro_batch, args.seed)
        path = args.time_out
    else:
        r = step_digest(args.steps, args.variant, args.batch, args.res, args.micro_batch, args.seed)
        path = args.out
    print(json.dumps(r, indent=1))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
