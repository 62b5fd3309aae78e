"""Cost of the latent DiT (transvae.dit, csrc/dit.hip).  GPU box.

    python tools/dit_bench.py [--iters 10] [--out profiles/dit_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `kernels`: device events around warmed-up loops, three windows each: the seven kernels of csrc/dit.hip at DiT-B's shape
              (256 samples x 256 tokens x 768; the flow kernels on 256 x 32 x 16 x 16 latents), each with its host glue; TB/s on the
              algorithmic bytes of the file's header.
2. `step`:    one training step of DiT-B at patch size 1 on 256 x 32 x 16 x 16 latents (`flow_matching_loss` + `FusedAdamW`), and
              beside it the eager form of the restatement (tests/dit_restatement.py) under bf16 autocast with
              `scaled_dot_product_attention` and `torch.optim.AdamW`, same box, same run.
3. `sample`:  fifty Euler steps at cfg_scale = 1.5 for 64 images with DiT-B, including the decode through TransVAE-large f16d32.
4. `trace`:   `iters` training steps and three Euler steps under `rocprofv3 --kernel-trace --stats`, a run of its own ->
              profiles/dit_kernel_stats.csv; the kernel-time TB/s figures and the split of the step into token GEMMs, attention,
              the row kernels of csrc/dit.hip and everything else (the torch conditioning path, the optimizer, copies) come from there.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, N, C, D, HW, P = 256, 256, 768, 32, 16, 1
T, LD = B * N, 32
LAT = B * D * HW * HW
BYTES = {"tv_adaln_fwd": 4 * T * C, "tv_adaln_bwd": 8 * T * C, "tv_gate_residual_fwd": 6 * T * C, "tv_gate_residual_bwd": 6 * T * C,
         "tv_flow_rows": 8 * LAT + 2 * T * LD, "tv_flow_loss": 8 * LAT + 4 * T * LD, "tv_flow_euler": 8 * LAT + 4 * T * LD}
KERNEL_OF = {"adaln_fwd_kernel": "tv_adaln_fwd", "adaln_bwd_kernel": "tv_adaln_bwd", "gate_fwd_kernel": "tv_gate_residual_fwd",
             "gate_bwd_kernel": "tv_gate_residual_bwd", "flow_rows_kernel": "tv_flow_rows", "flow_loss_kernel": "tv_flow_loss",
             "flow_euler_kernel": "tv_flow_euler"}


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


def kernel_cases():
    import torch
    from transvae import dit
    dev = torch.device("cuda:0")
    x = torch.randn(T, C, device=dev).bfloat16()
    y = torch.randn(T, C, device=dev).bfloat16()
    g = torch.randn(T, C, device=dev).bfloat16()
    mod = torch.randn(B, 6 * C, device=dev) * 0.1
    lat, noise = torch.randn(B, D, HW, HW, device=dev), torch.randn(B, D, HW, HW, device=dev)
    mean, rstd, t = torch.zeros(D, device=dev), torch.ones(D, device=dev), torch.rand(B, device=dev)
    pred = torch.randn(T, LD, device=dev).bfloat16()
    v2 = torch.randn(2 * T, LD, device=dev).bfloat16()
    xs = noise.clone()
    xg = x.clone().requires_grad_(True)
    yg = y.clone().requires_grad_(True)
    modg = mod.clone().requires_grad_(True)

    def adaln_bwd():
        a, hs = dit.adaln(xg, modg, 0, C, N)
        torch.autograd.backward([a, hs], [g, g])
        xg.grad = modg.grad = None

    def gate_bwd():
        dit.gate_residual(xg, yg, modg, 2 * C, N).backward(g)
        xg.grad = yg.grad = modg.grad = None
    return {"tv_adaln_fwd": lambda: dit.adaln(x, mod, 0, C, N),
            "tv_adaln_bwd": adaln_bwd,                       # (forward + backward: the forward's share is the row above)
            "tv_gate_residual_fwd": lambda: dit.gate_residual(x, y, mod, 2 * C, N),
            "tv_gate_residual_bwd": gate_bwd,                # (forward + backward)
            "tv_flow_rows": lambda: dit.flow_rows(lat, mean, rstd, P, noise, t),
            "tv_flow_loss": lambda: dit.flow_loss(pred, lat, mean, rstd, noise, P),
            "tv_flow_euler": lambda: dit.flow_euler(xs, v2, P, 0.02, 1.5)}


def step_cases():
    import torch
    import transvae
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(B, D, HW, HW, device=dev)
    labels = torch.randint(0, 1000, (B,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    m = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev).train()
    opt = transvae.optim.FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)

    def hip_step():
        opt.zero_grad(set_to_none=True)
        transvae.flow_matching_loss(m, lat, labels, stats, generator=gen, check_labels=False)
        opt.step()
    return m, hip_step, lat, labels, stats


def eager_case(lat, labels):
    import torch
    import dit_restatement as R
    dev = lat.device
    ref = R.DiTRef((HW, HW), P, D, C, 12, 1000).to(dev)
    eopt = torch.optim.AdamW(ref.parameters(), lr=1e-4, weight_decay=0.0)

    def eager_step():
        eopt.zero_grad(set_to_none=True)
        t = torch.sigmoid(torch.randn(B, device=dev))
        e = torch.randn_like(lat)
        tt = t.view(-1, 1, 1, 1)
        xt = tt * lat + (1 - tt) * e
        with torch.autocast("cuda", dtype=torch.bfloat16):
            v = ref(xt, t, labels)
        ((v.float() - (lat - e)) ** 2).mean().backward()
        eopt.step()
    return eager_step


def child_kernels(a):
    for name, fn in kernel_cases().items():
        ms = [timed(fn, a.iters) for _ in range(3)]
        print(json.dumps({"what": name + " (with its host glue; the bwd rows are forward + backward under autograd)",
                          "case": f"{B} x {N} x {C}" if "flow" not in name else f"{B} x {D} x {HW}^2, p = {P}",
                          "ms": [round(m, 4) for m in ms], "algorithmic_bytes": BYTES[name]}), flush=True)


def child_step(a):
    _, hip_step, lat, labels, _ = step_cases()
    mh = [timed(hip_step, a.iters) for _ in range(3)]
    print(json.dumps({"what": "one DiT-B training step, HIP path", "case": f"{B} x {D} x {HW}^2, p = {P}", "ms": [round(m, 3) for m in mh]}), flush=True)
    me = [timed(eager_case(lat, labels), a.iters) for _ in range(1)]
    print(json.dumps({"what": "one DiT-B training step, eager restatement (bf16 autocast, SDPA, torch.optim.AdamW)",
                      "case": f"{B} x {D} x {HW}^2, p = {P}", "ms": [round(m, 3) for m in me]}), flush=True)


def child_sample(a):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    m = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev).eval()
    vae = transvae.create_transvae("large", 16, 32).to(dev).eval()
    labels = torch.randint(0, 1000, (64,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    gen = torch.Generator(device=dev).manual_seed(0)
    fn = lambda: transvae.sample_images(vae, m, labels, steps=50, cfg_scale=1.5, generator=gen, stats=stats)
    ms = [timed(fn, 1, warmup=1) for _ in range(2)]
    lat_ms = timed(lambda: transvae.sample_latents(m, labels, steps=50, cfg_scale=1.5, generator=gen, stats=stats), 1, warmup=0)
    print(json.dumps({"what": "50 Euler steps at cfg_scale 1.5 for 64 images, DiT-B, with the TransVAE-large f16d32 decode",
                      "ms": [round(x, 2) for x in ms], "latents_only_ms": round(lat_ms, 2)}), flush=True)


def child_trace(a):
    import torch
    euler = kernel_cases()["tv_flow_euler"]
    for _ in range(3):
        euler()
    _, hip_step, _, _, _ = step_cases()
    for _ in range(a.iters):
        hip_step()
    torch.cuda.synchronize()


def run_child(step, a, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--iters", str(a.iters)]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"dit_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def group_of(name):
    if any(k in name for k in KERNEL_OF) or "mod_finalize" in name or "flow_loss_finalize" in name:
        return "row kernels (csrc/dit.hip)"
    if "attn" in name or "rope" in name:
        return "attention"
    if "igemm" in name or "wgrad" in name or "pack_weight" in name or "pack_multi" in name or "act_bwd" in name:      # (act_bwd: fc1's GELU backward)
        return "token GEMMs"
    if "opt_" in name or "adamw" in name or "grad_norm" in name:
        return "optimizer"
    return "conditioning path and other torch kernels"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dit_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "dit_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    children = {"kernels": child_kernels, "step": child_step, "sample": child_sample, "trace": child_trace}
    if a.child:
        return children[a.child](a)
    rows = []
    for step, limit in (("kernels", 240), ("step", 300)) + ((("sample", 300),) if not a.no_sample else ()):
        rows += [json.loads(l) for l in run_child(step, a, limit).splitlines() if l.startswith("{")]
    for r in rows:
        if "algorithmic_bytes" in r:
            r["tb_per_s_call"] = round(r["algorithmic_bytes"] / min(r["ms"]) / 1e9, 3)
        print(r)
    report = {"rows": rows}
    if not a.no_trace:
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="dit_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 300, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "dit", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            with open(a.stats_out) as f:
                table = list(csv.DictReader(f))
            # The trace child runs `iters` training steps (every kernel of csrc/dit.hip but the Euler step runs inside them at
            # DiT-B's shape: adaLN and gates 25 / 24 times a step, flow rows / loss once) and three stand-alone Euler steps.
            report["kernel_tb_per_s"] = {}
            groups = {}
            for row in table:
                name, total_ns = row.get("Name", ""), float(row.get("TotalDurationNs") or 0)
                avg_ns = float(row.get("AverageNs") or 0)
                for k, api in KERNEL_OF.items():
                    if k in name and avg_ns:
                        report["kernel_tb_per_s"][api] = {"avg_us": round(avg_ns / 1e3, 2), "calls": int(row.get("Calls") or 0),
                                                          "tb_per_s": round(BYTES[api] / avg_ns / 1e3, 3)}
                if "flow_euler" not in name:
                    groups[group_of(name)] = groups.get(group_of(name), 0.0) + total_ns
            ent = report["kernel_tb_per_s"].get("tv_adaln_bwd")
            if ent:
                ent["note"] = "8 T C bytes: 24 of the 25 calls of a step carry dres (the final layer's reads 6 T C)"
            tot = sum(groups.values()) or 1.0
            report["step_kernel_ms"] = {k: round(v / 1e6 / a.iters, 3) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])}
            report["step_kernel_share"] = {k: round(v / tot, 4) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])}
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
