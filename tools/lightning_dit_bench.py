"""Cost of the LightningDiT block (transvae.lightning_dit; csrc/lightning.hip and the RMS adaLN of csrc/dit.hip).  GPU box.

    python tools/lightning_dit_bench.py [--iters 10] [--out profiles/lightning_dit_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.  At most 16 host threads.
1. `kernels`: device events around warmed-up loops of C-ABI calls, three windows each: the block's six kernels at
              LightningDiT-B's shape (256 samples x 256 tokens x 768, 12 heads, Hp = 2048) and, in the same process, the yardstick:
              `tv_adaln_fwd` / `_bwd` and `tv_gate_residual_fwd` / `_bwd` of csrc/dit.hip at that shape.  TB/s on the algorithmic bytes
              of the files' headers (`tv_adaln_*_bwd` with `dres`, `tv_qknorm_rope_fwd` in place).
2. `step`:    one training step of LightningDiT-B at patch size 1 on 256 x 32 x 16 x 16 latents (`flow_matching_loss` + `FusedAdamW`),
              beside a DiT-B step and the eager form of the restatement (tests/lightning_restatement.py) under bf16 autocast with
              `scaled_dot_product_attention` and `torch.optim.AdamW`, same box, same run.
3. `sample`:  fifty Euler steps at cfg_scale = 1.5 for 64 images with LightningDiT-B (latents only).
4. `trace`:   the ten kernels of step 1, `iters` calls each, under `rocprofv3 --kernel-trace --stats`, a run of its own ->
              profiles/lightning_dit_kernel_stats.csv; the kernel-time TB/s figures come from there, and `rms_over_layernorm` is the
              ratio of `tv_adaln_rms_*` to its yardstick in that one trace (the two move the same bytes).
"""
import argparse
import csv
import ctypes as C
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
for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[var] = str(min(16, int(os.environ.get(var) or 16)))

B, N, C_, HEADS, HP, D, HW, P = 256, 256, 768, 12, 2048, 32, 16, 1
T = B * N
BYTES = {"tv_adaln_rms_fwd": 4 * T * C_, "tv_adaln_rms_bwd": 8 * T * C_, "tv_qknorm_rope_fwd": 8 * T * C_, "tv_qknorm_rope_bwd": 12 * T * C_,
         "tv_swiglu_fwd": 6 * T * HP, "tv_swiglu_bwd": 10 * T * HP,
         "tv_adaln_fwd": 4 * T * C_, "tv_adaln_bwd": 8 * T * C_, "tv_gate_residual_fwd": 6 * T * C_, "tv_gate_residual_bwd": 6 * T * C_}
# kernel name -> C-ABI call; the adaLN pair is one template, `adaln_*_kernel<KCH, RMS>`: its `true>` instantiations are tv_adaln_rms_*.
# The qk-norm pair is one template over head_dim (csrc/qk_norm.hip): this run launches, and attributes, the <64> instantiations only.
KERNEL_OF = {"adaln_fwd_kernel": "tv_adaln_fwd", "adaln_bwd_kernel": "tv_adaln_bwd", "qknorm_rope_fwd_kernel": "tv_qknorm_rope_fwd",
             "qknorm_rope_bwd_kernel": "tv_qknorm_rope_bwd", "swiglu_fwd_kernel": "tv_swiglu_fwd", "swiglu_bwd_kernel": "tv_swiglu_bwd",
             "gate_fwd_kernel": "tv_gate_residual_fwd", "gate_bwd_kernel": "tv_gate_residual_bwd"}
YARDSTICK = {"tv_adaln_rms_fwd": "tv_adaln_fwd", "tv_adaln_rms_bwd": "tv_adaln_bwd"}


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
    """name -> a call of the kernel through the C ABI on preallocated operands"""
    import torch
    from transvae.hip import _lib as L
    from transvae.modules.attention import RoPE2D
    lib = L.load()
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bf = lambda *s: torch.randn(*s, device=dev).bfloat16()
    x, y, g, dres, out = bf(T, C_), bf(T, C_), bf(T, C_), bf(T, C_), bf(T, C_)
    mod, dmod = torch.randn(B, 6 * C_, device=dev) * 0.1, torch.empty(B, 6 * C_, device=dev)
    w, dw = 1 + 0.1 * torch.randn(C_, device=dev), torch.empty(C_, device=dev)
    qkv, dqkv = bf(T, 3 * C_), bf(T, 3 * C_)
    wq, wk, dwq, dwk = torch.ones(64, device=dev), torch.ones(64, device=dev), torch.empty(64, device=dev), torch.empty(64, device=dev)
    tab = RoPE2D(64).to(dev).table(HW, HW).contiguous()
    u, du, dh, h = bf(T, 2 * HP), bf(T, 2 * HP), bf(T, HP), bf(T, HP)
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
    part_rms, part_ln = f32(lib.tv_adaln_rms_bwd_partial_count(B, N, C_)), f32(lib.tv_adaln_bwd_partial_count(B, N, C_))
    part_qk, part_g = f32(lib.tv_qknorm_rope_bwd_partial_count(B, N, HEADS)), f32(lib.tv_gate_residual_bwd_partial_count(B, N, C_))
    ld, eps = 6 * C_, 1e-6

    def call(name, *args):
        fn = getattr(lib, name)
        return lambda: L.check(fn(*args, st()), name)
    return {
        "tv_adaln_rms_fwd": call("tv_adaln_rms_fwd", p(x), p(w), p(mod), 0, C_, ld, p(out), B, N, C_, eps),
        "tv_adaln_rms_bwd": call("tv_adaln_rms_bwd", p(x), p(w), p(mod), 0, C_, ld, p(g), p(dres), p(out), p(dmod), p(dw), p(part_rms), B, N, C_, eps),
        "tv_qknorm_rope_fwd": call("tv_qknorm_rope_fwd", p(qkv), p(wq), p(wk), p(tab), p(qkv), B, N, HEADS, eps),
        "tv_qknorm_rope_bwd": call("tv_qknorm_rope_bwd", p(qkv), p(wq), p(wk), p(dqkv), p(dwq), p(dwk), p(part_qk), B, N, HEADS, eps),
        "tv_swiglu_fwd": call("tv_swiglu_fwd", p(u), p(h), T, HP),
        "tv_swiglu_bwd": call("tv_swiglu_bwd", p(u), p(dh), p(du), T, HP),
        "tv_adaln_fwd": call("tv_adaln_fwd", p(x), p(mod), 0, C_, ld, p(out), B, N, C_, eps),
        "tv_adaln_bwd": call("tv_adaln_bwd", p(x), p(mod), 0, C_, ld, p(g), p(dres), p(out), p(dmod), p(part_ln), B, N, C_, eps),
        "tv_gate_residual_fwd": call("tv_gate_residual_fwd", p(x), p(y), p(mod), 2 * C_, ld, p(out), B, N, C_),
        "tv_gate_residual_bwd": call("tv_gate_residual_bwd", p(g), p(y), p(mod), 2 * C_, ld, p(out), p(dmod), p(part_g), B, N, C_),
    }, (x, y, g, dres, out, mod, dmod, w, dw, qkv, dqkv, wq, wk, dwq, dwk, tab, u, du, dh, h, part_rms, part_ln, part_qk, part_g)


def child_kernels(a):
    cases, _keep = kernel_cases()
    for name, fn in cases.items():
        ms = [timed(fn, a.iters) for _ in range(3)]
        print(json.dumps({"what": name + " (one C-ABI call, finalise launches included)", "case": f"{B} x {N} x {C_}, {HEADS} heads, Hp = {HP}",
                          "ms": [round(m, 4) for m in ms], "algorithmic_bytes": BYTES[name]}), flush=True)


def hip_step_case(model):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(B, D, HW, HW, device=dev)
    labels = torch.randint(0, 1000, (B,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    m = model.to(dev).train()
    opt = transvae.optim.FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)

    def step():
        opt.zero_grad(set_to_none=True)
        transvae.flow_matching_loss(m, lat, labels, stats, generator=gen, check_labels=False)
        opt.step()
    return step, lat, labels


def eager_case(lat, labels):
    import torch
    import lightning_restatement as LR
    dev = lat.device
    ref = LR.LightningDiTRef((HW, HW), P, D, C_, 12, 1000).to(dev)
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


def child_step(a):
    import torch
    import transvae
    case = f"{B} x {D} x {HW}^2, p = {P}"
    light, lat, labels = hip_step_case(transvae.create_lightning_dit("LightningDiT-B", HW, P, D, 1000))
    plain, _, _ = hip_step_case(transvae.create_dit("DiT-B", HW, P, D, 1000))
    ml, mp = [], []
    for _ in range(3):                                            # alternating windows of the two models
        ml.append(timed(light, a.iters))
        mp.append(timed(plain, a.iters))
    print(json.dumps({"what": "one LightningDiT-B training step, HIP path", "case": case, "ms": [round(m, 3) for m in ml]}), flush=True)
    print(json.dumps({"what": "one DiT-B training step, HIP path", "case": case, "ms": [round(m, 3) for m in mp]}), flush=True)
    del light, plain
    torch.cuda.empty_cache()
    me = [timed(eager_case(lat, labels), a.iters) for _ in range(1)]
    print(json.dumps({"what": "one LightningDiT-B training step, eager restatement (bf16 autocast, SDPA, torch.optim.AdamW)", "case": case,
                      "ms": [round(m, 3) for m in me]}), flush=True)


def child_sample(a):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    m = transvae.create_lightning_dit("LightningDiT-B", HW, P, D, 1000).to(dev).eval()
    labels = torch.randint(0, 1000, (64,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    gen = torch.Generator(device=dev).manual_seed(0)
    fn = lambda: transvae.sample_latents(m, labels, steps=50, cfg_scale=1.5, generator=gen, stats=stats)
    ms = [timed(fn, 1, warmup=1 if i == 0 else 0) for i in range(3)]
    print(json.dumps({"what": "50 Euler steps at cfg_scale 1.5 for 64 images, LightningDiT-B, latents only", "ms": [round(x, 2) for x in ms]}), flush=True)


def child_trace(a):
    import torch
    cases, _keep = kernel_cases()
    for fn in cases.values():
        for _ in range(a.iters):
            fn()
    torch.cuda.synchronize()


def kernel_report(stats_path):
    """per-call kernel time and TB/s out of a rocprofv3 kernel_stats.csv (names come demangled or, for some, mangled)"""
    with open(stats_path) as f:
        table = list(csv.DictReader(f))
    kt = {}
    for row in table:
        name, avg_ns = row.get("Name", ""), float(row.get("AverageNs") or 0)
        for k, api in KERNEL_OF.items():
            if k in name and avg_ns and not (k.startswith("qknorm_") and ("<72>" in name or "ILi72E" in name)):
                if k.startswith("adaln_") and ("true>" in name or "Lb1EE" in name):
                    api = api.replace("tv_adaln_", "tv_adaln_rms_")
                kt[api] = {"avg_us": round(avg_ns / 1e3, 2), "calls": int(row.get("Calls") or 0), "tb_per_s": round(BYTES[api] / avg_ns / 1e3, 3)}
    return {"kernel_tb_per_s": kt,
            "rms_over_layernorm": {k: round(kt[k]["avg_us"] / kt[v]["avg_us"], 3) for k, v in YARDSTICK.items() if k in kt and v in kt}}


def run_child(step, a, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--iters", str(a.iters)]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"lightning_dit_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightning_dit_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "lightning_dit_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    children = {"kernels": child_kernels, "step": child_step, "sample": child_sample, "trace": child_trace}
    if a.child:
        return children[a.child](a)
    rows = []
    for step, limit in (("kernels", 240), ("step", 420)) + ((("sample", 300),) if not a.no_sample else ()):
        rows += [json.loads(l) for l in run_child(step, a, limit).splitlines() if l.startswith("{")]
    for r in rows:
        if "algorithmic_bytes" in r:
            r["tb_per_s_call"] = round(r["algorithmic_bytes"] / min(r["ms"]) / 1e9, 3)
        print(r)
    report = {"rows": rows}
    if not a.no_trace:
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="lightning_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 300, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "lightning", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            report.update(kernel_report(a.stats_out))
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
