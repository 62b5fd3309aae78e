"""Cost of the head_dim 72 kernels (csrc/attention_hd.hip, and the <72> instantiations of csrc/qk_norm.hip) and of the XL models (transvae.dit_xl / lightning_dit_xl).  GPU box.

    python tools/dit_xl_bench.py [--iters 5] [--out profiles/dit_xl_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.  At most 16 host threads.
1. `kernels`: device events around warmed-up loops of C-ABI calls, three alternating windows each, at 256 samples x 256 tokens x
              width 1152: the new attention forward and backward, `tv_rope_qk_hd` and the qk-norm pair at 16 heads of 72, beside
              the existing kernels at 18 heads of 64 in the same process -- the same width, hence the same qkv bytes and the same
              4 B N^2 C FLOPs per pass.  `ratio_72_over_64` is reported, not gated.
2. `step`:    one DiT-XL and one LightningDiT-XL training step at patch size 1 on 256 x 32 x 16 x 16 latents (`flow_matching_loss` +
              `FusedAdamW`) in alternating windows, beside the eager form of the restatement (tests/hd72_restatement.py) under bf16
              autocast with `scaled_dot_product_attention` at head_dim 72 and `torch.optim.AdamW`.  The eager form runs at the
              largest power-of-two batch up to 256 that fits; when that is below 256 the HIP steps are timed at that batch as well,
              and `hip_over_eager` compares equal batches.  The gate: `hip_over_eager` <= 1.
3. `sample`:  fifty Euler steps at cfg_scale = 1.5 for 64 images with each XL model (latents only).
4. `trace`:   the kernels of step 1, `iters` calls each, under `rocprofv3 --kernel-trace --stats`, a run of its own ->
              profiles/dit_xl_kernel_stats.csv; `kernel_us` holds the per-kernel averages.
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

B, N, C_, D, HW, P, DEPTH = 256, 256, 1152, 32, 16, 1, 28
GEOM = {72: 16, 64: 18}                       # head_dim -> heads at width 1152
FLOPS = 4 * B * N * N * C_                    # one pass of q k^T and P v (the backward: 2.5 x by the formulas, 3.5 x as split here)
KERNELS = ("attn72_fwd_kernel", "attn72_delta_kernel", "attn72_bwd_dq_kernel", "attn72_bwd_dkv_kernel", "rope_qk72_kernel",
           "qknorm_rope_fwd_kernel<72>", "qknorm_rope_bwd_kernel<72>", "qknorm_finalize_kernel<72>",
           "attn_fwd_kernel", "attn_delta_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel", "rope_qk_kernel",
           "qknorm_rope_fwd_kernel<64>", "qknorm_rope_bwd_kernel<64>", "qknorm_finalize_kernel<64>")
PAIRS = ("attn_fwd", "attn_bwd", "rope_qk", "qknorm_rope_fwd", "qknorm_rope_bwd")


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
    """(name, head_dim) -> a call of the kernel through the C ABI on preallocated operands"""
    import torch
    from transvae.hip import _lib as L
    from transvae.modules.attention import RoPE2D
    lib = L.load()
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bf = lambda *s: torch.randn(*s, device=dev).bfloat16()
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    qkv, dqkv, o, do = bf(B, N, 3 * C_), bf(B, N, 3 * C_), bf(B, N, C_), bf(B, N, C_)
    cases, keep = {}, [qkv, dqkv, o, do]

    def call(name, *args):
        fn = getattr(lib, name)
        return lambda: L.check(fn(*args, st()), name)
    for hd, heads in GEOM.items():
        s = "_hd" if hd == 72 else ""
        h = (hd,) if hd == 72 else ()
        lse, delta = f32(B, heads, N), f32(2, B, heads, N)
        tab = RoPE2D(hd).to(dev).table(HW, HW).contiguous()
        wq, wk, dwq, dwk = torch.ones(hd, device=dev), torch.ones(hd, device=dev), f32(hd), f32(hd)
        part = f32(getattr(lib, f"tv_qknorm_rope_bwd{s}_partial_count")(B, N, heads, *h))
        keep += [lse, delta, tab, wq, wk, dwq, dwk, part]
        scale = hd ** -0.5
        cases["attn_fwd", hd] = call("tv_attn_fwd" + s, p(qkv), p(o), p(lse), B, N, heads, *h, scale)
        cases["attn_bwd", hd] = call("tv_attn_bwd" + s, p(qkv), p(o), p(do), p(lse), p(delta), p(tab), p(dqkv), B, N, heads, *h, scale)
        cases["rope_qk", hd] = call("tv_rope_qk" + s, p(dqkv), p(tab), B, N, heads, *h, 0)
        cases["qknorm_rope_fwd", hd] = call("tv_qknorm_rope_fwd" + s, p(qkv), p(wq), p(wk), p(tab), p(dqkv), B, N, heads, *h, 1e-6)
        cases["qknorm_rope_bwd", hd] = call("tv_qknorm_rope_bwd" + s, p(qkv), p(wq), p(wk), p(dqkv), p(dwq), p(dwk), p(part), B, N, heads, *h, 1e-6)
    return cases, keep


def child_kernels(a):
    cases, _keep = kernel_cases()
    cases["attn_fwd", 72]()          # lse of the 72 geometry for its backward (the 64 backward reads its own below)
    for name in PAIRS:
        ms = {72: [], 64: []}
        for _ in range(3):           # alternating windows of the two head dimensions
            for hd in (72, 64):
                if name == "attn_bwd":
                    cases["attn_fwd", hd]()
                ms[hd].append(timed(cases[name, hd], a.iters))
        row = {"what": f"tv_{name} (one C-ABI call)", "case": f"{B} x {N} x {C_}: 16 heads of 72 | 18 heads of 64",
               "ms_72": [round(m, 4) for m in ms[72]], "ms_64": [round(m, 4) for m in ms[64]],
               "ratio_72_over_64": round(min(ms[72]) / min(ms[64]), 3)}
        if name.startswith("attn"):
            row["tflops_72"] = round(FLOPS * (1.0 if name == "attn_fwd" else 2.5) / min(ms[72]) / 1e9, 1)
            row["tflops_64"] = round(FLOPS * (1.0 if name == "attn_fwd" else 2.5) / min(ms[64]) / 1e9, 1)
        print(json.dumps(row), flush=True)


def hip_step_case(model, batch):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(batch, D, HW, HW, device=dev)
    labels = torch.randint(0, 1000, (batch,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    m = model.to(dev).train()
    opt = transvae.optim.FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)

    def step():
        opt.zero_grad(set_to_none=True)
        transvae.flow_matching_loss(m, lat, labels, stats, generator=gen, check_labels=False)
        opt.step()
    return step


def eager_case(kind, batch):
    import torch
    import hd72_restatement as H
    dev = torch.device("cuda:0")
    on = kind == "LightningDiT-XL"
    ref = H.HdRef((HW, HW), P, D, C_, DEPTH, 1000, head_dim=72, use_rmsnorm=on, use_qknorm=on, use_swiglu=on).to(dev)
    eopt = torch.optim.AdamW(ref.parameters(), lr=1e-4, weight_decay=0.0)
    lat = torch.randn(batch, D, HW, HW, device=dev)
    labels = torch.randint(0, 1000, (batch,), device=dev)

    def eager_step():
        eopt.zero_grad(set_to_none=True)
        t = torch.sigmoid(torch.randn(batch, device=dev))
        e = torch.randn_like(lat)
        tt = t.view(-1, 1, 1, 1)
        xt = tt * lat + (1 - tt) * e
        with torch.autocast("cuda", dtype=torch.bfloat16):
            v = ref(xt, t, labels)
        ((v.float() - (lat - e)) ** 2).mean().backward()
        eopt.step()
    return eager_step


def child_eager(a):
    """the eager form of a.kind at the largest power-of-two batch <= 256 that fits"""
    import torch
    batch = a.batch
    while batch >= 8:
        try:
            ms = [timed(eager_case(a.kind, batch), a.iters, warmup=1)]
            print(json.dumps({"what": f"one {a.kind} training step, eager restatement (bf16 autocast, SDPA at head_dim 72, torch.optim.AdamW)",
                              "case": f"{batch} x {D} x {HW}^2, p = {P}", "batch": batch, "kind": a.kind, "eager": True, "ms": [round(m, 3) for m in ms]}), flush=True)
            return
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
            batch //= 2
    raise SystemExit("the eager form fits at no batch of 8 or more")


def child_step(a):
    import transvae
    batches = sorted({B, a.batch}, reverse=True)
    for batch in batches:
        steps = {"DiT-XL": hip_step_case(transvae.dit_xl(HW, P, D, 1000), batch),
                 "LightningDiT-XL": hip_step_case(transvae.lightning_dit_xl(HW, P, D, 1000), batch)}
        ms = {k: [] for k in steps}
        for _ in range(3):                                            # alternating windows of the two models
            for k, fn in steps.items():
                ms[k].append(timed(fn, a.iters))
        for k in steps:
            print(json.dumps({"what": f"one {k} training step, HIP path", "case": f"{batch} x {D} x {HW}^2, p = {P}", "batch": batch, "kind": k,
                              "ms": [round(m, 3) for m in ms[k]]}), flush=True)
        del steps


def child_sample(a):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    for kind, make in (("DiT-XL", transvae.dit_xl), ("LightningDiT-XL", transvae.lightning_dit_xl)):
        m = make(HW, P, D, 1000).to(dev).eval()
        labels = torch.randint(0, 1000, (64,), device=dev)
        stats = (torch.zeros(D), torch.ones(D))
        gen = torch.Generator(device=dev).manual_seed(0)
        fn = lambda: transvae.sample_latents(m, labels, steps=50, cfg_scale=1.5, generator=gen, stats=stats)
        ms = [timed(fn, 1, warmup=1 if i == 0 else 0) for i in range(3)]
        print(json.dumps({"what": f"50 Euler steps at cfg_scale 1.5 for 64 images, {kind}, latents only", "ms": [round(x, 2) for x in ms]}), flush=True)
        del m


def child_trace(a):
    import torch
    cases, _keep = kernel_cases()
    for hd in (72, 64):
        for name in PAIRS:
            if name == "attn_bwd":
                cases["attn_fwd", hd]()
            for _ in range(a.iters):
                cases[name, hd]()
    torch.cuda.synchronize()


def is_kernel(k, name):
    """Whether a rocprofv3 kernel name is kernel k of KERNELS.  Names come demangled or, for some, mangled; the qk-norm kernels are
    one template over head_dim, `kernel<72>` demangled and `kernelILi72EE` mangled."""
    base, _, arg = k.partition("<")
    return f"::{k}(" in name or f"{len(base)}{base}" + (f"ILi{arg[:-1]}EE" if arg else "E") in name


def kernel_table(path):
    """kernel -> average time and calls out of a rocprofv3 kernel_stats.csv"""
    with open(path) as f:
        table = list(csv.DictReader(f))
    out = {}
    for row in table:
        name, avg_ns = row.get("Name", ""), float(row.get("AverageNs") or 0)
        for k in KERNELS:
            if is_kernel(k, name):
                out[k] = {"avg_us": round(avg_ns / 1e3, 2), "calls": int(row.get("Calls") or 0)}
    return out


def run_child(step, a, timeout, prefix=(), extra=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--iters", str(a.iters)] + list(extra)
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"dit_xl_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dit_xl_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "dit_xl_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--kind", default="DiT-XL")
    ap.add_argument("--batch", type=int, default=B)
    a = ap.parse_args()
    children = {"kernels": child_kernels, "step": child_step, "eager": child_eager, "sample": child_sample, "trace": child_trace}
    if a.child:
        return children[a.child](a)
    parse = lambda out: [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    rows = parse(run_child("kernels", a, 240))
    eager = [parse(run_child("eager", a, 420, extra=("--kind", k)))[0] for k in ("DiT-XL", "LightningDiT-XL")]
    eager_batch = min(e["batch"] for e in eager)
    if any(e["batch"] != eager_batch for e in eager):     # one batch for both eager forms
        eager = [parse(run_child("eager", a, 420, extra=("--kind", k, "--batch", str(eager_batch))))[0] for k in ("DiT-XL", "LightningDiT-XL")]
    rows += parse(run_child("step", a, 420, extra=("--batch", str(eager_batch)))) + eager
    if not a.no_sample:
        rows += parse(run_child("sample", a, 300))
    for r in rows:
        print(r)
    report = {"rows": rows, "eager_batch": eager_batch, "hip_over_eager": {}}
    for e in eager:
        hip = [r for r in rows if r.get("kind") == e["kind"] and r.get("batch") == eager_batch and not r.get("eager")]
        if hip:
            report["hip_over_eager"][e["kind"]] = round(min(hip[0]["ms"]) / min(e["ms"]), 3)
    if not a.no_trace:
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="dit_xl_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 300, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "dit_xl", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            report["kernel_us"] = kernel_table(a.stats_out)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)
    print(json.dumps({"hip_over_eager": report["hip_over_eager"], "eager_batch": eager_batch}))


if __name__ == "__main__":
    main()
