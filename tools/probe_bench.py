"""Cost of linear probing (transvae.probe, csrc/probe.hip).  GPU box.

    python tools/probe_bench.py [--iters 20] [--out profiles/probe_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `time`:  device events around warmed-up loops, three windows each:
            tv_softmax_xent at 4096 x 1000 and tv_probe_rows at 4096 x 32 x 16^2 with g = 16 and g = 4 (each with its host glue;
            TB/s on the algorithmic bytes of csrc/probe.hip's header);
            one training step at batch 4096, F = 8192, 1000 classes: LinearProbe + softmax_xent + FusedAdamW;
            beside it the eager form a user would write: F.linear + F.cross_entropy under bf16 autocast with torch.optim.AdamW.
2. `trace`: the two kernels under `rocprofv3 --kernel-trace --stats`, a run of its own -> profiles/probe_kernel_stats.csv; the
            kernel-time TB/s figures come from there.
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

B, NCLS, D, HW, FEAT = 4096, 1000, 32, 16, 8192
XENT_BYTES = 2 * B * NCLS * 2 + 8 * B


def rows_bytes(g):
    return 4 * B * D * HW * HW + 2 * B * g * g * D


def timed(fn, iters, warmup=3):
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


def cases():
    import torch
    import transvae
    from transvae import probe as P
    dev = torch.device("cuda:0")
    logits = torch.randn(B, NCLS, device=dev).bfloat16().requires_grad_(True)
    labels = torch.randint(0, NCLS, (B,), device=dev)
    lat = torch.randn(B, D, HW, HW, device=dev)
    mean, rstd = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    state = P.new_xent_state(dev)

    def xent():
        P.softmax_xent(logits, labels, NCLS, 0.1, state)

    def rows(g):
        return lambda: P._probe_rows(lat, mean, rstd, g, g)
    feats = torch.randn(B, FEAT, device=dev).bfloat16()
    probe = transvae.LinearProbe(FEAT, NCLS).to(dev)
    opt = transvae.optim.FusedAdamW(probe.parameters(), lr=1e-3, weight_decay=0.0)

    def hip_step():
        opt.zero_grad(set_to_none=True)
        P.softmax_xent(probe(feats), labels, NCLS, 0.1, state).backward()
        opt.step()
    lin = torch.nn.Linear(FEAT, NCLS).to(dev)
    eopt = torch.optim.AdamW(lin.parameters(), lr=1e-3, weight_decay=0.0)
    f32 = feats.float()

    def eager_step():
        eopt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = lin(f32)
        torch.nn.functional.cross_entropy(out.float(), labels, label_smoothing=0.1).backward()
        eopt.step()
    return xent, rows, hip_step, eager_step


def child_time(a):
    xent, rows, hip_step, eager_step = cases()
    ms = [timed(xent, a.iters) for _ in range(3)]
    print(json.dumps({"what": "tv_softmax_xent (with its host glue)", "case": f"{B} x {NCLS}, gradient on", "ms": [round(m, 4) for m in ms],
                      "algorithmic_bytes": XENT_BYTES, "tb_per_s_call": round(XENT_BYTES / min(ms) / 1e9, 3)}), flush=True)
    for g in (16, 4):
        ms = [timed(rows(g), a.iters) for _ in range(3)]
        print(json.dumps({"what": "tv_probe_rows (with its host glue)", "case": f"{B} x {D} x {HW}^2, g = {g}", "ms": [round(m, 4) for m in ms],
                          "algorithmic_bytes": rows_bytes(g), "tb_per_s_call": round(rows_bytes(g) / min(ms) / 1e9, 3)}), flush=True)
    mh = [timed(hip_step, a.iters) for _ in range(3)]
    me = [timed(eager_step, a.iters) for _ in range(3)]
    print(json.dumps({"what": "one training step", "case": f"batch {B}, F = {FEAT}, {NCLS} classes",
                      "hip_ms": [round(m, 4) for m in mh], "eager_bf16_autocast_adamw_ms": [round(m, 4) for m in me]}), flush=True)


def child_trace(a):
    import torch
    xent, rows, hip_step, _ = cases()
    for _ in range(5):
        xent()
        rows(16)()
        rows(4)()
    torch.cuda.synchronize()


def run_child(step, a, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--iters", str(a.iters)]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"probe_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "probe_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "time":
        return child_time(a)
    if a.child == "trace":
        return child_trace(a)
    rows = [json.loads(l) for l in run_child("time", a, 300).splitlines() if l.startswith("{")]
    for r in rows:
        print(r)
    report = {"rows": rows}
    if not a.no_trace:
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="probe_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 240, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "probe", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            with open(a.stats_out) as f:
                report["kernel_stats"] = [row for row in csv.DictReader(f) if "softmax_xent" in row.get("Name", "") or "probe_rows" in row.get("Name", "")]
            # kernel-time rates: the trace runs each case 5 times; probe_rows' two cases share a kernel name, so its figure is the
            # mean over both (the per-case figures are the device-event ones above)
            for row in report["kernel_stats"]:
                avg_ns = float(row.get("AverageNs") or row.get("Average") or 0)
                if "softmax_xent_kernel" in row["Name"] and avg_ns:
                    report["tv_softmax_xent_kernel_tb_per_s"] = round(XENT_BYTES / avg_ns / 1e3, 3)
                if "probe_rows_kernel" in row["Name"] and avg_ns:
                    report["tv_probe_rows_kernel_tb_per_s_mean_of_both_cases"] = round((rows_bytes(16) + rows_bytes(4)) / 2 / avg_ns / 1e3, 3)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
