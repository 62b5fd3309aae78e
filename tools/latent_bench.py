"""Cost of latent extraction and of the latent-space density metrics (transvae.latents, csrc/latent.hip).  GPU box.

    python tools/latent_bench.py [--points 65536] [--iters 5] [--out profiles/latent_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `time`:  device events around warmed-up loops, three windows each:
            tv_kde_logdensity at N = M = `points` for d = 2 and d = 32 (leave-one-out, Scott bandwidth), pairs per second;
            beside it the eager formulation on the same device: `torch.cdist` + `logsumexp` over query chunks of 4096;
            tv_latent_stats at 256 x 32 x 16^2, and the eager fp64 `mean` + centred `matmul` of the same tensor;
            `extract_latents` over 8 batches of 16 x 3 x 256^2 on the micro model against `model.encode` alone on the same batches
            (flip off, so both encode the same images; the difference is the statistics, the host copies and the shard writes).
2. `trace`: the two kernels under `rocprofv3 --kernel-trace --stats`, a run of its own -> profiles/latent_kernel_stats.csv.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))


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


def eager_logdensity(x, h, chunk=4096):
    """what a user would otherwise write: chunked cdist + logsumexp, the self term masked"""
    import torch
    out = []
    for i0 in range(0, x.shape[0], chunk):
        s = torch.cdist(x[i0:i0 + chunk], x).square_().mul_(-1.0 / (2.0 * h * h))
        idx = torch.arange(i0, min(i0 + chunk, x.shape[0]), device=x.device)
        s[idx - i0, idx] = float("-inf")
        out.append(torch.logsumexp(s, dim=1))
    return torch.cat(out)


def child_time(a):
    import torch
    import transvae
    from transvae import latents as T
    dev = torch.device("cuda:0")
    n = a.points
    for d in (2, 32):
        x = torch.randn(n, d, device=dev)
        h = float(n) ** (-1.0 / (d + 4))
        ms = [timed(lambda: T.kde_logdensity(x, None, h, exclude_self=True), a.iters) for _ in range(3)]
        me = [timed(lambda: eager_logdensity(x, h), a.iters) for _ in range(3)]
        dev_max = float((T.kde_logdensity(x, None, h, exclude_self=True) - eager_logdensity(x, h)).abs().max())
        print(json.dumps({"what": "tv_kde_logdensity", "case": f"N = M = {n}, d = {d}, leave-one-out", "ms": [round(m, 3) for m in ms],
                          "gpairs_per_s": round(n * n / min(ms) / 1e6, 1), "eager_cdist_logsumexp_ms": [round(m, 3) for m in me],
                          "max_abs_difference_from_eager": dev_max}), flush=True)
    lat = torch.randn(256, 32, 16, 16, device=dev)

    def stats():
        st = transvae.LatentStats(32)
        st.update(lat)
        return st

    def eager_stats():
        r = lat.double().permute(0, 2, 3, 1).reshape(-1, 32)
        c = r - r.mean(0)
        return c.T @ c / r.shape[0]
    ms = [timed(stats, 20) for _ in range(3)]
    me = [timed(eager_stats, 20) for _ in range(3)]
    print(json.dumps({"what": "tv_latent_stats (with its host glue)", "case": "256 x 32 x 16^2", "ms": [round(m, 4) for m in ms],
                      "eager_fp64_ms": [round(m, 4) for m in me]}), flush=True)

    from oracle import filler
    from oracle import transvae_oracle as O
    cfg = dict(O.MICRO)
    model = transvae.TransVAE(config=cfg, variant="micro", compression_ratio=16, latent_dim=4)
    model.load_state_dict(filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4)))
    model = model.to(dev).eval()
    batches = [torch.rand(16, 3, 256, 256, device=dev) for _ in range(8)]

    def encode_only():
        with torch.no_grad():
            for b in batches:
                model.encode(b)
        torch.cuda.synchronize()

    def wall(fn, reps=3):
        fn()
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t0)
        return best * 1e3
    with tempfile.TemporaryDirectory() as tmp:
        t_enc = wall(encode_only)
        t_ext = wall(lambda: transvae.extract_latents(model, batches, tmp, flip=False, device=dev))
    print(json.dumps({"what": "extract_latents over model.encode alone", "case": "micro model, 8 x 16 x 3 x 256^2, flip off, wall clock",
                      "encode_ms": round(t_enc, 2), "extract_ms": round(t_ext, 2), "overhead_percent": round(100 * (t_ext / t_enc - 1), 1)}),
          flush=True)


def child_trace(a):
    import torch
    import transvae
    from transvae import latents as T
    dev = torch.device("cuda:0")
    for d in (2, 32):
        x = torch.randn(a.points, d, device=dev)
        for _ in range(3):
            T.kde_logdensity(x, None, float(a.points) ** (-1.0 / (d + 4)), exclude_self=True)
    lat = torch.randn(256, 32, 16, 16, device=dev)
    for _ in range(5):
        transvae.LatentStats(32).update(lat)
    torch.cuda.synchronize()


def run_child(step, a, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--points", str(a.points), "--iters", str(a.iters)]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"latent_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "latent_kernel_stats.csv"))
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
    report = {"points": a.points, "rows": rows}
    if not a.no_trace:
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="latent_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 240, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "latent", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            with open(a.stats_out) as f:
                report["kernel_stats"] = [row for row in csv.DictReader(f) if "kde_" in row.get("Name", "") or "latent_" in row.get("Name", "")]
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
