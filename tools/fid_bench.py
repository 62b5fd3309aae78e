"""Cost of the rFID metric (transvae.metrics_fid, csrc/fid.hip).  GPU box.

    python tools/fid_bench.py [--batch 128] [--res 256] [--iters 10] [--out profiles/fid_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `time`:   the feature pass over 2B images (originals + reconstructions as one batch) at batch x 3 x res^2 and the
             `tv_fid_accumulate` step for the two sides, device events around warmed-up loops; every layer group on its own
             (stem, InceptionA x 3, B, C x 4, D, E x 2) -> TFLOP/s from 2 * kh * kw * Cin * Cout * output pixels; and
             evaluate()'s overhead with "rfid" over `model(images)` alone for the Large model at batch 64.
2. `trace`:  the feature pass and the accumulate step under `rocprofv3 --kernel-trace --stats`, a run of its own
             -> profiles/fid_kernel_stats.csv.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_net(dev):
    import fid_restatement as R      # seeded He-scaled weights: no trained Inception weights exist in this repository
    from transvae import InceptionFeatures
    return InceptionFeatures().load_fid_state_dict(R.plain_state_dict()).to(dev)


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


def group_flops():
    """{group: FLOP per image} from the layer table; a layer's output grid follows its block's input grid and its stride."""
    from transvae.metrics_fid import FID_LAYERS
    grid_in = {"Conv2d_1a": 299, "Conv2d_2a": 149, "Conv2d_2b": 147, "Conv2d_3b": 73, "Conv2d_4a": 73, "Mixed_5": 35, "Mixed_6a": 35,
               "Mixed_6": 17, "Mixed_7a": 17, "Mixed_7": 8}
    out = {}
    for name, c_in, c_out, kh, kw, stride, ph, pw in FID_LAYERS:
        key = next(k for k in sorted(grid_in, key=len, reverse=True) if name.startswith(k))
        g = grid_in[key]
        # inside a stride-2 block the 1x1 / padded layers keep the grid and only the stride-2 layer shrinks it
        go = (g + 2 * ph - kh) // stride + 1
        grp = "stem" if name.startswith("Conv2d") else name.split(".")[0]
        out[grp] = out.get(grp, 0) + 2.0 * kh * kw * c_in * c_out * go * ((g + 2 * pw - kw) // stride + 1)
    return out


def child_time(a):
    import torch
    from transvae import FrechetDistance, evaluate
    dev = torch.device("cuda:0")
    net = make_net(dev)
    torch.manual_seed(0)
    x = torch.rand(a.batch, 3, a.res, a.res, device=dev)
    r = (x + 0.05 * torch.randn_like(x)).clamp(0, 1)
    ms = [timed(lambda: net.features(x, r, clip=True), a.iters) for _ in range(3)]
    fl = group_flops()
    total = sum(fl.values()) * 2 * a.batch
    print(json.dumps({"what": "fid features, 2B images", "batch": a.batch, "res": a.res, "ms": [round(m, 3) for m in ms],
                      "TFLOPs": round(total / min(ms) / 1e9, 1)}), flush=True)
    f = net.features(x, r, clip=True)
    fd = FrechetDistance()
    m_acc = timed(lambda: fd.update(f[:a.batch], f[a.batch:]), a.iters)
    print(json.dumps({"what": "fid accumulate, both sides", "rows_per_side": a.batch, "ms": round(m_acc, 3),
                      "fp64_TFLOPs": round(2 * 3.0 * a.batch * 2048 * 2048 / m_acc / 1e9, 2)}), flush=True)
    # layer groups on their own, 2B images
    B2 = 2 * a.batch

    def act(g, c):
        return torch.relu(torch.randn(B2, g, g, c, device=dev)).to(torch.bfloat16)
    from transvae.hip import _lib as L
    groups = [("Mixed_5b", lambda h: net._inception_a(h, "Mixed_5b", 32), 35, 192), ("Mixed_5c", lambda h: net._inception_a(h, "Mixed_5c", 64), 35, 256),
              ("Mixed_5d", lambda h: net._inception_a(h, "Mixed_5d", 64), 35, 288), ("Mixed_6a", lambda h: net._inception_b(h, "Mixed_6a"), 35, 288)]
    groups += [(b, (lambda h, b=b: net._inception_c(h, b)), 17, 768) for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e")]
    groups += [("Mixed_7a", lambda h: net._inception_d(h, "Mixed_7a"), 17, 768), ("Mixed_7b", lambda h: net._inception_e(h, "Mixed_7b", L.POOL3_AVG_S1P1), 8, 1280),
               ("Mixed_7c", lambda h: net._inception_e(h, "Mixed_7c", L.POOL3_MAX_S1P1), 8, 2048)]
    with torch.no_grad():
        for name, fn, g, c in groups:
            h = act(g, c)
            m = timed(lambda: fn(h), a.iters)
            print(json.dumps({"what": "group", "group": name, "grid": g, "c_in": c, "ms": round(m, 4),
                              "TFLOPs": round(fl[name] * B2 / m / 1e9, 1)}), flush=True)
            del h
    # evaluate() with and without "rfid", Large at batch 64
    if a.model:
        from transvae import create_transvae
        model = create_transvae(a.model).to(dev)
        xb = torch.rand(64, 3, a.res, a.res, device=dev)
        with torch.no_grad():
            model.eval()
            m_model = timed(lambda: model(xb), 5)
        m_plain = timed(lambda: evaluate(model, [(xb, None)], metrics=("psnr",), device=dev), 5)
        m_rfid = timed(lambda: evaluate(model, [(xb, None)], metrics=("psnr", "rfid"), device=dev, fid_net=net), 5)
        print(json.dumps({"what": "evaluate overhead", "model": a.model, "batch": 64, "model_ms": round(m_model, 2), "evaluate_psnr_ms": round(m_plain, 2),
                          "evaluate_psnr_rfid_ms": round(m_rfid, 2), "note": "the rfid run includes compute(): two 2048^2 eigh on the host, once per evaluate()"}),
              flush=True)


def child_trace(a):
    import torch
    from transvae import FrechetDistance
    dev = torch.device("cuda:0")
    net = make_net(dev)
    torch.manual_seed(0)
    x = torch.rand(a.batch, 3, a.res, a.res, device=dev)
    fd = FrechetDistance()
    for _ in range(3):
        f = net.features(x, x, clip=True)
        fd.update(f[:a.batch], f[a.batch:])
    torch.cuda.synchronize()


def run_child(step, a, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--batch", str(a.batch), "--res", str(a.res),
                          "--iters", str(a.iters), "--model", a.model]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"fid_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--model", default="large", help="variant for the evaluate() overhead ('' skips it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "fid_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "time":
        return child_time(a)
    if a.child == "trace":
        return child_trace(a)
    rows = [json.loads(l) for l in run_child("time", a, 420).splitlines() if l.startswith("{")]
    for r in rows:
        print(r)
    report = {"batch": a.batch, "res": a.res, "rows": rows}
    if not a.no_trace:
        import tempfile
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="fid_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 300, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "fid", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            dst = a.stats_out
            with open(stats[-1]) as f, open(dst, "w") as g:
                g.write(f.read())
            with open(dst) as f:
                report["kernel_stats_top"] = [row for _, row in zip(range(12), csv.DictReader(f))]
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
