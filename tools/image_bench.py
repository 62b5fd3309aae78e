"""Cost of the image pipeline (transvae.image_io, csrc/image.hip).  GPU box.

    python tools/image_bench.py [--batch 128] [--iters 20] [--out profiles/image_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `time`:  device events around warmed-up loops, three windows each:
            tv_image_prep for `batch` images of 500x375 -> 256^2 and -> 512^2 (resize + crop + ToTensor, one launch), and for
            already-256^2 sources (no resample: the copy path of the same launch); effective bytes/s = (source bytes of the
            rows and columns that exist + fp32 bytes written) / time.  tv_image_grid_u8 for 64 x 3 x 256^2.
            PIL's per-image time for the same 500x375 -> 256 transform on ONE host core of the same box, when PIL is importable.
2. `trace`: the same calls under `rocprofv3 --kernel-trace --stats`, a run of its own -> profiles/image_kernel_stats.csv.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))


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


def make_batches(a, dev):
    import numpy as np
    from transvae.image_io import pack_uint8
    rng = np.random.default_rng(0)
    ragged = [rng.integers(0, 256, (375, 500, 3) if i % 2 else (500, 375, 3), dtype=np.uint8) for i in range(a.batch)]
    square = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(a.batch)]
    return ragged, pack_uint8(ragged).to(dev), pack_uint8(square).to(dev)


def child_time(a):
    import numpy as np
    import torch
    from transvae.image_io import ImagePrep, to_uint8_grid
    dev = torch.device("cuda:0")
    ragged_host, ragged, square = make_batches(a, dev)
    for name, batch, res in (("500x375 -> 256^2", ragged, 256), ("500x375 -> 512^2", ragged, 512), ("256^2 -> 256^2 (copy path)", square, 256)):
        prep = ImagePrep(res)
        prep(batch)
        ms = [timed(lambda: prep(batch), a.iters) for _ in range(3)]
        nbytes = batch.data.numel() + a.batch * 3 * res * res * 4
        print(json.dumps({"what": "tv_image_prep (with its host glue)", "case": name, "batch": a.batch, "ms": [round(m, 4) for m in ms],
                          "bytes_read_plus_written": nbytes, "effective_GBps": round(nbytes / min(ms) / 1e6, 1)}), flush=True)
    x = torch.randn(64, 3, 256, 256, device=dev)
    for tr in ("none", "sigmoid"):
        ms = [timed(lambda: to_uint8_grid(x, nrow=8, padding=2, transform=tr), a.iters) for _ in range(3)]
        g = to_uint8_grid(x, nrow=8, padding=2, transform=tr)
        nbytes = x.numel() * 4 + g.numel()
        print(json.dumps({"what": "tv_image_grid_u8", "case": f"64x3x256^2, {tr}", "ms": [round(m, 4) for m in ms],
                          "bytes_read_plus_written": nbytes, "effective_GBps": round(nbytes / min(ms) / 1e6, 1)}), flush=True)
    try:
        from PIL import Image
    except ImportError:
        print(json.dumps({"what": "PIL on one host core", "note": "PIL not importable on this box: not measured"}), flush=True)
        return
    torch.set_num_threads(1)
    n = min(32, a.batch)
    t0 = time.perf_counter()
    for im in ragged_host[:n]:
        h, w = im.shape[:2]
        oh, ow = (int(256 * h / w), 256) if w <= h else (256, int(256 * w / h))
        r = np.asarray(Image.fromarray(im, "RGB").resize((ow, oh), Image.BILINEAR))
        top, left = int(round((oh - 256) / 2.0)), int(round((ow - 256) / 2.0))
        torch.from_numpy(np.ascontiguousarray(r[top:top + 256, left:left + 256])).permute(2, 0, 1).float().div(255)
    print(json.dumps({"what": "PIL on one host core", "case": "500x375 -> 256^2, resize + crop + ToTensor", "images": n,
                      "ms_per_image": round((time.perf_counter() - t0) / n * 1e3, 3)}), flush=True)


def child_trace(a):
    import torch
    from transvae.image_io import ImagePrep, to_uint8_grid
    dev = torch.device("cuda:0")
    _, ragged, square = make_batches(a, dev)
    x = torch.randn(64, 3, 256, 256, device=dev)
    p256, p512 = ImagePrep(256), ImagePrep(512)
    for _ in range(5):
        p256(ragged)
        p512(ragged)
        p256(square)
        to_uint8_grid(x, nrow=8, padding=2)
    torch.cuda.synchronize()


def run_child(step, a, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--batch", str(a.batch), "--iters", str(a.iters)]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"image_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "image_kernel_stats.csv"))
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
    report = {"batch": a.batch, "rows": rows}
    if not a.no_trace:
        import tempfile
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="image_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 240, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "image", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            with open(a.stats_out) as f:
                report["kernel_stats"] = [row for row in csv.DictReader(f) if "image_" in row.get("Name", "")]
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
