"""Cost of the sampler's recipe options (transvae.dit.sample_latents: method / timestep_shift / cfg_interval) and of the two kernels
behind the recipe (tv_flow_loss_cos, tv_flow_heun).  GPU box.

    python tools/sampler_bench.py [--parent DIR] [--reps 2] [--out profiles/sampler_bench.json]

DiT-B at patch size 1 on 32 x 16 x 16 latents, 64 images, cfg_scale = 1.5, random weights, device events.  Every GPU step runs in a
fresh child process under its own `timeout`; a step that fails ends the run.
1. `recipe`:  three windows that alternate between the cases, `reps` calls per window:
                50 Euler steps with the default arguments;
                the same with cfg_interval = (0.125, 1.0) and timestep_shift = 0.3, beside the count of B-row and 2B-row evaluations;
                25 Heun steps (50 evaluations, as the first case);
              then the two kernels alone at the shape of dit_bench.py (256 x 32 x 16 x 16 latents), three windows each, with
              tv_flow_loss and tv_flow_euler beside them.
2. `default`: the default 50-step call alone, one window per process, alternating three times between `--parent DIR` (a built
              checkout of the parent commit) and this tree, the order within a pair swapped from one pair to the next: whether the default call got slower is read against the spread between
              the windows.  Without --parent the file says "not measured".
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HW, P, IMAGES, CFG = 32, 16, 1, 64, 1.5
KB, KT, LD = 256, 256 * 256, 32
LAT = KB * D * HW * HW
CASES = {"euler50_default": dict(steps=50),
         "euler50_interval_shift": dict(steps=50, cfg_interval=(0.125, 1.0), timestep_shift=0.3),
         "heun25": dict(steps=25, method="heun")}
BYTES = {"tv_flow_loss": 8 * LAT + 4 * KT * LD, "tv_flow_loss_cos": 8 * LAT + 4 * KT * LD, "tv_flow_euler": 8 * LAT + 4 * KT * LD,
         "tv_flow_heun": 8 * LAT + 8 * KT * LD}


def use_tree(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "deepl-project_amd"))


def timed(fn, iters, warmup=0):
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


def sampler(kw):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    m = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev).eval()
    labels = torch.randint(0, 1000, (IMAGES,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    gen = torch.Generator(device=dev).manual_seed(0)
    return lambda: transvae.sample_latents(m, labels, cfg_scale=CFG, generator=gen, stats=stats, **kw)


def evaluation_counts(kw):
    from transvae import dit
    grid = dit.time_grid(kw["steps"], kw.get("timestep_shift", 1.0))
    lo, hi = kw.get("cfg_interval", (0.0, 1.0))
    times = []
    for i in range(kw["steps"]):
        times += [grid[i]] + ([grid[i + 1]] if kw.get("method") == "heun" else [])
    two = sum(1 for t in times if lo <= t <= hi)
    return {"B_rows": len(times) - two, "2B_rows": two}


def child_recipe(a):
    import torch
    from transvae import dit
    use = {k: sampler(kw) for k, kw in CASES.items()}
    for fn in use.values():
        fn()                                                         # warm every case before the first window
    ms = {k: [] for k in use}
    for _ in range(3):
        for k, fn in use.items():
            ms[k].append(timed(fn, a.reps))
    for k, kw in CASES.items():
        print(json.dumps({"what": k, "arguments": {kk: vv for kk, vv in kw.items()}, "ms": [round(x, 2) for x in ms[k]],
                          "evaluations": evaluation_counts(kw)}), flush=True)
    dev = torch.device("cuda:0")
    lat, noise = torch.randn(KB, D, HW, HW, device=dev), torch.randn(KB, D, HW, HW, device=dev)
    mean, rstd = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    pred = torch.randn(KT, LD, device=dev).bfloat16()
    v1, v2 = torch.randn(2 * KT, LD, device=dev).bfloat16(), torch.randn(2 * KT, LD, device=dev).bfloat16()
    xs = noise.clone()
    kernels = {"tv_flow_loss": lambda: dit.flow_loss(pred, lat, mean, rstd, noise, P),
               "tv_flow_loss_cos": lambda: dit.flow_loss_cos(pred, lat, mean, rstd, noise, P, 1.0),
               "tv_flow_euler": lambda: dit.flow_euler(xs, v1, P, 0.02, CFG),
               "tv_flow_heun": lambda: dit.flow_heun(xs, v1, v2, P, 0.02, CFG, True, True)}
    for name, fn in kernels.items():
        w = [timed(fn, 2000, warmup=10) for _ in range(3)]          # (windows of 20-50 ms: the calls are 10-25 us each)
        print(json.dumps({"what": name + " (with its host glue)", "case": f"{KB} x {D} x {HW}^2, p = {P}, guided", "ms": [round(x, 4) for x in w],
                          "algorithmic_bytes": BYTES[name], "tb_per_s_call": round(BYTES[name] / min(w) / 1e9, 3)}), flush=True)


def child_default(a):
    fn = sampler(CASES["euler50_default"])
    print(json.dumps({"ms": round(timed(fn, a.reps, warmup=1), 2)}), flush=True)


def run_child(step, a, root, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--root", root, "--reps", str(a.reps)]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=root)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"sampler_bench: step '{step}' in {root} failed with status {r.returncode}; stopping")
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def spread(ms):
    return round(max(ms) / min(ms) - 1.0, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit; empty: the comparison is not measured")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        use_tree(os.path.abspath(a.root))
        return {"recipe": child_recipe, "default": child_default}[a.child](a)
    rows = run_child("recipe", a, ROOT, 420)
    by = {r["what"]: r for r in rows}
    base = min(by["euler50_default"]["ms"])
    for k in ("euler50_interval_shift", "heun25"):
        by[k]["saving_vs_default"] = round(1.0 - min(by[k]["ms"]) / base, 4)
    report = {"setup": f"DiT-B, {IMAGES} images, {D} x {HW}^2 latents, p = {P}, cfg_scale = {CFG}, device events, ms per call", "rows": rows}
    if a.parent:
        parent, here = [], []
        for r in range(3):                                           # parent, here | here, parent | parent, here
            for tree, ms in ((os.path.abspath(a.parent), parent), (ROOT, here))[::1 if r % 2 == 0 else -1]:
                ms.append(run_child("default", a, tree, 240)[0]["ms"])
        report["default_call_vs_parent"] = {"parent_ms": parent, "this_tree_ms": here, "parent_window_spread": spread(parent),
                                            "this_tree_window_spread": spread(here),
                                            "this_tree_over_parent": round(sorted(here)[1] / sorted(parent)[1], 4)}
    else:
        report["default_call_vs_parent"] = "not measured"
    for r in rows:
        print(r)
    print(report["default_call_vs_parent"])
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
