"""Cost of the generator evaluation (transvae.evaluate_dit, transvae.metrics_gen, csrc/genmetrics.hip, tv_opt_ema).  GPU box.

    python tools/gen_eval_bench.py [--points 10000,50000] [--samples 1024] [--steps 50] [--parent DIR] [--out profiles/gen_eval_bench.json]

Every GPU step runs in a fresh child process under its own `timeout`; a step that fails ends the run.
1. `pairwise`: device events around tv_knn_radius (through `knn_radius`, launches of 8192 queries) and tv_manifold_hits at N = M = each of
               `points`, d = 2048, k = 3; beside them, in the same run, the eager form a user would write: `torch.cdist` +
               `kthvalue` / a comparison against the radii, over query chunks of 4096.
2. `small`:    tv_softmax_stats at 256 x 1008; tv_opt_ema over DiT-B's parameters beside `torch._foreach_lerp_`; one DiT-B training
               step (256 x 32 x 16^2 latents, patch 1, `flow_matching_loss` + `FusedAdamW`) with and without the EMA update.
3. `evaluate`: `evaluate_dit` at `samples` images (DiT-B, `steps` Euler steps at cfg_scale 1.5, TransVAE-large f16d32 decode, batch 128,
               all four metrics against a reference of as many random-image features), and its three parts timed on their own:
               sampling, features, metrics.
4. `suite`:    the rest of the suite, device events in alternating windows: tv_poly_kernel_sums at 100 subsets x 1000 rows x 2048
               beside the eager fp32 `(X @ Y.T / d + 1) ** 3` summed per subset; tv_ball_counts at 10 000 x 10 000 x 2048 beside
               tv_manifold_hits; tv_spatial_rows at 256 images; `evaluate_dit` at `samples` images with ALL_METRICS beside the
               default list.
5. `default`:  the default `evaluate_dit` call alone, one window per process, alternating three times between `--parent DIR` (a
               built checkout of the parent commit) and this tree, the order within a pair swapped from one pair to the next:
               whether the default call got slower is read against the spread between a tree's own windows.  Without --parent
               the file says "not measured".
6. `trace`:    the kernels under `rocprofv3 --kernel-trace --stats`, a run of its own -> profiles/gen_eval_kernel_stats.csv.
A run of some steps (`--only`) keeps the rows of the others in the output file.
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

D_FEAT, K_NN = 2048, 3
B, D, HW, P = 256, 32, 16, 1


def timed(fn, iters, warmup=1):
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


def features_like(n, seed, dev):
    """non-negative rows of low intrinsic dimension, like pool3 features"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    A = torch.randn(8, D_FEAT, generator=g, device=dev)
    z = torch.randn(n, 8, generator=g, device=dev) @ A / 8 ** 0.5 + 0.1 * torch.randn(n, D_FEAT, generator=g, device=dev) + 0.5
    return z.clamp_min_(0).contiguous()


def eager_radius(x, k, chunk=4096):
    import torch
    out = []
    for i0 in range(0, x.shape[0], chunk):
        dist = torch.cdist(x[i0:i0 + chunk], x)
        idx = torch.arange(i0, min(i0 + chunk, x.shape[0]), device=x.device)
        dist[idx - i0, idx] = float("inf")
        out.append(torch.kthvalue(dist, k, dim=1).values.square_())
    return torch.cat(out)


def eager_hits(q, x, r2, chunk=4096):
    import torch
    r = r2.sqrt()
    return torch.cat([(torch.cdist(q[i0:i0 + chunk], x) <= r).any(1) for i0 in range(0, q.shape[0], chunk)]).int()


def child_pairwise(a):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    for n in [int(v) for v in a.points.split(",")]:
        x, q = features_like(n, 0, dev), features_like(n, 1, dev)
        iters = 2 if n <= 20000 else 1
        r2 = transvae.knn_radius(x, K_NN)
        ms = [timed(lambda: transvae.knn_radius(x, K_NN), iters, warmup=0) for _ in range(2)]
        me = [timed(lambda: eager_radius(x, K_NN), iters) for _ in range(2)]
        rel = float(((eager_radius(x, K_NN) - r2).abs() / r2).max())
        print(json.dumps({"what": "tv_knn_radius", "case": f"N = M = {n}, d = {D_FEAT}, k = {K_NN}", "ms": [round(m, 2) for m in ms],
                          "tflops_3NMd": round(3.0 * n * n * D_FEAT / min(ms) / 1e9, 2), "eager_cdist_kthvalue_ms": [round(m, 2) for m in me],
                          "max_relative_difference_from_eager": rel}), flush=True)
        ms = [timed(lambda: transvae.manifold_hits(q, x, r2), iters, warmup=0) for _ in range(2)]
        me = [timed(lambda: eager_hits(q, x, r2), iters) for _ in range(2)]
        differ = int((eager_hits(q, x, r2) != transvae.manifold_hits(q, x, r2)).sum())
        print(json.dumps({"what": "tv_manifold_hits", "case": f"N = M = {n}, d = {D_FEAT}", "ms": [round(m, 2) for m in ms],
                          "tflops_3NMd": round(3.0 * n * n * D_FEAT / min(ms) / 1e9, 2), "eager_cdist_compare_ms": [round(m, 2) for m in me],
                          "queries_decided_differently_by_eager": differ}), flush=True)
        del x, q


def dit_step():
    import torch
    import transvae
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(B, D, HW, HW, device=dev)
    labels = torch.randint(0, 1000, (B,), device=dev)
    stats = (torch.zeros(D), torch.ones(D))
    m = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev).train()
    opt = transvae.optim.FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.0)
    ema = transvae.ParamEMA(m.parameters(), decay=0.9999, optimizer=opt)

    def step(with_ema):
        opt.zero_grad(set_to_none=True)
        transvae.flow_matching_loss(m, lat, labels, stats, generator=gen, check_labels=False)
        opt.step()
        if with_ema:
            ema.update()
    return m, ema, step


def child_small(a):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    head = transvae.InceptionScore(torch.randn(1008, D_FEAT) * 0.02).to(dev)
    f = features_like(256, 2, dev)
    ms = [timed(lambda: head.update(f), 20, warmup=3) for _ in range(3)]
    logits = torch.addmm(head.bias, f, head.weight.t())
    mm = [timed(lambda: torch.addmm(head.bias, f, head.weight.t()), 20, warmup=3) for _ in range(3)]
    me = [timed(lambda: (torch.softmax(logits.double(), 1) * torch.log_softmax(logits.double(), 1)).sum(), 20, warmup=3) for _ in range(3)]
    print(json.dumps({"what": "InceptionScore.update (addmm + tv_softmax_stats)", "case": "256 x 1008", "ms": [round(m, 4) for m in ms],
                      "addmm_alone_ms": [round(m, 4) for m in mm], "eager_fp64_softmax_terms_ms": [round(m, 4) for m in me]}), flush=True)
    m, ema, step = dit_step()
    n_par = sum(p.numel() for p in m.parameters())
    ps, sh = list(m.parameters()), [e.clone() for e in ema.shadow]
    ms = [timed(ema.update, 20, warmup=3) for _ in range(3)]
    with torch.no_grad():
        me = [timed(lambda: torch._foreach_lerp_(sh, ps, 1e-4), 20, warmup=3) for _ in range(3)]
    print(json.dumps({"what": "tv_opt_ema (ParamEMA.update)", "case": f"DiT-B, {n_par} parameters in {len(ps)} tensors", "ms": [round(v, 4) for v in ms],
                      "algorithmic_bytes": 12 * n_par, "tb_per_s": round(12 * n_par / min(ms) / 1e9, 2),
                      "foreach_lerp_ms": [round(v, 4) for v in me]}), flush=True)
    rows = {}
    for rep in range(2):                                      # interleaved, in the same process
        for with_ema in (False, True):
            rows.setdefault(with_ema, []).append(timed(lambda: step(with_ema), a.iters, warmup=2))
    print(json.dumps({"what": "one DiT-B training step without / with the EMA update", "case": f"{B} x {D} x {HW}^2, p = {P}",
                      "without_ms": [round(v, 3) for v in rows[False]], "with_ms": [round(v, 3) for v in rows[True]],
                      "difference_ms": round(min(rows[True]) - min(rows[False]), 3)}), flush=True)


def child_evaluate(a):
    import torch
    import fid_restatement as R
    import transvae
    dev = torch.device("cuda:0")
    n, bs = a.samples, 128
    dit = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev).eval()
    with torch.no_grad():
        for p in dit.parameters():                            # adaLN-Zero leaves the output at zero: any weights do for timing
            if not bool(p.any()):
                p.normal_(0, 0.02)
    vae = transvae.create_transvae("large", 16, 32).to(dev).eval()
    net = transvae.InceptionFeatures().load_fid_state_dict(R.plain_state_dict()).to(dev)
    head = transvae.InceptionScore(torch.randn(1008, D_FEAT) * 0.02).to(dev)
    real = [(torch.rand(bs, 3, 256, 256, device=dev), None) for _ in range(max(1, n // bs))]
    ref = transvae.reference_statistics(real, net, is_head=head)
    kw = dict(fid_net=net, num_samples=n, batch_size=bs, steps=a.steps, cfg_scale=1.5, is_head=head)
    transvae.evaluate_dit(vae, dit, ref, **dict(kw, num_samples=bs, steps=1, metrics=("gfid", "is")))          # warm-up
    whole = timed(lambda: transvae.evaluate_dit(vae, dit, ref, **kw), 1, warmup=0)
    labels = torch.arange(n, device=dev) % 1000
    gen = torch.Generator(device=dev).manual_seed(0)
    stats = (torch.zeros(D), torch.ones(D))
    imgs = []

    def sampling():
        imgs.clear()
        for i0 in range(0, n, bs):
            imgs.append(transvae.sample_images(vae, dit, labels[i0:i0 + bs], steps=a.steps, cfg_scale=1.5, generator=gen, stats=stats).float())
    t_sample = timed(sampling, 1, warmup=0)
    feats = []

    def features():
        feats.clear()
        for im in imgs:
            feats.append(net.features(im, clip=True))
    t_feat = timed(features, 1, warmup=0)
    fake, real_f = torch.cat(feats), ref["features"].to(dev)

    def metrics():
        fd = transvae.FrechetDistance()
        head.reset()
        for f in feats:
            fd.update(None, f)
            head.update(f)
        transvae.precision_recall(real_f, fake, K_NN)
        _, mu, cov = fd.statistics(1)
        transvae.metrics_fid.frechet_from_statistics(ref["mean"].numpy(), ref["cov"].numpy(), mu, cov)
        head.compute()
    t_metrics = timed(metrics, 1, warmup=0)
    print(json.dumps({"what": "evaluate_dit, all four metrics", "case": f"{n} samples, batch {bs}, DiT-B, {a.steps} Euler steps at cfg_scale 1.5, "
                      "TransVAE-large f16d32 decode to 256^2", "whole_ms": round(whole, 1), "sampling_ms": round(t_sample, 1),
                      "features_ms": round(t_feat, 1), "metrics_ms (host eigh of two 2048^2 matrices included)": round(t_metrics, 1)}), flush=True)


def eval_setup(a, spatial):
    """(vae, dit, reference, keywords) of the evaluate_dit timing: DiT-B, TransVAE-large f16d32, random-image reference"""
    import torch
    import fid_restatement as R
    import transvae
    dev = torch.device("cuda:0")
    n, bs = a.samples, 128
    dit = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev).eval()
    with torch.no_grad():
        for p in dit.parameters():                            # adaLN-Zero leaves the output at zero: any weights do for timing
            if not bool(p.any()):
                p.normal_(0, 0.02)
    vae = transvae.create_transvae("large", 16, 32).to(dev).eval()
    net = transvae.InceptionFeatures().load_fid_state_dict(R.plain_state_dict()).to(dev)
    head = transvae.InceptionScore(torch.randn(1008, D_FEAT) * 0.02).to(dev)
    real = [(torch.rand(bs, 3, 256, 256, device=dev), None) for _ in range(max(1, n // bs))]
    ref = transvae.reference_statistics(real, net, is_head=head, **({"spatial": True} if spatial else {}))
    return vae, dit, ref, dict(fid_net=net, num_samples=n, batch_size=bs, steps=a.steps, cfg_scale=1.5, is_head=head)


def child_suite(a):
    import torch
    import transvae
    from transvae.evaluate_dit import ALL_METRICS
    from transvae.metrics_fid import SPATIAL_CHANNELS, SPATIAL_LD, spatial_rows
    dev = torch.device("cuda:0")
    # KID sums: 100 subsets of 1000 rows out of 10 000 a side
    x, y = features_like(10000, 0, dev), features_like(10000, 1, dev)
    ia, ib, m = transvae.kid_subsets(10000, 10000, 100, 1000, 0)
    ia, ib = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
    gamma = 1.0 / D_FEAT

    def eager():
        return torch.stack([((x[ia[s].long()] @ y[ib[s].long()].T) * gamma + 1.0).pow(3).sum() for s in range(ia.shape[0])])
    ours = transvae.poly_kernel_sums(x, ia, y, ib, gamma, 1.0, False)
    rel = float(((eager().double() - ours).abs() / ours).max())
    same = bool(torch.equal(transvae.poly_kernel_sums(x, ia, y, ib, gamma, 1.0, False), ours))
    ms, me = [], []
    for _ in range(3):                                        # alternating windows
        ms.append(timed(lambda: transvae.poly_kernel_sums(x, ia, y, ib, gamma, 1.0, False), 3))
        me.append(timed(eager, 3))
    print(json.dumps({"what": "tv_poly_kernel_sums", "case": f"100 subsets x {m} x {m} pairs, d = {D_FEAT}", "ms": [round(v, 2) for v in ms],
                      "tflops_2Sm2d": round(2.0 * 100 * m * m * D_FEAT / min(ms) / 1e9, 2), "eager_fp32_gram_cubed_ms": [round(v, 2) for v in me],
                      "max_relative_difference_from_eager": rel, "two_runs_same_bits": same,
                      "buys": "one fixed summation order in fp64 (the same bits on every run) and no gathered rows or m x m buffer"}), flush=True)
    # ball counts beside manifold hits
    r2 = transvae.knn_radius(x, 5)
    mc, mh = [], []
    for _ in range(3):
        mc.append(timed(lambda: transvae.ball_counts(y, x, r2, "data"), 2))
        mh.append(timed(lambda: transvae.manifold_hits(y, x, r2), 2))
    mq = [timed(lambda: transvae.ball_counts(x, y, r2, "query"), 2) for _ in range(2)]
    agree = bool(torch.equal((transvae.ball_counts(y, x, r2, "data") > 0).int(), transvae.manifold_hits(y, x, r2)))
    print(json.dumps({"what": "tv_ball_counts", "case": f"N = M = 10000, d = {D_FEAT}", "radius_per_data_ms": [round(v, 2) for v in mc],
                      "radius_per_query_ms": [round(v, 2) for v in mq], "tv_manifold_hits_ms": [round(v, 2) for v in mh],
                      "tflops_3NMd": round(3.0 * 1e8 * D_FEAT / min(mc) / 1e9, 2), "count_positive_equals_hits": agree}), flush=True)
    del x, y
    act = torch.randn(256, 17, 17, 768, device=dev).bfloat16()
    w = [timed(lambda: spatial_rows(act, 0, SPATIAL_CHANNELS, SPATIAL_LD), 200, warmup=10) for _ in range(3)]
    print(json.dumps({"what": "tv_spatial_rows (with its host glue)", "case": "256 images, 17 x 17 x 768 -> 2048 columns",
                      "ms": [round(v, 4) for v in w], "bytes_written": 256 * SPATIAL_LD * 4}), flush=True)
    del act
    vae, dit, ref, kw = eval_setup(a, True)
    transvae.evaluate_dit(vae, dit, ref, **dict(kw, num_samples=128, steps=1, metrics=ALL_METRICS))          # warm-up
    rows = {False: [], True: []}
    for r in range(2):
        for full in (False, True)[::1 if r % 2 == 0 else -1]:
            rows[full].append(timed(lambda: transvae.evaluate_dit(vae, dit, ref, **dict(kw, **({"metrics": ALL_METRICS} if full else {}))), 1))
    print(json.dumps({"what": "evaluate_dit, ALL_METRICS beside the default list", "case": f"{a.samples} samples, batch 128, DiT-B, {a.steps} Euler steps "
                      "at cfg_scale 1.5, TransVAE-large f16d32 decode to 256^2; KID 100 x 1000",
                      "default_ms": [round(v, 1) for v in rows[False]], "all_metrics_ms": [round(v, 1) for v in rows[True]],
                      "difference_ms": round(min(rows[True]) - min(rows[False]), 1)}), flush=True)


def child_default(a):
    import transvae
    vae, dit, ref, kw = eval_setup(a, False)
    transvae.evaluate_dit(vae, dit, ref, **dict(kw, num_samples=128, steps=1))                                 # warm-up
    print(json.dumps({"ms": round(timed(lambda: transvae.evaluate_dit(vae, dit, ref, **kw), 1), 1)}), flush=True)


def child_trace(a):
    import torch
    import transvae
    dev = torch.device("cuda:0")
    x, q = features_like(10000, 0, dev), features_like(10000, 1, dev)
    r2 = transvae.knn_radius(x, K_NN)
    transvae.manifold_hits(q, x, r2)
    if hasattr(transvae, "ball_counts"):
        from transvae.metrics_fid import SPATIAL_CHANNELS, SPATIAL_LD, spatial_rows
        transvae.ball_counts(q, x, r2, "data")
        transvae.ball_counts(x, q, r2, "query")
        ia, ib, _ = transvae.kid_subsets(10000, 10000, 100, 1000, 0)
        ia, ib = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
        transvae.poly_kernel_sums(x, ia, q, ib, 1.0 / D_FEAT, 1.0, False)
        spatial_rows(torch.randn(256, 17, 17, 768, device=dev).bfloat16(), 0, SPATIAL_CHANNELS, SPATIAL_LD)
    head = transvae.InceptionScore(torch.randn(1008, D_FEAT) * 0.02).to(dev)
    for _ in range(3):
        head.update(x[:256])
    m = transvae.create_dit("DiT-B", HW, P, D, 1000).to(dev)
    ema = transvae.ParamEMA(m.parameters())
    for _ in range(5):
        ema.update()
    torch.cuda.synchronize()


CHILDREN = {"pairwise": child_pairwise, "small": child_small, "evaluate": child_evaluate, "suite": child_suite, "default": child_default,
            "trace": child_trace}


def run_child(step, a, timeout, prefix=(), root=ROOT):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", step, "--points", a.points, "--iters", str(a.iters),
                          "--samples", str(a.samples), "--steps", str(a.steps), "--root", root]
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=root)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        raise SystemExit(f"gen_eval_bench: step '{step}' failed with status {r.returncode}; stopping")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="10000,50000")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="pairwise,small,evaluate,suite", help="which timing steps to run")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit; empty: the default call is not compared")
    ap.add_argument("--root", default=ROOT, help="(child) the tree whose package is imported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_eval_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "gen_eval_kernel_stats.csv"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a fresh temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        root = os.path.abspath(a.root)
        if root != ROOT:                                      # the parent's package, this file's timing code
            sys.path[:0] = [root, os.path.join(root, "deepl-project_amd")]
        return CHILDREN[a.child](a)
    report = {"rows": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            report = json.load(f)
    rows = []
    for step, limit in (("pairwise", 300), ("small", 240), ("evaluate", 420), ("suite", 420)):
        if step in a.only.split(","):
            new = [json.loads(l) for l in run_child(step, a, limit).splitlines() if l.startswith("{")]
            for r in new:
                print(r, flush=True)
            rows += new
    fresh = {(r["what"], r.get("case")) for r in rows}
    report.update({"points": a.points, "samples": a.samples, "steps": a.steps,
                   "rows": [r for r in report["rows"] if (r["what"], r.get("case")) not in fresh] + rows})
    if a.parent:
        parent, here = [], []
        for r in range(3):                                           # parent, here | here, parent | parent, here
            for tree, ms in ((os.path.abspath(a.parent), parent), (ROOT, here))[::1 if r % 2 == 0 else -1]:
                ms.append(json.loads([l for l in run_child("default", a, 240, root=tree).splitlines() if l.startswith("{")][0])["ms"])
        report["default_call_vs_parent"] = {"parent_ms": parent, "this_tree_ms": here, "parent_window_spread": round(max(parent) / min(parent) - 1.0, 4),
                                            "this_tree_window_spread": round(max(here) / min(here) - 1.0, 4),
                                            "this_tree_over_parent": round(sorted(here)[1] / sorted(parent)[1], 4)}
        print(report["default_call_vs_parent"], flush=True)
    elif "default_call_vs_parent" not in report:
        report["default_call_vs_parent"] = "not measured"
    if not a.no_trace:
        tdir = a.trace_dir or tempfile.mkdtemp(prefix="gen_eval_trace_")
        os.makedirs(tdir, exist_ok=True)
        run_child("trace", a, 240, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "gen_eval", "--output-format", "csv", "--"))
        stats = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            with open(stats[-1]) as f, open(a.stats_out, "w") as g:
                g.write(f.read())
            with open(a.stats_out) as f:
                report["kernel_stats"] = [row for row in csv.DictReader(f)
                                          if any(w in row.get("Name", "") for w in ("pairwise_", "softmax_rows", "softmax_state", "opt_ema", "poly_",
                                                                                    "spatial_rows"))]
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
