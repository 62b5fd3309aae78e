"""The FID Inception-v3 pool3 extractor restated in plain torch ops from its public definition (the pt_inception / pytorch-fid
`FIDInceptionV3` variant): the yardstick of tests/test_fid_host.py and tests/test_fid_gpu.py.  Neither pytorch_fid nor
torchvision is needed.

    x in [0, 1] -> F.interpolate(299 x 299, bilinear, align_corners=False) -> 2x - 1
    every layer: F.conv2d (no bias) -> F.batch_norm (eval, eps 1e-3) -> relu
    stem 3->32 3x3 s2, 32->32 3x3, 32->64 3x3 p1, max_pool 3 s2, 64->80 1x1, 80->192 3x3, max_pool 3 s2
    3 x InceptionA, InceptionB, 4 x InceptionC, InceptionD, 2 x InceptionE; branch average pools 3x3 s1 p1 with
    count_include_pad=False, the second InceptionE's pool branch a 3x3 s1 p1 max pool; adaptive average pool -> [B, 2048]

Weights are seeded and generated here, the same on every machine: convolutions He-scaled (std = sqrt(2 / (kh kw c_in))), BatchNorm
gamma in [0.9, 1.1], beta and running mean small, running variance in [0.5, 1.5], so 94 ReLU layers keep O(1) activations.

`python tests/fid_restatement.py --mint` rewrites tests/golden/fid_ref_bf16_autocast.json -- the restatement's OWN deviation under
torch.autocast("cpu", dtype=torch.bfloat16) from its fp32 run for each whole-network case of the GPU test, and the Frechet
distance (first 256 feature dimensions) between its autocast and its fp32 features of the FLOOR_N floor images -- and
tests/golden/fid_floor_ref_fp32.npz, its fp32 features (first 256 dimensions) of those images.
"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

SEED = 29917
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fid_ref_bf16_autocast.json")
GOLDEN_FLOOR = os.path.join(HERE, "golden", "fid_floor_ref_fp32.npz")
EPS = 1e-3

SHAPES = ((3, 256, 256), (2, 128, 192))      # whole-network cases of the GPU test
FLOOR_N, FLOOR_HW, FLOOR_DIMS = 512, 64, 256


def _layers():
    out = []

    def add(name, c_in, c_out, k=1, stride=1, pad=0):
        kh, kw = (k, k) if isinstance(k, int) else k
        out.append((name, c_in, c_out, kh, kw, stride, pad))

    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, 3)
    for blk, c_in, pool in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(f"{blk}.branch1x1", c_in, 64)
        add(f"{blk}.branch5x5_1", c_in, 48)
        add(f"{blk}.branch5x5_2", 48, 64, 5, 1, 2)
        add(f"{blk}.branch3x3dbl_1", c_in, 64)
        add(f"{blk}.branch3x3dbl_2", 64, 96, 3, 1, 1)
        add(f"{blk}.branch3x3dbl_3", 96, 96, 3, 1, 1)
        add(f"{blk}.branch_pool", c_in, pool)
    add("Mixed_6a.branch3x3", 288, 384, 3, 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(f"{blk}.branch1x1", 768, 192)
        add(f"{blk}.branch7x7_1", 768, c7)
        add(f"{blk}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(f"{blk}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(f"{blk}.branch7x7dbl_1", 768, c7)
        add(f"{blk}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(f"{blk}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(f"{blk}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(f"{blk}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(f"{blk}.branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for blk, c_in in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(f"{blk}.branch1x1", c_in, 320)
        add(f"{blk}.branch3x3_1", c_in, 384)
        add(f"{blk}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{blk}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{blk}.branch3x3dbl_1", c_in, 448)
        add(f"{blk}.branch3x3dbl_2", 448, 384, 3, 1, 1)
        add(f"{blk}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{blk}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{blk}.branch_pool", c_in, 192)
    return tuple(out)


LAYERS = _layers()
GEOMETRY = {l[0]: (l[5], l[6]) for l in LAYERS}     # name -> (stride, padding)


def plain_state_dict(seed=SEED):
    """The documented plain scheme: <layer>.weight, .gamma, .beta, .mean, .var (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, c_in, c_out, kh, kw, _, _ in LAYERS:
        sd[f"{name}.weight"] = torch.randn(c_out, c_in, kh, kw, generator=g) * math.sqrt(2.0 / (kh * kw * c_in))
        sd[f"{name}.gamma"] = 0.9 + 0.2 * torch.rand(c_out, generator=g)
        sd[f"{name}.beta"] = 0.05 * torch.randn(c_out, generator=g)
        sd[f"{name}.mean"] = 0.05 * torch.randn(c_out, generator=g)
        sd[f"{name}.var"] = 0.5 + torch.rand(c_out, generator=g)
    return sd


def pt_inception_state_dict(plain):
    """The same tensors under the key names of the pt_inception file (plus the entries a loader must ignore)."""
    sd = {}
    for name, *_ in LAYERS:
        sd[f"{name}.conv.weight"] = plain[f"{name}.weight"]
        sd[f"{name}.bn.weight"] = plain[f"{name}.gamma"]
        sd[f"{name}.bn.bias"] = plain[f"{name}.beta"]
        sd[f"{name}.bn.running_mean"] = plain[f"{name}.mean"]
        sd[f"{name}.bn.running_var"] = plain[f"{name}.var"]
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = torch.zeros(1008, 2048)
    sd["fc.bias"] = torch.zeros(1008)
    return sd


def features(x, sd):
    """x [B, 3, H, W] in [0, 1] -> [B, 2048]."""
    def c(h, name):
        stride, pad = GEOMETRY[name]
        dt = h.dtype
        h = F.conv2d(h, sd[f"{name}.weight"].to(dt), None, stride=stride, padding=pad)
        h = F.batch_norm(h, sd[f"{name}.mean"].to(dt), sd[f"{name}.var"].to(dt), sd[f"{name}.gamma"].to(dt), sd[f"{name}.beta"].to(dt),
                         False, 0.0, EPS)
        return F.relu(h)

    def chain(h, blk, names):
        for n in names:
            h = c(h, f"{blk}.{n}")
        return h

    def avg(h):
        return F.avg_pool2d(h, 3, stride=1, padding=1, count_include_pad=False)

    def inc_a(h, blk):
        return torch.cat([c(h, f"{blk}.branch1x1"), chain(h, blk, ("branch5x5_1", "branch5x5_2")),
                          chain(h, blk, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3")), c(avg(h), f"{blk}.branch_pool")], 1)

    def inc_b(h, blk):
        return torch.cat([c(h, f"{blk}.branch3x3"), chain(h, blk, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3")),
                          F.max_pool2d(h, 3, stride=2)], 1)

    def inc_c(h, blk):
        return torch.cat([c(h, f"{blk}.branch1x1"), chain(h, blk, ("branch7x7_1", "branch7x7_2", "branch7x7_3")),
                          chain(h, blk, ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5")),
                          c(avg(h), f"{blk}.branch_pool")], 1)

    def inc_d(h, blk):
        return torch.cat([chain(h, blk, ("branch3x3_1", "branch3x3_2")),
                          chain(h, blk, ("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4")), F.max_pool2d(h, 3, stride=2)], 1)

    def inc_e(h, blk, pool):
        t = c(h, f"{blk}.branch3x3_1")
        u = chain(h, blk, ("branch3x3dbl_1", "branch3x3dbl_2"))
        return torch.cat([c(h, f"{blk}.branch1x1"), c(t, f"{blk}.branch3x3_2a"), c(t, f"{blk}.branch3x3_2b"),
                          c(u, f"{blk}.branch3x3dbl_3a"), c(u, f"{blk}.branch3x3dbl_3b"), c(pool(h), f"{blk}.branch_pool")], 1)

    h = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    h = 2 * h - 1
    for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        h = c(h, n)
    h = F.max_pool2d(h, 3, stride=2)
    h = c(c(h, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
    h = F.max_pool2d(h, 3, stride=2)
    for blk in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        h = inc_a(h, blk)
    h = inc_b(h, "Mixed_6a")
    for blk in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        h = inc_c(h, blk)
    h = inc_d(h, "Mixed_7a")
    h = inc_e(h, "Mixed_7b", avg)
    h = inc_e(h, "Mixed_7c", lambda t: F.max_pool2d(t, 3, stride=1, padding=1))
    return F.adaptive_avg_pool2d(h, 1).flatten(1)


def smooth_images(n, H, W, seed):
    """Seeded smooth random fields in [0, 1]: low-resolution noise upsampled, plus a little fine noise."""
    g = torch.Generator().manual_seed(seed)
    t = F.interpolate(torch.rand(n, 3, max(2, H // 8), max(2, W // 8), generator=g), size=(H, W), mode="bilinear", align_corners=False)
    return (0.85 * t + 0.15 * torch.rand(n, 3, H, W, generator=g)).clamp(0, 1).contiguous()


def case_inputs(shape):
    B, H, W = shape
    return smooth_images(B, H, W, SEED + 7 * H + W)


def floor_images():
    return smooth_images(FLOOR_N, FLOOR_HW, FLOOR_HW, SEED + 1)


def run(x, sd, autocast=False, batch=64):
    outs = []
    with torch.no_grad():
        for i in range(0, x.shape[0], batch):
            with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
                outs.append(features(x[i:i + batch], sd).float())
    return torch.cat(outs)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def frechet_numpy(f1, f2):
    """Frechet distance between two full-rank feature sets [n, d] (n > d), fp64."""
    f1, f2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    mu1, mu2 = f1.mean(0), f2.mean(0)
    s1, s2 = np.cov(f1, rowvar=False), np.cov(f2, rowvar=False)
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    m = r @ s2 @ r
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    return float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())


def case_key(shape):
    return "x".join(map(str, shape))


def mint():
    sd = plain_state_dict()
    cases = {}
    for shape in SHAPES:
        x = case_inputs(shape)
        f32, f16 = run(x, sd), run(x, sd, autocast=True)
        assert torch.isfinite(f32).all() and float(f32.abs().max()) > 0
        cases[case_key(shape)] = {"features": rel_l2(f16, f32), "mean_abs_fp32": float(f32.abs().mean()), "max_abs_fp32": float(f32.abs().max())}
        print(case_key(shape), cases[case_key(shape)], flush=True)
    x = floor_images()
    f32, f16 = run(x, sd), run(x, sd, autocast=True)
    ref = f32[:, :FLOOR_DIMS].numpy().astype(np.float32)
    floor = {"n": FLOOR_N, "hw": FLOOR_HW, "dims": FLOOR_DIMS, "frechet_autocast_vs_fp32": frechet_numpy(f16[:, :FLOOR_DIMS].numpy(), ref),
             "features_rel_l2": rel_l2(f16, f32), "trace_cov_fp32": float(np.trace(np.cov(ref.astype(np.float64), rowvar=False)))}
    print("floor", floor, flush=True)
    np.savez_compressed(GOLDEN_FLOOR, features=ref)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "deviation of the plain-torch FID Inception-v3 restatement under torch.autocast('cpu', bfloat16) from its fp32 run: "
                           "rel-L2 of the features per case, and the Frechet distance between the two feature sets of the floor images",
                   "torch": torch.__version__, "cases": cases, "floor": floor}, f, indent=1)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        mint()
