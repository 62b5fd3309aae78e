"""SHA-256 digests of what the wave-per-row kernels write (csrc/row_wave.h: the row norms of csrc/norm.hip, the adaLN pairs of
csrc/dit.hip) and of what the per-head qk-norm kernels write (csrc/qk_norm.hip, head_dim 64 and 72), for proving that a change
to them moved no bit.  GPU box.

    python tools/row_kernel_digests.py --out new.json                      # the in-tree library
    TV_HIP_SO=/path/to/other.so python tools/row_kernel_digests.py --out old.json
    python tools/row_kernel_digests.py --out new.json --compare old.json     # exits 1 and names the first differing case

Inputs come from fixed-seed CPU generators, the calls go through the C ABI, and every output tensor is hashed as its raw bytes.
Shapes: C in {8, 128, 384, 768, 1152, 1536} (and 2560 for norm.hip) -- 1, 2, 3 and 5 chunks per lane, a single-chunk row, partly
filled last chunks and completely filled lanes -- times (B, N) in {(2, 1), (3, 65), (2, 256)}: one-row samples, a short last slab,
whole slabs.  Rows sit 8 standard deviations from 0, so that the centring matters.  The `dw` of tv_rownorm_bwd mode 1 is summed by
atomics in no fixed order: it is kept as values, not hashed, and --compare prints its largest
difference relative to the tensor's largest entry, which is order noise of about 1e-7.
The qk-norm pair at both head dims: forward out of place and in place, with and without a table (arbitrary fp32 [N, 4, hd / 2]);
backward: dqkv, dwq and dwk, all hashed (fixed-order sums).  (B, N, heads) in QK: a ragged last group, one-token samples, a short
slab, more than one backward pass per block (36864 head vectors against 1024 blocks of 32 or 16), more than one forward pass.
"""
import argparse
import base64
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deepl-project_amd"))

CS_ADALN = (8, 128, 384, 768, 1152, 1536)
CS_NORM = CS_ADALN + (2560,)
BN = ((2, 1), (3, 65), (2, 256))
QK = ((1, 5, 3), (2, 1, 6), (3, 65, 2), (3, 256, 24), (1, 16500, 1))
EPS = 1e-6


def digests():
    import numpy as np
    import torch
    from transvae.hip import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, values = {}, {}

    def sha(name, t):
        torch.cuda.synchronize()
        out[name] = hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

    def call(name, *args):
        L.check(getattr(lib, name)(*args, st()), name)

    for Cc in CS_NORM:
        for B, N in BN:
            T = B * N
            g = torch.Generator().manual_seed(1000 * Cc + T)
            rows = lambda: (torch.randn(T, Cc, generator=g) + 8.0).bfloat16().to(dev)
            x, dy, dres = rows(), torch.randn(T, Cc, generator=g).bfloat16().to(dev), torch.randn(T, Cc, generator=g).bfloat16().to(dev)
            w = (1 + 0.1 * torch.randn(Cc, generator=g)).to(dev)
            mod = (0.3 * torch.randn(B, 3 * Cc + 8, generator=g)).to(dev)
            gamma, beta = (1 + 0.1 * torch.randn(Cc, generator=g)).to(dev), (0.1 * torch.randn(Cc, generator=g)).to(dev)
            tag = f"C={Cc} B={B} N={N}"
            ld, shift_off, scale_off, gate_off = 3 * Cc + 8, Cc, 2 * Cc + 8, 8

            for mode in (0, 1, 2):
                y = torch.full_like(x, 7.0)
                call("tv_rownorm_fwd", p(x), p(w), p(y), T, Cc, mode, EPS, EPS)
                sha(f"tv_rownorm_fwd mode={mode} {tag}: y", y)
            for mode in (0, 1):
                for r in (None, dres):
                    dx, dw = torch.full_like(x, 7.0), torch.zeros(Cc, device=dev)
                    call("tv_rownorm_bwd", p(x), p(w), p(dy), p(r), p(dx), p(dw), T, Cc, mode, EPS, EPS)
                    name = f"tv_rownorm_bwd mode={mode} dres={int(r is not None)} {tag}"
                    sha(name + ": dx", dx)
                    if mode == 1:
                        values[name + ": dw"] = base64.b64encode(dw.cpu().numpy().astype(np.float32).tobytes()).decode()
            for skip in (0, 1):
                if skip < N:
                    y = torch.full((B * (N - skip), Cc), 7.0, device=dev)
                    call("tv_layernorm_rows", p(x), p(gamma), p(beta), p(y), B, N, skip, Cc, EPS)
                    sha(f"tv_layernorm_rows skip={skip} {tag}: y", y)
            if Cc not in CS_ADALN:
                continue

            for rms in (False, True):
                fn, head = ("tv_adaln_rms", (p(x), p(w))) if rms else ("tv_adaln", (p(x),))
                y = torch.full_like(x, 7.0)
                call(fn + "_fwd", *head, p(mod), shift_off, scale_off, ld, p(y), B, N, Cc, EPS)
                sha(f"{fn}_fwd {tag}: y", y)
                count = getattr(lib, fn + "_bwd_partial_count")(B, N, Cc)
                for r in (None, dres):
                    dx, dmod, dw = torch.full_like(x, 7.0), torch.full_like(mod, 7.0), torch.full((Cc,), 7.0, device=dev)
                    part = torch.empty(count, device=dev)
                    extra = (p(dw),) if rms else ()
                    call(fn + "_bwd", *head, p(mod), shift_off, scale_off, ld, p(dy), p(r), p(dx), p(dmod), *extra, p(part), B, N, Cc, EPS)
                    name = f"{fn}_bwd dres={int(r is not None)} {tag}"
                    sha(name + ": dx", dx)
                    sha(name + ": dshift", dmod[:, shift_off:shift_off + Cc])
                    sha(name + ": dscale", dmod[:, scale_off:scale_off + Cc])
                    sha(name + ": dmod (all columns, 7 where nothing is written)", dmod)
                    if rms:
                        sha(name + ": dw", dw)

            dyg, dmod = torch.full_like(x, 7.0), torch.full_like(mod, 7.0)
            part = torch.empty(lib.tv_gate_residual_bwd_partial_count(B, N, Cc), device=dev)
            call("tv_gate_residual_bwd", p(dy), p(x), p(mod), gate_off, ld, p(dyg), p(dmod), p(part), B, N, Cc)
            sha(f"tv_gate_residual_bwd {tag}: dy", dyg)
            sha(f"tv_gate_residual_bwd {tag}: dgate", dmod[:, gate_off:gate_off + Cc])

    for hd in (64, 72):
        s, h = ("", ()) if hd == 64 else ("_hd", (hd,))
        for B, N, heads in QK:
            g = torch.Generator().manual_seed(100 * hd + B + N + heads)
            qkv, dq = (torch.randn(B, N, 3 * heads * hd, generator=g).bfloat16().to(dev) for _ in range(2))
            wq, wk = ((1 + 0.1 * torch.randn(hd, generator=g)).to(dev) for _ in range(2))
            tab = torch.randn(N, 4, hd // 2, generator=g).to(dev)
            tag = f"hd={hd} B={B} N={N} heads={heads}"
            for t in (None, tab):
                y, z = torch.full_like(qkv, 7.0), qkv.clone()
                call(f"tv_qknorm_rope_fwd{s}", p(qkv), p(wq), p(wk), p(t), p(y), B, N, heads, *h, EPS)
                sha(f"tv_qknorm_rope_fwd{s} table={int(t is not None)} {tag}: out", y)
                call(f"tv_qknorm_rope_fwd{s}", p(z), p(wq), p(wk), p(t), p(z), B, N, heads, *h, EPS)
                sha(f"tv_qknorm_rope_fwd{s} table={int(t is not None)} in place {tag}: out", z)
            dqkv, dwq, dwk = dq.clone(), torch.full((hd,), 7.0, device=dev), torch.full((hd,), 7.0, device=dev)
            part = torch.empty(getattr(lib, f"tv_qknorm_rope_bwd{s}_partial_count")(B, N, heads, *h), device=dev)
            call(f"tv_qknorm_rope_bwd{s}", p(qkv), p(wq), p(wk), p(dqkv), p(dwq), p(dwk), p(part), B, N, heads, *h, EPS)
            for nm, t in (("dqkv", dqkv), ("dwq", dwq), ("dwk", dwk)):
                sha(f"tv_qknorm_rope_bwd{s} {tag}: {nm}", t)
    return {"library": L.SO_PATH, "sha256": out, "values": values}


def compare(new, old):
    import numpy as np
    if list(new["sha256"]) != list(old["sha256"]):
        print("row_kernel_digests: the two files hold different cases")
        return 1
    for name, h in new["sha256"].items():
        if old["sha256"][name] != h:
            print(f"row_kernel_digests: DIFFERENT at {name}\n  {new['library']}: {h}\n  {old['library']}: {old['sha256'][name]}")
            return 1
    worst, where = 0.0, ""
    for name, v in new["values"].items():
        a = np.frombuffer(base64.b64decode(v), dtype=np.float32).astype(np.float64)
        b = np.frombuffer(base64.b64decode(old["values"][name]), dtype=np.float32).astype(np.float64)
        rel = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
        if rel > worst:
            worst, where = rel, name
    print(f"row_kernel_digests: {len(new['sha256'])} digests equal; atomically summed dw: largest difference {worst:.3g} of the tensor's "
          f"largest entry ({where})")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", default=None, help="a file written by another run of this tool")
    a = ap.parse_args()
    res = digests()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"row_kernel_digests: {len(res['sha256'])} digests of {res['library']} -> {a.out}")
    if a.compare:
        with open(a.compare) as f:
            return compare(res, json.load(f))
    return 0


if __name__ == "__main__":
    sys.exit(main())
