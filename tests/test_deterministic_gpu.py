"""Deterministic mode on the GPU: every parameter gradient of the HIP kernels is the same bits on every run,
and those bits are the documented fixed-order sum -- slice 0 + slice 1 + ... in fp32 -- of the partial results the kernels store.

The references are sequential fp32 loops in torch on the CPU (IEEE fp32 adds give the same bits there) for the order, and the
fp64 references and bounds of tests/test_error_budget_host.py (rows W and N of the rounding contract, unchanged) for the values.
Every tuning hook a test sets is restored in a `finally`."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

from test_error_budget_host import (BF, EPS_LN, EPS_RMS, F64, ROWNORM_C_DW, WGRAD_C, check_fp32, gn_inputs, r16, rms_ln_inputs,
                                    rownorm_bwd64)
from wgrad_matrix_cases import wgrad_ref64       # (the descriptor's own gather in fp64; shared with test_wgrad_matrix_gpu.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


def seq_sum(slices: torch.Tensor) -> torch.Tensor:
    """S = fl(...fl(fl(P_0 + P_1) + P_2)... + P_{n-1}) in fp32 on the CPU; slices [n, ...]"""
    s = slices[0].clone()
    for k in range(1, slices.shape[0]):
        s = s + slices[k]
    return s


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. tv_reduce_slices
# ---------------------------------------------------------------------------------------------------------------------------
MAX_SLICES = 33


def _reduce_data(n: int) -> torch.Tensor:
    """[33, n] fp32: magnitudes over 2^-12 .. 2^12 so that almost every add rounds, plus -- at fixed columns where n allows --
    +-0, denormals and values 2^24 apart, whose sum depends on the order"""
    g = torch.Generator().manual_seed(n)
    p = torch.randn(MAX_SLICES, n, generator=g) * torch.exp2(torch.randint(-12, 13, (MAX_SLICES, n), generator=g).float())
    cols = list(range(min(n, 6)))
    special = [
        [-0.0] * MAX_SLICES,                                              # all -0: the sum is -0, not +0
        [0.0, -0.0] * 16 + [0.0],
        [1e-40, -3e-41, 1e-45] * 11,                                      # denormals
        [2.0 ** 24, 1.0, 1.0, -2.0 ** 24] + [1.0] * 29,                   # (2^24 + 1) + 1 = 2^24 in this order only
        [1.0, 2.0 ** 24, -2.0 ** 24, 1.0] + [2.0 ** -24] * 29,
        [-2.0 ** 24, 2.0 ** 24, 1.0] * 11,
    ]
    for c, v in zip(cols, special):
        p[:, c] = torch.tensor(v, dtype=torch.float32)
    return p


@pytest.mark.parametrize("n", [4, 60, 1, 7, 66, 1000003])
def test_reduce_slices_is_the_sequential_fp32_sum(n):
    """slices 1, 2, 7, 33 x accum 0 / 1 x (aligned, both pointers + 4 bytes, only `out` + 4 bytes) x slice stride n and larger:
    bit-equal to the CPU loop, -0 and denormals included.  n covers the vector body alone (4, 60), the scalar form (1), body +
    tail (7, 66) and many blocks with a tail (1000003)."""
    from transvae.hip import _lib as L
    lib = L.load()
    p = _reduce_data(n)
    old = torch.randn(n, generator=torch.Generator().manual_seed(7)) * 3
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wants = {k: seq_sum(p[:k]) for k in (1, 2, 7, 33)}
    for stride in (n, n + 1, (n + 3) // 4 * 4 + 8):
        for off_p, off_o in ((0, 0), (1, 1), (0, 1)):
            flat = torch.zeros(off_p + MAX_SLICES * stride, dtype=torch.float32)
            flat[off_p:].view(MAX_SLICES, stride)[:, :n] = p
            flat_d = flat.to(dev())
            for k in (1, 2, 7, 33):
                want = wants[k]
                for accum in (0, 1):
                    out = torch.full((n + 2,), float("nan"), dtype=torch.float32, device=dev())
                    o = out[off_o:off_o + n]
                    if accum:
                        o.copy_(old)
                    L.check(lib.tv_reduce_slices(C.c_void_p(flat_d.data_ptr() + 4 * off_p), k, n, stride, C.c_void_p(o.data_ptr()), accum,
                                                 stream), "tv_reduce_slices")
                    got = out.cpu()
                    ref = old + want if accum else want
                    assert same_bits(got[off_o:off_o + n], ref), (n, stride, off_p, off_o, k, accum)
                    assert bool(torch.isnan(torch.cat([got[:off_o], got[off_o + n:]])).all()), "stored outside [0, n)"


def test_reduce_slices_rejects_bad_arguments():
    from transvae.hip import _lib as L
    lib = L.load()
    t = torch.zeros(64, device=dev())
    p = C.c_void_p(t.data_ptr())
    assert lib.tv_reduce_slices(p, 0, 8, 8, p, 0, None) != 0
    assert lib.tv_reduce_slices(p, 2, 8, 4, p, 0, None) != 0       # overlapping slices
    assert lib.tv_reduce_slices(None, 2, 8, 8, p, 0, None) != 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def _wgrad_problem(mode, shape):
    """(descriptor, gathered operand shape, other operand shape, dw shape) of the launch ops.conv_wgrad makes for this layer:
    the layer's own geometry, or -- 'c3up' -- the adjoint problem whose result is folded onto the 3x3 taps afterwards"""
    from transvae.hip import ops
    if mode == "linear":
        T, ci, co = shape
        return ops._rows_desc(T, ci, co), (T, 1, 1, ci), (T, 1, 1, co), (co, 1, 1, ci)
    B, H, W, ci, co = shape
    k = {"c3s1": 3, "c3s2": 3, "c3up": 3, "c4s2": 4}[mode]
    geo = ops._Geo(mode, torch.empty(B, H, W, ci, device="meta"), torch.empty(co, k, k, ci, device="meta"))
    if mode == "c3up":
        d = geo.dgrad_desc()
        return d, (B, d.h_in, d.w_in, d.c_in), (B, d.h_out, d.w_out, d.c_out), (d.c_out, d.kh, d.kw, d.c_in)
    d = geo.fwd_desc(0)
    return d, (B, H, W, ci), (B, d.h_out, d.w_out, co), (co, k, k, ci)


WGRAD_CASES = [
    ("c3s1", (4, 64, 64, 192, 384)),        # kx3, 192 x 96 x 3 tiles
    ("c3s1", (5, 128, 128, 192, 192)),      # kx3, XCD-grouped block order, ragged last chunk
    ("c3s1", (2, 16, 16, 192, 96)),         # single-tap kernel, co tile past c_out
    ("linear", (4096, 384, 192)),           # kx3's one-tap instantiation
    ("linear", (2048 + 72, 1536, 768)),     # single-tap kernel, pixels no multiple of the K-step
    ("c3s2", (2, 32, 32, 64, 96)),
    ("c3up", (2, 32, 32, 64, 96)),
    ("c4s2", (2, 32, 32, 64, 96)),
    ("c3s1/single-tap", (4, 64, 64, 192, 384)),     # the first shape through the single-tap kernel (a block target switches kx3 off)
]


@pytest.mark.parametrize("mode,shape", WGRAD_CASES, ids=[f"{m}-" + "x".join(map(str, s)) for m, s in WGRAD_CASES])
def test_wgrad_is_the_ordered_sum_of_its_chunks(mode, shape):
    """With bias, split natural where the heuristic splits and forced through the tuning hooks where it gives one chunk (a layer of
    512 pixels cannot split: one chunk is then what is tested): (a) three calls bit-equal; (b) the workspace slices, added
    sequentially on the CPU, are dw / dbias bit for bit; (c) accumulating onto 0.5 / -0.25 gives 0.5 + S / -0.25 + S; (d) row W's
    bound against fp64."""
    from transvae.hip import _lib as L, ops
    lib = L.load()
    mode, forced_tn = mode.split("/")[0], mode.endswith("/single-tap")
    d, xs, gs, dws = _wgrad_problem(mode, shape)
    g = torch.Generator().manual_seed(sum(shape))
    x = r16(torch.randn(xs, generator=g, dtype=F64))
    gy = r16(torch.randn(gs, generator=g, dtype=F64) * torch.exp2(torch.randint(-3, 4, (1, 1, 1, gs[-1]), generator=g).to(F64)))
    xd, gd = x.to(dev(), BF).contiguous(), gy.to(dev(), BF).contiguous()
    n, co = dws[0] * dws[1] * dws[2] * dws[3], dws[0]
    try:
        if forced_tn:
            lib.tv_set_wgrad_config(0, 0, 1024)
        if ops.wgrad_det_plan(d)[0] == 1:
            lib.tv_set_wgrad_kx3(1, 0, 4096)
            if ops.wgrad_det_plan(d)[0] == 1:
                lib.tv_set_wgrad_config(0, 0, 4096)
        ny, nbytes = ops.wgrad_det_plan(d)
        assert nbytes == (ny * (n + co) * 4 if ny > 1 else 0)
        runs = []
        with ops.deterministic():
            for _ in range(3):
                dw = torch.full(dws, float("nan"), dtype=torch.float32, device=dev())      # (the call writes every element)
                db = torch.zeros(co, dtype=torch.float32, device=dev())
                ops.wgrad(d, xd, gd, dw, db)
                runs.append((dw.cpu(), db.cpu()))
            buf, info = ops.det_workspace()
            assert info["kind"] == "wgrad" and info["ny"] == ny and info["slice_elems"] == n and info["bias_elems"] == co
            if ny > 1:
                slices = buf[:ny * n].view(ny, n).cpu()
                bslices = buf[info["bias_offset"]:info["bias_offset"] + ny * co].view(ny, co).cpu()
            dw2 = torch.full(dws, 0.5, dtype=torch.float32, device=dev())
            db2 = torch.full((co,), -0.25, dtype=torch.float32, device=dev())
            ops.wgrad_acc(d, xd, gd, dw2, db2)
            torch.cuda.synchronize()
    finally:
        lib.tv_set_wgrad_kx3(2, 0, 0)
        lib.tv_set_wgrad_config(0, 0, 0)
    dw, db = runs[0]
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    for i in (1, 2):                                                                          # (a)
        assert same_bits(runs[i][0], dw), f"dw of run {i} differs in {int((runs[i][0] != dw).sum())} elements"
        assert same_bits(runs[i][1], db), f"dbias of run {i} differs in {int((runs[i][1] != db).sum())} elements"
    if ny > 1:                                                                                # (b)
        assert same_bits(seq_sum(slices), dw.flatten()), "dw is not the sequential sum of its slices"
        assert torch.equal(0.0 + seq_sum(bslices), db), "dbias is not 0 + the sequential sum of its slices"
        sb = seq_sum(bslices)
    else:
        sb = db
    assert same_bits(dw2.cpu(), 0.5 + dw), "accumulate: dw != 0.5 + S"                         # (c)
    assert same_bits(db2.cpu(), -0.25 + sb), "accumulate: dbias != -0.25 + S"
    dw64, adw = wgrad_ref64(x, gy, d.kh, d.kw, d.stride, d.pad, d.up_shift)                    # (d)
    r_w = check_fp32(dw, dw64, adw, WGRAD_C, f"deterministic dw {mode} {shape}")
    g2 = gy.to(F64).reshape(-1, co)
    r_b = check_fp32(db, g2.sum(0), g2.abs().sum(0), WGRAD_C, f"deterministic dbias {mode} {shape}")
    print(f"[deterministic] wgrad {mode} {shape}: ny {ny}, ratio to row W's bound dw {r_w:.3f} dbias {r_b:.3f}")


@pytest.mark.parametrize("mode,shape", [("linear", (512, 64, 64)), ("c3s1", (1, 16, 64, 192, 192))],
                         ids=["linear-512x64x64", "c3s1-1x16x64x192x192"])
def test_wgrad_agrees_with_the_default_call_where_the_order_cannot_matter(mode, shape):
    """The linear layer is one chunk: no workspace, the default instantiation's plain store, dw and dbias (one workgroup per
    output-channel tile in either mode) bit-equal to the default call.  The 3x3 layer is two chunks under today's heuristic:
    0 + P0 + P1 in either arrival order is the same fp32 number as P0 + P1, so dw still agrees bit for bit; its dbias is
    summed by six workgroups per chunk in the default call and by one here, and is held to repeatability instead."""
    from transvae.hip import ops
    d, xs, gs, dws = _wgrad_problem(mode, shape)
    ny = ops.wgrad_det_plan(d)[0]
    assert ny <= 2
    g = torch.Generator().manual_seed(11)
    xd = r16(torch.randn(xs, generator=g, dtype=F64)).to(dev(), BF)
    gd = r16(torch.randn(gs, generator=g, dtype=F64)).to(dev(), BF)
    out = []
    for on in (False, True, True):
        with ops.deterministic(on):
            dw = torch.zeros(dws, dtype=torch.float32, device=dev())
            db = torch.zeros(dws[0], dtype=torch.float32, device=dev())
            ops.wgrad(d, xd, gd, dw, db)
            out.append((dw.cpu(), db.cpu()))
    assert torch.equal(out[1][0], out[0][0]), "deterministic dw differs from the default call"
    assert same_bits(out[2][0], out[1][0]) and same_bits(out[2][1], out[1][1])
    if mode == "linear":
        assert ops.wgrad_det_plan(d) == (1, 0)
        assert torch.equal(out[1][1], out[0][1]), "deterministic dbias differs from the default call"


def test_wgrad_batch_chunked_launch_adds_later_chunks(monkeypatch):
    """A launch over the 2 GiB limit goes image chunk by image chunk, later chunks adding (ops._launch's rule): with the limit
    lowered so that every image is a launch, the deterministic result is repeatable and inside row W's bound"""
    from transvae.hip import ops
    mode, shape = "c3s1", (4, 32, 64, 192, 192)
    d, xs, gs, dws = _wgrad_problem(mode, shape)
    g = torch.Generator().manual_seed(5)
    x = r16(torch.randn(xs, generator=g, dtype=F64))
    gy = r16(torch.randn(gs, generator=g, dtype=F64))
    xd, gd = x.to(dev(), BF), gy.to(dev(), BF)
    monkeypatch.setattr(ops, "_LAUNCH_BYTES", 32 * 64 * 192 * 2 + 1)
    assert len(ops._batch_chunks(4, [xd, gd])) == 4
    runs = []
    with ops.deterministic():
        for _ in range(2):
            dw = torch.full(dws, float("nan"), dtype=torch.float32, device=dev())
            db = torch.zeros(dws[0], dtype=torch.float32, device=dev())
            ops.wgrad(d, xd, gd, dw, db)
            runs.append((dw.cpu(), db.cpu()))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    dw64, adw = wgrad_ref64(x, gy, 3, 3, 1, 1, 0)
    check_fp32(runs[0][0], dw64, adw, WGRAD_C, "chunked deterministic dw")


def test_wgrad_refuses_a_small_workspace():
    from transvae.hip import _lib as L, ops
    lib = L.load()
    d, xs, gs, dws = _wgrad_problem("linear", (4096, 384, 192))
    ny, need = ops.wgrad_det_plan(d)
    assert ny > 1
    xd = torch.zeros(xs, dtype=BF, device=dev())
    gd = torch.zeros(gs, dtype=BF, device=dev())
    dw = torch.zeros(dws, device=dev())
    ws = torch.zeros(need // 4, device=dev())
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.tv_wgrad_tn_det(C.byref(d), p(xd), p(gd), p(dw), None, 0, p(ws), need - 4, None)
    assert rc != 0 and b"workspace" in lib.tv_last_error()
    assert lib.tv_wgrad_tn_det(C.byref(d), p(xd), p(gd), p(dw), None, 0, None, 0, None) != 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. GroupNorm + SiLU backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cc", [(1, 64), (3, 64), (8, 64), (1, 192), (3, 192), (8, 192)])
def test_groupnorm_parameter_gradients_are_added_in_image_order(B, Cc):
    """dgamma / dbeta: three calls bit-equal, and equal to the fp32 sum over b = 0, 1, ... of the `red` rows the first backward
    pass wrote; dx bit-equal to the default path's (the same kernel with the parameter-gradient adds skipped)"""
    from transvae.hip import _lib as L, ops
    lib = L.load()
    G, H, W = 32, 24, 24                      # 576 pixels: a full 512-pixel slab and a ragged one
    x, gamma, beta = gn_inputs(B, H * W, Cc, G, seed=B * Cc)
    gy = r16(torch.randn(B, H * W, Cc, generator=torch.Generator().manual_seed(2), dtype=F64))
    xd = x.view(B, H, W, Cc).to(dev(), BF).contiguous()
    gyd = gy.view(B, H, W, Cc).to(dev(), BF).contiguous()
    gd, bd = gamma.float().to(dev()), beta.float().to(dev())
    _, mr = ops.gn_silu_fwd(xd, gd, bd, G, 1e-5)
    p = lambda t: C.c_void_p(t.data_ptr())
    red = torch.empty((B, Cc, 2), dtype=torch.float32, device=dev())
    part = torch.empty((lib.tv_gn_partial_count(B, H * W, Cc),), dtype=torch.float32, device=dev())
    L.check(lib.tv_gn_silu_bwd_reduce(p(xd), p(gyd), p(mr), p(gd), p(bd), p(red), p(part), B, H * W, Cc, G,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tv_gn_silu_bwd_reduce")
    want = seq_sum(red.cpu())                 # [C, 2]: (dbeta, dgamma)
    dx0, dg0, db0 = ops.gn_silu_bwd(xd, gyd, None, mr, gd, bd, G)
    with ops.deterministic():
        runs = [ops.gn_silu_bwd(xd, gyd, None, mr, gd, bd, G) for _ in range(3)]
    torch.cuda.synchronize()
    for dx, dg, db in runs:
        assert torch.equal(dx, dx0), "dx differs from the default path"
        assert torch.equal(dg.cpu(), 0.0 + want[:, 1]) and torch.equal(db.cpu(), 0.0 + want[:, 0])
        assert same_bits(dg.cpu(), runs[0][1].cpu()) and same_bits(db.cpu(), runs[0][2].cpu())
    # the default path adds the same rows by atomics: equal up to the order of B adds
    tol = 2.0 ** -22 * red.abs().sum(0).cpu()
    assert bool(((dg0.cpu() - want[:, 1]).abs() <= tol[:, 1] + 1e-30).all()) and bool(((db0.cpu() - want[:, 0]).abs() <= tol[:, 0] + 1e-30).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. row-norm backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Cc", [(65, 72), (4096, 384), (1000, 1536)])
def test_rownorm_weight_gradient_is_bit_reproducible(T, Cc):
    """mode 1 (RMSNorm weight, then LayerNorm): dw over three calls bit-equal, inside the existing row's bound against fp64
    (ROWNORM_C_DW), and the sequential sum of the per-workgroup slices; dx bit-equal to the default path's"""
    from transvae.hip import ops
    x, w, gy = rms_ln_inputs(T, Cc, seed=T + Cc)
    xd, wd, gd = x.to(dev(), BF), w.float().to(dev()), gy.to(dev(), BF)
    dx0, dw0 = ops.rownorm_bwd(xd, wd, gd, None, 1, EPS_RMS, EPS_LN)
    with ops.deterministic():
        runs = [ops.rownorm_bwd(xd, wd, gd, None, 1, EPS_RMS, EPS_LN) for _ in range(3)]
        buf, info = ops.det_workspace()
        assert info["kind"] == "rownorm" and info["slice_elems"] == Cc and info["ny"] == min((T + 3) // 4, 1024)
        slices = buf[:info["ny"] * Cc].view(info["ny"], Cc).cpu()
    torch.cuda.synchronize()
    dw = runs[0][1].cpu()
    for dx, dwi in runs:
        assert torch.equal(dx, dx0), "dx differs from the default path"
        assert same_bits(dwi.cpu(), dw), f"dw differs in {int((dwi.cpu() != dw).sum())} elements"
    assert torch.equal(dw, 0.0 + seq_sum(slices)), "dw is not 0 + the sequential sum of the workgroups' slices"
    _, _, dw64, dwt = rownorm_bwd64(x, w, gy, None, 1)
    r = check_fp32(dw, dw64, dwt, ROWNORM_C_DW, f"deterministic rms_ln_hat dw {T}x{Cc}")
    check_fp32(dw0.cpu(), dw64, dwt, ROWNORM_C_DW, "default rms_ln_hat dw")
    print(f"[deterministic] rownorm {T}x{Cc}: ratio to the row's bound {r:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. whole step   7. DiT
# ---------------------------------------------------------------------------------------------------------------------------
def _step_digest():
    spec = importlib.util.spec_from_file_location("step_digest", os.path.join(ROOT, "tools", "step_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_steps_have_equal_digests(monkeypatch):
    """tools/step_digest.step_digest twice from identical seeds: the micro model of tests/test_train_gpu.py (oracle.MICRO: five
    stages of depth 1), batch 4 at 64 x 64 in two micro-batches -- so that weight gradients are ADDED in place (the accumulate form of
    the deterministic launch, counted here) -- three optimizer steps
    of train_step + FusedAdamW + clip 1.0 inside transvae.deterministic().  Every digest -- each parameter, each gradient of the
    last step, every loss -- is equal.  (That the default mode differs is NOT asserted: at this size it often does not.)"""
    from oracle import transvae_oracle as O
    from transvae.hip import ops
    sd = _step_digest()
    assert sd.MICRO == O.MICRO
    launches = {False: 0, True: 0}
    inner = ops._wgrad_det

    def counting(desc, x, gy, dw, dbias, acc):
        launches[bool(acc)] += 1
        return inner(desc, x, gy, dw, dbias, acc)
    monkeypatch.setattr(ops, "_wgrad_det", counting)
    a = sd.step_digest(steps=3, variant="micro", batch=4, res=64, micro=2, seed=0, device=dev())
    assert launches[False] > 0 and launches[True] > 0, f"deterministic weight-gradient launches (write / add in place): {launches}"
    b = sd.step_digest(steps=3, variant="micro", batch=4, res=64, micro=2, seed=0, device=dev())
    assert not ops.is_deterministic()
    assert len(a["params"]) > 50 and len(a["grads"]) > 50
    assert a["loss"] == b["loss"], (a["loss"], b["loss"])
    for kind in ("params", "grads"):
        diff = [n for n in a[kind] if a[kind][n] != b[kind][n]]
        assert not diff, f"{len(diff)} of {len(a[kind])} {kind} digests differ: {diff[:8]}"
    c = sd.step_digest(steps=1, variant="micro", batch=4, res=64, micro=2, seed=1, device=dev())
    assert c["params"] != a["params"]         # (the digest does see the numbers)


def test_dit_gradients_of_the_hip_kernels_are_bit_reproducible():
    """A width-128, depth-2 LightningDiT, B = 4 on 8 x 8 latents, fixed t and noise: two flow_matching_loss backward passes inside
    the context give bit-equal gradients for every parameter whose gradient the HIP kernels produce: the token GEMMs' weights
    and biases (patch embedding, qkv, proj, SwiGLU, final linear), the RMSNorm weights and the qk-norm weights.  Left out: the
    conditioning path (timestep MLP, label embedding table, the adaLN modulation linears) -- it runs on torch's own operators
    under autograd, whose determinism torch.use_deterministic_algorithms governs (the embedding backward is an index-add)."""
    import transvae
    m = transvae.LightningDiT(8, 1, 32, 128, 2, 10, generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():                     # adaLN-Zero starts with every gate at 0, i.e. most gradients exactly 0: move off it
        for n, p in m.named_parameters():
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g) if p.dim() == 1 and "norm" in n else
                    torch.randn(p.shape, generator=g) * (0.1 if p.dim() == 1 else p.shape[1] ** -0.5))
    m = m.to(dev()).eval()
    B, D = 4, 32
    lat = torch.randn(B, D, 8, 8, generator=g).to(dev())
    labels = torch.randint(0, 10, (B,), generator=g).to(dev())
    t = torch.rand(B, generator=g).to(dev())
    noise = torch.randn(B, D, 8, 8, generator=g).to(dev())
    stats = {"mean": torch.zeros(1, D, 1, 1, device=dev()), "std": torch.ones(1, D, 1, 1, device=dev())}
    conditioning = ("t_embedder.", "y_embedder.", "adaLN_modulation.")
    owned = [n for n, _ in m.named_parameters() if not any(c in n for c in conditioning)]
    assert len(owned) == 29
    grads, losses = [], []
    with transvae.deterministic():
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            losses.append(float(transvae.flow_matching_loss(m, lat, labels, stats, t=t, noise=noise)))
            grads.append({n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if n in owned})
    assert losses[0] == losses[1]
    for n in owned:
        assert not n.endswith(".weight") or float(grads[0][n].abs().max()) > 0, f"{n}: the gradient is identically zero"
        assert same_bits(grads[0][n], grads[1][n]), f"{n}: {int((grads[0][n] != grads[1][n]).sum())} elements differ"
