"""The weight-gradient kernel matrix: which kernel the dispatch picks (ops.wgrad_which -- tv_wgrad_tn_which, the plan-only walk of
wgrad_impl down to the launch site), the set R of kernels it can reach with every hook at its default, and the table of small cases
-- one per member of R, plus the edges where such kernels break -- that tests/test_wgrad_matrix_gpu.py holds to row W of the
rounding contract.  tests/test_wgrad_matrix_host.py asserts that the table covers R; no GPU is needed here.

A case is (id, mode, shape, options, kernel, kernel_det): `kernel` / `kernel_det` are the instantiations the query must name for the
default and for the deterministic call with a bias gradient.  Options: ldx / ldo = extra columns of the operands' rows (a column
range of a wider row), tn / kx3 = arguments of tv_set_wgrad_config / tv_set_wgrad_kx3 for the case (restored by `hooks`)."""
import contextlib
import itertools
from typing import NamedTuple

import torch

F64 = torch.float64
CHANNELS = (8, 40, 64, 96, 128, 136, 160, 192, 200, 256, 384, 512, 576, 768, 1024, 1152, 1536)
GRIDS = ((8, 8), (6, 10), (16, 16), (32, 32), (64, 64), (16, 128))
TOKENS = (1, 9, 63, 64, 65, 512, 520, 576, 1000, 2048, 2120, 4096, 8192)
CONV_MODES = ("c3s1", "c3s2", "c3up", "unshuf", "shuf", "shuf_bias", "c4s2", "c4s1", "c1")
_TAPS = {"c3s1": 3, "c3s2": 3, "c3up": 3, "unshuf": 2, "shuf": 1, "shuf_bias": 1, "c4s2": 4, "c4s1": 4, "c1": 1}


def problem(mode, shape, ldx=0, ldo=0):
    """(descriptor, gathered operand shape, other operand shape, dw shape) of the launch ops.conv_wgrad makes for this layer: the
    layer's own geometry ('linear': token rows; the direct modes), the adjoint problem whose result is folded ('c3up') or transposed
    ('shuf') afterwards, or 'shuf_bias': the c_out = 8 launch of the transposed problem that sums the bias gradient against ones.
    ldx / ldo: extra columns in the rows of the gathered / the other operand."""
    from transvae.hip import ops
    if mode == "linear":
        T, ci, co = shape
        d, xs, gs, dws = ops._rows_desc(T, ci, co), (T, 1, 1, ci), (T, 1, 1, co), (co, 1, 1, ci)
    else:
        B, H, W, ci, co = shape
        k = _TAPS[mode]
        geo = ops._Geo(mode.split("_")[0], torch.empty(B, H, W, ci, device="meta"), torch.empty(co, k, k, ci, device="meta"))
        d = geo.dgrad_desc() if mode in ("c3up", "shuf", "shuf_bias") else geo.fwd_desc(0)
        if mode == "shuf_bias":
            d = ops._desc_like(d, c_out=8, ldo=8)
        xs, gs = (B, d.h_in, d.w_in, d.c_in), (B, d.h_out, d.w_out, d.c_out)
        dws = (d.c_out, d.kh, d.kw, d.c_in)
    if ldx or ldo:
        d = ops._desc_like(d, ldx=d.ldx + ldx, ldo=d.ldo + ldo)
    return d, xs, gs, dws


def valid(mode, shape):
    """the geometry conditions of ops._MODES and the kernels' channel granularity (multiples of 8)"""
    if mode == "linear":
        return True
    B, H, W, ci, co = shape
    if mode in ("c3s2", "unshuf", "c4s2") and (H % 2 or W % 2):
        return False
    if mode in ("shuf", "shuf_bias") and co % 32:
        return False
    return True


@contextlib.contextmanager
def hooks(tn=None, kx3=None):
    """tv_set_wgrad_config(*tn) / tv_set_wgrad_kx3(*kx3) for the block; every hook back at its default on exit"""
    from transvae.hip import _lib as L
    lib = L.load()
    try:
        if tn is not None:
            lib.tv_set_wgrad_config(*tn)
        if kx3 is not None:
            lib.tv_set_wgrad_kx3(*kx3)
        yield
    finally:
        lib.tv_set_wgrad_kx3(2, 0, 0)
        lib.tv_set_wgrad_config(0, 0, 0)
        lib.tv_set_wgrad_stages(0)


def grid():
    """every (mode, shape) of the enumeration: modes x channel pairs x image grids (one and three images) / token counts"""
    for ci, co in itertools.product(CHANNELS, CHANNELS):
        for T in TOKENS:
            yield "linear", (T, ci, co)
        for mode in CONV_MODES:
            for (H, W), B in itertools.product(GRIDS, (1, 3)):
                if valid(mode, (B, H, W, ci, co)):
                    yield mode, (B, H, W, ci, co)


def reachable():
    """(R of the default call, R of the deterministic call with a bias gradient): {kernel: first (mode, shape) that reaches it}.  Also
    checks, over the whole grid, that a deterministic call WITHOUT a bias gradient adds nothing: several chunks run the kernel of the
    call with one, a single chunk runs the default call's kernel (plain stores are already deterministic)."""
    from transvae.hip import ops
    r_def, r_det = {}, {}
    for mode, shape in grid():
        d = problem(mode, shape)[0]
        a, b, c = ops.wgrad_which(d, deterministic=False), ops.wgrad_which(d, deterministic=True), ops.wgrad_which(d, deterministic=True, has_bias=False)
        r_def.setdefault(a["kernel"], (mode, shape))
        r_det.setdefault(b["kernel"], (mode, shape))
        assert (a["ny"], a["chunk_px"], a["plain"]) == (b["ny"], b["chunk_px"], b["plain"]) == (c["ny"], c["chunk_px"], c["plain"]), (mode, shape)
        assert c["kernel"] == (b["kernel"] if c["ny"] > 1 else a["kernel"]), (mode, shape, a, b, c)
    return r_def, r_det


class Case(NamedTuple):
    id: str
    mode: str
    shape: tuple
    opt: dict
    kernel: str
    kernel_det: str


def _tn(tg, tx, bkp, waves, fast, det):
    return f"tn<{tg},{tx}> bkp={bkp} waves={waves} fast={fast} stages=2 det={det}"


def _kx(tg, tx, seg, ring, taps, det):
    return f"kx3<{tg},{tx}> seg={seg} ring={ring} var=4 taps={taps} det={det}"


def _case(id_, mode, shape, k, **opt):
    """k: ('tn', tg, tx, bkp, waves, fast) or ('kx3', tg, tx, seg, ring, taps): the same instantiation in both forms, DET apart"""
    f = _tn if k[0] == "tn" else _kx
    return Case(id_, mode, shape, opt, f(*k[1:], 0), f(*k[1:], 1))


TN, KX = "tn", "kx3"
CASES = [
    # ---- one case per member of R: the single-tap kernel, FAST staging (linear layers; token counts below one K-step, with a K
    # tail, past the chunk < 512 clamp), ragged tiles wherever the tile permits them
    _case("tn64x64-fast-T9", "linear", (9, 40, 24), (TN, 64, 64, 32, 4, 1)),
    _case("tn64x128-fast-T63", "linear", (63, 136, 24), (TN, 64, 128, 32, 4, 1)),
    _case("tn64x192-fast-T65", "linear", (65, 192, 40), (TN, 64, 192, 32, 4, 1)),
    _case("tn128x64-fast-T1", "linear", (1, 40, 136), (TN, 128, 64, 32, 4, 1)),
    _case("tn128x128-fast-T520", "linear", (520, 200, 136), (TN, 128, 128, 32, 4, 1)),
    _case("tn128x192-fast-T1000", "linear", (1000, 192, 160), (TN, 128, 192, 32, 4, 1)),
    _case("tn192x64-fast-T63", "linear", (63, 40, 192), (TN, 192, 64, 64, 4, 1)),
    _case("tn192x128-fast-T65", "linear", (65, 200, 192), (TN, 192, 128, 64, 8, 1)),
    _case("tn192x192-fast-both192", "linear", (1000, 576, 192), (TN, 192, 192, 64, 8, 1)),     # the modelled-time choice; 1000 % 64 != 0
    _case("tn256x256-fast-T520", "linear", (520, 256, 512), (TN, 256, 256, 32, 8, 1)),
    # ---- ... generic staging: grids that are no power of two, the stride-2 modes (their grids must be even; 6 x 10 gives an odd
    # 3 x 5 output), c4s1 at 31 -> 30, the adjoint problems of c3up / shuf and shuf's c_out = 8 bias launch; 1, 9, 63, 65, 520 pixels
    _case("tn64x64-gen-c3s2-M1", "c3s2", (1, 2, 2, 40, 24), (TN, 64, 64, 32, 4, 0)),
    _case("tn64x128-gen-c3up", "c3up", (3, 8, 8, 24, 136), (TN, 64, 128, 32, 4, 0)),
    _case("tn64x192-gen-shuf-bias", "shuf_bias", (3, 6, 10, 64, 768), (TN, 64, 192, 32, 4, 0)),
    _case("tn128x64-gen-c3s2-M9", "c3s2", (1, 6, 6, 40, 136), (TN, 128, 64, 32, 4, 0)),
    _case("tn128x64-gen-shuf", "shuf", (2, 6, 10, 136, 160), (TN, 128, 64, 32, 4, 0)),
    _case("tn128x128-gen-c3s1-M63", "c3s1", (1, 7, 9, 200, 136), (TN, 128, 128, 32, 4, 0)),
    _case("tn128x192-gen-c4s2", "c4s2", (3, 6, 10, 192, 160), (TN, 128, 192, 32, 4, 0)),
    _case("tn192x64-gen-unshuf", "unshuf", (3, 6, 10, 40, 192), (TN, 192, 64, 64, 4, 0)),
    _case("tn192x128-gen-c4s1-31", "c4s1", (1, 31, 31, 136, 192), (TN, 192, 128, 64, 8, 0)),
    _case("tn192x192-gen-c3s1-M65", "c3s1", (1, 5, 13, 192, 192), (TN, 192, 192, 64, 8, 0)),
    _case("tn256x256-gen-c1-M520", "c1", (1, 20, 26, 256, 512), (TN, 256, 256, 32, 8, 0)),
    # ---- ... the kx-triple kernel, both tiles, image widths 16 / 32 / 64 (SEG 16 / 32 / 64): 64, 128 and 192 pixels per launch,
    # fewer K-steps than the ring is deep -- and its one-tap instantiation at one K-step
    _case("kx128-w16-64px", "c3s1", (1, 4, 16, 128, 128), (KX, 128, 128, 16, 4, 3)),
    _case("kx128-w32-128px", "c3s1", (1, 4, 32, 128, 256), (KX, 128, 128, 32, 4, 3)),
    _case("kx128-w64-192px", "c3s1", (3, 1, 64, 256, 128), (KX, 128, 128, 64, 4, 3)),
    _case("kx192-w16-64px", "c3s1", (1, 4, 16, 96, 192), (KX, 192, 96, 16, 3, 3)),
    _case("kx192-w32-128px", "c3s1", (1, 4, 32, 192, 192), (KX, 192, 96, 32, 4, 3)),
    _case("kx192-w64-192px", "c3s1", (3, 1, 64, 96, 384), (KX, 192, 96, 64, 4, 3)),
    _case("tap1-M64", "linear", (64, 192, 192), (KX, 192, 192, 64, 3, 1)),
]
R_CASES = len(CASES)        # the cases above run with every hook at its default: together they are R

CASES += [
    # ---- edges, single-tap kernel: a natural split with a ragged last chunk (M = ny chunk - 8)
    _case("tn192x128-fast-ragged-split", "linear", (1720, 128, 192), (TN, 192, 128, 64, 8, 1)),
    _case("tn128x128-gen-ragged-split", "c3s1", (7, 10, 20, 136, 136), (TN, 128, 128, 32, 4, 0)),
    # XCD-grouped order with ny no multiple of 8 (phantom blocks), forced: the cost model does not choose it at these sizes
    _case("tn128x128-fast-xcd5", "linear", (2568, 200, 136), (TN, 128, 128, 32, 4, 1), tn=(0, 0, 20)),
    _case("tn192x192-gen-xcd3", "c3s1", (3, 20, 26, 192, 192), (TN, 192, 192, 64, 8, 0), tn=(0, 0, 27)),
    _case("tn192x192-fast-c3s1-forced", "c3s1", (1, 16, 64, 192, 192), (TN, 192, 192, 64, 8, 1), tn=(0, 0, 36)),   # a block target switches kx3 off
    # a column range of a wider row (the two-source GEMMs and the qkv thirds hand over such operands)
    _case("tn128x128-fast-ld64", "linear", (65, 200, 136), (TN, 128, 128, 32, 4, 1), ldx=64, ldo=64),
    _case("tn128x128-gen-ld64", "c3s1", (3, 6, 10, 200, 136), (TN, 128, 128, 32, 4, 0), ldx=64, ldo=64),
    # 3x3 on the FAST path (image rows under 16 pixels are not kx3's): the tap shift in the descriptor base
    _case("tn128x128-fast-c3s1-8x8", "c3s1", (2, 8, 8, 136, 160), (TN, 128, 128, 32, 4, 1)),
    _case("tn192x192-fast-c3s1-8x8", "c3s1", (4, 8, 8, 192, 192), (TN, 192, 192, 64, 8, 1)),
    # ---- edges, kx3 3x3: two K-steps per image row (W = 128), three images of one K-step each (every K-step's y-neighbours are
    # another image's rows), a natural split
    _case("kx128-w128-128px", "c3s1", (1, 1, 128, 128, 128), (KX, 128, 128, 64, 4, 3)),
    _case("kx192-w128-256px", "c3s1", (1, 2, 128, 96, 192), (KX, 192, 96, 64, 4, 3)),
    _case("kx128-3img", "c3s1", (3, 4, 16, 128, 128), (KX, 128, 128, 16, 4, 3)),
    _case("kx192-3img", "c3s1", (3, 4, 16, 192, 192), (KX, 192, 96, 16, 3, 3)),
    _case("kx128-w32-natural", "c3s1", (2, 32, 32, 128, 128), (KX, 128, 128, 32, 4, 3)),
    # a ragged last chunk of exactly one K-step in the XCD order with ny = 9, 10, 15 (forced)
    _case("kx128-w16-xcd9-ragged", "c3s1", (65, 4, 16, 128, 128), (KX, 128, 128, 16, 4, 3), kx3=(1, 0, 27)),
    _case("kx128-w64-xcd10-ragged", "c3s1", (73, 1, 64, 128, 128), (KX, 128, 128, 64, 4, 3), kx3=(1, 0, 30)),
    _case("kx192-w16-xcd15-ragged", "c3s1", (113, 4, 16, 96, 192), (KX, 192, 96, 16, 3, 3), kx3=(1, 0, 45)),
    _case("kx128-ld64", "c3s1", (1, 16, 16, 128, 128), (KX, 128, 128, 16, 4, 3), ldx=64, ldo=64),
    _case("kx192-ld64", "c3s1", (1, 8, 32, 96, 192), (KX, 192, 96, 32, 4, 3), ldx=64, ldo=64),
    # ---- edges, kx3 one-tap <192,192>: M = 64 and 64 x 9, with and without bias, natural and forced splits
    _case("tap1-M64-nobias", "linear", (64, 192, 192), (KX, 192, 192, 64, 3, 1), bias=False),
    _case("tap1-M576", "linear", (576, 384, 192), (KX, 192, 192, 64, 3, 1)),
    _case("tap1-M576-nobias", "linear", (576, 384, 192), (KX, 192, 192, 64, 3, 1), bias=False),
    _case("tap1-M576-forced2", "linear", (576, 384, 192), (KX, 192, 192, 64, 3, 1), kx3=(2, 0, 4)),
    _case("tap1-M576-forced2-nobias", "linear", (576, 384, 192), (KX, 192, 192, 64, 3, 1), kx3=(2, 0, 4), bias=False),
    _case("tap1-M576-forced-xcd", "linear", (576, 384, 192), (KX, 192, 192, 64, 3, 1), kx3=(2, 0, 16)),
    _case("tap1-M4096-natural", "linear", (4096, 384, 192), (KX, 192, 192, 64, 3, 1)),
]
# what the plan must say for the cases that exist for a particular launch shape: id -> (ny, xcd_order, pixels of the last chunk)
PLANS = {
    "tn128x128-fast-xcd5": (5, 1, 2568 - 4 * 544),
    "tn192x192-gen-xcd3": (3, 1, 1560 - 2 * 576),
    "tn192x192-fast-c3s1-forced": (2, 1, 512),
    "kx128-w16-xcd9-ragged": (9, 1, 64),
    "kx128-w64-xcd10-ragged": (10, 1, 64),
    "kx192-w16-xcd15-ragged": (15, 1, 64),
    "tap1-M576-forced2": (2, 0, 64),
    "tap1-M576-forced2-nobias": (2, 0, 64),
    "tap1-M576-forced-xcd": (2, 1, 64),
}


def plan(case, deterministic=False):
    """(descriptor, operand shapes, dw shape, the query's answer) for a case, under its hooks"""
    from transvae.hip import ops
    d, xs, gs, dws = problem(case.mode, case.shape, case.opt.get("ldx", 0), case.opt.get("ldo", 0))
    with hooks(case.opt.get("tn"), case.opt.get("kx3")):
        w = ops.wgrad_which(d, deterministic=deterministic, has_bias=case.opt.get("bias", True))
    return d, xs, gs, dws, w


def expected_kernel(case, deterministic, ny):
    """a one-chunk deterministic call without a bias gradient is the default call's plain store"""
    if deterministic and not (ny == 1 and not case.opt.get("bias", True)):
        return case.kernel_det
    return case.kernel


def wgrad_ref64(x, gy, kh, kw, stride, pad, up):
    """fp64 dw[co][ky][kx][ci] = sum_p gy[p][co] x_gathered[p][ky][kx][ci] of the descriptor's gather (nearest x2 upsampling, zero
    padding, stride) and the same sum of absolute values; x [B, H, W, Ci], gy [B, Ho, Wo, Co] -> ([Co, kh, kw, Ci], same)"""
    B, Ho, Wo, Co = gy.shape

    def one(xx, gg):
        xu = xx.repeat_interleave(2, 1).repeat_interleave(2, 2) if up else xx
        hn, wn = (Ho - 1) * stride + kh, (Wo - 1) * stride + kw
        xp = torch.zeros(B, max(hn, xu.shape[1] + 2 * pad), max(wn, xu.shape[2] + 2 * pad), xx.shape[-1], dtype=F64)
        xp[:, pad:pad + xu.shape[1], pad:pad + xu.shape[2]] = xu
        g2 = gg.reshape(-1, Co)
        dw = torch.empty(Co, kh, kw, xx.shape[-1], dtype=F64)
        for ky in range(kh):
            for kx in range(kw):
                xs = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
                dw[:, ky, kx] = g2.t() @ xs.reshape(-1, xx.shape[-1])
        return dw
    x, gy = x.to(F64), gy.to(F64)
    return one(x, gy), one(x.abs(), gy.abs())
