"""Row W of the rounding contract reaches every weight-gradient kernel the dispatch can pick -- the host half:
the reachable set R from the plan-only query (tv_wgrad_tn_which: host arithmetic, no GPU), set equality between R and the case table
of tests/wgrad_matrix_cases.py in both forms, the conditions the table must meet, which kernel the shapes of test_wgrad_widths run,
and mutation tests that show what row W's element-wise bound rejects and the old whole-tensor rel-L2 < 1e-2 passed."""
import pytest
import torch

import wgrad_matrix_cases as M
from test_error_budget_host import F64, WGRAD_C, check_fp32, r16, rel_l2


@pytest.fixture(scope="module")
def reach():
    return M.reachable()


def test_reachable_set_is_printed_and_covered_by_the_table(reach):
    """R: every kernel the query names over modes x channel counts x grids / token counts with all hooks at their defaults, for the
    default and for the deterministic call.  The hook-free cases of the table reach exactly R: a change to the dispatch that opens a
    new kernel fails here until a case is added."""
    r_def, r_det = reach
    for name, r in (("default", r_def), ("deterministic", r_det)):
        print(f"[wgrad-matrix] R, {name} call: {len(r)} kernels")
        for k in sorted(r):
            print(f"[wgrad-matrix]   {k}    first reached by {r[k]}")
    free = [c for c in M.CASES[:M.R_CASES]]
    assert all(not (c.opt.get("tn") or c.opt.get("kx3")) for c in free)
    got_def = {M.plan(c)[4]["kernel"] for c in free}
    got_det = {M.plan(c, True)[4]["kernel"] for c in free}
    assert got_def == set(r_def), (sorted(set(r_def) - got_def), sorted(got_def - set(r_def)))
    assert got_det == set(r_det), (sorted(set(r_det) - got_det), sorted(got_det - set(r_det)))
    assert all(k.endswith("det=0") for k in r_def) and all(k.endswith("det=1") for k in r_det)


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_case_identity_and_conditions(case):
    """the query names the kernel the table lists, in both forms; a forced split keeps chunks of >= 512 pixels; at most 16 chunks
    (the accumulate bound counts one rounding per chunk); the plans the edge cases exist for; the hooks are back at their defaults"""
    from transvae.hip import ops
    d, xs, gs, dws, w = M.plan(case)
    wd = M.plan(case, True)[4]
    assert w["kernel"] == M.expected_kernel(case, False, w["ny"]), (case.id, w)
    assert wd["kernel"] == M.expected_kernel(case, True, wd["ny"]), (case.id, wd)
    assert (w["ny"], w["chunk_px"], w["plain"], w["xcd_order"]) == (wd["ny"], wd["chunk_px"], wd["plain"], wd["xcd_order"])
    m = d.batch * d.h_out * d.w_out
    assert w["chunk_px"] >= 512 and w["ny"] == -(-m // w["chunk_px"]) and w["ny"] <= 16 and w["plain"] == (w["ny"] == 1)
    if case.id in M.PLANS:
        assert (w["ny"], w["xcd_order"], m - (w["ny"] - 1) * w["chunk_px"]) == M.PLANS[case.id], (case.id, w)
    if "ragged-split" in case.id:
        assert w["ny"] > 1 and w["ny"] * w["chunk_px"] - m == 8 and not (case.opt.get("tn") or case.opt.get("kx3")), (case.id, w)
    if "natural" in case.id:
        assert w["ny"] > 1 and not (case.opt.get("tn") or case.opt.get("kx3")), (case.id, w)
    # outside the case's block the same descriptor is back on its hook-free plan
    if case.opt.get("tn") or case.opt.get("kx3"):
        assert ops.wgrad_which(d, deterministic=False) != w


def test_the_query_follows_the_hooks_and_the_plan():
    """the query agrees with tv_wgrad_tn_overwrites and tv_wgrad_tn_plan under default and forced settings, and names the A/B
    variants when their hooks select them (they are not part of R)"""
    from transvae.hip import _lib as L, ops
    lib = L.load()
    d3 = M.problem("c3s1", (4, 64, 64, 128, 128))[0]
    dl = M.problem("linear", (4096, 256, 512))[0]
    for d in (d3, dl):
        for args in (dict(), dict(tn=(0, 0, 1024)), dict(tn=(32, 4, 0)), dict(tn=(0, 0, -1)), dict(kx3=(1, 0, 4096)), dict(kx3=(0, 0, 0))):
            with M.hooks(**args):
                w = ops.wgrad_which(d)
                assert w["plain"] == lib.tv_wgrad_tn_overwrites(d)
                assert w["ny"] == ops.wgrad_det_plan(d)[0]
    with M.hooks(kx3=(1, 13, 0)):
        assert ops.wgrad_which(d3)["kernel"] == "kx3<128,128> seg=64 ring=3 var=4 taps=3 det=0"     # (schedule 1 needs a ring of 4)
    with M.hooks(kx3=(1, 14, 0)):
        assert ops.wgrad_which(d3)["kernel"] == "kx3<128,128> seg=64 ring=4 var=1 taps=3 det=0"
    with M.hooks(kx3=(0, 0, 0)):
        assert ops.wgrad_which(d3)["kernel"] == "tn<128,128> bkp=32 waves=4 fast=1 stages=2 det=0"
    with M.hooks(tn=(0, 0, -1)):
        assert ops.wgrad_which(d3)["kernel"] == "tn<128,128> bkp=32 waves=4 fast=0 stages=2 det=0"
    with M.hooks(tn=(64, 8, -3)):
        assert ops.wgrad_which(dl)["kernel"] == "tn<128,128> bkp=64 waves=8 fast=1 stages=2 det=0"
    assert ops.wgrad_which(d3)["kernel"] == "kx3<128,128> seg=64 ring=4 var=4 taps=3 det=0"
    assert ops.wgrad_which(dl)["kernel"] == "tn<256,256> bkp=32 waves=8 fast=1 stages=2 det=0"
    bad = ops._desc_like(dl, c_in=252)
    with pytest.raises(RuntimeError):
        ops.wgrad_which(bad)


@pytest.mark.parametrize("W", [8, 16, 32, 64, 128])
def test_wgrad_widths_shapes_run_the_single_tap_kernel(W):
    """The widths correction: test_error_budget_gpu.test_wgrad_widths' 128 -> 192 layer is tn<192,128> at every width, 3x3 and linear
    half alike (128 % 96 != 0 and 192 % 128 != 0: neither kx3 tile divides it); the layers added to it resolve to kx3 from W = 16 on,
    3x3 and one-tap"""
    from transvae.hip import ops
    B, H = 4, 64 if W <= 32 else 16
    seg = min(W, 64)
    for ci, co, k3 in ((128, 192, None), (192, 192, f"kx3<192,96> seg={seg} ring={3 if seg == 16 else 4} var=4 taps=3 det=0"),
                       (128, 128, f"kx3<128,128> seg={seg} ring=4 var=4 taps=3 det=0")):
        conv = ops.wgrad_which(M.problem("c3s1", (B, H, W, ci, co))[0])
        lin = ops.wgrad_which(M.problem("linear", (B * H * W, ci, co))[0])
        print(f"[wgrad-matrix] widths W={W} {ci}->{co}: 3x3 {conv['kernel']} ny={conv['ny']}; linear {lin['kernel']} ny={lin['ny']}")
        if k3 is None:
            assert conv["tile"] == lin["tile"] == "tn<192,128>" and conv["fast"] == lin["fast"] == 1
        elif W >= 16:
            assert conv["kernel"] == k3
            assert lin["kernel"] == ("kx3<192,192> seg=64 ring=3 var=4 taps=1 det=0" if ci == 192 else "tn<128,128> bkp=32 waves=4 fast=1 stages=2 det=0")
        else:
            assert conv["family"] == "tn"


# ---------------------------------------------------------------------------------------------------------------------------
# mutations: what row W's bound rejects
# ---------------------------------------------------------------------------------------------------------------------------
def _ratio(y, y64, absterms):
    y, y64 = y.to(F64), y64.to(F64)
    return ((y - y64).abs() / (WGRAD_C * 2.0 ** -24 * absterms + 2.0 ** -24 * y64.abs() + 1e-300)).max().item()


def _gather3(x):
    """[B, H, W, C] -> [B, H, W, 3, 3, C]: the 3x3 / pad-1 gather (zeros outside the image)"""
    B, H, W, Cc = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Cc, dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return torch.stack([torch.stack([xp[:, ky:ky + H, kx:kx + W] for kx in range(3)], 3) for ky in range(3)], 3)


def _problem(case_id):
    case = next(c for c in M.CASES if c.id == case_id)
    d, xs, gs, dws, w = M.plan(case)
    g = torch.Generator().manual_seed(len(case_id))
    x = r16(torch.randn(xs, generator=g, dtype=F64))
    gy = r16(torch.randn(gs, generator=g, dtype=F64) * torch.exp2(torch.randint(-3, 4, (1, 1, 1, gs[-1]), generator=g).to(F64)))
    tail = r16(torch.randn(xs[:-1] + (8,), generator=g, dtype=F64))      # the 8 channels after c_in in a wider row (ldx > c_in)
    return d, x, gy, tail, w


def _mutation_report(name, y, y64, absterms, must_fail=True):
    r, l2 = _ratio(y, y64, absterms), rel_l2(y, y64)
    print(f"[wgrad-matrix] mutation {name}: {r:.3g} x row W's bound, rel-L2 {l2:.3g} ({'passes' if l2 < 1e-2 else 'fails'} a 1e-2 rel-L2 check)")
    if must_fail:
        with pytest.raises(AssertionError):
            check_fp32(y, y64, absterms, WGRAD_C, name)
    else:
        check_fp32(y, y64, absterms, WGRAD_C, name)
    return r, l2


def test_mutations_3x3():
    """On the table's forced kx3 case of 65 images x 4 x 16 pixels, 128 -> 128, nine chunks with a ragged last one of 64 pixels: the
    plain fp32 sum and the chunk partials added in two orders pass; a chunk partial through bf16, a pixel missing from the ragged
    chunk, the last K-step of a chunk counted twice in dbias, the kx = 0 tap at column 0 reading the previous row's last pixel,
    the ky = 0 tap at row 0 reading the previous image's last row, and a channel past c_in entering the sum are rejected"""
    d, x, gy, tail, w = _problem("kx128-w16-xcd9-ragged")
    ny, chunk = w["ny"], w["chunk_px"]
    B, H, W, Ci = x.shape
    Co = gy.shape[-1]
    m = B * H * W
    assert ny == 9 and m - 8 * chunk == 64
    xg = _gather3(x).reshape(m, 9 * Ci)
    g2 = gy.reshape(m, Co)
    dw64, adw = g2.t() @ xg, g2.abs().t() @ xg.abs()
    db64, adb = g2.sum(0), g2.abs().sum(0)
    xg32, g32 = xg.float(), g2.float()
    parts = [(g32[c * chunk:(c + 1) * chunk].t() @ xg32[c * chunk:(c + 1) * chunk]) for c in range(ny)]
    bparts = [g32[c * chunk:(c + 1) * chunk].sum(0) for c in range(ny)]

    def add(ps, order):
        s = torch.zeros_like(ps[0])
        for c in order:
            s = s + ps[c]
        return s
    fwd, rev = list(range(ny)), [8, 3, 5, 0, 7, 1, 6, 2, 4]
    _mutation_report("3x3 clean fp32 sum", g32.t() @ xg32, dw64, adw, must_fail=False)
    _mutation_report("3x3 clean chunks in order", add(parts, fwd), dw64, adw, must_fail=False)
    _mutation_report("3x3 clean chunks reordered", add(parts, rev), dw64, adw, must_fail=False)
    _mutation_report("3x3 clean dbias chunks reordered", add(bparts, rev), db64, adb, must_fail=False)
    out = {}
    # a chunk partial stored through bf16
    out["bf16 partial"] = _mutation_report("3x3 chunk partial through bf16", add([p if c != 4 else r16(p).float() for c, p in enumerate(parts)], fwd), dw64, adw)
    # one pixel of the last, ragged chunk missing
    keep = torch.ones(m, dtype=torch.bool)
    keep[8 * chunk + 37] = False
    out["missing pixel"] = _mutation_report("3x3 pixel missing from the ragged chunk", g32[keep].t() @ xg32[keep], dw64, adw)
    # the last K-step (64 pixels) of chunk 2 counted twice in dbias
    twice = add(bparts, fwd) + g32[3 * chunk - 64:3 * chunk].sum(0)
    out["bias tail twice"] = _mutation_report("3x3 dbias: last K-step of a chunk twice", twice, db64, adb)
    # the kx = 0 tap at column 0 reads the pixel before it in memory (the previous row's last pixel) instead of zero
    bad = _gather3(x).clone()
    for ky in range(3):
        for oy in range(H):
            if 1 <= oy + ky - 1 < H:          # (before row 0 of an image lies another image: the y case below)
                bad[:, oy, 0, ky, 0] = x[:, oy + ky - 2, W - 1]
    out["x wrap"] = _mutation_report("3x3 kx=0 at column 0 reads the previous row", g32.t() @ bad.reshape(m, 9 * Ci).float(), dw64, adw)
    # the ky = 0 tap at row 0 reads the previous image's last row instead of zero
    bad = _gather3(x).clone()
    bad[1:, 0, :, 0, 1] = x[:-1, H - 1]
    out["y wrap"] = _mutation_report("3x3 ky=0 at row 0 reads the previous image", g32.t() @ bad.reshape(m, 9 * Ci).float(), dw64, adw)
    # the channel after c_in (inside ldx) enters the sum of the last channel
    bad = _gather3(x).clone()
    bad[..., Ci - 1] += _gather3(tail)[..., 0]
    out["c_in tail"] = _mutation_report("3x3 channel past c_in enters the sum", g32.t() @ bad.reshape(m, 9 * Ci).float(), dw64, adw)
    assert all(r > 1.0 for r, _ in out.values())


def test_mutations_linear():
    """The mutations that apply to a linear layer, on the table's forced one-tap case of 576 tokens, 384 -> 192, two chunks (512 + 64)"""
    d, x, gy, tail, w = _problem("tap1-M576-forced2")
    ny, chunk = w["ny"], w["chunk_px"]
    m, Ci, Co = x.shape[0], x.shape[-1], gy.shape[-1]
    assert ny == 2 and m - chunk == 64
    x2, g2 = x.reshape(m, Ci), gy.reshape(m, Co)
    dw64, adw = g2.t() @ x2, g2.abs().t() @ x2.abs()
    db64, adb = g2.sum(0), g2.abs().sum(0)
    x32, g32 = x2.float(), g2.float()
    parts = [g32[:chunk].t() @ x32[:chunk], g32[chunk:].t() @ x32[chunk:]]
    _mutation_report("linear clean fp32 sum", g32.t() @ x32, dw64, adw, must_fail=False)
    _mutation_report("linear clean chunks in order", parts[0] + parts[1], dw64, adw, must_fail=False)
    _mutation_report("linear clean chunks reordered", parts[1] + parts[0], dw64, adw, must_fail=False)
    _mutation_report("linear chunk partial through bf16", r16(parts[0]).float() + parts[1], dw64, adw)
    keep = torch.ones(m, dtype=torch.bool)
    keep[chunk + 5] = False
    _mutation_report("linear token missing from the ragged chunk", g32[keep].t() @ x32[keep], dw64, adw)
    _mutation_report("linear dbias: last K-step of a chunk twice", g32.sum(0) + g32[chunk - 64:chunk].sum(0), db64, adb)
    bad = x32.clone()
    bad[:, Ci - 1] += tail.reshape(m, 8)[:, 0].float()
    _mutation_report("linear channel past c_in enters the sum", g32.t() @ bad, dw64, adw)
