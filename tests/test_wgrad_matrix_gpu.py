"""Row W of the rounding contract on every weight-gradient kernel the dispatch can pick -- the GPU half.  Each
case of tests/wgrad_matrix_cases.py (one per member of the reachable set R, plus the edges where such kernels break; the host file
tests/test_wgrad_matrix_host.py shows that the table covers R) runs one layer through ops.wgrad / ops.wgrad_acc and asserts

  identity    the plan-only query names the kernel the table lists, for the default and for the deterministic call;
  bounds      |dw - dw64| <= 16 2^-24 sum|x g| + 2^-24 |dw64| and the same for dbias with sum|g| -- the default call twice (atomics
              reorder the sums), the deterministic call twice (same bits) -- against the descriptor's own gather in fp64;
  guards      x and gy are views inside NaN-filled allocations (rows before and after, and the columns between c and ld where the
              case has ld > c): a padded K column or a row past M read into an MFMA gives NaN; dw and dbias are views inside buffers
              whose guard words must come back untouched.  Reading a guard is ordinary memory inside the same allocation;
  plain       where tv_wgrad_tn_overwrites answers 1, dw is handed in full of NaN and must come back finite; else zeros;
  accumulate  onto dw = 0.5, dbias = -0.25: 2^-24 (16 sum|x g| + ny |base|) + 2^-24 |result| -- row W for the sum plus one rounding
              at magnitude <= |base| + sum|x g| for each of the ny chunk adds; in the deterministic form bit-equal to base + S.

Inputs are bf16-exact, gy scaled per output channel by 2^k, k in -3 .. 3.  Every hook a case sets is restored in a `finally`
(wgrad_matrix_cases.hooks)."""
import pytest
import torch

import wgrad_matrix_cases as M
from test_error_budget_host import BF, F64, WGRAD_C, check_fp32, r16

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 0x7FC0DEAD            # the guard word of the output buffers (as fp32: a NaN with a payload no kernel produces)
OUT_GUARD = 64                # guard words before and after dw / dbias
WORST = {}                    # kernel (+ " accumulate" for the wgrad_acc call) -> worst ratios (dw, dbias) over the cases run so far


def dev():
    return torch.device("cuda:0")


def report(tag, val):
    print(f"[error-budget] {tag}: {val}")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded_in(t64, ld, guard_rows):
    """[rows, c] fp64 -> (the NaN-filled [guard + rows + guard, ld] bf16 allocation, its [rows, c] view)"""
    rows, c = t64.shape
    big = torch.full((2 * guard_rows + rows, ld), NAN, dtype=BF, device=dev())
    view = big[guard_rows:guard_rows + rows, :c]
    view.copy_(t64.to(BF))
    return big, view


class _Out:
    """an fp32 output of `shape` as a view inside a buffer of guard words"""

    def __init__(self, shape):
        n = 1
        for v in shape:
            n *= v
        self.n = n
        self.buf = torch.full((2 * OUT_GUARD + n,), GUARD, dtype=torch.int32, device=dev())
        self.view = self.buf[OUT_GUARD:OUT_GUARD + n].view(torch.float32).view(shape)

    def fill(self, v):
        self.view.fill_(v)
        return self.view

    def take(self, what):
        b = self.buf.cpu()
        assert bool((b[:OUT_GUARD] == GUARD).all()) and bool((b[OUT_GUARD + self.n:] == GUARD).all()), f"{what}: a guard word changed"
        return self.view.cpu().clone()


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_wgrad_kernel_holds_row_w(case):
    from transvae.hip import _lib as L, ops
    lib = L.load()
    d, xs, gs, dws = M.problem(case.mode, case.shape, case.opt.get("ldx", 0), case.opt.get("ldo", 0))
    bias = case.opt.get("bias", True)
    co = dws[0]
    g = torch.Generator().manual_seed(sum(case.shape) + len(case.id))
    x = r16(torch.randn(xs, generator=g, dtype=F64))
    gy = r16(torch.randn(gs, generator=g, dtype=F64) * torch.exp2(torch.randint(-3, 4, (1, 1, 1, gs[-1]), generator=g).to(F64)))
    rows_guard = 2 * max(d.w_in, d.w_out) + 80
    x_big, xv = _guarded_in(x.reshape(-1, xs[-1]), d.ldx, rows_guard)
    g_big, gv = _guarded_in(gy.reshape(-1, gs[-1]), d.ldo, rows_guard)
    dw_o, db_o = _Out(dws), _Out((co,))
    runs = {}
    with M.hooks(case.opt.get("tn"), case.opt.get("kx3")):
        w = ops.wgrad_which(d, deterministic=False, has_bias=bias)
        wd = ops.wgrad_which(d, deterministic=True, has_bias=bias)
        over = lib.tv_wgrad_tn_overwrites(d)
        for form in ("default#0", "default#1", "det#0", "det#1"):
            with ops.deterministic(form.startswith("det")):
                dw_o.fill(NAN if (over == 1 or form.startswith("det")) else 0.0)
                db_o.fill(0.0)
                ops.wgrad(d, xv, gv, dw_o.view, db_o.view if bias else None)
                runs[form] = (dw_o.take(f"{form} dw"), db_o.take(f"{form} dbias"))
        for form in ("default", "det"):
            with ops.deterministic(form == "det"):
                dw_o.fill(0.5)
                db_o.fill(-0.25)
                ops.wgrad_acc(d, xv, gv, dw_o.view, db_o.view if bias else None)
                runs[form + "+acc"] = (dw_o.take(f"{form} accumulate dw"), db_o.take(f"{form} accumulate dbias"))
        torch.cuda.synchronize()
    ny = w["ny"]
    assert w["kernel"] == M.expected_kernel(case, False, ny), w                                     # identity
    assert wd["kernel"] == M.expected_kernel(case, True, ny), wd
    assert over == w["plain"] == wd["plain"] and ny == wd["ny"] <= 16
    # the operands are untouched (a kernel writes neither) and still NaN around the data
    for big, view, t in ((x_big, xv, x), (g_big, gv, gy)):
        assert torch.equal(view.cpu().to(F64), t.reshape(view.shape))
        assert int(torch.isnan(big).sum()) == big.numel() - view.numel()
    dw64, adw = M.wgrad_ref64(x, gy, d.kh, d.kw, d.stride, d.pad, d.up_shift)
    g2 = gy.reshape(-1, co)
    db64, adb = g2.sum(0), g2.abs().sum(0)
    out = {}
    for form in ("default#0", "default#1", "det#0", "det#1"):                                       # bounds, no NaN from a guard
        dw, db = runs[form]
        assert bool(torch.isfinite(dw).all()), f"{case.id} {form}: {int((~torch.isfinite(dw)).sum())} elements of dw are not finite"
        out[f"dw {form}"] = check_fp32(dw, dw64, adw, WGRAD_C, f"{case.id} {form} dw")
        if bias:
            assert bool(torch.isfinite(db).all()), f"{case.id} {form}: dbias is not finite"
            out[f"db {form}"] = check_fp32(db, db64, adb, WGRAD_C, f"{case.id} {form} dbias")
        else:
            assert bool((db == 0).all()), f"{case.id} {form}: dbias written without being asked for"
    assert same_bits(runs["det#0"][0], runs["det#1"][0]), "deterministic dw differs between two runs"
    assert same_bits(runs["det#0"][1], runs["det#1"][1]), "deterministic dbias differs between two runs"
    if ny == 1:            # one chunk: plain stores, the same bits in either form
        assert same_bits(runs["default#0"][0], runs["default#1"][0]) and same_bits(runs["default#0"][0], runs["det#0"][0])
    # accumulate: row W for the sum + one rounding per chunk add
    dwa, dba = runs["default+acc"]
    out["dw acc"] = check_fp32(dwa, 0.5 + dw64, adw + ny * 0.5 / WGRAD_C, WGRAD_C, f"{case.id} accumulate dw")
    assert same_bits(runs["det+acc"][0], 0.5 + runs["det#0"][0]), "deterministic accumulate: dw != 0.5 + S"
    if bias:
        out["db acc"] = check_fp32(dba, -0.25 + db64, adb + ny * 0.25 / WGRAD_C, WGRAD_C, f"{case.id} accumulate dbias")
        assert same_bits(runs["det+acc"][1], -0.25 + runs["det#0"][1]), "deterministic accumulate: dbias != -0.25 + S"
    else:
        assert bool((dba == -0.25).all()) and bool((runs["det+acc"][1] == -0.25).all())
    for kernel, key in ((w["kernel"], "default"), (wd["kernel"], "det"), (w["kernel"] + " accumulate", "acc")):
        now = tuple(max([v for k, v in out.items() if k.startswith(o) and key in k] or [0.0]) for o in ("dw", "db"))
        WORST[kernel] = tuple(max(p, n) for p, n in zip(WORST.get(kernel, (0.0, 0.0)), now))
    report(f"[W] {case.id}: {w['kernel']} / det={wd['det']}, ny {ny} chunk {w['chunk_px']} xcd {w['xcd_order']}",
           {k: round(v, 3) for k, v in out.items()})


def test_wgrad_matrix_report():
    """prints the worst ratio to row W's bound per kernel over the cases that ran in this process (dw, dbias)"""
    for kernel in sorted(WORST):
        report(f"[W] worst ratio, {kernel}", tuple(round(v, 3) for v in WORST[kernel]))
    fam = {}
    for kernel, (rw, rb) in WORST.items():
        key = kernel.split("<")[0] + (" one-tap" if "taps=1" in kernel else "") + (" det" if "det=1" in kernel else "") + (" accumulate" if kernel.endswith("accumulate") else "")
        fam[key] = (max(fam.get(key, (0, 0))[0], rw), max(fam.get(key, (0, 0))[1], rb))
    for key in sorted(fam):
        report(f"[W] worst ratio per family, {key}", tuple(round(v, 3) for v in fam[key]))
