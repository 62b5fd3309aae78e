"""Launch transcripts of the op layer (transvae/hip/ops.py, fused.py, and the qk-norm attention of transvae/lightning_dit.py),
recorded on the CPU.

The library is replaced by a recorder: every entry point appends (name, arguments) to a list and returns 0, so the whole
op layer -- descriptors, chunking, caches, in-place accumulation -- runs on CPU tensors and what it WOULD launch can be
compared record by record against tests/golden/op_launch_transcripts.json.  Nothing is computed; tensor contents are
whatever torch.empty left.

A record is [entry name, arg, arg, ...].  Integers and floats are written as they are, a ConvDesc as a dict of its fields,
a pointer as None, as "label+byte offset" when it falls inside a tensor the case created itself (inputs, parameters and
their .grad), or as "tmp" (anything the op layer allocated: outputs, packed operands, scratch).

Only these points of the op layer are touched: _lib.load, _lib.check, ops._need_gpu, the stream / current-device queries,
ops._LAUNCH_BYTES (chunking cases), ops.C4S2_DGRAD_FORM, ops.acc_stats and ops.in_place_params.  The file therefore
records any revision of the op layer that keeps its public surface;  `python tests/launch_transcript.py OUT.json` writes
the transcripts of the tree it is run in.
"""
import ctypes as C
import json
import os
import sys
import types

import torch

BF = torch.bfloat16
GELU, SILU, DERIV, SAVE_DERIV = 1, 2, 3, 16          # _lib.ACT_*
MODES = ("linear", "c3s1", "c3s2", "c3up", "unshuf", "shuf", "c4s2", "c4s1", "c3v1", "c3v2", "c5s1", "c1")
TRAINABLE = MODES[:8]
TAPS = {"linear": None, "c3s1": 3, "c3s2": 3, "c3up": 3, "unshuf": 2, "shuf": 1, "c4s2": 4, "c4s1": 4, "c3v1": 3, "c3v2": 3,
        "c5s1": 5, "c1": 1}
NEEDS_EVEN = ("c3s2", "unshuf", "c4s2")


class Recorder:
    """Stands in for the ctypes library: every attribute is a function that records its call."""

    def __init__(self):
        self.records = []
        self.labels = []              # (label, tensor), in the order the case created them
        self.cat2_unsupported = False

    def label(self, name, t):
        self.labels.append((name, t))
        return t

    def _ptr(self, addr):
        if not addr:
            return None
        for name, t in self.labels:
            for suffix, u in (("", t), (".grad", t.grad if t.is_leaf else None)):
                if u is not None and u.numel() and 0 <= addr - u.data_ptr() < u.numel() * u.element_size():
                    return f"{name}{suffix}+{addr - u.data_ptr()}"
        return "tmp"

    def _arg(self, a):
        if hasattr(a, "_obj"):        # ctypes.byref(...)
            a = a._obj
        if isinstance(a, C.Structure):
            return {f: int(getattr(a, f)) for f, _ in a._fields_}
        if isinstance(a, C.c_void_p):
            return self._ptr(a.value)
        if a is None or isinstance(a, float):
            return a
        if isinstance(a, (bool, int)):
            return int(a)
        raise TypeError(f"unexpected launch argument {a!r}")

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            self.records.append([name] + [self._arg(a) for a in args])
            return 4 if (name == "tv_igemm_nt_cat2" and self.cat2_unsupported) else 0
        return entry


def install(monkeypatch):
    """Patch the library out; returns (recorder, ops, fused)."""
    from transvae.hip import _lib, fused, ops
    rec = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, what="": None)
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    if hasattr(fused, "_stream"):
        monkeypatch.setattr(fused, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: None)
    monkeypatch.setattr(ops, "acc_stats", {"in_place": 0, "autograd": 0})      # fresh counters for the case, the session's restored after it
    monkeypatch.setattr(ops, "in_place_params", set())
    return rec, ops, fused


# ---- tensors ----------------------------------------------------------------------------------------------------------------
def act(rec, name, *shape, grad=False):
    return rec.label(name, torch.zeros(shape, dtype=BF).requires_grad_(grad))


def par(rec, name, *shape, grad=True, with_grad=False):
    p = torch.nn.Parameter(torch.zeros(shape, dtype=torch.float32), requires_grad=grad)
    if with_grad:
        p.grad = torch.zeros_like(p)
    return rec.label(name, p)


def buf(rec, name, *shape):
    return rec.label(name, torch.zeros(shape, dtype=torch.float32))


def layer(rec, mode, H, W, Cin=32, Cout=64, B=2):
    if mode == "linear":
        return act(rec, "x", B * H * W, Cin), par(rec, "w", Cout, Cin)
    k = TAPS[mode]
    return act(rec, "x", B, H, W, Cin), par(rec, "w", Cout, k, k, Cin)


def grids(mode):
    return [(6, 8)] if mode in NEEDS_EVEN else [(5, 7), (6, 8)]


# ---- cases ------------------------------------------------------------------------------------------------------------------
def case_fwd_desc(rec, ops, fused):
    for mode in MODES:
        for H, W in grids(mode) + ([(8, 9)] if mode == "c3v2" else []):
            x, w = layer(rec, mode, H, W, Cout=128 if mode == "shuf" else 64)
            g = ops._Geo(mode, x, w)
            geo = [g.mode, g.B, g.H, g.W, g.Cin, g.Cout, g.KH, g.KW, g.Ho, g.Wo, list(g.out_shape)]
            for a in (0, GELU, GELU | SAVE_DERIV):
                rec.records.append(["fwd_desc", geo, a, rec._arg(g.fwd_desc(a))])


def _layer_case(mode, H, W, form=None):
    def run(rec, ops, fused):
        if form is not None:
            ops.C4S2_DGRAD_FORM = form
        x, w = layer(rec, mode, H, W, Cout=128 if mode == "shuf" else 64)
        b = par(rec, "b", w.shape[0])
        out, pre, g, wc = ops.conv_forward(x, w, b, None, mode, GELU, "deriv")
        gz = act(rec, "gz", *out.shape)
        ops.conv_dgrad(g, wc, gz, x.shape)
        ops.conv_dgrad(g, wc, gz, x.shape, residual=act(rec, "dres", *x.shape), aux=act(rec, "aux", *x.shape), aux_act=DERIV)
        ops.conv_wgrad(g, wc, x, gz, True)
        ops.conv_wgrad(g, wc, x, gz, False)
        if mode == "c3up":
            ops.conv_wgrad(g, wc, x, gz, True, out=(buf(rec, "dw", *w.shape), buf(rec, "db", w.shape[0])), accumulate=True)
        elif mode != "shuf":
            ops.conv_wgrad(g, wc, x, gz, True, out=ops.conv_wgrad_alloc(g, wc, True, x, gz))
        ops.conv_forward(x, w, None, act(rec, "res", *out.shape), mode, 0, False)
    return run


def case_linear_rope(rec, ops, fused):
    N = 16
    x, w = act(rec, "x", 2 * N, 64), par(rec, "w", 192, 64)
    tab = rec.label("tab", torch.zeros((N, 4, 32)))
    ops.conv_forward(x, w, par(rec, "b", 192), None, "linear", 0, False, rope=(tab, N, 64))


def case_forward_only_dgrad(rec, ops, fused):
    """conv_dgrad raises on the four Inception modes; only the error is part of the contract (launches in front of it are not)."""
    for mode in MODES[8:]:
        x, w = layer(rec, mode, 6, 8)
        out, _, g, wc = ops.conv_forward(x, w, None, None, mode, 0, False)
        n = len(rec.records)
        try:
            ops.conv_dgrad(g, wc, torch.zeros_like(out), x.shape)
            err = None
        except Exception as e:      # noqa: BLE001 -- the type and the text are what is compared
            err = [type(e).__name__, str(e)]
        del rec.records[n:]
        rec.records.append(["conv_dgrad raises", mode, err])


def _zero_backward(out):
    out.backward(torch.zeros_like(out))


def _res_args(rec, freeze=False, with_grad=False):
    C_ = 64
    p = lambda n, *s, grad=True: par(rec, n, *s, grad=grad, with_grad=with_grad and grad)   # noqa: E731
    return (act(rec, "x", 2, 4, 4, C_, grad=True), p("g1", C_), p("b1", C_), p("w1", C_, 3, 3, C_, grad=not freeze),
            p("c1b", C_, grad=not freeze), p("g2", C_), p("b2", C_), p("w2", C_, 3, 3, C_), p("c2b", C_), 1e-5, 1e-6)


def _resblock(recompute=False, freeze=False, chunk=False):
    def run(rec, ops, fused):
        if chunk:
            ops._LAUNCH_BYTES = 4 * 4 * 64 * 2 + 1           # one image per launch
        _zero_backward(fused.ResBlockFn.apply(*_res_args(rec, freeze), recompute))
    return run


def case_attn(rec, ops, fused):
    B, N, C_ = 2, 16, 64
    t = act(rec, "t", B * N, C_, grad=True)
    tab = rec.label("tab", torch.zeros((N, 4, 32)))
    _zero_backward(fused.AttnBranchFn.apply(t, par(rec, "w_rms", C_), par(rec, "wqkv", 3 * C_, C_), par(rec, "bqkv", 3 * C_),
                                            par(rec, "wp", C_, C_), par(rec, "bp", C_), tab, B, N, 1, 0.125, 1e-6, 1e-5))


def _attention(hd, table):
    """ops.attention forward and backward on qkv [2, 16, 3 * hd] (one head)."""
    def run(rec, ops, fused):
        B, N = 2, 16
        qkv = act(rec, "qkv", B, N, 3 * hd, grad=True)
        tab = rec.label("tab", torch.zeros((N, 4, hd // 2))) if table else None
        _zero_backward(ops.attention(qkv, tab, 1, 0.125, head_dim=hd))
    return run


def _qk_norm_attention(hd, grad):
    """lightning_dit.qk_norm_rope_attention with a table: raw projections kept and the backward run, or in place under no_grad."""
    def run(rec, ops, fused):
        from transvae import lightning_dit
        B, N = 2, 16
        qkv = act(rec, "qkv", B, N, 3 * hd, grad=grad)
        wq, wk = par(rec, "wq", hd), par(rec, "wk", hd)
        tab = rec.label("tab", torch.zeros((N, 4, hd // 2)))
        if grad:
            _zero_backward(lightning_dit.qk_norm_rope_attention(qkv, wq, wk, tab, 1, 0.125, 1e-6, head_dim=hd))
        else:
            with torch.no_grad():
                lightning_dit.qk_norm_rope_attention(qkv, wq, wk, tab, 1, 0.125, 1e-6, head_dim=hd)
    return run


def _ffn_args(rec, with_grad=False, freeze=False):
    d, hid, mid = 64, 256, 64
    p = lambda n, *s, grad=True: par(rec, n, *s, grad=grad, with_grad=with_grad and grad)   # noqa: E731
    return (act(rec, "t", 32, d, grad=True), p("w_in", hid, d, grad=not freeze), p("b_in", hid, grad=not freeze), p("w1", mid, hid),
            p("b1", mid), p("w2", mid, 3, 3, mid), p("b2", mid), p("w3", hid, mid), p("b3", hid), p("w_out", d, hid), p("b_out", d),
            2, 4, 4, 1e-6)


def _ffn(how="plain"):
    def run(rec, ops, fused):
        rec.cat2_unsupported = how == "cat2_unsupported"
        args = _ffn_args(rec, with_grad=how == "in_place", freeze=how == "frozen")
        once = lambda: _zero_backward(fused.ConvFFNBranchFn.apply(*args))   # noqa: E731
        if how == "cache":
            with ops.packed_weight_cache():
                once()
                once()
        elif how == "in_place":
            with ops.accumulate_grads_in_place(True):
                once()
        elif how == "in_place_cache":      # the shape of a train step: first micro-batch through autograd, second in place
            with ops.packed_weight_cache():
                once()
                with ops.accumulate_grads_in_place(True):
                    once()
        elif how == "defer":
            with ops.defer_chain_grads(True):
                once()
        else:
            once()
    return run


def _down(dc, in_place=False):
    def run(rec, ops, fused):
        C_ = 64
        p = lambda n, *s: par(rec, n, *s, with_grad=in_place)   # noqa: E731
        args = (act(rec, "x", 2, 4, 4, C_, grad=True), p("w0", C_, 3, 3, C_), p("b0", C_), p("w2", C_, 3, 3, C_), p("b2", C_),
                p("wdc", C_, 2, 2, C_) if dc else None, p("bdc", C_) if dc else None)
        with ops.accumulate_grads_in_place(in_place):
            _zero_backward(fused.DownsampleFn.apply(*args))
    return run


def _up(dc, in_place=False):
    def run(rec, ops, fused):
        C_ = 64
        p = lambda n, *s: par(rec, n, *s, with_grad=in_place)   # noqa: E731
        args = (act(rec, "x", 2, 4, 4, C_, grad=True), p("w1", C_, 3, 3, C_), p("b1", C_), p("w3", C_, 3, 3, C_), p("b3", C_),
                p("wdc", 4 * C_, 1, 1, C_) if dc else None, p("bdc", 4 * C_) if dc else None)
        with ops.accumulate_grads_in_place(in_place):
            _zero_backward(fused.UpsampleFn.apply(*args))
    return run


def case_chunk_rope(rec, ops, fused):
    N = 16
    ops._LAUNCH_BYTES = 192 * 2 * N + 1                       # one image of N tokens per launch
    case_linear_rope(rec, ops, fused)


def case_chunk_wgrad(rec, ops, fused):
    x, w = layer(rec, "c3s1", 5, 7)
    g = ops._Geo("c3s1", x, w)
    gy = act(rec, "gy", *g.out_shape)
    ops._LAUNCH_BYTES = 5 * 7 * 64 * 2 + 1
    d = g.fwd_desc(0)
    rec.records.append(["wgrad_plan_desc", rec._arg(ops.wgrad_plan_desc(d, x, gy))])
    ops.wgrad(d, x, gy, buf(rec, "dw", *w.shape), buf(rec, "db", 64))
    ops.wgrad_acc(d, x, gy, rec.labels[-2][1], rec.labels[-1][1])
    ops.conv_wgrad(g, w, x, gy, True)


def _cases():
    cases = {"fwd_desc": case_fwd_desc, "linear_rope": case_linear_rope, "forward_only_dgrad": case_forward_only_dgrad}
    for mode in TRAINABLE:
        for H, W in grids(mode):
            for form in (("polyphase", "dilated") if mode == "c4s2" else (None,)):
                cases[f"layer_{mode}_{H}x{W}" + (f"_{form}" if form else "")] = _layer_case(mode, H, W, form)
    cases.update({
        "resblock": _resblock(), "resblock_recompute": _resblock(recompute=True), "resblock_frozen_w1": _resblock(freeze=True),
        "resblock_recompute_frozen_w1": _resblock(recompute=True, freeze=True), "attn": case_attn,
        "ffn": _ffn(), "ffn_cache_twice": _ffn("cache"), "ffn_in_place": _ffn("in_place"), "ffn_in_place_cache": _ffn("in_place_cache"),
        "ffn_defer_chain": _ffn("defer"), "ffn_cat2_unsupported": _ffn("cat2_unsupported"), "ffn_frozen_w_in": _ffn("frozen"),
        "down": _down(False), "down_dc": _down(True), "down_dc_in_place": _down(True, True),
        "up": _up(False), "up_dc": _up(True), "up_dc_in_place": _up(True, True),
        "chunk_resblock": _resblock(chunk=True), "chunk_rope": case_chunk_rope, "chunk_wgrad": case_chunk_wgrad,
    })
    for hd in (64, 72):
        cases.update({f"attention_hd{hd}": _attention(hd, False), f"attention_hd{hd}_rope": _attention(hd, True),
                      f"qk_norm_attention_hd{hd}": _qk_norm_attention(hd, True), f"qk_norm_attention_hd{hd}_no_grad": _qk_norm_attention(hd, False)})
    return cases


CASES = _cases()


def run_case(name, monkeypatch):
    """The transcript of one case: {"records": [...], "acc_stats": {...}, "in_place_params": n}."""
    rec, ops, fused = install(monkeypatch)
    monkeypatch.setattr(ops, "_LAUNCH_BYTES", ops._LAUNCH_BYTES)        # (restored after the case)
    monkeypatch.setattr(ops, "C4S2_DGRAD_FORM", ops.C4S2_DGRAD_FORM)
    CASES[name](rec, ops, fused)
    return {"records": rec.records, "acc_stats": dict(ops.acc_stats), "in_place_params": len(ops.in_place_params)}


def dumps(transcripts) -> str:
    """One record per line."""
    out = ["{"]
    names = list(transcripts)
    for name in names:
        t = transcripts[name]
        out.append(f' {json.dumps(name)}: {{"acc_stats": {json.dumps(t["acc_stats"])}, "in_place_params": {t["in_place_params"]}, "records": [')
        out.extend("  " + json.dumps(r, separators=(",", ":")) + ("," if i + 1 < len(t["records"]) else "") for i, r in enumerate(t["records"]))
        out.append(" ]}" + ("," if name != names[-1] else ""))
    out.append("}")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "deepl-project_amd")]
    got = {}
    for case in CASES:
        with pytest.MonkeyPatch.context() as mp:
            got[case] = run_case(case, mp)
    with open(sys.argv[1], "w") as f:
        f.write(dumps(got))
    print(sum(len(t["records"]) for t in got.values()), "records in", len(got), "cases")
