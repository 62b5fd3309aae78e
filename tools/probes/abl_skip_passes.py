"""UPPER BOUNDS on two fusions that are not built ("Upper bounds on the two north-star fusions"): the
benchmark with one HBM pass REMOVED, i.e. with the fusion's work for free.

RESULTS ARE WRONG BY CONSTRUCTION.  Only images/s is read; losses, gradients and anything else the run prints mean nothing.

    python tools/probes/abl_skip_passes.py gn_stats    [bench.py arguments]
    python tools/probes/abl_skip_passes.py rownorm_fwd [bench.py arguments]

  gn_stats     no tv_gn_stats pass in the block Functions: the statistics are a cached constant (mean = the pivot pixel,
               variance 1) -- what GroupNorm statistics in the producing convolution's epilogue could save AT MOST
  rownorm_fwd  no x-hat pass in front of the QKV / Conv-FFN projections: the first x-hat of a shape is reused (finite,
               wrong) -- what x-hat inside the GEMM could save at most

The package has no switch for this; the two functions the block Functions call (fused.gn_silu_fwd, fused.rownorm_fwd) are
replaced from here, then bench.main() runs.  Compare against plain bench.py runs on the same box, alternating.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepl-project_amd")]
from transvae.hip import _lib as L, fused   # noqa: E402
from transvae.hip.ops import _p, _stream     # noqa: E402

_cache = {}


def gn_silu_fwd_without_stats(x, gamma, beta, groups, eps):
    B, H, W, Cc = x.shape
    key = ("gn", B, H * W, Cc, x.device)
    stats = _cache.get(key)
    if stats is None:
        stats = torch.zeros((B, Cc, 2), dtype=torch.float32, device=x.device)
        stats[..., 1] = float(H * W)
        _cache[key] = stats
    mr = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    L.check(L.load().tv_gn_silu_fwd(_p(x), _p(stats), _p(gamma), _p(beta), _p(mr), _p(y), B, H * W, Cc, groups, eps, _stream()),
            "tv_gn_silu_fwd")
    return y, mr


_rownorm_fwd = fused.rownorm_fwd


def rownorm_fwd_first_only(x, w, norm, eps_rms, eps_ln):
    key = ("rownorm", tuple(x.shape), norm, x.device)
    y = _cache.get(key)
    if y is None:
        y = _cache[key] = _rownorm_fwd(x, w, norm, eps_rms, eps_ln)
    return y


if __name__ == "__main__":
    which = sys.argv.pop(1) if len(sys.argv) > 1 else None
    if which == "gn_stats":
        fused.gn_silu_fwd = gn_silu_fwd_without_stats
    elif which == "rownorm_fwd":
        fused.rownorm_fwd = rownorm_fwd_first_only
    else:
        raise SystemExit(__doc__)
    print(f"abl_skip_passes: {which} pass removed -- results are wrong by construction, read the step time only", flush=True)
    import bench
    bench.main()
