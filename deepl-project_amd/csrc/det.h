// Host-side plumbing of the deterministic parameter-gradient paths, shared by wgrad_tn.hip, wgrad_kx3.hip,
// norm.hip and det_reduce.hip.
#pragma once
#include "common.h"

// One deterministic weight-gradient call.  The launch code that settles the split fills `ny` and `need`; with more than one
// pixel chunk it redirects the kernel to the workspace: [ny][c_out * taps * c_in] weight slices, then [ny][c_out] bias slices.
struct TvDetCtx {
    float* ws = nullptr;
    long long ws_bytes = 0;
    int ny = 0;                 // out: pixel chunks of the launch
    long long dw_elems = 0;     // out: elements of one weight slice
    int c_out = 0;              // out: elements of one bias slice
    long long need = 0;         // out: workspace bytes the launch needs (0 with one chunk)
};

// The kernel a weight-gradient call picks (tv_wgrad_tn_which, wgrad_tn.hip).  While g_wgrad_pick is set, a plan-only walk goes on
// past the split to the launch site -- launch_st<> / kx3_launch_v<> -- which records its template arguments here instead of launching.
struct TvWgradPick {
    int has_bias = 0;           // in: the call would carry a dbias (a one-chunk deterministic call without one runs the default form)
    int family = 0;             // out: 0 = nothing recorded, 1 = wgrad_tn_kernel, 2 = wgrad_kx3_kernel
    int tg = 0, tx = 0, det = 0;
    int bkp = 0, waves = 0, fast = 0, stages = 0;      // tn
    int seg = 0, ring = 0, var = 0, taps = 0;          // kx3
    int ny = 0, chunk_px = 0, plain = 0, xcd_order = 0;
};
extern TvWgradPick* g_wgrad_pick;

inline long long tv_det_need(int ny, long long dw_elems, int c_out) { return ny > 1 ? (long long)ny * (dw_elems + c_out) * 4 : 0; }

// out[i] = (accum ? out[i] : nothing) + (P_0[i] + P_1[i] + ... in slice order); no argument checks, no tv_init (det_reduce.hip)
int tv_reduce_slices_launch(const float* part, int n_slices, long long n, long long slice_stride, float* out, int accum, hipStream_t s);
