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

inline long long tv_det_need(int ny, long long dw_elems, int c_out) { return ny > 1 ? (long long)ny * (dw_elems + c_out) * 4 : 0; }

// out[i] = (accum ? out[i] : nothing) + (P_0[i] + P_1[i] + ... in slice order); no argument checks, no tv_init (det_reduce.hip)
int tv_reduce_slices_launch(const float* part, int n_slices, long long n, long long slice_stride, float* out, int accum, hipStream_t s);
