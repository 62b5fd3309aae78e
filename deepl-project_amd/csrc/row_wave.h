// One wave per token row: the core shared by the row norms (norm.hip) and the adaLN kernels (dit.hip).
//
// A 64-lane wave holds a row of C = 8 nch elements in registers as float v[KCH][8]; lane l owns the 16-byte chunks l + 64 k, k < KCH,
// and the chunks at or past nch hold zeros.  Every chain runs k outer, e inner, and every sum ends in tv_wave_sum.
//
// NOTHING HERE MAY BE CONTRACTABLE: norm.hip compiles with the default contraction, dit.hip with `fp contract(off)`, and each
// kernel's rounding contract follows its own file.  A multiply-add in this header is an
// explicit fmaf or it is absent; expressions such as `sum * inv_c + eps` or `(v - mu) * s` belong to the kernels, and the functor
// of rw_store is written there too, so it keeps its file's mode.  A bare add or subtract here can still fuse with a PRODUCT the
// calling kernel hands it where that kernel contracts: rw_sum and rw_centre take loaded rows (and a mean), never a row of products
// -- mode 1 of the row norms keeps its own chains over u = (x r) w for that reason.  tools/row_kernel_digests.py hashes every
// output of the kernels built on this header: run it against the previous library when anything here changes.
#pragma once
#include "common.h"

template <int KCH>
__device__ __forceinline__ void rw_load(const bf16* __restrict__ row, int lane, int nch, float (&v)[KCH][8]) {
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
        bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ch < nch) t = *(const bf16x8*)(row + ch * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[k][e] = (float)t[e];
    }
}

// a per-channel fp32 vector (w, shift, or 1 + scale with ONE_PLUS) in the row's layout, `fill` in the lanes past the row
template <int KCH, bool ONE_PLUS = false>
__device__ __forceinline__ void rw_load_cols(const float* __restrict__ p, int lane, int nch, float fill, float (&o)[KCH][8]) {
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[k][e] = fill;
        if (ch < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[k][e] = ONE_PLUS ? 1.0f + p[ch * 8 + e] : p[ch * 8 + e];
        }
    }
}

template <int KCH>
__device__ __forceinline__ float rw_sum(const float (&v)[KCH][8]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KCH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[k][e];
    return tv_wave_sum(s);
}

template <int KCH>
__device__ __forceinline__ float rw_sumsq(const float (&v)[KCH][8]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KCH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(v[k][e], v[k][e], s);
    return tv_wave_sum(s);
}

// v -= mu in the row, 0 in the lanes past it; returns the row's sum of squared deviations
template <int KCH>
__device__ __forceinline__ float rw_centre(float (&v)[KCH][8], int lane, int nch, float mu) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[k][e] = (ch < nch) ? v[k][e] - mu : 0.f;
            s = fmaf(v[k][e], v[k][e], s);
        }
    }
    return tv_wave_sum(s);
}

// dst[off + 8 ch + e] = bf16(f(k, e, res)) for the chunks of the row at element offset `off`; res = the matching element of `res`
// (0 when the pointer is null: the forward passes nullptr, the backward its optional dres)
template <int KCH, class F>
__device__ __forceinline__ void rw_store(bf16* __restrict__ dst, const bf16* __restrict__ res, size_t off, int lane, int nch, F f) {
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
        if (ch < nch) {
            bf16x8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (res) rv = *(const bf16x8*)(res + off + ch * 8);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)f(k, e, (float)rv[e]);
            *(bf16x8*)(dst + off + ch * 8) = o;
        }
    }
}

// f(std::integral_constant<int, K>) for the first K of the list with kch <= K (the last one otherwise): chunks per lane -> KCH
template <int K0, int... KS, class F>
inline void rw_dispatch(int kch, F&& f) {
    if constexpr (sizeof...(KS) == 0) f(std::integral_constant<int, K0>{});
    else if (kch <= K0) f(std::integral_constant<int, K0>{});
    else rw_dispatch<KS...>(kch, f);
}
