// Shared device/host helpers for the TransVAE gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/transvae_hip.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define TV_LDS(ptr) ((__attribute__((address_space(3))) void*)(ptr))
#define TV_GLB(ptr) ((const __attribute__((address_space(1))) void*)(ptr))

// ---------------------------------------------------------------------------
// error plumbing (host)
// ---------------------------------------------------------------------------
void tv_set_error(const char* fmt, ...);
const void* tv_zero_page();  // >= 4 KiB of device zeros (source for padded LDS-DMA lanes)

// Per-device "done once" flag for hipFuncSetAttribute (function attributes are per device: a second GPU in the same
// process needs its own > 64 KiB dynamic-LDS opt-in).  Usage:  static TvPerDeviceOnce once;  if (once.first()) { ... }
struct TvPerDeviceOnce {
    bool done[64] = {};
    bool first() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
        if (done[dev]) return false;
        done[dev] = true;
        return true;
    }
};

#define TV_CHECK_ARG(cond, ...)        \
    do {                               \
        if (!(cond)) {                 \
            tv_set_error(__VA_ARGS__); \
            return TV_ERR_ARG;         \
        }                              \
    } while (0)

#define TV_CHECK_LAUNCH(name)                                                  \
    do {                                                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            tv_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return TV_ERR_LAUNCH;                                              \
        }                                                                      \
    } while (0)

// ---------------------------------------------------------------------------
// activations (device).  erf by Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7),
// i.e. the exact (erf) GELU of the reference to fp32 rounding noise.
// ---------------------------------------------------------------------------
#define TV_ACT_NONE 0
#define TV_ACT_GELU 1
#define TV_ACT_SILU 2
#ifndef TV_ACT_DERIV
#define TV_ACT_DERIV 3        // (aux_act only) the saved tensor already holds act'(pre-activation)
#endif
#ifndef TV_ACT_ADD
#define TV_ACT_ADD 4          // (aux_act only) the second tensor is added: out = acc + residual + aux
#endif
#define TV_ACT_SAVE_DERIV 16  // (flag on desc.act) pre_act receives act'(pre-activation) instead of the pre-activation
// ReLU (frozen VGG layers of the perceptual loss): desc.act, and as aux_act / tv_act_bwd's act with the layer's own OUTPUT as the
// saved tensor (mask = output > 0).  Named outside the TV_ACT_ family on purpose, here and in the public header alike: that
// family is pinned to six ids.
#ifndef TV_ACTX_RELU
#define TV_ACTX_RELU 5
#endif
// LeakyReLU, slope 0.2 (the PatchGAN discriminator, csrc/gan.hip): same rules as TV_ACTX_RELU -- the saved tensor is the layer's
// own bf16 OUTPUT y (slope > 0, so sign(y) = sign(z)) and the factor is y > 0 ? 1 : 0.2.
#ifndef TV_ACTX_LRELU
#define TV_ACTX_LRELU 6
#endif
#define TV_LRELU_SLOPE 0.2f

__device__ __forceinline__ float tv_fast_exp(float x) { return __expf(x); }
// v_rcp_f32 (1 ulp).  `__frcp_rn` compiles to the IEEE-correct division sequence (v_div_scale x2, v_rcp, 4 FMAs, v_div_fmas,
// v_div_fixup: ten instructions) -- it was a third of the GELU / SiLU epilogue arithmetic, which runs with the matrix pipe idle.
__device__ __forceinline__ float tv_fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// erf(x) with e = exp(-x^2) handed back (the Gaussian the GELU gradient needs as well)
__device__ __forceinline__ float tv_erf_e(float x, float& e) {
    const float ax = fabsf(x);
    const float t = tv_fast_rcp(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    p *= t;
    e = tv_fast_exp(-ax * ax);
    const float r = fmaf(-p, e, 1.0f);
    return copysignf(r, x);
}
__device__ __forceinline__ float tv_erf(float x) {
    float e;
    return tv_erf_e(x, e);
}

__device__ __forceinline__ float tv_gelu(float z) { return 0.5f * z * (1.0f + tv_erf(z * 0.70710678118654752f)); }

// d/dz gelu(z) = Phi(z) + z*phi(z);  phi(z) = exp(-z^2/2)/sqrt(2 pi) is the exp(-x^2) of the erf at x = z/sqrt(2): one
// exponential per element (the activation-gradient epilogues are VALU-bound on exactly this arithmetic)
__device__ __forceinline__ float tv_gelu_grad(float z) {
    float e;
    const float cdf = fmaf(0.5f, tv_erf_e(z * 0.70710678118654752f, e), 0.5f);
    return fmaf(z * 0.3989422804014327f, e, cdf);
}

__device__ __forceinline__ float tv_sigmoid(float z) { return tv_fast_rcp(1.0f + tv_fast_exp(-z)); }
__device__ __forceinline__ float tv_silu(float z) { return z * tv_sigmoid(z); }
__device__ __forceinline__ float tv_silu_grad(float z) {
    const float s = tv_sigmoid(z);
    return s * fmaf(z, 1.0f - s, 1.0f);
}

template <int ACT>
__device__ __forceinline__ float tv_act(float z) {
    if constexpr (ACT == TV_ACT_GELU) return tv_gelu(z);
    if constexpr (ACT == TV_ACT_SILU) return tv_silu(z);
    return z;
}
__device__ __forceinline__ float tv_act_rt(int act, float z) {
    if (act == TV_ACT_GELU) return tv_gelu(z);
    if (act == TV_ACT_SILU) return tv_silu(z);
    return z;
}
__device__ __forceinline__ float tv_act_grad_rt(int act, float z) {
    if (act == TV_ACT_GELU) return tv_gelu_grad(z);
    if (act == TV_ACT_SILU) return tv_silu_grad(z);
    return 1.0f;
}
template <int ACT>
__device__ __forceinline__ float tv_act_with_grad(float z, float& g) {
    if constexpr (ACT == TV_ACT_GELU) {
        float e;
        const float cdf = fmaf(0.5f, tv_erf_e(z * 0.70710678118654752f, e), 0.5f);
        g = fmaf(z * 0.3989422804014327f, e, cdf);
        return z * cdf;
    } else if constexpr (ACT == TV_ACT_SILU) {
        const float s = tv_sigmoid(z);
        g = s * fmaf(z, 1.0f - s, 1.0f);
        return z * s;
    } else {
        g = 1.0f;
        return z;
    }
}
// act(z) with its derivative from the same erf / exponential / sigmoid (forward epilogue that saves the derivative)
__device__ __forceinline__ float tv_act_with_grad_rt(int act, float z, float& g) {
    if (act == TV_ACT_GELU) {
        float e;
        const float cdf = fmaf(0.5f, tv_erf_e(z * 0.70710678118654752f, e), 0.5f);
        g = fmaf(z * 0.3989422804014327f, e, cdf);
        return z * cdf;
    }
    if (act == TV_ACT_SILU) {
        const float s = tv_sigmoid(z);
        g = s * fmaf(z, 1.0f - s, 1.0f);
        return z * s;
    }
    g = 1.0f;
    return z;
}

// ---------------------------------------------------------------------------
// LDS-DMA through a buffer descriptor (SGPR base + 32-bit per-lane offset + scalar offset)
// ---------------------------------------------------------------------------
constexpr int OOB_OFFSET = (int)0x80000000u;  // beyond any < 2 GiB buffer: the LDS-DMA writes zeros (probed: tools/probes)

// lds[base + lane*16] = buf[voff + soff .. +16), or zeros if that range is outside [0, bytes).
// The descriptor type only exists in the device pass (a kernel body naming it loses its host stub), hence the guard.
__device__ __forceinline__ void buffer_load_lds16(const void* base, unsigned bytes, char* lds, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000),
                                             TV_LDS(lds), 16, voff, soff, 0, 0);
#endif
}

// ---------------------------------------------------------------------------
// waits and transposed LDS reads shared by the MFMA kernels
// ---------------------------------------------------------------------------
// counted wait: at most N of this wave's vector-memory instructions (LDS-DMA pieces, loads, stores) still in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// ds_read_b64_tr_b16 through inline asm: with the builtin, hipcc (ROCm 7.2) puts an s_waitcnt vmcnt(0) in front of every
// transposed read while an LDS-DMA is in flight (it does not for plain ds_read_b128), which serialises the DMA ring with
// compute.  An asm read is invisible to that pass; callers wait for its completion with lds_wait_all() before use
// (cdna_hip_programming.md section 5.7, rule 18).
__device__ __forceinline__ bf16x4 lds_tr16(unsigned lds_addr) {
    bf16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(lds_addr) : "memory");
    return r;
}
// (the asm read has no compiler-visible addressing mode: a compile-time part of the address goes into its offset field by hand)
template <int OFF>
__device__ __forceinline__ bf16x4 lds_tr16_imm(unsigned lds_addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
    bf16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "n"(OFF) : "memory");
    return r;
}
__device__ __forceinline__ void lds_wait_all() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// f(integral_constant<int, I>) for I = 0 .. N-1: an unrolled loop whose index is usable as a template argument
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// ---------------------------------------------------------------------------
// wave / block reductions (wave = 64 lanes)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float tv_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float tv_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

static inline int tv_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
