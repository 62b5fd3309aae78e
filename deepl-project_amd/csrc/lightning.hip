// The SwiGLU pair of the LightningDiT block (transvae/lightning_dit.py drives it; the token GEMMs and attention are tv_igemm_nt /
// tv_wgrad_tn / tv_attn_*).  DESIGN.md section 3.1 row J holds the rounding contract, section 3.6 the protocol.  The conventions are
// those of dit.hip, which also holds the block's RMSNorm adaLN (tv_adaln_rms_fwd / _bwd, one kernel pair with tv_adaln_fwd / _bwd):
// token matrices are bf16 [B N, C].  The block's per-head qk-norm (tv_qknorm_rope_fwd / _bwd) is qk_norm.hip.
//
//   tv_swiglu_fwd         h = bf16(silu(x1) x2), u = [x1 | x2]
//   tv_swiglu_bwd         du1 = bf16(dh x2 s (1 + x1 (1 - s))), du2 = bf16(dh silu(x1)), s = sigmoid(x1)
//
// Algorithmic bytes per call (what tools/lightning_dit_bench.py divides by kernel time), T = B N rows:
//   tv_swiglu_fwd  6 T Hp                                        tv_swiglu_bwd  10 T Hp
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

// ---- SwiGLU ---------------------------------------------------------------------------------------------------------------------
// s = 1 / (1 + expf(-x1)) with the IEEE division: expf overflows to +inf at x1 < -88.7, where s = 0 and silu = -0, and gives 0 at
// large x1, where s = 1, 1 - s = 0 and the derivative is exactly 1; nothing here forms inf - inf or 0 * inf.
__device__ __forceinline__ float lt_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const bf16* __restrict__ u, bf16* __restrict__ h, long long total, int hch) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / hch;
        const int ch = (int)(idx - row * hch);
        const bf16* __restrict__ ur = u + (row * 2 * hch + ch) * 8;
        const bf16x8 a = *(const bf16x8*)ur, b = *(const bf16x8*)(ur + (size_t)hch * 8);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x1 = (float)a[e];
            o[e] = (bf16)((x1 * lt_sigmoid(x1)) * (float)b[e]);
        }
        *(bf16x8*)(h + idx * 8) = o;
    }
}

__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const bf16* __restrict__ u, const bf16* __restrict__ dh, bf16* __restrict__ du, long long total,
                                                         int hch) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / hch;
        const int ch = (int)(idx - row * hch);
        const size_t off = (size_t)(row * 2 * hch + ch) * 8;
        const bf16x8 a = *(const bf16x8*)(u + off), b = *(const bf16x8*)(u + off + (size_t)hch * 8), d = *(const bf16x8*)(dh + idx * 8);
        bf16x8 o1, o2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x1 = (float)a[e], dv = (float)d[e];
            const float s = lt_sigmoid(x1);
            o1[e] = (bf16)((dv * (float)b[e]) * (s * fmaf(x1, 1.0f - s, 1.0f)));
            o2[e] = (bf16)(dv * (x1 * s));
        }
        *(bf16x8*)(du + off) = o1;
        *(bf16x8*)(du + off + (size_t)hch * 8) = o2;
    }
}

int sw_check(const char* name, long long T, int Hp) {
    if (T <= 0 || Hp <= 0 || Hp % 32 != 0 || T >= (1ll << 31)) {
        tv_set_error("%s: bad shape T=%lld Hp=%d (Hp %% 32 == 0, T < 2^31)", name, T, Hp);
        return TV_ERR_ARG;
    }
    return TV_OK;
}

unsigned sw_blocks(long long total) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace

extern "C" int tv_swiglu_fwd(const void* u, void* h, long long T, int Hp, void* stream) {
    if (sw_check("tv_swiglu_fwd", T, Hp)) return TV_ERR_ARG;
    TV_CHECK_ARG(u && h, "tv_swiglu_fwd: null pointer");
    TV_CHECK_ARG((((uintptr_t)u | (uintptr_t)h) & 15) == 0, "tv_swiglu_fwd: u / h must be 16-byte aligned");
    const long long total = T * (Hp >> 3);
    hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(sw_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)u, (bf16*)h, total, Hp >> 3);
    TV_CHECK_LAUNCH("tv_swiglu_fwd");
    return TV_OK;
}

extern "C" int tv_swiglu_bwd(const void* u, const void* dh, void* du, long long T, int Hp, void* stream) {
    if (sw_check("tv_swiglu_bwd", T, Hp)) return TV_ERR_ARG;
    TV_CHECK_ARG(u && dh && du, "tv_swiglu_bwd: null pointer");
    TV_CHECK_ARG((((uintptr_t)u | (uintptr_t)dh | (uintptr_t)du) & 15) == 0, "tv_swiglu_bwd: u / dh / du must be 16-byte aligned");
    const long long total = T * (Hp >> 3);
    hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(sw_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)u, (const bf16*)dh, (bf16*)du, total, Hp >> 3);
    TV_CHECK_LAUNCH("tv_swiglu_bwd");
    return TV_OK;
}
