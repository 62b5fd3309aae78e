// LightningDiT block variants of the latent DiT (transvae/lightning_dit.py drives them; the token GEMMs and attention are
// tv_igemm_nt / tv_wgrad_tn / tv_attn_*).  DESIGN.md section 3.1 row J holds the rounding contract, section 3.6 the protocol.  The
// conventions are those of dit.hip, which also holds the block's RMSNorm adaLN (tv_adaln_rms_fwd / _bwd, one kernel pair with
// tv_adaln_fwd / _bwd): token matrices are bf16 [B N, C].
//
//   tv_qknorm_rope_fwd    per (token, head), q and k alike: r = rsqrt(mean_64(q^2) + eps), out = bf16(rope(q r w)); v copied
//   tv_qknorm_rope_bwd    in place on dqkv: dq_raw = bf16(r (g - qh mean_64(g qh))), g = dq w, qh = q r; dw_j = sum dq_j qh_j
//   tv_swiglu_fwd         h = bf16(silu(x1) x2), u = [x1 | x2]
//   tv_swiglu_bwd         du1 = bf16(dh x2 s (1 + x1 (1 - s))), du2 = bf16(dh silu(x1)), s = sigmoid(x1)
//
// Every sum that crosses rows is taken in a fixed order through scratch partials and written: no atomics, the same bits on every
// run.  tv_qknorm_rope_bwd: a head vector is eight lanes; per lane group its vectors in pass order, the 32 groups of a block in order,
// then 64 block lanes (block k in lane k % 64, in order) and the lanes in order.
//
// Algorithmic bytes per call (what tools/lightning_dit_bench.py divides by kernel time), T = B N rows:
//   tv_qknorm_rope_fwd  8 T C in place (12 T C out of place)     tv_qknorm_rope_bwd  12 T C
//   tv_swiglu_fwd  6 T Hp                                        tv_swiglu_bwd  10 T Hp
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int QK_GROUPS = 32;       // head vectors per block pass (256 threads / 8 lanes)
constexpr int QK_MAX_BLOCKS = 1024;
constexpr int QK_FIN_LANES = 64;    // block lanes of the dwq / dwk finalise

// ---- per-head RMSNorm of q and k with the 2-D RoPE ----------------------------------------------------------------------------
__device__ __forceinline__ float group8_sum(float v) {
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// A lane group (eight lanes of 16 bytes) takes one third of one token, unit u = token * nwhich + which, and walks its heads: the
// token's table row is loaded once for all of them (loaded per head vector it is four times the vector's own bytes, and the kernel
// is bound by those loads).  nwhich = 3 out of place (the v third is copied), 2 in place (v stays where it is).
// in and out may alias: a vector belongs to one lane group, which reads it whole (the butterfly needs every lane's load) before
// any of its lanes stores.
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const bf16* in, const float* __restrict__ wq, const float* __restrict__ wk,
                                                              const float* __restrict__ tab, bf16* out, long long units, int nwhich, int N, int heads,
                                                              float eps) {
    const int l8 = threadIdx.x & 7, grp = threadIdx.x >> 3;
    float wqv[8], wkv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        wqv[e] = wq[l8 * 8 + e];
        wkv[e] = wk[l8 * 8 + e];
    }
    for (long long base = (long long)blockIdx.x * QK_GROUPS; base < units; base += (long long)gridDim.x * QK_GROUPS) {   // (block-uniform)
        const long long u = base + grp;
        if (u >= units) continue;                              // (uniform over the lane group: its butterfly stays whole)
        const long long tok = u / nwhich;
        const int which = (int)(u - tok * nwhich);
        const size_t off = ((size_t)(tok * 3 + which) * heads) * 64 + l8 * 8;
        if (which == 2) {                                      // v: bit for bit
            for (int hd = 0; hd < heads; ++hd) *(bf16x8*)(out + off + (size_t)hd * 64) = *(const bf16x8*)(in + off + (size_t)hd * 64);
            continue;
        }
        f32x4 c1 = {1.f, 1.f, 1.f, 1.f}, s1 = {0.f, 0.f, 0.f, 0.f}, c2 = c1, s2 = s1;
        if (tab) {
            const float* tb = tab + (size_t)(tok % N) * 128 + l8 * 4;
            c1 = *(const f32x4*)(tb), s1 = *(const f32x4*)(tb + 32), c2 = *(const f32x4*)(tb + 64), s2 = *(const f32x4*)(tb + 96);
        }
        for (int hd = 0; hd < heads; ++hd) {
            const bf16x8 t = *(const bf16x8*)(in + off + (size_t)hd * 64);
            float x[8], ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                x[e] = (float)t[e];
                ss = fmaf(x[e], x[e], ss);
            }
            const float r = rsqrtf(group8_sum(ss) * (1.0f / 64.0f) + eps);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (x[e] * r) * (which == 0 ? wqv[e] : wkv[e]);
            bf16x8 o;
            if (tab) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float a = x[2 * p], bb = x[2 * p + 1];
                    o[2 * p] = (bf16)(a * c1[p] - bb * s1[p]);
                    o[2 * p + 1] = (bf16)(a * s2[p] + bb * c2[p]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)x[e];
            }
            *(bf16x8*)(out + off + (size_t)hd * 64) = o;
        }
    }
}

// head vector u of the q and k thirds: token = u / (2 heads), which = (u / heads) % 2
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const bf16* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                                              bf16* __restrict__ dqkv, float* __restrict__ part, long long units, int heads, float eps) {
    __shared__ float s_acc[QK_GROUPS][128];
    const int l8 = threadIdx.x & 7, grp = threadIdx.x >> 3;
    float wqv[8], wkv[8], aq[8], ak[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        wqv[e] = wq[l8 * 8 + e];
        wkv[e] = wk[l8 * 8 + e];
        aq[e] = ak[e] = 0.f;
    }
    for (long long base = (long long)blockIdx.x * QK_GROUPS; base < units; base += (long long)gridDim.x * QK_GROUPS) {   // (block-uniform)
        const long long u = base + grp;
        const bool live = u < units;
        const long long th = live ? u / heads : 0;
        const int head = live ? (int)(u - th * heads) : 0;
        const int which = (int)(th & 1);
        const size_t off = ((size_t)((th >> 1) * 3 + which) * heads + head) * 64 + l8 * 8;
        bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0}, dv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
            t = *(const bf16x8*)(qkv + off);
            dv = *(const bf16x8*)(dqkv + off);
        }
        float x[8], g[8], ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = (float)t[e];
            ss = fmaf(x[e], x[e], ss);
        }
        const float r = rsqrtf(group8_sum(ss) * (1.0f / 64.0f) + eps);
        float m = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = (float)dv[e];
            x[e] *= r;                                          // qh
            g[e] = d * (which == 0 ? wqv[e] : wkv[e]);
            m = fmaf(g[e], x[e], m);
            const float p = d * x[e];
            aq[e] += which == 0 ? p : 0.f;
            ak[e] += which == 0 ? 0.f : p;
        }
        m = group8_sum(m) * (1.0f / 64.0f);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)(r * fmaf(-x[e], m, g[e]));
        if (live) *(bf16x8*)(dqkv + off) = o;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s_acc[grp][l8 * 8 + e] = aq[e];
        s_acc[grp][64 + l8 * 8 + e] = ak[e];
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        float a = 0.f;
        for (int gI = 0; gI < QK_GROUPS; ++gI) a += s_acc[gI][threadIdx.x];
        part[(size_t)blockIdx.x * 128 + threadIdx.x] = a;
    }
}

// out[j] (j < 64: dwq, else dwk) = sum over the blocks of part[block][j]: block k in lane k % 64 in order, then the lanes in order.
// One launch block is 16 columns x 64 block lanes.
__global__ __launch_bounds__(1024) void qknorm_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ dwq, float* __restrict__ dwk) {
    __shared__ float s_acc[QK_FIN_LANES][16];
    const int col = threadIdx.x & 15, bl = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + col;
    float a = 0.f;
#pragma unroll 4
    for (int k = bl; k < nblk; k += QK_FIN_LANES) a += part[(size_t)k * 128 + j];
    s_acc[bl][col] = a;
    __syncthreads();
    if (bl == 0) {
        float t = 0.f;
        for (int i = 0; i < QK_FIN_LANES; ++i) t += s_acc[i][col];
        if (j < 64) dwq[j] = t; else dwk[j - 64] = t;
    }
}

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

int qk_check(const char* name, int B, int N, int heads) {
    if (B <= 0 || N <= 0 || heads <= 0 || (long long)B * N * 3 * heads >= (1ll << 31)) {
        tv_set_error("%s: bad shape B=%d N=%d heads=%d (positive, B N 3 heads < 2^31)", name, B, N, heads);
        return TV_ERR_ARG;
    }
    return TV_OK;
}

int qk_blocks(long long units) {
    const long long blocks = (units + QK_GROUPS - 1) / QK_GROUPS;
    return (int)(blocks < QK_MAX_BLOCKS ? blocks : QK_MAX_BLOCKS);
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

extern "C" int tv_qknorm_rope_fwd(const void* qkv, const float* wq, const float* wk, const float* rope_tab, void* out, int B, int N, int heads, float eps,
                                  void* stream) {
    if (qk_check("tv_qknorm_rope_fwd", B, N, heads)) return TV_ERR_ARG;
    TV_CHECK_ARG(qkv && wq && wk && out, "tv_qknorm_rope_fwd: null pointer");
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)rope_tab) & 15) == 0, "tv_qknorm_rope_fwd: qkv / out / rope_tab must be 16-byte aligned");
    const long long bytes = (long long)B * N * 3 * heads * 128;
    const char *a = (const char*)qkv, *b = (const char*)out;
    TV_CHECK_ARG(a == b || a + bytes <= b || b + bytes <= a, "tv_qknorm_rope_fwd: out must be qkv itself or not overlap it");
    const int nwhich = qkv == out ? 2 : 3;
    const long long units = (long long)B * N * nwhich;
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel, dim3(qk_blocks(units)), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, wq, wk, rope_tab, (bf16*)out, units,
                       nwhich, N, heads, eps);
    TV_CHECK_LAUNCH("tv_qknorm_rope_fwd");
    return TV_OK;
}

extern "C" long long tv_qknorm_rope_bwd_partial_count(int B, int N, int heads) {
    if (B <= 0 || N <= 0 || heads <= 0) return -1;
    return (long long)qk_blocks((long long)B * N * 2 * heads) * 128;          // floats
}

extern "C" int tv_qknorm_rope_bwd(const void* qkv, const float* wq, const float* wk, void* dqkv, float* dwq, float* dwk, float* partials, int B, int N,
                                  int heads, float eps, void* stream) {
    if (qk_check("tv_qknorm_rope_bwd", B, N, heads)) return TV_ERR_ARG;
    TV_CHECK_ARG(qkv && wq && wk && dqkv && dwq && dwk && partials, "tv_qknorm_rope_bwd: null pointer");
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)dqkv) & 15) == 0, "tv_qknorm_rope_bwd: qkv / dqkv must be 16-byte aligned");
    TV_CHECK_ARG(qkv != dqkv, "tv_qknorm_rope_bwd: dqkv must not be qkv");
    const long long units = (long long)B * N * 2 * heads;
    const int nblk = qk_blocks(units);
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, wq, wk, (bf16*)dqkv, partials, units, heads, eps);
    TV_CHECK_LAUNCH("tv_qknorm_rope_bwd");
    hipLaunchKernelGGL(qknorm_finalize_kernel, dim3(8), dim3(1024), 0, (hipStream_t)stream, (const float*)partials, nblk, dwq, dwk);
    TV_CHECK_LAUNCH("tv_qknorm_rope_bwd (finalise)");
    return TV_OK;
}

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
