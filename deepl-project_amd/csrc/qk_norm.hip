// The per-head RMSNorm of q and k with the 2-D RoPE (LightningDiT's qk-norm), one kernel family for head_dim 64 and 72
// (transvae/lightning_dit.py drives it; attention itself is tv_attn_* of attention.hip at 64 and tv_attn_*_hd of attention_hd.hip at
// 72).  DESIGN.md section 3.1 rows J (64) and Y (72) hold the rounding contract, section 3.6 the protocol.  qkv is bf16
// [B, N, 3, heads, HD], the weights fp32 [HD], the RoPE table fp32 [N, 4, HD / 2] = cos1, sin1, cos2, sin2 of the HD / 2 pairs.
//
//   tv_qknorm_rope_fwd(_hd)   per (token, head), q and k alike: r = rsqrt(mean_HD(q^2) + eps), out = bf16(rope(q r w)); v copied
//   tv_qknorm_rope_bwd(_hd)   in place on dqkv: dq_raw = bf16(r (g - qh mean_HD(g qh))), g = dq w, qh = q r; dw_j = sum dq_j qh_j
//
// A head vector is HD / 8 pieces of 16 bytes, one per lane of a lane group:
//   64   eight lanes, all live: per lane a chain of 8 FMAs from 0, then the xor butterfly over lane distances 1, 2, 4: 8 + 3
//        roundings; the mean is the sum times 1 / 64.
//   72   a 16-lane group holds one head vector, lanes 0..8 one piece each, lanes 9..15 the constant 0 (no load): per lane
//        a chain of 8 FMAs from 0, then the xor butterfly over lane distances 1, 2, 4, 8: 8 + 4 roundings; the mean is the
//        sum times fp32(1 / 72) (one more rounding).
// Used for mean(q^2) and mean(g qh) alike.
//
// Every sum that crosses rows is taken in a fixed order through scratch partials and written: no atomics, the same bits on every
// run.  dwq / dwk: per lane group its vectors in pass order, the groups of a block (32 at 64, 16 at 72) in order, then 64 block
// lanes (block k in lane k % 64, in order) and the lanes in order.
//
// Algorithmic bytes per call (what tools/lightning_dit_bench.py divides by kernel time), T = B N rows:
//   tv_qknorm_rope_fwd  8 T C in place (12 T C out of place)     tv_qknorm_rope_bwd  12 T C
//
// Deliberately NOT part of this family, although they look alike:
//   * rope_qk_kernel (elementwise.hip) and rope_adjoint4 (attention.hip) compile with the default contraction, their head_dim 72
//     twins in attention_hd.hip with contraction off: a shared body would change the bits of one side (the hazard row_wave.h
//     documents).  This file is contract(off), as both of its parents were.
//   * the two attention delta kernels sum in different, contract-stated orders (an 8-lane butterfly at 64, one thread over nine
//     piece sums at 72).
//   * the MFMA kernels of attention.hip (DMA ring, ablation bits, tuned) and of attention_hd.hip (plain staging).
#include "common.h"

#include <math.h>
#include <stdio.h>

#pragma clang fp contract(off)

namespace {

constexpr int QK_MAX_BLOCKS = 1024;
constexpr int QK_FIN_LANES = 64;    // block lanes of the dwq / dwk finalise

template <int HD>
struct Qk {
    static_assert(HD == 64 || HD == 72, "head_dim 64 or 72");
    static constexpr int PIECES = HD / 8;               // 16-byte pieces of a head vector
    static constexpr int LANES = HD == 64 ? 8 : 16;     // lanes of a group: 0 .. PIECES-1 hold one piece each, the rest zeros (no memory)
    static constexpr bool PADDED = PIECES < LANES;      // false at 64: every `live lane` test below is a compile-time true
    static constexpr int GROUPS = 256 / LANES;          // head vectors per block pass
    static constexpr float INV = 1.0f / HD;
    static constexpr int PAIRS = HD / 2;                // one plane of a table row; a row is four planes
};

template <int HD>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = 1; o < Qk<HD>::LANES; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bf16x8 zero8() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// A lane group takes one third of one token, unit u = token * nwhich + which, and walks its heads: the token's table row is loaded
// once for all of them (loaded per head vector it is four times the vector's own bytes, and the kernel is bound by those loads).
// nwhich = 3 out of place (the v third is copied), 2 in place (v stays where it is).
// in and out may alias: a vector belongs to one lane group, which reads it whole (the butterfly needs every live lane's load)
// before any of its lanes stores.
template <int HD>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const bf16* in, const float* __restrict__ wq, const float* __restrict__ wk,
                                                              const float* __restrict__ tab, bf16* out, long long units, int nwhich, int N, int heads,
                                                              float eps) {
    using G = Qk<HD>;
    const int ln = threadIdx.x & (G::LANES - 1), grp = threadIdx.x / G::LANES;
    const bool live = !G::PADDED || ln < G::PIECES;
    float wqv[8], wkv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        wqv[e] = live ? wq[ln * 8 + e] : 0.f;
        wkv[e] = live ? wk[ln * 8 + e] : 0.f;
    }
    for (long long base = (long long)blockIdx.x * G::GROUPS; base < units; base += (long long)gridDim.x * G::GROUPS) {   // (block-uniform)
        const long long u = base + grp;
        if (u >= units) continue;                              // (uniform over the lane group: its butterfly stays whole)
        const long long tok = u / nwhich;
        const int which = (int)(u - tok * nwhich);
        const size_t off = ((size_t)(tok * 3 + which) * heads) * HD + (live ? ln : 0) * 8;
        if (which == 2) {                                      // v: bit for bit
            if (live)
                for (int hd = 0; hd < heads; ++hd) *(bf16x8*)(out + off + (size_t)hd * HD) = *(const bf16x8*)(in + off + (size_t)hd * HD);
            continue;
        }
        f32x4 c1 = {1.f, 1.f, 1.f, 1.f}, s1 = {0.f, 0.f, 0.f, 0.f}, c2 = c1, s2 = s1;
        if (tab && live) {
            const float* tb = tab + (size_t)(tok % N) * (4 * G::PAIRS) + ln * 4;
            c1 = *(const f32x4*)(tb), s1 = *(const f32x4*)(tb + G::PAIRS), c2 = *(const f32x4*)(tb + 2 * G::PAIRS), s2 = *(const f32x4*)(tb + 3 * G::PAIRS);
        }
        for (int hd = 0; hd < heads; ++hd) {
            bf16x8 t = zero8();
            if (live) t = *(const bf16x8*)(in + off + (size_t)hd * HD);
            float x[8], ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                x[e] = (float)t[e];
                ss = fmaf(x[e], x[e], ss);
            }
            const float r = rsqrtf(group_sum<HD>(ss) * G::INV + eps);
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
            if (live) *(bf16x8*)(out + off + (size_t)hd * HD) = o;
        }
    }
}

// head vector u of the q and k thirds: token = u / (2 heads), which = (u / heads) % 2
template <int HD>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const bf16* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                                              bf16* __restrict__ dqkv, float* __restrict__ part, long long units, int heads, float eps) {
    using G = Qk<HD>;
    __shared__ float s_acc[G::GROUPS][2 * HD];
    const int ln = threadIdx.x & (G::LANES - 1), grp = threadIdx.x / G::LANES;
    const bool lane_live = !G::PADDED || ln < G::PIECES;
    float wqv[8], wkv[8], aq[8], ak[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        wqv[e] = lane_live ? wq[ln * 8 + e] : 0.f;
        wkv[e] = lane_live ? wk[ln * 8 + e] : 0.f;
        aq[e] = ak[e] = 0.f;
    }
    for (long long base = (long long)blockIdx.x * G::GROUPS; base < units; base += (long long)gridDim.x * G::GROUPS) {   // (block-uniform)
        const long long u = base + grp;
        const bool live = u < units && lane_live;
        const long long th = live ? u / heads : 0;
        const int head = live ? (int)(u - th * heads) : 0;
        const int which = (int)(th & 1);
        const size_t off = ((size_t)((th >> 1) * 3 + which) * heads + head) * HD + (!G::PADDED || live ? ln : 0) * 8;
        bf16x8 t = zero8(), dv = zero8();
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
        const float r = rsqrtf(group_sum<HD>(ss) * G::INV + eps);
        float m = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = (float)dv[e];
            x[e] *= r;                                          // qh
            g[e] = d * (which == 0 ? wqv[e] : wkv[e]);
            m = fmaf(g[e], x[e], m);
            const float pr = d * x[e];
            aq[e] += which == 0 ? pr : 0.f;
            ak[e] += which == 0 ? 0.f : pr;
        }
        m = group_sum<HD>(m) * G::INV;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)(r * fmaf(-x[e], m, g[e]));
        if (live) *(bf16x8*)(dqkv + off) = o;
    }
    if (lane_live) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s_acc[grp][ln * 8 + e] = aq[e];
            s_acc[grp][HD + ln * 8 + e] = ak[e];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * HD) {
        float a = 0.f;
        for (int gI = 0; gI < G::GROUPS; ++gI) a += s_acc[gI][threadIdx.x];
        part[(size_t)blockIdx.x * (2 * HD) + threadIdx.x] = a;
    }
}

// out[j] (j < HD: dwq, else dwk) = sum over the blocks of part[block][j]: block k in lane k % 64 in order, then the lanes in order.
// One launch block is 16 columns x 64 block lanes; 2 HD / 16 launch blocks cover the columns.
template <int HD>
__global__ __launch_bounds__(1024) void qknorm_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ dwq, float* __restrict__ dwk) {
    __shared__ float s_acc[QK_FIN_LANES][16];
    const int col = threadIdx.x & 15, bl = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + col;
    float a = 0.f;
#pragma unroll 4
    for (int k = bl; k < nblk; k += QK_FIN_LANES) a += part[(size_t)k * (2 * HD) + j];
    s_acc[bl][col] = a;
    __syncthreads();
    if (bl == 0) {
        float t = 0.f;
        for (int i = 0; i < QK_FIN_LANES; ++i) t += s_acc[i][col];
        if (j < HD) dwq[j] = t; else dwk[j - HD] = t;
    }
}

// head_dim is what the caller passed: the plain entries pass their own 64, so only an _hd entry can fail the first test
int qk_check(const char* name, int B, int N, int heads, int head_dim, int HD) {
    if (head_dim != HD) {
        tv_set_error("%s: head_dim=%d is not supported (72 only; head_dim 64 has its own entries)", name, head_dim);
        return TV_ERR_ARG;
    }
    if (B <= 0 || N <= 0 || heads <= 0 || (long long)B * N * 3 * heads >= (1ll << 31)) {
        tv_set_error("%s: bad shape B=%d N=%d heads=%d (positive, B N 3 heads < 2^31)", name, B, N, heads);
        return TV_ERR_ARG;
    }
    return TV_OK;
}

template <int HD>
int qk_blocks(long long units) {
    const long long blocks = (units + Qk<HD>::GROUPS - 1) / Qk<HD>::GROUPS;
    return (int)(blocks < QK_MAX_BLOCKS ? blocks : QK_MAX_BLOCKS);
}

template <int HD>
int qk_fwd(const char* name, const void* qkv, const float* wq, const float* wk, const float* rope_tab, void* out, int B, int N, int heads, int head_dim,
           float eps, void* stream) {
    if (int rc = qk_check(name, B, N, heads, head_dim, HD)) return rc;
    TV_CHECK_ARG(qkv && wq && wk && out, "%s: null pointer", name);
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)rope_tab) & 15) == 0, "%s: qkv / out / rope_tab must be 16-byte aligned", name);
    const long long bytes = (long long)B * N * 3 * heads * HD * 2;
    const char *a = (const char*)qkv, *b = (const char*)out;
    TV_CHECK_ARG(a == b || a + bytes <= b || b + bytes <= a, "%s: out must be qkv itself or not overlap it", name);
    const int nwhich = qkv == out ? 2 : 3;
    const long long units = (long long)B * N * nwhich;
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel<HD>, dim3(qk_blocks<HD>(units)), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, wq, wk, rope_tab,
                       (bf16*)out, units, nwhich, N, heads, eps);
    TV_CHECK_LAUNCH(name);
    return TV_OK;
}

template <int HD>
long long qk_partial_count(int B, int N, int heads, int head_dim) {
    if (B <= 0 || N <= 0 || heads <= 0 || head_dim != HD) return -1;
    return (long long)qk_blocks<HD>((long long)B * N * 2 * heads) * (2 * HD);          // floats
}

template <int HD>
int qk_bwd(const char* name, const void* qkv, const float* wq, const float* wk, void* dqkv, float* dwq, float* dwk, float* partials, int B, int N, int heads,
           int head_dim, float eps, void* stream) {
    if (int rc = qk_check(name, B, N, heads, head_dim, HD)) return rc;
    TV_CHECK_ARG(qkv && wq && wk && dqkv && dwq && dwk && partials, "%s: null pointer", name);
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)dqkv) & 15) == 0, "%s: qkv / dqkv must be 16-byte aligned", name);
    TV_CHECK_ARG(qkv != dqkv, "%s: dqkv must not be qkv", name);
    const long long units = (long long)B * N * 2 * heads;
    const int nblk = qk_blocks<HD>(units);
    hipLaunchKernelGGL(qknorm_rope_bwd_kernel<HD>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, wq, wk, (bf16*)dqkv, partials, units, heads,
                       eps);
    TV_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(qknorm_finalize_kernel<HD>, dim3(2 * HD / 16), dim3(1024), 0, (hipStream_t)stream, (const float*)partials, nblk, dwq, dwk);
    char fin[64];
    snprintf(fin, sizeof fin, "%s (finalise)", name);
    TV_CHECK_LAUNCH(fin);
    return TV_OK;
}

}  // namespace

extern "C" int tv_qknorm_rope_fwd(const void* qkv, const float* wq, const float* wk, const float* rope_tab, void* out, int B, int N, int heads, float eps,
                                  void* stream) {
    return qk_fwd<64>("tv_qknorm_rope_fwd", qkv, wq, wk, rope_tab, out, B, N, heads, 64, eps, stream);
}

extern "C" int tv_qknorm_rope_fwd_hd(const void* qkv, const float* wq, const float* wk, const float* rope_tab, void* out, int B, int N, int heads,
                                     int head_dim, float eps, void* stream) {
    return qk_fwd<72>("tv_qknorm_rope_fwd_hd", qkv, wq, wk, rope_tab, out, B, N, heads, head_dim, eps, stream);
}

extern "C" long long tv_qknorm_rope_bwd_partial_count(int B, int N, int heads) { return qk_partial_count<64>(B, N, heads, 64); }

extern "C" long long tv_qknorm_rope_bwd_hd_partial_count(int B, int N, int heads, int head_dim) { return qk_partial_count<72>(B, N, heads, head_dim); }

extern "C" int tv_qknorm_rope_bwd(const void* qkv, const float* wq, const float* wk, void* dqkv, float* dwq, float* dwk, float* partials, int B, int N,
                                  int heads, float eps, void* stream) {
    return qk_bwd<64>("tv_qknorm_rope_bwd", qkv, wq, wk, dqkv, dwq, dwk, partials, B, N, heads, 64, eps, stream);
}

extern "C" int tv_qknorm_rope_bwd_hd(const void* qkv, const float* wq, const float* wk, void* dqkv, float* dwq, float* dwk, float* partials, int B, int N,
                                     int heads, int head_dim, float eps, void* stream) {
    return qk_bwd<72>("tv_qknorm_rope_bwd_hd", qkv, wq, wk, dqkv, dwq, dwk, partials, B, N, heads, head_dim, eps, stream);
}
