// LightningDiT block variants of the latent DiT (transvae/lightning_dit.py drives them; the token GEMMs and attention are
// tv_igemm_nt / tv_wgrad_tn / tv_attn_*).  DESIGN.md section 3.1 row J holds the rounding contract, section 3.6 the protocol.  The
// conventions are those of dit.hip: token matrices are bf16 [B N, C], row r belongs to sample r / N, whose modulation is row r / N
// of an fp32 [B, ld] matrix read by column offsets.
//
//   tv_adaln_rms_fwd      y = bf16(fma(z, 1 + scale, shift)), z = xhat w (one rounding), xhat = x rsqrt(mean(x^2) + eps); one wave per row
//   tv_adaln_rms_bwd      dx = bf16(rstd (g - xhat mean(g xhat)) + dres), g = dy ((1 + scale) w); dshift = sum_n dy; with
//                         S = sum_n dy xhat: dscale = w S, dw = sum_b (1 + scale_b) S_b
//   tv_qknorm_rope_fwd    per (token, head), q and k alike: r = rsqrt(mean_64(q^2) + eps), out = bf16(rope(q r w)); v copied
//   tv_qknorm_rope_bwd    in place on dqkv: dq_raw = bf16(r (g - qh mean_64(g qh))), g = dq w, qh = q r; dw_j = sum dq_j qh_j
//   tv_swiglu_fwd         h = bf16(silu(x1) x2), u = [x1 | x2]
//   tv_swiglu_bwd         du1 = bf16(dh x2 s (1 + x1 (1 - s))), du2 = bf16(dh silu(x1)), s = sigmoid(x1)
//
// Every sum that crosses rows is taken in a fixed order through scratch partials and written: no atomics, the same bits on every
// run.  tv_adaln_rms_bwd: per wave its 16 rows of a 64-row slab in order, the four waves in order, the slabs of a sample in order
// (that is S), then for dw sixteen sample lanes (sample b in lane b % 16, in order) and the lanes in order.  tv_qknorm_rope_bwd: a head
// vector is eight lanes; per lane group its vectors in pass order, the 32 groups of a block in order, then 64 block lanes (block
// k in lane k % 64, in order) and the lanes in order.
//
// Algorithmic bytes per call (what tools/lightning_dit_bench.py divides by kernel time), T = B N rows:
//   tv_adaln_rms_fwd  4 T C     tv_adaln_rms_bwd  6 T C (8 T C with dres)     tv_qknorm_rope_fwd  8 T C in place (12 T C out of place)
//   tv_qknorm_rope_bwd  12 T C  tv_swiglu_fwd  6 T Hp                         tv_swiglu_bwd  10 T Hp
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int LR_RPB = 64;          // rows of one sample per block (4 waves x 16 rows)
constexpr int LR_MAX_C = 1536;      // 3 chunks per lane; the backward's LDS is 32 C bytes
constexpr int LR_DW_LANES = 16;     // sample lanes of the dw sum
constexpr int QK_GROUPS = 32;       // head vectors per block pass (256 threads / 8 lanes)
constexpr int QK_MAX_BLOCKS = 1024;
constexpr int QK_FIN_LANES = 64;    // block lanes of the dwq / dwk finalise

template <int KCH>
struct RmsRow {
    float v[KCH][8];   // x, then xhat (0 in the lanes past the row)
    float rstd;
};

// the statistic of one row held by a wave: one fma chain per lane over its elements, a butterfly, no mean
template <int KCH>
__device__ __forceinline__ void rms_load_row(const bf16* __restrict__ xr, int lane, int nch, float inv_c, float eps, RmsRow<KCH>& r) {
    float sv = 0.f;
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
        bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ch < nch) t = *(const bf16x8*)(xr + ch * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            r.v[k][e] = (float)t[e];
            sv = fmaf(r.v[k][e], r.v[k][e], sv);
        }
    }
    r.rstd = rsqrtf(tv_wave_sum(sv) * inv_c + eps);
#pragma unroll
    for (int k = 0; k < KCH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) r.v[k][e] *= r.rstd;
}

template <int KCH>
__global__ __launch_bounds__(256) void adaln_rms_fwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ mod,
                                                            int shift_off, int scale_off, int ld, bf16* __restrict__ y, int N, int C, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = C >> 3, b = blockIdx.y;
    const float inv_c = 1.0f / (float)C;
    const float* __restrict__ mb = mod + (size_t)b * ld;
    float sc1[KCH][8], sh[KCH][8], wv[KCH][8];
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc1[k][e] = (ch < nch) ? 1.0f + mb[scale_off + ch * 8 + e] : 0.f;
            sh[k][e] = (ch < nch) ? mb[shift_off + ch * 8 + e] : 0.f;
            wv[k][e] = (ch < nch) ? w[ch * 8 + e] : 0.f;
        }
    }
    const int r0 = blockIdx.x * LR_RPB, r1 = min(N, r0 + LR_RPB);
    for (int n = r0 + wave; n < r1; n += 4) {                // (wave-uniform)
        const size_t row = (size_t)b * N + n;
        RmsRow<KCH> r;
        rms_load_row<KCH>(x + row * C, lane, nch, inv_c, eps, r);
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const int ch = lane + 64 * k;
            if (ch < nch) {
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)fmaf(r.v[k][e] * wv[k][e], sc1[k][e], sh[k][e]);
                *(bf16x8*)(y + row * C + ch * 8) = o;
            }
        }
    }
}

template <int KCH>
__global__ __launch_bounds__(256) void adaln_rms_bwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ mod,
                                                            int scale_off, int ld, const bf16* __restrict__ dy, const bf16* __restrict__ dres,
                                                            bf16* __restrict__ dx, float* __restrict__ part, int N, int C, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_acc = (float*)smem;      // [4 waves][2][C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = C >> 3, b = blockIdx.y;
    const float inv_c = 1.0f / (float)C;
    const float* __restrict__ mb = mod + (size_t)b * ld;
    float gw[KCH][8], ds[KCH][8], dq[KCH][8];
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            gw[k][e] = (ch < nch) ? (1.0f + mb[scale_off + ch * 8 + e]) * w[ch * 8 + e] : 0.f;
            ds[k][e] = dq[k][e] = 0.f;
        }
    }
    const int r0 = blockIdx.x * LR_RPB, r1 = min(N, r0 + LR_RPB);
    for (int n = r0 + wave; n < r1; n += 4) {                // (wave-uniform)
        const size_t row = (size_t)b * N + n;
        RmsRow<KCH> r;
        rms_load_row<KCH>(x + row * C, lane, nch, inv_c, eps, r);
        float g[KCH][8];
        float a2 = 0.f;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const int ch = lane + 64 * k;
            bf16x8 u = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ch < nch) u = *(const bf16x8*)(dy + row * C + ch * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = (float)u[e];
                g[k][e] = d * gw[k][e];
                a2 = fmaf(g[k][e], r.v[k][e], a2);
                ds[k][e] += d;
                dq[k][e] = fmaf(d, r.v[k][e], dq[k][e]);
            }
        }
        a2 = tv_wave_sum(a2) * inv_c;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const int ch = lane + 64 * k;
            if (ch < nch) {
                bf16x8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
                if (dres) rv = *(const bf16x8*)(dres + row * C + ch * 8);
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)(r.rstd * fmaf(-r.v[k][e], a2, g[k][e]) + (float)rv[e]);
                *(bf16x8*)(dx + row * C + ch * 8) = o;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int ch = lane + 64 * k;
        if (ch < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s_acc[(wave * 2 + 0) * C + ch * 8 + e] = ds[k][e];
                s_acc[(wave * 2 + 1) * C + ch * 8 + e] = dq[k][e];
            }
        }
    }
    __syncthreads();
    float* __restrict__ dst = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        float a = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) a += s_acc[wv * 2 * C + i];
        dst[i] = a;
    }
}

// dshift[b][c] = sum over the slabs of part[b][slab][0][c]; S = the same of set 1: dscale[b][c] = w[c] S, and S is kept in
// sums[b][c] for the dw pass
__global__ __launch_bounds__(256) void rms_mod_finalize_kernel(const float* __restrict__ part, const float* __restrict__ w, float* __restrict__ out,
                                                               float* __restrict__ sums, int nblk, int C, int ld, int shift_off, int scale_off) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = 2 * C;
    if (i >= n) return;
    const float* __restrict__ src = part + (size_t)b * nblk * n + i;
    float a = 0.f;
    for (int k = 0; k < nblk; ++k) a += src[(size_t)k * n];
    if (i < C) {
        out[(size_t)b * ld + shift_off + i] = a;
    } else {
        const int c = i - C;
        out[(size_t)b * ld + scale_off + c] = w[c] * a;
        sums[(size_t)b * C + c] = a;
    }
}

// dw[c] = sum_b fma(1 + scale[b][c], S[b][c], .): sample b in lane b % 16 in order, then the sixteen lanes in order.  A block is 16
// columns x 16 sample lanes, so that the B / 16 dependent steps of a lane (not B of them) bound the launch.
__global__ __launch_bounds__(256) void rms_dw_kernel(const float* __restrict__ sums, const float* __restrict__ mod, int scale_off, int ld,
                                                     float* __restrict__ dw, int B, int C) {
    __shared__ float s_acc[LR_DW_LANES][16];
    const int col = threadIdx.x & 15, bl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + col;
    float a = 0.f;
    if (c < C) {
#pragma unroll 4
        for (int b = bl; b < B; b += LR_DW_LANES) a = fmaf(1.0f + mod[(size_t)b * ld + scale_off + c], sums[(size_t)b * C + c], a);
    }
    s_acc[bl][col] = a;
    __syncthreads();
    if (bl == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < LR_DW_LANES; ++i) t += s_acc[i][col];
        dw[c] = t;
    }
}

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

int lr_check(const char* name, int B, int N, int C, int ld) {
    if (B <= 0 || N <= 0 || C <= 0 || C % 8 != 0 || C > LR_MAX_C || ld < C || B > 65535 || (long long)B * N >= (1ll << 31)) {
        tv_set_error("%s: bad shape B=%d N=%d C=%d ld=%d (C %% 8 == 0, C <= %d, ld >= C, B <= 65535, B N < 2^31)", name, B, N, C, ld, LR_MAX_C);
        return TV_ERR_ARG;
    }
    return TV_OK;
}

bool lr_range(int off, int C, int ld) { return off >= 0 && (long long)off + C <= ld; }

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

extern "C" int tv_adaln_rms_fwd(const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, void* y, int B, int N, int C,
                                float eps, void* stream) {
    if (lr_check("tv_adaln_rms_fwd", B, N, C, ld)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && w && mod && y, "tv_adaln_rms_fwd: null pointer");
    TV_CHECK_ARG(lr_range(shift_off, C, ld) && lr_range(scale_off, C, ld), "tv_adaln_rms_fwd: column ranges %d / %d + %d outside ld=%d", shift_off,
                 scale_off, C, ld);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "tv_adaln_rms_fwd: x / y must be 16-byte aligned");
    const dim3 grid(tv_cdiv(N, LR_RPB), B);
    const int kch = tv_cdiv(C >> 3, 64);
#define TV_LR_FWD(K) hipLaunchKernelGGL(adaln_rms_fwd_kernel<K>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, w, mod, shift_off, scale_off, ld, (bf16*)y, N, C, eps)
    if (kch <= 1) TV_LR_FWD(1); else if (kch == 2) TV_LR_FWD(2); else TV_LR_FWD(3);
#undef TV_LR_FWD
    TV_CHECK_LAUNCH("tv_adaln_rms_fwd");
    return TV_OK;
}

extern "C" long long tv_adaln_rms_bwd_partial_count(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return -1;
    return (long long)B * tv_cdiv(N, LR_RPB) * 2 * C + (long long)B * C;          // floats: the slab partials, then S
}

extern "C" int tv_adaln_rms_bwd(const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, const void* dy, const void* dres,
                                void* dx, float* dmod, float* dw, float* partials, int B, int N, int C, float eps, void* stream) {
    if (lr_check("tv_adaln_rms_bwd", B, N, C, ld)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && w && mod && dy && dx && dmod && dw && partials, "tv_adaln_rms_bwd: null pointer");
    TV_CHECK_ARG(lr_range(shift_off, C, ld) && lr_range(scale_off, C, ld) && (shift_off + C <= scale_off || scale_off + C <= shift_off),
                 "tv_adaln_rms_bwd: column ranges %d / %d + %d outside ld=%d or overlapping", shift_off, scale_off, C, ld);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dres | (uintptr_t)dx) & 15) == 0, "tv_adaln_rms_bwd: x / dy / dres / dx must be 16-byte aligned");
    const int nblk = tv_cdiv(N, LR_RPB);
    const dim3 grid(nblk, B);
    const int kch = tv_cdiv(C >> 3, 64);
    const size_t lds = (size_t)8 * C * sizeof(float);
    float* sums = partials + (size_t)B * nblk * 2 * C;
#define TV_LR_BWD(K) hipLaunchKernelGGL(adaln_rms_bwd_kernel<K>, grid, dim3(256), lds, (hipStream_t)stream, (const bf16*)x, w, mod, scale_off, ld, (const bf16*)dy, (const bf16*)dres, (bf16*)dx, partials, N, C, eps)
    if (kch <= 1) TV_LR_BWD(1); else if (kch == 2) TV_LR_BWD(2); else TV_LR_BWD(3);
#undef TV_LR_BWD
    TV_CHECK_LAUNCH("tv_adaln_rms_bwd");
    hipLaunchKernelGGL(rms_mod_finalize_kernel, dim3(tv_cdiv(2 * C, 256), B), dim3(256), 0, (hipStream_t)stream, (const float*)partials, w, dmod, sums, nblk, C,
                       ld, shift_off, scale_off);
    TV_CHECK_LAUNCH("tv_adaln_rms_bwd (finalise)");
    hipLaunchKernelGGL(rms_dw_kernel, dim3(tv_cdiv(C, 16)), dim3(256), 0, (hipStream_t)stream, (const float*)sums, mod, scale_off, ld, dw, B, C);
    TV_CHECK_LAUNCH("tv_adaln_rms_bwd (dw)");
    return TV_OK;
}

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
