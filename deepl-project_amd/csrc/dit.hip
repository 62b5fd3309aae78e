// Latent DiT: the adaLN conditioning arithmetic of its two block variants and the flow-matching edge (transvae/dit.py and
// transvae/lightning_dit.py drive them; the token GEMMs and attention are tv_igemm_nt / tv_wgrad_tn / tv_attn_*).  DESIGN.md section 3.1
// rows E and J hold the rounding contracts, sections 3.4, 3.6 and 3.7 the protocols.  Rows are tokens: row r of a [B N, C] matrix belongs to
// sample r / N, whose modulation is row r / N of an fp32 [B, ld] matrix; shift / scale / gate are column ranges of it, given as offsets.
//
//   tv_adaln_fwd           y = bf16(fma(xhat, 1 + scale, shift)), xhat = (x - mean) rstd, two-pass statistics, one wave per row
//   tv_adaln_bwd           dx = bf16(rstd (g - mean g - xhat mean(g xhat)) + dres), g = dy (1 + scale); dshift = sum_n dy, dscale = sum_n dy xhat
//   tv_adaln_rms_fwd       y = bf16(fma(z, 1 + scale, shift)), z = xhat w (one rounding), xhat = x rsqrt(mean(x^2) + eps); the same kernel, RMS = true
//   tv_adaln_rms_bwd       dx = bf16(rstd (g - xhat mean(g xhat)) + dres), g = dy ((1 + scale) w); dshift = sum_n dy; with
//                          S = sum_n dy xhat: dscale = w S, dw = sum_b (1 + scale_b) S_b
//   tv_gate_residual_fwd   out = bf16(fma(gate, y, x))
//   tv_gate_residual_bwd   dy = bf16(gate dout); dgate = sum_n dout y
//   tv_flow_rows           patch rows of x_t = fma(t, x, (1 - t) e), x = (lat - mean) rstd   (no noise: the rows of x)
//   tv_flow_loss           mean over the real columns of (pred - (x - e))^2 and its gradient
//   tv_flow_euler          x += dt (v_u + s (v_c - v_u)), un-patchified on the fly
//   tv_flow_loss_cos       tv_flow_loss plus cos_weight times the mean over the latent pixels of 1 - cos(pred, x - e), one gradient
//   tv_flow_heun           the corrector of a Heun step: x += dt / 2 (g2 - g1), each g as in tv_flow_euler
//
// The per-sample sums never cross a sample inside a block: the grids of the reducing kernels are cut per sample (blockIdx.y = sample,
// blockIdx.x = a slab of its rows), so a row count that is no multiple of the slab leaves a short last slab instead of a block that
// straddles two samples.  Every sum is taken in a fixed order (lane: its rows in order; block: its waves or row lanes in order;
// finalise: the slabs in order; for the dw of tv_adaln_rms_bwd then sixteen sample lanes, sample b in lane b % 16 in order, and the
// lanes in order): no atomics, the same bits on every run.
//
// Algorithmic bytes per call (what tools/dit_bench.py and tools/lightning_dit_bench.py divide by kernel time), T = B N rows:
//   tv_adaln_fwd, tv_adaln_rms_fwd  4 T C        tv_adaln_bwd, tv_adaln_rms_bwd  6 T C (8 T C with dres)
//   tv_gate_residual_fwd  6 T C      tv_gate_residual_bwd  6 T C
//   tv_flow_rows  4 B D h w (8 with noise) + 2 T ld     tv_flow_loss  8 B D h w + 4 T ld     tv_flow_euler  8 B D h w + 2 T ld (4 guided)
//   tv_flow_loss_cos  as tv_flow_loss     tv_flow_heun  8 B D h w + 2 T ld per unguided, 4 T ld per guided evaluation
#include "row_wave.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int AD_RPB = 64;          // rows of one sample per block (4 waves x 16 rows)
constexpr int AD_MAX_C = 1536;      // 3 chunks per lane; the backward's LDS is 32 C bytes
constexpr int AD_DW_LANES = 16;     // sample lanes of the dw sum
constexpr int GR_RPB = 64;
constexpr int GR_MAX_C = 2048;      // one 16-byte chunk per thread column
constexpr int FL_MAX_BLOCKS = 1024;
constexpr double FL_COS_EPS2 = 1e-16;   // eps^2 of the cosine term, eps = 1e-8: max(n, eps) = sqrt(max(n^2, eps^2))

// xhat of one row held by a wave (row_wave.h), in place; returns rstd
//   RMS = false  two passes: the mean, then the squared deviations from it (the scheme of tv_rownorm_fwd mode 2); xhat = (x - mean) rstd
//   RMS = true   one fma chain per lane over its elements, a butterfly, no mean; xhat = x rstd
template <int KCH, bool RMS>
__device__ __forceinline__ float ad_load_xhat(const bf16* __restrict__ xr, int lane, int nch, float inv_c, float eps, float (&v)[KCH][8]) {
    rw_load<KCH>(xr, lane, nch, v);
    float sv;
    if constexpr (RMS) sv = rw_sumsq<KCH>(v);
    else sv = rw_centre<KCH>(v, lane, nch, rw_sum<KCH>(v) * inv_c);
    const float rstd = rsqrtf(sv * inv_c + eps);
#pragma unroll
    for (int k = 0; k < KCH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[k][e] *= rstd;
    return rstd;
}

// RMS: xhat = x rstd is scaled by the weight w before the modulation (tv_adaln_rms_fwd); otherwise w is not read
template <int KCH, bool RMS>
__global__ __launch_bounds__(256) void adaln_fwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ mod,
                                                        int shift_off, int scale_off, int ld, bf16* __restrict__ y, int N, int C, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = C >> 3, b = blockIdx.y;
    const float inv_c = 1.0f / (float)C;
    const float* __restrict__ mb = mod + (size_t)b * ld;
    float sc1[KCH][8], sh[KCH][8], wv[KCH][8];
    rw_load_cols<KCH, true>(mb + scale_off, lane, nch, 0.f, sc1);
    rw_load_cols<KCH>(mb + shift_off, lane, nch, 0.f, sh);
    if constexpr (RMS) rw_load_cols<KCH>(w, lane, nch, 0.f, wv);
    const int r0 = blockIdx.x * AD_RPB, r1 = min(N, r0 + AD_RPB);
    for (int n = r0 + wave; n < r1; n += 4) {                // (wave-uniform)
        const size_t row = (size_t)b * N + n;
        float xh[KCH][8];
        ad_load_xhat<KCH, RMS>(x + row * C, lane, nch, inv_c, eps, xh);
        rw_store<KCH>(y, nullptr, row * C, lane, nch, [&](int k, int e, float) {
            float z = xh[k][e];
            if constexpr (RMS) z *= wv[k][e];
            return fmaf(z, sc1[k][e], sh[k][e]);
        });
    }
}

// RMS: g = dy ((1 + scale) w) and no `- mean g` term (tv_adaln_rms_bwd); part[b][slab] = {sum_n dy, sum_n dy xhat} either way
template <int KCH, bool RMS>
__global__ __launch_bounds__(256) void adaln_bwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ mod,
                                                        int scale_off, int ld, const bf16* __restrict__ dy, const bf16* __restrict__ dres,
                                                        bf16* __restrict__ dx, float* __restrict__ part, int N, int C, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_acc = (float*)smem;      // [4 waves][2][C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = C >> 3, b = blockIdx.y;
    const float inv_c = 1.0f / (float)C;
    float gs[KCH][8], ds[KCH][8], dq[KCH][8];      // gs: the factor of g = dy gs
    rw_load_cols<KCH, true>(mod + (size_t)b * ld + scale_off, lane, nch, 0.f, gs);
    if constexpr (RMS) {
        float wv[KCH][8];
        rw_load_cols<KCH>(w, lane, nch, 0.f, wv);
#pragma unroll
        for (int k = 0; k < KCH; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) gs[k][e] *= wv[k][e];   // (1 + scale) w, rounded once per channel
    }
#pragma unroll
    for (int k = 0; k < KCH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) ds[k][e] = dq[k][e] = 0.f;
    const int r0 = blockIdx.x * AD_RPB, r1 = min(N, r0 + AD_RPB);
    for (int n = r0 + wave; n < r1; n += 4) {                // (wave-uniform)
        const size_t row = (size_t)b * N + n;
        float xh[KCH][8], g[KCH][8];
        const float rstd = ad_load_xhat<KCH, RMS>(x + row * C, lane, nch, inv_c, eps, xh);
        rw_load<KCH>(dy + row * C, lane, nch, g);
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < KCH; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = g[k][e];
                g[k][e] = d * gs[k][e];
                if constexpr (!RMS) a1 += g[k][e];
                a2 = fmaf(g[k][e], xh[k][e], a2);
                ds[k][e] += d;
                dq[k][e] = fmaf(d, xh[k][e], dq[k][e]);
            }
        if constexpr (!RMS) a1 = tv_wave_sum(a1) * inv_c;
        a2 = tv_wave_sum(a2) * inv_c;
        rw_store<KCH>(dx, dres, row * C, lane, nch, [&](int k, int e, float res) {
            float t = g[k][e];
            if constexpr (!RMS) t -= a1;
            return rstd * fmaf(-xh[k][e], a2, t) + res;
        });
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

// out[b][off(set) + c] = sum over the slabs of part[b][slab][set][c], in slab order.  With w (tv_adaln_rms_bwd) set 1 is
// S = sum_n dy xhat: dscale[b][c] = w[c] S, and S is kept in sums[b][c] for the dw pass
__global__ __launch_bounds__(256) void mod_finalize_kernel(const float* __restrict__ part, const float* __restrict__ w, float* __restrict__ out,
                                                           float* __restrict__ sums, int nblk, int nsets, int C, int ld, int off0, int off1) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = nsets * C;
    if (i >= n) return;
    const float* __restrict__ src = part + (size_t)b * nblk * n + i;
    float a = 0.f;
    for (int k = 0; k < nblk; ++k) a += src[(size_t)k * n];
    const int set = i / C, c = i - set * C;
    if (w && set == 1) {
        sums[(size_t)b * C + c] = a;
        a = w[c] * a;
    }
    out[(size_t)b * ld + (set == 0 ? off0 : off1) + c] = a;
}

// dw[c] = sum_b fma(1 + scale[b][c], S[b][c], .): sample b in lane b % 16 in order, then the sixteen lanes in order.  A block is 16
// columns x 16 sample lanes, so that the B / 16 dependent steps of a lane (not B of them) bound the launch.
__global__ __launch_bounds__(256) void rms_dw_kernel(const float* __restrict__ sums, const float* __restrict__ mod, int scale_off, int ld,
                                                     float* __restrict__ dw, int B, int C) {
    __shared__ float s_acc[AD_DW_LANES][16];
    const int col = threadIdx.x & 15, bl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + col;
    float a = 0.f;
    if (c < C) {
#pragma unroll 4
        for (int b = bl; b < B; b += AD_DW_LANES) a = fmaf(1.0f + mod[(size_t)b * ld + scale_off + c], sums[(size_t)b * C + c], a);
    }
    s_acc[bl][col] = a;
    __syncthreads();
    if (bl == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < AD_DW_LANES; ++i) t += s_acc[i][col];
        dw[c] = t;
    }
}

__global__ __launch_bounds__(256) void gate_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ y, const float* __restrict__ mod, int gate_off,
                                                       int ld, bf16* __restrict__ out, long long total, int N, int nch) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / nch;
        const int ch = (int)(idx - row * nch);
        const float* __restrict__ g = mod + (size_t)(row / N) * ld + gate_off + ch * 8;
        const bf16x8 xv = *(const bf16x8*)(x + idx * 8), yv = *(const bf16x8*)(y + idx * 8);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)fmaf(g[e], (float)yv[e], (float)xv[e]);
        *(bf16x8*)(out + idx * 8) = o;
    }
}

__global__ __launch_bounds__(256) void gate_bwd_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ y, const float* __restrict__ mod,
                                                       int gate_off, int ld, bf16* __restrict__ dy, float* __restrict__ part, int N, int C) {
    __shared__ float s_acc[GR_MAX_C];     // [row lanes][C], row lanes * C <= 2048
    const int nch = C >> 3, b = blockIdx.y;
    const int rows = 256 / nch;
    const int chunk = threadIdx.x % nch, prow = threadIdx.x / nch;
    if (prow < rows) {
        float gt[8], s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            gt[e] = mod[(size_t)b * ld + gate_off + chunk * 8 + e];
            s[e] = 0.f;
        }
        const int r0 = blockIdx.x * GR_RPB, r1 = min(N, r0 + GR_RPB);
        for (int n = r0 + prow; n < r1; n += rows) {
            const size_t off = ((size_t)b * N + n) * C + chunk * 8;
            const bf16x8 gv = *(const bf16x8*)(dout + off), yv = *(const bf16x8*)(y + off);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = (float)gv[e];
                o[e] = (bf16)(gt[e] * d);
                s[e] = fmaf(d, (float)yv[e], s[e]);
            }
            *(bf16x8*)(dy + off) = o;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s_acc[prow * C + chunk * 8 + e] = s[e];
    }
    __syncthreads();
    float* __restrict__ dst = part + ((size_t)b * gridDim.x + blockIdx.x) * C;
    for (int i = threadIdx.x; i < C; i += 256) {
        float a = 0.f;
        for (int r = 0; r < rows; ++r) a += s_acc[r * C + i];
        dst[i] = a;
    }
}

// ---- flow matching: patch rows <-> latents -----------------------------------------------------------------------------------
struct FlowGeo {
    long long sn, sc;      // element strides of the latents' batch and channel axes
    int D, h, w, p, gw, N, F, ldv;
};

// element (row, col) of the patch matrix -> offsets into the latents (strided) and a dense [B, D, h, w] tensor; c = its channel
__device__ __forceinline__ void flow_index(const FlowGeo& g, long long row, int col, long long& lat_off, long long& dense_off, int& c) {
    const long long b = row / g.N;
    const int tok = (int)(row - b * g.N);
    const int q = col / g.D;
    c = col - q * g.D;
    const int py = q / g.p, px = q - py * g.p;
    const int ty = tok / g.gw, tx = tok - ty * g.gw;
    const long long pos = (long long)(ty * g.p + py) * g.w + (tx * g.p + px);
    lat_off = b * g.sn + (long long)c * g.sc + pos;
    dense_off = (b * g.D + c) * (long long)g.h * g.w + pos;
}

__global__ __launch_bounds__(256) void flow_rows_kernel(const float* __restrict__ lat, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ noise, const float* __restrict__ t, bf16* __restrict__ rows,
                                                        long long total, FlowGeo g) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / g.ldv;
        const int col0 = (int)(idx - row * g.ldv) * 8;
        float tb = 0.f, ub = 0.f;
        if (noise) {
            tb = t[row / g.N];
            ub = 1.0f - tb;
        }
        bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            if (col < g.F) {
                long long lo, no;
                int c;
                flow_index(g, row, col, lo, no, c);
                const float xv = (lat[lo] - mean[c]) * rstd[c];
                o[e] = noise ? (bf16)fmaf(tb, xv, ub * noise[no]) : (bf16)xv;
            }
        }
        *(bf16x8*)(rows + idx * 8) = o;
    }
}

__global__ __launch_bounds__(256) void flow_loss_kernel(const bf16* __restrict__ pred, const float* __restrict__ lat, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ noise, bf16* __restrict__ dpred,
                                                        double* __restrict__ partials, long long total, FlowGeo g, float coef) {
    __shared__ double wpart[4];
    double acc = 0.0;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / g.ldv;
        const int col0 = (int)(idx - row * g.ldv) * 8;
        const bf16x8 pv = *(const bf16x8*)(pred + idx * 8);
        bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            if (col < g.F) {
                long long lo, no;
                int c;
                flow_index(g, row, col, lo, no, c);
                const float v = (lat[lo] - mean[c]) * rstd[c] - noise[no];
                const float d = (float)pv[e] - v;
                acc += (double)d * (double)d;
                o[e] = (bf16)(coef * d);
            }
        }
        if (dpred) *(bf16x8*)(dpred + idx * 8) = o;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wpart[0] + wpart[1]) + wpart[2]) + wpart[3];
}

// out[0] = sum of the block partials (lane l: blocks l, l + 64, ... in order, then a butterfly), out[1] = out[0] / count
__global__ __launch_bounds__(64) void flow_loss_finalize_kernel(const double* __restrict__ partials, int nblk, double count, double* __restrict__ out) {
    double a = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) a += partials[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = a / count;
    }
}

__global__ __launch_bounds__(256) void flow_euler_kernel(float* __restrict__ x, const bf16* __restrict__ v, long long total, long long half, FlowGeo g,
                                                         float dt, float s, int guided) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / g.ldv;
        const int col0 = (int)(idx - row * g.ldv) * 8;
        if (col0 >= g.F) continue;
        const bf16x8 vc = *(const bf16x8*)(v + idx * 8);
        bf16x8 vu = {0, 0, 0, 0, 0, 0, 0, 0};
        if (guided) vu = *(const bf16x8*)(v + half + idx * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            if (col < g.F) {
                long long lo, no;
                int c;
                flow_index(g, row, col, lo, no, c);
                float vel = (float)vc[e];
                if (guided) vel = fmaf(s, vel - (float)vu[e], (float)vu[e]);
                x[no] = fmaf(dt, vel, x[no]);
            }
        }
    }
}

// tv_flow_loss with the per-position cosine term.  The thread layout, the grid and the fp64 order of the squared-error sum are those of
// flow_loss_kernel, so that half of the result has the same bits.  A position is the D columns q D .. q D + D - 1 of a row; a thread
// forms the three sums of every position that its eight columns touch (fp32 fma chains over c = 0 .. D - 1, the same bits in every
// thread that forms them: a position that spans several vectors is summed once per vector), cos and the two reciprocal norms from them
// in fp64 rounded once each, and the thread that holds column q D adds 1 - cos to the second sum.
__global__ __launch_bounds__(256) void flow_loss_cos_kernel(const bf16* __restrict__ pred, const float* __restrict__ lat, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ noise, bf16* __restrict__ dpred,
                                                            double* __restrict__ partials, long long total, FlowGeo g, float cmse, float ccos) {
    __shared__ double wpart[2][4];
    double acc = 0.0, accc = 0.0;
    const long long hw = (long long)g.h * g.w;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / g.ldv;
        const int col0 = (int)(idx - row * g.ldv) * 8;
        const bf16* __restrict__ prow = pred + row * g.ldv * 8;
        const bf16x8 pv = *(const bf16x8*)(pred + idx * 8);
        bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
        int qcur = -1;
        bool live = false;
        float cosv = 0.f, rp = 0.f, rv = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            if (col < g.F) {
                const int q = col / g.D, c = col - q * g.D;
                long long lo, no;
                int cc;
                if (q != qcur) {
                    qcur = q;
                    flow_index(g, row, q * g.D, lo, no, cc);
                    float np2 = 0.f, nv2 = 0.f, dot = 0.f;
                    for (cc = 0; cc < g.D; ++cc) {
                        const float vv = (lat[lo + cc * g.sc] - mean[cc]) * rstd[cc] - noise[no + cc * hw];
                        const float pp = (float)prow[q * g.D + cc];
                        np2 = fmaf(pp, pp, np2);
                        nv2 = fmaf(vv, vv, nv2);
                        dot = fmaf(pp, vv, dot);
                    }
                    live = (double)np2 > FL_COS_EPS2;          // n_p <= eps: cos = 0 and no gradient from the term
                    cosv = rp = rv = 0.f;
                    if (live) {
                        const double nvc = fmax((double)nv2, FL_COS_EPS2);
                        cosv = (float)((double)dot / sqrt((double)np2 * nvc));
                        rp = (float)(1.0 / sqrt((double)np2));
                        rv = (float)(1.0 / sqrt(nvc));
                    }
                    if (c == 0) accc += 1.0 - (double)cosv;
                }
                flow_index(g, row, col, lo, no, cc);
                const float v = (lat[lo] - mean[cc]) * rstd[cc] - noise[no];
                const float pp = (float)pv[e];
                const float d = pp - v;
                acc += (double)d * (double)d;
                float gr = cmse * d;
                if (live) gr = fmaf(-ccos, (v * rv - (cosv * pp) * rp) * rp, gr);
                o[e] = (bf16)gr;
            }
        }
        if (dpred) *(bf16x8*)(dpred + idx * 8) = o;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        accc += __shfl_xor(accc, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wpart[0][threadIdx.x >> 6] = acc;
        wpart[1][threadIdx.x >> 6] = accc;
    }
    __syncthreads();
    if (threadIdx.x < 2) partials[threadIdx.x * gridDim.x + blockIdx.x] = ((wpart[threadIdx.x][0] + wpart[threadIdx.x][1]) + wpart[threadIdx.x][2]) + wpart[threadIdx.x][3];
}

// partials: the nblk squared-error sums, then the nblk cosine sums; each summed as flow_loss_finalize_kernel does
// out = {mse sum, mse mean, cos sum, cos mean, mse mean + cos_weight cos mean}
__global__ __launch_bounds__(64) void flow_loss_cos_finalize_kernel(const double* __restrict__ partials, int nblk, double count, double count_pos,
                                                                    double cos_weight, double* __restrict__ out) {
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) {
        a += partials[k];
        b += partials[nblk + k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = a / count;
        out[2] = b;
        out[3] = b / count_pos;
        out[4] = out[1] + cos_weight * out[3];
    }
}

// the corrector of a Heun step on x that holds the predictor's x + dt g1: x = fma(dt / 2, g2 - g1, x), g_k as in flow_euler_kernel
__global__ __launch_bounds__(256) void flow_heun_kernel(float* __restrict__ x, const bf16* __restrict__ v1, const bf16* __restrict__ v2, long long total,
                                                        long long half, FlowGeo g, float hdt, float s, int guided1, int guided2) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / g.ldv;
        const int col0 = (int)(idx - row * g.ldv) * 8;
        if (col0 >= g.F) continue;
        const bf16x8 c1 = *(const bf16x8*)(v1 + idx * 8), c2 = *(const bf16x8*)(v2 + idx * 8);
        bf16x8 u1 = {0, 0, 0, 0, 0, 0, 0, 0}, u2 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (guided1) u1 = *(const bf16x8*)(v1 + half + idx * 8);
        if (guided2) u2 = *(const bf16x8*)(v2 + half + idx * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            if (col < g.F) {
                long long lo, no;
                int c;
                flow_index(g, row, col, lo, no, c);
                float g1 = (float)c1[e], g2 = (float)c2[e];
                if (guided1) g1 = fmaf(s, g1 - (float)u1[e], (float)u1[e]);
                if (guided2) g2 = fmaf(s, g2 - (float)u2[e], (float)u2[e]);
                x[no] = fmaf(hdt, g2 - g1, x[no]);
            }
        }
    }
}

int ad_check(const char* name, int B, int N, int C, int ld, int max_c) {
    if (B <= 0 || N <= 0 || C <= 0 || C % 8 != 0 || C > max_c || ld < C || B > 65535 || (long long)B * N >= (1ll << 31)) {
        tv_set_error("%s: bad shape B=%d N=%d C=%d ld=%d (C %% 8 == 0, C <= %d, ld >= C, B <= 65535, B N < 2^31)", name, B, N, C, ld, max_c);
        return TV_ERR_ARG;
    }
    return TV_OK;
}

bool ad_range(int off, int C, int ld) { return off >= 0 && (long long)off + C <= ld; }

// tv_adaln_fwd (w unused) and tv_adaln_rms_fwd
template <bool RMS>
int adaln_fwd(const char* name, const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, void* y, int B, int N, int C,
              float eps, void* stream) {
    if (ad_check(name, B, N, C, ld, AD_MAX_C)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && (w || !RMS) && mod && y, "%s: null pointer", name);
    TV_CHECK_ARG(ad_range(shift_off, C, ld) && ad_range(scale_off, C, ld), "%s: column ranges %d / %d + %d outside ld=%d", name, shift_off, scale_off, C,
                 ld);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "%s: x / y must be 16-byte aligned", name);
    rw_dispatch<1, 2, 3>(tv_cdiv(C >> 3, 64), [&](auto K) {
        hipLaunchKernelGGL((adaln_fwd_kernel<decltype(K)::value, RMS>), dim3(tv_cdiv(N, AD_RPB), B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, w, mod,
                           shift_off, scale_off, ld, (bf16*)y, N, C, eps);
    });
    TV_CHECK_LAUNCH(name);
    return TV_OK;
}

// the row pass of tv_adaln_bwd (w, dw unused) and tv_adaln_rms_bwd: dx and the slab partials; the callers finalise
template <bool RMS>
int adaln_bwd(const char* name, const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, const void* dy, const void* dres,
              void* dx, const float* dmod, const float* dw, float* partials, int B, int N, int C, float eps, void* stream) {
    if (ad_check(name, B, N, C, ld, AD_MAX_C)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && (w || !RMS) && mod && dy && dx && dmod && (dw || !RMS) && partials, "%s: null pointer", name);
    TV_CHECK_ARG(ad_range(shift_off, C, ld) && ad_range(scale_off, C, ld) && (shift_off + C <= scale_off || scale_off + C <= shift_off),
                 "%s: column ranges %d / %d + %d outside ld=%d or overlapping", name, shift_off, scale_off, C, ld);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dres | (uintptr_t)dx) & 15) == 0, "%s: x / dy / dres / dx must be 16-byte aligned", name);
    rw_dispatch<1, 2, 3>(tv_cdiv(C >> 3, 64), [&](auto K) {
        hipLaunchKernelGGL((adaln_bwd_kernel<decltype(K)::value, RMS>), dim3(tv_cdiv(N, AD_RPB), B), dim3(256), (size_t)8 * C * sizeof(float),
                           (hipStream_t)stream, (const bf16*)x, w, mod, scale_off, ld, (const bf16*)dy, (const bf16*)dres, (bf16*)dx, partials, N, C, eps);
    });
    TV_CHECK_LAUNCH(name);
    return TV_OK;
}

int flow_geo(const char* name, long long sn, long long sc, int B, int D, int h, int w, int p, int ld, FlowGeo& g) {
    if (B <= 0 || D <= 0 || h <= 0 || w <= 0 || p <= 0 || h % p != 0 || w % p != 0) {
        tv_set_error("%s: bad shape B=%d D=%d h=%d w=%d patch=%d (the patch must divide the grid)", name, B, D, h, w, p);
        return TV_ERR_ARG;
    }
    const long long F = (long long)p * p * D, N = (long long)(h / p) * (w / p);
    if (ld % 32 != 0 || ld < F || (long long)ld >= (1ll << 30) || (long long)B * N >= (1ll << 31)) {
        tv_set_error("%s: ld=%d must be a multiple of 32 that covers %lld columns, and B N < 2^31", name, ld, F);
        return TV_ERR_ARG;
    }
    if (sc < (long long)h * w || sn < (long long)(D - 1) * sc + (long long)h * w) {
        tv_set_error("%s: strides (%lld, %lld) overlap for D=%d, h=%d, w=%d", name, sn, sc, D, h, w);
        return TV_ERR_ARG;
    }
    g.sn = sn; g.sc = sc; g.D = D; g.h = h; g.w = w; g.p = p; g.gw = w / p; g.N = (int)N; g.F = (int)F; g.ldv = ld / 8;
    return TV_OK;
}

unsigned flow_blocks(long long total, int cap) {
    long long blocks = (total + 255) / 256;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

extern "C" int tv_adaln_fwd(const void* x, const float* mod, int shift_off, int scale_off, int ld, void* y, int B, int N, int C, float eps,
                            void* stream) {
    return adaln_fwd<false>("tv_adaln_fwd", x, nullptr, mod, shift_off, scale_off, ld, y, B, N, C, eps, stream);
}

extern "C" int tv_adaln_rms_fwd(const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, void* y, int B, int N, int C,
                                float eps, void* stream) {
    return adaln_fwd<true>("tv_adaln_rms_fwd", x, w, mod, shift_off, scale_off, ld, y, B, N, C, eps, stream);
}

extern "C" long long tv_adaln_bwd_partial_count(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return -1;
    return (long long)B * tv_cdiv(N, AD_RPB) * 2 * C;          // floats
}

extern "C" long long tv_adaln_rms_bwd_partial_count(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return -1;
    return (long long)B * tv_cdiv(N, AD_RPB) * 2 * C + (long long)B * C;          // floats: the slab partials, then S
}

extern "C" int tv_adaln_bwd(const void* x, const float* mod, int shift_off, int scale_off, int ld, const void* dy, const void* dres, void* dx,
                            float* dmod, float* partials, int B, int N, int C, float eps, void* stream) {
    if (int rc = adaln_bwd<false>("tv_adaln_bwd", x, nullptr, mod, shift_off, scale_off, ld, dy, dres, dx, dmod, nullptr, partials, B, N, C, eps, stream))
        return rc;
    hipLaunchKernelGGL(mod_finalize_kernel, dim3(tv_cdiv(2 * C, 256), B), dim3(256), 0, (hipStream_t)stream, (const float*)partials, nullptr, dmod, nullptr,
                       tv_cdiv(N, AD_RPB), 2, C, ld, shift_off, scale_off);
    TV_CHECK_LAUNCH("tv_adaln_bwd (finalise)");
    return TV_OK;
}

extern "C" int tv_adaln_rms_bwd(const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, const void* dy, const void* dres,
                                void* dx, float* dmod, float* dw, float* partials, int B, int N, int C, float eps, void* stream) {
    if (int rc = adaln_bwd<true>("tv_adaln_rms_bwd", x, w, mod, shift_off, scale_off, ld, dy, dres, dx, dmod, dw, partials, B, N, C, eps, stream)) return rc;
    const int nblk = tv_cdiv(N, AD_RPB);
    float* sums = partials + (size_t)B * nblk * 2 * C;
    hipLaunchKernelGGL(mod_finalize_kernel, dim3(tv_cdiv(2 * C, 256), B), dim3(256), 0, (hipStream_t)stream, (const float*)partials, w, dmod, sums, nblk, 2, C,
                       ld, shift_off, scale_off);
    TV_CHECK_LAUNCH("tv_adaln_rms_bwd (finalise)");
    hipLaunchKernelGGL(rms_dw_kernel, dim3(tv_cdiv(C, 16)), dim3(256), 0, (hipStream_t)stream, (const float*)sums, mod, scale_off, ld, dw, B, C);
    TV_CHECK_LAUNCH("tv_adaln_rms_bwd (dw)");
    return TV_OK;
}

extern "C" int tv_gate_residual_fwd(const void* x, const void* y, const float* mod, int gate_off, int ld, void* out, int B, int N, int C,
                                    void* stream) {
    if (ad_check("tv_gate_residual_fwd", B, N, C, ld, GR_MAX_C)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && y && mod && out, "tv_gate_residual_fwd: null pointer");
    TV_CHECK_ARG(ad_range(gate_off, C, ld), "tv_gate_residual_fwd: column range %d + %d outside ld=%d", gate_off, C, ld);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 15) == 0, "tv_gate_residual_fwd: x / y / out must be 16-byte aligned");
    const long long total = (long long)B * N * (C >> 3);
    hipLaunchKernelGGL(gate_fwd_kernel, dim3(flow_blocks(total, 65536)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)y, mod, gate_off, ld,
                       (bf16*)out, total, N, C >> 3);
    TV_CHECK_LAUNCH("tv_gate_residual_fwd");
    return TV_OK;
}

extern "C" long long tv_gate_residual_bwd_partial_count(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return -1;
    return (long long)B * tv_cdiv(N, GR_RPB) * C;              // floats
}

extern "C" int tv_gate_residual_bwd(const void* dout, const void* y, const float* mod, int gate_off, int ld, void* dy, float* dmod, float* partials,
                                    int B, int N, int C, void* stream) {
    if (ad_check("tv_gate_residual_bwd", B, N, C, ld, GR_MAX_C)) return TV_ERR_ARG;
    TV_CHECK_ARG(dout && y && mod && dy && dmod && partials, "tv_gate_residual_bwd: null pointer");
    TV_CHECK_ARG(ad_range(gate_off, C, ld), "tv_gate_residual_bwd: column range %d + %d outside ld=%d", gate_off, C, ld);
    TV_CHECK_ARG((((uintptr_t)dout | (uintptr_t)y | (uintptr_t)dy) & 15) == 0, "tv_gate_residual_bwd: dout / y / dy must be 16-byte aligned");
    const int nblk = tv_cdiv(N, GR_RPB);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)dout, (const bf16*)y, mod, gate_off, ld, (bf16*)dy,
                       partials, N, C);
    TV_CHECK_LAUNCH("tv_gate_residual_bwd");
    hipLaunchKernelGGL(mod_finalize_kernel, dim3(tv_cdiv(C, 256), B), dim3(256), 0, (hipStream_t)stream, (const float*)partials, nullptr, dmod, nullptr, nblk, 1, C, ld,
                       gate_off, gate_off);
    TV_CHECK_LAUNCH("tv_gate_residual_bwd (finalise)");
    return TV_OK;
}

extern "C" int tv_flow_rows(const float* lat, long long sn, long long sc, const float* mean, const float* rstd, const float* noise, const float* t,
                            void* rows, int B, int D, int h, int w, int patch, int ld, void* stream) {
    FlowGeo g;
    if (flow_geo("tv_flow_rows", sn, sc, B, D, h, w, patch, ld, g)) return TV_ERR_ARG;
    TV_CHECK_ARG(lat && mean && rstd && rows && (!noise || t), "tv_flow_rows: null pointer (noise needs t)");
    TV_CHECK_ARG(((uintptr_t)rows & 15) == 0, "tv_flow_rows: rows must be 16-byte aligned");
    const long long total = (long long)B * g.N * g.ldv;
    hipLaunchKernelGGL(flow_rows_kernel, dim3(flow_blocks(total, 65536)), dim3(256), 0, (hipStream_t)stream, lat, mean, rstd, noise, t, (bf16*)rows, total, g);
    TV_CHECK_LAUNCH("tv_flow_rows");
    return TV_OK;
}

extern "C" long long tv_flow_loss_partial_count(int B, int D, int h, int w, int patch, int ld) {
    if (B <= 0 || D <= 0 || h <= 0 || w <= 0 || patch <= 0 || ld <= 0 || h % patch || w % patch) return -1;
    return flow_blocks((long long)B * (h / patch) * (w / patch) * (ld / 8), FL_MAX_BLOCKS);      // doubles
}

extern "C" int tv_flow_loss(const void* pred, const float* lat, long long sn, long long sc, const float* mean, const float* rstd, const float* noise,
                            void* dpred, double* out, double* partials, int B, int D, int h, int w, int patch, int ld, float grad_scale, void* stream) {
    FlowGeo g;
    if (flow_geo("tv_flow_loss", sn, sc, B, D, h, w, patch, ld, g)) return TV_ERR_ARG;
    TV_CHECK_ARG(pred && lat && mean && rstd && noise && out && partials, "tv_flow_loss: null pointer");
    TV_CHECK_ARG((((uintptr_t)pred | (uintptr_t)dpred) & 15) == 0 && (((uintptr_t)out | (uintptr_t)partials) & 7) == 0,
                 "tv_flow_loss: pred / dpred must be 16-byte aligned, out / partials 8-byte aligned");
    const long long total = (long long)B * g.N * g.ldv;
    const double count = (double)B * g.N * g.F;
    const unsigned nblk = flow_blocks(total, FL_MAX_BLOCKS);
    hipLaunchKernelGGL(flow_loss_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16*)pred, lat, mean, rstd, noise, (bf16*)dpred, partials,
                       total, g, (float)(2.0 * (double)grad_scale / count));
    TV_CHECK_LAUNCH("tv_flow_loss");
    hipLaunchKernelGGL(flow_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, (int)nblk, count, out);
    TV_CHECK_LAUNCH("tv_flow_loss (finalise)");
    return TV_OK;
}

extern "C" int tv_flow_euler(float* x, const void* v, int B, int D, int h, int w, int patch, int ld, float dt, float cfg_scale, int guided,
                             void* stream) {
    FlowGeo g;
    if (flow_geo("tv_flow_euler", (long long)D * h * w, (long long)h * w, B, D, h, w, patch, ld, g)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && v, "tv_flow_euler: null pointer");
    TV_CHECK_ARG(((uintptr_t)v & 15) == 0, "tv_flow_euler: v must be 16-byte aligned");
    const long long total = (long long)B * g.N * g.ldv;
    hipLaunchKernelGGL(flow_euler_kernel, dim3(flow_blocks(total, 65536)), dim3(256), 0, (hipStream_t)stream, x, (const bf16*)v, total, total * 8, g, dt,
                       cfg_scale, guided ? 1 : 0);
    TV_CHECK_LAUNCH("tv_flow_euler");
    return TV_OK;
}

extern "C" long long tv_flow_loss_cos_partial_count(int B, int D, int h, int w, int patch, int ld) {
    const long long n = tv_flow_loss_partial_count(B, D, h, w, patch, ld);
    return n < 0 ? n : 2 * n;          // doubles: the squared-error partials, then the cosine partials
}

extern "C" int tv_flow_loss_cos(const void* pred, const float* lat, long long sn, long long sc, const float* mean, const float* rstd,
                                const float* noise, void* dpred, double* out, double* partials, int B, int D, int h, int w, int patch, int ld,
                                float cos_weight, float grad_scale, void* stream) {
    FlowGeo g;
    if (flow_geo("tv_flow_loss_cos", sn, sc, B, D, h, w, patch, ld, g)) return TV_ERR_ARG;
    TV_CHECK_ARG(pred && lat && mean && rstd && noise && out && partials, "tv_flow_loss_cos: null pointer");
    TV_CHECK_ARG((((uintptr_t)pred | (uintptr_t)dpred) & 15) == 0 && (((uintptr_t)out | (uintptr_t)partials) & 7) == 0,
                 "tv_flow_loss_cos: pred / dpred must be 16-byte aligned, out / partials 8-byte aligned");
    TV_CHECK_ARG(cos_weight >= 0.f && cos_weight < INFINITY, "tv_flow_loss_cos: cos_weight=%g must be finite and not negative", (double)cos_weight);
    const long long total = (long long)B * g.N * g.ldv;
    const double count = (double)B * g.N * g.F, count_pos = (double)B * g.h * g.w;
    const unsigned nblk = flow_blocks(total, FL_MAX_BLOCKS);
    hipLaunchKernelGGL(flow_loss_cos_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16*)pred, lat, mean, rstd, noise, (bf16*)dpred,
                       partials, total, g, (float)(2.0 * (double)grad_scale / count), (float)((double)grad_scale * (double)cos_weight / count_pos));
    TV_CHECK_LAUNCH("tv_flow_loss_cos");
    hipLaunchKernelGGL(flow_loss_cos_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, (int)nblk, count, count_pos,
                       (double)cos_weight, out);
    TV_CHECK_LAUNCH("tv_flow_loss_cos (finalise)");
    return TV_OK;
}

extern "C" int tv_flow_heun(float* x, const void* v1, const void* v2, int B, int D, int h, int w, int patch, int ld, float dt, float cfg_scale,
                            int guided1, int guided2, void* stream) {
    FlowGeo g;
    if (flow_geo("tv_flow_heun", (long long)D * h * w, (long long)h * w, B, D, h, w, patch, ld, g)) return TV_ERR_ARG;
    TV_CHECK_ARG(x && v1 && v2, "tv_flow_heun: null pointer");
    TV_CHECK_ARG((((uintptr_t)v1 | (uintptr_t)v2) & 15) == 0, "tv_flow_heun: v1 / v2 must be 16-byte aligned");
    const long long total = (long long)B * g.N * g.ldv;
    hipLaunchKernelGGL(flow_heun_kernel, dim3(flow_blocks(total, 65536)), dim3(256), 0, (hipStream_t)stream, x, (const bf16*)v1, (const bf16*)v2, total,
                       total * 8, g, 0.5f * dt, cfg_scale, guided1 ? 1 : 0, guided2 ? 1 : 0);
    TV_CHECK_LAUNCH("tv_flow_heun");
    return TV_OK;
}
