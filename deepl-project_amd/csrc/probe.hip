// Linear probing of latents: the classifier's bf16 operand (tv_probe_rows) and the softmax cross-entropy with its gradient and
// accuracy counts (tv_softmax_xent).  transvae/probe.py drives both; the classifier itself is a tv_igemm_nt / tv_wgrad_tn pair.
//
// tv_probe_rows.  fp32 latents [B, D, h, w] (batch and channel strides free) -> bf16 rows [B, ld]: every channel average-pooled to
// a gh x gw grid (fp32 sum of the window in scan order, one multiply by 1 / window), standardised ((v - mean_c) * rstd_c, two
// roundings, no contraction), rounded once to bf16.  Column (py * gw + px) * D + c; columns F = gh gw D .. ld - 1 are 0.  One thread
// owns 8 columns (one 16-byte store).  With D a multiple of 8 a wave's loads of one element index cover whole 64-byte pieces of
// (D / 8 .. 4) channel planes, and every byte fetched is used by that wave within its eight loads.
//
// tv_softmax_xent.  bf16 logits [B, ld], columns 0 .. n - 1 valid.  One wave owns a row; with n <= 4096 the row lives in
// registers (NV = 1 / 2 / 4 / 8 16-byte vectors per lane, read once), above that the same three sweeps read memory.
//   sweep 1   m = max x; rank of the label: columns with x > x_y, plus columns j < y with x == x_y
//   sweep 2   s = sum exp(x - m), q = sum (m - x)     (fp32, per lane in column order, then a butterfly with fixed pairing)
//   sweep 3   dlogits = scale * (exp(x - m) / s - target), target = (1 - eps) [j == y] + eps / n, fp32, rounded once
// The row loss lse - (1 - eps) x_y - (eps / n) sum x is formed as log s + (1 - eps)(m - x_y) + (eps / n) q: the same number as a
// sum of non-negative terms, so a saturated row (x_y = m, s = 1) gives exactly 0; the three products are fp64.  A row whose label
// is outside [0, n) gets a zero gradient row and is not counted.  Each wave adds its rows' {loss, rows, top-1, top-5} in row order in
// fp64, a block adds its four waves in order, and a one-wave finalise adds the block partials (lane l: blocks l, l + 64, ... in
// order, then a butterfly) to the state: no atomics, the same bits on every run.
//
// Algorithmic bytes per call (what tools/probe_bench.py divides by kernel time):
//   tv_probe_rows     4 B D h w read + 2 B ld written
//   tv_softmax_xent   2 B ld read + 2 B ld written (+ 8 B labels); evaluation (dlogits NULL): the read alone
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int SX_THREADS = 256;            // 4 waves = 4 rows in flight per block
constexpr int SX_WAVES = SX_THREADS / 64;
constexpr int SX_MAX_BLOCKS = 2048;
constexpr int SX_REG_CLASSES = 4096;       // the row fits 8 vectors per lane up to here

inline int sx_blocks(int B) {
    const int n = tv_cdiv(B, SX_WAVES);
    return n < SX_MAX_BLOCKS ? n : SX_MAX_BLOCKS;
}

__global__ __launch_bounds__(256) void probe_rows_kernel(const float* __restrict__ x, long long sn, long long sc,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         bf16* __restrict__ rows, long long total, int D, int w, int gw, int wh, int ww, int F,
                                                         int ldv, float inv_win) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int piece = (int)(idx % ldv);
        const long long b = idx / ldv;
        int col = piece * 8;
        int c = col % D, cell = col / D;
        bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e, ++col) {
            if (col < F) {
                const int py = cell / gw, px = cell - py * gw;
                const float* __restrict__ src = x + b * sn + (long long)c * sc + (long long)(py * wh) * w + px * ww;
                float s = 0.f;
                for (int i = 0; i < wh; ++i)
                    for (int j = 0; j < ww; ++j) s += src[i * w + j];
                const float v = s * inv_win;
                o[e] = (bf16)((v - mean[c]) * rstd[c]);
            }
            if (++c == D) { c = 0; ++cell; }
        }
        *(bf16x8*)(rows + idx * 8) = o;
    }
}

__device__ __forceinline__ int sx_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// exp(-d), d >= 0: v_exp_f32 of one rounded product.  Results below the smallest normal may flush to 0
__device__ __forceinline__ float sx_exp_neg(float d) { return __builtin_amdgcn_exp2f(d * -1.44269504088896340736f); }

// NV > 0: the row's vectors lane, lane + 64, ... live in registers; NV == 0: every sweep reads them from memory
template <int NV>
__global__ __launch_bounds__(SX_THREADS) void softmax_xent_kernel(const bf16* __restrict__ logits, const long long* __restrict__ labels,
                                                                  bf16* __restrict__ dlogits, double* __restrict__ partials, int B, int n, int ld,
                                                                  float eps, float scale) {
    __shared__ double wpart[SX_WAVES][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = (n + 7) >> 3, ldv = ld >> 3;          // vectors that hold a valid column (nvec <= ldv); vectors of a row
    const int iters = NV > 0 ? NV : (nvec + 63) >> 6;
    const float t_hit = (1.0f - eps) + eps / (float)n, t_miss = eps / (float)n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int row = blockIdx.x * SX_WAVES + wave; row < B; row += gridDim.x * SX_WAVES) {     // (wave-uniform)
        const bf16* __restrict__ xr = logits + (size_t)row * ld;
        bf16* __restrict__ dr = dlogits ? dlogits + (size_t)row * ld : nullptr;
        const long long y = labels[row];
        const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
        if (y < 0 || y >= n) {                                // ignored: a zero gradient row, nothing counted
            if (dr)
                for (int v = lane; v < ldv; v += 64) *(bf16x8*)(dr + v * 8) = zero;
            continue;
        }
        const float xy = (float)xr[y];
        bf16x8 reg[NV > 0 ? NV : 1];
        if constexpr (NV > 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int v = lane + 64 * k;
                reg[k] = v < nvec ? *(const bf16x8*)(xr + v * 8) : zero;
            }
        }
        auto vec = [&](int k, int v) -> bf16x8 {
            if constexpr (NV > 0) return reg[k];
            else return *(const bf16x8*)(xr + v * 8);
        };
        // sweep 1
        float m = -INFINITY;
        int gt = 0, eqlo = 0;
#pragma unroll(NV > 0 ? NV : 1)
        for (int k = 0; k < iters; ++k) {
            const int v = lane + 64 * k;
            if (v < nvec) {
                const bf16x8 xv = vec(k, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int j = v * 8 + e;
                    const float xf = (float)xv[e];
                    if (j < n) {
                        m = fmaxf(m, xf);
                        gt += xf > xy;
                        eqlo += (xf == xy) & (j < (int)y);
                    }
                }
            }
        }
        m = tv_wave_max(m);
        const int rank = sx_wave_sum(gt) + sx_wave_sum(eqlo);
        // sweep 2
        float s = 0.f, q = 0.f;
#pragma unroll(NV > 0 ? NV : 1)
        for (int k = 0; k < iters; ++k) {
            const int v = lane + 64 * k;
            if (v < nvec) {
                const bf16x8 xv = vec(k, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (v * 8 + e < n) {
                        const float d = m - (float)xv[e];
                        s += sx_exp_neg(d);
                        q += d;
                    }
                }
            }
        }
        s = tv_wave_sum(s);
        q = tv_wave_sum(q);
        acc[0] += (double)logf(s) + (1.0 - (double)eps) * (double)(m - xy) + ((double)eps / (double)n) * (double)q;
        acc[1] += 1.0;
        acc[2] += rank == 0 ? 1.0 : 0.0;
        acc[3] += rank < 5 ? 1.0 : 0.0;
        // sweep 3
        if (dr) {
            const float inv = 1.0f / s;
#pragma unroll(NV > 0 ? NV : 1)
            for (int k = 0; k < iters; ++k) {
                const int v = lane + 64 * k;
                if (v < nvec) {
                    const bf16x8 xv = vec(k, v);
                    bf16x8 o;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int j = v * 8 + e;
                        const float p = sx_exp_neg(m - (float)xv[e]) * inv;
                        o[e] = j < n ? (bf16)(scale * (p - (j == (int)y ? t_hit : t_miss))) : (bf16)0.f;
                    }
                    *(bf16x8*)(dr + v * 8) = o;
                }
            }
            for (int v = nvec + lane; v < ldv; v += 64) *(bf16x8*)(dr + v * 8) = zero;     // whole pad vectors
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wpart[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int wv = 0; wv < SX_WAVES; ++wv) t += wpart[wv][threadIdx.x];
        partials[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void softmax_xent_finalize_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ state) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nblk; k += 64) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] += partials[(size_t)k * 4 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[i] += __shfl_xor(a[i], o, 64);
    }
    if (threadIdx.x < 4) state[threadIdx.x] += a[threadIdx.x];
}

template <int NV>
void sx_launch(int nblk, hipStream_t s, const bf16* logits, const long long* labels, bf16* dlogits, double* partials, int B, int n, int ld,
               float eps, float scale) {
    hipLaunchKernelGGL(softmax_xent_kernel<NV>, dim3(nblk), dim3(SX_THREADS), 0, s, logits, labels, dlogits, partials, B, n, ld, eps, scale);
}

}  // namespace

extern "C" int tv_probe_rows(const float* x, long long sn, long long sc, const float* mean, const float* rstd, void* rows, int B, int D, int h,
                             int w, int gh, int gw, int ld, void* stream) {
    TV_CHECK_ARG(x && mean && rstd && rows && B > 0 && D > 0 && h > 0 && w > 0, "tv_probe_rows: bad arguments");
    TV_CHECK_ARG(gh > 0 && gw > 0 && h % gh == 0 && w % gw == 0, "tv_probe_rows: the pooled grid %d x %d must divide the latent grid %d x %d", gh, gw,
                 h, w);
    const long long F = (long long)gh * gw * D;
    TV_CHECK_ARG(ld % 32 == 0 && ld >= F && (long long)ld < (1ll << 30), "tv_probe_rows: ld=%d must be a multiple of 32 and cover %lld columns", ld, F);
    TV_CHECK_ARG(sc >= (long long)h * w && sn >= (long long)(D - 1) * sc + (long long)h * w,
                 "tv_probe_rows: strides (%lld, %lld) overlap for D=%d, h=%d, w=%d", sn, sc, D, h, w);
    TV_CHECK_ARG(((uintptr_t)rows & 15) == 0, "tv_probe_rows: rows must be 16-byte aligned");
    const int ldv = ld / 8, wh = h / gh, ww = w / gw;
    const long long total = (long long)B * ldv;
    long long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(probe_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, sn, sc, mean, rstd, (bf16*)rows, total, D, w, gw,
                       wh, ww, (int)F, ldv, (float)(1.0 / (double)(wh * ww)));
    TV_CHECK_LAUNCH("tv_probe_rows");
    return TV_OK;
}

extern "C" long long tv_softmax_xent_partial_count(int B) {
    if (B <= 0) return -1;
    return 4ll * sx_blocks(B);                   // doubles
}

extern "C" int tv_softmax_xent(const void* logits, const long long* labels, void* dlogits, double* state, double* partials, int B, int n_classes,
                               int ld, float label_smoothing, float grad_scale, void* stream) {
    TV_CHECK_ARG(logits && labels && state && partials && B > 0, "tv_softmax_xent: logits, labels, state, partials are required");
    TV_CHECK_ARG(n_classes >= 2 && ld % 8 == 0 && ld >= n_classes, "tv_softmax_xent: n_classes=%d (at least 2), ld=%d (a multiple of 8, >= n_classes)",
                 n_classes, ld);
    TV_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 1.f, "tv_softmax_xent: label_smoothing must be in [0, 1)");
    TV_CHECK_ARG((((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0 && (((uintptr_t)state | (uintptr_t)partials | (uintptr_t)labels) & 7) == 0,
                 "tv_softmax_xent: logits / dlogits must be 16-byte aligned, labels / state / partials 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = sx_blocks(B), nvec = (n_classes + 7) / 8;
    const bf16* lg = (const bf16*)logits;
    bf16* dl = (bf16*)dlogits;
    if (n_classes > SX_REG_CLASSES) sx_launch<0>(nblk, s, lg, labels, dl, partials, B, n_classes, ld, label_smoothing, grad_scale);
    else if (nvec <= 64) sx_launch<1>(nblk, s, lg, labels, dl, partials, B, n_classes, ld, label_smoothing, grad_scale);
    else if (nvec <= 128) sx_launch<2>(nblk, s, lg, labels, dl, partials, B, n_classes, ld, label_smoothing, grad_scale);
    else if (nvec <= 256) sx_launch<4>(nblk, s, lg, labels, dl, partials, B, n_classes, ld, label_smoothing, grad_scale);
    else sx_launch<8>(nblk, s, lg, labels, dl, partials, B, n_classes, ld, label_smoothing, grad_scale);
    TV_CHECK_LAUNCH("tv_softmax_xent");
    hipLaunchKernelGGL(softmax_xent_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, nblk, state);
    TV_CHECK_LAUNCH("tv_softmax_xent (finalise)");
    return TV_OK;
}
