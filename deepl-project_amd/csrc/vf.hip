// The VF alignment term (R/transvae/losses/vae_loss.py:119-196): what the DINOv2 ViT feature extractor needs besides GEMMs,
// attention and LayerNorm, and the loss head.
//
//   tv_vf_prep            fp32 NCHW image -> bilinear resize -> (optional) ImageNet normalisation -> 14x14 / stride-14 patch rows
//                         [B*gh*gw, 608] bf16 (588 = 3*14*14 used, (c, ky, kx) order: the flattened patch-embedding weight)
//   tv_vit_tokens         bf16 patch embeddings + fp32 position table (+ cls) -> token matrix [B, 1 + P, D] bf16
//   tv_vf_head            latent (resized on the fly) -> projection -> cosine per position against the features -> value and
//                         d loss / d (resized latent), fp32 throughout, the mean in fp64 from block partials in block order
//   tv_vf_head_dproj      d proj.weight, d proj.bias from what the head saved; slab partials added in slab order
//   tv_bilinear_nchw_bwd  adjoint of the latent resize: every latent element gathers its contributions in a fixed order
//
// The plain LayerNorm (tv_rownorm_fwd mode 2, tv_layernorm_rows) lives with the other row norms in csrc/norm.hip.  Nothing here
// uses atomics: value, latent gradient and projection gradients have the same bits on every run.
#include "common.h"

namespace {

constexpr int VF_PATCH = 14;
constexpr int VF_K = 3 * VF_PATCH * VF_PATCH;   // 588
constexpr int VF_KPAD = 608;                    // 19 * 32: the GEMM's K granule
constexpr int VF_MAXDIM = 16384;                // (2 o + 1) n_in stays inside an int

// F.interpolate(mode='bilinear', align_corners=False): output index o of an axis resampled n_in -> n_out reads
// src = (o + 0.5) n_in / n_out - 0.5, clamped at 0, i.e. taps i0 = floor(src), i1 = min(i0 + 1, n_in - 1) with weights 1 - l, l.
// Integer arithmetic: src = num / den exactly, so l has ONE fp32 rounding (an fp32 src near 256 would leave l only 2^-16).
__device__ __forceinline__ void bilin_taps(int o, int n_in, int n_out, int& i0, int& i1, float& l) {
    const int num = (2 * o + 1) * n_in - n_out, den = 2 * n_out;
    if (num <= 0) {
        i0 = 0;
        l = 0.f;
    } else {
        i0 = num / den;
        l = (float)(num - i0 * den) / (float)den;
    }
    i1 = min(i0 + 1, n_in - 1);
}

__device__ __forceinline__ float bilin_sample(const float* __restrict__ p, int W, int y0, int y1, float ly, int x0, int x1, float lx) {
    const float top = (1.f - lx) * p[(size_t)y0 * W + x0] + lx * p[(size_t)y0 * W + x1];
    const float bot = (1.f - lx) * p[(size_t)y1 * W + x0] + lx * p[(size_t)y1 * W + x1];
    return (1.f - ly) * top + ly * bot;
}

// one thread per 8 columns of a patch row; the normalisation is applied to the fp32 sample, then ONE rounding to bf16
__global__ __launch_bounds__(256) void vf_prep_kernel(const float* __restrict__ img, bf16* __restrict__ rows, long long total, int H, int W, int gh,
                                                      int gw, int norm) {
    const int Ho = gh * VF_PATCH, Wo = gw * VF_PATCH;
    constexpr int VPR = VF_KPAD / 8;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % VPR);
        const long long t = idx / VPR;
        const int px = (int)(t % gw);
        const long long r = t / gw;
        const int py = (int)(r % gh);
        const long long b = r / gh;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = v * 8 + e;
            float f = 0.f;
            if (k < VF_K) {
                const int c = k / (VF_PATCH * VF_PATCH), rr = k - c * (VF_PATCH * VF_PATCH);
                const int ky = rr / VF_PATCH, kx = rr - ky * VF_PATCH;
                int y0, y1, x0, x1;
                float ly, lx;
                bilin_taps(py * VF_PATCH + ky, H, Ho, y0, y1, ly);
                bilin_taps(px * VF_PATCH + kx, W, Wo, x0, x1, lx);
                f = bilin_sample(img + ((size_t)b * 3 + c) * H * W, W, y0, y1, ly, x0, x1, lx);
                if (norm) {
                    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
                    const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
                    f = (f - mean) / sd;
                }
            }
            o[e] = (bf16)f;
        }
        *(bf16x8*)(rows + idx * 8) = o;
    }
}

// tok[b, 0] = cls + pos[0];  tok[b, 1 + p] = patch[b, p] + pos[1 + p]: one fp32 sum, one rounding
__global__ __launch_bounds__(256) void vit_tokens_kernel(const bf16* __restrict__ patch, const float* __restrict__ cls, const float* __restrict__ pos,
                                                         bf16* __restrict__ tok, long long total, int N, int D) {
    const int dv = D >> 3;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % dv);
        const long long row = idx / dv;
        const int n = (int)(row % N);
        const long long b = row / N;
        const float* pr = pos + (size_t)n * D + v * 8;
        float a[8];
        if (n == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = cls[v * 8 + e];
        } else {
            const bf16x8 pv = *(const bf16x8*)(patch + ((size_t)b * (N - 1) + (n - 1)) * D + v * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = (float)pv[e];
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)(a[e] + pr[e]);
        *(bf16x8*)(tok + idx * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// VF head.  Position t = (b, py, px) of the gh x gw feature grid:
//     z = bilinear sample of latent[b, :, :, :] (the identity when the grids agree)             [D]
//     y = W z + bias  (PROJ)  or  y = z  (D == C)                                                [C]
//     cos_t = y . f / (max(|y|, 1e-12) max(|f|, 1e-12))                                          F.normalize, eps 1e-12
//     similarity = mean_t cos_t ;  loss = max(margin - similarity, 0)
// One wave per position, lane c + 64 j owns channel c + 64 j: y is never stored.  With alpha = g / (ny nf), beta = g (y.f) / (ny^3 nf)
// (beta = 0 where |y| is clamped), g = -1 / T:   d loss / d y = alpha f - beta y,   d loss / d z = W^T (alpha f - beta y)
// -- the lanes accumulate A_d = sum_c f_c W_cd and B_d = sum_c y_c W_cd while W's rows are in registers, so W is read once.
// The gradient is written UNGATED; the finalise launch leaves gate = (margin - similarity >= 0) next to the value and the
// adjoint / projection-gradient launches that follow multiply by it (exact zeros when shut).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int VH_TOK_PER_WAVE = 4, VH_TOK_PER_BLOCK = 4 * VH_TOK_PER_WAVE;
constexpr float VH_EPS = 1e-12f;

template <int DP, bool PROJ>
__global__ __launch_bounds__(256) void vf_head_kernel(const float* __restrict__ lat, const float* __restrict__ feat, const float* __restrict__ Wp,
                                                      const float* __restrict__ bp, double* __restrict__ partials, float* __restrict__ dzr,
                                                      float* __restrict__ zr, float* __restrict__ ab, int T, int C, int D, int Hl, int Wl, int gh,
                                                      int gw, float gscale) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int i = 0; i < VH_TOK_PER_WAVE; ++i) {
        const int t = blockIdx.x * VH_TOK_PER_BLOCK + wave * VH_TOK_PER_WAVE + i;
        if (t >= T) break;   // (uniform over the wave)
        const int px = t % gw, r = t / gw, py = r % gh, b = r / gh;
        float zl = 0.f;
        if (lane < D) {
            int y0, y1, x0, x1;
            float ly, lx;
            bilin_taps(py, Hl, gh, y0, y1, ly);
            bilin_taps(px, Wl, gw, x0, x1, lx);
            zl = bilin_sample(lat + ((size_t)b * D + lane) * Hl * Wl, Wl, y0, y1, ly, x0, x1, lx);
            if (zr) zr[(size_t)t * D + lane] = zl;
        }
        float yf = 0.f, yy = 0.f, ff = 0.f;
        if constexpr (PROJ) {
            float z[DP], A[DP], Bv[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                z[d] = __shfl(zl, d, 64);
                A[d] = Bv[d] = 0.f;
            }
            for (int c = lane; c < C; c += 64) {
                const float f = feat[(size_t)t * C + c];
                const float* wr = Wp + (size_t)c * D;
                float w[DP];
#pragma unroll
                for (int d = 0; d < DP; ++d) w[d] = d < D ? wr[d] : 0.f;
                float y = bp[c];
#pragma unroll
                for (int d = 0; d < DP; ++d) y = fmaf(w[d], z[d], y);
                yf = fmaf(y, f, yf);
                yy = fmaf(y, y, yy);
                ff = fmaf(f, f, ff);
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    A[d] = fmaf(f, w[d], A[d]);
                    Bv[d] = fmaf(y, w[d], Bv[d]);
                }
            }
            yf = tv_wave_sum(yf);
            yy = tv_wave_sum(yy);
            ff = tv_wave_sum(ff);
            const float ny = sqrtf(yy), nf = sqrtf(ff);
            const float cy = fmaxf(ny, VH_EPS), cf = fmaxf(nf, VH_EPS);
            acc += (double)(yf / (cy * cf));
            const float alpha = gscale / (cy * cf);
            const float beta = ny > VH_EPS ? gscale * yf / (cy * cy * cy * cf) : 0.f;
            float mine = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const float g = tv_wave_sum(alpha * A[d] - beta * Bv[d]);
                if (lane == d) mine = g;
            }
            if (lane < D) dzr[(size_t)t * D + lane] = mine;
            if (ab && lane == 0) {
                ab[2 * (size_t)t] = alpha;
                ab[2 * (size_t)t + 1] = beta;
            }
        } else {   // D == C <= 64: lane c owns channel c
            const float f = lane < C ? feat[(size_t)t * C + lane] : 0.f;
            yf = tv_wave_sum(zl * f);
            yy = tv_wave_sum(zl * zl);
            ff = tv_wave_sum(f * f);
            const float ny = sqrtf(yy), nf = sqrtf(ff);
            const float cy = fmaxf(ny, VH_EPS), cf = fmaxf(nf, VH_EPS);
            acc += (double)(yf / (cy * cf));
            const float alpha = gscale / (cy * cf);
            const float beta = ny > VH_EPS ? gscale * yf / (cy * cy * cy * cf) : 0.f;
            if (lane < D) dzr[(size_t)t * D + lane] = alpha * f - beta * zl;
        }
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// out[0] = loss, out[1] = gate (1 when margin - similarity >= 0: torch.clamp's backward passes at equality), out[2] = similarity
__global__ void vf_head_finalize_kernel(const double* __restrict__ partials, float* __restrict__ out, int nblk, double inv_t, float margin) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += partials[k];
    const double sim = s * inv_t;
    const double m = (double)margin - sim;
    out[0] = m > 0.0 ? (float)m : 0.f;
    out[1] = m >= 0.0 ? 1.f : 0.f;
    out[2] = (float)sim;
}

// d proj.weight[c, :] = sum_t gy_tc z_t,  d proj.bias[c] = sum_t gy_tc,  gy_tc = alpha_t f_tc - beta_t (W_c . z_t + bias_c).
// One thread per channel (its W row and its gradient row in registers), a slab of positions per blockIdx.y.
constexpr int VH_SLABS = 64;
__host__ __device__ inline int vh_slabs(int T) { return T < VH_SLABS * 64 ? (T + 63) / 64 : VH_SLABS; }

template <int DP>
__global__ __launch_bounds__(256) void vf_head_dproj_kernel(const float* __restrict__ feat, const float* __restrict__ zr, const float* __restrict__ ab,
                                                            const float* __restrict__ Wp, const float* __restrict__ bp, float* __restrict__ part,
                                                            int T, int C, int D, int per_slab) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool ok = c < C;
    const int t0 = blockIdx.y * per_slab, t1 = min(T, t0 + per_slab);
    float w[DP], dw[DP], db = 0.f;
    const float bias = ok ? bp[c] : 0.f;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        w[d] = (ok && d < D) ? Wp[(size_t)c * D + d] : 0.f;
        dw[d] = 0.f;
    }
    for (int t = t0; t < t1; ++t) {
        const float f = ok ? feat[(size_t)t * C + c] : 0.f;
        const float alpha = ab[2 * (size_t)t], beta = ab[2 * (size_t)t + 1];
        float z[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) z[d] = d < D ? zr[(size_t)t * D + d] : 0.f;
        float y = bias;
#pragma unroll
        for (int d = 0; d < DP; ++d) y = fmaf(w[d], z[d], y);
        const float gy = alpha * f - beta * y;
        db += gy;
#pragma unroll
        for (int d = 0; d < DP; ++d) dw[d] = fmaf(gy, z[d], dw[d]);
    }
    if (ok) {
        float* dst = part + ((size_t)blockIdx.y * C + c) * (D + 1);
#pragma unroll
        for (int d = 0; d < DP; ++d)
            if (d < D) dst[d] = dw[d];
        dst[D] = db;
    }
}

__global__ __launch_bounds__(256) void vf_head_dproj_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gate,
                                                                     float* __restrict__ dw, float* __restrict__ db, int nslab, int C, int D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C * (D + 1)) return;
    const int c = i / (D + 1), d = i - c * (D + 1);
    float s = 0.f;
    if (gate[0] != 0.f)
        for (int k = 0; k < nslab; ++k) s += part[(size_t)k * C * (D + 1) + i];
    if (d < D) dw[(size_t)c * D + d] = s;
    else db[c] = s;
}

// dlat[b, d, Y, X] = gate * sum over the output positions (y, x) whose taps include (Y, X), rows then columns, of
// wy wx g[b, y, x, d];  g is token-major [B, gh, gw, D].  The candidate range is the inverse image of (Y - 1, Y + 1) with a
// margin; the taps themselves decide (the same integer arithmetic as the forward).
__device__ __forceinline__ void adj_range(int Y, int n_in, int n_out, int& lo, int& hi) {
    const float sc = (float)n_out / (float)n_in;
    lo = max(0, (int)floorf(((float)Y - 0.5f) * sc - 0.5f) - 1);
    hi = min(n_out - 1, (int)ceilf(((float)Y + 1.5f) * sc - 0.5f) + 1);
}
__device__ __forceinline__ float adj_weight(int o, int Y, int n_in, int n_out) {
    int i0, i1;
    float l;
    bilin_taps(o, n_in, n_out, i0, i1, l);
    return (i0 == Y ? 1.f - l : 0.f) + (i1 == Y ? l : 0.f);
}

__global__ __launch_bounds__(256) void bilinear_nchw_bwd_kernel(const float* __restrict__ g, const float* __restrict__ gate, float* __restrict__ dlat,
                                                                long long total, int D, int Hl, int Wl, int gh, int gw) {
    const bool shut = gate && gate[0] == 0.f;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int X = (int)(idx % Wl);
        long long r = idx / Wl;
        const int Y = (int)(r % Hl);
        r /= Hl;
        const int d = (int)(r % D);
        const long long b = r / D;
        float acc = 0.f;
        if (!shut) {
            int ylo, yhi, xlo, xhi;
            adj_range(Y, Hl, gh, ylo, yhi);
            adj_range(X, Wl, gw, xlo, xhi);
            for (int y = ylo; y <= yhi; ++y) {
                const float wy = adj_weight(y, Y, Hl, gh);
                if (wy == 0.f) continue;
                for (int x = xlo; x <= xhi; ++x) {
                    const float wx = adj_weight(x, X, Wl, gw);
                    if (wx == 0.f) continue;
                    acc = fmaf(wy * wx, g[(((size_t)b * gh + y) * gw + x) * D + d], acc);
                }
            }
        }
        dlat[idx] = acc;
    }
}

inline int vf_grid(long long n) {
    long long g = (n + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" int tv_vf_prep(const float* img, void* rows, int B, int H, int W, int gh, int gw, int imagenet_norm, void* stream) {
    TV_CHECK_ARG(img && rows && B > 0 && H > 0 && W > 0 && gh > 0 && gw > 0, "tv_vf_prep: bad arguments");
    TV_CHECK_ARG(H <= VF_MAXDIM && W <= VF_MAXDIM && gh * VF_PATCH <= VF_MAXDIM && gw * VF_PATCH <= VF_MAXDIM,
                 "tv_vf_prep: image sides above %d are not supported", VF_MAXDIM);
    TV_CHECK_ARG(((uintptr_t)rows & 15) == 0, "tv_vf_prep: rows must be 16-byte aligned");
    const long long total = (long long)B * gh * gw * (VF_KPAD / 8);
    hipLaunchKernelGGL(vf_prep_kernel, dim3(vf_grid(total)), dim3(256), 0, (hipStream_t)stream, img, (bf16*)rows, total, H, W, gh, gw, imagenet_norm);
    TV_CHECK_LAUNCH("tv_vf_prep");
    return TV_OK;
}

extern "C" int tv_vit_tokens(const void* patch, const float* cls, const float* pos, void* tok, int B, int n_patch, int D, void* stream) {
    TV_CHECK_ARG(patch && cls && pos && tok && B > 0 && n_patch > 0 && D > 0 && D % 8 == 0, "tv_vit_tokens: bad arguments (D %% 8 == 0)");
    TV_CHECK_ARG((((uintptr_t)patch | (uintptr_t)tok) & 15) == 0, "tv_vit_tokens: patch / tok must be 16-byte aligned");
    const long long total = (long long)B * (n_patch + 1) * (D / 8);
    hipLaunchKernelGGL(vit_tokens_kernel, dim3(vf_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)patch, cls, pos, (bf16*)tok, total,
                       n_patch + 1, D);
    TV_CHECK_LAUNCH("tv_vit_tokens");
    return TV_OK;
}

extern "C" long long tv_vf_head_partial_count(int T) { return T > 0 ? tv_cdiv(T, VH_TOK_PER_BLOCK) : -1; }

extern "C" int tv_vf_head(const float* lat, const float* feat, const float* w, const float* bias, void* partials, float* out, float* dzr, float* zr,
                          float* ab, int B, int D, int Hl, int Wl, int gh, int gw, int C, float margin, void* stream) {
    TV_CHECK_ARG(lat && feat && partials && out && dzr && B > 0 && D > 0 && Hl > 0 && Wl > 0 && gh > 0 && gw > 0 && C > 0, "tv_vf_head: bad arguments");
    TV_CHECK_ARG(Hl <= VF_MAXDIM && Wl <= VF_MAXDIM && gh <= VF_MAXDIM && gw <= VF_MAXDIM && (long long)B * gh * gw < (1ll << 31),
                 "tv_vf_head: grid too large");
    TV_CHECK_ARG(((uintptr_t)partials & 7) == 0, "tv_vf_head: partials must be 8-byte aligned");
    TV_CHECK_ARG((w != nullptr) == (bias != nullptr), "tv_vf_head: the projection has a weight and a bias, or neither");
    TV_CHECK_ARG(w ? D <= 32 : (D == C && D <= 64), "tv_vf_head: D=%d C=%d (projection: D <= 32; without one D == C <= 64)", D, C);
    TV_CHECK_ARG(!ab || (w && zr), "tv_vf_head: ab (for tv_vf_head_dproj) needs the projection and zr");
    const int T = B * gh * gw;
    const int nblk = tv_cdiv(T, VH_TOK_PER_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    const float gscale = -1.f / (float)T;
#define TV_VH(DP, PROJ) hipLaunchKernelGGL((vf_head_kernel<DP, PROJ>), dim3(nblk), dim3(256), 0, s, lat, feat, w, bias, (double*)partials, dzr, zr, ab, T, C, D, Hl, Wl, gh, gw, gscale)
    if (!w) TV_VH(1, false);
    else if (D <= 16) TV_VH(16, true);
    else TV_VH(32, true);
#undef TV_VH
    TV_CHECK_LAUNCH("tv_vf_head");
    hipLaunchKernelGGL(vf_head_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, out, nblk, 1.0 / (double)T, margin);
    TV_CHECK_LAUNCH("tv_vf_head (finalise)");
    return TV_OK;
}

extern "C" long long tv_vf_head_dproj_partial_count(int T, int C, int D) {
    if (T <= 0 || C <= 0 || D <= 0) return -1;
    return (long long)vh_slabs(T) * C * (D + 1);
}

extern "C" int tv_vf_head_dproj(const float* feat, const float* zr, const float* ab, const float* w, const float* bias, const float* gate,
                                float* partials, float* dw, float* db, int T, int C, int D, void* stream) {
    TV_CHECK_ARG(feat && zr && ab && w && bias && gate && partials && dw && db && T > 0 && C > 0 && D > 0 && D <= 32,
                 "tv_vf_head_dproj: bad arguments (D <= 32)");
    const int nslab = vh_slabs(T);
    const int per = tv_cdiv(T, nslab);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tv_cdiv(C, 256), (unsigned)nslab);
    if (D <= 16) hipLaunchKernelGGL(vf_head_dproj_kernel<16>, grid, dim3(256), 0, s, feat, zr, ab, w, bias, partials, T, C, D, per);
    else hipLaunchKernelGGL(vf_head_dproj_kernel<32>, grid, dim3(256), 0, s, feat, zr, ab, w, bias, partials, T, C, D, per);
    TV_CHECK_LAUNCH("tv_vf_head_dproj");
    hipLaunchKernelGGL(vf_head_dproj_finalize_kernel, dim3((unsigned)tv_cdiv((long long)C * (D + 1), 256)), dim3(256), 0, s, partials, gate, dw, db,
                       nslab, C, D);
    TV_CHECK_LAUNCH("tv_vf_head_dproj (finalise)");
    return TV_OK;
}

extern "C" int tv_bilinear_nchw_bwd(const float* g, const float* gate, float* dlat, int B, int D, int Hl, int Wl, int gh, int gw, void* stream) {
    TV_CHECK_ARG(g && dlat && B > 0 && D > 0 && Hl > 0 && Wl > 0 && gh > 0 && gw > 0, "tv_bilinear_nchw_bwd: bad arguments");
    TV_CHECK_ARG(Hl <= VF_MAXDIM && Wl <= VF_MAXDIM && gh <= VF_MAXDIM && gw <= VF_MAXDIM, "tv_bilinear_nchw_bwd: grid too large");
    const long long total = (long long)B * D * Hl * Wl;
    hipLaunchKernelGGL(bilinear_nchw_bwd_kernel, dim3(vf_grid(total)), dim3(256), 0, (hipStream_t)stream, g, gate, dlat, total, D, Hl, Wl, gh, gw);
    TV_CHECK_LAUNCH("tv_bilinear_nchw_bwd");
    return TV_OK;
}
