// The parts of the LPIPS (VGG-16) perceptual term that are not a convolution: input preparation and its adjoint, 2x2 max-pool
// forward / backward, and the per-tap head (unit-normalise over channels, weighted squared difference, spatial mean) with its
// gradient.  The thirteen convolutions are tv_igemm_nt launches with the ReLU epilogue (TV_ACTX_RELU).
//
// All four are bandwidth kernels: 16-byte accesses on the bf16 NHWC tensors, no LDS except the head's block sum, 64-bit element
// indices (a 2B-image batch of 64-channel 256 x 256 activations is above 2 GiB).
//
// Algorithmic bytes (what tools/lpips_bench.py divides by kernel time), per call, activations bf16:
//   tv_maxpool2x2_fwd   2 * B*H*W*C read + 2 * B*(H/2)*(W/2)*C written                                  = 2.5  B*H*W*C
//   tv_maxpool2x2_bwd   2 * B*H*W*C (x) + 0.5 * B*H*W*C (gy) [+ 2 * B*H*W*C (add)] read, 2 * B*H*W*C written = 4.5 [6.5] B*H*W*C
//   tv_lpips_head       2 * 2 * B*HW*C read (x and t, once each) [+ 2 * B*HW*C gradient written]         = 4 [6] B*HW*C
#include "common.h"

// no implicit FMA contraction: f_c - g_c must be exactly 0 for identical inputs (a contracted x*a - (t*b) keeps the rounding
// residue of one product), and the fused operations below are written out as fmaf
#pragma clang fp contract(off)

namespace {

constexpr int PREP_MAP = 1, PREP_SIGMOID = 2, PREP_CLAMP = 4;

// ---------------------------------------------------------------------------------------------------------------------
// max-pool 2x2 / stride 2, floor semantics (a trailing odd row / column belongs to no window)
// ---------------------------------------------------------------------------------------------------------------------
// torch's scan (aten/native/cpu/MaxPoolKernel, the CUDA kernel alike): rows then columns, a later element replaces the
// running maximum only if it is GREATER or NaN -- so of equal maxima the first in (dy, dx) order wins.
__device__ __forceinline__ void pool_scan(const bf16x8& a, const bf16x8& b, const bf16x8& c, const bf16x8& d, bf16x8& mx, int (&arg)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float m = (float)a[e];
        int k = 0;
        const float vb = (float)b[e], vc = (float)c[e], vd = (float)d[e];
        if (vb > m || vb != vb) { m = vb; k = 1; }
        if (vc > m || vc != vc) { m = vc; k = 2; }
        if (vd > m || vd != vd) { m = vd; k = 3; }
        mx[e] = k == 0 ? a[e] : (k == 1 ? b[e] : (k == 2 ? c[e] : d[e]));
        arg[e] = k;
    }
}

__global__ __launch_bounds__(256) void maxpool2x2_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, long long total, int H, int W,
                                                             int C) {
    const int cv = C >> 3, Ho = H >> 1, Wo = W >> 1;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const long long pix = idx / cv;
        const int ox = (int)(pix % Wo);
        const long long r = pix / Wo;
        const int oy = (int)(r % Ho);
        const long long b = r / Ho;
        const bf16* s = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + v * 8;   // 2*oy+1 < H and 2*ox+1 < W by the floor
        const bf16x8 a = *(const bf16x8*)s, bq = *(const bf16x8*)(s + C), c = *(const bf16x8*)(s + (size_t)W * C),
                     d = *(const bf16x8*)(s + (size_t)W * C + C);
        bf16x8 mx;
        int arg[8];
        pool_scan(a, bq, c, d, mx, arg);
        *(bf16x8*)(y + idx * 8) = mx;
    }
}

// gx = route(gy) [+ add] [masked by x > 0].  One thread per 2x2 CELL of the input grid (cells = ceil(H/2) x ceil(W/2)) and 8
// channels: the argmax is recomputed from the saved input x, every input pixel is written exactly once; pixels of a trailing
// odd row / column get no routed gradient.  `add`: a second gradient of the same tensor (the LPIPS head's at a tap) joined here
// in one fp32 sum with one rounding; `relu_mask`: x is a ReLU output and gx is wanted w.r.t. its pre-activation.
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ gy, const bf16* __restrict__ add,
                                                             bf16* __restrict__ gx, long long total, int H, int W, int C, int relu_mask) {
    const int cv = C >> 3, Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const long long pix = idx / cv;
        const int cx = (int)(pix % Wc);
        const long long r = pix / Wc;
        const int cy = (int)(r % Hc);
        const long long b = r / Hc;
        const bool in_y = 2 * cy + 1 < H, in_x = 2 * cx + 1 < W;     // the cell's second row / column exists
        const bool window = cy < Ho && cx < Wo;                      // (== in_y && in_x)
        const size_t o00 = (((size_t)b * H + 2 * cy) * W + 2 * cx) * C + v * 8;
        const size_t off[4] = {o00, o00 + C, o00 + (size_t)W * C, o00 + (size_t)W * C + C};
        const bool ok[4] = {true, in_x, in_y, in_x && in_y};
        bf16x8 xv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = ok[k] ? *(const bf16x8*)(x + off[k]) : zero8;
        bf16x8 g = zero8, mx;
        int arg[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) arg[e] = -1;
        if (window) {
            g = *(const bf16x8*)(gy + ((((size_t)b * Ho + cy) * Wo + cx) * C + v * 8));
            pool_scan(xv[0], xv[1], xv[2], xv[3], mx, arg);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            bf16x8 o;
            if (add) {
                const bf16x8 av = *(const bf16x8*)(add + off[k]);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)((arg[e] == k ? (float)g[e] : 0.f) + (float)av[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = arg[e] == k ? g[e] : (bf16)0.f;
            }
            if (relu_mask) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (float)xv[k][e] > 0.f ? o[e] : (bf16)0.f;
            }
            *(bf16x8*)(gx + off[k]) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// input preparation: fp32 NCHW image -> rows of 3x3 / pad-1 patches of the SCALED image, (ky, kx, c) order, 32 bf16 per pixel
// (27 used), the operand of conv1_1 as a K = 32 GEMM.  Per element, in this order (P/transvae/losses/vae_loss.py:80-91 and
// lpips.LPIPS.forward): sigmoid, 2x - 1, clamp to [-1, 1], then LPIPS's scaling layer (v - shift_c) / scale_c.  The
// convolution's zero padding applies to the scaled image, so out-of-image taps are 0.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float prep_value(float v, int flags, float shift, float scale) {
    if (flags & PREP_SIGMOID) v = tv_sigmoid(v);
    if (flags & PREP_MAP) v = fmaf(2.f, v, -1.f);
    if (flags & PREP_CLAMP) v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);   // torch.clamp: a NaN passes through (fminf / fmaxf drop it)
    return (v - shift) / scale;
}

// images b < B0 come from `a` (flags_a), the others from `bsrc` (flags_b): reconstruction and target as one batch
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ a, const float* __restrict__ bsrc, bf16* __restrict__ dst,
                                                         long long total, int B0, int H, int W, int flags_a, int flags_b,
                                                         const float* __restrict__ shift_scale) {
    float sh[3], sc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { sh[c] = shift_scale[c]; sc[c] = shift_scale[3 + c]; }
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx & 3);
        const long long pix = idx >> 2;
        const int x = (int)(pix % W);
        const long long r = pix / W;
        const int y = (int)(r % H);
        const long long b = r / H;
        const bool first = b < B0;
        const float* src = first ? a + (size_t)b * 3 * H * W : bsrc + (size_t)(b - B0) * 3 * H * W;
        const int flags = first ? flags_a : flags_b;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = v * 8 + e;
            float f = 0.f;
            if (k < 27) {
                const int tap = k / 3, c = k - tap * 3;
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                    f = prep_value(src[((size_t)c * H + iy) * W + ix], flags, sh[c], sc[c]);
            }
            o[e] = (bf16)f;
        }
        *(bf16x8*)(dst + idx * 8) = o;
    }
}

// adjoint: dcols [B, H, W, 32] bf16 (gradient of the patch rows) -> fp32 NCHW gradient of the image that was prepared with `flags`.
// One thread per pixel: the 9 patch rows that hold this pixel, 3 channels each, summed in fp32 in tap order.
__global__ __launch_bounds__(256) void lpips_prep_bwd_kernel(const bf16* __restrict__ dcols, const float* __restrict__ src, float* __restrict__ dst,
                                                             long long total, int H, int W, int flags, const float* __restrict__ shift_scale) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x = (int)(idx % W);
        const long long r = idx / W;
        const int y = (int)(r % H);
        const long long b = r / H;
        float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int py = y - (tap / 3) + 1, px = x - (tap % 3) + 1;   // the patch whose tap (ky, kx) is this pixel
            if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) {
                const bf16* row = dcols + (((size_t)b * H + py) * W + px) * 32 + tap * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] += (float)row[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t o = (((size_t)b * 3 + c) * H + y) * W + x;
            float gv = g[c] / shift_scale[3 + c];
            if (flags & (PREP_SIGMOID | PREP_CLAMP)) {
                float v = src[o], ds = 1.f;
                if (flags & PREP_SIGMOID) { v = tv_sigmoid(v); ds = v * (1.f - v); }
                if (flags & PREP_MAP) v = fmaf(2.f, v, -1.f);
                if ((flags & PREP_CLAMP) && !(v >= -1.f && v <= 1.f)) ds = 0.f;   // (torch.clamp's gradient: 1 on the closed interval)
                gv *= ds;
            }
            if (flags & PREP_MAP) gv *= 2.f;
            dst[o] = gv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// LPIPS head of one tap.  feat [2B, HW, C]: images 0..B-1 are x (reconstruction), B..2B-1 are t (target).  Per pixel
//     f = x / (sqrt(sum_c x_c^2) + 1e-10),  g likewise from t,  d = sum_c w_c (f_c - g_c)^2 ;  out[b] (+)= mean_pixels d
// and, when `grad` is given,  grad[b, p, k] = scale * a (s_k - x_k a S / n)  with n = sqrt(sum x^2), a = 1 / (n + 1e-10),
// s_k = 2 w_k (f_k - g_k), S = sum_c s_c x_c, scale = upstream / HW -- the derivative of the above; a pixel with n == 0 gets a
// zero gradient (x is a ReLU output there: its pre-activation gradient is masked to zero anyway, and the formula is 0/0).
//
// A pixel's C channels sit in registers of C/8 neighbouring lanes, 8 consecutive channels (one 16-byte load) per lane: at
// C = 512 one wave owns one pixel, at C = 64 eight pixels; both inputs are read once, every sum is fp32.  Sums over channels:
// 8 sequential adds per lane, then an xor-butterfly over the C/8 lanes.  Sums over pixels: each lane adds its own pixels in
// order, a butterfly over the wave, the block's 4 waves in order -> partial[b][block]; the finalise kernel adds an image's
// partials in block order.  The block count depends on HW and C only, so a value does not depend on the batch around it.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HEAD_ITERS = 16;   // pixel groups per wave
__host__ __device__ inline int head_pixels_per_block(int C) { return 4 * (512 / C) * HEAD_ITERS; }

__global__ __launch_bounds__(256) void lpips_head_kernel(const bf16* __restrict__ feat, const float* __restrict__ w, float* __restrict__ partial,
                                                         bf16* __restrict__ grad, int B, int HW, int C, float scale) {
    __shared__ float wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lpp = C >> 3;                 // lanes per pixel (a power of two, <= 64)
    const int ppw = 64 / lpp;               // pixels per wave and iteration
    const int sub = lane / lpp, cl = lane - sub * lpp;
    const int b = blockIdx.y;
    const int ppb = head_pixels_per_block(C);
    const int p_begin = blockIdx.x * ppb;
    const bf16* xb = feat + (size_t)b * HW * C;
    const bf16* tb = feat + (size_t)(B + b) * HW * C;
    float wv[8];
    {
        const f32x4 w0 = *(const f32x4*)(w + cl * 8), w1 = *(const f32x4*)(w + cl * 8 + 4);
        wv[0] = w0[0]; wv[1] = w0[1]; wv[2] = w0[2]; wv[3] = w0[3]; wv[4] = w1[0]; wv[5] = w1[1]; wv[6] = w1[2]; wv[7] = w1[3];
    }
    float acc = 0.f;
    for (int it = 0; it < HEAD_ITERS; ++it) {
        const int p = p_begin + (it * 4 + wave) * ppw + sub;
        const bool ok = p < HW;             // (lanes past the image take part in the butterflies with zeros)
        const size_t o = (size_t)(ok ? p : 0) * C + cl * 8;
        bf16x8 xv = *(const bf16x8*)(xb + o), tv = *(const bf16x8*)(tb + o);
        float xf[8], tf[8], sx = 0.f, st = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xf[e] = ok ? (float)xv[e] : 0.f;
            tf[e] = ok ? (float)tv[e] : 0.f;
            sx = fmaf(xf[e], xf[e], sx);
            st = fmaf(tf[e], tf[e], st);
        }
        for (int m = 1; m < lpp; m <<= 1) {
            sx += __shfl_xor(sx, m, 64);
            st += __shfl_xor(st, m, 64);
        }
        const float nx = sqrtf(sx), nt = sqrtf(st);
        const float ax = 1.f / (nx + 1e-10f), at = 1.f / (nt + 1e-10f);
        float s[8], d = 0.f, S = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float df = xf[e] * ax - tf[e] * at;
            d = fmaf(wv[e] * df, df, d);
            s[e] = 2.f * wv[e] * df;
            S = fmaf(s[e], xf[e], S);
        }
        for (int m = 1; m < lpp; m <<= 1) {
            d += __shfl_xor(d, m, 64);
            S += __shfl_xor(S, m, 64);
        }
        if (cl == 0) acc += d;              // (d of a masked pixel is 0)
        if (grad && ok) {
            bf16x8 gv;
            const float k = nx > 0.f ? S * ax / nx : 0.f;
            const float sa = nx > 0.f ? scale * ax : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) gv[e] = (bf16)(sa * (s[e] - xf[e] * k));
            *(bf16x8*)(grad + (size_t)b * HW * C + o) = gv;
        }
    }
    acc = tv_wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void lpips_head_finalize_kernel(const float* __restrict__ partial, float* __restrict__ out, int B, int nblk,
                                                                 float inv_hw, int accumulate) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += partial[(size_t)b * nblk + i];
    s *= inv_hw;
    out[b] = accumulate ? out[b] + s : s;
}

inline int bw_grid(long long n) {
    long long g = (n + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" int tv_maxpool2x2_fwd(const void* x, void* y, int B, int H, int W, int C, void* stream) {
    TV_CHECK_ARG(x && y && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0, "tv_maxpool2x2_fwd: needs H, W >= 2 and C %% 8 == 0 (got %dx%dx%d)", H, W, C);
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(maxpool2x2_fwd_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)y, total, H, W, C);
    TV_CHECK_LAUNCH("tv_maxpool2x2_fwd");
    return TV_OK;
}

extern "C" int tv_maxpool2x2_bwd(const void* x, const void* gy, const void* add, void* gx, int B, int H, int W, int C, int relu_mask, void* stream) {
    TV_CHECK_ARG(x && gy && gx && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0, "tv_maxpool2x2_bwd: needs H, W >= 2 and C %% 8 == 0 (got %dx%dx%d)", H, W, C);
    const long long total = (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
    hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)gy,
                       (const bf16*)add, (bf16*)gx, total, H, W, C, relu_mask);
    TV_CHECK_LAUNCH("tv_maxpool2x2_bwd");
    return TV_OK;
}

extern "C" int tv_lpips_prep(const float* a, const float* b, void* cols, int Ba, int Bb, int H, int W, int flags_a, int flags_b,
                             const float* shift_scale, void* stream) {
    TV_CHECK_ARG(a && cols && shift_scale && Ba > 0 && Bb >= 0 && (Bb == 0 || b) && H > 0 && W > 0, "tv_lpips_prep: bad arguments");
    TV_CHECK_ARG(((flags_a | flags_b) & ~7) == 0, "tv_lpips_prep: unknown flags");
    const long long total = (long long)(Ba + Bb) * H * W * 4;
    hipLaunchKernelGGL(lpips_prep_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, a, b, (bf16*)cols, total, Ba, H, W, flags_a,
                       flags_b, shift_scale);
    TV_CHECK_LAUNCH("tv_lpips_prep");
    return TV_OK;
}

extern "C" int tv_lpips_prep_bwd(const void* dcols, const float* a, float* da, int B, int H, int W, int flags, const float* shift_scale,
                                 void* stream) {
    TV_CHECK_ARG(dcols && a && da && shift_scale && B > 0 && H > 0 && W > 0 && (flags & ~7) == 0, "tv_lpips_prep_bwd: bad arguments");
    const long long total = (long long)B * H * W;
    hipLaunchKernelGGL(lpips_prep_bwd_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)dcols, a, da, total, H, W, flags,
                       shift_scale);
    TV_CHECK_LAUNCH("tv_lpips_prep_bwd");
    return TV_OK;
}

extern "C" long long tv_lpips_head_partial_count(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C < 8 || C > 512 || (C & (C - 1))) return -1;
    return (long long)B * tv_cdiv(HW, head_pixels_per_block(C));
}

extern "C" int tv_lpips_head(const void* feat, const float* w, float* partials, float* out, void* grad, int B, int HW, int C, float upstream,
                             int accumulate, void* stream) {
    TV_CHECK_ARG(feat && w && partials && out && B > 0 && B <= 65535 && HW > 0, "tv_lpips_head: bad arguments (B=%d, HW=%d)", B, HW);
    TV_CHECK_ARG(C >= 8 && C <= 512 && (C & (C - 1)) == 0, "tv_lpips_head: C=%d must be a power of two in [8, 512]", C);
    const int nblk = tv_cdiv(HW, head_pixels_per_block(C));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, s, (const bf16*)feat, w, partials, (bf16*)grad, B, HW, C,
                       upstream / (float)HW);
    TV_CHECK_LAUNCH("tv_lpips_head");
    hipLaunchKernelGGL(lpips_head_finalize_kernel, dim3((unsigned)tv_cdiv(B, 64)), dim3(64), 0, s, partials, out, B, nblk, 1.f / (float)HW, accumulate);
    TV_CHECK_LAUNCH("tv_lpips_head (finalise)");
    return TV_OK;
}
