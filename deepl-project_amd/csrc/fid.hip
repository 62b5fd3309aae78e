// The parts of the rFID metric that are not a convolution: input preparation of the FID Inception-v3 (bilinear 299 x 299 resize,
// 2x - 1, patch rows of the first convolution), 3x3 pools, the row gather that turns a 1x7 / 7x1 / 1x3 / 3x1 convolution into a
// GEMM, global average pooling, and the streaming fp64 moments of the pool3 features.  The 94 convolutions are tv_igemm_nt
// launches with the ReLU epilogue (TV_ACTX_RELU); transvae/metrics_fid.py drives them.
//
// The bf16 kernels are bandwidth kernels like those of csrc/lpips.hip: one 16-byte access per thread and tensor, 64-bit element
// indices, every index derived from the element count the host computed (grid-stride loops, no out-of-range lane touches memory).
//
// Algorithmic bytes per call (what tools/fid_bench.py divides by kernel time), activations bf16:
//   tv_fid_prep          12 * B*H*W read (fp32, through the cache: every source pixel is used ~ (299/H)^2 * 9/4 times) + 64 * B*149*149 written
//   tv_pool3x3           2 * B*H*W*C read + 2 * B*Ho*Wo*C written
//   tv_gather_line       2 * B*H*W*C read + 2 * taps * B*H*W*C written
//   tv_global_avgpool    2 * B*HW*C read
//   tv_fid_accumulate    8 * D*D read and written once per call; 2 * B * D*D fp64 multiply-adds
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FID_SIDE = 299;                 // the network's input grid
constexpr int FID_OUT = (FID_SIDE - 3) / 2 + 1;   // 149: grid of the first convolution (3x3, stride 2, no padding)

inline int bw_grid(long long n) {
    long long g = (n + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    if (g < 1) g = 1;
    return (int)g;
}

// ---------------------------------------------------------------------------------------------------------------------
// input preparation.  F.interpolate(x, (299, 299), mode="bilinear", align_corners=False): destination index d reads the source
// coordinate s = max(0, (d + 0.5) * S / 299 - 0.5) = max(0, ((2d + 1) S - 299) / 598), rows floor(s) and min(floor(s) + 1, S - 1)
// with weights 1 - l and l, l = s - floor(s).  The coordinate is kept as the integer numerator, so floor(s) is exact and l is the
// correctly rounded fp32 of an exact fraction.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bilinear_tap(int d, int S, int& i0, int& i1, float& l) {
    const int num = (2 * d + 1) * S - FID_SIDE;     // < 2 * 299 * S: far inside int for any image
    if (num <= 0) { i0 = 0; i1 = S > 1 ? 1 : 0; l = 0.f; return; }
    i0 = num / (2 * FID_SIDE);
    l = (float)(num - i0 * (2 * FID_SIDE)) / (float)(2 * FID_SIDE);
    i1 = i0 + 1 < S ? i0 + 1 : S - 1;
    if (i0 > S - 1) i0 = S - 1;                     // (cannot happen for d < 299; keeps the read in range whatever d is)
}

// images b < B0 come from `a`, the others from `bsrc`; 4 threads per output pixel, 8 of the 32 patch columns each
__global__ __launch_bounds__(256) void fid_prep_kernel(const float* __restrict__ a, const float* __restrict__ bsrc, bf16* __restrict__ dst,
                                                       long long total, int B0, int H, int W, int clip) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx & 3);
        const long long pix = idx >> 2;
        const int ox = (int)(pix % FID_OUT);
        const long long r = pix / FID_OUT;
        const int oy = (int)(r % FID_OUT);
        const long long b = r / FID_OUT;
        const float* src = b < B0 ? a + (size_t)b * 3 * H * W : bsrc + (size_t)(b - B0) * 3 * H * W;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = v * 8 + e;
            float f = 0.f;
            if (k < 27) {
                const int tap = k / 3, c = k - tap * 3;
                int y0, y1, x0, x1;
                float ly, lx;
                bilinear_tap(2 * oy + tap / 3, H, y0, y1, ly);      // rows / columns 2 o + k <= 298 of the 299 grid
                bilinear_tap(2 * ox + tap % 3, W, x0, x1, lx);
                const float* p = src + (size_t)c * H * W;
                float v00 = p[(size_t)y0 * W + x0], v01 = p[(size_t)y0 * W + x1], v10 = p[(size_t)y1 * W + x0], v11 = p[(size_t)y1 * W + x1];
                if (clip) {
                    // torch.clamp: a NaN passes through into every output pixel that reads it (fminf / fmaxf drop it)
                    v00 = v00 < 0.f ? 0.f : (v00 > 1.f ? 1.f : v00); v01 = v01 < 0.f ? 0.f : (v01 > 1.f ? 1.f : v01);
                    v10 = v10 < 0.f ? 0.f : (v10 > 1.f ? 1.f : v10); v11 = v11 < 0.f ? 0.f : (v11 > 1.f ? 1.f : v11);
                }
                const float top = fmaf(lx, v01 - v00, v00), bot = fmaf(lx, v11 - v10, v10);
                f = fmaf(2.f, fmaf(ly, bot - top, top), -1.f);
            }
            o[e] = (bf16)f;
        }
        *(bf16x8*)(dst + idx * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3x3 pools on bf16 NHWC.  MODE 0: max, stride 2, no padding (floor);  1: max, stride 1, pad 1;  2: average, stride 1, pad 1,
// divided by the number of in-bounds taps (count_include_pad=False).  The maximum follows torch's scan: start at -inf, taps in
// (dy, dx) order, a later tap replaces the running maximum only if it is greater or NaN.  The average is an fp32 sum in tap
// order, one IEEE division, one rounding to bf16.  The output row stride is ldo (a column range of a wider tensor).
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void pool3x3_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, long long total, int H, int W, int C,
                                                      int Ho, int Wo, int ldo) {
    constexpr int S = MODE == 0 ? 2 : 1, P = MODE == 0 ? 0 : 1;
    const int cv = C >> 3;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const long long pix = idx / cv;
        const int ox = (int)(pix % Wo);
        const long long r = pix / Wo;
        const int oy = (int)(r % Ho);
        const long long b = r / Ho;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = MODE == 2 ? 0.f : -INFINITY;
        int cnt = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = oy * S + dy - P, ix = ox * S + dx - P;
                if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
                const bf16x8 t = *(const bf16x8*)(x + (((size_t)b * H + iy) * W + ix) * C + v * 8);
                ++cnt;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float f = (float)t[e];
                    if (MODE == 2) acc[e] += f;
                    else if (f > acc[e] || f != f) acc[e] = f;
                }
            }
        }
        bf16x8 o;
        const float n = (float)cnt;      // >= 4 for pad 1 on H, W >= 2; 9 for the unpadded form
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)(MODE == 2 ? acc[e] / n : acc[e]);
        *(bf16x8*)(y + (size_t)pix * ldo + v * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// row gather along one axis: out[(b, y, x), t, c] = x[b, y + (axis == 0) (t - taps/2), x + (axis == 1) (t - taps/2), c], zero
// outside the image.  A 1 x taps (axis 1) or taps x 1 (axis 0) convolution with "same" padding is then a GEMM with K = taps * C.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_line_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, long long total, int H, int W, int C,
                                                          int taps, int axis) {
    const int cv = C >> 3, half = taps >> 1;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const long long q = idx / cv;
        const int t = (int)(q % taps);
        const long long pix = q / taps;
        const int px = (int)(pix % W);
        const long long r = pix / W;
        const int py = (int)(r % H);
        const long long b = r / H;
        const int iy = axis == 0 ? py + t - half : py, ix = axis == 0 ? px : px + t - half;
        bf16x8 o = zero8;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) o = *(const bf16x8*)(x + (((size_t)b * H + iy) * W + ix) * C + v * 8);
        *(bf16x8*)(y + idx * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// global average pool: out[b, c] = mean over the HW pixels, summed in pixel order in fp64 (a sum of bf16 values: exact up to
// 2^-53), one rounding to fp32.  One thread per image and 8 channels.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_avgpool_kernel(const bf16* __restrict__ x, float* __restrict__ out, long long total, int HW, int C) {
    const int cv = C >> 3;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const long long b = idx / cv;
        double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16* p = x + (size_t)b * HW * C + v * 8;
        for (int i = 0; i < HW; ++i) {
            const bf16x8 t = *(const bf16x8*)(p + (size_t)i * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += (double)(float)t[e];
        }
        float* o = out + (size_t)b * C + v * 8;
        f32x4 o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o0[e] = (float)(s[e] / (double)HW); o1[e] = (float)(s[4 + e] / (double)HW); }
        *(f32x4*)o = o0;
        *(f32x4*)(o + 4) = o1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// spatial rows (sFID): out[b, p * nc + c] = x[b, p, c0 + c] for p < HW, c < nc, bf16 -> fp32 (exact); zeros from HW * nc up to
// ldo.  One thread per output element: consecutive threads write consecutive floats and read nc-element runs ldc apart.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spatial_rows_kernel(const bf16* __restrict__ x, float* __restrict__ out, long long total, int HW, int ldc,
                                                           int c0, int nc, int ldo) {
    const int used = HW * nc;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int col = (int)(idx % ldo);
        const long long b = idx / ldo;
        float v = 0.f;
        if (col < used) {
            const int p = col / nc, c = col - p * nc;
            v = (float)x[((size_t)b * HW + p) * ldc + c0 + c];
        }
        out[idx] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Streaming moments in fp64.  state = {count, unused, mean[D], M2[D * D]} with M2 = sum_i (x_i - mean)(x_i - mean)^T of the
// samples seen so far.  A batch is merged SAMPLE BY SAMPLE, in row order, with the pairwise (Chan et al.) merge of the running
// statistics and a single sample -- Welford's update:
//     n = n + 1;  d = x - mean;  mean += d / n;  M2 += (n - 1) / n * d d^T
// so the state after N samples is one fixed sequence of operations on the sample stream: it depends neither on how the stream
// was cut into batches nor on the launch geometry, and nothing is ever formed as a difference of large sums.
//   fid_delta_kernel   one thread per column: the running mean over the batch's rows; d_i is kept in `scratch` [B, D]
//   fid_scatter_kernel one 64 x 64 tile of M2 per block, a 4 x 4 register tile per thread, the d_i staged through LDS 16 rows
//                      at a time; element (j, k):  M2 = fma(d_j * d_k, (n_i - 1) / n_i, M2)  for i in row order (d_j * d_k
//                      commutes, so M2 stays bit-symmetric)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fid_delta_kernel(const float* __restrict__ x, int B, int D, int ldx, long long n0, double* __restrict__ state,
                                                        double* __restrict__ scratch) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D) return;
    double m = state[2 + j];
    for (int i = 0; i < B; ++i) {
        const double d = (double)x[(size_t)i * ldx + j] - m;
        m += d / (double)(n0 + i + 1);
        scratch[(size_t)i * D + j] = d;
    }
    state[2 + j] = m;
    if (j == 0) state[0] = (double)(n0 + B);
}

constexpr int SC_ROWS = 16;

__global__ __launch_bounds__(256) void fid_scatter_kernel(const double* __restrict__ scratch, int B, int D, long long n0, double* __restrict__ m2) {
    __shared__ double da[SC_ROWS][64], db[SC_ROWS][64];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int j0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = m2[(size_t)(j0 + ty * 4 + r) * D + k0 + tx * 4 + c];
    for (int i0 = 0; i0 < B; i0 += SC_ROWS) {
        __syncthreads();
        for (int e = threadIdx.x; e < SC_ROWS * 64; e += 256) {
            const int r = e >> 6, c = e & 63;
            const bool ok = i0 + r < B;                          // rows past the batch stage zeros and are skipped below
            da[r][c] = ok ? scratch[(size_t)(i0 + r) * D + j0 + c] : 0.0;
            db[r][c] = ok ? scratch[(size_t)(i0 + r) * D + k0 + c] : 0.0;
        }
        __syncthreads();
        const int rows = B - i0 < SC_ROWS ? B - i0 : SC_ROWS;
        for (int r = 0; r < rows; ++r) {
            const long long n = n0 + i0 + r + 1;
            const double w = (double)(n - 1) / (double)n;
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { a[q] = da[r][ty * 4 + q]; b[q] = db[r][tx * 4 + q]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p] * b[q], w, acc[p][q]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) m2[(size_t)(j0 + ty * 4 + r) * D + k0 + tx * 4 + c] = acc[r][c];
}

}  // namespace

extern "C" int tv_fid_prep(const float* a, const float* b, void* cols, int Ba, int Bb, int H, int W, int clip, void* stream) {
    TV_CHECK_ARG(a && cols && Ba > 0 && Bb >= 0 && (Bb == 0 || b), "tv_fid_prep: bad arguments");
    TV_CHECK_ARG(H >= 8 && W >= 8 && H <= 16384 && W <= 16384, "tv_fid_prep: H, W must be in [8, 16384] (got %dx%d)", H, W);
    const long long total = (long long)(Ba + Bb) * FID_OUT * FID_OUT * 4;
    hipLaunchKernelGGL(fid_prep_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, a, b, (bf16*)cols, total, Ba, H, W, clip ? 1 : 0);
    TV_CHECK_LAUNCH("tv_fid_prep");
    return TV_OK;
}

extern "C" int tv_pool3x3(const void* x, void* y, int B, int H, int W, int C, int ldo, int mode, void* stream) {
    TV_CHECK_ARG(x && y && B > 0 && C > 0 && C % 8 == 0 && ldo >= C && ldo % 8 == 0, "tv_pool3x3: needs C %% 8 == 0 and ldo >= C, ldo %% 8 == 0 (C=%d, ldo=%d)", C, ldo);
    TV_CHECK_ARG(mode >= TV_POOL3_MAX_S2 && mode <= TV_POOL3_AVG_S1P1, "tv_pool3x3: unknown mode %d", mode);
    TV_CHECK_ARG(mode == TV_POOL3_MAX_S2 ? (H >= 3 && W >= 3) : (H >= 2 && W >= 2), "tv_pool3x3: grid %dx%d too small", H, W);
    const int Ho = mode == TV_POOL3_MAX_S2 ? (H - 3) / 2 + 1 : H, Wo = mode == TV_POOL3_MAX_S2 ? (W - 3) / 2 + 1 : W;
    const long long total = (long long)B * Ho * Wo * (C / 8);
    const dim3 g(bw_grid(total)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    if (mode == TV_POOL3_MAX_S2) hipLaunchKernelGGL(pool3x3_kernel<0>, g, blk, 0, s, (const bf16*)x, (bf16*)y, total, H, W, C, Ho, Wo, ldo);
    else if (mode == TV_POOL3_MAX_S1P1) hipLaunchKernelGGL(pool3x3_kernel<1>, g, blk, 0, s, (const bf16*)x, (bf16*)y, total, H, W, C, Ho, Wo, ldo);
    else hipLaunchKernelGGL(pool3x3_kernel<2>, g, blk, 0, s, (const bf16*)x, (bf16*)y, total, H, W, C, Ho, Wo, ldo);
    TV_CHECK_LAUNCH("tv_pool3x3");
    return TV_OK;
}

extern "C" int tv_gather_line(const void* x, void* y, int B, int H, int W, int C, int taps, int axis, void* stream) {
    TV_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "tv_gather_line: needs C %% 8 == 0 (got %d)", C);
    TV_CHECK_ARG((taps == 3 || taps == 7) && (axis == 0 || axis == 1), "tv_gather_line: taps must be 3 or 7 and axis 0 (H) or 1 (W)");
    const long long total = (long long)B * H * W * taps * (C / 8);
    hipLaunchKernelGGL(gather_line_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (bf16*)y, total, H, W, C, taps, axis);
    TV_CHECK_LAUNCH("tv_gather_line");
    return TV_OK;
}

extern "C" int tv_global_avgpool(const void* x, float* out, int B, int HW, int C, void* stream) {
    TV_CHECK_ARG(x && out && B > 0 && HW > 0 && C > 0 && C % 8 == 0, "tv_global_avgpool: needs C %% 8 == 0 (got %d)", C);
    const long long total = (long long)B * (C / 8);
    hipLaunchKernelGGL(global_avgpool_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, out, total, HW, C);
    TV_CHECK_LAUNCH("tv_global_avgpool");
    return TV_OK;
}

extern "C" int tv_spatial_rows(const void* x, int B, int HW, int C, int ldc, int c0, int nc, float* out, int ldo, void* stream) {
    TV_CHECK_ARG(x && out && B > 0 && HW > 0 && C > 0, "tv_spatial_rows: bad arguments");
    TV_CHECK_ARG(ldc >= C, "tv_spatial_rows: ldc=%d must be at least C=%d", ldc, C);
    TV_CHECK_ARG(c0 >= 0 && nc >= 1 && nc <= C - c0, "tv_spatial_rows: channels c0=%d .. c0 + nc=%d - 1 must lie in [0, C=%d)", c0, nc, C);
    TV_CHECK_ARG((long long)HW * nc <= (long long)ldo, "tv_spatial_rows: ldo=%d must be at least HW * nc = %lld", ldo, (long long)HW * nc);
    const long long total = (long long)B * ldo;
    hipLaunchKernelGGL(spatial_rows_kernel, dim3(bw_grid(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, out, total, HW, ldc, c0, nc, ldo);
    TV_CHECK_LAUNCH("tv_spatial_rows");
    return TV_OK;
}

extern "C" long long tv_fid_state_doubles(int D) {
    if (D <= 0 || D % 64 != 0 || D > 8192) return -1;
    return 2 + (long long)D + (long long)D * D;
}

extern "C" int tv_fid_accumulate(const float* x, int B, int D, int ldx, long long n0, double* state, double* scratch, void* stream) {
    TV_CHECK_ARG(x && state && scratch && B > 0 && n0 >= 0, "tv_fid_accumulate: bad arguments");
    TV_CHECK_ARG(D > 0 && D % 64 == 0 && D <= 8192 && ldx >= D, "tv_fid_accumulate: D=%d must be a multiple of 64 up to 8192 and ldx=%d >= D", D, ldx);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fid_delta_kernel, dim3((unsigned)tv_cdiv(D, 256)), dim3(256), 0, s, x, B, D, ldx, n0, state, scratch);
    TV_CHECK_LAUNCH("tv_fid_accumulate (means)");
    hipLaunchKernelGGL(fid_scatter_kernel, dim3((unsigned)(D / 64), (unsigned)(D / 64)), dim3(256), 0, s, (const double*)scratch, B, D, n0,
                       state + 2 + D);
    TV_CHECK_LAUNCH("tv_fid_accumulate (scatter)");
    return TV_OK;
}
