// The adversarial stage: everything of the PatchGAN discriminator that is not a convolution, and the GAN loss terms.
//   tv_patch4x4s2 / _bwd            fp32 image -> bf16 patch rows of the first layer (a K = 64 GEMM) and the adjoint
//   tv_bn_stats, tv_bn_lrelu_*      BatchNorm2d (training statistics) + LeakyReLU(0.2) over rows [M, C], forward and backward
//   tv_gan_loss                     generator BCE / bce / hinge / wgan on fp32 logits, value and gradients in one pass
// The convolutions are tv_igemm_nt / tv_wgrad_tn launches (kh = kw = 4), the first one with the LeakyReLU epilogue (TV_ACTX_LRELU).
//
// The row kernels are bandwidth kernels: 16-byte accesses on the bf16 tensors, each algorithmic byte moved once, 64-bit element
// indices.  Every reduction writes one partial per block and a finalise launch adds the partials in a fixed order in fp64: no
// atomics, the same bits on every run.  (tv_gan_loss carries its sums in fp64 throughout: the wgan form is a difference of means.)
//
// Algorithmic bytes per call (what tools/gan_bench.py divides by kernel time), activations bf16, P = B*H*W pixels of the image:
//   tv_patch4x4s2            12 P read (fp32, 3 channels) + 128 * P/4 written                  = 44 P
//   tv_patch4x4s2_bwd        128 * P/4 read (+ 12 P with the sigmoid) + 12 P written           = 44 [56] P
//   tv_bn_stats              2 M C read
//   tv_bn_lrelu_apply        2 M C read + 2 M C written                                         = 4 M C
//   tv_bn_lrelu_bwd_reduce   4 M C read (x, dy)
//   tv_bn_lrelu_bwd_apply    4 M C read + 2 M C written                                         = 6 M C
//   tv_gan_loss              4 n read + 4 n written per logit tensor
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_BLOCKS = 1024;
constexpr int BN_MIN_ROWS = 64;      // rows per block at least (small tensors: fewer blocks, not thinner ones)

__host__ __device__ inline int bn_blocks(long long M) {
    long long n = (M + BN_MIN_ROWS - 1) / BN_MIN_ROWS;
    return (int)(n < 1 ? 1 : (n > BN_MAX_BLOCKS ? BN_MAX_BLOCKS : n));
}

__device__ __forceinline__ float lrelu(float h) { return h > 0.f ? h : h * TV_LRELU_SLOPE; }
__device__ __forceinline__ float sigmoid_exact(float v) { return 1.0f / (1.0f + expf(-v)); }

// ---------------------------------------------------------------------------------------------------------------------
// first-layer operand: 4x4 / stride-2 / pad-1 patches of an fp32 image as bf16 rows of 64 columns
// ---------------------------------------------------------------------------------------------------------------------
// one thread per 8-column piece of a row (a 16-byte store); pieces 6 and 7 are the zero padding
__global__ __launch_bounds__(256) void patch4x4s2_kernel(const float* __restrict__ img, long long sn, long long sc, long long sh, long long sw,
                                                         bf16* __restrict__ rows, long long total, int H, int W, int sig) {
    const int Ho = H >> 1, Wo = W >> 1;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int piece = (int)(idx & 7);
        const long long row = idx >> 3;
        bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
        if (piece < 6) {
            const int ox = (int)(row % Wo);
            const long long r = row / Wo;
            const int oy = (int)(r % Ho);
            const long long b = r / Ho;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = piece * 8 + e;          // (ky*4 + kx)*3 + c
                const int c = k % 3, t = k / 3;
                const int y = 2 * oy + (t >> 2) - 1, x = 2 * ox + (t & 3) - 1;
                float v = 0.f;                         // (the padding is zero AFTER the sigmoid: the convolution pads its input)
                if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
                    v = img[b * sn + c * sc + y * sh + x * sw];
                    if (sig) v = sigmoid_exact(v);
                }
                o[e] = (bf16)v;
            }
        }
        *(bf16x8*)(rows + idx * 8) = o;
    }
}

// adjoint, gather form: pixel (y, x) is tap (ky, kx) of patch (oy, ox) iff y = 2 oy + ky - 1: ky has the parity of y + 1, so
// two candidate rows and two candidate columns -- at most four patches, summed in a fixed order in fp32
__global__ __launch_bounds__(256) void patch4x4s2_bwd_kernel(const bf16* __restrict__ drows, const float* __restrict__ img, long long sn, long long sc,
                                                             long long sh, long long sw, float* __restrict__ dimg, long long total, int H, int W,
                                                             int sig) {
    const int Ho = H >> 1, Wo = W >> 1;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x = (int)(idx % W);
        const long long r = idx / W;
        const int y = (int)(r % H);
        const long long b = r / H;
        float acc[3] = {0.f, 0.f, 0.f};
        const int ky0 = (y + 1) & 1, kx0 = (x + 1) & 1;
#pragma unroll
        for (int jy = 0; jy < 2; ++jy) {
            const int ky = ky0 + 2 * jy, oy = (y + 1 - ky) >> 1;      // (y + 1 - ky is even; may be -2 .. : checked below)
            if (y + 1 - ky < 0 || oy >= Ho) continue;
#pragma unroll
            for (int jx = 0; jx < 2; ++jx) {
                const int kx = kx0 + 2 * jx, ox = (x + 1 - kx) >> 1;
                if (x + 1 - kx < 0 || ox >= Wo) continue;
                const bf16* s = drows + (((size_t)b * Ho + oy) * Wo + ox) * 64 + (ky * 4 + kx) * 3;
                acc[0] += (float)s[0];
                acc[1] += (float)s[1];
                acc[2] += (float)s[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float g = acc[c];
            if (sig) {
                // sigmoid'(v) = e / (1 + e)^2 with e = exp(-|v|): no 1 - s cancellation where the sigmoid saturates
                const float e = expf(-fabsf(img[b * sn + c * sc + y * sh + x * sw]));
                g *= e / ((1.0f + e) * (1.0f + e));
            }
            dimg[(((size_t)b * 3 + c) * H + y) * W + x] = g;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm (training) + LeakyReLU over rows [M, C]
// ---------------------------------------------------------------------------------------------------------------------
// Block layout of the two reductions: cv = C/8 column vectors, R = 256 / cv row lanes; thread (r, v) walks rows r, r + R, ... of
// the block's contiguous row range and keeps 8 channels x 2 sums in registers; the R row lanes are then added in lane order
// through LDS.  KIND 0: sums of (x - piv), (x - piv)^2;  KIND 1: sums of dh, dh * xhat.
template <int KIND>
__global__ __launch_bounds__(BN_THREADS) void bn_reduce_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, const float* __restrict__ mr,
                                                               const float* __restrict__ ss, float* __restrict__ partials, long long M, int C) {
    __shared__ float red[4096];          // [R][C][2], R * C <= 2048
    const int cv = C >> 3, R = BN_THREADS / cv;
    const int v = threadIdx.x % cv, r = threadIdx.x / cv;
    const int nblk = gridDim.x;
    const long long per = (M + nblk - 1) / nblk;
    const long long m0 = (long long)blockIdx.x * per;
    const long long m1 = m0 + per < M ? m0 + per : M;
    float s1[8], s2[8], p0[8], p1[8], q0[8], q1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
    if (r < R) {
        if constexpr (KIND == 0) {
            const bf16x8 pv = *(const bf16x8*)(x + v * 8);       // the pivot: row 0 of the tensor, the same for every block
#pragma unroll
            for (int e = 0; e < 8; ++e) p0[e] = (float)pv[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                p0[e] = mr[v * 8 + e];
                p1[e] = mr[C + v * 8 + e];
                q0[e] = ss[v * 8 + e];
                q1[e] = ss[C + v * 8 + e];
            }
        }
        for (long long m = m0 + r; m < m1; m += R) {
            const bf16x8 xv = *(const bf16x8*)(x + (size_t)m * C + v * 8);
            if constexpr (KIND == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = (float)xv[e] - p0[e];
                    s1[e] += d;
                    s2[e] = fmaf(d, d, s2[e]);
                }
            } else {
                const bf16x8 gv = *(const bf16x8*)(dy + (size_t)m * C + v * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xf = (float)xv[e];
                    const float h = fmaf(xf, q0[e], q1[e]);
                    const float dh = h > 0.f ? (float)gv[e] : (float)gv[e] * TV_LRELU_SLOPE;
                    s1[e] += dh;
                    s2[e] = fmaf(dh, (xf - p0[e]) * p1[e], s2[e]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[((size_t)r * C + v * 8 + e) * 2] = s1[e];
            red[((size_t)r * C + v * 8 + e) * 2 + 1] = s2[e];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += BN_THREADS) {
        float a = 0.f, b = 0.f;
        for (int rr = 0; rr < R; ++rr) {
            a += red[((size_t)rr * C + c) * 2];
            b += red[((size_t)rr * C + c) * 2 + 1];
        }
        partials[((size_t)blockIdx.x * 2) * C + c] = a;
        partials[((size_t)blockIdx.x * 2 + 1) * C + c] = b;
    }
}

// One wave per channel: lane l adds partials l, l + 64, ... in that order (fp64), then a butterfly whose pairing is fixed -- the
// same bits on every run, and 16 dependent adds per lane instead of 1024 in one thread.
__device__ __forceinline__ void bn_partial_sums(const float* __restrict__ partials, int nblk, int C, int c, double& a, double& b) {
    a = 0.0;
    b = 0.0;
    for (int k = threadIdx.x & 63; k < nblk; k += 64) {
        a += (double)partials[((size_t)k * 2) * C + c];
        b += (double)partials[((size_t)k * 2 + 1) * C + c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
}

__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const bf16* __restrict__ x, const float* __restrict__ partials, int nblk,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ mr, float* __restrict__ ss, float* __restrict__ rmean,
                                                                float* __restrict__ rvar, long long M, int C, float eps, float momentum) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                     // (wave-uniform)
    double a, b;
    bn_partial_sums(partials, nblk, C, c, a, b);
    if ((threadIdx.x & 63) != 0) return;
    const double piv = (double)(float)x[c];
    const double dm = a / (double)M;                       // mean - pivot
    double var = b / (double)M - dm * dm;                  // about the pivot (a sample of the channel itself): |dm| is of the
    if (var < 0.0) var = 0.0;                              // order of the spread, so this difference does not cancel
    const float mean = (float)(piv + dm);
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    mr[c] = mean;
    mr[C + c] = rstd;
    if (ss) {
        const float sc = gamma[c] * rstd;
        ss[c] = sc;
        ss[C + c] = beta[c] - mean * sc;
    }
    if (rmean) {
        const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
        rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * (piv + dm));
        rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unb);
    }
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partials, int nblk, float* __restrict__ red,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int C, int accumulate) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                     // (wave-uniform)
    double a, b;
    bn_partial_sums(partials, nblk, C, c, a, b);
    if ((threadIdx.x & 63) != 0) return;
    red[c] = (float)a;
    red[C + c] = (float)b;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)a : (float)a;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)b : (float)b;
}

__global__ __launch_bounds__(256) void bn_lrelu_apply_kernel(const bf16* __restrict__ x, const float* __restrict__ ss, bf16* __restrict__ y,
                                                             long long total, int C) {
    const int cv = C >> 3;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const bf16x8 xv = *(const bf16x8*)(x + idx * 8);
        const f32x4 a0 = *(const f32x4*)(ss + v * 8), a1 = *(const f32x4*)(ss + v * 8 + 4);
        const f32x4 b0 = *(const f32x4*)(ss + C + v * 8), b1 = *(const f32x4*)(ss + C + v * 8 + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (bf16)lrelu(fmaf((float)xv[e], a0[e], b0[e]));
            o[e + 4] = (bf16)lrelu(fmaf((float)xv[e + 4], a1[e], b1[e]));
        }
        *(bf16x8*)(y + idx * 8) = o;
    }
}

__global__ __launch_bounds__(256) void bn_lrelu_bwd_apply_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, const float* __restrict__ mr,
                                                                 const float* __restrict__ ss, const float* __restrict__ red, bf16* __restrict__ dx,
                                                                 long long total, int C, float inv_m, int eval_mode) {
    const int cv = C >> 3;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int v = (int)(idx % cv);
        const bf16x8 xv = *(const bf16x8*)(x + idx * 8);
        const bf16x8 gv = *(const bf16x8*)(dy + idx * 8);
        float sc[8], sh[8], mu[8], rs[8], r0[8], r1[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = v * 8 + q * 4;
            const f32x4 a = *(const f32x4*)(ss + c), b = *(const f32x4*)(ss + C + c);
            f32x4 m = {0.f, 0.f, 0.f, 0.f}, r = m, p0 = m, p1 = m;
            if (!eval_mode) {
                m = *(const f32x4*)(mr + c);
                r = *(const f32x4*)(mr + C + c);
                p0 = *(const f32x4*)(red + c);
                p1 = *(const f32x4*)(red + C + c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sc[q * 4 + e] = a[e]; sh[q * 4 + e] = b[e]; mu[q * 4 + e] = m[e]; rs[q * 4 + e] = r[e];
                r0[q * 4 + e] = p0[e]; r1[q * 4 + e] = p1[e];
            }
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xf = (float)xv[e];
            const float h = fmaf(xf, sc[e], sh[e]);
            const float dh = h > 0.f ? (float)gv[e] : (float)gv[e] * TV_LRELU_SLOPE;
            float g = dh;
            if (!eval_mode) {
                const float xh = (xf - mu[e]) * rs[e];
                g = dh - (r0[e] + xh * r1[e]) * inv_m;
            }
            o[e] = (bf16)(sc[e] * g);
        }
        *(bf16x8*)(dx + idx * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// GAN loss terms
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GL_THREADS = 256;
constexpr int GL_PER_BLOCK = 4096;       // logits per block
constexpr int GL_MAX_BLOCKS = 1024;

__host__ __device__ inline int gl_blocks(long long n) {
    long long k = (n + GL_PER_BLOCK - 1) / GL_PER_BLOCK;
    return (int)(k < 1 ? 1 : (k > GL_MAX_BLOCKS ? GL_MAX_BLOCKS : k));
}

// per-element term and its derivative.  which = 0: tensor a (generator's fake logits / real logits), 1: tensor b (fake logits)
__device__ __forceinline__ float gan_term(int mode, int which, float x, float& dv) {
    if (mode == TV_GAN_GEN || mode == TV_GAN_BCE) {
        const float t = which == 0 ? 1.0f : 0.0f;
        const float e = expf(-fabsf(x));                      // in (0, 1]: no overflow at any logit
        const float sg = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);   // sigmoid(x), saturating to exactly 0 / 1
        dv = sg - t;
        return fmaxf(x, 0.f) - x * t + log1pf(e);
    }
    if (mode == TV_GAN_HINGE) {
        const float m = which == 0 ? 1.0f - x : 1.0f + x;
        dv = m > 0.f ? (which == 0 ? -1.0f : 1.0f) : 0.f;
        return fmaxf(m, 0.f);
    }
    dv = which == 0 ? -1.0f : 1.0f;                           // wgan
    return which == 0 ? -x : x;
}

// blocks 0 .. na_blk-1 walk a, the others b; one partial per block.  The terms are fp32, their SUM is carried in fp64 from the
// first add on: -mean(a) + mean(b) of the wgan form cancels, and an fp32 running sum of a few thousand logits would leave 1e-6 of
// the means, not of their difference
__global__ __launch_bounds__(GL_THREADS) void gan_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ da,
                                                              float* __restrict__ db, double* __restrict__ partials, long long n_a, long long n_b,
                                                              int na_blk, int mode, float ga, float gb) {
    __shared__ double wsum[GL_THREADS / 64];
    const int which = (int)blockIdx.x >= na_blk;
    const int blk = which ? blockIdx.x - na_blk : blockIdx.x;
    const int nblk = which ? gridDim.x - na_blk : na_blk;
    const float* __restrict__ src = which ? b : a;
    float* __restrict__ dst = which ? db : da;
    const long long n = which ? n_b : n_a;
    const float gs = which ? gb : ga;
    const long long per = ((n + nblk - 1) / nblk + 3) & ~3ll;     // a block's range starts on a 16-byte boundary
    const long long i0 = (long long)blk * per;
    const long long i1 = i0 + per < n ? i0 + per : n;
    double acc = 0.0;
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    for (long long i = i0 + threadIdx.x * 4ll; i < i1; i += GL_THREADS * 4ll) {
        if (vec && i + 4 <= i1) {
            const f32x4 xv = *(const f32x4*)(src + i);
            f32x4 dvv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float dv;
                acc += (double)gan_term(mode, which, xv[e], dv);
                dvv[e] = dv * gs;
            }
            if (dst) *(f32x4*)(dst + i) = dvv;
        } else {
            for (long long j = i; j < i1 && j < i + 4; ++j) {
                float dv;
                acc += (double)gan_term(mode, which, src[j], dv);
                if (dst) dst[j] = dv * gs;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < GL_THREADS / 64; ++w) s += wsum[w];
        partials[blockIdx.x] = s;
    }
}

__global__ void gan_loss_finalize_kernel(const double* __restrict__ partials, float* __restrict__ out, int na_blk, int nb_blk, double inv_a,
                                         double inv_b, double scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < na_blk; ++k) sa += partials[k];
    for (int k = 0; k < nb_blk; ++k) sb += partials[na_blk + k];
    out[0] = (float)((sa * inv_a + sb * inv_b) * scale);
}

inline int ew_blocks(long long n_threads) {
    long long g = (n_threads + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

extern "C" int tv_patch4x4s2(const float* img, long long sn, long long sc, long long sh, long long sw, void* rows, int B, int H, int W,
                             int sigmoid, void* stream) {
    TV_CHECK_ARG(img && rows && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "tv_patch4x4s2: B=%d H=%d W=%d (H, W even)", B, H, W);
    TV_CHECK_ARG(((uintptr_t)rows & 15) == 0, "tv_patch4x4s2: rows must be 16-byte aligned");
    const long long total = (long long)B * (H / 2) * (W / 2) * 8;
    hipLaunchKernelGGL(patch4x4s2_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, img, sn, sc, sh, sw, (bf16*)rows, total, H, W,
                       sigmoid);
    TV_CHECK_LAUNCH("tv_patch4x4s2");
    return TV_OK;
}

extern "C" int tv_patch4x4s2_bwd(const void* drows, const float* img, long long sn, long long sc, long long sh, long long sw, float* dimg, int B,
                                 int H, int W, int sigmoid, void* stream) {
    TV_CHECK_ARG(drows && dimg && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "tv_patch4x4s2_bwd: B=%d H=%d W=%d (H, W even)", B, H, W);
    TV_CHECK_ARG(!sigmoid || img, "tv_patch4x4s2_bwd: the sigmoid form needs the image");
    const long long total = (long long)B * H * W;
    hipLaunchKernelGGL(patch4x4s2_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)drows, img, sn, sc, sh, sw,
                       dimg, total, H, W, sigmoid);
    TV_CHECK_LAUNCH("tv_patch4x4s2_bwd");
    return TV_OK;
}

static bool bn_shape_ok(long long M, int C) { return M > 0 && C >= 8 && C % 8 == 0 && C <= 2048 && M < (1ll << 40); }

extern "C" long long tv_bn_partial_count(long long M, int C) {
    if (!bn_shape_ok(M, C)) return -1;
    return (long long)bn_blocks(M) * 2 * C;
}

extern "C" int tv_bn_stats(const void* x, const float* gamma, const float* beta, float* partials, float* mr, float* ss, float* running_mean,
                           float* running_var, long long M, int C, float eps, float momentum, void* stream) {
    TV_CHECK_ARG(bn_shape_ok(M, C), "tv_bn_stats: M=%lld C=%d (C a multiple of 8, at most 2048)", M, C);
    TV_CHECK_ARG(x && partials && mr && (!ss || (gamma && beta)) && (!running_mean == !running_var),
                 "tv_bn_stats: x, partials, mr are required; ss needs gamma and beta; running_mean and running_var come together");
    TV_CHECK_ARG(((uintptr_t)x & 15) == 0, "tv_bn_stats: x must be 16-byte aligned");
    const int nblk = bn_blocks(M);
    hipLaunchKernelGGL(bn_reduce_kernel<0>, dim3(nblk), dim3(BN_THREADS), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, partials, M, C);
    TV_CHECK_LAUNCH("tv_bn_stats");
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(tv_cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, partials, nblk, gamma, beta,
                       mr, ss, running_mean, running_var, M, C, eps, momentum);
    TV_CHECK_LAUNCH("tv_bn_stats (finalise)");
    return TV_OK;
}

extern "C" int tv_bn_lrelu_apply(const void* x, const float* ss, void* y, long long M, int C, void* stream) {
    TV_CHECK_ARG(bn_shape_ok(M, C) && x && ss && y, "tv_bn_lrelu_apply: M=%lld C=%d (C a multiple of 8, at most 2048)", M, C);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)ss) & 15) == 0, "tv_bn_lrelu_apply: x, y, ss must be 16-byte aligned");
    const long long total = M * (C / 8);
    hipLaunchKernelGGL(bn_lrelu_apply_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ss, (bf16*)y, total, C);
    TV_CHECK_LAUNCH("tv_bn_lrelu_apply");
    return TV_OK;
}

extern "C" int tv_bn_lrelu_bwd_reduce(const void* x, const void* dy, const float* mr, const float* ss, float* partials, float* red, float* dgamma,
                                      float* dbeta, long long M, int C, int accumulate, void* stream) {
    TV_CHECK_ARG(bn_shape_ok(M, C) && x && dy && mr && ss && partials && red, "tv_bn_lrelu_bwd_reduce: M=%lld C=%d (C a multiple of 8, at most 2048)",
                 M, C);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy) & 15) == 0, "tv_bn_lrelu_bwd_reduce: x, dy must be 16-byte aligned");
    const int nblk = bn_blocks(M);
    hipLaunchKernelGGL(bn_reduce_kernel<1>, dim3(nblk), dim3(BN_THREADS), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)dy, mr, ss, partials, M,
                       C);
    TV_CHECK_LAUNCH("tv_bn_lrelu_bwd_reduce");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(tv_cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, partials, nblk, red, dgamma, dbeta, C,
                       accumulate);
    TV_CHECK_LAUNCH("tv_bn_lrelu_bwd_reduce (finalise)");
    return TV_OK;
}

extern "C" int tv_bn_lrelu_bwd_apply(const void* x, const void* dy, const float* mr, const float* ss, const float* red, void* dx, long long M, int C,
                                     int eval_mode, void* stream) {
    TV_CHECK_ARG(bn_shape_ok(M, C) && x && dy && mr && ss && dx && (eval_mode || red),
                 "tv_bn_lrelu_bwd_apply: M=%lld C=%d (C a multiple of 8, at most 2048)", M, C);
    TV_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)mr | (uintptr_t)ss | (uintptr_t)red) & 15) == 0,
                 "tv_bn_lrelu_bwd_apply: x, dy, dx, mr, ss, red must be 16-byte aligned");
    const long long total = M * (C / 8);
    hipLaunchKernelGGL(bn_lrelu_bwd_apply_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)dy, mr, ss,
                       red, (bf16*)dx, total, C, (float)(1.0 / (double)M), eval_mode);
    TV_CHECK_LAUNCH("tv_bn_lrelu_bwd_apply");
    return TV_OK;
}

extern "C" long long tv_gan_loss_partial_count(long long n_a, long long n_b) {
    if (n_a <= 0 || n_b < 0) return -1;
    return 2ll * (gl_blocks(n_a) + (n_b > 0 ? gl_blocks(n_b) : 0));     // one fp64 partial per block
}

extern "C" int tv_gan_loss(const float* a, const float* b, float* da, float* db, float* partials, float* out, long long n_a, long long n_b, int mode,
                           float weight, void* stream) {
    TV_CHECK_ARG(mode >= TV_GAN_GEN && mode <= TV_GAN_WGAN, "tv_gan_loss: unknown mode %d", mode);
    TV_CHECK_ARG(a && partials && out && n_a > 0, "tv_gan_loss: a, partials, out are required");
    TV_CHECK_ARG(((uintptr_t)partials & 7) == 0, "tv_gan_loss: partials must be 8-byte aligned");
    TV_CHECK_ARG(mode == TV_GAN_GEN ? (!b && n_b == 0 && !db) : (b && n_b > 0),
                 "tv_gan_loss: the generator term takes one tensor, the discriminator forms two");
    const int na = gl_blocks(n_a), nb = n_b > 0 ? gl_blocks(n_b) : 0;
    const double half = (mode == TV_GAN_BCE || mode == TV_GAN_HINGE) ? 0.5 : 1.0;
    const double scale = (double)weight * half;
    const double inv_a = 1.0 / (double)n_a, inv_b = n_b > 0 ? 1.0 / (double)n_b : 0.0;
    hipLaunchKernelGGL(gan_loss_kernel, dim3(na + nb), dim3(GL_THREADS), 0, (hipStream_t)stream, a, b, da, db, (double*)partials, n_a, n_b, na, mode,
                       (float)(scale * inv_a), (float)(scale * inv_b));
    TV_CHECK_LAUNCH("tv_gan_loss");
    hipLaunchKernelGGL(gan_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, out, na, nb, inv_a, inv_b, scale);
    TV_CHECK_LAUNCH("tv_gan_loss (finalise)");
    return TV_OK;
}
