// The edge between decoded images and tensors, both ways.
//
// tv_image_prep: Resize(res) -> CenterCrop(res) -> ToTensor() of the reference's scripts (R/train.py:141-144, R/evaluate.py:39-42,
// P/generate_images.py:152-155 ...) for a ragged batch of uint8 HWC images in ONE launch.  The resize is PIL's 8-bit bilinear
// resample, which is integer arithmetic: per axis a table of (first tap, tap count, int32 coefficients with 22 fraction bits)
// built on the host in float64, the horizontal pass first, rounded and clipped to uint8, then the vertical pass on those
// uint8 values; each pass is clip((2^21 + sum pixel * k) >> 22, 0, 255).  A pass whose output size equals its input size is
// skipped (a copy), as PIL skips it.  The contract is equality of bits with PIL, not a tolerance.
//
//   one workgroup = one IMG_TH x IMG_TW tile of the cropped output of one image (blockIdx.y = image):
//     1. horizontal pass for the input rows the tile's vertical taps reach, straight from global memory (byte loads: 3-byte
//        pixels, arbitrary offsets and row strides, nothing to align) into LDS as uint8 planes [row][channel][IMG_TW]
//     2. vertical pass out of LDS (lanes of a wave read consecutive bytes of one plane row: conflict-free broadcast reads)
//     3. ToTensor through a 256-entry table (float(v) / 255.0f, or that times 2 minus 1) and row-contiguous fp32 stores per
//        channel plane
//   Rows and columns outside the crop are never computed: the tables hold the surviving output indices only.
//   LDS: rows x 3 x IMG_TW bytes, sized per launch from the tables (a ratio-16 down-scale needs (IMG_TH + 2) * 16 + 2 = 290 rows
//   = 55.7 KB, under the 64 KB a workgroup gets without an opt-in).
//
// tv_image_grid_u8: torchvision's make_grid + save_image quantisation, fp32 [B, 3, H, W] (any strides) -> one uint8 HWC canvas.
#include <algorithm>

#include "common.h"

namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_TW = 64;
constexpr int IMG_TH = 16;
constexpr int IMG_PB = 22;                 // PIL's PRECISION_BITS
constexpr int IMG_MAX_RATIO = 16;
constexpr int IMG_LDS_BYTES = 64 * 1024;

__device__ __forceinline__ int img_clip8(int acc) { return min(max(acc >> IMG_PB, 0), 255); }

__global__ __launch_bounds__(IMG_THREADS) void image_prep_kernel(const uint8_t* __restrict__ src, const tv_image_desc* __restrict__ desc,
                                                                 const int* __restrict__ coef, const float* __restrict__ lut,
                                                                 float* __restrict__ out, int res_h, int res_w, int tiles_x,
                                                                 int lds_rows) {
    extern __shared__ uint8_t s_rows[];    // [rows][3][IMG_TW]
    const int tid = threadIdx.x, b = blockIdx.y;
    const tv_image_desc d = desc[b];
    const int ty0 = ((int)blockIdx.x / tiles_x) * IMG_TH, tx0 = ((int)blockIdx.x % tiles_x) * IMG_TW;
    const int th = min(IMG_TH, res_h - ty0), tw = min(IMG_TW, res_w - tx0);
    const bool hpass = d.xtab >= 0, vpass = d.ytab >= 0;
    const int* xmin = coef + (hpass ? d.xtab : 0);
    const int* xcnt = xmin + res_w;
    const int* xk = xcnt + res_w;
    const int* ymin = coef + (vpass ? d.ytab : 0);
    const int* ycnt = ymin + res_h;
    const int* yk = ycnt + res_h;

    int row0 = d.crop_top + ty0, nrows = th;
    if (vpass) {
        row0 = ymin[ty0];
        nrows = ymin[ty0 + th - 1] + ycnt[ty0 + th - 1] - row0;
    }
    nrows = min(nrows, lds_rows);          // the host checked every tile against lds_rows already
    const uint8_t* img = src + d.offset;

    for (int i = tid; i < nrows * 3 * IMG_TW; i += IMG_THREADS) {
        const int x = i % IMG_TW, c = (i / IMG_TW) % 3, r = i / (3 * IMG_TW);
        if (x >= tw) continue;
        const uint8_t* rowp = img + (long long)(row0 + r) * d.row_stride + c;
        int v;
        if (hpass) {
            const int ox = tx0 + x, n = xcnt[ox];
            const uint8_t* p = rowp + xmin[ox] * 3;
            const int* k = xk + (long long)ox * d.xk;
            int acc = 1 << (IMG_PB - 1);
            for (int t = 0; t < n; ++t) acc += (int)p[t * 3] * k[t];
            v = img_clip8(acc);
        } else {
            v = rowp[(d.crop_left + tx0 + x) * 3];
        }
        s_rows[i] = (uint8_t)v;
    }
    __syncthreads();

    for (int i = tid; i < th * 3 * IMG_TW; i += IMG_THREADS) {
        const int x = i % IMG_TW, c = (i / IMG_TW) % 3, y = i / (3 * IMG_TW);
        if (x >= tw) continue;
        int v;
        if (vpass) {
            const int oy = ty0 + y, n = ycnt[oy];
            const uint8_t* p = s_rows + ((ymin[oy] - row0) * 3 + c) * IMG_TW + x;
            const int* k = yk + (long long)oy * d.yk;
            int acc = 1 << (IMG_PB - 1);
            for (int t = 0; t < n; ++t) acc += (int)p[t * 3 * IMG_TW] * k[t];
            v = img_clip8(acc);
        } else {
            v = s_rows[i];
        }
        out[(((long long)b * 3 + c) * res_h + ty0 + y) * res_w + tx0 + x] = lut[v];
    }
}

__device__ __forceinline__ uint8_t img_quant(float v) {
    // save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two roundings, no FMA; fmaxf drops a NaN, so NaN -> 0
    float t = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
    t = fminf(fmaxf(t, 0.f), 255.f);
    return (uint8_t)(int)t;
}

__global__ __launch_bounds__(IMG_THREADS) void image_grid_kernel(const float* __restrict__ img, long long sn, long long sc, long long sh,
                                                                 long long sw, uint8_t* __restrict__ out, int B, int H, int W, int xmaps,
                                                                 int pad, int Hg, int Wg, float pad_value, int transform) {
    const long long idx = (long long)blockIdx.x * IMG_THREADS + threadIdx.x;
    if (idx >= (long long)Hg * Wg) return;
    const int gy = (int)(idx / Wg), gx = (int)(idx % Wg);
    const int cell_h = H + pad, cell_w = W + pad;
    const int qy = gy / cell_h, ry = gy % cell_h, qx = gx / cell_w, rx = gx % cell_w;
    const long long k = (long long)qy * xmaps + qx;
    uint8_t* o = out + idx * 3;
    if (ry < pad || rx < pad || qx >= xmaps || k >= B) {
        const uint8_t p = img_quant(pad_value);
        o[0] = p;
        o[1] = p;
        o[2] = p;
        return;
    }
    const float* px = img + k * sn + (long long)(ry - pad) * sh + (long long)(rx - pad) * sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = px[c * sc];
        if (transform == TV_IMAGE_SIGMOID) v = 1.f / (1.f + expf(-v));
        o[c] = img_quant(v);
    }
}

// Host-side check of one axis table of one image against the coefficient buffer and the input size (tv_image_prep checks
// everything its kernel will index before the launch); 0 when it holds, -1 with the error text set otherwise.
int img_check_axis(const int* coef, long long coef_len, int tab, int ksize, int n_out, int in_size, const char* axis, int image) {
    if (tab < 0 || ksize < 1 || (long long)tab + 2ll * n_out + (long long)n_out * ksize > coef_len) {
        tv_set_error("tv_image_prep: image %d: %s table (offset %d, %d taps) outside the coefficient buffer", image, axis, tab, ksize);
        return -1;
    }
    const int* mn = coef + tab;
    const int* cnt = mn + n_out;
    for (int i = 0; i < n_out; ++i) {
        if (mn[i] < 0 || cnt[i] < 0 || cnt[i] > ksize || (long long)mn[i] + cnt[i] > in_size) {
            tv_set_error("tv_image_prep: image %d: %s table entry %d reaches [%d, %d) of %d input samples", image, axis, i, mn[i],
                         mn[i] + cnt[i], in_size);
            return -1;
        }
    }
    return 0;
}

}  // namespace

extern "C" int tv_image_prep(const void* src, long long src_bytes, const tv_image_desc* desc_host, const tv_image_desc* desc_dev, int B,
                             const int* coef_host, const int* coef_dev, long long coef_len, const float* lut, float* out, int res_h,
                             int res_w, void* stream) {
    TV_CHECK_ARG(src && desc_host && desc_dev && lut && out, "tv_image_prep: null pointer");
    TV_CHECK_ARG(B > 0 && B <= 65535, "tv_image_prep: batch of %d images (1 .. 65535)", B);
    TV_CHECK_ARG(res_h > 0 && res_w > 0, "tv_image_prep: empty output %dx%d", res_h, res_w);
    TV_CHECK_ARG(coef_len >= 0 && (coef_len == 0 || (coef_host && coef_dev)), "tv_image_prep: coefficient buffer missing");
    int lds_rows = IMG_TH;
    for (int b = 0; b < B; ++b) {
        const tv_image_desc& d = desc_host[b];
        if (d.channels != 3 || d.in_h <= 0 || d.in_w <= 0) {
            tv_set_error("tv_image_prep: image %d is %dx%dx%d: only non-empty 3-channel images are supported", b, d.in_h, d.in_w, d.channels);
            return TV_ERR_UNSUPPORTED;
        }
        TV_CHECK_ARG(d.out_h > 0 && d.out_w > 0, "tv_image_prep: image %d: empty resized size %dx%d", b, d.out_h, d.out_w);
        if ((long long)d.in_h > (long long)IMG_MAX_RATIO * d.out_h || (long long)d.in_w > (long long)IMG_MAX_RATIO * d.out_w) {
            tv_set_error("tv_image_prep: image %d: %dx%d -> %dx%d is a down-scale by more than %d", b, d.in_h, d.in_w, d.out_h, d.out_w,
                         IMG_MAX_RATIO);
            return TV_ERR_UNSUPPORTED;
        }
        TV_CHECK_ARG(d.row_stride >= 3ll * d.in_w && d.offset >= 0 &&
                         d.offset + (long long)(d.in_h - 1) * d.row_stride + 3ll * d.in_w <= src_bytes,
                     "tv_image_prep: image %d (offset %lld, %d rows of %d bytes) lies outside the %lld source bytes", b, d.offset, d.in_h,
                     d.row_stride, src_bytes);
        TV_CHECK_ARG(d.crop_top >= 0 && d.crop_left >= 0 && (long long)d.crop_top + res_h <= d.out_h &&
                         (long long)d.crop_left + res_w <= d.out_w,
                     "tv_image_prep: image %d: crop (%d, %d) + %dx%d outside the resized %dx%d", b, d.crop_top, d.crop_left, res_h, res_w,
                     d.out_h, d.out_w);
        if (d.xtab >= 0) {
            if (img_check_axis(coef_host, coef_len, d.xtab, d.xk, res_w, d.in_w, "horizontal", b) < 0) return TV_ERR_ARG;
        } else {
            TV_CHECK_ARG(d.out_w == d.in_w, "tv_image_prep: image %d: no horizontal table but width %d -> %d", b, d.in_w, d.out_w);
        }
        if (d.ytab >= 0) {
            if (img_check_axis(coef_host, coef_len, d.ytab, d.yk, res_h, d.in_h, "vertical", b) < 0) return TV_ERR_ARG;
            const int* mn = coef_host + d.ytab;
            const int* cnt = mn + res_h;
            for (int y0 = 0; y0 < res_h; y0 += IMG_TH) {       // the kernel stages [first row's start, last row's end)
                const int y1 = std::min(y0 + IMG_TH, res_h) - 1;
                const int lo = mn[y0], hi = mn[y1] + cnt[y1];
                for (int y = y0; y <= y1; ++y)
                    TV_CHECK_ARG(mn[y] >= lo && mn[y] + cnt[y] <= hi, "tv_image_prep: image %d: vertical table is not monotonic at row %d", b, y);
                lds_rows = std::max(lds_rows, hi - lo);
            }
        } else {
            TV_CHECK_ARG(d.out_h == d.in_h, "tv_image_prep: image %d: no vertical table but height %d -> %d", b, d.in_h, d.out_h);
        }
    }
    const long long lds = (long long)lds_rows * 3 * IMG_TW;
    if (lds > IMG_LDS_BYTES) {
        tv_set_error("tv_image_prep: a tile needs %d staged rows (%lld bytes of LDS, limit %d)", lds_rows, lds, IMG_LDS_BYTES);
        return TV_ERR_UNSUPPORTED;
    }
    const int tiles_x = tv_cdiv(res_w, IMG_TW), tiles_y = tv_cdiv(res_h, IMG_TH);
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)B), dim3(IMG_THREADS), (size_t)lds,
                       (hipStream_t)stream, (const uint8_t*)src, desc_dev, coef_dev, lut, out, res_h, res_w, tiles_x, lds_rows);
    TV_CHECK_LAUNCH("tv_image_prep");
    return TV_OK;
}

extern "C" int tv_image_grid_u8(const float* img, long long sn, long long sc, long long sh, long long sw, void* out, int B, int H, int W,
                                int nrow, int padding, float pad_value, int transform, void* stream) {
    TV_CHECK_ARG(img && out, "tv_image_grid_u8: null pointer");
    TV_CHECK_ARG(B > 0 && H > 0 && W > 0, "tv_image_grid_u8: empty batch");
    TV_CHECK_ARG(nrow > 0 && padding >= 0, "tv_image_grid_u8: nrow %d, padding %d", nrow, padding);
    TV_CHECK_ARG(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "tv_image_grid_u8: negative stride");
    TV_CHECK_ARG(transform == TV_IMAGE_NONE || transform == TV_IMAGE_SIGMOID, "tv_image_grid_u8: unknown transform %d", transform);
    const int pad = B == 1 ? 0 : padding;              // make_grid returns a single image as it is
    const int xmaps = std::min(nrow, B), ymaps = tv_cdiv(B, xmaps);
    const long long Hg = (long long)(H + pad) * ymaps + pad, Wg = (long long)(W + pad) * xmaps + pad;
    TV_CHECK_ARG(Hg <= 0x7fffffffll && Wg <= 0x7fffffffll && Hg * Wg <= 0x7fffffffll * IMG_THREADS, "tv_image_grid_u8: canvas %lld x %lld too large",
                 Hg, Wg);
    const long long blocks = (Hg * Wg + IMG_THREADS - 1) / IMG_THREADS;
    hipLaunchKernelGGL(image_grid_kernel, dim3((unsigned)blocks), dim3(IMG_THREADS), 0, (hipStream_t)stream, img, sn, sc, sh, sw,
                       (uint8_t*)out, B, H, W, xmaps, pad, (int)Hg, (int)Wg, pad_value, transform);
    TV_CHECK_LAUNCH("tv_image_grid_u8");
    return TV_OK;
}
