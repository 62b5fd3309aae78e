// Per-image reconstruction metrics of a batch of fp32 image pairs: MSE, PSNR and SSIM (evaluation side, no gradient).
//
//   TV_SSIM_SKIMAGE : skimage.metrics.structural_similarity(data_range=R, channel_axis=...) defaults, the metric of
//                     R/evaluate.py:105-124: 7x7 uniform window, scipy.ndimage 'reflect' border (d c b a | a b c d),
//                     sample covariance (x 49/48), map cropped by 3 px on each side, mean per channel, then over channels
//   TV_SSIM_BOX11   : P/evaluate_transvae.py:56-77: F.avg_pool2d(k=11, s=1, padding=5) (zero border, always / 121),
//                     population covariance, mean over the whole map
//   C1 = (0.01 R)^2, C2 = (0.03 R)^2;  PSNR = 10 log10(R^2 / mse), +inf when mse == 0 (both references)
//
// Launch 1 (stencil): one workgroup per (tile, image x channel).  It stages its TW x TH output tile plus the K-1 halo of
// both inputs in LDS once, as transformed fp32, and accumulates sum (x - y)^2 over the tile's own pixels on the way.  Each
// thread then owns one output column of one half of the tile and walks down its rows: the horizontal K-term sums of the
// five moments (x, y, xx, yy, xy) of one LDS row go into a ring of K rows held in registers, and every output row sums its
// ring directly (K terms, no running add / subtract along a row: that drifts in fp32 over 1024 rows).  One fp32 pair
// (sum of the SSIM map inside the averaging region, sum (x - y)^2) per workgroup; no atomics.
// Launch 2 (finalise): one block per image adds that image's partials in a fixed order in fp64, so an image's values are
// bit-reproducible and do not depend on the other images of the batch.
//
// The moments are taken about a per-tile pivot (the transformed value of the tile's centre pixel, one for x and one for
// y): covariances do not change, and E[x^2] - E[x]^2 then cancels far less in flat regions, where C2 = 9e-4 makes the
// SSIM sensitive to the variance's rounding.
#include "common.h"

namespace {

constexpr int MET_THREADS = 256;
constexpr int MET_TW = 128;                      // output tile width: one column per thread, two row halves
template <int K> struct MetTile {
    static constexpr int TH = K == 7 ? 64 : 56;  // raw tile (TW+K-1) x (TH+K-1) x 2 inputs: 75.0 / 72.9 KB -> 2 blocks per CU
    static constexpr int H = K / 2;              // halo
    static constexpr int NR = TH + K - 1, NC = MET_TW + K - 1;
    static constexpr int ROWS = TH / 2;          // output rows per thread
};

__device__ __forceinline__ float met_transform(float v, int xform, bool is_recon) {
    // np.clip / torch.clamp: a NaN is neither below 0 nor above 1 and passes through, so a diverged reconstruction reports
    // NaN (fminf / fmaxf return the other operand and would report the metrics of a black pixel)
    if (xform == TV_METRIC_CLIP) return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    if (xform == TV_METRIC_SIGMOID && is_recon) return 1.f / (1.f + expf(-v));
    return v;
}

// scipy.ndimage mode 'reflect' for one overhang of at most 3 (H, W >= 7), clamped so that coordinates of the part of a
// tile that lies beyond the image (outputs that are never counted) still address the image
__device__ __forceinline__ int met_reflect(int i, int n) {
    i = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
    return min(max(i, 0), n - 1);
}

template <int K>
__global__ __launch_bounds__(MET_THREADS, 2) void recon_metrics_tile_kernel(
    const float* __restrict__ xr, const float* __restrict__ yt, long long xsn, long long xsc, long long xsh, long long xsw,
    long long ysn, long long ysc, long long ysh, long long ysw, int C, int H, int W, int tiles_x, int xform, float data_range,
    float2* __restrict__ partial) {
    using T = MetTile<K>;
    constexpr bool REFLECT = K == 7;
    __shared__ float s_x[T::NR * T::NC];
    __shared__ float s_y[T::NR * T::NC];
    __shared__ float s_red[2][MET_THREADS / 64];

    const int tid = threadIdx.x;
    const int plane = blockIdx.y, b = plane / C, c = plane - b * C;
    const int ty0 = ((int)blockIdx.x / tiles_x) * T::TH, tx0 = ((int)blockIdx.x % tiles_x) * MET_TW;
    const float* xp = xr + b * xsn + c * xsc;
    const float* yp = yt + b * ysn + c * ysc;

    // pivots: the tile's centre pixel (inside the image)
    const int pr = min(ty0 + T::TH / 2, H - 1), pc = min(tx0 + MET_TW / 2, W - 1);
    const float px = met_transform(xp[pr * xsh + pc * xsw], xform, true);
    const float py = met_transform(yp[pr * ysh + pc * ysw], xform, false);

    // stage the tile + halo (transformed, about the pivots); sum (x - y)^2 over the tile's own pixels.  All of a thread's
    // loads are issued before the first is used: one HBM latency per tile instead of one per element.
    constexpr int NE = T::NR * T::NC, NL = (NE + MET_THREADS - 1) / MET_THREADS;
    float vx[NL], vy[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int e = tid + k * MET_THREADS;
        const int lr = e / T::NC, lc = e - lr * T::NC;
        const int r = ty0 - T::H + lr, cc = tx0 - T::H + lc;
        bool load = e < NE;
        int gr = r, gc = cc;
        if (REFLECT) {
            gr = met_reflect(r, H);
            gc = met_reflect(cc, W);
        } else {
            load = load && r >= 0 && r < H && cc >= 0 && cc < W;
        }
        vx[k] = load ? xp[gr * xsh + gc * xsw] : 0.f;
        vy[k] = load ? yp[gr * ysh + gc * ysw] : 0.f;
    }
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int e = tid + k * MET_THREADS;
        const int lr = e / T::NC, lc = e - lr * T::NC;
        const int r = ty0 - T::H + lr, cc = tx0 - T::H + lc;
        // zero border (box11) in the transformed domain: a padded element stays 0 whatever the transform
        const bool inside = REFLECT || (r >= 0 && r < H && cc >= 0 && cc < W);
        const float x = inside ? met_transform(vx[k], xform, true) : 0.f;
        const float y = inside ? met_transform(vy[k], xform, false) : 0.f;
        const bool own = lr >= T::H && lr < T::H + T::TH && lc >= T::H && lc < T::H + MET_TW && r < H && cc < W;
        const float d = x - y;
        sq = own ? fmaf(d, d, sq) : sq;
        if (e < NE) {
            s_x[e] = x - px;
            s_y[e] = y - py;
        }
    }
    __syncthreads();

    constexpr float inv_np = 1.f / (K * K);
    constexpr float cov_norm = REFLECT ? (float)(K * K) / (float)(K * K - 1) : 1.f;
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    const int lo = REFLECT ? T::H : 0;   // averaging region [lo, H - lo) x [lo, W - lo)
    const int col = tid % MET_TW, half = tid / MET_TW;
    const int gcol = tx0 + col;
    const bool col_in = gcol >= lo && gcol < W - lo;
    const int row0 = half * T::ROWS;          // first output row (tile-local) of this thread; LDS rows row0 .. row0+ROWS+K-2
    const float* sx = s_x + row0 * T::NC + col;
    const float* sy = s_y + row0 * T::NC + col;

    float ring[K][5];
    float ssum = 0.f;
    constexpr int NIN = T::ROWS + K - 1;
    for (int i0 = 0; i0 < NIN; i0 += K) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = i0 + k;   // LDS row (relative to row0) entering the ring at slot k
            if (i < NIN) {
                float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float x = sx[i * T::NC + j], y = sy[i * T::NC + j];
                    m0 += x;
                    m1 += y;
                    m2 = fmaf(x, x, m2);
                    m3 = fmaf(y, y, m3);
                    m4 = fmaf(x, y, m4);
                }
                ring[k][0] = m0;
                ring[k][1] = m1;
                ring[k][2] = m2;
                ring[k][3] = m3;
                ring[k][4] = m4;
                if (i >= K - 1) {
                    float v[5];
#pragma unroll
                    for (int m = 0; m < 5; ++m) {
                        float s = 0.f;
#pragma unroll
                        for (int q = 0; q < K; ++q) s += ring[q][m];
                        v[m] = s * inv_np;
                    }
                    const float mx = v[0], my = v[1];
                    const float vx = cov_norm * (v[2] - mx * mx), vy = cov_norm * (v[3] - my * my);
                    const float vxy = cov_norm * (v[4] - mx * my);
                    const float ux = mx + px, uy = my + py;
                    const float num = (2.f * ux * uy + c1) * (2.f * vxy + c2);
                    const float den = (ux * ux + uy * uy + c1) * (vx + vy + c2);
                    const int grow = ty0 + row0 + i - (K - 1);
                    const bool in = col_in && grow >= lo && grow < H - lo;
                    ssum += in ? num / den : 0.f;
                }
            }
        }
    }

    ssum = tv_wave_sum(ssum);
    sq = tv_wave_sum(sq);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
        s_red[0][wave] = ssum;
        s_red[1][wave] = sq;
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, d = 0.f;
#pragma unroll
        for (int w = 0; w < MET_THREADS / 64; ++w) {
            a += s_red[0][w];
            d += s_red[1][w];
        }
        partial[(long long)plane * gridDim.x + blockIdx.x] = make_float2(a, d);
    }
}

// out[0][b] = mse, out[1][b] = psnr, out[2][b] = ssim (mean over channels of the per-channel mean SSIM)
__global__ __launch_bounds__(256) void recon_metrics_finalize_kernel(const float2* __restrict__ partial, int B, int C, int tiles,
                                                                     double ssim_count, double mse_count, double r2,
                                                                     float* __restrict__ out) {
    __shared__ double s_red[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double ssim_acc = 0.0, sq_acc = 0.0;   // meaningful in thread 0
    for (int c = 0; c < C; ++c) {
        const float2* p = partial + ((long long)b * C + c) * tiles;
        double a = 0.0, d = 0.0;
        for (int t = tid; t < tiles; t += 256) {
            const float2 v = p[t];
            a += (double)v.x;
            d += (double)v.y;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            d += __shfl_xor(d, o, 64);
        }
        if (lane == 0) {
            s_red[0][wave] = a;
            s_red[1][wave] = d;
        }
        __syncthreads();
        if (tid == 0) {
            ssim_acc += (s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]) / ssim_count;
            sq_acc += s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mse = sq_acc / mse_count;
        out[b] = (float)mse;
        out[B + b] = mse == 0.0 ? __builtin_huge_valf() : (float)(10.0 * log10(r2 / mse));
        out[2 * B + b] = (float)(ssim_acc / C);
    }
}

int met_tiles(int H, int W, int kind) {
    const int th = kind == TV_SSIM_SKIMAGE ? MetTile<7>::TH : MetTile<11>::TH;
    return tv_cdiv(H, th) * tv_cdiv(W, MET_TW);
}

}  // namespace

extern "C" long long tv_recon_metrics_partial_count(int B, int C, int H, int W, int kind) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (kind != TV_SSIM_SKIMAGE && kind != TV_SSIM_BOX11)) return -1;
    return 2ll * B * C * met_tiles(H, W, kind);
}

extern "C" int tv_recon_metrics(const float* recon, const float* target, long long rsn, long long rsc, long long rsh, long long rsw,
                                long long tsn, long long tsc, long long tsh, long long tsw, int B, int C, int H, int W, int kind,
                                int transform, float data_range, float* partials, float* out, void* stream) {
    TV_CHECK_ARG(recon && target && partials && out, "tv_recon_metrics: null pointer");
    TV_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "tv_recon_metrics: empty batch");
    TV_CHECK_ARG(kind == TV_SSIM_SKIMAGE || kind == TV_SSIM_BOX11, "tv_recon_metrics: unknown SSIM kind %d", kind);
    TV_CHECK_ARG(transform == TV_METRIC_NONE || transform == TV_METRIC_CLIP || transform == TV_METRIC_SIGMOID,
                 "tv_recon_metrics: unknown transform %d", transform);
    TV_CHECK_ARG(kind != TV_SSIM_SKIMAGE || (H >= 7 && W >= 7), "tv_recon_metrics: the skimage window needs H, W >= 7 (got %dx%d)",
                 H, W);
    TV_CHECK_ARG(data_range > 0.f, "tv_recon_metrics: data_range must be positive");
    TV_CHECK_ARG(rsn >= 0 && rsc >= 0 && rsh >= 0 && rsw >= 0 && tsn >= 0 && tsc >= 0 && tsh >= 0 && tsw >= 0,
                 "tv_recon_metrics: negative stride");
    TV_CHECK_ARG((long long)B * C <= 65535, "tv_recon_metrics: B * C > 65535");
    const int tiles_x = tv_cdiv(W, MET_TW), tiles = met_tiles(H, W, kind);
    hipStream_t s = (hipStream_t)stream;
    float2* part = reinterpret_cast<float2*>(partials);
    const dim3 grid((unsigned)tiles, (unsigned)(B * C));
    double ssim_count;
    if (kind == TV_SSIM_SKIMAGE) {
        hipLaunchKernelGGL(recon_metrics_tile_kernel<7>, grid, dim3(MET_THREADS), 0, s, recon, target, rsn, rsc, rsh, rsw, tsn, tsc,
                           tsh, tsw, C, H, W, tiles_x, transform, data_range, part);
        ssim_count = (double)(H - 6) * (double)(W - 6);
    } else {
        hipLaunchKernelGGL(recon_metrics_tile_kernel<11>, grid, dim3(MET_THREADS), 0, s, recon, target, rsn, rsc, rsh, rsw, tsn, tsc,
                           tsh, tsw, C, H, W, tiles_x, transform, data_range, part);
        ssim_count = (double)H * (double)W;
    }
    const double r = (double)data_range;
    hipLaunchKernelGGL(recon_metrics_finalize_kernel, dim3((unsigned)B), dim3(256), 0, s, part, B, C, tiles, ssim_count,
                       (double)C * H * W, r * r, out);
    TV_CHECK_LAUNCH("tv_recon_metrics");
    return TV_OK;
}
