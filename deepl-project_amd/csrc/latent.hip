// Latent-space statistics: the streaming fp64 moments of every latent the encoder produces (tv_latent_stats) and a Gaussian
// kernel density estimate in the log domain (tv_kde_logdensity).  transvae/latents.py drives both.
//
// tv_latent_stats.  A sample is one (image, position) pair of x [B, D, P]; S = B * P samples per call.
//   1. latent_mean_kernel     one block per channel: 256 per-thread fp64 sums over samples t, t + 256, ..., added by a fixed LDS
//                             tree; batch mean, its offset from the running mean, and the running mean's update
//   2. latent_scatter_kernel  G = min(256, ceil(S / 512)) blocks, each the D x D scatter of its own sample range about the batch
//                             mean: acc[j][k] = fma(d_j, d_k, acc[j][k]) sample by sample.  (j, k) and (k, j) see the same
//                             operands in the same order, so the partials are bit-symmetric
//   3. latent_merge_kernel    partials added in block order, then Chan's update M2 += M2b + delta_j delta_k (na nb / n)
//   No atomics; the geometry is a function of (B, P) alone, so the same sequence of calls gives the same bits.
//
// tv_kde_logdensity.  One thread owns one query (its d <= 64 coordinates in registers), a block of 256 queries shares 128-point
// data tiles staged in LDS (every lane reads the same address: a broadcast, no bank conflicts).  Squared distances are direct
// differences, an fmaf chain over k in order, 8 independent data points in flight per thread.  The running reference is the
// smallest distance so far (= the largest score): a_j = -inv_2h2 * (dist_j - dmin) <= 0, two roundings, and EXACTLY 0 at the
// nearest point (a rounded product inv_2h2 * dmin as the reference would be off by up to u |s|, which at |s| > 1.5e9 -- a point at
// 1e3 with h = 0.01 -- pushes every exponent below the underflow).  p_j = exp2(a_j * log2(e)) (v_exp_f32).  Eight p_j are added
// as a fp32 tree, the running sum is fp64, and when the reference moves the sum is rescaled by an fp64 exponential (rare, and
// free of fp32 error).  The result log(sum) - inv_2h2 * dmin is formed in fp64 (the product of two floats is exact there) and
// rounded once.
// When M < 2048 the data range is cut into up to 64 slices (grid.y); each (query, slice) leaves {ref, sum} and a second launch
// merges them in slice order.  Work: N * M * (2 d + ~6) fp32 operations; bytes: N * d * 4 per 256 queries.
// Inner loop as compiled (plain -O3): the SLP pass pairs neighbouring data points into v_pk_add_f32 / v_pk_fma_f32.  Each half
// is an IEEE operation, so the bits are those of the scalar chain; there is no MFMA beside them whose issue they could delay,
// which is where packed fp32 costs on this chip.  No kernel here spills (248 VGPRs at d = 64, one wave per SIMD there).
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// tv_latent_stats
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LS_MAXG = 256;        // scatter partials at most
constexpr int LS_CHUNK = 512;       // samples per scatter block at least
constexpr int LS_ROWS = 32;         // samples staged per step
constexpr int LS_HDR = 192;         // scratch: mb[64], delta[64], na, padding; the partials follow

__device__ __forceinline__ double ls_load(const float* __restrict__ x, long long s, int c, int P, long long sn, long long sc) {
    const long long b = s / P;
    return (double)x[b * sn + (long long)c * sc + (s - b * P)];
}

__global__ __launch_bounds__(256) void latent_mean_kernel(const float* __restrict__ x, long long sn, long long sc, long long S, int P,
                                                          double* __restrict__ state, double* __restrict__ scratch) {
    __shared__ double sm[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double acc = 0.0;
    for (long long s = t; s < S; s += 256) acc += ls_load(x, s, c, P, sn, sc);
    sm[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sm[t] += sm[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const double na = state[0], nb = (double)S;
        const double mb = sm[0] / nb, delta = mb - state[1 + c];
        scratch[c] = mb;
        scratch[64 + c] = delta;
        if (c == 0) scratch[128] = na;
        state[1 + c] += delta * (nb / (na + nb));
    }
}

// thread (ty, tx) of 16 x 16 owns the TS x TS entries (ty TS + p, tx TS + q); 16 TS >= D
template <int TS>
__global__ __launch_bounds__(256) void latent_scatter_kernel(const float* __restrict__ x, long long sn, long long sc, long long S, int P,
                                                             int D, long long chunk, const double* __restrict__ scratch,
                                                             double* __restrict__ part) {
    constexpr int W = 16 * TS;
    __shared__ double da[LS_ROWS][W];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const long long sbeg = (long long)blockIdx.x * chunk;
    const long long send = sbeg + chunk < S ? sbeg + chunk : S;
    double acc[TS][TS];
#pragma unroll
    for (int p = 0; p < TS; ++p)
#pragma unroll
        for (int q = 0; q < TS; ++q) acc[p][q] = 0.0;
    for (long long s0 = sbeg; s0 < send; s0 += LS_ROWS) {
        __syncthreads();
        for (int e = t; e < LS_ROWS * W; e += 256) {
            const int r = e % LS_ROWS, c = e / LS_ROWS;
            const bool ok = s0 + r < send && c < D;              // rows past the range and channels past D stage zeros
            da[r][c] = ok ? ls_load(x, s0 + r, c, P, sn, sc) - scratch[c] : 0.0;
        }
        __syncthreads();
        const int rows = send - s0 < LS_ROWS ? (int)(send - s0) : LS_ROWS;
        for (int r = 0; r < rows; ++r) {
            double a[TS], b[TS];
#pragma unroll
            for (int p = 0; p < TS; ++p) { a[p] = da[r][ty * TS + p]; b[p] = da[r][tx * TS + p]; }
#pragma unroll
            for (int p = 0; p < TS; ++p)
#pragma unroll
                for (int q = 0; q < TS; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
        }
    }
    double* dst = part + (size_t)blockIdx.x * D * D;
#pragma unroll
    for (int p = 0; p < TS; ++p)
#pragma unroll
        for (int q = 0; q < TS; ++q) {
            const int j = ty * TS + p, k = tx * TS + q;
            if (j < D && k < D) dst[j * D + k] = acc[p][q];
        }
}

__global__ __launch_bounds__(256) void latent_merge_kernel(const double* __restrict__ scratch, const double* __restrict__ part, int G, int D,
                                                           long long S, double* __restrict__ state) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= D * D) return;
    double m2b = 0.0;
    for (int g = 0; g < G; ++g) m2b += part[(size_t)g * D * D + e];
    const double na = scratch[128], nb = (double)S, n = na + nb;
    const double w = na * (nb / n);
    const double dd = scratch[64 + e / D] * scratch[64 + e % D];
    double* m2 = state + 1 + D;
    m2[e] = m2[e] + (m2b + dd * w);
    if (e == 0) state[0] = n;
}

// ---------------------------------------------------------------------------------------------------------------------
// tv_kde_logdensity
// ---------------------------------------------------------------------------------------------------------------------
constexpr int KDE_TJ = 128;            // data points per LDS tile
constexpr int KDE_JU = 8;              // data points in flight per thread
constexpr int KDE_SPLIT_BELOW = 2048;  // fewer queries than this: the data range is split across blocks
constexpr int KDE_SPLIT_MIN = 1024;    // data points per slice at least
constexpr int KDE_SPLIT_MAX = 64;      // slices at most

inline int kde_slices(int N, int M) {
    if (M >= KDE_SPLIT_BELOW) return 1;
    const int s = tv_cdiv(N, KDE_SPLIT_MIN);
    return s < KDE_SPLIT_MAX ? s : KDE_SPLIT_MAX;
}

template <int DP, bool EXCL>
__global__ __launch_bounds__(256) void kde_kernel(const float* __restrict__ x, int N, const float* __restrict__ q, int M, int d, int ldx,
                                                  int ldq, float inv, int per, int slices, float* __restrict__ out,
                                                  double* __restrict__ part) {
    __shared__ float tile[KDE_TJ * DP];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int iq = i < M ? i : M - 1;                     // lanes past M compute a copy of the last query and store nothing
    float qv[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) qv[k] = k < d ? q[(size_t)iq * ldq + k] : 0.f;   // padded coordinates: 0 - 0, the chain adds 0
    const int jbeg = blockIdx.y * per;
    const int jend = jbeg + per < N ? jbeg + per : N;
    float dmin = INFINITY;
    double sum = 0.0;
    for (int j0 = jbeg; j0 < jend; j0 += KDE_TJ) {
        __syncthreads();
        for (int e = threadIdx.x; e < KDE_TJ * DP; e += 256) {
            const int j = j0 + e / DP, k = e % DP;
            tile[e] = (j < jend && k < d) ? x[(size_t)j * ldx + k] : 0.f;
        }
        __syncthreads();
        const int jn = jend - j0 < KDE_TJ ? jend - j0 : KDE_TJ;
        for (int g = 0; g < jn; g += KDE_JU) {
            float dist[KDE_JU];
#pragma unroll
            for (int u = 0; u < KDE_JU; ++u) dist[u] = 0.f;
#pragma unroll
            for (int k = 0; k < DP; ++k)
#pragma unroll
                for (int u = 0; u < KDE_JU; ++u) {
                    const float t = qv[k] - tile[(g + u) * DP + k];
                    dist[u] = fmaf(t, t, dist[u]);
                }
            float gmin = INFINITY;
#pragma unroll
            for (int u = 0; u < KDE_JU; ++u) {
                if (g + u >= jn || (EXCL && j0 + g + u == i)) dist[u] = INFINITY;   // dropped by index: p = exp2(-inf) = 0
                gmin = fminf(gmin, dist[u]);
            }
            if (gmin < dmin) {                              // the reference moves: rescale the fp64 sum by an fp64 exponential
                if (sum != 0.0) sum *= exp((double)inv * ((double)gmin - (double)dmin));
                dmin = gmin;
            }
            const float dref = dmin < INFINITY ? dmin : 0.f;   // nothing finite yet: every dist is inf, and inf - inf is not wanted
            float p[KDE_JU];
#pragma unroll
            for (int u = 0; u < KDE_JU; ++u) p[u] = __builtin_amdgcn_exp2f(-inv * (dist[u] - dref) * 1.44269504088896340736f);
            sum += (double)(((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
        }
    }
    if (i >= M) return;
    const bool empty = !(dmin < INFINITY);
    const double ref = (double)inv * (double)dmin;         // exact: 24 x 24 bits
    if (slices == 1) {
        out[i] = empty ? -INFINITY : (float)(log(sum) - ref);
    } else {
        double* dst = part + ((size_t)i * slices + blockIdx.y) * 2;
        dst[0] = empty ? (double)INFINITY : ref;
        dst[1] = empty ? 0.0 : sum;
    }
}

__global__ __launch_bounds__(256) void kde_merge_kernel(const double* __restrict__ part, int M, int slices, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double* src = part + (size_t)i * slices * 2;
    double r = INFINITY;
    for (int s = 0; s < slices; ++s) r = fmin(r, src[2 * s]);
    if (!(r < INFINITY)) { out[i] = -INFINITY; return; }
    double tot = 0.0;
    for (int s = 0; s < slices; ++s)
        if (src[2 * s] < INFINITY) tot += src[2 * s + 1] * exp(r - src[2 * s]);
    out[i] = (float)(log(tot) - r);
}

template <int DP>
void kde_launch(dim3 grid, hipStream_t s, bool excl, const float* x, int N, const float* q, int M, int d, int ldx, int ldq, float inv, int per,
                int slices, float* out, double* part) {
    if (excl) hipLaunchKernelGGL((kde_kernel<DP, true>), grid, dim3(256), 0, s, x, N, q, M, d, ldx, ldq, inv, per, slices, out, part);
    else hipLaunchKernelGGL((kde_kernel<DP, false>), grid, dim3(256), 0, s, x, N, q, M, d, ldx, ldq, inv, per, slices, out, part);
}

}  // namespace

extern "C" int tv_latent_stats(const float* x, long long sn, long long sc, int B, int D, int P, double* state, double* scratch, void* stream) {
    TV_CHECK_ARG(x && state && scratch && B > 0 && P > 0, "tv_latent_stats: bad arguments");
    TV_CHECK_ARG(D >= 1 && D <= 64, "tv_latent_stats: D=%d must be in [1, 64]", D);
    TV_CHECK_ARG(sc >= P && sn >= (long long)(D - 1) * sc + P, "tv_latent_stats: strides (%lld, %lld) overlap for D=%d, P=%d", sn, sc, D, P);
    hipStream_t s = (hipStream_t)stream;
    const long long S = (long long)B * P;
    long long G = (S + LS_CHUNK - 1) / LS_CHUNK;
    if (G > LS_MAXG) G = LS_MAXG;
    long long chunk = (S + G - 1) / G;
    chunk = (chunk + LS_ROWS - 1) / LS_ROWS * LS_ROWS;
    G = (S + chunk - 1) / chunk;
    double* part = scratch + LS_HDR;
    hipLaunchKernelGGL(latent_mean_kernel, dim3((unsigned)D), dim3(256), 0, s, x, sn, sc, S, P, state, scratch);
    TV_CHECK_LAUNCH("tv_latent_stats (means)");
    if (D <= 16) hipLaunchKernelGGL(latent_scatter_kernel<1>, dim3((unsigned)G), dim3(256), 0, s, x, sn, sc, S, P, D, chunk, (const double*)scratch, part);
    else if (D <= 32) hipLaunchKernelGGL(latent_scatter_kernel<2>, dim3((unsigned)G), dim3(256), 0, s, x, sn, sc, S, P, D, chunk, (const double*)scratch, part);
    else hipLaunchKernelGGL(latent_scatter_kernel<4>, dim3((unsigned)G), dim3(256), 0, s, x, sn, sc, S, P, D, chunk, (const double*)scratch, part);
    TV_CHECK_LAUNCH("tv_latent_stats (scatter)");
    hipLaunchKernelGGL(latent_merge_kernel, dim3((unsigned)tv_cdiv(D * D, 256)), dim3(256), 0, s, (const double*)scratch, (const double*)part, (int)G, D,
                       S, state);
    TV_CHECK_LAUNCH("tv_latent_stats (merge)");
    return TV_OK;
}

extern "C" int tv_kde_logdensity(const float* x, int N, const float* q, int M, int d, int ldx, int ldq, float inv_2h2, int exclude_self,
                                 float* out, double* scratch, void* stream) {
    TV_CHECK_ARG(x && q && out && N >= 1 && N <= (1 << 30) && M >= 1, "tv_kde_logdensity: bad arguments");
    TV_CHECK_ARG(d >= 1 && d <= 64 && ldx >= d && ldq >= d, "tv_kde_logdensity: d=%d must be in [1, 64] with ldx=%d, ldq=%d >= d", d, ldx, ldq);
    TV_CHECK_ARG(inv_2h2 > 0.f && inv_2h2 < INFINITY, "tv_kde_logdensity: inv_2h2 must be positive and finite");
    TV_CHECK_ARG(!exclude_self || (N >= 2 && M == N), "tv_kde_logdensity: exclude_self needs q == x (M == N) and N >= 2 (N=%d, M=%d)", N, M);
    const int slices0 = kde_slices(N, M);
    const int per = tv_cdiv(tv_cdiv(N, slices0), KDE_TJ) * KDE_TJ;
    const int slices = tv_cdiv(N, per);
    TV_CHECK_ARG(slices == 1 || scratch, "tv_kde_logdensity: M=%d < %d needs scratch", M, KDE_SPLIT_BELOW);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tv_cdiv(M, 256), (unsigned)slices);
    const bool ex = exclude_self != 0;
    if (d <= 2) kde_launch<2>(grid, s, ex, x, N, q, M, d, ldx, ldq, inv_2h2, per, slices, out, scratch);
    else if (d <= 4) kde_launch<4>(grid, s, ex, x, N, q, M, d, ldx, ldq, inv_2h2, per, slices, out, scratch);
    else if (d <= 8) kde_launch<8>(grid, s, ex, x, N, q, M, d, ldx, ldq, inv_2h2, per, slices, out, scratch);
    else if (d <= 16) kde_launch<16>(grid, s, ex, x, N, q, M, d, ldx, ldq, inv_2h2, per, slices, out, scratch);
    else if (d <= 32) kde_launch<32>(grid, s, ex, x, N, q, M, d, ldx, ldq, inv_2h2, per, slices, out, scratch);
    else kde_launch<64>(grid, s, ex, x, N, q, M, d, ldx, ldq, inv_2h2, per, slices, out, scratch);
    TV_CHECK_LAUNCH("tv_kde_logdensity");
    if (slices > 1) {
        hipLaunchKernelGGL(kde_merge_kernel, dim3((unsigned)tv_cdiv(M, 256)), dim3(256), 0, s, (const double*)scratch, M, slices, out);
        TV_CHECK_LAUNCH("tv_kde_logdensity (merge)");
    }
    return TV_OK;
}
