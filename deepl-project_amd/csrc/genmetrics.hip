// Generation metrics (transvae/metrics_gen.py drives them all):
//   tv_knn_radius        squared distance to the k-th nearest neighbour inside one feature set   (improved precision / recall,
//   tv_manifold_hits     is a query inside any of the k-NN balls of a set                          Kynkaanniemi et al. 2019)
//   tv_ball_counts       how many balls hold a query / how many points a query's ball holds      (density / coverage, Naeem et al. 2020)
//   tv_poly_kernel_sums  sums of (gamma x.y + c0)^3 over index-addressed subsets of rows         (KID, Binkowski et al. 2018)
//   tv_softmax_stats     streaming fp64 sums of p log p and of p over classifier rows            (Inception Score)
//
// Squared distance, shared by the two pairwise kernels.  D(a, b) = sum_c (a_c - b_c)^2 as ONE fp32 chain over c = 0 .. d - 1 in
// order: diff = a_c - b_c (one rounding), acc = fmaf(diff, diff, acc).  No partial chains: the accumulator of a (query, point) pair
// lives in a register across all d-chunks.  Never the Gram form.  a - b and b - a differ in sign only, so D(a, b) and D(b, a) are
// the same bits; the chain does not depend on the tile, the slice or the load path.  Coordinates past d stage as 0 on both sides:
// fmaf(0, 0, acc) = acc exactly.  Bound against fp64: (d + 2) u D (every term is non-negative).
//
// Geometry.  256 threads own a 64-query x 64-point tile, thread (ty, tx) of 16 x 16 the 4 x 4 pairs (ty 4 + p, tx 4 + q).  d goes
// through LDS in chunks of 32 floats per side, stored coordinate-major with a row stride of 68 floats: a thread's operands are two
// ds_read_b128 per coordinate (four addresses per wave on the query side: a broadcast; sixteen consecutive float4 on the data side:
// every bank once), and the transposing stores are 2-way conflicted.  The next chunk is loaded from memory into registers while the
// current one is consumed.  A block keeps its 64 queries and walks its data range tile by tile; the query strip is re-read from L2.
// When ceil(M / 64) < 512 blocks would leave the chip idle, the data range is cut into up to 32 slices of at least 256 points
// (grid.y) and a second launch merges the slices in slice order.  float4 loads when every row is 16-byte aligned, scalar otherwise.
//   knn: a thread keeps a sorted list of the 8 smallest distances per query row (min / max insertion); the 16 lists of a row
//        are merged through LDS in tx order; r2 = entry k - 1.  Self is dropped by index, points past N by index.
//   hits: hit |= D <= r2[j] on the fp32 values; the 16 flags of a row are OR-ed through LDS.
//   counts: count += D <= r2[j] (one radius per data point) or D <= r2[i] (one radius per query), the same comparison on the same
//        chain; the 16 counts of a row are added through LDS, the slices by the merge launch.  Integer sums carry no order question.
// The k smallest values of a multiset do not depend on the order they are met in, and neither does an OR: no atomics, the same bits
// on every run and for every cut of the query range into launches.  Inputs must be finite: fminf / fmaxf drop a NaN distance and
// repeat a list entry in its place, so a non-finite row corrupts the radii silently; the callers check.
//
// tv_poly_kernel_sums.  The same staging (pw_tile: loader, PW_LD layout, float4 or scalar loads, zeros past d) with the product
// chain dot = fmaf(a_c, b_c, dot) in place of the difference chain; the rows of a tile are addressed through int32 index lists, one
// pair of lists per subset (grid.z), so nothing is gathered and no m x m matrix exists.  Per pair, fp64 with contraction off:
// t = (double)dot * gamma + coef0, k = (t * t) * t.  A thread adds its 16 pairs in (p, e) order, thread 0 adds the 256 thread
// partials in thread order, and the finalise launch adds the block partials of a subset in block order: no atomics, the same bits on
// every run and for both load paths.
//
// tv_softmax_stats.  One block per row: z - max, exp, p = e / s, log p = (z - max) - log s, all fp64; the row sum s and the row's
// sum of p log p are added by one thread in k order.  A second launch adds the rows to the state one at a time in row order.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int PW_T = 64;          // tile side (queries and points)
constexpr int PW_C = 32;          // coordinates per chunk
constexpr int PW_LD = 68;         // LDS row stride (floats): 16-byte aligned rows, transposing stores 2-way conflicted
constexpr int PW_K = 8;           // list length = largest k
constexpr int PW_SIDE = PW_C * PW_LD;
constexpr int PW_FULL_BLOCKS = 512;   // query blocks from which the data range is not cut
constexpr int PW_TARGET = 1024;       // blocks aimed at when it is
constexpr int PW_SLICE_MIN = 256;     // data points per slice at least
constexpr int PW_SLICE_MAX = 32;      // slices at most

inline int pw_slices(int N, int M) {
    const int qb = tv_cdiv(M, PW_T);
    if (qb >= PW_FULL_BLOCKS) return 1;
    int s = tv_cdiv(PW_TARGET, qb);
    const int cap = tv_cdiv(N, PW_SLICE_MIN);
    if (s > cap) s = cap;
    if (s > PW_SLICE_MAX) s = PW_SLICE_MAX;
    return s < 1 ? 1 : s;
}

// four coordinates col .. col + 3 of one row (nullptr: a row past the range); coordinates past d are 0
template <bool VEC>
__device__ __forceinline__ f32x4 pw_load(const float* __restrict__ row, int col, int d) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row) return v;
    if (VEC && col + 3 < d) return *(const f32x4*)(row + col);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (col + e < d) v[e] = row[col + e];
    return v;
}

typedef __attribute__((ext_vector_type(8))) float f32x8;   // a sorted list: a vector, so that it stays in registers
static_assert(PW_K == 8, "the list type holds PW_K entries");

__device__ __forceinline__ void pw_insert(f32x8& l, float v) {
#pragma unroll
    for (int s = 0; s < PW_K; ++s) {
        const float lo = fminf(l[s], v);
        v = fmaxf(l[s], v);
        l[s] = lo;
    }
}

__device__ __forceinline__ float pw_kth(const f32x8& l, int k) {
    float r = l[0];
#pragma unroll
    for (int s = 1; s < PW_K; ++s)
        if (s == k - 1) r = l[s];
    return r;
}

// One 64 x 64 tile of pairs: acc[p][e] = the chain over c = 0 .. d - 1 of the pair (row ty 4 + p of the q side, row tx 4 + e of the x
// side).  DOT false: diff = a_c - b_c, acc = fmaf(diff, diff, acc) (squared distance); DOT true: acc = fmaf(a_c, b_c, acc) (dot
// product).  Thread t loads rows lr = t >> 3 and lr + 32 of either side (qrow / xrow; nullptr: a row past the range, staged as zeros).
template <bool VEC, bool DOT>
__device__ __forceinline__ void pw_tile(const float* (&qrow)[2], const float* (&xrow)[2], int d, float* __restrict__ qs,
                                        float* __restrict__ xs, float (&acc)[4][4]) {
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int lr = t >> 3, lc = (t & 7) * 4;            // loader: rows lr and lr + 32, coordinates lc .. lc + 3 of the chunk
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[p][c] = 0.f;
    f32x4 pq[2], px[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        pq[s] = pw_load<VEC>(qrow[s], lc, d);
        px[s] = pw_load<VEC>(xrow[s], lc, d);
    }
    for (int c0 = 0; c0 < d; c0 += PW_C) {
        __syncthreads();                                // the previous chunk (or the previous tile's epilogue) has been read
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                qs[(lc + e) * PW_LD + lr + 32 * s] = pq[s][e];
                xs[(lc + e) * PW_LD + lr + 32 * s] = px[s][e];
            }
        __syncthreads();
        if (c0 + PW_C < d) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                pq[s] = pw_load<VEC>(qrow[s], c0 + PW_C + lc, d);
                px[s] = pw_load<VEC>(xrow[s], c0 + PW_C + lc, d);
            }
        }
#pragma unroll
        for (int c = 0; c < PW_C; ++c) {
            const f32x4 a = *(const f32x4*)&qs[c * PW_LD + ty * 4];
            const f32x4 b = *(const f32x4*)&xs[c * PW_LD + tx * 4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (DOT) {
                        acc[p][e] = fmaf(a[p], b[e], acc[p][e]);
                    } else {
                        const float df = a[p] - b[e];
                        acc[p][e] = fmaf(df, df, acc[p][e]);
                    }
                }
        }
    }
}

// MODE 0: knn radius (out, part: float; self = index in x of query 0).  MODE 1: hits (out, part: int; r2 per data point).
// MODE 2 / 3: ball counts (out, part: int) with r2 per data point / per query.
// (MODE 3 asks for two blocks per CU: left alone, the scheduler hoists LDS reads until it holds 257 registers and one wave per SIMD
// remains, which doubles the kernel's time; the other modes settle at 176-204 on their own and are built as before)
template <int MODE, bool VEC>
__global__ __launch_bounds__(256, MODE == 3 ? 2 : 1) void pairwise_kernel(const float* __restrict__ q, int M, int ldq, const float* __restrict__ x, int N, int ldx,
                                                       int d, int self, const float* __restrict__ r2, int per, int slices, int k,
                                                       void* __restrict__ out, void* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[PW_T * 16 * PW_K];   // staging (2 x 32 x 68) first, the row merge afterwards
    float* qs = sm;
    float* xs = sm + PW_SIDE;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int qi0 = blockIdx.x * PW_T;
    const int jbeg = blockIdx.y * per;
    const int jend = jbeg + per < N ? jbeg + per : N;
    const int lr = t >> 3;                              // loader rows lr and lr + 32 (pw_tile)
    const float* qrow[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int r = qi0 + lr + 32 * s;
        qrow[s] = r < M ? q + (size_t)r * ldq : nullptr;
    }
    f32x8 list[4];
    bool hit[4] = {false, false, false, false};
    int cnt[4] = {0, 0, 0, 0};
    float rq[4] = {-1.f, -1.f, -1.f, -1.f};             // MODE 3: the radii of this thread's four queries (past the range: never stored)
    if (MODE == 3) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (qi0 + ty * 4 + p < M) rq[p] = r2[qi0 + ty * 4 + p];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int s = 0; s < PW_K; ++s) list[p][s] = INFINITY;

    for (int j0 = jbeg; j0 < jend; j0 += PW_T) {
        const float* xrow[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int r = j0 + lr + 32 * s;
            xrow[s] = r < jend ? x + (size_t)r * ldx : nullptr;
        }
        float acc[4][4];
        pw_tile<VEC, false>(qrow, xrow, d, qs, xs, acc);
        if (MODE == 0) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = j0 + tx * 4 + e;
                    const bool drop = j >= jend || j == self + qi0 + ty * 4 + p;   // past the range, or the query itself: by index
                    pw_insert(list[p], drop ? INFINITY : acc[p][e]);
                }
        } else if (MODE == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + tx * 4 + e;
                const float rj = j < jend ? r2[j] : -1.f;                         // D >= 0 > -1: a point past the range never hits
#pragma unroll
                for (int p = 0; p < 4; ++p) hit[p] = hit[p] || acc[p][e] <= rj;
            }
        } else if (MODE == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + tx * 4 + e;
                const float rj = j < jend ? r2[j] : -1.f;
#pragma unroll
                for (int p = 0; p < 4; ++p) cnt[p] += acc[p][e] <= rj ? 1 : 0;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lim = j0 + tx * 4 + e < jend ? INFINITY : -1.f;       // a point past the range never counts: D >= 0 > -1
#pragma unroll
                for (int p = 0; p < 4; ++p) cnt[p] += acc[p][e] <= fminf(rq[p], lim) ? 1 : 0;
            }
        }
    }

    __syncthreads();                                    // staging no longer read: the buffer becomes the row merge
    const int i = qi0 + t;
    if (MODE == 0) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int s = 0; s < PW_K; ++s) sm[((ty * 4 + p) * 16 + tx) * PW_K + s] = list[p][s];
        __syncthreads();
        if (t >= PW_T || i >= M) return;
        f32x8 l;
#pragma unroll
        for (int s = 0; s < PW_K; ++s) l[s] = sm[t * 16 * PW_K + s];
        for (int u = 1; u < 16; ++u)
#pragma unroll
            for (int s = 0; s < PW_K; ++s) pw_insert(l, sm[(t * 16 + u) * PW_K + s]);
        if (slices == 1) {
            ((float*)out)[i] = pw_kth(l, k);
        } else {
            float* dst = (float*)part + ((size_t)i * slices + blockIdx.y) * PW_K;
#pragma unroll
            for (int s = 0; s < PW_K; ++s) dst[s] = l[s];
        }
    } else if (MODE == 1) {
        int* flags = (int*)sm;
#pragma unroll
        for (int p = 0; p < 4; ++p) flags[(ty * 4 + p) * 16 + tx] = hit[p] ? 1 : 0;
        __syncthreads();
        if (t >= PW_T || i >= M) return;
        int h = 0;
        for (int u = 0; u < 16; ++u) h |= flags[t * 16 + u];
        if (slices == 1) ((int*)out)[i] = h;
        else ((int*)part)[(size_t)i * slices + blockIdx.y] = h;
    } else {
        int* counts = (int*)sm;
#pragma unroll
        for (int p = 0; p < 4; ++p) counts[(ty * 4 + p) * 16 + tx] = cnt[p];
        __syncthreads();
        if (t >= PW_T || i >= M) return;
        int h = 0;
        for (int u = 0; u < 16; ++u) h += counts[t * 16 + u];
        if (slices == 1) ((int*)out)[i] = h;
        else ((int*)part)[(size_t)i * slices + blockIdx.y] = h;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void pairwise_merge_kernel(const void* __restrict__ part, int M, int slices, int k, void* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    if (MODE == 0) {
        const float* src = (const float*)part + (size_t)i * slices * PW_K;
        f32x8 l;
#pragma unroll
        for (int s = 0; s < PW_K; ++s) l[s] = INFINITY;
        for (int u = 0; u < slices * PW_K; ++u) pw_insert(l, src[u]);
        ((float*)out)[i] = pw_kth(l, k);
    } else if (MODE == 1) {
        const int* src = (const int*)part + (size_t)i * slices;
        int h = 0;
        for (int u = 0; u < slices; ++u) h |= src[u];
        ((int*)out)[i] = h;
    } else {
        const int* src = (const int*)part + (size_t)i * slices;
        int h = 0;
        for (int u = 0; u < slices; ++u) h += src[u];
        ((int*)out)[i] = h;
    }
}

template <int MODE>
int pw_run(const float* q, int M, int ldq, const float* x, int N, int ldx, int d, int self, const float* r2, int k, void* out, void* scratch,
           hipStream_t s, const char* name) {
    const int slices0 = pw_slices(N, M);
    const int per = tv_cdiv(tv_cdiv(N, slices0), PW_T) * PW_T;
    const int slices = tv_cdiv(N, per);
    TV_CHECK_ARG(slices == 1 || scratch, "%s: M=%d, N=%d cuts the data range into %d slices and needs scratch", name, M, N, slices);
    const bool vec = ((((uintptr_t)q) | ((uintptr_t)x)) & 15) == 0 && ldq % 4 == 0 && ldx % 4 == 0;
    const dim3 grid((unsigned)tv_cdiv(M, PW_T), (unsigned)slices);
    if (vec) hipLaunchKernelGGL((pairwise_kernel<MODE, true>), grid, dim3(256), 0, s, q, M, ldq, x, N, ldx, d, self, r2, per, slices, k, out, scratch);
    else hipLaunchKernelGGL((pairwise_kernel<MODE, false>), grid, dim3(256), 0, s, q, M, ldq, x, N, ldx, d, self, r2, per, slices, k, out, scratch);
    TV_CHECK_LAUNCH(name);
    if (slices > 1) {
        hipLaunchKernelGGL(pairwise_merge_kernel<MODE>, dim3((unsigned)tv_cdiv(M, 256)), dim3(256), 0, s, (const void*)scratch, M, slices, k, out);
        TV_CHECK_LAUNCH(name);
    }
    return TV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// tv_poly_kernel_sums
// ---------------------------------------------------------------------------------------------------------------------
// block (bx, by, s): the pairs (i, j) of subset s with i in [64 by, 64 by + 64), j in [64 bx, 64 bx + 64); row i of the a side is
// a[ia[s m + i]], row j of the b side b[ib[s m + j]].  part: one double per block, subset-major, then by, then bx.
template <bool VEC>
__global__ __launch_bounds__(256) void poly_sums_kernel(const float* __restrict__ a, int lda, const int* __restrict__ ia,
                                                        const float* __restrict__ b, int ldb, const int* __restrict__ ib, int m, int d,
                                                        double gamma, double coef0, int skip, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[2 * PW_SIDE];        // staging first, the 256 thread partials (fp64) afterwards
    static_assert(2 * PW_SIDE * sizeof(float) >= 256 * sizeof(double), "the thread partials fit the staging buffer");
    float* qs = sm;
    float* xs = sm + PW_SIDE;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int lr = t >> 3;
    const int i0 = blockIdx.y * PW_T, j0 = blockIdx.x * PW_T;
    const int* sa = ia + (size_t)blockIdx.z * m;
    const int* sb = ib + (size_t)blockIdx.z * m;
    const float* qrow[2];
    const float* xrow[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = i0 + lr + 32 * s, j = j0 + lr + 32 * s;
        qrow[s] = i < m ? a + (size_t)sa[i] * lda : nullptr;
        xrow[s] = j < m ? b + (size_t)sb[j] * ldb : nullptr;
    }
    float acc[4][4];
    pw_tile<VEC, true>(qrow, xrow, d, qs, xs, acc);
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + ty * 4 + p, j = j0 + tx * 4 + e;
            if (i < m && j < m && !(skip && i == j)) {
                const double v = (double)acc[p][e] * gamma + coef0;
                sum += (v * v) * v;
            }
        }
    __syncthreads();                                    // staging no longer read
    double* red = (double*)sm;
    red[t] = sum;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int u = 0; u < 256; ++u) s += red[u];      // thread order
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void poly_finalise_kernel(const double* __restrict__ part, int per, int S, double* __restrict__ sums) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const double* src = part + (size_t)s * per;
    double v = 0.0;
    for (int u = 0; u < per; ++u) v += src[u];          // block order
    sums[s] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// tv_softmax_stats
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SS_MAXK = 4096;

// scratch: row b at b (K + 1): {sum_k p log p, p[K]}
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ z, int K, int ld, double* __restrict__ scratch) {
    __shared__ double e[SS_MAXK];
    __shared__ float wmax[4];
    __shared__ double bc[1];
    const int t = threadIdx.x;
    const float* row = z + (size_t)blockIdx.x * ld;
    double* dst = scratch + (size_t)blockIdx.x * (K + 1);
    float m = -INFINITY;
    for (int c = t; c < K; c += 256) m = fmaxf(m, row[c]);
    m = tv_wave_max(m);
    if ((t & 63) == 0) wmax[t >> 6] = m;
    __syncthreads();
    const double mx = (double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));   // a maximum: exact in any order
    for (int c = t; c < K; c += 256) e[c] = exp((double)row[c] - mx);
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int c = 0; c < K; ++c) s += e[c];                  // k order
        bc[0] = s;
    }
    __syncthreads();
    const double s = bc[0], ls = log(s);
    for (int c = t; c < K; c += 256) {
        const double p = e[c] / s;
        const double lp = ((double)row[c] - mx) - ls;
        dst[1 + c] = p;
        e[c] = p * lp;                                           // each thread rewrites only the entries it read
    }
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        for (int c = 0; c < K; ++c) a += e[c];                  // k order
        dst[0] = a;
    }
}

// state {rows, S, psum[K]}: entry c + 1 takes row 0, row 1, ... of its scratch column, one at a time
__global__ __launch_bounds__(256) void softmax_state_kernel(const double* __restrict__ scratch, int B, int K, double* __restrict__ state) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > K) return;
    double a = state[1 + c];
    for (int b = 0; b < B; ++b) a += scratch[(size_t)b * (K + 1) + c];
    state[1 + c] = a;
    if (c == 0) state[0] += (double)B;
}

}  // namespace

extern "C" int tv_knn_radius(const float* x, int N, int d, int ldx, int i0, int M, int k, float* r2, float* scratch, void* stream) {
    TV_CHECK_ARG(x && r2, "tv_knn_radius: x and r2 must not be NULL");
    TV_CHECK_ARG(k >= 1 && k <= PW_K, "tv_knn_radius: k=%d must be in [1, %d]", k, PW_K);
    TV_CHECK_ARG(N >= k + 1 && N <= (1 << 30), "tv_knn_radius: N=%d must be in [k + 1 = %d, 2^30]", N, k + 1);
    TV_CHECK_ARG(d >= 1 && d <= 8192, "tv_knn_radius: d=%d must be in [1, 8192]", d);
    TV_CHECK_ARG(ldx >= d, "tv_knn_radius: ldx=%d must be at least d=%d", ldx, d);
    TV_CHECK_ARG(i0 >= 0 && M >= 1 && M <= N - i0, "tv_knn_radius: queries i0=%d .. i0 + M=%d - 1 must lie in [0, N=%d)", i0, M, N);
    return pw_run<0>(x + (size_t)i0 * ldx, M, ldx, x, N, ldx, d, i0, nullptr, k, r2, scratch, (hipStream_t)stream, "tv_knn_radius");
}

extern "C" int tv_manifold_hits(const float* q, int M, int ldq, const float* x, int N, int ldx, const float* r2, int d, int* hit, int* scratch,
                                void* stream) {
    TV_CHECK_ARG(q && x && r2 && hit, "tv_manifold_hits: q, x, r2 and hit must not be NULL");
    TV_CHECK_ARG(M >= 1 && M <= (1 << 30), "tv_manifold_hits: M=%d must be in [1, 2^30]", M);
    TV_CHECK_ARG(N >= 1 && N <= (1 << 30), "tv_manifold_hits: N=%d must be in [1, 2^30]", N);
    TV_CHECK_ARG(d >= 1 && d <= 8192, "tv_manifold_hits: d=%d must be in [1, 8192]", d);
    TV_CHECK_ARG(ldq >= d && ldx >= d, "tv_manifold_hits: ldq=%d and ldx=%d must be at least d=%d", ldq, ldx, d);
    return pw_run<1>(q, M, ldq, x, N, ldx, d, 0, r2, 0, hit, scratch, (hipStream_t)stream, "tv_manifold_hits");
}

extern "C" int tv_ball_counts(const float* q, int M, int ldq, const float* x, int N, int ldx, const float* r2, int d, int radius_of, int* count,
                              int* scratch, void* stream) {
    TV_CHECK_ARG(q && x && r2 && count, "tv_ball_counts: q, x, r2 and count must not be NULL");
    TV_CHECK_ARG(M >= 1 && M <= (1 << 30), "tv_ball_counts: M=%d must be in [1, 2^30]", M);
    TV_CHECK_ARG(N >= 1 && N <= (1 << 30), "tv_ball_counts: N=%d must be in [1, 2^30]", N);
    TV_CHECK_ARG(d >= 1 && d <= 8192, "tv_ball_counts: d=%d must be in [1, 8192]", d);
    TV_CHECK_ARG(ldq >= d && ldx >= d, "tv_ball_counts: ldq=%d and ldx=%d must be at least d=%d", ldq, ldx, d);
    TV_CHECK_ARG(radius_of == 0 || radius_of == 1, "tv_ball_counts: radius_of=%d must be 0 (one radius per data point) or 1 (per query)", radius_of);
    if (radius_of == 0) return pw_run<2>(q, M, ldq, x, N, ldx, d, 0, r2, 0, count, scratch, (hipStream_t)stream, "tv_ball_counts");
    return pw_run<3>(q, M, ldq, x, N, ldx, d, 0, r2, 0, count, scratch, (hipStream_t)stream, "tv_ball_counts");
}

extern "C" long long tv_poly_kernel_scratch_doubles(int m, int S) {
    if (m < 1 || m > (1 << 16) || S < 1 || S > 65535) return -1;
    const long long tiles = tv_cdiv(m, PW_T);
    return tiles * tiles * S;
}

extern "C" int tv_poly_kernel_sums(const float* a, int lda, const int* ia, const float* b, int ldb, const int* ib, int m, int S, int d, double gamma,
                                   double coef0, int skip_equal_position, double* sums, double* scratch, void* stream) {
    TV_CHECK_ARG(a && ia && b && ib && sums && scratch, "tv_poly_kernel_sums: a, ia, b, ib, sums and scratch must not be NULL");
    TV_CHECK_ARG(m >= 1 && m <= (1 << 16), "tv_poly_kernel_sums: m=%d must be in [1, 2^16]", m);
    TV_CHECK_ARG(S >= 1 && S <= 65535, "tv_poly_kernel_sums: S=%d must be in [1, 65535]", S);
    TV_CHECK_ARG(d >= 1 && d <= 8192, "tv_poly_kernel_sums: d=%d must be in [1, 8192]", d);
    TV_CHECK_ARG(lda >= d && ldb >= d, "tv_poly_kernel_sums: lda=%d and ldb=%d must be at least d=%d", lda, ldb, d);
    const int tiles = tv_cdiv(m, PW_T);
    const long long blocks = (long long)tiles * tiles * S;
    TV_CHECK_ARG(blocks < (1 << 24), "tv_poly_kernel_sums: m=%d, S=%d is %lld blocks; at most 2^24 - 1 per launch", m, S, blocks);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0 && lda % 4 == 0 && ldb % 4 == 0;
    const dim3 grid((unsigned)tiles, (unsigned)tiles, (unsigned)S);
    const int skip = skip_equal_position ? 1 : 0;
    if (vec) hipLaunchKernelGGL(poly_sums_kernel<true>, grid, dim3(256), 0, s, a, lda, ia, b, ldb, ib, m, d, gamma, coef0, skip, scratch);
    else hipLaunchKernelGGL(poly_sums_kernel<false>, grid, dim3(256), 0, s, a, lda, ia, b, ldb, ib, m, d, gamma, coef0, skip, scratch);
    TV_CHECK_LAUNCH("tv_poly_kernel_sums");
    hipLaunchKernelGGL(poly_finalise_kernel, dim3((unsigned)tv_cdiv(S, 256)), dim3(256), 0, s, (const double*)scratch, tiles * tiles, S, sums);
    TV_CHECK_LAUNCH("tv_poly_kernel_sums (finalise)");
    return TV_OK;
}

extern "C" int tv_softmax_stats(const float* logits, int B, int K, int ld, double* state, double* scratch, void* stream) {
    TV_CHECK_ARG(logits && state && scratch, "tv_softmax_stats: logits, state and scratch must not be NULL");
    TV_CHECK_ARG(B >= 1, "tv_softmax_stats: B=%d must be positive", B);
    TV_CHECK_ARG(K >= 1 && K <= SS_MAXK, "tv_softmax_stats: K=%d must be in [1, %d]", K, SS_MAXK);
    TV_CHECK_ARG(ld >= K, "tv_softmax_stats: ld=%d must be at least K=%d", ld, K);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)B), dim3(256), 0, s, logits, K, ld, scratch);
    TV_CHECK_LAUNCH("tv_softmax_stats (rows)");
    hipLaunchKernelGGL(softmax_state_kernel, dim3((unsigned)tv_cdiv(K + 1, 256)), dim3(256), 0, s, (const double*)scratch, B, K, state);
    TV_CHECK_LAUNCH("tv_softmax_stats (state)");
    return TV_OK;
}
