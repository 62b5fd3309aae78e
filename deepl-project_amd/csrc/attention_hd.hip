// The head_dim 72 kernel family (DiT-XL / LightningDiT-XL: 1152 = 16 heads of 72): flash attention forward and backward, the
// in-place RoPE.  The qk-norm pair of this head_dim (tv_qknorm_rope_fwd_hd / _bwd_hd) is qk_norm.hip, one template with head_dim 64's;
// its summation orders are stated there and below.  A first, sound form: plain LDS staging between two __syncthreads per tile, no DMA ring.
// DESIGN.md section 3.1 row Y holds the rounding contract; tv_*_hd in include/transvae_hip.h are the entries.
//
// Data: qkv [B, N, 3, heads, 72] bf16, o [B, N, heads, 72] bf16, lse [B, heads, N] fp32 (natural log), delta [2, B, heads, N] fp32
// scratch (-delta, then -lse log2(e)), RoPE table [N, 4, 36] fp32 = cos1, sin1, cos2, sin2 of the 36 pairs.  A head vector is
// 144 bytes = nine 16-byte pieces; every global load and store is one whole piece (or 8 bytes of one) of the head vector, token
// row or statistics row it belongs to, and nothing is loaded in order to be masked.
//
// The padding rule.  v_mfma_f32_32x32x16_bf16 sums q.k over 80 = 5 k-steps and writes P V over 96 = 3 row tiles.  The pads exist
// in registers and LDS only and are zeros by construction:
//   * the fragment of k-step 4 held in registers (q, dO, k, v on the lane) is piece 8 in lane half 0 and the constant 0 in half 1;
//   * a row-major LDS tile is [64][80]: pieces 0..8 of a row are staged, piece 9 (d 72..79) is written 0 once, before the loop;
//   * a transposed LDS tile is [96][72] (d, then 64 rows + 8 columns that are never read): rows d = 72..95 are written 0 once;
//   * rows of a tile past N are staged as zeros without a load; a key past N gets the score -inf, hence p = 0 exactly; results
//     of queries (keys, for dk / dv) past N and of d >= 72 are not stored.
//
// Forward policy (attn_fwd_emul of the tests, its parameters unchanged): block = 4 waves x 32 queries, query on the MFMA lane;
// key blocks of 64; S^T = K Q^T in fp32 from bf16; a wave rescales its running (m, l, O) only when some row's block maximum
// exceeds m by more than 8 in log2 units; p = exp2(s c2 - m c2) in fp32, c2 = scale log2(e); l sums the fp32 p (each lane half
// its 32 keys of a block in register order, the halves added once after the loop); P is rounded to bf16 once, as the B operand
// of O^T = V^T P^T; O in fp32; o = bf16(O / l); lse = (m c2 + log2 l) ln 2.
//
// Backward policy (row A's, attn_bwd_emul of the tests): delta = sum_d dO o in fp32; P = exp2(s c2 - lse log2(e)) in fp32 with S
// recomputed; dS = P (dP - delta) rounded to bf16 for dq and dk, P rounded to bf16 for dv; fp32 sums; `scale` applied to the fp32
// sum; with a table the adjoint a' = ga c1 + gb s2, b' = -ga s1 + gb c2 is applied to the scaled fp32 sums in the store; every
// output rounded once.  dv and delta do not see the table.  Three kernels, no atomics, the same bits on every run:
//   delta  one thread per (token, head)
//   dq     block = 4 waves x 32 queries (query on the lane), key blocks of 64: K by rows and transposed, V by rows
//   dk/dv  block = 4 waves x 32 keys (key on the lane), query blocks of 64: Q and dO by rows and transposed, -lse and -delta rows
//
// Order of every sum of 72 terms outside the MFMAs:
//   delta        per piece a chain of 8 FMAs from 0 (d ascending), then the nine piece sums added in piece order: 8 + 8 roundings
//   qk-norm      a 16-lane group holds one head vector, lanes 0..8 one piece each, lanes 9..15 the constant 0 (no load): per lane
//                a chain of 8 FMAs from 0, then the xor butterfly over lane distances 1, 2, 4, 8: 8 + 4 roundings; the mean is the
//                sum times fp32(1 / 72) (one more rounding).  Used for mean(q^2) and mean(g qh) alike.
//   dwq / dwk    per lane group its vectors in pass order, the 16 groups of a block in order, block k in lane k % 64 in order,
//                the 64 lanes in order; fixed-order partials in scratch, no atomics.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int HD = 72;        // head_dim
constexpr int HP = 9;         // 16-byte pieces of a head vector
constexpr int ROWP = 80;      // elements per row of a row-major LDS tile (piece 9 = zeros)
constexpr int TRP = 72;       // elements per row of a transposed LDS tile: 64 rows of the source + 8 never read
constexpr int TRROWS = 96;    // d rows of a transposed tile (72..95 = zeros)
constexpr int KBLK = 64;      // keys (queries, for dk / dv) per staged block
constexpr float LAZY = 8.f;   // forward: rescale when a row's maximum grew by more than this (log2 units)
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

struct AttnHdArgs {
    const bf16* qkv;
    const bf16* o;
    const bf16* d_o;
    bf16* out;           // fwd: o ; bwd: dqkv
    float* lse;
    float* delta;
    const float* rope;   // backward only: table [N][4][36]
    int B, N, heads;
    float scale;
};

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bf16x8 zero8() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ float xhalf(float x) { return __shfl_xor(x, 32, 64); }

// registers 8s..8s+7 of an accumulator tile -> bf16 fragment (B operand of the next MFMA): element j of lane half h is row
// 16s + 8(j>>2) + 4h + (j&3) of the tile
__device__ __forceinline__ bf16x8 pack_acc(const f32x16& a, int s) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (bf16)a[8 * s + j];
    return r;
}

// block -> (sequence tile of 128 rows, head, image)
__device__ __forceinline__ void attn_block(const AttnHdArgs& p, int& tile, int& head, int& b) {
    const int tiles = (p.N + 127) / 128;
    const int lin = blockIdx.x;
    tile = lin % tiles;
    const int hb = lin / tiles;
    head = hb % p.heads;
    b = hb / p.heads;
}

// the zeros of the pads, written once before a kernel's loop (its first barrier publishes them; staging never touches them)
__device__ __forceinline__ void zero_row_pad(bf16* tile) {
    for (int r = threadIdx.x; r < KBLK; r += 256) *(bf16x8*)(tile + r * ROWP + HD) = zero8();
}
__device__ __forceinline__ void zero_tr_pad(bf16* tile) {
    for (int i = threadIdx.x; i < (TRROWS - HD) * TRP / 8; i += 256) *(bf16x8*)(tile + HD * TRP + i * 8) = zero8();
}

// rows row0 .. row0+63 of the head slice at `base` (row pitch ld elements) -> rows[64][ROWP] and / or tr[d][row]; rows >= nrows
// are zeros (no load)
template <bool ROWS, bool TR>
__device__ __forceinline__ void stage(bf16* rows, bf16* tr, const bf16* base, size_t ld, int row0, int nrows) {
    for (int i = threadIdx.x; i < KBLK * HP; i += 256) {
        const int r = TR ? (i & 63) : (i / HP), pc = TR ? (i >> 6) : (i - r * HP);
        bf16x8 v = zero8();
        if (row0 + r < nrows) v = *(const bf16x8*)(base + (size_t)(row0 + r) * ld + pc * 8);
        if (ROWS) *(bf16x8*)(rows + r * ROWP + pc * 8) = v;
        if (TR) {
#pragma unroll
            for (int e = 0; e < 8; ++e) tr[(pc * 8 + e) * TRP + r] = v[e];
        }
    }
}

// the five k-step fragments of a head vector held on the lane (row = lane & 31, lane half h): piece 2 st + h, piece 9 = 0
__device__ __forceinline__ void load_frags(bf16x8 (&f)[5], const bf16* vec, bool ok, int h) {
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        bf16x8 v = zero8();
        if (ok && 2 * st + h < HP) v = *(const bf16x8*)(vec + (2 * st + h) * 8);
        f[st] = v;
    }
}
// A operand by rows: row (lane & 31) of the 32-row tile at `tile`, k-step st
__device__ __forceinline__ bf16x8 read_rows(const bf16* tile, int lane, int st) {
    return *(const bf16x8*)(tile + (lane & 31) * ROWP + st * 16 + (lane >> 5) * 8);
}
// A operand = transposed tile: row d = 32 db + (lane & 31), k = source rows c0 + 16 ss + 8(j>>2) + 4h + (j&3) (pack_acc's k order)
__device__ __forceinline__ bf16x8 read_tr(const bf16* tr, int lane, int db, int c0) {
    const bf16* ptr = tr + (db * 32 + (lane & 31)) * TRP + c0 + 4 * (lane >> 5);
    const bf16x4 lo = *(const bf16x4*)ptr, hi = *(const bf16x4*)(ptr + 8);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// adjoint of the reference's (non-orthogonal) RoPE 2x2 on channels ch0 .. ch0+3 of a head (two pairs); tab_row [4][36]
__device__ __forceinline__ void rope_adjoint4(float (&v)[4], const float* tab_row, int ch0) {
    const float* tb = tab_row + (ch0 >> 1);
    const float c1a = tb[0], c1b = tb[1], s1a = tb[36], s1b = tb[37], c2a = tb[72], c2b = tb[73], s2a = tb[108], s2b = tb[109];
    const float a0 = v[0], b0 = v[1], a1 = v[2], b1 = v[3];
    v[0] = a0 * c1a + b0 * s2a;
    v[1] = -a0 * s1a + b0 * c2a;
    v[2] = a1 * c1b + b1 * s2b;
    v[3] = -a1 * s1b + b1 * c2b;
}

// accumulator tiles t[3] hold rows d = 32 db + (r&3) + 8(r>>2) + 4h of the lane's column: store d < 72 as bf16(f(t)), 8 bytes a time
template <class F>
__device__ __forceinline__ void store_cols(bf16* row, const f32x16 (&t)[3], int h, F&& f) {
#pragma unroll
    for (int db = 0; db < 3; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (db == 2 && g > 0) continue;   // d >= 72: pad rows of the third tile
            const int d0 = db * 32 + 8 * g + 4 * h;
            float x[4] = {t[db][4 * g], t[db][4 * g + 1], t[db][4 * g + 2], t[db][4 * g + 3]};
            f(x, d0);
            *(bf16x4*)(row + d0) = bf16x4{(bf16)x[0], (bf16)x[1], (bf16)x[2], (bf16)x[3]};
        }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn72_fwd_kernel(const AttnHdArgs p) {
    __shared__ __attribute__((aligned(16))) bf16 sK[KBLK * ROWP];
    __shared__ __attribute__((aligned(16))) bf16 sVt[TRROWS * TRP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    int tile, head, b;
    attn_block(p, tile, head, b);
    const int C = p.heads * HD;
    const size_t ld = (size_t)3 * C;
    const bf16* qbase = p.qkv + (size_t)b * p.N * ld + head * HD;
    const bf16* kbase = qbase + C;
    const bf16* vbase = qbase + 2 * C;
    const int qi = tile * 128 + wave * 32 + (lane & 31);
    const bool q_ok = qi < p.N;
    bf16x8 qf[5];
    load_frags(qf, qbase + (size_t)(q_ok ? qi : 0) * ld, q_ok, h);
    f32x16 ot[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) ot[0][i] = ot[1][i] = ot[2][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float c2 = p.scale * LOG2E;
    const int nblk = (p.N + KBLK - 1) / KBLK;
    zero_row_pad(sK);
    zero_tr_pad(sVt);
    for (int t = 0; t < nblk; ++t) {
        __syncthreads();                                   // the previous block's fragment reads are done
        stage<true, false>(sK, nullptr, kbase, ld, t * KBLK, p.N);
        stage<false, true>(nullptr, sVt, vbase, ld, t * KBLK, p.N);
        __syncthreads();
        f32x16 s[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[0][i] = s[1][i] = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int st = 0; st < 5; ++st) s[kt] = mfma32(read_rows(sK + kt * 32 * ROWP, lane, st), qf[st], s[kt]);
        const int kv0 = t * KBLK;
        if (kv0 + KBLK > p.N) {   // the ragged last block: keys >= N take no part (block-uniform branch)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kv0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= p.N) s[kt][r] = -INFINITY;
        }
        float mloc = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[kt][r]);
        mloc = fmaxf(mloc, xhalf(mloc));
        if (__any((mloc - m) * c2 > LAZY)) {   // (wave-uniform; the first block always: m = -inf)
            const float mnew = fmaxf(m, mloc);
            const float alpha = __builtin_amdgcn_exp2f((m - mnew) * c2);
            m = mnew;
            l *= alpha;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                ot[0][i] *= alpha;
                ot[1][i] *= alpha;
                ot[2][i] *= alpha;
            }
        }
        const float mc = m * c2;
        float rs = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c2, -mc));
                s[kt][r] = pv;
                rs += pv;
            }
        l += rs;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 pf = pack_acc(s[kt], ss);
#pragma unroll
                for (int db = 0; db < 3; ++db) ot[db] = mfma32(read_tr(sVt, lane, db, kt * 32 + 16 * ss), pf, ot[db]);
            }
    }
    l += xhalf(l);
    if (q_ok) {
        const float inv = 1.0f / l;
        store_cols(p.out + ((size_t)b * p.N + qi) * C + head * HD, ot, h, [&](float (&x)[4], int) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] *= inv;
        });
        if (h == 0) p.lse[((size_t)b * p.heads + head) * p.N + qi] = (m * c2 + __log2f(l)) * LN2;
    }
}

// ------------------------------------------------------------------------------------------------
// delta[b][head][q] = -sum_d dO[q][d] O[q][d], and -lse log2(e) in the second plane
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn72_delta_kernel(const AttnHdArgs p) {
    const long long total = (long long)p.B * p.N * p.heads;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int head = (int)(idx % p.heads);
        const long long tok = idx / p.heads;  // b*N + n
        const size_t off = (size_t)idx * HD;
        float acc = 0.f;
#pragma unroll
        for (int pc = 0; pc < HP; ++pc) {
            const bf16x8 a = *(const bf16x8*)(p.o + off + pc * 8);
            const bf16x8 g = *(const bf16x8*)(p.d_o + off + pc * 8);
            float part = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) part = fmaf((float)a[e], (float)g[e], part);
            acc = pc == 0 ? part : acc + part;
        }
        const long long bb = tok / p.N;
        const int n = (int)(tok - bb * p.N);
        const size_t at = ((size_t)bb * p.heads + head) * p.N + n;
        p.delta[at] = -acc;
        p.delta[(size_t)p.B * p.heads * p.N + at] = -p.lse[at] * LOG2E;
    }
}

// ------------------------------------------------------------------------------------------------
// dq:  dS^T = P^T o (dP^T - delta),  dQ^T = K^T dS^T
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn72_bwd_dq_kernel(const AttnHdArgs p) {
    __shared__ __attribute__((aligned(16))) bf16 sK[KBLK * ROWP];
    __shared__ __attribute__((aligned(16))) bf16 sV[KBLK * ROWP];
    __shared__ __attribute__((aligned(16))) bf16 sKt[TRROWS * TRP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    int tile, head, b;
    attn_block(p, tile, head, b);
    const int C = p.heads * HD;
    const size_t ld = (size_t)3 * C;
    const bf16* qbase = p.qkv + (size_t)b * p.N * ld + head * HD;
    const bf16* kbase = qbase + C;
    const bf16* vbase = qbase + 2 * C;
    const int qi = tile * 128 + wave * 32 + (lane & 31);
    const bool q_ok = qi < p.N;
    const size_t qrow = q_ok ? qi : 0;
    bf16x8 qf[5], gf[5];
    load_frags(qf, qbase + qrow * ld, q_ok, h);
    load_frags(gf, p.d_o + ((size_t)b * p.N + qrow) * C + head * HD, q_ok, h);
    float nl = 0.f, nd = 0.f;   // -lse log2(e), -delta (a query past N: q = dO = 0, P = 1, dS = 0)
    if (q_ok) {
        const size_t at = ((size_t)b * p.heads + head) * p.N + qi;
        nd = p.delta[at];
        nl = p.delta[(size_t)p.B * p.heads * p.N + at];
    }
    const float c2 = p.scale * LOG2E;
    f32x16 dqt[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) dqt[0][i] = dqt[1][i] = dqt[2][i] = 0.f;
    const int nblk = (p.N + KBLK - 1) / KBLK;
    zero_row_pad(sK);
    zero_row_pad(sV);
    zero_tr_pad(sKt);
    for (int t = 0; t < nblk; ++t) {
        __syncthreads();
        stage<true, true>(sK, sKt, kbase, ld, t * KBLK, p.N);
        stage<true, false>(sV, nullptr, vbase, ld, t * KBLK, p.N);
        __syncthreads();
        const int kv0 = t * KBLK;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
            for (int st = 0; st < 5; ++st) {
                s = mfma32(read_rows(sK + kt * 32 * ROWP, lane, st), qf[st], s);
                dp = mfma32(read_rows(sV + kt * 32 * ROWP, lane, st), gf[st], dp);
            }
            if (kv0 + KBLK > p.N) {   // keys >= N: P = 0 (their V rows are zeros: dP is finite)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kv0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= p.N) s[r] = -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, nl)) * (dp[r] + nd);   // dS^T without `scale`
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 df = pack_acc(s, ss);
#pragma unroll
                for (int db = 0; db < 3; ++db) dqt[db] = mfma32(read_tr(sKt, lane, db, kt * 32 + 16 * ss), df, dqt[db]);
            }
        }
    }
    if (q_ok) {
        const float* tab_row = p.rope ? p.rope + (size_t)qi * (2 * HD) : nullptr;
        store_cols(p.out + ((size_t)b * p.N + qi) * ld + head * HD, dqt, h, [&](float (&x)[4], int d0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] *= p.scale;
            if (tab_row) rope_adjoint4(x, tab_row, d0);
        });
    }
}

// ------------------------------------------------------------------------------------------------
// dk / dv: key on the lane.  S = Q K^T, dP = dO V^T (query on the accumulator row); dV^T = dO^T P, dK^T = Q^T dS
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn72_bwd_dkv_kernel(const AttnHdArgs p) {
    __shared__ __attribute__((aligned(16))) bf16 sQ[KBLK * ROWP];
    __shared__ __attribute__((aligned(16))) bf16 sG[KBLK * ROWP];
    __shared__ __attribute__((aligned(16))) bf16 sQt[TRROWS * TRP];
    __shared__ __attribute__((aligned(16))) bf16 sGt[TRROWS * TRP];
    __shared__ __attribute__((aligned(16))) float sNl[KBLK];
    __shared__ __attribute__((aligned(16))) float sNd[KBLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    int tile, head, b;
    attn_block(p, tile, head, b);
    const int C = p.heads * HD;
    const size_t ld = (size_t)3 * C;
    const bf16* qbase = p.qkv + (size_t)b * p.N * ld + head * HD;
    const bf16* kbase = qbase + C;
    const bf16* vbase = qbase + 2 * C;
    const bf16* gbase = p.d_o + (size_t)b * p.N * C + head * HD;
    const float* del_b = p.delta + ((size_t)b * p.heads + head) * p.N;   // -delta
    const float* lse_b = del_b + (size_t)p.B * p.heads * p.N;            // -lse log2(e)
    const int ki = tile * 128 + wave * 32 + (lane & 31);
    const bool k_ok = ki < p.N;
    const size_t krow = k_ok ? ki : 0;
    bf16x8 kf[5], vf[5];
    load_frags(kf, kbase + krow * ld, k_ok, h);
    load_frags(vf, vbase + krow * ld, k_ok, h);
    f32x16 dkt[3], dvt[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) dkt[0][i] = dkt[1][i] = dkt[2][i] = dvt[0][i] = dvt[1][i] = dvt[2][i] = 0.f;
    const float c2 = p.scale * LOG2E;
    const int nblk = (p.N + KBLK - 1) / KBLK;
    zero_row_pad(sQ);
    zero_row_pad(sG);
    zero_tr_pad(sQt);
    zero_tr_pad(sGt);
    for (int t = 0; t < nblk; ++t) {
        __syncthreads();
        stage<true, true>(sQ, sQt, qbase, ld, t * KBLK, p.N);
        stage<true, true>(sG, sGt, gbase, (size_t)C, t * KBLK, p.N);
        if (threadIdx.x < 2 * KBLK) {   // a query past N: Q = dO = 0 and lse = delta = 0, so P = 1, dS = 0 and dO^T P adds 0
            const int r = threadIdx.x & (KBLK - 1), q = t * KBLK + r;
            const bool second = threadIdx.x >= KBLK;
            const float v = q < p.N ? (second ? del_b[q] : lse_b[q]) : 0.f;
            (second ? sNd : sNl)[r] = v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (t * KBLK + u * 32 >= p.N) continue;   // (block-uniform) a tile of queries past N adds nothing
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
            for (int st = 0; st < 5; ++st) {
                s = mfma32(read_rows(sQ + u * 32 * ROWP, lane, st), kf[st], s);
                dp = mfma32(read_rows(sG + u * 32 * ROWP, lane, st), vf[st], dp);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // accumulator rows (queries) 8g + 4h + {0..3}
                const f32x4 nl = *(const f32x4*)(sNl + u * 32 + 8 * g + 4 * h), nd = *(const f32x4*)(sNd + u * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(s[4 * g + e], c2, nl[e]));
                    s[4 * g + e] = pv;
                    dp[4 * g + e] = pv * (dp[4 * g + e] + nd[e]);
                }
            }
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 pf = pack_acc(s, ss), df = pack_acc(dp, ss);
#pragma unroll
                for (int db = 0; db < 3; ++db) {
                    dvt[db] = mfma32(read_tr(sGt, lane, db, u * 32 + 16 * ss), pf, dvt[db]);
                    dkt[db] = mfma32(read_tr(sQt, lane, db, u * 32 + 16 * ss), df, dkt[db]);
                }
            }
        }
    }
    if (k_ok) {
        bf16* krow_out = p.out + ((size_t)b * p.N + ki) * ld + C + head * HD;
        const float* tab_row = p.rope ? p.rope + (size_t)ki * (2 * HD) : nullptr;
        store_cols(krow_out, dkt, h, [&](float (&x)[4], int d0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] *= p.scale;
            if (tab_row) rope_adjoint4(x, tab_row, d0);
        });
        store_cols(krow_out + C, dvt, h, [](float (&)[4], int) {});
    }
}

// ---- RoPE in place on the q and k thirds; tab [N][4][36]: one thread per 16-byte piece (pairs 4v .. 4v+3) ---------------------
__global__ __launch_bounds__(256) void rope_qk72_kernel(bf16* __restrict__ qkv, const float* __restrict__ tab, long long total, int N, int heads,
                                                        int transpose) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        long long r = idx;
        const int v = (int)(r % HP);
        r /= HP;
        const int head = (int)(r % heads);
        r /= heads;
        const int which = (int)(r & 1);
        r >>= 1;
        const int n = (int)(r % N);
        const long long b = r / N;
        bf16* ptr = qkv + ((((size_t)b * N + n) * 3 + which) * heads + head) * HD + v * 8;
        const bf16x8 t = *(const bf16x8*)ptr;
        const float* tb = tab + (size_t)n * (2 * HD) + v * 4;
        const f32x4 c1 = *(const f32x4*)(tb), s1 = *(const f32x4*)(tb + 36), c2 = *(const f32x4*)(tb + 72), s2 = *(const f32x4*)(tb + 108);
        bf16x8 o;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float a = (float)t[2 * p], bb = (float)t[2 * p + 1];
            float o1, o2;
            if (!transpose) {
                o1 = a * c1[p] - bb * s1[p];
                o2 = a * s2[p] + bb * c2[p];
            } else {  // adjoint of the (non-orthogonal) 2x2
                o1 = a * c1[p] + bb * s2[p];
                o2 = -a * s1[p] + bb * c2[p];
            }
            o[2 * p] = (bf16)o1;
            o[2 * p + 1] = (bf16)o2;
        }
        *(bf16x8*)ptr = o;
    }
}

int hd_check(const char* name, int B, int N, int heads, int head_dim) {
    if (head_dim != HD) {
        tv_set_error("%s: head_dim=%d is not supported (72 only; head_dim 64 has its own entries)", name, head_dim);
        return TV_ERR_ARG;
    }
    if (B <= 0 || N <= 0 || heads <= 0 || (long long)B * N >= (1ll << 31) || (long long)B * N * 3 * heads >= (1ll << 31)) {
        tv_set_error("%s: bad shape B=%d N=%d heads=%d (positive, B N 3 heads < 2^31)", name, B, N, heads);
        return TV_ERR_ARG;
    }
    return TV_OK;
}

unsigned attn_grid(int B, int N, int heads) { return (unsigned)((long long)tv_cdiv(N, 128) * heads * B); }

}  // namespace

extern "C" int tv_attn_fwd_hd(const void* qkv, void* o, float* lse, int B, int N, int heads, int head_dim, float scale, void* stream) {
    if (int rc = hd_check("tv_attn_fwd_hd", B, N, heads, head_dim)) return rc;
    TV_CHECK_ARG(scale > 0.f, "tv_attn_fwd_hd: scale=%g must be positive", (double)scale);
    TV_CHECK_ARG(qkv && o && lse, "tv_attn_fwd_hd: null pointer");
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)o) & 15) == 0, "tv_attn_fwd_hd: qkv / o must be 16-byte aligned");
    if (tv_init() != TV_OK) return TV_ERR_INIT;
    AttnHdArgs a{};
    a.qkv = (const bf16*)qkv; a.out = (bf16*)o; a.lse = lse;
    a.B = B; a.N = N; a.heads = heads; a.scale = scale;
    hipLaunchKernelGGL(attn72_fwd_kernel, dim3(attn_grid(B, N, heads)), dim3(256), 0, (hipStream_t)stream, a);
    TV_CHECK_LAUNCH("tv_attn_fwd_hd");
    return TV_OK;
}

extern "C" int tv_attn_bwd_hd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, const float* rope_tab, void* dqkv, int B,
                              int N, int heads, int head_dim, float scale, void* stream) {
    if (int rc = hd_check("tv_attn_bwd_hd", B, N, heads, head_dim)) return rc;
    TV_CHECK_ARG(scale > 0.f, "tv_attn_bwd_hd: scale=%g must be positive", (double)scale);
    TV_CHECK_ARG(qkv && o && d_o && lse && delta && dqkv, "tv_attn_bwd_hd: null pointer");
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dqkv) & 15) == 0, "tv_attn_bwd_hd: qkv / o / d_o / dqkv must be 16-byte aligned");
    if (tv_init() != TV_OK) return TV_ERR_INIT;
    AttnHdArgs a{};
    a.qkv = (const bf16*)qkv; a.o = (const bf16*)o; a.d_o = (const bf16*)d_o; a.out = (bf16*)dqkv;
    a.lse = const_cast<float*>(lse); a.delta = delta; a.rope = rope_tab;
    a.B = B; a.N = N; a.heads = heads; a.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    long long g = ((long long)B * N * heads + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(attn72_delta_kernel, dim3((unsigned)g), dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn72_bwd_dq_kernel, dim3(attn_grid(B, N, heads)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn72_bwd_dkv_kernel, dim3(attn_grid(B, N, heads)), dim3(256), 0, s, a);
    TV_CHECK_LAUNCH("tv_attn_bwd_hd");
    return TV_OK;
}

extern "C" int tv_rope_qk_hd(void* qkv, const float* tab, int B, int N, int heads, int head_dim, int transpose, void* stream) {
    if (int rc = hd_check("tv_rope_qk_hd", B, N, heads, head_dim)) return rc;
    TV_CHECK_ARG(qkv && tab, "tv_rope_qk_hd: null pointer");
    TV_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)tab) & 15) == 0, "tv_rope_qk_hd: qkv / tab must be 16-byte aligned");
    const long long total = (long long)B * N * 2 * heads * HP;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(rope_qk72_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (bf16*)qkv, tab, total, N, heads,
                       transpose);
    TV_CHECK_LAUNCH("tv_rope_qk_hd");
    return TV_OK;
}
