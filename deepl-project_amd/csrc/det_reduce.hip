// Fixed-order slice reduce: the second launch of every deterministic parameter-gradient path.
//
//     S[i]   = fl(...fl(fl(P_0[i] + P_1[i]) + P_2[i])... + P_{n_slices-1}[i]),      P_s = part + s * slice_stride
//     out[i] = accum ? fl(out[i] + S[i]) : S[i]
//
// The contributors (split-K chunks of the weight-gradient kernels, blocks of the row-norm backward) store their partial
// results with plain vector stores into a slice each; here one thread owns four consecutive elements and walks the slices in
// ascending index, so the association order is the formula above whatever the grid, the hardware queue or the run.  No atomics.
// A bandwidth kernel: n_slices x n floats in, n out, 16-byte loads (the slices of one element are slice_stride apart, the
// lanes of a wave read 1 KiB runs).  Pointers off the 16-byte grid or strides off the 4-element grid take the scalar form,
// one element per thread; the last n % 4 elements of the vector form are scalar too.
#include "common.h"

namespace {

template <bool VEC>
__global__ __launch_bounds__(256) void reduce_slices_kernel(const float* __restrict__ part, int n_slices, long long n, long long slice_stride,
                                                            float* out, int accum) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        const long long n4 = n >> 2;
        if (t < n4) {
            const f32x4* p = (const f32x4*)part + t;
            f32x4 s = *p;
            for (int k = 1; k < n_slices; ++k) {
                p += slice_stride >> 2;
                s += *p;
            }
            f32x4* o = (f32x4*)out + t;
            if (accum) s = *o + s;
            *o = s;
            return;
        }
        const long long i = n4 * 4 + (t - n4);      // the n % 4 tail: one thread per element
        if (i >= n) return;
        const float* p = part + i;
        float s = *p;
        for (int k = 1; k < n_slices; ++k) {
            p += slice_stride;
            s += *p;
        }
        out[i] = accum ? out[i] + s : s;
    } else {
        if (t >= n) return;
        const float* p = part + t;
        float s = *p;
        for (int k = 1; k < n_slices; ++k) {
            p += slice_stride;
            s += *p;
        }
        out[t] = accum ? out[t] + s : s;
    }
}

}  // namespace

// (shared by wgrad_tn.hip and norm.hip: arguments are checked, no tv_init -- the callers have made it)
int tv_reduce_slices_launch(const float* part, int n_slices, long long n, long long slice_stride, float* out, int accum, hipStream_t s) {
    const bool vec = (((uintptr_t)part | (uintptr_t)out) & 15) == 0 && (slice_stride & 3) == 0 && n >= 4;
    if (vec) {
        const long long threads = (n >> 2) + (n & 3);
        hipLaunchKernelGGL(reduce_slices_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, part, n_slices, n, slice_stride, out, accum);
    } else {
        hipLaunchKernelGGL(reduce_slices_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, n_slices, n, slice_stride, out, accum);
    }
    return 0;
}

extern "C" int tv_reduce_slices(const float* part, int n_slices, long long n, long long slice_stride, float* out, int accum, void* stream) {
    TV_CHECK_ARG(part && out, "tv_reduce_slices: null pointer");
    TV_CHECK_ARG(n_slices >= 1 && n >= 1 && n < (1ll << 40), "tv_reduce_slices: n_slices=%d n=%lld", n_slices, n);
    TV_CHECK_ARG(slice_stride >= n || n_slices == 1, "tv_reduce_slices: slice_stride=%lld is below n=%lld (slices would overlap)", slice_stride, n);
    TV_CHECK_ARG(accum == 0 || accum == 1, "tv_reduce_slices: accum=%d", accum);
    if (tv_init() != TV_OK) return TV_ERR_INIT;
    tv_reduce_slices_launch(part, n_slices, n, slice_stride, out, accum, (hipStream_t)stream);
    TV_CHECK_LAUNCH("tv_reduce_slices");
    return TV_OK;
}
