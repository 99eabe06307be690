// train_flow.h -- what the conditional flow's kernels share: the training forward and backward (train_kernels.hip) and the
// posterior sampler, the flow's inverse (train_sample.hip).  The parameter block of a flow as the kernels receive it, the
// activation, the LDS-only barrier and the sized raw buffer that drops stores past a tile's valid rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nddm_train {

constexpr int H = 128;        // hidden width

__device__ __forceinline__ float elu(float v) { return v > 0.0f ? v : expm1f(v); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// A barrier that orders LDS traffic only.  __syncthreads() also waits for every global load and store the thread has in flight
// -- which is exactly what the forward's weight prefetch must not do: its loads are issued a half-layer ahead and nothing in
// this kernel reads global memory that the kernel wrote.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The rows [r0, r0 + rows) of a row-major global array as a RAW BUFFER of just their size: a store to a row beyond them (the rows of
// a tile past R) is dropped by the hardware's range check -- the `if (r0 + r < R)` around every one of a phase's stores compiled
// to a branch, an exec save / restore and a 64-bit address each.
struct RowBuf {
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ RowBuf(float *first_row, int rows, int ld)
        : r(__builtin_amdgcn_make_buffer_rsrc(first_row, 0, (rows > 0 ? rows : 0) * ld * 4, 0x00020000)) {}
    __device__ __forceinline__ void put(int off_floats, float v) const
    { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, off_floats * 4, 0, 0); }
};

constexpr int L_MAX = 8, D_MAX = 8;
struct HalfP { const float *W1, *b1, *W2, *b2, *W3, *b3; };
struct LayerP { const float *scale, *bias; HalfP a, b; };
struct FlowP { LayerP layer[L_MAX]; unsigned char perm[L_MAX][D_MAX]; };

/* params: L x 14 device pointers per layer -- ActNorm log-scale [D] and bias [D], then W1 [H, Dh + C], b1 [H], W2 [H, H], b2 [H],
 * W3 [2 Dt, H], b3 [2 Dt] of sub-network 1 (conditioned on the first d1 columns) and of sub-network 2; perm: L x D host ints. */
static inline void fill(FlowP &P, int L, int D, const void *const *params, const int *perm)
{
    for (int l = 0; l < L; ++l) {
        const float *const *q = reinterpret_cast<const float *const *>(params) + 14 * l;
        P.layer[l] = {q[0], q[1], {q[2], q[3], q[4], q[5], q[6], q[7]}, {q[8], q[9], q[10], q[11], q[12], q[13]}};
        for (int d = 0; d < D; ++d) P.perm[l][d] = (unsigned char)perm[l * D + d];
    }
}

}  // namespace nddm_train
