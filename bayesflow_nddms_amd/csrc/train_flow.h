// train_flow.h -- the vocabulary of the conditional flow's kernels: the training forward and backward (train_kernels.hip) and the
// posterior sampler, the flow's inverse (train_sample.hip).  The parameter block of a flow as the kernels receive it, a
// half-layer's shape, and every step that more than one kernel takes: the activation and its gradient, the soft clamp, the LDS-only
// barrier, the sized raw buffer that drops stores past a tile's valid rows, the k-block permutation, the 128-long MFMA dot
// and the two MFMA epilogues.  What occurs once stays in its kernel -- and so does each kernel's weight prefetch, a literal macro:
// written as shared helpers it cost the forward code and time (see train_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nddm_train {

constexpr int H = 128;        // hidden width
constexpr int LDR = H + 4;    // row stride of the [row][unit] tiles and of W2 in LDS: 16-byte aligned rows whose operand reads
                              // (16 rows x 4 column groups per wave instruction) spread evenly over the banks
constexpr int DI_MAX = 32;    // inputs of a sub-network (x_h columns + condition columns)
constexpr int M_MAX = 16;     // outputs (2 * transformed columns)
constexpr int L_MAX = 8, D_MAX = 8;

__device__ __forceinline__ float elu(float v) { return v > 0.0f ? v : expm1f(v); }

// ELU' from the saved PRE-activation: exp(a) itself.  (Until round 5 the forward saved the OUTPUT h and the backward took h + 1: an
// absolute 2^-24 on a factor that can be far below 1 -- PyTorch keeps the input -- which left the activation-gradient chain at ~2 x
// PyTorch's error against float64, tools/fused_accuracy.py.  The saved tensors h_all now hold a = W in + b; the weight-gradient kernel
// re-derives h = elu(a) when it stages its tiles.)
__device__ __forceinline__ float elu_grad_from_pre(float a) { return a > 0.0f ? 1.0f : expf(a); }   // alpha = 1

// the coupling's log-scale from the sub-network's raw output
__device__ __forceinline__ float soft_clamp(float o, float clamp) { return clamp * tanhf(o / clamp); }

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

// ------------------------------------------------------------------------------------------------ the parameter block
template <class F> struct HalfOf { F *W1, *b1, *W2, *b2, *W3, *b3; };
template <class F> struct LayerOf { F *scale, *bias; HalfOf<F> a, b; };
typedef HalfOf<const float> HalfP;
typedef LayerOf<const float> LayerP;
struct FlowP { LayerP layer[L_MAX]; unsigned char perm[L_MAX][D_MAX]; };

/* params (and, with F = float, grads): L x 14 device pointers per layer -- ActNorm log-scale [D] and bias [D], then W1 [H, Dh + C], b1 [H],
 * W2 [H, H], b2 [H], W3 [2 Dt, H], b3 [2 Dt] of sub-network 1 (conditioned on the first d1 columns) and of sub-network 2; perm: L x D host ints. */
template <class F> static inline LayerOf<F> layer_of(const void *rows, int l)
{
    F *const *q = reinterpret_cast<F *const *>(rows) + 14 * l;
    return {q[0], q[1], {q[2], q[3], q[4], q[5], q[6], q[7]}, {q[8], q[9], q[10], q[11], q[12], q[13]}};
}
static inline void fill(FlowP &P, int L, int D, const void *const *params, const int *perm)
{
    for (int l = 0; l < L; ++l) {
        P.layer[l] = layer_of<const float>(params, l);
        for (int d = 0; d < D; ++d) P.perm[l][d] = (unsigned char)perm[l * D + d];
    }
}
static inline bool perm_ok(const int *perm, int L, int D)
{
    for (int i = 0; i < L * D; ++i) if (perm[i] < 0 || perm[i] >= D) return false;
    return true;
}

// A half-layer's shape.  first (sub-network 1):  conditioned on the row's first d1 columns, transforms the other d2;
//                        second (sub-network 2): conditioned on the last d2, transforms the first d1.
struct HalfShape { int Dh, Dt, DI, M, xh0, xt0; };    // conditioning / transformed columns, inputs Dh + C, outputs 2 Dt, the first
                                                      // conditioning / transformed column of the row
__host__ __device__ __forceinline__ HalfShape half_shape(int d1, int d2, int C, bool second)
{
    return second ? HalfShape{d2, d1, d2 + C, 2 * d1, d1, 0} : HalfShape{d1, d2, d1 + C, 2 * d2, 0, d1};
}

// ------------------------------------------------------------------------------------------------ the 128-long MFMA dot
// Which 32 k's a lane group takes in a v_mfma_f32_16x16x4_f32 over K = 128 is free -- the instruction sums over all four groups --
// and it decides the LDS banks: ds_read_b128 serves lanes {0-3, 12-15, 20-27} together, i.e. rows n of group 0 with rows n' of
// group 1, on 64 banks = 16 slots of 16 bytes; with a row stride of 33 slots, groups 0 and 1 must start a multiple of 16 slots =
// 64 floats apart, not 32, or every read is a 2-way conflict: groups 0, 1, 2, 3 take the k blocks 0, 2, 1, 3.
__device__ __forceinline__ int kblock(int kk) { return ((kk & 1) << 1) | (kk >> 1); }

// [16 rows x 128] x [128 x 16 units] on LDS operands read 16 bytes at a time: lane l holds A[row l & 15][k] at ap and B[k][unit l & 15]
// at bp for its group's 32 k's; the even and the odd groups of four k's go to two accumulators (a shorter dependent chain).
__device__ __forceinline__ f32x4 mfma_k128(const float4 *ap, const float4 *bp)
{
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
#pragma unroll
    for (int q4 = 0; q4 < 8; q4 += 2) {
        const float4 a0 = ap[q4], b0 = bp[q4], a1 = ap[q4 + 1], b1 = bp[q4 + 1];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// The two epilogues of a 16 x 16 x 4 MFMA whose D is [row][unit]: lane l holds unit u = tile base + (l & 15) of the rows
// 4 (l >> 4) + register.  Forward: bias, the PRE-activation to global memory (the backward's), its ELU to LDS.
__device__ __forceinline__ void mfma_epilogue_elu(f32x4 acc, float bias, int kk, int u, float (*h)[LDR], const RowBuf &pre)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 4 * kk + q;
        const float a = acc[q] + bias;
        h[r][u] = elu(a);
        pre.put(r * H + u, a);
    }
}
// Backward: times ELU' of the saved pre-activation, to LDS (the next product's operand) and to global memory (the weight gradients').
__device__ __forceinline__ void mfma_epilogue_elu_grad(f32x4 acc, int kk, int u, const float (*pre)[LDR], float (*d)[LDR], const RowBuf &out)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 4 * kk + q;
        const float v = acc[q] * elu_grad_from_pre(pre[r][u]);
        d[r][u] = v;
        out.put(r * H + u, v);
    }
}

}  // namespace nddm_train
